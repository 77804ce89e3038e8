"""The exact reference of the weight-streaming decode linears -- gemm_skinny16_kernel, decode_linear_fp8_kernel,
decode_linear_mxfp4_kernel, gemm_skinny32p_kernel and gemm_skinny_kernel (csrc/gemm_impl.inc, decode_fp8_impl.inc,
decode_mxfp4_impl.inc, skinny16_parts.inc) -- shared by tests/test_skinny_ref_cpu.py and tests/test_skinny_edges_gpu.py.
Plain torch on the CPU.

What is here:
  FORMS      one record per template instantiation a launcher can send (NW waves split K in blocks of kblk, U blocks per
             trip, a ring of NBUF register buffers, MT token tiles, prologue PRO) and the launch sites it is sent from;
             launch_table() reads the same facts out of the sources, so the table cannot drift from them unnoticed
  blocks()   the trip model: the K blocks wave w multiplies, trip by trip;  edges(): the K-block counts at which such a
             loop goes wrong (a wave without a block, a clamped and skipped u = 1 block, the ring's first and second wrap)
  Census     seeded inputs on which EVERY partial sum of the kernel is an exact fp32 number in any summation order, so
             the output has no rounding freedom: it must equal RNE_e16(exact * scale + residual) bit for bit.  Three
             families, one per prologue: plain (integers), RMSNorm (a fixed census of magnitudes per 64 elements: the
             mean square is a power of two), SwiGLU (one gate value per row, chosen away from every rounding tie)
  residual() the cancelling residual -RNE(exact) +- one ulp: the kernel's fp32 sum and the add are exact, what is stored
             is exact - RNE(exact) +- ulp, so an error of ONE quantum anywhere in the sum shows in the output bits even
             where |exact| is hundreds of ulps of the output type
  Census.check()  asserts the exactness conditions and the sharpness caps from the reference alone

Measured by tests/test_skinny_ref_cpu.py (check() returns them and the test prints them; the largest over all shapes the GPU
test launches):
  sum_k |x w| in quanta        plain 10128 (16-bit, N = 4097, K = 6720), 10068 (e4m3), 32412 (MXFP4, K = 8320, quanta of 1/2);
                               RMSNorm 30573 quanta of 1/4 (16-bit, K = 6720), 154829 of 1/8 (MXFP4, M = 1, K = 13440);
                               the cap is 2^24 = 16777216
  SwiGLU bits(s_m) + bits(sum |up w|)   24 at most, by construction: `up` stays dense (uniform in {0, +-1, +-2}: at K = 6720
                               the largest sum is about 1.0e4, 14 bits) and the gate of a row is drawn among the accepted
                               candidates whose rounded silu has few enough significant bits for that row's sum (f16 at
                               K = 6720: 10 of its 11); measured 22 (bf16) and 24 (f16)
  gate candidates accepted     bf16 1276 of 1282, f16 10135 of 10242 (the fp64 silu times 1 +- 2^-18)
  hidden (tile, K block) sites M >= 3: none at any shape;  M = 1: at most 0.023 % (N = 4097, K = 1088; cap 0.1 %)
  hidden (row, 8-chunk) sites  M >= 3: plain 0.082 %, RMSNorm 0.023 %, SwiGLU 0.064 % at most (cap 1 %)
  largest |exact * scale| over all leading K: 15730 (e4m3 SwiGLU, K = 6720), far below f16's 65504
"""
import collections
import functools
import os
import re

import torch

H16 = (torch.bfloat16, torch.float16)
MANT = {torch.bfloat16: 8, torch.float16: 11}                 # significant bits
FP8 = torch.float8_e4m3fn
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "macaw_llm_amd", "csrc")

# ------------------------------------------------------------------------------------------------- the rules --
WIDE_N, WIDE_K = 4096, 4096            # mk_decode_linear_plan: 16 waves where N <= 4096 and K <= 4096
SKINNY32_N = 8192                      # skinny32_cfg: 17 ... 32 rows take cfg 22 from N = 8192, else cfg 19
LDS_BYTES = 40 * 1024                  # prologue forms: M * (K + 8) * 2 bytes of prepared token rows
EPS = 1e-6                             # RMSNorm eps of the GPU cases


def wide(N, K):
    return N <= WIDE_N and K <= WIDE_K


def skinny32_cfg(N):
    return 22 if N >= SKINNY32_N else 19


def prologue_fits(M, K):
    return M <= 16 and M * (K + 8) * 2 <= LDS_BYTES


# ------------------------------------------------------------------------------------------------ form table --
# fmt: weight format (e16 / fp8 / mxfp4); kernel: the __global__ template; NW, U, PRO, NBUF, MT: its arguments with the
# defaults written out (gemm_skinny_kernel<8> has no U / NBUF: its loop is two blocks per trip and a one-block tail,
# modelled as U = 2, NBUF = 1); kblk: elements of K per block; mmax: token rows; wrows: weight rows per workgroup;
# wide: True / False for the forms mk_decode_linear_plan's rule selects, None where the rule does not apply;
# sites: (launcher, branch) pairs of the MK_LAUNCH lines that send it; reach: how a test gets it --
# "decode" = ops.decode_linear / _fp8 / _mxfp4 by shape, an int = mk_gemm under mk_gemm_set_cfg(int).
Form = collections.namedtuple("Form", "name fmt kernel NW U PRO NBUF MT kblk mmax wrows wide sites reach")


def _forms():
    out = []
    k16, k8, k4 = "gemm_skinny16_kernel", "decode_linear_fp8_kernel", "decode_linear_mxfp4_kernel"
    for p in (0, 1, 2):
        out.append(Form(f"e16 wide pro{p}", "e16", k16, 16, 2, p, 2, 1, 64, 16, 16, True,
                        (("launch_decode_linear", f"pro{p} wide"),) + ((("launch_skinny", "sk18"),) if p == 0 else ()), "decode"))
        out.append(Form(f"e16 narrow pro{p}", "e16", k16, 8, 2, p, 3, 1, 64, 16, 16, False,
                        (("launch_decode_linear", f"pro{p} narrow"),) + ((("launch_skinny", "sk17"),) if p == 0 else ()), "decode"))
    out.append(Form("e16 cfg18", "e16", k16, 16, 2, 0, 2, 1, 64, 16, 16, True, (("launch_skinny", "sk18"),), 18))
    out.append(Form("e16 cfg17", "e16", k16, 8, 2, 0, 3, 1, 64, 16, 16, None, (("launch_skinny", "sk17"),), 17))
    out.append(Form("e16 cfg19 two tiles", "e16", k16, 8, 2, 0, 2, 2, 64, 32, 16, None, (("launch_skinny", "sk19"),), 19))
    out.append(Form("e16 cfg22 32 x 32", "e16", "gemm_skinny32p_kernel", 8, 1, 0, 3, 1, 64, 32, 32, None,
                    (("launch_skinny", "sk22"),), 22))
    out.append(Form("e16 cfg13", "e16", k16, 8, 2, 0, 2, 1, 64, 16, 16, None, (("launch_skinny", "sk13"),), 13))
    out.append(Form("e16 cfg12", "e16", "gemm_skinny_kernel", 8, 2, 0, 1, 1, 64, 32, 32, None, (("launch_skinny", "else"),), 12))
    for p in (0, 1, 2):
        out.append(Form(f"fp8 wide pro{p}", "fp8", k8, 16, 2, p, 2, 1, 64, 16, 16, True,
                        (("launch_decode_linear_fp8", f"pro{p} wide"),), "decode"))
        out.append(Form(f"fp8 narrow pro{p}", "fp8", k8, 8, 2, p, 3, 1, 64, 16, 16, False,
                        (("launch_decode_linear_fp8", f"pro{p} narrow"),), "decode"))
    out.append(Form("fp8 two tiles", "fp8", k8, 8, 2, 0, 2, 2, 64, 32, 16, None, (("launch_decode_linear_fp8", "m32"),), "decode"))
    out.append(Form("mxfp4 wide pro0", "mxfp4", k4, 16, 1, 0, 3, 1, 128, 16, 16, True,
                    (("launch_decode_linear_mxfp4", "pro0 wide"),), "decode"))
    out.append(Form("mxfp4 narrow pro0", "mxfp4", k4, 8, 1, 0, 4, 1, 128, 16, 16, False,
                    (("launch_decode_linear_mxfp4", "pro0 narrow"),), "decode"))
    for p in (1, 2):
        out.append(Form(f"mxfp4 wide pro{p}", "mxfp4", k4, 16, 2, p, 2, 1, 128, 16, 16, True,
                        (("launch_decode_linear_mxfp4", f"pro{p} wide"),), "decode"))
        out.append(Form(f"mxfp4 narrow pro{p}", "mxfp4", k4, 8, 2, p, 3, 1, 128, 16, 16, False,
                        (("launch_decode_linear_mxfp4", f"pro{p} narrow"),), "decode"))
    out.append(Form("mxfp4 two tiles", "mxfp4", k4, 8, 1, 0, 2, 2, 128, 32, 16, None,
                    (("launch_decode_linear_mxfp4", "m32"),), "decode"))
    return out


FORMS = _forms()
BY_NAME = {f.name: f for f in FORMS}
TEMPLATE_FIELDS = ("NW", "U", "PRO", "NBUF", "MT")


# ------------------------------------------------------------------------------------- the table, from source --
def _function_body(text, head):
    """the text of the function whose definition starts with `head`, braces balanced"""
    i = text.index(head)
    j = text.index("{", i)
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        k += 1
        if depth == 0:
            return text[j:k]


def kernel_templates(text):
    """{kernel: [(parameter, default or None), ...]} of the __global__ templates of a source text"""
    out = {}
    for params, name in re.findall(r"template <([^>]*)>\s*\n__global__[^\n]*\bvoid (\w+)\(", text):
        out[name] = [(m.group(1), int(m.group(2)) if m.group(2) else None)
                     for m in re.finditer(r"int (\w+)(?: = (\d+))?", params)]
    return out


def kernel_kblk(text, kernel):
    """the divisor of `const int nkb = g.K / ...` in the kernel's body"""
    body = _function_body(text, re.search(r"void " + kernel + r"\(", text).group(0))
    return int(re.search(r"const int nkb = g\.K / (\d+);", body).group(1))


def _launches(body, templates):
    """[(line, kernel, {parameter: value}, threads, grid)] of the MK_LAUNCH lines of a launcher body"""
    out = []
    for line in body.splitlines():
        m = re.search(r"MK_LAUNCH\(\(?(\w+)(?:<([^>]*)>)?\)?, ([^,]+(?:\([^)]*\))?[^,]*), dim3\((\d+)\)", line)
        if not m:
            continue
        kernel, args, grid, threads = m.group(1), m.group(2), m.group(3), int(m.group(4))
        vals = [int(a) for a in args.split(",")] if args else []
        params = templates[kernel]
        assert len(vals) <= len(params), line
        full = {}
        for i, (name, default) in enumerate(params):
            full[name] = vals[i] if i < len(vals) else default
            assert full[name] is not None, f"{kernel}: no value for {name} in: {line.strip()}"
        out.append((line, kernel, full, threads, grid.strip()))
    return out


def launch_table(csrc=CSRC):
    """{(launcher, branch): (kernel, {template parameter: value}, threads, weight rows per workgroup, kblk)} read from the
    MK_LAUNCH lines of launch_skinny, launch_decode_linear (gemm_impl.inc), launch_decode_linear_fp8 and
    launch_decode_linear_mxfp4.  A branch is "sk<cfg>" / "else" in launch_skinny and "m32" (more than 16 rows) or
    "pro<p> wide|narrow" in the decode launchers."""
    table = {}
    for fname, launchers in (("gemm_impl.inc", ("launch_skinny", "launch_decode_linear")),
                             ("decode_fp8_impl.inc", ("launch_decode_linear_fp8",)),
                             ("decode_mxfp4_impl.inc", ("launch_decode_linear_mxfp4",))):
        text = open(os.path.join(csrc, fname)).read()
        templates = kernel_templates(text)
        for launcher in launchers:
            body = _function_body(text, f"void {launcher}(")
            pro = None
            for line, kernel, full, threads, grid in _launches(body, templates):
                if launcher == "launch_skinny":
                    m = re.search(r"sk == (\d+)", line)
                    branch = f"sk{m.group(1)}" if m else "else"
                else:
                    # the prologue of a launch line: the closest `prologue == p` / `} else {` above it in the body
                    head = body[:body.index(line)]
                    marks = [(head.rfind("prologue == 0"), 0), (head.rfind("prologue == 1"), 1), (head.rfind("} else {"), 2)]
                    pro = max(marks)[1] if max(marks)[0] >= 0 else None
                    if "g.M > 16" in line or "M > 16" in line:
                        branch = "m32"
                    else:
                        assert pro is not None, line
                        assert ("if (wide)" in line) != line.lstrip().startswith("else"), line
                        branch = f"pro{pro} " + ("wide" if "if (wide)" in line else "narrow")
                wrows = 32 if "32)" in grid else 16
                assert (launcher, branch) not in table, (launcher, branch)
                table[(launcher, branch)] = (kernel, full, threads, wrows, kernel_kblk(text, kernel))
    return table


def source_rules(csrc=CSRC):
    """the numbers of the selection rules, read from common.h, gemm.hip and gemm_impl.inc"""
    common = open(os.path.join(csrc, "common.h")).read()
    gemm = open(os.path.join(csrc, "gemm.hip")).read()
    impl = open(os.path.join(csrc, "gemm_impl.inc")).read()
    m = re.search(r"\*wide = N <= (\d+) \* (\d+) && K <= (\d+);", common)
    r = {"wide_n": int(m.group(1)) * int(m.group(2)), "wide_k": int(m.group(3))}
    m = re.search(r"\*lds > (\d+) \* 1024 \? MK_ERR_UNSUPPORTED", common)
    r["lds_bytes"] = int(m.group(1)) * 1024
    assert re.search(r"\*lds = prologue \? \(size_t\)M \* \(K \+ 8\) \* 2 : 0;", common)
    m = re.search(r"M > \(prologue \? (\d+) : (\d+)\)", common)
    r["mmax"] = (int(m.group(1)), int(m.group(2)))
    m = re.search(r"return N >= (\d+) \? (\d+) : (\d+);", _function_body(gemm, "int skinny32_cfg(int N)"))
    r["skinny32"] = (int(m.group(1)), int(m.group(2)), int(m.group(3)))
    m = re.search(r"int sk = d->M <= 16 \? \(\(d->N <= (\d+) \* (\d+) && d->K <= (\d+)\) \? (\d+) : (\d+)\) : skinny32_cfg\(d->N\);", gemm)
    r["mk_gemm"] = (int(m.group(1)) * int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))
    m = re.search(r"if \(\(g_force_cfg == (\d+) \|\| g_force_cfg == (\d+) \|\| g_force_cfg == (\d+)\) \|\|\s*"
                  r"\(\(g_force_cfg == (\d+) \|\| g_force_cfg == (\d+) \|\| g_force_cfg == (\d+)\) && d->M <= 16\)\) sk = g_force_cfg;", gemm)
    r["forced"] = (tuple(int(m.group(i)) for i in (1, 2, 3)), tuple(int(m.group(i)) for i in (4, 5, 6)))
    assert "skinny32_cfg(N), N, st)" in _function_body(gemm, 'extern "C" int mk_decode_linear(')
    r["cfg12_loop"] = bool(re.search(r"for \(; kb \+ NW < nkb; kb \+= 2 \* NW\)", _function_body(impl, "void gemm_skinny_kernel(")))
    return r


# ------------------------------------------------------------------------------------------------ trip model --
def blocks(form, w, nkb):
    """the K blocks wave w multiplies, one list per trip: w + NW (t U + u), u < U, a block past the end skipped"""
    NW, U = form.NW, form.U
    trips = []
    if form.kernel == "gemm_skinny_kernel":                     # two blocks per trip while both exist, then a tail of one
        kb = w
        while kb + NW < nkb:
            trips.append([kb, kb + NW])
            kb += 2 * NW
        if kb < nkb:
            trips.append([kb])
        return trips
    t = 0
    while w + NW * t * U < nkb:
        trips.append([w + NW * (t * U + u) for u in range(U) if w + NW * (t * U + u) < nkb])
        t += 1
    return trips


def nkb_reach(form, M=3):
    """the largest K-block count the form can be launched with at M token rows"""
    lim = 1 << 30
    if form.wide:
        lim = WIDE_K // form.kblk
    if form.PRO:
        lim = min(lim, (LDS_BYTES // (2 * M) - 8) // form.kblk)
    return lim


def edges(form, M=3):
    """{1} + {j NW U + d NW + delta: j = 0 ... 2 NBUF, d < U, delta = -1, 0, 1}, clipped to what the form can reach; a wide
    form's largest reachable count is an edge of its own"""
    s = {1}
    for j in range(2 * form.NBUF + 1):
        for d in range(form.U):
            for delta in (-1, 0, 1):
                s.add(j * form.NW * form.U + d * form.NW + delta)
    lim = nkb_reach(form, M)
    s = {n for n in s if 1 <= n <= lim}
    if form.wide:
        s.add(lim)
    return sorted(s)


def census_runs(form):
    """[(M, N, [nkb, ...])]: the census launches of tests/test_skinny_edges_gpu.py, whose inputs test_skinny_ref_cpu.py checks.
    One-tile forms: M = 3 over the edge list (13 of 16 token lanes clamped; the MXFP4 prologue forms, whose LDS rows end at 53
    blocks with three rows, run the rest of the list with one), M = 1, 15, 16 at nkb = 1, NW + 1, NW U + 1 as far as the
    prepared rows fit, M = 16 at the largest K that fits 40 KiB, and the narrow forms once more reached through K (N = 33,
    the first K past the wide rule).  Two-tile and 32-row forms: M = 17, 31, 32 (and 3 where the entry point takes it) over
    the edge list."""
    N, runs = census_N(form), []
    if form.mmax == 32:
        for M in ((3,) if form.reach != "decode" else ()) + (17, 31, 32):
            runs.append((M, N, edges(form, M)))
        return runs
    runs.append((3, N, edges(form, 3)))
    rest = [n for n in edges(form, 1) if n not in edges(form, 3)]
    small = {1, form.NW + 1, form.NW * form.U + 1}
    for M in (1, 15, 16):
        nk = {n for n in small if n <= nkb_reach(form, M)}
        if M == 1:
            nk |= set(rest)
        if M == 16 and form.PRO:
            nk.add(nkb_reach(form, 16))
        runs.append((M, N, sorted(nk)))
    if form.wide is False and form.reach == "decode":
        runs.append((3, 33, [WIDE_K // form.kblk + 1]))
    return runs


def census_N(form):
    """N of the census launches: 4097 reaches the narrow forms (and leaves the last workgroup one real weight row), 40 is two
    full tiles and a half one"""
    return 4097 if (form.wide is False and form.reach == "decode") else 40


# ---------------------------------------------------------------------------------------------- 16-bit maths --
def rne(v, dtype):
    """float64 -> dtype, correctly rounded: v must be an exact fp32 number (as every exact result here is), so that the
    conversion rounds once"""
    f = v.to(torch.float32)
    assert torch.equal(f.double(), v), "not an exact fp32 number: the reference would round twice"
    return f.to(dtype)


def bits16(t):
    return t.contiguous().view(torch.int16)


def _ulp(y, dtype):
    """ulp of the 16-bit value y (float64); 1 for y = 0"""
    _, e = torch.frexp(y.abs())
    u = torch.ldexp(torch.ones_like(y), e - MANT[dtype])
    return torch.where(y == 0, torch.ones_like(y), u)


def residual(v, dtype, seed):
    """the cancelling residual of the exact results v (float64): -(RNE(v) + c ulp), c in {-1, 0, 1} seeded; a value of dtype"""
    y = rne(v, dtype).double()
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(-1, 2, v.shape, generator=g).double()
    r = -(y + c * _ulp(y, dtype))
    r16 = r.to(torch.float32).to(dtype)
    assert torch.equal(r16.double(), r), "residual not representable"
    return r16


def expected(v, dtype, res=None):
    """RNE(v + residual) as a tensor of dtype"""
    return rne(v if res is None else v + res.double(), dtype)


def sig_bits(v):
    """significant bits of each (float64) value: 0 for 0"""
    m, _ = torch.frexp(v.abs())
    n = torch.zeros(v.shape, dtype=torch.int64)
    frac = m.clone()
    for _ in range(53):
        live = frac != 0
        if not bool(live.any()):
            break
        n += live.to(torch.int64)
        frac = frac * 2
        frac = frac - torch.floor(frac)
    return n


# -------------------------------------------------------------------------------------------------- census --
@functools.lru_cache(maxsize=4)
def _base_weight(seed, N, K):
    return torch.randint(-2, 3, (N, K), generator=torch.Generator().manual_seed(seed), dtype=torch.int8)


@functools.lru_cache(maxsize=None)
def gate_candidates(dtype):
    """(g, s = RNE(silu(g)), candidates, accepted): the 16-bit values with 0.25 <= |g| <= 8 whose rounded silu does not move
    when the fp64 silu is perturbed by a factor 1 +- 2^-18"""
    allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype).double()
    g = allv[torch.isfinite(allv) & (allv.abs() >= 0.25) & (allv.abs() <= 8)]
    silu = g / (1 + torch.exp(-g))
    s = silu.to(torch.float32).to(dtype)
    keep = torch.ones_like(g, dtype=torch.bool)
    for f in (1 - 2.0 ** -18, 1 + 2.0 ** -18):
        keep &= (silu * f).to(torch.float32).to(dtype) == s
    return g[keep], s[keep].double(), int(g.numel()), int(keep.sum())


class Census:
    """Seeded exact inputs for `form` at M rows, N weight rows and nkb K-blocks; a launch at fewer blocks takes the leading
    columns (every condition below is per block or monotone in K, so check() at nkb covers them all).
      x        what the kernel gets: e16 [M, K]; for PRO 2 the pair (gate, up), each [M, K], launched as [gate | up]
      tok      the token operand of the MFMAs, exact (f32 [M, K]): x, the RMSNorm rows or the SwiGLU rows
      weff     the de-quantised weight the MFMAs see (f32 [N, K]); oscale [N] (f64): the e4m3 kernel's epilogue scale
      weights  the kernel's weight operands: e16 {"W"}, fp8 {"Wq", "s"}, mxfp4 {"q", "e"}
      norm_w   PRO 1: e16 [K]"""

    def __init__(self, form, dtype, M, N=None, nkb=None, seed=0):
        self.form, self.dtype, self.M = form, dtype, M
        self.N = N = census_N(form) if N is None else N
        self.nkb = nkb = max(edges(form, M)) if nkb is None else nkb
        self.K = K = nkb * form.kblk
        g = torch.Generator().manual_seed(1000 * seed + 17 * M + (dtype == torch.float16) + 2 * FORMS.index(form))
        wi = (_base_weight(seed, 4097, 13440) if N <= 4097 else _base_weight(seed, N, K))[:N, :K].to(torch.float32)
        self.oscale = torch.ones(N, dtype=torch.float64)
        self.qw = 1.0                                           # quantum of weff
        if form.fmt == "e16":
            self.weff = wi
            self.weights = {"W": wi.to(dtype)}
        elif form.fmt == "fp8":                                 # the byte codes of the integers, a power of two per row
            self.weff = wi
            self.oscale = torch.pow(2.0, torch.randint(-2, 3, (N,), generator=g).double())
            self.weights = {"Wq": wi.to(FP8).view(torch.uint8), "s": self.oscale.float()}
        else:                                                   # e2m1 codes of the integers, block exponents 126 ... 128
            a = wi.abs().to(torch.uint8)
            code = torch.where(a == 2, 4, torch.where(a == 1, 2, 0)).to(torch.uint8) | ((wi < 0).to(torch.uint8) << 3)
            e = torch.randint(126, 129, (N, K // 32), generator=g, dtype=torch.uint8)
            self.weights = {"q": (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous(), "e": e}
            self.weff = (wi.view(N, K // 32, 32) * torch.pow(2.0, e.float() - 127.0)[:, :, None]).view(N, K)
            self.qw = 0.5
        self.norm_w = None
        if form.PRO == 0:
            self.x = torch.randint(-2, 3, (M, K), generator=g).to(dtype)
            self.tok, self.qt = self.x.float(), 1.0
        elif form.PRO == 1:
            mags = torch.tensor([3.0] * 20 + [2.0] * 16 + [1.0] * 12 + [0.0] * 16)
            perm = torch.rand((M, K // 64, 64), generator=g).argsort(-1)
            sign = torch.randint(0, 2, (M, K // 64, 64), generator=g).float() * 2 - 1
            self.row_scale = torch.pow(2.0, torch.randint(-3, 4, (M, 1), generator=g).float())
            self.normed = (mags[perm] * sign).view(M, K) / 2    # x * rstd, ideally: {0, +-1/2, +-1, +-3/2}
            self.x = (self.normed * 2 * self.row_scale).to(dtype)
            nw = torch.randint(-4, 5, (K,), generator=g).float() / 2
            self.norm_w = nw.to(dtype)
            self.tok, self.qt = nw[None, :] * self.normed, 0.25
        else:
            up = torch.randint(-2, 3, (M, K), generator=g).float()
            sums = (up.abs() @ self.weff.abs().t()).amax(1).double() / self.qw       # per row: max_n sum_k |up w|, in quanta
            cg, cs, _, _ = gate_candidates(dtype)
            cbits = sig_bits(cs)
            gate, s, used = [], [], set()
            for m in range(M):
                ok = (cbits + sig_bits(sums[m:m + 1]) <= 24).nonzero().flatten()
                assert ok.numel() >= 4 * M, "no gate value leaves this row's sum exact: lower the density of up"
                for i in ok[torch.randperm(ok.numel(), generator=g)].tolist():
                    if i not in used:
                        used.add(i)
                        gate.append(cg[i])
                        s.append(cs[i])
                        break
            self.gate_row, self.s_row, self.up_sums = torch.stack(gate), torch.stack(s), sums
            self.x = (self.gate_row[:, None].expand(M, K).to(torch.float32).to(dtype).contiguous(), up.to(dtype))
            self.tok, self.qt = self.s_row.float()[:, None] * up, None
        self._partials = None

    # -- the exact result
    def partials(self):
        """[nkb, M, N] float64: tok[:, block] . weff[:, block]^T (exact in f32: check() asserts the bound that makes it so)"""
        if self._partials is None:
            nb, kb = self.nkb, self.form.kblk
            t = self.tok.view(self.M, nb, kb).permute(1, 0, 2)
            w = self.weff.view(self.N, nb, kb).permute(1, 2, 0)
            self._partials = torch.bmm(t, w).double()
        return self._partials

    def exact(self, nkb):
        """[M, N] float64: tok[:, :K] . weff[:, :K]^T, K = nkb blocks, before the e4m3 scale"""
        return self.partials()[:nkb].sum(0)

    def by_trips(self, nkb, blocks_fn=blocks):
        """the same sum taken as the kernel takes it: per wave the blocks of its trips, then the waves in order"""
        P = self.partials()
        total = torch.zeros(self.M, self.N, dtype=torch.float64)
        for w in range(self.form.NW):
            for trip in blocks_fn(self.form, w, nkb):
                for b in trip:
                    total += P[b]
        return total

    # -- the conditions
    def check(self):
        """asserts, from the reference alone, that the expectation has no rounding freedom and that the inputs are sharp;
        returns the measured figures"""
        f, M, N, K, dtype = self.form, self.M, self.N, self.K, self.dtype
        out = {}
        assert torch.equal(self.weff.to(dtype).float(), self.weff)              # the 16-bit type holds every weight
        sums = self.tok.abs().double() @ self.weff.abs().double().t()           # [M, N]
        if f.PRO == 2:
            assert torch.equal(self.tok.to(dtype).float(), self.tok)            # rnd(s * up) rounds nothing
            b = sig_bits(self.s_row) + sig_bits(self.up_sums)
            out["swiglu_bits"] = int(b.max())
            assert int(b.max()) <= 24, b
            cg, cs, n_all, n_ok = gate_candidates(dtype)
            out["gates"] = (n_ok, n_all)
            assert len(set(self.gate_row.tolist())) == M
            g = self.gate_row
            silu = g / (1 + torch.exp(-g))
            for fct in (1 - 2.0 ** -18, 1.0, 1 + 2.0 ** -18):
                assert torch.equal((silu * fct).to(torch.float32).to(dtype).double(), self.s_row)
        else:
            q = self.qt * self.qw
            out["sum_abs_quanta"] = float(sums.max() / q)
            assert out["sum_abs_quanta"] < 2 ** 24
            assert torch.equal(torch.round(self.tok / self.qt) * self.qt, self.tok)
        peak = (self.partials().cumsum(0).abs().amax((0, 1)) * self.oscale).max()
        out["peak"] = float(peak)
        assert out["peak"] < 3.0e4              # below f16's 65504 at every leading K, alpha = 2 and a residual included
        if f.PRO == 1:
            x = self.x.double()
            s2 = (self.row_scale.double() ** 2) * 4
            assert torch.equal((x * x).view(M, K // 64, 64).mean(-1), s2.expand(M, K // 64))
            for eps in (0.0, 1e-6):
                for pert in (1 - 2.0 ** -20, 1.0, 1 + 2.0 ** -20):
                    rstd = pert / torch.sqrt(s2 + eps)
                    n16 = (x * rstd).to(torch.float32).to(dtype)
                    assert torch.equal(n16.float(), self.normed), (eps, pert)
            assert torch.equal(self.tok.to(dtype).float(), self.tok)
        # sharpness: a dropped or doubled K block of any workgroup, or 16-byte load of any lane, must move an output
        P = self.partials()
        tiles = -(-N // f.wrows)
        nz = (P != 0).any(1)                                                    # [nkb, N]
        nz = torch.cat((nz, torch.zeros(self.nkb, tiles * f.wrows - N, dtype=torch.bool)), 1)
        hidden = 1.0 - nz.view(self.nkb, tiles, f.wrows).any(2).float().mean().item()
        out["hidden_block_share"] = hidden
        assert hidden == 0.0 if M >= 3 else hidden <= 1e-3, hidden
        if M >= 3:
            wv = self.weff.view(N, K // 8, 8)
            seen = torch.zeros(N, K // 8, dtype=torch.bool)
            for m in range(M):
                seen |= (wv * self.tok[m].view(1, K // 8, 8)).sum(-1) != 0
            out["hidden_chunk_share"] = 1.0 - seen.float().mean().item()
            assert out["hidden_chunk_share"] <= 0.01, out
        return out


@functools.lru_cache(maxsize=2)
def census(form_name, dtype, M, N=None, nkb=None, seed=0):
    return Census(BY_NAME[form_name], dtype, M, N, nkb, seed)
