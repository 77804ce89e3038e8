"""The fused attention kernels (csrc/attention_impl.inc) at the layouts and mask edges the model uses, against the fp32
reference of tests/attn_ref.py on the same 16-bit inputs:

  A. the engine's layouts -- q | k | v as column slices of one [M][3D] buffer, o / dout at another pitch, dq | dk | dv
     into a second fused buffer, a batch stride one row larger than S * ld, k / v out of a [B][Tmax][2D] cache whose
     rows beyond T are NaN -- each compared with the reference AND bit for bit with the same call on contiguous copies
     (geometry must not change arithmetic), with guards: outputs NaN-prefilled and fully written, every pad column and
     gap row unchanged;
  B. a mask census: q = 0 makes every visible score exactly 0, so lse = log(n_visible) and o = the mean of the visible
     v rows -- one key too many or too few among n moves lse by > 1 / (n + 1), which a 1e-5 bound sees and the max-norm
     bounds on random data do not;
  C. the tiled backward on random data at the edges no other test reaches (causal + padding at head_dim 128, Lq != Lk
     both ways, rows without a key, a fully padded sample);
  D. the kernels behind process-wide switches (MK_ATTN_DQ_ASYNC, MK_ATTN_NO_SHORT_BWD, MK_ATTN_NO_XCD_GROUP), each in a
     child process of its own.

Bounds are the project's (test_kernels_gpu.py): _close for o (bf16 rounding of P and of the output), rtol 1e-4 /
atol 2e-4 for lse, 2e-2 max|ref| + 2e-3 for gradients (16-bit P / dS operands)."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from macaw_llm_amd import ops  # noqa: E402
import attn_ref as R  # noqa: E402

H16 = [torch.bfloat16, torch.float16]
NAN = float("nan")
FWD_ENV = ("MK_ATTN_FWD8_MIN", "MK_ATTN_FWD8_HD64")


def _close(got, ref, what=""):
    """test_kernels_gpu._close for the 16-bit types: rtol 8e-3 of max|ref| + 8e-3"""
    got = got.float().cpu()
    ref = ref.float()
    err = (got - ref).abs().max().item()
    lim = 8e-3 + 8e-3 * ref.abs().max().item()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


def _lse_close(got, ref, what=""):
    got = got.float().cpu()
    dead = torch.isneginf(ref)
    assert torch.equal(torch.isneginf(got), dead), f"{what}: lse = -inf exactly on the rows without a visible key"
    assert not torch.isnan(got).any() and not torch.isposinf(got).any(), what
    if (~dead).any():
        torch.testing.assert_close(got[~dead], ref[~dead].float(), rtol=1e-4, atol=2e-4, msg=lambda m: f"{what}: {m}")


def _grad_close(got, ref, what=""):
    got = got.float().cpu()
    err = (got - ref).abs().max().item()
    lim = 2e-2 * ref.abs().max().item() + 2e-3
    assert torch.isfinite(got).all(), f"{what}: rows not written or non-finite"
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


# ------------------------------------------------------------------------------------------------ layouts
def _sentinel(rows, ld, dtype, dev):
    """finite, position-dependent and exact in both 16-bit types (multiples of 1/8 in -15.625 .. 15.625)"""
    n = torch.arange(rows * ld, device=dev)
    return (((n % 251) - 125).float() / 8).to(dtype).view(rows, ld)


class _Op:
    """a token-major [B, L, D] operand inside a wider allocation `base` [B * (L + gap)][ld]: columns col0 .. col0 + D
    of the first L rows of every sample (row pitch ld, batch stride (L + gap) * ld)"""

    def __init__(self, base, B, L, D, col0=0, gap=0, out=False):
        self.base, self.out, self.geom = base, out, (B, L + gap, L, col0, D)
        self.ld, self.bs = base.shape[1], (L + gap) * base.shape[1]
        self.t = self._of(base)
        assert self.ld % 8 == 0 and self.bs % 8 == 0 and self.t.data_ptr() % 16 == 0 and col0 + D <= self.ld

    def _of(self, base):
        B, Lp, L, col0, D = self.geom
        return base.view(B, Lp, base.shape[1])[:, :L, col0:col0 + D]

    def get(self):
        return self.t.detach().cpu().contiguous()


def _layout(kind, dev, dtype, B, Lq, Lk, D, bwd):
    S = lambda rows, ld: _sentinel(rows, ld, dtype, dev)  # noqa: E731
    L = {}
    if kind == "contig":
        mk = lambda n, out: _Op(S(B * n, D), B, n, D, out=out)  # noqa: E731
        L.update(q=mk(Lq, False), k=mk(Lk, False), v=mk(Lk, False), o=mk(Lq, True))
        if bwd:
            L.update(do=mk(Lq, False), dq=mk(Lq, True), dk=mk(Lk, True), dv=mk(Lk, True))
    elif kind in ("fused", "fused_gap"):          # LlamaLayerFn: one [M][3D] projection buffer, o at its own pitch
        assert Lq == Lk
        gap = 1 if kind == "fused_gap" else 0
        rows = B * (Lq + gap)
        qkv = S(rows, 3 * D)
        L.update(q=_Op(qkv, B, Lq, D, 0, gap), k=_Op(qkv, B, Lq, D, D, gap), v=_Op(qkv, B, Lq, D, 2 * D, gap),
                 o=_Op(S(rows, D + 8), B, Lq, D, 0, gap, out=True))
        if bwd:                                   # dout is read with o's geometry, dq | dk | dv written with q | k | v's
            dqkv = S(rows, 3 * D)
            L.update(do=_Op(S(rows, D + 8), B, Lq, D, 0, gap),
                     dq=_Op(dqkv, B, Lq, D, 0, gap, out=True), dk=_Op(dqkv, B, Lq, D, D, gap, out=True),
                     dv=_Op(dqkv, B, Lq, D, 2 * D, gap, out=True))
    elif kind == "cache":                         # cached prefill: k | v halves of [B][Tmax][2D], rows T .. Tmax - 1 NaN
        assert not bwd
        gap = 7
        cache = torch.full((B * (Lk + gap), 2 * D), NAN, dtype=dtype, device=dev)
        L.update(q=_Op(S(B * Lq, 3 * D), B, Lq, D, 0), k=_Op(cache, B, Lk, D, 0, gap), v=_Op(cache, B, Lk, D, D, gap),
                 o=_Op(S(B * Lq, D), B, Lq, D, out=True))
    else:
        raise ValueError(kind)
    return L


def _run(dev, hd, H, q, k, v, do, causal, km, kind="contig", bwd=True):
    """mk_flash_attn_fwd (+ _bwd) on the token-major CPU tensors q, k, v, do laid out as `kind`; outputs NaN-prefilled.
    Checks the guards (every addressed output element written and finite, every other byte of every allocation
    unchanged) and returns the results as contiguous CPU tensors."""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    L = _layout(kind, dev, q.dtype, B, Lq, Lk, D, bwd)
    for name, x in (("q", q), ("k", k), ("v", v), ("do", do)):
        if name in L:
            L[name].t.copy_(x.to(dev))
    for op in L.values():
        if op.out:
            op.t.fill_(NAN)
    bases = {}
    for op in L.values():
        ent = bases.setdefault(id(op.base), [op.base, op.base.clone(), torch.zeros_like(op.base, dtype=torch.bool)])
        if op.out:
            op._of(ent[2]).fill_(True)
    lse = torch.full((B, H, Lq), NAN, dtype=torch.float32, device=dev)
    km_d = km.to(dev) if km is not None else None
    scale = hd ** -0.5
    geo = (L["q"].ld, L["q"].bs, L["k"].ld, L["k"].bs, L["v"].ld, L["v"].bs, L["o"].ld, L["o"].bs)
    ops.flash_attn_fwd(L["q"].t, L["k"].t, L["v"].t, L["o"].t, B, H, Lq, Lk, hd, *geo, scale, kmask=km_d,
                       causal=causal, lse=lse)
    if bwd:
        assert (L["do"].ld, L["do"].bs) == (L["o"].ld, L["o"].bs)
        for g, x in (("dq", "q"), ("dk", "k"), ("dv", "v")):
            assert (L[g].ld, L[g].bs) == (L[x].ld, L[x].bs)
        ops.flash_attn_bwd(L["q"].t, L["k"].t, L["v"].t, L["o"].t, L["do"].t, lse, L["dq"].t, L["dk"].t, L["dv"].t,
                           B, H, Lq, Lk, hd, *geo, scale, kmask=km_d, causal=causal)
    torch.cuda.synchronize()
    for base, snap, written in bases.values():
        assert torch.isfinite(base[written]).all(), f"{kind}: an addressed output element is unwritten or non-finite"
        assert torch.equal(base.view(torch.int16)[~written], snap.view(torch.int16)[~written]), \
            f"{kind}: an input, pad column or gap row changed"
    assert not torch.isnan(lse).any(), "lse not fully written"
    out = {name: L[name].get() for name in ("o", "dq", "dk", "dv") if name in L}
    out["lse"] = lse.cpu()
    return out


def _set_fwd_env(setenv, delenv, env):
    for name in FWD_ENV:
        delenv(name)
    for name, val in env.items():
        setenv(name, val)


def _mp_env(monkeypatch, env):
    _set_fwd_env(monkeypatch.setenv, lambda n: monkeypatch.delenv(n, raising=False), env)


@functools.lru_cache(maxsize=None)
def _inputs(dtype, hd, B, H, Lq, Lk, causal, mask, zero_q=False):
    """seeded q, k, v, dout, kmask of a case (the same in the test process and in the child processes)"""
    seed = Lq * 31 + Lk * 7 + hd + (dtype == torch.float16)
    q, k, v, do = R.make_inputs(seed, dtype, B, H, Lq, Lk, hd, zero_q=zero_q)
    return q, k, v, do, R.kmask_pattern(mask, B, Lk)


@functools.lru_cache(maxsize=None)
def _case(dtype, hd, B, H, Lq, Lk, causal, mask, zero_q=False):
    """the inputs of a case and their fp32 reference, computed once and shared (nothing mutates them)"""
    q, k, v, do, km = _inputs(dtype, hd, B, H, Lq, Lk, causal, mask, zero_q)
    ref = R.attention_ref(q, k, v, H, hd ** -0.5, causal=causal, kmask=km, dout=do)
    return q, k, v, do, km, ref


def _check_against_ref(got, ref, what, grads=True):
    _close(got["o"], ref["o"], what=f"{what}: o")
    _lse_close(got["lse"], ref["lse"], what=f"{what}: lse")
    if grads:
        for g in ("dq", "dk", "dv"):
            _grad_close(got[g], ref[g], what=f"{what}: {g}")


def _check_exact_zeros(got, B, Lq, Lk, causal, km, what):
    """rows without a visible key: o = 0, lse = -inf, dq = 0; keys no query sees: dk = dv = 0 -- exactly"""
    vis = R.visible(B, Lq, Lk, causal, km)
    dead, unseen = ~vis.any(-1), ~vis.any(1)
    assert (got["o"][dead] == 0).all(), f"{what}: o of a row without a visible key"
    assert torch.isneginf(got["lse"].transpose(1, 2)[dead]).all(), f"{what}: lse of a row without a visible key"
    if "dq" in got:
        assert (got["dq"][dead] == 0).all(), f"{what}: dq of a row without a visible key"
        assert (got["dk"][unseen] == 0).all() and (got["dv"][unseen] == 0).all(), f"{what}: dk / dv of an unseen key"


def _same_bits(a, b, what, names=("o", "lse", "dq", "dk", "dv")):
    for name in names:
        if name in a:
            assert torch.equal(a[name], b[name]), \
                (what, name, (a[name].float() - b[name].float()).abs().nan_to_num(0.0).max().item())


# ------------------------------------------------------------------------------------- A. engine layouts
@pytest.mark.parametrize("kind", ["fused", "fused_gap"])
@pytest.mark.parametrize("hd,S,causal,mask", [(64, 200, True, "pad37"), (64, 257, False, "none"),
                                              (128, 200, True, "pad37"), (128, 257, False, "none"),
                                              (128, 144, True, "pad37"), (128, 144, False, "none")])
@pytest.mark.parametrize("dtype", H16)
def test_fused_qkv_layout_is_the_contiguous_call_bit_for_bit(dev, dtype, hd, S, causal, mask, kind):
    """LlamaLayerFn's geometry: q | k | v column slices of one [B S][3D] buffer (q_ld = k_ld = v_ld = 3D), o and dout at
    pitch D + 8, dq | dk | dv slices of a second fused buffer; `fused_gap`: every batch stride one row larger than
    S * ld.  A kernel that took o's pitch for q's (or wrote dk where dq belongs) fails the reference comparison; one
    that strays into a pad column or gap row fails the guards of _run."""
    B, H = 3, 3
    q, k, v, do, km, ref = _case(dtype, hd, B, H, S, S, causal, mask)
    got = _run(dev, hd, H, q, k, v, do, causal, km, kind=kind)
    _check_against_ref(got, ref, kind)
    _check_exact_zeros(got, B, S, S, causal, km, kind)
    same = _run(dev, hd, H, q, k, v, do, causal, km, kind="contig")
    _same_bits(got, same, f"{kind} vs contiguous")


@pytest.mark.parametrize("Lq,Lk,env", [(3, 200, {}), (70, 333, {}), (300, 333, {"MK_ATTN_FWD8_MIN": "256",
                                                                              "MK_ATTN_FWD8_HD64": "1"})])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", H16)
def test_cache_layout_forward_never_reads_the_unwritten_rows(dev, dtype, hd, Lq, Lk, env, monkeypatch):
    """the cached prefill: k, v are the column halves of [B][Tmax][2D] (pitch 2D, batch stride Tmax * 2D), q a slice
    of the chunk's [M][3D] buffer, causal with Lq < Lk = T.  Rows T .. Tmax - 1 are NaN: a staging path that loaded
    one and multiplied it by P = 0 would give NaN.  (300, 333) with MK_ATTN_FWD8_MIN=256 is the 8-wave kernel."""
    B, H = 3, 3
    _mp_env(monkeypatch, env)
    q, k, v, do, km, ref = _case(dtype, hd, B, H, Lq, Lk, True, "none")
    got = _run(dev, hd, H, q, k, v, None, True, None, kind="cache", bwd=False)
    _check_against_ref(got, ref, "cache", grads=False)
    same = _run(dev, hd, H, q, k, v, None, True, None, kind="contig", bwd=False)
    _same_bits(got, same, "cache vs contiguous")


# --------------------------------------------------------------------------------------- B. mask census
CENSUS = [(Lq, Lk, c, 3, 3) for (Lq, Lk, c) in R.CENSUS_SHAPES] + [(520, 520, False, 2, 9)]
# one key too many or too few among n <= 600 moves lse by at least log(601 / 600) = 1.67e-3 > 1 / 601: two orders above
LSE_CENSUS_BOUND = 1e-5


def _fwd_variants(Lq):
    """every forward kernel that admits the shape: the default dispatch (short kernel at hd 128, Lq = Lk <= 160; else
    the 4-wave kernel), the 8-wave kernel switched off, and the 8-wave kernel from 256 rows.  The launcher's default
    threshold is 1024 rows and no census shape is that long, so today "default" and "fwd8 off" launch the same kernel:
    the second pass pins that MK_ATTN_FWD8_MIN=0 means "never" and keeps the 4-wave kernel covered should the default
    threshold ever drop below 520 rows.  Which kernel a setting selects is read from the launcher (mk_flash_attn_fwd),
    not observed here: should its condition on MK_ATTN_FWD8_MIN / MK_ATTN_FWD8_HD64 change, the "fwd8" pass would
    silently repeat the 4-wave kernel."""
    vs = [("default", {}), ("fwd8 off", {"MK_ATTN_FWD8_MIN": "0"})]
    if Lq >= 256:
        vs.append(("fwd8", {"MK_ATTN_FWD8_MIN": "256", "MK_ATTN_FWD8_HD64": "1"}))
    return vs


@pytest.mark.parametrize("mask", R.CENSUS_MASKS)
@pytest.mark.parametrize("Lq,Lk,causal,B,H", CENSUS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", H16)
def test_mask_census_with_zero_queries(dev, dtype, hd, Lq, Lk, causal, B, H, mask, monkeypatch):
    """q = 0: every visible score is exactly 0, every p exactly 1, l an exact integer in fp32, so
    lse[b, h, i] = log(n_visible(b, i)) up to the hardware log2 (a few ulp at values <= 9.3: bound 1e-5 absolute; one
    key too many or too few among n <= 600 moves lse by > 1.6e-3) and o = the mean of the visible v rows.  Rows with
    n = 0: exactly -inf and exact zeros.  (520, 520) non-causal is also the XCD-grouped 1-D grid with B H = 9 and 18
    (two and three groups of eight (b, h)).  Backward of the same inputs (dout random) against the reference.
    The 1e-5 bound is derived from the precision of the hardware log2; measured on an MI355X over all these cases the
    largest |lse - log n| is 8.6e-7 in the 4-wave and the 8-wave kernel and 5.2e-7 in the short kernel (the same at
    both dtypes and head dims), so the derived bound stands."""
    q, k, v, do, km, ref = _case(dtype, hd, B, H, Lq, Lk, causal, mask, True)
    n, lse_x, o_x = R.census_expect(v, H, Lq, causal, km)
    dead = torch.isneginf(lse_x)
    for tag, env in _fwd_variants(Lq):
        _mp_env(monkeypatch, env)
        first = tag == "default"
        got = _run(dev, hd, H, q, k, v, do, causal, km, bwd=first)
        what = f"census {Lq}x{Lk} {tag}"
        assert torch.equal(torch.isneginf(got["lse"]), dead), f"{what}: lse = -inf exactly where n = 0"
        if (~dead).any():
            err = (got["lse"].double()[~dead] - lse_x[~dead]).abs().max().item()
            assert err <= LSE_CENSUS_BOUND, f"{what}: max |lse - log n| = {err:.3e}"
        _close(got["o"], o_x, what=f"{what}: o")
        _check_exact_zeros(got, B, Lq, Lk, causal, km, what)
        if first:
            for g in ("dq", "dk", "dv"):
                _grad_close(got[g], ref[g], what=f"{what}: {g}")


# -------------------------------------------------------------------- C. backward edges on random data
@pytest.mark.parametrize("Lq,Lk,causal,mask", R.BWD_EDGE_CASES)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", H16)
def test_tiled_backward_edges(dev, dtype, hd, Lq, Lk, causal, mask):
    """flash_bwd_prep / _dq / _dkv at both head dims where only the end-to-end tests reached them: causal with key
    padding beyond the short-kernel limit (the LLaMA layer at S > 160), causal with Lq != Lk both ways ((300, 130): rows
    0 .. 169 see nothing, dq exactly 0), five rows over six key tiles, a fully padded sample (its dq, dk, dv exactly
    0), five query blocks with padding.  NaN-prefilled outputs fully written; a second call bit-identical."""
    B, H = 3, 3
    q, k, v, do, km, ref = _case(dtype, hd, B, H, Lq, Lk, causal, mask)
    got = _run(dev, hd, H, q, k, v, do, causal, km)
    what = f"bwd {Lq}x{Lk}"
    _check_against_ref(got, ref, what)
    _check_exact_zeros(got, B, Lq, Lk, causal, km, what)
    again = _run(dev, hd, H, q, k, v, do, causal, km)
    _same_bits(got, again, f"{what}: second call")


# ------------------------------------------------- D. kernel variants behind process-wide switches
SHORT_S = (160, 144, 33, 1)            # MK_ATTN_NO_SHORT_BWD: hd 128, causal with padding
XCD_BH = ((3, 3), (2, 9))              # MK_ATTN_NO_XCD_GROUP: (520, 520) non-causal, B H = 9 and 18
XCD_FWD = (("4-wave", {"MK_ATTN_FWD8_MIN": "0"}), ("fwd8", {"MK_ATTN_FWD8_MIN": "256", "MK_ATTN_FWD8_HD64": "1"}))
SWITCHES = {"default": {}, "dq_async": {"MK_ATTN_DQ_ASYNC": "1"}, "no_short_bwd": {"MK_ATTN_NO_SHORT_BWD": "1"},
            "no_xcd_group": {"MK_ATTN_NO_XCD_GROUP": "1"}}
_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_attention_edges_gpu as T; " \
         "T.child_main(sys.argv[3], sys.argv[4])"


def _name(dtype):
    return str(dtype).split(".")[1]           # (plain strings in the saved keys)


def child_main(mode, path):
    """runs in a child process whose environment holds the switch of `mode`: all shapes of the variant, one .pt"""
    dev = torch.device("cuda:0")
    setenv = lambda n, val: os.environ.__setitem__(n, val)  # noqa: E731
    delenv = lambda n: os.environ.pop(n, None)  # noqa: E731
    res = {}
    for dtype in H16:
        for hd in (64, 128):
            if mode in ("default", "dq_async"):
                _set_fwd_env(setenv, delenv, {})
                for Lq, Lk, causal, mask in R.BWD_EDGE_CASES:
                    q, k, v, do, km = _inputs(dtype, hd, 3, 3, Lq, Lk, causal, mask)
                    res[("bwd", _name(dtype), hd, Lq, Lk)] = _run(dev, hd, 3, q, k, v, do, causal, km)
            if mode in ("default", "no_xcd_group"):
                for B, H in XCD_BH:
                    for tag, env in XCD_FWD:
                        _set_fwd_env(setenv, delenv, env)
                        q, k, v, do, km = _inputs(dtype, hd, B, H, 520, 520, False, "pad77")
                        res[("xcd", _name(dtype), hd, B * H, tag)] = _run(dev, hd, H, q, k, v, None, False, km, bwd=False)
        if mode in ("default", "no_short_bwd"):
            _set_fwd_env(setenv, delenv, {})
            for S in SHORT_S:
                q, k, v, do, km = _inputs(dtype, 128, 3, 3, S, S, True, "pad11")
                res[("short", _name(dtype), S)] = _run(dev, 128, 3, q, k, v, do, True, km)
    torch.save(res, path)


def _child(mode, tmp):
    """one fresh process per variant (the switches are read once per process); no retry, its stderr in the message"""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MK_ATTN_")}
    env.update(SWITCHES[mode])
    f = str(tmp / f"{mode}.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(tests), tests, mode, f], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"{mode}: exit {r.returncode}\n{r.stderr[-3000:]}"
    return torch.load(f)


@pytest.fixture(scope="module")
def default_process(dev, tmp_path_factory):
    return _child("default", tmp_path_factory.mktemp("attn_default"))


def test_async_dq_kernel_is_bit_identical_to_the_synchronous_one(dev, default_process, tmp_path):
    """MK_ATTN_DQ_ASYNC=1 (flash_bwd_dq_kernel<.., ASYNC = true>: the next K / V tile fetched under the MFMAs) on the
    shapes of test_tiled_backward_edges: against the reference, and dq BIT-IDENTICAL to the default process -- the
    variant moves loads, not arithmetic (the other outputs come from the same kernels: identical too)."""
    res = _child("dq_async", tmp_path)
    for key, got in res.items():
        _, dn, hd, Lq, Lk = key
        dtype = getattr(torch, dn)
        causal, mask = next((c, m) for (a, b, c, m) in R.BWD_EDGE_CASES if (a, b) == (Lq, Lk))
        ref = _case(dtype, hd, 3, 3, Lq, Lk, causal, mask)[5]
        _check_against_ref(got, ref, f"dq async {key}")
        _same_bits(got, default_process[key], f"dq async vs sync {key}")
    assert len(res) == 2 * 2 * len(R.BWD_EDGE_CASES)


def test_tiled_backward_below_the_short_kernel_limit(dev, default_process, tmp_path):
    """MK_ATTN_NO_SHORT_BWD=1 at head_dim 128, S in {160, 144, 33, 1}, causal with padding: the tiled backward where
    production runs flash_bwd_short_kernel -- against the reference and against the short kernel's result, both within
    the gradient bound"""
    res = _child("no_short_bwd", tmp_path)
    for key, got in res.items():
        _, dn, S = key
        dtype = getattr(torch, dn)
        ref = _case(dtype, 128, 3, 3, S, S, True, "pad11")[5]
        short = default_process[key]
        _check_against_ref(got, ref, f"tiled {key}")
        _check_against_ref(short, ref, f"short {key}")
        for g in ("dq", "dk", "dv"):
            err = (got[g].float() - short[g].float()).abs().max().item()
            lim = 2e-2 * ref[g].abs().max().item() + 2e-3
            assert err <= lim, (key, g, err, lim)
    assert len(res) == 2 * len(SHORT_S)


def test_xcd_grouped_grid_only_renames_workgroups(dev, default_process, tmp_path):
    """MK_ATTN_NO_XCD_GROUP=1 (the 3-D grid) against the grouped 1-D grid of the default process: o and lse of the
    (520, 520) non-causal forward, B H = 9 and 18, 4-wave and 8-wave kernel, bit-identical -- and both correct"""
    res = _child("no_xcd_group", tmp_path)
    for key, got in res.items():
        _, dn, hd, BH, tag = key
        dtype = getattr(torch, dn)
        B, H = next(bh for bh in XCD_BH if bh[0] * bh[1] == BH)
        ref = _case(dtype, hd, B, H, 520, 520, False, "pad77")[5]
        _check_against_ref(default_process[key], ref, f"grouped {key}", grads=False)
        _same_bits(got, default_process[key], f"3-D grid vs grouped {key}")
    assert len(res) == 2 * 2 * len(XCD_BH) * len(XCD_FWD)
