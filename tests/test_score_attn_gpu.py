"""mk_score_attn (the attention of LlamaForCausalLM.score(): F teacher-forced rows per option over a prompt cache stored once
per prompt and a tail cache per option) pinned to mk_decode_step_attn BIT FOR BIT: a live row's output and appended key are
those of the plain entry point called for the row alone (B = 1, the one-workgroup-per-head form) at the row's position over
a physically gathered cache (tests/shared_attn_ref.py).

One shape throughout: H = 2, B = 2 prompts, n = 3 options with len = (F, 1, 0) for prompt 0 and (F - 1, F, 2) for prompt 1:
full, short and dead options in one launch.  For every S0 of shared_attn_ref.edge_table one launch whose F reaches the
table's largest p, so that a single launch crosses every (S0, p) edge, with t_off in {none, [0, -3], [-S0 + 1, 0]}.  Every
live tail row is compared with decode_attn_ref.rope16 | the value row; the plain reference runs at the table's edges only
(and at every row of the launch with the fewest rows), which keeps a test within a few seconds.  Everything the call must
not read holds NaN bits, everything it must not write is compared with a clone.  A second, independent pin holds one case
per (dtype, hd) to the fp64 reference of tests/decode_attn_ref.py under that module's committed bound.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_ref as R  # noqa: E402
import score_ref as SR  # noqa: E402
import shared_attn_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

DEV = "cuda:0"
H, B, N, PAD = 2, 2, 3, 2
H16 = [torch.bfloat16, torch.float16]
HDS = [16, 32, 64, 128]


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.view(torch.int16)


def _nan_fill(t):
    _bits(t).fill_(torch.tensor(float("nan"), dtype=t.dtype).view(torch.int16).item())


def _lens(F):
    return [F, 1, 0, F - 1, F, 2]


def _offsets(S0):
    return [None, [0, -3]] + ([[-S0 + 1, 0]] if S0 >= 1 else [])


class _Launch:
    """one mk_score_attn launch over poisoned buffers, and what it must have produced"""

    def __init__(self, dtype, hd, S0, F, off, seed):
        D = H * hd
        self.dtype, self.hd, self.S0, self.F, self.D = dtype, hd, S0, F, D
        self.Ls = [SR.prompt_len(S0, o) for o in (off or [0] * B)]
        self.f = SR.fed_rows(_lens(F), F)
        g = torch.Generator().manual_seed(seed)
        self.prompt = torch.randn((B, S0, 2 * D), generator=g).to(dtype).to(DEV)
        self.qkv = torch.randn((B * N * F, 3 * D), generator=g).to(dtype).to(DEV)
        self.tail = torch.empty((B * N, F, 2 * D), dtype=dtype, device=DEV)
        cos, sin = R.tables(hd, S0 + F, dtype)
        self.cos, self.sin = cos.to(DEV), sin.to(DEV)
        self.live = (torch.arange(F, device=DEV)[None, :] < _i32(self.f)[:, None])             # [B * n, F]
        self.pos = (torch.tensor(self.Ls, device=DEV).repeat_interleave(N)[:, None] + torch.arange(F, device=DEV)[None, :])
        # what the call must not read: prompt rows >= L_b, the whole tail, the q / k / v of dead rows
        for b in range(B):
            _nan_fill(self.prompt[b, self.Ls[b]:])
        _nan_fill(self.tail)
        self.qkv.view(B * N, F, 3 * D)[~self.live] = float("nan")
        self.prompt0 = self.prompt.clone()
        self.out = torch.full((B * N * F, D), float("nan"), dtype=dtype, device=DEV)
        ops.score_attn(self.qkv, self.qkv, self.qkv, 3 * D, self.cos, self.sin, self.prompt, self.tail, _i32(_lens(F)),
                       None if off is None else _i32(off), S0, B, N, H, hd, self.out, hd ** -0.5, k_off=D, v_off=2 * D)
        # the expected tail: rope16 of every row's key at its position | its value
        k_rot = R.rope16(self.qkv[:, D:2 * D], self.cos, self.sin, self.pos.reshape(-1), hd)
        self.want_tail = torch.cat([k_rot, self.qkv[:, 2 * D:]], dim=1).view(B * N, F, 2 * D)
        self.what = (str(dtype), hd, S0, F, off)

    def check_poison_and_tail(self):
        out, live, what = self.out.view(B * N, self.F, self.D), self.live, self.what
        assert bool(torch.isfinite(out[live].float()).all()) and bool(torch.isfinite(self.tail[live].float()).all()), what
        assert bool((_bits(out[~live]) == 0).all()), ("a dead row's output is exactly zero", what)
        nan = torch.tensor(float("nan"), dtype=self.dtype).view(torch.int16).item()
        assert bool((_bits(self.tail[~live]) == nan).all()), ("a dead tail row was written", what)
        assert torch.equal(_bits(self.prompt), _bits(self.prompt0)), ("prompt bytes", what)
        assert torch.equal(_bits(self.tail[live]), _bits(self.want_tail[live])), ("live tail rows", what)

    def check_row(self, opt, g):
        """row (opt, g) against mk_decode_step_attn for the row alone over the gathered cache built from the EXPECTED tail"""
        D, hd, Lb = self.D, self.hd, self.Ls[opt // N]
        assert g < self.f[opt]
        p, r = Lb + g, opt * self.F + g
        rows = p + 1 + PAD
        cache = S.gather_cache(self.prompt, self.want_tail, opt, N, Lb, g, rows)
        want = torch.full((1, D), float("nan"), dtype=self.dtype, device=DEV)
        ops.decode_step_attn(self.qkv[r:r + 1], self.qkv[r:r + 1], self.qkv[r:r + 1], 3 * D, self.cos, self.sin, cache,
                             _i32([p]), rows, 1, H, hd, want, hd ** -0.5, k_off=D, v_off=2 * D)
        assert torch.equal(_bits(self.out[r:r + 1]), _bits(want)), ("output", self.what, opt, g, p)
        assert torch.equal(_bits(self.tail[opt, g]), _bits(cache[0, p])), ("appended row", self.what, opt, g, p)

    def check_position(self, p):
        """every live row of the launch that runs at position p"""
        n = 0
        for opt in range(B * N):
            g = p - self.Ls[opt // N]
            if 0 <= g < self.f[opt]:
                self.check_row(opt, g)
                n += 1
        return n


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_every_live_row_is_the_plain_step_on_its_gathered_cache_bit_for_bit(dtype, hd):
    table = S.edge_table(R.one_head(hd))
    p_max = max(e.p for e in table)
    smallest, checked = None, 0
    for k, S0 in enumerate(sorted({e.S0 for e in table})):
        for j, off in enumerate(_offsets(S0)):
            Ls = [SR.prompt_len(S0, o) for o in (off or [0] * B)]
            F = max(p_max - min(Ls) + 1, 3)                 # the full options reach the table's largest p
            run = _Launch(dtype, hd, S0, F, off, seed=100 * k + j)
            run.check_poison_and_tail()
            for e in table:
                if e.S0 == S0:
                    n = run.check_position(e.p)
                    assert n >= 1 or e.p < min(Ls), (run.what, e)
                    checked += n
            if smallest is None or F < smallest.F:
                smallest = run
    for opt, g in SR.live_rows(_lens(smallest.F), smallest.F):     # every row of the launch with the fewest rows
        smallest.check_row(opt, g)
    print(f"[score-attn] {dtype} hd{hd}: {checked} rows pinned at the table's edges, p up to {p_max}")


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_poison_stays_where_it_was_and_dead_rows_are_zero(dtype, hd):
    body = R.one_head(hd)
    for S0, off in ((body.kpp + 1, [0, -3]), (0, None), (5, [-4, 0])):
        run = _Launch(dtype, hd, S0, 7, off, seed=S0 + hd)
        run.check_poison_and_tail()
        assert int(run.live.sum()) == 7 + 1 + 0 + 6 + 7 + 2
        for opt, g in SR.live_rows(_lens(7), 7):
            run.check_row(opt, g)
    # a count outside [0, F] clamps: -5 is a dead option, F + 9 a full one
    D, F, S0 = H * hd, 4, 6
    run = _Launch(dtype, hd, S0, F, None, seed=1)
    out = torch.full_like(run.out, float("nan"))
    tail = torch.full_like(run.tail, 0)
    qkv = run.qkv.clone()
    qkv.view(B * N, F, 3 * D)[0] = torch.randn((F, 3 * D)).to(dtype).to(DEV)        # option 0 is live in both launches
    ops.score_attn(qkv, qkv, qkv, 3 * D, run.cos, run.sin, run.prompt, tail, _i32([F + 9, -5, 0, 0, 0, 0]), None, S0, B, N, H,
                   hd, out, hd ** -0.5, k_off=D, v_off=2 * D)
    out = out.view(B * N, F, D)
    assert bool(torch.isfinite(out[0].float()).all()) and bool((_bits(out[1:]) == 0).all())
    assert bool((_bits(tail[1:]) == 0).all()) and bool(torch.isfinite(tail[0].float()).all())


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_one_case_per_type_and_head_size_meets_the_fp64_bound(dtype, hd):
    body = R.one_head(hd)
    S0, F, D = body.trip + 1, body.trip + body.kpp + 3, H * hd
    run = _Launch(dtype, hd, S0, F, None, seed=7)
    run.check_poison_and_tail()
    opts = [0, N + 1]                                        # the two full options; their last rows run at p = S0 + F - 1
    rows = torch.tensor([o * F + F - 1 for o in opts], device=DEV)
    q_rot = run.qkv[rows, :D].clone()
    ops.rope_(q_rot, run.cos, run.sin, _i32([S0 + F - 1] * 2), H, hd)
    cache = torch.cat([run.prompt, run.tail[opts]], dim=1).cpu()          # the caches after the call
    ref, o_abs = R.ref16(q_rot.cpu(), cache, H, hd, hd ** -0.5)
    R.assert_within(run.out[rows], ref, o_abs, dtype, f"score attention hd{hd} S0 {S0} F {F}")


def test_many_rows_split_over_launches_give_the_same_bits_as_few():
    """B * n * F > 65535 rows: grid.y cannot carry them in one launch.  One prompt's options are those of the small launch
    above, repeated: every repetition must come out with the same bits"""
    dtype, hd, S0, F = torch.bfloat16, 16, 3, 6
    D, n, Bb = H * hd, 32, 400                                # 400 * 32 * 6 = 76800 rows
    g = torch.Generator().manual_seed(5)
    prompt1 = torch.randn((1, S0, 2 * D), generator=g).to(dtype).to(DEV)
    qkv1 = torch.randn((n * F, 3 * D), generator=g).to(dtype).to(DEV)
    lens1 = torch.randint(0, F + 1, (n,), generator=g).to(torch.int32).to(DEV)
    cos, sin = (t.to(DEV) for t in R.tables(hd, S0 + F, dtype))

    def run(Bx):
        out = torch.full((Bx * n * F, D), float("nan"), dtype=dtype, device=DEV)
        tail = torch.zeros((Bx * n, F, 2 * D), dtype=dtype, device=DEV)
        q = qkv1.repeat(Bx, 1)
        ops.score_attn(q, q, q, 3 * D, cos, sin, prompt1.repeat(Bx, 1, 1).contiguous(), tail, lens1.repeat(Bx).contiguous(),
                       None, S0, Bx, n, H, hd, out, hd ** -0.5, k_off=D, v_off=2 * D)
        return out, tail
    o1, t1 = run(1)
    oB, tB = run(Bb)
    assert torch.equal(_bits(oB.view(Bb, -1)), _bits(o1.view(1, -1)).expand(Bb, -1))
    assert torch.equal(_bits(tB.view(Bb, -1)), _bits(t1.view(1, -1)).expand(Bb, -1))


# ------------------------------------------------------------------------------------------ return codes --
def test_bad_arguments_return_their_codes_and_launch_nothing():
    dtype, hd, S0, F = torch.bfloat16, 64, 5, 4
    D = H * hd
    SENT = 7.0
    g = torch.Generator().manual_seed(3)
    prompt = torch.randn((B, S0, 2 * D), generator=g).to(dtype).to(DEV)
    tail = torch.randn((B * N, F, 2 * D), generator=g).to(dtype).to(DEV)
    qkv = torch.randn((B * N * F, 3 * D), generator=g).to(dtype).to(DEV)
    cos, sin = (t.to(DEV) for t in R.tables(hd, S0 + F, dtype))
    out = torch.full((B * N * F, D), SENT, dtype=dtype, device=DEV)
    lens, off = _i32(_lens(F)), _i32([0, -1])
    prompt0, tail0 = prompt.clone(), tail.clone()
    lib = L.load()
    es = 2

    def raw(q=qkv.data_ptr(), kp=prompt.data_ptr(), kt=tail.data_ptr(), ln=lens.data_ptr(), toff=off.data_ptr(), S0=S0, F=F,
            B=B, n=N, H=H, hd=hd, dt=ops.dt(qkv), in_bs=3 * D, p_ld=2 * D, t_ld=2 * D, o=out.data_ptr(), cs=cos.data_ptr()):
        return lib.mk_score_attn(q, qkv.data_ptr() + D * es, qkv.data_ptr() + 2 * D * es, in_bs, cs, sin.data_ptr(), kp,
                                 kp + D * es if kp else None, p_ld, S0 * 2 * D, kt, kt + D * es if kt else None, t_ld,
                                 F * 2 * D, o, D, ln, toff, S0, F, B, n, H, hd, hd ** -0.5, dt,
                                 torch.cuda.current_stream().cuda_stream)
    BAD, UNS = -1, -2
    assert raw(n=0) == BAD and raw(n=-1) == BAD and raw(S0=-1) == BAD and raw(F=0) == BAD and raw(B=0) == BAD
    assert raw(H=0) == BAD and raw(q=None) == BAD and raw(kt=None) == BAD and raw(ln=None) == BAD and raw(o=None) == BAD
    assert raw(cs=None) == BAD
    assert raw(kp=None) == BAD                                  # a prompt of S0 > 0 rows without a pointer
    assert raw(hd=48) == UNS and raw(dt=ops.dt(torch.zeros(1))) == UNS
    assert raw(q=qkv.data_ptr() + 2) == UNS and raw(in_bs=3 * D + 4) == UNS and raw(p_ld=2 * D + 4) == UNS
    assert raw(t_ld=2 * D + 4) == UNS and raw(toff=off.data_ptr() + 2) == UNS and raw(ln=lens.data_ptr() + 2) == UNS
    kw = dict(k_off=D, v_off=2 * D)

    def call(prompt=prompt, tail=tail, lens=lens, off=off, n=N, S0=S0, out=out, cos=cos):
        ops.score_attn(qkv, qkv, qkv, 3 * D, cos, sin, prompt, tail, lens, off, S0, B, n, H, hd, out, hd ** -0.5, **kw)
    for bad in (dict(prompt=prompt.float()), dict(prompt=prompt[:, :4]), dict(prompt=prompt.transpose(0, 1)),
                dict(tail=tail[:B * N - 1]), dict(tail=tail.float()), dict(tail=tail[:, :, :D]), dict(off=off.long()),
                dict(off=_i32([0, 0, 0])), dict(lens=lens.long()), dict(lens=lens[:5]), dict(out=out[:B]), dict(S0=S0 + 1),
                dict(n=N + 1)):
        with pytest.raises(MacawHipError):                      # the wrapper's own checks
            call(**bad)
    with pytest.raises(MacawHipError, match="table rows"):      # RoPE tables shorter than the last position
        call(cos=cos[:S0 + F - 1])
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and torch.equal(_bits(tail), _bits(tail0)) and torch.equal(_bits(prompt), _bits(prompt0))
    assert raw() == 0 and raw(toff=None) == 0                   # ... and the good calls are taken
    torch.cuda.synchronize()
    assert not bool((out == SENT).any()) and torch.equal(_bits(prompt), _bits(prompt0))
    for dt in H16:
        assert all(ops.score_attn_ok(dt, h) for h in HDS) and not ops.score_attn_ok(dt, 48)
    assert not ops.score_attn_ok(torch.float32, 64) and not ops.score_attn_ok(torch.bfloat16, 64, 0)
