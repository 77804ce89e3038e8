"""mk_decode_step_attn_shared (the step attention of generate(num_samples=n): a prompt cache stored once per prompt plus a
tail cache per row) pinned to mk_decode_step_attn BIT FOR BIT: every row's output and appended key are those of the plain
entry point called for the row alone (B = 1, the one-workgroup-per-head form) at the row's position over a physically
gathered cache (tests/shared_attn_ref.py), at every (S0, p) edge of that module's table, for n below, at and above the
rows of a tile with a ragged last tile, with and without per-prompt offsets.  Everything the call must not read holds NaN
bits, everything it must not write is compared with a clone.  A second, independent pin holds one case per (dtype, hd) to
the fp64 reference of tests/decode_attn_ref.py under that module's committed bound.
MK_SHARED_ATTN_ROWS is read at every call, so the R = 1 form is compared in this process.
"""
import hashlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_ref as R  # noqa: E402
import shared_attn_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

DEV = "cuda:0"
H, B, PAD = 2, 2, 2
H16 = [torch.bfloat16, torch.float16]
NS = [1, 2, 3, 5, 9, 32]


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.view(torch.int16)


def _nan_fill(t):
    _bits(t).fill_(torch.tensor(float("nan"), dtype=t.dtype).view(torch.int16).item())


def _inputs(dtype, hd, n, S0, Tn, seed):
    """random prompt [B, S0, 2D], tail [B * n, Tn, 2D], new rows qkv [B * n, 3D] and the model's RoPE tables, on the GPU"""
    D = H * hd
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randn((B, S0, 2 * D), generator=g).to(dtype).to(DEV)
    tail = torch.randn((B * n, Tn, 2 * D), generator=g).to(dtype).to(DEV)
    qkv = torch.randn((B * n, 3 * D), generator=g).to(dtype).to(DEV)
    cos, sin = R.tables(hd, S0 + Tn, dtype)
    return prompt, tail, qkv, cos.to(DEV), sin.to(DEV)


def _shared(qkv, cos, sin, prompt, tail, t_dev, off, S0, n, hd):
    D = H * hd
    out = torch.full((B * n, D), float("nan"), dtype=qkv.dtype, device=DEV)
    ops.decode_step_attn_shared(qkv, qkv, qkv, 3 * D, cos, sin, prompt, tail, _i32([t_dev]),
                                None if off is None else _i32(off), S0, B, n, H, hd, out, hd ** -0.5, k_off=D, v_off=2 * D)
    return out


def _plain_rows(qkv, cos, sin, prompt, tail, Ls, i, n, hd):
    """mk_decode_step_attn for every row alone (B = 1) at *t_dev = L_b + i over its gathered cache -> (outputs [B * n, D],
    appended cache rows [B * n, 2D])"""
    D = H * hd
    out = torch.full((B * n, D), float("nan"), dtype=qkv.dtype, device=DEV)
    app = torch.empty((B * n, 2 * D), dtype=qkv.dtype, device=DEV)
    for b, Lb in enumerate(Ls):
        rows, pos = Lb + i + 1 + PAD, _i32([Lb + i])
        caches = S.gather_caches(prompt, tail, b, n, Lb, i, rows)
        for j in range(n):
            r = b * n + j
            ops.decode_step_attn(qkv[r:r + 1], qkv[r:r + 1], qkv[r:r + 1], 3 * D, cos, sin, caches[j:j + 1], pos, rows, 1, H,
                                 hd, out[r:r + 1], hd ** -0.5, k_off=D, v_off=2 * D)
        app[b * n:(b + 1) * n] = caches[:, Lb + i]
    return out, app


def _check_edge(dtype, hd, n, S0, p, off, seed, t_dev=None, Tn=None):
    """one launch at table edge (S0, p) -- the common counter *t_dev = p, so i = p - S0 -- against the plain calls"""
    i_want = p - S0
    Tn = i_want + 1 + PAD if Tn is None else Tn
    t_dev = p if t_dev is None else t_dev
    i = S.tail_row(t_dev, S0, Tn)
    prompt, tail, qkv, cos, sin = _inputs(dtype, hd, n, S0, Tn, seed)
    Ls = [S.prompt_len(S0, o) for o in (off or [0] * B)]
    for b in range(B):                     # what the call must not read: prompt rows >= L_b, tail rows >= i
        _nan_fill(prompt[b, Ls[b]:])
    _nan_fill(tail[:, i:])
    prompt0, tail0 = prompt.clone(), tail.clone()
    want, app = _plain_rows(qkv, cos, sin, prompt, tail, Ls, i, n, hd)
    got = _shared(qkv, cos, sin, prompt, tail, t_dev, off, S0, n, hd)
    what = (str(dtype), hd, n, S0, p, off, t_dev)
    assert torch.equal(_bits(got), _bits(want)), ("output", what)
    assert torch.equal(_bits(tail[:, i]), _bits(app)), ("appended row", what)
    assert bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(tail[:, i].float()).all()), what
    assert torch.equal(_bits(prompt), _bits(prompt0)), ("prompt bytes", what)
    keep = [t for t in range(Tn) if t != i]
    assert torch.equal(_bits(tail[:, keep]), _bits(tail0[:, keep])), ("other tail bytes", what)
    return got, tail


def _offsets(S0):
    """no offsets, then B = 2 with t_off = [0, -3] and, where S0 >= 1, [-S0 + 1, 0]"""
    return [None, [0, -3]] + ([[-S0 + 1, 0]] if S0 >= 1 else [])


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_every_row_is_the_plain_step_on_its_gathered_cache_bit_for_bit(dtype, hd, n):
    for k, e in enumerate(S.edge_table(R.one_head(hd))):
        for j, off in enumerate(_offsets(e.S0)):
            _check_edge(dtype, hd, n, e.S0, e.p, off, seed=1000 * k + 10 * j + n)


@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_the_position_clamps_into_the_tail(dtype):
    hd, n, S0, Tn = 64, 3, 37, 4
    for t_dev in (-7, S0 - 2, S0, S0 + Tn - 1, S0 + Tn, S0 + Tn + 50):
        for off in (None, [0, -3]):
            _check_edge(dtype, hd, n, S0, S0 + S.tail_row(t_dev, S0, Tn), off, seed=t_dev + 100, t_dev=t_dev, Tn=Tn)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_one_case_per_type_and_head_size_meets_the_fp64_bound(dtype, hd):
    body = R.one_head(hd)
    n, S0, p = 3, body.trip + 1, 2 * body.trip + body.kpp + 1
    i, D = p - S0, H * hd
    got, tail = _check_edge(dtype, hd, n, S0, p, None, seed=7)
    prompt, _, qkv, cos, sin = _inputs(dtype, hd, n, S0, i + 1 + PAD, 7)
    q_rot = qkv[:, :D].clone()
    ops.rope_(q_rot, cos, sin, _i32([p] * (B * n)), H, hd)
    rows = torch.cat([prompt.repeat_interleave(n, 0), tail[:, :i + 1]], 1).cpu()       # the cache after the call
    ref, o_abs = R.ref16(q_rot.cpu(), rows, H, hd, hd ** -0.5)
    R.assert_within(got, ref, o_abs, dtype, f"shared step hd{hd} n{n} S0 {S0} p {p}")


# ------------------------------------------------------------------------------------------ the R = 1 form --
def _digests():
    """{case: sha256 of the output's and the tail's bytes} over a fixed set of cases"""
    out = {}
    for dtype in H16:
        for hd in (64, 128):
            body = R.one_head(hd)
            for n in (3, 32):
                for S0, p, off in ((0, 1, None), (body.kpp, body.trip + 1, [0, -3]),
                                   (body.trip + 1, 2 * body.trip + body.kpp + 1, None)):
                    Tn = p - S0 + 1 + PAD
                    prompt, tail, qkv, cos, sin = _inputs(dtype, hd, n, S0, Tn, 31 * hd + n + p)
                    got = _shared(qkv, cos, sin, prompt, tail, p, off, S0, n, hd)
                    h = hashlib.sha256(_bits(got).cpu().numpy().tobytes())
                    h.update(_bits(tail).cpu().numpy().tobytes())
                    out[f"{dtype} hd{hd} n{n} S0 {S0} p {p} off {off}"] = h.hexdigest()
    return out


def test_the_untiled_form_gives_the_same_bits():
    """MK_SHARED_ATTN_ROWS=1 selects the R = 1 instantiation of the same body, =4 the tiled one; the variable is read at
    every call (os.environ writes through to the C environment), so both run here.  The R = 1 form also passes the whole
    edge table at one n."""
    before = os.environ.get("MK_SHARED_ATTN_ROWS")
    got = {}
    try:
        for rows in ("4", "1"):
            os.environ["MK_SHARED_ATTN_ROWS"] = rows
            got[rows] = _digests()
        for k, e in enumerate(S.edge_table(R.one_head(128))):      # (still "1")
            _check_edge(torch.bfloat16, 128, 3, e.S0, e.p, [0, -3], seed=k)
    finally:
        if before is None:
            del os.environ["MK_SHARED_ATTN_ROWS"]
        else:
            os.environ["MK_SHARED_ATTN_ROWS"] = before
    assert len(got["1"]) == 24 and got["1"] == got["4"]
    assert _digests() == got["4"]                                 # the default is one of the two


# ------------------------------------------------------------------------------------------ return codes --
def test_bad_arguments_return_their_codes_and_launch_nothing():
    dtype, hd, n, S0, Tn = torch.bfloat16, 64, 3, 5, 4
    D = H * hd
    SENT = 7.0
    prompt, tail, qkv, cos, sin = _inputs(dtype, hd, n, S0, Tn, 3)
    out = torch.full((B * n, D), SENT, dtype=dtype, device=DEV)
    t_dev, off = _i32([S0 + 1]), _i32([0, -1])
    prompt0, tail0 = prompt.clone(), tail.clone()
    lib = L.load()
    es = 2

    def raw(q=qkv.data_ptr(), kp=prompt.data_ptr(), kt=tail.data_ptr(), t=t_dev.data_ptr(), toff=off.data_ptr(), S0=S0,
            Tn=Tn, B=B, n=n, H=H, hd=hd, dt=ops.dt(qkv), in_bs=3 * D, p_ld=2 * D, t_ld=2 * D, o=out.data_ptr()):
        return lib.mk_decode_step_attn_shared(q, qkv.data_ptr() + D * es, qkv.data_ptr() + 2 * D * es, in_bs,
                                              cos.data_ptr(), sin.data_ptr(), kp, kp + D * es if kp else None, p_ld,
                                              S0 * 2 * D, kt, kt + D * es if kt else None, t_ld, Tn * 2 * D, o, D, t, toff, S0,
                                              Tn, B, n, H, hd, hd ** -0.5, dt, torch.cuda.current_stream().cuda_stream)
    BAD, UNS = -1, -2
    assert raw(n=0) == BAD and raw(n=-1) == BAD and raw(S0=-1) == BAD and raw(Tn=0) == BAD and raw(B=0) == BAD
    assert raw(H=0) == BAD and raw(q=None) == BAD and raw(kt=None) == BAD and raw(t=None) == BAD and raw(o=None) == BAD
    assert raw(kp=None) == BAD                                  # a prompt of S0 > 0 rows without a pointer
    assert raw(n=33) == UNS and raw(hd=48) == UNS and raw(dt=ops.dt(torch.zeros(1))) == UNS
    assert raw(q=qkv.data_ptr() + 2) == UNS and raw(in_bs=3 * D + 4) == UNS and raw(p_ld=2 * D + 4) == UNS
    assert raw(t_ld=2 * D + 4) == UNS and raw(toff=off.data_ptr() + 2) == UNS
    kw = dict(k_off=D, v_off=2 * D)

    def call(prompt=prompt, tail=tail, off=off, n=n, S0=S0, out=out):
        ops.decode_step_attn_shared(qkv, qkv, qkv, 3 * D, cos, sin, prompt, tail, t_dev, off, S0, B, n, H, hd, out,
                                    hd ** -0.5, **kw)
    for bad in (dict(prompt=prompt.float()), dict(prompt=prompt[:, :4]), dict(prompt=prompt.transpose(0, 1)),
                dict(tail=tail[:B * n - 1]), dict(tail=tail.float()), dict(tail=tail[:, :, :D]), dict(off=off.long()),
                dict(off=_i32([0, 0, 0])), dict(out=out[:B]), dict(S0=S0 + 1), dict(n=n + 1)):
        with pytest.raises(MacawHipError):                      # the wrapper's own checks
            call(**bad)
    with pytest.raises(MacawHipError, match="table rows"):      # RoPE tables shorter than the last position
        ops.decode_step_attn_shared(qkv, qkv, qkv, 3 * D, cos[:S0 + Tn - 1], sin, prompt, tail, t_dev, off, S0, B, n, H, hd,
                                    out, hd ** -0.5, **kw)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and torch.equal(_bits(tail), _bits(tail0)) and torch.equal(_bits(prompt), _bits(prompt0))
    assert raw() == 0                                           # ... and the good call is taken
    torch.cuda.synchronize()
    assert not bool((out == SENT).any()) and torch.equal(_bits(prompt), _bits(prompt0))
    assert ops.shared_attn_ok(dtype, hd, 32) and not ops.shared_attn_ok(dtype, hd, 33)
    assert not ops.shared_attn_ok(dtype, hd, 0) and not ops.shared_attn_ok(torch.float32, hd, 2)
    assert not ops.shared_attn_ok(dtype, 48, 2)

