"""GPU: the template instantiations and host branches that the shapes of tests/test_kernels_gpu.py do not select, against
fp32 / float64 torch restatements on the same rounded inputs (tolerances: test_kernels_gpu._tol / _close):
  - RMSNorm / LayerNorm backward with more rows than blocks (a block owns several rows: the next-row prefetch of the
    narrow RMSNorm kernel and the per-block dw / db sums), and the CH = 4 / 8 instantiations;
  - mk_sumsq (global gradient norm): scalar tail, one block, and the grid-stride loop past 1024 blocks;
  - mk_swiglu2d_bwd at the LLaMA FF widths, mk_argmax_rows (pitched, padded, ties, -inf and NaN rows), and the
    > 1024-repeats fallback of mk_embedding_bwd."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_kernels_gpu import DTYPES, _close, _rand  # noqa: E402

from macaw_llm_amd import ops  # noqa: E402
from oracle import restate  # noqa: E402


# ------------------------------------------------------------------------------------------ norms --
# rows > blocks (ops.RMSNORM_BLOCKS = 256, ops.NORM_BLOCKS = 512).  RMSNorm instantiation by CH = ceil(cols / 8 / 256)
# for 16-bit, ceil(cols / 4 / 256) for fp32: 4096 -> CH 2 with prefetch (16-bit) / CH 4 (fp32); 5120 -> CH 4 (16-bit) /
# CH 8 (fp32); 8704 -> CH 8 (16-bit); 1024 fp32 -> CH 1 with prefetch
RMS_CASES = [(dtype, 4608, 4096) for dtype in DTYPES] + [(dtype, 1100, 5120) for dtype in DTYPES] + \
            [(torch.bfloat16, 600, 8704), (torch.float16, 600, 8704), (torch.float32, 777, 1024)]


@pytest.mark.parametrize("dtype,rows,cols", RMS_CASES)
def test_rmsnorm_bwd_blocks_own_several_rows(dev, dtype, rows, cols):
    assert rows > ops.RMSNORM_BLOCKS
    g = torch.Generator().manual_seed(rows + cols)
    x = _rand((rows, cols), dtype, g)
    w = (1 + 0.1 * torch.randn(cols, generator=g)).to(dtype)
    dy, dres = _rand((rows, cols), dtype, g), _rand((rows, cols), dtype, g)
    h, _, rstd = ops.rmsnorm_fwd(x.to(dev), w.to(dev), 1e-6)
    hf, wf = x.float().requires_grad_(True), w.float().requires_grad_(True)
    restate.rms_norm(hf, wf, 1e-6).backward(dy.float())
    dx, dw = ops.rmsnorm_bwd(dy.to(dev), h, w.to(dev), rstd, dres=dres.to(dev))
    dx2, dw2 = ops.rmsnorm_bwd(dy.to(dev), h, w.to(dev), rstd, dres=dres.to(dev))
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)
    _close(dx, hf.grad + dres.float(), dtype, scale=2.0, what="rmsnorm dx")
    _close(dw, wf.grad, dtype, scale=math.sqrt(rows), what="rmsnorm dw")
    # without the residual gradient (the prefetch selects the dy stream in its place)
    dx3, _ = ops.rmsnorm_bwd(dy.to(dev), h, w.to(dev), rstd)
    _close(dx3, hf.grad, dtype, scale=2.0, what="rmsnorm dx (no dres)")


# LayerNorm: CH = ceil(cols / 256): 512 -> 2, 1024 -> 4, 1280 -> 8
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(1300, 1024), (1300, 512), (1300, 1280)])
def test_layernorm_bwd_blocks_own_several_rows(dev, dtype, rows, cols):
    assert rows > ops.NORM_BLOCKS
    g = torch.Generator().manual_seed(rows * cols)
    x = _rand((rows, cols), dtype, g)
    w, b = (1 + 0.1 * torch.randn(cols, generator=g)).to(dtype), (0.1 * torch.randn(cols, generator=g)).to(dtype)
    dy, dres = _rand((rows, cols), dtype, g), _rand((rows, cols), dtype, g)
    _, mean, rstd = ops.layernorm_fwd(x.to(dev), w.to(dev), b.to(dev), 1e-5)
    xf, wf, bf = x.float().requires_grad_(True), w.float().requires_grad_(True), b.float().requires_grad_(True)
    F.layer_norm(xf, (cols,), wf, bf, 1e-5).backward(dy.float())
    dx, dw, db = ops.layernorm_bwd(dy.to(dev), x.to(dev), w.to(dev), mean, rstd, dres=dres.to(dev))
    dx2, dw2, db2 = ops.layernorm_bwd(dy.to(dev), x.to(dev), w.to(dev), mean, rstd, dres=dres.to(dev))
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    _close(dx, xf.grad + dres.float(), dtype, scale=2.0, what="layernorm dx")
    _close(dw, wf.grad, dtype, scale=math.sqrt(rows), what="layernorm dw")
    _close(db, bf.grad, dtype, scale=math.sqrt(rows), what="layernorm db")


# ------------------------------------------------------------------------------------------ sumsq --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 8192, 8 * 2 ** 20 + 13])
def test_sumsq_tail_single_block_and_grid_stride(dev, dtype, n):
    """n = 1, 7: no full vector, block 0's scalar tail only; 8192: one block; 8 Mi + 13: 1024 blocks that stride over
    the rest, plus a tail of 13 % (16 B / element size) elements"""
    g = torch.Generator().manual_seed(n)
    x = _rand((n,), dtype, g)
    xd = x.to(dev)
    assert xd.data_ptr() % 16 == 0
    ref = float(x.double().pow(2).sum())
    s1 = ops.sumsq(xd)
    s2 = ops.sumsq(xd)
    assert torch.equal(s1, s2)
    assert abs(float(s1) - ref) <= 1e-5 * ref, (float(s1), ref)
    acc = torch.full((1,), 3.25, dtype=torch.float32, device=dev)
    ops.sumsq(xd, out=acc, accumulate=True)
    assert abs(float(acc) - (ref + 3.25)) <= 1e-5 * (ref + 3.25), (float(acc), ref)
    ops.sumsq(xd, out=acc, accumulate=False)
    assert torch.equal(acc, s1)


# ------------------------------------------------------------------------------------ swiglu2d bwd --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(37, 11008), (21, 13824)])
def test_swiglu2d_bwd_at_the_ff_widths(dev, dtype, rows, cols):
    g = torch.Generator().manual_seed(rows + cols)
    gu, da = _rand((rows, 2 * cols), dtype, g), _rand((rows, cols), dtype, g)
    dgu = ops.swiglu2d_bwd(gu.to(dev), da.to(dev), cols)
    gf = gu[:, :cols].float().requires_grad_(True)
    uf = gu[:, cols:].float().requires_grad_(True)
    a = F.silu(gf) * uf
    _close(ops.swiglu2d_fwd(gu.to(dev), cols), a.detach(), dtype, what="swiglu2d fwd")
    a.backward(da.float())
    _close(dgu[:, :cols], gf.grad, dtype, scale=2.0, what="swiglu2d dgate")
    _close(dgu[:, cols:], uf.grad, dtype, scale=2.0, what="swiglu2d dup")


# ------------------------------------------------------------------------------------------ argmax --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [32000, 32007])
def test_argmax_rows_pitched_ties_inf_and_nan(dev, dtype, V):
    """torch.argmax of the fp32 row: first maximum, a row of -inf gives 0, a row with NaN gives its first NaN; the
    pad columns [V, ld) hold garbage that must not be read"""
    g = torch.Generator().manual_seed(V)
    rows, ld = 8, 32064
    x = _rand((rows, ld), dtype, g)
    x[:, V:] = 1e4
    x[:, V + 1] = float("nan")
    x[1, 17] = x[1, 900] = x[1, V - 1] = 30.0               # tie: lowest index
    x[2, V - 1] = 30.0                                       # the last valid column
    x[3, :V] = float("-inf")                                 # all -inf
    x[4, 5000] = x[4, 6000] = float("nan")                   # first NaN, not the maximum
    x[4, 100] = 30.0
    x[5, :V] = float("nan")                                  # all NaN
    x[6, :V] = -3.0                                          # all equal
    x[6, :V // 2] = float("-inf")
    want = x[:, :V].float().argmax(1)
    assert want[1:7].tolist() == [17, V - 1, 0, 5000, 0, V // 2]
    xd = x.to(dev)
    got = ops.argmax_rows(xd[:, :V], V)
    assert torch.equal(got.cpu(), want), (got.cpu(), want)


# ------------------------------------------------------------------------------------- embedding bwd --
@pytest.mark.parametrize("dtype", DTYPES)
def test_embedding_bwd_many_repeats_padding_and_out_of_range(dev, dtype):
    """4096 tokens: one id 1500 times (> MAXM = 1024 later occurrences: the linear-scan fallback), one id 1025 times
    (exactly MAXM later occurrences: the LDS list), padding_idx and out-of-range ids (skipped), against a float64
    scatter-add; two runs bit-identical"""
    g = torch.Generator().manual_seed(4096)
    V, D, T, pad = 3000, 1032, 4096, 11
    ids = torch.randint(0, V, (T,), generator=g)
    perm = torch.randperm(T, generator=g)
    ids[perm[:1500]] = 7
    ids[perm[1500:2525]] = 2999
    ids[perm[2525:2600]] = pad
    ids[perm[2600:2610]] = V + 5
    ids[perm[2610:2620]] = -3
    dout = _rand((T, D), dtype, g)
    dt0 = _rand((V, D), dtype, g)
    keep = (ids >= 0) & (ids < V) & (ids != pad)
    ref = dt0.double().index_add(0, ids[keep], dout[keep].double())
    outs = []
    for _ in range(2):
        dtab = dt0.to(dev)
        ops.embedding_bwd_(dtab, dout.to(dev), ids.to(dev), padding_idx=pad)
        outs.append(dtab)
    assert torch.equal(outs[0], outs[1])
    _close(outs[0], ref, dtype, scale=math.sqrt(1500), what="embedding bwd")
    assert torch.equal(outs[0][pad].cpu(), dt0[pad])
