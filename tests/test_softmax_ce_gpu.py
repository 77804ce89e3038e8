"""GPU: csrc/softmax.hip -- the eager attention softmax (forward and backward), the attention dropout and the shifted
cross-entropy -- against the float64 reference and the derived elementwise bounds of tests/softmax_ref.py, at every
branch of the dispatch (softmax_fwd_t / softmax_bwd_t: the table is beside softmax_ref.branch), on both sides of every
threshold, in all three dtypes, with NaN in the pad columns of every buffer that goes in.

The rows are few (B = 2, H = 3, Lq = 5: 30 rows, no multiple of the wave kernels' 4 rows per block); the pitches are the
kernels' own.  Dropout is checked exactly, against the numpy restatement of the hash, never against the kernel's own
output.  tests/test_softmax_ref_cpu.py shows that a float32 restatement alone stays inside every bound used here.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import softmax_ref as R  # noqa: E402
from test_kernels_gpu import DTYPES  # noqa: E402

from macaw_llm_amd import ops  # noqa: E402

NZ = R.B * R.H
SEED = R.DROPOUT_SEED
OFFSET = 777_777_777_777          # (above 2^32 as well)


def _pitched(x, ld, dev):
    """x [..., n] -> device buffer [..., ld] whose pad columns [n, ld) are NaN"""
    buf = torch.full(x.shape[:-1] + (ld,), float("nan"), dtype=x.dtype, device=dev)
    buf[..., :x.shape[-1]] = x.to(dev)
    return buf


def _fwd(buf, Lk, ld, km=None, causal=False, **kw):
    return ops.softmax_fwd(buf, NZ, R.H, R.LQ, Lk, ld, kmask=km, causal=causal, **kw)


def _bwd(probs, dP, Lk, ld, dev, **kw):
    """dS of the pitched, NaN-padded gradient, in place as engine.attention_bwd runs it"""
    return ops.softmax_bwd_(probs, _pitched(dP, ld, dev), NZ, R.LQ, Lk, ld, scale=R.BWD_SCALE, **kw)


def _pads_are_zero(buf, n, what):
    assert (buf[..., n:] == 0).all(), f"{what}: pad columns not exactly 0"


def _softmax_case(dev, dtype, Lk, ld, mode, score_scale):
    s, dP = R.make_scores(dtype, Lk, ld, score_scale)
    km, causal = R.kmask_mode(mode, Lk)
    kd = km.to(dev) if km is not None else None
    buf = _pitched(s, ld, dev)
    probs, _ = _fwd(buf, Lk, ld, kd, causal)
    ref = R.softmax_ref(s, km, causal, R.LQ, Lk, dtype)
    ratio = R.check_inside(probs[..., :Lk], ref, R.probs_bound(ref, dtype), "probs")
    _pads_are_zero(probs, Lk, "probs")
    if mode == "causal_left":          # query rows 0, 1 of sample 1 have no allowed key
        assert torch.equal(probs[1, :, :2, :Lk].cpu(), R.uniform_value(Lk, dtype).expand(R.H, 2, Lk))
    if mode == "full1":
        assert torch.equal(probs[1, ..., :Lk].cpu(), R.uniform_value(Lk, dtype).expand(R.H, R.LQ, Lk))
    again, _ = _fwd(buf, Lk, ld, kd, causal)
    assert torch.equal(again, probs), "two runs differ"
    inplace = buf.clone()
    _fwd(inplace, Lk, ld, kd, causal, probs=inplace)       # as engine.attention_fwd calls it
    assert torch.equal(inplace, probs), "in place differs from out of place"
    # backward, from the kernel's own rounded P
    dS_ref, mag = R.softmax_bwd_ref(probs[..., :Lk].cpu(), dP, None, 0.0, R.BWD_SCALE)
    dS = _bwd(probs, dP, Lk, ld, dev)
    ratio_d = R.check_inside(dS[..., :Lk], dS_ref, R.dS_bound(mag, dtype), "dS")
    _pads_are_zero(dS, Lk, "dS")
    print(f"softmax {dtype} Lk={Lk} ld={ld} {mode}: fwd {R.branch(dtype, ld)} {ratio:.3f} of the bound, "
          f"bwd {R.branch(dtype, ld, True)} {ratio_d:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", R.MASK_MODES)
@pytest.mark.parametrize("Lk,ld", R.SWEEP_SHAPES)
def test_softmax_dispatch_sweep(dev, dtype, Lk, ld, mode):
    _softmax_case(dev, dtype, Lk, ld, mode, 2.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lk,ld,mode,score_scale", R.EXTRA_CASES)
def test_softmax_fully_masked_sample_and_wide_scores(dev, dtype, Lk, ld, mode, score_scale):
    _softmax_case(dev, dtype, Lk, ld, mode, score_scale)


def _dropout_fwd_bwd(dev, dtype, Lk, ld, p, seed, mask_seed):
    """forward and backward with dropout at `seed`, held to the numpy mask of `mask_seed` -> (probs_dropped, dS)"""
    s, dP = R.make_scores(dtype, Lk, ld)
    buf = _pitched(s, ld, dev)
    plain, _ = _fwd(buf, Lk, ld)
    probs, pd = _fwd(buf, Lk, ld, dropout_p=p, seed=seed, want_dropped=True)
    assert torch.equal(probs, plain), "probs depend on the dropout"
    keep = R.softmax_keep(mask_seed, R.NROWS, Lk, p)
    assert torch.equal(pd[..., :Lk].cpu(), R.dropped_f32(probs[..., :Lk].cpu(), keep, p)), "probs_dropped"
    _pads_are_zero(pd, Lk, "probs_dropped")
    dS_ref, mag = R.softmax_bwd_ref(probs[..., :Lk].cpu(), dP, keep, p, R.BWD_SCALE)
    dS = _bwd(probs, dP, Lk, ld, dev, dropout_p=p, seed=seed)
    R.check_inside(dS[..., :Lk], dS_ref, R.dS_bound(mag, dtype), "dropout dS")
    _pads_are_zero(dS, Lk, "dropout dS")
    return pd, dS


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ld,p", [(ld, R.DROPOUT_P) for ld in R.DROPOUT_PITCHES] + [(520, 0.5)])
def test_dropout_is_exactly_the_hashed_mask(dev, dtype, ld, p):
    _dropout_fwd_bwd(dev, dtype, ld - 3, ld, p, SEED, SEED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lk,ld8,ld64", R.SAME_LK_PITCHES)
def test_dropout_pattern_does_not_depend_on_the_pitch(dev, dtype, Lk, ld8, ld64):
    s, _ = R.make_scores(dtype, Lk, ld8)
    keep = R.softmax_keep(SEED, R.NROWS, Lk, R.DROPOUT_P)
    got = []
    for ld in (ld8, ld64):
        probs, pd = _fwd(_pitched(s, ld, dev), Lk, ld, dropout_p=R.DROPOUT_P, seed=SEED, want_dropped=True)
        assert torch.equal(pd[..., :Lk].cpu(), R.dropped_f32(probs[..., :Lk].cpu(), keep, R.DROPOUT_P))
        _pads_are_zero(pd, Lk, "probs_dropped")
        got.append(pd[..., :Lk])
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ld", [264, 4104])          # a wave kernel and the block kernel, forward and backward
def test_dropout_seed_offset_in_device_memory(dev, dtype, ld):
    Lk, p = ld - 3, R.DROPOUT_P
    want_pd, want_dS = _dropout_fwd_bwd(dev, dtype, Lk, ld, p, SEED + OFFSET, SEED + OFFSET)
    t = torch.tensor([OFFSET], dtype=torch.int64, device=dev)
    try:
        ops.set_dropout_seed_offset(t)
        pd, dS = _dropout_fwd_bwd(dev, dtype, Lk, ld, p, SEED, SEED + OFFSET)
        assert torch.equal(pd, want_pd) and torch.equal(dS, want_dS)
        t.add_(1)                                    # what a replayed training step does between two replays
        pd2, _ = _dropout_fwd_bwd(dev, dtype, Lk, ld, p, SEED, SEED + OFFSET + 1)
        assert not torch.equal(pd2 != 0, pd != 0)
    finally:
        ops.set_dropout_seed_offset(None)
    _dropout_fwd_bwd(dev, dtype, Lk, ld, p, SEED, SEED)      # cleared: the seed argument alone again


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.CE_CASES))
def test_cross_entropy_cases(dev, dtype, name):
    logits, labels, V = R.make_ce(name, dtype)
    rows, ld = logits.shape[0], R.pad64(V)           # the pitch LMHeadLossFn builds
    buf = _pitched(logits, ld, dev)
    lab = labels.to(dev)
    ref = R.ce_ref(logits, labels, V, dtype)
    row_loss, row_lse, sc = ops.cross_entropy(buf, lab, V)
    R.check_inside(row_lse, ref["row_lse"], ref["row_lse_bound"], "row_lse")
    R.check_inside(row_loss, ref["row_loss"], ref["row_loss_bound"], "row_loss")
    bad = ~ref["valid"]
    assert (row_lse.cpu()[bad] == 0).all() and (row_loss.cpu()[bad] == 0).all()
    sc_h = sc.double().cpu()
    print(f"ce {name} {dtype}: sum_cnt {sc_h.tolist()} ref {ref['sum']} {ref['n']} {ref['mean']}")
    assert torch.isfinite(sc_h).all()
    assert abs(sc_h[0].item() - ref["sum"]) <= ref["sum_bound"]
    assert sc_h[1].item() == ref["n"]
    assert abs(sc_h[2].item() - ref["mean"]) <= ref["mean_bound"]
    assert sc_h[3].item() == 0
    # the backward as the engine calls it: part of the scale in device memory
    half = torch.tensor(0.5, dtype=torch.float32, device=dev)
    dl = ops.cross_entropy_bwd(buf, lab, row_lse, sc, V, grad_scale=2.0, grad_scale_dev=half)
    dl_host = ops.cross_entropy_bwd(buf, lab, row_lse, sc, V, grad_scale=1.0)
    assert torch.equal(dl, dl_host)
    R.check_inside(dl[:, :V], ref["dlogits"], ref["dlogits_bound"], "dlogits")
    _pads_are_zero(dl, V, "dlogits")
    assert (dl.cpu()[bad] == 0).all()
    if name == "ignored":
        assert sc_h.tolist() == [0, 0, 0, 0] and (dl == 0).all()
