"""The reference and the bounds that tests/test_softmax_ce_gpu.py holds csrc/softmax.hip to (tests/softmax_ref.py) are
themselves checked here, on the CPU: a float32 torch restatement of every kernel, rounded to each dtype, stays inside
every bound at every case the GPU file runs ("the reference alone stays within it" -- a later choice of inputs that does
not satisfy this fails here, not on the GPU); masked_scores is the model's mask rule (oracle/restate.py decoder_mask);
softmax_keep keeps the right fraction, saturates, and depends on the seed and on Lk but not on the pitch; and the
pitch lists select every branch of softmax_fwd_t / softmax_bwd_t on both sides of every threshold."""
import numpy as np
import pytest
import torch

import softmax_ref as R
from oracle import restate

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SOFTMAX_CASES = ([(Lk, ld, m, 2.0) for (Lk, ld) in R.SWEEP_SHAPES for m in R.MASK_MODES] + R.EXTRA_CASES)


@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_restatement_of_the_softmax_stays_inside_the_bounds(dtype):
    worst_p = worst_d = 0.0
    for Lk, ld, mode, sc in SOFTMAX_CASES:
        s, dP = R.make_scores(dtype, Lk, ld, sc)
        km, causal = R.kmask_mode(mode, Lk)
        ref = R.softmax_ref(s, km, causal, R.LQ, Lk, dtype)
        P = R.softmax_f32(s, km, causal, R.LQ, Lk, dtype)
        worst_p = max(worst_p, R.check_inside(P, ref, R.probs_bound(ref, dtype), f"probs {Lk} {mode}"))
        dS_ref, mag = R.softmax_bwd_ref(P, dP, None, 0.0, R.BWD_SCALE)
        dS = R.softmax_bwd_f32(P, dP, None, 0.0, R.BWD_SCALE)
        worst_d = max(worst_d, R.check_inside(dS, dS_ref, R.dS_bound(mag, dtype), f"dS {Lk} {mode}"))
    print(f"{dtype}: worst ratio probs {worst_p:.3f}, dS {worst_d:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_restatement_of_the_dropout_backward_stays_inside_the_bound(dtype):
    for p, pitches in [(R.DROPOUT_P, R.DROPOUT_PITCHES), (0.5, [520])]:
        for ld in pitches:
            Lk = ld - 3
            s, dP = R.make_scores(dtype, Lk, ld)
            P = R.softmax_f32(s, None, False, R.LQ, Lk, dtype)
            keep = R.softmax_keep(R.DROPOUT_SEED, R.NROWS, Lk, p)
            dS_ref, mag = R.softmax_bwd_ref(P, dP, keep, p, R.BWD_SCALE)
            dS = R.softmax_bwd_f32(P, dP, keep, p, R.BWD_SCALE)
            R.check_inside(dS, dS_ref, R.dS_bound(mag, dtype), f"dropout dS {Lk} p={p}")


def test_the_pitch_lists_select_every_branch_on_both_sides_of_every_threshold():
    for dtype in DTYPES:
        n = 4 if dtype == torch.float32 else 8
        for backward, maxcs in [(False, (1, 2, 4, 8)), (True, (1, 2, 4))]:
            want = {f"wave{m}" for m in maxcs} | {"block"}
            assert {R.branch(dtype, ld, backward) for ld in R.PITCHES} == want
            assert {R.branch(dtype, ld, backward) for ld in R.DROPOUT_PITCHES} == want
            for m in maxcs:                                  # the threshold pitch and the next pitch above it
                assert 64 * m * n in R.PITCHES and 64 * m * n + 8 in R.PITCHES
                assert R.branch(dtype, 64 * m * n, backward) != R.branch(dtype, 64 * m * n + 8, backward)
        for Lk, ld in R.SWEEP_SHAPES:
            assert ld % 8 == 0 and 0 < Lk <= ld
    # the pad64 shapes have whole pad chunks, one in a wave and one in the block kernel of the 16-bit forward
    assert [(ld - Lk) // 8 >= 1 and ld % 64 == 0 for Lk, ld in R.SWEEP_SHAPES[-2:]] == [True, True]
    assert {R.branch(torch.bfloat16, ld) for _, ld in R.SWEEP_SHAPES[-2:]} == {"block", "wave8"}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", ["none", "right", "left"])
def test_masked_scores_is_the_decoder_mask_rule(dtype, pad):
    S = 13
    g = torch.Generator().manual_seed(5)
    s = (torch.randn((R.B, R.H, S, S), generator=g) * 2).to(dtype)
    km = None
    if pad != "none":
        km = torch.ones(R.B, S, dtype=torch.int32)
        if pad == "right":
            km[1, -4:] = 0
        else:
            km[1, :3] = 0                                    # rows 0 .. 2 of sample 1 have no allowed key
    m = restate.decoder_mask(km, R.B, S, dtype, torch.device("cpu"))
    model = torch.max(s + m, torch.tensor(torch.finfo(dtype).min, dtype=dtype))
    ours = R.masked_scores(s, km, True, S, S, dtype)
    assert torch.equal(model.double(), ours)
    if pad == "left":
        P = R.softmax_ref(s, km, True, S, S, dtype)
        assert torch.equal(P[1, :, :3], torch.full((R.H, 3, S), 1.0 / S, dtype=torch.float64))
        assert torch.equal(R.softmax_f32(s, km, True, S, S, dtype)[1, :, :3],
                           R.uniform_value(S, dtype).expand(R.H, 3, S))


def test_the_rows_the_gpu_test_expects_uniform_are_uniform():
    for Lk, ld in R.SWEEP_SHAPES:
        km, causal = R.kmask_mode("causal_left", Lk)
        ok = R.allowed(km, causal, R.B, R.LQ, Lk)[:, 0]
        assert not ok[1, :2].any() and ok[1, 2:].any(-1).all() and ok[0].any(-1).all()
        km, causal = R.kmask_mode("kmask", Lk)
        assert R.allowed(km, causal, R.B, R.LQ, Lk)[:, 0].any(-1).all()       # (every row keeps a key)


def test_softmax_keep_fraction_saturation_and_what_it_depends_on():
    nrows, Lk = R.NROWS, 4101
    for p in (0.1, 0.5):
        keep = R.softmax_keep(R.DROPOUT_SEED, nrows, Lk, p)
        n = nrows * Lk
        # five standard deviations of a binomial count
        assert abs(int(keep.sum()) - n * (1 - p)) <= 5 * np.sqrt(n * p * (1 - p))
    # a threshold that saturates keeps everything: (1 - p) 2^32 >= 2^32 - 1
    assert R.keep_threshold(1e-12) == 0xFFFFFFFF and R.softmax_keep(7, nrows, Lk, 1e-12).all()
    assert R.keep_threshold(0.5) == 1 << 31
    a = R.softmax_keep(R.DROPOUT_SEED, nrows, Lk, 0.1)
    assert not torch.equal(a, R.softmax_keep(R.DROPOUT_SEED + 1, nrows, Lk, 0.1))
    # the seed counts modulo 2^64, and its bits above 2^32 count
    assert torch.equal(a, R.softmax_keep(R.DROPOUT_SEED + 2 ** 64, nrows, Lk, 0.1))
    assert not torch.equal(a, R.softmax_keep(R.DROPOUT_SEED - 2 ** 40, nrows, Lk, 0.1))
    # the index is row * Lk + k: another Lk is another pattern, and there is no pitch to depend on -- the pattern of
    # Lk read at a pitch (row * ld + k) is a different one
    b = R.softmax_keep(R.DROPOUT_SEED, nrows, Lk + 3, 0.1)
    assert not torch.equal(a[1:], b[1:, :Lk])
    assert torch.equal(a[0], b[0, :Lk])
    # fp32 1 / (1 - p), as the kernels compute it, is the rounded exact value
    for p in (0.1, 0.5):
        assert R.drop_scale(p) == np.float32(1.0 / (1.0 - p))
    assert R.drop_scale(0.0) == np.float32(1.0)


def test_hash32_matches_the_integer_definition():
    mask = R.MASK64
    for seed, idx in [(123, 7), (R.DROPOUT_SEED, 30 * 4101 - 1), (mask, 2 ** 40 + 5)]:
        z = (idx * 0x9E3779B97F4A7C15 + seed) & mask
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & mask
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        assert int(R.hash32(seed, np.array([idx], dtype=np.uint64))[0]) == (z >> 16) & 0xFFFFFFFF


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.CE_CASES))
def test_f32_restatement_of_the_cross_entropy_stays_inside_the_bounds(name, dtype):
    logits, labels, V = R.make_ce(name, dtype)
    ref = R.ce_ref(logits, labels, V, dtype)
    row_loss, row_lse, sc, dl = R.ce_f32(logits, labels, V)
    R.check_inside(row_lse, ref["row_lse"], ref["row_lse_bound"], "row_lse")
    R.check_inside(row_loss, ref["row_loss"], ref["row_loss_bound"], "row_loss")
    assert abs(sc[0].item() - ref["sum"]) <= ref["sum_bound"]
    assert sc[1].item() == ref["n"]
    assert abs(sc[2].item() - ref["mean"]) <= ref["mean_bound"]
    R.check_inside(dl, ref["dlogits"], ref["dlogits_bound"], "dlogits")
    assert (dl[~ref["valid"]] == 0).all() and (ref["dlogits"][~ref["valid"]] == 0).all()
    rows = logits.shape[0]
    if name == "ignored":
        assert ref["n"] == 0 and ref["sum"] == 0.0 and ref["mean"] == 0.0
    else:
        assert 0 < ref["n"] < rows
    if name == "reduce":
        assert rows > 2 * 256 and ((labels >= V).sum() == 7) and (labels == -100).sum() == rows // 5
    if name == "extreme":
        # past exp's fp32 range: without the max subtraction sum exp(logit) is inf
        assert ref["mean"] > 100 and logits.float().max() > 89 and torch.isfinite(ref["row_lse"]).all()
