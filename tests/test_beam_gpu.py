"""GPU: beam search -- mk_beam_emit (csrc/beam.hip) against the float64 restatement of tests/beam_ref.py, ties and
non-finite logits, finished samples and the state hand-off, mk_decode_step_attn_beam against mk_decode_step_attn on a
physically gathered cache (bit for bit), and generate(num_beams=K) end to end on the hipGraph path, the
kernel-by-kernel loop and use_cache=False.

Score bound of the selection test (derived per case and printed): what a step adds to a score is a log-probability,
x - lse; torch's own fp32 log_softmax differs from float64 by e on the same rows, and the kernel is allowed 4 e."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_ref as R  # noqa: E402
from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_decode_kv8_gpu import _Spy, _ids, _small_llama  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.MM_LLMs.set_beam_search()
    ops.clear_fp8_cache()


def _log_softmax_bound(xq):
    """4 x the error of torch's fp32 log_softmax against float64 on these rows (xq: float32 tensor of the quantised
    logits, any leading shape)"""
    x = xq.reshape(-1, xq.shape[-1])
    e = (torch.log_softmax(x.float(), -1).double() - torch.log_softmax(x.double(), -1)).abs()
    return 4.0 * float(e[torch.isfinite(e)].max())


def _load(ref, bs, state, scores, hist, ind, pools, col, S0=11):
    """the same prepared mid-search state into the restatement and the device books"""
    B, K = ref.B, ref.K
    ref.scores[:] = scores.astype(np.float64)
    ref.hist[:] = hist
    ref.ind[:] = ind
    ref.col = col
    bs.scores.copy_(torch.from_numpy(scores.reshape(-1)))
    bs.hist.copy_(torch.from_numpy(hist).to(torch.int32))
    bs.ind.copy_(torch.from_numpy(ind.reshape(B * K, -1)).to(torch.int32))
    ps = torch.zeros((B, K))
    pi = torch.zeros((B, K + 1, 4), dtype=torch.int32)
    for b in range(B):
        ref.pool[b] = [[float(np.float32(s)), c, p, q] for s, c, p, q in pools[b]]
        ref.seq[b] = len(pools[b])
        for e, (s, c, p, q) in enumerate(pools[b]):
            ps[b, e] = float(np.float32(s))
            pi[b, e, :3] = torch.tensor([c, p, q])
        pi[b, K, 0] = pi[b, K, 1] = len(pools[b])
    bs.pool_score.copy_(ps)
    bs.pool_info.copy_(pi)
    state.copy_(torch.tensor([S0 + col, col, 0, 0], dtype=torch.int32))


def _compare(ref, bs, state, bound, col, S0=11):
    """every field of the books after a step: exact, except the scores (bound)"""
    B, K = ref.B, ref.K
    assert state.tolist() == [S0 + col + 1, col + 1, 0, 0]
    assert bs.tok.cpu().view(B, K).tolist() == ref.tok.tolist()
    assert np.array_equal(bs.hist.cpu().numpy(), ref.hist)
    assert np.array_equal(bs.ind.cpu().numpy().reshape(B, K, -1), ref.ind)
    assert bs.done.cpu().tolist() == ref.done
    sc = bs.scores.cpu().double().numpy().reshape(B, K)
    fin = np.isfinite(ref.scores)
    assert np.array_equal(np.isfinite(sc), fin) and (sc[~fin] == -np.inf).all()
    worst = float(np.abs(sc[fin] - ref.scores[fin]).max()) if fin.any() else 0.0
    pi, ps = bs.pool_info.cpu().numpy(), bs.pool_score.cpu().double().numpy()
    for b in range(B):
        assert pi[b, K, :2].tolist() == [len(ref.pool[b]), ref.seq[b]], b
        for e, (s, c, p, q) in enumerate(ref.pool[b]):
            assert pi[b, e].tolist() == [c, p, q, 0], (b, e)
            worst = max(worst, abs(ps[b, e] - s))
    assert worst <= bound, (worst, bound)
    return worst


# --------------------------------------------------------------------------- 1. mk_beam_emit vs the restatement --
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_beam_emit_equals_the_restatement(dev, case):
    B, K, K_in, V, ld, dtype, spiked, seed = case
    i = R.CASES.index(case)
    lp, early = (1.0, 0.7, 0.0, 2.0)[i % 4], i % 3 == 0
    td = getattr(torch, dtype)
    x, scores = R.beam_inputs(case)
    xq = torch.from_numpy(x).to(td)
    g = np.random.default_rng(i)
    col = 0 if K_in == 1 else 3
    n_max = col + 1
    pad, eos = V - 1, R.EOS_COL
    hist = np.zeros((n_max, B, K, 2), dtype=np.int64)
    ind = np.zeros((B, K, n_max), dtype=np.int64)
    hist[:col] = g.integers(0, K, (col, B, K, 2))
    ind[:, :, :col] = g.integers(0, K, (B, K, col))
    pools = [[] for _ in range(B)]
    if K_in == K:                   # a partly filled pool: K - 1 entries, K for the odd samples (full and not done)
        for b in range(B):
            pools[b] = [(float(g.uniform(-2.5, -0.2)), int(g.integers(1, col + 1)), int(g.integers(0, K)), e)
                        for e in range(K - 1 + b % 2)]
    ref = R.BeamRef(B, K, n_max, pad, eos, lp, early)
    bs = ops.BeamState(B, K, n_max, pad, dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    _load(ref, bs, state, scores, hist, ind, pools, col)
    ops.beam_emit(xq.to(dev)[:, :V], V, K_in, pad, eos, lp, early, bs, state)
    ref.step(xq[:, :V].double().numpy().reshape(B, K_in, V))
    bound = _log_softmax_bound(xq[:, :V].float())
    worst = _compare(ref, bs, state, bound, col)
    print(f"beam_emit {R.case_id(case)} lp={lp} early={early}: score error {worst:.3e}, bound 4 x e = {bound:.3e}, "
          f"done {ref.done}, pool sizes {[len(p) for p in ref.pool]}")


# ------------------------------------------------------------------------------ 2. ties and non-finite logits --
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_ties_go_to_the_lower_flat_index_and_nan_or_minus_inf_are_never_selected(dev, dtype):
    B, K, V, pad = 1, 2, 2100, 0
    x = torch.full((K, V), -4.0)
    x[0, 1500] = x[0, 17] = 5.0             # two columns of one row with identical logits
    x[1, 17] = 5.0                          # ... and the same values in the other row, at an equal score
    x[1, 1500] = 5.0
    x[0, 3] = float("nan")
    x[1, 4] = float("-inf")
    x[0, 2000] = float("nan")
    bs = ops.BeamState(B, K, 2, pad, dev)
    ref = R.BeamRef(B, K, 2, pad, None)
    state = torch.tensor([9, 1, 0, 0], dtype=torch.int32, device=dev)
    ref.col = 1
    bs.scores.fill_(-1.0)
    ref.scores[:] = -1.0
    ops.beam_emit(x.to(dtype).to(dev), V, K, pad, None, 1.0, False, bs, state)
    ref.step(x.to(dtype).double().numpy().reshape(B, K, V))
    # row 1 has one finite column more than row 0 (one NaN fewer): a larger lse, so row 0's pair ranks first
    assert bs.hist.cpu()[1, 0].tolist() == [[17, 0], [1500, 0]] == ref.hist[1, 0].tolist()
    # a whole row of equal logits: the 2K lowest columns in order, across the threads' interleaved columns
    flat = torch.zeros((1, V))
    flat[0, 0] = float("nan")
    flat[0, 2] = float("-inf")
    bs = ops.BeamState(1, 4, 1, pad, dev)
    state = torch.tensor([9, 0, 0, 0], dtype=torch.int32, device=dev)
    ops.beam_emit(flat.to(dtype).to(dev), V, 1, pad, None, 1.0, False, bs, state)
    assert bs.tok.cpu().tolist() == [1, 3, 4, 5]
    assert bs.hist.cpu()[0, 0, :, 1].tolist() == [0] * 4
    s = bs.scores.cpu()
    assert bool((s == s[0]).all()) and abs(float(s[0]) + np.log(V - 2)) < 1e-5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_fewer_than_k_finite_candidates_leave_beams_unfilled(dev, dtype):
    B, K, V, pad = 2, 4, 8, 6
    x = torch.full((B * K, V), float("-inf"))
    x[0, 2], x[0, 5] = 1.0, 0.5             # sample 0: two finite candidates in row 0, rows 1 ... 3 have none
    x[1, :] = float("nan")
    x[4:, :] = torch.randn(4, V, generator=torch.Generator().manual_seed(5))           # sample 1: ordinary rows, but only beam 0 has a finite score
    x[5, 1] = float("inf")                  # ... and a row with +inf in it has no candidate either
    bs = ops.BeamState(B, K, 2, pad, dev)
    ref = R.BeamRef(B, K, 2, pad, 7)
    state = torch.tensor([9, 1, 0, 0], dtype=torch.int32, device=dev)
    ref.col = 1
    sc = np.array([[-0.5, -0.6, -0.7, -0.8], [-0.1, -np.inf, -np.inf, -np.inf]], dtype=np.float32)
    bs.scores.copy_(torch.from_numpy(sc.reshape(-1)))
    ref.scores[:] = sc
    xq = x.to(dtype)
    ops.beam_emit(xq.to(dev), V, K, pad, 7, 1.0, False, bs, state)
    ref.step(xq.double().numpy().reshape(B, K, V))
    h = bs.hist.cpu()[1]
    assert h[0].tolist() == [[2, 0], [5, 0], [pad, 0], [pad, 0]]
    assert bs.scores.cpu()[2:4].tolist() == [float("-inf")] * 2 and bs.tok.cpu()[:4].tolist() == [2, 5, pad, pad]
    assert np.array_equal(h.numpy(), ref.hist[1]) and bs.tok.cpu().view(B, K).tolist() == ref.tok.tolist()
    assert (h[1, :, 1] == 0).all()          # sample 1: every new beam descends from beam 0
    got, want = bs.scores.cpu().double().numpy().reshape(B, K), ref.scores
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.allclose(got[np.isfinite(want)], want[np.isfinite(want)], atol=1e-5)


# ---------------------------------------------------------------------- 3. finished samples, the state hand-off --
def test_a_done_sample_keeps_its_books_and_emits_pad_and_the_state_moves_like_decode_emit(dev):
    B, K, V, pad, eos, col = 3, 4, 1000, 999, R.EOS_COL, 2
    case = (B, K, K, V, V, "bfloat16", True, 0)
    x, scores = R.beam_inputs(case)
    xd = torch.from_numpy(x).to(torch.bfloat16).to(dev)
    bs = ops.BeamState(B, K, 6, pad, dev)
    g = torch.Generator().manual_seed(0)
    bs.scores.copy_(torch.from_numpy(scores.reshape(-1)))
    bs.ind[:, :col] = torch.randint(0, K, (B * K, col), generator=g).int().to(dev)
    bs.pool_score.copy_(-torch.rand((B, K), generator=g))
    bs.pool_info[:, :K, 0] = 1
    bs.pool_info[:, :K, 2] = torch.arange(K, dtype=torch.int32, device=dev)
    bs.pool_info[:, K, :2] = K
    bs.done[1] = True
    state = torch.tensor([20 + col, col, 0, 0], dtype=torch.int32, device=dev)
    books = lambda: [t[1].clone() for t in (bs.scores.view(B, K), bs.pool_score, bs.pool_info, bs.done)]  # noqa: E731
    before, ind0 = books(), bs.ind.view(B, K, -1)[1].clone()
    for step in range(3):
        ops.beam_emit(xd, V, K, pad, eos, 1.0, False, bs, state)
        assert state.tolist() == [20 + col + step + 1, col + step + 1, 0, 0]          # state[2] left zero
        assert all(torch.equal(a, b) for a, b in zip(before, books()))                # bit-identical books
        assert bs.tok.view(B, K)[1].tolist() == [pad] * K
        if step == 0:
            assert int(bs.tok.view(B, K)[0, 0]) != pad                                # the others go on
        assert bs.hist[col + step, 1].tolist() == [[pad, j] for j in range(K)]
        now = bs.ind.view(B, K, -1)[1]
        assert torch.equal(now[:, :col], ind0[:, :col])                               # its table rows are not permuted
        assert now[:, col:col + step + 1].tolist() == [[j] * (step + 1) for j in range(K)]
    # mk_decode_emit on the same step state moves it the same way
    st2 = torch.tensor([20 + col, col, 0, 0], dtype=torch.int32, device=dev)
    tok, done = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.bool, device=dev)
    out = torch.zeros((B, 8), dtype=torch.long, device=dev)
    for step in range(3):
        ops.decode_emit(xd[:B], V, pad, eos, tok, done, out, st2)
    assert st2.tolist() == state.tolist()


def test_beam_emit_bad_arguments_return_codes(dev):
    x = torch.zeros((4, 40), dtype=torch.float32, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    bs = ops.BeamState(2, 2, 4, 0, dev)
    with pytest.raises(MacawHipError, match="BAD_ARG"):
        ops.beam_emit(x[:, :3], 3, 2, 0, 1, 1.0, False, bs, state)                    # V < 2K
    bs17 = ops.BeamState(1, 17, 4, 0, dev)
    with pytest.raises(MacawHipError, match="BAD_ARG"):
        ops.beam_emit(torch.zeros((17, 40), device=dev), 40, 17, 0, 1, 1.0, False, bs17, state)       # K > 16
    bs3 = ops.BeamState(1, 3, 4, 0, dev)
    with pytest.raises(MacawHipError, match="BAD_ARG"):
        ops.beam_emit(torch.zeros((2, 40), device=dev), 40, 2, 0, 1, 1.0, False, bs3, state)          # K_in not in {1, K}
    assert state.tolist() == [0, 0, 0, 0] and bool((bs.tok == 0).all())               # nothing was launched


# ------------------------------------------------------ 4. mk_decode_step_attn_beam vs a physically gathered cache --
SENT = 77.0


def _attn_case(dev, dtype, B, K, H, hd, S0, p, seed):
    D, Tmax, R_ = H * hd, max(S0 + 10, p + 1), B * K
    g = torch.Generator().manual_seed(seed)
    cache = torch.full((B, K, Tmax, 2 * D), SENT, dtype=dtype)
    cache[:, 0, :S0] = torch.randn((B, S0, 2 * D), generator=g).to(dtype)             # the prompt: slot 0 only
    cache[:, :, S0:p] = torch.randn((B, K, p - S0, 2 * D), generator=g).to(dtype)     # every slot's own new rows
    ind = torch.full((R_, Tmax - S0), -12345, dtype=torch.int32)                      # unread entries are poison
    ind[:, :p - S0] = torch.randint(0, K, (R_, p - S0), generator=g).int()
    gathered = torch.full((R_, Tmax, 2 * D), SENT, dtype=dtype)
    for r in range(R_):
        b = r // K
        gathered[r, :S0] = cache[b, 0, :S0]
        for t in range(S0, p):
            gathered[r, t] = cache[b, int(ind[r, t - S0]), t]
    qkv = torch.randn((R_, 3 * D), generator=g).to(dtype).to(dev)
    ang = torch.rand((Tmax, hd), generator=g) * 6.28
    cos, sin = ang.cos().to(dtype).to(dev), ang.sin().to(dtype).to(dev)
    return cache.to(dev), ind.to(dev), gathered.to(dev), qkv, cos, sin, D, Tmax


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,K,H,hd,ps", [(2, 3, 4, 64, range(5, 15)), (2, 3, 4, 128, range(5, 15)),
                                         (2, 16, 32, 128, (5, 6, 14)),
                                         # both sides of the first pass and of the first trip (one head: 8 waves x 64 / (hd / 8)
                                         # keys, x 8 in flight; four heads: 8 and 64), hd 16 / 32 behind their first pass
                                         (2, 3, 4, 64, (63, 64, 65, 511, 512, 513)), (2, 3, 4, 128, (31, 32, 33, 255, 256, 257)),
                                         (2, 16, 32, 128, (7, 8, 9, 63, 64, 65)), (2, 3, 4, 16, (257,)), (2, 3, 4, 32, (129,))],
                         ids=["hd64", "hd128", "four-heads", "hd64-edges", "hd128-edges", "four-heads-edges", "hd16", "hd32"])
def test_step_attn_beam_is_the_plain_kernel_on_a_gathered_cache_bit_for_bit(dev, dtype, B, K, H, hd, ps):
    S0 = 5          # (the table is consulted for every key from 5 on: in the second pass and the second trip too)
    for p in ps:
        cache, ind, gathered, qkv, cos, sin, D, Tmax = _attn_case(dev, dtype, B, K, H, hd, S0, p, 100 * hd + p)
        t_dev = torch.tensor([p], dtype=torch.int32, device=dev)
        scale = hd ** -0.5
        want = torch.full((B * K, D), SENT, dtype=dtype, device=dev)
        ops.decode_step_attn(qkv, qkv, qkv, 3 * D, cos, sin, gathered, t_dev, Tmax, B * K, H, hd, want, scale, k_off=D,
                             v_off=2 * D)
        before = cache.clone()
        got = torch.full((B * K, D), SENT, dtype=dtype, device=dev)
        ops.decode_step_attn_beam(qkv, qkv, qkv, 3 * D, cos, sin, cache, t_dev, ind, S0, Tmax, B, K, H, hd, got, scale,
                                  k_off=D, v_off=2 * D)
        assert bool(torch.isfinite(want.float()).all()) and not bool((want == SENT).all())
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (p, (got.float() - want.float()).abs().max())
        # row p of every row's own slot holds the rotated key and the value; every other byte is untouched
        assert torch.equal(cache.view(B * K, Tmax, 2 * D)[:, p].view(torch.int16), gathered[:, p].view(torch.int16)), p
        assert torch.equal(cache[:, :, p, D:], qkv[:, 2 * D:].view(B, K, D))
        cache[:, :, p] = before[:, :, p]
        assert torch.equal(cache.view(torch.int16), before.view(torch.int16)), p


def test_step_attn_beam_bad_arguments_return_codes_and_launch_nothing(dev):
    B, K, H, hd, S0, p = 2, 3, 4, 64, 5, 7
    cache, ind, _, qkv, cos, sin, D, Tmax = _attn_case(dev, torch.bfloat16, B, K, H, hd, S0, p, 1)
    t_dev = torch.tensor([p], dtype=torch.int32, device=dev)
    out = torch.full((B * K, D), SENT, dtype=torch.bfloat16, device=dev)
    before = cache.clone()

    def call(ind=ind, S0=S0, K=K, cache=cache, B=B):
        ops.decode_step_attn_beam(qkv, qkv, qkv, 3 * D, cos, sin, cache, t_dev, ind, S0, Tmax, B, K, H, hd, out, 0.125,
                                  k_off=D, v_off=2 * D)
    with pytest.raises(MacawHipError, match="BAD_ARG"):
        call(ind=ind[:, :Tmax - S0 - 1].contiguous())                   # a table shorter than the new positions
    with pytest.raises(MacawHipError, match="BAD_ARG"):
        call(S0=Tmax + 1)
    with pytest.raises(MacawHipError, match="BAD_ARG"):
        call(S0=-1)
    with pytest.raises(MacawHipError, match="BAD_ARG"):                 # 17 beams
        call(K=17, B=1, cache=torch.zeros((1, 17, Tmax, 2 * D), dtype=torch.bfloat16, device=dev),
             ind=torch.zeros((17, Tmax), dtype=torch.int32, device=dev))
    with pytest.raises(MacawHipError):                                  # the wrapper's own checks
        call(cache=cache.view(B * K, Tmax, 2 * D))
    with pytest.raises(MacawHipError):
        call(ind=ind.long())
    assert bool((out == SENT).all()) and torch.equal(cache, before)


# ------------------------------------------------------------------------------------------------ 5. generate() --
def _kw(cfg_l, B, dev, **over):
    return {**dict(input_ids=_ids(cfg_l, B, dev), max_new_tokens=12, eos_token_id=-1, pad_token_id=0), **over}


@pytest.fixture(scope="module")
def llama(dev):
    return _small_llama(dev)


def test_one_beam_is_todays_greedy_bit_for_bit_on_every_weight_format(dev, llama):
    lm, cfg_l = llama
    for extra in ({}, dict(decode_weights="fp8"), dict(decode_weights="mxfp4")):
        kw = _kw(cfg_l, 3, dev, **extra)
        with _Spy("decode_emit", "beam_emit", "decode_step_attn_beam", "decode_step_attn") as spy:
            greedy = lm.generate(**kw)
            n_emit, n_attn = len(spy.calls["decode_emit"]), len(spy.calls["decode_step_attn"])
            got = lm.generate(num_beams=1, length_penalty=2.0, early_stopping=True, num_return_sequences=3,
                              return_beam_scores=True, **kw)
            assert len(spy.calls["decode_emit"]) == 2 * n_emit and len(spy.calls["decode_step_attn"]) == 2 * n_attn
            assert spy.calls["beam_emit"] == [] and spy.calls["decode_step_attn_beam"] == []
        assert torch.is_tensor(got) and torch.equal(got, greedy), extra


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_graph_path_and_kernel_by_kernel_loop_return_identical_ids_and_scores(dev, dtype):
    lm, cfg_l = _small_llama(dev, dtype)
    nl = cfg_l["num_hidden_layers"]
    kw = _kw(cfg_l, 3, dev, num_beams=4, num_return_sequences=4, return_beam_scores=True)
    with _Spy("beam_emit", "decode_step_attn_beam", "decode_step_attn", "decode_emit", "copy2d") as spy:
        ids, sc = lm.generate(**kw)
        # token 0, one eager step, ONE captured step; the prefill at batch B writes the cache without a beam launch
        assert len(spy.calls["beam_emit"]) == 3 and len(spy.calls["decode_step_attn_beam"]) == 2 * nl
        assert spy.calls["decode_step_attn"] == [] and spy.calls["decode_emit"] == []
        assert spy.calls["beam_emit"][0][0].shape[0] == 3 and spy.calls["beam_emit"][1][0].shape[0] == 12
        n_copy = len(spy.calls["copy2d"])
        ids2, sc2 = lm.generate(decode_graph=False, **kw)
        assert len(spy.calls["beam_emit"]) == 3 + 12 and len(spy.calls["decode_step_attn_beam"]) == (2 + 11) * nl
        assert len(spy.calls["copy2d"]) == 2 * n_copy                 # the steps copy no cache row on either path
    assert ids.shape == (12, 12) and ids.dtype == torch.long and sc.shape == (12,) and sc.dtype == torch.float32
    assert torch.equal(ids, ids2) and torch.equal(sc, sc2)
    assert torch.equal(lm.generate(**{**kw, "return_beam_scores": False}), ids)
    short = lm.generate(**{**kw, "max_new_tokens": 2})               # max_new_tokens <= 2: the loop
    assert short[0].shape == (12, 2)


def _teacher_forced(lm, prompt, ids, V):
    """float64 log-probabilities [n, L] of ids [n, L] after prompt [n, S0], from ONE full forward"""
    full = torch.cat([prompt, ids], 1)
    with torch.no_grad():
        logits = lm(input_ids=full).logits[:, prompt.shape[1] - 1:-1, :V].double()
    return torch.log_softmax(logits, -1).gather(2, ids.unsqueeze(-1)).squeeze(-1)


def test_fp32_recompute_path_equals_the_restatement_driven_by_full_forward_logits(dev):
    lm, cfg_l = _small_llama(dev, torch.float32)
    B, K, N, V = 2, 4, 8, cfg_l["vocab_size"]
    prompt = _ids(cfg_l, B, dev)
    kw = dict(input_ids=prompt, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, use_cache=False, num_beams=K,
              num_return_sequences=K, return_beam_scores=True)
    ids, sc = lm.generate(**kw)
    ref = R.BeamRef(B, K, N, 0, None, 1.0, False)
    bound = 0.0
    for t in range(N):
        if t == 0:
            pre = prompt
        else:
            seqs = torch.tensor([ref.sequence(b, t - 1, k) for b in range(B) for k in range(K)], device=dev)
            pre = torch.cat([prompt.repeat_interleave(K, 0), seqs], 1)
        with torch.no_grad():
            logits = lm(input_ids=pre).logits[:, -1, :V].float()
        bound = max(bound, _log_softmax_bound(logits.cpu()))
        ref.step(logits.double().cpu().numpy().reshape(B, -1, V))
    rows, scores = ref.finalize(K)
    err = float(np.abs(sc.cpu().double().numpy() - np.array(scores)).max())
    print(f"fp32 use_cache=False vs restatement: score error {err:.3e}, bound {bound:.3e}")
    assert ids.cpu().tolist() == R.padded(rows, 0)
    assert err <= bound, (err, bound)
    # the same call with a cache refuses fp32 and points to use_cache=False
    with pytest.raises(ValueError, match="use_cache=False"):
        lm.generate(**{**kw, "use_cache": True})


def test_cached_beam_scores_are_the_teacher_forced_log_probabilities_of_the_returned_ids(dev, llama):
    lm, cfg_l = llama
    B, K, N, V, lp = 3, 4, 12, cfg_l["vocab_size"], 0.8
    prompt = _ids(cfg_l, B, dev)
    # The bound, measured on the greedy code as it stands: 4 x the largest per-token log-prob gap between the CACHED greedy
    # path and one full forward over the greedy ids.  The cached path is the one of the hipGraph loop -- the five-launch
    # step with ops.decode_step_attn, which a beam step runs too -- and its logits are visible per token only where those
    # launches run kernel by kernel: the loop of a padded batch (one masked pad token in front of every prompt; each
    # sample generates what its valid tokens generate alone, through the per-sample-position form of the same kernels).
    # decode_graph=False WITHOUT a mask runs the general layer path (rope, copy, flash attention): other kernels, whose
    # gap says nothing about the step kernels'.  Greedy runs at B * K prompts: the row count of a beam step (the streamed
    # launches choose their form by it) and as many token events as the beam call scores.
    gprompt = _ids(cfg_l, B * K, dev)
    padded = torch.cat([torch.zeros_like(gprompt[:, :1]), gprompt], 1)
    mask = torch.ones_like(padded)
    mask[:, 0] = 0
    seen = []
    real = ops.argmax_rows

    def spy(x, cols=None):
        seen.append(x[:, :V].double().clone())
        return real(x, cols)
    ops.argmax_rows = spy
    try:
        with _Spy("decode_step_attn_var") as steps:
            greedy = lm.generate(input_ids=padded, attention_mask=mask, max_new_tokens=N, eos_token_id=-1, pad_token_id=0,
                                 decode_graph=False)
    finally:
        ops.argmax_rows = real
    assert len(steps.calls["decode_step_attn_var"]) == (N - 1) * cfg_l["num_hidden_layers"]       # the step kernels ran
    assert torch.equal(greedy, lm.generate(input_ids=gprompt, max_new_tokens=N, eos_token_id=-1, pad_token_id=0))
    cached = torch.stack([torch.log_softmax(x, -1) for x in seen], 1).gather(2, greedy.unsqueeze(-1)).squeeze(-1)
    bound = 4.0 * float((cached - _teacher_forced(lm, gprompt, greedy, V)).abs().max())
    ids, sc = lm.generate(input_ids=prompt, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, num_beams=K,
                          num_return_sequences=K, length_penalty=lp, return_beam_scores=True)
    tf = _teacher_forced(lm, prompt.repeat_interleave(K, 0), ids, V).sum(1)
    err = float((sc.double() * float(N) ** lp - tf).abs().max())
    print(f"cached beam scores vs teacher forcing: error {err:.3e}, bound (4 x greedy per-token gap) {bound:.3e}")
    assert err <= bound, (err, bound)


def test_eos_ends_a_hypothesis_pad_follows_and_early_stopping_stops_a_sample(dev, llama):
    lm, cfg_l = llama
    B, K, N = 3, 4, 16
    kw = _kw(cfg_l, B, dev, max_new_tokens=N, num_beams=K, num_return_sequences=K, return_beam_scores=True)
    free, _ = lm.generate(**kw)
    eos = int(free[:, 1:5].flatten().mode().values)             # an id the eos-free run emits early
    for early in (True, False):
        with _Spy("beam_emit") as spy:
            ids, sc = lm.generate(**{**kw, "eos_token_id": eos, "early_stopping": early})
        bs = spy.calls["beam_emit"][0][7]                       # the books of that call, as the loop left them
        hit = (ids == eos).cumsum(1) > 0
        assert bool(hit.any())
        after = torch.zeros_like(hit)
        after[:, 1:] = hit[:, :-1]
        assert bool((ids[after] == 0).all())                    # the hypothesis ends at its eos and pad follows
        assert bool(((ids == eos).sum(1) <= 1).all())
        lens = torch.where(hit.any(1), hit.long().argmax(1) + 1, torch.full((B * K,), ids.shape[1], device=dev))
        assert ids.shape[1] == int(lens.max())                  # the width is the longest returned hypothesis
        s_ = sc.view(B, K)
        assert bool((s_[:, :-1] >= s_[:, 1:]).all())
        done, pool_n = bs.done.cpu(), bs.pool_info[:, K, 0].cpu()
        assert bool(done.any()), "the eos chosen finishes no sample: the case checks nothing"
        if early:                                               # done exactly when K hypotheses have finished
            assert torch.equal(done, pool_n == K)
        else:
            assert bool((pool_n[done] == K).all())
        for b in range(B):                                      # a done sample returns finished hypotheses only
            if bool(done[b]):
                assert bool(hit[b * K:(b + 1) * K].any(1).all())
        if bool(done.all()):                                    # ... and the loop ended within 8 tokens of the last one
            assert int(spy.calls["beam_emit"][0][8][1]) <= N


def test_num_return_sequences_returns_k_distinct_hypotheses_in_descending_score(dev, llama):
    lm, cfg_l = llama
    B, K = 3, 4
    kw = _kw(cfg_l, B, dev, num_beams=K, return_beam_scores=True)
    ids, sc = lm.generate(num_return_sequences=K, **kw)
    assert ids.shape == (B * K, 12)
    for b in range(B):
        rows = {tuple(r) for r in ids[b * K:(b + 1) * K].tolist()}
        assert len(rows) == K
        s = sc[b * K:(b + 1) * K]
        assert bool((s[:-1] >= s[1:]).all())
    one, s1 = lm.generate(**kw)                                  # the default returns the best of them
    assert torch.equal(one, ids[::K]) and torch.equal(s1, sc[::K])
    two, _ = lm.generate(num_return_sequences=2, **kw)
    assert torch.equal(two.view(B, 2, -1), ids.view(B, K, -1)[:, :2])
    # beam search never scores below greedy: the greedy path is one of the candidates it keeps or beats
    greedy = lm.generate(**_kw(cfg_l, B, dev))
    g = _teacher_forced(lm, kw["input_ids"], greedy, cfg_l["vocab_size"]).sum(1) / 12.0
    print("best beam score - greedy score per sample:", (s1.double() - g).tolist())


def test_lora_and_both_decode_weights_modes_run_with_four_beams(dev, llama):
    from test_lora_gpu import _mm_lora
    lm, cfg_l = llama
    kw = _kw(cfg_l, 3, dev, num_beams=4, return_beam_scores=True)
    base, _ = lm.generate(**kw)
    for mode, op in (("fp8", "decode_linear_fp8"), ("mxfp4", "decode_linear_mxfp4")):
        with _Spy(op, "decode_step_attn_beam", "beam_emit") as spy:
            ids, sc = lm.generate(decode_weights=mode, **kw)
            assert len(spy.calls[op]) > 0 and len(spy.calls["decode_step_attn_beam"]) > 0
            # the streams see B * K token rows (the e4m3 lm_head also the prefill's B rows, for token 0)
            assert {12} <= {a[0].shape[0] for a in spy.calls[op]} <= {3, 12}
        assert ids.shape == base.shape and bool(torch.isfinite(sc).all())
        assert torch.equal(ids, lm.generate(decode_weights=mode, **kw)[0])
        with pytest.raises(ValueError, match=r"B x num_beams = 9 x 4 = 36"):
            lm.generate(decode_weights=mode, **_kw(cfg_l, 9, dev, num_beams=4))
    model, fx = _mm_lora(dev, p=0.0)
    with torch.no_grad():
        for n, q in model.llm.named_parameters():
            if ".lora_B." in n:
                q.copy_(torch.randn_like(q.float()) * 0.05)
    model.eval()
    emb = fx["inputs_embeds"].to(dev).to(torch.bfloat16)
    args = dict(inputs_embeds=emb, max_new_tokens=8, eos_token_id=2, pad_token_id=106, num_beams=4, return_beam_scores=True)
    with _Spy("decode_step_attn_beam") as spy:
        a, sa = model.llm.generate(**args)
        assert len(spy.calls["decode_step_attn_beam"]) > 0
    assert a.shape[0] == emb.shape[0] and bool(torch.isfinite(sa).all())
    b, sb = model.llm.generate(decode_graph=False, **args)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_each_refusal_names_its_condition(dev, llama):
    lm, cfg_l = llama
    kw = _kw(cfg_l, 2, dev)
    for bad in (0, 17, 2.5, "3"):
        with pytest.raises(ValueError, match="num_beams"):
            lm.generate(num_beams=bad, **kw)
    with pytest.raises(ValueError, match="num_return_sequences"):
        lm.generate(num_beams=2, num_return_sequences=3, **kw)
    with pytest.raises(ValueError, match="do_sample"):
        lm.generate(num_beams=2, do_sample=True, **kw)
    with pytest.raises(ValueError, match="kv_cache"):
        lm.generate(num_beams=2, kv_cache="fp8", **kw)
    mask = torch.ones((2, 21), dtype=torch.long, device=dev)
    assert lm.generate(num_beams=2, attention_mask=mask, **kw).shape[0] == 2      # a mask without a zero is no padding
    mask[1, :3] = 0
    with pytest.raises(ValueError, match="attention_mask"):
        lm.generate(num_beams=2, attention_mask=mask, **kw)
    from transformers import LlamaConfig
    tiny = Mo.fuse_model(Mo.LlamaForCausalLM(LlamaConfig(**{**cfg_l, "vocab_size": 24})).to(dev).to(torch.bfloat16)).eval()
    ids24 = torch.randint(3, 24, (2, 9), generator=torch.Generator().manual_seed(0)).to(dev)
    with pytest.raises(ValueError, match="vocabulary"):
        tiny.generate(input_ids=ids24, max_new_tokens=4, num_beams=16)
    assert tiny.generate(input_ids=ids24, max_new_tokens=4, num_beams=12, eos_token_id=None).shape == (2, 4)
    with pytest.raises(ValueError, match="decode_graph=False"):                   # the weight modes keep their refusals
        lm.generate(num_beams=2, decode_weights="fp8", decode_graph=False, **kw)


def test_set_beam_search_reaches_generate(dev):
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    with torch.no_grad(), _Spy("decode_emit", "beam_emit") as spy:
        base = model(inputs=inp)
        assert spy.calls["beam_emit"] == [] and len(spy.calls["decode_emit"]) > 0
        Mo.MM_LLMs.set_beam_search(num_beams=3, length_penalty=0.5, early_stopping=True, num_return_sequences=2)
        ids = model(inputs=inp)
        calls = spy.calls["beam_emit"]
        assert len(calls) > 0 and tuple(calls[0][2:7]) == (1, 32006, 2, 0.5, True) and calls[0][7].K == 3
        assert ids.shape[0] == 2 * base.shape[0] and ids.dtype == torch.long
        Mo.MM_LLMs.set_beam_search()
        n = len(spy.calls["beam_emit"])
        assert torch.equal(model(inputs=inp), base) and len(spy.calls["beam_emit"]) == n
