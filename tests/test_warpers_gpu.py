"""GPU: the four warpers behind top-p -- min_p, typical_p, epsilon_cutoff, eta_cutoff (csrc/sample.hip; rule 6 next to
mk_sample_rows in include/macaw_hip.h) -- against the float64 reference of tests/warpers_ref.py.

The mask test holds ops.sample_keep_rows, row by row, to one of the reference's alternatives: the kept sets that remain
when every UNDECIDED column (a decision within the window W = 2^-16 of its stage's threshold, the EPS of
tests/test_sampling_gpu.py for the reason given there) is decided either way.  A row with more than 4 undecided columns is
left out; such rows are counted against the caps tests/test_warpers_cpu.py checks on the reference alone (a quarter of a
case, 2 % of all rows).  The draw test then holds ops.sample_rows_warp to the kernel's own mask, verified above, and to the CDF
interval of u * Z over it widened by 4 W Z -- the existing draw test's rule.  The cases without arithmetic are exact."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import warpers_ref as R  # noqa: E402
from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_decode_kv8_gpu import _Spy, _ids, _small_llama  # noqa: E402
from test_sampling_cpu import filter_row, uniform  # noqa: E402
from test_sampling_gpu import DTYPES, EPS, SHAPES, _logits  # noqa: E402

from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
IDS = ["bf16", "fp16", "fp32"]
ALL_ROWS = sum(rows for _, rows, _ in R.SHAPES) * len(R.SIGMAS) * len(R.DTYPES) * len(R.TUPLES)
LEFT_OUT = {}                                                        # (case, tuple) -> rows left out, over the session


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.MM_LLMs.set_sampling()
    Mo.MM_LLMs.set_grammar(None)
    ops.clear_fp8_cache()


# --------------------------------------------------------------------------------------------------- 1. the mask --
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("sigma", R.SIGMAS)
@pytest.mark.parametrize("V,rows,ld", SHAPES)
def test_mask_is_one_of_the_reference_alternatives(dev, V, rows, ld, sigma, dtype):
    assert SHAPES == R.SHAPES
    xd, xh = _logits(V, rows, ld, sigma, dtype)
    assert np.array_equal(xh, R.logits_host(V, rows, ld, sigma, NAME[dtype])[1])      # the reference's fixture
    for tup in R.TUPLES:
        got = ops.sample_keep_rows(xd[:, :V], V, *tup)
        assert got.dtype == torch.bool and tuple(got.shape) == (rows, V)
        got = got.cpu().numpy()
        ref = R.case(V, rows, ld, sigma, NAME[dtype], tup)
        lo = 0
        for r in range(rows):
            kept, alts, und = ref[r]
            if alts is None:
                lo += 1
                continue
            diff = np.nonzero(got[r] != kept)[0]
            assert any(np.array_equal(got[r], a) for a in alts), (tup, r, diff[:8].tolist(), und, int(kept.sum()))
        print(V, sigma, NAME[dtype], tup, "left out", lo, "of", rows)
        assert 4 * lo <= rows, (tup, lo)
        LEFT_OUT[(V, sigma, dtype, tup)] = lo
    assert 50 * sum(LEFT_OUT.values()) <= ALL_ROWS, sum(LEFT_OUT.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V,rows,ld", SHAPES)
def test_mask_with_the_four_off_is_the_kept_set_of_rules_1_to_3(dev, V, rows, ld, dtype):
    xd, xh = _logits(V, rows, ld, 3.0, dtype)
    for T, k, p in [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95), (1.0, V + 5, 1.0)]:
        got = ops.sample_keep_rows(xd[:, :V], V, T, k, p).cpu().numpy()
        for r in range(rows):
            relaxed = filter_row(xh[r], V, T, k, p, p_slack=EPS)["kept"]
            strict = filter_row(xh[r], V, T, k, p, p_slack=-EPS)["kept"]
            assert not (got[r] & ~relaxed).any() and not (strict & ~got[r]).any(), (T, k, p, r)
            if p == 1.0:
                assert np.array_equal(got[r], strict)


# --------------------------------------------------------------------------------------------------- 2. the draw --
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("sigma", R.SIGMAS)
@pytest.mark.parametrize("V,rows,ld", SHAPES)
def test_draw_lies_in_the_kernels_mask_and_its_cdf_interval(dev, V, rows, ld, sigma, dtype):
    xd, xh = _logits(V, rows, ld, sigma, dtype)
    seed = 0x0FED_CBA9_8765_4321 + V
    for tup in R.TUPLES:
        T, k = tup[0], tup[1]
        mask = ops.sample_keep_rows(xd[:, :V], V, *tup).cpu().numpy()
        got = torch.stack([ops.sample_rows_warp(xd[:, :V], V, *tup[:3], seed, *tup[3:], step=step) for step in range(16)])
        got = got.cpu().numpy()
        assert got.min() >= 0 and got.max() < V, tup
        for r in range(rows):
            assert mask[r].any() and mask[r, got[:, r]].all(), (tup, r)
            e = np.where(mask[r], filter_row(xh[r], V, T, k, 1.0)["e"], 0.0)
            cum = np.cumsum(e)
            Z = cum[-1]
            for step in range(16):
                c = int(got[step, r])
                uZ = uniform(seed, step, r) * Z
                lo, hi = cum[c] - e[c], cum[c]
                assert lo - 4 * EPS * Z <= uZ <= hi + 4 * EPS * Z, (tup, r, step, c, lo / Z, hi / Z, uZ / Z)


# -------------------------------------------------------------------------- 3. exact where no arithmetic is involved --
def _draws(x, V, n=64, **kw):
    return torch.stack([ops.sample_rows_warp(x, V, 1.0, 0, 1.0, 11, step=step, **kw) for step in range(n)])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_min_p_1_and_cutoffs_near_1_are_argmax_bit_for_bit(dev, dtype):
    V, rows, ld = 32007, 8, 32064
    xd, _ = _logits(V, rows, ld, 3.0, dtype, seed=1)
    xu = xd.clone()                                                   # unique maxima far above the rest: p(max) = 1
    lo = xd.clone()                                                   # unique maxima with 0.8 < p(max) < 1: both branches
    for r in range(rows):
        xu[r, (r * 4001) % V] = 70.0 + r
        lo[r, (r * 4001) % V] = 17.0 + 0.5 * r
    for x in (xu, lo):
        am = ops.argmax_rows(x[:, :V], V)
        assert am.tolist() == [(r * 4001) % V for r in range(rows)]
        for step in range(4):
            assert torch.equal(ops.sample_rows_warp(x[:, :V], V, 1.0, 0, 1.0, 5, step=step, min_p=1.0), am)
            assert torch.equal(ops.sample_rows_warp(x[:, :V], V, 0.7, 50, 0.9, 5, step=step, min_p=1.0), am)
            assert torch.equal(ops.sample_rows_warp(x[:, :V], V, 1.0, 0, 1.0, 5, step=step, epsilon_cutoff=0.99), am)
            assert torch.equal(ops.sample_rows_warp(x[:, :V], V, 1.0, 0, 1.0, 5, step=step, epsilon_cutoff=0.99, eta_cutoff=0.99), am)
        assert torch.equal(ops.sample_keep_rows(x[:, :V], V, min_p=1.0).sum(1), torch.ones_like(am))
    am = ops.argmax_rows(xu[:, :V], V)                               # entropy ~ 0: eta's threshold is eta itself
    for step in range(4):
        assert torch.equal(ops.sample_rows_warp(xu[:, :V], V, 1.0, 0, 1.0, 5, step=step, eta_cutoff=0.99), am)
    # a duplicated maximum: min_p = 1 keeps exactly its tie group
    xd[1, 4000] = xd[1, 17] = xd[1, 31000] = 50.0
    seen = set(_draws(xd[:, :V], V, min_p=1.0)[:, 1].tolist())
    assert seen == {17, 4000, 31000}, seen
    assert ops.sample_keep_rows(xd[:, :V], V, min_p=1.0)[1].nonzero().flatten().tolist() == [17, 4000, 31000]
    assert ops.sample_keep_rows(xd[:, :V], V, epsilon_cutoff=0.5)[1].nonzero().flatten().tolist() == [17, 4000, 31000]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_typical_band_drops_the_maximum_and_keeps_tie_groups_whole(dev, dtype):
    row = torch.tensor([[.4, .15, .15, .15, .15]]).log().to(dtype).to(dev)
    assert ops.sample_keep_rows(row, 5, typical_p=0.5)[0].tolist() == [False, True, True, True, True]
    assert set(_draws(row, 5, typical_p=0.5).flatten().tolist()) == {1, 2, 3, 4}
    assert set(_draws(row, 5).flatten().tolist()) == {0, 1, 2, 3, 4}  # (the maximum is drawn without the stage)
    # a tie group in t that spans threads: one column of probability 0.4 and 2099 that share 0.6 -- the group is nearer
    # to the entropy and reaches the mass 0.5 alone, so it stays whole and the maximum goes
    V = 2100
    x = torch.full((1, V), float(np.log(.6 / (V - 1))))
    x[0, 700] = float(np.log(.4))
    x = x.to(dtype).to(dev)
    want = [c != 700 for c in range(V)]
    assert ops.sample_keep_rows(x, V, typical_p=0.5)[0].tolist() == want
    got = _draws(x, V, typical_p=0.5).flatten().tolist()
    assert 700 not in got and len(set(got)) > 32 and max(got) > 1400 and min(got) < 700
    assert ops.sample_keep_rows(x, V, typical_p=0.7)[0].all()        # past the group's mass: both groups


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_and_minus_inf_are_never_drawn_and_a_row_without_finite_logits_is_greedy(dev, dtype):
    nan, ninf = float("nan"), float("-inf")
    bad = torch.tensor([[nan, ninf, 0.5, nan, 0.25, ninf, 0.0], [ninf, ninf, ninf, ninf, ninf, ninf, ninf],
                        [ninf, ninf, nan, ninf, nan, ninf, ninf]], dtype=dtype, device=dev)
    for tup in R.TUPLES + [(1.0, 0, 1.0, 1.0, 1.0, 0.0, 0.0), (1.0, 0, 1.0, 0.0, .01, 0.0, 0.0),
                           (1.0, 0, 1.0, 0.0, 1.0, .99, 0.0), (1.0, 0, 1.0, 0.0, 1.0, 0.0, .99)]:
        out = torch.stack([ops.sample_rows_warp(bad, 7, *tup[:3], 8, *tup[3:], step=step) for step in range(64)])
        assert set(out[:, 0].tolist()) <= {2, 4, 6}, tup
        assert set(out[:, 1].tolist()) == {0} and set(out[:, 2].tolist()) == {2}      # no finite logit: greedy's choice
        mask = ops.sample_keep_rows(bad, 7, *tup)
        assert not mask[1:].any() and mask[0].any() and not mask[0, [0, 1, 3, 5]].any(), tup
        assert set(out[:, 0].tolist()) <= set(mask[0].nonzero().flatten().tolist())
    # e = 1, e^-.25 = .78, e^-.5 = .61 against min_p = 0.7
    assert ops.sample_keep_rows(bad, 7, min_p=0.7)[0].tolist() == [False, False, True, False, True, False, False]


# ----------------------------------------------------------------------------------------------- 4. off means off --
def _raw_rows(x, V, T, k, p, seed, step, warp):
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    lib = L.load()
    L.check(lib.mk_sample_rows_warp(x.data_ptr(), x.stride(0), x.shape[0], V, T, k, p, *warp, seed, step, out.data_ptr(),
                                    ops.dt(x), None), "mk_sample_rows_warp")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("V,rows,ld", [(32007, 8, 32064), (1000, 3, 1000)])
def test_with_the_four_off_the_ids_are_the_old_entries(dev, V, rows, ld):
    xd, _ = _logits(V, rows, ld, 3.0, torch.bfloat16, seed=4)
    torch.cuda.synchronize()
    for T, k, p in [(1.0, 0, 1.0), (0.8, 40, 0.95), (1.0, 0, 0.9)]:
        for step in range(8):
            old = ops.sample_rows(xd[:, :V], V, T, k, p, 99, step)
            assert torch.equal(ops.sample_rows_warp(xd[:, :V], V, T, k, p, 99, 0.0, 1.0, 0.0, 0.0, step=step), old)
            assert torch.equal(_raw_rows(xd, V, T, k, p, 99, step, (0.0, 1.0, 0.0, 0.0)), old)     # the C entry itself
        # ... and the emit: the _warp entry at (0, 1, 0, 0) against the old one, two steps from the same books
        books = []
        for entry in ("old", "warp"):
            tok = torch.full((rows,), -1, dtype=torch.long, device=dev)
            done = torch.zeros(rows, dtype=torch.bool, device=dev)
            out = torch.full((rows, 12), -7, dtype=torch.long, device=dev)
            state = torch.tensor([3, 0, 0, 0], dtype=torch.int32, device=dev)
            for _ in range(8):
                if entry == "old":
                    ops.decode_emit_sample(xd[:, :V], V, 0, -1, tok, done, out, state, T, k, p, 99)
                else:
                    torch.cuda.synchronize()
                    L.check(L.load().mk_decode_emit_sample_warp(
                        xd.data_ptr(), xd.stride(0), V, rows, 0, -1, tok.data_ptr(), done.data_ptr(), out.data_ptr(),
                        out.stride(0), state.data_ptr(), T, k, p, 0.0, 1.0, 0.0, 0.0, 99, ops.dt(xd), None), "emit_warp")
                    torch.cuda.synchronize()
            books.append((out.clone(), state.tolist()))
        assert torch.equal(books[0][0], books[1][0]) and books[0][1] == books[1][1] == [11, 8, 0, 0]


def _kw(cfg_l, B, dev, **over):
    return {**dict(input_ids=_ids(cfg_l, B, dev), max_new_tokens=12, eos_token_id=-1, pad_token_id=0), **over}


def test_generate_with_the_four_off_makes_the_calls_without_them(dev):
    lm, cfg_l = _small_llama(dev)
    for path in (dict(), dict(decode_graph=False)):
        kw = _kw(cfg_l, 3, dev, do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=4, **path)
        with _Spy("decode_emit_sample", "sample_rows", "decode_emit_sample_warp", "sample_rows_warp") as spy:
            a = lm.generate(**kw)
            n = {k: len(v) for k, v in spy.calls.items()}
            assert n["decode_emit_sample"] + n["sample_rows"] > 0
            b = lm.generate(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, **kw)
            c = lm.generate(min_p=None, **kw)
            for call in spy.calls["decode_emit_sample"]:
                assert tuple(call[8:]) == (0.9, 30, 0.95, 4)          # the 4-tuple: today's call
            for call in spy.calls["sample_rows"]:
                assert tuple(call[2:]) == (0.9, 30, 0.95, 4)
            assert {k: len(v) for k, v in spy.calls.items()} == {k: 3 * v for k, v in n.items()}
            assert spy.calls["decode_emit_sample_warp"] == [] and spy.calls["sample_rows_warp"] == []
            d = lm.generate(min_p=0.05, **kw)                         # one of the four on: the _warp ops, the 8-tuple
            assert {k: len(v) for k, v in spy.calls.items()} == {
                **{k: 3 * v for k, v in n.items()}, "decode_emit_sample_warp": n["decode_emit_sample"],
                "sample_rows_warp": n["sample_rows"]}
            for call in spy.calls["decode_emit_sample_warp"]:
                assert tuple(call[8:]) == (0.9, 30, 0.95, 4, 0.05, 1.0, 0.0, 0.0)
            for call in spy.calls["sample_rows_warp"]:
                assert tuple(call[2:]) == (0.9, 30, 0.95, 4, 0.05, 1.0, 0.0, 0.0)
        assert torch.equal(a, b) and torch.equal(a, c) and d.shape == a.shape
    # ignored by greedy decoding, whatever they hold
    kw = _kw(cfg_l, 2, dev)
    assert torch.equal(lm.generate(min_p=7.0, typical_p=-1.0, epsilon_cutoff="x", eta_cutoff=None, **kw), lm.generate(**kw))
    for bad, name in ((dict(min_p=1.5), "min_p"), (dict(typical_p=0.0), "typical_p"), (dict(epsilon_cutoff=1.0), "epsilon_cutoff"),
                      (dict(eta_cutoff=float("nan")), "eta_cutoff"), (dict(min_p=True), "min_p")):
        with pytest.raises(ValueError, match=name):
            lm.generate(do_sample=True, **bad, **kw)
    with pytest.raises(ValueError, match="do_sample"):               # beams and prompt lookup go on refusing do_sample
        lm.generate(do_sample=True, min_p=0.1, num_beams=2, **kw)
    with pytest.raises(ValueError, match="do_sample"):
        lm.generate(do_sample=True, min_p=0.1, prompt_lookup_num_tokens=3, **kw)


# --------------------------------------------------------------------------- 5. decode_emit_sample vs sample_rows --
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B", [1, 3, 33])
def test_decode_emit_sample_warp_draws_sample_rows_token_and_keeps_decode_emits_books(dev, B, dtype):
    V, ld, step, pad = 1000, 1008, 5, 1003
    xd, _ = _logits(V, B, ld, 3.0, dtype, seed=3)
    args, warp = (0.8, 40, 0.95, 4242), (0.02, 0.9, 1e-2, 2e-3)
    want = ops.sample_rows_warp(xd[:, :V], V, *args, *warp, step=step)
    eos = int(want[0])                                                # sample 0 draws eos at this step
    tok = torch.full((B,), -1, dtype=torch.long, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    if B > 1:
        done[1] = True
    out = torch.full((B, step + 3), -7, dtype=torch.long, device=dev)
    state = torch.tensor([11, step, 0, 0], dtype=torch.int32, device=dev)
    ops.decode_emit_sample_warp(xd[:, :V], V, pad, eos, tok, done, out, state, *args, *warp)
    exp = want.clone()
    if B > 1:
        exp[1] = pad
    assert torch.equal(out[:, step], exp) and torch.equal(tok, exp)
    assert bool((out[:, :step] == -7).all()) and bool((out[:, step + 1:] == -7).all())
    assert torch.equal(done, (exp == eos) | (torch.arange(B, device=dev) == 1) & (B > 1))
    assert state.tolist() == [12, step + 1, 0, 0]
    # the next step reads its counter from the device: column step + 1 holds sample_rows(step + 1), pad where finished
    ops.decode_emit_sample_warp(xd[:, :V], V, pad, eos, tok, done.clone(), out, state, *args, *warp)
    nxt = torch.where(done, torch.full_like(want, pad), ops.sample_rows_warp(xd[:, :V], V, *args, *warp, step=step + 1))
    assert torch.equal(out[:, step + 1], nxt) and state.tolist() == [13, step + 2, 0, 0]
    ops.decode_emit(xd[:, :V], V, pad, eos, tok, done.clone(), out, state)
    assert state.tolist() == [14, step + 3, 0, 0]


# ------------------------------------------------------------------------------------------------ 6. generate() --
WARP = dict(do_sample=True, temperature=0.8, top_k=40, top_p=0.95, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4,
            eta_cutoff=2e-3, seed=21)


def test_generate_paths_emit_the_same_ids_with_the_warpers_on(dev):
    """the hipGraph path, the eager loop, the padded-batch loops and use_cache=False with one seed and the warpers on.
    Ids are compared where the paths' logits agree far below a draw's resolution: the graph path against the eager loop
    of the plain and the padded batch in fp16 (a padded batch's eager loop makes the graph path's launches one by one),
    and the cached loop against use_cache=False in fp32 (logits apart by 1e-6).  In 16 bits use_cache=False recomputes
    the prefix with other kernels and its logits differ in their last bits, so a draw on a boundary differs (generate's
    docstring; tests/test_stopping_gpu.py: sampled ids are reproducible per path only) -- measured here in fp16 at this
    seed: rows 1 and 2 of 3 identical over 12 tokens, row 0 apart from token 1 on; in bf16 the eager loop of the plain
    batch left the graph path's ids in row 0 at token 4.  That is the logits' doing, with or without the warpers."""
    lm, cfg_l = _small_llama(dev, torch.float16)
    V = cfg_l["vocab_size"]
    ids = _ids(cfg_l, 3, dev)
    mask = torch.ones_like(ids)
    for b in range(3):
        mask[b, :2 + 3 * b] = 0
    sharp = {**WARP, "temperature": 0.5, "min_p": 0.2}
    off = dict(min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    for extra in (dict(), dict(attention_mask=mask)):                # the plain batch, then the padded-batch loops
        kw = _kw(cfg_l, 3, dev, **sharp, **extra)
        with _Spy("decode_emit_sample_warp", "sample_rows_warp", "decode_emit_sample", "sample_rows") as spy:
            graph = lm.generate(**kw)
            assert len(spy.calls["decode_emit_sample_warp"]) == 3     # token 0, one eager step, one captured step
            assert tuple(spy.calls["decode_emit_sample_warp"][0][8:]) == (0.5, 40, 0.95, 21, 0.2, 0.9, 3e-4, 2e-3)
            eager = lm.generate(decode_graph=False, **kw)
            nocache = lm.generate(use_cache=False, **kw)
            assert len(spy.calls["sample_rows_warp"]) == 24
            assert spy.calls["decode_emit_sample"] == [] and spy.calls["sample_rows"] == []
        assert graph.shape == (3, 12) and int(graph.min()) >= 0 and int(graph.max()) < V
        assert nocache.shape == (3, 12) and int(nocache.min()) >= 0 and int(nocache.max()) < V
        assert torch.equal(graph, eager), (graph.tolist(), eager.tolist())
        assert torch.equal(graph, lm.generate(**kw))                  # the same call, the same ids
        assert torch.equal(nocache, lm.generate(use_cache=False, **kw))
        assert not torch.equal(graph, lm.generate(**{**kw, "seed": 22}))
        assert not torch.equal(graph, lm.generate(**{**kw, **off}))   # the warpers are felt
        assert not torch.equal(graph, lm.generate(**{k: v for k, v in kw.items() if k not in WARP}))   # ... and it is no argmax
    lm, cfg_l = _small_llama(dev, torch.float32)
    kw = _kw(cfg_l, 3, dev, **sharp)
    cached, nocache = lm.generate(**kw), lm.generate(use_cache=False, **kw)
    assert torch.equal(cached, nocache), (cached.tolist(), nocache.tolist())
    assert not torch.equal(cached, lm.generate(**{**kw, **off}))


def test_generate_min_p_1_is_greedy(dev):
    lm, cfg_l = _small_llama(dev, torch.float32)                      # fp32 logits: no tie at a maximum
    for path in (dict(), dict(decode_graph=False), dict(use_cache=False)):
        kw = _kw(cfg_l, 3, dev, **path)
        assert torch.equal(lm.generate(do_sample=True, temperature=1.3, top_k=0, min_p=1.0, seed=3, **kw), lm.generate(**kw))
    lm, cfg_l = _small_llama(dev)
    kw = _kw(cfg_l, 3, dev)
    got = lm.generate(do_sample=True, temperature=1.3, top_k=0, min_p=1.0, seed=3, **kw)
    assert got.shape == (3, 12)


def test_generate_num_samples_is_the_repeated_batch(dev):
    lm, cfg_l = _small_llama(dev)
    kw = _kw(cfg_l, 2, dev, **WARP)
    got = lm.generate(num_samples=3, **kw)
    want = lm.generate(**{**kw, "input_ids": kw["input_ids"].repeat_interleave(3, 0)})
    assert got.shape == (6, 12) and torch.equal(got, want), (got.tolist(), want.tolist())
    assert not torch.equal(got[0], got[1])


def test_generate_with_a_grammar_emits_only_allowed_ids(dev):
    from test_grammar_gpu import NUMBER, _answer, _model_vocab
    from macaw_llm_amd.grammar import TokenDFA
    lm, cfg_l = _small_llama(dev)
    V, eos = cfg_l["vocab_size"], 2
    g = TokenDFA.from_regex(NUMBER, _model_vocab(V))
    for path in (dict(), dict(decode_graph=False)):
        got = lm.generate(grammar=g, **_kw(cfg_l, 3, dev, max_new_tokens=24, eos_token_id=eos, **WARP, **path))
        for row in got.tolist():
            answer, _ = _answer(row, 0, eos, 24)
            assert len(answer) > 0 and g.walk(answer) is not None, (path, row)       # every id allowed where it stands


def test_set_sampling_carries_the_warpers_to_generate(dev):
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    seen = {}
    real = model.llm.generate

    def generate(**kw):
        seen.update(kw)
        seen["ids"] = real(**kw)
        return seen["ids"]
    with torch.no_grad(), _Spy("decode_emit", "decode_emit_sample", "decode_emit_sample_warp") as spy:
        Mo.MM_LLMs.set_sampling(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=4)
        plain = model(inputs=inp)
        assert tuple(spy.calls["decode_emit_sample"][0][8:]) == (0.9, 30, 0.95, 4)
        Mo.MM_LLMs.set_sampling(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=4, min_p=0.1, typical_p=0.8)
        model.llm.generate = generate
        try:
            ids = model(inputs=inp)
        finally:
            del model.llm.generate
        assert tuple(spy.calls["decode_emit_sample_warp"][-1][8:]) == (0.9, 30, 0.95, 4, 0.1, 0.8, 0.0, 0.0)
        assert (seen["min_p"], seen["typical_p"], seen["epsilon_cutoff"], seen["eta_cutoff"]) == (0.1, 0.8, 0.0, 0.0)
        direct = real(**{k: v for k, v in seen.items() if k != "ids"})            # the direct call with these arguments
        assert torch.equal(ids, direct) and torch.equal(ids, model(inputs=inp))
        assert ids.dtype == torch.long and ids.shape[0] == plain.shape[0]
        Mo.MM_LLMs.set_sampling()
        n = len(spy.calls["decode_emit_sample"]) + len(spy.calls["decode_emit_sample_warp"])
        model(inputs=inp)
        assert len(spy.calls["decode_emit_sample"]) + len(spy.calls["decode_emit_sample_warp"]) == n and Mo.SAMPLING_WARPERS[0]["min_p"] is None


# ---------------------------------------------------------------------------------------------- 7. determinism --
def test_same_call_same_ids_and_seed_and_step_matter(dev):
    V, rows, ld = 32007, 8, 32064
    xd, _ = _logits(V, rows, ld, 3.0, torch.bfloat16, seed=2)
    warp = (0.01, 0.95, 3e-4, 2e-3)
    a = [ops.sample_rows_warp(xd[:, :V], V, 1.3, 0, 0.9, 77, *warp, step=step) for step in range(8)]
    b = [ops.sample_rows_warp(xd[:, :V], V, 1.3, 0, 0.9, 77, *warp, step=step) for step in range(8)]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = [ops.sample_rows_warp(xd[:, :V], V, 1.3, 0, 0.9, 78, *warp, step=step) for step in range(8)]
    assert any(not torch.equal(x, y) for x, y in zip(a, c))           # another seed
    assert any(not torch.equal(a[0], x) for x in a[1:])               # another step
    m = [ops.sample_keep_rows(xd[:, :V], V, 1.3, 0, 0.9, *warp) for _ in range(3)]
    assert torch.equal(m[0], m[1]) and torch.equal(m[0], m[2])
