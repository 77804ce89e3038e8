"""GPU: sampled decoding -- ops.sample_rows / ops.decode_emit_sample (csrc/sample.hip) against the float64 reference of
tests/test_sampling_cpu.py, the cases that involve no arithmetic held exactly, determinism, the step bookkeeping against
ops.decode_emit's, and generate(do_sample=True) end to end on the hipGraph path and the two eager loops.

The draw test accepts an emitted column c iff (a) it is in the reference's kept set with the top-p rule relaxed to
above < (p + EPS) * Z and (b) its CDF interval widened by 4 * EPS * Z contains u * Z, EPS = 2^-16: about three times the
worst-case fp32 error of a 32k-term blocked sum plus the error of exp (the kernel's fixed-point masses are far inside
it).  Every case is held to that rule.  The rule was meant to come with a precondition asserted on the fixtures -- no
column heavier than EPS * Z has its top-p criterion within EPS * Z of the threshold, so that an EPS-accurate kernel could
never be failed for keeping or dropping such a column -- but randn fixtures cannot meet it: at V = 32007, sigma = 3, p = 0.9
the criteria of neighbouring columns lie about 4e-5 * Z apart around the threshold against a window of 3e-5 * Z, and each of
the torch seeds 0 ... 39 had a row inside it (every dtype).  The precondition only ever protected the kernel from a false
failure, so it is dropped and the rule applied regardless: that asks more of the kernel, not less.  It passes because its
masses carry a relative error near 2^-19 (the fp32 rounding of x - x_max, expf), not 2^-16."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_decode_kv8_gpu import _Spy, _ids, _small_llama  # noqa: E402
from test_sampling_cpu import filter_row, sample_row, uniform  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

EPS = 2.0 ** -16
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SHAPES = [(32007, 8, 32064), (1000, 3, 1000), (1, 2, 1), (8193, 33, 8193)]         # V, rows, pitch


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.MM_LLMs.set_sampling()
    ops.clear_fp8_cache()


def _logits(V, rows, ld, sigma, dtype, seed=0):
    """randn * sigma rounded to dtype, pad columns [V, ld) = +1e4 -> (device tensor [rows, ld], fp32 numpy [rows, V])"""
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(seed + V)) * sigma
    full = torch.full((rows, ld), 1e4)
    full[:, :V] = x
    full = full.to(dtype)
    return full.cuda(), full[:, :V].float().numpy()


# ------------------------------------------------------------------------------------ 1. the draw vs the reference --
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("sigma", [3.0, 6.0])
@pytest.mark.parametrize("V,rows,ld", SHAPES)
def test_draw_lies_in_the_reference_kept_set_and_cdf_interval(dev, V, rows, ld, sigma, dtype):
    xd, xh = _logits(V, rows, ld, sigma, dtype)
    seed = 0x1234_5678_9ABC_DEF0 + V
    for T, k, p in [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95), (1.0, V + 5, 1.0)]:
        got = torch.stack([ops.sample_rows(xd[:, :V], V, T, k, p, seed, step) for step in range(16)]).cpu().numpy()
        assert got.min() >= 0 and got.max() < V, (T, k, p)            # never a pad column
        for r in range(rows):
            f = filter_row(xh[r], V, T, k, p)
            relaxed = filter_row(xh[r], V, T, k, p, p_slack=EPS)["kept"]
            e = np.where(f["kept"], f["e"], 0.0)
            cum = np.cumsum(e)
            Z = cum[-1]
            for step in range(16):
                c = int(got[step, r])
                uZ = uniform(seed, step, r) * Z
                lo, hi = cum[c] - e[c], cum[c]
                assert relaxed[c], (T, k, p, r, step, c)
                assert lo - 4 * EPS * Z <= uZ <= hi + 4 * EPS * Z, (T, k, p, r, step, c, lo / Z, hi / Z, uZ / Z)


# -------------------------------------------------------------------------- 2. exact where no arithmetic is involved --
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_top_k_1_and_tiny_top_p_are_argmax_bit_for_bit(dev, dtype):
    V, rows, ld = 32007, 8, 32064
    xd, _ = _logits(V, rows, ld, 3.0, dtype, seed=1)
    xd[1, 4000] = xd[1, 17] = xd[1, 31000] = 50.0                     # a duplicated maximum: the lower column wins
    xd[2, V - 1] = 60.0
    am = ops.argmax_rows(xd[:, :V], V)
    assert int(am[1]) == 17 and int(am[2]) == V - 1
    for step in range(4):
        for T in (1.0, 0.7):
            assert torch.equal(ops.sample_rows(xd[:, :V], V, T, 1, 1.0, 5, step), am)
            assert torch.equal(ops.sample_rows(xd[:, :V], V, T, 1, 0.5, 5, step), am)
    xu = xd.clone()                                                   # unique maxima
    xu[1, 4000] = xu[1, 31000] = 0.0
    for r in range(rows):
        xu[r, (r * 4001) % V] = 70.0 + r
    am = ops.argmax_rows(xu[:, :V], V)
    for step in range(4):
        assert torch.equal(ops.sample_rows(xu[:, :V], V, 1.0, 0, 1e-6, 5, step), am)
        assert torch.equal(ops.sample_rows(xu[:, :V], V, 0.9, 50, 1e-6, 5, step), am)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_tie_row_keeps_the_lower_columns_and_nan_or_minus_inf_are_never_drawn(dev, dtype):
    tie = torch.tensor([[5.0, 3.0, 3.0, 3.0, 1.0]], dtype=dtype, device=dev)
    seen = {int(ops.sample_rows(tie, 5, 1.0, 2, 1.0, 21, step)) for step in range(64)}
    assert seen == {0, 1}, seen
    seen = {int(ops.sample_rows(tie, 5, 4.0, 3, 1.0, 21, step)) for step in range(64)}
    assert seen == {0, 1, 2}, seen
    # a tie group that spans threads: 2100 equal values, k admits the first 1500 of them
    V = 2100
    flat = torch.zeros((1, V), dtype=dtype, device=dev)
    got = torch.cat([ops.sample_rows(flat, V, 1.0, 1500, 1.0, 3, step) for step in range(64)])
    ref = [sample_row(np.zeros(V, np.float32), V, 1.0, 1500, 1.0, 3, step) for step in range(64)]
    assert got.tolist() == ref and max(ref) < 1500                    # equal masses: integer arithmetic on both sides
    nan, ninf = float("nan"), float("-inf")
    bad = torch.tensor([[nan, ninf, 0.5, nan, 0.25, ninf, 0.0], [ninf, ninf, ninf, ninf, ninf, ninf, ninf],
                        [ninf, ninf, nan, ninf, nan, ninf, ninf]], dtype=dtype, device=dev)
    for k, p in ((0, 1.0), (6, 0.99)):
        out = torch.stack([ops.sample_rows(bad, 7, 1.0, k, p, 8, step) for step in range(64)])
        assert set(out[:, 0].tolist()) == {2, 4, 6}
        assert set(out[:, 1].tolist()) == {0} and set(out[:, 2].tolist()) == {2}      # no finite logit: greedy's choice


# ---------------------------------------------------------------------------------------------- 3. determinism --
def test_same_call_same_ids_and_seed_and_step_matter(dev):
    V, rows, ld = 32007, 8, 32064
    xd, _ = _logits(V, rows, ld, 3.0, torch.bfloat16, seed=2)
    a = [ops.sample_rows(xd[:, :V], V, 0.8, 40, 0.95, 77, step) for step in range(8)]
    b = [ops.sample_rows(xd[:, :V], V, 0.8, 40, 0.95, 77, step) for step in range(8)]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = [ops.sample_rows(xd[:, :V], V, 0.8, 40, 0.95, 78, step) for step in range(8)]
    assert any(not torch.equal(x, y) for x, y in zip(a, c))           # another seed
    assert any(not torch.equal(a[0], x) for x in a[1:])               # another step


# --------------------------------------------------------------------------- 4. decode_emit_sample vs sample_rows --
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_decode_emit_sample_draws_sample_rows_token_and_keeps_decode_emits_books(dev, B, dtype):
    V, ld, step, pad = 1000, 1008, 5, 1003
    xd, _ = _logits(V, B, ld, 3.0, dtype, seed=3)
    args = (0.8, 40, 0.95, 4242)
    want = ops.sample_rows(xd[:, :V], V, *args, step=step)
    eos = int(want[0])                                                # sample 0 draws eos at this step
    tok = torch.full((B,), -1, dtype=torch.long, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    if B > 1:
        done[1] = True
    out = torch.full((B, step + 3), -7, dtype=torch.long, device=dev)
    state = torch.tensor([11, step, 0, 0], dtype=torch.int32, device=dev)
    ops.decode_emit_sample(xd[:, :V], V, pad, eos, tok, done, out, state, *args)
    exp = want.clone()
    if B > 1:
        exp[1] = pad
    assert torch.equal(out[:, step], exp) and torch.equal(tok, exp)
    assert bool((out[:, :step] == -7).all()) and bool((out[:, step + 1:] == -7).all())
    assert torch.equal(done, (exp == eos) | (torch.arange(B, device=dev) == 1) & (B > 1))
    assert state.tolist() == [12, step + 1, 0, 0]
    # the next step reads its counter from the device: column step + 1 holds sample_rows(step + 1), pad where finished
    ops.decode_emit_sample(xd[:, :V], V, pad, eos, tok, done.clone(), out, state, *args)
    nxt = torch.where(done, torch.full_like(want, pad), ops.sample_rows(xd[:, :V], V, *args, step=step + 1))
    assert torch.equal(out[:, step + 1], nxt) and state.tolist() == [13, step + 2, 0, 0]
    # greedy's bookkeeping on the same inputs moves the state the same way
    ops.decode_emit(xd[:, :V], V, pad, eos, tok, done.clone(), out, state)
    assert state.tolist() == [14, step + 3, 0, 0]


# ------------------------------------------------------------------------------------------------ 5. generate() --
def _kw(cfg_l, B, dev, **over):
    return {**dict(input_ids=_ids(cfg_l, B, dev), max_new_tokens=12, eos_token_id=-1, pad_token_id=0), **over}


def test_generate_top_k_1_is_greedy_on_every_weight_and_cache_format(dev):
    lm, cfg_l = _small_llama(dev)
    for extra in ({}, dict(decode_weights="fp8"), dict(kv_cache="fp8"), dict(decode_weights="fp8", kv_cache="fp8")):
        kw = _kw(cfg_l, 3, dev, **extra)
        with _Spy("decode_emit", "decode_emit_sample") as spy:
            greedy = lm.generate(**kw)
            assert len(spy.calls["decode_emit"]) == 3 and spy.calls["decode_emit_sample"] == []
            got = lm.generate(do_sample=True, top_k=1, temperature=0.7, seed=3, **kw)
            assert len(spy.calls["decode_emit"]) == 3 and len(spy.calls["decode_emit_sample"]) == 3   # the graph path
        assert torch.equal(got, greedy), extra


def test_generate_seed_governs_the_ids(dev):
    lm, cfg_l = _small_llama(dev)
    V = cfg_l["vocab_size"]
    kw = _kw(cfg_l, 4, dev, do_sample=True, temperature=1.5, top_k=0)
    a = lm.generate(seed=1, **kw)
    assert a.shape == (4, 12) and a.dtype == torch.long and int(a.min()) >= 0 and int(a.max()) < V
    assert torch.equal(a, lm.generate(seed=1, **kw))
    assert not torch.equal(a, lm.generate(seed=2, **kw))              # fails where do_sample is swallowed
    torch.manual_seed(123)
    b = lm.generate(**kw)
    torch.manual_seed(123)
    assert torch.equal(b, lm.generate(**kw))
    assert not torch.equal(b, lm.generate(**kw))                      # the generator has moved on: a fresh seed
    # the defaults (top_k = 50, top_p = 1) and a top-p call run and stay inside the vocabulary
    for extra in (dict(), dict(top_p=0.9), dict(top_k=None, top_p=0.5)):
        c = lm.generate(**{**_kw(cfg_l, 4, dev, do_sample=True, seed=5), **extra})
        assert c.shape == (4, 12) and int(c.min()) >= 0 and int(c.max()) < V


def test_generate_sampled_eos_marks_a_row_done_and_pad_follows(dev):
    lm, cfg_l = _small_llama(dev)
    kw = _kw(cfg_l, 4, dev, max_new_tokens=24, do_sample=True, temperature=1.2, top_k=8, seed=17)
    free = lm.generate(**kw)
    eos = int(free[:, 2:8].flatten().mode().values)
    f = lm.generate(**{**kw, "eos_token_id": eos})
    hit = (f == eos).cumsum(1) > 0
    assert bool(hit.any())
    assert bool(hit[:, -1].all()) or f.shape[1] == 24
    after = torch.zeros_like(hit)
    after[:, 1:] = hit[:, :-1]
    assert bool((f[after] == 0).all())                                # pad after a row's eos
    assert torch.equal(f[~after], free[:, :f.shape[1]][~after])       # the same draws before it (counter = column)


def test_generate_eager_loops_are_self_consistent(dev):
    lm, cfg_l = _small_llama(dev)
    V = cfg_l["vocab_size"]
    for path in (dict(decode_graph=False), dict(use_cache=False)):
        kw = _kw(cfg_l, 3, dev, do_sample=True, temperature=1.3, top_k=20, top_p=0.9, **path)
        with _Spy("sample_rows", "decode_emit_sample", "argmax_rows") as spy:
            a = lm.generate(seed=9, **kw)
            assert len(spy.calls["sample_rows"]) == 12 and spy.calls["decode_emit_sample"] == []
            assert spy.calls["argmax_rows"] == []
        assert a.shape == (3, 12) and int(a.min()) >= 0 and int(a.max()) < V
        assert torch.equal(a, lm.generate(seed=9, **kw))
        assert not torch.equal(a, lm.generate(seed=10, **{**kw, "temperature": 3.0, "top_k": 0, "top_p": 1.0}))


def test_generate_refuses_bad_sampling_arguments_only_when_sampling(dev):
    lm, cfg_l = _small_llama(dev)
    kw = _kw(cfg_l, 2, dev)
    for bad, name in ((dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
                      (dict(temperature=float("nan")), "temperature"), (dict(top_p=0.0), "top_p"),
                      (dict(top_p=1.01), "top_p"), (dict(top_k=-2), "top_k")):
        with pytest.raises(ValueError, match=name):
            lm.generate(do_sample=True, **bad, **kw)
        assert torch.equal(lm.generate(**bad, **kw), lm.generate(**kw))       # ignored by greedy decoding


def test_set_sampling_reaches_generate(dev):
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    with torch.no_grad(), _Spy("decode_emit", "decode_emit_sample") as spy:
        base = model(inputs=inp)
        assert spy.calls["decode_emit_sample"] == [] and len(spy.calls["decode_emit"]) > 0
        Mo.MM_LLMs.set_sampling(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=4)
        ids = model(inputs=inp)
        calls = spy.calls["decode_emit_sample"]
        assert len(calls) > 0 and tuple(calls[0][8:]) == (0.9, 30, 0.95, 4)
        assert torch.equal(ids, model(inputs=inp))                    # an integer seed: the same ids again
        Mo.MM_LLMs.set_sampling(do_sample=True, top_k=1)
        assert torch.equal(model(inputs=inp), base)                   # top_k = 1: greedy's ids
        Mo.MM_LLMs.set_sampling()
        n = len(spy.calls["decode_emit_sample"])
        assert torch.equal(model(inputs=inp), base) and len(spy.calls["decode_emit_sample"]) == n
    assert ids.dtype == torch.long and ids.shape[0] == base.shape[0]
