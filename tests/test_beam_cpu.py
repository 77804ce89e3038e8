"""CPU: beam search -- the rule of include/macaw_hip.h as restated in tests/beam_ref.py on hand-worked cases (expected
values written here), the host half of generate(num_beams=K) (macaw_llm_amd/beam.py) on the same cases, the ABI of the
two new entry points, the public arguments and their refusals, the launch sequence of a beam step (the fake-ops
technique of tests/test_decode_trace_cpu.py), and the precondition of the GPU selection test's input generator."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import beam_ref as R
from test_decode_trace_cpu import RETURNS, Trace, _t

from macaw_llm_amd import beam as hostbeam
from macaw_llm_amd import engine as eng
from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
ln = math.log


# ------------------------------------------------------------------------------------ 1. hand-worked cases --
# V = 8, K = 2, eos = 7, pad = 0, three steps.  Rows are PROBABILITIES (each sums to 1, so lse = 0 and cand = s_k +
# ln p); the expected values below are worked out by hand from them.
def _row(**p):
    """a probability row over 8 tokens: t<i>=p for the named ones, the rest share what is left equally"""
    row = np.zeros(8)
    named = {int(k[1:]): v for k, v in p.items()}
    rest = (1.0 - sum(named.values())) / (8 - len(named))
    row[:] = rest
    for i, v in named.items():
        row[i] = v
    assert abs(row.sum() - 1.0) < 1e-12
    return np.log(row)


STEP0 = [[_row(t1=0.4, t2=0.3)]]                    # the others 0.05 each: the eos is not among the best four
# beams after step 0: [1] ln .4, [2] ln .3
STEP1 = [[_row(t7=0.5, t3=0.25, t4=0.15), _row(t5=0.45, t7=0.4, t6=0.05)]]
# candidates: (0, eos) .2 | (1, 5) .135 | (1, eos) .12 | (0, 3) .10 | (0, 4) .06 ...
#   rank 0 eos -> pool A = ln(.2) / 2;  rank 1 -> beam 0 = [2, 5];  rank 2 eos, rank >= K: SKIPPED;  rank 3 -> beam 1 = [1, 3]
STEP2_A = [[_row(t1=0.9, t7=0.05, t2=0.02), _row(t7=0.9, t2=0.04)]]
# candidates: (0, 1) .1215 | (1, eos) .09 | (0, eos) .00675 | (1, 2) .004 | (0, 2) .0027 ...
#   rank 0 -> beam 0 = [2, 5, 1];  rank 1 eos -> pool B = ln(.09) / 3 (the pool is full);  rank 2 eos: skipped;
#   rank 3 -> beam 1 = [1, 3, 2]
STEP2_B = [[_row(t7=0.9, t1=0.04), _row(t7=0.9, t2=0.04)]]
# candidates: (0, eos) .1215 | (1, eos) .09 | (0, 1) .0054 | (1, 2) .004 ...
#   rank 0 eos -> pool B' = ln(.1215) / 3 appended;  rank 1 eos -> C = ln(.09) / 3 > A = ln(.2) / 2: REPLACES A
A, B_, C = ln(0.2) / 2, ln(0.09) / 3, ln(0.09) / 3
assert C > A


def _run(steps, early, lp=1.0):
    ref = R.BeamRef(1, 2, 3, pad=0, eos=7, length_penalty=lp, early_stopping=early)
    for s in steps:
        ref.step(np.array(s))
    return ref


def _close(a, b):
    assert len(a) == len(b) and all(abs(x - y) < 1e-9 for x, y in zip(a, b)), (a, b)


def test_hand_worked_steps_0_and_1_eos_enters_below_rank_K_and_is_skipped_above():
    ref = _run([STEP0, STEP1], early=False)
    assert ref.hist[0, 0].tolist() == [[1, 0], [2, 0]]
    assert ref.hist[1, 0].tolist() == [[5, 1], [3, 0]]                  # (token, parent)
    _close(ref.scores[0], [ln(0.135), ln(0.10)])
    assert len(ref.pool[0]) == 1                                        # the eos at rank 2 was skipped
    _close(ref.pool[0][0][:1], [A])
    assert ref.pool[0][0][1:] == [1, 0, 0]                              # column 1, parent beam 0, insertion 0
    assert ref.done == [False]
    assert ref.ind[0, :, :2].tolist() == [[1, 0], [0, 1]]               # beam 0 continues slot 1, beam 1 slot 0
    assert ref.tok[0].tolist() == [5, 3]


def test_hand_worked_early_stopping_modes_finalisation_and_two_return_sequences():
    # early_stopping=True: done as soon as the pool holds K
    ref = _run([STEP0, STEP1, STEP2_A], early=True)
    assert ref.done == [True] and len(ref.pool[0]) == 2
    rows, scores = ref.finalize(2)
    assert R.padded(rows, 0) == [[1, 3, 7], [1, 7, 0]]                  # B = [1, 3, eos], then A = [1, eos] + pad
    _close(scores, [B_, A])
    # early_stopping=False: the best running beam, ln(.1215) / 3, still beats the worst entry A: not done
    ref = _run([STEP0, STEP1, STEP2_A], early=False)
    assert ref.done == [False]
    _close(ref.scores[0], [ln(0.1215), ln(0.004)])
    # ... so the sample is finalised: beam 0 replaces A (strictly greater), beam 1 (ln(.004) / 3) does not get in
    rows, scores = ref.finalize(2)
    assert rows == [[2, 5, 1], [1, 3, 7]]
    _close(scores, [ln(0.1215) / 3, B_])
    rows1, scores1 = _run([STEP0, STEP1, STEP2_A], early=False).finalize(1)
    assert rows1 == [[2, 5, 1]] and abs(scores1[0] - ln(0.1215) / 3) < 1e-9
    # a further step changes nothing in the books of a done sample, and its rows are fed pad
    ref = _run([STEP0, STEP1, STEP2_A], early=True)
    ref.n_max = 4
    ref.hist = np.concatenate([ref.hist, np.zeros((1, 1, 2, 2), dtype=np.int64)])
    ref.ind = np.concatenate([ref.ind, np.zeros((1, 2, 1), dtype=np.int64)], axis=2)
    before = (ref.scores.copy(), [list(e) for e in ref.pool[0]])
    ref.step(np.array(STEP2_B))
    assert ref.tok[0].tolist() == [0, 0] and ref.hist[3, 0].tolist() == [[0, 0], [0, 1]]
    assert np.array_equal(ref.scores, before[0]) and ref.pool[0] == before[1]


def test_hand_worked_pool_replacement_inside_a_step():
    for early in (False, True):
        ref = _run([STEP0, STEP1, STEP2_B], early=early)
        assert ref.done == [True]                                       # ln(.0054) / 3 <= the worst entry
        assert [e[1:] for e in ref.pool[0]] == [[2, 1, 2], [2, 0, 1]]   # C took A's place; B' was appended
        rows, scores = ref.finalize(2)
        assert rows == [[2, 5, 7], [1, 3, 7]]
        _close(scores, [ln(0.1215) / 3, C])
    # length_penalty = 0: the scores are the plain sums, and A = ln(.2) now beats C = ln(.09): no replacement
    ref = _run([STEP0, STEP1, STEP2_B], early=False, lp=0.0)
    rows, scores = ref.finalize(2)
    assert rows == [[1, 7], [2, 5, 7]]
    _close(scores, [ln(0.2), ln(0.1215)])


def test_eos_none_never_matches_and_k1_is_argmax_decoding():
    g = np.random.default_rng(0)
    ref = R.BeamRef(3, 1, 6, pad=0, eos=None)
    want = []
    for t in range(6):
        x = g.standard_normal((3, 1, 50))
        ref.step(x)
        want.append(x[:, 0].argmax(1))
    rows, scores = ref.finalize(1)
    assert rows == np.stack(want, 1).tolist()
    assert ref.done == [False] * 3 and all(len(p) == 1 for p in ref.pool)


# ------------------------------------------------------------- 2. the host half (macaw_llm_amd/beam.py) on the same --
def _books(ref):
    """BeamRef -> the CPU tensors ops.BeamState would hold"""
    B, K = ref.B, ref.K
    hist = torch.from_numpy(ref.hist[..., :]).to(torch.int32)
    scores = torch.from_numpy(ref.scores.reshape(-1)).float()
    ps = torch.zeros((B, K))
    pi = torch.zeros((B, K + 1, 4), dtype=torch.int32)
    for b in range(B):
        for e, (s, col, par, seq) in enumerate(ref.pool[b]):
            ps[b, e] = s
            pi[b, e, :3] = torch.tensor([col, par, seq])
        pi[b, K, 0], pi[b, K, 1] = len(ref.pool[b]), ref.seq[b]
    return hist, scores, ps, pi, torch.tensor(ref.done)


@pytest.mark.parametrize("steps,early,lp", [([STEP0, STEP1, STEP2_A], True, 1.0), ([STEP0, STEP1, STEP2_A], False, 1.0),
                                            ([STEP0, STEP1, STEP2_B], False, 1.0), ([STEP0, STEP1, STEP2_B], False, 0.0),
                                            ([STEP0, STEP1], False, 0.7)])
@pytest.mark.parametrize("nret", [1, 2])
def test_beam_result_finalises_sorts_and_backtracks_like_the_restatement(steps, early, lp, nret):
    ref = _run(steps, early, lp)
    ids, sc = hostbeam.beam_result(*_books(ref), ref.col, lp, nret, 0, 7)
    rows, scores = ref.finalize(nret)
    assert ids.tolist() == R.padded(rows, 0) and ids.dtype == torch.long
    assert sc.dtype == torch.float32 and np.allclose(sc.numpy(), scores, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------- 3. the ABI --
def _arity(name):
    src = open(HEADER).read()
    m = re.search(r"^int " + name + r"\((.*?)\);", src, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/macaw_hip.h"
    return len(m.group(1).split(","))


def test_header_declares_both_entry_points_with_the_arity_of_the_prototypes_and_abi_11():
    for name in ("mk_beam_emit", "mk_decode_step_attn_beam"):
        assert _arity(name) == len(L.SIGNATURES[name]), name
    src = open(HEADER).read()
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == 11 == L.ABI_VERSION
    for phrase in ("Take the 2K best candidates by value descending", "replace the latest inserted",
                   "A sample that was already done changes nothing in its books", "State layout"):
        assert phrase in src, phrase


def test_the_library_exports_them_and_bad_arguments_return_codes():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    assert lib.mk_abi_version() == 11
    for name in ("mk_beam_emit", "mk_decode_step_attn_beam"):           # null pointers: a code, nothing launched
        args = [None if t is L._vp else t(0) for t in L.SIGNATURES[name]]
        assert getattr(lib, name)(*args) == -1, name


# ------------------------------------------------------------------------- 4. public arguments and refusals --
def test_generate_and_set_beam_search_carry_the_new_arguments():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    want = dict(num_beams=1, length_penalty=1.0, early_stopping=False, num_return_sequences=1, return_beam_scores=False)
    for k, v in want.items():
        assert p[k].default == v and type(p[k].default) is type(v), k
    p = inspect.signature(Mo.MM_LLMs.set_beam_search).parameters
    for k in ("num_beams", "length_penalty", "early_stopping", "num_return_sequences"):
        assert p[k].default == want[k], k
    try:
        Mo.MM_LLMs.set_beam_search(num_beams=4, length_penalty=0.5, early_stopping=True, num_return_sequences=2)
        assert Mo.BEAM_SEARCH[0] == dict(num_beams=4, length_penalty=0.5, early_stopping=True, num_return_sequences=2)
        with pytest.raises(ValueError, match="num_return_sequences"):
            Mo.MM_LLMs.set_beam_search(num_beams=2, num_return_sequences=3)
    finally:
        Mo.MM_LLMs.set_beam_search()
    assert Mo.BEAM_SEARCH[0]["num_beams"] == 1
    assert "**BEAM_SEARCH[0]" in inspect.getsource(Mo.MM_LLMs.forward)


def test_beam_check_raises_for_each_bad_value_and_ignores_everything_at_one_beam():
    chk = hostbeam.beam_check
    for bad in (0, 17, -1, 2.0, "4", None, True):
        with pytest.raises(ValueError, match="num_beams"):
            chk("generate", bad)
    assert chk("generate", 1, num_return_sequences=5, vocab=1, do_sample=True, kv_cache="fp8", padded=True) == 1
    assert chk("generate", 16, 16, vocab=32) == 16
    with pytest.raises(ValueError, match="num_return_sequences"):
        chk("generate", 4, 5)
    with pytest.raises(ValueError, match="num_return_sequences"):
        chk("generate", 4, 0)
    with pytest.raises(ValueError, match="vocabulary"):
        chk("generate", 4, 1, vocab=7)
    with pytest.raises(ValueError, match="do_sample"):
        chk("generate", 2, 1, vocab=100, do_sample=True)
    with pytest.raises(ValueError, match="kv_cache"):
        chk("generate", 2, 1, vocab=100, kv_cache="fp8")
    with pytest.raises(ValueError, match="attention_mask"):
        chk("generate", 2, 1, vocab=100, padded=True)
    with pytest.raises(ValueError, match="length_penalty"):
        chk("generate", 2, 1, length_penalty=float("nan"))


def test_decode_weights_limit_names_b_times_k():
    chk = Mo._decode_fp8_check          # (dtype, head size, B, S0, max_new_tokens, use_cache, why no graph is captured)
    chk(torch.bfloat16, 64, 8, 5, 12, True, None, value="mxfp4", beams=4)              # 32 rows: inside
    with pytest.raises(ValueError, match=r"B x num_beams = 9 x 4 = 36"):
        chk(torch.bfloat16, 64, 9, 5, 12, True, None, value="fp8", beams=4)
    with pytest.raises(ValueError, match="33 sequences"):                              # the greedy text is unchanged
        chk(torch.bfloat16, 64, 33, 5, 12, True, None)


# ---------------------------------------------------------------------- 5. the launch sequence of a beam step --
BF, U8, F32, I32 = torch.bfloat16, torch.uint8, torch.float32, torch.int32
BEAM_RETURNS = {**RETURNS,
                "decode_linear_mxfp4": lambda a: (a["out"] if a.get("out") is not None else
                                                  _t(a["x"].shape[0], a["Wq"].shape[0], dtype=a["x"].dtype)),
                "decode_step_attn_beam": lambda a: a["out"],
                "decode_step_attn_var": lambda a: a["out"]}


SIGS = {name: inspect.signature(getattr(ops, name)) for name in BEAM_RETURNS}      # of the real ops, taken once


class BeamTrace(Trace):
    def __init__(self, monkeypatch):
        self.calls, self.bufs, self.keep = [], {}, []
        for name, ret in BEAM_RETURNS.items():
            monkeypatch.setattr(ops, name, self._rec(name, SIGS[name], ret))

    def _rec(self, name, sig, ret):
        def rec(*args, **kw):
            a = sig.bind(*args, **kw)
            a.apply_defaults()
            self.calls.append((name, dict(a.arguments)))
            return ret(dict(a.arguments))
        return rec


def _layer_case(monkeypatch, weights, B=2, K=4, D=128, FF=256, hd=64, S0=5, TMAX=12, fused=True):
    H, M = D // hd, B * K
    tr = BeamTrace(monkeypatch)
    x2 = _t(M, D)
    wqkv, wgu = _t(3 * D, D), _t(2 * FF, D)
    wq, wk, wv, wg, wu = wqkv[:D], wqkv[D:2 * D], wqkv[2 * D:], wgu[:FF], wgu[FF:]
    wo, wd, ln1, ln2 = _t(D, D), _t(D, FF), _t(D), _t(D)
    q8 = lambda N, Kd: (_t(N, Kd, dtype=U8), _t(N, dtype=F32))                    # noqa: E731
    q4 = lambda N, Kd: (_t(N, Kd // 2, dtype=U8), _t(N, Kd // 32, dtype=U8))      # noqa: E731
    mk = {"w16": None, "fp8": q8, "mxfp4": q4}[weights]
    w8 = None if mk is None else (mk(3 * D, D), mk(D, D), mk(2 * FF, D), mk(D, FF))
    kvc = _t(B, K, TMAX, 2 * D)
    ind = _t(M, TMAX - S0, dtype=I32)
    t_dev = _t(1, dtype=I32)
    out = eng.llama_layer_cached(x2, B, 1, 0, kvc, TMAX, t_dev, _t(TMAX, hd), _t(TMAX, hd), H, 1e-6, wq, wk, wv, wo, wg,
                                 wu, wd, ln1, ln2, wqkv if fused else None, wgu if fused else None, t_dev=t_dev, w8=w8,
                                 beam=eng.Beam(ind, K, S0))
    assert tuple(out.shape) == (M, D)
    return tr.calls, dict(kvc=kvc, ind=ind, t_dev=t_dev, B=B, K=K, H=H, hd=hd, S0=S0, TMAX=TMAX, D=D)


@pytest.mark.parametrize("weights,lin", [("w16", "decode_linear"), ("fp8", "decode_linear_fp8"),
                                         ("mxfp4", "decode_linear_mxfp4")])
def test_beam_step_of_the_layer_is_the_five_launches_with_the_beam_attention(monkeypatch, weights, lin):
    calls, c = _layer_case(monkeypatch, weights)
    assert [n for n, _ in calls] == [lin, "decode_step_attn_beam", lin, lin, lin]
    assert [a["prologue"] for n, a in calls if n == lin] == [1, 0, 1, 2]
    a = calls[1][1]
    assert a["cache"] is c["kvc"] and a["ind"] is c["ind"] and a["t_dev"] is c["t_dev"]
    assert (a["B"], a["K"], a["H"], a["hd"], a["S0"], a["t_max"]) == (c["B"], c["K"], c["H"], c["hd"], c["S0"], c["TMAX"])
    assert (a["in_bs"], a["q_off"], a["k_off"], a["v_off"]) == (3 * c["D"], 0, c["D"], 2 * c["D"])
    assert a["q"] is a["k_new"] is a["v_new"] and tuple(a["q"].shape) == (c["B"] * c["K"], 3 * c["D"])
    for n, args in calls:                               # every weight stream sees the B * K token rows
        if n == lin:
            assert args["x"].shape[0] == c["B"] * c["K"]
    # the same sequence as the greedy step at B * K samples, the attention launch apart
    tr = BeamTrace(monkeypatch)
    D, M = c["D"], c["B"] * c["K"]
    wqkv, wgu = _t(3 * D, D), _t(512, D)
    eng.llama_layer_cached(_t(M, D), M, 1, 0, _t(M, c["TMAX"], 2 * D), c["TMAX"], c["t_dev"], _t(12, 64), _t(12, 64), 2, 1e-6,
                           wqkv[:D], wqkv[D:2 * D], wqkv[2 * D:], _t(D, D), wgu[:256], wgu[256:], _t(D, 256), _t(D), _t(D),
                           wqkv, wgu, t_dev=c["t_dev"])
    if weights == "w16":
        assert [n for n, _ in tr.calls] == [("decode_step_attn" if n == "decode_step_attn_beam" else n) for n, _ in calls]


def test_beam_step_on_unfused_storage_takes_the_general_path_with_the_beam_attention(monkeypatch):
    calls, c = _layer_case(monkeypatch, "w16", fused=False)
    names = [n for n, _ in calls]
    assert names.count("decode_step_attn_beam") == 1 and "decode_step_attn" not in names and "rope_" not in names
    assert "copy2d" not in names                        # no cache row is copied


def test_beam_refuses_what_it_does_not_compose_with(monkeypatch):
    BeamTrace(monkeypatch)
    D = 128
    w = _t(3 * D, D)
    args = (_t(8, D), 2, 1, 0, _t(2, 4, 12, 2 * D), 12, _t(1, dtype=I32), _t(12, 64), _t(12, 64), 2, 1e-6, w[:D], w[D:2 * D],
            w[2 * D:], _t(D, D), _t(256, D), _t(256, D), _t(D, 256), _t(D), _t(D))
    beam = eng.Beam(_t(8, 7, dtype=I32), 4, 5)
    with pytest.raises(ValueError, match="beam"):       # no device position
        eng.llama_layer_cached(*args, beam=beam)
    with pytest.raises(ValueError, match="beam"):       # an e4m3 cache
        eng.llama_layer_cached(*args, t_dev=_t(1, dtype=I32), kv8=_t(2, 12, 4, dtype=F32), beam=beam)
    with pytest.raises(ValueError, match="beam"):       # rows != B * K
        eng.llama_layer_cached(_t(6, D), *args[1:], t_dev=_t(1, dtype=I32), beam=beam)


class _FakeGraph:
    log = None

    def replay(self):
        _FakeGraph.log.append("replay")


class _FakeCapture:
    def __init__(self, g):
        pass

    def __enter__(self):
        _FakeGraph.log.append("capture{")

    def __exit__(self, *exc):
        _FakeGraph.log.append("}")


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "loop"])
@pytest.mark.parametrize("N", [1, 2, 12])
def test_beam_loop_emits_once_from_the_prefill_then_runs_one_fixed_step_per_token(monkeypatch, graph, N):
    """the decode loop on the CPU with recorders in place of the launches: token 0 from the prefill's B rows (K_in = 1),
    then per token embedding -> layers (engine.Beam on the emit's own table) -> logits -> emit (K_in = K); on the graph
    path one eager step, one captured step, then replays only -- the host launches nothing per token"""
    B, K, S0, V, D = 2, 3, 5, 40, 16
    log = _FakeGraph.log = []
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", _FakeCapture)
    seen = {}

    def emb(table, ids):
        log.append(("embedding_fwd", tuple(ids.shape)))
        seen["tok"] = ids
        return torch.zeros(ids.numel(), D)

    def emit(logits, V_, K_in, pad, eos, lp, early, bs, state):
        log.append(("beam_emit", tuple(logits.shape), K_in, pad, eos, lp, early))
        seen["bs"] = bs
        state[0] += 1
        state[1] += 1

    def run(x, Sn, t0, pos=None, t_dev=None, beam=None):
        log.append(("run", tuple(x.shape), Sn, beam.K, beam.S0))
        assert beam.ind is seen["bs"].ind and t_dev is pos and int(t_dev[0]) == S0 + len([e for e in log if e[0] == "run"]) - 1
        return x

    monkeypatch.setattr(ops, "embedding_fwd", emb)
    monkeypatch.setattr(ops, "beam_emit", emit)

    class Head:
        weight = torch.zeros(V, D)

    class Fake:
        lm_head = Head()
    bs, state = Mo.LlamaForCausalLM._generate_beam.__wrapped__(
        Fake(), run, lambda h: torch.zeros(h.shape[0], V), torch.zeros(B, D), None, B, K, S0, N, 7, 0, "cpu", 0.5, True, graph)
    step = [("embedding_fwd", (B * K,)), ("run", (B * K, D), 1, K, S0), ("beam_emit", (B * K, V), K, 0, 7, 0.5, True)]
    first = [("beam_emit", (B, V), 1, 0, 7, 0.5, True)]
    if not graph or N <= 2:
        assert log == first + step * (N - 1)
    else:
        assert log == first + step + ["capture{"] + step + ["}"] + ["replay"] * (N - 2)
    assert seen.get("tok", bs.tok) is bs.tok and tuple(bs.hist.shape) == (N, B, K, 2) and tuple(bs.ind.shape) == (B * K, N)
    assert tuple(bs.pool_info.shape) == (B, K + 1, 4) and bs.ind.dtype == torch.int32


def test_generate_keeps_the_greedy_path_for_one_beam_and_routes_the_rest(monkeypatch):
    """with one beam not one launch or host read differs from the plain greedy call, whatever the other beam arguments
    say; with more, every selection is ops.beam_emit and every step of the cached loops carries engine.Beam on the
    emit's own table (the loop test above), on the graph path, on the loop and without a cache.  All of it is read off
    generate()'s own launch log (tests/test_generate_trace_cpu.py), not off its source"""
    import test_generate_trace_cpu as T
    beams = dict(T.BEAMS)
    for more in ({}, dict(decode_graph=False), dict(use_cache=False)):
        with monkeypatch.context() as mp:
            plain = T.run_trace_case(dict(N=12, finish=3, kw=more), mp)
        with monkeypatch.context() as mp:
            one = T.run_trace_case(dict(N=12, finish=3, kw={**beams, "num_beams": 1, **more}), mp)
        assert one == plain
        with monkeypatch.context() as mp:
            log = T.run_trace_case(dict(N=12, finish=3, kw={**beams, **more}), mp)["log"]
        names = [e if isinstance(e, str) else e[0] for e in log]
        assert "beam_emit" in names and not {"decode_emit", "argmax_rows", "sample_rows"} & set(names)
        steps = [e for e in log if e[0] == "llama_layer_cached" and e[3] == 1]         # (Sn = 1: behind the prefill)
        assert all(e[-2][0] == "Beam" and e[-2][2:] == [beams["num_beams"], T.S0] for e in steps)
        assert bool(steps) == more.get("use_cache", True)


class _Flags:
    """done flags that turn true once `after` replays have run; every host look at them is logged"""

    def __init__(self, log, after):
        self.log, self.after = log, after

    def all(self):
        self.log.append("read")
        return self.log.count("replay") > self.after


@pytest.mark.parametrize("r", [0, 7, 8])
def test_decode_steps_captures_one_graph_and_reads_the_flags_after_every_eighth_replay(monkeypatch, r):
    """the one loop driver under the three decode loops: one eager step, ONE captured step, then replays only, and a done
    flag that turns true at replay r stops the loop after replay 8 * (r // 8) + 7 and not earlier"""
    log = _FakeGraph.log = []
    made = []
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: made.append(_FakeGraph()) or made[-1])
    monkeypatch.setattr(torch.cuda, "graph", _FakeCapture)
    ran = Mo._decode_steps(lambda: log.append("step"), _Flags(log, r), 40, True)
    last = 8 * (r // 8) + 7
    want = ["read", "step", "read", "capture{", "step", "}"]
    for i in range(last + 1):
        want += ["replay"] + (["read"] if (i & 7) == 7 else [])
    assert log == want and ran == 1 + last + 1 and len(made) == 1
    # the steps end with n_steps where no flag turns true, without a last look
    log.clear()
    assert Mo._decode_steps(lambda: log.append("step"), _Flags(log, 99), 12, True) == 12
    assert log.count("replay") == 11 and log[-1] == "replay" and log.count("read") == 3
    # without a graph: a look before every step, none behind the last
    log.clear()
    assert Mo._decode_steps(lambda: log.append("step"), _Flags(log, -1 if r else 99), 3, False) == (0 if r else 3)
    assert log == (["read"] if r else ["read", "step"] * 3) and len(made) == 2


# ------------------------------------------------------------- 6. the input generator of the GPU selection test --
def _quantiser(dtype):
    td = getattr(torch, dtype)
    return lambda x: torch.from_numpy(x).to(td).double().numpy()


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_selection_inputs_keep_the_best_candidates_apart(case):
    """for every case and seed the GPU test uses: the float64 candidates of the QUANTISED logits, best 2K + 1, have
    consecutive gaps above 1e-4 -- far above the fp32 error of a candidate, so the selection is decided"""
    gap = R.top_gaps(case, _quantiser(case[5]))
    assert gap > R.MIN_GAP, gap
    x, scores = R.beam_inputs(case)
    B, K, K_in, V, ld = case[:5]
    assert x.shape == (B * K_in, ld) and (x[:, V:] == 1e4).all() and scores.shape == (B, K)
    x2, s2 = R.beam_inputs(case)
    assert np.array_equal(x, x2) and np.array_equal(scores, s2)         # a pure function of the case


# ------------------------------------------------------------------------- 7. cross-check against transformers --
def test_restatement_matches_transformers_beam_search_on_a_table_lookup_lm():
    """The installed transformers (5.x) has no BeamSearchScorer any more, but its generate(num_beams=) can be driven on
    the CPU by a toy LM whose logits are a table lookup of (position, last token).  With early_stopping=False it returns
    the restatement's hypotheses and scores.  early_stopping=True is NOT compared: there 5.x also merges the running beams
    of a sample that has already finished K hypotheses when the length limit is reached, and lets a finished sample's
    pool go on changing while other samples of the batch run; the classic scorer (and the rule here) freezes a done
    sample.  One sample per call and a position-dependent table keep exact score ties (equal multisets of transitions)
    out of the comparison."""
    from transformers import GenerationMixin, PretrainedConfig, PreTrainedModel
    from transformers.modeling_outputs import CausalLMOutputWithPast

    class Cfg(PretrainedConfig):
        model_type = "toy_table"

        def __init__(self, vocab_size=12, **kw):
            super().__init__(**kw)
            self.vocab_size = vocab_size

    class Toy(PreTrainedModel, GenerationMixin):
        config_class = Cfg

        def __init__(self, cfg, table):
            super().__init__(cfg)
            self.table = torch.nn.Parameter(table, requires_grad=False)

        def forward(self, input_ids=None, attention_mask=None, **kw):
            return CausalLMOutputWithPast(logits=self.table[input_ids.shape[1] - 1][input_ids])

        def prepare_inputs_for_generation(self, input_ids, **kw):
            return {"input_ids": input_ids}

    V, N, K, pad, eos = 12, 6, 3, 9, 7
    for lp in (1.0, 0.0, 2.0):
        for seed in range(8):
            table = torch.randn(N + 1, V, V, generator=torch.Generator().manual_seed(seed)) * 2
            first = seed % V
            out = Toy(Cfg(vocab_size=V), table).eval().generate(
                torch.tensor([[first]]), num_beams=K, max_new_tokens=N, do_sample=False, eos_token_id=eos, pad_token_id=pad,
                num_return_sequences=K, length_penalty=lp, early_stopping=False, output_scores=True,
                return_dict_in_generate=True, use_cache=False)
            ref = R.BeamRef(1, K, N, pad, eos, lp, False)
            t64 = table.double().numpy()
            for t in range(N):
                if all(ref.done):
                    break
                ref.step(t64[0][[first]][:, None, :] if t == 0 else t64[t][ref.tok])
            rows, scores = ref.finalize(K)
            got = out.sequences[:, 1:].tolist()
            width = max(len(got[0]), max(len(r) for r in rows))
            assert [r + [pad] * (width - len(r)) for r in got] == [r + [pad] * (width - len(r)) for r in rows], (lp, seed)
            assert np.allclose(out.sequences_scores.numpy(), scores, rtol=0, atol=1e-5), (lp, seed)
