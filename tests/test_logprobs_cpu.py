"""CPU: token log-probabilities -- the rule of include/macaw_hip.h as restated in tests/logprobs_ref.py against torch's
log_softmax / topk and on hand-worked rows, the ABI of the two new entry points, the public arguments and every refusal,
and what generate(return_logprobs=True) launches on the recorders of tests/test_generate_trace_cpu.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import logprobs_ref as R
import test_generate_trace_cpu as T

from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
NEW = {"mk_token_logprobs": 11, "mk_decode_emit_logprobs": 17}
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------ 1. the ABI --
def test_header_declares_the_two_entry_points_states_the_rule_and_keeps_abi_11():
    src = open(HEADER).read()
    for name, arity in NEW.items():
        m = re.search(rf"^int {name}\((.*?)\);", src, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/macaw_hip.h"
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name]) == arity, name
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == 11 == L.ABI_VERSION
    for phrase in ("ties go to the LOWER column", "as they stand in front of the selection", "finished BEFORE this step",
                   "a single rounding", "degenerate row is NaN", "id -1 with log-probability -inf",
                   "a thread's own columns, then the lane tree, then wave order", "zero before the first launch"):
        assert phrase in src, phrase
    from macaw_llm_amd import build
    assert "logprobs.hip" in build.SOURCES
    kernel = open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "logprobs.hip")).read()
    assert "asm" not in kernel                                           # plain HIP only
    assert '"beam.hip"' not in kernel and '"sample.hip"' not in kernel   # the select is this file's own copy


def test_the_library_exports_them_and_bad_arguments_return_codes():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    assert lib.mk_abi_version() == 11
    for name in NEW:                                                     # null pointers: a code, nothing launched
        assert getattr(lib, name)(*[None if t is L._vp else t(0) for t in L.SIGNATURES[name]]) == -1, name
    fake = 4096                                                          # never dereferenced: every call below is refused

    def tl(logits=fake, ld=40, rows=2, V=40, ids=fake, n_top=5, lp=fake, top_ids=fake, top_lp=fake, dtype=L.MK_BF16):
        return lib.mk_token_logprobs(logits, ld, rows, V, ids, n_top, lp, top_ids, top_lp, dtype, None)

    for bad in (dict(logits=None), dict(ids=None), dict(lp=None), dict(top_ids=None), dict(top_lp=None), dict(rows=0),
                dict(rows=-1), dict(V=0), dict(ld=39), dict(n_top=-1)):
        assert tl(**bad) == -1, bad
    for bad in (dict(n_top=21), dict(V=(1 << 23) + 1, ld=(1 << 23) + 1), dict(dtype=L.MK_FP8), dict(dtype=7)):
        assert tl(**bad) == -2, bad

    def el(logits=fake, ld=40, V=40, B=2, pad=0, tok=fake, done=fake, state=fake, fin=fake, n_max=8, n_top=5, lp=fake,
           lp_ld=8, top_ids=fake, top_lp=fake, dtype=L.MK_F16):
        return lib.mk_decode_emit_logprobs(logits, ld, V, B, pad, tok, done, state, fin, n_max, n_top, lp, lp_ld, top_ids,
                                           top_lp, dtype, None)

    for bad in (dict(logits=None), dict(tok=None), dict(done=None), dict(state=None), dict(fin=None), dict(lp=None),
                dict(top_ids=None), dict(top_lp=None), dict(B=0), dict(V=0), dict(ld=39), dict(n_top=-1), dict(n_max=-1),
                dict(lp_ld=7)):
        assert el(**bad) == -1, bad
    for bad in (dict(n_top=21), dict(V=(1 << 23) + 1, ld=(1 << 23) + 1), dict(dtype=L.MK_FP8)):
        assert el(**bad) == -2, bad
    for name, op in (("mk_token_logprobs", ops.token_logprobs), ("mk_decode_emit_logprobs", ops.decode_emit_logprobs)):
        assert name in inspect.getsource(op)


def test_logprob_state_is_the_books_of_the_header():
    s = ops.LogprobState(3, 12, 5, 9, "cpu")
    assert (s.B, s.n_max, s.n_top, s.pad) == (3, 12, 5, 9)
    assert s.lp.dtype == torch.float32 and tuple(s.lp.shape) == (3, 12) and not bool(s.lp.any())
    assert s.top_ids.dtype == torch.long and tuple(s.top_ids.shape) == (3, 12, 5) and bool((s.top_ids == 9).all())
    assert s.top_lp.dtype == torch.float32 and tuple(s.top_lp.shape) == (3, 12, 5) and not bool(s.top_lp.any())
    assert s.fin.dtype == torch.uint8 and tuple(s.fin.shape) == (3,) and not bool(s.fin.any())
    s = ops.LogprobState(2, 4, 0, 9, "cpu")
    assert s.top_ids is None and s.top_lp is None and tuple(s.lp.shape) == (2, 4)
    assert ops.MAX_TOP_LOGPROBS == 20


# --------------------------------------------------------------------------------------- 2. the restatement --
@pytest.mark.parametrize("V,n", [(7, 3), (40, 5), (1025, 20), (32000, 5)])
def test_restatement_is_log_softmax_and_topk_on_tie_free_rows(V, n):
    g = torch.Generator().manual_seed(V)
    x = torch.stack([torch.randperm(V, generator=g).float() * (24.0 / V) - 12.0 for _ in range(3)])   # distinct in fp32
    assert all(len(set(row.tolist())) == V for row in x)                 # tie-free
    ids = torch.randint(0, V, (3,), generator=g)
    lp, ti, tl, lp64, tl64 = R.token_logprobs(x, ids, n)
    want = torch.log_softmax(x.double(), dim=-1)
    tv, tk = torch.topk(want, n, dim=-1)
    assert np.array_equal(ti, tk.numpy())
    assert np.allclose(lp64, want[torch.arange(3), ids].numpy(), rtol=0, atol=1e-12)
    assert np.allclose(tl64, tv.numpy(), rtol=0, atol=1e-12)
    assert np.array_equal(lp, lp64.astype(np.float32)) and np.array_equal(tl, tl64.astype(np.float32))
    assert R.within(lp, lp64) == (True, R.within(lp, lp64)[1]) and R.within(lp, lp64)[1] <= 0.5   # the rounding alone


def test_restatement_follows_the_rule_on_hand_worked_rows():
    ln = np.log
    # ties go to the lower column, a tie group cut by n
    x = [1.0, 3.0, 3.0, 0.0, 3.0, 1.0]
    assert R.top(x, 2).tolist() == [1, 2] and R.top(x, 4).tolist() == [1, 2, 4, 0] and R.top(x, 6).tolist() == [1, 2, 4, 0, 5, 3]
    assert R.top([0.0, -0.0, 0.0], 3).tolist() == [0, 1, 2]              # -0 == +0
    # two equal logits: ln(1/2) each; a -inf column gives -inf and takes no mass
    lp, ti, tl, lp64, _ = R.token_logprobs([[2.0, 2.0, -INF]], [1], 3)
    assert abs(lp64[0] - ln(0.5)) < 1e-15 and ti.tolist() == [[0, 1, 2]]
    assert tl[0, 0] == tl[0, 1] == np.float32(ln(0.5)) and tl[0, 2] == -INF
    # a NaN column gives NaN, takes no mass and is never a top column; V < n: -1 / -inf behind
    lp, ti, tl, _, _ = R.token_logprobs([[0.0, NAN, ln(3.0)], [0.0, NAN, ln(3.0)]], [0, 1], 4)
    assert lp[0] == np.float32(ln(0.25)) and np.isnan(lp[1])
    assert ti.tolist() == [[2, 0, -1, -1]] * 2
    assert tl[0, 0] == np.float32(ln(0.75)) and tl[0, 1] == np.float32(ln(0.25)) and tl[0, 2] == tl[0, 3] == -INF
    # +inf: degenerate, every value NaN, the ids still the largest keys
    lp, ti, tl, _, _ = R.token_logprobs([[1.0, INF, 5.0, -INF]], [2], 3)
    assert np.isnan(lp[0]) and ti.tolist() == [[1, 2, 0]] and np.isnan(tl).all()
    # all -inf: degenerate; the columns in order
    lp, ti, tl, _, _ = R.token_logprobs([[-INF] * 4], [0], 5)
    assert np.isnan(lp[0]) and ti.tolist() == [[0, 1, 2, 3, -1]] and np.isnan(tl[0, :4]).all() and tl[0, 4] == -INF
    # one column: log-probability 0; an id outside [0, V): NaN
    lp, ti, tl, _, _ = R.token_logprobs([[-3.5], [-3.5], [-3.5]], [0, 1, -1], 1)
    assert lp[0] == 0.0 and np.isnan(lp[1]) and np.isnan(lp[2]) and ti.tolist() == [[0]] * 3 and tl[0, 0] == 0.0
    # the bound: equal patterns are required, the ratio is measured against 2e-6 + 2^-23 |ref|
    assert R.within([-1.0, -INF, NAN], [-1.0, -INF, NAN]) == (True, 0.0)
    assert not R.within([-1.0, -INF], [-1.0, NAN])[0] and not R.within([-1.0, 0.0], [-1.0, -INF])[0]
    ok, ratio = R.within([-10.0 + 1e-6], [-10.0])
    assert ok and 0.3 < ratio < 0.4
    assert not R.within([-10.0 + 4e-6], [-10.0])[0]


# ------------------------------------------------------------------------------ 3. public arguments, refusals --
def test_generate_and_set_logprobs_carry_the_new_arguments():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    for k, v in dict(return_logprobs=False, top_logprobs=0).items():
        assert p[k].default == v and type(p[k].default) is type(v), k
    p = inspect.signature(Mo.MM_LLMs.set_logprobs).parameters
    assert {k: p[k].default for k in p} == dict(return_logprobs=False, top_logprobs=0)
    assert Mo.GenerateLogprobs._fields == ("ids", "logprobs", "top_ids", "top_logprobs")
    off = dict(return_logprobs=False, top_logprobs=0)
    assert Mo.LOGPROBS[0] == off
    try:
        Mo.MM_LLMs.set_logprobs(True, top_logprobs=5)
        assert Mo.LOGPROBS[0] == dict(return_logprobs=True, top_logprobs=5)
        for bad in (21, -1, 2.0, "4", True, None):
            with pytest.raises(ValueError, match="top_logprobs"):
                Mo.MM_LLMs.set_logprobs(True, bad)
        with pytest.raises(ValueError, match="top_logprobs=3 without return_logprobs=True"):
            Mo.MM_LLMs.set_logprobs(False, 3)
        assert Mo.LOGPROBS[0] == dict(return_logprobs=True, top_logprobs=5)      # a refused call changes nothing
        Mo.MM_LLMs.set_logprobs(True)
        assert Mo.LOGPROBS[0] == dict(return_logprobs=True, top_logprobs=0)
    finally:
        Mo.MM_LLMs.set_logprobs()
    assert Mo.LOGPROBS[0] == off
    fwd = inspect.getsource(Mo.MM_LLMs.forward)
    assert 'LOGPROBS[0] if LOGPROBS[0]["return_logprobs"] else {}' in fwd     # passed through only when it is on
    doc = Mo.LlamaForCausalLM.generate.__doc__
    for phrase in ("as they stand in front of the selection", "compute_transition_scores", "unwarped distribution"):
        assert phrase in " ".join(doc.split()), phrase


def test_set_logprobs_reaches_generate_through_forward_only_when_it_is_on():
    seen = []

    class LLM:
        _lora = None

        def generate(self, **kw):
            seen.append(kw)
            return "ids"

    class Fake:
        llm = LLM()

        def _param_dtype(self):
            return torch.bfloat16

        def prepare_inputs_for_generation(self, inputs):
            return "emb", None, None
    try:
        assert Mo.MM_LLMs.forward(Fake(), {"inference": True}) == "ids"
        assert "return_logprobs" not in seen[-1] and "top_logprobs" not in seen[-1]
        Mo.MM_LLMs.set_logprobs(True, 5)
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert seen[-1]["return_logprobs"] is True and seen[-1]["top_logprobs"] == 5
    finally:
        Mo.MM_LLMs.set_logprobs()


class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates what it can before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(**kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(1, 2, 4, dtype=torch.bfloat16), **kw)


def test_every_refusal_raises_through_generate_and_names_its_condition():
    for bad in (21, -1, 2.0, "4", True, False, None):
        with pytest.raises(ValueError, match=r"generate: top_logprobs must be an integer in \[0, 20\]"):
            _generate(return_logprobs=True, top_logprobs=bad)
    with pytest.raises(ValueError, match="top_logprobs=5 without return_logprobs=True"):
        _generate(top_logprobs=5)
    with pytest.raises(ValueError, match=r"return_logprobs=True.*num_beams=2.*not built.*return_beam_scores"):
        _generate(return_logprobs=True, num_beams=2)
    with pytest.raises(ValueError, match=r"return_logprobs=True.*prompt_lookup_num_tokens=4.*not built"):
        _generate(return_logprobs=True, prompt_lookup_num_tokens=4)
    # the existing refusals come first, with their text
    with pytest.raises(ValueError, match="num_beams must be"):
        _generate(return_logprobs=True, top_logprobs=99, num_beams=0)
    for kw in (dict(), dict(return_logprobs=True), dict(return_logprobs=True, top_logprobs=20),
               dict(return_logprobs=True, do_sample=True, seed=1), dict(return_logprobs=True, repetition_penalty=1.3),
               dict(return_logprobs=True, kv_cache="fp8"), dict(return_logprobs=True, use_cache=False),
               dict(return_logprobs=True, num_beams=1, prompt_lookup_num_tokens=0)):
        with pytest.raises(_PastTheChecks):
            _generate(**kw)


# ----------------------------------------------------------------------------------------- 4. the launch trace --
N_TOP = 3


def _recorders(tr, mp):
    """recorders for the two new ops next to those of tests/test_generate_trace_cpu.py.  The fake step op keeps the
    kernel's books: the column is state[1] - 1, the latch follows done"""
    def rec(name, effect):
        sig = inspect.signature(getattr(ops, name))

        def f(*args, **kw):
            a = sig.bind(*args, **kw)
            a.apply_defaults()
            a = dict(a.arguments)
            tr.quiet += 1
            try:
                # (the books, and the fresh ids of a selection: naming them would renumber the buffers behind them)
                tr.log.append([name] + [tr.item(v) for k, v in a.items() if k not in ("ls", "ids")])
                return effect(a)
            finally:
                tr.quiet -= 1
        return f

    def emit_lp(a):
        ls, col = a["ls"], int(a["state"][1]) - 1
        for b in range(ls.B):
            if not bool(ls.fin[b]):
                ls.lp[b, col] = -(1.0 + col + 0.25 * b)
                if ls.n_top:
                    ls.top_ids[b, col] = torch.arange(ls.n_top)
                    ls.top_lp[b, col] = -(1.0 + col + 0.25 * b) - torch.arange(ls.n_top)
            ls.fin[b] = int(a["done"][b])

    def tok_lp(a):
        rows, n = a["logits"].shape[0], a["top_n"]
        assert a["ids"].dtype == torch.long and tuple(a["ids"].shape) == (rows,)
        assert a["ids"].tolist() == [tr.script.tok(tr.col - 1, b) for b in range(rows)]      # the selection's own ids
        col = tr.col - 1                                               # the recorders' select has just counted the column
        lp = -(1.0 + col + 0.25 * torch.arange(rows))
        if not n:
            return lp, None, None
        return lp, torch.arange(n).repeat(rows, 1), lp[:, None] - torch.arange(n)

    mp.setattr(ops, "decode_emit_logprobs", rec("decode_emit_logprobs", tr._state(emit_lp)))
    mp.setattr(ops, "token_logprobs", rec("token_logprobs", tok_lp))


def _call(mp, spec, lp_kw=None):
    """T.call with the two recorders added -> (log, result)"""
    real = T.GenTrace

    def make(mp_, lm, script):
        tr = real(mp_, lm, script)
        _recorders(tr, mp_)
        return tr
    mp.setattr(T, "GenTrace", make)
    if lp_kw and not lp_kw.get("top_logprobs"):          # T.call lists tensors: leave the two Nones out of the result
        mp.setattr(Mo, "GenerateLogprobs", lambda ids, lp, ti, tl: (ids, lp))
    spec = dict(spec, kw=dict(spec.get("kw", {}), **(lp_kw or {})))
    tr, res = T.call(mp, spec)
    return T._plain(tr.log), res


LP = dict(return_logprobs=True, top_logprobs=N_TOP)
GRAPH_CASES = {"greedy": {}, "sample": dict(kw=T.SAMPLE), "proc": dict(kw=T.PROC, inputs="both"), "left": dict(mask="left"),
               "kv8": dict(kw=dict(kv_cache="fp8")), "w8": dict(kw=dict(decode_weights="fp8"))}


@pytest.mark.parametrize("case", list(GRAPH_CASES))
@pytest.mark.parametrize("N,finish", [(12, 3), (12, None), (3, None)])
def test_graph_loop_holds_one_logprob_launch_behind_every_emit_and_reads_nothing_more(monkeypatch, case, N, finish):
    spec = dict(GRAPH_CASES[case], N=N, finish=finish)
    with monkeypatch.context() as mp:
        plain, res0 = _call(mp, spec)
    with monkeypatch.context() as mp:
        got, res = _call(mp, spec, LP)
    emits = ("decode_emit", "decode_emit_sample")
    name = lambda e: e if isinstance(e, str) else e[0]       # noqa: E731
    # the same launches, host reads and graph events with the new launch taken out
    assert [e for e in got if name(e) != "decode_emit_logprobs"] == plain
    assert not any(name(e) in ("decode_emit_logprobs", "token_logprobs") for e in plain)
    # directly behind every emit, token 0's included, on the same logits, tokens, flags and state
    at = [i for i, e in enumerate(got) if name(e) in emits]
    assert at and [i for i, e in enumerate(got) if name(e) == "decode_emit_logprobs"] == [i + 1 for i in at]
    for i in at:
        e, l = got[i], got[i + 1]
        sig = list(inspect.signature(getattr(ops, e[0])).parameters)
        arg = dict(zip(sig, e[1:]))
        buf = lambda s: s.split("=")[0] if isinstance(s, str) else s     # noqa: E731 -- the buffer, not its values
        assert [buf(v) for v in l[1:]] == [buf(arg[k]) for k in ("logits", "V", "tok", "done", "state")]
    # the captured step: exactly one, behind its emit
    lo, hi = got.index("capture{"), got.index("}")
    inside = [name(e) for e in got[lo + 1:hi]]
    assert inside.count("decode_emit_logprobs") == 1 and inside[-2] in emits and inside[-1] == "decode_emit_logprobs"
    assert "token_logprobs" not in [name(e) for e in got]
    # the result: the plain call's ids, and books trimmed to the same columns; zeros / pad behind a sample's end
    (ids,), (ids2, lp, ti, tl) = res0, res
    assert ids2 == ids
    B, W = ids[0]
    assert lp[0] == [B, W] and lp[1] == "float32" and ti[0] == tl[0] == [B, W, N_TOP] and ti[1] == "int64"
    for b in range(B):
        end = ids[2][b].index(T.EOS) + 1 if T.EOS in ids[2][b] else W
        assert lp[2][b][:end] == [-(1.0 + c + 0.25 * b) for c in range(end)]
        assert lp[2][b][end:] == [0.0] * (W - end)
        assert ti[2][b][:end] == [list(range(N_TOP))] * end and ti[2][b][end:] == [[T.PAD] * N_TOP] * (W - end)
        assert tl[2][b][end:] == [[0.0] * N_TOP] * (W - end)


EAGER_CASES = {"nograph": dict(kw=dict(decode_graph=False)), "fp32": dict(dtype="fp32"), "nocache": dict(kw=dict(use_cache=False)),
               "left-nograph": dict(kw=dict(decode_graph=False), mask="left"), "left-nocache-fp32": dict(kw=dict(use_cache=False), mask="left", dtype="fp32"),
               "sample+proc-nocache": dict(kw=dict(T.SAMPLE, **T.PROC, use_cache=False)), "small": dict(N=2)}


@pytest.mark.parametrize("case", list(EAGER_CASES))
@pytest.mark.parametrize("n_top", [0, N_TOP])
def test_eager_loops_call_token_logprobs_once_per_token_behind_the_selection(monkeypatch, case, n_top):
    spec = dict(dict(N=6, finish=3), **EAGER_CASES[case])
    with monkeypatch.context() as mp:
        plain, res0 = _call(mp, spec)
    with monkeypatch.context() as mp:
        got, res = _call(mp, spec, dict(return_logprobs=True, top_logprobs=n_top))
    name = lambda e: e if isinstance(e, str) else e[0]       # noqa: E731
    assert [e for e in got if name(e) != "token_logprobs"] == plain      # no host read more, no launch moved
    sel = [i for i, e in enumerate(got) if name(e) in ("argmax_rows", "sample_rows")]
    assert sel and [i for i, e in enumerate(got) if name(e) == "token_logprobs"] == [i + 1 for i in sel]
    for i in sel:                                                        # the logits the selection read, V, its ids
        assert got[i + 1][1] == got[i][1] and got[i + 1][2] == T.V and got[i + 1][3] == n_top
    assert "decode_emit_logprobs" not in [name(e) for e in got]
    (ids,) = res0
    if n_top == 0:                                                       # (the two Nones: the test below)
        assert res[0] == ids and res[1][0] == ids[0] and res[1][1] == "float32"
        return
    ids2, lp, ti, tl = res
    assert ids2 == ids and len(sel) == ids[0][1]
    B, W = ids[0]
    assert lp[0] == [B, W] and ti[0] == tl[0] == [B, W, n_top]
    for b in range(B):
        end = ids[2][b].index(T.EOS) + 1 if T.EOS in ids[2][b] else W
        assert lp[2][b][:end] == [-(1.0 + c + 0.25 * b) for c in range(end)] and lp[2][b][end:] == [0.0] * (W - end)
        assert ti[2][b][end:] == [[T.PAD] * n_top] * (W - end) and tl[2][b][end:] == [[0.0] * n_top] * (W - end)


def test_top_logprobs_zero_returns_none_for_the_top_matrices(monkeypatch):
    with monkeypatch.context() as mp:
        lm = T.make_model()
        tr = T.GenTrace(mp, lm, T.Script(3, 2))
        _recorders(tr, mp)
        for kw in (dict(), dict(decode_graph=False), dict(use_cache=False)):
            tr.col = 0
            out = lm.generate(inputs_embeds=torch.zeros((2, T.S0, T.D), dtype=torch.bfloat16), max_new_tokens=6,
                              eos_token_id=T.EOS, pad_token_id=T.PAD, return_logprobs=True, **kw)
            assert isinstance(out, Mo.GenerateLogprobs) and out.top_ids is None and out.top_logprobs is None
            assert out.logprobs.dtype == torch.float32 and out.logprobs.shape == out.ids.shape


def test_the_defaults_allocate_and_launch_nothing(monkeypatch):
    """with (False, 0) generate() must not reach the new code at all: the state class and both ops raise"""
    def boom(*a, **k):
        raise AssertionError("reached with the defaults")
    with monkeypatch.context() as mp:
        lm = T.make_model()
        T.GenTrace(mp, lm, T.Script(3, 2))
        for n in ("LogprobState", "decode_emit_logprobs", "token_logprobs"):
            mp.setattr(ops, n, boom)
        mp.setattr(Mo, "_logprobs_check", boom)
        for kw in (dict(), dict(decode_graph=False), dict(use_cache=False)):
            out = lm.generate(inputs_embeds=torch.zeros((2, T.S0, T.D), dtype=torch.bfloat16), max_new_tokens=6,
                              eos_token_id=T.EOS, pad_token_id=T.PAD, **kw)
            assert torch.is_tensor(out)
