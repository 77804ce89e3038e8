"""CPU: stop_sequences and bad_words_ids of generate() -- the rules of include/macaw_hip.h as restated in tests/stop_ref.py:
the ban against the installed transformers' NoBadWordsLogitsProcessor (fp32, bit for bit wherever every sequence has
L >= n) and both rules on hand-worked cases, the header and the ctypes prototypes, the exported symbols and their
error codes, the public arguments, MM_LLMs.set_stopping, every refusal, and the place of the two launches in every
decode loop on the recorders of tests/test_generate_trace_cpu.py."""
import inspect
import os
import re

import pytest
import torch

import stop_ref as R
import test_generate_trace_cpu as T
from test_logprobs_cpu import _recorders as _logprob_recorders

from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
NEW = {"mk_seq_ban": 18, "mk_stop_match": 11}
INF = float("inf")


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------ 1. the ban rule --
def _hf(logits, history, seqs, eos=None):
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor
    return NoBadWordsLogitsProcessor([list(q) for q in seqs], eos)(torch.tensor([history], dtype=torch.long),
                                                                   logits[None].clone())[0]


def test_ban_restatement_is_the_installed_no_bad_words_processor_bit_for_bit_where_the_history_is_long_enough():
    """3000 random cases in fp32 with L >= n for every sequence.  The logits hold finite values, +0 and -inf: HF ADDS its
    bias, which makes a +inf or NaN column NaN and a -0 column +0 (x + 0.0), where the rule here SETS the banned columns
    and leaves every other bit alone -- both written down in the header"""
    V = 23
    g = torch.Generator().manual_seed(11)
    fired = 0
    for case in range(3000):
        n_seq = int(torch.randint(1, 6, (1,), generator=g))
        lens = torch.randint(1, 5, (n_seq,), generator=g).tolist()
        L_ = int(torch.randint(max(lens), max(lens) + 6, (1,), generator=g))
        h = torch.randint(0, 4, (L_,), generator=g).tolist()             # four values: tails match often
        seqs = [torch.randint(0, 4, (n - 1,), generator=g).tolist() + [int(torch.randint(0, V, (1,), generator=g))]
                for n in lens]
        if case % 3 == 0:                                                # a sequence cut from the history: a certain match
            n = lens[0]
            seqs[0] = h[L_ - (n - 1):] + [seqs[0][-1]] if n > 1 else seqs[0]
        x = torch.randn(V, generator=g) * 4
        x[torch.randint(0, V, (3,), generator=g)] = 0.0
        x[torch.randint(0, V, (3,), generator=g)] = -INF
        eos = [None, 5, seqs[0][-1]][case % 3]
        want = _hf(x, h, seqs, eos)
        kept = Mo._stopping_check("generate", None, seqs, eos)[1] or []   # what generate() hands the kernel: [eos] dropped
        assert kept == R.drop_eos(seqs, eos)
        got = R.ban_row(x, h, kept)
        assert got.dtype == torch.float32 and torch.equal(_bits(got), _bits(want)), (case, h, seqs, eos)
        fired += not torch.equal(_bits(got), _bits(x))
    assert fired > 1500


def test_ban_restatement_by_hand():
    x = torch.tensor([2.0, -2.0, 0.0, -0.0, -INF, 3.0, INF, float("nan")])
    same = lambda a, b: torch.equal(_bits(a), _bits(b))     # noqa: E731

    def banned(h, seqs):
        got = R.ban_row(x, h, seqs)
        cols = [c for c in range(8) if not same(got[c:c + 1], x[c:c + 1])]
        assert all(_bits(got[c:c + 1]).item() == _bits(torch.tensor([-INF])).item() for c in cols)
        return cols
    # L == n - 1, the difference from HF: the history IS the prefix, and the last id is banned (HF skips the sequence)
    assert banned([5, 1], [[5, 1, 0]]) == [0]
    y = torch.tensor([2.0, -2.0, 0.0, 1.0, -INF, 3.0])
    assert same(_hf(y, [5, 1], [[5, 1, 0]]), y) and R.ban_row(y, [5, 1], [[5, 1, 0]])[0] == -INF
    assert _hf(y, [3, 5, 1], [[5, 1, 0]])[0] == -INF                     # one id more and HF bans it too
    # L == n - 2 and L == 0: the prefix cannot lie in the history
    assert banned([1], [[5, 1, 0]]) == [] and banned([], [[5, 1, 0]]) == [] and banned([], [[1, 0]]) == []
    # n == 1 is banned whatever the history, the empty one included; the column is SET: +inf and NaN become -inf
    assert banned([], [[0]]) == [0] and banned([3, 3], [[6], [7]]) == [6, 7]
    # a -inf column stays -inf (no bit changes); -0 keeps its sign next to a ban
    assert banned([5], [[5, 4]]) == [] and R.ban_row(x, [5], [[5, 4]])[4] == -INF
    # [eos] is dropped, a longer sequence that ends in eos is not; generate()'s own check does the same
    assert R.drop_eos([[2], [1, 2], [3]], 2) == [[1, 2], [3]] and R.drop_eos([[2]], None) == [[2]]
    assert Mo._stopping_check("generate", None, [[2], [1, 2], [3]], 2)[1] == [[1, 2], [3]]
    # duplicates, and two sequences naming one column
    assert banned([5, 1], [[1, 0], [1, 0], [5, 1, 0], [2]]) == [0, 2]
    # only the tail counts: the prefix earlier in the history bans nothing
    assert banned([5, 1, 3], [[5, 1, 0]]) == [] and banned([5, 1, 3, 5, 1], [[5, 1, 0]]) == [0]
    # a tail that straddles prompt and generated tokens (ban() joins them); an id outside [0, V) names no column but is compared
    got = R.ban(torch.stack([x, x]), [[9, 5], [9, 4]], [[1], [1]], [[5, 1, 0], [1, 99], [99, 1, 2]])
    assert got[0, 0] == -INF and same(got[0, 1:], x[1:]) and same(got[1], x)
    got = R.ban(x[None], None, [[99, 1]], [[99, 1, 2]])
    assert got[0, 2] == -INF
    # 16-bit rows keep their type
    for dt in (torch.bfloat16, torch.float16):
        got = R.ban_row(x.to(dt), [5], [[5, 0]])
        assert got.dtype == dt and got[0] == -INF and same(got[1:], x.to(dt)[1:])


# ----------------------------------------------------------------------------------------- 2. the stop rule --
def _table(seqs):
    """the sequences as the kernels read them: through ops.SeqTable's ids and offsets and back"""
    t = ops.SeqTable(seqs, "cpu")
    return [t.ids[t.off[s]:t.off[s + 1]].tolist() for s in range(t.n)]


def test_stop_restatement_by_hand():
    def stops_row(g, seqs):
        return R.stops_row(g, _table(seqs))

    def stop_match(out, n, seqs, done):
        return R.stop_match(out, n, _table(seqs), done)
    assert not stops_row([7], [[5, 7]])                                 # n < m: never reaches into a prompt
    assert stops_row([7], [[7]]) and stops_row([5, 7], [[5, 7]])        # a match at column 0; the whole row
    assert not stops_row([5, 7, 3], [[5, 7]])                           # occurs earlier, not at the tail
    assert stops_row([5, 7, 3, 5, 7], [[9], [5, 7]]) and not stops_row([], [[1]])
    # a finished row is not examined and stays finished; the count decides what the row holds
    out = [[5, 7, 0, 0], [5, 7, 0, 0], [1, 2, 3, 4]]
    assert stop_match(out, 2, [[5, 7]], [False, True, False]) == [True, True, False]
    assert stop_match(out, 3, [[5, 7]], [False, False, False]) == [False, False, False]
    assert stop_match(out, 4, [[3, 4], [9]], [False, True, False]) == [False, True, True]
    # the finish column and the cut: eos or a stop sequence, whichever comes first; the width is the last row's end
    assert R.finish_column([4, 5, 7, 5, 7], [[5, 7]], 2) == 2 and R.finish_column([4, 2, 5, 7], [[5, 7]], 2) == 1
    assert R.finish_column([4, 5, 6], [[5, 7]], 2) is None
    ids = torch.tensor([[4, 5, 7, 8, 9], [2, 5, 7, 1, 1], [5, 7, 3, 3, 3]])
    assert R.cut(ids, [[5, 7]], 2, 0).tolist() == [[4, 5, 7], [2, 0, 0], [5, 7, 0]]
    assert R.cut(ids, [[5, 7, 8]], 2, 0).tolist() == [[4, 5, 7, 8, 0], [2, 0, 0, 0, 0], [5, 7, 3, 3, 3]]


# ------------------------------------------------------------------------------------------------ 3. the ABI --
def test_header_declares_both_entry_points_with_the_prototypes_arity_and_states_the_rules():
    src = open(HEADER).read()
    for name, arity in NEW.items():
        m = re.search(rf"^int {name}\((.*?)\);", src, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/macaw_hip.h"
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name]) == arity, name
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION
    flat = re.sub(r"\s*\n \*\s*", " ", src)                              # the comment's text without its line breaks
    for phrase in ("h[L - m + 1 .. L) == q[0 .. m - 1)", "L >= m - 1 suffices", "skips a multi-token sequence while L < m",
                   "SET to -inf whatever it held", "BEHIND mk_logits_process", "gives HF's chain exactly",
                   "out[b][n - m .. n) == q", "never reaches into the prompt", "in front of mk_decode_emit_logprobs",
                   "A row whose done byte is set is not examined", "no other byte is written", "names no column",
                   "n_seq > 65536"):
        assert phrase in flat, phrase
    from macaw_llm_amd import build
    assert "stop.hip" in build.SOURCES
    kernel = open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "stop.hip")).read()
    assert "asm" not in kernel and "atomic" not in kernel               # plain loads and stores only


def test_the_library_exports_them_and_bad_arguments_return_codes():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    for name in NEW:                                                    # null pointers: a code, nothing launched
        assert getattr(lib, name)(*[None if t is L._vp else t(0) for t in L.SIGNATURES[name]]) == -1, name
    fake = 4096                                                         # never dereferenced: every call below is refused

    def ban(logits=fake, ld=64, V=64, B=1, prompt=None, p_ld=0, P=0, p_len=None, out=fake, out_ld=8, n_max=8, n_dev=None,
            n_add=0, ids=fake, off=fake, n_seq=1, dtype=L.MK_F32):
        return lib.mk_seq_ban(logits, ld, V, B, prompt, p_ld, P, p_len, out, out_ld, n_max, n_dev, n_add, ids, off, n_seq,
                              dtype, None)

    for bad in (dict(logits=None), dict(out=None), dict(ids=None), dict(off=None), dict(prompt=fake, P=4, p_ld=4),
                dict(prompt=fake, p_len=fake, P=4, p_ld=3), dict(prompt=fake, p_len=fake, P=-1), dict(V=0), dict(B=0),
                dict(B=-1), dict(n_seq=0), dict(n_seq=-1), dict(ld=63), dict(n_max=-1), dict(out_ld=7)):
        assert ban(**bad) == -1, bad
    for bad in (dict(n_seq=(1 << 16) + 1), dict(dtype=L.MK_FP8), dict(dtype=7)):
        assert ban(**bad) == -2, bad

    def stop(out=fake, out_ld=8, n_max=8, B=1, n_dev=None, n_add=0, ids=fake, off=fake, n_seq=1, done=fake):
        return lib.mk_stop_match(out, out_ld, n_max, B, n_dev, n_add, ids, off, n_seq, done, None)

    for bad in (dict(out=None), dict(ids=None), dict(off=None), dict(done=None), dict(B=0), dict(B=-1), dict(n_seq=0),
                dict(n_seq=-1), dict(n_max=-1), dict(out_ld=7)):
        assert stop(**bad) == -1, bad
    assert stop(n_seq=(1 << 16) + 1) == -2
    for name, op in (("mk_seq_ban", ops.seq_ban), ("mk_stop_match", ops.stop_match)):
        assert name in inspect.getsource(op)


def test_seq_table_is_the_table_of_the_header():
    t = ops.SeqTable([[5], [7, 8, 9], [5]], "cpu")
    assert t.n == 3 and t.ids.dtype == torch.long and t.ids.tolist() == [5, 7, 8, 9, 5]
    assert t.off.dtype == torch.int32 and t.off.tolist() == [0, 1, 4, 5]
    assert (ops.MAX_SEQS, ops.MAX_SEQ_LEN) == (65536, 64)
    for bad in ([], [[]], [[1] * 65]):
        with pytest.raises(L.MacawHipError, match="SeqTable"):
            ops.SeqTable(bad, "cpu")


# ------------------------------------------------------------------------------ 4. public arguments, refusals --
OFF = dict(stop_sequences=None, bad_words_ids=None)


def test_generate_and_set_stopping_carry_the_new_arguments():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    for k in OFF:
        assert p[k].default is None, k
    p = inspect.signature(Mo.MM_LLMs.set_stopping).parameters
    assert {k: p[k].default for k in p} == OFF
    assert Mo.STOPPING[0] == OFF
    try:
        Mo.MM_LLMs.set_stopping(stop_sequences=[[5, 7]], bad_words_ids=[[3], [4, 4]])
        assert Mo.STOPPING[0] == dict(stop_sequences=[[5, 7]], bad_words_ids=[[3], [4, 4]])
        with pytest.raises(ValueError, match="set_stopping: bad_words_ids"):
            Mo.MM_LLMs.set_stopping(bad_words_ids=[[]])
        assert Mo.STOPPING[0]["stop_sequences"] == [[5, 7]]             # a refused call changes nothing
        Mo.MM_LLMs.set_stopping(bad_words_ids=[[9]])
        assert Mo.STOPPING[0] == dict(stop_sequences=None, bad_words_ids=[[9]])
    finally:
        Mo.MM_LLMs.set_stopping()
    assert Mo.STOPPING[0] == OFF
    doc = " ".join(Mo.LlamaForCausalLM.generate.__doc__.split())
    for phrase in ("stop_sequences", "bad_words_ids", "NoBadWordsLogitsProcessor", "never reaches into the prompt",
                   "L >= n - 1"):
        assert phrase in doc, phrase


def test_set_stopping_reaches_generate_through_forward_only_when_it_is_set():
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
        assert "stop_sequences" not in seen[-1] and "bad_words_ids" not in seen[-1]
        Mo.MM_LLMs.set_stopping(stop_sequences=[[5, 7]])
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert seen[-1]["stop_sequences"] == [[5, 7]] and "bad_words_ids" not in seen[-1]
        Mo.MM_LLMs.set_stopping(bad_words_ids=[[1, 2]])
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert seen[-1]["bad_words_ids"] == [[1, 2]] and "stop_sequences" not in seen[-1]
    finally:
        Mo.MM_LLMs.set_stopping()


class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates its arguments before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(**kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(1, 2, 4, dtype=torch.bfloat16), **kw)


def test_every_refusal_names_its_argument_and_the_defaults_raise_nothing():
    for name in OFF:
        for bad in ([], [[]], [[1], []], [1, 2], [(1, 2)], ([1, 2],), "ab", 5, [[1.0]], [[-1]], [["a"]], [[True]],
                    [[1], [2, None]], [[1]] * 65537, [[1] * 65]):
            with pytest.raises(ValueError, match=f"generate: {name}"):
                _generate(**{name: bad})
            with pytest.raises(ValueError, match=f"set_stopping: {name}"):
                Mo.MM_LLMs.set_stopping(**{name: bad})
        with pytest.raises(ValueError, match=f"{name}.*num_beams=2.*not built"):
            _generate(num_beams=2, **{name: [[1, 2]]})
        with pytest.raises(ValueError, match=f"{name}.*prompt_lookup_num_tokens=4.*not built"):
            _generate(prompt_lookup_num_tokens=4, **{name: [[1, 2]]})
        for ok in ([[1]], [[1, 2], [3]], [[1] * 64], [[0]] * 65536):
            with pytest.raises(_PastTheChecks):
                _generate(**{name: ok})
        with pytest.raises(_PastTheChecks):
            _generate(num_beams=1, prompt_lookup_num_tokens=0, **{name: [[1]]})
    assert Mo.STOPPING[0] == OFF
    # the existing refusals come first, with their text
    with pytest.raises(ValueError, match="num_beams must be"):
        _generate(stop_sequences=[], num_beams=0)
    for kw in (dict(), dict(num_beams=4), dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=2)):
        with pytest.raises(_PastTheChecks):
            _generate(**kw)
    # what the check hands on: lists of ints, a banned [eos] dropped, nothing left: off
    assert Mo._stopping_check("generate", [[5, 7]], [[2], [3, 2]], eos=2) == ([[5, 7]], [[3, 2]])
    assert Mo._stopping_check("generate", None, [[2]], eos=2) == (None, None)
    assert Mo._stopping_check("generate", [[2]], [[2]], eos=None) == ([[2]], [[2]])


# ----------------------------------------------------------------------------------------- 5. the launch trace --
STOP = [[3 + (7 * 4 + 3 * 0) % 30, 3 + (7 * 5 + 3 * 0) % 30]]           # the script's columns 4 and 5 of sample 0
BAD = [[9], [4, 5, 6]]


class _Late:
    """a tensor argument of a new launch: its values as they are now, its buffer's number once the call is over --
    numbering it here would renumber the buffers the plain call's launches name behind it"""

    def __init__(self, tr, v):
        self.v, self.vals = v, ""
        if v.dtype in (torch.bool, torch.int32, torch.int64, torch.uint8) and 0 < v.numel() <= 40:
            self.vals = "=" + str([[int(c) for c in r] for r in v.tolist()] if v.dim() == 2 else
                                  [int(c) for c in v.tolist()]).replace(" ", "")

    def resolve(self, tr, fresh):
        v, key = self.v, self.v.untyped_storage()._cdata
        name = f"b{tr.bufs[key]}" if key in tr.bufs else f"n{fresh.setdefault(key, len(fresh))}"
        s = f"{name}{list(v.shape)}{str(v.dtype).replace('torch.', '')}".replace(" ", "")
        if not v.is_contiguous() or v.storage_offset():
            s += f"s{list(v.stride())}o{v.storage_offset()}".replace(" ", "")
        return s + self.vals


def _resolve(tr):
    fresh = {}
    tr.quiet += 1
    for e in tr.log:
        if not isinstance(e, str):
            e[:] = [x.resolve(tr, fresh) if isinstance(x, _Late) else x for x in e]
    tr.quiet -= 1


def _recorders(tr, mp):
    """recorders for the two new ops (and the log-probability ones) next to those of tests/test_generate_trace_cpu.py;
    the fake match is the restatement on the recorded buffers"""
    _logprob_recorders(tr, mp)

    def item(k, v):
        if k == "table":
            return v.ids.tolist()
        if torch.is_tensor(v) and tr.names.get(tr._key(v)) is None:
            return _Late(tr, v)
        return tr.item(v)

    def rec(name, effect):
        sig = inspect.signature(getattr(ops, name))

        def f(*args, **kw):
            a = sig.bind(*args, **kw)
            a.apply_defaults()
            a = dict(a.arguments)
            tr.quiet += 1
            try:
                tr.log.append([name] + [item(k, v) for k, v in a.items()])
                return effect(a)
            finally:
                tr.quiet -= 1
        return f

    def match(a):
        n = (int(a["n_dev"][0]) if a["n_dev"] is not None else 0) + a["n_add"]
        seqs = [a["table"].ids[a["table"].off[s]:a["table"].off[s + 1]].tolist() for s in range(a["table"].n)]
        for b, d in enumerate(R.stop_match(a["out"].tolist(), n, seqs, a["done"].tolist())):
            a["done"][b] = d

    mp.setattr(ops, "seq_ban", rec("seq_ban", lambda a: a["logits"]))
    mp.setattr(ops, "stop_match", rec("stop_match", tr._state(match)))


def _call(mp, spec, more=None):
    real = T.GenTrace

    def make(mp_, lm, script):
        tr = real(mp_, lm, script)
        _recorders(tr, mp_)
        return tr
    mp.setattr(T, "GenTrace", make)
    spec = dict(spec, kw=dict(spec.get("kw", {}), **(more or {})))
    tr, res = T.call(mp, spec)
    _resolve(tr)
    return T._plain(tr.log), res


_name = lambda e: e if isinstance(e, str) else e[0]       # noqa: E731
_buf = lambda s: s.split("=")[0] if isinstance(s, str) else s     # noqa: E731 -- the buffer, not its values
EMITS = ("decode_emit", "decode_emit_sample")
SELECTS = ("argmax_rows", "sample_rows")
GRAPH_CASES = {"greedy": {}, "sample": dict(kw=T.SAMPLE), "proc": dict(kw=T.PROC, inputs="both"), "left": dict(mask="left"),
               "kv8": dict(kw=dict(kv_cache="fp8")), "w8": dict(kw=dict(decode_weights="fp8"))}


@pytest.mark.parametrize("case", list(GRAPH_CASES))
def test_graph_loop_order_is_ban_emit_stop_match_logprobs_inside_one_captured_step(monkeypatch, case):
    spec = dict(GRAPH_CASES[case], N=12, finish=None)
    both = dict(stop_sequences=[[99, 98]], bad_words_ids=BAD, return_logprobs=True, top_logprobs=2)   # a stop that never fires
    with monkeypatch.context() as mp:
        plain, _ = _call(mp, spec)
    with monkeypatch.context() as mp:
        got, _ = _call(mp, spec, both)
    new = ("seq_ban", "stop_match", "decode_emit_logprobs")
    # behind the loop the width is found by matching every column's tail once more: no host read more, no launch moved
    loop_end = max(i for i, e in enumerate(got) if _name(e) == "replay")
    last = max(i for i, e in enumerate(got) if _name(e) == "host")      # the look at the flags behind the loop
    assert got[last] == ["host", "__bool__", [], 0]
    assert [e for i, e in enumerate(got) if _name(e) not in new and i != last] == plain
    assert not any(_name(e) in new for e in plain)
    at = [i for i, e in enumerate(got) if _name(e) in EMITS]
    assert len(at) == 3                                                 # token 0, the eager step, the captured step
    for i in at:
        assert [_name(e) for e in got[i - 1:i + 3]] == ["seq_ban", _name(got[i]), "stop_match", "decode_emit_logprobs"]
        arg = dict(zip(inspect.signature(getattr(ops, got[i][0])).parameters, got[i][1:]))
        ban = dict(zip(inspect.signature(ops.seq_ban).parameters, got[i - 1][1:]))
        stop = dict(zip(inspect.signature(ops.stop_match).parameters, got[i + 1][1:]))
        assert ban["logits"] == arg["logits"] and ban["V"] == T.V and ban["table"] == [9, 4, 5, 6]
        assert _buf(ban["out"]) == _buf(arg["out"]) == _buf(stop["out"]) and stop["table"] == [99, 98]
        assert _buf(stop["done"]) == _buf(arg["done"]) and (ban["n_add"], stop["n_add"]) == (0, 0)
        col = at.index(i)
        # the emit has advanced the counter the match reads (the captured launches do not run: both see column 2)
        assert ban["n_dev"].endswith(f"=[{col}]") and stop["n_dev"].endswith(f"=[{min(col + 1, 2)}]")
        assert _buf(ban["n_dev"]) == _buf(stop["n_dev"])
        if case == "proc":                                              # behind the processors, on their history
            proc = dict(zip(inspect.signature(ops.logits_process).parameters, got[i - 2][1:]))
            assert _name(got[i - 2]) == "logits_process" and proc["logits"] == ban["logits"]
            assert (proc["prompt"], proc["prompt_len"]) == (ban["prompt"], ban["prompt_len"]) and ban["prompt"] is not None
        else:
            assert ban["prompt"] is None and ban["prompt_len"] is None
    lo, hi = got.index("capture{"), got.index("}")
    assert [_name(e) for e in got[lo + 1:hi]][-4:] == ["seq_ban", _name(got[at[2]]), "stop_match", "decode_emit_logprobs"]
    # no sample finished: nothing is matched behind the loop (one look at the flags more, the only one)
    assert [e for e in got[loop_end:] if _name(e) == "stop_match"] == []


@pytest.mark.parametrize("case", ["greedy", "sample", "left"])
def test_graph_loop_stops_at_the_sequence_pads_behind_it_and_returns_the_eager_width(monkeypatch, case):
    """sample 0 emits the stop sequence at columns 4 and 5, sample 1 its eos from column 3 on: the flags the match sets
    feed the pad, the early exit and the trim exactly as eos does"""
    spec = dict(GRAPH_CASES[case], N=12, finish=None)
    script = T.Script(None, 2)
    mixed = type("S", (), dict(tok=lambda self, col, b: T.EOS if b == 1 and col >= 3 else script.tok(col, b)))()
    res = {}
    for path, kw in (("graph", {}), ("nograph", dict(decode_graph=False))):
        with monkeypatch.context() as mp:
            mp.setattr(T, "Script", lambda finish, B: mixed)
            log, res[path] = _call(mp, dict(spec, kw=dict(spec.get("kw", {}), **kw)), dict(stop_sequences=STOP))
        if path == "graph":
            assert len([e for e in log if _name(e) == "replay"]) == 8   # the host looks at the flags after the 8th replay
            # every sample has finished: behind the loop one match per column that ran, the count from the host
            loop_end = max(i for i, e in enumerate(log) if _name(e) == "replay")
            tail = [dict(zip(inspect.signature(ops.stop_match).parameters, e[1:])) for e in log[loop_end:] if _name(e) == "stop_match"]
            assert [a["n_add"] for a in tail] == list(range(1, 11)) and all(a["n_dev"] is None for a in tail)
    (shape, _, ids), = res["graph"]
    assert shape == [2, 6] and res["nograph"] == res["graph"]
    assert ids[0] == [script.tok(c, 0) for c in range(6)] and ids[0][4:] == STOP[0]
    assert ids[1] == [script.tok(c, 1) for c in range(3)] + [T.EOS, T.PAD, T.PAD]


EAGER_CASES = {"nograph": dict(kw=dict(decode_graph=False)), "fp32": dict(dtype="fp32"), "nocache": dict(kw=dict(use_cache=False)),
               "left-nograph": dict(kw=dict(decode_graph=False), mask="left"),
               "left-nocache-fp32": dict(kw=dict(use_cache=False), mask="left", dtype="fp32"),
               "sample+proc-nocache": dict(kw=dict(T.SAMPLE, **T.PROC, use_cache=False))}


@pytest.mark.parametrize("case", list(EAGER_CASES))
def test_eager_loops_ban_in_front_of_every_selection_and_match_behind_it(monkeypatch, case):
    spec = dict(dict(N=6, finish=None), **EAGER_CASES[case])
    with monkeypatch.context() as mp:
        plain, res0 = _call(mp, spec)
    with monkeypatch.context() as mp:
        got, res = _call(mp, spec, dict(stop_sequences=[[99, 98]], bad_words_ids=BAD, return_logprobs=True,
                                           top_logprobs=2))
    new = ("seq_ban", "stop_match", "token_logprobs")
    assert [e for e in got if _name(e) not in new] == plain and not any(_name(e) in new for e in plain)
    sel = [i for i, e in enumerate(got) if _name(e) in SELECTS]
    assert len(sel) == 6
    for t, i in enumerate(sel):
        assert [_name(e) for e in got[i - 1:i + 3]] == ["seq_ban", _name(got[i]), "token_logprobs", "stop_match"]
        ban = dict(zip(inspect.signature(ops.seq_ban).parameters, got[i - 1][1:]))
        stop = dict(zip(inspect.signature(ops.stop_match).parameters, got[i + 2][1:]))
        assert ban["logits"] == got[i][1] and (ban["n_dev"], ban["n_add"]) == (None, t)
        assert (stop["n_dev"], stop["n_add"]) == (None, t + 1) and _buf(stop["out"]) == _buf(ban["out"])
        have = [row[:t + 1] + [T.PAD] * (5 - t) for row in res0[0][2]]   # the ids selected so far, this token included
        assert stop["out"].endswith("=" + str(have).replace(" ", ""))
    assert res[0] == res0[0]


@pytest.mark.parametrize("path", ["nograph", "nocache", "fp32"])
def test_eager_loops_stop_at_the_sequence_and_give_its_token_a_real_logprob(monkeypatch, path):
    spec = dict(dict(N=12, finish=None), **EAGER_CASES[path])
    script = T.Script(None, 2)
    stops = [STOP[0], [script.tok(2, 1)]]                               # sample 1 stops on a single token at column 2
    with monkeypatch.context() as mp:
        mp.setattr(Mo, "GenerateLogprobs", lambda ids, lp, ti, tl: (ids, lp))
        _, res = _call(mp, spec, dict(stop_sequences=stops, return_logprobs=True))
    (shape, _, ids), (_, _, lp) = res
    assert shape == [2, 6] and ids[0] == [script.tok(c, 0) for c in range(6)]
    assert ids[1] == [script.tok(c, 1) for c in range(3)] + [T.PAD] * 3
    assert lp[1][:3] == [-(1.0 + c + 0.25) for c in range(3)] and lp[1][3:] == [0.0] * 3
    assert lp[0] == [-(1.0 + c) for c in range(6)]


def test_the_defaults_allocate_and_launch_nothing(monkeypatch):
    """with (None, None) generate() must not reach the new code at all: the table class, both ops and the check raise"""
    def boom(*a, **k):
        raise AssertionError("reached with the defaults")
    with monkeypatch.context() as mp:
        lm = T.make_model()
        T.GenTrace(mp, lm, T.Script(3, 2))
        for n in ("SeqTable", "seq_ban", "stop_match"):
            mp.setattr(ops, n, boom)
        mp.setattr(Mo, "_stopping_check", boom)
        for kw in (dict(), dict(decode_graph=False), dict(use_cache=False), T.PROC, dict(num_beams=2)):
            out = lm.generate(inputs_embeds=torch.zeros((2, T.S0, T.D), dtype=torch.bfloat16), max_new_tokens=6,
                              eos_token_id=T.EOS, pad_token_id=T.PAD, **kw)
            assert torch.is_tensor(out)
    # a banned [eos] alone is dropped: the call is the plain one
    with monkeypatch.context() as mp:
        lm = T.make_model()
        T.GenTrace(mp, lm, T.Script(3, 2))
        for n in ("SeqTable", "seq_ban", "stop_match"):
            mp.setattr(ops, n, boom)
        out = lm.generate(inputs_embeds=torch.zeros((2, T.S0, T.D), dtype=torch.bfloat16), max_new_tokens=6,
                          eos_token_id=T.EOS, pad_token_id=T.PAD, bad_words_ids=[[T.EOS]])
        assert torch.is_tensor(out)
