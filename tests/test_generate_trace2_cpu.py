"""CPU: what LlamaForCausalLM.generate() launches, reads and refuses for the switches that came after its first trace,
pinned against tests/golden/generate_launch_trace2.json.

The harness is tests/test_generate_trace_cpu.py's (T): the same tiny model and shapes (B = 2, S0 = 5, 2 layers, V = 40), its
recorders, its scripted tokens, its fake graph and its host-read log.  This file adds what the later switches reach:

  * recorders for ops.decode_emit_sample_warp / _table, ops.sample_rows_warp / _table, ops.cfg_combine and
    ops.logits_penalize, with T's scripted emit and selection as their effect;
  * ops.token_logprobs, ops.decode_emit_logprobs, ops.seq_ban, ops.stop_match, ops.grammar_mask and ops.grammar_advance
    with the fakes tests/test_logprobs_cpu.py, tests/test_stopping_cpu.py and tests/test_grammar_cpu.py already have (one
    chain of _recorders), each wrapped so that the entry it logs is this file's: every argument, at call time;
  * the constructors ops.SeqTable, ops.BiasTable, ops.SampleTable, ops.LogprobState and grammar.combine: logged with
    their arguments, then the real one runs;
  * item() records the device tables by content (a grammar's transition table by shape, flags and checksum); the
    engine's argument records (Ragged, SharedPrompt, Adapters with its AdapterGroups, Beam, Spec, Chunk) are named
    tuples, which T's item() already lists field by field.

A trace case is one generate() call, or two for a session (the second continues the first's session; the session's
books are logged behind each).  The first section holds one log per switch alone on every loop it reaches -- the captured
loop, decode_graph=False, fp32 at a host position, use_cache=False, a left-padded mask -- and one per composition that
shares code in generate().  The second holds refusals: every refusal the later switches added, alone by name, and one
call per pair of them that can be violated together, in the order itertools.combinations gives (the golden file holds
that list's checksum), with the exception type, the full message and the launches before it.

The golden file was written by `python tests/test_generate_trace2_cpu.py --write` on the commit BEFORE generate() got its
one selection chain, and must not be regenerated to make a change pass: a difference is a launch, a host read or a
message that moved."""
import inspect
import itertools
import json
import os
import sys
import zlib

import pytest
import torch

if __name__ == "__main__":      # run as a script (--write): the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_generate_trace_cpu as T
import test_grammar_cpu as TG
import test_lora_bgmv_ref_cpu as TB
import test_stopping_cpu as TS

from macaw_llm_amd import grammar as Gr
from macaw_llm_amd import lora
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_launch_trace2.json")
FIRST_GOLDEN_BYTES = 232273     # tests/golden/generate_launch_trace.json when this file was written: this one's limit

# the launches with a fake of their own here, those whose fake the three older files share, and the constructors: the
# real signatures and classes, taken once, before any recorder
NEW = ("decode_emit_sample_warp", "decode_emit_sample_table", "sample_rows_warp", "sample_rows_table", "cfg_combine",
       "logits_penalize")
SHARED = ("token_logprobs", "decode_emit_logprobs", "seq_ban", "stop_match", "grammar_mask", "grammar_advance")
CTORS = ("SeqTable", "BiasTable", "SampleTable", "LogprobState")
SIGS = {name: inspect.signature(getattr(ops, name)) for name in NEW + SHARED}
REAL = {name: getattr(ops, name) for name in CTORS}
REAL_COMBINE = Gr.combine


class GenTrace2(T.GenTrace):
    """T.GenTrace with the later switches' recorders"""

    def __init__(self, mp, lm, script):
        super().__init__(mp, lm, script)
        TG._recorders(self, mp)         # grammar -> stop sequences and bad words -> log-probabilities
        for name in SHARED:
            mp.setattr(ops, name, self._mine(name, getattr(ops, name)))
        effects = {"decode_emit_sample_warp": self._state(self._emit), "decode_emit_sample_table": self._state(self._emit),
                   "sample_rows_warp": self._select, "sample_rows_table": self._select,
                   "cfg_combine": lambda a: a["logits"][:a["B"]], "logits_penalize": lambda a: a["logits"]}
        for name, eff in effects.items():
            mp.setattr(ops, name, self._rec(name, SIGS[name], eff))
        for name in CTORS:
            mp.setattr(ops, name, self._ctor(name))
        mp.setattr(Gr, "combine", self._combine)

    def item(self, v):
        if isinstance(v, REAL["LogprobState"]):
            return ["LogprobState", v.n_top, self.item(v.lp), self.item(v.fin)]
        if isinstance(v, REAL["SeqTable"]):
            return ["SeqTable", v.ids.tolist(), v.off.tolist()]
        if isinstance(v, REAL["BiasTable"]):
            return ["BiasTable", v.B, v.on] + ([v.off.tolist(), v.ids.tolist(), v.val.tolist()] if v.on else [])
        if isinstance(v, REAL["SampleTable"]):
            return ["SampleTable", [list(v.RECORD.unpack(bytes(r))) for r in v.records.tolist()]]
        if isinstance(v, ops.GrammarTable):
            return ["GrammarTable", v.n_states, v.V, v.flags.tolist(), zlib.crc32(v.next.contiguous().numpy().tobytes())]
        if isinstance(v, Gr.TokenDFA):
            return ["TokenDFA", v.n_states, v.start]
        if isinstance(v, dict):
            return ["dict"] + [[k, self.item(x)] for k, x in sorted(v.items())]
        return super().item(v)

    def _entry(self, name, sig, args, kw):
        a = sig.bind(*args, **kw)
        a.apply_defaults()
        self.quiet += 1
        try:
            return [name] + [self.item(v) for v in a.arguments.values()]
        finally:
            self.quiet -= 1

    def _mine(self, name, shared):
        """the shared fake runs; what it logged gives way to this file's entry: every argument as it is at the call"""
        def rec(*args, **kw):
            entry, n = self._entry(name, SIGS[name], args, kw), len(self.log)
            out = shared(*args, **kw)
            self.log[n:] = [entry]
            return out
        return rec

    def _ctor(self, name):
        real, tr = REAL[name], self
        sig = inspect.signature(real)

        class Rec(real):
            def __init__(self, *args, **kw):
                tr.log.append(tr._entry(name, sig, args, kw))
                tr.quiet += 1
                try:
                    real.__init__(self, *args, **kw)
                finally:
                    tr.quiet -= 1
        return Rec

    def _combine(self, grammars, device, vocab_size):
        self.log.append(self._entry("combine", inspect.signature(REAL_COMBINE), (grammars, device, vocab_size), {}))
        self.quiet += 1
        try:
            return REAL_COMBINE(grammars, device, vocab_size)
        finally:
            self.quiet -= 1


# ---------------------------------------------------------------------------------------------------- calls --
TOK = T.Script(None, 2).tok
WARP = dict(T.SAMPLE, min_p=0.05, typical_p=0.9)
LP = dict(return_logprobs=True, top_logprobs=2)
PEN = dict(frequency_penalty=0.5, presence_penalty=[0.25, -0.5], logit_bias=[{7: 2.0, 3: -100}, None])
SP_MIX = dict(sampling_params=[None, dict(temperature=0.7, top_k=5, seed=11)])
SP_ALL = dict(sampling_params=[dict(temperature=0.8, seed=3), dict(top_p=0.9, min_p=0.1, seed=4)])
SP_GREEDY = dict(sampling_params=[None, dict(temperature=0, top_k=3)])
NS = dict(T.SAMPLE, num_samples=2)
ADAPT = dict(adapter_names=["a1", "__base__"])
STOP_LONG = TS.STOP                                     # sample 0's columns 4 and 5
STOP_SHORT = [[TOK(1, 1), TOK(2, 1)]]                   # sample 1's columns 1 and 2
nog, noc = dict(decode_graph=False), dict(use_cache=False)


def _markers(kw, B, dtype):
    """the arguments a spec names by a word, made per call: tensors, grammars and sessions"""
    kw = dict(kw)
    neg = kw.get("negative_prompt_ids")
    if isinstance(neg, str):
        rows, cols = {"neg3": (B, 3), "neg5": (B, 5), "neg-rows": (1, 3)}.get(neg, (0, 0))
        kw["negative_prompt_ids"] = (5 + torch.arange(6) % 7) if neg == "neg-1d" else (5 + torch.arange(rows * cols) % 7).view(rows, cols)
    emb = kw.get("negative_inputs_embeds")
    if isinstance(emb, str):
        shape, dt = {"emb3": ((B, 3, T.D), dtype), "emb-hidden": ((B, 3, T.D // 2), dtype), "emb-dtype": ((B, 3, T.D), "fp16")}[emb]
        kw["negative_inputs_embeds"] = torch.zeros(shape, dtype=T.DTYPES[dt])
    if isinstance(kw.get("negative_prompt_attention_mask"), str):
        kw["negative_prompt_attention_mask"] = torch.ones((B, 4), dtype=torch.long)
    if isinstance(kw.get("frequency_penalty"), str):
        kw["frequency_penalty"] = torch.zeros((2, 2))
    g = kw.get("grammar")
    if isinstance(g, str):
        free = lambda: Gr.TokenDFA.from_edges(1, [(0, t, 0) for t in range(T.V)], [0], vocab_size=T.V)    # noqa: E731
        g0 = Gr.TokenDFA.from_choices([[TOK(c, 0) for c in range(3)]])
        g1 = Gr.TokenDFA.from_choices([[TOK(c, 1) for c in range(5)], [TOK(c, 1) for c in range(2)]], vocab_size=T.V)
        kw["grammar"] = {"free": free, "half": lambda: [g0, None], "two": lambda: [g0, g1], "three": lambda: [g0, None, g1],
                         "v41": lambda: Gr.TokenDFA.from_choices([[3, 4]], vocab_size=41)}[g]()
    if kw.get("session") == "fresh":
        kvc = [torch.zeros((2, 24, 2 * T.D), dtype=torch.bfloat16) for _ in range(T.LAYERS)]
        kw["session"] = Mo.GenerateSession(kvc, [5, 4], torch.tensor([4, 6]), [[3, 4, 5], [6]], T.D, torch.device("cpu"))
    return kw


def call2(mp, spec, models=None, state=None):
    """T.call with this file's recorders.  More keys of a spec: bank (the model gets an AdapterBank with the adapter "a1"),
    live (and a live adapter's marker); kw may name tensors, grammars and sessions by a word (_markers), session="prev"
    being the session the call before it in `state` returned.  A result comes back as the tuple of its tensors"""
    spec = dict(spec)
    bank, live = spec.pop("bank", False), spec.pop("live", False)
    dtype, vocab, fused = spec.get("dtype", "bf16"), spec.get("vocab", T.V), spec.get("fused", True)
    models = {} if models is None else models
    state = {} if state is None else state
    key = (dtype, vocab, fused, bank, live)
    if key not in models:
        lm = models[key] = T.make_model(dtype, vocab, fused)
        if bank:
            cfg, sd = TB._adapter(lm, 8, 16, ["q_proj", "v_proj", "down_proj"], 1)
            lora.AdapterBank(lm).add("a1", state_dict=sd, config=cfg)
        if live:
            lm._lora = object()
    lm = models[key]
    kw = _markers(spec.get("kw", {}), spec.get("B", T.B0), dtype)
    if kw.get("session") == "prev":
        kw["session"] = state["session"]
    real = lm.generate

    def generate(**k):
        res = real(**k)
        if k.get("return_session"):
            res, state["session"] = res
        elif k.get("session") is not None:
            state["session"] = k["session"]
        return tuple(r for r in (res if isinstance(res, tuple) else (res,)) if r is not None)
    torch.manual_seed(0)
    mp.setattr(T, "GenTrace", GenTrace2)
    lm.generate = generate
    try:
        tr, res = T.call(mp, dict(spec, kw=kw), {(dtype, vocab, fused): lm})
    finally:
        del lm.generate
    s = state.get("session")
    if s is not None and not isinstance(res, dict):
        tr.log.append(["session", list(s._cached_host), s._pending.tolist(), s.ids, s.turns, s.capacity])
    return tr, res


MODES = {"graph": (dict(), 12, 10), "nograph": (dict(kw=nog), 12, 3), "fp32": (dict(dtype="fp32"), 3, None),
         "nocache": (dict(kw=noc), 12, 3), "left": (dict(mask="left"), 12, 10)}


def trace_cases():
    c = {}

    def add(name, mode, kw, turn2=None, **spec):
        base, N, f = MODES[mode]
        case = dict(base, **spec, N=N, finish=f, kw=dict(kw, **base.get("kw", {})))
        if turn2 is not None:
            case["turn2"] = {**base, **turn2, "N": N, "finish": f,
                             "kw": dict(turn2.get("kw", {}), session="prev", **base.get("kw", {}))}
        c[f"{name}-{mode}"] = case

    def stop(mode):
        return dict(stop_sequences=STOP_LONG if MODES[mode][1:] == (12, 10) else STOP_SHORT)

    cfg = dict(guidance_scale=1.5, negative_prompt_ids="neg3")
    for mode in MODES:
        add("warp", mode, WARP)
        add("lp", mode, LP)
        # (fp32 over a cache has no padded batch: prompts of one length run the unpadded path at 2B rows)
        add("cfg", mode, dict(cfg, negative_prompt_ids="neg5") if mode == "fp32" else cfg)
        add("stop", mode, stop(mode))
        add("bad", mode, dict(bad_words_ids=TS.BAD), inputs="both")
        add("gram", mode, dict(grammar="half"))
        add("pen", mode, PEN)
        add("sp", mode, SP_MIX)
        if mode != "fp32":                  # (the shared-prompt step attention takes bf16 / fp16)
            add("ns", mode, NS)
    for mode in ("graph", "nograph", "left"):       # a session is its cache, adapters run the cached layer: bf16 / fp16
        add("sess", mode, dict(return_session=True), turn2=dict(inputs="ids", mask="hole" if mode == "left" else None))
        add("adapt", mode, ADAPT, bank=True)
    # compositions that share code in generate()
    for mode in ("graph", "nograph"):
        add("gram+stop+lp", mode, dict(LP, grammar="two", stop_sequences=[[TOK(3, 1), TOK(4, 1)]]))
        add("pen+proc+bad", mode, dict(PEN, **T.PROC, bad_words_ids=TS.BAD), inputs="both")
        add("cfg+lp+stop", mode, dict(cfg, **LP, **stop(mode)))
    for mode in ("graph", "nograph"):
        add("sess+stop+proc", mode, dict(T.PROC, **stop(mode), return_session=True), inputs="both",
            turn2=dict(inputs="ids", kw=dict(T.PROC, **stop(mode), return_session=True)))
        add("sp-greedy", mode, SP_GREEDY)
    add("ns+sp+gram", "graph", dict(SP_ALL, num_samples=2, grammar="free"))
    add("adapt+w8", "graph", dict(ADAPT, decode_weights="fp8"), bank=True)
    return c


# all-greedy sampling_params: the plain greedy log of the first golden file
SAME_AS_FIRST = {"sp-greedy-graph": "greedy-graph-N12-f10", "sp-greedy-nograph": "greedy-nograph-N12-f3"}


def violations():
    """every condition the later switches refuse, alone: name -> spec"""
    v = {}

    def add(name, kw=None, **spec):
        v[name] = dict(spec, kw=kw or {})

    look, b2, ds = dict(prompt_lookup_num_tokens=4), dict(num_beams=2), dict(do_sample=True)
    # the warpers
    add("minp-high", dict(ds, min_p=1.5))
    add("minp-bool", dict(ds, min_p=True))
    add("typical-0", dict(ds, typical_p=0.0))
    add("eps-1", dict(ds, epsilon_cutoff=1.0))
    add("eta-nan", dict(ds, eta_cutoff=float("nan")))
    # log-probabilities
    add("top-21", dict(return_logprobs=True, top_logprobs=21))
    add("top-bool", dict(return_logprobs=True, top_logprobs=True))
    add("top-alone", dict(top_logprobs=5))
    add("lp-beams", dict(b2, return_logprobs=True))
    add("lp-look", dict(look, return_logprobs=True))
    # guidance
    g = dict(guidance_scale=1.5)
    gn = dict(g, negative_prompt_ids="neg3")
    add("cfg-nan", dict(guidance_scale=float("nan")))
    add("cfg-str", dict(guidance_scale="2"))
    add("cfg-noneg", g)
    add("cfg-both", dict(gn, negative_inputs_embeds="emb3"))
    add("cfg-beams", dict(gn, **b2))
    add("cfg-look", dict(gn, **look))
    add("cfg-neg-rows", dict(g, negative_prompt_ids="neg-rows"))
    add("cfg-neg-1d", dict(g, negative_prompt_ids="neg-1d"))
    add("cfg-emb-hidden", dict(g, negative_inputs_embeds="emb-hidden"))
    add("cfg-emb-dtype", dict(g, negative_inputs_embeds="emb-dtype"))
    add("cfg-negmask", dict(gn, negative_prompt_attention_mask="short"))
    add("cfg-padded-fp32", gn, dtype="fp32")
    add("cfg-w8-rows", dict(gn, decode_weights="fp8"), B=17)
    # stop sequences and bad words
    for name in ("stop_sequences", "bad_words_ids"):
        s = name[:4].rstrip("_")
        add(f"{s}-empty", {name: []})
        add(f"{s}-inner", {name: [[3], []]})
        add(f"{s}-neg", {name: [[3, -1]]})
        add(f"{s}-float", {name: [[3.0]]})
        add(f"{s}-long", {name: [list(range(65))]})
        add(f"{s}-beams", dict(b2, **{name: [[3]]}))
        add(f"{s}-look", dict(look, **{name: [[3]]}))
    add("stop-many", dict(stop_sequences=[[3]] * 65537))
    # parallel samples
    add("ns-0", dict(ds, num_samples=0))
    add("ns-33", dict(ds, num_samples=33))
    add("ns-float", dict(ds, num_samples=2.0))
    add("ns-greedy", dict(num_samples=2))
    add("ns-beams", dict(ds, num_samples=2, **b2))
    add("ns-look", dict(ds, num_samples=2, **look))
    add("ns-cfg", dict(ds, num_samples=2, **gn))
    add("ns-kv8", dict(ds, num_samples=2, kv_cache="fp8"))
    add("ns-fp32", dict(ds, num_samples=2), dtype="fp32")
    add("ns-long", dict(ds, num_samples=2), N=16000)
    add("ns-sp-greedy", dict(num_samples=2, sampling_params=[dict(temperature=0.5), None]))
    # sessions
    rs = dict(return_session=True)
    add("sess-type", dict(session="a session"))
    add("sess-nocache", dict(rs, use_cache=False))
    add("sess-beams", dict(rs, **b2))
    add("sess-ns", dict(rs, **ds, num_samples=2))
    add("sess-look", dict(rs, **look))
    add("sess-cfg", dict(rs, **gn))
    add("sess-kv8", dict(rs, kv_cache="fp8"))
    add("sess-cap-0", dict(rs, session_capacity=0))
    add("sess-cap-low", dict(rs, session_capacity=3))
    add("sess-fp32", rs, dtype="fp32")
    add("sess-long", rs, N=16000)
    fresh = dict(session="fresh")
    add("cont-nocache", dict(fresh, use_cache=False))
    add("cont-batch", fresh, B=3)
    add("cont-dtype", fresh, dtype="fp16")
    add("cont-mask-shape", fresh, mask="short")
    add("cont-mask-dead", fresh, mask="dead")
    # adapters
    add("ad-nobank", ADAPT)
    add("ad-live", ADAPT, bank=True, live=True)
    add("ad-beams", dict(ADAPT, **b2), bank=True)
    add("ad-ns", dict(ADAPT, **ds, num_samples=2), bank=True)
    add("ad-look", dict(ADAPT, **look), bank=True)
    add("ad-cfg", dict(ADAPT, **gn), bank=True)
    add("ad-sess", dict(ADAPT, **rs), bank=True)
    add("ad-nocache", dict(ADAPT, use_cache=False), bank=True)
    add("ad-count", dict(adapter_names=["a1", "__base__", "a1"]), bank=True)
    add("ad-unknown", dict(adapter_names=["a1", "a9"]), bank=True)
    add("ad-fp32", ADAPT, bank=True, dtype="fp32")
    add("ad-unfused", ADAPT, bank=True, fused=False)
    add("ad-33", dict(adapter_names=["a1"] * 33), bank=True, B=33)
    add("ad-long", ADAPT, bank=True, N=16000)
    # grammars
    add("gr-type", dict(grammar=5))
    add("gr-entry", dict(grammar=[None, "a grammar"]))
    add("gr-empty", dict(grammar=[]))
    add("gr-beams", dict(b2, grammar="free"))
    add("gr-look", dict(look, grammar="free"))
    add("gr-sess", dict(rs, grammar="free"))
    add("gr-count", dict(grammar="three"))
    add("gr-vocab", dict(grammar="v41"))
    # penalties and the bias
    add("fp-high", dict(frequency_penalty=2.5))
    add("pp-nan", dict(presence_penalty=float("nan")))
    add("pp-bool", dict(presence_penalty=True))
    add("fp-count", dict(frequency_penalty=[0.1, 0.2, 0.3]))
    add("fp-2d", dict(frequency_penalty="2d"))
    add("lb-type", dict(logit_bias=5))
    add("lb-row", dict(logit_bias=[5, None]))
    add("lb-count", dict(logit_bias=[None, None, {3: 1.0}]))
    add("lb-id-neg", dict(logit_bias={-1: 1.0}))
    add("lb-id-V", dict(logit_bias={T.V: 1.0}))
    add("lb-val", dict(logit_bias={3: 101}))
    add("lb-many", dict(logit_bias={i: 1.0 for i in range(1025)}))
    add("pen-beams", dict(b2, presence_penalty=0.5))
    add("pen-look", dict(look, logit_bias={3: 1.0}))
    # per-request sampling
    sp = [dict(temperature=0.5), dict(temperature=0.5)]
    add("sp-dosample", dict(ds, sampling_params=sp))
    add("sp-type", dict(sampling_params=dict(temperature=0.5)))
    add("sp-count", dict(sampling_params=sp[:1]))
    add("sp-entry", dict(sampling_params=[5, None]))
    add("sp-key", dict(sampling_params=[dict(temp=0.5), None]))
    add("sp-temp", dict(sampling_params=[dict(temperature=-1.0), None]))
    add("sp-minp", dict(sampling_params=[None, dict(temperature=0, min_p=2)]))
    add("sp-seed", dict(sampling_params=[dict(seed=1.5), None]))
    add("sp-beams", dict(b2, sampling_params=sp))
    add("sp-look", dict(look, sampling_params=sp))
    return v


def _merge(a, b):
    """the two specs in one call, or None where they set one argument differently"""
    out = {}
    for k in set(a) | set(b):
        if k == "kw":
            continue
        if k in a and k in b and a[k] != b[k]:
            return None
        out[k] = a[k] if k in a else b[k]
    kw = dict(a["kw"])
    for k, val in b["kw"].items():
        if k in kw and kw[k] != val and not (kw[k] != kw[k] and val != val):
            return None
        kw[k] = val
    return dict(out, kw=kw)


def refusal_pairs():
    """[(name, spec)] of every pair of violations that one call can hold, in combinations' order"""
    v, out = violations(), []
    for (na, a), (nb, b) in itertools.combinations(v.items(), 2):
        m = _merge(a, b)
        if m is not None and m != a and m != b:
            out.append((f"{na}+{nb}", m))
    return out


def run_trace_case(spec):
    spec = dict(spec)
    turns, models, state, log, returns = [spec, spec.pop("turn2", None)], {}, {}, [], []
    for turn in turns:
        if turn is None:
            continue
        with pytest.MonkeyPatch.context() as mp:        # (a second turn's recorders bind to the real signatures again)
            tr, res = call2(mp, {k: v for k, v in turn.items() if v is not None}, models, state)
        log += (["turn"] if log else []) + tr.log
        returns.append(res)
    return {"log": log, "returns": returns}


def run_refusal_case(spec, models):
    """as T.run_refusal_case: the error and the names of what was launched before it; a pair that cancels runs, to column 3"""
    with pytest.MonkeyPatch.context() as mp:
        tr, res = call2(mp, dict(spec, finish=3), models)
    before = [e if isinstance(e, str) else e[0] for e in tr.log if isinstance(e, str) or e[0] not in ("host", "cast")]
    if isinstance(res, dict):
        return dict(res, before=before)
    return {"raises": None}


# ------------------------------------------------------------------------------------------------ the tests --
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models():
    return {}


def _want(golden, ref):
    return {"raises": None} if ref is None else dict(golden["messages"][ref[0]], before=golden["befores"][ref[1]])


def _pair_refs(golden):
    """the pairs' references, stored as message * len(befores) + before (-1: the pair cancels and the call runs)"""
    nb = len(golden["befores"])
    return [None if r < 0 else divmod(r, nb) for r in golden["pairs"]]


@pytest.mark.parametrize("case", list(trace_cases()))
def test_generate_launches_and_reads_what_the_golden_trace_says(case, golden):
    got = T._plain(run_trace_case(trace_cases()[case]))
    want = golden["traces"][case]
    want_log = [golden["entries"][i] for i in want["log"]]
    for i, (g, w) in enumerate(itertools.zip_longest(got["log"], want_log)):
        assert g == w, f"{case}: entry {i} moved:\n  now      {g}\n  expected {w}"
    assert got["returns"] == want["returns"], case


@pytest.mark.parametrize("case,plain", list(SAME_AS_FIRST.items()))
def test_all_greedy_sampling_params_are_the_plain_greedy_call(case, plain, golden):
    with open(T.GOLDEN) as f:
        first = json.load(f)
    mine, theirs = golden["traces"][case], first["traces"][plain]
    assert [golden["entries"][i] for i in mine["log"]] == [first["entries"][i] for i in theirs["log"]]
    assert mine["returns"] == [theirs["returns"]]


def test_every_refusal_keeps_its_type_message_and_place(golden, models):
    singles = violations()
    assert sorted(singles) == sorted(golden["refusals"])
    for name, spec in singles.items():
        got = T._plain(run_refusal_case(spec, models))
        want = _want(golden, golden["refusals"][name])
        assert got == want, f"{name}:\n  now      {got}\n  expected {want}"
        assert got["raises"] is not None, name


def test_every_pair_of_refusals_keeps_its_precedence(golden, models):
    pairs = refusal_pairs()
    assert zlib.crc32("\n".join(n for n, _ in pairs).encode()) == golden["pair_names_crc"]
    assert len(pairs) == len(golden["pairs"])
    for (name, spec), ref in zip(pairs, _pair_refs(golden)):
        got = T._plain(run_refusal_case(spec, models))
        want = _want(golden, ref)
        assert got == want, f"{name}:\n  now      {got}\n  expected {want}"


def test_a_refused_call_has_allocated_no_cache_and_copied_no_weight(golden):
    for ref in list(golden["refusals"].values()) + _pair_refs(golden):
        if ref is not None and "unfused" not in golden["messages"][ref[0]]["message"]:     # (found per layer, behind the caches)
            assert set(golden["befores"][ref[1]]) <= {"embedding_fwd"}, golden["messages"][ref[0]]
    assert {m["raises"] for m in golden["messages"]} == {"ValueError"}


def test_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden["traces"]) == sorted(trace_cases())
    assert os.path.getsize(GOLDEN) <= FIRST_GOLDEN_BYTES


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_generate_trace2_cpu.py --write   (on the commit the traces are taken from)")
    entries, eidx, traces = [], {}, {}
    for name, spec in trace_cases().items():
        got = T._plain(run_trace_case(spec))
        traces[name] = {"log": [T._intern(e, entries, eidx) for e in got["log"]], "returns": got["returns"]}
    messages, midx, befores, bidx, mods = [], {}, [], {}, {}

    def ref(spec):
        got = T._plain(run_refusal_case(spec, mods))
        if got["raises"] is None:
            return None
        before = got.pop("before")
        return [T._intern(got, messages, midx), T._intern(before, befores, bidx)]
    refusals = {name: ref(spec) for name, spec in violations().items()}
    pairs = refusal_pairs()
    pair_refs = [ref(spec) for _, spec in pairs]
    pair_refs = [-1 if r is None else r[0] * len(befores) + r[1] for r in pair_refs]
    dump = lambda o: json.dumps(o, separators=(",", ":"))     # noqa: E731

    def lines(d):
        return "{\n" + ",\n".join(f"{json.dumps(k)}:{dump(val)}" for k, val in d.items()) + "\n}"
    with open(GOLDEN, "w") as f:
        f.write('{"entries":[\n' + ",\n".join(dump(e) for e in entries) + '\n],\n"traces":' + lines(traces)
                + ',\n"messages":[\n' + ",\n".join(dump(e) for e in messages) + '\n],\n"befores":' + dump(befores)
                + ',\n"refusals":' + lines(refusals) + f',\n"pair_names_crc":{zlib.crc32(chr(10).join(n for n, _ in pairs).encode())}'
                + ',\n"pairs":' + dump(pair_refs) + "\n}\n")
    print(f"wrote {len(traces)} traces ({len(entries)} distinct entries), {len(refusals)} refusals and {len(pairs)} pairs "
          f"({len(messages)} distinct messages), {os.path.getsize(GOLDEN)} bytes")
