"""CPU: what LlamaForCausalLM.generate() launches, reads and refuses, pinned against tests/golden/generate_launch_trace.json.

The real generate() runs on CPU tensors against a real tiny LlamaForCausalLM (D = 128, 2 heads, 2 layers, V = 40, fused
projections).  Nothing is launched: _dev_check passes, and engine.llama_layer_cached, engine._stream_linear, the
model's own forward (the use_cache=False loops), beam_result and every ops.<launch> generate() reaches are recorders that
bind the call to the real signature and append [name, one item per argument] to the case's log.  A tensor is recorded
as a model parameter's name or as its buffer (numbered in the order the buffers first appear in the case), shape and
dtype, with stride and offset where it is not a plain contiguous tensor and with its values where it is a small integer
or bool tensor (positions, counters, flags, masks).  The predicates (ops.decode_attn_ok, ops.spec_attn_ok, the *_ok of
the streamed linears) are the real ones.

The fake emits advance the device state as the real ones do -- position and output column of decode_emit /
beam_emit's state, the books of ops.BeamState, the per-sample position and count of ops.SpecState -- and emit a
scripted token: 3 + (7 col + 3 b) % 30, and eos from column F - 1 (sample 0) / F (sample 1) on when the case finishes at
F.  torch.cuda.CUDAGraph / torch.cuda.graph are fakes with a real graph's semantics: a captured launch is logged but
does not run, and every replay runs the captured launches' effects on the same buffers.  Every host look at a tensor
(bool(), int(), .cpu()) outside the recorders is logged where it happens, so the reads of the done flags stand between
the launches they stood between.

A second section holds refusals: every kind of refused call the tests make and one call per pair of conditions that
can be violated together, with the exception type, its full message and the launches that ran before it.

The golden file was written by `python tests/test_generate_trace_cpu.py --write` on the commit BEFORE generate() got its
single decode loop driver and refusal stage, and must not be regenerated to make a change pass: a difference is a
launch, a host read or a message that moved."""
import inspect
import itertools
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":      # run as a script (--write): the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from macaw_llm_amd import engine as eng
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_launch_trace.json")
B0, S0, D, HEADS, LAYERS, V, FF = 2, 5, 128, 2, 2, 40, 256
EOS, PAD = 2, 0
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}

# the launches generate() itself reaches, with the signatures of the real ops (taken once, before any recorder)
OPS = ("embedding_fwd", "copy2d", "rmsnorm_fwd", "linear_fwd", "argmax_rows", "sample_rows", "decode_emit",
       "decode_emit_sample", "beam_emit", "spec_lookup", "spec_verify_emit", "logits_process", "kv8_cache", "fp8_weight",
       "quantize_fp8_rows", "mxfp4_weight", "quantize_mxfp4_rows", "cast")
SIGS = {name: inspect.signature(getattr(ops, name)) for name in OPS}
SIGS["llama_layer_cached"] = inspect.signature(eng.llama_layer_cached)
SIGS["_stream_linear"] = inspect.signature(eng._stream_linear)
SIGS["beam_result"] = inspect.signature(Mo.beam_result)


def make_model(dtype="bf16", vocab=V, fused=True):
    from transformers import LlamaConfig
    cfg = LlamaConfig(hidden_size=D, intermediate_size=FF, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                      num_key_value_heads=HEADS, vocab_size=vocab, max_position_embeddings=64)
    lm = Mo.LlamaForCausalLM(cfg).to(DTYPES[dtype]).eval()
    if fused:
        for lyr in lm.model.layers:
            lyr.fuse_projections()
    return lm


class Script:
    """the token of (output column, sample), and the column from which a sample emits eos (None: never)"""

    def __init__(self, finish, B):
        self.finish, self.B = finish, B

    def fin(self, b):
        return None if self.finish is None else max(self.finish - (self.B - 1 - b), 0)

    def tok(self, col, b):
        f = self.fin(b)
        return EOS if f is not None and col >= f else 3 + (7 * col + 3 * b) % 30


class GenTrace:
    """the recorders of one generate() call"""

    def __init__(self, mp, lm, script):
        self.log, self.bufs, self.keep, self.names = [], {}, [], {}
        self.quiet, self.capture, self.col, self.script = 0, None, 0, script
        tr = self
        for i, lyr in enumerate(lm.model.layers):
            a, m = lyr.self_attn, lyr.mlp
            wqkv, wgu = lyr.fused_weights()
            for n, t in (("wq", a.q_proj.weight), ("wk", a.k_proj.weight), ("wv", a.v_proj.weight), ("wo", a.o_proj.weight),
                         ("wg", m.gate_proj.weight), ("wu", m.up_proj.weight), ("wd", m.down_proj.weight), ("wqkv", wqkv),
                         ("wgu", wgu), ("ln1", lyr.input_layernorm.weight), ("ln2", lyr.post_attention_layernorm.weight)):
                if t is not None:
                    self.names[self._key(t)] = f"L{i}.{n}"
        for n, t in (("head", lm.lm_head.weight), ("emb", lm.model.embed_tokens.weight), ("norm", lm.model.norm.weight)):
            self.names[self._key(t)] = n

        effects = {
            "embedding_fwd": lambda a: a["out"] if a["out"] is not None else
            torch.zeros((a["ids"].numel(), a["table"].shape[1]), dtype=a["table"].dtype),
            "copy2d": lambda a: a["dst"],
            "rmsnorm_fwd": lambda a: (a["x"], torch.zeros(tuple(a["x"].shape), dtype=a["x"].dtype), None),
            "linear_fwd": lambda a: torch.zeros((a["x"].shape[0], a["W"].shape[0]), dtype=a["x"].dtype),
            "_stream_linear": lambda a: torch.zeros((a["x"].shape[0], a["W"].shape[0]), dtype=a["x"].dtype),
            "llama_layer_cached": lambda a: a["x2"],
            "argmax_rows": self._select, "sample_rows": self._select,
            "decode_emit": self._state(self._emit), "decode_emit_sample": self._state(self._emit),
            "beam_emit": self._state(self._beam_emit), "spec_lookup": self._state(self._lookup),
            "spec_verify_emit": self._state(self._verify),
            "logits_process": lambda a: a["logits"],
            "kv8_cache": lambda a: (torch.empty((a["B"], a["t_max"], 2 * a["H"] * a["hd"]), dtype=torch.uint8),
                                    torch.empty((a["B"], a["t_max"], 2 * a["H"]), dtype=torch.float32)),
            "fp8_weight": lambda a: self._q8(a["W"]), "quantize_fp8_rows": lambda a: self._q8(a["x"]),
            "mxfp4_weight": lambda a: self._q4(a["W"]), "quantize_mxfp4_rows": lambda a: self._q4(a["x"]),
            "cast": lambda a: a["x"].to(a["dtype"]),
            "beam_result": lambda a: REAL_BEAM_RESULT(**a),
        }
        for name, eff in effects.items():
            where = eng if name in ("llama_layer_cached", "_stream_linear") else Mo if name == "beam_result" else ops
            mp.setattr(where, name, self._rec(name, SIGS[name], eff))
        mp.setattr(Mo, "_dev_check", lambda t: None)

        def model_forward(model, inputs_embeds=None, attention_mask=None, position_ids=None, **kw):
            assert not kw, kw
            tr.log.append(["model", tr.item(inputs_embeds), tr.item(attention_mask), tr.item(position_ids),
                           bool(getattr(model, "_defer_final_norm", False))])
            return inputs_embeds
        mp.setattr(Mo.LlamaModel, "forward", model_forward)

        class Graph:
            def __init__(self):
                self.thunks = []
                tr.log.append("graph")

            def replay(self):
                tr.log.append("replay")
                tr.quiet += 1
                try:
                    for th in self.thunks:
                        th()
                finally:
                    tr.quiet -= 1

        class Capture:
            def __init__(self, g):
                self.g = g

            def __enter__(self):
                tr.log.append("capture{")
                tr.capture = self.g

            def __exit__(self, *exc):
                tr.log.append("}")
                tr.capture = None
        mp.setattr(torch.cuda, "CUDAGraph", Graph)
        mp.setattr(torch.cuda, "graph", Capture)
        # every host look at a tensor outside the recorders
        for meth in ("__bool__", "__int__", "cpu"):
            mp.setattr(torch.Tensor, meth, self._host_read(meth, getattr(torch.Tensor, meth)))

    # ------------------------------------------------------------------------------------------- recording --
    @staticmethod
    def _key(t):
        return (t.untyped_storage()._cdata, t.storage_offset(), tuple(t.shape), t.stride())

    def item(self, v):
        if torch.is_tensor(v):
            name = self.names.get(self._key(v))
            if name is not None:
                return name
            key = v.untyped_storage()._cdata
            if key not in self.bufs:
                self.bufs[key] = len(self.bufs)
                self.keep.append(v)             # a freed storage's address could come back as another buffer's
            s = f"b{self.bufs[key]}{list(v.shape)}{str(v.dtype).replace('torch.', '')}".replace(" ", "")
            if not v.is_contiguous() or v.storage_offset():
                s += f"s{list(v.stride())}o{v.storage_offset()}".replace(" ", "")
            if v.dtype in (torch.bool, torch.int32, torch.int64, torch.uint8) and 0 < v.numel() <= 40:
                self.quiet += 1
                s += "=" + json.dumps(v.tolist(), separators=(",", ":")).replace("true", "1").replace("false", "0")
                self.quiet -= 1
            return s
        if isinstance(v, ops.BeamState):
            return ["BeamState", self.item(v.tok), self.item(v.done), self.item(v.ind)]
        if isinstance(v, ops.SpecState):
            return ["SpecState", self.item(v.pos), self.item(v.n_out), self.item(v.done), self.item(v.tok)]
        if isinstance(v, (tuple, list)):
            return ([type(v).__name__] if hasattr(v, "_fields") else []) + [self.item(e) for e in v]
        if isinstance(v, (torch.dtype, torch.device)):
            return str(v)
        if isinstance(v, float) and v != v:
            return "nan"
        assert v is None or isinstance(v, (bool, int, float, str)), v
        return v

    def _rec(self, name, sig, effect):
        def rec(*args, **kw):
            a = sig.bind(*args, **kw)
            a.apply_defaults()
            a = dict(a.arguments)
            self.quiet += 1
            try:
                self.log.append([name] + [self.item(v) for v in a.values()])
                return effect(a)
            finally:
                self.quiet -= 1
        return rec

    def _host_read(self, meth, real):
        tr = self

        def read(t, *args, **kw):
            out = real(t, *args, **kw)
            if tr.quiet == 0:
                tr.log.append(["host", meth, list(t.shape)] + ([] if meth == "cpu" else [int(out)]))
            return out
        return read

    def _state(self, fn):
        """an op that changes device state: inside a capture it is recorded for the replays and does not run"""
        def eff(a):
            if self.capture is not None:
                self.capture.thunks.append(lambda: fn(a))
            else:
                fn(a)
        return eff

    # ----------------------------------------------------------------------------------------- the fakes --
    @staticmethod
    def _q8(W):
        return torch.empty(tuple(W.shape), dtype=torch.uint8), torch.empty(W.shape[0], dtype=torch.float32)

    @staticmethod
    def _q4(W):
        return (torch.empty((W.shape[0], W.shape[1] // 2), dtype=torch.uint8),
                torch.empty((W.shape[0], W.shape[1] // 32), dtype=torch.uint8))

    def _select(self, a):           # the host-selection loops: one call per output column
        col = a["step"] if "step" in a else self.col
        self.col = col + 1
        return torch.tensor([self.script.tok(col, b) for b in range(a["x"].shape[0])], dtype=torch.long)

    def _emit(self, a):
        st, tok, done, out = a["state"], a["tok"], a["done"], a["out"]
        col = int(st[1])
        for b in range(tok.numel()):
            nxt = a["pad"] if bool(done[b]) else self.script.tok(col, b)
            out[b, col] = nxt
            tok[b] = nxt
            done[b] |= nxt == a["eos"]
        st[0] += 1
        st[1] = col + 1

    def _beam_emit(self, a):
        bs, st, pad = a["bs"], a["state"], a["pad"]
        K, col = bs.K, int(st[1])
        for b in range(bs.B):
            for k in range(K):
                row = b * K + k
                if bool(bs.done[b]) or self.script.tok(col, b) == a["eos"]:
                    bs.tok[row] = pad
                    bs.hist[col, b, k, 0], bs.hist[col, b, k, 1] = pad, k
                else:
                    bs.tok[row] = self.script.tok(col, b) + k
                    bs.hist[col, b, k, 0], bs.hist[col, b, k, 1] = int(bs.tok[row]), ((k + 1) % K if col > 0 else 0)
                    bs.scores[row] -= 0.25 * (k + 1)
                bs.ind[row, col] = k
            if not bool(bs.done[b]) and self.script.tok(col, b) == a["eos"]:      # K hypotheses end here
                for e in range(K):
                    bs.pool_score[b, e] = -(e + 1.0) - b
                    bs.pool_info[b, e] = torch.tensor([col, e, e, 0], dtype=torch.int32)
                bs.pool_info[b, K, 0], bs.pool_info[b, K, 1] = K, K
                bs.done[b] = True
        st[0] += 1
        st[1] = col + 1

    def _lookup(self, a):
        ss = a["ss"]
        for b in range(ss.B):
            ss.n_draft[b] = 0 if bool(ss.done[b]) else ss.G
            ss.tok[b, 1:] = ss.pad if bool(ss.done[b]) else torch.arange(5, 5 + ss.G)

    def _verify(self, a):
        ss, eos = a["ss"], a["eos"]
        R = a["logits"].shape[0] // ss.B
        for b in range(ss.B):
            if bool(ss.done[b]):
                continue
            for _ in range(1 if R == 1 else 2):       # a verify step keeps one draft token and adds one
                col = int(ss.n_out[b])
                nxt = self.script.tok(col, b)
                ss.out[b, col] = nxt
                ss.tok[b, 0] = nxt
                ss.n_out[b] += 1
                ss.pos[b] += 1
                if nxt == eos or col + 1 >= ss.n_max:
                    ss.done[b] = True
                    break
            ss.steps[b] += 1


REAL_BEAM_RESULT = Mo.beam_result


# ---------------------------------------------------------------------------------------------------- calls --
MASKS = {"left": [[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]], "hole": [[1, 0, 1, 1, 1], [0, 1, 1, 0, 1]], "ones": [[1] * 5] * 2,
         "dead": [[0] * 5, [1] * 5], "short": [[1, 1, 1, 1]] * 2}
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2)
BEAMS = dict(num_beams=3, length_penalty=0.5, early_stopping=True, num_return_sequences=2)
SAMPLE = dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, seed=7)
LOOK = dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=3)


def call(mp, spec, models=None):
    """one generate() call from a spec: N, finish, dtype, B, vocab, fused, env, inputs ("emb", "ids", "both", "ids1":
    embeddings with ids of one row, "idsw": with ids of S0 + 1 columns), mask (a name of MASKS), kw (generate's own arguments) -> (trace, result or error)"""
    spec = dict(spec)
    kw = dict(spec.pop("kw", {}))
    N, finish, dtype = spec.pop("N", 12), spec.pop("finish", None), spec.pop("dtype", "bf16")
    B, vocab, fused = spec.pop("B", B0), spec.pop("vocab", V), spec.pop("fused", True)
    env, inputs, mask = spec.pop("env", False), spec.pop("inputs", "emb"), spec.pop("mask", None)
    assert not spec, spec
    key = (dtype, vocab, fused)
    lm = models[key] if models is not None and key in models else make_model(dtype, vocab, fused)
    if models is not None:
        models[key] = lm
    if env:
        mp.setenv("MACAW_NO_DECODE_GRAPH", "1")
    else:
        mp.delenv("MACAW_NO_DECODE_GRAPH", raising=False)
    if inputs != "ids":
        kw["inputs_embeds"] = torch.zeros((B, S0, D), dtype=DTYPES[dtype])
    if inputs != "emb":
        cols = S0 + 1 if inputs == "idsw" else S0
        kw["input_ids"] = (3 + torch.arange(B * cols) % 11).view(B, cols)[:1 if inputs == "ids1" else B]
    if mask is not None:
        kw["attention_mask"] = torch.tensor(MASKS[mask])
    tr = GenTrace(mp, lm, Script(finish, B))
    try:
        res = lm.generate(max_new_tokens=N, eos_token_id=EOS, pad_token_id=PAD, **kw)
    except Exception as e:      # noqa: BLE001 -- a refusal is a result
        tr.quiet += 1
        return tr, {"raises": type(e).__name__, "message": str(e)}
    tr.quiet += 1
    tr.log.append(["defer_after", bool(getattr(lm.model, "_defer_final_norm", False))])
    res = res if isinstance(res, tuple) else (res,)
    return tr, [[list(r.shape), str(r.dtype).replace("torch.", ""), r.tolist()] for r in res]


def trace_cases():
    c = {}
    modes = {"graph": {}, "nograph": dict(kw=dict(decode_graph=False)), "env": dict(env=True), "fp32": dict(dtype="fp32"),
             "nocache": dict(kw=dict(use_cache=False))}
    runs = [(1, None), (2, None), (3, None), (12, None), (12, 3), (12, 10)]
    for (m, spec), (N, f) in itertools.product(modes.items(), runs):
        c[f"greedy-{m}-N{N}-f{f}"] = dict(spec, N=N, finish=f)

    def add(name, N=12, finish=None, kw=None, **spec):
        c[f"{name}-N{N}-f{finish}"] = dict(spec, N=N, finish=finish, kw=kw or {})

    nog, noc = dict(decode_graph=False), dict(use_cache=False)
    # sampling
    add("sample-graph", 12, 10, SAMPLE)
    add("sample-nograph", 3, None, {**SAMPLE, **nog})
    add("sample-nocache", 3, None, {**SAMPLE, **noc})
    # the processors, with and without the prompt's ids
    add("proc-graph-both", 12, 10, PROC, inputs="both")
    add("proc-graph-emb", 12, 3, PROC)
    add("proc-graph-ids", 3, None, PROC, inputs="ids")
    add("proc-nograph-both", 12, 3, {**PROC, **nog}, inputs="both")
    add("proc-nograph-emb", 3, None, {**PROC, **nog})
    add("proc-fp32-both", 3, None, PROC, inputs="both", dtype="fp32")
    add("proc-nocache-both", 12, 3, {**PROC, **noc}, inputs="both")
    add("proc-nocache-emb", 3, None, {**PROC, **noc})
    add("proc+sample-graph-both", 12, 3, {**PROC, **SAMPLE}, inputs="both")
    add("proc+sample-nocache-emb", 3, None, {**PROC, **SAMPLE, **noc})
    add("proc+left-graph-both", 12, 3, PROC, inputs="both", mask="left")
    add("proc+left-nograph-both", 3, None, {**PROC, **nog}, inputs="both", mask="left")
    add("proc+hole-nocache-both", 3, None, {**PROC, **noc}, inputs="both", mask="hole")
    add("proc+kv8-graph-emb", 12, 3, {**PROC, "kv_cache": "fp8"})
    # padded batches
    for mk in ("left", "hole"):
        add(f"{mk}-graph", 12, 10, mask=mk)
        add(f"{mk}-graph", 3, None, mask=mk)
        add(f"{mk}-nograph", 12, 3, nog, mask=mk)
        add(f"{mk}-small", 2, None, mask=mk)
        add(f"{mk}-nocache", 12, 3, noc, mask=mk)
        add(f"{mk}-nocache-fp32", 3, None, noc, mask=mk, dtype="fp32")
    add("ones-graph", 12, 10, mask="ones")
    add("left+kv8+sample-graph", 12, 3, {**SAMPLE, "kv_cache": "fp8"}, mask="left")
    add("left-env", 12, 3, mask="left", env=True)
    # the e4m3 cache and the streamed weight copies
    add("kv8-graph", 12, 10, dict(kv_cache="fp8"))
    add("kv8-graph", 3, None, dict(kv_cache="fp8"))
    add("kv8+w8-graph", 12, 3, dict(kv_cache="fp8", decode_weights="fp8"))
    for w in ("fp8", "mxfp4"):
        add(f"w-{w}-graph", 12, 3, dict(decode_weights=w))
        add(f"w-{w}-graph", 3, None, dict(decode_weights=w))
    add("kv8-unfused-graph", 3, None, dict(kv_cache="fp8"), fused=False)
    # beam search
    for N, f in runs:
        add("beam-graph", N, f, BEAMS)
    for N, f in ((2, None), (3, None), (12, 3)):
        add("beam-nograph", N, f, {**BEAMS, **nog})
        add("beam-nocache", N, f, {**BEAMS, **noc})
    add("beam-env", 12, 3, BEAMS, env=True)
    add("beam-nocache-fp32-scores", 3, None, {**BEAMS, **noc, "return_beam_scores": True}, dtype="fp32")
    add("beam+mxfp4-graph", 12, 3, {**BEAMS, "decode_weights": "mxfp4"})
    add("beam+ones-graph-scores", 12, 10, {**BEAMS, "return_beam_scores": True}, mask="ones")
    add("onebeam-graph", 12, 10, {**BEAMS, "num_beams": 1})
    add("onebeam-nocache", 12, 3, {**BEAMS, "num_beams": 1, **noc})
    # prompt lookup
    for N, f in runs:
        add("look-graph-emb", N, f, LOOK)
    add("look-graph-both", 12, 10, LOOK, inputs="both")
    add("look-graph-ids", 12, 3, LOOK, inputs="ids")
    for N, f in ((2, None), (3, None), (12, 3), (12, None)):
        add("look-nograph-emb", N, f, {**LOOK, **nog})
    add("look-nograph-both", 12, 3, {**LOOK, **nog}, inputs="both")
    add("look-env-ids", 12, 10, LOOK, inputs="ids", env=True)
    add("look+fp8-graph-both-stats", 12, 3, {**LOOK, "decode_weights": "fp8", "return_lookup_stats": True}, inputs="both")
    add("look+ones-graph", 12, 3, LOOK, mask="ones")
    add("nolook-graph", 12, 10, dict(prompt_lookup_num_tokens=0, max_matching_ngram_size=3))
    add("nolook-nograph", 12, 3, dict(prompt_lookup_num_tokens=0, max_matching_ngram_size=3, **nog))
    return c


# the traces that must equal the plain greedy trace of the same shape
SAME_AS = {"onebeam-graph-N12-f10": "greedy-graph-N12-f10", "onebeam-nocache-N12-f3": "greedy-nocache-N12-f3",
           "nolook-graph-N12-f10": "greedy-graph-N12-f10", "nolook-nograph-N12-f3": "greedy-nograph-N12-f3",
           "ones-graph-N12-f10": None}      # (a mask without a zero: the same launches behind the host's look at the mask)


def violations():
    """every condition generate() refuses, alone: name -> spec.  The order is the order of the checks as they stood"""
    v = {}

    def add(name, kw=None, **spec):
        v[name] = dict(spec, kw=kw or {})

    look, b2 = dict(prompt_lookup_num_tokens=4), dict(num_beams=2)
    add("beams-0", dict(num_beams=0))
    add("beams-17", dict(num_beams=17))
    add("beams-float", dict(num_beams=2.5))
    add("penalty-0", dict(repetition_penalty=0.0))
    add("ngram-neg", dict(no_repeat_ngram_size=-1))
    add("minnew-float", dict(min_new_tokens=2.0))
    add("proc-beams", dict(num_beams=2, no_repeat_ngram_size=2))
    add("weights-int8", dict(decode_weights="int8"))
    add("kv-int4", dict(kv_cache="int4"))
    add("look-16", dict(prompt_lookup_num_tokens=16))
    add("look-ngram-0", dict(look, max_matching_ngram_size=0))
    add("look-beams", dict(look, **b2))
    add("look-sample", dict(look, do_sample=True))
    add("look-proc", dict(look, repetition_penalty=1.2))
    add("look-kv8", dict(look, kv_cache="fp8"))
    add("look-nocache", dict(look, use_cache=False))
    add("look-padded", look, mask="left")
    add("look-rows", look, B=7)
    add("look-fp32-emb", look, dtype="fp32")
    add("temperature-0", dict(do_sample=True, temperature=0.0))
    add("top_p-high", dict(do_sample=True, top_p=1.01))
    add("top_k-neg", dict(do_sample=True, top_k=-2))
    add("mask-shape", mask="short")
    add("mask-dead", mask="dead")
    add("proc-ids-rows", dict(PROC), inputs="ids1")
    add("proc-ids-cols", dict(PROC), inputs="idsw", mask="left")
    add("beams-nret", dict(b2, num_return_sequences=3))
    add("beams-nret-0", dict(b2, num_return_sequences=0))
    add("beams-lp-nan", dict(b2, length_penalty=float("nan")))
    add("beams-vocab", dict(num_beams=16), vocab=24)
    add("beams-sample", dict(b2, do_sample=True))
    add("beams-kv8", dict(b2, kv_cache="fp8"))
    add("beams-padded", b2, mask="left")
    add("beams-fp32", b2, dtype="fp32")
    add("beams-long", b2, N=16000)
    for name, sw in (("w8", dict(decode_weights="fp8")), ("w4", dict(decode_weights="mxfp4")), ("kv8", dict(kv_cache="fp8"))):
        add(f"{name}-fp32", sw, dtype="fp32")
        add(f"{name}-nocache", dict(sw, use_cache=False))
        add(f"{name}-nograph", dict(sw, decode_graph=False))
        add(f"{name}-env", sw, env=True)
        add(f"{name}-N2", sw, N=2)
        add(f"{name}-long", sw, N=16000)
    add("w8-33", dict(decode_weights="fp8"), B=33)
    add("w4-33", dict(decode_weights="mxfp4"), B=33)
    add("w8-beams-rows", dict(decode_weights="fp8", num_beams=4), B=9)
    add("w8-unfused", dict(decode_weights="fp8"), fused=False)
    add("w4-unfused", dict(decode_weights="mxfp4"), fused=False)
    add("look-fp32-ids", look, dtype="fp32", inputs="ids")
    add("look-ids-rows", look, inputs="ids1")
    add("padded-fp32", mask="left", dtype="fp32")
    add("padded-fp32-nograph", dict(decode_graph=False), mask="left", dtype="fp32")
    add("padded-long", mask="left", N=16000)
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


def refusal_cases():
    v = violations()
    c = dict(v)
    for (na, a), (nb, b) in itertools.combinations(v.items(), 2):
        m = _merge(a, b)
        if m is not None and m != a and m != b:
            c[f"{na}+{nb}"] = m
    return c


def run_trace_case(spec, mp):
    tr, res = call(mp, spec)
    return {"log": tr.log, "returns": res}


def run_refusal_case(spec, mp, models):
    """a refused call: the error and the names of what was launched before it; a pair that cancels (use_cache=False next
    to a refusal that names it) runs, to column 3, and records that"""
    tr, res = call(mp, dict(spec, finish=3), models)
    before = [e if isinstance(e, str) else e[0] for e in tr.log if isinstance(e, str) or e[0] not in ("host", "cast")]
    if isinstance(res, dict):
        return dict(res, before=before)
    return {"raises": None}


# ------------------------------------------------------------------------------------------------ the tests --
def _intern(obj, table, index):
    s = json.dumps(obj, separators=(",", ":"))
    if s not in index:
        index[s] = len(table)
        table.append(obj)
    return index[s]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models():
    return {}


def _plain(x):
    return json.loads(json.dumps(x))


@pytest.mark.parametrize("case", list(trace_cases()))
def test_generate_launches_and_reads_what_the_golden_trace_says(case, monkeypatch, golden):
    with monkeypatch.context() as mp:
        got = _plain(run_trace_case(trace_cases()[case], mp))
    want = golden["traces"][case]
    want_log = [golden["entries"][i] for i in want["log"]]
    for i, (g, w) in enumerate(itertools.zip_longest(got["log"], want_log)):
        assert g == w, f"{case}: entry {i} moved:\n  now      {g}\n  expected {w}"
    assert got["returns"] == want["returns"], case


@pytest.mark.parametrize("case,plain", [(k, v) for k, v in SAME_AS.items() if v is not None])
def test_one_beam_and_zero_lookup_tokens_are_the_plain_greedy_call(case, plain, golden):
    assert golden["traces"][case] == golden["traces"][plain]


def test_every_refusal_keeps_its_type_message_and_place(monkeypatch, golden, models):
    cases = refusal_cases()
    assert sorted(cases) == sorted(golden["refusals"])
    for name, spec in cases.items():
        with monkeypatch.context() as mp:
            got = _plain(run_refusal_case(spec, mp, models))
        want = golden["refusals"][name]
        want = {"raises": None} if want is None else dict(golden["messages"][want[0]], before=golden["befores"][want[1]])
        assert got == want, f"{name}:\n  now      {got}\n  expected {want}"


def test_a_refused_call_has_allocated_no_cache_and_copied_no_weight(golden):
    for name, ref in golden["refusals"].items():
        if ref is not None and "unfused" not in golden["messages"][ref[0]]["message"]:     # (found per layer, behind the caches)
            assert set(golden["befores"][ref[1]]) <= {"embedding_fwd"}, name
    kinds = {m["raises"] for m in golden["messages"]}
    assert kinds == {"ValueError"}, kinds


def test_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden["traces"]) == sorted(trace_cases())
    assert os.path.getsize(GOLDEN) < 512 * 1024


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_generate_trace_cpu.py --write   (on the commit the traces are taken from)")
    mp = pytest.MonkeyPatch()
    entries, eidx, traces = [], {}, {}
    for name, spec in trace_cases().items():
        with mp.context() as m:
            got = _plain(run_trace_case(spec, m))
        traces[name] = {"log": [_intern(e, entries, eidx) for e in got["log"]], "returns": got["returns"]}
    messages, midx, befores, bidx, refusals, mods = [], {}, [], {}, {}, {}
    for name, spec in refusal_cases().items():
        with mp.context() as m:
            got = _plain(run_refusal_case(spec, m, mods))
        if got["raises"] is None:
            refusals[name] = None
        else:
            before = got.pop("before")
            refusals[name] = [_intern(got, messages, midx), _intern(before, befores, bidx)]
    dump = lambda o: json.dumps(o, separators=(",", ":"))     # noqa: E731

    def lines(d):
        return "{\n" + ",\n".join(f"{json.dumps(k)}:{dump(val)}" for k, val in d.items()) + "\n}"
    with open(GOLDEN, "w") as f:
        f.write('{"entries":[\n' + ",\n".join(dump(e) for e in entries) + '\n],\n"traces":' + lines(traces)
                + ',\n"messages":[\n' + ",\n".join(dump(e) for e in messages) + '\n],\n"befores":' + dump(befores)
                + ',\n"refusals":' + lines(refusals) + "\n}\n")
    print(f"wrote {len(traces)} traces ({len(entries)} distinct entries), {len(refusals)} refusals ({len(messages)} distinct "
          f"messages), {os.path.getsize(GOLDEN)} bytes")
