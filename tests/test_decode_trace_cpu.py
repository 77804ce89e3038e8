"""CPU: the launch sequence of the cached decoder layer (engine.llama_layer_cached) and of generate()'s lm_head, pinned
against tests/golden/decode_launch_trace.json.

Every ops.<launch> the layer reaches is replaced by a recorder that launches nothing: it binds the call to the real
op's signature (so a default and the same value spelled out are one trace), appends [op name, one item per argument]
and returns a meta tensor of the shape and dtype the real op returns.  A tensor argument is recorded as its buffer
(numbered in the order the buffers first appear in the case, so the data flow between the launches is part of the
trace), shape, stride, storage offset and dtype; a scalar as its value.  The predicates that choose between the
launches (ops.decode_linear_ok, ops.decode_linear_fp8_ok, ops.decode_attn_ok, engine.flash_ok) are the real ones.

One argument is recorded in a canonical form: `eps` of decode_linear / decode_linear_fp8 is None unless prologue = 1.
The kernels read it only inside the RMSNorm prologue (csrc/skinny16_parts.inc: `if constexpr (PRO == 1)`), and the callers have always disagreed about what to pass where it is dead (0.0 or the layer's eps).

The file of expected traces was written by `python tests/test_decode_trace_cpu.py --write` on the commit BEFORE the
decode step got its single body and the streamed-linear helper, and must not be regenerated to make a change pass:
a difference is a launch that moved."""
import inspect
import itertools
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":      # run as a script (--write): the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from macaw_llm_amd import engine as eng
from macaw_llm_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_launch_trace.json")
BF, U8, F32, I32 = torch.bfloat16, torch.uint8, torch.float32, torch.int32
TMAX, EPS = 8, 1e-6


def _t(*shape, dtype=BF):
    return torch.empty(shape, dtype=dtype, device="meta")


def _mn(a, N):
    return a["out"] if a.get("out") is not None else _t(a["x"].shape[0], N, dtype=a["x"].dtype)


# what each faked launch returns, from its bound arguments (shapes and dtypes of the real ops in macaw_llm_amd/ops.py)
RETURNS = {
    "rmsnorm_fwd": lambda a: (a["x"] if a["res"] is None else torch.empty_like(a["x"]), torch.empty_like(a["x"]),
                              _t(a["x"].shape[0], dtype=F32)),
    "linear_fwd": lambda a: _mn(a, a["W"].shape[0]),
    "decode_linear": lambda a: _mn(a, a["W"].shape[0]),
    "decode_linear_fp8": lambda a: _mn(a, a["Wq"].shape[0]),
    "swiglu_fwd": lambda a: torch.empty_like(a["g"]),
    "swiglu2d_fwd": lambda a: _t(a["gu"].shape[0], a["cols"], dtype=a["gu"].dtype),
    "rope_": lambda a: a["x"],
    "copy2d": lambda a: a["dst"],
    "gemm_raw": lambda a: a["Cc"],
    "softmax_fwd": lambda a: (a["probs"] if a["probs"] is not None else torch.empty_like(a["scores"]), None),
    "flash_attn_fwd": lambda a: a["o"],
    "kv_quant_append": lambda a: (a["cache"], a["scales"]),
    "decode_step_attn": lambda a: a["out"],
    "decode_step_attn_kv8": lambda a: a["out"],
}


class Trace:
    """the recorders of one case"""

    def __init__(self, monkeypatch):
        self.calls, self.bufs, self.keep = [], {}, []
        for name in RETURNS:
            monkeypatch.setattr(ops, name, self._recorder(name, inspect.signature(getattr(ops, name))))

    def _item(self, v):
        if torch.is_tensor(v):
            key = v.untyped_storage()._cdata
            if key not in self.bufs:
                self.bufs[key] = len(self.bufs)
                self.keep.append(v)             # a freed storage's address could come back as another buffer's
            return {"buf": self.bufs[key], "shape": list(v.shape), "stride": list(v.stride()),
                    "offset": v.storage_offset(), "dtype": str(v.dtype).replace("torch.", "")}
        if isinstance(v, (tuple, list)):
            return [self._item(e) for e in v]
        assert v is None or isinstance(v, (bool, int, float)), v
        return v

    def _recorder(self, name, sig):
        def rec(*args, **kw):
            a = sig.bind(*args, **kw)
            a.apply_defaults()
            a = dict(a.arguments)
            shown = dict(a)
            if name in ("decode_linear", "decode_linear_fp8") and a["prologue"] != 1:
                shown["eps"] = None             # dead outside the RMSNorm prologue: see the module docstring
            self.calls.append([name] + [self._item(v) for v in shown.values()])
            return RETURNS[name](a)
        return rec


# ------------------------------------------------------------------------------------------------- the layer --
# rows and K: prologue form allowed / only the plain form (M > 16) / the prologue forms over the LDS budget / past
# the streamed kernels' 32 rows (a device-position step then takes the general path)
DIMS = {"B2D128": (2, 128, 256), "B20D128": (20, 128, 256), "B8D4096": (8, 4096, 11008), "B40D128": (40, 128, 256)}
CALLS = {"prefill": (5, 0, False), "step": (1, 5, False), "tdev": (1, 5, True)}       # Sn, t0, device position


def layer_cases():
    for st, call, kv, w, dims in itertools.product(("fused", "unfused"), CALLS, ("kv16", "kv8"),
                                                   ("w16", "w8", "w8mixed"), DIMS):
        for hd in ((64, 8) if call == "prefill" and dims == "B2D128" else (64,)):
            case = f"{st}-{call}-{kv}-{w}-{dims}-hd{hd}"
            # a rejected combination launches nothing: once per kind (at B = 2), and fused w8 past 32 rows
            if rejected(case) is None or dims == "B2D128" or (st, call, dims) == ("fused", "tdev", "B40D128"):
                yield case


def run_layer_case(case, monkeypatch):
    """the trace of one llama_layer_cached call, or {"raises": ...} for a combination it rejects"""
    st, call, kv, w, dims, hd = case.split("-")
    B, D, FF = DIMS[dims]
    Sn, t0, dyn = CALLS[call]
    hd = int(hd[2:])
    H, M = D // hd, B * Sn
    tr = Trace(monkeypatch)
    x2 = _t(M, D)
    if st == "fused":
        wqkv, wgu = _t(3 * D, D), _t(2 * FF, D)
        wq, wk, wv, wg, wu = wqkv[:D], wqkv[D:2 * D], wqkv[2 * D:], wgu[:FF], wgu[FF:]
    else:
        wqkv = wgu = None
        wq, wk, wv, wg, wu = _t(D, D), _t(D, D), _t(D, D), _t(FF, D), _t(FF, D)
    wo, wd, ln1, ln2 = _t(D, D), _t(D, FF), _t(D), _t(D)
    kvc = _t(B, TMAX, 2 * D, dtype=U8 if kv == "kv8" else BF)
    kv8 = _t(B, TMAX, 2 * H, dtype=F32) if kv == "kv8" else None
    q8 = lambda N, K: (_t(N, K, dtype=U8), _t(N, dtype=F32))  # noqa: E731
    w8 = {"w16": None, "w8": (q8(3 * D, D), q8(D, D), q8(2 * FF, D), q8(D, FF)),
          "w8mixed": (q8(3 * D, D), None, q8(2 * FF, D), None)}[w]
    pos, cos, sin = _t(M, dtype=I32), _t(TMAX, hd), _t(TMAX, hd)
    t_dev = _t(1, dtype=I32) if dyn else None
    try:
        out = eng.llama_layer_cached(x2, B, Sn, t0, kvc, TMAX, pos, cos, sin, H, EPS, wq, wk, wv, wo, wg, wu, wd, ln1,
                                     ln2, wqkv, wgu, t_dev=t_dev, w8=w8, kv8=kv8)
    except ValueError as e:
        assert tr.calls == [], "a rejected call must not have launched anything"
        return {"raises": "ValueError", "names": [k for k in ("w8", "kv8") if k in str(e)]}
    assert tuple(out.shape) == (M, D) and out.dtype == BF
    return tr.calls + [["return", tr._item(out)]]


def rejected(case):
    """what llama_layer_cached's contract says about the combination: w8 is for the device-position step on fused
    storage with at most 32 rows; an e4m3 cache takes a prefill from 0 or device-position steps"""
    st, call, kv, w, dims, _ = case.split("-")
    if kv == "kv8" and call == "step":
        return ["kv8"]
    if w != "w16" and not (call == "tdev" and st == "fused" and DIMS[dims][0] <= 32):
        return ["w8"]
    return None


# ------------------------------------------------------------------------------------------------ the lm_head --
def logits_cases():
    for layout, head, B in itertools.product(("contiguous", "pitched"), ("w16", "w8"), (2, 20)):
        yield f"logits-{layout}-{head}-B{B}"


def _logits_operands(case):
    _, layout, head, B = case.split("-")
    B, D, V = int(B[1:]), 128, 320
    h_last = _t(B, D) if layout == "contiguous" else _t(B, 2 * D)[:, :D]
    w8_head = (_t(V, D, dtype=U8), _t(V, dtype=F32)) if head == "w8" else None
    return h_last, _t(V, D), _t(D), w8_head


def logits_before(h_last, lm_w, norm_w, w8_head, eps=EPS):
    """generate()'s logits() as it stood before the streamed-linear helper, as a composition of ops calls: the
    reference the helper's use in generate() is held to"""
    if w8_head is not None and h_last.is_contiguous():
        if ops.decode_linear_fp8_ok(h_last, w8_head[0], 1):
            return ops.decode_linear_fp8(h_last, *w8_head, 1, norm_w, eps)
        _, y, _ = ops.rmsnorm_fwd(h_last, norm_w, eps)
        return ops.decode_linear_fp8(y, *w8_head)
    if h_last.is_contiguous() and ops.decode_linear_ok(h_last, lm_w, 1):
        return ops.decode_linear(h_last, lm_w, 1, norm_w, eps)
    _, y, _ = ops.rmsnorm_fwd(h_last, norm_w, eps)
    return ops.linear_fwd(y, lm_w)


def logits_now(h_last, lm_w, norm_w, w8_head, eps=EPS):
    """generate()'s logits() on the helper: the contiguity guard, then the 16-bit fall-through"""
    if h_last.is_contiguous():
        return eng._stream_linear(h_last, lm_w, w8_head, 1, norm_w, eps, None, 0)
    _, y, _ = ops.rmsnorm_fwd(h_last, norm_w, eps)
    return ops.linear_fwd(y, lm_w)


def run_logits_case(case, monkeypatch, fn):
    tr = Trace(monkeypatch)
    out = fn(*_logits_operands(case))
    return tr.calls + [["return", tr._item(out)]]


# ------------------------------------------------------------------------------------------------- the tests --
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _same(got, want, case):
    got = json.loads(json.dumps(got))
    if got != want and isinstance(got, list) and isinstance(want, list):
        for i, (g, w) in enumerate(itertools.zip_longest(got, want)):
            assert g == w, f"{case}: launch {i} moved:\n  now      {g}\n  expected {w}"
    assert got == want, case


@pytest.mark.parametrize("case", list(layer_cases()))
def test_llama_layer_cached_launches_what_the_golden_trace_says(case, monkeypatch, golden):
    got = run_layer_case(case, monkeypatch)
    names = rejected(case)
    if names is not None:
        assert got == {"raises": "ValueError", "names": names}, (case, got)
    else:
        assert isinstance(got, list), (case, got)
    _same(got, golden[case], case)


@pytest.mark.parametrize("case", list(logits_cases()))
def test_logits_reference_composition_matches_the_golden_trace(case, monkeypatch, golden):
    _same(run_logits_case(case, monkeypatch, logits_before), golden[case], case)


@pytest.mark.parametrize("case", list(logits_cases()))
def test_logits_on_the_stream_linear_helper_matches_the_golden_trace(case, monkeypatch, golden):
    if not hasattr(eng, "_stream_linear"):
        pytest.skip("engine._stream_linear is not in this tree (the commit the golden file was written on)")
    _same(run_logits_case(case, monkeypatch, logits_now), golden[case], case)


def test_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted([*layer_cases(), *logits_cases()])
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_generate_reaches_the_lm_head_through_the_helper_behind_its_contiguity_guard():
    """logits_now above restates generate()'s closure.  What generate() itself does is pinned by its launch trace
    (tests/test_generate_trace_cpu.py runs the real generate() on recorders): there every logits row comes from
    engine._stream_linear(rows, lm_head, the e4m3 copy or None, prologue 1, the final norm's weight and eps, no residual,
    0) on contiguous rows, in every mode, and generate() reaches no streamed-linear launch on its own"""
    with open(os.path.join(os.path.dirname(GOLDEN), "generate_launch_trace.json")) as f:
        g = json.load(f)
    heads = [e for e in g["entries"] if e[0] == "_stream_linear"]
    emits = [e for e in g["entries"] if e[0] in ("decode_emit", "decode_emit_sample", "beam_emit", "spec_verify_emit",
                                                 "argmax_rows", "sample_rows")]
    assert heads and len(emits) >= len(heads)
    for name, rows, W, q8, pro, w_ln, eps, residual, FF in heads:
        assert (W, pro, w_ln, residual, FF) == ("head", 1, "norm", None, 0) and eps > 0 and "s[" not in rows
        assert q8 is None or (len(q8) == 2 and "uint8" in q8[0] and "float32" in q8[1])
    assert not [e for e in g["entries"] if e[0] in ("linear_fwd", "rmsnorm_fwd") or "decode_linear" in e[0]]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_decode_trace_cpu.py --write   (on the commit the traces are taken from)")
    mp = pytest.MonkeyPatch()
    out = {}
    for c in layer_cases():
        with mp.context() as m:
            out[c] = run_layer_case(c, m)
    for c in logits_cases():
        with mp.context() as m:
            out[c] = run_logits_case(c, m, logits_before)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items())
                + "\n}\n")
    print(f"wrote {len(out)} traces, {os.path.getsize(GOLDEN)} bytes")
