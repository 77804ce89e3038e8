"""CPU: classifier-free guidance -- the rule of include/macaw_hip.h as restated in tests/cfg_ref.py against the installed
transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor and on hand-made rows, the ABI and the resources of the new
kernel, the public arguments and every refusal, and what generate(guidance_scale=) launches on the recorders of
tests/test_generate_trace_cpu.py."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import cfg_ref as R
import test_generate_trace_cpu as T
import test_logprobs_cpu as TL

from macaw_llm_amd import engine as eng
from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

LLVM_TOOLS = all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objcopy", "llvm-readelf"))
INF, NAN = float("inf"), float("nan")


# --------------------------------------------------------------------------------------- 1. the restatement --
@pytest.mark.parametrize("V", [2, 40, 1025])
@pytest.mark.parametrize("s", [0.0, 0.5, 1.5, 7.5])
def test_restatement_is_hf_unbatched_cfg_within_its_fp32_roundings(V, s):
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor as HF
    g = torch.Generator().manual_seed(1000 * V + int(10 * s))
    B = 3
    c, u = torch.randn((B, V), generator=g) * 4.0, torch.randn((B, V), generator=g) * 4.0
    proc = HF(s, model=None)
    proc.get_unconditional_logits = lambda input_ids: u[:, None, :]      # [B, 1, V]: HF takes logits[:, -1]
    hf = proc(None, c.clone()).double().numpy()
    ref = R.combine(torch.cat([c, u]), V, B, s)
    checked = 0
    for b in range(B):
        bound = R.hf_bound(c[b], u[b], s)
        err = np.abs(hf[b] - ref[b])
        print(f"V={V} s={s} b={b}: largest |hf - ref| / bound = {(err / bound).max():.3g}, bound <= {bound.max():.3g}")
        assert (err <= bound).all(), (V, s, b, float((err / bound).max()))
        top2 = np.sort(ref[b])[-2:]
        if top2[1] - top2[0] > 2 * bound.max():
            assert int(np.argmax(hf[b])) == int(np.argmax(ref[b]))
            checked += 1
    assert checked or V == 2                                             # (the gaps of these rows are far above the bound)


def test_restatement_follows_rule_3_and_4_on_hand_made_rows():
    ln = np.log
    # finite rows: g = lu + s (lc - lu) of the two log-softmaxes; s = 1 is log_softmax(c), s = 0 is log_softmax(u)
    c, u = [0.0, ln(3.0)], [ln(3.0), 0.0]
    assert np.allclose(R.combine_row(c, u, 1.0), [ln(0.25), ln(0.75)], rtol=0, atol=1e-15)
    assert np.allclose(R.combine_row(c, u, 0.0), [ln(0.75), ln(0.25)], rtol=0, atol=1e-15)
    assert np.allclose(R.combine_row(c, u, 2.0), [2 * ln(0.25) - ln(0.75), 2 * ln(0.75) - ln(0.25)], rtol=0, atol=1e-15)
    # a masked conditional column stays masked; a column the negative prompt rules out is not guided: g = lc there
    g = R.combine_row([0.0, -INF, 0.0, 0.0], [0.0, 0.0, -INF, 0.0], 3.0)
    lc = R.row_lp64([0.0, -INF, 0.0, 0.0])
    assert g[1] == -INF and g[2] == lc[2] == ln(1 / 3)
    assert np.allclose(g[[0, 3]], ln(1 / 3), rtol=0, atol=1e-15)         # (lc == lu there: the scale changes nothing)
    both = R.combine_row([1.0, -INF, 2.0], [1.0, -INF, 0.0], 1.5)
    assert both[1] == -INF and np.isfinite(both[[0, 2]]).all()
    # NaN propagates from either row, column by column; -inf in c wins over NaN in u (rule 3 first)
    g = R.combine_row([0.0, NAN, 0.0, -INF], [0.0, 0.0, NAN, NAN], 1.5)
    assert np.isfinite(g[0]) and np.isnan(g[1]) and np.isnan(g[2]) and g[3] == -INF
    # a degenerate row is all NaN: c degenerate -> every column NaN; u degenerate -> NaN except where c is masked
    assert np.isnan(R.combine_row([0.0, INF, -INF], [0.0, 1.0, 2.0], 1.5)).all()
    assert np.isnan(R.combine_row([-INF, -INF], [0.0, 1.0], 1.5)).all()
    g = R.combine_row([0.0, -INF, 1.0], [-INF, -INF, -INF], 1.5)
    assert np.isnan(g[0]) and g[1] == -INF and np.isnan(g[2])
    # s is the fp32 value; one rounding to each type, ties to even
    # (the third value rounds to -1.0 when it goes through fp32 first: two roundings)
    assert R.round_to([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -30)], "bfloat16").tolist() == \
        [1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7)]
    assert R.round_to([1.0 + 2.0 ** -11, 65520.0, NAN, -INF], "float16").tolist()[:2] == [1.0, INF]
    x = (torch.randn(257, generator=torch.Generator().manual_seed(3)) * 3).float()    # from fp32, torch's rounding is single too
    assert np.array_equal(R.round_to(x.double().numpy(), "bfloat16"), x.to(torch.bfloat16).double().numpy())
    # the bound: equal patterns are required
    assert R.within([-1.0, -INF, NAN], [-1.0, -INF, NAN], 1.5, "float32") == (True, 0.0)
    assert not R.within([-1.0, -INF], [-1.0, NAN], 1.5, "float32")[0]
    assert R.within([-10.0 + 3e-6], [-10.0], 1.5, "float32")[0] and not R.within([-10.0 + 6e-6], [-10.0], 1.5, "float32")[0]
    assert R.within([-10.0 + 0.03], [-10.0], 0.0, "bfloat16")[0] and not R.within([-10.0 + 0.05], [-10.0], 0.0, "bfloat16")[0]


# ------------------------------------------------------------------------------------------------ 2. the ABI --
def test_header_declares_the_entry_point_states_the_rule_and_keeps_abi_11():
    src = open(HEADER).read()
    m = re.search(r"^int mk_cfg_combine\((.*?)\);", src, flags=re.M | re.S)
    assert m, "mk_cfg_combine is not declared in include/macaw_hip.h"
    assert len(m.group(1).split(",")) == len(L.SIGNATURES["mk_cfg_combine"]) == 7
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == 11 == L.ABI_VERSION
    for phrase in ("Classifier-free guidance", "g = lu + s * (lc - lu)", "Where lc or lu is -inf, g = lc", "NaN propagates",
                   "rounded ONCE", "Rows [B, 2B)"):
        assert phrase in src, phrase
    from macaw_llm_amd import build
    assert "cfg.hip" in build.SOURCES
    assert "asm" not in open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "cfg.hip")).read()       # plain HIP only


def test_the_library_exports_it_and_bad_arguments_return_minus_one():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    assert lib.mk_abi_version() == 11
    assert lib.mk_cfg_combine(*[None if t is L._vp else t(0) for t in L.SIGNATURES["mk_cfg_combine"]]) == -1
    fake = 4096                                                          # never dereferenced: every call below is refused

    def cc(logits=fake, ld=40, V=40, B=2, scale=1.5, dtype=L.MK_BF16):
        return lib.mk_cfg_combine(logits, ld, V, B, scale, dtype, None)

    for bad in (dict(logits=None), dict(B=0), dict(B=-1), dict(V=0), dict(ld=39), dict(scale=INF), dict(scale=-INF),
                dict(scale=NAN), dict(dtype=L.MK_FP8), dict(dtype=7), dict(dtype=-1)):
        assert cc(**bad) == -1, bad
    assert "mk_cfg_combine" in inspect.getsource(ops.cfg_combine)
    with pytest.raises(L.MacawHipError, match=r"cfg_combine: logits \(3, 8\)"):
        ops.cfg_combine(torch.zeros((3, 8)), 8, 2, 1.5)


@pytest.mark.skipif(not (LLVM_TOOLS and os.path.exists(kr.LIB)),
                    reason="needs the built library and ROCm's llvm-objcopy / llvm-readelf")
def test_the_kernel_has_no_spill_and_no_scratch():
    from macaw_llm_amd import build
    build.build()
    ks = {k: v for k, v in kr.kernels().items() if "cfg_combine_kernel" in k}
    assert len(ks) == 3, sorted(ks)                                      # bf16, fp16, fp32 (c++filt leaves the 16-bit names)
    for k, v in ks.items():
        assert v["vgpr_count"] <= 128, (k, v)                            # 1024 threads: 4 waves per SIMD need <= 128
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (k, v)


# ------------------------------------------------------------------------------ 3. public arguments, refusals --
NEW = dict(guidance_scale=None, negative_prompt_ids=None, negative_prompt_attention_mask=None, negative_inputs_embeds=None)


def test_generate_and_set_guidance_carry_the_new_arguments():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    for k, v in NEW.items():
        assert p[k].default is v and p[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, k
    p = inspect.signature(Mo.MM_LLMs.set_guidance).parameters
    assert {k: p[k].default for k in p} == dict(guidance_scale=1.0)
    assert Mo.GUIDANCE[0] == 1.0
    try:
        Mo.MM_LLMs.set_guidance(2.0)
        assert Mo.GUIDANCE[0] == 2.0
        for bad in (INF, NAN, "2", True, [2.0]):
            with pytest.raises(ValueError, match="set_guidance: guidance_scale must be"):
                Mo.MM_LLMs.set_guidance(bad)
        assert Mo.GUIDANCE[0] == 2.0                                     # a refused call changes nothing
        Mo.MM_LLMs.set_guidance(0)
        assert Mo.GUIDANCE[0] == 0.0
    finally:
        Mo.MM_LLMs.set_guidance()
    assert Mo.GUIDANCE[0] == 1.0


def test_set_guidance_reaches_generate_through_forward_only_when_it_is_on(monkeypatch):
    seen = []

    class LLM:
        _lora = None

        class model:
            class embed_tokens:
                weight = torch.arange(20.0).view(10, 2)

        def generate(self, **kw):
            seen.append(kw)
            return "ids"

    class Fake:
        llm = LLM()

        def _param_dtype(self):
            return torch.bfloat16

        def prepare_inputs_for_generation(self, inputs):
            return "emb", "extended mask", None
    monkeypatch.setattr(ops, "embedding_fwd", lambda table, ids, out=None: table[ids])
    inputs = {"inference": True, "input_ids": torch.tensor([[1, 4, 2], [3, 3, 0]]), "attention_mask": "text mask"}
    try:
        assert Mo.MM_LLMs.forward(Fake(), inputs) == "ids"
        assert not set(NEW) & set(seen[-1])                              # off: exactly the call without it
        Mo.MM_LLMs.set_guidance(2.0)
        Mo.MM_LLMs.forward(Fake(), inputs)
        kw = seen[-1]
        assert kw["guidance_scale"] == 2.0 and kw["negative_prompt_attention_mask"] is None and kw["attention_mask"] is None
        assert kw["negative_inputs_embeds"].tolist() == [[[2, 3], [8, 9], [4, 5]], [[6, 7], [6, 7], [0, 1]]]
        assert "negative_prompt_ids" not in kw
        Mo.MM_LLMs.set_generate_mask(True)
        Mo.MM_LLMs.forward(Fake(), inputs)
        assert seen[-1]["negative_prompt_attention_mask"] == "text mask" and seen[-1]["attention_mask"] == "extended mask"
        Mo.MM_LLMs.set_guidance()
        Mo.MM_LLMs.forward(Fake(), inputs)
        assert not set(NEW) & set(seen[-1])
    finally:
        Mo.MM_LLMs.set_guidance()
        Mo.MM_LLMs.set_generate_mask(False)


def _generate(**kw):
    return Mo.LlamaForCausalLM.generate(TL._NoModel(), inputs_embeds=torch.zeros(1, 2, 4, dtype=torch.bfloat16), **kw)


def test_refusals_of_the_arguments_alone_raise_before_the_model_is_touched():
    neg = dict(negative_inputs_embeds=torch.zeros(1, 3, 4, dtype=torch.bfloat16))
    for bad in (INF, -INF, NAN, "1.5", True, [1.5]):
        with pytest.raises(ValueError, match="generate: guidance_scale must be None or a finite number"):
            _generate(guidance_scale=bad, **neg)
    with pytest.raises(ValueError, match=r"guidance_scale=1.5\) without a negative prompt.*not built"):
        _generate(guidance_scale=1.5)
    with pytest.raises(ValueError, match="both negative_prompt_ids and negative_inputs_embeds"):
        _generate(guidance_scale=1.5, negative_prompt_ids=torch.zeros(1, 3, dtype=torch.long), **neg)
    with pytest.raises(ValueError, match=r"guidance_scale=1.5\) with num_beams=2.*not built"):
        _generate(guidance_scale=1.5, num_beams=2, **neg)
    with pytest.raises(ValueError, match=r"guidance_scale=1.5\) with prompt_lookup_num_tokens=4.*not built"):
        _generate(guidance_scale=1.5, prompt_lookup_num_tokens=4, **neg)
    with pytest.raises(ValueError, match="num_beams must be"):           # the existing refusals come first, with their text
        _generate(guidance_scale=INF, num_beams=0)
    # off: the negative prompt is ignored, whatever it is; on and valid: past the checks
    for kw in (dict(), dict(guidance_scale=1.0), dict(guidance_scale=1), dict(guidance_scale=None, **neg),
               dict(guidance_scale=1.0, negative_prompt_ids="x", negative_inputs_embeds="y", num_beams=2),
               dict(guidance_scale=1.0, prompt_lookup_num_tokens=4), dict(guidance_scale=1.5, **neg),
               dict(guidance_scale=0.0, **neg), dict(guidance_scale=-1, negative_prompt_ids=torch.zeros(1, 3, dtype=torch.long)),
               dict(guidance_scale=1.5, do_sample=True, seed=1, repetition_penalty=1.2, return_logprobs=True, **neg)):
        with pytest.raises(TL._PastTheChecks):
            _generate(**kw)


def _trace(mp, dtype="bf16"):
    lm = T.make_model(dtype)
    return lm, T.GenTrace(mp, lm, T.Script(3, 2))


def _emb(S, dtype=torch.bfloat16, B=2, D=T.D):
    return torch.zeros((B, S, D), dtype=dtype)


def test_refusals_that_need_the_shapes_raise_on_cpu_tensors_before_any_launch(monkeypatch):
    f32 = torch.float32
    cases = [
        (dict(negative_inputs_embeds=_emb(3, B=3)), "bf16", r"negative prompt should be \[2, Sn >= 1, 128\].*\(3, 3, 128\)"),
        (dict(negative_inputs_embeds=_emb(3, D=64)), "bf16", r"negative prompt should be \[2, Sn >= 1, 128\].*\(2, 3, 64\)"),
        (dict(negative_inputs_embeds=_emb(3)[0]), "bf16", r"negative prompt should be"),
        (dict(negative_inputs_embeds=_emb(3, torch.float16)), "bf16", r"negative prompt is torch.float16, the prompt torch.bfloat16"),
        (dict(negative_prompt_ids=torch.zeros((3, 4), dtype=torch.long)), "bf16", r"negative_prompt_ids should be \[2, Sn\].*\(3, 4\)"),
        (dict(negative_inputs_embeds=_emb(3), negative_prompt_attention_mask=torch.ones((2, 4))), "bf16",
         r"negative_prompt_attention_mask should be of size \(2, 3\), but is \(2, 4\)"),
        (dict(negative_inputs_embeds=_emb(3), attention_mask=torch.ones((2, 4))), "bf16",
         r"attention_mask should be of size \(2, 5\), but is \(2, 4\)"),
        (dict(negative_inputs_embeds=_emb(3), negative_prompt_attention_mask=torch.tensor([[1, 1, 1], [0, 0, 0]])), "bf16",
         r"sample\(s\) \[3\] have no valid token"),
        # the padded-batch refusal: two lengths, or a padded mask, with fp32 parameters or outside ops.decode_attn_ok
        (dict(negative_inputs_embeds=_emb(3, f32)), "fp32", r"guidance_scale=1.5\) with prompts of two lengths or a padded mask "
         r"and use_cache=True: fp32 parameters.*pass use_cache=False"),
        (dict(negative_inputs_embeds=_emb(5, f32), attention_mask=torch.tensor(T.MASKS["left"])), "fp32",
         r"and use_cache=True: fp32 parameters.*pass use_cache=False"),
        (dict(negative_inputs_embeds=_emb(3), max_new_tokens=16000), "bf16", r"ops.decode_attn_ok is false.*pass use_cache=False"),
        (dict(negative_inputs_embeds=_emb(3), decode_weights="fp8", B=17), "bf16",
         r"decode_weights='fp8'\): 2 x B = 2 x 17 = 34 rows under guidance_scale.*at most 32"),
    ]
    for kw, dtype, match in cases:
        kw = dict(kw)
        B = kw.pop("B", 2)
        if B != 2:
            kw["negative_inputs_embeds"] = _emb(3, B=B)
        with monkeypatch.context() as mp:
            lm, tr = _trace(mp, dtype)
            with pytest.raises(ValueError, match=match):
                lm.generate(inputs_embeds=_emb(T.S0, T.DTYPES[dtype], B=B), eos_token_id=T.EOS, pad_token_id=T.PAD,
                            guidance_scale=1.5, **dict(dict(max_new_tokens=6), **kw))
            tr.quiet += 1
            assert [e for e in tr.log if not (isinstance(e, list) and e[0] == "host")] == [], (match, tr.log)
    # the same shapes run where the refusal points to, and equal lengths need no per-sample kernels: fp32 takes them
    for kw in (dict(negative_inputs_embeds=_emb(3, f32), use_cache=False), dict(negative_inputs_embeds=_emb(T.S0, f32))):
        with monkeypatch.context() as mp:
            lm, tr = _trace(mp, "fp32")
            mp.setattr(ops, "cfg_combine", lambda logits, V, B, scale: logits[:B])
            out = lm.generate(inputs_embeds=_emb(T.S0, f32), max_new_tokens=6, eos_token_id=T.EOS, pad_token_id=T.PAD,
                              guidance_scale=1.5, **kw)
            assert tuple(out.shape) == (2, 4)


# ----------------------------------------------------------------------------------------- 4. the launch trace --
def _call(mp, spec, kw):
    """T.call with recorders for cfg_combine and the two log-probability ops -> (log, result)"""
    real = T.GenTrace

    def make(mp_, lm, script):
        tr = real(mp_, lm, script)
        TL._recorders(tr, mp_)
        sig = inspect.signature(ops.cfg_combine)

        def cfg_combine(*args, **kws):
            a = sig.bind(*args, **kws)
            a = dict(a.arguments)
            tr.quiet += 1
            try:
                tr.log.append(["cfg_combine"] + [tr.item(v) for v in a.values()])
                return a["logits"][:a["B"]]
            finally:
                tr.quiet -= 1
        mp_.setattr(ops, "cfg_combine", cfg_combine)
        return tr
    mp.setattr(T, "GenTrace", make)
    spec = dict(spec, kw=dict(spec.get("kw", {}), **kw))
    tr, res = T.call(mp, spec)
    return T._plain(tr.log), res


def _name(e):
    return e if isinstance(e, str) else e[0]


def _arg(e, where, name):
    return dict(zip(inspect.signature(getattr(where, e[0])).parameters, e[1:]))[name]


def _shape(item):
    return [int(v) for v in re.match(r"b\d+\[([\d,]*)\]", item).group(1).split(",")]


def _guided(S_neg, dtype="bf16", **kw):
    return dict(guidance_scale=1.5, negative_inputs_embeds=_emb(S_neg, T.DTYPES[dtype]), **kw)


GRAPH_CASES = {"two-lengths": (3, {}, {}), "equal": (T.S0, {}, {}), "proc": (3, dict(inputs="both"), T.PROC),
               "sample+kv8": (3, {}, dict(T.SAMPLE, kv_cache="fp8")), "w8": (7, {}, dict(decode_weights="fp8")),
               "left+logprobs": (3, dict(mask="left"), dict(return_logprobs=True, top_logprobs=3))}


@pytest.mark.parametrize("case", list(GRAPH_CASES))
def test_graph_loop_runs_2b_rows_combines_behind_the_lm_head_and_emits_b(monkeypatch, case):
    S_neg, spec, kw = GRAPH_CASES[case]
    B, R_ = T.B0, 2 * T.B0
    with monkeypatch.context() as mp:
        log, res = _call(mp, dict(spec, N=12, finish=10), _guided(S_neg, **kw))
    assert not isinstance(res, dict), res
    padded = S_neg != T.S0 or "mask" in spec
    # the layers and the lm_head see 2B rows, in the prefill and in every step; a padded batch runs the ragged path
    layers = [e for e in log if _name(e) == "llama_layer_cached"]
    assert layers and all(_arg(e, eng, "B") == R_ for e in layers)
    assert all((_arg(e, eng, "ragged") is not None) == padded for e in layers)
    heads = [e for e in log if _name(e) == "_stream_linear" and _arg(e, eng, "W") == "head"]
    assert heads and all(_shape(_arg(e, eng, "x")) == [R_, T.D] for e in heads)
    # per token: lm_head -> cfg_combine -> (logits_process) -> emit -> (decode_emit_logprobs), on one buffer of logits
    emits = ("decode_emit", "decode_emit_sample")
    at = [i for i, e in enumerate(log) if _name(e) == "cfg_combine"]
    assert len(at) == len(heads) == len([e for e in log if _name(e) in emits])
    for i in at:
        assert log[i - 1] in heads and log[i][2:] == [T.V, B, 1.5] and _shape(log[i][1]) == [R_, T.V]
        j = i + 1
        if "repetition_penalty" in kw:
            assert _name(log[j]) == "logits_process" and _shape(_arg(log[j], ops, "logits")) == [B, T.V]
            assert _shape(_arg(log[j], ops, "out")) == [B, 12] and _shape(_arg(log[j], ops, "prompt"))[0] == B
            j += 1
        assert _name(log[j]) in emits
        lg = _arg(log[j], ops, "logits")
        assert _shape(lg) == [B, T.V] and lg.split("[")[0] == log[i][1].split("[")[0]       # the view of rows [0, B)
        assert _shape(_arg(log[j], ops, "tok")) == [B] and _shape(_arg(log[j], ops, "done")) == [B]
        assert _shape(_arg(log[j], ops, "out")) == [B, 12]
        if "return_logprobs" in kw:
            assert _name(log[j + 1]) == "decode_emit_logprobs" and log[j + 1][1] == lg
    # the captured step: two gathers of the B tokens into the halves of one [2B, D] buffer, the layers, the head, the
    # combine, the emit -- and no host read
    lo, hi = log.index("capture{"), log.index("}")
    inside = log[lo + 1:hi]
    names = [_name(e) for e in inside]
    assert "host" not in names and names[:2] == ["embedding_fwd", "embedding_fwd"] and names.count("cfg_combine") == 1
    g0, g1 = inside[0], inside[1]
    assert _shape(_arg(g0, ops, "ids")) == [B] and _arg(g0, ops, "ids").split("=")[0] == _arg(g1, ops, "ids").split("=")[0]
    o0, o1 = _arg(g0, ops, "out"), _arg(g1, ops, "out")
    assert _shape(o0) == _shape(o1) == [B, T.D] and o0.split("[")[0] == o1.split("[")[0] and o1.endswith(f"o{B * T.D}")
    assert names.index("_stream_linear", names.index("cfg_combine") - 1) == names.index("cfg_combine") - 1
    allowed = {"embedding_fwd", "llama_layer_cached", "_stream_linear", "cfg_combine", "logits_process", "decode_emit",
               "decode_emit_sample", "decode_emit_logprobs"}
    assert set(names) <= allowed, set(names) - allowed
    # the host's work per token stays one replay, the flags every 8 steps
    tail = [e for e in log[hi + 1:] if _name(e) in ("replay", "host")]
    assert [_name(e) for e in tail[:9]] == ["replay"] * 8 + ["host"]
    ids = res[0]
    assert ids[0][0] == B and ids[1] == "int64"


EAGER_CASES = {"nograph-two-lengths": (3, "bf16", {}, dict(decode_graph=False)),
               "nograph-equal": (T.S0, "bf16", {}, dict(decode_graph=False)),
               "fp32-equal": (T.S0, "fp32", {}, {}),
               "nocache-fp32": (3, "fp32", {}, dict(use_cache=False)),
               "nocache-proc-sample": (7, "bf16", dict(inputs="both"), dict(T.PROC, **T.SAMPLE, use_cache=False)),
               "nocache-hole-logprobs": (T.S0, "bf16", dict(mask="hole"), dict(use_cache=False, return_logprobs=True, top_logprobs=2))}


@pytest.mark.parametrize("case", list(EAGER_CASES))
def test_eager_loops_combine_between_the_lm_head_and_the_selection(monkeypatch, case):
    S_neg, dtype, spec, kw = EAGER_CASES[case]
    B, R_ = T.B0, 2 * T.B0
    with monkeypatch.context() as mp:
        log, res = _call(mp, dict(spec, N=6, finish=3, dtype=dtype), _guided(S_neg, dtype, **kw))
    assert not isinstance(res, dict), res
    names = [_name(e) for e in log]
    sel = [i for i, n in enumerate(names) if n in ("argmax_rows", "sample_rows")]
    at = [i for i, n in enumerate(names) if n == "cfg_combine"]
    assert len(sel) == len(at) == res[0][0][1] == 4
    for i, j in zip(at, sel):
        assert names[i - 1] in ("_stream_linear", "linear_fwd") and _shape(log[i][1]) == [R_, T.V] and log[i][2:] == [T.V, B, 1.5]
        assert j == i + (2 if "repetition_penalty" in kw else 1)
        assert _shape(_arg(log[j], ops, "x")) == [B, T.V]
        if "return_logprobs" in kw:
            assert names[j + 1] == "token_logprobs" and _shape(log[j + 1][1]) == [B, T.V]
    if kw.get("use_cache") is False:                                     # 2B prefixes, one column longer per token
        models = [e for e in log if _name(e) == "model"]
        S = max(S_neg, T.S0)
        assert [_shape(e[1]) for e in models] == [[R_, S + t, T.D] for t in range(4)]
        padded = S_neg != T.S0 or "mask" in spec
        assert all((e[2] is not None) == padded for e in models)
        assert "llama_layer_cached" not in names
    else:
        layers = [e for e in log if _name(e) == "llama_layer_cached"]
        assert layers and all(_arg(e, eng, "B") == R_ for e in layers)
        step = [e for e in log if _name(e) == "embedding_fwd" and _arg(e, ops, "out") is not None]
        assert len(step) == 2 * 3 and all(_shape(_arg(e, ops, "ids")) == [B] for e in step)
    assert res[0][0][0] == B


@pytest.mark.parametrize("mode", ["graph", "nograph", "nocache"])
@pytest.mark.parametrize("scale", [None, 1.0, 1])
def test_the_defaults_launch_read_and_allocate_what_the_plain_call_does(monkeypatch, mode, scale):
    def boom(*a, **k):
        raise AssertionError("reached with guidance off")
    kw = {"graph": {}, "nograph": dict(decode_graph=False), "nocache": dict(use_cache=False)}[mode]
    with monkeypatch.context() as mp:
        plain, res0 = TL._call(mp, dict(N=12, finish=3, kw=kw))
    with monkeypatch.context() as mp:
        mp.setattr(Mo, "_guided_batch", boom)
        mp.setattr(ops, "cfg_combine", boom)
        got, res = TL._call(mp, dict(N=12, finish=3, kw=dict(kw, guidance_scale=scale, negative_inputs_embeds=_emb(3),
                                                             negative_prompt_attention_mask="ignored")))
    assert got == plain and res == res0
