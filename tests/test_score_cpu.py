"""CPU: the surface of LlamaForCausalLM.score() -- engine.score_layout against the restatement of tests/score_ref.py, the
header, the ctypes prototype, the public signatures, every refusal that the arguments alone decide, and the register
budget of the two kernels of mk_score_attn."""
import inspect
import os
import re
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402
import score_ref as SR  # noqa: E402

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")

RAGGED = [[[5, 6, 7, 8, 9, 10], [11], [12, 13, 14, 15]], [[16, 17], [18, 19, 20, 21, 22, 23]], [[1, 2, 3, 4, 5], [6, 7, 8]]]
CASES = {
    "ragged counts and lengths, a length-1 option, an absent option": RAGGED,
    "all options of length 1 (F = 0)": [[[3], [4]], [[5]]],
    "one prompt, one option": [[[9, 8, 7]]],
    "a single token": [[[2]]],
}


# -------------------------------------------------------------------------------------------------- layout --
@pytest.mark.parametrize("name", list(CASES))
def test_score_layout_is_the_restated_layout(name):
    conts = CASES[name]
    want = SR.layout(conts)
    got = eng.score_layout(continuations=conts, B=len(conts), V=107)
    assert (got.n, got.F, got.Lc) == (want["n"], want["F"], want["Lc"])
    assert got.fed.dtype == torch.int64 and got.fed.tolist() == want["fed"] and got.fed.numel() == len(conts) * got.n * got.F
    assert got.lens.dtype == torch.int32 and got.lens.tolist() == want["lens"]
    assert got.targets.dtype == torch.int64 and got.targets.tolist() == want["targets"]
    assert got.lengths.dtype == torch.int64 and got.lengths.tolist() == want["lengths"]
    assert all(t.device.type == "cpu" and t.is_contiguous() for t in (got.fed, got.lens, got.targets, got.lengths))
    assert SR.fed_rows(want["lens"], want["F"]) == want["lens"]          # the layout's counts are inside the kernel's clamp


def test_the_ragged_case_holds_what_its_name_says():
    lay = eng.score_layout(continuations=RAGGED)
    assert lay.lengths.tolist() == [[6, 1, 4], [2, 6, 0], [5, 3, 0]] and lay.lens.tolist() == [5, 0, 3, 1, 5, 0, 4, 2, 0]
    assert lay.F == 5 and lay.fed.view(3, 3, 5)[0, 1].tolist() == [0] * 5          # a length-1 option feeds nothing
    assert lay.fed.view(3, 3, 5)[1, 2].tolist() == [0] * 5                           # nor does an absent one
    assert lay.fed.view(3, 3, 5)[0, 2].tolist() == [12, 13, 14, 0, 0]                # the last token is scored, never fed
    f0 = eng.score_layout(continuations=CASES["all options of length 1 (F = 0)"])
    assert f0.F == 0 and f0.fed.numel() == 0 and f0.lens.tolist() == [0, 0, 0, 0] and f0.lengths.tolist() == [[1, 1], [1, 0]]


def test_the_tensor_form_equals_the_list_form_whatever_lies_behind_an_options_end():
    a = eng.score_layout(continuations=RAGGED, V=107)
    ids = a.targets.clone()
    junk = torch.arange(a.Lc) >= a.lengths[..., None]
    ids[junk] = -1                                                   # pad behind the end, as generate() leaves it
    for lengths in (a.lengths, a.lengths.to(torch.int32)):
        b = eng.score_layout(continuation_ids=ids, continuation_lengths=lengths, V=107)
        assert (b.n, b.F, b.Lc) == (a.n, a.F, a.Lc)
        for x, y in zip(a[:4], b[:4]):
            assert x.dtype == y.dtype and torch.equal(x, y)
    # lengths are clamped into [0, Lc], fed ids into [0, V)
    c = eng.score_layout(continuation_ids=torch.tensor([[[5, 300, 7]]]), continuation_lengths=torch.tensor([[9]]), V=107)
    assert c.lengths.tolist() == [[3]] and c.lens.tolist() == [2] and c.fed.tolist() == [5, 106]
    assert c.targets.tolist() == [[[5, 300, 7]]]
    d = eng.score_layout(continuation_ids=torch.tensor([[[5, 6, 7]]]), continuation_lengths=torch.tensor([[-2]]))
    assert d.lengths.tolist() == [[0]] and d.lens.tolist() == [0] and d.targets.tolist() == [[[0, 0, 0]]]


def test_score_layout_refuses_by_name():
    ids, lens = torch.zeros((2, 2, 3), dtype=torch.int64), torch.ones((2, 2), dtype=torch.int64)
    for kw, match in (
            (dict(), "exactly one of continuations .* neither"),
            (dict(continuations=[[[1]]], continuation_ids=ids[:1], continuation_lengths=lens[:1]), "exactly one .* both"),
            (dict(continuations=[[[1]]], continuation_lengths=lens), "continuation_lengths goes with continuation_ids"),
            (dict(continuations=[[[1]], [[2]]], B=3), "2 lists of continuations for a batch of 3"),
            (dict(continuations=[[[1]], []]), "at least one continuation"),
            (dict(continuations=[]), "at least one continuation"),
            (dict(continuations=[[[1], []]]), r"empty continuation\(s\) at \(prompt, option\) \[\(0, 1\)\]"),
            (dict(continuations=[[[1, 107]]], V=107), r"token id\(s\) \[107\] outside \[0, 107\)"),
            (dict(continuations=[[[1, -1]]], V=107), r"token id\(s\) \[-1\] outside"),
            (dict(continuations=[[[1]] * 33]), "33 continuations for one prompt; at most 32"),
            (dict(continuation_ids=ids), "needs continuation_lengths"),
            (dict(continuation_ids=ids.int(), continuation_lengths=lens), r"int64 \[B, n, Lc >= 1\]"),
            (dict(continuation_ids=ids[0], continuation_lengths=lens), r"int64 \[B, n, Lc >= 1\]"),
            (dict(continuation_ids=ids, continuation_lengths=lens[:1]), "continuation_lengths should be"),
            (dict(continuation_ids=ids, continuation_lengths=lens.float()), "continuation_lengths should be"),
            (dict(continuation_ids=ids, continuation_lengths=lens, B=3), "for 2 prompts and a batch of 3"),
            (dict(continuation_ids=torch.zeros((1, 33, 2), dtype=torch.int64),
                  continuation_lengths=torch.ones((1, 33), dtype=torch.int64)), "33 continuations per prompt")):
        with pytest.raises(ValueError, match=match):
            eng.score_layout(**kw)
    assert eng.score_layout(continuations=[[[1]] * 32]).n == 32


# ------------------------------------------------------------------------------------------------ refusals --
def _fake_lm(dtype=torch.bfloat16, heads=2, hidden=128, V=107, table=64):
    """what score() reads of the model before it allocates: shapes, dtype, the head count, the table's length"""
    w = types.SimpleNamespace
    layer = w(self_attn=w(num_heads=heads))
    return w(model=w(embed_tokens=w(weight=torch.zeros((V, hidden), dtype=dtype)), layers=[layer], norm=w(variance_epsilon=1e-6)),
             lm_head=w(weight=torch.zeros((V, hidden), dtype=dtype)), config=w(max_position_embeddings=table))


def _score(lm=None, **kw):
    kw.setdefault("input_ids", torch.ones((2, 5), dtype=torch.long))
    return Mo.LlamaForCausalLM.score(lm or _fake_lm(), **kw)


def test_score_refuses_what_the_arguments_alone_decide_before_it_touches_the_device():
    good = [[[1, 2]], [[3]]]
    for kw, match in (
            (dict(), "exactly one of continuations"),
            (dict(continuations=good, continuation_ids=torch.zeros((2, 1, 2), dtype=torch.int64),
                  continuation_lengths=torch.ones((2, 1), dtype=torch.int64)), "exactly one of continuations"),
            (dict(continuations=good, input_ids=None), "exactly one of inputs_embeds and input_ids"),
            (dict(continuations=good, inputs_embeds=torch.zeros((2, 5, 128))), "exactly one of inputs_embeds and input_ids"),
            (dict(continuations=good[:1]), "1 lists of continuations for a batch of 2"),
            (dict(continuations=[[[1, 2]], [[]]]), "empty continuation"),
            (dict(continuations=[[[1, 2]], [[107]]]), r"outside \[0, 107\)"),
            (dict(continuations=[[[1]] * 33, [[2]]]), "at most 32"),
            (dict(continuations=good, top_logprobs=21), r"top_logprobs must be an integer in \[0, 20\]"),
            (dict(continuations=good, top_logprobs=-1), "top_logprobs must be"),
            (dict(continuations=good, top_logprobs=True), "top_logprobs must be"),
            (dict(continuations=good, top_logprobs=2.0), "top_logprobs must be"),
            (dict(continuations=[[[1] * 60], [[3]]]), r"prompt\(s\) \[0\]: L_b \+ len = \[65\] positions are beyond the rotary table"),
            (dict(continuation_ids=torch.zeros((2, 1, 60), dtype=torch.int64),
                  continuation_lengths=torch.ones((2, 1), dtype=torch.int64)), "beyond the rotary table"),
            (dict(continuations=good, attention_mask=torch.ones((2, 4))), r"attention_mask should be of size \(2, 5\)"),
            (dict(continuations=good, attention_mask=torch.tensor([[1] * 5, [0] * 5])), "have no valid token")):
        with pytest.raises(ValueError, match=match):
            _score(**kw)
    # a padded prompt leaves room that a full one does not have: L_b counts the valid tokens
    mask = torch.tensor([[0, 0, 1, 1, 1], [1] * 5])
    with pytest.raises(ValueError, match=r"prompt\(s\) \[1\]"):
        _score(continuations=[[[1] * 60], [[1] * 60]], attention_mask=mask, use_cache=False)
    with pytest.raises(ValueError, match=r"use_cache=True: fp32 parameters.*use use_cache=False"):
        _score(_fake_lm(torch.float32), continuations=good)
    with pytest.raises(ValueError, match=r"ops.score_attn_ok is false for head size 48.*use use_cache=False"):
        _score(_fake_lm(heads=2, hidden=96), continuations=good)
    # nothing left to refuse: the call reaches the device check (there is no CPU path)
    for kw in (dict(continuations=good), dict(continuations=good, use_cache=False), dict(continuations=good, top_logprobs=20),
               dict(continuations=[[[1] * 59], [[3]]])):
        with pytest.raises(Mo.MacawHipError, match="HIP device only"):
            _score(**kw)
    with pytest.raises(Mo.MacawHipError, match="HIP device only"):
        _score(_fake_lm(torch.float32), continuations=good, use_cache=False)


# --------------------------------------------------------------------------------------- ABI and signatures --
def test_the_header_declares_mk_score_attn_with_the_bindings_arity_and_states_the_rule():
    src = open(HEADER).read()
    m = re.search(r"\nint mk_score_attn\(([^;]*)\);", src)
    assert m, "include/macaw_hip.h does not declare mk_score_attn"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["q", "k_new", "v_new", "in_bs", "cos_t", "sin_t", "kp", "vp", "p_ld", "p_bs", "kt", "vt", "t_ld", "t_bs",
                     "o", "o_bs", "len", "t_off", "S0", "F", "B", "n", "H", "hd", "scale", "dtype", "stream"]
    import ctypes as C
    kinds = {"void*": C.c_void_p, "int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    want = [kinds[re.sub(r"\bconst\b", "", " ".join(p.split()[:-1])).replace(" ", "")] for p in params]
    assert L.SIGNATURES["mk_score_attn"] == want
    flat = " ".join(src.split())
    for phrase in ("lp[b, j, g] = log_softmax(logits of the model at position L_b + g - 1",
                   "F = (longest option) - 1", "o is exactly zero", "BIT FOR BIT", "len int32 [B * n] ON * THE DEVICE"):
        assert phrase.replace(" * ", " ") in flat.replace(" * ", " "), phrase
    if os.path.exists(L.LIB_PATH):
        assert hasattr(L.load(), "mk_score_attn")


def test_the_public_signatures_and_the_layer_signature_that_must_not_move():
    p = inspect.signature(Mo.LlamaForCausalLM.score).parameters
    assert list(p) == ["self", "inputs_embeds", "input_ids", "continuations", "continuation_ids", "continuation_lengths",
                       "attention_mask", "top_logprobs", "use_cache"]
    assert p["top_logprobs"].default == 0 and p["use_cache"].default is True
    assert Mo.ScoreResult._fields == ("token_logprobs", "lengths", "sums", "top_ids", "top_logprobs")
    assert list(inspect.signature(Mo.MM_LLMs.score).parameters)[:3] == ["self", "inputs", "continuations"]
    assert list(inspect.signature(eng.llama_layer_cached).parameters) == [
        "x2", "B", "Sn", "t0", "kvc", "Tmax", "pos", "cos", "sin", "n_heads", "eps", "wq", "wk", "wv", "wo", "wg", "wu", "wd",
        "ln1", "ln2", "wqkv", "wgu", "t_dev", "w8", "kv8", "ragged", "beam", "spec"]
    assert list(inspect.signature(ops.score_attn).parameters) == [
        "q", "k_new", "v_new", "in_bs", "cos_t", "sin_t", "prompt", "tail", "lens", "t_off", "S0", "B", "n", "H", "hd", "out",
        "scale", "q_off", "k_off", "v_off"]
    for dt in (torch.bfloat16, torch.float16):
        for hd in (16, 32, 64, 128):
            assert ops.score_attn_ok(dt, hd) and ops.score_attn_ok(dt, hd, 65535) and not ops.score_attn_ok(dt, hd, 65536)
    assert not ops.score_attn_ok(torch.float32, 64) and not ops.score_attn_ok(torch.bfloat16, 48)
    assert not ops.score_attn_ok(torch.bfloat16, 64, 0)
    doc = " ".join(Mo.LlamaForCausalLM.score.__doc__.split())
    for phrase in ("lp[b, j, g] = log_softmax(", "use_cache=False", "ops.score_attn", "SCORE_LOGITS_ELEMS // V", "merged copies",
                   "-inf for an absent option", "use use_cache=False"):
        assert phrase in doc, phrase


def test_mm_llms_score_runs_the_towers_once_and_passes_the_mask_under_the_inference_switch():
    seen = []

    class Fake:
        llm = types.SimpleNamespace(score=lambda **kw: seen.append(kw) or "result")

        def _param_dtype(self):
            return torch.bfloat16

        def prepare_inputs_for_generation(self, inputs):
            seen.append("prepare")
            return "emb", "mask", None
    try:
        assert Mo.MM_LLMs.score(Fake(), {"x": 1}, [[[1]]], top_logprobs=3) == "result"
        assert seen == ["prepare", dict(inputs_embeds="emb", continuations=[[[1]]], attention_mask=None, top_logprobs=3)]
        Mo.MM_LLMs.set_generate_mask(True)
        del seen[:]
        Mo.MM_LLMs.score(Fake(), {"x": 1}, continuation_ids="ids", continuation_lengths="lens", use_cache=False)
        assert seen == ["prepare", dict(inputs_embeds="emb", continuations=None, attention_mask="mask", continuation_ids="ids",
                                        continuation_lengths="lens", use_cache=False)]
    finally:
        Mo.MM_LLMs.set_generate_mask(False)


# ---------------------------------------------------------------------------------------- kernel resources --
LLVM_TOOLS = all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objcopy", "llvm-readelf"))


@pytest.mark.skipif(not (LLVM_TOOLS and os.path.exists(kr.LIB)),
                    reason="needs the built library and ROCm's llvm-objcopy / llvm-readelf")
def test_both_score_kernels_exist_for_every_type_and_head_size_without_scratch():
    """the attention kernel is the step body at 512 threads per workgroup = two waves per SIMD: at most 256 VGPRs; neither
    kernel spills or uses scratch"""
    from macaw_llm_amd import build
    build.build()                       # no-op when the stamp matches the sources
    ks = {k: v for k, v in kr.kernels().items() if "score_attn_" in k or "score_append_" in k}
    for ns, f16 in (("e_bf16::", ""), ("e_f16::", "f16_")):
        for hd in (16, 32, 64, 128):
            assert any(k.startswith(f"void {ns}score_attn_{f16}kernel<{hd}, 8>") for k in ks), (ns, hd)
            assert any(k.startswith(f"void {ns}score_append_{f16}kernel<{hd}>") for k in ks), (ns, hd)
    assert len(ks) == 16
    for k, v in ks.items():
        assert v["vgpr_count"] <= 256, (k, v)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
        assert v["max_flat_workgroup_size"] == (512 if "score_attn_" in k else 256), (k, v)
