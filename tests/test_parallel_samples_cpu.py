"""CPU: the surface of generate(num_samples=n) -- the header, the ctypes prototype and the ABI version of
mk_decode_step_attn_shared, the public arguments, MM_LLMs.set_parallel_samples, the refusals that need no model, the
engine's guard, and the register budget of every shipped instantiation of the kernel."""
import inspect
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))
import kernel_resources as kr  # noqa: E402

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")


# --------------------------------------------------------------------------------------- ABI and signatures --
def test_the_header_declares_the_entry_point_with_the_bindings_arity_and_the_abi_stays_11():
    src = open(HEADER).read()
    m = re.search(r"\nint mk_decode_step_attn_shared\(([^;]*)\);", src)
    assert m, "include/macaw_hip.h does not declare mk_decode_step_attn_shared"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 27 and len(L.SIGNATURES["mk_decode_step_attn_shared"]) == 27
    names = [re.sub(r"/\*.*?\*/", "", p).split()[-1].lstrip("*") for p in params]
    assert names == ["q", "k_new", "v_new", "in_bs", "cos_t", "sin_t", "kp", "vp", "p_ld", "p_bs", "kt", "vt", "t_ld", "t_bs",
                     "o", "o_bs", "t_dev", "t_off", "S0", "Tn", "B", "n", "H", "hd", "scale", "dtype", "stream"]
    # pointers, 64-bit strides, 32-bit counts and the float, position by position
    import ctypes as C
    kinds = {"void*": C.c_void_p, "int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    want = [kinds[re.sub(r"\bconst\b", "", " ".join(p.split()[:-1])).replace(" ", "")] for p in params]
    assert L.SIGNATURES["mk_decode_step_attn_shared"] == want
    assert re.search(r"#define MK_ABI_VERSION 11\b", src) and L.ABI_VERSION == 11
    assert "MK_SHARED_ATTN_ROWS" in src
    if os.path.exists(L.LIB_PATH):
        assert L.load().mk_abi_version() == 11 and hasattr(L.load(), "mk_decode_step_attn_shared")


def test_generate_takes_num_samples_as_a_real_parameter_and_the_layer_signature_is_unchanged():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    assert "num_samples" in p and p["num_samples"].default == 1
    assert p["num_samples"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD      # not swallowed by **_
    assert list(inspect.signature(eng.llama_layer_cached).parameters) == [
        "x2", "B", "Sn", "t0", "kvc", "Tmax", "pos", "cos", "sin", "n_heads", "eps", "wq", "wk", "wv", "wo", "wg", "wu", "wd",
        "ln1", "ln2", "wqkv", "wgu", "t_dev", "w8", "kv8", "ragged", "beam", "spec"]
    assert list(inspect.signature(eng._stream_linear).parameters) == ["x", "W", "q8", "pro", "w_ln", "eps", "residual", "FF"]
    assert eng.SharedPrompt._fields == ("prompt", "tail", "n", "S0")
    assert list(inspect.signature(ops.decode_step_attn_shared).parameters) == [
        "q", "k_new", "v_new", "in_bs", "cos_t", "sin_t", "prompt", "tail", "t_dev", "t_off", "S0", "B", "n", "H", "hd", "out",
        "scale", "q_off", "k_off", "v_off"]
    for dt in (torch.bfloat16, torch.float16):
        for hd in (16, 32, 64, 128):
            assert ops.shared_attn_ok(dt, hd, 1) and ops.shared_attn_ok(dt, hd, 32) and not ops.shared_attn_ok(dt, hd, 33)
    assert not ops.shared_attn_ok(torch.float32, 64, 2) and not ops.shared_attn_ok(torch.bfloat16, 48, 2)
    assert not ops.shared_attn_ok(torch.bfloat16, 64, 0)
    doc = " ".join(Mo.LlamaForCausalLM.generate.__doc__.split())
    for phrase in ("num_samples=n in [1, 32]", "row b * n + j", "ops.decode_step_attn_shared", "engine.SharedPrompt",
                   "B * n <= 32"):
        assert phrase in doc, phrase


def test_set_parallel_samples_validates_reaches_generate_only_when_on_and_leaves_sampling_alone():
    assert Mo.PARALLEL_SAMPLES == [1]
    assert Mo.SAMPLING[0] == dict(do_sample=False, temperature=1.0, top_k=50, top_p=1.0, seed=None)
    p = inspect.signature(Mo.MM_LLMs.set_parallel_samples).parameters
    assert {k: p[k].default for k in p} == dict(num_samples=1)
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
            seen.append("prepare")
            return "emb", None, None
    try:
        for bad in (0, 33, -2, 1.5, "2", True, None):
            with pytest.raises(ValueError, match="set_parallel_samples: num_samples"):
                Mo.MM_LLMs.set_parallel_samples(bad)
        assert Mo.PARALLEL_SAMPLES == [1]                           # a refused call changes nothing
        assert Mo.MM_LLMs.forward(Fake(), {"inference": True}) == "ids"
        assert "num_samples" not in seen[-1]
        Mo.MM_LLMs.set_parallel_samples(4)
        assert Mo.PARALLEL_SAMPLES == [4] and "num_samples" not in Mo.SAMPLING[0]
        del seen[:]
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert seen[0] == "prepare" and len(seen) == 2 and seen[-1]["num_samples"] == 4      # the towers run once
        Mo.MM_LLMs.set_parallel_samples()
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert "num_samples" not in seen[-1]
    finally:
        Mo.MM_LLMs.set_parallel_samples()
    assert Mo.PARALLEL_SAMPLES == [1]


# ------------------------------------------------------------------------------------------------ refusals --
class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates its arguments before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(**kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(1, 2, 4, dtype=torch.bfloat16), **kw)


def test_the_refusals_that_need_no_model_name_their_condition_and_the_default_raises_nothing():
    for bad in (0, 33, -1, 2.0, "3", True, None, [2]):
        with pytest.raises(ValueError, match=r"generate: num_samples must be an integer in \[1, 32\]"):
            _generate(num_samples=bad, do_sample=True)
    with pytest.raises(ValueError, match=r"num_samples=2\) with do_sample=False"):
        _generate(num_samples=2)
    with pytest.raises(ValueError, match=r"num_samples=2\) with num_beams=3.*not built"):
        _generate(num_samples=2, do_sample=True, num_beams=3)
    with pytest.raises(ValueError, match=r"prompt_lookup_num_tokens=4.*not built"):
        _generate(num_samples=2, do_sample=True, prompt_lookup_num_tokens=4)
    with pytest.raises(ValueError, match=r"num_samples=2\) with guidance_scale=1.5.*not built"):
        _generate(num_samples=2, do_sample=True, guidance_scale=1.5, negative_prompt_ids=torch.zeros(1, 2, dtype=torch.long))
    with pytest.raises(ValueError, match=r"num_samples=2\) with kv_cache='fp8'.*not built"):
        _generate(num_samples=2, do_sample=True, kv_cache="fp8")
    for kw in (dict(), dict(num_samples=1), dict(num_samples=1, num_beams=3), dict(num_samples=1, kv_cache="fp8"),
               dict(num_samples=2, do_sample=True), dict(num_samples=32, do_sample=True, top_k=1),
               dict(num_samples=2, do_sample=True, guidance_scale=1.0)):
        with pytest.raises(_PastTheChecks):
            _generate(**kw)
    # the existing refusals come first, with their text
    with pytest.raises(ValueError, match="num_beams must be"):
        _generate(num_samples=0, num_beams=0)
    with pytest.raises(ValueError, match="temperature"):
        _generate(num_samples=0, do_sample=True, temperature=0.0)


def test_the_engine_refuses_a_shared_prompt_outside_a_device_position_step():
    sp = eng.SharedPrompt(torch.empty(2, 3, 16), torch.empty(4, 5, 16), 2, 3)
    x = torch.zeros(4, 8)
    t_dev = torch.zeros(1, dtype=torch.int32)
    w = [None] * 9

    def layer(x2=x, **kw):
        return eng.llama_layer_cached(x2, 2, 1, 0, sp, 8, None, None, None, 2, 1e-6, *w, **kw)
    for kw in (dict(), dict(t_dev=t_dev, kv8=torch.zeros(1)), dict(t_dev=t_dev, beam=eng.Beam(torch.zeros(1), 2, 3)),
               dict(t_dev=t_dev, x2=torch.zeros(5, 8))):
        with pytest.raises(ValueError, match="SharedPrompt"):
            layer(**kw)
    with pytest.raises(ValueError):                                  # spec's own guard speaks first
        layer(t_dev=t_dev, spec=eng.Spec(torch.zeros(1), 2))


# ---------------------------------------------------------------------------------------- kernel resources --
LLVM_TOOLS = all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objcopy", "llvm-readelf"))


@pytest.mark.skipif(not (LLVM_TOOLS and os.path.exists(kr.LIB)),
                    reason="needs the built library and ROCm's llvm-objcopy / llvm-readelf")
def test_every_shared_step_kernel_fits_512_threads_without_scratch():
    """512 threads per workgroup = two waves per SIMD: at most 256 VGPRs, no spill, no scratch, for both element types,
    every head size and every R shipped (1: the untiled form MK_SHARED_ATTN_ROWS=1 selects, 4: the tile)"""
    from macaw_llm_amd import build
    build.build()                       # no-op when the stamp matches the sources
    ks = {k: v for k, v in kr.kernels().items() if "decode_step_attn_shared" in k}
    for ns, stem in (("e_bf16::", "decode_step_attn_shared_kernel<"), ("e_f16::", "decode_step_attn_shared_f16_kernel<")):
        for hd in (16, 32, 64, 128):
            for rows in (1, 4):
                assert any(k.startswith(f"void {ns}{stem}{hd}, 8, {rows}>") for k in ks), (ns, hd, rows)
    assert len(ks) == 16
    for k, v in ks.items():
        assert v["vgpr_count"] <= 256, (k, v)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
        assert v["max_flat_workgroup_size"] == 512, (k, v)
