"""CPU: the public surface of the e4m3 KV cache -- generate(kv_cache=...) and MM_LLMs.set_kv_cache validate their
argument before any device work, kv_cache is a NAMED parameter of generate() (not swallowed by **_), and the two new
entry points are declared in include/macaw_hip.h with ctypes signatures of the declared arity (test_abi_cpu.py then
checks on its own that the library exports every declared symbol)."""
import inspect
import os
import re

import pytest
import torch

from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")


def _tiny_llama():
    from transformers import LlamaConfig
    cfg = LlamaConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=2, vocab_size=40, max_position_embeddings=64)
    return Mo.LlamaForCausalLM(cfg).eval()


def test_generate_rejects_an_unknown_kv_cache_without_a_device():
    lm = _tiny_llama()
    ids = torch.randint(3, 40, (1, 5))
    with pytest.raises(ValueError, match="kv_cache"):
        lm.generate(input_ids=ids, max_new_tokens=4, kv_cache="int4")
    par = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    assert "kv_cache" in par and par["kv_cache"].default is None and par["kv_cache"].kind is not inspect.Parameter.VAR_KEYWORD


def test_set_kv_cache_validates_and_is_a_process_wide_switch():
    assert Mo.KV_CACHE[0] is None
    with pytest.raises(ValueError, match="set_kv_cache"):
        Mo.MM_LLMs.set_kv_cache("x")
    assert Mo.KV_CACHE[0] is None
    try:
        Mo.MM_LLMs.set_kv_cache("fp8")
        assert Mo.KV_CACHE[0] == "fp8"
    finally:
        Mo.MM_LLMs.set_kv_cache(None)
    assert Mo.KV_CACHE[0] is None


@pytest.mark.parametrize("name", ["mk_kv_quant_append", "mk_decode_step_attn_kv8"])
def test_the_kv8_entry_points_are_declared_and_bound(name):
    src = open(HEADER).read()
    m = re.search(r"^int " + name + r"\(([^;]*)\);", src, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/macaw_hip.h"
    assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    assert len(L.SIGNATURES[name]) == len(m.group(1).split(","))
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION


def test_the_header_states_the_cache_format():
    src = open(HEADER).read()
    assert "[B][t_max][2 * D]" in src and "[B][t_max][2 * H]" in src and "amax / 448" in src
