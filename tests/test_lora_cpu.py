"""LoRA (macaw_llm_amd/lora.py) host logic: config checks, peft's target matching, the trainable set after
get_peft_model on an MM_LLMs, and the adapter save / load round trip.  No GPU."""
import json
import os

import pytest
import torch

from oracle import configs
from macaw_llm_amd import lora as L
from macaw_llm_amd import modeling as M
from macaw_llm_amd.factory import make_config

from golden_util import load_case

REF_TARGETS = ["q_proj", "k_proj", "v_proj", "out_proj", "fc_in", "fc_out", "wte", "embed_tokens", "lm_head"]


@pytest.fixture(scope="module")
def cfg():
    return configs.get(load_case("micro_all")["config_name"])


def _mm(cfg):
    torch.manual_seed(0)
    m = M.MM_LLMs(make_config(cfg))
    for n, p in m.named_parameters():       # run_clm_llms.py:390-393: the encoders are frozen
        p.requires_grad_("encoder" not in n)
    return m


def test_the_reference_list_names_embed_tokens_and_lm_head(cfg):
    m = _mm(cfg)
    lc = L.LoraConfig(r=8, lora_alpha=16, target_modules=REF_TARGETS, lora_dropout=0.05, bias="none",
                      task_type="CAUSAL_LM")
    with pytest.raises(NotImplementedError) as e:
        L.get_peft_model(m.llm, lc)
    assert "embed_tokens" in str(e.value) and "lm_head" in str(e.value)
    assert not any(".lora_" in n for n, _ in m.named_parameters())


def test_the_reference_list_without_them_targets_exactly_qkv_in_every_layer(cfg):
    m = _mm(cfg)
    lc = L.LoraConfig(r=8, lora_alpha=16, target_modules=REF_TARGETS[:-2], lora_dropout=0.05)
    assert L.get_peft_model(m.llm, lc) is m.llm
    names = {n for n, _ in m.llm.named_parameters() if ".lora_" in n}
    nl = cfg["llm"]["num_hidden_layers"] if "llm" in cfg else len(m.llm.model.layers)
    want = {f"model.layers.{i}.self_attn.{p}_proj.lora_{ab}.weight" for i in range(len(m.llm.model.layers))
            for p in "qkv" for ab in "AB"}
    assert names == want and nl == len(m.llm.model.layers)
    lyr = m.llm.model.layers[0].self_attn
    D = lyr.q_proj.in_features
    assert lyr.q_proj.lora_A.weight.shape == (8, D) and lyr.q_proj.lora_B.weight.shape == (D, 8)
    assert torch.count_nonzero(lyr.q_proj.lora_B.weight) == 0 and torch.count_nonzero(lyr.q_proj.lora_A.weight) > 0
    bound = 1.0 / D ** 0.5            # kaiming_uniform_(a=sqrt(5)) on [r, in]: U(-1/sqrt(in), 1/sqrt(in))
    assert float(lyr.q_proj.lora_A.weight.detach().abs().max()) <= bound


def test_a_list_that_matches_nothing_raises(cfg):
    m = _mm(cfg)
    with pytest.raises(ValueError):
        L.get_peft_model(m.llm, L.LoraConfig(r=8, target_modules=["out_proj", "fc_in", "wte"]))


@pytest.mark.parametrize("kw", [dict(bias="all"), dict(bias="lora_only"), dict(r=12)])
def test_unsupported_settings_are_refused(cfg, kw):
    m = _mm(cfg)
    with pytest.raises(NotImplementedError):
        L.get_peft_model(m.llm, L.LoraConfig(**{"r": 8, "target_modules": ["q_proj"], **kw}))


def test_lora_with_fp8_is_refused(cfg):
    m = _mm(cfg)
    try:
        M.MM_LLMs.set_fp8(True, True, False)
        with pytest.raises(NotImplementedError):
            L.get_peft_model(m.llm, L.LoraConfig(r=8, target_modules=["q_proj"]))
    finally:
        M.MM_LLMs.set_fp8(False, False, False)


def test_trainable_set_after_get_peft_model(cfg):
    m = _mm(cfg)
    before = {n for n, p in m.named_parameters() if p.requires_grad}
    m.llm = L.get_peft_model(m.llm, L.LoraConfig(r=16, lora_alpha=32, target_modules=list(
        ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")), lora_dropout=0.05))
    after = {n for n, p in m.named_parameters() if p.requires_grad}
    lora = {n for n in after if ".lora_A." in n or ".lora_B." in n}
    assert len(lora) == 14 * len(m.llm.model.layers)
    assert all(n.startswith("llm.") for n in lora)
    # the MM_LLMs glue (conv / linear projections, alignment attention, ...) keeps training; nothing else of the LLM
    assert after - lora == {n for n in before if not n.startswith("llm.")}
    assert not any("encoder" in n for n in after)
    assert {n for n, p in m.named_parameters() if n.startswith("llm.") and p.requires_grad} == lora


def test_adapter_save_load_round_trip_with_peft_keys(cfg, tmp_path):
    m = _mm(cfg)
    lc = L.LoraConfig(r=8, lora_alpha=16, target_modules=["q_proj", "v_proj", "down_proj"], lora_dropout=0.05)
    L.get_peft_model(m.llm, lc)
    with torch.no_grad():
        for n, p in m.llm.named_parameters():
            if ".lora_B." in n:
                p.normal_()
    sd = L.lora_state_dict(m.llm)
    assert "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight" in sd
    assert "base_model.model.model.layers.0.mlp.down_proj.lora_B.weight" in sd
    assert len(sd) == 6 * len(m.llm.model.layers)
    L.save_lora(m.llm, str(tmp_path))
    with open(os.path.join(tmp_path, "adapter_config.json")) as f:
        c = json.load(f)
    assert c["peft_type"] == "LORA" and c["r"] == 8 and c["lora_alpha"] == 16 and c["lora_dropout"] == 0.05
    assert c["target_modules"] == ["q_proj", "v_proj", "down_proj"] and c["bias"] == "none"
    assert c["task_type"] == "CAUSAL_LM" and c["fan_in_fan_out"] is False and "inference_mode" in c
    assert set(torch.load(os.path.join(tmp_path, "adapter_model.bin"))) == set(sd)
    m2 = _mm(cfg)
    L.load_lora(m2.llm, str(tmp_path))
    sd2 = L.lora_state_dict(m2.llm)
    assert sd2.keys() == sd.keys()
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    assert m2.llm._lora.config.scaling == 2.0


def test_targets_follow_peft_suffix_and_regex_rules(cfg):
    """peft 0.3: a list entry is a plain suffix of the module name ('_proj' takes all seven projections), a str is
    a regular expression over the whole name"""
    m = _mm(cfg)
    L.get_peft_model(m.llm, L.LoraConfig(r=8, target_modules=["_proj"]))
    n_layers = len(m.llm.model.layers)
    assert sum(".lora_A." in n for n, _ in m.llm.named_parameters()) == 7 * n_layers
    m = _mm(cfg)
    L.get_peft_model(m.llm, L.LoraConfig(r=8, target_modules=r"model\.layers\.0\.self_attn\.(q|v)_proj"))
    assert {n for n, _ in m.llm.named_parameters() if ".lora_" in n} == {
        f"model.layers.0.self_attn.{p}_proj.lora_{ab}.weight" for p in "qv" for ab in "AB"}
    m = _mm(cfg)
    with pytest.raises(NotImplementedError) as e:     # a regex that reaches lm_head
        L.get_peft_model(m.llm, L.LoraConfig(r=8, target_modules=r".*(q_proj|lm_head)"))
    assert "lm_head" in str(e.value)
    m = _mm(cfg)
    with pytest.raises(ValueError):                   # peft: only nn.Linear can carry an adapter
        L.get_peft_model(m.llm, L.LoraConfig(r=8, target_modules=["self_attn"]))
    assert not any(".lora_" in n for n, _ in m.llm.named_parameters())


def test_a_regex_config_survives_the_save_load_round_trip(cfg, tmp_path):
    m = _mm(cfg)
    L.get_peft_model(m.llm, L.LoraConfig(r=8, target_modules=r".*\.(k|o)_proj"))
    L.save_lora(m.llm, str(tmp_path))
    with open(os.path.join(tmp_path, "adapter_config.json")) as f:
        assert json.load(f)["target_modules"] == r".*\.(k|o)_proj"
    m2 = _mm(cfg)
    L.load_lora(m2.llm, str(tmp_path))
    assert L.lora_state_dict(m2.llm).keys() == L.lora_state_dict(m.llm).keys()
