"""CPU: the fp64 restatement of the mixed-adapter LoRA kernels (tests/lora_bgmv_ref.py) against a plain x (W + s B A)^T,
lora.AdapterBank's stacking against its restatement (ragged ranks, zero fill, untargeted modules, name -> index, s per
adapter), and every refusal of AdapterBank.add, generate(adapter_names=) and MM_LLMs.set_adapters that needs no GPU."""
import inspect
import json
import os
import re

import pytest
import torch

import lora_bgmv_ref as R
from elementwise_ref import ulp

from macaw_llm_amd import engine as eng
from macaw_llm_amd import lib as L
from macaw_llm_amd import lora
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, FF, LAYERS, HEADS, V = 32, 48, 2, 2, 40


def _lm(dtype=torch.bfloat16, fused=True):
    from transformers import LlamaConfig
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=D, intermediate_size=FF, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                      num_key_value_heads=HEADS, vocab_size=V, max_position_embeddings=64)
    lm = Mo.LlamaForCausalLM(cfg).to(dtype).eval()
    if fused:
        for lyr in lm.model.layers:
            lyr.fuse_projections()
    return lm


def _adapter(lm, r, alpha, targets, seed):
    """(LoraConfig, state dict under peft's keys) of a random adapter"""
    cfg = lora.LoraConfig(r=r, lora_alpha=alpha, target_modules=targets)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, _, _, lin in lora._targets(lm, cfg):
        sd[f"base_model.model.{key}.lora_A.weight"] = torch.randn((r, lin.in_features), generator=g).to(torch.bfloat16)
        sd[f"base_model.model.{key}.lora_B.weight"] = (torch.randn((lin.out_features, r), generator=g) * 0.05).to(torch.bfloat16)
    return cfg, sd


def _bank(lm):
    bank = lora.AdapterBank(lm)
    c1, s1 = _adapter(lm, 8, 16, ["q_proj", "v_proj", "down_proj"], 1)
    c2, s2 = _adapter(lm, 24, 12, r".*layers\.1\..*(k_proj|gate_proj|up_proj)", 2)
    bank.add("a1", state_dict=s1, config=c1).add("a2", state_dict=s2, config=c2)
    return bank, ((c1, s1), (c2, s2))


# ------------------------------------------------------------------------------------------ the restatement --
@pytest.mark.parametrize("G,K,N,r", [(3, 40, 24, 8), (2, 24, 56, 24), (1, 56, 16, 16)])
def test_restatement_is_x_times_w_plus_sba(G, K, N, r):
    """without roundings shrink + expand on Y0 = x W^T is x (W + s B A)^T module by module; with them the difference is
    what the two roundings allow: U's half ulp through |s| |B|, and the half ulp of the sum"""
    g = torch.Generator().manual_seed(G)
    M, n = 5, 3
    x = torch.randn((M, K), generator=g).to(torch.bfloat16)
    W = torch.randn((G * N, K), generator=g).to(torch.bfloat16)
    A = torch.randn((n, G * r, K), generator=g).to(torch.bfloat16)
    B = (torch.randn((n, G * N, r), generator=g) * 0.1).to(torch.bfloat16)
    s = torch.tensor([2.0, 0.5, 1.25])
    idx = [2, -1, 0, 3, 1]
    Y0 = x.double() @ W.double().t()
    plain = Y0.clone()
    for m, a in enumerate(idx):
        if 0 <= a < n:
            for i in range(G):
                Wi = (W[i * N:(i + 1) * N].double() +
                      float(s[a]) * B[a, i * N:(i + 1) * N].double() @ A[a, i * r:(i + 1) * r].double())
                plain[m, i * N:(i + 1) * N] = Wi @ x[m].double()
    U = R.shrink(x, A, idx)
    assert bool((U[1] == 0).all()) and bool((U[3] == 0).all())
    Y = R.expand(U, B, s, idx, Y0, G)
    assert float((Y - plain).abs().max()) <= 1e-9 * float(plain.abs().max())
    assert torch.equal(Y[1], Y0[1]) and torch.equal(Y[3], Y0[3])
    # with the kernels' roundings
    U16 = R.shrink(x, A, idx, torch.bfloat16)
    Y016 = Y0.to(torch.bfloat16)
    Y16 = R.expand(U16, B, s, idx, Y016, G, torch.bfloat16)
    slack = torch.zeros_like(plain)
    for m, a in enumerate(idx):
        if 0 <= a < n:
            for i in range(G):
                hu = 0.5 * ulp(U[m, i * r:(i + 1) * r], torch.bfloat16)
                slack[m, i * N:(i + 1) * N] = float(s[a]) * (B[a, i * N:(i + 1) * N].double().abs() @ hu)
    slack = slack + 0.5 * ulp(Y0, torch.bfloat16)                 # the base launch's own rounding
    slack = slack + 0.5 * ulp(plain.abs() + slack, torch.bfloat16)
    assert bool(((Y16.double() - plain).abs() <= slack).all())
    assert torch.equal(Y16[1], Y016[1])


def test_prologues_restate_the_stream_kernels_rounding_points():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 64), generator=g).to(torch.bfloat16)
    w = (1 + 0.1 * torch.randn(64, generator=g)).to(torch.bfloat16)
    assert R.rows(x, 0) is x
    y = R.rows(x, 1, w, 1e-6)
    ex = w.double() * (x.double() * torch.rsqrt((x.double() ** 2).mean(1, keepdim=True) + 1e-6))
    assert y.dtype == x.dtype and bool(((y.double() - ex).abs() <= 1.5 * ulp(ex, torch.bfloat16)).all())
    a = R.rows(x, 2)
    ex = torch.nn.functional.silu(x[:, :32].double()) * x[:, 32:].double()
    assert a.shape == (3, 32) and bool(((a.double() - ex).abs() <= 1.5 * ulp(ex, torch.bfloat16)).all())


def test_bounds_have_the_form_the_issue_states():
    ref, mag = torch.tensor([1.0, 0.0, -3.0]).double(), torch.tensor([2.0, 0.0, 8.0]).double()
    g = 2 * 4096 * 2.0 ** -24 * mag
    assert torch.equal(R.shrink_bound(ref, mag, 4096, torch.bfloat16), g + 0.5 * ulp(ref.abs() + g, torch.bfloat16))
    g = 2 * (16 + 2) * 2.0 ** -24 * mag
    assert torch.equal(R.expand_bound(ref, mag, 16, torch.float16), g + 0.5 * ulp(ref.abs() + g, torch.float16))


# ------------------------------------------------------------------------------------------------- the bank --
def test_bank_stacks_ragged_ranks_zero_fill_and_untargeted_modules():
    lm = _lm()
    bank, ads = _bank(lm)
    assert lm._lora_bank is bank and bank.names == ["a1", "a2"] and bank.scalings() == (2.0, 0.5)
    restated = []
    for cfg, sd in ads:
        ws = {(li, mi): (sd[f"base_model.model.{key}.lora_A.weight"], sd[f"base_model.model.{key}.lora_B.weight"])
              for key, li, mi, _ in lora._targets(lm, cfg)}
        restated.append((cfg.r, cfg.lora_alpha, ws))
    shapes = {"qkv": (D, D), "o": (D, D), "gu": (FF, D), "down": (D, FF)}
    st = bank.stacks()
    assert st is bank.stacks() and len(st) == LAYERS            # built once
    for li in range(LAYERS):
        for gi, (name, members) in enumerate(R.GROUPS):
            N, K = shapes[name]
            want = R.stack(restated, li, members, N, K, torch.bfloat16)
            got = st[li][gi]
            if want is None:
                assert got is None, (li, name)
                continue
            assert isinstance(got, eng.AdapterGroup) and got.G == len(members)
            assert got.A.shape == (2, len(members) * 24, K) and got.B.shape == (2, len(members) * N, 24)
            assert torch.equal(got.A, want[0]) and torch.equal(got.B, want[1]) and torch.equal(got.s, want[2])
            assert got.A.is_contiguous() and got.B.is_contiguous() and got.s.dtype == torch.float32
    # o is targeted by nobody; gate|up only by a2 at layer 1; q|k|v at layer 0 only by a1 (q, v), its k block zero
    assert st[0][1] is None and st[1][1] is None and st[0][2] is None and st[1][2] is not None
    qkv0 = st[0][0]
    assert bool((qkv0.A[1] == 0).all()) and bool((qkv0.B[1] == 0).all())               # a2 has nothing at layer 0
    assert bool((qkv0.A[0, 24:48] == 0).all()) and bool((qkv0.B[0, D:2 * D] == 0).all())   # k_proj untargeted by a1
    assert bool((qkv0.A[0, 8:24] == 0).all()) and bool((qkv0.B[0, :, 8:] == 0).all())       # rank 8 inside r_max = 24
    assert bool((qkv0.A[0, :8] != 0).any()) and bool((qkv0.B[0, :D, :8] != 0).any())
    # zero fill is exact: the stacked slab computes what the adapter computes
    x = torch.randn((1, D), generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    U = R.shrink(x, qkv0.A, [0])
    A_q = ads[0][1]["base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"]
    assert torch.equal(U[0, :8], A_q.double() @ x[0].double()) and bool((U[0, 8:48] == 0).all())
    # rebuilt when an adapter is added
    c3, s3 = _adapter(lm, 8, 8, ["o_proj"], 3)
    bank.add("a3", state_dict=s3, config=c3)
    st2 = bank.stacks()
    assert st2 is not st and st2[0][1] is not None and st2[0][0].A.shape[0] == 3 and bank.scalings() == (2.0, 0.5, 1.0)


def test_names_map_to_indices_and_runs():
    lm = _lm()
    bank, _ = _bank(lm)
    names = ["__base__", "a1", "a2", "a1", "a1", "__base__", "__base__", "a2"]
    idx = bank.indices(names)
    assert idx == [-1, 0, 1, 0, 0, -1, -1, 1] == R.name_indices(names, bank.names)
    assert bank.runs(idx) == ((1, 2, 0), (2, 3, 1), (3, 5, 0), (7, 8, 1)) == R.runs(idx)
    assert bank.runs([-1, -1]) == () and bank.runs([]) == () and bank.runs([1, 1, 1]) == ((0, 3, 1),)
    with pytest.raises(ValueError, match=r"unknown adapter name.*nope"):
        bank.indices(["a1", "nope"])


def test_bank_adds_a_saved_directory_and_a_live_snapshot(tmp_path):
    lm = _lm()
    src = _lm()
    lora.get_peft_model(src, lora.LoraConfig(r=8, lora_alpha=32, target_modules=["q_proj", "up_proj"]))
    with torch.no_grad():
        for n, q in src.named_parameters():
            if ".lora_B." in n:
                q.copy_(torch.randn(q.shape, generator=torch.Generator().manual_seed(5)) * 0.05)
    d = str(tmp_path / "ad")
    os.makedirs(d)
    with open(os.path.join(d, "adapter_config.json"), "w") as f:      # save_lora's files (it needs no device either)
        json.dump(src._lora.config.to_dict(), f)
    torch.save({k: v.clone() for k, v in lora.lora_state_dict(src).items()}, os.path.join(d, "adapter_model.bin"))
    bank = lora.AdapterBank(lm)
    bank.add("disk", d)
    bank.add("live", state_dict=lora.lora_state_dict(src), config=src._lora.config)
    st = bank.stacks()
    assert torch.equal(st[0][0].A[0], st[0][0].A[1]) and torch.equal(st[1][2].B[0], st[1][2].B[1])
    assert torch.equal(st[0][0].A[0, :8], src.model.layers[0].self_attn.q_proj.lora_A.weight)
    assert torch.equal(st[1][2].B[1, FF:, :8], src.model.layers[1].mlp.up_proj.lora_B.weight)
    assert bank.scalings() == (4.0, 4.0)
    assert not any(".lora_" in n for n, _ in lm.named_parameters())       # the bank lives next to the model


def test_bank_refusals():
    lm = _lm()
    bank, ((c1, s1), _) = _bank(lm)
    with pytest.raises(ValueError, match="__base__"):
        bank.add("__base__", state_dict=s1, config=c1)
    with pytest.raises(ValueError, match="already has an adapter 'a1'"):
        bank.add("a1", state_dict=s1, config=c1)
    with pytest.raises(ValueError, match="directory, or state_dict="):
        bank.add("x")
    with pytest.raises(ValueError, match="directory, or state_dict="):
        bank.add("x", state_dict=s1)
    missing = dict(list(s1.items())[1:])
    with pytest.raises(KeyError, match="adapter file does not match the model: missing"):
        bank.add("x", state_dict=missing, config=c1)
    extra = {**s1, "base_model.model.model.layers.0.self_attn.o_proj.lora_A.weight": torch.zeros(8, D)}
    with pytest.raises(KeyError, match="unexpected"):
        bank.add("x", state_dict=extra, config=c1)
    with pytest.raises(NotImplementedError, match="bias"):
        bank.add("x", state_dict=s1, config=lora.LoraConfig(r=8, target_modules=c1.target_modules, bias="all"))
    with pytest.raises(NotImplementedError, match="rank r=12"):
        bank.add("x", state_dict=s1, config=lora.LoraConfig(r=12, target_modules=c1.target_modules))
    with pytest.raises(NotImplementedError, match="lm_head"):
        bank.add("x", state_dict=s1, config=lora.LoraConfig(r=8, target_modules=["lm_head"]))
    assert bank.names == ["a1", "a2"]
    with pytest.raises(TypeError):
        lora.AdapterBank(torch.nn.Linear(2, 2))


# -------------------------------------------------------------------------------------------- generate() --
def test_generate_refuses_what_adapter_names_does_not_compose_with(monkeypatch):
    """every ValueError of generate(adapter_names=) is raised before anything is launched: a CPU model gets that far"""
    monkeypatch.setattr(Mo, "_dev_check", lambda t: None)
    lm = _lm()
    emb = torch.zeros((2, 5, D), dtype=torch.bfloat16)
    names = ["a1", "__base__"]
    kw = dict(inputs_embeds=emb, max_new_tokens=4, adapter_names=names)
    with pytest.raises(ValueError, match=r"adapter_names=\): the model has no adapter bank"):
        lm.generate(**kw)
    bank, _ = _bank(lm)
    ids = torch.ones((2, 5), dtype=torch.long)
    for over, why in ((dict(num_beams=2), "num_beams=2"),
                      (dict(num_samples=2, do_sample=True), "num_samples=2"),
                      (dict(prompt_lookup_num_tokens=2, input_ids=ids), "prompt_lookup_num_tokens=2"),
                      (dict(guidance_scale=2.0, negative_prompt_ids=ids), "guidance_scale=2.0"),
                      (dict(return_session=True), "session"),
                      (dict(use_cache=False), "use_cache=False")):
        with pytest.raises(ValueError, match=r"adapter_names=\): " + re.escape(why)):
            lm.generate(**{**kw, **over})
    with pytest.raises(ValueError, match=r"adapter_names=\): 3 names for 2 samples"):
        lm.generate(**{**kw, "adapter_names": names + ["a2"]})
    with pytest.raises(ValueError, match="unknown adapter name"):
        lm.generate(**{**kw, "adapter_names": ["a1", "a9"]})
    with pytest.raises(ValueError, match=r"adapter_names=\): 33 rows"):
        lm.generate(inputs_embeds=torch.zeros((33, 5, D), dtype=torch.bfloat16), max_new_tokens=4,
                    adapter_names=["a1"] * 33)
    # fp32, unfused storage, a live adapter next to the bank
    lm32 = _lm(torch.float32)
    b32 = lora.AdapterBank(lm32)
    c, s = _adapter(lm32, 8, 16, ["q_proj"], 1)
    b32.add("a1", state_dict=s, config=c)
    with pytest.raises(ValueError, match=r"adapter_names=\): fp32 parameters"):
        lm32.generate(inputs_embeds=emb.float(), max_new_tokens=4, adapter_names=names)
    unf = _lm(fused=False)
    lora.AdapterBank(unf).add("a1", state_dict=s, config=c)
    with pytest.raises(ValueError, match=r"adapter_names=\): unfused q/k/v or gate/up storage"):
        unf.generate(**kw)
    lora.get_peft_model(lm, lora.LoraConfig(r=8, target_modules=["q_proj"]))
    with pytest.raises(ValueError, match=r"adapter_names=\): the model also carries a live adapter"):
        lm.generate(**kw)


def test_surface_signatures_and_the_switch():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    assert p["adapter_names"].default is None and p["adapter_names"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert "adapter_names" in Mo.LlamaForCausalLM.generate.__doc__
    # the spec travels in place of w8 / q8: the signatures every other caller binds to are what they were
    assert list(inspect.signature(eng.llama_layer_cached).parameters)[-6:] == ["t_dev", "w8", "kv8", "ragged", "beam", "spec"]
    assert list(inspect.signature(eng._stream_linear).parameters) == ["x", "W", "q8", "pro", "w_ln", "eps", "residual", "FF"]
    assert eng.Adapters._fields == ("idx", "runs", "s_host", "qkv", "o", "gu", "down", "w8")
    assert eng.Adapters._field_defaults == {"w8": None}
    assert Mo.ADAPTERS == [None]
    try:
        Mo.MM_LLMs.set_adapters(["a", "__base__"])
        assert Mo.ADAPTERS == [["a", "__base__"]]
        for bad in ("a", [1], 3):
            with pytest.raises(ValueError, match="set_adapters"):
                Mo.MM_LLMs.set_adapters(bad)
        assert Mo.ADAPTERS == [["a", "__base__"]]
    finally:
        Mo.MM_LLMs.set_adapters()
    assert Mo.ADAPTERS == [None]


def test_the_engine_refuses_adapters_where_rows_are_not_samples():
    ad = eng.Adapters(torch.zeros(4, dtype=torch.int32), (), (), None, None, None, None)
    x = torch.zeros((4, 32), dtype=torch.bfloat16)
    sp = eng.SharedPrompt(torch.empty(1), torch.empty(1), 2, 1)
    with pytest.raises(ValueError, match="Adapters map rows to samples"):
        eng.llama_layer_cached(x, 2, 1, 0, sp, 8, None, None, None, 2, 1e-6, *([None] * 9), w8=ad)
    with pytest.raises(ValueError, match="Adapters map rows to samples"):
        eng.llama_layer_cached(x, 2, 2, 0, None, 8, None, None, None, 2, 1e-6, *([None] * 9), w8=ad,
                               beam=eng.Beam(torch.empty(1), 2, 1), t_dev=torch.zeros(1, dtype=torch.int32))


def test_abi_declares_and_binds_the_two_kernels():
    src = open(os.path.join(ROOT, "include", "macaw_hip.h")).read()
    for name, n_args in (("mk_lora_bgmv_shrink", 16), ("mk_lora_bgmv_expand", 14)):
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", src, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == n_args == len(L.SIGNATURES[name]), name
    for word in ("rnd16", "outside [0, n_adapters)", "do not depend on M"):
        assert word in src
    for f in ("lora_bgmv_shrink", "lora_bgmv_expand_", "lora_bgmv_ok"):
        assert callable(getattr(ops, f))
