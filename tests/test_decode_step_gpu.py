"""GPU: the one five-launch decode step of engine.llama_layer_cached against the same five launches composed by hand
from ops calls -- bit for bit, output and KV cache -- where tests/test_decode_fp8_gpu.py and tests/test_decode_kv8_gpu.py
compare paths under tolerances: mixed e4m3 / 16-bit weights, and more than 16 rows (the separate RMSNorm / SwiGLU
kernel, then the plain launch) with and without e4m3 weights.  And generate(decode_weights="fp8") with LoRA adapters on
a one-layer model: the named weight set through the merged path, ids equal to the merged-and-unloaded model's."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import lora as L  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

D, H, FF, TMAX, T0, EPS = 128, 2, 256, 8, 5, 1e-6
HD = D // H


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    ops.clear_fp8_cache()


def _layer(B, dev, seed):
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16).to(dev)  # noqa: E731
    W = {n: bf(torch.randn(N, K, generator=g) * 0.05)
         for n, (N, K) in dict(wqkv=(3 * D, D), wo=(D, D), wgu=(2 * FF, D), wd=(D, FF)).items()}
    W["ln1"], W["ln2"] = bf(1 + 0.1 * torch.randn(D, generator=g)), bf(1 + 0.1 * torch.randn(D, generator=g))
    x2 = bf(torch.randn(B, D, generator=g))
    cache = torch.zeros((B, TMAX, 2 * D), dtype=torch.bfloat16)
    cache[:, :T0] = torch.randn(B, T0, 2 * D, generator=g).to(torch.bfloat16)
    inv = 1.0 / (10000.0 ** (torch.arange(0, HD, 2).float() / HD))
    ang = torch.cat((torch.outer(torch.arange(TMAX).float(), inv),) * 2, dim=-1)
    return W, x2, cache.to(dev), bf(ang.cos()), bf(ang.sin())


def _by_hand(W, q8, x2, B, kvc, cos, sin, t_dev, folded):
    """the five launches; q8[name] = the e4m3 pair of a weight or None; folded: the prologue forms (<= 16 rows here)"""
    def linear(x, name, pro=0, w_ln=None, residual=None):
        if not folded and pro:
            x, pro = (ops.rmsnorm_fwd(x, w_ln, EPS)[1] if pro == 1 else ops.swiglu2d_fwd(x, FF)), 0
        if q8[name] is not None:
            return ops.decode_linear_fp8(x, *q8[name], pro, w_ln if pro else None, EPS, residual)
        if folded or name == "wo":
            return ops.decode_linear(x, W[name], pro, w_ln if pro else None, EPS, residual)
        return ops.linear_fwd(x, W[name], residual=residual)

    qkv = linear(x2, "wqkv", 1, W["ln1"])
    att = torch.empty((B, D), dtype=x2.dtype, device=x2.device)
    ops.decode_step_attn(qkv, qkv, qkv, 3 * D, cos, sin, kvc, t_dev, TMAX, B, H, HD, att, 1.0 / math.sqrt(HD),
                         k_off=D, v_off=2 * D)
    h1 = linear(att, "wo", residual=x2)
    gu = linear(h1, "wgu", 1, W["ln2"])
    return linear(gu, "wd", 2, residual=h1)


@pytest.mark.parametrize("B,which", [(2, "mixed"), (20, "fp8"), (20, "16bit")])
def test_device_position_step_is_bit_equal_to_the_five_launches_composed_by_hand(dev, B, which):
    W, x2, cache, cos, sin = _layer(B, dev, 7 + B)
    fp8 = {"mixed": ("wqkv", "wgu"), "fp8": ("wqkv", "wo", "wgu", "wd"), "16bit": ()}[which]
    q8 = {n: ops.quantize_fp8_rows(W[n]) if n in fp8 else None for n in ("wqkv", "wo", "wgu", "wd")}
    w8 = None if which == "16bit" else (q8["wqkv"], q8["wo"], q8["wgu"], q8["wd"])
    t_dev = torch.tensor([T0], dtype=torch.int32, device=dev)
    pos = torch.full((B,), T0, dtype=torch.int32, device=dev)
    kv_a, kv_b = cache.clone(), cache.clone()
    with torch.no_grad():
        got = eng.llama_layer_cached(x2, B, 1, 0, kv_a, TMAX, pos, cos, sin, H, EPS, W["wqkv"][:D], W["wqkv"][D:2 * D],
                                     W["wqkv"][2 * D:], W["wo"], W["wgu"][:FF], W["wgu"][FF:], W["wd"], W["ln1"],
                                     W["ln2"], W["wqkv"], W["wgu"], t_dev=t_dev, w8=w8)
        want = _by_hand(W, q8, x2, B, kv_b, cos, sin, t_dev, folded=B <= 16)
    assert torch.isfinite(want.float()).all() and want.float().abs().max().item() > 0.1
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
    assert torch.equal(kv_a, kv_b) and not torch.equal(kv_a[:, T0], cache[:, T0])


def test_generate_fp8_with_adapters_on_one_layer_gives_the_merged_models_ids(dev):
    from transformers import LlamaConfig
    torch.manual_seed(5)
    Mo.AUTO_FUSE = True
    cfg = LlamaConfig(vocab_size=320, hidden_size=D, intermediate_size=FF, num_hidden_layers=1, num_attention_heads=H,
                      max_position_embeddings=64, rms_norm_eps=EPS)
    lm = Mo.fuse_model(Mo.LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16)).eval()
    lm = L.get_peft_model(lm, L.LoraConfig(r=8, lora_alpha=16, target_modules=list(eng.LORA_MODULES)))
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if ".lora_B." in n:
                p.copy_(torch.randn_like(p.float()) * 0.05)
    lm.eval()
    ids = torch.randint(3, 320, (2, 4), generator=torch.Generator().manual_seed(1)).to(dev)
    kw = dict(input_ids=ids, max_new_tokens=4, eos_token_id=-1, pad_token_id=0, decode_weights="fp8")
    a = lm.generate(**kw)
    b = L.merge_and_unload(lm).generate(**kw)
    assert a.shape == (2, 4)
    assert torch.equal(a, b), (a, b)
