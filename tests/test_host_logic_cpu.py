"""CPU tests of the host-side mirror of the reference surface: integer prefix plumbing against
the reference's own outputs (golden), state-dict key parity, config round trip."""
import os

import pytest
import torch

from golden_util import load_case
from oracle import configs


def _lq(fx, cfg):
    mm = cfg["mm"]
    n_img = (cfg["clip"]["vision_config"]["image_size"] // cfg["clip"]["vision_config"]["patch_size"]) ** 2
    n_aud = cfg["whisper"]["max_source_positions"]
    out = {}
    inp = fx["inputs"]
    if inp["images"] is not None:
        out["image"] = (n_img - mm["image_conv_kernel"]) // mm["image_conv_stride"] + 1
    if inp["audios"] is not None:
        out["audio"] = (n_aud - mm["audio_conv_kernel"]) // mm["audio_conv_stride"] + 1
    if inp["videos"] is not None:
        out["video"] = (n_img * mm["n_frames"] - mm["video_conv_kernel"]) // mm["video_conv_stride"] + 1
    return out


@pytest.mark.parametrize("case", ["micro_all", "micro_image"])
def test_prefix_layout_bit_exact_vs_reference(case):
    from macaw_llm_amd.modeling import build_prefix_layout
    fx = load_case(case)
    cfg = configs.get(fx["config_name"])
    ids_full, slots, am, lab = build_prefix_layout(fx["inputs"], _lq(fx, cfg))
    assert torch.equal(am, fx["attention_mask"]) and am.dtype == fx["attention_mask"].dtype
    assert torch.equal(lab, fx["labels"]) and lab.dtype == fx["labels"].dtype
    # token rows of the reference's inputs_embeds are exactly E[ids_full]; -1 marks feature slots
    E = fx["state"]["llm.model.embed_tokens.weight"]
    emb = fx["inputs_embeds"]
    tok = ids_full >= 0
    assert torch.equal(emb[tok], E[ids_full[tok]])
    covered = torch.zeros_like(tok)
    for name, (start, n) in slots.items():
        covered[:, start:start + n] = True
        s, e = cfg["tags"][name]
        assert (ids_full[:, start - 1] == s).all() and (ids_full[:, start + n] == e).all()
    assert torch.equal(covered, ~tok)
    order = [n for n in ("image", "audio", "video") if n in slots]
    starts = [slots[n][0] for n in order]
    assert starts == sorted(starts) and (ids_full[:, 0] == 1).all()     # [BOS][image][audio][video][text]


def test_text_only_layout_keeps_integer_dtypes():
    from macaw_llm_amd.modeling import build_prefix_layout
    inp = dict(input_ids=torch.tensor([[1, 5, 6]]), attention_mask=torch.ones(1, 3, dtype=torch.int64),
               labels=torch.tensor([[-100, 5, 6]]))
    ids_full, slots, am, lab = build_prefix_layout(inp, {})
    assert torch.equal(ids_full, inp["input_ids"]) and slots == {}
    assert am.dtype == torch.int64 and lab.dtype == torch.int64 and torch.equal(lab, inp["labels"])


def _reference_state_dict():
    """the whole state dict of the reference's MM_LLMs on the micro config at seed 1234, as recorded in tests/golden/:
    the hot-path tensors of micro_state_seed1234.pt + the rest (reference_checks.pt)"""
    from golden_util import GOLDEN_DIR
    rc = torch.load(os.path.join(GOLDEN_DIR, "reference_checks.pt"), weights_only=False)
    return {**torch.load(os.path.join(GOLDEN_DIR, rc["state_file"]), weights_only=False), **rc["state_rest"]}


def test_state_dict_keys_cover_golden_and_match_reference():
    from macaw_llm_amd.factory import make_config
    from macaw_llm_amd import modeling as M
    fx = load_case("micro_all")
    cfg = configs.get("micro")
    model = M.MM_LLMs(make_config(cfg))
    mine = model.state_dict()
    for k, v in fx["state"].items():
        assert k in mine and mine[k].shape == v.shape, k
    # 'encoder' naming used by run_clm_llms.py:390-393 to freeze the towers
    enc = [n for n, _ in model.named_parameters() if "encoder" in n]
    assert any(n.startswith("image_encoder.") for n in enc) and any(n.startswith("audio_encoder.") for n in enc)
    assert not any("encoder" in n for n, _ in model.llm.named_parameters())
    rs = _reference_state_dict()
    assert set(rs) == set(mine)
    assert all(rs[k].shape == mine[k].shape for k in rs)


def test_config_surface_round_trip(tmp_path):
    from macaw_llm_amd.factory import make_config
    from macaw_llm_amd import modeling as M
    cfg = configs.get("micro")
    c = make_config(cfg)
    assert c.hidden_size == max(cfg["llama"]["hidden_size"], cfg["clip"]["projection_dim"], cfg["whisper"]["d_model"])
    d = c.to_dict()
    assert d["model_type"] == "mm_llms" and d["image_conv_kernel"] == cfg["mm"]["image_conv_kernel"]
    assert isinstance(d["llm_config"], dict) and d["llm_config"]["hidden_size"] == cfg["llama"]["hidden_size"]
    c.save_pretrained(tmp_path)
    c2 = M.MM_LLMs_Config.from_pretrained(str(tmp_path))
    assert c2.llm_config.hidden_size == c.llm_config.hidden_size
    assert c2.audio_config.d_model == c.audio_config.d_model
    assert c2.image_config.projection_dim == c.image_config.projection_dim


def test_root_modeling_shim_exports_reference_names():
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    m = importlib.import_module("modeling")
    for name in ("MM_LLMs", "MM_LLMs_Config", "LlamaForCausalLM", "LlamaModel", "LlamaDecoderLayer",
                 "LlamaAttention", "LlamaMLP", "LlamaRMSNorm", "LlamaRotaryEmbedding"):
        assert hasattr(m, name), name


def test_checkpoint_round_trip_with_fused_projections(tmp_path):
    """save_pretrained / MM_LLMs.from_pretrained(dir, config=...) as
    run_clm_llms_inference.py:455 does, with the q|k|v / gate|up weights living in fused storage."""
    from macaw_llm_amd.factory import build_model, make_config
    from macaw_llm_amd import modeling as M
    cfg = configs.get("micro")
    m = build_model(cfg, dtype=torch.float32, device="cpu", fuse=True)
    l0 = m.llm.model.layers[0]
    assert l0._fused_view((l0.self_attn.q_proj.weight, l0.self_attn.k_proj.weight,
                           l0.self_attn.v_proj.weight)) is not None
    m.save_pretrained(tmp_path)
    m2 = M.MM_LLMs.from_pretrained(str(tmp_path), config=make_config(cfg))
    a, b = m.state_dict(), m2.state_dict()
    assert set(a) == set(b)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_loads_a_checkpoint_written_by_the_reference(tmp_path):
    """state-dict interchange: a checkpoint saved by the reference's MM_LLMs loads into ours"""
    from macaw_llm_amd.factory import make_config
    from macaw_llm_amd import modeling as M
    cfg = configs.get("micro")
    from safetensors.torch import save_file
    rs = _reference_state_dict()
    # (the reference's own save_pretrained cannot run under transformers 5.x: its config class
    # has no default constructor; write its state dict and a config the way HF would)
    save_file(rs, str(tmp_path / "model.safetensors"), metadata={"format": "pt"})
    make_config(cfg).save_pretrained(tmp_path)
    mine = M.MM_LLMs.from_pretrained(str(tmp_path), config=make_config(cfg))
    ms = mine.state_dict()
    assert set(rs) == set(ms)
    assert all(torch.equal(rs[k], ms[k]) for k in rs)


def test_gradient_checkpointing_flag_surface():
    """modeling.py:325-329,474: HF's enable/disable toggles LlamaModel.gradient_checkpointing,
    which the layer loop turns into LlamaLayerFn(recompute=True) while training"""
    from transformers import LlamaConfig
    from macaw_llm_amd import modeling as M
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      vocab_size=100)
    m = M.LlamaForCausalLM(cfg)
    assert m.supports_gradient_checkpointing and m.model.gradient_checkpointing is False
    m.gradient_checkpointing_enable()
    assert m.model.gradient_checkpointing is True
    m.gradient_checkpointing_disable()
    assert m.model.gradient_checkpointing is False


def test_grad_weight_side_stream_auto_rule_and_switches(monkeypatch):
    """engine.DW_SIDE "auto": the grad-weight GEMMs go to the second stream exactly where the [M, D] grad-input GEMMs leave
    CUs idle (the four BASELINE training shapes on 256 CUs), never on the CPU engines; the RoPE-fusion switch takes its
    three values and refuses anything else."""
    from macaw_llm_amd import engine, ops
    assert engine.dw_side_auto(2176, 4096, 256)          # cfg 2: 144 tiles, less than one round
    assert not engine.dw_side_auto(4608, 4096, 256)      # cfg 3: 288 = 256 + 32 (the tail runs as eighth-tiles)
    assert not engine.dw_side_auto(8192, 4096, 256)      # cfg 4: two whole rounds
    assert engine.dw_side_auto(4608, 5120, 256)          # cfg 5: 360 = 256 + 104
    assert not engine.dw_side_auto(144, 4096, 256)       # one sample: skinny kernels
    import torch
    sd = engine._DwSide(torch.device("cpu"), 2176, 4096)
    assert sd.side is None and sd.fork() is None
    sd.join()
    for v in ("off", "bwd", "full"):
        monkeypatch.setenv("MACAW_ROPE_FUSE", v)
        assert ops.rope_fuse_mode() == v
    monkeypatch.setenv("MACAW_ROPE_FUSE", "yes")
    import pytest
    with pytest.raises(ops.MacawHipError):
        ops.rope_fuse_mode()
    monkeypatch.delenv("MACAW_ROPE_FUSE")
    assert ops.rope_fuse_mode() == "off"


def test_adamw_slice_size_has_one_source():
    """the multi-tensor AdamW's chunk table (host) and its kernel (library) must cut the tensors into the same slices: the host asks
    the library (mk_adamw_chunk) instead of repeating the constant"""
    from macaw_llm_amd import lib as L
    from macaw_llm_amd.optim import FusedAdamW
    import torch
    chunk = int(L.load().mk_adamw_chunk())
    assert chunk > 0 and chunk % 1024 == 0          # whole trips of 256 threads x 4 elements
    opt = FusedAdamW([torch.nn.Parameter(torch.zeros(8))], lr=1e-3)
    assert opt._CHUNK == chunk
