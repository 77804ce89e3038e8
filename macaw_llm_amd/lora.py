"""LoRA fine-tuning of the LLaMA decoder projections, with the semantics of peft's LoraConfig / LoraLayer (0.3).

    from macaw_llm_amd.lora import LoraConfig, get_peft_model
    lora_config = LoraConfig(r=8, lora_alpha=16, target_modules=["q_proj", "k_proj", "v_proj"],
                             lora_dropout=0.05, bias="none", task_type="CAUSAL_LM")
    model.llm = get_peft_model(model.llm, lora_config)      # run_clm_llms.py:498-508, unchanged

A targeted projection y = x W^T becomes y = x W^T + s (drop(x) A^T) B^T with s = lora_alpha / r, A [r, in]
(kaiming_uniform_(a=sqrt(5))) and B [out, r] (zeros): a fresh adapter computes exactly what the base model
computes.  `drop` is an inverted dropout (p = lora_dropout) on the adapter branch only, in train() mode only,
with an independent mask per module.  The adapters are child modules of the targeted nn.Linear
(`...self_attn.q_proj.lora_A.weight` / `.lora_B.weight`); every other parameter of the LLM is frozen.

The products run in csrc/lora.hip, called by engine.LlamaLayerFn at four points of the layer (q|k|v before
RoPE, o after its residual GEMM, gate|up before SwiGLU, down after its residual GEMM).  Masks are regenerated
from a counter hash of (step seed, layer, module, element), never stored.  generate() merges the adapters
into temporary copies of the targeted weights for the duration of the call (see LlamaForCausalLM.generate).

Several frozen adapters of one base model decode in ONE batch through AdapterBank (below) and
generate(adapter_names=[...]): nothing is merged, every row names its adapter ("__base__" for none), and the decode
step adds it with the mk_lora_bgmv kernels of csrc/lora_bgmv.hip.
"""
from __future__ import annotations

import json
import math
import os
import re
from typing import List, Optional

import torch
from torch import nn

from . import engine as eng
from . import ops

PEFT_TYPE = "LORA"
_NOT_YET = ("embed_tokens", "lm_head")


class LoraConfig:
    """peft.LoraConfig's fields (the ones the reference sets, run_clm_llms.py:498-508)"""

    def __init__(self, r: int = 8, lora_alpha: int = 8, target_modules: Optional[List[str]] = None,
                 lora_dropout: float = 0.0, bias: str = "none", task_type: str = "CAUSAL_LM",
                 fan_in_fan_out: bool = False, inference_mode: bool = False, **_):
        self.peft_type = PEFT_TYPE
        self.r, self.lora_alpha, self.lora_dropout = int(r), lora_alpha, float(lora_dropout)
        # a str is a regular expression matched against whole module names (peft 0.3); else a list of name suffixes
        if target_modules is None:
            target_modules = ["q_proj", "v_proj"]
        self.target_modules = target_modules if isinstance(target_modules, str) else list(target_modules)
        self.bias, self.task_type = bias, task_type
        self.fan_in_fan_out, self.inference_mode = bool(fan_in_fan_out), bool(inference_mode)

    @property
    def scaling(self) -> float:
        return self.lora_alpha / self.r

    def to_dict(self) -> dict:
        return {"peft_type": self.peft_type, "r": self.r, "lora_alpha": self.lora_alpha,
                "lora_dropout": self.lora_dropout, "bias": self.bias,
                "target_modules": self.target_modules if isinstance(self.target_modules, str) else list(self.target_modules),
                "task_type": self.task_type, "fan_in_fan_out": self.fan_in_fan_out,
                "inference_mode": self.inference_mode, "base_model_name_or_path": None}

    @classmethod
    def from_dict(cls, d: dict) -> "LoraConfig":
        if d.get("peft_type", PEFT_TYPE) != PEFT_TYPE:
            raise ValueError(f"not a LoRA adapter config: peft_type={d.get('peft_type')!r}")
        return cls(**{k: v for k, v in d.items() if k != "peft_type"})


class LoraState:
    """per-model adapter state shared by the targeted layers: config, and the dropout seed of the step"""

    SLOT = 41                   # MM_LLMs dropout slot of the adapters (slots 0-2 and 40 are taken)

    def __init__(self, config: LoraConfig):
        self.config = config
        self.seed = 0
        self.ext_seed = None    # set by MM_LLMs.forward from its own step seed (hipGraph-replayable)
        self.step = 0           # a LlamaForCausalLM used on its own counts its steps here

    def begin_step(self, training: bool):
        if self.ext_seed is not None:
            self.seed, self.ext_seed = self.ext_seed, None
        elif training:
            self.step += 1
            self.seed = (0x5EED * 1000003 + self.step * 64 + self.SLOT) & 0x7FFFFFFFFFFF


def _check(config: LoraConfig):
    if config.bias != "none":
        raise NotImplementedError(f"LoRA bias={config.bias!r} is not implemented; use bias='none'")
    if config.fan_in_fan_out:
        raise NotImplementedError("fan_in_fan_out=True is for Conv1D (GPT-2) layers; LLaMA has nn.Linear")
    if not (8 <= config.r <= 128 and config.r % 8 == 0):
        raise NotImplementedError(f"LoRA rank r={config.r}: the kernels take r a multiple of 8 in [8, 128]")
    if not 0.0 <= config.lora_dropout < 1.0:
        raise ValueError(f"lora_dropout={config.lora_dropout} must be in [0, 1)")
    if any(eng.FP8.values()):
        raise NotImplementedError("LoRA adapters cannot be combined with the fp8 switches (MM_LLMs.set_fp8)")


def _matches(key: str, target_modules) -> bool:
    """peft 0.3's rule (LoraModel._find_and_replace): a str is a regex that must match the whole module name,
    a list matches every module name that ends with one of its entries (a plain suffix, no dot needed)"""
    if isinstance(target_modules, str):
        return re.fullmatch(target_modules, key) is not None
    return any(key.endswith(t) for t in target_modules)


def _targets(model, config: LoraConfig):
    """[(qualified name, layer index, module index, nn.Linear)] of the modules peft would target.  Entries that
    match nothing are ignored, as peft does; matching embed_tokens / lm_head (not implemented here) or a module
    that is not one of the decoder projections (peft: not an nn.Linear) is an error"""
    from .modeling import LlamaDecoderLayer
    proj = {}
    for lname, layer in model.named_modules():
        if isinstance(layer, LlamaDecoderLayer):
            idx = int(lname.rsplit(".", 1)[-1])
            for mname, mod in layer.named_modules():
                leaf = mname.rsplit(".", 1)[-1]
                if leaf in eng.LORA_MODULES and isinstance(mod, nn.Linear):
                    proj[f"{lname}.{mname}"] = (idx, eng.LORA_MODULES.index(leaf), mod)
    out, not_yet, other = [], [], []
    for key, mod in model.named_modules():
        if not key or not _matches(key, config.target_modules):
            continue
        if key in proj:
            out.append((key, *proj[key]))
        elif key.rsplit(".", 1)[-1] in _NOT_YET:
            not_yet.append(key)
        else:
            other.append(f"{key} ({type(mod).__name__})")
    if not_yet:
        raise NotImplementedError(
            f"LoRA on {' and '.join(_NOT_YET)} is not implemented (target_modules matches {not_yet}); drop "
            f"{' and '.join(repr(n) for n in _NOT_YET)} from target_modules")
    if other:
        raise ValueError(f"target_modules matches modules that LoRA does not support here: {other[:4]} (supported: "
                         f"the decoder projections {list(eng.LORA_MODULES)})")
    return out


def _llama_causal(model):
    from .modeling import LlamaForCausalLM
    if isinstance(model, LlamaForCausalLM):
        return model
    raise TypeError(f"get_peft_model: expected the LLaMA language model (MM_LLMs.llm), got {type(model).__name__}")


def get_peft_model(model, config: LoraConfig):
    """Freeze every parameter of `model` (a LlamaForCausalLM), add LoRA adapters to the targeted decoder
    projections and return `model` itself, modified in place."""
    _check(config)
    model = _llama_causal(model)
    if getattr(model, "_lora", None) is not None:
        raise ValueError("get_peft_model: the model already has LoRA adapters")
    tg = _targets(model, config)
    if not tg:
        raise ValueError(f"get_peft_model: target_modules {config.target_modules} match no LLaMA projection "
                         f"(candidates: {list(eng.LORA_MODULES)})")
    for p in model.parameters():
        p.requires_grad_(False)
    state = LoraState(config)
    r = config.r
    for _, li, mi, lin in tg:
        w = lin.weight
        a = nn.Linear(lin.in_features, r, bias=False).to(device=w.device, dtype=w.dtype)
        b = nn.Linear(r, lin.out_features, bias=False).to(device=w.device, dtype=w.dtype)
        with torch.no_grad():
            t = torch.empty((r, lin.in_features), dtype=torch.float32)
            nn.init.kaiming_uniform_(t, a=math.sqrt(5))          # peft LoraLayer.reset_parameters
            a.weight.copy_(t)
            b.weight.zero_()
        lin.lora_A, lin.lora_B = a, b
    for i, layer in enumerate(model.model.layers):
        layer._lora_state, layer._lora_layer = state, i
    model._lora = state
    model.peft_config = {"default": config}
    return model


def lora_layers(model):
    """[(layer index, layer)] of the decoder layers that carry at least one adapter"""
    return [(i, l) for i, l in enumerate(_llama_causal(model).model.layers) if layer_adapters(l)]


def layer_adapters(layer):
    """[(module index, nn.Linear)] of the adapted projections of one decoder layer, in LORA_MODULES order"""
    a, m = layer.self_attn, layer.mlp
    lins = (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj)
    return [(i, lin) for i, lin in enumerate(lins) if hasattr(lin, "lora_A")]


def lora_state_dict(model) -> dict:
    """the adapter weights under peft's saved-adapter keys (base_model.model.<name>.lora_A.weight)"""
    model = _llama_causal(model)
    return {f"base_model.model.{n}": p.detach() for n, p in model.named_parameters()
            if ".lora_A." in n or ".lora_B." in n}


def save_lora(model, directory: str):
    """adapter_config.json + adapter_model.bin, as peft's save_pretrained writes them"""
    model = _llama_causal(model)
    os.makedirs(directory, exist_ok=True)
    cfg = model._lora.config.to_dict()
    with open(os.path.join(directory, "adapter_config.json"), "w") as f:
        json.dump(cfg, f, indent=2, sort_keys=True)
    torch.save({k: v.to("cpu").clone() for k, v in lora_state_dict(model).items()},
               os.path.join(directory, "adapter_model.bin"))


def load_lora(model, directory: str):
    """add the adapters saved in `directory` to `model` (get_peft_model with the saved config, then the saved
    weights); returns `model`"""
    with open(os.path.join(directory, "adapter_config.json")) as f:
        cfg = LoraConfig.from_dict(json.load(f))
    model = _llama_causal(model)
    if getattr(model, "_lora", None) is None:
        get_peft_model(model, cfg)
    sd = torch.load(os.path.join(directory, "adapter_model.bin"), map_location="cpu")
    params = dict(model.named_parameters())
    want = {f"base_model.model.{n}" for n in params if ".lora_A." in n or ".lora_B." in n}
    if set(sd) != want:
        raise KeyError(f"adapter file does not match the model: missing {sorted(want - set(sd))[:4]}, "
                       f"unexpected {sorted(set(sd) - want)[:4]}")
    with torch.no_grad():
        for k, v in sd.items():
            params[k[len("base_model.model."):]].copy_(v)
    return model


def merged_weight(lin, s, out=None):
    """W + s B A of one adapted nn.Linear (fp32 product, one rounding), into `out` (a copy of W) or W itself"""
    W = lin.weight.data if out is None else out
    if not W.is_cuda:
        raise ops.MacawHipError("merge_and_unload: the model must be on the HIP device")
    return ops.lora_merge_(W, lin.lora_A.weight.data, lin.lora_B.weight.data, s)


@torch.no_grad()
def merged_layer_weights(model, layer):
    """(layer, engine.LayerWeights) with every adapted projection replaced by a merged COPY (W + s B A); fused
    q|k|v / gate|up buffers are copied whole so that the one-GEMM decode path stays"""
    s = model._lora.config.scaling
    a, m = layer.self_attn, layer.mlp
    lins = (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj)
    ws = [lin.weight for lin in lins]
    wqkv, wgu = layer.fused_weights()
    ad = dict(layer_adapters(layer))
    for fused, members in ((wqkv, (0, 1, 2)), (wgu, (4, 5))):
        if fused is not None and any(i in ad for i in members):
            cp = fused.clone()
            off = 0
            for i in members:
                n = ws[i].shape[0]
                ws[i] = cp[off:off + n]
                off += n
                if i in ad:
                    merged_weight(ad[i], s, ws[i])
            if members[0] == 0:
                wqkv = cp
            else:
                wgu = cp
    for i, lin in ad.items():
        if ws[i] is lin.weight:
            ws[i] = merged_weight(lin, s, lin.weight.detach().clone())
    return layer, eng.LayerWeights(*ws, wqkv, wgu)


@torch.no_grad()
def merge_and_unload(model):
    """W <- W + s B A for every adapter (csrc/lora.hip merge: fp32, rounded once), then remove the adapters;
    returns the plain model"""
    model = _llama_causal(model)
    state = model._lora
    s = state.config.scaling
    for layer in model.model.layers:
        for _, lin in layer_adapters(layer):
            merged_weight(lin, s)
            del lin.lora_A, lin.lora_B
        if hasattr(layer, "_lora_state"):
            del layer._lora_state, layer._lora_layer
    model._lora = None
    if hasattr(model, "peft_config"):
        del model.peft_config
    return model


# =========================================================================
# Mixed-adapter decoding: generate(adapter_names=[...])
# =========================================================================
BASE = "__base__"       # the name of "no adapter" in generate(adapter_names=), as in peft's mixed adapter batches


class AdapterBank:
    """Frozen, inference-only adapters of one LlamaForCausalLM for generate(adapter_names=[...]), kept next to the model
    (model._lora_bank), never inside it: the model's own parameters and modules stay what they are.

        bank = AdapterBank(model.llm)
        bank.add("image", "out/lora_image")                      # a save_lora / peft directory
        bank.add("live", state_dict=lora_state_dict(m), config=m._lora.config)
        model.llm.generate(..., adapter_names=["image", "__base__", "live", "image"])

    Adapters may differ in rank and in target modules.  Per (layer, group of engine.LORA_GROUPS) the bank keeps the
    stacks the mk_lora_bgmv kernels index by a row's adapter: A [n, G r_max, K], B [n, G N, r_max] and s [n] =
    lora_alpha / r of each adapter, the group's modules row-concatenated; a smaller rank and an untargeted module are
    zero-filled, which is exact (their products are zeros).  A group no adapter targets at a layer has no stack, and no
    launch.  The stacks are built on first use and rebuilt after an add()."""

    def __init__(self, model):
        self.model = _llama_causal(model)
        self.names: List[str] = []      # adapter i is names[i]
        self.configs: List[LoraConfig] = []
        self._weights = []              # per adapter {(layer, module index): (A [r, K], B [N, r])}
        self._stacks = None
        self.model._lora_bank = self

    def add(self, name: str, directory: Optional[str] = None, *, state_dict: Optional[dict] = None,
            config: Optional[LoraConfig] = None):
        """add the adapter saved in `directory` (save_lora's / peft's adapter_config.json + adapter_model.bin), or the
        given state_dict (lora_state_dict's keys) with its LoraConfig, under `name`; returns the bank"""
        if name == BASE:
            raise ValueError(f"AdapterBank.add: {BASE!r} names the base model in adapter_names; choose another name")
        if name in self.names:
            raise ValueError(f"AdapterBank.add: the bank already has an adapter {name!r}")
        if (directory is None) == (state_dict is None) or (state_dict is not None and config is None):
            raise ValueError("AdapterBank.add: pass a directory, or state_dict= with its config=")
        if directory is not None:
            with open(os.path.join(directory, "adapter_config.json")) as f:
                config = LoraConfig.from_dict(json.load(f))
            state_dict = torch.load(os.path.join(directory, "adapter_model.bin"), map_location="cpu")
        elif isinstance(config, dict):
            config = LoraConfig.from_dict(config)
        _check(config)
        tg = _targets(self.model, config)
        want = {f"base_model.model.{key}.lora_{ab}.weight" for key, _, _, _ in tg for ab in "AB"}
        if set(state_dict) != want:
            raise KeyError(f"adapter file does not match the model: missing {sorted(want - set(state_dict))[:4]}, "
                           f"unexpected {sorted(set(state_dict) - want)[:4]}")
        ws = {}
        for key, li, mi, lin in tg:
            w = lin.weight
            A = state_dict[f"base_model.model.{key}.lora_A.weight"].detach().to(device=w.device, dtype=w.dtype)
            B = state_dict[f"base_model.model.{key}.lora_B.weight"].detach().to(device=w.device, dtype=w.dtype)
            if tuple(A.shape) != (config.r, lin.in_features) or tuple(B.shape) != (lin.out_features, config.r):
                raise KeyError(f"adapter file does not match the model: {key} has A {tuple(A.shape)}, B {tuple(B.shape)} "
                               f"for r = {config.r} on a [{lin.out_features}, {lin.in_features}] projection")
            ws[(li, mi)] = (A.clone(), B.clone())
        self.names.append(name)
        self.configs.append(config)
        self._weights.append(ws)
        self._stacks = None
        return self

    def indices(self, names) -> List[int]:
        """adapter_names -> the index of each in the bank, -1 for "__base__"; ValueError for an unknown name"""
        lut = {n: i for i, n in enumerate(self.names)}
        unknown = [n for n in names if n != BASE and n not in lut]
        if unknown:
            raise ValueError(f"generate(adapter_names=): unknown adapter name(s) {unknown[:4]}; the bank has "
                             f"{self.names} and {BASE!r} for none")
        return [-1 if n == BASE else lut[n] for n in names]

    @staticmethod
    def runs(indices):
        """((b0, b1, a), ...): the maximal runs of consecutive samples [b0, b1) with the same adapter a >= 0"""
        out, b0 = [], 0
        for b in range(1, len(indices) + 1):
            if b == len(indices) or indices[b] != indices[b0]:
                if indices[b0] >= 0:
                    out.append((b0, b, indices[b0]))
                b0 = b
        return tuple(out)

    def scalings(self):
        return tuple(float(c.scaling) for c in self.configs)

    @torch.no_grad()
    def stacks(self):
        """per layer the four engine.AdapterGroup (or None) in engine.LORA_GROUPS order"""
        if self._stacks is not None:
            return self._stacks
        n = len(self.names)
        rmax = max((c.r for c in self.configs), default=0)
        out = []
        for li, layer in enumerate(self.model.model.layers):
            a, m = layer.self_attn, layer.mlp
            lins = (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj)
            groups = []
            for _, members in eng.LORA_GROUPS:
                if not any((li, mi) in ws for ws in self._weights for mi in members):
                    groups.append(None)
                    continue
                G, w0 = len(members), lins[members[0]].weight
                N, K = w0.shape
                if any(tuple(lins[mi].weight.shape) != (N, K) for mi in members):
                    raise NotImplementedError("AdapterBank: the projections of a group differ in shape (grouped-query "
                                              "attention is not built)")
                A = torch.zeros((n, G * rmax, K), dtype=w0.dtype, device=w0.device)
                B = torch.zeros((n, G * N, rmax), dtype=w0.dtype, device=w0.device)
                for ai, ws in enumerate(self._weights):
                    for i, mi in enumerate(members):
                        if (li, mi) in ws:
                            Aa, Ba = ws[(li, mi)]
                            A[ai, i * rmax:i * rmax + Aa.shape[0]] = Aa
                            B[ai, i * N:(i + 1) * N, :Ba.shape[1]] = Ba
                s = torch.tensor(self.scalings(), dtype=torch.float32, device=w0.device)
                groups.append(eng.AdapterGroup(A, B, s, G))
            out.append(tuple(groups))
        self._stacks = out
        return out
