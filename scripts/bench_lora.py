"""LoRA fine-tuning at BASELINE cfg 3 (CLIP + Whisper + LLaMA-7B, image + 30 s audio + 128 tokens, bf16, 32
samples per GPU): the same model, inputs and step runtime as bench.py (factory.build_model, BucketedStep), with
the LLM frozen and LoRA adapters (macaw_llm_amd/lora.py) on all seven decoder projections and on the reference's
q|k|v subset, r = 8, lora_alpha = 16, lora_dropout = 0.05.  One JSON line per variant:

  samples_per_s, ms_per_step   wall time of the timed steps (after --warmup untimed ones)
  lora_ms                      device time of the adapter launches of ONE step (in-library profiler, kind 4)
  lora_gb, lora_tb_s           their HBM traffic from the shapes (operands read + outputs read-modify-written)
                               and the effective bandwidth

    python scripts/bench_lora.py --steps 5 --warmup 2 [--variants full,all7,qkv] [--layers N]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ALL7 = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
VARIANTS = {"full": None, "all7": ALL7, "qkv": ["q_proj", "k_proj", "v_proj"]}


def lora_bytes(M, D, FF, layers, targets, r=8, es=2):
    """HBM bytes of one step's adapter launches: per group, forward reads X and read-modify-writes the outputs;
    backward reads dY twice (dU, dB), X once (dA) and read-modify-writes dX (the rank-r operands are noise)"""
    groups = [(("q_proj", "k_proj", "v_proj"), D, D), (("o_proj",), D, D), (("gate_proj", "up_proj"), D, FF),
              (("down_proj",), FF, D)]
    tot = 0
    for mods, K, N in groups:
        G = sum(m in targets for m in mods)
        if G:
            tot += M * K * es + 2 * M * N * G * es                     # down + up-add
            tot += 2 * M * N * G * es + M * K * es + 2 * M * K * es     # bwd-dy (2 reads), bwd-x
    return tot * layers


def run(variant, args):
    from macaw_llm_amd import ops
    from macaw_llm_amd import lora as L
    from macaw_llm_amd.bucketed import BucketedStep
    from macaw_llm_amd.factory import baseline_config, build_model, synthetic_inputs
    from macaw_llm_amd.optim import FusedAdamW
    import bench
    spec = bench.CONFIGS[3]
    dev = torch.device("cuda:0")
    cfg = baseline_config(spec["model"])
    if args.layers is not None:
        cfg["llama"]["num_hidden_layers"] = args.layers
    model = build_model(cfg, dtype=torch.bfloat16, device=dev, seed=1234).train()
    targets = VARIANTS[variant]
    if targets is not None:
        model.llm = L.get_peft_model(model.llm, L.LoraConfig(r=8, lora_alpha=16, target_modules=targets,
                                                             lora_dropout=0.05))
    params = [p for p in model.parameters() if p.requires_grad]
    opt = FusedAdamW(params, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    rt = BucketedStep(params, opt, model=model)
    B = spec["batch"]
    inputs = synthetic_inputs(cfg, B, spec["text_len"], modalities=spec["modalities"], seed=1, device=dev)

    def step():
        rt.begin()
        loss = model(inputs=inputs).loss
        loss.backward()
        rt.finish()
        return loss

    step()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    res = dict(variant=variant, targets=targets, r=8, batch=B, layers=cfg["llama"]["num_hidden_layers"],
               ms_per_step=round(ms, 2), samples_per_s=round(B * 1e3 / ms, 2), loss=float(loss.detach()),
               trainable_params=sum(p.numel() for p in params))
    if targets is not None:
        ops.prof_begin()
        step()
        lms, _, n = ops.prof_sum(ops.PROF_LORA)
        ops.prof_end()
        M = B * spec["seq"]
        gb = lora_bytes(M, cfg["llama"]["hidden_size"], cfg["llama"]["intermediate_size"],
                        cfg["llama"]["num_hidden_layers"], targets) / 1e9
        res.update(lora_ms=round(lms, 2), lora_launches=n, lora_gb=round(gb, 1),
                   lora_tb_s=round(gb / lms, 2) if lms else None)
    rt.remove()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variants", default="full,all7,qkv")
    ap.add_argument("--layers", type=int, default=None, help="truncate the LLaMA stack (quick runs)")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        print(json.dumps(run(args.one, args)), flush=True)
        return
    import subprocess
    for v in args.variants.split(","):      # one fresh process per variant (the 7B model and its state each)
        cmd = [sys.executable, os.path.abspath(__file__), "--one", v, "--steps", str(args.steps),
               "--warmup", str(args.warmup)] + (["--layers", str(args.layers)] if args.layers is not None else [])
        r = subprocess.run(cmd, cwd=ROOT)
        if r.returncode != 0:
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
