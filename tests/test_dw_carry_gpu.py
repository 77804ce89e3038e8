"""engine.DW_CARRY: one grad-weight queue for the whole backward pass (ops.DW_WINDOW, opened by bucketed.BucketedStep.begin) against
the same model with the mode off, where every layer drains its own queue.  Every tile is computed by the same instruction stream
on the same operands, so every comparison is bit for bit.

A decoder of 3 layers (modeling.LlamaForCausalLM, vocabulary 256, bf16) in three set-ups:
  micro      D = 256 (2 heads of 128), FF = 512, B S = 2 x 256 = 512, all CUs
  micro-8    the same with mk_gemm_set_cus(8)
  mid-8      D = 768 (6 heads), FF = 1024, B S = 2 x 384 = 768, mk_gemm_set_cus(8): the shape of tests/test_dw_fill_layer_gpu.py
The micro products are so small (dW of 1 to 4 tiles, dx of 2 or 4) that every launch uses its queue up, at 8 CUs too: carry mode
plans them as the balance mode does when the queue runs dry.  In mid-8 the grad-input launches are 12, 9, 9 and 9 tiles on 8
workgroups with 12 + 24 + 9 + 27 grad-weight tiles queued per layer, so tiles stay queued behind every layer and run inside the
launches of the next one; the assertions about carried tiles use that set-up."""
import csv

import pytest
import torch
from transformers import LlamaConfig

pytestmark = pytest.mark.gpu

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import modeling as M  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.bucketed import BucketedStep  # noqa: E402
from macaw_llm_amd.optim import FusedAdamW  # noqa: E402

SETUPS = {"micro": (256, 512, 256, 0), "micro-8": (256, 512, 256, 8), "mid-8": (768, 1024, 384, 8)}   # D, FF, S, planned CUs
LAYERS, VOCAB, BATCH = 3, 256, 2
ALL = pytest.mark.parametrize("setup", list(SETUPS))


def _model(dev, setup, dtype=torch.bfloat16, lora=False):
    D, FF, S, _ = SETUPS[setup]
    torch.manual_seed(5)
    cfg = LlamaConfig(vocab_size=VOCAB, hidden_size=D, intermediate_size=FF, num_hidden_layers=LAYERS, num_attention_heads=D // 128,
                      max_position_embeddings=S, rms_norm_eps=1e-6, pad_token_id=0, hidden_act="silu")
    model = M.LlamaForCausalLM(cfg).to(dtype).to(dev).eval()
    if lora:
        from macaw_llm_amd.lora import LoraConfig, get_peft_model
        get_peft_model(model, LoraConfig(r=8, lora_alpha=16, target_modules=["q_proj", "v_proj", "down_proj"]))
    model.SEED_STRIDE = 0                 # (train.GraphedStep advances a dropout seed by it; this model has no dropout)
    ids = torch.randint(1, VOCAB, (BATCH, S), generator=torch.Generator().manual_seed(6)).to(dev)
    return model, ids


def _run(dev, setup, carry, *, steps=1, micros=1, graphed=False, callback=True, finish=True, profile=None, dtype=torch.bfloat16,
         lora=False, **kw):
    """`steps` optimizer steps of `micros` micro-batches.  Returns the losses, the gradient buckets and every .grad as the last
    backward of each step left them (read BEFORE finish()), the parameters at the end, and the counters."""
    model, ids = _model(dev, setup, dtype, lora)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = FusedAdamW(params, lr=1e-3, weight_decay=0.01)
    rt = BucketedStep(params, opt, bucket_bytes=kw.pop("bucket_bytes", 64 << 10), accumulate_steps=micros, model=model, **kw)
    lib = L.load()
    old = eng.DW_CARRY["on"], eng._dw_window_flush
    eng.DW_CARRY["on"], eng.DW_FILL["layers"] = carry, 0
    ops.DW_WINDOW.update(carried=0, flushed=0)
    if not callback:      # the end-of-backward callback launches nothing: finish() has to
        eng._dw_window_flush = lambda: ops.DW_WINDOW.__setitem__("callback", False)
    out = {"loss": [], "buckets": [], "grads": [], "rt": rt}
    lib.mk_gemm_set_cus(SETUPS[setup][3])
    try:
        if profile:
            ops.prof_begin()
        if graphed:
            from macaw_llm_amd.train import GraphedStep
            gs = GraphedStep(model, lambda: model(input_ids=ids, labels=ids).loss, rt)
            out["loss"] = [gs.step().clone() for _ in range(steps)]
        for _ in range(0 if graphed else steps):
            for m in range(micros):
                rt.begin()
                loss = model(input_ids=ids, labels=ids).loss
                loss.backward()
                if m == micros - 1:
                    if callback:
                        q = ops.DW_WINDOW["q"]
                        assert q is None or not q.items, "the backward pass ended with grad-weight tiles queued"
                        out["buckets"].append([b.g.clone() for b in rt.buckets])
                        out["grads"].append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
                    if not finish:
                        rt.abort()
                        break
                rt.finish()
            out["loss"].append(loss.detach().clone())
        torch.cuda.synchronize()
        if profile:
            ops.prof_report(profile)
            out["flops"] = ops.prof_sum(0)[1]
    finally:
        if profile:
            ops.prof_end()
        lib.mk_gemm_set_cus(0)
        eng.DW_CARRY["on"], eng._dw_window_flush = old
        rt.abort()
        rt.remove()
    assert ops.DW_WINDOW["q"] is None and not ops.DW_WINDOW["callback"], "the window outlived finish() / abort()"
    out["params"] = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    out["layers"], out["carried"], out["flushed"] = eng.DW_FILL["layers"], ops.DW_WINDOW["carried"], ops.DW_WINDOW["flushed"]
    return out


_REF = {}


def _ref(dev, setup, **kw):
    """the run with carry off, made once per (set-up, arguments) and shared"""
    key = (setup, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REF:
        _REF[key] = _run(dev, setup, False, **kw)
        assert _REF[key]["carried"] == 0
    return _REF[key]


def _same(got, ref, what, keys=("loss", "buckets", "grads", "params")):
    for key in keys:
        a, b = got[key], ref[key]
        if key == "params":
            a, b = [a], [b]
        assert len(a) == len(b) and len(a) > 0, f"{what}: {key}"
        for step, (x, y) in enumerate(zip(a, b)):
            if isinstance(x, torch.Tensor):
                x, y = [x], [y]
            if isinstance(x, dict):
                assert x.keys() == y.keys(), f"{what}: {key} of step {step}"
                names, x, y = list(x), list(x.values()), [y[n] for n in x]
            else:
                names = list(range(len(x)))
            for n, t, r in zip(names, x, y):
                assert t.shape == r.shape and torch.equal(t, r), f"{what}: {key} {n} of step {step} differs"
                assert torch.isfinite(t.float()).all(), f"{what}: {key} {n} of step {step} not finite"


@ALL
def test_one_step_is_bit_identical(dev, setup):
    """the loss, every gradient bucket before the update, every .grad, the parameters after it"""
    got, ref = _run(dev, setup, True), _ref(dev, setup)
    assert got["layers"] == ref["layers"] == LAYERS          # every layer took the fill path on both sides
    _same(got, ref, "one step")


@ALL
def test_two_steps_leak_nothing_across_the_window(dev, setup):
    got, ref = _run(dev, setup, True, steps=2), _ref(dev, setup, steps=2)
    _same(got, ref, "two steps")
    if setup == "mid-8":
        assert got["carried"] > 0


@ALL
def test_finish_flushes_what_the_backward_left_queued(dev, setup):
    """without the end-of-backward callback the tiles are still queued when finish() is called: its flush stands in front of
    the update (two steps, so that a tile left behind would show in the second)"""
    got, ref = _run(dev, setup, True, steps=2, callback=False), _ref(dev, setup, steps=2)
    _same(got, ref, "flush in finish()", keys=("loss", "params"))
    if setup == "mid-8":
        assert got["flushed"] > 0


@ALL
def test_gradient_accumulation_drains_the_second_micro_batch_per_layer(dev, setup):
    got, ref = _run(dev, setup, True, micros=2), _ref(dev, setup, micros=2)
    _same(got, ref, "two micro-batches")


@ALL
def test_local_overlap_updates_stand_behind_the_flush(dev, setup):
    """per-bucket AdamW launches on the side stream while the backward runs (from the second step on, once the bucket order is
    frozen); buckets of 256 KiB close inside every layer, and the flush in _launch puts complete gradients in front of each"""
    kw = dict(steps=3, local_overlap=True, bucket_bytes=256 << 10)
    got, ref = _run(dev, setup, True, **kw), _ref(dev, setup, **kw)
    assert got["rt"].local_overlap and len(got["rt"].buckets) > 2 * LAYERS
    assert any(b.updated for b in got["rt"].buckets), "no update went out behind the backward"
    _same(got, ref, "local_overlap", keys=("loss", "params"))
    _same(got, _ref(dev, setup, steps=3, bucket_bytes=256 << 10), "local_overlap against the serial update", keys=("loss", "params"))


@ALL
def test_backward_without_finish_leaves_complete_gradients(dev, setup):
    """loss.backward() inside an opened window, then .grad is read without finish(): the end-of-backward callback flushed"""
    got, ref = _run(dev, setup, True, finish=False), _ref(dev, setup)
    _same(got, ref, "no finish()", keys=("buckets", "grads"))


@ALL
def test_the_captured_step_replays_the_eager_one(dev, setup):
    """train.GraphedStep: one eager step, then capture and two replays, against three eager steps with carry off"""
    got, ref = _run(dev, setup, True, steps=3, graphed=True), _ref(dev, setup, steps=3)
    _same(got, ref, "captured", keys=("loss", "params"))


@pytest.mark.parametrize("setup", ["micro", "micro-8"])
def test_fp32_and_lora_models_keep_todays_path(dev, setup):
    for kw in (dict(dtype=torch.float32), dict(lora=True)):
        got, ref = _run(dev, setup, True, **kw), _ref(dev, setup, **kw)
        assert got["layers"] == 0 and got["carried"] == 0 and got["flushed"] == 0, kw
        _same(got, ref, str(kw))


def test_tiles_of_a_layer_run_inside_the_launches_of_the_next(dev, tmp_path):
    """mid-8: with carry off the backward is 4 grouped launches per layer, each layer's 72 grad-weight tiles inside its own four.
    With carry on tiles stay queued behind every layer (the counter on the window) and run in the next layer's launches: the same
    4 launches per layer plus the filler-only launch of the final flush, and the same GEMM FLOPs in all."""
    paths = [str(tmp_path / "off.csv"), str(tmp_path / "on.csv")]
    off = _run(dev, "mid-8", False, profile=paths[0])
    on = _run(dev, "mid-8", True, profile=paths[1])
    _same(on, off, "profiled step")
    launches, alone = [], []
    for path in paths:
        with open(path) as f:
            rows = [r for r in csv.DictReader(f) if r["kind"] == "gemm"]
        launches.append(sum(int(r["launches"]) for r in rows if int(r["cfg"]) == 16))
        # grad-weight GEMMs on their own (layout 3): lm_head's and no other, the same on both sides
        alone.append(sorted((int(r["M"]), int(r["N"]), int(r["K"]), int(r["launches"])) for r in rows
                            if int(r["layout"]) == 3 and int(r["cfg"]) != 16))
    assert launches[0] == 4 * LAYERS and launches[1] == 4 * LAYERS + 1, launches
    assert alone[0] == alone[1], alone
    assert on["flops"] == off["flops"]
    # behind every layer between half a round and a round and a half of tiles (4 .. 12 at 8 workgroups) wait for the next one
    assert off["carried"] == 0 and 4 * LAYERS <= on["carried"] <= 12 * LAYERS, on["carried"]
    assert 4 <= on["flushed"] <= 12, on["flushed"]
