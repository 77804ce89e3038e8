"""GPU: LoRA adapters (csrc/lora.hip, engine.LlamaLayerFn, macaw_llm_amd/lora.py) against fp32 torch restatements
computed here: every kernel at LLaMA-7B widths, one decoder layer (fused and unfused projections, activation
checkpointing), a whole MM_LLMs training step, the hipGraph-replayed step, two ranks on one GPU, and generate()."""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from softmax_ref import hash32  # noqa: E402
from test_model_gpu import build_model, to_dev  # noqa: E402

from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd import lora as L  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402

ALL7 = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def keep_mask(seed, tag, M, K, p, dev):
    thr = min(int((1.0 - p) * 4294967296.0), 0xFFFFFFFF)
    idx = (np.uint64(tag) << np.uint64(40)) + np.arange(M * K, dtype=np.uint64)
    h = hash32(seed, idx)
    keep = h < np.uint32(thr) if thr < 0xFFFFFFFF else np.ones(M * K, bool)
    return torch.from_numpy(keep.reshape(M, K)).to(dev)


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _rand(shape, dtype, dev, scale=1.0, gen=None):
    return (torch.randn(shape, generator=gen, device=dev) * scale).to(dtype)


# q|k|v group: every rank x dtype x M x dropout, M ragged against the 16-row tiles (4600), not a multiple of 8
# (4601: Ut / dUt carry pad columns) and whole (4608); the FF widths (gate|up, down) on a reduced grid
CASES = [("qkv", dtype, r, M, p) for dtype in (torch.bfloat16, torch.float16) for r in (8, 16, 64)
         for M in (4600, 4601, 4608) for p in (0.0, 0.05)]
CASES += [(shape, dtype, r, M, p) for shape in ("gu", "down") for dtype, r in ((torch.bfloat16, 8), (torch.bfloat16, 64),
                                                                             (torch.float16, 64))
          for M, p in ((4600, 0.05), (4601, 0.05), (4608, 0.0))]


# the rank-tile instantiations (RT = ceil(r / 16) = 1, 2, 4, 8: csrc/lora.hip rowred_launch / colred_launch) with ragged
# ranks (r % 16 == 8: a half-used last tile), one partial row tile (M = 1, 9), a row tile past 16 (17), three LORA_SLAB
# slabs of the dA / dB partials (1025), widths whose last 64- and 256-column blocks are cut (K = 1000, N = 1032) and the
# 13B widths (5120 / 13824) at the largest rank
WIDTHS = {"qkv": (4096, 4096, 3), "gu": (4096, 11008, 2), "down": (11008, 4096, 1), "odd": (1000, 1032, 3),
          "odd2": (1032, 1000, 2), "qkv13": (5120, 5120, 3), "gu13": (5120, 13824, 2), "down13": (13824, 5120, 1)}
RANK_CASES = [("qkv", torch.bfloat16, 24, 9, 0.05), ("qkv", torch.float16, 32, 1025, 0.0),
              ("qkv", torch.bfloat16, 40, 17, 0.0), ("qkv", torch.float16, 72, 1, 0.05),
              ("qkv", torch.bfloat16, 128, 1025, 0.05), ("gu", torch.float16, 24, 17, 0.0),
              ("gu", torch.bfloat16, 72, 9, 0.05), ("gu", torch.bfloat16, 32, 1, 0.05),
              ("down", torch.bfloat16, 40, 1025, 0.05), ("down", torch.float16, 128, 9, 0.0),
              ("odd", torch.bfloat16, 72, 17, 0.05), ("odd", torch.float16, 24, 1025, 0.05),
              ("odd", torch.bfloat16, 8, 1, 0.0), ("odd2", torch.float16, 40, 9, 0.0),
              ("odd2", torch.bfloat16, 128, 17, 0.05), ("qkv13", torch.bfloat16, 128, 1025, 0.0),
              ("gu13", torch.bfloat16, 128, 17, 0.05), ("down13", torch.float16, 128, 9, 0.05)]


def _rank_tiles(r):
    return (r + 15) // 16 if r <= 32 else 4 if r <= 64 else 8


def test_lora_cases_select_every_rank_tile_instantiation():
    """guard on the parametrization: every RT bucket, full and half-used last tile, both dtypes, dropout on / off, every
    group shape and the M edges stay covered"""
    cases = [(dtype, r, M, p, WIDTHS[shape][2]) for shape, dtype, r, M, p in RANK_CASES + CASES]
    assert {_rank_tiles(c[1]) for c in cases} == {1, 2, 4, 8}
    for rt in (1, 2, 4, 8):
        rs = {c[1] for c in cases if _rank_tiles(c[1]) == rt}
        assert any(r % 16 == 8 for r in rs) and any(r % 16 == 0 for r in rs), (rt, rs)
        for dtype in (torch.bfloat16, torch.float16):
            assert any(c[0] == dtype for c in cases if _rank_tiles(c[1]) == rt), (rt, dtype)
        assert {c[3] > 0 for c in cases if _rank_tiles(c[1]) == rt} == {True, False}, rt
    assert {c[4] for c in cases} == {1, 2, 3}
    assert {1, 9, 17, 1025} <= {c[2] for c in cases}
    assert any(K % 64 and N % 64 for K, N, _ in WIDTHS.values())
    assert {WIDTHS[s][:2] for s, _, r, _, _ in RANK_CASES if r == 128} >= {(5120, 13824), (13824, 5120)}


@pytest.mark.parametrize("shape,dtype,r,M,p", CASES)
def test_lora_kernels_against_fp32_restatement(dev, shape, dtype, r, M, p):
    _check_lora_kernels(dev, *WIDTHS[shape], dtype, r, M, p)


@pytest.mark.parametrize("shape,dtype,r,M,p", RANK_CASES)
def test_lora_kernels_every_rank_tile_and_edge(dev, shape, dtype, r, M, p):
    _check_lora_kernels(dev, *WIDTHS[shape], dtype, r, M, p)


def _check_lora_kernels(dev, K, N, G, dtype, r, M, p):
    g = torch.Generator(device=dev).manual_seed(r * 7 + M)
    s, seed, tags = 2.0, 123456789 + r, [8 * 5 + i for i in range(G)]
    x = _rand((M, K), dtype, dev, 1.0, g)
    As = [_rand((r, K), dtype, dev, K ** -0.5, g) for _ in range(G)]
    Bs = [_rand((N, r), dtype, dev, 0.05, g) for _ in range(G)]
    Y = _rand((M, G * N), dtype, dev, 1.0, g)
    Ys = [Y[:, i * N:(i + 1) * N] for i in range(G)]
    dY = _rand((M, G * N), dtype, dev, 1.0, g)
    dYs = [dY[:, i * N:(i + 1) * N] for i in range(G)]
    inv = 1.0 / (1.0 - p)
    xd = [torch.where(keep_mask(seed, t, M, K, p, dev), x.float() * inv, 0.0).to(dtype).float() if p > 0 else x.float()
          for t in tags]

    # down
    U, Ut = ops.lora_down(x, As, p, seed, tags)
    Ur = torch.cat([xd[i] @ As[i].float().t() for i in range(G)], dim=1)
    assert _rel(U, Ur) < 1e-2 and torch.equal(Ut[:, :M], U.t()) and not Ut[:, M:].any()
    assert Ut.shape[1] == (M + 7) // 8 * 8
    # up-add
    Y0 = Y.clone()
    ops.lora_up_add_(U, Bs, Ys, s)
    for i in range(G):
        ref = Y0[:, i * N:(i + 1) * N].float() + s * U[:, i * r:(i + 1) * r].float() @ Bs[i].float().t()
        assert (Ys[i].float() - ref).abs().max() <= 2e-2 * ref.abs().max(), i
    # bwd-dy: twice, bit-identical
    dU, dUt, dB = ops.lora_bwd_dy(dYs, Bs, Ut, s)
    dU2, _, dB2 = ops.lora_bwd_dy(dYs, Bs, Ut, s)
    assert torch.equal(dU, dU2) and all(torch.equal(a, b) for a, b in zip(dB, dB2))
    for i in range(G):
        assert _rel(dU[:, i * r:(i + 1) * r], s * dYs[i].float() @ Bs[i].float()) < 1e-2, i
        assert _rel(dB[i], s * dYs[i].float().t() @ U[:, i * r:(i + 1) * r].float()) < 1e-2, i
    # bwd-x: twice, bit-identical
    dx0 = _rand((M, K), dtype, dev, 1.0, g)
    dx, dx2 = dx0.clone(), dx0.clone()
    dA = ops.lora_bwd_x_(x, dU, dUt, As, dx, p, seed, tags)
    dA2 = ops.lora_bwd_x_(x, dU, dUt, As, dx2, p, seed, tags)
    assert torch.equal(dx, dx2) and all(torch.equal(a, b) for a, b in zip(dA, dA2))
    ref = dx0.float()
    for i, t in enumerate(tags):
        c = dU[:, i * r:(i + 1) * r].float() @ As[i].float()
        if p > 0:
            c = torch.where(keep_mask(seed, t, M, K, p, dev), c * inv, 0.0)
        ref = ref + c
        assert _rel(dA[i], dU[:, i * r:(i + 1) * r].float().t() @ xd[i]) < 1e-2, i
    assert (dx.float() - ref).abs().max() <= 2e-2 * ref.abs().max()
    # merge (fp32 product, one rounding)
    W = _rand((N, K), dtype, dev, 0.02, g)
    Wm = ops.lora_merge_(W.clone(), As[0], Bs[0], s)
    ref = (W.float() + s * Bs[0].float() @ As[0].float()).to(dtype)
    assert (Wm.float() - ref.float()).abs().max() <= 2 * (ref.float().abs().max() * 2 ** -7)
    assert float((Wm != ref).float().mean()) < 0.01


# ------------------------------------------------------------------------------------------ one layer --
def _layer(cfg_l, dtype, dev, fuse, seed=0):
    from transformers import LlamaConfig
    torch.manual_seed(seed)
    Mo.AUTO_FUSE = bool(fuse)
    lm = Mo.LlamaForCausalLM(LlamaConfig(**cfg_l)).to(dev).to(dtype)
    if fuse:
        Mo.fuse_model(lm)
    return lm


def _cfg():
    return configs.get(load_case("micro_all")["config_name"])


def _adapted(dev, fuse, p, dtype=torch.bfloat16):
    lm = _layer(_cfg()["llama"], dtype, dev, fuse)
    L.get_peft_model(lm, L.LoraConfig(r=8, lora_alpha=16, target_modules=ALL7, lora_dropout=p))
    with torch.no_grad():
        for n, q in lm.named_parameters():
            if ".lora_B." in n:
                q.copy_(torch.randn_like(q.float()) * 0.05)
    return lm


def _run_layer(lm, x, pos, recompute, seed=777):
    lyr = lm.model.layers[0]
    lm._lora.seed = seed
    xi = x.clone().requires_grad_(True)
    out = lyr(xi, pos=pos, recompute=recompute)[0]
    go = torch.randn_like(out.float(), generator=torch.Generator(device=x.device).manual_seed(5)).to(out.dtype)
    out.backward(go)
    grads = {n: q.grad.clone() for n, q in lyr.named_parameters() if q.grad is not None}
    return out.detach(), xi.grad.clone(), grads, go


@pytest.mark.parametrize("fuse", [True, False])
def test_decoder_layer_with_seven_adapters_matches_the_merged_weights(dev, fuse):
    """p = 0: the adapted layer computes what the plain layer computes with W + s B A (restated in fp32 and
    rounded once); the adapters' gradients are dA = s B^T dW, dB = s dW A^T of that merged weight's gradient"""
    lm = _adapted(dev, fuse, 0.0).train()
    lyr = lm.model.layers[0]
    B_, S, D = 2, 40, lyr.hidden_size
    x = torch.randn(B_, S, D, device=dev).to(torch.bfloat16)
    pos = torch.arange(S, dtype=torch.int32, device=dev).repeat(B_)
    out, dx, grads, go = _run_layer(lm, x, pos, False)
    # the restatement: a plain copy of the layer with merged weights, trainable
    plain = _layer(_cfg()["llama"], torch.bfloat16, dev, fuse)
    pl = plain.model.layers[0]
    s = 2.0
    with torch.no_grad():
        for i, lin in L.layer_adapters(lyr):
            name = [k for k, m in lyr.named_modules() if m is lin][0]
            tgt = dict(pl.named_modules())[name]
            tgt.weight.copy_((lin.weight.float() + s * lin.lora_B.weight.float() @ lin.lora_A.weight.float()).to(torch.bfloat16))
        for (n, q) in pl.named_parameters():
            if not any(k in n for k in ALL7):
                q.copy_(dict(lyr.named_parameters())[n])
    for q in pl.parameters():
        q.requires_grad_(True)
    xi = x.clone().requires_grad_(True)
    out_r = pl(xi, pos=pos)[0]
    out_r.backward(go)
    assert _rel(out, out_r) < 2e-2 and _rel(dx, xi.grad) < 3e-2
    for i, lin in L.layer_adapters(lyr):
        name = [k for k, m in lyr.named_modules() if m is lin][0]
        dW = dict(pl.named_modules())[name].weight.grad.float()
        A, B = lin.lora_A.weight.float(), lin.lora_B.weight.float()
        assert _rel(grads[f"{name}.lora_A.weight"], s * B.t() @ dW) < 3e-2, name
        assert _rel(grads[f"{name}.lora_B.weight"], s * dW @ A.t()) < 3e-2, name
    assert not any(q.grad is not None for n, q in lyr.named_parameters() if ".lora_" not in n)


@pytest.mark.parametrize("fuse", [True, False])
def test_checkpointed_layer_reproduces_masks_and_gradients_bit_for_bit(dev, fuse):
    lm = _adapted(dev, fuse, 0.05).train()
    D = lm.model.layers[0].hidden_size
    x = torch.randn(2, 40, D, device=dev).to(torch.bfloat16)
    pos = torch.arange(40, dtype=torch.int32, device=dev).repeat(2)
    o1, dx1, g1, _ = _run_layer(lm, x, pos, False)
    for q in lm.parameters():
        q.grad = None
    o2, dx2, g2, _ = _run_layer(lm, x, pos, True)
    assert torch.equal(o1, o2) and torch.equal(dx1, dx2) and g1.keys() == g2.keys() and len(g1) == 14
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    for q in lm.parameters():
        q.grad = None
    o3, _, _, _ = _run_layer(lm, x, pos, False, seed=778)       # another step: other masks
    assert not torch.equal(o1, o3)


# ------------------------------------------------------------------------------------------ model --
def _mm_lora(dev, targets=ALL7, p=0.05, fuse=True):
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=fuse)
    torch.manual_seed(3)
    model.llm = L.get_peft_model(model.llm, L.LoraConfig(r=8, lora_alpha=16, target_modules=targets, lora_dropout=p))
    return model, fx


def test_a_freshly_adapted_model_computes_the_base_model_bit_for_bit(dev):
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    inp = to_dev(fx["inputs"], dev)
    base = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    ob = base(inputs=inp)
    model, _ = _mm_lora(dev)
    oa = model.eval()(inputs=inp)
    assert torch.equal(ob.logits, oa.logits) and torch.equal(ob.loss, oa.loss)


def test_bucketed_step_trains_only_the_adapters(dev):
    from macaw_llm_amd.optim import FusedAdamW
    from macaw_llm_amd.bucketed import BucketedStep
    model, fx = _mm_lora(dev)
    model.train()
    inp = to_dev(fx["inputs"], dev)
    base0 = {n: q.detach().clone() for n, q in model.llm.named_parameters() if ".lora_" not in n}
    ad0 = {n: q.detach().clone() for n, q in model.llm.named_parameters() if ".lora_" in n}
    params = [q for q in model.parameters() if q.requires_grad]
    opt = FusedAdamW(params, lr=1e-3, weight_decay=0.0)
    rt = BucketedStep(params, opt, bucket_bytes=64 << 10, model=model)
    losses = []
    for _ in range(6):
        rt.begin()
        loss = model(inputs=inp).loss
        loss.backward()
        rt.finish()
        losses.append(loss.item())
    torch.cuda.synchronize()
    rt.remove()
    now = dict(model.llm.named_parameters())
    assert all(torch.equal(base0[n], now[n]) for n in base0)
    assert all(not torch.equal(ad0[n], now[n]) for n in ad0), [n for n in ad0 if torch.equal(ad0[n], now[n])][:3]
    assert losses[-1] < losses[0], losses


def test_graphed_step_with_adapters_and_dropout_is_bit_identical_to_the_eager_step(dev):
    from macaw_llm_amd.optim import FusedAdamW
    from macaw_llm_amd.train import GraphedStep
    from macaw_llm_amd.bucketed import BucketedStep
    fx = load_case("micro_all")
    inp = to_dev(fx["inputs"], dev)

    def run(graphed):
        model, _ = _mm_lora(dev)
        model.train()
        params = [q for q in model.parameters() if q.requires_grad]
        opt = FusedAdamW(params, lr=1e-3, weight_decay=0.01)
        gs = GraphedStep(model, lambda: model(inputs=inp).loss, BucketedStep(params, opt, bucket_bytes=64 << 10))
        losses = []
        for it in range(6):
            opt.lr = 1e-3 * (1.0 - 0.1 * it)
            losses.append(float(gs.step() if graphed and it != 4 else gs.eager_step()))
        torch.cuda.synchronize()
        gs.rt.remove()
        return losses, {n: q.detach().clone() for n, q in model.llm.named_parameters()}, gs

    le, pe, _ = run(False)
    lg, pg, gs = run(True)
    assert gs.graph is not None and gs._graph_steps == 4
    assert le == lg, (le, lg)
    assert len(set(le)) > 1
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n


def test_generate_with_adapters_matches_merge_and_unload(dev):
    model, fx = _mm_lora(dev, p=0.0)
    with torch.no_grad():
        for n, q in model.llm.named_parameters():
            if ".lora_B." in n:
                q.copy_(torch.randn_like(q.float()) * 0.05)
    model.eval()
    emb = fx["inputs_embeds"].to(dev).to(torch.bfloat16)
    w0 = {n: q.detach().clone() for n, q in model.llm.named_parameters() if ".lora_" not in n}
    a = model.llm.generate(inputs_embeds=emb, max_new_tokens=12, eos_token_id=2, pad_token_id=106)
    assert all(torch.equal(w0[n], q) for n, q in model.llm.named_parameters() if n in w0)   # nothing merged in place
    ref = {}
    for _, lyr in L.lora_layers(model.llm):
        for _, lin in L.layer_adapters(lyr):
            ref[id(lin)] = (lin.weight.float() + 2.0 * lin.lora_B.weight.float() @ lin.lora_A.weight.float()
                            ).to(torch.bfloat16)
    lins = [lin for _, lyr in L.lora_layers(model.llm) for _, lin in L.layer_adapters(lyr)]
    plain = L.merge_and_unload(model.llm)
    assert plain is model.llm and not any(".lora_" in n for n, _ in plain.named_parameters())
    for lin in lins:
        d = (lin.weight.detach().float() - ref[id(lin)].detach().float()).abs()
        assert float(d.max()) <= float(ref[id(lin)].detach().float().abs().max()) * 2 ** -7
        assert float((d > 0).float().mean()) < 0.01
    b = plain.generate(inputs_embeds=emb, max_new_tokens=12, eos_token_id=2, pad_token_id=106)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ two ranks --
def _worker_lora_two_ranks(rank, world, port, q):
    import os
    import sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from golden_util import load_case
        from test_model_gpu import to_dev
        from macaw_llm_amd.optim import FusedAdamW
        from macaw_llm_amd.bucketed import BucketedStep
        from conftest import poison_allocator
        dev = torch.device("cuda:0")
        poison_allocator(256, 256)
        model, fx = _mm_lora(dev, p=0.05)
        model.train()
        h = lambda t: hashlib.sha1(t.detach().float().cpu().numpy().tobytes()).hexdigest()  # noqa: E731
        base0 = {n: h(p) for n, p in model.llm.named_parameters() if ".lora_" not in n}
        params = [p for p in model.parameters() if p.requires_grad]
        opt = FusedAdamW(params, lr=1e-3, weight_decay=0.01)
        poison_allocator(256, 256)
        rt = BucketedStep(params, opt, bucket_bytes=64 << 10, model=model)
        inp = to_dev(fx["inputs"], dev)
        mine = {k: (v[rank:rank + 1] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 else v)
                for k, v in inp.items()}
        for _ in range(3):
            rt.begin()
            model(inputs=mine).loss.backward()
            rt.finish()
        torch.cuda.synchronize()
        rt.remove()
        lora = {n: h(p) for n, p in model.llm.named_parameters() if ".lora_" in n}
        base = {n: h(p) for n, p in model.llm.named_parameters() if ".lora_" not in n}
        q.put((rank, rt.collective, lora, base, base0))
    except Exception as e:
        q.put((rank, "error", repr(e)))
    finally:
        dist.destroy_process_group()


def test_lora_two_ranks_share_one_gpu_through_gloo(dev):
    """world 2 (ZeRO-1 buckets that hold only the adapters and the MM_LLMs glue), dropout on: after three steps
    both ranks hold the same adapters bit for bit, every adapter moved, and no frozen LLaMA weight changed"""
    import torch.multiprocessing as mp
    from test_train_gpu import _free_port, _require_gloo_on_cuda
    _require_gloo_on_cuda()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_lora_two_ranks, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    assert not any(r[1] == "error" for r in res), "; ".join(str(r[2]) for r in res if r[1] == "error")
    (_, c0, lora0, base0, init0), (_, c1, lora1, base1, init1) = res
    assert c0 is True and c1 is True
    fresh, _ = _mm_lora(dev, p=0.05)            # same seed: the adapters every rank started from
    start = {n: hashlib.sha1(p.detach().float().cpu().numpy().tobytes()).hexdigest()
             for n, p in fresh.llm.named_parameters() if ".lora_" in n}
    assert lora0.keys() == lora1.keys() == start.keys() and len(start) == 14 * len(fresh.llm.model.layers)
    assert [n for n in lora0 if lora0[n] != lora1[n]] == []       # replicas: identical adapters
    assert [n for n in lora0 if lora0[n] == start[n]] == []       # every adapter trained
    assert base0 == init0 and base1 == init1 and init0 == init1   # frozen weights: bit-unchanged, identical
