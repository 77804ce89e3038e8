"""engine.DW_FILL: the decoder layer's backward with its grad-weight GEMMs computed as fillers inside the four grad-input launches
(ops.DwQueue / mk_gemm_grouped) against the same layer with the mode off.

One layer, forward + backward: B S = 2 x 384 = 768 rows, D = 768 (6 heads of 128), FF = 1024, bf16, 8 planned CUs, fused q|k|v and
gate|up storage.  The grad-input GEMMs are 768 x 1024 (12 tiles), 768 x 768 (9), 768 x 768 (9) and 768 x 768 (9) on 8 workgroups:
every one ends in a partial round, so grad-weight tiles ride in each launch.  Every tile is computed by the instruction stream
that mk_gemm's 256 x 256 kernels run on it, so the comparison is bit for bit: dx and all nine parameter gradients.

Both sides run with kernel configuration 15 forced (mk_gemm_set_cfg), the configuration that every decoder grad-weight and
grad-input GEMM has at the model's shapes (profiles/r06_gemm_shapes_per_step.csv).  Left to the automatic choice, this small layer
under 8 planned CUs sends dW(q|k|v) (27 tiles) to the 128 x 128 kernel with a K-split tail, which sums K in another order than
any whole-tile kernel: "off" would then differ from "on" in the last tile row of dW(v) for a reason that has nothing to do with
the fill mode."""
import csv
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

B, S, D, H, FF = 2, 384, 768, 6, 1024
NAMES = ["wq", "wk", "wv", "wo", "wg", "wu", "wd", "ln1", "ln2"]


def _layer(dev, dtype):
    """seeded inputs; wq / wk / wv and wg / wu are leaves that alias rows of one fused buffer each"""
    g = torch.Generator().manual_seed(11)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype).to(dev)  # noqa: E731
    wqkv, wgu = r(3 * D, D, scale=D ** -0.5), r(2 * FF, D, scale=D ** -0.5)
    w = {"wq": wqkv[:D], "wk": wqkv[D:2 * D], "wv": wqkv[2 * D:], "wo": r(D, D, scale=D ** -0.5), "wg": wgu[:FF], "wu": wgu[FF:],
         "wd": r(D, FF, scale=FF ** -0.5), "ln1": 1 + r(D, scale=0.1), "ln2": 1 + r(D, scale=0.1)}
    w = {k: v.detach().requires_grad_(True) for k, v in w.items()}
    hd = D // H
    inv = 1.0 / (10000 ** (torch.arange(0, hd, 2).float() / hd))
    emb = torch.cat((torch.einsum("i,j->ij", torch.arange(S).float(), inv),) * 2, dim=-1)
    return dict(w=w, wqkv=wqkv, wgu=wgu, x=r(B, S, D).requires_grad_(True), dout=r(B, S, D), cos=emb.cos().to(dtype).to(dev),
                sin=emb.sin().to(dtype).to(dev), pos=torch.arange(S, dtype=torch.int32).repeat(B).to(dev))


def _grads(c, recompute=False):
    """[dx, nine parameter gradients] of one forward + backward"""
    w = c["w"]
    y = eng.LlamaLayerFn.apply(c["x"], None, c["pos"], c["cos"], c["sin"], H, 1e-6, w["wq"], w["wk"], w["wv"], w["wo"], w["wg"],
                               w["wu"], w["wd"], w["ln1"], w["ln2"], c["wqkv"], c["wgu"], recompute)
    return list(torch.autograd.grad(y, [c["x"]] + [w[n] for n in NAMES], c["dout"]))


class _Mode:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = eng.DW_FILL["on"]
        eng.DW_FILL["on"], eng.DW_FILL["layers"] = self.on, 0
        L.load().mk_gemm_set_cus(8)
        L.load().mk_gemm_set_cfg(15)

    def __exit__(self, *exc):
        eng.DW_FILL["on"] = self.old
        L.load().mk_gemm_set_cus(0)
        L.load().mk_gemm_set_cfg(-1)
        ops.GRAD_DST.clear()
        ops.GRAD_DST_TAKEN.clear()


def _same(got, ref, what):
    for n, a, b in zip(["dx"] + NAMES, got, ref):
        assert a.shape == b.shape and torch.equal(a, b), f"{what}: {n} differs"
        assert torch.isfinite(a.float()).all(), f"{what}: {n} not finite"


@pytest.fixture(scope="module")
def case(dev):
    c = _layer(dev, torch.bfloat16)
    with _Mode(False):
        ops.prof_begin()
        try:
            c["ref"] = [t.clone() for t in _grads(c)]
            c["ref_flops"] = ops.prof_sum(0)[1]
        finally:
            ops.prof_end()
        assert eng.DW_FILL["layers"] == 0
    return c


def test_fill_on_against_off_is_bit_identical_and_says_so_in_the_profile(dev, case, tmp_path):
    path = str(tmp_path / "prof.csv")
    with _Mode(True):
        ops.prof_begin()
        try:
            got = _grads(case)
            ops.prof_report(path)
            flops = ops.prof_sum(0)[1]
        finally:
            ops.prof_end()
        assert eng.DW_FILL["layers"] == 1
    _same(got, case["ref"], "fill on")
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if r["kind"] == "gemm"]
    grouped = [r for r in rows if int(r["cfg"]) == 16]
    # the four grad-input launches (shapes [768, FF], [768, D] x 3 with K = D, 2 FF, D, 3 D) and nothing else in the backward
    assert sorted((int(r["N"]), int(r["K"]), int(r["launches"])) for r in grouped) == sorted(
        [(FF, D, 1), (D, 2 * FF, 1), (D, D, 1), (D, 3 * D, 1)]), grouped
    assert not [r for r in rows if int(r["layout"]) == 3 and int(r["batch"]) == 1 and int(r["cfg"]) != 16], \
        "a grad-weight GEMM ran on its own"
    # the profile counts every tile exactly once: the same GEMM FLOPs as with the mode off, and at least the twelve
    # projection GEMMs of the forward and the backward
    assert flops == case["ref_flops"] >= 3 * 2.0 * B * S * (3 * D * D + D * D + 2 * FF * D + FF * D)


def test_gradients_land_in_registered_bucket_slots_without_a_copy(dev, case):
    w = case["w"]
    with _Mode(True):
        slots = {}
        for key, t in (("wqkv", case["wqkv"]), ("wgu", case["wgu"]), ("wo", w["wo"]), ("wd", w["wd"])):
            slots[key] = torch.full(t.shape, float("nan"), dtype=t.dtype, device=dev)
            ops.GRAD_DST[(t.data_ptr(), t.numel())] = slots[key]
        got = _grads(case)
    _same(got, case["ref"], "bucket slots")
    g = dict(zip(["dx"] + NAMES, got))
    # the returned gradients ARE the slots (row slices of the fused ones): nothing was copied
    assert g["wq"].data_ptr() == slots["wqkv"].data_ptr() and g["wk"].data_ptr() == slots["wqkv"][D:].data_ptr()
    assert g["wv"].data_ptr() == slots["wqkv"][2 * D:].data_ptr()
    assert g["wg"].data_ptr() == slots["wgu"].data_ptr() and g["wu"].data_ptr() == slots["wgu"][FF:].data_ptr()
    assert g["wo"].data_ptr() == slots["wo"].data_ptr() and g["wd"].data_ptr() == slots["wd"].data_ptr()


def test_fill_with_activation_checkpointing(dev, case):
    with _Mode(True):
        got = _grads(case, recompute=True)
        assert eng.DW_FILL["layers"] == 1
    _same(got, case["ref"], "recompute")


def test_fill_inside_a_captured_graph(dev, case):
    with _Mode(True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _grads(case)                      # warm-up outside the capture (allocator pools, kernel attributes)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = _grads(case)
        for t in got:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert eng.DW_FILL["layers"] == 2
    _same(got, case["ref"], "captured graph")


def test_an_fp32_layer_keeps_the_old_path(dev, tmp_path):
    c = _layer(dev, torch.float32)
    path = str(tmp_path / "prof.csv")
    with _Mode(True):
        ops.prof_begin()
        try:
            got = _grads(c)
            ops.prof_report(path)
        finally:
            ops.prof_end()
        assert eng.DW_FILL["layers"] == 0
    with _Mode(False):
        ref = _grads(c)
    _same(got, ref, "fp32")
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if r["kind"] == "gemm"]
    assert rows and all(int(r["cfg"]) != 16 for r in rows), rows
    assert math.isfinite(sum(float(r["total_ms"]) for r in rows))
