"""The case table of tests/test_gemm_plans_gpu.py (tests/gemm_cases.py) checked against the plan rules restated beside it,
and its float64 reference checked against torch on views it does not use itself.

This guards the TABLE against arithmetic slips: that every row really is the "walking + eighths" or "split with an empty
piece" problem its label says, and that every plan named for sections A and B has a row.  It is NOT a test of the launcher:
the rules in gemm_cases.py are a restatement of csrc/gemm.hip (mk_gemm), and a deliberate change of the launcher's rules
updates both.
"""
import torch

import gemm_cases as G


def test_every_256_tile_row_is_the_plan_its_label_says():
    for n, M, N, K, ldc, plan_k, plan_red, on_v9 in G.A_ROWS:
        assert G.label256(n, M, N, False) == plan_k, (n, M, N)
        assert G.label256(n, M, N, True) == plan_red, (n, M, N)
        assert K in (128, 192, 448) and ldc > N
        if on_v9:      # cfg 15: whole tiles only, and at least one round of them, or the launch is v7's
            assert M % 256 == 0 and N % 256 == 0 and ldc % 4 == 0
            assert G.plan256(n, M, N, False)[0] >= n and G.plan256(n, M, N, True)[0] >= n


def test_every_256_tile_plan_has_a_row():
    have = {r[5] for r in G.A_ROWS} | {r[6] for r in G.A_ROWS}
    assert have == set(G.A_PLANS)
    v9 = {r[5] for r in G.A_ROWS if r[7]} | {r[6] for r in G.A_ROWS if r[7]}
    assert v9 == set(G.A_PLANS)                       # the ragged row repeats a plan of a whole-tile row
    assert {r[3] for r in G.A_ROWS} == {128, 192, 448}
    # the one row with edges inside the tiles has a C pitch that is no multiple of 8
    ragged = [r for r in G.A_ROWS if r[1] % 256 or r[2] % 256]
    assert len(ragged) == 1 and ragged[0][4] % 8 != 0


def test_the_automatic_choice_shapes_are_9_16_and_17_tiles():
    assert [G.cdiv(M, 256) * G.cdiv(N, 256) for M, N, _ in G.AUTO_SHAPES] == [9, 16, 17]


def test_every_k_split_row_is_the_plan_its_label_says():
    for cfg, n, M, N, K, plan in G.B_ROWS:
        for a_red, b_red in G.b_layouts(cfg):
            p = G.plan128(n, M, N, K, a_red, b_red)
            assert p["cfg"] == cfg and p["R"] == 1, (cfg, K)
            assert G.label128(n, M, N, K, a_red, b_red) == plan, (cfg, K)
    for cfg, plans in G.B_PLANS.items():
        have = {r[5] for r in G.B_ROWS if r[0] == cfg}
        assert set(plans) <= have, (cfg, set(plans) - have)
    # the K list of cfg 5 runs on cfg 7 as well
    assert {r[4] for r in G.B_ROWS if r[0] == 5} <= {r[4] for r in G.B_ROWS if r[0] == 7}


def test_k_split_piece_shapes():
    """the three piece shapes by hand: 18 K-tiles in 9 pieces of 2; 7 in 3, 3, 1; 9 in 3, 3, 3 and an empty fourth"""
    p = G.plan128(8, 2176, 128, 1152, False, False)
    assert (p["Tb"], p["dp"], p["sp"], p["kpp"], p["need"]) == (17, 16, 9, 2, 4096 + 9 * 65536)
    p = G.plan128(8, 2176, 128, 448, False, False)
    assert (p["sp"], p["kpp"], p["nkt"]) == (3, 3, 7)
    p = G.plan128(8, 2176, 128, 576, False, True)
    assert (p["sp"], p["kpp"], p["nkt"]) == (4, 3, 9)
    p = G.plan128(8, 2176, 128, 128, True, False)
    assert (p["sp"], p["dp"], p["need"]) == (1, 17, 0)
    p = G.plan128(8, 4224, 128, 288, True, True)
    assert (p["cfg"], p["Tb"], p["dp"], p["sp"], p["kpp"], p["nkt"]) == (7, 33, 32, 4, 3, 9)


def test_batched_patterns_hit_the_fold_the_way_section_c_wants():
    for name in G.C_PATTERNS:
        p = G.c_problem(name, torch.bfloat16)
        assert p.nbatch == (3 if name == "shared" else 6)
        all_cus = G.plan128(256, p.M, p.N, p.K, p.a_red, p.b_red, p.nbatch)
        eight = G.plan128(8, p.M, p.N, p.K, p.a_red, p.b_red, p.nbatch)
        if name.startswith("scores"):
            assert all_cus["sp"] == 1 and eight["sp"] == 1 and all_cus["nkt"] == (1 if name == "scores" else 2)
            assert p.M % 128 != 0
            continue
        # all CUs: fewer tiles than slots, the split takes the whole problem
        assert all_cus["sp"] >= 2 and all_cus["dp"] == 0, name
        # 8 CUs: whole tiles and tail tiles, the tail in a later batch than the first whole tiles
        assert eight["sp"] >= 2 and 0 < eight["dp"] < eight["Tb"], name
        assert eight["dp"] // eight["per"] == p.nbatch - 1, name
        assert eight["need"] <= 72 << 20
    assert G.plan128(8, 648, 64, 320, True, True, 6)["cfg"] == 7
    for name, (sizes, n) in G.C_V7.items():
        p = G.c_problem(name, torch.bfloat16, sizes)
        assert p.M > 128 and p.N > 128 and p.K >= 128 and p.K % 64 == 0, name       # legal on the 256 x 256 kernel
        dp, tail, walk = G.plan256(n or 256, p.M, p.N, p.a_red, p.nbatch)
        assert tail is not None and walk == 0, name
        assert dp > 0 or n == 0, name


def test_reference_agrees_with_torch_on_the_semantic_views():
    """the index-arithmetic reference against einsum on the buffers' own [B, H, ...] shapes (which it never uses)"""
    dt = torch.bfloat16
    p = G.c_problem("scores", dt)
    idx, val = p.reference()
    q = p.A.double().view(2, 136, 3, 64)
    k = p.B.double().view(2, 136, 3, 64)
    want = torch.einsum("bshd,bthd->bhst", q, k) / 8.0
    got = torch.full((p.C.numel(),), float("nan"), dtype=torch.float64)
    got[idx] = val
    got = got.view(p.C.shape)
    assert torch.allclose(got[:, :, :136, :136], want, rtol=1e-12, atol=1e-12)
    assert torch.isnan(got[:, :, 136:]).all() and torch.isnan(got[:, :, :, 136:]).all()
    assert idx.unique().numel() == idx.numel() == 6 * 136 * 136

    p = G.c_problem("dstq", dt)
    idx, val = p.reference()
    Lk, Lq, hd, D = 648, 320, 64, 192
    P = p.A.double()[..., :Lk]                                     # [B, H, Lq, Lk]
    X = p.B.double()[..., :D].reshape(2, Lq, 3, hd)                # q: the first third
    want = torch.einsum("bhqk,bqhd->bkhd", P, X).reshape(2, Lk, D)
    got = torch.full((p.C.numel(),), float("nan"), dtype=torch.float64)
    got[idx] = val
    got = got.view(p.C.shape)
    assert torch.allclose(got[:, :Lk, D:2 * D], want, rtol=1e-12, atol=1e-12)
    assert torch.isnan(got[:, Lk:]).all() and torch.isnan(got[:, :, :D]).all() and torch.isnan(got[:, :, 2 * D:]).all()

    p = G.c_problem("shared", dt)
    idx, val = p.reference()
    Gr, E = 264, 192
    x = p.A.double()[:, 1:]
    W = p.B.double()[E:]
    want = torch.nn.functional.gelu(x @ W.t() + p.bias.double()) + p.R.double()[1:]
    got = torch.full((p.C.numel(),), float("nan"), dtype=torch.float64)
    got[idx] = val
    got = got.view(p.C.shape)
    assert torch.allclose(got[:, 1:Gr + 1, :E], want, rtol=1e-9, atol=1e-9)
    assert torch.isnan(got[:, 0]).all() and torch.isnan(got[:, Gr + 1:]).all() and torch.isnan(got[:, :, E:]).all()


def test_reference_of_a_single_product_with_the_full_epilogue():
    for a_red, b_red in G.LAYOUTS:
        p = G.single(torch.float16, 200, 104, 128, a_red, b_red, "bias+gelu+residual+accumulate")
        idx, val = p.reference()
        A = p.A.double()[:, :200].t() if a_red else p.A.double()
        B = p.B.double()[:, :104] if b_red else p.B.double().t()
        want = torch.nn.functional.gelu(A @ B + p.bias.double()) + p.R.double()[:, :104] + p.C.double()[:, :104]
        got = torch.full((p.C.numel(),), float("nan"), dtype=torch.float64)
        got[idx] = val
        got = got.view(p.C.shape)
        assert torch.allclose(got[:, :104], want, rtol=1e-9, atol=1e-9)
        assert torch.isnan(got[:, 104:]).all()
