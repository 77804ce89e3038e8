"""The reference the fused-attention edge tests are held to (tests/attn_ref.py) is itself checked here, on the CPU: against
F.scaled_dot_product_attention on the rows that have a visible key, its rows without a visible key (o = 0, lse = -inf,
zero gradients), NaN-freedom at every shape the GPU tests use, and the census identity (q = 0: lse = log(n_visible),
o = mean of the visible v rows)."""
import pytest
import torch
import torch.nn.functional as F

import attn_ref as R

B, H, HD = 3, 3, 16            # (the reference does not depend on head_dim: a small one keeps this file quick)
ALL_CASES = [(Lq, Lk, c, m) for (Lq, Lk, c) in R.CENSUS_SHAPES for m in R.CENSUS_MASKS] + R.BWD_EDGE_CASES


def _finite_or_neg_inf_lse(out):
    for name, t in out.items():
        if name == "lse":
            assert not torch.isnan(t).any() and not torch.isposinf(t).any(), name
        else:
            assert torch.isfinite(t).all(), name


@pytest.mark.parametrize("Lq,Lk,causal,mask", ALL_CASES)
def test_reference_is_nan_free_and_agrees_with_sdpa(Lq, Lk, causal, mask):
    q, k, v, do = R.make_inputs(Lq * 13 + Lk, torch.bfloat16, B, H, Lq, Lk, HD)
    km = R.kmask_pattern(mask, B, Lk)
    scale = HD ** -0.5
    out = R.attention_ref(q, k, v, H, scale, causal=causal, kmask=km, dout=do)
    _finite_or_neg_inf_lse(out)
    vis = R.visible(B, Lq, Lk, causal, km)
    alive = vis.any(-1)                                            # [B, Lq]
    # rows without a visible key: o = 0, lse = -inf, dq = 0 -- exactly
    dead = ~alive
    assert (out["o"][dead] == 0).all() and (out["dq"][dead] == 0).all()
    assert (out["lse"].transpose(1, 2)[dead] == float("-inf")).all()
    assert torch.isfinite(out["lse"].transpose(1, 2)[alive]).all()
    # keys no query sees: dk = dv = 0 exactly
    unseen = ~vis.any(1)                                           # [B, Lk]
    assert (out["dk"][unseen] == 0).all() and (out["dv"][unseen] == 0).all()
    # the live rows of every sample: torch's own attention and its autograd (a dead row adds nothing to dk, dv, so the
    # sample's dk and dv are those of its live rows alone)
    for b in range(B):
        rows = alive[b]
        n = int(rows.sum())
        if n == 0:
            continue
        qf, kf, vf = (t.float().view(1, L, H, HD).transpose(1, 2).clone().requires_grad_(True)
                      for t, L in ((q[b][rows], n), (k[b], Lk), (v[b], Lk)))
        ref = F.scaled_dot_product_attention(qf, kf, vf, attn_mask=vis[b][rows][None, None], scale=scale)
        ref.backward(do[b][rows].float().view(1, n, H, HD).transpose(1, 2))
        back = lambda t, L: t.transpose(1, 2).reshape(L, H * HD)  # noqa: E731
        torch.testing.assert_close(out["o"][b][rows], back(ref.detach(), n), rtol=1e-5, atol=1e-5)
        for name, got, g, L in (("dq", out["dq"][b][rows], qf.grad, n), ("dk", out["dk"][b], kf.grad, Lk),
                                ("dv", out["dv"][b], vf.grad, Lk)):
            torch.testing.assert_close(got, back(g, L), rtol=1e-4, atol=1e-5, msg=name)


@pytest.mark.parametrize("mask", R.CENSUS_MASKS)
@pytest.mark.parametrize("Lq,Lk,causal", R.CENSUS_SHAPES)
def test_census_identity_holds_for_the_reference(Lq, Lk, causal, mask):
    """q = 0: lse = log(n_visible) and o = the mean of the visible v rows; the fp32 reference meets the bound the kernels
    are held to (1e-5 on lse) with room to spare, and the n = 0 rows are exact"""
    q, k, v, do = R.make_inputs(Lq * 7 + Lk, torch.float16, B, H, Lq, Lk, HD, zero_q=True)
    km = R.kmask_pattern(mask, B, Lk)
    out = R.attention_ref(q, k, v, H, HD ** -0.5, causal=causal, kmask=km, dout=do)
    _finite_or_neg_inf_lse(out)
    n, lse, o = R.census_expect(v, H, Lq, causal, km)
    assert int(n.max()) <= 600
    dead = (n == 0)[:, None, :].expand(B, H, Lq)
    assert (out["lse"][dead] == float("-inf")).all()
    if (~dead).any():
        assert (out["lse"][~dead].double() - lse[~dead]).abs().max().item() <= 2e-6
    assert (out["o"].double() - o).abs().max().item() <= 1e-5
    assert (out["o"][n == 0] == 0).all()
    assert (out["dk"] == 0).all()                                  # dk = dS^T q with q = 0


def test_causal_rule_and_mask_patterns():
    vis = R.visible(1, 3, 5, True, None)[0]                        # Lk - Lq = 2: row i sees keys 0 .. i + 2
    assert vis.sum(-1).tolist() == [3, 4, 5]
    vis = R.visible(1, 5, 3, True, None)[0]                        # Lk - Lq = -2: rows 0, 1 see nothing
    assert vis.sum(-1).tolist() == [0, 0, 1, 2, 3]
    pads = [int((R.kmask_pattern(m, 3, 200)[b] == 0).sum()) for m in ("padA", "padB") for b in range(3)]
    assert pads == [1, 31, 32, 33, 64, 0]
    hole = R.kmask_pattern("hole", 3, 200)
    assert (hole[0, 40:70] == 0).all() and hole[0].sum() == 170 and hole[1].sum() == 0 and hole[2].sum() == 200
    assert R.kmask_pattern("padB", 3, 33)[0].sum() == 0 and R.kmask_pattern("none", 3, 9) is None
