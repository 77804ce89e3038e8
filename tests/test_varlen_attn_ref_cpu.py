"""No GPU: the reference of the variable-length causal forward (tests/varlen_attn_ref.py) against attn_ref.attention_ref
with a key mask where the two rules coincide, its dead rows, and the host side of a continued generate() call --
engine.chunk_layout against hand-written tables."""
import math

import pytest
import torch

import attn_ref as R
import varlen_attn_ref as V

from macaw_llm_amd import engine as eng

H, HD = 2, 16


def _inputs(B, Lq, Lk, seed=7):
    q, k, v, _ = R.make_inputs(seed, torch.bfloat16, B, H, Lq, Lk, HD)
    return q, k, v


@pytest.mark.parametrize("Lq,Lk,shift,k_len", [(9, 40, 31, [40, 33, 32]), (17, 17, 0, [17, 5, 1]), (6, 70, 3, [9, 4, 5])])
def test_varlen_ref_is_the_masked_causal_reference_where_all_samples_share_the_shift(Lq, Lk, shift, k_len):
    """k_len[b] - q_len[b] = shift for every sample: the rows i < q_len[b] see keys j <= i + shift -- attention_ref on
    Lk' = Lq + shift keys, causal, with a key mask that cuts sample b's keys at k_len[b] (rows past q_len[b] are dead in
    the variable-length rule and compared as such)"""
    B = len(k_len)
    q_len = [kl - shift for kl in k_len]
    assert all(0 < a <= Lq for a in q_len)
    q, k, v = _inputs(B, Lq, Lk)
    scale = 1 / math.sqrt(HD)
    got = V.varlen_ref(q, k, v, H, scale, q_len, k_len)
    Lk2 = Lq + shift
    km = torch.zeros(B, Lk2, dtype=torch.int32)
    for b, kl in enumerate(k_len):
        km[b, :kl] = 1
    ref = R.attention_ref(q, k[:, :Lk2], v[:, :Lk2], H, scale, causal=True, kmask=km)
    for b, ql in enumerate(q_len):
        torch.testing.assert_close(got["o"][b, :ql], ref["o"][b, :ql], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(got["lse"][b, :, :ql], ref["lse"][b, :, :ql], rtol=1e-5, atol=1e-6)
        assert bool((got["o"][b, ql:] == 0).all()) and bool(torch.isneginf(got["lse"][b, :, ql:]).all())


def test_varlen_ref_dead_rows_clamps_and_the_census():
    Lq, Lk = 7, 12
    q, k, v = _inputs(4, Lq, Lk, seed=9)
    q_len, k_len = [7, 0, 5, 99], [4, 9, -2, 99]        # 3 dead leading rows; no query; no key; clamped to (7, 12)
    got = V.varlen_ref(q, k, v, H, 0.25, q_len, k_len)
    vis = V.visible(q_len, k_len, Lq, Lk)
    assert vis[0].sum(-1).tolist() == [0, 0, 0, 1, 2, 3, 4]
    assert int(vis[1].sum()) == 0 and int(vis[2].sum()) == 0
    assert vis[3].sum(-1).tolist() == [6, 7, 8, 9, 10, 11, 12]
    alive = vis.any(-1)
    assert torch.equal(torch.isfinite(got["lse"]), alive[:, None, :].expand(4, H, Lq))
    assert bool((got["o"][~alive] == 0).all()) and not torch.isnan(got["o"]).any()
    # poison behind the lengths never enters the reference
    k2, v2, q2 = k.clone(), v.clone(), q.clone()
    k2[0, 4:], v2[0, 4:], q2[2, 5:] = float("nan"), float("nan"), float("nan")
    again = V.varlen_ref(q2, k2, v2, H, 0.25, q_len, k_len)
    assert torch.equal(again["o"], got["o"]) and torch.equal(again["lse"], got["lse"])
    n, lse, o = V.census_expect(v2, H, q_len, k_len, Lq)
    assert torch.equal(n, vis.sum(-1)) and not torch.isnan(o).any()
    z = V.varlen_ref(torch.zeros_like(q), k, v, H, 0.25, q_len, k_len)
    a3 = alive[:, None, :].expand(4, H, Lq)
    torch.testing.assert_close(z["lse"][a3].double(), lse[a3], rtol=0, atol=1e-6)
    torch.testing.assert_close(z["o"].double(), o, rtol=0, atol=1e-6)


def test_the_gpu_cases_cross_the_kernel_edges():
    """every case has Lq = its largest q_len, and together they put a length on each side of the 32-key sub-block, the
    64-key tile, the 32-row wave slice and the 128-row block"""
    qs = [a for _, lens in V.CASES for a, _ in lens]
    ks = [b for _, lens in V.CASES for _, b in lens]
    for Lq, lens in V.CASES:
        assert Lq == max(a for a, _ in lens)
    assert {31, 32, 33} <= set(qs) and {129, 130} & set(qs) and 0 in qs
    assert {64, 65} <= set(ks) and {95, 96, 97} <= set(ks) and any(b < a for _, lens in V.CASES for a, b in lens)


# ------------------------------------------------------------------------------------ engine.chunk_layout --
def _masks():
    return torch.tensor([[0, 0, 1, 1, 1],          # left padding, v = 3
                         [1, 1, 0, 0, 0],          # right padding, v = 2
                         [1, 0, 1, 0, 1],          # holes, v = 3
                         [0, 0, 0, 1, 0],          # v = 1
                         [1, 1, 1, 1, 1]])         # v = 5


def test_chunk_layout_against_hand_written_tables():
    cached = [10, 4, 7, 20, 0]
    n_valid = (_masks() != 0).sum(1).tolist()
    assert n_valid == [3, 2, 3, 1, 5]
    ck, pos, last, S0n, t_off = eng.chunk_layout(cached, n_valid)
    for t in (ck.q_len, ck.k_len, ck.slot, pos, t_off):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert last.dtype == torch.int64
    assert ck.q_len.tolist() == [4, 3, 4, 2, 6] == list(ck.q_host)           # n_b = 1 + v_b: the pending token leads
    assert ck.k_len.tolist() == [14, 7, 11, 22, 6] == list(ck.k_host)         # C_b + n_b
    assert ck.Lk == S0n == 22
    assert ck.slot.tolist() == [[10, 11, 12, 13, -1, -1],
                                [4, 5, 6, -1, -1, -1],
                                [7, 8, 9, 10, -1, -1],
                                [20, 21, -1, -1, -1, -1],
                                [0, 1, 2, 3, 4, 5]]
    assert pos.view(5, 6).tolist() == [[10, 11, 12, 13, 13, 13],
                                       [4, 5, 6, 6, 6, 6],
                                       [7, 8, 9, 10, 10, 10],
                                       [20, 21, 21, 21, 21, 21],
                                       [0, 1, 2, 3, 4, 5]]
    assert last.tolist() == [0 * 6 + 3, 1 * 6 + 2, 2 * 6 + 3, 3 * 6 + 1, 4 * 6 + 5]
    assert t_off.tolist() == [-8, -15, -11, 0, -16]                         # k_len - S0': Ragged.t_off's meaning
    # the decode steps that follow: step t of sample b runs at row S0' + t + t_off[b] = k_len[b] + t
    assert [S0n + o for o in t_off.tolist()] == ck.k_len.tolist()


def test_chunk_layout_one_new_token_and_equal_histories():
    ck, pos, last, S0n, t_off = eng.chunk_layout([5, 5], [1, 1])
    assert ck.q_len.tolist() == [2, 2] and ck.k_len.tolist() == [7, 7] and S0n == 7 and t_off.tolist() == [0, 0]
    assert ck.slot.tolist() == [[5, 6], [5, 6]] and pos.tolist() == [5, 6, 5, 6] and last.tolist() == [1, 3]


def test_chunk_layout_refuses_what_it_cannot_lay_out():
    with pytest.raises(ValueError, match="no valid token"):
        eng.chunk_layout([3, 3], [2, 0])
    with pytest.raises(ValueError, match="cached"):
        eng.chunk_layout([3], [2, 1])
    with pytest.raises(ValueError, match="negative"):
        eng.chunk_layout([3, -1], [2, 1])
