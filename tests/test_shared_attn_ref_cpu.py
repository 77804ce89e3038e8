"""CPU: tests/shared_attn_ref.py checked against itself -- the gather that builds the plain kernel's cache for a row of a
parallel-sampling step, the rule's clamps, and the (S0, p) edge table: it must hold every way a trip of the online softmax
can lie relative to the prompt's end."""
import pytest
import torch

import decode_attn_ref as R
import shared_attn_ref as S

BODIES = [R.one_head(hd) for hd in (128, 64, 32, 16)]


def test_the_gather_builds_prompt_rows_then_tail_rows_then_nan():
    B, n, S0, Tn, D2 = 2, 3, 5, 4, 8
    prompt = torch.arange(B * S0 * D2, dtype=torch.float32).view(B, S0, D2)
    tail = -1.0 - torch.arange(B * n * Tn * D2, dtype=torch.float32).view(B * n, Tn, D2)
    for r in range(B * n):
        for L in (0, 3, S0):
            for i in (0, 2, Tn - 1):
                g = S.gather_cache(prompt, tail, r, n, L, i, L + i + 3)
                assert g.shape == (1, L + i + 3, D2)
                assert torch.equal(g[0, :L], prompt[r // n, :L])
                assert torch.equal(g[0, L:L + i], tail[r, :i])
                assert bool(torch.isnan(g[0, L + i:]).all())
    with pytest.raises(AssertionError):
        S.gather_cache(prompt, tail, 0, n, S0, 2, S0 + 2)      # no room for the appended row
    for b in range(B):                                         # the batched form is the same gather, row by row
        g = S.gather_caches(prompt, tail, b, n, 3, 2, 8)
        for j in range(n):
            one = S.gather_cache(prompt, tail, b * n + j, n, 3, 2, 8)
            assert torch.equal(torch.nan_to_num(g[j:j + 1], nan=7.0), torch.nan_to_num(one, nan=7.0))


def test_the_rules_clamps():
    assert [S.tail_row(t, 10, 4) for t in (-5, 9, 10, 11, 13, 14, 99)] == [0, 0, 0, 1, 3, 3, 3]
    assert [S.prompt_len(10, off) for off in (0, -3, -10, -11, 2)] == [10, 7, 0, 0, 10]


@pytest.mark.parametrize("body", BODIES, ids=lambda b: b.name)
def test_the_edge_table_follows_its_rule(body):
    tab = S.edge_table(body)
    assert tab == sorted(set(tab)) and all(0 <= e.S0 <= e.p for e in tab)
    ps = R.edge_positions(body)
    assert sorted({e.p for e in tab}) == ps
    for p in ps:
        want = {s for s in (0, 1, body.kpp - 1, body.kpp, body.kpp + 1, body.trip - 1, body.trip, body.trip + 1, p - 1, p)
                if 0 <= s <= p}
        assert {e.S0 for e in tab if e.p == p} == want
    assert S.Edge(0, 0) in tab                                  # no prompt, one key
    assert any(e.S0 == e.p and e.p > body.trip for e in tab)    # a first step behind more than a trip of prompt
    assert max(e.p for e in tab) == 2 * body.trip + body.kpp + 1


@pytest.mark.parametrize("body", BODIES, ids=lambda b: b.name)
def test_the_edge_table_holds_every_position_of_a_trip_relative_to_the_prompts_end(body):
    tab = S.edge_table(body)
    kinds = {e: S.trip_kinds(body, e.S0, e.p) for e in tab}
    assert any("prompt" in k for k in kinds.values())           # a trip wholly in the prompt
    assert any("tail" in k for k in kinds.values())             # a trip wholly in the tail
    assert any("straddle" in k for k in kinds.values())         # a trip that straddles S0
    assert any(k[:2] == ["prompt", "prompt"] and k[-1] != "prompt" for k in kinds.values())   # two shared trips, then others
    assert any(k[0] == "straddle" and "tail" in k for k in kinds.values())

    def straddles_at(e, unit, coarser):     # S0 inside a trip, on a multiple of `unit` but not of `coarser`
        return (e.S0 % unit == 0 and e.S0 % coarser != 0 and
                any(lo < e.S0 < hi for lo, hi in S.trips(body, e.p)))
    assert any(straddles_at(e, body.kpw, body.kpp) for e in tab), "a straddle at a wave's boundary"
    assert any(straddles_at(e, body.kpp, body.trip) for e in tab), "a straddle at a pass's boundary"
    # where the two caches meet inside the key -> lane map: in one trip a wave reads both, and in one trip some waves read
    # the prompt alone while others read the tail alone
    src = {e: S.wave_sources(body, e.S0, e.p) for e in tab}
    both, one = {"prompt", "tail"}, [{"prompt"}, {"tail"}]
    assert any(any(both in t for t in s) for s in src.values())
    assert any(any(one[0] in t and one[1] in t for t in s) for s in src.values())
    for e, s in src.items():
        for kind, t in zip(kinds[e], s):
            if kind != "straddle":
                assert all(w <= {kind} for w in t), e


@pytest.mark.parametrize("body", BODIES, ids=lambda b: b.name)
def test_a_waves_keys_of_a_trip_partition_the_trip(body):
    keys = sorted(k for w in range(R.NWV) for k in S.wave_trip_keys(body, body.trip, w))
    assert keys == list(range(body.trip, 2 * body.trip))
