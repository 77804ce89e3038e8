"""CPU: the fp64 reference, the input families and the geometry of tests/decode_attn_ref.py checked against themselves --
a second, differently written formulation of the reference, the closed forms of the census families, the leak of the K
census, the SHARPNESS of the census (a single dropped or doubled key moves the expectation far beyond the bound the kernels
are held to), and the edge positions."""
import math

import pytest
import torch

import decode_attn_ref as R
import fp8_ref

H16 = [torch.bfloat16, torch.float16]
ONE_HEAD = [R.one_head(hd) for hd in (128, 64, 32, 16)]
BODIES = ONE_HEAD + [R.FOUR16, R.FOUR8]


def census_shape(body):
    """(H, B) of the census launch of a body: the smallest that owns every window (four heads: the smallest the entry
    points send to that body)"""
    if body in (R.FOUR16, R.FOUR8):
        return 32, 16
    H = 8 if body.hd == 16 else 4
    return H, -(-R.windows(R.census_length(body), body.hd) // H)


# ---------------------------------------------------------------------------------- a second formulation --
def _e4m3(byte):
    """OCP e4m3fn from its bits"""
    s, e, m = byte >> 7, (byte >> 3) & 15, byte & 7
    if e == 15 and m == 7:
        return float("nan")
    mag = (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return -mag if s else mag


def _loop_ref(q, k, v, scale):
    """q [H][hd], k, v [T][H][hd] as nested float64 tensors of ONE sample: key by key, weights through log-sum-exp"""
    H, hd = q.shape
    T = k.shape[0]
    sc = float(torch.tensor(scale, dtype=torch.float32))
    o, o_abs = torch.zeros(H, hd, dtype=torch.float64), torch.zeros(H, hd, dtype=torch.float64)
    for h in range(H):
        s = [sc * float((q[h] * k[t, h]).sum()) for t in range(T)]
        m = max(s)
        lse = m + math.log(sum(math.exp(x - m) for x in s))
        for t in range(T):
            w = math.exp(s[t] - lse)
            o[h] += w * v[t, h]
            o_abs[h] += w * v[t, h].abs()
    return o.reshape(-1), o_abs.reshape(-1)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("hd,H,ps", [(16, 2, (0, 5, 37)), (32, 3, (1, 40)), (64, 1, (70,)), (128, 2, (33,))])
@pytest.mark.parametrize("family", ["random", "ramp_up", "ramp_down"])
def test_ref16_equals_the_key_by_key_log_sum_exp_formulation(family, hd, H, ps, dtype):
    c = R.make_case(family, dtype, hd, H, ps, seed=hd + len(ps))
    o, o_abs = R.case_reference(c)
    for b, p in enumerate(ps):
        kv = c.rows[b, :p + 1].double().view(p + 1, 2, H, hd)
        lo, la = _loop_ref(c.q_rot[b].double().view(H, hd), kv[:, 0], kv[:, 1], c.scale)
        assert bool(((o[b] - lo).abs() <= 1e-12 * (1 + la)).all()), (o[b] - lo).abs().max().item()
        assert bool(((o_abs[b] - la).abs() <= 1e-12 * (1 + la)).all())
        assert bool((o[b].abs() <= o_abs[b] * (1 + 1e-12)).all())
    # the cache before the step: rows behind p are NaN bits, rows in front are the rows the reference read
    for b, p in enumerate(ps):
        assert bool(torch.isnan(c.cache[b, p:].float()).all())
        assert torch.equal(c.cache[b, :p].view(torch.int16), c.rows[b, :p].view(torch.int16))


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("hd,H,ps", [(16, 2, (0, 5, 37)), (64, 2, (70,)), (128, 1, (33,))])
@pytest.mark.parametrize("family", ["random", "ramp_down"])
def test_ref_kv8_equals_the_key_by_key_formulation_over_hand_decoded_bytes(family, hd, H, ps, dtype):
    c = R.make_case(family, dtype, hd, H, ps, seed=3 * hd + len(ps), kv8=True)
    o, o_abs = R.case_reference(c)
    qb, sc = fp8_ref.quant_rows_bytes(c.rows.reshape(-1, hd))
    qb, sc = qb.reshape(c.B, c.Tmax, 2, H, hd), sc.reshape(c.B, c.Tmax, 2, H)
    lut = torch.tensor([_e4m3(i) for i in range(256)], dtype=torch.float64)
    for b, p in enumerate(ps):
        kv = lut[qb[b, :p + 1].long()] * sc[b, :p + 1].double()[..., None]
        lo, la = _loop_ref(c.q_rot[b].double().view(H, hd), kv[:, 0], kv[:, 1], c.scale)
        assert bool(((o[b] - lo).abs() <= 1e-12 * (1 + la)).all()), (o[b] - lo).abs().max().item()
        assert bool(((o_abs[b] - la).abs() <= 1e-12 * (1 + la)).all())
        assert torch.equal(c.cbytes[b, :p], qb[b, :p].reshape(p, 2 * H * hd))
        assert bool((c.cbytes[b, p:] == R.NAN_BYTE).all()) and bool(torch.isnan(c.cscales[b, p:]).all())
    assert bool(torch.isnan(fp8_ref.decode_bytes(torch.tensor([0x7F, 0xFF], dtype=torch.uint8))).all())
    assert bool(torch.equal(fp8_ref.decode_bytes(torch.arange(256, dtype=torch.uint8)).nan_to_num(7e7), lut.nan_to_num(7e7)))


# ------------------------------------------------------------------------------------------------ census --
@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("body,kv8", [(b, k) for b in ONE_HEAD for k in (False, True)] + [(R.FOUR16, False), (R.FOUR8, True)],
                         ids=[f"{b.name}-{'kv8' if k else '16bit'}" for b in ONE_HEAD for k in (False, True)]
                         + [R.FOUR16.name, R.FOUR8.name])
def test_census_expectations_are_the_closed_forms_and_the_k_census_does_not_leak(body, kv8, dtype):
    H, B = census_shape(body)
    T, hd = R.census_length(body), body.hd
    for family in ("v_census", "k_census"):
        c = R.make_case(family, dtype, hd, H, [T - 1] * B, seed=T, kv8=kv8)
        o, o_abs = R.case_reference(c)
        assert bool(((o - c.expect).abs() <= 1e-9).all()), (family, (o - c.expect).abs().max().item())
        assert bool(((o_abs - c.expect).abs() <= 1e-9).all())
        owned = torch.zeros(T, dtype=torch.bool)
        for r in range(B * H):
            lo, hi = R.window_of(r, T, hd)
            owned[lo:hi] = True
        assert bool(owned.all())
        if family == "k_census":            # the weight of the keys outside a head row's window
            rows = R.dequant_kv8(*fp8_ref.quant_rows_bytes(c.rows.reshape(-1, hd)), hd).reshape(c.rows.shape) if kv8 \
                else c.rows.double()
            k = rows[:, :T, :H * hd].reshape(B, T, H, hd)
            s = torch.einsum("bhd,bthd->bht", c.q_rot.double().view(B, H, hd), k) * c.scale
            p = torch.softmax(s, -1)
            for b in range(B):
                for h in range(H):
                    lo, hi = R.window_of(b * H + h, T, hd)
                    leak = 1.0 - p[b, h, lo:hi].sum().item()
                    assert abs(leak) < 1e-10, (b, h, leak)


@pytest.mark.parametrize("body", BODIES, ids=[b.name for b in BODIES])
def test_census_is_sharp_a_single_dropped_or_doubled_key_moves_it_eight_bounds(body):
    """For the census shape of every body: removing or doubling ANY single key t of [0, T) moves the expectation of the
    head row that owns t, at the element t mod hd, by at least 8x the bound at a = A_CAP -- in the closed forms, which the
    test above ties to the reference.  Sampled: every 7th key and both ends of every window."""
    T, hd = R.census_length(body), body.hd
    worst = {}
    for j in range(R.windows(T, hd)):
        lo, hi = R.window_of(j, T, hd)
        n = hi - lo
        cnt = R.census_counts(lo, hi, hd)
        keys = sorted({lo, hi - 1} | set(range(lo + (-lo) % 7, hi, 7)))
        for dtype in H16:
            for fam, e0, total in (("v", cnt / T, T), ("k", cnt / n, n)):
                bnd = R.bound(e0, e0, dtype, a=R.A_CAP)
                for t in keys:
                    d = t % hd
                    for step in (-1, 1):
                        if total + step == 0:
                            continue            # (a window of one key: nothing left to normalise)
                        c1 = cnt.clone()
                        c1[d] += step
                        ratio = ((c1 / (total + step) - e0).abs() / bnd)[d].item()
                        worst[dtype, fam] = min(worst.get((dtype, fam), float("inf")), ratio)
    print(f"{body.name} T={T}: smallest move / bound {worst}")
    assert worst and min(worst.values()) >= 8.0, worst


def test_a_is_within_the_cap_the_sharpness_was_proven_for():
    assert 0 < R.A <= R.A_CAP == 2.0 ** -14


# ---------------------------------------------------------------------------------------------- geometry --
@pytest.mark.parametrize("body", BODIES, ids=[b.name for b in BODIES])
def test_edge_positions_are_sorted_unique_and_inside_three_trips(body):
    ps = R.edge_positions(body)
    assert ps == sorted(set(ps)) and ps[0] == 0 and ps[-1] == 2 * body.trip + body.kpp + 1
    assert {body.trip - 1, body.trip, body.trip + 1, body.kpp, 2 * body.trip} <= set(ps)
    assert len(ps) <= 14


def test_geometry_table():
    assert [(b.kpw, b.kpp, b.trip) for b in ONE_HEAD] == [(4, 32, 256), (8, 64, 512), (16, 128, 1024), (32, 256, 2048)]
    assert (R.FOUR16.kpw, R.FOUR16.kpp, R.FOUR16.trip) == (1, 8, 64)
    assert (R.FOUR8.kpw, R.FOUR8.kpp, R.FOUR8.trip) == (2, 16, 128)
    assert [R.attn3(hd).kpp for hd in (128, 64, 32, 16)] == [16, 32, 64, 128]
    assert [R.census_length(b) for b in BODIES] == [291, 579, 1155, 2307, 75, 147]
    assert R.ATTN3_T_MAX == 15360
    assert R.four_heads(128, 32, 16) and not R.four_heads(128, 4, 16) and not R.four_heads(64, 32, 16)
