"""GPU: the decode attention kernels -- mk_decode_step_attn and its _var, _beam, _kv8 and _kv8_var forms, mk_decode_attn --
against the fp64 reference of tests/decode_attn_ref.py at every edge of their key -> lane maps: both sides of a wave's
share, of a pass and of a trip of the online softmax, the second trip, a third one with a ragged pass (edge_positions).
Bit-identity among the forms is pinned elsewhere (test_decode_ragged_gpu, test_beam_gpu, test_prompt_lookup_gpu); here every
body meets arithmetic that is not the project's own.

Inputs (decode_attn_ref.make_case): random; ramp up (the maximum rises on every trip: every earlier sum is rescaled) and
ramp down (later keys weigh ~0, the ragged last trip is -inf padded), scores from -60 to +60; the V census (equal scores,
one-hot values inside a window of 4 hd keys per head row) and the K census (one-hot values everywhere, keys that select the
window): a key that is skipped, read twice or paired with the wrong value row moves an expectation by >= 58 bounds
(test_decode_attn_ref_cpu.py).  Cache rows behind the position hold NaN bits (kv8: NaN codes and NaN scales): a read past p
poisons the output, and an untouched row keeps its bits.

Bound, per output element (decode_attn_ref.bound):   |out - ref| <= u max(|ref|, tiny) + a o_abs
with u = 2^-8 (bf16) / 2^-11 (f16), the one rounding of the fp32 quotient; tiny = the output type's smallest normal (below it
that rounding is absolute: an expectation of 1e-15 IS 0 in f16); o_abs = sum_t p_t |v_t|; and a = decode_attn_ref.A for fp32
accumulation and __expf.  Measured a = max (|out - ref| - u max(|ref|, tiny)) / o_abs over every case of this file, on the
kernels as they were before this file existed (every test prints its own value):

    body                              bf16        f16
    one head, hd 16,  16-bit          < 0         7.7e-07        (< 0: the rounding term alone covered every element)
    one head, hd 16,  kv8             < 0         7.8e-08
    one head, hd 32,  16-bit          3.9e-08     1.4e-06
    one head, hd 32,  kv8             1.0e-06     7.8e-07
    one head, hd 64,  16-bit          1.4e-06     1.1e-06
    one head, hd 64,  kv8             2.9e-06     1.3e-07
    one head, hd 128, 16-bit          < 0         2.7e-06
    one head, hd 128, kv8             2.4e-07     1.8e-06
    four heads, 16-bit                2.5e-06     3.7e-06
    four heads, kv8                   2.7e-06     4.9e-06        <- the largest: 4.88e-06 (plain entry, random, p = 127)
    mk_decode_attn, hd 16             < 0         < 0
    mk_decode_attn, hd 128            < 0         4.2e-09
    beam, hd 16 and hd 64             < 0         < 0            (measured in the second run, with A already set)

A = 4 x the largest of them = 1.95e-5 = 2^-15.6; test_decode_attn_ref_cpu.py asserts A <= 2^-14, the value the census's
sharpness is proven for.  The two older step tests (test_kernels_gpu, test_decode_kv8_gpu) measured at most 4.1e-06.

Departures from a plain reading of the cases, each to make a check possible, none to loosen one: the bound's relative term
has the floor `tiny` (above); mk_decode_attn's V census takes as many samples as own every window (B = 2 only where two
suffice); the beam test rotates its query with decode_attn_ref.rope16, not ops.rope_, because test_beam_gpu._attn_case's
tables are random across the whole width and mk_rope reads the first half's column for both halves (the step kernels read
column d for element d) -- the appended key is compared bit for bit with rope16's to tie the two together.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_attn_ref as R  # noqa: E402

from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

H16 = [torch.bfloat16, torch.float16]
IDS16 = ["bf16", "f16"]
KV = [False, True]
KVIDS = ["16bit", "kv8"]
DEV = "cuda:0"


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _step(case, var):
    """one launch of the step kernel over `case` (kv8 if the case holds an e4m3 cache; var: sample b at its own position
    through t_off, else every sample at the one position).  Checks that nothing but row p_b of a sample's cache changed and
    that row p_b holds the value row, then returns (out, ref, o_abs) with the reference taken from ops.rope_'s query and
    the cache as it stands after the call."""
    B, H, hd, Tmax = case.B, case.H, case.hd, case.Tmax
    D = H * hd
    kv8 = case.cbytes is not None
    qkv, cos, sin = case.qkv.to(DEV), case.cos.to(DEV), case.sin.to(DEV)
    q_rot = qkv[:, :D].clone()
    ops.rope_(q_rot, cos, sin, _i32(case.ps), H, hd)
    out = torch.full((B, D), float("nan"), dtype=case.dtype, device=DEV)
    pmax = max(case.ps)
    if var:
        pos = (_i32([pmax]), _i32([p - pmax for p in case.ps]))
    else:
        assert min(case.ps) == pmax
        pos = (_i32([pmax]),)
    kw = dict(k_off=D, v_off=2 * D)
    if kv8:
        cache, scales = case.cbytes.to(DEV), case.cscales.to(DEV)
        fn = ops.decode_step_attn_kv8_var if var else ops.decode_step_attn_kv8
        fn(qkv, qkv, qkv, 3 * D, cos, sin, cache, scales, *pos, Tmax, B, H, hd, out, case.scale, **kw)
        got_b, got_s = cache.cpu(), scales.cpu()
    else:
        cache = case.cache.to(DEV)
        fn = ops.decode_step_attn_var if var else ops.decode_step_attn
        fn(qkv, qkv, qkv, 3 * D, cos, sin, cache, *pos, Tmax, B, H, hd, out, case.scale, **kw)
        got = cache.cpu()
    for b, p in enumerate(case.ps):
        rest = [t for t in range(Tmax) if t != p]
        if kv8:
            assert torch.equal(got_b[b, rest], case.cbytes[b, rest]), (b, p)
            assert torch.equal(got_s[b, rest].view(torch.int32), case.cscales[b, rest].view(torch.int32)), (b, p)
            assert bool(torch.isfinite(got_s[b, p]).all()) and bool(((got_b[b, p] & 0x7F) != R.NAN_BYTE).all()), (b, p)
        else:
            assert torch.equal(got[b, rest].view(torch.int16), case.cache[b, rest].view(torch.int16)), (b, p)
            assert torch.equal(got[b, p, D:].view(torch.int16), case.qkv[b, 2 * D:].view(torch.int16)), (b, p)
            assert bool(torch.isfinite(got[b, p].float()).all()), (b, p)
    if kv8:
        ref, o_abs = R.case_reference(case, q_rot=q_rot.cpu(), cbytes=got_b, cscales=got_s)
    else:
        ref, o_abs = R.case_reference(case, q_rot=q_rot.cpu(), rows=got)
    return out, ref, o_abs


def _label(body, kv8):
    return body.name if body in (R.FOUR16, R.FOUR8) else f"{body.name} {'kv8' if kv8 else '16-bit'}"


# ------------------------------------------------------------------ (a) one head per workgroup through _var --
@pytest.mark.parametrize("dtype", H16, ids=IDS16)
@pytest.mark.parametrize("kv8", KV, ids=KVIDS)
@pytest.mark.parametrize("family", ["random", "ramp_up", "ramp_down"])
@pytest.mark.parametrize("hd", [16, 32, 64, 128])
def test_one_head_var_meets_the_reference_at_every_edge_position(hd, family, kv8, dtype):
    """ONE launch, H = 2, sample b at edge_positions[b]"""
    body = R.one_head(hd)
    ps = R.edge_positions(body)
    assert not R.four_heads(hd, 2, len(ps))
    case = R.make_case(family, dtype, hd, 2, ps, seed=11 * hd + len(family), kv8=kv8)
    out, ref, o_abs = _step(case, var=True)
    R.assert_within(out, ref, o_abs, dtype, f"{_label(body, kv8)} | var {family}")


# ------------------------------------------------------------ (b) the plain instantiations, position by position --
@pytest.mark.parametrize("dtype", H16, ids=IDS16)
@pytest.mark.parametrize("kv8", KV, ids=KVIDS)
@pytest.mark.parametrize("hd", [16, 32, 64, 128])
def test_one_head_plain_meets_the_reference_at_every_edge_position(hd, kv8, dtype):
    """one launch per position, B = 2, H = 2: random at every edge position, ramp up on both sides of the trip boundary
    and in the third trip"""
    body = R.one_head(hd)
    tr = body.trip
    todo = [("random", p) for p in R.edge_positions(body)]
    todo += [("ramp_up", p) for p in (tr - 1, tr, tr + 1, 2 * tr + body.kpp + 1)]
    for family, p in todo:
        case = R.make_case(family, dtype, hd, 2, [p, p], seed=7 * hd + p, kv8=kv8)
        out, ref, o_abs = _step(case, var=False)
        R.assert_within(out, ref, o_abs, dtype, f"{_label(body, kv8)} | plain {family} p={p}")


# ------------------------------------------------------------------------------- (c) four heads per workgroup --
FOUR_H, FOUR_B = 32, 16


def _four(kv8):
    assert R.four_heads(128, FOUR_H, FOUR_B)
    return R.FOUR8 if kv8 else R.FOUR16


@pytest.mark.parametrize("dtype", H16, ids=IDS16)
@pytest.mark.parametrize("kv8", KV, ids=KVIDS)
@pytest.mark.parametrize("family", ["random", "ramp_up", "ramp_down"])
def test_four_heads_var_meets_the_reference_at_every_edge_position(family, kv8, dtype):
    """hd 128, H = 32, B = 16 (B H = 512): the 16 samples on the body's edge positions, the first ones repeated"""
    body = _four(kv8)
    ps = R.edge_positions(body)
    ps = [ps[b % len(ps)] for b in range(FOUR_B)]
    case = R.make_case(family, dtype, 128, FOUR_H, ps, seed=5 + len(family), kv8=kv8)
    out, ref, o_abs = _step(case, var=True)
    R.assert_within(out, ref, o_abs, dtype, f"{_label(body, kv8)} | var {family}")


@pytest.mark.parametrize("dtype", H16, ids=IDS16)
@pytest.mark.parametrize("kv8", KV, ids=KVIDS)
def test_four_heads_plain_meets_the_reference_around_the_trip(kv8, dtype):
    body = _four(kv8)
    for p in (body.trip - 1, body.trip, 2 * body.trip + body.kpp + 1):
        case = R.make_case("random", dtype, 128, FOUR_H, [p] * FOUR_B, seed=p, kv8=kv8)
        out, ref, o_abs = _step(case, var=False)
        R.assert_within(out, ref, o_abs, dtype, f"{_label(body, kv8)} | plain random p={p}")


# ------------------------------------------------------------------------------------------------- (d) census --
CENSUS = [(R.one_head(hd), k) for hd in (128, 64, 32, 16) for k in KV] + [(R.FOUR16, False), (R.FOUR8, True)]


@pytest.mark.parametrize("dtype", H16, ids=IDS16)
@pytest.mark.parametrize("body,kv8", CENSUS, ids=[_label(b, k) for b, k in CENSUS])
def test_census_every_key_is_counted_once_with_its_own_value_row(body, kv8, dtype):
    """T = trip + pass + 3 through the plain entry points; every key of [0, T) is owned by a head row.  Against the
    reference (under the bound) -- which test_decode_attn_ref_cpu.py ties to the closed forms count / T and count / window"""
    T, hd = R.census_length(body), body.hd
    if body in (R.FOUR16, R.FOUR8):
        H, B = FOUR_H, FOUR_B
    else:
        H = 8 if hd == 16 else 4
        B = -(-R.windows(T, hd) // H)
    assert R.four_heads(hd, H, B) == (body in (R.FOUR16, R.FOUR8))
    for family in ("v_census", "k_census"):
        case = R.make_case(family, dtype, hd, H, [T - 1] * B, seed=T, kv8=kv8)
        out, ref, o_abs = _step(case, var=False)
        R.assert_within(out, ref, o_abs, dtype, f"{_label(body, kv8)} | {family} T={T}")
        assert bool(((ref - case.expect).abs() <= 1e-7 * case.expect + 1e-9).all())       # (the GPU's own RoPE and append)


# --------------------------------------------------------------------------------------------------- (e) beam --
@pytest.mark.parametrize("dtype", H16, ids=IDS16)
@pytest.mark.parametrize("hd", [16, 64])
def test_beam_meets_the_reference_on_the_gathered_cache_behind_a_pass_and_a_trip(hd, dtype):
    """B = 2, K = 3, S0 = 5, a random table: the keys behind the first pass and behind the first trip come through ind[]"""
    from test_beam_gpu import _attn_case
    body = R.one_head(hd)
    B, K, H, S0 = 2, 3, 4, 5
    for p in (body.kpp + 1, body.trip + 1):
        cache, ind, gathered, qkv, cos, sin, D, Tmax = _attn_case(torch.device(DEV), dtype, B, K, H, hd, S0, p, 31 * hd + p)
        # (that case's tables are random over the whole width: the step kernels take column d for element d, which
        # rope16 restates; mk_rope takes the first half's column for both halves, as the model's tables allow)
        pos = torch.full((B * K,), p)
        q_rot = R.rope16(qkv[:, :D].cpu(), cos.cpu(), sin.cpu(), pos, hd)
        k_rot = R.rope16(qkv[:, D:2 * D].cpu(), cos.cpu(), sin.cpu(), pos, hd)
        out = torch.full((B * K, D), float("nan"), dtype=dtype, device=DEV)
        scale = hd ** -0.5
        ops.decode_step_attn_beam(qkv, qkv, qkv, 3 * D, cos, sin, cache, _i32([p]), ind, S0, Tmax, B, K, H, hd, out, scale,
                                  k_off=D, v_off=2 * D)
        rows = gathered.clone()
        rows[:, p] = cache.view(B * K, Tmax, 2 * D)[:, p]
        rows = rows.cpu()
        assert torch.equal(rows[:, p, :D].view(torch.int16), k_rot.view(torch.int16))     # rope16 is the kernel's RoPE
        ref, o_abs = R.ref16(q_rot, rows[:, :p + 1], H, hd, scale)
        R.assert_within(out, ref, o_abs, dtype, f"beam hd{hd} | random p={p}")


# ----------------------------------------------------------------------------------------- (f) mk_decode_attn --
def _attn3(q, cache, T, t_max, B, H, hd, dtype, scale):
    D = H * hd
    out = torch.full((B, D), float("nan"), dtype=dtype, device=DEV)
    ops.decode_attn(q, cache, cache, out, _i32([T - 1]), 1, t_max, B, H, hd, D, 2 * D, t_max * 2 * D, 2 * D, t_max * 2 * D, D,
                    scale, v_off=D)
    return out


@pytest.mark.parametrize("dtype", H16, ids=IDS16)
@pytest.mark.parametrize("hd", [16, 128])
def test_decode_attn_meets_the_reference_at_its_pass_and_stride_edges(hd, dtype):
    """H = 2; B = 2, or as many samples as own every window of the V census.  The query is taken as it is (no RoPE in this
    kernel) and row T - 1 holds the new rows as they are; rows behind T hold NaN bits"""
    body = R.attn3(hd)
    H = 2
    D = H * hd
    for T in R.attn3_lengths(body):
        B = max(2, -(-R.windows(T, hd) // H))
        for family in ("random", "v_census"):
            case = R.make_case(family, dtype, hd, H, [T - 1] * B, seed=3 * hd + T)
            cache = case.cache.clone()
            cache[:, T - 1] = case.qkv[:, D:]
            q = case.qkv[:, :D].contiguous()
            out = _attn3(q.to(DEV), cache.to(DEV), T, case.Tmax, B, H, hd, dtype, case.scale)
            ref, o_abs = R.ref16(q, cache[:, :T], H, hd, case.scale)
            R.assert_within(out, ref, o_abs, dtype, f"{body.name} | {family} T={T}")
            if family == "v_census":
                assert bool(((ref - case.expect).abs() <= 1e-12).all())


@pytest.mark.parametrize("dtype", H16, ids=IDS16)
def test_decode_attn_at_its_largest_t_max_and_the_refusal_one_past_it(dtype):
    """T = t_max = 15360 (60 KiB of scores in LDS) at hd 16 runs and meets the bound; t_max = 15361 returns
    MK_ERR_UNSUPPORTED and launches nothing"""
    hd, H, B, T = 16, 2, 1, R.ATTN3_T_MAX
    D = H * hd
    case = R.make_case("random", dtype, hd, H, [T - 1], seed=T)
    q = case.qkv[:, :D].contiguous()
    cache = case.rows[:, :T].contiguous()
    out = _attn3(q.to(DEV), cache.to(DEV), T, T, B, H, hd, dtype, case.scale)
    ref, o_abs = R.ref16(q, cache, H, hd, case.scale)
    R.assert_within(out, ref, o_abs, dtype, f"{R.attn3(hd).name} | random T={T}")
    big = case.rows[:, :T + 1].contiguous().to(DEV)
    sent = torch.full((B, D), 77.0, dtype=dtype, device=DEV)
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
        ops.decode_attn(q.to(DEV), big, big, sent, _i32([T]), 1, T + 1, B, H, hd, D, 2 * D, (T + 1) * 2 * D, 2 * D,
                        (T + 1) * 2 * D, D, case.scale, v_off=D)
    torch.cuda.synchronize()
    assert bool((sent == 77.0).all())
