"""mk_flash_attn_varlen_fwd (csrc/attention_impl.inc: flash_fwd_kernel over FlashVarlenArgs) -- the causal fused forward
with per-sample lengths read on the device -- against the fp32 reference of tests/varlen_attn_ref.py.

Every launch uses the layout of a continued generate() call: q a column slice of a fused [B * Lq][3D] projection
buffer, k / v the two halves of a [B][t_max][2D] cache with t_max = Lk + 37 rows, o and lse NaN-prefilled (a dead row
must be WRITTEN as 0 / -inf).  Per case:

  random   o within the project's bound for the fused attention (_close of test_attention_edges_gpu.py: rtol 8e-3 of
           max|ref| + 8e-3), lse within rtol 1e-4 / atol 2e-4, dead rows exactly 0 and -inf;
  census   q = 0: lse = log(n_visible) and o = the mean of the visible v rows (pins the visibility rule exactly);
  poison   k / v rows >= k_len[b] and q rows >= q_len[b] NaN: bit-identical to the run where they are finite;
  batch    sample b of the batched launch bit-identical to the same launch with B = 1 on that sample;
and the entry point's domain / argument checks, after which nothing has been touched."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402
import attn_ref as R  # noqa: E402
import varlen_attn_ref as V  # noqa: E402

H = 2
SLACK = 37
NAN = float("nan")
H16 = [torch.bfloat16, torch.float16]
IDS = [f"Lq{Lq}" for Lq, _ in V.CASES]


def _close(got, ref, what=""):
    """test_attention_edges_gpu._close: rtol 8e-3 of max|ref| + 8e-3"""
    got = got.float().cpu()
    ref = ref.float()
    err = (got - ref).abs().max().item()
    lim = 8e-3 + 8e-3 * ref.abs().max().item()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


@functools.lru_cache(maxsize=None)
def _case(ci, dtype, hd, zero_q=False):
    """(q, k, v, q_len, k_len, Lq, Lk) of case ci on the CPU -- seeded, built once, never modified"""
    Lq, lens = V.CASES[ci]
    q_len, k_len = [a for a, _ in lens], [b for _, b in lens]
    Lk = max(k_len)
    q, k, v, _ = R.make_inputs(4100 + 10 * ci + hd, dtype, len(lens), H, Lq, Lk, hd, zero_q=zero_q)
    return q, k, v, q_len, k_len, Lq, Lk


@functools.lru_cache(maxsize=None)
def _ref(ci, dtype, hd):
    q, k, v, q_len, k_len, _, _ = _case(ci, dtype, hd)
    return V.varlen_ref(q, k, v, H, hd ** -0.5, q_len, k_len)


def _launch(dev, hd, q, k, v, q_len, k_len, Lq, Lk, fill, samples=None):
    """one launch on the samples `samples` (all by default); rows of the cache at or past k_len[b] (the 37 slack rows
    among them) and rows of q at or past q_len[b] hold `fill`.  Returns (o [B, Lq, D], lse [B, H, Lq]) on the CPU."""
    D = H * hd
    samples = list(range(q.shape[0])) if samples is None else samples
    B, t_max = len(samples), Lk + SLACK
    qkv = torch.full((B * Lq, 3 * D), fill, dtype=q.dtype, device=dev)
    cache = torch.full((B, t_max, 2 * D), fill, dtype=q.dtype, device=dev)
    for i, b in enumerate(samples):
        ql, kl = min(max(q_len[b], 0), Lq), min(max(k_len[b], 0), Lk)
        qkv.view(B, Lq, 3 * D)[i, :ql, :D] = q[b, :ql].to(dev)
        cache[i, :kl, :D] = k[b, :kl].to(dev)
        cache[i, :kl, D:] = v[b, :kl].to(dev)
    o = torch.full((B, Lq, D), NAN, dtype=q.dtype, device=dev)
    lse = torch.full((B, H, Lq), NAN, dtype=torch.float32, device=dev)
    ql_d = torch.tensor([q_len[b] for b in samples], dtype=torch.int32, device=dev)
    kl_d = torch.tensor([k_len[b] for b in samples], dtype=torch.int32, device=dev)
    ops.flash_attn_varlen_fwd(qkv, cache, cache, o, ql_d, kl_d, B, H, Lq, Lk, hd, 3 * D, Lq * 3 * D, 2 * D,
                              t_max * 2 * D, 2 * D, t_max * 2 * D, D, Lq * D, hd ** -0.5, lse=lse, v_off=D)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def _dead_rows_exact(o, lse, q_len, k_len, Lq, what):
    for b, (ql, kl) in enumerate(zip(q_len, k_len)):
        dead = torch.ones(Lq, dtype=torch.bool)
        dead[max(ql - kl, 0):ql] = False
        assert bool((o[b, dead].float() == 0).all()), f"{what}: sample {b}: o of a row without a key is exactly 0"
        assert bool(torch.isneginf(lse[b][:, dead]).all()), f"{what}: sample {b}: lse of such a row is -inf"
        assert bool(torch.isfinite(lse[b][:, ~dead]).all()), f"{what}: sample {b}: a live row has a finite lse"


@pytest.mark.parametrize("ci", range(len(V.CASES)), ids=IDS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "fp16"])
def test_varlen_forward_matches_the_reference_on_random_data(dev, dtype, hd, ci):
    q, k, v, q_len, k_len, Lq, Lk = _case(ci, dtype, hd)
    ref = _ref(ci, dtype, hd)
    o, lse = _launch(dev, hd, q, k, v, q_len, k_len, Lq, Lk, 0.0)
    what = f"case {ci} {dtype} hd {hd}"
    assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any(), f"{what}: every row is written"
    _dead_rows_exact(o, lse, q_len, k_len, Lq, what)
    _close(o, ref["o"], what + " o")
    live = torch.isfinite(ref["lse"])
    assert torch.equal(torch.isneginf(lse), ~live), what
    torch.testing.assert_close(lse[live], ref["lse"][live], rtol=1e-4, atol=2e-4)


@pytest.mark.parametrize("ci", range(len(V.CASES)), ids=IDS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "fp16"])
def test_varlen_census_pins_the_visibility_rule(dev, dtype, hd, ci):
    """q = 0: one key too many or too few among n moves lse by more than 1 / (n + 1) >= 1 / 334; the bound is 1e-5 + the
    fp32 rounding of log(n) -- and a 16-bit rounding of o, the mean of n 16-bit values"""
    q, k, v, q_len, k_len, Lq, Lk = _case(ci, dtype, hd, True)
    n, lse_x, o_x = V.census_expect(v, H, q_len, k_len, Lq)
    o, lse = _launch(dev, hd, q, k, v, q_len, k_len, Lq, Lk, NAN)
    what = f"census case {ci} {dtype} hd {hd}"
    alive = n > 0
    assert torch.equal(torch.isneginf(lse), ~alive[:, None, :].expand_as(lse)), what
    a3 = alive[:, None, :].expand_as(lse)
    err = (lse[a3].double() - lse_x[a3]).abs().max().item()
    assert err <= 1e-5, f"{what}: lse off log(n_visible) by {err:.3e}"
    _dead_rows_exact(o, lse, q_len, k_len, Lq, what)
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    # p = 1 / n rounded to 16 bits inside the kernel (relative eps each), the output rounded once more
    lim = 3 * eps * v.float().abs().max().item()
    assert (o.double() - o_x).abs().max().item() <= lim, what


@pytest.mark.parametrize("ci", range(len(V.CASES)), ids=IDS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "fp16"])
def test_varlen_rows_past_the_lengths_are_never_used_and_samples_are_independent(dev, dtype, hd, ci):
    q, k, v, q_len, k_len, Lq, Lk = _case(ci, dtype, hd)
    o, lse = _launch(dev, hd, q, k, v, q_len, k_len, Lq, Lk, 0.25)
    o_p, lse_p = _launch(dev, hd, q, k, v, q_len, k_len, Lq, Lk, NAN)
    assert torch.equal(o.view(torch.int16), o_p.view(torch.int16)), "NaN behind the lengths changed o"
    assert torch.equal(lse.view(torch.int32), lse_p.view(torch.int32)), "NaN behind the lengths changed lse"
    for b in range(q.shape[0]):
        o1, lse1 = _launch(dev, hd, q, k, v, q_len, k_len, Lq, Lk, NAN, samples=[b])
        assert torch.equal(o1[0].view(torch.int16), o_p[b].view(torch.int16)), f"sample {b} alone: o differs"
        assert torch.equal(lse1[0].view(torch.int32), lse_p[b].view(torch.int32)), f"sample {b} alone: lse differs"


def test_varlen_lengths_are_clamped_to_the_launch_bounds(dev):
    """q_len > Lq, k_len > Lk and negative lengths are clamped on the device (Lq, Lk, 0): no row past the bounds is
    addressed"""
    dtype, hd = torch.bfloat16, 64
    q, k, v, _, _, Lq, Lk = _case(1, dtype, hd)
    q_len, k_len = [Lq + 5, -3, 7, Lq], [Lk + 9, 20, -1, Lk]
    ref = V.varlen_ref(q, k, v, H, hd ** -0.5, q_len, k_len)
    o, lse = _launch(dev, hd, q, k, v, q_len, k_len, Lq, Lk, NAN)
    _close(o, ref["o"], "clamped o")
    assert torch.equal(torch.isneginf(lse), torch.isneginf(ref["lse"]))


def test_varlen_domain_is_checked_in_the_entry_point(dev):
    """hd = 48, fp32, a misaligned pointer, a pitch that breaks the 16-byte accesses, int64 lengths, null pointers and
    zero sizes: an error each and nothing is launched (o and lse keep their contents)"""
    dtype, hd, B, Lq, Lk = torch.bfloat16, 64, 2, 8, 24
    D = H * hd
    lib = ops._L.load()
    buf = torch.randn(B * Lk * (3 * D + 8) + 8, device=dev).to(dtype)
    good = buf[:B * Lk * 3 * D]
    o = torch.full((B, Lq, D), 7.0, dtype=dtype, device=dev)
    lse = torch.full((B, H, Lq), 7.0, dtype=torch.float32, device=dev)
    ql = torch.tensor([3, 8], dtype=torch.int32, device=dev)
    kl = torch.tensor([24, 9], dtype=torch.int32, device=dev)

    def call(x=good, ld=3 * D, hd=hd, ql=ql, kl=kl, o=o):
        ops.flash_attn_varlen_fwd(x, x, x, o, ql, kl, B, H, Lq, Lk, hd, ld, Lq * ld, ld, Lk * ld, ld, Lk * ld,
                                  H * hd, Lq * H * hd, 0.125, lse=lse, k_off=H * hd, v_off=2 * H * hd)

    def untouched():
        torch.cuda.synchronize()
        assert bool((o == 7.0).all()) and bool((lse == 7.0).all())

    for kw in (dict(x=buf[1:1 + B * Lk * 3 * D]), dict(ld=3 * D + 4), dict(hd=48), dict(x=good.float()),
               dict(o=o.view(-1)[1:])):
        with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
            call(**kw)
        untouched()
    for kw in (dict(ql=ql.long()), dict(kl=kl.float())):
        with pytest.raises(MacawHipError, match="int32"):
            call(**kw)
        untouched()
    assert not ops.flash_varlen_ok(torch.float32, 64) and not ops.flash_varlen_ok(dtype, 32)
    assert ops.flash_varlen_ok(dtype, 64) and ops.flash_varlen_ok(torch.float16, 128)

    def raw(**kw):
        a = dict(q=good.data_ptr(), k=good.data_ptr() + 2 * D, v=good.data_ptr() + 4 * D, o=o.data_ptr(),
                 q_len=ql.data_ptr(), k_len=kl.data_ptr(), B=B, H=H, Lq=Lq, Lk=Lk)
        a.update(kw)
        ld = 3 * D
        return lib.mk_flash_attn_varlen_fwd(a["q"], a["k"], a["v"], a["o"], lse.data_ptr(), a["q_len"], a["k_len"],
                                            a["B"], a["H"], a["Lq"], a["Lk"], hd, ld, Lq * ld, ld, Lk * ld, ld, Lk * ld,
                                            D, Lq * D, 0.125, ops.dt(good), None)

    for name in ("q", "k", "v", "o", "q_len", "k_len"):
        assert raw(**{name: None}) == -1, f"null {name}: MK_ERR_BAD_ARG"
    for name in ("B", "H", "Lq", "Lk"):
        assert raw(**{name: 0}) == -1 and raw(**{name: -2}) == -1, f"{name} <= 0: MK_ERR_BAD_ARG"
    untouched()
    call()                                                      # the aligned call is inside the domain
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.float()).all()) and not bool((o == 7.0).all())
