"""GPU: the e4m3 KV cache of generate(kv_cache="fp8") -- mk_kv_quant_append and mk_decode_step_attn_kv8 against the
quantiser restatement of tests/fp8_ref.py (rows = heads) and the fp64 reference of tests/decode_attn_ref.py, the
entry points' domain, and generate() end to end: the path that really ran, batch independence, eos handling, a
teacher-forced accuracy comparison against the e4m3 FORMAT's own error, one layer at LLaMA-7B width, the refusals.
The other tolerances are those the 16-bit kernels are already held to (tests/test_kernels_gpu.py, test_decode_fp8_gpu.py,
test_fp8_gpu.py), taken over unchanged."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_attn_ref  # noqa: E402
import fp8_ref  # noqa: E402
from golden_util import load_case  # noqa: E402
from oracle import configs, restate  # noqa: E402
from test_kernels_gpu import DECODE_STEP_SHAPES, H16  # noqa: E402

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

FP8 = torch.float8_e4m3fn
SENT_BYTE, SENT_SCALE = 0x7F, float("nan")          # the e4m3 NaN code and a NaN scale: a read past p poisons the output


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    ops.clear_fp8_cache()


def _tables(hd, Tmax, dtype, dev):
    cos, sin = restate.rotary_tables(hd, Tmax)
    return cos.to(dtype).to(dev), sin.to(dtype).to(dev)


def _quant_heads(x, hd):
    """x [..., 2 * H * hd] (16-bit or fp32, CPU) -> (bytes uint8 [..., 2 * H * hd], scales f32 [..., 2 * H]): the
    project's row quantiser with rows = heads"""
    q, s = fp8_ref.quant_rows_bytes(x.reshape(-1, hd))
    return q.reshape(x.shape), s.reshape(*x.shape[:-1], x.shape[-1] // hd)


def _dequant(q, s, hd):
    """fp32 values of a cache: bytes [..., n * hd] x scales [..., n]"""
    return (q.view(FP8).float().reshape(*s.shape, hd) * s[..., None]).reshape(q.shape)


def _same_bytes(a, b):
    a, b = a.clone(), b.clone()
    a[(a & 0x7F) == 0], b[(b & 0x7F) == 0] = 0, 0               # (apart from the sign of a zero)
    return torch.equal(a, b)


def _random_kv(B, T, H, hd, dtype, g):
    """random [B, T, 2 * H * hd] rows in the 16-bit type; every (sample, position, key or value, head) block carries its
    own power of two 2^-6 ... 2^6, so that neighbouring scales differ by orders of magnitude and a wrong scale index
    cannot pass"""
    x = torch.randn((B, T, 2 * H, hd), generator=g)
    x = x * torch.pow(2.0, torch.randint(-6, 7, (B, T, 2 * H, 1), generator=g).float())
    return x.to(dtype).reshape(B, T, 2 * H * hd)


_CACHE_MEMO = {}


def _cache_case(hd, H, B, T, dtype):
    """(16-bit rows, bytes, scales) of T random cache rows, computed once per shape and never modified"""
    key = (hd, H, B, T, dtype)
    if key not in _CACHE_MEMO:
        g = torch.Generator().manual_seed(7 * hd + 3 * T + B)
        x = _random_kv(B, T, H, hd, dtype, g)
        _CACHE_MEMO[key] = (x, *_quant_heads(x, hd))
    return _CACHE_MEMO[key]


# ------------------------------------------------------------------------------------------------ kernels --
@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("Sn", [1, 21])
@pytest.mark.parametrize("hd,H,B,T", DECODE_STEP_SHAPES)
def test_kv_quant_append_writes_the_restated_bytes_and_scales_and_nothing_else(hd, H, B, T, Sn, dtype):
    """rows [0, Sn) of the cache equal fp8_ref.quant_rows_bytes with rows = heads (bytes exactly, apart from the sign of
    a zero; scales at the bound of the existing quantiser test); every other row of both tensors keeps its sentinel.
    k and v are slices of one fused [B * Sn, 3D] buffer, as the prefill passes them."""
    dev = torch.device("cuda:0")
    D, Tmax = H * hd, Sn + 3
    x, _, _ = _cache_case(hd, H, B, 21, dtype)
    kvn = x[:, :Sn]                                             # [B, Sn, 2D] = [k | v]
    qkv = torch.zeros((B, Sn, 3 * D), dtype=dtype)
    qkv[:, :, D:] = kvn
    qkv = qkv.reshape(B * Sn, 3 * D).to(dev)
    cache, scales = ops.kv8_cache(B, Tmax, H, hd, dev)
    cache.fill_(SENT_BYTE)
    scales.fill_(SENT_SCALE)
    ops.kv_quant_append(qkv[:, D:2 * D], qkv[:, 2 * D:], 3 * D, Sn * 3 * D, cache, scales, 0, Sn, Tmax, B, H, hd)
    want_q, want_s = _quant_heads(kvn, hd)
    got_q, got_s = cache.cpu(), scales.cpu()
    assert _same_bytes(got_q[:, :Sn], want_q), (got_q[:, :Sn] != want_q).float().mean().item()
    assert torch.allclose(got_s[:, :Sn], want_s, rtol=1e-6, atol=0)
    assert bool((got_q[:, Sn:] == SENT_BYTE).all()) and bool(torch.isnan(got_s[:, Sn:]).all())


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("hd,H,B,T", DECODE_STEP_SHAPES)
def test_decode_step_attn_kv8_appends_the_quantised_row_and_attends_over_the_stored_cache(hd, H, B, T, dtype):
    """cache row p = the quantiser restatement of ops.rope_'s key and of the value, all other rows untouched (rows past p
    hold NaN codes and NaN scales: reading one would poison the output); the output against the fp64 reference of
    tests/decode_attn_ref.py (the rope_-rotated query over the DE-QUANTISED rows 0 ... p of the cache as stored after the
    call) under its bound; then the same launch with *t_dev = 0: the position is read at execution time."""
    dev = torch.device("cuda:0")
    D, Tmax, p = H * hd, T + 5, T - 1
    _, q0, s0 = _cache_case(hd, H, B, T, dtype)
    cq = torch.full((B, Tmax, 2 * D), SENT_BYTE, dtype=torch.uint8)
    cs = torch.full((B, Tmax, 2 * H), SENT_SCALE)
    cq[:, :p], cs[:, :p] = q0[:, :p], s0[:, :p]
    g = torch.Generator().manual_seed(3 * hd + T)
    qkv = torch.randn((B, 3 * D), generator=g)
    qkv[:, D:] = _random_kv(B, 1, H, hd, dtype, g)[:, 0].float()
    qkv = qkv.to(dtype).to(dev)
    cos, sin = _tables(hd, Tmax, dtype, dev)
    scale = 1.0 / hd ** 0.5

    def run(pos):
        cache, scales = cq.to(dev), cs.to(dev)
        t_dev = torch.tensor([pos], dtype=torch.int32, device=dev)
        ref_qkv = qkv.clone()
        ops.rope_(ref_qkv[:, :2 * D], cos, sin, torch.full((B,), pos, dtype=torch.int32, device=dev), 2 * H, hd)
        out = torch.full((B, D), float("nan"), dtype=dtype, device=dev)
        ops.decode_step_attn_kv8(qkv, qkv, qkv, 3 * D, cos, sin, cache, scales, t_dev, Tmax, B, H, hd, out, scale,
                                 k_off=D, v_off=2 * D)
        want_q, want_s = cq.clone(), cs.clone()
        want_q[:, pos], want_s[:, pos] = _quant_heads(ref_qkv[:, D:].cpu(), hd)
        got_q, got_s = cache.cpu(), scales.cpu()
        assert _same_bytes(got_q[:, pos], want_q[:, pos]), (got_q[:, pos] != want_q[:, pos]).float().mean().item()
        assert torch.allclose(got_s[:, pos], want_s[:, pos], rtol=1e-6, atol=0)
        rest = [t for t in range(Tmax) if t != pos]
        assert torch.equal(got_q[:, rest], want_q[:, rest])
        assert torch.equal(got_s[:, rest].view(torch.int32), want_s[:, rest].view(torch.int32))
        return (out.float().cpu(), ref_qkv[:, :D].cpu(), (got_q[:, :pos + 1], got_s[:, :pos + 1]),
                _dequant(got_q[:, :pos + 1], got_s[:, :pos + 1], hd))

    out, q, (got_q, got_s), _ = run(p)
    ref, o_abs = decode_attn_ref.ref_kv8(q, got_q, got_s, H, hd, scale)
    decode_attn_ref.assert_within(out, ref, o_abs, dtype, f"decode_step_attn_kv8 hd={hd} H={H} B={B} T={T}")
    # *t_dev = 0: one key, probability 1 -> the output is the de-quantised value row 0 of the cache as STORED (its own
    # scales: the restated ones agree to rtol 1e-6 only), the fp32 product of code and scale rounded once to the output type
    out0, _, _, kv0 = run(0)
    want0 = kv0[:, 0, D:].to(dtype).float()
    assert torch.equal(out0, want0), (out0 - want0).abs().max().item()


def test_kv8_domain_is_checked_in_the_entry_points(dtype=torch.bfloat16):
    """a misaligned pointer, a pitch that breaks the 16-byte loads and hd = 48: MK_ERR_UNSUPPORTED through MacawHipError
    from both entry points, and nothing is launched (cache, scales and output keep their contents)"""
    dev = torch.device("cuda:0")
    B, H, hd, Tmax = 2, 4, 64, 8
    D = H * hd

    def fresh(H=H, hd=hd):
        cache, scales = ops.kv8_cache(B, Tmax, H, hd, dev)
        cache.fill_(3)
        scales.fill_(7.0)
        return cache, scales, torch.full((B, H * hd), 7.0, device=dev).to(dtype)

    def untouched(cache, scales, out):
        torch.cuda.synchronize()
        assert bool((cache == 3).all()) and bool((scales == 7.0).all()) and bool((out == 7.0).all())

    cos, sin = _tables(hd, Tmax, dtype, dev)
    t_dev = torch.tensor([2], dtype=torch.int32, device=dev)
    buf = torch.randn(B * (3 * D + 8) + 8, device=dev).to(dtype)
    good = buf[:B * 3 * D].view(B, 3 * D)
    off = buf[1:1 + B * 3 * D].view(B, 3 * D)                   # 2 bytes off a 16-byte boundary
    pitched = buf[:B * (3 * D + 4)].view(B, 3 * D + 4)          # sample stride % 8 != 0

    def step(x, in_bs, H=H, hd=hd, cs=(cos, sin)):
        c = fresh(H, hd)
        Dh = H * hd
        with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
            ops.decode_step_attn_kv8(x, x, x, in_bs, *cs, c[0], c[1], t_dev, Tmax, B, H, hd, c[2], 0.125,
                                     k_off=Dh, v_off=2 * Dh)
        untouched(*c)

    def append(x, ld, in_bs, H=H, hd=hd):
        c = fresh(H, hd)
        Dh = H * hd
        with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
            ops.kv_quant_append(x[:, Dh:2 * Dh], x[:, 2 * Dh:], ld, in_bs, c[0], c[1], 0, 1, Tmax, B, H, hd)
        untouched(*c)

    c = fresh()
    ops.decode_step_attn_kv8(good, good, good, 3 * D, cos, sin, c[0], c[1], t_dev, Tmax, B, H, hd, c[2], 0.125,
                             k_off=D, v_off=2 * D)            # the aligned calls are inside the domain
    ops.kv_quant_append(good[:, D:2 * D], good[:, 2 * D:], 3 * D, 3 * D, c[0], c[1], 0, 1, Tmax, B, H, hd)
    step(off, 3 * D)
    append(off, 3 * D, 3 * D)
    step(pitched, 3 * D + 4)
    append(pitched, 3 * D + 4, 3 * D + 4)
    step(good, 3 * 4 * 48, H=4, hd=48, cs=_tables(48, Tmax, dtype, dev))      # (B * 3 * 192 elements fit in `good`)
    append(good, 3 * 4 * 48, 3 * 4 * 48, H=4, hd=48)
    with pytest.raises(MacawHipError, match="MK_ERR_BAD_ARG"):                # rows past the end of the cache
        ops.kv_quant_append(good[:, D:2 * D], good[:, 2 * D:], 3 * D, 3 * D, c[0], c[1], Tmax, 1, Tmax, B, H, hd)


# --------------------------------------------------------------------------------------------- generate() --
def _small_llama(dev, dtype=torch.bfloat16, seed=0):
    """the micro decoder with FF = 384 (test_decode_fp8_gpu._small_llama: all four projections inside the fp8 domain)"""
    from transformers import LlamaConfig
    cfg_l = dict(configs.get(load_case("micro_all")["config_name"])["llama"])
    cfg_l["intermediate_size"] = 384
    torch.manual_seed(seed)
    Mo.AUTO_FUSE = True
    lm = Mo.LlamaForCausalLM(LlamaConfig(**cfg_l)).to(dev).to(dtype)
    return Mo.fuse_model(lm).eval(), cfg_l


class _Spy:
    """wraps ops.<name> for the duration of a with block and records every call's arguments"""

    def __init__(self, *names):
        self.names, self.calls, self.real = names, {n: [] for n in names}, {}

    def __enter__(self):
        for n in self.names:
            self.real[n] = getattr(ops, n)

            def wrapped(*a, _n=n, **kw):
                self.calls[_n].append(a)
                return self.real[_n](*a, **kw)
            setattr(ops, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n in self.names:
            setattr(ops, n, self.real[n])


def _ids(cfg_l, B, dev, S=21):
    return torch.randint(3, cfg_l["vocab_size"], (B, S), generator=torch.Generator().manual_seed(B)).to(dev)


@pytest.mark.parametrize("B", [2, 8])
def test_generate_kv8_really_runs_on_the_e4m3_cache(dev, B):
    """no 16-bit step-attention launch, n_layers quantising cache writes in the prefill, n_layers kv8 step launches per
    eager / captured step, every one of them on a uint8 cache with fp32 scales; deterministic; composes with
    decode_weights="fp8"."""
    lm, cfg_l = _small_llama(dev)
    nl = cfg_l["num_hidden_layers"]
    kw = dict(input_ids=_ids(cfg_l, B, dev), max_new_tokens=12, eos_token_id=-1, pad_token_id=0, kv_cache="fp8")
    with _Spy("decode_step_attn", "decode_step_attn_kv8", "kv_quant_append", "decode_linear_fp8") as spy:
        out = lm.generate(**kw)
        assert out.shape == (B, 12) and out.dtype == torch.long
        assert spy.calls["decode_step_attn"] == []
        assert len(spy.calls["kv_quant_append"]) == nl
        # token 1: one eager step; then ONE captured step
        assert len(spy.calls["decode_step_attn_kv8"]) == 2 * nl
        for a in spy.calls["kv_quant_append"]:
            assert a[4].dtype == torch.uint8 and a[5].dtype == torch.float32
        for a in spy.calls["decode_step_attn_kv8"]:
            assert a[6].dtype == torch.uint8 and a[7].dtype == torch.float32
        assert spy.calls["decode_linear_fp8"] == []
        assert torch.equal(out, lm.generate(**kw))
        both = lm.generate(decode_weights="fp8", **kw)
        assert both.shape == out.shape and len(spy.calls["decode_linear_fp8"]) > 0
        assert spy.calls["decode_step_attn"] == [] and len(spy.calls["decode_step_attn_kv8"]) == 6 * nl
    ref = lm.generate(**{**kw, "kv_cache": None})
    assert ref.shape == out.shape                                           # (a quantised cache: the ids may differ)


def test_generate_kv8_samples_do_not_depend_on_the_batch(dev):
    """the ids of a B = 3 call equal those of the three prompts run singly: same kernels, deterministic sums (catches the
    sample strides of the cache and of its scales)"""
    lm, cfg_l = _small_llama(dev)
    ids = _ids(cfg_l, 3, dev)
    kw = dict(max_new_tokens=12, eos_token_id=-1, pad_token_id=0, kv_cache="fp8")
    out = lm.generate(input_ids=ids, **kw)
    for b in range(3):
        one = lm.generate(input_ids=ids[b:b + 1].contiguous(), **kw)
        assert torch.equal(one[0], out[b]), (b, one[0].tolist(), out[b].tolist())


def test_generate_kv8_eos_and_pad_follow_the_16bit_conventions(dev):
    """an early eos (the most frequent greedy token): a finished sample emits pad from then on, the output stops at the
    column at which every sample has finished, exactly as the 16-bit call shapes its result"""
    lm, cfg_l = _small_llama(dev)
    kw = dict(input_ids=_ids(cfg_l, 4, dev), max_new_tokens=24, pad_token_id=0)
    free = lm.generate(eos_token_id=-1, kv_cache="fp8", **kw)
    eos = int(free[:, 2:].flatten().mode().values)
    f = lm.generate(eos_token_id=eos, kv_cache="fp8", **kw)
    b = lm.generate(eos_token_id=eos, **kw)
    assert f.dtype == b.dtype == torch.long and f.shape[0] == b.shape[0] == 4 and f.shape[1] <= 24
    hit = (f == eos).cumsum(1) > 0
    assert bool(hit[:, -1].all()) or f.shape[1] == 24           # stops at the column where the last sample finishes
    if 2 <= f.shape[1] < 24:
        assert not bool(hit[:, -2].all())
    after = torch.zeros_like(hit)
    after[:, 1:] = hit[:, :-1]
    assert bool((f[after] == 0).all())                          # pad after a sample's eos
    assert torch.equal(f[~after], free[:, :f.shape[1]][~after])  # and the unconstrained ids before it
    hb = (b == eos).cumsum(1) > 0                               # the 16-bit call: the same conventions
    assert bool(hb[:, -1].all()) or b.shape[1] == 24


# --------------------------------------------------------------------------------------- accuracy yardstick --
def _ref_layers(x, Ws, H, eps, cos, sin, S0, fq):
    """the decoder recurrence of engine.llama_layer_cached in fp32 torch (oracle.restate's rms_norm / apply_rope pieces)
    over ALL positions at once: prompt positions (< S0) attend over plain keys / values as the prefill does, later
    positions over keys / values passed through `fq` (identity, or the e4m3 fake quantisation per head)"""
    B, S, D = x.shape
    hd = D // H
    pos = torch.arange(S).unsqueeze(0).expand(B, S)
    causal = torch.full((S, S), float("-inf")).triu(1)
    for wq, wk, wv, wo, wg, wu, wd, ln1, ln2 in Ws:
        y = restate.rms_norm(x, ln1, eps)
        heads = lambda t: t.view(B, S, H, hd).transpose(1, 2)  # noqa: E731
        q, k = restate.apply_rope(heads(y @ wq.t()), heads(y @ wk.t()), cos, sin, pos)
        v = heads(y @ wv.t())

        def attend(k, v):
            return (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd) + causal, -1) @ v).transpose(1, 2).reshape(B, S, D)

        att = torch.where((torch.arange(S) >= S0).view(1, S, 1), attend(fq(k), fq(v)), attend(k, v))
        h = x + att @ wo.t()
        y2 = restate.rms_norm(h, ln2, eps)
        x = h + (torch.nn.functional.silu(y2 @ wg.t()) * (y2 @ wu.t())) @ wd.t()
    return x[:, S0:]


def test_kv8_teacher_forced_steps_against_the_format_yardstick(dev, dtype=torch.bfloat16):
    """Two decoder layers through a prefill of 21 positions and 12 decode steps with FIXED input rows (no sampling: every
    route sees the same tokens), once on the e4m3 cache and once on the 16-bit cache, against the same recurrence in
    fp32 torch -- plain, and with ONLY the per-head e4m3 fake quantisation of the keys and values the steps read.  That
    last run's error is what the FORMAT costs; the HIP kv8 path is held to
        e_kv8 <= 1.5 * hypot(e_fmt, e_16) + 1e-3      (relative L2 of the step outputs)
    the form and factor of test_fp8_gpu.test_model_with_fp8_against_the_oracle_and_the_format_yardstick."""
    B, S0, NS, D, H, FF, NL, eps = 2, 21, 12, 256, 4, 384, 2, 1e-6
    hd, S = D // H, S0 + NS
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype)  # noqa: E731
    Ws = []
    for _ in range(NL):
        # (keys / queries large enough for a peaked softmax: the cache's rounding must matter to the output)
        Ws.append((rnd(D, D, sc=0.15), rnd(D, D, sc=0.15), rnd(D, D, sc=0.06), rnd(D, D, sc=0.06), rnd(FF, D, sc=0.06),
                   rnd(FF, D, sc=0.06), rnd(D, FF, sc=0.06), (1 + 0.1 * torch.randn(D, generator=g)).to(dtype),
                   (1 + 0.1 * torch.randn(D, generator=g)).to(dtype)))
    x = rnd(B, S, D)
    cos32, sin32 = restate.rotary_tables(hd, S)
    cos16, sin16 = cos32.to(dtype), sin32.to(dtype)
    Wf = [tuple(w.float() for w in ws) for ws in Ws]
    ref = _ref_layers(x.float(), Wf, H, eps, cos16.float(), sin16.float(), S0, lambda t: t)
    fmt = _ref_layers(x.float(), Wf, H, eps, cos16.float(), sin16.float(), S0, fp8_ref.fq_rows)

    Wd = []
    for wq, wk, wv, wo, wg, wu, wd, ln1, ln2 in Ws:
        wqkv, wgu = torch.cat((wq, wk, wv)).to(dev), torch.cat((wg, wu)).to(dev)
        Wd.append((wqkv[:D], wqkv[D:2 * D], wqkv[2 * D:], wo.to(dev), wgu[:FF], wgu[FF:], wd.to(dev), ln1.to(dev),
                   ln2.to(dev), wqkv, wgu))
    xd, cosd, sind = x.to(dev), cos16.to(dev), sin16.to(dev)

    def hip(kv8):
        if kv8:
            caches = [ops.kv8_cache(B, S, H, hd, dev) for _ in range(NL)]
        else:
            caches = [(torch.empty((B, S, 2 * D), dtype=dtype, device=dev), None) for _ in range(NL)]
        t_dev = torch.zeros(1, dtype=torch.int32, device=dev)

        def run(h, Sn, t0, pos, td):
            for (kvc, kvs), w in zip(caches, Wd):
                h = eng.llama_layer_cached(h, B, Sn, t0, kvc, S, pos, cosd, sind, H, eps, *w, t_dev=td, kv8=kvs)
            return h

        with torch.no_grad():
            run(xd[:, :S0].reshape(B * S0, D).contiguous(), S0, 0,
                torch.arange(S0, dtype=torch.int32, device=dev).repeat(B), None)
            outs = []
            for i in range(NS):
                t_dev.fill_(S0 + i)
                outs.append(run(xd[:, S0 + i].contiguous(), 1, 0, t_dev, t_dev).float().cpu())
        return torch.stack(outs, dim=1)

    with _Spy("decode_step_attn", "decode_step_attn_kv8") as spy:
        o8 = hip(True)
        assert spy.calls["decode_step_attn"] == [] and len(spy.calls["decode_step_attn_kv8"]) == NL * NS
        o16 = hip(False)
        assert len(spy.calls["decode_step_attn"]) == NL * NS

    def nerr(a, r):
        return (a - r).norm().item() / r.norm().item()

    e_kv8, e_fmt, e_16 = nerr(o8, ref), nerr(fmt, ref), nerr(o16, ref)
    print(f"teacher-forced step outputs, rel L2 vs fp32: HIP kv8 {e_kv8:.3e}, e4m3 format yardstick {e_fmt:.3e}, "
          f"HIP 16-bit {e_16:.3e}")
    assert torch.isfinite(o8).all()
    assert e_kv8 <= 1.5 * math.hypot(e_fmt, e_16) + 1e-3, (e_kv8, e_fmt, e_16)


# ---------------------------------------------------------------------------------------------- real width --
@pytest.mark.parametrize("B", [1, 32])
def test_kv8_decode_step_real_dimension_layer_vs_16bit_step(dev, B):
    """One LLaMA-7B-dimension decode step of a layer at position 150 on the e4m3 cache against the 16-bit step whose
    cache holds the same de-quantised values rounded to bf16, under the output bound of
    test_decode_fp8_gpu.test_fp8_decode_step_real_dimension_layer_vs_16bit_step.  B = 32: B x H = 1024 (sample, head)
    pairs, the four-heads-per-workgroup kernel."""
    D, FF, H = 4096, 11008, 32
    T0, Tmax, hd = 150, 160, D // H
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(11 + B)
    w = lambda N, K: (torch.randn((N, K), generator=g, device=dev) * 0.02).to(dtype)  # noqa: E731
    wqkv, wo, wgu, wd = w(3 * D, D), w(D, D), w(2 * FF, D), w(D, FF)
    ln1 = (1 + 0.1 * torch.randn(D, generator=g, device=dev)).to(dtype)
    ln2 = (1 + 0.1 * torch.randn(D, generator=g, device=dev)).to(dtype)
    x2 = torch.randn((B, D), generator=g, device=dev).to(dtype)
    kv = torch.randn((B, T0, 2 * D), generator=g, device=dev).to(dtype).cpu()
    q0, s0 = _quant_heads(kv, hd)
    cache8, scales8 = ops.kv8_cache(B, Tmax, H, hd, dev)
    cache8.fill_(SENT_BYTE)
    scales8.fill_(SENT_SCALE)
    cache8[:, :T0], scales8[:, :T0] = q0.to(dev), s0.to(dev)
    cache16 = torch.zeros((B, Tmax, 2 * D), dtype=dtype, device=dev)
    cache16[:, :T0] = _dequant(q0, s0, hd).to(dtype).to(dev)
    cos, sin = _tables(hd, Tmax, dtype, dev)
    pos = torch.full((B,), T0, dtype=torch.int32, device=dev)
    t_dev = torch.tensor([T0], dtype=torch.int32, device=dev)
    args = (H, 1e-6, wqkv[:D], wqkv[D:2 * D], wqkv[2 * D:], wo, wgu[:FF], wgu[FF:], wd, ln1, ln2, wqkv, wgu)
    with torch.no_grad(), _Spy("decode_step_attn", "decode_step_attn_kv8") as spy:
        out8 = eng.llama_layer_cached(x2, B, 1, 0, cache8, Tmax, pos, cos, sin, *args, t_dev=t_dev, kv8=scales8)
        assert len(spy.calls["decode_step_attn_kv8"]) == 1 and spy.calls["decode_step_attn"] == []
        out16 = eng.llama_layer_cached(x2, B, 1, 0, cache16, Tmax, pos, cos, sin, *args, t_dev=t_dev)
    assert torch.equal(cache8[:, :T0].cpu(), q0) and bool((cache8[:, T0 + 1:] == SENT_BYTE).all())
    # the appended row: the quantiser restatement of the row the 16-bit step appended
    wq_, ws_ = _quant_heads(cache16[:, T0].cpu(), hd)
    assert _same_bytes(cache8[:, T0].cpu(), wq_) and torch.allclose(scales8[:, T0].cpu(), ws_, rtol=1e-6, atol=0)
    d = (out8.float() - out16.float()).abs().max().item()
    ref = out16.float().abs().max().item()
    print(f"kv8 step vs 16-bit step B={B}: output diff {d:.3e} of {ref:.3e}")
    assert torch.isfinite(out8).all()
    assert d <= 2.0 ** -6 * ref + 1e-3, (d, ref)


# ------------------------------------------------------------------------------------------------ refusals --
def test_generate_kv8_refusals_and_default(dev, monkeypatch):
    """kv_cache="fp8" raises a ValueError naming the condition that keeps the call off the hipGraph decode path; more
    than 32 sequences and unfused storage are NOT among them; None is the 16-bit path (no kv8 call);
    MM_LLMs.set_kv_cache routes inputs["inference"] = True; a prefill at t0 > 0 is refused by the engine"""
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    emb = fx["inputs_embeds"].to(dev).to(torch.bfloat16)
    kw = dict(inputs_embeds=emb, max_new_tokens=8, eos_token_id=-1, pad_token_id=106)
    with _Spy("decode_step_attn_kv8", "kv_quant_append") as spy:
        assert torch.equal(model.llm.generate(**kw), model.llm.generate(kv_cache=None, **kw))
        assert spy.calls["decode_step_attn_kv8"] == [] and spy.calls["kv_quant_append"] == []
        with pytest.raises(ValueError, match="kv_cache"):
            model.llm.generate(kv_cache="int4", **kw)
        with pytest.raises(ValueError, match="use_cache"):
            model.llm.generate(kv_cache="fp8", use_cache=False, **kw)
        with pytest.raises(ValueError, match="decode_graph"):
            model.llm.generate(kv_cache="fp8", decode_graph=False, **kw)
        with pytest.raises(ValueError, match="max_new_tokens"):
            model.llm.generate(kv_cache="fp8", **{**kw, "max_new_tokens": 2})
        with pytest.raises(ValueError, match="decode_attn_ok"):
            model.llm.generate(kv_cache="fp8", **{**kw, "max_new_tokens": 16000})
        monkeypatch.setenv("MACAW_NO_DECODE_GRAPH", "1")
        with pytest.raises(ValueError, match="MACAW_NO_DECODE_GRAPH"):
            model.llm.generate(kv_cache="fp8", **kw)
        monkeypatch.delenv("MACAW_NO_DECODE_GRAPH")
        m32 = build_model(cfg, fx["state"], torch.float32, dev).eval()
        with pytest.raises(ValueError, match="fp32"):
            m32.llm.generate(kv_cache="fp8", **{**kw, "inputs_embeds": fx["inputs_embeds"].to(dev)})
        assert spy.calls["decode_step_attn_kv8"] == [] and spy.calls["kv_quant_append"] == []
        # not refused: 33 sequences (the separate-kernel step), unfused q / k / v storage
        out33 = model.llm.generate(kv_cache="fp8", **{**kw, "inputs_embeds": emb[:1].expand(33, -1, -1).contiguous()})
        assert out33.shape == (33, 8) and bool((out33 == out33[:1]).all())
        mu = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=False).eval()      # (lazy fusion off)
        n0 = len(spy.calls["decode_step_attn_kv8"])
        assert mu.llm.generate(kv_cache="fp8", **kw).shape == (emb.shape[0], 8)
        assert len(spy.calls["decode_step_attn_kv8"]) > n0
    # the multimodal entry point: a process-wide switch next to set_decode_weights
    with pytest.raises(ValueError):
        Mo.MM_LLMs.set_kv_cache("int4")
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    Mo.AUTO_FUSE = True
    with torch.no_grad():
        base = model(inputs=inp)
        Mo.MM_LLMs.set_kv_cache("fp8")
        with _Spy("decode_step_attn_kv8") as spy:
            ids = model(inputs=inp)
        Mo.MM_LLMs.set_kv_cache(None)
    assert len(spy.calls["decode_step_attn_kv8"]) > 0 and ids.dtype == torch.long and ids.shape[0] == base.shape[0]
    # the engine refuses a quantised prefill that does not start at position 0
    cache, scales = ops.kv8_cache(1, 8, 2, 16, dev)
    z = torch.zeros((2, 32), dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="t0"):
        eng.llama_layer_cached(z, 1, 2, 3, cache, 8, None, None, None, 2, 1e-6, *([None] * 9), kv8=scales)
