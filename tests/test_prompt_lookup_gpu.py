"""GPU: prompt-lookup speculative decoding -- ops.decode_step_attn_multi bit for bit against ops.decode_step_attn run once
per row, ops.spec_lookup / ops.spec_verify_emit (csrc/spec.hip) against the numpy restatement of tests/spec_ref.py field by
field, and generate(prompt_lookup_num_tokens=G) end to end: the step count against spec_ref.simulate on the path's own
output, every emitted id against the fp32 oracle (the rule of tests/test_decode_ragged_gpu.py), the graph path against the
kernel-by-kernel loop, eos, the max_new_tokens cut, fp8 weight streaming, the default path, the refusals and MM_LLMs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spec_ref as R  # noqa: E402
from test_decode_kv8_gpu import _tables  # noqa: E402
from test_decode_ragged_cpu import restated_masked_greedy  # noqa: E402
from test_logits_processors_gpu import _Spy, _small_llama  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

H16 = [torch.bfloat16, torch.float16]
NEW_OPS = ("spec_lookup", "spec_verify_emit", "decode_step_attn_multi")
NAN = float("nan")


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.MM_LLMs.set_prompt_lookup()
    ops.clear_fp8_cache()


def _bits(t):
    return t.contiguous().view(torch.int16)


# --------------------------------------------------------------------------- 1. the attention, bit for bit --
def _attn_case(hd, H, Q, pos, Tmax, dtype, dev, seed):
    """one multi-query launch against the plain kernel run Q times per sample on a single-sample clone of the cache.
    Cache rows below pos[b] are random, every row from pos[b] on holds NaN: a key read past a row's own position
    poisons its output, and an untouched row keeps its NaN bits."""
    B, D = len(pos), H * hd
    g = torch.Generator(device=dev).manual_seed(seed)
    cache0 = torch.randn((B, Tmax, 2 * D), generator=g, device=dev).to(dtype)
    for b, p in enumerate(pos):
        cache0[b, max(p, 0):] = NAN
    qkv = torch.randn((B * Q, 3 * D), generator=g, device=dev).to(dtype)
    cos, sin = _tables(hd, Tmax, dtype, dev)
    scale = 1.0 / hd ** 0.5
    cache = cache0.clone()
    out = torch.full((B * Q, D), NAN, dtype=dtype, device=dev)
    ops.decode_step_attn_multi(qkv, qkv, qkv, 3 * D, cos, sin, cache, torch.tensor(pos, dtype=torch.int32, device=dev), Tmax,
                               B, Q, H, hd, out, scale, k_off=D, v_off=2 * D)
    for b, p in enumerate(pos):
        rc = cache0[b:b + 1].clone()
        inside = [g_ for g_ in range(Q) if p + g_ < Tmax]
        for g_ in inside:
            row = qkv[b * Q + g_:b * Q + g_ + 1]
            ro = torch.full((1, D), NAN, dtype=dtype, device=dev)
            ops.decode_step_attn(row, row, row, 3 * D, cos, sin, rc, torch.tensor([p + g_], dtype=torch.int32, device=dev),
                                 Tmax, 1, H, hd, ro, scale, k_off=D, v_off=2 * D)
            assert torch.equal(_bits(out[b * Q + g_]), _bits(ro[0])), (b, g_, p)
            assert bool(torch.isfinite(ro.float()).all()), (b, g_, p)
        for g_ in range(Q):                                     # a row past t_max: zeros, nothing written
            if g_ not in inside:
                assert bool((_bits(out[b * Q + g_]) == 0).all()), (b, g_, p)
        # the rows written are exactly pos[b] ... pos[b] + Q - 1 (inside the cache), with the plain kernel's bits ...
        assert torch.equal(_bits(cache[b]), _bits(rc[0])), (b, p)
        rest = [t for t in range(Tmax) if not p <= t < p + Q]
        # ... and every other byte is untouched
        assert torch.equal(_bits(cache[b, rest]), _bits(cache0[b, rest])), (b, p)
        assert bool(torch.isfinite(cache[b, p:min(p + Q, Tmax)].float()).all()), (b, p)


@pytest.mark.parametrize("dtype", H16, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Q", [1, 3, 8])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_multi_query_step_attention_is_the_plain_kernel_row_by_row(dev, hd, Q, dtype):
    """pos = 0 (no cached key) next to another position, and pos + Q - 1 == t_max - 1 next to a short sample"""
    Tmax = 24
    _attn_case(hd, 2, Q, [0, 5], Tmax, dtype, dev, seed=hd + Q)
    _attn_case(hd, 2, Q, [Tmax - Q, 3], Tmax, dtype, dev, seed=hd + Q + 1)


@pytest.mark.parametrize("dtype", H16, ids=["bf16", "fp16"])
@pytest.mark.parametrize("hd,pos,Tmax", [(16, 62, 70), (64, 62, 70), (128, 62, 70), (128, 254, 260), (16, 254, 260),
                                          (64, 510, 520), (32, 1022, 1030), (16, 2046, 2056)])
def test_multi_query_step_attention_across_a_pass_boundary(dev, hd, pos, Tmax, dtype):
    """Q = 4 rows from position 62: they cross the 64-key pass of hd = 64 (8 waves x 8 keys) and two 32-key passes of
    hd = 128; from 254: the 256-key trip of hd = 128 (32 keys x 8 in flight) and the 256-key pass of hd = 16; from 510,
    1022 and 2046: the trips of hd = 64, 32 and 16"""
    _attn_case(hd, 2, 4, [pos, pos - 1], Tmax, dtype, dev, seed=pos + hd)


@pytest.mark.parametrize("dtype", H16, ids=["bf16", "fp16"])
def test_multi_query_rows_past_t_max_write_nothing_and_bad_arguments_return_codes(dev, dtype):
    H, hd, Tmax = 2, 64, 24
    D = H * hd
    _attn_case(hd, H, 4, [Tmax - 2, 1], Tmax, dtype, dev, seed=3)       # rows 2, 3 of sample 0 lie past the cache
    _attn_case(hd, H, 3, [Tmax, Tmax - 1], Tmax, dtype, dev, seed=4)    # a whole sample past it
    B, Q = 2, 3
    qkv = torch.zeros((B * 17, 3 * D), dtype=dtype, device=dev)
    cos, sin = _tables(hd, Tmax, dtype, dev)
    cache = torch.zeros((B, Tmax, 2 * D), dtype=dtype, device=dev)
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    out = torch.zeros((B * 17, D), dtype=dtype, device=dev)

    def call(q=None, Q=Q, H=H, hd=hd, cache=cache, k_off=D, B=B, pos=pos):
        q = qkv[:B * Q] if q is None else q
        ops.decode_step_attn_multi(q, q, q, 3 * D, cos, sin, cache, pos, Tmax, B, Q, H, hd, out[:B * Q], 0.125, k_off=k_off,
                                   v_off=2 * D)

    call()                                                              # the good call
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
        call(Q=17)
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
        call(H=4, hd=32, k_off=D + 4)                                   # k_new 8 bytes off a 16-byte boundary
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
        ops.decode_step_attn_multi(qkv[:6].float(), qkv[:6].float(), qkv[:6].float(), 3 * D, cos, sin, cache.float(), pos,
                                   Tmax, B, Q, H, hd, out[:6].float(), 0.125)
    lib = ops._L.load()
    p = lambda t: t.data_ptr()  # noqa: E731
    base = [p(qkv), p(qkv) + 2 * D, p(qkv) + 4 * D, 3 * D, p(cos), p(sin), p(cache), p(cache) + 2 * D, 2 * D, Tmax * 2 * D, p(out),
            D, p(pos), Tmax, B, Q, H, hd, 0.125, ops.dt(qkv), None]
    assert lib.mk_decode_step_attn_multi(*base) == 0
    for i, bad in ((12, None), (0, None), (10, None), (14, 0), (15, 0), (13, 0), (16, 0)):     # pos, q, o, B, Q, t_max, H
        args = list(base)
        args[i] = bad
        with pytest.raises(MacawHipError, match="MK_ERR_BAD_ARG"):
            ops._L.check(lib.mk_decode_step_attn_multi(*args), f"argument {i}")
    args = list(base)
    args[17] = 48
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
        ops._L.check(lib.mk_decode_step_attn_multi(*args), "hd = 48")
    torch.cuda.synchronize()


# ------------------------------------------------------------- 2. lookup and verify against the restatement --
V, PAD, EOS = 40, 39, 2


def _state_from(books, G, n_max, dev):
    ss = ops.SpecState(len(books), G, n_max, PAD, dev)
    ss.pos.copy_(torch.tensor([b.pos for b in books], dtype=torch.int32))
    ss.n_out.copy_(torch.tensor([b.n_out for b in books], dtype=torch.int32))
    ss.done.copy_(torch.tensor([b.done for b in books]))
    ss.steps.copy_(torch.tensor([b.steps for b in books], dtype=torch.int32))
    ss.n_draft.copy_(torch.tensor([b.n_draft for b in books], dtype=torch.int32))
    ss.out.copy_(torch.tensor([b.out for b in books]))
    ss.tok.copy_(torch.tensor([b.tok for b in books]))
    return ss


def _assert_state(ss, books, what):
    got = dict(pos=ss.pos.tolist(), n_out=ss.n_out.tolist(), done=ss.done.tolist(), steps=ss.steps.tolist(),
               out=ss.out.tolist(), tok=ss.tok.tolist(), n_draft=ss.n_draft.tolist())
    for k, v in got.items():
        assert v == [b.fields()[k] for b in books], (what, k, v, [b.fields()[k] for b in books])


def _prepared(G, n_max, seed):
    """three samples: a running one whose history repeats (ids over a small alphabet, an eos and an id outside the
    vocabulary among them), one close to max_new_tokens, one finished; tok columns hold junk that the lookup must replace"""
    g = np.random.default_rng(seed)
    P = 12
    prompt = g.integers(3, 8, size=(3, P))
    prompt[0, 4], prompt[0, 9] = EOS, 50 + seed                          # an eos and an id outside [0, V) in a history
    prompt[1, 3] = -1
    p_len = [P, P - 3, P]
    books = []
    for b, (n_out, done) in enumerate(((5, False), (n_max - 2, False), (4, True))):
        bk = R.Books(G, n_max, PAD, pos=20 + b)
        bk.n_out, bk.done, bk.steps = n_out, done, n_out - b
        bk.out[:n_out] = g.integers(3, 8, size=n_out).tolist()
        bk.tok = [int(bk.out[n_out - 1])] + [7] * G
        bk.n_draft = G
        books.append(bk)
    return prompt, p_len, books


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("G", [1, 4, 15])
def test_lookup_and_verify_are_the_restatement_field_by_field(dev, G, dtype):
    Q, n_max, ld = G + 1, 24, 48
    hits = cuts = 0
    for seed in range(6):
        prompt, p_len, books = _prepared(G, n_max, seed)
        n = 1 + seed % 3
        with_prompt = seed != 5                                          # once without a prompt history
        ss = _state_from(books, G, n_max, dev)
        if with_prompt:
            ops.spec_lookup(ss, V, n, EOS, torch.tensor(prompt, device=dev), torch.tensor(p_len, dtype=torch.int32, device=dev))
        else:
            ops.spec_lookup(ss, V, n, EOS)
        for b, bk in enumerate(books):
            R.draft_into(bk, prompt[b, :p_len[b]].tolist() if with_prompt else [], n, EOS, V)
        _assert_state(ss, books, ("lookup", seed))
        hits += sum(bk.n_draft > 0 for bk in books)
        # logits: row g of sample b favours the draft token for the first `acc` rows, then something else; a tie (the first
        # column wins), a row holding NaN (the first NaN wins) and a row of -inf (column 0) among them
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(3 * Q, ld, generator=gen)
        x[:, V:] = 1e4                                                   # the padding columns are never looked at
        for b, bk in enumerate(books):
            acc = (seed + b) % (bk.n_draft + 2)
            for g_ in range(min(acc, bk.n_draft)):
                x[b * Q + g_, bk.tok[1 + g_]] = 50.0
            if seed == 1:                                                # an eos inside the accepted run
                x[b * Q + min(1, G), :V] = -1.0
                x[b * Q + min(1, G), EOS] = 60.0
        x[Q - 1, 11], x[Q - 1, 30] = 70.0, 70.0                          # sample 0's last row: a tie above everything
        x[Q + 1, :V] = -float("inf")                                     # sample 1, row 1: a row of -inf
        x = x.to(dtype)
        a = [[R.argmax(x[b * Q + g_, :V].double().numpy()) for g_ in range(Q)] for b in range(3)]
        assert a[0][Q - 1] == 11 and a[1][1] == 0                        # the first of the tie; column 0
        ops.spec_verify_emit(x.to(dev)[:, :V], V, EOS, ss)
        for b, bk in enumerate(books):
            R.verify(bk, a[b], EOS)
        cuts += books[1].n_out == n_max
        _assert_state(ss, books, ("verify", seed))
        # token 0's form: one row per sample, the draft is not read; a row holding NaN and -inf (the first NaN wins)
        x1 = torch.randn(3, ld, generator=gen)
        x1[:, V:] = 1e4
        x1[0, 17], x1[0, 23], x1[0, 5] = NAN, NAN, -float("inf")
        x1 = x1.to(dtype)
        a1 = [R.argmax(x1[b, :V].double().numpy()) for b in range(3)]
        assert a1[0] == 17
        ops.spec_verify_emit(x1.to(dev)[:, :V], V, EOS, ss)
        for b, bk in enumerate(books):
            R.verify(bk, [a1[b]], EOS)
        _assert_state(ss, books, ("token 0", seed))
    assert hits >= 6 and cuts >= 1                                       # drafts were found, the max_new_tokens cut was hit


# ------------------------------------------------------------------------------------------ 3. end to end --
N_NEW, G_E2E, NGRAM = 12, 4, 2
_MEMO = {}


def _fixture(dev):
    """the small LLaMA in bf16, a prompt of distinct ids per sample and plain greedy's ids for it: computed once"""
    if "fx" not in _MEMO:
        lm, cfg_l = _small_llama(dev)
        Vm, B, S0 = cfg_l["vocab_size"], 2, 21
        g = torch.Generator().manual_seed(7)
        prompt = torch.stack([torch.randperm(Vm - 3, generator=g)[:S0] + 3 for _ in range(B)]).to(dev)
        kw = dict(max_new_tokens=N_NEW, eos_token_id=-1, pad_token_id=0)
        with _Spy(*NEW_OPS) as spy:
            y = lm.generate(input_ids=prompt, **kw)
            y0 = lm.generate(input_ids=prompt, prompt_lookup_num_tokens=0, **kw)
            assert all(spy.calls[n] == [] for n in NEW_OPS)             # None and 0: none of the three ops is called
        assert torch.equal(y, y0) and y.shape == (B, N_NEW)
        emb = ops.embedding_fwd(lm.model.embed_tokens.weight, prompt.reshape(-1)).view(B, S0, -1)
        _MEMO["fx"] = (lm, cfg_l, prompt, emb, y, kw)
    return _MEMO["fx"]


def _sim(hist, row, eos, max_new, G=G_E2E):
    row = [int(t) for t in row]
    if eos in row:
        row = row[:row.index(eos) + 1]
    return R.simulate([int(t) for t in hist], row[:max_new], G, NGRAM, eos, max_new)


def _assert_oracle(lm, cfg_l, emb, got, tag):
    """every emitted id is the argmax of the fp32 restatement teacher-forced on the path's own ids, or loses to it by at
    most 3.0 x the bf16 noise there (tests/test_decode_ragged_gpu.py)"""
    sd32 = {"llm." + k: v.detach().float() for k, v in lm.state_dict().items()}
    sd16 = {k: v.to(torch.bfloat16) for k, v in sd32.items()}
    mask = torch.ones(emb.shape[:2], dtype=torch.long, device=emb.device)
    with torch.no_grad():
        _, z32 = restated_masked_greedy(sd32, emb.float(), mask, cfg_l, got.shape[1], force_ids=got)
        _, z16 = restated_masked_greedy(sd16, emb.to(torch.bfloat16), mask, cfg_l, got.shape[1], force_ids=got)
    z32, z16 = z32.float(), z16.float()
    margin = z32.max(-1).values - z32.gather(-1, got[..., None]).squeeze(-1)
    noise = (z16 - z32).abs().max(-1).values
    print(f"{tag}: ids off the oracle's argmax {(margin > 0).sum().item()}, worst margin / noise "
          f"{(margin / noise.clamp_min(1e-12)).max().item():.3f}")
    assert (margin <= 3.0 * noise).all(), (tag, margin.tolist(), noise.tolist())


def _accepting(dev, lm, prompt, emb, y, kw, **more):
    hist = torch.cat([prompt, y, prompt[:, -2:]], dim=1)                # the last two prompt ids again: the draft is y
    look = dict(inputs_embeds=emb, input_ids=hist, prompt_lookup_num_tokens=G_E2E, max_matching_ngram_size=NGRAM,
                return_lookup_stats=True, **more)
    return hist, look, lm.generate(**look, **kw)


def test_generate_accepts_drafts_from_a_history_that_holds_the_answer(dev):
    lm, cfg_l, prompt, emb, y, kw = _fixture(dev)
    nl = cfg_l["num_hidden_layers"]
    with _Spy(*NEW_OPS) as spy:
        hist, look, (got, steps) = _accepting(dev, lm, prompt, emb, y, kw)
        # token 0 + one eager step + one captured step: every other step is a replay
        assert len(spy.calls["spec_verify_emit"]) == 3 and len(spy.calls["spec_lookup"]) == 2
        assert len(spy.calls["decode_step_attn_multi"]) == 2 * nl
    assert got.dtype == torch.long and got.shape == (2, N_NEW) and steps.dtype == torch.int32
    print("greedy", y.tolist(), "lookup", got.tolist(), "steps", steps.tolist())
    for b in range(2):
        counts, want = _sim(hist[b], got[b], -1, N_NEW)
        assert int(steps[b]) == want and sum(counts) == N_NEW, (b, steps.tolist(), counts)
        assert int(steps[b]) < N_NEW                                    # steps < n_out: drafts were accepted
    _assert_oracle(lm, cfg_l, emb, got, "accepting")
    e, esteps = lm.generate(decode_graph=False, **look, **kw)           # the same launches, kernel by kernel
    assert torch.equal(e, got) and torch.equal(esteps, steps)
    assert torch.equal(lm.generate(**{**look, "return_lookup_stats": False}, **kw), got)


def test_generate_cold_history_runs_one_token_per_step_until_its_own_output_repeats(dev):
    lm, cfg_l, prompt, emb, y, kw = _fixture(dev)
    look = dict(inputs_embeds=emb, prompt_lookup_num_tokens=G_E2E, return_lookup_stats=True)     # history: generated ids only
    got, steps = lm.generate(**look, **kw)
    assert got.shape == (2, N_NEW)
    for b in range(2):
        counts, want = _sim([], got[b], -1, N_NEW)
        assert int(steps[b]) == want, (b, steps.tolist(), counts)
        if len(set(got[b].tolist())) == N_NEW:                          # the output never repeats: nothing to look up
            assert want == N_NEW
    _assert_oracle(lm, cfg_l, emb, got, "cold")
    e, esteps = lm.generate(decode_graph=False, **look, **kw)
    assert torch.equal(e, got) and torch.equal(esteps, steps)


def test_generate_eos_ends_one_sample_inside_a_run_and_the_other_runs_on(dev):
    lm, cfg_l, prompt, emb, y, kw = _fixture(dev)
    hist, look, (got, steps) = _accepting(dev, lm, prompt, emb, y, kw)
    pick = None                                                         # (sample, index): a token emitted behind an accepted draft
    for b in range(2):
        counts, _ = _sim(hist[b], got[b], -1, N_NEW)
        at = 0
        for c in counts:
            for i in range(at + 1, at + c - 1):                         # inside the run: neither its first nor its last token
                t = int(got[b, i])
                if pick is None and t not in got[1 - b].tolist() and got[b].tolist().index(t) == i:
                    pick = (b, i)
            at += c
    assert pick is not None, (got.tolist(), "no token inside an accepted run is unique to its sample")
    b0, i0 = pick
    eos = int(got[b0, i0])
    order = [b0, 1 - b0]                                                # the sample that ends comes first
    hist2, emb2 = hist[order].contiguous(), emb[order].contiguous()
    kw2 = dict(kw, eos_token_id=eos)
    look2 = dict(look, inputs_embeds=emb2, input_ids=hist2)
    out, st = lm.generate(**look2, **kw2)
    assert out.shape == (2, N_NEW)
    assert out[0, :i0 + 1].tolist() == got[b0, :i0 + 1].tolist() and bool((out[0, i0 + 1:] == 0).all())    # pad behind the eos
    assert eos not in out[1].tolist() and out[1].tolist() == got[1 - b0].tolist()                         # the other runs on
    for b in range(2):
        counts, want = _sim(hist2[b], out[b], eos, N_NEW)
        assert int(st[b]) == want, (b, st.tolist(), counts)
    e, est = lm.generate(decode_graph=False, **look2, **kw2)
    assert torch.equal(e, out) and torch.equal(est, st)
    twice, _ = lm.generate(**dict(look2, inputs_embeds=emb2[[0, 0]].contiguous(), input_ids=hist2[[0, 0]].contiguous()), **kw2)
    assert twice.shape == (2, i0 + 1)                                   # trimmed at the column where every sample has finished
    assert twice.tolist() == [out[0, :i0 + 1].tolist()] * 2


def test_generate_cuts_the_last_step_at_max_new_tokens(dev):
    lm, cfg_l, prompt, emb, y, kw = _fixture(dev)
    hist, look, (got, steps) = _accepting(dev, lm, prompt, emb, y, kw)
    counts, _ = _sim(hist[0], got[0], -1, N_NEW)
    k = next(i for i, c in enumerate(counts) if c >= 3)                 # a step that emits at least three tokens ...
    n_cut = sum(counts[:k]) + 2                                         # ... is cut after its second
    out, st = lm.generate(**look, **dict(kw, max_new_tokens=n_cut))
    assert out.shape == (2, n_cut)
    for b in range(2):
        c, want = _sim(hist[b], out[b], -1, n_cut)
        assert int(st[b]) == want and sum(c) == n_cut, (b, st.tolist(), c)
    c0, _ = _sim(hist[0], out[0], -1, n_cut)
    assert c0[-1] == 2 and c0[:-1] == counts[:k]
    assert torch.equal(out, got[:, :n_cut])


def test_generate_lookup_composes_with_fp8_weight_streaming(dev):
    """the weights snapped to e4m3-exact values (test_decode_fp8_gpu._snap_fp8_exact): the quantised copies hold the
    masters' numbers, so the fp32 oracle on the masters is the oracle of the path and the rule keeps its bound"""
    from test_decode_fp8_gpu import _snap_fp8_exact
    lm, cfg_l = _small_llama(dev, seed=1)
    with torch.no_grad():
        for lyr in lm.model.layers:
            a, m = lyr.self_attn, lyr.mlp
            for lin in (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj):
                lin.weight.copy_(_snap_fp8_exact(lin.weight)[0].to(lin.weight.dtype).to(dev))
        lm.lm_head.weight.copy_(_snap_fp8_exact(lm.lm_head.weight)[0].to(lm.lm_head.weight.dtype).to(dev))
    _, _, prompt, _, _, kw = _fixture(dev)
    emb = ops.embedding_fwd(lm.model.embed_tokens.weight, prompt.reshape(-1)).view(*prompt.shape, -1)
    y = lm.generate(input_ids=prompt, decode_weights="fp8", **kw)
    with _Spy("decode_linear_fp8", "decode_linear", *NEW_OPS) as spy:
        hist, look, (got, steps) = _accepting(dev, lm, prompt, emb, y, kw, decode_weights="fp8")
        assert len(spy.calls["decode_linear_fp8"]) > 0 and len(spy.calls["decode_step_attn_multi"]) > 0
        rows = [a[0].shape[0] for a in spy.calls["decode_linear_fp8"]]  # token 0's lm_head at B rows, then B * Q rows
        assert set(rows) == {2, 2 * (G_E2E + 1)} and rows.count(2) == 1
    print("greedy", y.tolist(), "lookup", got.tolist(), "steps", steps.tolist())
    for b in range(2):
        counts, want = _sim(hist[b], got[b], -1, N_NEW)
        assert int(steps[b]) == want and int(steps[b]) < N_NEW, (b, steps.tolist(), counts)
    _assert_oracle(lm, cfg_l, emb, got, "fp8 weights")


def test_generate_refusals_on_the_device_path(dev):
    lm, cfg_l, prompt, emb, y, kw = _fixture(dev)
    on = dict(input_ids=prompt, prompt_lookup_num_tokens=4)
    with _Spy(*NEW_OPS) as spy:
        for bad in (16, -1, 2.0, "4"):
            with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
                lm.generate(**{**on, "prompt_lookup_num_tokens": bad}, **kw)
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            lm.generate(max_matching_ngram_size=0, **on, **kw)
        mask = torch.ones_like(prompt)
        mask[0, :2] = 0
        for more, what in ((dict(num_beams=2), "num_beams=2"), (dict(do_sample=True), "do_sample=True"),
                           (dict(repetition_penalty=1.3), "logits processor"), (dict(no_repeat_ngram_size=2), "logits processor"),
                           (dict(min_new_tokens=2), "logits processor"), (dict(kv_cache="fp8"), "kv_cache='fp8'"),
                           (dict(use_cache=False), "use_cache=False"), (dict(attention_mask=mask), "padded attention_mask")):
            with pytest.raises(ValueError, match=rf"prompt_lookup_num_tokens=4.*{what}.*not built"):
                lm.generate(**on, **more, **kw)
        big = prompt[:1].expand(7, -1).contiguous()
        with pytest.raises(ValueError, match=r"7 x 5 = 35 rows.*not built"):
            lm.generate(**{**on, "input_ids": big}, **kw)
        with pytest.raises(ValueError, match="fp32 parameters.*not built"):
            lm.generate(inputs_embeds=emb.float(), prompt_lookup_num_tokens=4, **kw)
        with pytest.raises(ValueError, match="lookup history"):
            lm.generate(inputs_embeds=emb, input_ids=prompt[:1], prompt_lookup_num_tokens=4, **kw)
        assert all(spy.calls[n] == [] for n in NEW_OPS)
        # an all-ones mask is no padded mask, and six samples of five rows are inside the limit
        full = lm.generate(attention_mask=torch.ones_like(prompt), **on, **kw)
        assert full.shape == (2, N_NEW) and len(spy.calls["spec_verify_emit"]) == 3
        six = lm.generate(**{**on, "input_ids": prompt[:1].expand(6, -1).contiguous()}, **kw)
        assert six.shape == (6, N_NEW) and bool((six == six[:1]).all())         # samples do not depend on the batch
    lm32, _ = _small_llama(dev, torch.float32)
    with pytest.raises(ValueError, match="fp32 parameters.*not built"):
        lm32.generate(**on, **kw)


def test_mm_llms_switch_reaches_the_loop_with_the_text_ids_as_history(dev):
    from golden_util import load_case
    from oracle import configs
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    B = inp["input_ids"].shape[0]
    with torch.no_grad(), _Spy(*NEW_OPS) as spy:
        base = model(inputs=inp)
        assert all(spy.calls[n] == [] for n in NEW_OPS)                 # off: exactly today's call
        Mo.MM_LLMs.set_prompt_lookup(3, max_matching_ngram_size=2)
        ids = model(inputs=inp)
        assert len(spy.calls["spec_verify_emit"]) >= 1 and len(spy.calls["decode_step_attn_multi"]) > 0
        for a in spy.calls["spec_lookup"]:                              # (ss, V, ngram, eos, prompt, prompt_len)
            assert a[0].G == 3 and a[2] == 2 and a[3] == 2
            assert torch.equal(a[4], inp["input_ids"].long()) and a[5].tolist() == [inp["input_ids"].shape[1]] * B
        Mo.MM_LLMs.set_prompt_lookup()
        again = model(inputs=inp)
    assert torch.equal(again, base)
    assert ids.dtype == torch.long and ids.shape[0] == B and 1 <= ids.shape[1] <= 128
