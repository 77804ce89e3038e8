"""generate(num_samples=n): parallel sampling over a prompt cache stored once per prompt (engine.SharedPrompt,
ops.decode_step_attn_shared; the kernel itself is pinned in tests/test_shared_attn_gpu.py).  The layout and the seeds, n = 1
as today's call, the two decode paths against each other, that the prompt really is prefilled, stored and read once, the
returned log-probabilities against ONE full forward over [prompt | emitted ids] (which catches a wrong key), stops, bans,
weight formats, LoRA, refusals and the MM_LLMs switch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_decode_kv8_gpu import _Spy, _ids, _small_llama  # noqa: E402

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.MM_LLMs.set_sampling()
    Mo.MM_LLMs.set_parallel_samples()
    ops.clear_fp8_cache()


@pytest.fixture(scope="module")
def llama(dev):
    return _small_llama(dev)


def _kw(cfg_l, B, dev, **over):
    return {**dict(input_ids=_ids(cfg_l, B, dev), max_new_tokens=12, eos_token_id=-1, pad_token_id=0, do_sample=True, seed=11),
            **over}


class _LayerSpy:
    """records (rows of x2, B, Sn, kvc) of every engine.llama_layer_cached call inside the with block"""

    def __enter__(self):
        self.real, self.calls = eng.llama_layer_cached, []

        def wrapped(x2, B, Sn, t0, kvc, *a, **kw):
            self.calls.append((x2.shape[0], B, Sn, kvc))
            return self.real(x2, B, Sn, t0, kvc, *a, **kw)
        eng.llama_layer_cached = wrapped
        return self

    def __exit__(self, *exc):
        eng.llama_layer_cached = self.real


# ------------------------------------------------------------------------------------------- shape and layout --
def test_rows_are_prompt_major_pad_follows_each_rows_own_eos_and_the_seed_decides(dev, llama):
    lm, cfg_l = llama
    B, n, N = 2, 3, 12
    kw = _kw(cfg_l, B, dev)
    ids = lm.generate(num_samples=n, **kw)
    assert ids.shape == (B * n, N) and ids.dtype == torch.long
    assert torch.equal(ids, lm.generate(num_samples=n, **kw))
    assert not torch.equal(ids, lm.generate(num_samples=n, **{**kw, "seed": 12}))
    assert len({tuple(r) for r in ids.tolist()}) > B              # the rows of a prompt are samples, not copies
    eos = int(ids[:, 2:6].flatten().mode().values)                # an id the eos-free run emits early
    got = lm.generate(num_samples=n, **{**kw, "eos_token_id": eos})
    hit = (ids == eos).cumsum(1) > 0
    assert bool(hit.any())
    w = got.shape[1]
    for r in range(B * n):                                        # the same draws up to the row's own eos, then pad
        cut = int(hit[r].long().argmax()) + 1 if bool(hit[r].any()) else N
        assert torch.equal(got[r, :min(cut, w)], ids[r, :min(cut, w)]), r
        assert bool((got[r, cut:] == 0).all()), r


# ------------------------------------------------------------------------------------------------------- n = 1 --
def test_one_sample_is_todays_sampled_call_on_every_weight_format(dev, llama):
    lm, cfg_l = llama
    for extra in ({}, dict(decode_weights="fp8"), dict(decode_weights="mxfp4")):
        kw = _kw(cfg_l, 3, dev, **extra)
        with _Spy("decode_step_attn", "decode_step_attn_shared", "embedding_fwd") as spy:
            today = lm.generate(**kw)
            n_attn, n_emb = len(spy.calls["decode_step_attn"]), len(spy.calls["embedding_fwd"])
            got = lm.generate(num_samples=1, **kw)
            assert len(spy.calls["decode_step_attn"]) == 2 * n_attn and len(spy.calls["embedding_fwd"]) == 2 * n_emb
            assert spy.calls["decode_step_attn_shared"] == []
        assert torch.equal(got, today), extra
    assert torch.equal(lm.generate(num_samples=1, **_kw(cfg_l, 3, dev, do_sample=False)),     # greedy takes n = 1 too
                       lm.generate(**_kw(cfg_l, 3, dev, do_sample=False)))


# -------------------------------------------------------------------------------------------------- graph path --
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_graph_path_and_kernel_by_kernel_loop_return_identical_ids_and_logprobs(dev, dtype):
    lm, cfg_l = _small_llama(dev, dtype)
    nl = cfg_l["num_hidden_layers"]
    kw = _kw(cfg_l, 2, dev, num_samples=3, return_logprobs=True, top_logprobs=2)
    with _Spy("decode_step_attn_shared", "decode_step_attn", "decode_step_attn_var", "decode_emit_sample") as spy:
        a = lm.generate(**kw)
        # token 0, one eager step, ONE captured step
        assert len(spy.calls["decode_step_attn_shared"]) == 2 * nl and len(spy.calls["decode_emit_sample"]) == 3
        b = lm.generate(decode_graph=False, **kw)
        assert len(spy.calls["decode_step_attn_shared"]) == (2 + 11) * nl
        assert spy.calls["decode_step_attn"] == [] and spy.calls["decode_step_attn_var"] == []
    assert a.ids.shape == (6, 12) and a.logprobs.shape == (6, 12) and a.top_ids.shape == (6, 12, 2)
    assert torch.equal(a.ids, b.ids) and torch.equal(a.logprobs, b.logprobs)
    assert torch.equal(a.top_ids, b.top_ids) and torch.equal(a.top_logprobs, b.top_logprobs)
    short = lm.generate(**{**kw, "max_new_tokens": 2})               # max_new_tokens <= 2: the loop
    assert short.ids.shape == (6, 2) and torch.equal(short.ids, a.ids[:, :2])


def test_under_top_k_1_the_rows_of_a_prompt_are_identical(dev, llama):
    lm, cfg_l = llama
    B, n = 2, 5
    ids = lm.generate(num_samples=n, top_k=1, **_kw(cfg_l, B, dev)).view(B, n, -1)
    assert torch.equal(ids, ids[:, :1].expand_as(ids))
    assert not torch.equal(ids[0, 0], ids[1, 0])


# ------------------------------------------------------------------------------------------- sharing is real --
@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "left-padded"])
def test_the_prompt_is_prefilled_stored_and_read_once_per_prompt(dev, llama, padded):
    lm, cfg_l = llama
    B, n, N, S0 = 2, 4, 6, 21
    D, nl = cfg_l["hidden_size"], cfg_l["num_hidden_layers"]
    kw = _kw(cfg_l, B, dev, max_new_tokens=N, num_samples=n)
    if padded:
        mask = torch.ones((B, S0), dtype=torch.long, device=dev)
        mask[1, :4] = 0
        kw["attention_mask"] = mask
    with _LayerSpy() as layers, _Spy("decode_step_attn_shared", "decode_step_attn", "decode_step_attn_var") as spy:
        ids = lm.generate(**kw)
    assert ids.shape == (B * n, N)
    pre, steps = layers.calls[:nl], layers.calls[nl:]
    for rows, b, sn, kvc in pre:                                   # the prefill ran on B * S0 rows into prompt [B, S0, 2D]
        assert (rows, b, sn) == (B * S0, B, S0) and torch.is_tensor(kvc) and tuple(kvc.shape) == (B, S0, 2 * D)
    assert len(steps) == 2 * nl                                    # one eager step, one captured step
    for rows, b, sn, kvc in steps:
        assert (rows, b, sn) == (B * n, B, 1) and isinstance(kvc, eng.SharedPrompt)
        assert tuple(kvc.prompt.shape) == (B, S0, 2 * D) and tuple(kvc.tail.shape) == (B * n, N, 2 * D)
        assert (kvc.n, kvc.S0) == (n, S0)
    # layer by layer the steps read the buffer the prefill wrote; no [B * n, S0 + ...] cache exists
    assert [c[3].prompt.data_ptr() for c in steps[:nl]] == [c[3].data_ptr() for c in pre]
    assert spy.calls["decode_step_attn"] == [] and spy.calls["decode_step_attn_var"] == []
    assert len(spy.calls["decode_step_attn_shared"]) == 2 * nl
    for a in spy.calls["decode_step_attn_shared"]:
        assert (a[9] is not None) == padded                        # t_off: one offset per prompt
        if padded:
            assert a[9].tolist() == [0, -4]


# ------------------------------------------------------------------------------------------- teacher forcing --
def _teacher_forced(lm, prompt, ids, V):
    """float64 log-probabilities [R, L] of ids [R, L] after prompt [R, S], from ONE full forward"""
    full = torch.cat([prompt, ids], 1)
    with torch.no_grad():
        logits = lm(input_ids=full).logits[:, prompt.shape[1] - 1:-1, :V].double()
    return torch.log_softmax(logits, -1).gather(2, ids.unsqueeze(-1)).squeeze(-1)


@pytest.fixture(scope="module")
def greedy_gap(dev, llama):
    """The bound of the teacher-forcing test, derived as test_beam_gpu's
    test_cached_beam_scores_are_the_teacher_forced_log_probabilities_of_the_returned_ids derives its own: 4 x the largest
    per-token log-probability gap between the CACHED greedy path -- the five-launch step of the hipGraph loop, visible per
    token where those launches run kernel by kernel: the loop of a padded batch, one masked token in front of every
    prompt -- and one full forward over the greedy ids, at B * n = 8 prompts (the row count of the sampled steps)."""
    lm, cfg_l = llama
    V, N = cfg_l["vocab_size"], 12
    gprompt = _ids(cfg_l, 8, dev)
    padded = torch.cat([torch.zeros_like(gprompt[:, :1]), gprompt], 1)
    mask = torch.ones_like(padded)
    mask[:, 0] = 0
    seen, real = [], ops.argmax_rows

    def spy(x, cols=None):
        seen.append(x[:, :V].double().clone())
        return real(x, cols)
    ops.argmax_rows = spy
    try:
        greedy = lm.generate(input_ids=padded, attention_mask=mask, max_new_tokens=N, eos_token_id=-1, pad_token_id=0,
                             decode_graph=False)
    finally:
        ops.argmax_rows = real
    cached = torch.stack([torch.log_softmax(x, -1) for x in seen], 1).gather(2, greedy.unsqueeze(-1)).squeeze(-1)
    return 4.0 * float((cached - _teacher_forced(lm, gprompt, greedy, V)).abs().max())


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "left-padded"])
def test_returned_logprobs_are_the_teacher_forced_ones_of_the_emitted_ids(dev, llama, greedy_gap, padded):
    """The yardstick is one full forward over [prompt_b | emitted ids] per row, valid tokens only, never the cached path.
    Bound: 4 x the cached greedy path's own per-token gap to such a forward (greedy_gap).
    Measured on an MI355X (bf16): largest deviation 3.926e-03 in both the unpadded and the left-padded case, bound 1.559e-02;
    the bound fits, so it stands as derived."""
    lm, cfg_l = llama
    B, n, N, V = 2, 4, 12, cfg_l["vocab_size"]
    prompt = _ids(cfg_l, B, dev)
    kw = dict(input_ids=prompt, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, do_sample=True, seed=5,
              return_logprobs=True, num_samples=n)
    lens = [prompt.shape[1]] * B
    if padded:                                                     # left padding, two lengths
        mask = torch.ones_like(prompt)
        mask[1, :5] = 0
        kw["attention_mask"] = mask
        lens[1] -= 5
    got = lm.generate(**kw)
    assert got.ids.shape == (B * n, N)
    assert len({tuple(r) for r in got.ids.tolist()}) > B
    err = 0.0
    for b in range(B):
        own = prompt[b:b + 1, prompt.shape[1] - lens[b]:].repeat_interleave(n, 0)
        tf = _teacher_forced(lm, own, got.ids[b * n:(b + 1) * n], V)
        err = max(err, float((got.logprobs[b * n:(b + 1) * n].double() - tf).abs().max()))
    print(f"[parallel samples] {'left-padded' if padded else 'unpadded'}: log-probabilities vs teacher forcing: largest "
          f"deviation {err:.3e}, bound (4 x greedy per-token gap) {greedy_gap:.3e}")
    assert err <= greedy_gap, (err, greedy_gap)


# ----------------------------------------------------------------------------------------------- stops and bans --
def test_stop_sequences_end_rows_independently(dev, llama):
    lm, cfg_l = llama
    B, n, N = 2, 4, 12
    kw = _kw(cfg_l, B, dev, num_samples=n)
    free = lm.generate(**kw)
    seq = free[0, 2:4].tolist()                                     # row 0 ends with it at column 3
    for path in ({}, dict(decode_graph=False)):
        got = lm.generate(stop_sequences=[seq], **kw, **path)
        w = got.shape[1]
        ends = []
        for r in range(B * n):
            row = free[r].tolist()
            cut = next((c + 2 for c in range(N - 1) if row[c:c + 2] == seq), N)
            ends.append(cut)
            assert torch.equal(got[r, :min(cut, w)], free[r, :min(cut, w)]), (r, path)
            assert bool((got[r, cut:] == 0).all()), (r, path)
        assert ends[0] == 4 and max(ends) > 4                      # row 0 stopped, another row went on
        assert w == min(max(ends), N)


def test_bans_and_the_repetition_penalty_see_each_rows_own_prompt(dev, llama):
    lm, cfg_l = llama
    B, n, N = 2, 3, 8
    prompt = _ids(cfg_l, B, dev)
    kw = dict(input_ids=prompt, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, do_sample=True, seed=3, top_k=1,
              num_samples=n)
    free = lm.generate(**kw)
    first = [int(free[b * n, 0]) for b in range(B)]
    last = [int(prompt[b, -1]) for b in range(B)]
    assert last[0] != last[1]
    # a pair that straddles prompt 0's end, and a single id: rows of prompt 0 may not open with first[0]; rows of prompt 1,
    # whose history ends otherwise, still may
    solo = int(free[0, 3])
    bans = [[last[0], first[0]], [solo]]
    f32, _ = _small_llama(dev, torch.float32)
    for model, extra in ((lm, {}), (lm, dict(decode_graph=False)), (f32, dict(use_cache=False))):
        got = model.generate(bad_words_ids=bans, repetition_penalty=1.3, **kw, **extra)
        assert got.shape == (B * n, N)
        assert not bool((got == solo).any()), extra
        assert bool((got[:n, 0] != first[0]).all()), extra
        for r in range(B * n):                                      # the pair never appears, across the prompt's end or inside
            row = [int(prompt[r // n, -1])] + got[r].tolist()
            assert all(row[c:c + 2] != bans[0] for c in range(N)), (r, extra)
    same = lm.generate(bad_words_ids=[[last[0], first[0]]], **kw)
    assert bool((same[n:, 0] == first[1]).all())                   # prompt 1's rows are not touched by prompt 0's history
    # stops: compared with the fp32 recompute reference only in what is exact -- each row ends at its own match
    seq = [int(free[0, 1])]
    for model, extra in ((lm, {}), (f32, dict(use_cache=False))):
        got = model.generate(stop_sequences=[seq], **kw, **extra)
        for r in range(got.shape[0]):
            row = got[r].tolist()
            if seq[0] in row:
                c = row.index(seq[0])
                assert all(x == 0 for x in row[c + 1:]), (r, extra)


# --------------------------------------------------------------------------------------------- weights and LoRA --
def test_both_decode_weights_modes_and_lora_run(dev, llama):
    from test_lora_gpu import _mm_lora
    lm, cfg_l = llama
    kw = _kw(cfg_l, 2, dev, num_samples=4)
    base = lm.generate(**kw)
    for mode, op in (("fp8", "decode_linear_fp8"), ("mxfp4", "decode_linear_mxfp4")):
        with _Spy(op, "decode_step_attn_shared") as spy:
            ids = lm.generate(decode_weights=mode, **kw)
            assert len(spy.calls[op]) > 0 and len(spy.calls["decode_step_attn_shared"]) > 0
            # the streams see B * n = 8 token rows (the e4m3 lm_head also the gathered rows of token 0)
            assert {a[0].shape[0] for a in spy.calls[op]} == {8}
        assert ids.shape == base.shape
        assert torch.equal(ids, lm.generate(decode_weights=mode, **kw))
        with pytest.raises(ValueError, match="33 sequences"):
            lm.generate(decode_weights=mode, **_kw(cfg_l, 3, dev, num_samples=11))
    model, fx = _mm_lora(dev, p=0.0)
    with torch.no_grad():
        for name, q in model.llm.named_parameters():
            if ".lora_B." in name:
                q.copy_(torch.randn_like(q.float()) * 0.05)
    model.eval()
    emb = fx["inputs_embeds"].to(dev).to(torch.bfloat16)
    args = dict(inputs_embeds=emb, max_new_tokens=8, eos_token_id=2, pad_token_id=106, do_sample=True, seed=1, num_samples=3)
    with _Spy("decode_step_attn_shared") as spy:
        a = model.llm.generate(**args)
        assert len(spy.calls["decode_step_attn_shared"]) > 0
    assert a.shape[0] == 3 * emb.shape[0]
    assert torch.equal(a, model.llm.generate(decode_graph=False, **args))


# ---------------------------------------------------------------------------------------- refusals and switches --
def test_each_refusal_names_its_condition(dev, llama):
    lm, cfg_l = llama
    kw = _kw(cfg_l, 2, dev)
    for bad in (0, 33, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="num_samples"):
            lm.generate(num_samples=bad, **kw)
    with pytest.raises(ValueError, match="do_sample=False"):
        lm.generate(num_samples=2, **{**kw, "do_sample": False})
    with pytest.raises(ValueError, match=r"num_beams=2.*not built"):
        lm.generate(num_samples=2, num_beams=2, **kw)
    with pytest.raises(ValueError, match=r"prompt_lookup_num_tokens=3.*not built"):
        lm.generate(num_samples=2, prompt_lookup_num_tokens=3, **{**kw, "do_sample": True})
    with pytest.raises(ValueError, match=r"guidance_scale=2.0.*not built"):
        lm.generate(num_samples=2, guidance_scale=2.0, negative_prompt_ids=kw["input_ids"], **kw)
    with pytest.raises(ValueError, match=r"kv_cache='fp8'.*not built"):
        lm.generate(num_samples=2, kv_cache="fp8", **kw)
    f32, _ = _small_llama(dev, torch.float32)
    with pytest.raises(ValueError, match=r"num_samples=2.*fp32.*use_cache=False"):
        f32.generate(num_samples=2, **kw)
    ref = f32.generate(num_samples=2, use_cache=False, **kw)       # ... which works: the prompt repeated through the recompute loop
    assert ref.shape == (4, 12)
    assert torch.equal(ref, f32.generate(use_cache=False, **{**kw, "input_ids": kw["input_ids"].repeat_interleave(2, 0)}))
    with pytest.raises(ValueError, match=r"num_samples=2.*decode_attn_ok.*use_cache=False"):
        lm.generate(num_samples=2, **{**kw, "max_new_tokens": 16000})
    with pytest.raises(ValueError, match="decode_graph=False"):     # the weight modes keep their refusals
        lm.generate(num_samples=2, decode_weights="fp8", decode_graph=False, **kw)
    with pytest.raises(ValueError, match="SharedPrompt"):           # the engine's own guard
        sp = eng.SharedPrompt(torch.empty(1), torch.empty(1), 2, 1)
        x = torch.zeros((4, cfg_l["hidden_size"]), dtype=torch.bfloat16, device=dev)
        eng.llama_layer_cached(x, 2, 1, 0, sp, 8, None, None, None, 4, 1e-6, *([None] * 9))


def test_set_parallel_samples_reaches_generate_and_resets(dev):
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    for bad in (0, 33, 1.5, None):
        with pytest.raises(ValueError, match="set_parallel_samples"):
            Mo.MM_LLMs.set_parallel_samples(bad)
    assert Mo.PARALLEL_SAMPLES == [1]
    real, seen = model.prepare_inputs_for_generation, []

    def prepare(inputs):
        seen.append(1)
        return real(inputs)
    model.prepare_inputs_for_generation = prepare
    with torch.no_grad(), _Spy("decode_step_attn_shared") as spy:
        base = model(inputs=inp)
        assert spy.calls["decode_step_attn_shared"] == []
        Mo.MM_LLMs.set_sampling(do_sample=True, seed=4)
        Mo.MM_LLMs.set_parallel_samples(3)
        assert Mo.PARALLEL_SAMPLES == [3] and "num_samples" not in Mo.SAMPLING[0]
        seen.clear()
        ids = model(inputs=inp)
        assert len(seen) == 1                                      # the towers and the alignment ran once per prompt
        assert len(spy.calls["decode_step_attn_shared"]) > 0 and spy.calls["decode_step_attn_shared"][0][12] == 3
        assert ids.shape[0] == 3 * base.shape[0] and ids.dtype == torch.long
        Mo.MM_LLMs.set_parallel_samples()
        n_calls = len(spy.calls["decode_step_attn_shared"])
        again = model(inputs=inp)
        assert len(spy.calls["decode_step_attn_shared"]) == n_calls and again.shape[0] == base.shape[0]
        Mo.MM_LLMs.set_sampling()
        assert torch.equal(model(inputs=inp), base)
