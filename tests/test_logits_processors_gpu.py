"""GPU: the logits processors -- ops.logits_process (csrc/logits_process.hip) against the restatement of
tests/logits_proc_ref.py bit for bit, its place in front of the two emits, and generate(repetition_penalty=,
no_repeat_ngram_size=, min_new_tokens=) end to end: the properties the processors promise on the hipGraph path with
every weight and cache format, the fp32 eager loops against a test-side loop, padded batches, and the defaults."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import logits_proc_ref as R  # noqa: E402
from test_decode_kv8_gpu import _Spy, _ids, _small_llama  # noqa: E402
from test_decode_ragged_cpu import masks_of, restated_masked_greedy  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

INF = float("inf")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SHAPES = [(40, 1, 40), (1000, 3, 1024), (32000, 33, 32000)]            # V, rows, pitch
PAD_VALUE = 1e4                                                         # what the columns [V, ld) hold


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.MM_LLMs.set_logits_processors()
    ops.clear_fp8_cache()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _logits(V, rows, ld, dtype, seed):
    """randn * 4 with +0, -0 and -inf sprinkled in, rounded to dtype; pad columns = 1e4 (CPU tensor [rows, ld])"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 4
    for val in (0.0, -0.0, -INF):
        x[torch.randint(0, rows, (V // 10,), generator=g), torch.randint(0, V, (V // 10,), generator=g)] = val
    full = torch.full((rows, ld), PAD_VALUE)
    full[:, :V] = x
    return full.to(dtype)


def _id_rows(V, rows, width, seed):
    """[rows, width] ids, row b drawn from a pool of 7, 50 or V values (b % 3): heavy duplication, repeated n-grams"""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty((rows, width), dtype=torch.long)
    for b in range(rows):
        pool = torch.randint(0, V, ((7, 50, V)[b % 3],), generator=g)
        out[b] = pool[torch.randint(0, pool.numel(), (width,), generator=g)]
    return out


# (theta, n, m relative to the generated count: None = off, 0 = count == m, 1 = count == m - 1)
CONFIGS = [(0.7, 0, None), (1.3, 0, None), (1.0, 1, None), (1.0, 2, None), (1.0, 3, None), (1.0, 5, None), (1.0, 0, 1),
           (1.0, 0, 0), (1.3, 3, 1), (0.7, 2, 1), (1.3, 5, 0), (0.7, 1, 1)]


# ----------------------------------------------------------------------------- 1. the kernel vs the restatement --
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("V,rows,ld", SHAPES)
def test_kernel_is_the_restatement_bit_for_bit(dev, V, rows, ld, dtype):
    """history lengths 0, 1, n - 1, n, 300 and 1100 (a 1000-id prompt + 100 generated: more than one pass of the 1024
    threads), spread over the rows through the per-row prompt count; the count once through n_add and once through a
    device int32; a call without a prompt; the padding columns and every column the history does not name keep their
    bits"""
    x0 = _logits(V, rows, ld, dtype, seed=V)
    prompt = _id_rows(V, rows, 1000, seed=V + 1)
    gen = _id_rows(V, rows, 100, seed=V + 2)
    gen_buf = torch.full((rows, 128), -5, dtype=torch.long)             # (columns past the count are never read)
    gen_buf[:, :100] = gen
    prompt_d, gen_d = prompt.to(dev), gen_buf.to(dev)
    eos = int(prompt[0, 0])
    for ci, (theta, n, mrel) in enumerate(CONFIGS):
        scenarios = [([0, 1, max(n - 1, 0), n, 300, 1000], 0), ([0, 200, 1000], 100), (None, 1), (None, max(n - 1, 0)),
                     (None, n), (None, 100)]
        if rows == 1:                                                   # one row: its prompt count per launch
            scenarios = [([p], c) for ps, c in scenarios[:2] for p in ps] + scenarios[2:]
        for lens, count in scenarios:
            m = 0 if mrel is None else count + mrel
            if lens is None:
                prompts, p_d, l_d = None, None, None
            else:
                pl = [lens[(b + ci) % len(lens)] for b in range(rows)]
                prompts = [prompt[b, :pl[b]].tolist() for b in range(rows)]
                p_d, l_d = prompt_d, torch.tensor(pl, dtype=torch.int32, device=dev)
            want = x0.clone()
            want[:, :V] = R.process(x0[:, :V], prompts, [gen[b, :count].tolist() for b in range(rows)], theta, n, m, eos)
            xa = x0.to(dev)
            ops.logits_process(xa[:, :V], V, gen_d, None, count, p_d, l_d, theta, n, m, eos)
            xb = x0.to(dev)
            n_dev = torch.tensor([count - 3, 77], dtype=torch.int32, device=dev)        # n = *n_dev + n_add
            ops.logits_process(xb[:, :V], V, gen_d, n_dev, 3, p_d, l_d, theta, n, m, eos)
            assert torch.equal(_bits(xa.cpu()), _bits(want)), (theta, n, m, lens, count)
            assert torch.equal(_bits(xb), _bits(xa)), (theta, n, m, lens, count)
            if theta != 1.0 and count == 100 and lens is not None:      # the case does something
                assert not torch.equal(_bits(want), _bits(x0))
    assert n_dev.tolist() == [97, 77]                                   # the counter is only read


def test_everything_off_launches_nothing_and_out_of_range_ids_change_nothing(dev):
    V = 64
    x0 = _logits(V, 2, V, torch.float32, seed=5)
    gen = torch.tensor([[3, -1, 64, 10 ** 12, 3], [70, 3, 9, 70, 3]], device=dev)
    x = x0.to(dev)
    ops.logits_process(x, V, gen, None, 5)                                              # the defaults
    ops.logits_process(x, V, gen, None, 0, min_new_tokens=4, eos=None)                  # no eos: min_new_tokens is off
    assert torch.equal(_bits(x.cpu()), _bits(x0))
    ops.logits_process(x, V, gen, None, 5, repetition_penalty=1.5, no_repeat_ngram_size=2)
    want = R.process(x0, None, gen.tolist(), 1.5, 2)                    # ids outside [0, V) name no column
    assert torch.equal(_bits(x.cpu()), _bits(want))
    assert want[1, 9] == -INF                                           # (70, 3) repeats: 9 followed it
    rest = [c for c in range(V) if c not in (3, 9)]
    assert torch.equal(_bits(want[:, rest]), _bits(x0[:, rest]))        # row 0 bans -1, which is no column


# ------------------------------------------------------------------------------------- 2. in front of the emits --
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_process_then_emit_gives_the_restatements_argmax_and_keeps_the_books(dev, B, dtype):
    V, ld, col, pad = 1000, 1008, 5, 1003
    x0 = _logits(V, B, ld, dtype, seed=B)
    top = x0[:, :V].float().argmax(-1)
    gen = _id_rows(V, B, col, seed=B + 1)
    gen[:, col - 1] = top                                               # greedy's token is in every history: it is hit
    prompt = _id_rows(V, B, 9, seed=B + 2)
    p_len = torch.full((B,), 9, dtype=torch.int32, device=dev)
    args = (1e30, 2, col + 1)                                           # theta, n, m
    want = R.process(x0[:, :V], prompt.tolist(), gen.tolist(), *args, eos=7).float().argmax(-1)
    assert not torch.equal(want, top)
    for sampled in (False, True):
        x = x0.to(dev)
        out = torch.full((B, col + 3), -7, dtype=torch.long, device=dev)
        out[:, :col] = gen.to(dev)
        tok = torch.full((B,), -1, dtype=torch.long, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        if B > 1:
            done[1] = True
        state = torch.tensor([11, col, 0, 0], dtype=torch.int32, device=dev)
        ops.logits_process(x[:, :V], V, out, state[1:2], 0, prompt.to(dev), p_len, *args, eos=7)
        assert state.tolist() == [11, col, 0, 0]
        if sampled:
            ops.decode_emit_sample(x[:, :V], V, pad, 7, tok, done, out, state, 0.8, 1, 1.0, 42)
        else:
            ops.decode_emit(x[:, :V], V, pad, 7, tok, done, out, state)
        exp = want.clone().to(dev)
        if B > 1:
            exp[1] = pad
        assert torch.equal(out[:, col], exp) and torch.equal(tok, exp), sampled
        assert torch.equal(out[:, :col], gen.to(dev)) and bool((out[:, col + 1:] == -7).all())
        assert state.tolist() == [12, col + 1, 0, 0]
        assert not bool((exp == 7).any()) and torch.equal(done, (torch.arange(B, device=dev) == 1) & (B > 1))


# ------------------------------------------------------------------------------------ 3. generate(): hipGraph path --
MODES = [dict(), dict(decode_weights="fp8"), dict(decode_weights="mxfp4"), dict(kv_cache="fp8")]
MODE_IDS = ["16bit", "w-fp8", "w-mxfp4", "kv-fp8"]
N_GRAM, N_LONG, N_DISTINCT = 2, 64, 24


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_generate_graph_path_keeps_the_three_promises(dev, mode, dtype):
    lm, cfg_l = _small_llama(dev, dtype)
    V = cfg_l["vocab_size"]
    B = 3
    ids = _ids(cfg_l, B, dev)
    kw = dict(input_ids=ids, eos_token_id=-1, pad_token_id=0, **mode)
    assert N_DISTINCT <= V // 4
    with _Spy("logits_process", "decode_emit", "decode_emit_sample") as spy:
        plain = lm.generate(max_new_tokens=N_LONG, **kw)
        assert spy.calls["logits_process"] == [] and len(spy.calls["decode_emit"]) == 3
        # greedy loops: without the argument the ids repeat an n-gram, so the property below shows something
        assert any(R.has_repeated_ngram(plain[b].tolist(), N_GRAM) for b in range(B)), plain.tolist()
        got = lm.generate(max_new_tokens=N_LONG, no_repeat_ngram_size=N_GRAM, **kw)
        # token 0, one eager step, one captured step: the other N_LONG - 3 tokens are replays
        assert len(spy.calls["logits_process"]) == 3 and len(spy.calls["decode_emit"]) == 6
    assert got.shape == (B, N_LONG)
    for b in range(B):
        assert not R.has_repeated_ngram(got[b].tolist(), N_GRAM), (b, got[b].tolist())
        assert not R.completes_repeated_ngram(ids[b].tolist(), got[b].tolist(), N_GRAM), b  # the prompt is history
    # the distinct-token property: the penalty makes every positive seen logit ~0 and every negative one ~-inf
    d = lm.generate(max_new_tokens=N_DISTINCT, repetition_penalty=1e30, **kw)
    assert d.shape == (B, N_DISTINCT)
    assert all(len(set(d[b].tolist())) == N_DISTINCT for b in range(B)), d.tolist()
    # min_new_tokens: eos = plain greedy's first token of row 0
    eos, m = int(plain[0, 0]), 9
    short = lm.generate(max_new_tokens=N_DISTINCT, **{**kw, "eos_token_id": eos})
    assert int(short[0, 0]) == eos and bool((short[0, 1:] == 0).all())
    late = lm.generate(max_new_tokens=N_DISTINCT, min_new_tokens=m, **{**kw, "eos_token_id": eos})
    assert late.shape[1] >= m and not bool((late[:, :m] == eos).any()), late.tolist()
    # sampling runs behind the processors: top_k = 1 draws the processed argmax
    pk = dict(max_new_tokens=N_DISTINCT, repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=m,
              **{**kw, "eos_token_id": eos})
    with _Spy("logits_process", "decode_emit_sample") as spy:
        greedy = lm.generate(**pk)
        sampled = lm.generate(do_sample=True, top_k=1, temperature=0.7, seed=3, **pk)
        assert len(spy.calls["decode_emit_sample"]) == 3 and len(spy.calls["logits_process"]) == 6
    assert torch.equal(greedy, sampled)
    assert not bool((greedy[:, :m] == eos).any())
    assert not any(R.completes_repeated_ngram(ids[b].tolist(), greedy[b].tolist(), 3) for b in range(B)
                   if not bool((greedy[b] == eos).any()))


def test_generate_eager_cached_loop_keeps_the_promises_with_the_host_count(dev):
    """decode_graph=False in 16 bits: the eager cached loop, one launch per token, the count through n_add"""
    lm, cfg_l = _small_llama(dev)
    kw = dict(input_ids=_ids(cfg_l, 3, dev), max_new_tokens=N_DISTINCT, eos_token_id=-1, pad_token_id=0,
              repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4)
    with _Spy("logits_process") as spy:
        g = lm.generate(**kw)
        e = lm.generate(decode_graph=False, **kw)
        assert len(spy.calls["logits_process"]) == 3 + N_DISTINCT
    assert g.shape == e.shape == (3, N_DISTINCT)
    for b in range(3):
        assert not R.has_repeated_ngram(e[b].tolist(), 2) and not R.has_repeated_ngram(g[b].tolist(), 2)


# -------------------------------------------------------------------------------- 4. fp32: the two eager loops --
@pytest.mark.parametrize("with_ids", [True, False], ids=["prompt-history", "generated-only"])
def test_generate_fp32_loops_emit_the_ids_of_forward_restatement_argmax(dev, with_ids):
    lm, cfg_l = _small_llama(dev, torch.float32)
    B, N = 2, 12
    ids = _ids(cfg_l, B, dev)
    args = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=5)
    with torch.no_grad():
        eos = int(lm(input_ids=ids).logits[0, -1].argmax())             # plain greedy's first token of row 0
        seq, gen, done = ids.clone(), [[] for _ in range(B)], [False] * B
        for t in range(N):                                              # generate()'s loop: pad once a row has its eos
            z = lm(input_ids=seq).logits[:, -1].float().cpu()
            p = R.process(z, ids.tolist() if with_ids else None, gen, eos=eos, **args)
            nxt = [0 if done[b] else int(p[b].argmax()) for b in range(B)]
            for b in range(B):
                gen[b].append(nxt[b])
                done[b] = done[b] or nxt[b] == eos
            if all(done):
                break
            seq = torch.cat([seq, torch.tensor(nxt, device=dev)[:, None]], dim=1)
    want = torch.tensor(gen)
    assert want.shape[1] > 5 and not bool((want[:, :5] == eos).any())
    kw = dict(max_new_tokens=N, eos_token_id=eos, pad_token_id=0, **args)
    kw.update(dict(input_ids=ids) if with_ids else dict(inputs_embeds=lm.model.embed_tokens(ids)))
    for path in (dict(use_cache=True), dict(use_cache=False)):
        with _Spy("logits_process", "decode_emit") as spy:
            got = lm.generate(**kw, **path)
            assert len(spy.calls["logits_process"]) == want.shape[1] and spy.calls["decode_emit"] == []
        assert torch.equal(got.cpu(), want), (path, got.tolist(), want.tolist())
    both = lm.generate(**{**kw, "input_ids": ids, "inputs_embeds": lm.model.embed_tokens(ids)})
    if with_ids:
        assert torch.equal(both.cpu(), want)                            # input_ids next to inputs_embeds is history


# ------------------------------------------------------------------------------------------ 5. padded batches --
def _pad_masks(B, S0):
    ms = masks_of(B, S0)
    for b in range(B):
        ms["left"][b, :2 + 3 * b] = 0
    return {k: ms[k] for k in ("left", "holes")}


@pytest.mark.parametrize("kind", ["left", "holes"])
def test_generate_padded_fp32_ids_are_those_of_each_sample_alone(dev, kind):
    """use_cache=False in fp32 (the loop that takes a padded mask in every dtype): sample b of the padded batch emits
    what its valid ids alone, unpadded, emit with the same processors -- only the valid prompt ids are history"""
    lm, cfg_l = _small_llama(dev, torch.float32)
    B, S0, N = 3, 21, 12
    ids = _ids(cfg_l, B, dev)
    mask = _pad_masks(B, S0)[kind].to(dev)
    kw = dict(max_new_tokens=N, eos_token_id=-1, pad_token_id=0, use_cache=False, repetition_penalty=1.3,
              no_repeat_ngram_size=2)
    got = lm.generate(input_ids=ids, attention_mask=mask, **kw)
    assert got.shape == (B, N)
    differs = False
    for b in range(B):
        solo_ids = ids[b:b + 1][:, mask[b].bool()].contiguous()
        one = lm.generate(input_ids=solo_ids, **kw)
        assert torch.equal(one[0], got[b]), (b, one[0].tolist(), got[b].tolist())
        assert not R.completes_repeated_ngram(solo_ids[0].tolist(), got[b].tolist(), 2)
        differs |= not torch.equal(lm.generate(input_ids=solo_ids, **{**kw, "repetition_penalty": 1.0,
                                                                      "no_repeat_ngram_size": 0})[0], got[b])
    assert differs                                                      # the processors changed something


@pytest.mark.parametrize("kind", ["left", "holes"])
def test_generate_padded_bf16_graph_ids_against_the_fp32_oracle(dev, kind):
    """the rule of test_decode_ragged_gpu for greedy, on the processed logits: every id emitted on the hipGraph path and
    on the kernel-by-kernel step loop is the argmax of the restated processors over the fp32 oracle's logits,
    teacher-forced on the path's own ids with each sample's valid prompt ids as history, or loses to it by no more than
    the bf16 noise there: p32[top] - p32[id] <= 3.0 * max|p16 - p32| over the columns that are finite in both"""
    lm, cfg_l = _small_llama(dev)
    B, S0, N = 3, 21, 12
    ids = _ids(cfg_l, B, dev)
    mask = _pad_masks(B, S0)[kind].to(dev)
    args = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, **args)
    with _Spy("logits_process", "decode_step_attn_var") as spy:
        g = lm.generate(**kw)
        assert len(spy.calls["logits_process"]) == 3 and len(spy.calls["decode_step_attn_var"]) > 0
        e = lm.generate(decode_graph=False, **kw)
    assert g.shape == e.shape == (B, N) and torch.equal(g, e)
    valid = [ids[b][mask[b].bool()].tolist() for b in range(B)]
    sd32 = {"llm." + k: v.detach().float() for k, v in lm.state_dict().items()}
    sd16 = {k: v.to(torch.bfloat16) for k, v in sd32.items()}
    emb = torch.nn.functional.embedding(ids, sd32["llm.model.embed_tokens.weight"])
    with torch.no_grad():
        _, z32 = restated_masked_greedy(sd32, emb, mask, cfg_l, N, force_ids=g)
        _, z16 = restated_masked_greedy(sd16, emb.to(torch.bfloat16), mask, cfg_l, N, force_ids=g)
    z32, z16, gc = z32.float().cpu(), z16.float().cpu(), g.cpu()
    for t in range(N):
        gen = [gc[b, :t].tolist() for b in range(B)]
        p32, p16 = R.process(z32[:, t], valid, gen, **args), R.process(z16[:, t], valid, gen, **args)
        for b in range(B):
            c = int(gc[b, t])
            fin = torch.isfinite(p32[b]) & torch.isfinite(p16[b])
            assert p32[b, c] > -INF, (t, b, c)                          # never a banned id
            margin = float(p32[b].max() - p32[b, c])
            noise = float((p16[b][fin] - p32[b][fin]).abs().max())
            assert margin <= 3.0 * noise, (kind, t, b, margin, noise)
    assert not any(R.completes_repeated_ngram(valid[b], gc[b].tolist(), 2) for b in range(B))


# ------------------------------------------------------------------------------------------------ 6. defaults --
def test_default_generate_never_calls_logits_process_and_the_model_wide_switch_reaches_it(dev):
    lm, cfg_l = _small_llama(dev)
    kw = dict(input_ids=_ids(cfg_l, 2, dev), max_new_tokens=8, eos_token_id=-1, pad_token_id=0)
    with _Spy("logits_process") as spy:
        a = lm.generate(**kw)
        b = lm.generate(decode_graph=False, **kw)
        c = lm.generate(use_cache=False, **kw)
        d = lm.generate(num_beams=2, **kw)
        lm.generate(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, **kw)
        assert spy.calls["logits_process"] == []
    assert a.shape == b.shape == c.shape == (2, 8) and d.shape[0] == 2
    with pytest.raises(ValueError, match="no_repeat_ngram_size.*not built"):
        lm.generate(num_beams=2, no_repeat_ngram_size=2, **kw)
    from golden_util import load_case
    from oracle import configs
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    model = build_model(configs.get(fx["config_name"]), fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    with torch.no_grad(), _Spy("logits_process") as spy:
        base = model(inputs=inp)
        assert spy.calls["logits_process"] == []
        Mo.MM_LLMs.set_logits_processors(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8)
        ids = model(inputs=inp)
        calls = spy.calls["logits_process"]
        assert len(calls) > 0 and tuple(calls[0][7:10]) == (1.2, 3, 8) and calls[0][5] is None   # no prompt history
        Mo.MM_LLMs.set_logits_processors()
        n = len(calls)
        assert torch.equal(model(inputs=inp), base) and len(spy.calls["logits_process"]) == n
    assert not bool((ids[:, :8] == 2).any())                            # min_new_tokens = 8 with the call's eos = 2
    for b in range(ids.shape[0]):
        row = ids[b].tolist()
        row = row[:row.index(2) + 1] if 2 in row else row
        assert not R.has_repeated_ngram(row, 3), (b, row)
