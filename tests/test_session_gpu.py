"""generate(return_session=True) / generate(session=s) on the GPU: three turns of a batch of three on two micro decoders
(hidden 128, FF 384, 2 layers, vocab 107, bf16) -- 2 heads (head size 64: mk_flash_attn_varlen_fwd) and 4 heads (head
size 32: the per-sample host loop) -- held to the rule of GenerateSession:

  turn 1   B = 3, S0 = 21, the `left` mask of test_decode_ragged_gpu._lm_masks, 6 new tokens, eos = the most frequent
           free-running token, so the samples end at different columns;
  turn 2   a [3, 9] prompt with 9, 4 (padded right) and 1 (padded left) valid tokens, 8 new tokens;
  turn 3   one new token per sample (Sn = 1, q_len = 2).

1. oracle: every emitted id is the argmax of the fp32 restatement (restated_masked_greedy, teacher-forced on the call's
   own ids over the concatenated history with its mask) or loses to it by no more than the bf16 noise there,
   z32[top] - z32[id] <= 3.0 * max|z16 - z32| (the rule of test_decode_ragged_gpu);  2. exact: graph == eager step loop
   (ids and log-probabilities), regrown == preallocated caches, the session's books;  3. routing;  4. the history
   matters;  5. composition;  6. refused calls leave the session as it was;  7. MM_LLMs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
import logits_proc_ref as LP  # noqa: E402
from test_decode_ragged_cpu import masks_of, restated_masked_greedy  # noqa: E402

B, S0, N1, N2, N3, PAD = 3, 21, 6, 8, 5, 0
T2_MASK = torch.tensor([[1] * 9, [1] * 4 + [0] * 5, [0] * 8 + [1]])      # 9, 4 (padded right) and 1 (padded left) valid


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    Mo.AUTO_FUSE = True
    Mo.MM_LLMs.set_session()


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


_LM = {}


def _small_llama(dev, heads):
    """test_decode_ragged_gpu._small_llama with `heads` attention heads; built once per head count, never modified"""
    if heads not in _LM:
        from transformers import LlamaConfig
        cfg_l = dict(configs.get(load_case("micro_all")["config_name"])["llama"])
        cfg_l.update(intermediate_size=384, num_attention_heads=heads, num_key_value_heads=heads)
        torch.manual_seed(0)
        Mo.AUTO_FUSE = True
        lm = Mo.LlamaForCausalLM(LlamaConfig(**cfg_l)).to(dev).to(torch.bfloat16)
        lm = Mo.fuse_model(lm).eval()
        sd32 = {"llm." + k: v.detach().float() for k, v in lm.state_dict().items()}
        _LM[heads] = (lm, cfg_l, sd32, {k: v.to(torch.bfloat16) for k, v in sd32.items()})
    return _LM[heads]


def _prompts(cfg_l, dev):
    g = torch.Generator().manual_seed(B)
    ids1 = torch.randint(3, cfg_l["vocab_size"], (B, S0), generator=g)
    mask1 = masks_of(B, S0)["left"]
    for b in range(B):                                  # (_lm_masks: every sample padded somewhere)
        mask1[b, :2 + 3 * b] = 0
    ids2 = torch.randint(3, cfg_l["vocab_size"], (B, 9), generator=g)
    ids3 = torch.randint(3, cfg_l["vocab_size"], (B, 1), generator=g)
    return [(ids1.to(dev), mask1.to(dev)), (ids2.to(dev), T2_MASK.to(dev)), (ids3.to(dev), None)]


_EOS = {}


def _eos(dev, heads):
    """the most frequent free-running token of turn 1 behind its first two columns (the trick of
    test_generate_padded_early_stop_...): some sample meets it early"""
    if heads not in _EOS:
        lm, cfg_l = _small_llama(dev, heads)[:2]
        ids, mask = _prompts(cfg_l, dev)[0]
        free = lm.generate(input_ids=ids, attention_mask=mask, max_new_tokens=N1, eos_token_id=-1, pad_token_id=PAD)
        _EOS[heads] = int(free[:, 2:].flatten().mode().values)
    return _EOS[heads]


def _final(row, eos, stop=None):
    """the rule, restated: generated tokens up to and including the eos / the stop sequence's last id / the last token"""
    for t in range(len(row)):
        if row[t] == eos or any(len(q) <= t + 1 and row[t + 1 - len(q):t + 1] == q for q in (stop or [])):
            return t + 1
    return len(row)


class _Talk:
    """the histories of the batch by the rule, kept by the test itself"""

    def __init__(self):
        self.hist = [[] for _ in range(B)]

    def prompt(self, ids, mask):
        new = [ids[b].cpu()[(mask[b].cpu() != 0) if mask is not None else slice(None)].tolist() for b in range(B)]
        before = [list(h) for h in self.hist]
        for h, n in zip(self.hist, new):
            h.extend(n)
        return before, new

    def answer(self, got, eos, stop=None):
        rows = got.cpu().tolist()
        c = [_final(r, eos, stop) for r in rows]
        for h, r, cb in zip(self.hist, rows, c):
            h.extend(r[:cb])
        return c


def _oracle(model, hist, got, c, what, dev, process=None):
    """hist[b]: the ids sample b's call ran on (history by the rule + valid new tokens); got [B, w] the call's ids; c[b]
    its tokens up to the final one.  Columns behind c[b] hold pad and are not looked at."""
    lm, cfg_l, sd32, sd16 = model
    L = max(len(h) for h in hist)
    ids = torch.zeros((B, L), dtype=torch.long)
    mask = torch.zeros((B, L), dtype=torch.long)
    for b, h in enumerate(hist):                        # right padding: any pattern is the same sample alone
        ids[b, :len(h)] = torch.tensor(h)
        mask[b, :len(h)] = 1
    ids, mask = ids.to(dev), mask.to(dev)
    emb = torch.nn.functional.embedding(ids, sd32["llm.model.embed_tokens.weight"])
    w = got.shape[1]
    with torch.no_grad():
        _, z32 = restated_masked_greedy(sd32, emb, mask, cfg_l, w, force_ids=got)
        _, z16 = restated_masked_greedy(sd16, emb.to(torch.bfloat16), mask, cfg_l, w, force_ids=got)
    z32, z16, gc = z32.float().cpu(), z16.float().cpu(), got.cpu()
    worst, off = 0.0, 0
    for b in range(B):
        for t in range(c[b]):
            p32, p16 = z32[b, t], z16[b, t]
            if process is not None:
                p32, p16 = process(p32, b, gc[b, :t].tolist()), process(p16, b, gc[b, :t].tolist())
            fin = torch.isfinite(p32) & torch.isfinite(p16)
            margin = float(p32.max() - p32[gc[b, t]])
            noise = float((p16[fin] - p32[fin]).abs().max())
            worst, off = max(worst, margin / max(noise, 1e-12)), off + (margin > 0)
            assert margin <= 3.0 * noise, (what, b, t, margin, noise)
    print(f"{what}: ids off the oracle's argmax {off}, worst margin / noise {worst:.3f}")


def _turn(lm, turn, prompts, eos, session=None, n=None, **kw):
    ids, mask = prompts[turn]
    n = n if n is not None else (N1, N2, N3)[turn]
    args = dict(input_ids=ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=PAD, **kw)
    if mask is not None:
        args["attention_mask"] = mask
    if session is None:
        return lm.generate(return_session=True, **args)
    return lm.generate(session=session, **args), session


def _state(s):
    return (s.batch, s.lengths, s.capacity, s.turns, s.ids, s._cached.tolist(), s._pending.tolist(), s._cached_host,
            [k.data_ptr() for k in s._kvc])


# ---------------------------------------------------------------------------------- 1., 2. oracle and books --
@pytest.mark.parametrize("heads", [2, 4], ids=["hd64-varlen", "hd32-host-loop"])
def test_three_turns_against_the_fp32_oracle_with_the_books_the_rule_says(dev, heads):
    model = _small_llama(dev, heads)
    lm, cfg_l = model[:2]
    prompts, eos = _prompts(cfg_l, dev), _eos(dev, heads)
    talk, s, s_big = _Talk(), None, None
    for turn in range(3):
        before, new = talk.prompt(*prompts[turn])
        got, s = _turn(lm, turn, prompts, eos, s)
        big, s_big = _turn(lm, turn, prompts, eos, s_big, **(dict(session_capacity=96) if turn == 0 else {}))
        assert got.dtype == torch.long and got.shape[0] == B and got.shape[1] <= (N1, N2, N3)[turn]
        ran_on = [h + n for h, n in zip(before, new)]
        c = talk.answer(got, eos)
        print(f"heads {heads} turn {turn + 1}: ids {got.tolist()}, tokens up to the final one {c}")
        _oracle(model, ran_on, got, c, f"heads {heads} turn {turn + 1}", dev)
        # the books: lengths, turns and ids are what the rule says
        assert isinstance(s, Mo.GenerateSession) and s.batch == B and s.turns == turn + 1
        assert s.ids == talk.hist and s.lengths == [len(h) for h in talk.hist]
        assert s._cached.tolist() == [n - 1 for n in s.lengths] and s._pending.tolist() == [h[-1] for h in talk.hist]
        if turn == 0:
            assert len(set(s.lengths)) > 1, s.lengths           # the samples' histories differ in length
            assert s.capacity == S0 + N1 and s_big.capacity == 96
        # a session that had to regrow == one allocated large enough for all turns
        assert torch.equal(big, got), (turn, big.tolist(), got.tolist())
        assert s_big.lengths == s.lengths and s_big.ids == s.ids
    assert s.capacity > S0 + N1 and s_big.capacity == 96            # one regrew, the other never had to


def test_graph_and_eager_step_loop_agree_on_a_continued_call(dev):
    model = _small_llama(dev, 2)
    lm, cfg_l = model[:2]
    prompts, eos = _prompts(cfg_l, dev), _eos(dev, 2)
    outs = []
    for path in (dict(), dict(decode_graph=False)):
        _, s = _turn(lm, 0, prompts, eos)
        r, _ = _turn(lm, 1, prompts, eos, s, return_logprobs=True, top_logprobs=2, **path)
        outs.append((r, _state(s)[:8]))
    (g, sg), (e, se) = outs
    assert isinstance(g, Mo.GenerateLogprobs) and torch.equal(g.ids, e.ids)
    assert torch.equal(g.logprobs, e.logprobs) and torch.equal(g.top_ids, e.top_ids)
    assert torch.equal(g.top_logprobs, e.top_logprobs)
    assert sg == se


# ------------------------------------------------------------------------------------------------ 3. routing --
@pytest.mark.parametrize("heads", [2, 4], ids=["hd64-varlen", "hd32-host-loop"])
def test_a_continued_call_runs_the_new_prefill_and_the_ragged_steps_only(dev, heads):
    lm, cfg_l = _small_llama(dev, heads)[:2]
    nl = cfg_l["num_hidden_layers"]
    prompts, eos = _prompts(cfg_l, dev), _eos(dev, heads)
    names = ("flash_attn_varlen_fwd", "flash_attn_fwd", "kv_append_rows", "decode_step_attn_var", "decode_step_attn",
             "softmax_fwd")
    with _Spy(*names) as spy:
        plain = lm.generate(input_ids=prompts[0][0], max_new_tokens=N1, eos_token_id=-1, pad_token_id=PAD)
        assert spy.calls["flash_attn_varlen_fwd"] == [] and spy.calls["kv_append_rows"] == []     # the defaults: none
        assert spy.calls["decode_step_attn_var"] == [] and len(spy.calls["decode_step_attn"]) == 2 * nl
    _, s = _turn(lm, 0, prompts, eos)
    with _Spy(*names) as spy:
        first = lm.generate(input_ids=prompts[0][0], max_new_tokens=N1, eos_token_id=-1, pad_token_id=PAD,
                            return_session=True)[0]
        assert torch.equal(first, plain)                           # a first call runs exactly today's launches
        assert spy.calls["flash_attn_varlen_fwd"] == [] and spy.calls["kv_append_rows"] == []
        assert spy.calls["decode_step_attn_var"] == [] and len(spy.calls["decode_step_attn"]) == 2 * nl
    Sc = 1 + int(T2_MASK.sum(1).max())
    with _Spy(*names) as spy:
        _turn(lm, 1, prompts, -1, s)                               # (no eos: the loop reaches its captured step)
        assert len(spy.calls["kv_append_rows"]) == nl
        assert len(spy.calls["decode_step_attn_var"]) == 2 * nl and spy.calls["decode_step_attn"] == []
        assert spy.calls["flash_attn_fwd"] == []
        if heads == 2:
            assert len(spy.calls["flash_attn_varlen_fwd"]) == nl and spy.calls["softmax_fwd"] == []
            assert all(a[8] == Sc and a[6] == B for a in spy.calls["flash_attn_varlen_fwd"])       # Lq = Sc
        else:
            assert spy.calls["flash_attn_varlen_fwd"] == [] and len(spy.calls["softmax_fwd"]) == nl * B


# ----------------------------------------------------------------------------------------- 4. it matters --
def test_the_kept_history_changes_what_the_second_turn_says(dev):
    lm, cfg_l = _small_llama(dev, 2)[:2]
    prompts, eos = _prompts(cfg_l, dev), _eos(dev, 2)
    _, s = _turn(lm, 0, prompts, eos)
    kept, _ = _turn(lm, 1, prompts, eos, s)
    ids, mask = prompts[1]
    fresh = lm.generate(input_ids=ids, attention_mask=mask, max_new_tokens=N2, eos_token_id=eos, pad_token_id=PAD)
    print(f"turn 2 over the session {kept.tolist()}, on its prompt alone {fresh.tolist()}")
    w = min(kept.shape[1], fresh.shape[1])
    assert kept.shape != fresh.shape or not torch.equal(kept[:, :w], fresh[:, :w])


# ------------------------------------------------------------------------------------------ 5. composition --
def test_a_continued_call_composes_with_fp8_weights_and_sampling(dev):
    lm, cfg_l = _small_llama(dev, 2)[:2]
    prompts, eos = _prompts(cfg_l, dev), _eos(dev, 2)
    _, s = _turn(lm, 0, prompts, eos)
    with _Spy("decode_linear_fp8", "flash_attn_varlen_fwd") as spy:
        got, _ = _turn(lm, 1, prompts, -1, s, decode_weights="fp8")
        assert len(spy.calls["decode_linear_fp8"]) > 0 and len(spy.calls["flash_attn_varlen_fwd"]) == cfg_l["num_hidden_layers"]
    assert got.shape == (B, N2) and s.turns == 2 and s.lengths == [len(r) for r in s.ids]
    drawn = []
    for _ in range(2):
        _, s = _turn(lm, 0, prompts, eos)
        drawn.append(_turn(lm, 1, prompts, -1, s, do_sample=True, seed=1234, temperature=1.3)[0])
    assert torch.equal(drawn[0], drawn[1]), (drawn[0].tolist(), drawn[1].tolist())
    _, s = _turn(lm, 0, prompts, eos)
    other = _turn(lm, 1, prompts, -1, s, do_sample=True, seed=99, temperature=1.3)[0]
    assert not torch.equal(other, drawn[0])


def test_the_penalised_history_of_a_continued_call_includes_the_earlier_turns(dev):
    model = _small_llama(dev, 2)
    lm, cfg_l = model[:2]
    prompts, eos = _prompts(cfg_l, dev), _eos(dev, 2)
    talk = _Talk()
    talk.prompt(*prompts[0])
    got1, s = _turn(lm, 0, prompts, eos)
    talk.answer(got1, eos)
    before, new = talk.prompt(*prompts[1])
    known = [h + n for h, n in zip(before, new)]
    args = dict(repetition_penalty=1.3)
    with _Spy("logits_process") as spy:
        got, _ = _turn(lm, 1, prompts, -1, s, **args)
        calls = spy.calls["logits_process"]
    # ops.logits_process(lg, V, gen, n_dev, n_add, hist, hist_len, ...): the history table handed to the kernel
    hist, hist_len = calls[-1][5].cpu(), calls[-1][6].cpu().tolist()
    assert hist_len == [len(k) for k in known]
    assert all(hist[b, :hist_len[b]].tolist() == known[b] for b in range(B))
    c = talk.answer(got, -1)
    assert c == [N2] * B
    _oracle(model, known, got, c, "repetition_penalty over the session's history", dev,
            process=lambda z, b, gen: LP.process_row(z, known[b] + gen, len(gen), **args))
    # (and the earlier turns do add ids of their own to that history)
    assert any(set(before[b]) - set(new[b]) - set(got[b].tolist()) for b in range(B))


def test_a_stop_sequence_ends_a_sample_and_its_last_id_leads_the_next_chunk(dev):
    model = _small_llama(dev, 2)
    lm, cfg_l = model[:2]
    prompts, eos = _prompts(cfg_l, dev), _eos(dev, 2)
    _, s = _turn(lm, 0, prompts, eos)
    free, _ = _turn(lm, 1, prompts, -1, s)
    stop = [free[0, 1:3].tolist()]                      # sample 0's second and third token of the free-running turn
    talk = _Talk()
    talk.prompt(*prompts[0])
    got1, s = _turn(lm, 0, prompts, eos)
    talk.answer(got1, eos)
    talk.prompt(*prompts[1])
    got2, _ = _turn(lm, 1, prompts, -1, s, stop_sequences=stop)
    c = talk.answer(got2, -1, stop)
    assert c[0] == 3 and got2[0, :3].tolist() == free[0, :3].tolist() and bool((got2[0, 3:] == PAD).all())
    assert s._pending.tolist()[0] == stop[0][-1] and s.ids == talk.hist and s.lengths == [len(h) for h in talk.hist]
    before, new = talk.prompt(*prompts[2])
    got3, _ = _turn(lm, 2, prompts, -1, s)
    _oracle(model, [h + n for h, n in zip(before, new)], got3, talk.answer(got3, -1), "the turn behind a stop sequence", dev)
    assert s.ids == talk.hist


# --------------------------------------------------------------------------------------------- 6. refusals --
def test_refused_calls_leave_the_session_as_it_was(dev):
    lm, cfg_l = _small_llama(dev, 2)[:2]
    prompts, eos = _prompts(cfg_l, dev), _eos(dev, 2)
    _, s = _turn(lm, 0, prompts, eos)
    was = _state(s)
    ids, mask = prompts[1]
    kw = dict(max_new_tokens=N2, eos_token_id=eos, pad_token_id=PAD)
    emb = lm.model.embed_tokens(ids)
    with _Spy("flash_attn_varlen_fwd", "kv_append_rows", "copy2d") as spy:
        with pytest.raises(ValueError, match="dtype torch.float32 of this call does not match the session's"):
            lm.generate(session=s, inputs_embeds=emb.float(), **kw)
        with pytest.raises(ValueError, match="kv_cache='fp8'"):
            lm.generate(session=s, input_ids=ids, kv_cache="fp8", **kw)
        with pytest.raises(ValueError, match="batch 2 of this call does not match the session's"):
            lm.generate(session=s, input_ids=ids[:2].contiguous(), **kw)
        dead = mask.clone()
        dead[1] = 0
        with pytest.raises(ValueError, match=r"sample\(s\) \[1\] have no valid token"):
            lm.generate(session=s, input_ids=ids, attention_mask=dead, **kw)
        with pytest.raises(ValueError, match="attention_mask should be of size"):
            lm.generate(session=s, input_ids=ids, attention_mask=mask[:, :-1], **kw)
        with pytest.raises(ValueError, match="hidden 64 of this call does not match"):
            lm.generate(session=s, inputs_embeds=emb[..., :64].contiguous(), **kw)
        with pytest.raises(ValueError, match="decode_attn_ok"):
            lm.generate(session=s, input_ids=ids, **{**kw, "max_new_tokens": 16000})
        assert all(v == [] for v in spy.calls.values())             # nothing was launched into a cache
    assert _state(s) == was
    lm32 = Mo.LlamaForCausalLM(lm.config).to(dev).float().eval()
    with pytest.raises(ValueError, match=r"return_session=True\): fp32 parameters"):
        lm32.generate(input_ids=prompts[0][0], return_session=True, **kw)
    with pytest.raises(ValueError, match="session_capacity=5 is below"):
        lm.generate(input_ids=prompts[0][0], return_session=True, session_capacity=5, **kw)
    got, _ = _turn(lm, 1, prompts, eos, s)                          # and the session still continues
    assert s.turns == 2 and got.shape[0] == B


# --------------------------------------------------------------------------------------------- 7. MM_LLMs --
def test_mm_llms_follow_up_turn_runs_no_tower_and_equals_the_direct_call(dev):
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    Mo.AUTO_FUSE = True
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    follow = torch.randint(3, cfg["llama"]["vocab_size"], (inp["input_ids"].shape[0], 5),
                           generator=torch.Generator().manual_seed(5)).to(dev)
    seen = []
    real = {n: getattr(model, n) for n in ("encode_image", "encode_audio", "encode_video_long")}
    real_prefix = eng.PrefixAssembleFn

    class Counting:
        @staticmethod
        def apply(*a):
            seen.append("PrefixAssembleFn")
            return real_prefix.apply(*a)

    def counted(n):
        def f(*a, **kw):
            seen.append(n)
            return real[n](*a, **kw)
        return f
    for n in real:
        setattr(model, n, counted(n))
    eng.PrefixAssembleFn = Counting
    try:
        with torch.no_grad():
            plain = model(inputs=inp)
            assert torch.is_tensor(plain) and sorted(set(seen)) == sorted([*real, "PrefixAssembleFn"])
            Mo.MM_LLMs.set_session(True)
            sessions = []
            for _ in range(2):
                out, s = model(inputs=inp)
                assert torch.equal(out, plain) and isinstance(s, Mo.GenerateSession) and s.turns == 1
                sessions.append(s)
            del seen[:]
            with _Spy("flash_attn_varlen_fwd", "kv_append_rows", "decode_step_attn_var") as spy:
                got, s_back = model(inputs=dict(input_ids=follow, session=sessions[0], inference=True))
                assert len(spy.calls["kv_append_rows"]) == cfg["llama"]["num_hidden_layers"]
                assert len(spy.calls["decode_step_attn_var"]) > 0
            assert seen == [] and s_back is sessions[0] and s_back.turns == 2
            E = model.llm.model.embed_tokens.weight
            direct, _ = model.llm.generate(session=sessions[1], return_session=True, max_new_tokens=128, eos_token_id=2,
                                           bos_token_id=1, pad_token_id=32006,
                                           inputs_embeds=ops.embedding_fwd(E, follow.reshape(-1)).view(*follow.shape, -1))
            assert torch.equal(got, direct), (got.tolist(), direct.tolist())
            assert sessions[0].lengths == sessions[1].lengths
            with pytest.raises(ValueError, match="images next to inputs\\['session'\\]"):
                model(inputs=dict(input_ids=follow, session=sessions[0], inference=True, images=inp["images"]))
            assert sessions[0].turns == 2
    finally:
        eng.PrefixAssembleFn = real_prefix
        for n in real:
            delattr(model, n)
