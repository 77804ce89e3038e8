"""GPU: stop_sequences and bad_words_ids -- ops.seq_ban and ops.stop_match (csrc/stop.hip) against the restatement of
tests/stop_ref.py exactly (integers and the -inf bit pattern only), and generate(stop_sequences=, bad_words_ids=) end to
end.  Stopping changes no logit, so the expected ids under stop_sequences are the plain call's own ids cut by the
restatement, pad behind, on every decode path; the sequences are taken from the plain call's ids, so a match is certain,
and every test asserts that its constraint fired."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import stop_ref as R  # noqa: E402
from test_decode_kv8_gpu import _Spy, _ids, _small_llama  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

INF, NAN = float("inf"), float("nan")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SHAPES = [(40, 1, 40), (1000, 3, 1024), (1000, 33, 1024)]              # V, rows, pitch
PAD_VALUE = 1e4                                                         # what the columns [V, ld) hold
P_MAX, N_MAX, N_GEN = 80, 24, 20


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.MM_LLMs.set_stopping()
    ops.clear_fp8_cache()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _logits(V, rows, ld, dtype, seed):
    """randn * 4 with +0, -0, -inf, +inf and NaN sprinkled in, rounded to dtype; pad columns = 1e4 (CPU [rows, ld])"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 4
    for val in (0.0, -0.0, -INF, INF, NAN):
        x[torch.randint(0, rows, (V // 10,), generator=g), torch.randint(0, V, (V // 10,), generator=g)] = val
    full = torch.full((rows, ld), PAD_VALUE)
    full[:, :V] = x
    return full.to(dtype)


def _pool(V):
    return [1, 2, V - 1, V + 5, 10 ** 12, 0]                            # six values, two of them outside [0, V)


def _id_rows(V, rows, width, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(_pool(V))[torch.randint(0, 6, (rows, width), generator=g)]


def _history(prompt, pl, gen, n, b):
    return ([] if prompt is None else prompt[b, :pl[b]].tolist()) + gen[b, :n].tolist()


def _sequences(V, histories, n_seq, seed):
    """n_seq sequences for these histories.  The crafted ones come first: per history a sequence of 64 ids whose prefix is
    the history's tail (where it is long enough), one that agrees with the tail except in its FIRST id, the tail of 1, 2
    and 3 ids in front of three different columns of which the test below lets only some match, a prefix that holds ids
    >= V, a matching prefix in front of a last id >= V, a duplicate; then single ids; the rest random, 1 to 5 ids from
    the histories' own pool, so that many of them match"""
    g = torch.Generator().manual_seed(seed)
    col = lambda: int(torch.randint(0, V, (1,), generator=g))     # noqa: E731
    seqs = []
    for h in histories:
        if len(h) >= 63:
            seqs.append(h[len(h) - 63:] + [col()])
            seqs.append([h[len(h) - 63] + 1] + h[len(h) - 62:] + [col()])
        for m in (1, 2, 3):
            if len(h) >= m:
                seqs.append(h[len(h) - m:] + [col()])
                seqs.append(h[len(h) - m:] + [V + m])                   # names no column
        if len(h) >= 2:
            seqs.append([h[-2] + 1, h[-1], col()])                      # the wrong length-3 tail next to the right ones
            seqs.append(seqs[-1])
    seqs += [[col()], [V], [10 ** 12]]
    seqs = seqs[:n_seq]
    pool = _pool(V)
    while len(seqs) < n_seq:
        m = int(torch.randint(1, 6, (1,), generator=g))
        seqs.append([pool[int(i)] for i in torch.randint(0, 6, (m - 1,), generator=g)] + [col()])
    return seqs


# ------------------------------------------------------------------------------- 1. mk_seq_ban vs the restatement --
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("V,rows,ld", SHAPES)
def test_seq_ban_is_the_restatement_bit_for_bit(dev, V, rows, ld, dtype):
    """tables of 1 sequence (of 1 id, of 64 ids) and of 1000 (four passes of the 256 threads); histories of 0, 1, 62, 63
    and 100 ids through a ragged per-row prompt count, a call without a prompt, the generated count once through n_add
    and once through a device int32, its clamp at n_max and at 0; ids >= V inside a prefix and as the last id.  The
    whole [rows, ld] image is compared by bit pattern: the banned columns are -inf, every other column and the padding
    keep their bits"""
    x0 = _logits(V, rows, ld, dtype, seed=V + rows)
    prompt, gen = _id_rows(V, rows, P_MAX, seed=V + 1), _id_rows(V, rows, N_MAX, seed=V + 2)
    prompt_d, gen_d = prompt.to(dev), gen.to(dev)
    neg_inf = _bits(torch.tensor([-INF]).to(dtype)).item()
    fired = 0
    # (prompt counts spread over the rows or None = no prompt, n through n_add, n the kernel must arrive at)
    scenarios = [([0, 1, 43, 80, 42], N_GEN, N_GEN), ([80, 0, 37], 0, 0), (None, N_GEN, N_GEN), (None, 1, 1), (None, 0, 0),
                 ([62, 80], 1000, N_MAX), ([5], -3, 0)]
    if rows == 1:
        scenarios = [([p], a, n) for ps, a, n in scenarios[:2] for p in ps] + scenarios[2:]
    for si, (lens, n_add, n) in enumerate(scenarios):
        pl = None if lens is None else [lens[(b + si) % len(lens)] for b in range(rows)]
        hists = [_history(None if pl is None else prompt, pl, gen, n, b) for b in range(rows)]
        p_d = None if pl is None else prompt_d
        l_d = None if pl is None else torch.tensor(pl, dtype=torch.int32, device=dev)
        tables = [_sequences(V, hists, 1000, seed=si), [[7]], [[V + 1]]]
        long = [h for h in hists if len(h) >= 63]
        tables += [[long[0][len(long[0]) - 63:] + [3]]] if long else []
        tables += [[hists[0][-1:] + [5]]] if hists[0] else []
        for seqs in tables:
            tab = ops.SeqTable(seqs, dev)
            want = x0.clone()
            want[:, :V] = R.ban(x0[:, :V], None, hists, seqs)
            xa = x0.to(dev)
            ops.seq_ban(xa[:, :V], V, gen_d, tab, None, n_add, p_d, l_d)
            xb = x0.to(dev)
            n_dev = torch.tensor([n_add - 3, 77], dtype=torch.int32, device=dev)       # n = *n_dev + n_add
            ops.seq_ban(xb[:, :V], V, gen_d, tab, n_dev, 3, p_d, l_d)
            assert torch.equal(_bits(xa.cpu()), _bits(want)), (si, len(seqs))
            assert torch.equal(_bits(xb), _bits(xa)), (si, len(seqs))
            assert n_dev.tolist() == [n_add - 3, 77]                    # the counter is only read
            changed = _bits(want) != _bits(x0)
            assert bool((_bits(want)[changed] == neg_inf).all())        # -inf by bit pattern, nothing else
            fired += int(changed.sum())
    assert fired >= 10 * rows, fired


def test_seq_ban_several_lengths_of_which_one_matches_and_out_of_range_ids(dev):
    V = 64
    x0 = _logits(V, 2, V, torch.float32, seed=5)
    gen = torch.tensor([[3, 70, 9, 4, 0, 0], [9, 4, 10 ** 12, 4, 0, 0]], device=dev)
    #       no tail   row 0's 2   row 0's 3       wrong 3        row 1's 2, an id >= V    last ids >= V: no column
    seqs = [[5, 11], [9, 4, 12], [70, 9, 4, 13], [3, 9, 4, 14], [10 ** 12, 4, 15], [4, 64], [9, 4, 10 ** 12]]
    tab = ops.SeqTable(seqs, dev)
    x = x0.to(dev)
    ops.seq_ban(x, V, gen, tab, None, 4)
    want = R.ban(x0, None, [gen[b, :4].tolist() for b in range(2)], seqs)
    assert torch.equal(_bits(x.cpu()), _bits(want))
    banned = [[c for c in range(V) if want[b, c] == -INF and not x0[b, c] == -INF] for b in range(2)]
    assert set(banned[0]) <= {12, 13} and set(banned[1]) <= {15}
    assert want[0, 12] == want[0, 13] == want[1, 15] == -INF
    for b, keep in ((0, (11, 14, 15)), (1, (11, 12, 13, 14))):
        assert torch.equal(_bits(want[b, list(keep)]), _bits(x0[b, list(keep)]))


# ---------------------------------------------------------------------------- 2. mk_stop_match vs the restatement --
@pytest.mark.parametrize("B", [1, 3, 33])
def test_stop_match_is_the_restatement_and_writes_no_other_byte(dev, B):
    """rows of 70 columns; tables of 1 sequence (1 id, 64 ids) and of 1000; the count through n_add and through a device
    int32, clamped at n_max and at 0; n < m, a match of the whole row (column 0), a sequence that occurs earlier but not
    at the tail; rows that are finished keep their byte (7: not a value the kernel writes), the bytes in front of and
    behind the B flags keep theirs"""
    V, n_max = 1000, 70
    out = _id_rows(V, B, n_max, seed=B)
    out_d = out.to(dev)
    fired = 0
    for si, (n_add, n) in enumerate([(70, 70), (64, 64), (63, 63), (5, 5), (1, 1), (0, 0), (1000, 70), (-4, 0)]):
        rows = [out[b, :n].tolist() for b in range(B)]
        crafted = [r[:] for r in rows if 1 <= len(r) <= 64]                            # the whole row: a match at column 0
        crafted += [r[len(r) - 64:] for r in rows if len(r) >= 64]                     # 64 ids at the tail
        crafted += [r[len(r) - 65:len(r) - 1] for r in rows if len(r) >= 65]           # 64 ids one column early
        crafted += [[r[-3] + 1] + r[-2:] for r in rows if len(r) >= 3]                 # the tail but for its first id
        crafted += [r[:2] for r in rows if len(r) >= 3] + [[5], [V + 5]]
        tables = [_sequences(V, rows, 1000, seed=si)[:1000 - len(crafted[:300])] + crafted[:300], [[V + 5]], [[3]]]
        tables += [[r[len(r) - 64:]] for r in rows[:1] if len(r) >= 64]
        tables += [[out[0, :n + 1].tolist()]] if n < 64 else []                        # n < m
        for seqs in tables:
            tab = ops.SeqTable(seqs, dev)
            before = [7 if (b + si) % 4 == 1 else 0 for b in range(B)]
            want = [7 if d else int(hit) for d, hit in zip(before, R.stop_match(rows, n, seqs, [False] * B))]
            for via_dev in (False, True):
                flags = torch.full((B + 16,), 0xAB, dtype=torch.uint8, device=dev)
                flags[8:8 + B] = torch.tensor(before, dtype=torch.uint8, device=dev)
                if via_dev:
                    n_dev = torch.tensor([n_add - 2, 9], dtype=torch.int32, device=dev)
                    ops.stop_match(out_d, tab, flags[8:8 + B], n_dev, 2)
                    assert n_dev.tolist() == [n_add - 2, 9]
                else:
                    ops.stop_match(out_d, tab, flags[8:8 + B], None, n_add)
                assert flags[8:8 + B].tolist() == want, (si, len(seqs), via_dev)
                assert flags[:8].tolist() == [0xAB] * 8 and flags[8 + B:].tolist() == [0xAB] * 8
            assert R.stop_match(rows, n, seqs, [bool(d) for d in before]) == [bool(w) for w in want]
            fired += sum(w == 1 for w in want)
    assert fired >= 5
    assert torch.equal(out_d.cpu(), out)                                 # the ids are only read
    flags = torch.zeros(B, dtype=torch.bool, device=dev)                 # the loops' own flags are bool
    ops.stop_match(out_d, ops.SeqTable([out[0, 2:5].tolist()], dev), flags, None, 5)
    assert flags.tolist() == R.stop_match(out.tolist(), 5, [out[0, 2:5].tolist()], [False] * B) and flags[0]


# -------------------------------------------------------------------------------------- 3. generate(): stopping --
N = 24
PATHS = {"graph": dict(), "nograph": dict(decode_graph=False), "nocache": dict(use_cache=False), "kv-fp8": dict(kv_cache="fp8"),
         "w-fp8": dict(decode_weights="fp8"), "sample": dict(do_sample=True, temperature=0.9, top_k=20, seed=5),
         "padded": "mask", "guided": "neg", "nocache-fp32": dict(use_cache=False), "cached-fp32": dict()}


def _path_kw(path, cfg_l, ids, dev):
    if path == "padded":
        mask = torch.ones_like(ids)
        for b in range(ids.shape[0]):
            mask[b, :2 + 3 * b] = 0
        return dict(attention_mask=mask)
    if path == "guided":
        neg = torch.randint(3, cfg_l["vocab_size"], (ids.shape[0], 9), generator=torch.Generator().manual_seed(77)).to(dev)
        return dict(negative_prompt_ids=neg, guidance_scale=1.5)
    return dict(PATHS[path])


def _choose(plain, pad):
    """a stop sequence of 2 ids and an eos from the plain ids [3, N] such that, by the restatement, one row stops on the
    sequence, one on eos and one on neither -> (seqs, eos, ends) or None"""
    rows = plain.tolist()
    for a, b, c in itertools.permutations(range(3)):
        for j in range(1, N - 2):
            for k in range(1, N - 1):
                seqs, eos = [rows[a][j:j + 2]], rows[b][k]
                ends = [R.finish_column(r, seqs, eos) for r in rows]
                if (ends[a] == j + 1 and eos not in rows[a][:j + 2] and ends[b] == k
                        and not R.stops_row(rows[b][:k + 1], seqs) and ends[c] is None):
                    return seqs, eos, ends
    return None


@pytest.mark.parametrize("path", list(PATHS))
def test_generate_stops_where_the_restatement_cuts_the_plain_ids(dev, path):
    """one sample stops on a sequence, one on eos, one on neither; the ids are the plain ids of the same path, cut"""
    lm, cfg_l = _small_llama(dev, torch.float32 if path.endswith("fp32") else torch.bfloat16)
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, max_new_tokens=N, pad_token_id=0, **_path_kw(path, cfg_l, ids, dev))
    plain = lm.generate(eos_token_id=-1, **kw)
    assert plain.shape == (3, N)
    chosen = _choose(plain.cpu(), 0)
    assert chosen is not None, plain.tolist()
    seqs, eos, ends = chosen
    want = R.cut(plain.cpu(), seqs, eos, 0)
    assert want.shape == (3, N) and sorted(e is None for e in ends) == [False, False, True]
    with _Spy("stop_match", "seq_ban") as spy:
        got = lm.generate(eos_token_id=eos, stop_sequences=seqs + [[10 ** 9, 5]], **kw)
        assert len(spy.calls["stop_match"]) > 0 and spy.calls["seq_ban"] == []
    assert torch.equal(got.cpu(), want), (path, got.tolist(), want.tolist())
    assert not torch.equal(want, plain.cpu())                            # the constraints fired
    for b, e in enumerate(ends):
        if e is not None:
            assert bool((got[b, e + 1:] == 0).all()) and int(got[b, e]) == int(plain[b, e])


@pytest.mark.parametrize("path", ["graph", "nograph", "nocache", "padded", "kv-fp8", "sample", "guided", "nocache-fp32"])
def test_all_samples_stopping_at_column_2_of_40_return_width_3(dev, path):
    lm, cfg_l = _small_llama(dev, torch.float32 if path.endswith("fp32") else torch.bfloat16)
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, eos_token_id=-1, pad_token_id=0, **_path_kw(path, cfg_l, ids, dev))
    plain = lm.generate(max_new_tokens=8, **kw)
    seqs = [plain[b, :3].tolist() for b in range(3)]                     # m == n == 3: each row's own first three ids
    assert all(R.finish_column(plain[b].tolist(), seqs, -1) == 2 for b in range(3))
    got = lm.generate(max_new_tokens=40, stop_sequences=seqs, **kw)
    assert got.shape == (3, 3) and torch.equal(got, plain[:, :3])


@pytest.mark.parametrize("path", ["graph", "nograph", "nocache"])
def test_the_stop_token_keeps_its_logprob_and_the_columns_behind_it_hold_zero(dev, path):
    lm, cfg_l = _small_llama(dev)
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, max_new_tokens=N, pad_token_id=0, return_logprobs=True, top_logprobs=3, **PATHS[path])
    plain = lm.generate(eos_token_id=-1, **kw)
    seqs, eos, ends = _choose(plain.ids.cpu(), 0)
    got = lm.generate(eos_token_id=eos, stop_sequences=seqs, **kw)
    assert torch.equal(got.ids.cpu(), R.cut(plain.ids.cpu(), seqs, eos, 0))
    for b, e in enumerate(ends):
        e = N - 1 if e is None else e
        assert torch.equal(got.logprobs[b, :e + 1], plain.logprobs[b, :e + 1]) and bool((got.logprobs[b, :e + 1] < 0).all())
        assert torch.equal(got.top_ids[b, :e + 1], plain.top_ids[b, :e + 1])
        assert bool((got.logprobs[b, e + 1:] == 0).all()) and bool((got.top_ids[b, e + 1:] == 0).all())
        assert bool((got.top_logprobs[b, e + 1:] == 0).all())
    assert sum(e is not None for e in ends) == 2


# ------------------------------------------------------------------------------------- 4. generate(): banned words --
def _holds(row, q):
    return any(row[i:i + len(q)] == q for i in range(len(row) - len(q) + 1))


BAN_PATHS = ["graph", "nograph", "padded", "guided", "sample", "kv-fp8", "w-fp8", "cached-fp32"]


@pytest.mark.parametrize("path", BAN_PATHS)
def test_generate_never_emits_a_banned_sequence_and_the_cached_paths_give_the_use_cache_false_ids(dev, path):
    """the bans are cut from the plain ids: two ids from the middle of row 0, row 1's first id alone, and row 2's last
    prompt id with its first new id (a tail that straddles prompt and generated tokens).  Every one occurs in the plain
    output and none in the constrained one.  The reference of the cached paths is the use_cache=False call with the same
    arguments.  Three paths keep the property alone: the e4m3 cache and weights have no such call (use_cache=False refuses
    them), and sampled ids are reproducible on every path by itself but not between paths, whose logits differ in their
    last bits (generate's docstring; tests/test_sampling_gpu.py compares each path with itself for the same reason)"""
    fp32 = path.endswith("fp32")
    lm, cfg_l = _small_llama(dev, torch.float32 if fp32 else torch.bfloat16)
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, **_path_kw(path, cfg_l, ids, dev))
    plain = lm.generate(**kw).tolist()
    prompts = ids.tolist()
    if path == "padded":
        prompts = [[c for c, m in zip(p, mk) if m] for p, mk in zip(prompts, kw["attention_mask"].tolist())]
    bans = [plain[0][5:7], [plain[1][0]], [prompts[2][-1], plain[2][0]]]
    full = [p + r for p, r in zip(prompts, plain)]
    assert all(any(_holds(h, q) for h in full) for q in bans)
    with _Spy("seq_ban", "stop_match") as spy:
        got = lm.generate(bad_words_ids=bans + [[10 ** 9, 3]], **kw)
        assert len(spy.calls["seq_ban"]) > 0 and spy.calls["stop_match"] == []
    assert got.shape == (3, N)
    for b in range(3):
        h = prompts[b] + got[b].tolist()
        for q in bans:
            for i in range(len(prompts[b]) - len(q) + 1, len(h) - len(q) + 1):    # every window that ends in a new id
                assert h[i:i + len(q)] != q, (path, b, q, i)
    assert got.tolist() != plain
    if path not in ("kv-fp8", "w-fp8", "sample"):
        ref = lm.generate(bad_words_ids=bans, **{**kw, "use_cache": False})
        assert torch.equal(got, ref), (path, got.tolist(), ref.tolist())
    # a banned [eos] is dropped: the call launches nothing and is the plain call
    with _Spy("seq_ban") as spy:
        same = lm.generate(bad_words_ids=[[int(plain[1][0])]], **{**kw, "eos_token_id": int(plain[1][0])})
        assert spy.calls["seq_ban"] == []
    assert same[1].tolist() == [plain[1][0]] + [0] * (same.shape[1] - 1)


def test_bans_processors_stop_and_logprobs_together_on_generated_history_alone(dev):
    """embeddings alone (MM_LLMs' call): the history is the generated tokens, so a banned pair whose first id is token 0
    shows the L == n - 1 rule; the processors run in front of the ban, the log-probabilities score the banned logits"""
    lm, cfg_l = _small_llama(dev)
    ids = _ids(cfg_l, 3, dev)
    emb = lm.model.embed_tokens(ids)
    kw = dict(inputs_embeds=emb, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, no_repeat_ngram_size=3)
    plain = lm.generate(**kw)
    bans = [plain[0, :2].tolist(), plain[1, 2:5].tolist()]              # L == n - 1 == 1 when token 1 of row 0 is chosen
    stop = [plain[2, 1:3].tolist()]
    e = R.finish_column(plain[2].tolist(), stop, -1)                    # column 2, or 1 where the row opens with one id thrice
    assert e in (1, 2)
    # a ban moves a token only where the plain ids complete it: none does inside row 2's prefix, which therefore stays
    assert not any(_holds(plain[2, :e + 1].tolist(), q) for q in bans)
    for path in (dict(), dict(decode_graph=False), dict(use_cache=False)):
        with _Spy("logits_process", "seq_ban", "stop_match") as spy:
            got = lm.generate(bad_words_ids=bans, stop_sequences=stop, return_logprobs=True, **kw, **path)
            # (the graph path matches every returned column once more behind its loop, for the width)
            assert 0 < len(spy.calls["logits_process"]) == len(spy.calls["seq_ban"]) <= len(spy.calls["stop_match"])
        g = got.ids
        assert g[0, :2].tolist() != bans[0] and int(g[0, 0]) == int(plain[0, 0])
        assert not any(_holds(g[b].tolist(), q) for b in range(3) for q in bans)
        assert g[2, :e + 1].tolist() == plain[2, :e + 1].tolist() and bool((g[2, e + 1:] == 0).all())
        assert bool((got.logprobs[2, e + 1:] == 0).all()) and bool((got.logprobs[2, :e + 1] < 0).all())
        assert bool(torch.isfinite(got.logprobs).all())                  # a banned id is never the emitted one


# ------------------------------------------------------------------------------------------------ 5. defaults --
def test_default_generate_launches_neither_and_the_model_wide_switch_reaches_both(dev):
    lm, cfg_l = _small_llama(dev)
    kw = dict(input_ids=_ids(cfg_l, 2, dev), max_new_tokens=8, eos_token_id=-1, pad_token_id=0)
    with _Spy("seq_ban", "stop_match") as spy:
        a = lm.generate(**kw)
        lm.generate(decode_graph=False, **kw)
        lm.generate(use_cache=False, **kw)
        lm.generate(num_beams=2, **kw)
        lm.generate(stop_sequences=None, bad_words_ids=None, **kw)
        assert spy.calls["seq_ban"] == [] and spy.calls["stop_match"] == []
    assert a.shape == (2, 8)
    for name in ("stop_sequences", "bad_words_ids"):
        with pytest.raises(ValueError, match=f"{name}.*not built"):
            lm.generate(num_beams=2, **{name: [[5]]}, **kw)
    from golden_util import load_case
    from oracle import configs
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    model = build_model(configs.get(fx["config_name"]), fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    with torch.no_grad(), _Spy("seq_ban", "stop_match") as spy:
        base = model(inputs=inp)
        assert spy.calls["seq_ban"] == [] and spy.calls["stop_match"] == []
        rows = base.tolist()
        seqs = [rows[0][1:3]]
        want = R.cut(base.cpu(), seqs, 2, 32006)
        assert want.shape[1] < base.shape[1] or not torch.equal(want, base.cpu())
        Mo.MM_LLMs.set_stopping(stop_sequences=seqs)
        got = model(inputs=inp)
        assert len(spy.calls["stop_match"]) > 0 and spy.calls["seq_ban"] == []
        assert torch.equal(got.cpu(), want)
        Mo.MM_LLMs.set_stopping(bad_words_ids=[rows[0][:2], [2]])        # generated history alone; [eos] is dropped
        banned = model(inputs=inp)
        assert len(spy.calls["seq_ban"]) > 0 and spy.calls["seq_ban"][0][3].ids.tolist() == rows[0][:2]
        assert banned[0, :2].tolist() != rows[0][:2] and int(banned[0, 0]) == rows[0][0]
        Mo.MM_LLMs.set_stopping()
        n = len(spy.calls["seq_ban"]), len(spy.calls["stop_match"])
        assert torch.equal(model(inputs=inp), base) and n == (len(spy.calls["seq_ban"]), len(spy.calls["stop_match"]))
