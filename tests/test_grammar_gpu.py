"""GPU: grammar-constrained decoding -- ops.grammar_build, ops.grammar_mask and ops.grammar_advance (csrc/grammar.hip)
against the restatement of tests/grammar_ref.py exactly (integers and the -inf bit pattern only), a table whose row
offset passes 2^31 elements, and generate(grammar=) end to end on every decode path.  Every end-to-end test asserts that
its constraint fired: the plain ids violate the grammar."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grammar_ref as R  # noqa: E402
from test_decode_kv8_gpu import _Spy, _ids, _small_llama  # noqa: E402
from test_stopping_gpu import _bits, _logits, _path_kw  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.grammar import TokenDFA  # noqa: E402

INF = float("inf")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
JSON = r'\{"name": "[a-z ]{1,12}", "n": (0|[1-9]\d?)\}'
NUMBER = r'-?(0|[1-9]\d{0,5})(\.\d{1,3})?'
ALPHABET = b'{}":, name0123456789abcxyz.-'


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.MM_LLMs.set_grammar()
    ops.clear_fp8_cache()


# ---------------------------------------------------------------------------- 1. mk_grammar_build vs the restatement --
def _vocab(V, seed):
    """the synthetic vocabulary with tokens of 0, 1, 2, 15, 16, 17, 64 and 300 bytes among its pieces (and None entries)"""
    vocab = R.synthetic_vocab(V, seed, alphabet=ALPHABET)
    rng = np.random.default_rng(seed + 1)
    letters = np.frombuffer(b"abc xyz", dtype=np.uint8)
    for k, n in enumerate((0, 1, 2, 15, 16, 17, 64, 300)):
        for j, alpha in enumerate((letters, np.frombuffer(ALPHABET, dtype=np.uint8))):
            vocab[300 + 2 * k + j] = bytes(rng.choice(alpha, size=n).tolist())
    vocab[V - 1] = bytes(rng.choice(letters, size=300).tolist())         # the last token is a long one
    return vocab


def _random_char_next(S, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, S, size=(S, 256)).astype(np.int32)
    t[rng.random((S, 256)) < 0.05] = -1
    return t


_TABLES = {}


def _build_case(name):
    """(char_next, vocab, the restated table), computed once per case and left unchanged"""
    if name not in _TABLES:
        S, V = {"S1": (1, 1000), "S35": (35, 1000), "S1000": (1000, 1000), "S35-V32007": (35, 32007)}[name]
        vocab = _vocab(V, seed=S)
        if S == 35:
            cn = TokenDFA.from_regex(JSON, vocab).char_next
            assert cn.shape == (35, 256)
        elif S == 1:
            cn = np.where(np.arange(256) % 3 == 0, -1, 0).astype(np.int32).reshape(1, 256)
            cn[0, list(b"abc xyz")] = 0
        else:
            cn = _random_char_next(S, seed=5)
        _TABLES[name] = (cn, vocab, R.token_table(cn, vocab))
    return _TABLES[name]


@pytest.mark.parametrize("case", ["S1", "S35", "S1000", "S35-V32007"])
def test_grammar_build_is_the_restated_byte_walk_exactly(dev, case):
    cn, vocab, want = _build_case(case)
    S, V = want.shape
    lens = np.array([0 if t is None else len(t) for t in vocab])
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    data = torch.from_numpy(np.frombuffer(b"".join(t for t in vocab if t), dtype=np.uint8).copy())
    assert {0, 1, 2, 15, 16, 17, 64, 300} <= set(lens.tolist())
    got = ops.grammar_build(torch.from_numpy(cn), data, off, dev)
    assert got.shape == (S, V) and got.dtype == torch.int32 and got.stride(0) % 4 == 0 and got.stride(0) >= V
    assert np.array_equal(got.cpu().numpy(), want)
    assert int((want >= 0).sum()) > 0
    if S != 35:                                  # (a record's name holds 12 letters at the most)
        assert int((want[:, lens >= 64] >= 0).sum()) > 0                 # long tokens survive somewhere
    assert bool((want[:, lens == 0] == -1).all())
    # any pitch, device inputs, and the padding [V, ld) keeps its -1
    got = ops.grammar_build(torch.from_numpy(cn).to(dev), data.to(dev), off.to(dev), ld_next=V + 3)
    assert got.stride(0) == V + 3 and np.array_equal(got.cpu().numpy(), want)
    full = got.as_strided((S, V + 3), (V + 3, 1))
    assert bool((full[:, V:] == -1).all())
    if case == "S35":                            # TokenDFA.table: this table, trimmed on the device, with its flags
        g = TokenDFA.from_regex(JSON, vocab)
        tab, start = g.table(dev)
        acc = [g.is_accepting(s) for s in range(S)]
        trimmed, flags = R.trim(want, acc)
        assert start == 0 and np.array_equal(tab.next.cpu().numpy(), trimmed) and tab.flags.tolist() == flags.tolist()
        assert g.table(dev)[0] is tab
        assert [g.allowed(s) for s in range(S)] == [np.nonzero(trimmed[s] >= 0)[0].tolist() for s in range(S)]


def test_the_token_trim_removes_what_the_vocabulary_cannot_finish(dev):
    """'ab|cd' over a vocabulary without any 'd': the byte automaton lets 'c' through, the token table must not"""
    vocab = [None, b"a", b"b", b"c", b"ab", b"x"]
    g = TokenDFA.from_regex("ab|cd", vocab)
    tab, start = g.table(dev)
    raw = R.token_table(g.char_next, vocab)
    want, flags = R.trim(raw, [g.is_accepting(s) for s in range(g.n_states)])
    assert raw[0, 3] >= 0 and want[0, 3] == -1                           # 'c' went
    assert np.array_equal(tab.next.cpu().numpy(), want) and tab.flags.tolist() == flags.tolist()
    assert g.allowed(start) == [1, 4]
    with pytest.raises(ValueError, match="cannot spell the grammar"):
        TokenDFA.from_regex("cd", vocab).table(dev)


# ------------------------------------------------------------------------------ 2. mk_grammar_mask bit for bit --
def _mask_table(V, n_states, seed):
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, n_states, size=(n_states, V)).astype(np.int32)
    nxt[rng.random((n_states, V)) < 0.5] = -1
    nxt[1] = -1                                                          # a state that allows nothing
    nxt[2] = 0                                                           # one that allows everything
    flags = rng.integers(0, 2, size=n_states).astype(np.uint8)
    flags[0], flags[1], flags[2] = 0, 3, 1                              # not accepting; terminal; accepting
    return nxt, flags


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("V,rows,ld", [(40, 1, 40), (1000, 3, 1024), (32007, 33, 32064)])
def test_grammar_mask_is_the_restatement_bit_for_bit(dev, V, rows, ld, dtype):
    """rows that hold live states (accepting or not, one that allows nothing, one that allows everything), -1, -2, an
    index >= n_states and set done bytes; eos inside [0, V) -- once on a column the table allows, once on one it bans --,
    outside and absent; the table at pitch V (four 4-byte loads where V is odd), at a multiple of 4 (16-byte loads) and at
    that pitch one element behind an aligned address (4-byte loads again).
    The whole [rows, ld] image is compared by bit pattern: banned columns are -inf, allowed columns, +-0, +-inf, NaN and the
    pad columns keep their bits"""
    n_states = 7
    nxt, flags = _mask_table(V, n_states, seed=V)
    x0 = _logits(V, rows, ld, dtype, seed=V + rows)
    neg_inf = _bits(torch.tensor([-INF]).to(dtype)).item()
    ref = R.mask if V == 40 else R.mask_fast
    fired = 0
    eos_in_allowed, eos_in_banned = int(np.nonzero(nxt[0] >= 0)[0][0]), int(np.nonzero(nxt[0] < 0)[0][-1])
    # (pitch, elements the table lies behind its allocation's start): a pitch that is a multiple of 4 on a base that is not
    # 16-byte aligned must take the 4-byte loads too
    for ld_next, shift in ((V, 0), ((V + 3) // 4 * 4 + 4, 0), ((V + 3) // 4 * 4 + 4, 1)):
        flat = torch.full((n_states * ld_next + shift,), 12345, dtype=torch.int32)       # (the row padding is never used)
        flat[shift:].view(n_states, ld_next)[:, :V] = torch.from_numpy(nxt)
        view = flat.to(dev)[shift:].view(n_states, ld_next)[:, :V]
        tab = ops.GrammarTable(view, torch.from_numpy(flags).to(dev))
        assert tab.ld == ld_next and view.data_ptr() % 16 == 4 * shift
        for k, eos in enumerate((eos_in_allowed, eos_in_banned, V - 1, V + 5, None, -1)):
            cycle = [0, 2, 1, -1, 3, -2, n_states, 4, 5, 6, n_states + 10 ** 6]
            state = [cycle[(b + k) % len(cycle)] for b in range(rows)] if rows > 1 else [cycle[k % 3]]
            done = [1 if (b + k) % 5 == 4 else 0 for b in range(rows)]
            st_d = torch.tensor(state, dtype=torch.int32, device=dev)
            dn_d = torch.tensor(done, dtype=torch.uint8, device=dev)
            x = x0.to(dev)
            assert ops.grammar_mask(x[:, :V], V, tab, st_d, dn_d, eos) is not None
            want = x0.clone()
            want[:, :V] = ref(x0[:, :V], V, nxt, flags, state, done, None if eos in (None, -1) else eos)
            assert torch.equal(_bits(x.cpu()), _bits(want)), (ld_next, eos)
            xb = x0.to(dev)                                              # the loops' own flags are bool
            ops.grammar_mask(xb[:, :V], V, tab, st_d, dn_d.bool(), eos)
            assert torch.equal(_bits(xb), _bits(x))
            changed = _bits(want) != _bits(x0)
            assert bool((_bits(want)[changed] == neg_inf).all()) and not bool(changed[:, V:].any())
            assert st_d.tolist() == state and dn_d.tolist() == done      # both are only read
            fired += int(changed.sum())
        assert torch.equal(tab.next.cpu(), torch.from_numpy(nxt))
    assert fired >= V // 4, fired
    with pytest.raises(ops.MacawHipError, match="columns"):
        ops.grammar_mask(x0.to(dev)[:, :V - 1], V - 1, tab, st_d, dn_d)


# ------------------------------------------------------------------------------- 3. mk_grammar_advance exactly --
@pytest.mark.parametrize("B", [1, 3, 33, 300])
def test_grammar_advance_is_the_restatement_and_writes_no_other_byte(dev, B):
    """a transition, a terminal hit (done, end), a token the table bans and one outside [0, V) (broken: -2), rows that
    are done, unconstrained (-1) or broken already; n through n_add and through a device counter, n = 0 and the clamp at
    n_max; the bytes in front of and behind state, done and end keep their values, the ids and the table are only read"""
    V, n_states, n_max = 50, 6, 12
    rng = np.random.default_rng(B)
    nxt = rng.integers(0, n_states, size=(n_states, V)).astype(np.int32)
    nxt[rng.random((n_states, V)) < 0.4] = -1
    nxt[5] = -1
    flags = np.array([0, 1, 0, 1, 0, 3], dtype=np.uint8)                 # state 5 is terminal
    pool = np.array(list(range(V)) + [V, V + 7, 10 ** 12, -1, -5], dtype=np.int64)
    out = pool[rng.integers(0, len(pool), size=(B, n_max))]
    out[:, 0] = pool[rng.integers(0, V, size=B)]
    tab = ops.GrammarTable(torch.from_numpy(nxt).to(dev), torch.from_numpy(flags).to(dev))
    out_d = torch.from_numpy(out).to(dev)
    seen = set()
    for si, (n_add, n) in enumerate([(1, 1), (2, 2), (12, 12), (0, 0), (1000, 12), (-4, 0), (5, 5)]):
        state = [[0, 1, 2, 3, 4, -1, -2, 0, 2][(b + si) % 9] for b in range(B)]
        done = [1 if (b + si) % 4 == 3 else 0 for b in range(B)]
        end = [-1 if (b % 3) else 77 for b in range(B)]
        want = R.advance(out.tolist(), n_add, V, nxt, flags, state, done, end)
        for via_dev in (False, True):
            st = torch.full((B + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            en = torch.full((B + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            dn = torch.full((B + 16,), 0xAB, dtype=torch.uint8, device=dev)
            st[4:4 + B] = torch.tensor(state, dtype=torch.int32, device=dev)
            en[4:4 + B] = torch.tensor(end, dtype=torch.int32, device=dev)
            dn[8:8 + B] = torch.tensor(done, dtype=torch.uint8, device=dev)
            if via_dev:
                n_dev = torch.tensor([n_add - 2, 9], dtype=torch.int32, device=dev)
                ops.grammar_advance(out_d, tab, st[4:4 + B], dn[8:8 + B], en[4:4 + B], n_dev, 2)
                assert n_dev.tolist() == [n_add - 2, 9]
            else:
                ops.grammar_advance(out_d, tab, st[4:4 + B], dn[8:8 + B], en[4:4 + B], None, n_add)
            got = (st[4:4 + B].tolist(), dn[8:8 + B].tolist(), en[4:4 + B].tolist())
            assert got == want, (si, via_dev)
            assert st[:4].tolist() == st[4 + B:].tolist() == en[:4].tolist() == en[4 + B:].tolist() == [0x5A5A5A5A] * 4
            assert dn[:8].tolist() == dn[8 + B:].tolist() == [0xAB] * 8
        for b in range(B):
            if not done[b] and state[b] >= 0:
                s2 = want[0][b]
                seen.add("broken" if s2 == -2 else "terminal" if flags[s2] & 2 else "moved")
                assert want[2][b] == (n if s2 == -2 or flags[s2] & 2 else end[b])
            else:
                assert (want[0][b], want[1][b], want[2][b]) == (state[b], done[b], end[b])
    if B >= 33:
        assert seen == {"broken", "terminal", "moved"}
    assert torch.equal(out_d.cpu(), torch.from_numpy(out)) and torch.equal(tab.next.cpu(), torch.from_numpy(nxt))
    flags_b = torch.zeros(B, dtype=torch.bool, device=dev)               # the loops' own flags are bool
    st = torch.full((B,), 5, dtype=torch.int32, device=dev)
    en = torch.full((B,), -1, dtype=torch.int32, device=dev)
    ops.grammar_advance(out_d, tab, st, flags_b, en, None, 1)            # state 5 allows nothing: every row breaks
    assert st.tolist() == [-2] * B and flags_b.tolist() == [True] * B and en.tolist() == [1] * B


# ------------------------------------------------------------------------------------ 4. a row offset past 2^31 --
def test_a_table_whose_row_offset_passes_2_to_the_31_elements(dev):
    """67 109 states at V = 32007: state * ld_next = 2 147 927 756 > 2^31 for the last state.  The table is one torch.full;
    only the first and the last row are written"""
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 24 << 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB free on the device; the 8.6 GB table is only made with 24 GiB free")
    V, S = 32007, 67109
    assert (S - 1) * V > 2 ** 31
    nxt = torch.full((S, V), -1, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    rows = {0: rng.integers(0, S, size=V).astype(np.int32), S - 1: rng.integers(0, S, size=V).astype(np.int32)}
    for s, r in rows.items():
        r[rng.random(V) < 0.5] = -1
        nxt[s] = torch.from_numpy(r).to(dev)
    rows[S - 1][77] = S - 2                                              # a transition out of the last row
    nxt[S - 1, 77] = S - 2
    flags = torch.zeros(S, dtype=torch.uint8, device=dev)
    flags[S - 2] = 3
    tab = ops.GrammarTable(nxt, flags)
    x0 = _logits(V, 2, V, torch.float32, seed=1)
    x = x0.to(dev)
    state = torch.tensor([S - 1, 0], dtype=torch.int32, device=dev)
    done = torch.zeros(2, dtype=torch.bool, device=dev)
    ops.grammar_mask(x, V, tab, state, done, None)
    want = x0.clone()
    for b, s in enumerate((S - 1, 0)):
        want[b][torch.from_numpy(rows[s] < 0)] = -INF
    assert torch.equal(_bits(x.cpu()), _bits(want))
    out = torch.tensor([[77, 0], [int(np.nonzero(rows[0] >= 0)[0][0]), 0]], device=dev)
    end = torch.full((2,), -1, dtype=torch.int32, device=dev)
    ops.grammar_advance(out, tab, state, done, end, None, 1)
    moved = int(rows[0][int(out[1, 0])])
    assert state.tolist() == [S - 2, moved] and done.tolist() == [True, moved == S - 2]
    assert end.tolist() == [1, 1 if moved == S - 2 else -1]
    del nxt, tab
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------- 5. generate(grammar=) --
N = 24
PATHS = ["graph", "nograph", "nocache", "padded", "kv-fp8", "w-fp8", "sample", "guided", "nocache-fp32"]
OWN_REFERENCE = ("kv-fp8", "w-fp8", "sample")       # no use_cache=False call / ids not comparable between paths


def _model(dev, path):
    return _small_llama(dev, torch.float32 if path.endswith("fp32") else torch.bfloat16)


def _model_vocab(V):
    """a synthetic vocabulary of the model's size: three specials, the digits, '-', '.', pieces of several bytes that a
    number may or may not contain, letters"""
    vocab = [None] * 3 + [bytes([c]) for c in b"0123456789-."]
    vocab += [b"10", b"25", b"00", b".5", b"-1", b"12.", b"3.14", b"999999", b"1e5", b"--", b"..", b"0.", b"-0", b"07"]
    rng = np.random.default_rng(V)
    while len(vocab) < V:
        vocab.append(bytes(rng.choice(np.frombuffer(b"abcdefgh ,", dtype=np.uint8), size=int(rng.integers(1, 5))).tolist()))
    return vocab[:V]


def _answer(row, pad, eos, n_max=None):
    """the ids of a returned row up to its end (eos excluded), and whether the row ended before max_new_tokens (n_max: the
    call's; None: the row's own width)"""
    row = list(row)
    n = len(row)
    while n and row[n - 1] == pad:
        n -= 1
    ended = n < (len(row) if n_max is None else n_max)
    if n and row[n - 1] == eos:
        n, ended = n - 1, True
    return row[:n], ended


@pytest.mark.parametrize("path", PATHS)
def test_a_grammar_that_bans_one_token_is_bad_words_ids_of_that_token(dev, path):
    lm, cfg_l = _model(dev, path)
    V = cfg_l["vocab_size"]
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, **_path_kw(path, cfg_l, ids, dev))
    plain = lm.generate(**kw)
    X = int(plain[0, 3])                                                 # from the plain ids, so that it fires
    g = TokenDFA.from_edges(1, [(0, t, 0) for t in range(V) if t != X], [0], vocab_size=V)
    with _Spy("grammar_mask", "grammar_advance", "seq_ban") as spy:
        got = lm.generate(grammar=g, **kw)
        assert len(spy.calls["grammar_mask"]) == len(spy.calls["grammar_advance"]) > 0 and spy.calls["seq_ban"] == []
    want = lm.generate(bad_words_ids=[[X]], **kw)
    assert got.shape == (3, N) and torch.equal(got, want), (path, got.tolist(), want.tolist())
    assert not bool((got == X).any()) and bool((plain == X).any())


@pytest.mark.parametrize("path", PATHS)
def test_choices_return_exactly_the_choice_and_the_width_of_the_longest(dev, path):
    """every row may only say its own first five plain ids: the terminal state ends it there, and the call returns
    width 5 of max_new_tokens=40"""
    lm, cfg_l = _model(dev, path)
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, eos_token_id=-1, pad_token_id=0, **_path_kw(path, cfg_l, ids, dev))
    plain = lm.generate(max_new_tokens=8, **kw)
    gs = [TokenDFA.from_choices([plain[b, :5].tolist()]) for b in range(3)]
    got = lm.generate(max_new_tokens=40, grammar=gs, **kw)
    assert got.shape == (3, 5) and torch.equal(got, plain[:, :5]), (path, got.tolist())
    # rows of different lengths: pad behind the shorter ones, the width is the longest's; a proper prefix ends only by eos
    gs = [TokenDFA.from_choices([plain[0, :2].tolist()]), TokenDFA.from_choices([plain[1, :6].tolist(), plain[1, :3].tolist()]),
          TokenDFA.from_choices([plain[2, :4].tolist()])]
    got = lm.generate(max_new_tokens=40, grammar=gs, **kw)
    assert got.shape == (3, 6), (path, got.tolist())
    for b, n in enumerate((2, 6, 4)):
        assert got[b, :n].tolist() == plain[b, :n].tolist() and bool((got[b, n:] == 0).all())


@pytest.mark.parametrize("path", PATHS)
def test_a_regex_holds_on_every_path_and_the_cached_paths_give_the_use_cache_false_ids(dev, path):
    """a number pattern on a synthetic vocabulary of the model's size, which the plain ids violate: every returned row
    walks the automaton from its start, and a row that ended before max_new_tokens spells a full match.  The reference of
    the cached 16-bit paths is the use_cache=False call with the same arguments; the e4m3 cache and weights have no such
    call and sampled ids are reproducible per path only (tests/test_stopping_gpu.py documents both)"""
    lm, cfg_l = _model(dev, path)
    V, eos = cfg_l["vocab_size"], 2
    vocab = _model_vocab(V)
    g = TokenDFA.from_regex(NUMBER, vocab)
    rx = re.compile(NUMBER.encode())
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=eos, pad_token_id=0, **_path_kw(path, cfg_l, ids, dev))
    plain = lm.generate(**kw)
    assert not any(g.is_accepting(g.walk(_answer(r, 0, eos)[0])) for r in plain.tolist())      # the model alone says no number
    got = lm.generate(grammar=g, **kw)
    assert got.shape[0] == 3 and got.shape[1] <= 12                      # at most 11 tokens and an eos
    for row in got.tolist():
        answer, ended = _answer(row, 0, eos, N)
        state = g.walk(answer)
        assert state is not None and len(answer) > 0, (path, row)
        assert ended and g.is_accepting(state) and rx.fullmatch(b"".join(vocab[t] for t in answer)), (path, row)
    if path not in OWN_REFERENCE:
        ref = lm.generate(grammar=g, **{**kw, "use_cache": False})
        assert torch.equal(got, ref), (path, got.tolist(), ref.tolist())
    assert torch.equal(got, lm.generate(grammar=g, **kw))                # the grammar object is not used up by a call


@pytest.mark.parametrize("path", ["graph", "nograph", "nocache", "padded", "sample"])
def test_a_none_row_of_a_list_is_the_plain_calls_row(dev, path):
    lm, cfg_l = _model(dev, path)
    V = cfg_l["vocab_size"]
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, **_path_kw(path, cfg_l, ids, dev))
    plain = lm.generate(**kw)
    g = TokenDFA.from_regex(NUMBER, _model_vocab(V))
    c = TokenDFA.from_choices([plain[2, :3].tolist()])
    got = lm.generate(grammar=[g, None, c], **kw)                        # two distinct tables back to back, and a free row
    assert got.shape == (3, N) and torch.equal(got[1], plain[1])
    assert g.is_terminal(g.walk(_answer(got[0].tolist(), 0, -1)[0])) and not g.is_accepting(g.walk(_answer(plain[0].tolist(), 0, -1)[0]))
    assert got[2].tolist() == plain[2, :3].tolist() + [0] * (N - 3)


@pytest.mark.parametrize("cache", [True, False])
def test_parallel_samples_repeat_each_prompts_start_state(dev, cache):
    lm, cfg_l = _small_llama(dev)
    V = cfg_l["vocab_size"]
    vocab = _model_vocab(V)
    g, rx = TokenDFA.from_regex(NUMBER, vocab), re.compile(NUMBER.encode())
    c = TokenDFA.from_choices([[5, 6, 7], [8, 9]])
    kw = dict(input_ids=_ids(cfg_l, 2, dev), max_new_tokens=N, eos_token_id=2, pad_token_id=0, do_sample=True, temperature=1.5,
              seed=11, num_samples=3, use_cache=cache)
    got = lm.generate(grammar=[g, c], **kw)
    assert got.shape[0] == 6
    answers = [_answer(r, 0, 2, N) for r in got.tolist()]
    for a, ended in answers[:3]:
        assert ended and rx.fullmatch(b"".join(vocab[t] for t in a)), a
    for a, ended in answers[3:]:
        assert ended and a in ([5, 6, 7], [8, 9]), a
    assert len({tuple(a) for a, _ in answers[:3]}) > 1                   # three samples, not one answer thrice


@pytest.mark.parametrize("path", ["graph", "nograph", "nocache"])
def test_logprobs_are_those_of_the_masked_logits(dev, path):
    """the terminal token keeps its real value and the columns behind it hold 0.0 / pad; a forced token (one allowed
    column) has probability 1"""
    lm, cfg_l = _small_llama(dev)
    V = cfg_l["vocab_size"]
    ids = _ids(cfg_l, 3, dev)
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, return_logprobs=True, top_logprobs=3,
              **_path_kw(path, cfg_l, ids, dev))
    g = TokenDFA.from_regex(NUMBER, _model_vocab(V))
    got = lm.generate(grammar=g, **kw)
    for b, row in enumerate(got.ids.tolist()):
        answer, ended = _answer(row, 0, -1, N)
        e = len(answer) - 1
        assert ended and g.is_terminal(g.walk(answer))                   # without an eos only the terminal state ends a row
        lp = got.logprobs[b]
        assert bool(torch.isfinite(lp).all()) and float(lp[e]) < 0.0     # one of ten digits: a real value
        assert bool((lp[e + 1:] == 0).all()) and bool((got.top_ids[b, e + 1:] == 0).all())
        assert bool((got.top_logprobs[b, e + 1:] == 0).all())
        state = g.start
        for t, tok in enumerate(answer):                                 # renormalised over the allowed set, as in HF
            allowed = g.allowed(state)
            assert int(got.top_ids[b, t, 0]) in allowed
            if len(allowed) == 1:
                assert float(lp[t]) == 0.0
            state = g.walk([tok], state)
    plain = lm.generate(**{**kw, "max_new_tokens": 8})
    two = [TokenDFA.from_choices([plain.ids[b, :4].tolist(), [(int(plain.ids[b, 0]) + 1) % V, 5]]) for b in range(3)]
    got = lm.generate(grammar=two, **{**kw, "max_new_tokens": 40})
    assert got.ids.shape == (3, 4) and torch.equal(got.ids, plain.ids[:, :4])
    assert bool((got.logprobs[:, 0] < 0).all()) and bool((got.logprobs[:, 1:].exp() == 1).all())
    assert bool((got.top_logprobs[:, 1:, 0] == 0).all())


def test_the_graph_path_launches_both_once_per_captured_step_and_the_default_call_none(dev):
    lm, cfg_l = _small_llama(dev)
    V = cfg_l["vocab_size"]
    free = TokenDFA.from_edges(1, [(0, t, 0) for t in range(V)], [0], vocab_size=V)
    kw = dict(input_ids=_ids(cfg_l, 2, dev), eos_token_id=-1, pad_token_id=0)
    with _Spy("grammar_mask", "grammar_advance", "grammar_build") as spy:
        plain = lm.generate(max_new_tokens=24, **kw)
        lm.generate(max_new_tokens=8, decode_graph=False, **kw)
        lm.generate(max_new_tokens=8, use_cache=False, **kw)
        lm.generate(max_new_tokens=8, grammar=None, **kw)
        lm.generate(max_new_tokens=8, grammar=[None, None], **kw)
        assert spy.calls == {"grammar_mask": [], "grammar_advance": [], "grammar_build": []}
        counts = []
        for n in (8, 24):
            got = lm.generate(max_new_tokens=n, grammar=free, **kw)
            counts.append((len(spy.calls["grammar_mask"]), len(spy.calls["grammar_advance"])))
            assert torch.equal(got, plain[:, :n])                        # it allows everything: the plain ids
        # token 0, the eager step, the captured step: three Python-level calls whatever max_new_tokens is
        assert counts == [(3, 3), (6, 6)]
        lm.generate(max_new_tokens=8, grammar=free, decode_graph=False, **kw)
        assert (len(spy.calls["grammar_mask"]), len(spy.calls["grammar_advance"])) == (14, 14)
    for bad, msg in ((dict(num_beams=2), "num_beams=2.*not built"), (dict(prompt_lookup_num_tokens=2), "not built"),
                     (dict(return_session=True), "not built"), (dict(grammar=[free]), "a list of 1 grammars for 2 prompts")):
        with pytest.raises(ValueError, match=msg):
            lm.generate(max_new_tokens=8, **{**dict(grammar=free), **bad}, **kw)
    with pytest.raises(ValueError, match="is not the model's"):
        lm.generate(max_new_tokens=8, grammar=TokenDFA.from_choices([[5]], vocab_size=V + 1), **kw)


def test_the_model_wide_switch_reaches_the_inference_call_and_is_cleared_again(dev):
    from golden_util import load_case
    from oracle import configs
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    model = build_model(configs.get(fx["config_name"]), fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    with torch.no_grad(), _Spy("grammar_mask", "grammar_advance") as spy:
        base = model(inputs=inp)
        assert spy.calls["grammar_mask"] == [] and spy.calls["grammar_advance"] == []
        rows = base.tolist()
        choice = []
        for r in rows:                                                   # the row's first ids, up to 3, in front of its eos
            k = min(3, r.index(2) if 2 in r else 3)
            choice.append(r[:k] if k else None)
        assert any(c for c in choice)
        Mo.MM_LLMs.set_grammar([TokenDFA.from_choices([c]) if c else None for c in choice])
        got = model(inputs=inp)
        assert len(spy.calls["grammar_mask"]) > 0 and len(spy.calls["grammar_advance"]) > 0
        for b, c in enumerate(choice):
            if c:
                assert got[b, :len(c)].tolist() == c and bool((got[b, len(c):] == 32006).all())
            else:
                assert got[b].tolist() == rows[b][:got.shape[1]]
        if all(choice):
            assert got.shape[1] == max(len(c) for c in choice) < base.shape[1]
        Mo.MM_LLMs.set_grammar()
        n = len(spy.calls["grammar_mask"]), len(spy.calls["grammar_advance"])
        assert torch.equal(model(inputs=inp), base) and n == (len(spy.calls["grammar_mask"]), len(spy.calls["grammar_advance"]))
