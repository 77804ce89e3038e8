"""CPU: grammar-constrained decoding -- grammar.TokenDFA's regex compiler against `re` on bytes, the other constructors
and host methods, vocab_bytes, the restated mask (tests/grammar_ref.py) against the installed transformers'
PrefixConstrainedLogitsProcessor, the header, the ctypes prototypes, the exported symbols and their error codes, every
refusal of generate(grammar=), the place of the two launches in every decode loop on the recorders of
tests/test_generate_trace_cpu.py, and that grammar=None reaches none of it."""
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch

import grammar_ref as R
import test_generate_trace_cpu as T

from macaw_llm_amd import grammar as G
from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops
from macaw_llm_amd.grammar import TokenDFA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
NEW = {"mk_grammar_mask": 13, "mk_grammar_advance": 15, "mk_grammar_build": 8}
INF = float("inf")

PATTERNS = [r'(yes|no|maybe)',
            r'-?(0|[1-9]\d{0,5})(\.\d{1,3})?',
            r'\{"name": "[a-z ]{1,12}", "n": (0|[1-9]\d?)\}',
            r'[^"\n]*"',
            r'(ab|a)(bc|c)*',
            r'a{3}',
            r'\w+( \w+){0,3}\.']
JSON = PATTERNS[2]
# the pieces' alphabet: the bytes the patterns speak of, so that pieces of several bytes are allowed somewhere
ALPHABET = b'yesnomaybc0123456789.-{}":, _AZ\n'
VOCAB = R.synthetic_vocab(1000, seed=7, alphabet=ALPHABET)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# --------------------------------------------------------------------------------- 1. the compiler against re --
def _distances(g):
    """tokens still needed to reach an accepting state, per state reachable from the start (by the host methods alone)"""
    succ, order = {}, [g.start]
    for s in order:
        succ[s] = sorted({g.walk([t], s) for t in g.allowed(s)})
        order += [d for d in succ[s] if d not in succ and d not in order]
    dist = {s: 0 for s in order if g.is_accepting(s)}
    changed = True
    while changed:
        changed = False
        for s in order:
            best = min((dist[d] + 1 for d in succ[s] if d in dist), default=None)
            if best is not None and best < dist.get(s, 1 << 30):
                dist[s], changed = best, True
    return order, dist


@pytest.mark.parametrize("pattern", PATTERNS)
def test_from_regex_agrees_with_re_fullmatch_on_bytes(pattern):
    """3000 walks over allowed tokens, each until a terminal state or its own cap (1 to 64 tokens; for three walks in ten 1 to
    3, so that the finite patterns see unfinished answers too); a third of them are steered towards acceptance (a step along a shortest path with probability 1/2), which is what completes the JSON
    record.  The end state is accepting exactly when re.fullmatch accepts the walk's bytes; every accepted string,
    re-tokenised at random cut points, is accepted again; mutated strings, fed byte by byte, are accepted exactly when
    re accepts them; every reachable state can reach acceptance"""
    g = TokenDFA.from_regex(pattern, VOCAB)
    rx = re.compile(pattern.encode())
    rng = random.Random(len(pattern))
    states, dist = _distances(g)
    assert set(states) == set(dist), "a reachable state cannot reach acceptance"
    by_bytes = {}
    for t, tok in enumerate(VOCAB):
        if tok:
            by_bytes.setdefault(tok, t)
    accepted = rejected = retok = 0
    for w in range(3000):
        s, data, steer = g.start, b"", rng.random() < 1 / 3
        cap = rng.randint(1, 3) if rng.random() < 0.3 else rng.randint(1, 64)
        for _ in range(cap):
            al = g.allowed(s)
            if not al:
                assert g.is_terminal(s)
                break
            if steer and rng.random() < 0.5:
                al = [t for t in al if dist[g.walk([t], s)] == dist[s] - 1] or al
            t = rng.choice(al)
            data += VOCAB[t]
            s = g.walk([t], s)
            assert s is not None
        ok = rx.fullmatch(data) is not None
        assert ok == g.is_accepting(s), (pattern, data)
        accepted += ok
        rejected += not ok
        if ok and rng.random() < 0.5:                     # the same bytes, cut at other points
            ids, p = [], 0
            while p < len(data):
                cands = [n for n in range(1, 18) if data[p:p + n] in by_bytes and p + n <= len(data)]
                n = rng.choice(cands)
                ids.append(by_bytes[data[p:p + n]])
                p += n
            assert g.is_accepting(g.walk(ids)), (pattern, data, ids)
            retok += 1
        if data and rng.random() < 0.25:                 # a near miss, byte by byte
            m = bytearray(data)
            k = rng.randrange(len(m))
            if rng.random() < 0.5:
                m[k] = rng.choice(ALPHABET + b"\xc3\xa9")
            else:
                del m[k]
            end = g.walk([by_bytes[bytes([c])] for c in m])
            assert g.is_accepting(end) == (rx.fullmatch(bytes(m)) is not None), (pattern, bytes(m))
    assert accepted > 0 and rejected > 0 and retok > 0, (pattern, accepted, rejected, retok)     # the run saw both


def test_the_json_pattern_has_35_states_and_its_host_rows_are_the_restated_trimmed_table():
    g = TokenDFA.from_regex(JSON, VOCAB)
    assert g.n_states == 35 and g.start == 0 and g.vocab_size == 1000 and g.char_next.shape == (35, 256)
    acc = [g.is_accepting(s) for s in range(35)]
    want, flags = R.trim(R.token_table(g.char_next, VOCAB), acc)
    for s in range(35):
        assert g.allowed(s) == np.nonzero(want[s] >= 0)[0].tolist()
        assert [g.walk([t], s) for t in g.allowed(s)] == want[s][want[s] >= 0].tolist()
        assert g.is_terminal(s) == bool(flags[s] & 2) and g.is_accepting(s) == bool(flags[s] & 1)
    assert sum(acc) == 1 and g.is_terminal(acc.index(True))
    assert all(t >= 3 for s in range(35) for t in g.allowed(s))          # a None token is never allowed


def test_bytes_semantics_dot_negated_classes_and_utf8_literals():
    vocab = [bytes([i]) for i in range(256)] + ["é".encode(), b"", None]
    ok = lambda p, data: TokenDFA.from_regex(p, vocab).walk(list(data)) is not None and TokenDFA.from_regex(    # noqa: E731
        p, vocab).is_accepting(TokenDFA.from_regex(p, vocab).walk(list(data)))
    for p, data in ((".", b"\n"), (".", b"\xff"), (r"[^a]", b"\xc3"), (r"[^a]", b"a"), (r"\W", b"\xe9"), (r"\w", b"\xe9"),
                    ("é", "é".encode()), ("é+", b"\xc3\xa9\xa9"), ("é+", b"\xc3\xa9\xc3\xa9"), (r"\D\S", b"\x80\x81"),
                    (r"\x41\x80", b"A\x80"), (r"a{2,}", b"a"), (r"a{2,}", b"aaaa"), (r"a{,2}", b""), (r"a{", b"a{"),
                    (r"[]a]+", b"]a"), (r"[a\-z]", b"-"), (r"[\d.]", b"."), (r"(?:ab)*|c", b"abab"), ("", b"")):
        assert ok(p, data) == (re.fullmatch(p.encode(), data) is not None), (p, data)
    g = TokenDFA.from_regex("éa", vocab)
    assert g.walk([256, 0x61]) is not None and g.allowed(g.start) == [0xC3, 256]      # the two-byte token and its first byte
    assert 257 not in g.allowed(g.start) and 258 not in g.allowed(g.start)


@pytest.mark.parametrize("pattern,what", [
    ("^a", "anchor"), ("a$", "anchor"), (r"\bA", "anchor"), (r"a\Z", "anchor"), (r"(a)\1", "back-reference"),
    ("(?=a)b", "look-ahead"), ("(?!a)b", "look-ahead"), ("(?<=a)b", "look-behind"), ("(?<!a)b", "look-behind"),
    ("a*?", "lazy"), ("a+?", "lazy"), ("a??", "lazy"), ("a{2}?", "lazy"), ("a*+", "possessive"), ("a++", "possessive"),
    ("(?i)a", "flag"), ("(?P<n>a)", "named group"), ("[é]", "non-ASCII character inside a class"), ("a**", "multiple repeat"),
    ("*a", "nothing to repeat"), ("(a", "unbalanced"), ("a)", "unbalanced"), ("[a", "unterminated class"),
    (r"\q", "escape"), ("a\\", "trailing backslash"), (r"\xg1", r"\\x escape"), ("[z-a]", "range"), ("a{3,2}", "max < min")])
def test_every_unsupported_construct_raises_a_value_error_that_names_it(pattern, what):
    with pytest.raises(ValueError, match=f"from_regex: .*{what}"):
        TokenDFA.from_regex(pattern, VOCAB)


def test_the_state_cap_and_the_table_size_cap_raise_naming_the_count():
    with pytest.raises(ValueError, match="max_states=10 states"):
        TokenDFA.from_regex(JSON, VOCAB, max_states=10)
    assert TokenDFA.from_regex(JSON, VOCAB, max_states=35).n_states == 35
    with pytest.raises(ValueError, match=rf"35 states x 1000 tokens takes {35 * 1000 * 4} bytes.*max_table_bytes=139999"):
        TokenDFA.from_regex(JSON, VOCAB, max_table_bytes=35 * 1000 * 4 - 1)
    assert TokenDFA.from_regex(JSON, VOCAB, max_table_bytes=35 * 1000 * 4).n_states == 35
    with pytest.raises(ValueError, match="max_table_bytes"):
        TokenDFA.from_edges(3, [(0, 1, 1)], [1], vocab_size=100, max_table_bytes=1199)
    assert G.MAX_STATES == 65536 and G.MAX_TABLE_BYTES == 2 << 30
    sig = inspect.signature(TokenDFA.from_regex).parameters
    assert sig["max_states"].default == 65536 and sig["max_table_bytes"].default == 2 << 30
    for bad in ([], [b"a", "b"], None):
        with pytest.raises((ValueError, TypeError)):
            TokenDFA.from_regex("a", bad)
    with pytest.raises(ValueError, match="matches nothing"):
        TokenDFA.from_regex("[^\\x00-\\xff]", VOCAB)
    with pytest.raises(ValueError, match="cannot spell the grammar"):
        TokenDFA.from_regex("ab", [b"a", b"c", None]).allowed(0)
    with pytest.raises(TypeError):
        TokenDFA()


def test_from_choices_is_a_trie_and_a_proper_prefix_ends_only_by_eos():
    g = TokenDFA.from_choices([[5, 6, 7], [5, 6], [5, 9], [8]])
    assert g.n_states == 6 and g.vocab_size is None
    assert g.allowed(g.start) == [5, 8] and g.walk([4]) is None and g.walk([5, 7]) is None and g.walk([100]) is None
    s56, s567, s59, s8 = g.walk([5, 6]), g.walk([5, 6, 7]), g.walk([5, 9]), g.walk([8])
    assert g.is_accepting(s56) and not g.is_terminal(s56) and g.allowed(s56) == [7]      # [5, 6] ends only by eos
    for s in (s567, s59, s8):
        assert g.is_accepting(s) and g.is_terminal(s) and g.allowed(s) == []
    assert not g.is_accepting(g.walk([5])) and not g.is_accepting(g.start) and not g.is_accepting(None)
    assert g.walk([7], state=s56) == s567
    for bad in ([], [[]], [[1], []], [[-1]], [[1.5]], [[True]]):
        with pytest.raises(ValueError, match="from_choices"):
            TokenDFA.from_choices(bad)
    with pytest.raises(ValueError, match="outside"):
        TokenDFA.from_choices([[5, 50]], vocab_size=40)


def test_from_edges_walks_trims_and_refuses_what_is_not_an_automaton():
    # 0 -1-> 1 -2-> 2 (accepting, loops on 3); 0 -4-> 3 (a dead end: trimmed); 1 -5-> 4 (accepting, terminal)
    g = TokenDFA.from_edges(5, [(0, 1, 1), (1, 2, 2), (2, 3, 2), (0, 4, 3), (1, 5, 4)], [2, 4], vocab_size=8)
    assert g.n_states == 5 and g.vocab_size == 8 and g.allowed(0) == [1] and g.walk([4]) is None
    assert g.walk([1, 2, 3, 3]) == 2 and g.is_accepting(2) and not g.is_terminal(2) and g.is_terminal(4)
    assert g.allowed(1) == [2, 5] and g.allowed(3) == [] and not g.is_terminal(3)
    g1 = TokenDFA.from_edges(2, [(1, 0, 1)], [1], start=1, vocab_size=3)
    assert g1.start == 1 and g1.walk([0, 0]) == 1
    with pytest.raises(ValueError, match="not deterministic"):
        TokenDFA.from_edges(2, [(0, 1, 1), (0, 1, 0)], [1])
    for kw in (dict(n_states=0, edges=[], accepting=[]), dict(n_states=2, edges=[(0, 1, 2)], accepting=[1]),
               dict(n_states=2, edges=[(0, -1, 1)], accepting=[1]), dict(n_states=2, edges=[(0, 9, 1)], accepting=[1], vocab_size=9),
               dict(n_states=2, edges=[(0, 1, 1)], accepting=[2]), dict(n_states=2, edges=[], accepting=[1], start=2)):
        with pytest.raises(ValueError, match="from_edges"):
            TokenDFA.from_edges(**kw)
    with pytest.raises(ValueError, match="cannot spell the grammar"):
        TokenDFA.from_edges(2, [(0, 1, 1)], [], vocab_size=4).allowed(0)


def test_the_device_table_plumbing_on_cpu_tensors_trims_offsets_and_caches():
    """from_edges / from_choices tables are a torch.full(-1) plus a scatter and the torch trim: they need no kernel"""
    g = TokenDFA.from_edges(5, [(0, 1, 1), (1, 2, 2), (2, 3, 2), (0, 4, 3), (1, 5, 4)], [2, 4], vocab_size=8)
    tab, start = g.table("cpu")
    assert start == 0 and (tab.n_states, tab.V, tab.ld) == (5, 8, 8) and g.table("cpu")[0] is tab
    raw = np.full((5, 8), -1, dtype=np.int32)
    for s, t, d in [(0, 1, 1), (1, 2, 2), (2, 3, 2), (0, 4, 3), (1, 5, 4)]:
        raw[s, t] = d
    want, flags = R.trim(raw, [False, False, True, False, True])
    assert want[0, 4] == -1 and raw[0, 4] == 3                           # the dead end went
    assert np.array_equal(tab.next.numpy(), want) and tab.flags.tolist() == flags.tolist() == [0, 0, 1, 0, 3]
    c = TokenDFA.from_choices([[5, 6]])
    both, starts = G.combine([g, None, c, g], "cpu", 8)
    assert starts == [0, -1, 5, 0] and both.n_states == 8 and both.V == 8 and both.ld % 4 == 0
    assert np.array_equal(both.next[:5].numpy(), want) and both.next[5, 5] == 6 and both.next[6, 6] == 7
    assert both.flags.tolist() == [0, 0, 1, 0, 3, 0, 0, 3]
    assert G.combine([g, c], "cpu", 8)[0] is both                        # the joined table is cached on the grammar that leads it
    assert G.combine([c, g], "cpu", 8)[0] is not both and G.combine([c, g], "cpu", 8)[1] == [0, 3]
    small = TokenDFA.from_edges(5, [(0, 1, 1), (1, 2, 2)], [2], vocab_size=8, max_table_bytes=5 * 8 * 4)
    assert small.table("cpu")[0].n_states == 5                           # alone it fits its cap; joined, 8 states do not
    with pytest.raises(ValueError, match=r"joined device table of 2 grammars, 8 states x 8 tokens, takes 256 bytes.*=160"):
        G.combine([small, c], "cpu", 8)
    with pytest.raises(ValueError, match="outside a vocabulary of 6"):
        c.table("cpu", 6)
    with pytest.raises(L.MacawHipError, match="GrammarTable"):
        ops.GrammarTable(torch.zeros((2, 4), dtype=torch.int64), torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(L.MacawHipError, match="GrammarTable"):
        ops.GrammarTable(torch.zeros((2, 4), dtype=torch.int32), torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(L.MacawHipError, match="shorter than the row pitch"):
        ops.GrammarTable(torch.zeros(15, dtype=torch.int32).as_strided((2, 7), (8, 1)), torch.zeros(2, dtype=torch.uint8))


def test_vocab_bytes_handles_the_space_mark_byte_pieces_and_specials():
    pieces = ["<unk>", "<s>", "</s>", "<0x0A>", "<0xff>", "▁yes", "no", "▁", "é", "<0xZZ>", "▁a▁b"]
    assert G.vocab_bytes(pieces, special_ids=[0, 1, 2]) == [None, None, None, b"\n", b"\xff", b" yes", b"no", b" ",
                                                            "é".encode(), b"<0xZZ>", b" a b"]
    assert G.vocab_bytes(["a"]) == [b"a"]
    assert "▁yes" in G.vocab_bytes.__doc__ and " ?(yes|no)" in G.vocab_bytes.__doc__
    g = TokenDFA.from_regex(" ?(yes|no)", G.vocab_bytes(pieces, [0, 1, 2]))
    assert g.allowed(g.start) == [5, 6, 7] and g.is_terminal(g.walk([5])) and g.is_terminal(g.walk([7, 6]))


# --------------------------------------------------------------------------------------------- 2. the rules --
def test_restated_mask_is_the_installed_prefix_constrained_processor_bit_for_bit():
    """HF's PrefixConstrainedLogitsProcessor with the callback allowed(state) + [eos if accepting], on finite non-zero
    fp32 logits (HF ADDS its mask, which would turn a banned +inf or NaN into NaN and -0 into +0: the header's two
    deliberate differences)"""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    V, eos = 1000, 2
    g = TokenDFA.from_regex(JSON, VOCAB)
    acc = [g.is_accepting(s) for s in range(g.n_states)]
    nxt, flags = R.trim(R.token_table(g.char_next, VOCAB), acc)
    rng = random.Random(3)
    gen = torch.Generator().manual_seed(3)
    states = [0, acc.index(True)] + [rng.randrange(g.n_states) for _ in range(10)]
    x = torch.randn(len(states), V, generator=gen) * 4
    x[x == 0] = 1.0
    for b, s in enumerate(states):
        hf = PrefixConstrainedLogitsProcessor(lambda batch_id, ids, s=s: g.allowed(s) + ([eos] if g.is_accepting(s) else []), 1)
        want = hf(torch.zeros((1, 1), dtype=torch.long), x[b:b + 1].clone())
        got = R.mask(x[b:b + 1], V, nxt, flags, [s], [0], eos)
        assert torch.equal(_bits(got), _bits(want)), s
        assert torch.equal(_bits(R.mask_fast(x[b:b + 1], V, nxt, flags, [s], [0], eos)), _bits(want))
        assert int((got > -INF).sum()) == len(g.allowed(s)) + g.is_accepting(s)


def test_restated_mask_and_advance_by_hand():
    # 0 -1-> 1 -2-> 2 (accepting, terminal); 1 -3-> 1
    nxt = np.array([[-1, 1, -1, -1, 5], [-1, -1, 2, 1, -1], [-1, -1, -1, -1, -1]], dtype=np.int32)
    nxt[0, 4] = 2                                                        # the table allows column 4 = eos in state 0 ...
    flags = [0, 0, 3]
    x = torch.tensor([[1.0, -0.0, INF, float("nan"), 2.0, 1e4]] * 5)
    got = R.mask(x, 5, nxt, flags, state=[0, 1, -1, 3, 2], done=[0, 0, 0, 0, 1], eos=4)
    assert got[0].tolist()[:1] == [-INF] and _bits(got[0, 1:2]).item() == _bits(torch.tensor([-0.0])).item()
    assert got[0, 2] == -INF and got[0, 3] == -INF and got[0, 4] == -INF      # ... and the mask ignores that: not accepting
    assert got[0, 5] == 1e4                                              # the padding keeps its value
    assert got[1, :2].tolist() == [-INF, -INF] and got[1, 2] == INF and got[1, 3] != got[1, 3] and got[1, 4] == -INF
    for b in (2, 3, 4):                                                  # unconstrained, outside the table, done
        assert torch.equal(_bits(got[b]), _bits(x[b]))
    acc = R.mask(x[:1], 5, nxt, flags, [2], [0], eos=4)                  # terminal: eos alone
    assert acc[0, :4].tolist() == [-INF] * 4 and acc[0, 4] == 2.0
    assert R.mask(x[:1], 5, nxt, flags, [2], [0], eos=None)[0, :5].tolist() == [-INF] * 5
    assert R.mask(x[:1], 5, nxt, flags, [2], [0], eos=7)[0, :5].tolist() == [-INF] * 5
    out = [[1, 3, 2, 0], [1, 2, 0, 0], [9, 0, 0, 0], [1, 1, 0, 0], [2, 0, 0, 0], [1, 0, 0, 0]]
    st, dn, en = R.advance(out, 1, 5, nxt, flags, [0, 0, 0, 0, -1, 0], [0, 0, 0, 0, 0, 1], [-1] * 6)
    assert (st, dn, en) == ([1, 1, -2, 1, -1, 0], [0, 0, 1, 0, 0, 1], [-1, -1, 1, -1, -1, -1])
    st, dn, en = R.advance(out, 2, 5, nxt, flags, st, dn, en)
    assert (st, dn, en) == ([1, 2, -2, -2, -1, 0], [0, 1, 1, 1, 0, 1], [-1, 2, 1, 2, -1, -1])
    st, dn, en = R.advance(out, 3, 5, nxt, flags, st, dn, en)
    assert (st, dn, en) == ([2, 2, -2, -2, -1, 0], [1, 1, 1, 1, 0, 1], [3, 2, 1, 2, -1, -1])
    assert R.advance(out[:1], 0, 5, nxt, flags, [0], [0], [-1]) == ([-2], [1], [0])       # n = 0: there is no token
    assert R.advance(out[:1], 99, 5, nxt, flags, [1], [0], [-1]) == ([-2], [1], [4])      # clamped at n_max; token 0 is banned
    live = R.live_states(np.array([[1, -1], [-1, -1], [-1, 0]]), [False, True, False])
    assert live.tolist() == [True, True, True]
    t, f = R.trim(np.array([[1, 2], [-1, -1], [-1, 2]]), [False, True, False])
    assert t.tolist() == [[1, -1], [-1, -1], [-1, -1]] and f.tolist() == [0, 3, 0]


# ------------------------------------------------------------------------------------------------ 3. the ABI --
def test_header_declares_the_three_entry_points_and_states_the_rules():
    src = open(HEADER).read()
    for name, arity in NEW.items():
        m = re.search(rf"^int {name}\((.*?)\);", src, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/macaw_hip.h"
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name]) == arity, name
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION == 11
    flat = re.sub(r"\s*\n \*\s*", " ", src)
    for phrase in ("next int32 [n_states][V] at row pitch ld_next >= V", "bit 0 = accepting, bit 1 = terminal",
                   "token-trimmed", "-1 an unconstrained row, -2 a broken one", "BEHIND mk_logits_process and mk_seq_ban",
                   "the table's own entry in that column is ignored", "PrefixConstrainedLogitsProcessor",
                   "SET to -inf whatever it held", "in front of mk_stop_match", "state[b] = -2, done[b] = 1, end[b] = n",
                   "end int32 [B] starts at -1", "exactly once per step", "computed in 64 bits",
                   "-1 on a dead byte transition or an empty token", "no other byte is written"):
        assert phrase in flat, phrase
    from macaw_llm_amd import build
    assert "grammar.hip" in build.SOURCES
    kernel = open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "grammar.hip")).read()
    assert "asm" not in kernel and "atomic" not in kernel               # plain loads and stores only


def test_the_library_exports_them_and_bad_arguments_return_codes_without_a_launch():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    assert lib.mk_abi_version() == 11
    for name in NEW:                                                    # null pointers: a code, nothing launched
        assert getattr(lib, name)(*[None if t is L._vp else t(0) for t in L.SIGNATURES[name]]) == -1, name
    fake = 4096                                                         # never dereferenced: every call below is refused

    def mask(logits=fake, ld=64, V=64, B=1, next=fake, ld_next=64, n_states=3, flags=fake, state=fake, done=fake, eos=2,
             dtype=L.MK_F32):
        return lib.mk_grammar_mask(logits, ld, V, B, next, ld_next, n_states, flags, state, done, eos, dtype, None)

    for bad in (dict(logits=None), dict(next=None), dict(flags=None), dict(state=None), dict(done=None), dict(B=0),
                dict(B=-1), dict(V=0), dict(ld=63), dict(ld_next=63), dict(n_states=0), dict(n_states=-1)):
        assert mask(**bad) == -1, bad
    for bad in (dict(dtype=L.MK_FP8), dict(dtype=7), dict(B=65536)):
        assert mask(**bad) == -2, bad

    def adv(out=fake, out_ld=8, n_max=8, B=1, V=64, n_dev=None, n_add=0, next=fake, ld_next=64, n_states=3, flags=fake,
            state=fake, done=fake, end=fake):
        return lib.mk_grammar_advance(out, out_ld, n_max, B, V, n_dev, n_add, next, ld_next, n_states, flags, state, done,
                                      end, None)

    for bad in (dict(out=None), dict(next=None), dict(flags=None), dict(state=None), dict(done=None), dict(end=None),
                dict(B=0), dict(V=0), dict(ld_next=63), dict(n_states=0), dict(out_ld=7), dict(n_max=-1)):
        assert adv(**bad) == -1, bad

    def bld(char_next=fake, tok_bytes=fake, tok_off=fake, S=3, V=64, next=fake, ld_next=64):
        return lib.mk_grammar_build(char_next, tok_bytes, tok_off, S, V, next, ld_next, None)

    for bad in (dict(char_next=None), dict(tok_bytes=None), dict(tok_off=None), dict(next=None), dict(S=0), dict(V=0),
                dict(ld_next=63)):
        assert bld(**bad) == -1, bad
    assert bld(S=(1 << 31) - 1, V=(1 << 31) - 1, ld_next=1 << 31) == -2
    assert bld(S=1 << 16, V=1 << 16, ld_next=1 << 16) == -2              # one thread per entry: 2^32 of them is no launch
    with pytest.raises(L.MacawHipError, match="needs a GPU device"):     # host tensors never reach the launch
        ops.grammar_build(torch.zeros((2, 256), dtype=torch.int32), torch.zeros(3, dtype=torch.uint8),
                          torch.tensor([0, 1, 3], dtype=torch.int32))
    with pytest.raises(L.MacawHipError, match="needs a GPU device"):
        TokenDFA.from_regex("ab", [b"a", b"b"]).table("cpu")
    for name, op in (("mk_grammar_mask", ops.grammar_mask), ("mk_grammar_advance", ops.grammar_advance),
                     ("mk_grammar_build", ops.grammar_build)):
        assert name in inspect.getsource(op)
    # offsets that do not ascend from 0 are refused on the host, in front of the upload and the launch
    cn = torch.zeros((2, 256), dtype=torch.int32)
    for off in ([1, 2, 3], [0, 2, 1], [0, 1, 2]):
        with pytest.raises(L.MacawHipError, match="ascend from 0"):
            ops.grammar_build(cn, torch.zeros(3, dtype=torch.uint8), torch.tensor(off, dtype=torch.int32))


# ------------------------------------------------------------------------------ 4. public arguments, refusals --
class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates its arguments before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(**kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(1, 2, 4, dtype=torch.bfloat16), **kw)


def test_generate_and_set_grammar_carry_the_argument_and_refuse_what_is_not_built():
    assert inspect.signature(Mo.LlamaForCausalLM.generate).parameters["grammar"].default is None
    assert inspect.signature(Mo.MM_LLMs.set_grammar).parameters["g"].default is None and Mo.GRAMMAR[0] is None
    g = TokenDFA.from_choices([[5, 6]])
    for bad in ("a+", 5, [g, "a"], [5], (g, 1.0), {"a": 1}):
        with pytest.raises(ValueError, match="generate: grammar must be .*TokenDFA"):
            _generate(grammar=bad)
        with pytest.raises(ValueError, match="set_grammar: grammar must be .*TokenDFA"):
            Mo.MM_LLMs.set_grammar(bad)
    with pytest.raises(ValueError, match="grammar is an empty list"):
        _generate(grammar=[])
    with pytest.raises(ValueError, match=r"grammar=\) with num_beams=2.*not built"):
        _generate(grammar=g, num_beams=2)
    with pytest.raises(ValueError, match=r"grammar=\) with prompt_lookup_num_tokens=4.*not built"):
        _generate(grammar=g, prompt_lookup_num_tokens=4)
    with pytest.raises(ValueError, match=r"grammar=\) with session= / return_session=True.*not built"):
        _generate(grammar=g, return_session=True)
    for ok in (g, [g], [None], [g, None]):
        with pytest.raises(_PastTheChecks):
            _generate(grammar=ok)
    # the existing refusals come first, with their text
    with pytest.raises(ValueError, match="num_beams must be"):
        _generate(grammar="a+", num_beams=0)
    with pytest.raises(ValueError, match="generate: stop_sequences"):
        _generate(grammar="a+", stop_sequences=[])
    with pytest.raises(ValueError, match=r"num_samples=2\) with do_sample=False"):
        _generate(grammar="a+", num_samples=2)
    assert Mo.GRAMMAR[0] is None                                         # a refused set_grammar changes nothing
    doc = " ".join(Mo.LlamaForCausalLM.generate.__doc__.split())
    for phrase in ("grammar=g", "TokenDFA.from_regex", "max_new_tokens can cut an answer short",
                   "never ends by itself", "still one replay per token"):
        assert phrase in doc, phrase
    assert "max_new_tokens can cut an answer short" in " ".join(TokenDFA.__doc__.split())


def test_refusals_that_need_the_batch_and_the_vocabulary_run_before_anything_is_launched(monkeypatch):
    g40, g41 = TokenDFA.from_choices([[5, 6]], vocab_size=T.V), TokenDFA.from_choices([[5, 6]], vocab_size=T.V + 1)
    for gr, msg in (([g40], "a list of 1 grammars for 2 prompts"), ([g40, None, g40], "a list of 3 grammars for 2 prompts"),
                    (g41, "vocabulary size 41 is not the model's \\(40\\)"), ([None, g41], "vocabulary size 41"),
                    (TokenDFA.from_choices([[5, 40]]), "token id 40 of the grammar is outside a vocabulary of 40")):
        for path in (dict(), dict(use_cache=False), dict(decode_graph=False)):
            with monkeypatch.context() as mp:
                tr, res = T.call(mp, dict(N=6, kw=dict(grammar=gr, **path)))
            assert res["raises"] == "ValueError" and re.search(msg, res["message"]), res
            assert [e for e in tr.log if not isinstance(e, str) and e[0] != "host"] == [], tr.log
    with monkeypatch.context() as mp:                                    # with parallel samples the list counts the prompts
        tr, res = T.call(mp, dict(N=6, kw=dict(grammar=[g40] * 6, num_samples=3, **T.SAMPLE)))
    assert res["raises"] == "ValueError" and "a list of 6 grammars for 2 prompts" in res["message"]


def test_set_grammar_reaches_generate_through_forward_only_while_it_is_set():
    seen = []

    class LLM:
        _lora = None

        def generate(self, **kw):
            seen.append(kw)
            return "ids"

    class Fake:
        llm = LLM()

        def _param_dtype(self):
            return torch.bfloat16

        def prepare_inputs_for_generation(self, inputs):
            return "emb", None, None
    g = TokenDFA.from_choices([[5, 6]])
    try:
        assert Mo.MM_LLMs.forward(Fake(), {"inference": True}) == "ids" and "grammar" not in seen[-1]
        Mo.MM_LLMs.set_grammar(g)
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert seen[-1]["grammar"] is g
        Mo.MM_LLMs.set_grammar([g, None])
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert seen[-1]["grammar"] == [g, None]
        Mo.MM_LLMs.set_grammar()
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert "grammar" not in seen[-1] and Mo.GRAMMAR[0] is None
    finally:
        Mo.MM_LLMs.set_grammar()


# ----------------------------------------------------------------------------------------- 5. the launch trace --
def _recorders(tr, mp):
    """recorders for the two launches next to those of tests/test_generate_trace_cpu.py (and of the stop sequences): the
    fake advance is the restatement on the recorded buffers, and like every op that changes device state it is recorded,
    not run, inside a capture"""
    from test_stopping_cpu import _recorders as stop_recorders
    stop_recorders(tr, mp)

    def rec(name, effect):
        sig = inspect.signature(getattr(ops, name))

        def f(*args, **kw):
            a = sig.bind(*args, **kw)
            a.apply_defaults()
            a = dict(a.arguments)
            tr.quiet += 1
            try:
                tr.log.append([name, {k: (v.tolist() if torch.is_tensor(v) and v.numel() <= 8 else v) for k, v in a.items()}])
                return effect(a)
            finally:
                tr.quiet -= 1
        return f

    def adv(a):
        n = (int(a["n_dev"][0]) if a["n_dev"] is not None else 0) + a["n_add"]
        tab = a["table"]
        st, dn, en = R.advance(a["out"].tolist(), n, tab.V, tab.next.numpy(), tab.flags.tolist(), a["state"].tolist(),
                               a["done"].tolist(), a["end"].tolist())
        a["state"].copy_(torch.tensor(st, dtype=torch.int32))
        a["done"].copy_(torch.tensor(dn).to(a["done"].dtype))
        a["end"].copy_(torch.tensor(en, dtype=torch.int32))

    mp.setattr(ops, "grammar_mask", rec("grammar_mask", lambda a: a["logits"]))
    mp.setattr(ops, "grammar_advance", rec("grammar_advance", tr._state(adv)))


def _call(mp, spec, more=None):
    real = T.GenTrace

    def make(mp_, lm, script):
        tr = real(mp_, lm, script)
        _recorders(tr, mp_)
        return tr
    mp.setattr(T, "GenTrace", make)
    spec = dict(spec, kw=dict(spec.get("kw", {}), **(more or {})))
    tr, res = T.call(mp, spec)
    from test_stopping_cpu import _resolve
    _resolve(tr)
    return tr.log, res


_name = lambda e: e if isinstance(e, str) else e[0]       # noqa: E731
SCRIPT = T.Script(None, 2)
PATHS = {"graph": {}, "sample": dict(kw=T.SAMPLE), "left": dict(mask="left"), "kv8": dict(kw=dict(kv_cache="fp8")),
         "nograph": dict(kw=dict(decode_graph=False)), "env": dict(env=True), "fp32": dict(dtype="fp32"),
         "nocache": dict(kw=dict(use_cache=False)), "left-nocache-fp32": dict(kw=dict(use_cache=False), mask="left", dtype="fp32")}
GRAPH = ("graph", "sample", "left", "kv8")


@pytest.mark.parametrize("path", list(PATHS))
def test_every_loop_masks_in_front_of_the_selection_and_advances_once_behind_it(monkeypatch, path):
    """a grammar that never ends (one state, every token allowed) next to processors, a ban, a stop sequence that never
    fires and log-probabilities: the plain call's launches with the new ones between them, mask behind seq_ban and in
    front of the selection, advance behind it and in front of stop_match, the same ids"""
    V = T.V
    free = TokenDFA.from_edges(1, [(0, t, 0) for t in range(V)], [0], vocab_size=V)
    free.table("cpu")                 # made once and cached on the grammar: the call itself then reads nothing on the host
    others = dict(bad_words_ids=[[9]], stop_sequences=[[99, 98]], return_logprobs=True)
    spec = dict(PATHS[path], N=6, finish=None)
    with monkeypatch.context() as mp:
        mp.setattr(Mo, "GenerateLogprobs", lambda ids, lp, ti, tl: (ids, lp))
        plain, res0 = _call(mp, spec, others)
    with monkeypatch.context() as mp:
        mp.setattr(Mo, "GenerateLogprobs", lambda ids, lp, ti, tl: (ids, lp))
        got, res = _call(mp, spec, dict(others, grammar=free))
    new = ("grammar_mask", "grammar_advance")
    assert [e for e in got if _name(e) not in new] == plain and not any(_name(e) in new for e in plain)
    assert res == res0
    picks = [i for i, e in enumerate(got) if _name(e) in ("decode_emit", "decode_emit_sample", "argmax_rows", "sample_rows")]
    assert len(picks) == (3 if path in GRAPH else 6)                    # token 0, the eager step, the captured step
    for k, i in enumerate(picks):
        names = [_name(e) for e in got[i - 2:i + 4]]
        assert names[:3] == ["seq_ban", "grammar_mask", _name(got[i])], names
        if path in GRAPH:
            assert names[3:] == ["grammar_advance", "stop_match", "decode_emit_logprobs"], names
        else:
            assert names[3:] == ["token_logprobs", "grammar_advance", "stop_match"], names
        m, a = got[i - 1][1], got[i + 1 if path in GRAPH else i + 2][1]
        assert m["V"] == V and m["eos"] == T.EOS and m["state"] == [0, 0] and m["done"] == [False, False]
        assert a["state"] == [0, 0] and a["end"] == [-1, -1]
        if path in GRAPH:
            assert (m["n_dev"] if "n_dev" in m else None) is None and a["n_add"] == 0 and a["n_dev"] is not None
        else:
            assert a["n_dev"] is None and a["n_add"] == k + 1
    assert len([e for e in got if _name(e) in new]) == 2 * len(picks)   # the width's re-match does not run the advance
    if path in GRAPH:
        lo, hi = got.index("capture{"), got.index("}")
        assert [_name(e) for e in got[lo + 1:hi]][-6:] == ["seq_ban", "grammar_mask", _name(got[picks[2]]), "grammar_advance",
                                                           "stop_match", "decode_emit_logprobs"]


@pytest.mark.parametrize("path", list(PATHS))
def test_a_terminal_state_ends_a_row_pads_behind_it_and_gives_the_width(monkeypatch, path):
    """row 0 must say its scripted first three tokens, row 1 its first five or (a prefix choice) its first two: row 0 ends
    at column 2 by itself, row 1 goes on to column 4; the width is 5 at max_new_tokens=12, pad behind row 0's end"""
    tok = SCRIPT.tok
    g0 = TokenDFA.from_choices([[tok(c, 0) for c in range(3)]])
    g1 = TokenDFA.from_choices([[tok(c, 1) for c in range(5)], [tok(c, 1) for c in range(2)]], vocab_size=T.V)
    spec = dict(PATHS[path], N=12, finish=None)
    with monkeypatch.context() as mp:
        log, res = _call(mp, spec, dict(grammar=[g0, g1]))
    (shape, _, ids), = res
    assert shape == [2, 5], res
    assert ids[0] == [tok(c, 0) for c in range(3)] + [T.PAD] * 2 and ids[1] == [tok(c, 1) for c in range(5)]
    adv = [e[1] for e in log if _name(e) == "grammar_advance"]
    if path in GRAPH:                                                   # one captured advance, replayed; the host looks after 8
        assert len(adv) == 3 and len([e for e in log if _name(e) == "replay"]) == 8
    else:
        assert len(adv) == 5 and [a["n_add"] for a in adv] == [1, 2, 3, 4, 5]
    # with a stop sequence as well the loop's re-match runs the match alone, and both ends count
    with monkeypatch.context() as mp:
        log, res = _call(mp, spec, dict(grammar=[g0, None], stop_sequences=[[tok(3, 1), tok(4, 1)]]))
    (shape, _, ids), = res
    assert shape == [2, 5] and ids[0][3:] == [T.PAD] * 2 and ids[1] == [tok(c, 1) for c in range(5)]
    assert len([e for e in log if _name(e) == "grammar_advance"]) == (3 if path in GRAPH else 5)


def test_the_default_reaches_no_grammar_code(monkeypatch):
    """with grammar=None generate() must not reach the new code at all: the table class, the three ops, the checks and
    the module's own entry points raise"""
    def boom(*a, **k):
        raise AssertionError("reached with the default")
    with monkeypatch.context() as mp:
        lm = T.make_model()
        T.GenTrace(mp, lm, T.Script(3, 2))
        for n in ("GrammarTable", "grammar_mask", "grammar_advance", "grammar_build"):
            mp.setattr(ops, n, boom)
        for n in ("_grammar_check", "_grammar_rows"):
            mp.setattr(Mo, n, boom)
        for n in ("combine", "trim_table_"):
            mp.setattr(G, n, boom)
        mp.setattr(TokenDFA, "table", boom)
        for kw in (dict(), dict(decode_graph=False), dict(use_cache=False), T.PROC, dict(num_beams=2), dict(grammar=None)):
            out = lm.generate(inputs_embeds=torch.zeros((2, T.S0, T.D), dtype=torch.bfloat16), max_new_tokens=6,
                              eos_token_id=T.EOS, pad_token_id=T.PAD, **kw)
            assert torch.is_tensor(out)
    # a list of unconstrained rows is the plain call too
    with monkeypatch.context() as mp:
        lm = T.make_model()
        T.GenTrace(mp, lm, T.Script(3, 2))
        for n in ("GrammarTable", "grammar_mask", "grammar_advance", "grammar_build"):
            mp.setattr(ops, n, boom)
        out = lm.generate(inputs_embeds=torch.zeros((2, T.S0, T.D), dtype=torch.bfloat16), max_new_tokens=6,
                          eos_token_id=T.EOS, pad_token_id=T.PAD, grammar=[None, None])
        assert torch.is_tensor(out)
