"""Grammars for generate(grammar=): deterministic automata over token ids.

A TokenDFA is made on the host -- from a regular expression and the vocabulary's bytes, from a list of allowed answers,
or from explicit token edges -- and needs no device until generate() asks for its table (TokenDFA.table: the token table
of include/macaw_hip.h, "Grammar-constrained decoding", made by ops.grammar_build and trimmed on the device, cached per
device).  generate() then masks the logits in front of every selection and advances one state per sample behind every
emit, both from device memory: a constrained call is still one hipGraph replay per token.

No regex-to-automaton library is needed: from_regex parses the pattern itself (Thompson NFA -> subset construction ->
removal of the states that cannot reach acceptance)."""
from __future__ import annotations

import numpy as np

MAX_STATES = 65536
MAX_TABLE_BYTES = 2 << 30

_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_CLASSES = {ord("d"): _DIGIT, ord("w"): _WORD, ord("s"): _SPACE, ord("D"): _ALL - _DIGIT, ord("W"): _ALL - _WORD,
            ord("S"): _ALL - _SPACE}
_CONTROL = {ord("n"): 0x0A, ord("t"): 0x09, ord("r"): 0x0D}
_HEX = b"0123456789abcdefABCDEF"


# ------------------------------------------------------------------------------------------------ the pattern --
class _Parser:
    """pattern bytes -> syntax tree: ("set", frozenset of bytes), ("cat", [nodes]), ("alt", [nodes]), ("rep", node, m, n or
    None).  The language is that of re.fullmatch(pattern.encode(), data) on bytes, so a quantifier behind a non-ASCII
    literal repeats its last byte, as it does there"""

    def __init__(self, pattern: str):
        self.src, self.p, self.i = pattern, pattern.encode("utf-8"), 0

    def fail(self, what):
        raise ValueError(f"TokenDFA.from_regex: {what} at byte {self.i} of {self.src!r} is not supported")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("an unbalanced ')'")
        return node

    def alt(self):
        arms = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in b"|)":
            items.append(self.quantified(self.atom()))
        return ("cat", items)

    def hex_byte(self):
        h = self.p[self.i:self.i + 2]
        if len(h) != 2 or h[0] not in _HEX or h[1] not in _HEX:
            self.fail("an incomplete \\x escape")
        self.i += 2
        return int(h, 16)

    def escape(self, in_class):
        """behind a backslash -> a frozenset (a class escape) or an int (one byte)"""
        c = self.peek()
        if c is None:
            self.fail("a trailing backslash")
        self.i += 1
        if c in _CLASSES:
            return _CLASSES[c]
        if c in _CONTROL:
            return _CONTROL[c]
        if c == ord("x"):
            return self.hex_byte()
        if 0x30 <= c <= 0x39:
            self.i -= 1
            self.fail("a back-reference or octal escape (\\%c)" % c)
        if c in b"AZbB":
            self.i -= 1
            self.fail("an anchor (\\%c)" % c)
        if c >= 0x80 or chr(c).isalnum():
            self.i -= 1
            self.fail("the escape \\%s" % (chr(c) if c < 0x80 else "<non-ASCII>"))
        return c                                   # an escaped metacharacter or punctuation

    def klass(self):
        negate = self.peek() == ord("^")
        if negate:
            self.i += 1
        members, first = set(), True
        while True:
            c = self.peek()
            if c is None:
                self.fail("an unterminated class")
            if c == ord("]") and not first:
                self.i += 1
                break
            first = False
            lo = self.class_item()
            if isinstance(lo, frozenset):
                members |= lo
                continue
            if self.peek() == ord("-") and self.i + 1 < len(self.p) and self.p[self.i + 1] != ord("]"):
                self.i += 1
                hi = self.class_item()
                if isinstance(hi, frozenset) or hi < lo:
                    self.fail("a bad class range")
                members |= set(range(lo, hi + 1))
            else:
                members.add(lo)
        return ("set", frozenset(_ALL - members if negate else members))

    def class_item(self):
        c = self.peek()
        if c is None:
            self.fail("an unterminated class")
        if c >= 0x80:
            self.fail("a non-ASCII character inside a class")
        self.i += 1
        if c == ord("\\"):
            return self.escape(True)
        return c

    def atom(self):
        c = self.peek()
        if c == ord("("):
            self.i += 1
            if self.peek() == ord("?"):
                if self.p[self.i:self.i + 2] != b"?:":
                    kind = {b"?=": "look-ahead", b"?!": "look-ahead", b"?<": "look-behind or a named group",
                            b"?P": "a named group or reference", b"?#": "a comment group"}.get(self.p[self.i:self.i + 2],
                                                                                               "an inline flag group")
                    self.fail(f"{kind} '({self.p[self.i:self.i + 2].decode('latin1')}'")
                self.i += 2
            node = self.alt()
            if self.peek() != ord(")"):
                self.fail("an unbalanced '('")
            self.i += 1
            return node
        if c == ord("["):
            self.i += 1
            return self.klass()
        if c == ord("."):
            self.i += 1
            return ("set", frozenset(_ALL - {0x0A}))
        if c == ord("\\"):
            self.i += 1
            e = self.escape(False)
            return ("set", e if isinstance(e, frozenset) else frozenset([e]))
        if c in b"^$":
            self.fail("an anchor (%c)" % c)
        if c in b"*+?":
            self.fail("a quantifier with nothing to repeat")
        if c == ord("{") and self.bounds(self.i) is not None:
            self.fail("a quantifier with nothing to repeat")
        self.i += 1
        return ("set", frozenset([c]))             # a literal byte ('{' and '}' outside a quantifier included, as in re)

    def bounds(self, i):
        """a {m}, {m,}, {m,n} or {,n} at byte i -> (m, n or None, index behind it), else None ('{' is then a literal)"""
        j = self.p.find(b"}", i)
        if j < 0:
            return None
        body = self.p[i + 1:j]
        lo, sep, hi = body.partition(b",")
        if not (lo.isdigit() or (lo == b"" and sep and hi.isdigit())) or not (hi == b"" or hi.isdigit()):
            return None
        m = int(lo) if lo else 0
        n = m if not sep else (int(hi) if hi else None)
        return m, n, j + 1

    def quantified(self, node):
        c = self.peek()
        if c is None:
            return node
        if c in b"*+?":
            self.i += 1
            m, n = {ord("*"): (0, None), ord("+"): (1, None), ord("?"): (0, 1)}[c]
        elif c == ord("{") and self.bounds(self.i) is not None:
            m, n, self.i = self.bounds(self.i)
            if n is not None and n < m:
                self.fail("a repeat with max < min")
        else:
            return node
        c = self.peek()
        if c == ord("?"):
            self.fail("a lazy quantifier")
        if c == ord("+"):
            self.fail("a possessive quantifier")
        if c == ord("*") or (c == ord("{") and self.bounds(self.i) is not None):
            self.fail("a multiple repeat")
        return ("rep", node, m, n)


class _NFA:
    """Thompson's construction: a state has epsilon edges and at most one byte-set edge"""

    LIMIT = 1 << 21

    def __init__(self):
        self.eps, self.edge, self.sets, self.set_ids = [], [], [], {}

    def new(self):
        if len(self.eps) >= self.LIMIT:
            raise ValueError(f"TokenDFA.from_regex: the pattern needs more than {self.LIMIT} NFA states (a repeat count "
                             "too large)")
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def build(self, node):
        kind = node[0]
        a, z = self.new(), self.new()
        if kind == "set":
            k = self.set_ids.setdefault(node[1], len(self.sets))
            if k == len(self.sets):
                self.sets.append(node[1])
            self.edge[a] = (k, z)
        elif kind == "cat":
            cur = a
            for item in node[1]:
                s, e = self.build(item)
                self.eps[cur].append(s)
                cur = e
            self.eps[cur].append(z)
        elif kind == "alt":
            for arm in node[1]:
                s, e = self.build(arm)
                self.eps[a].append(s)
                self.eps[e].append(z)
        else:
            _, sub, m, n = node
            cur = a
            for _ in range(m):
                s, e = self.build(sub)
                self.eps[cur].append(s)
                cur = e
            if n is None:                          # a star behind the m copies
                s, e = self.build(sub)
                self.eps[cur] += [s, z]
                self.eps[e] += [s, z]
            else:                                  # n - m optional copies, each of which may leave for the end
                for _ in range(n - m):
                    s, e = self.build(sub)
                    self.eps[cur] += [s, z]
                    cur = e
                self.eps[cur].append(z)
        return a, z


def _compile(pattern, max_states):
    """pattern -> (char_next int32 [S, 256], accepting bool [S]) with start state 0, every state able to reach acceptance"""
    nfa = _NFA()
    start, final = nfa.build(_Parser(pattern).parse())
    n_sets = len(nfa.sets)
    member = np.zeros((max(n_sets, 1), 256), dtype=bool)
    for k, s in enumerate(nfa.sets):
        member[k, list(s)] = True
    # bytes that no set tells apart behave alike: one column per class of bytes
    _, rep, class_of = np.unique(member, axis=1, return_index=True, return_inverse=True)
    class_of = np.asarray(class_of).reshape(-1)
    fires = [np.nonzero(member[k, rep])[0].tolist() for k in range(n_sets)]
    n_cls = len(rep)
    closure_memo = {}

    def closure(q):
        got = closure_memo.get(q)
        if got is None:
            seen, stack = {q}, [q]
            while stack:
                for r in nfa.eps[stack.pop()]:
                    if r not in seen:
                        seen.add(r)
                        stack.append(r)
            got = closure_memo[q] = frozenset(seen)
        return got

    first = closure(start)
    ids, order, rows = {first: 0}, [first], []
    i = 0
    while i < len(order):
        buckets = {}
        for q in order[i]:
            e = nfa.edge[q]
            if e is not None:
                for k in fires[e[0]]:
                    buckets.setdefault(k, set()).add(e[1])
        row = [-1] * n_cls
        for k, targets in buckets.items():
            sub = frozenset().union(*(closure(t) for t in targets))
            j = ids.get(sub)
            if j is None:
                j = ids[sub] = len(order)
                order.append(sub)
                if len(order) > max_states:
                    raise ValueError(f"TokenDFA.from_regex: the pattern needs more than max_states={max_states} states "
                                     f"({len(order)} and counting)")
            row[k] = j
        rows.append(row)
        i += 1
    table = np.array(rows, dtype=np.int32).reshape(len(order), n_cls)
    acc = np.array([final in s for s in order], dtype=bool)
    # states that cannot reach acceptance go; the rest are renumbered in the order they were found (the start stays 0)
    src, col = np.nonzero(table >= 0)
    live = _backward_live(src, table[src, col], acc)
    if not live[0]:
        raise ValueError(f"TokenDFA.from_regex: {pattern!r} matches nothing")
    renum = np.full(len(order) + 1, -1, dtype=np.int32)       # (the last entry serves the index -1)
    renum[:-1][live] = np.arange(int(live.sum()), dtype=np.int32)
    table = renum[table[live]]
    return np.ascontiguousarray(table[:, class_of]), acc[live]


def _backward_live(src, dst, accepting):
    """the states from which an accepting state can be reached along the edges src -> dst (accepting ones included)"""
    live = np.array(accepting, dtype=bool, copy=True)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    while True:
        new = live[dst] & ~live[src]
        if not new.any():
            return live
        live[src[new]] = True


# ----------------------------------------------------------------------------------------------- the automaton --
class TokenDFA:
    """A deterministic automaton over token ids: a start state, accepting states, and per (state, token) the next state.
    States are 0 ... n_states - 1.  A sample constrained by it may only emit tokens the current state allows; eos is
    allowed exactly in accepting states; a TERMINAL state (accepting, no allowed token) ends the sample by itself.

    The table is token-trimmed: a token that leads into a state from which no accepting state can be reached by tokens of
    this vocabulary is not allowed, so a constrained sample can always still finish.  A start state that cannot raises
    ValueError ("the vocabulary cannot spell the grammar") when the table, or the first host answer, is made.

    Two limits of generate(grammar=): max_new_tokens can cut an answer short -- check with walk(ids) / is_accepting -- and
    without an eos_token_id an accepting state that still has allowed tokens never ends by itself."""

    def __init__(self):
        raise TypeError("use TokenDFA.from_regex, TokenDFA.from_choices or TokenDFA.from_edges")

    @classmethod
    def _make(cls, n_states, accepting, start, vocab_size, max_table_bytes):
        g = object.__new__(cls)
        g.n_states, g.start, g.vocab_size = int(n_states), int(start), vocab_size
        g._acc = np.asarray(accepting, dtype=bool)
        g._char_next = g._tok_bytes = g._tok_off = None
        g._e_src = g._e_tok = g._e_dst = None
        g._live, g._rows, g._tables, g._joined = None, {}, {}, {}
        g._max_table_bytes = max_table_bytes
        if vocab_size is not None:
            g._size_check(vocab_size)
        return g

    def _size_check(self, V):
        need = self.n_states * V * 4
        if need > self._max_table_bytes:
            raise ValueError(f"TokenDFA: the device table of {self.n_states} states x {V} tokens takes {need} bytes, more "
                             f"than max_table_bytes={self._max_table_bytes}")

    # ------------------------------------------------------------------------------------------ constructors --
    @classmethod
    def from_regex(cls, pattern: str, vocab, max_states=MAX_STATES, max_table_bytes=MAX_TABLE_BYTES):
        """The language of re.fullmatch(pattern.encode(), data) on BYTES over a vocabulary of byte strings: vocab is a
        list of bytes | None, one entry per token id; None or b"" is a token that is never allowed (specials, pad, bos,
        eos, added tokens).  `.` is any byte but \\n; \\d \\w \\s and their negations are ASCII; a negated class matches
        bytes >= 0x80 too; a non-ASCII literal is its UTF-8 bytes.  Syntax: literals, escapes (\\d\\w\\s\\D\\W\\S\\n\\t\\r
        \\xHH and escaped metacharacters), `.`, classes with ranges and ^, ( ), (?: ), |, * + ?, {m}, {m,}, {m,n}.
        Anchors, back-references, look-around, lazy or possessive quantifiers, flags and a non-ASCII character inside a
        class raise ValueError naming the construct; more than max_states states, or a device table (n_states * V * 4
        bytes) above max_table_bytes, raise ValueError naming the count."""
        if not isinstance(pattern, str):
            raise ValueError(f"TokenDFA.from_regex: pattern must be a str, got {type(pattern).__name__}")
        vocab = list(vocab)
        if not vocab or any(not (t is None or isinstance(t, (bytes, bytearray))) for t in vocab):
            raise ValueError("TokenDFA.from_regex: vocab must be a non-empty list of bytes | None, one entry per token id")
        char_next, acc = _compile(pattern, int(max_states))
        g = cls._make(char_next.shape[0], acc, 0, len(vocab), max_table_bytes)
        g._char_next = char_next
        lens = np.array([0 if t is None else len(t) for t in vocab], dtype=np.int64)
        if int(lens.sum()) >= 1 << 31:
            raise ValueError(f"TokenDFA.from_regex: the vocabulary holds {int(lens.sum())} bytes; at most 2^31 - 1")
        g._tok_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        g._tok_bytes = np.frombuffer(b"".join(bytes(t) for t in vocab if t), dtype=np.uint8)
        g._by_len = np.argsort(-lens, kind="stable")
        g._lens = lens
        return g

    @classmethod
    def from_edges(cls, n_states, edges, accepting, start=0, vocab_size=None, max_table_bytes=MAX_TABLE_BYTES):
        """The general form: edges are (state, token, next_state) triples, accepting a collection of states.  vocab_size
        None: any vocabulary that holds the edges' tokens (the model's, when generate() makes the table)."""
        n_states = int(n_states)
        e = np.asarray(list(edges), dtype=np.int64).reshape(-1, 3)
        acc_ids = np.asarray(list(accepting), dtype=np.int64).reshape(-1)
        if n_states < 1 or not 0 <= int(start) < n_states:
            raise ValueError(f"TokenDFA.from_edges: {n_states} states with start {start}")
        if e.size and (e[:, [0, 2]].min() < 0 or e[:, [0, 2]].max() >= n_states or e[:, 1].min() < 0
                       or (vocab_size is not None and e[:, 1].max() >= vocab_size)):
            raise ValueError("TokenDFA.from_edges: an edge names a state outside [0, n_states) or a token outside the "
                             "vocabulary")
        if acc_ids.size and (acc_ids.min() < 0 or acc_ids.max() >= n_states):
            raise ValueError("TokenDFA.from_edges: an accepting state outside [0, n_states)")
        key = e[:, 0] * (int(e[:, 1].max()) + 1 if e.size else 1) + e[:, 1]
        if np.unique(key).size != key.size:
            raise ValueError("TokenDFA.from_edges: two edges leave one state by the same token (not deterministic)")
        acc = np.zeros(n_states, dtype=bool)
        acc[acc_ids] = True
        g = cls._make(n_states, acc, start, None if vocab_size is None else int(vocab_size), max_table_bytes)
        order = np.argsort(e[:, 0], kind="stable")
        g._e_src, g._e_tok, g._e_dst = e[order, 0], e[order, 1], e[order, 2]
        g._e_off = np.searchsorted(g._e_src, np.arange(n_states + 1))
        return g

    @classmethod
    def from_choices(cls, choices, vocab_size=None, max_table_bytes=MAX_TABLE_BYTES):
        """A trie at token level: the answer is exactly one of the token-id sequences.  A choice that is a proper prefix
        of another ends only by eos (its state is accepting, not terminal)."""
        choices = [list(c) for c in choices]
        if not choices or any(len(c) == 0 for c in choices) or any(
                isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0 for c in choices for t in c):
            raise ValueError("TokenDFA.from_choices: choices must be a non-empty list of non-empty lists of token ids >= 0")
        child, edges, accepting = {}, [], set()
        n = 1
        for c in choices:
            s = 0
            for t in c:
                nxt = child.get((s, int(t)))
                if nxt is None:
                    nxt = child[(s, int(t))] = n
                    edges.append((s, int(t), nxt))
                    n += 1
                s = nxt
            accepting.add(s)
        return cls.from_edges(n, edges, accepting, 0, vocab_size, max_table_bytes)

    # ---------------------------------------------------------------------------------------------- the host --
    @property
    def char_next(self):
        """from_regex: the byte automaton, int32 [n_states, 256], -1 where a byte is dead (None for the other forms)"""
        return self._char_next

    def _V(self):
        if self.vocab_size is not None:
            return self.vocab_size
        return int(self._e_tok.max()) + 1 if self._e_tok.size else 1

    def _raw_row(self, s, V=None):
        """next state per token from state s, before the token trim: int32 [V]"""
        V = self._V() if V is None else V
        if self._char_next is None:
            row = np.full(V, -1, dtype=np.int32)
            lo, hi = self._e_off[s], self._e_off[s + 1]
            row[self._e_tok[lo:hi]] = self._e_dst[lo:hi]
            return row
        cur = np.where(self._lens > 0, s, -1).astype(np.int32)
        order, lens, j = self._by_len, self._lens, 0
        n_act = int((lens > 0).sum())
        while n_act:
            act = order[:n_act]                    # the tokens longer than j bytes, longest first
            c = cur[act]
            ok = c >= 0
            byte = self._tok_bytes[self._tok_off[act[ok]].astype(np.int64) + j]
            c[ok] = self._char_next[c[ok], byte]
            cur[act] = c
            j += 1
            n_act = int(np.searchsorted(-lens[order], -j, side="left"))       # lens > j
        return cur

    def _ensure_live(self):
        if self._live is None:
            src, dst = [], []
            for s in range(self.n_states):
                r = self._raw_row(s)
                d = np.unique(r[r >= 0])
                src.append(np.full(d.size, s, dtype=np.int64))
                dst.append(d.astype(np.int64))
            self._set_live(_backward_live(np.concatenate(src), np.concatenate(dst), self._acc))
        return self._live

    def _set_live(self, live):
        if not live[self.start]:
            raise ValueError("TokenDFA: the vocabulary cannot spell the grammar (no accepting state can be reached from "
                             "the start state by its tokens)")
        self._live = live

    def _row(self, s):
        """the trimmed row of state s: int32 [V], -1 where the token is not allowed"""
        if not 0 <= s < self.n_states:
            raise ValueError(f"TokenDFA: state {s} outside [0, {self.n_states})")
        row = self._rows.get(s)
        if row is None:
            live = self._ensure_live()
            row = self._raw_row(s)
            row[(row >= 0) & ~live[np.maximum(row, 0)]] = -1
            if len(self._rows) >= 256:
                self._rows.pop(next(iter(self._rows)))
            self._rows[s] = row
        return row

    def walk(self, ids, state=None):
        """the state behind the token ids, from `state` (default: the start state); None when a token is not allowed"""
        s = self.start if state is None else int(state)
        for t in ids:
            row = self._row(s)
            t = int(t)
            if not 0 <= t < row.size or row[t] < 0:
                return None
            s = int(row[t])
        return s

    def allowed(self, state):
        """the sorted token ids allowed in `state` (eos is not among them: it is allowed exactly where is_accepting)"""
        return np.nonzero(self._row(int(state)) >= 0)[0].tolist()

    def is_accepting(self, state):
        return state is not None and bool(self._acc[int(state)])

    def is_terminal(self, state):
        """accepting with no allowed token: the sample ends by itself"""
        return self.is_accepting(state) and not bool((self._row(int(state)) >= 0).any())

    # -------------------------------------------------------------------------------------------- the device --
    def table(self, device, vocab_size=None):
        """-> (ops.GrammarTable on `device`, start state): the trimmed token table and its flags, made once per device
        (and vocabulary size, for a grammar made without one) and cached on this object"""
        import torch

        from . import ops
        device = torch.device(device)
        V = self.vocab_size if self.vocab_size is not None else vocab_size
        if V is None:
            V = self._V()
        if self.vocab_size is None and self._e_tok.size and int(self._e_tok.max()) >= V:
            raise ValueError(f"TokenDFA: token id {int(self._e_tok.max())} of the grammar is outside a vocabulary of {V}")
        key = (str(device), int(V))
        got = self._tables.get(key)
        if got is not None:
            return got, self.start
        self._size_check(V)
        if self._char_next is not None:
            nxt = ops.grammar_build(torch.from_numpy(self._char_next), torch.from_numpy(self._tok_bytes.copy()),
                                    torch.from_numpy(self._tok_off), device)
        else:
            ld = (V + 3) // 4 * 4
            full = torch.full((self.n_states, ld), -1, dtype=torch.int32, device=device)
            if self._e_src.size:
                full.view(-1)[torch.from_numpy(self._e_src * ld + self._e_tok).to(device)] = torch.from_numpy(
                    self._e_dst.astype(np.int32)).to(device)
            nxt = full[:, :V]
        live, flags = trim_table_(nxt, torch.from_numpy(self._acc).to(device))
        if self._live is None:
            self._set_live(live.cpu().numpy())
        got = self._tables[key] = ops.GrammarTable(nxt, flags)
        return got, self.start


def trim_table_(nxt, accepting):
    """The token trim on the device, in place: nxt int32 [S, V] (a view at any pitch), accepting bool [S] -> (live bool
    [S], flags uint8 [S]).  The state graph (which state leads to which, by any token) is taken off the table in row
    blocks, the backward reachability runs on that small graph on the host, then every transition into a state that is
    not live becomes -1 and the flags are bit 0 accepting, bit 1 accepting without an allowed token"""
    import torch
    S, V = nxt.shape
    dev = nxt.device
    rows = max(1, (1 << 23) // V)
    keys = []
    for r0 in range(0, S, rows):
        blk = nxt[r0:r0 + rows]
        src = torch.arange(r0, r0 + blk.shape[0], device=dev, dtype=torch.long).view(-1, 1).expand_as(blk)
        ok = blk >= 0
        keys.append(torch.unique(src[ok] * S + blk[ok].long()))
    k = torch.cat(keys).cpu().numpy()
    live_h = _backward_live(k // S, k % S, accepting.cpu().numpy())
    live = torch.from_numpy(live_h).to(dev)
    has = torch.zeros(S, dtype=torch.bool, device=dev)
    for r0 in range(0, S, rows):
        blk = nxt[r0:r0 + rows]
        dead = (blk >= 0) & ~live[blk.clamp(min=0).long()]
        blk.masked_fill_(dead, -1)
        has[r0:r0 + rows] = (blk >= 0).any(1)
    acc = accepting.to(torch.bool)
    flags = acc.to(torch.uint8) | ((acc & ~has).to(torch.uint8) << 1)
    return live, flags.contiguous()


def combine(grammars, device, vocab_size):
    """generate()'s table for a list of TokenDFA | None, one entry per row: the distinct objects' tables back to back,
    their states offset -> (ops.GrammarTable, start state per row, -1 for None).  The joined table is cached like a
    single grammar's (the last 8 combinations that a grammar leads) and held to the smallest max_table_bytes of its parts"""
    import torch

    from . import ops
    distinct = []
    for g in grammars:
        if g is not None and all(g is not d for d in distinct):
            distinct.append(g)
    tables = [g.table(device, vocab_size)[0] for g in distinct]
    offs = np.concatenate([[0], np.cumsum([t.n_states for t in tables])]).tolist()
    starts = [-1 if g is None else offs[[g is d for d in distinct].index(True)] + g.start for g in grammars]
    if len(tables) == 1:
        return tables[0], starts
    # the joined table is kept on the first grammar, with the others it was made of (alive, so their ids stay theirs)
    first = distinct[0]
    key = (tuple(id(g) for g in distinct[1:]), str(torch.device(device)), int(vocab_size))
    got = first._joined.get(key)
    if got is None:
        need, cap = offs[-1] * vocab_size * 4, min(g._max_table_bytes for g in distinct)
        if need > cap:
            raise ValueError(f"TokenDFA: the joined device table of {len(distinct)} grammars, {offs[-1]} states x {vocab_size} "
                             f"tokens, takes {need} bytes, more than max_table_bytes={cap}")
        ld = (vocab_size + 3) // 4 * 4
        full = torch.full((offs[-1], ld), -1, dtype=torch.int32, device=torch.device(device))
        for t, o in zip(tables, offs):
            full[o:o + t.n_states, :vocab_size] = torch.where(t.next >= 0, t.next + o, t.next)
        if len(first._joined) >= 8:
            first._joined.pop(next(iter(first._joined)))
        got = first._joined[key] = (ops.GrammarTable(full[:, :vocab_size], torch.cat([t.flags for t in tables])), distinct[1:])
    return got[0], starts


def vocab_bytes(pieces, special_ids=()):
    """The vocabulary of TokenDFA.from_regex from the strings a LLaMA SentencePiece tokenizer reports
    (tokenizer.convert_ids_to_tokens(range(V))): `▁` becomes a space, `<0xHH>` becomes that byte, the ids in
    special_ids become None (never allowed).  Pieces are taken AS THEY STAND: `▁yes` is b" yes", so the grammar's
    author writes the leading space into the pattern: ` ?(yes|no)`."""
    special = set(int(i) for i in special_ids)
    out = []
    for i, p in enumerate(pieces):
        if i in special or p is None:
            out.append(None)
        elif len(p) == 6 and p.startswith("<0x") and p.endswith(">") and all(c in "0123456789abcdefABCDEF" for c in p[3:5]):
            out.append(bytes([int(p[3:5], 16)]))
        else:
            out.append(p.replace("▁", " ").encode("utf-8"))
    return out
