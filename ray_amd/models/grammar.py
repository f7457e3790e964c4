"""Token-level automata for grammar-constrained decoding (host side, numpy only).

A ``TokenDFA`` is a deterministic automaton over token ids: ``next[q, t]`` is the state after
emitting token ``t`` in state ``q``, or -1 when ``t`` is not allowed there. EOS is an ordinary
column: ``next[q, eos] = q`` in an accepting state, -1 elsewhere, so the device ops
(``rf.grammar_mask`` / ``rf.grammar_advance``, ops/csrc/grammar.hip) know nothing about
acceptance: they ban the columns that hold a negative entry and follow the others.

Three constructors: ``from_choices`` (one of these token sequences), ``from_byte_dfa`` (a DFA
over bytes lifted to a vocabulary of byte strings) and ``from_regex`` (a stated regex subset
over bytes, full-match semantics). Every automaton is validated: no reachable state is a
dead end, so a constrained request can always go on and can always finish.
"""

from __future__ import annotations

import numpy as np

GRAMMAR_NONE = -1  # a row's state: unconstrained
GRAMMAR_DEAD = -2  # a row's state: it emitted a token its grammar forbids (mask: keep bytes)
MAX_STATES = 32767  # states are int16


def padded_vocab(vocab_size: int) -> int:
    """The width of a device table row: V rounded up to 8 (16-byte aligned int16 rows)."""
    return (int(vocab_size) + 7) // 8 * 8


class TokenDFA:
    """``next`` int [n_states, V], ``start``, ``eos_token_id``. Validates (``ValueError``):
    values in ``[-1, n_states)``; every state reachable from ``start`` allows a token and can
    reach a state that allows EOS; at most ``MAX_STATES`` states. Unreachable states are
    dropped (the kept ones are renumbered in their old order)."""

    def __init__(self, next, start, eos_token_id):
        nxt = np.asarray(next)
        if nxt.ndim != 2 or nxt.shape[0] < 1 or nxt.shape[1] < 1 or nxt.dtype.kind not in "iu":
            raise ValueError("TokenDFA: next must be an integer table [n_states >= 1, V >= 1]")
        nxt = nxt.astype(np.int64, copy=False)
        Q, V = nxt.shape
        for name, v, hi in (("start", start, Q), ("eos_token_id", eos_token_id, V)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < hi:
                raise ValueError(f"TokenDFA: {name} must be an int in [0, {hi}), got {v!r}")
        if nxt.min() < -1 or nxt.max() >= Q:
            raise ValueError(f"TokenDFA: next holds values outside [-1, {Q})")
        start, eos = int(start), int(eos_token_id)
        succ = [np.unique(row[row >= 0]) for row in nxt]
        reach = np.zeros(Q, dtype=bool)
        reach[start] = True
        todo = [start]
        while todo:
            for s in succ[todo.pop()]:
                if not reach[s]:
                    reach[s] = True
                    todo.append(int(s))
        if int(reach.sum()) > MAX_STATES:
            raise ValueError(f"TokenDFA: {int(reach.sum())} states, at most {MAX_STATES} fit")
        for q in np.flatnonzero(reach):
            if len(succ[q]) == 0:
                raise ValueError(f"TokenDFA: state {q} is reachable and allows no token")
        # the states that can reach one allowing EOS: backwards from those
        pred = [[] for _ in range(Q)]
        for q in np.flatnonzero(reach):
            for s in succ[q]:
                pred[int(s)].append(int(q))
        good = reach & (nxt[:, eos] >= 0)
        todo = [int(q) for q in np.flatnonzero(good)]
        while todo:
            for p in pred[todo.pop()]:
                if not good[p]:
                    good[p] = True
                    todo.append(p)
        bad = np.flatnonzero(reach & ~good)
        if len(bad):
            raise ValueError(f"TokenDFA: state {int(bad[0])} is reachable and cannot reach a "
                             f"state that allows EOS")
        new_id = np.full(Q + 1, -1, dtype=np.int64)  # [-1] stays -1
        new_id[:Q][reach] = np.arange(int(reach.sum()))
        self.next = new_id[nxt[reach]].astype(np.int16)
        self.next.setflags(write=False)
        self.start = int(new_id[start])
        self.eos_token_id = eos

    @property
    def n_states(self) -> int:
        return self.next.shape[0]

    @property
    def vocab_size(self) -> int:
        return self.next.shape[1]

    def walk(self, tokens, state=None) -> int:
        """The state after ``tokens`` from ``state`` (default ``start``), -1 once a token is
        not allowed (or is no token id)."""
        q = self.start if state is None else int(state)
        for t in tokens:
            t = int(t)
            if q < 0 or not 0 <= t < self.vocab_size:
                return -1
            q = int(self.next[q, t])
        return q

    def accepts(self, tokens) -> bool:
        """True iff every token is allowed where it stands and the last one is EOS (which is
        allowed in accepting states only, and stays there: trailing EOS repeats are fine)."""
        tokens = [int(t) for t in tokens]
        return bool(tokens) and tokens[-1] == self.eos_token_id and self.walk(tokens) >= 0

    def table(self, offset: int = 0) -> np.ndarray:
        """int16 [n_states, padded_vocab(V)] for the device: states shifted by ``offset`` (the
        automaton's first row in a shared pool), -1 kept, the padding columns -1."""
        if offset < 0 or offset + self.n_states > MAX_STATES:
            raise ValueError(f"TokenDFA: states {offset}..{offset + self.n_states} do not fit "
                             f"int16")
        t = np.full((self.n_states, padded_vocab(self.vocab_size)), -1, dtype=np.int16)
        t[:, : self.vocab_size] = np.where(self.next >= 0, self.next + np.int16(offset),
                                           np.int16(-1))
        return t

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_choices(cls, choices, vocab_size, eos_token_id):
        """Exactly one of ``choices`` (non-empty token sequences), then EOS: a trie; a node
        that ends a choice is accepting and keeps its children."""
        V, eos = int(vocab_size), int(eos_token_id)
        choices = [tuple(int(t) for t in c) for c in choices]
        if not choices:
            raise ValueError("from_choices: no choices")
        if len(set(choices)) != len(choices):
            raise ValueError("from_choices: duplicate choices")
        rows = [np.full(V, -1, dtype=np.int64)]
        accepting = [False]
        for c in choices:
            if not c:
                raise ValueError("from_choices: an empty choice")
            q = 0
            for t in c:
                if not 0 <= t < V:
                    raise ValueError(f"from_choices: token {t} outside [0, {V})")
                if t == eos:
                    raise ValueError("from_choices: EOS inside a choice")
                if rows[q][t] < 0:
                    rows[q][t] = len(rows)
                    rows.append(np.full(V, -1, dtype=np.int64))
                    accepting.append(False)
                q = int(rows[q][t])
            accepting[q] = True
        for q, acc in enumerate(accepting):
            if acc:
                rows[q][eos] = q
        return cls(np.stack(rows), 0, eos)

    @classmethod
    def from_byte_dfa(cls, vocab, trans, start, accepting, eos_token_id):
        """Lifts a DFA over bytes (``trans`` int [Q, 256], -1 dead; ``accepting`` the set of
        accepting states) to ``vocab``, a list of V ``bytes`` (an empty entry: never allowed;
        the entry of ``eos_token_id`` is ignored). Token t is allowed in q iff walking its
        bytes from q stays alive and ends where an accepting state is still reachable with
        tokens of the vocabulary. One numpy step per byte position over all (state, token)."""
        trans = np.asarray(trans)
        if trans.ndim != 2 or trans.shape[1] != 256 or trans.shape[0] < 1 or \
                trans.dtype.kind not in "iu":
            raise ValueError("from_byte_dfa: trans must be an integer table [Q, 256]")
        Q, V, eos = trans.shape[0], len(vocab), int(eos_token_id)
        if trans.min() < -1 or trans.max() >= Q:
            raise ValueError(f"from_byte_dfa: trans holds values outside [-1, {Q})")
        if not 0 <= int(start) < Q or not 0 <= eos < V:
            raise ValueError("from_byte_dfa: start or eos_token_id out of range")
        acc = np.zeros(Q, dtype=bool)
        for q in accepting:
            if not 0 <= int(q) < Q:
                raise ValueError(f"from_byte_dfa: accepting state {q} outside [0, {Q})")
            acc[int(q)] = True
        lens = np.array([len(v) for v in vocab], dtype=np.int64)
        lens[eos] = 0
        L = int(lens.max()) if V else 0
        byt = np.zeros((V, max(L, 1)), dtype=np.int64)
        for t, v in enumerate(vocab):
            if lens[t]:
                byt[t, : lens[t]] = np.frombuffer(bytes(v), dtype=np.uint8)
        tr = np.concatenate([trans.astype(np.int32), np.full((1, 256), Q, np.int32)])
        tr[tr < 0] = Q  # row Q: the dead state, which stays dead
        cur = np.broadcast_to(np.arange(Q, dtype=np.int32)[:, None], (Q, V)).copy()
        for p in range(L):
            live = lens > p
            cur[:, live] = tr[cur[:, live], byt[live, p][None, :]]
        nxt = np.where((cur < Q) & (lens > 0)[None, :], cur, -1).astype(np.int64)
        # keep only the transitions into states that can still finish with these tokens
        pred = [[] for _ in range(Q)]
        for q in range(Q):
            for s in np.unique(nxt[q][nxt[q] >= 0]):
                pred[int(s)].append(q)
        good = acc.copy()
        todo = [int(q) for q in np.flatnonzero(acc)]
        while todo:
            for p in pred[todo.pop()]:
                if not good[p]:
                    good[p] = True
                    todo.append(p)
        nxt[~np.concatenate([good, [False]])[nxt]] = -1  # (-1 indexes the spare False)
        nxt[:, eos] = np.where(acc, np.arange(Q), -1)
        if not good[int(start)]:
            raise ValueError("from_byte_dfa: no token sequence of this vocabulary is accepted")
        return cls(nxt, int(start), eos)

    @classmethod
    def from_regex(cls, pattern, vocab, eos_token_id):
        """The token sequences whose bytes ``pattern`` matches in full. Supported, over bytes:
        literals and escapes (``\\n \\t \\r \\f \\v \\0 \\xHH`` and escaped punctuation),
        ``.`` (any byte but newline), classes ``[a-z0-9_]`` and negated classes,
        ``\\d \\w \\s`` (and ``\\D \\W \\S``), groups ``( )`` and ``(?: )``, ``|``, ``* + ?``,
        ``{m}`` and ``{m,n}`` with n <= 64. Anything else raises ``ValueError`` naming the
        construct. Thompson construction, subset construction, then ``from_byte_dfa``."""
        trans, start, accepting = regex_to_byte_dfa(pattern)
        return cls.from_byte_dfa(vocab, trans, start, accepting, eos_token_id)


# ---------------------------------------------------------------------- regex -> byte DFA
_MAX_REPEAT = 64


def _mask(*bytes_or_ranges):
    m = np.zeros(256, dtype=bool)
    for x in bytes_or_ranges:
        if isinstance(x, tuple):
            m[x[0]: x[1] + 1] = True
        else:
            m[x] = True
    return m


_DIGIT = _mask((0x30, 0x39))
_WORD = _mask((0x30, 0x39), (0x41, 0x5A), (0x61, 0x7A), 0x5F)
_SPACE = _mask(0x20, (0x09, 0x0D))
_SHORT = {ord("d"): _DIGIT, ord("w"): _WORD, ord("s"): _SPACE,
          ord("D"): ~_DIGIT, ord("W"): ~_WORD, ord("S"): ~_SPACE}
_CTRL = {ord("n"): 10, ord("t"): 9, ord("r"): 13, ord("f"): 12, ord("v"): 11, ord("0"): 0,
         ord("a"): 7}
_PUNCT = set(b".^$*+?{}[]()|\\/-\"' #&~<>=!:,;@%`_")


class _Parser:
    """Recursive descent over the pattern's bytes into ('set', mask) | ('cat', [..]) |
    ('alt', [..]) | ('rep', node, m, n) with n None for unbounded."""

    def __init__(self, pat: bytes):
        self.p, self.i = pat, 0

    def fail(self, what):
        raise ValueError(f"from_regex: unsupported construct: {what} (at offset {self.i})")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in b"|)":
            items.append(self.rep())
        return ("cat", items)

    def rep(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == ord("*"):
                m, n = 0, None
            elif c == ord("+"):
                m, n = 1, None
            elif c == ord("?"):
                m, n = 0, 1
            elif c == ord("{"):
                j = self.p.find(b"}", self.i)
                body = self.p[self.i + 1: j] if j > 0 else b""
                lo, sep, hi = body.partition(b",")
                if j < 0 or not lo.isdigit() or (sep and not hi.isdigit()):
                    self.fail("counted repetition other than {m} or {m,n} "
                              f"('{self.p[self.i: j + 1 if j > 0 else None].decode('latin-1')}')")
                m = int(lo)
                n = int(hi) if sep else m
                if n > _MAX_REPEAT or m > n:
                    self.fail(f"{{m,n}} needs m <= n <= {_MAX_REPEAT}")
                self.i = j  # the '}' is consumed below
            else:
                return node
            self.i += 1
            if self.peek() is not None and self.peek() in b"?+":
                self.fail("lazy or possessive quantifier")
            node = ("rep", node, m, n)

    def escape(self, in_class):
        """After a backslash: a mask."""
        c = self.peek()
        if c is None:
            self.fail("trailing backslash")
        self.i += 1
        if c in _SHORT:
            return _SHORT[c]
        if c == ord("x"):
            h = self.p[self.i: self.i + 2]
            try:
                v = int(h.decode("latin-1"), 16) if len(h) == 2 else -1
            except ValueError:
                v = -1
            if v < 0:
                self.fail("\\x without two hex digits")
            self.i += 2
            return _mask(v)
        if c in _CTRL and not (c == ord("0") and self.peek() is not None
                               and chr(self.peek()).isdigit()):
            return _mask(_CTRL[c])
        if c == ord("b") and in_class:
            return _mask(8)
        if c in _PUNCT:
            return _mask(c)
        self.fail(f"escape '\\{chr(c)}'")

    def atom(self):
        c = self.peek()
        if c == ord("("):
            self.i += 1
            if self.peek() == ord("?"):
                if self.p[self.i: self.i + 2] != b"?:":
                    self.fail("group extension '(?...' other than '(?:'")
                self.i += 2
            node = self.alt()
            if self.peek() != ord(")"):
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == ord("["):
            return self.cls()
        if c == ord("."):
            self.i += 1
            return ("set", ~_mask(10))
        if c == ord("\\"):
            self.i += 1
            return ("set", self.escape(False))
        if c in b"^$":
            self.fail(f"anchor '{chr(c)}' (the match is always a full match)")
        if c in b"*+?{":
            self.fail(f"quantifier '{chr(c)}' with nothing to repeat")
        if c in b"]}":
            self.fail(f"unescaped '{chr(c)}'")
        self.i += 1
        return ("set", _mask(c))

    def cls(self):
        self.i += 1  # '['
        neg = self.peek() == ord("^")
        if neg:
            self.i += 1
        m = np.zeros(256, dtype=bool)
        first = True
        while True:
            c = self.peek()
            if c is None:
                self.fail("unterminated class")
            if c == ord("]") and not first:
                self.i += 1
                break
            first = False
            if c == ord("[") and self.p[self.i: self.i + 2] in (b"[:", b"[=", b"[."):
                self.fail("POSIX class")
            self.i += 1
            if c == ord("\\"):
                lo = self.escape(True)
                single = int(lo.sum()) == 1
            else:
                lo, single = _mask(c), True
            if self.peek() == ord("-") and self.i + 1 < len(self.p) and \
                    self.p[self.i + 1] != ord("]"):
                if not single:
                    self.fail("class range from a character set")
                self.i += 1
                d = self.peek()
                self.i += 1
                if d == ord("\\"):
                    hi = self.escape(True)
                    if int(hi.sum()) != 1:
                        self.fail("class range to a character set")
                else:
                    hi = _mask(d)
                a, b = int(np.flatnonzero(lo)[0]), int(np.flatnonzero(hi)[0])
                if a > b:
                    self.fail("reversed class range")
                m |= _mask((a, b))
            else:
                m |= lo
        return ("set", ~m if neg else m)


class _NFA:
    def __init__(self):
        self.eps, self.edge = [], []  # per state: epsilon targets; (mask, target) or None

    def new(self):
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def build(self, node):
        """(entry, exit) of a fresh fragment for ``node``."""
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            self.edge[s] = (node[1], e)
            return s, e
        if kind == "cat":
            s = e = self.new()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == "alt":
            s, e = self.new(), self.new()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, m, n = node
        s = e = self.new()
        for _ in range(m):
            a, b = self.build(sub)
            self.eps[e].append(a)
            e = b
        if n is None:  # sub*
            a, b = self.build(sub)
            loop = self.new()
            self.eps[e].append(loop)
            self.eps[loop].append(a)
            self.eps[b].append(loop)
            return s, loop
        end = self.new()
        for _ in range(n - m):  # (sub(sub(...)?)?)?
            a, b = self.build(sub)
            self.eps[e].append(end)
            self.eps[e].append(a)
            e = b
        self.eps[e].append(end)
        return s, end

    def closure(self, states):
        seen = set(states)
        todo = list(states)
        while todo:
            for t in self.eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)


def regex_to_byte_dfa(pattern):
    """``(trans int32 [Q, 256] with -1 dead, start, accepting states)`` of the subset of
    regular expressions that ``TokenDFA.from_regex`` states."""
    if isinstance(pattern, str):
        pattern = pattern.encode("utf-8")
    if not isinstance(pattern, (bytes, bytearray)):
        raise ValueError("from_regex: pattern must be str or bytes")
    nfa = _NFA()
    entry, final = nfa.build(_Parser(bytes(pattern)).parse())
    start = nfa.closure([entry])
    ids = {start: 0}
    order = [start]
    rows = []
    i = 0
    while i < len(order):
        edges = [nfa.edge[s] for s in sorted(order[i]) if nfa.edge[s] is not None]
        row = np.full(256, -1, dtype=np.int32)
        if edges:
            fires = np.stack([m for m, _ in edges])  # [E, 256]
            # bytes with the same column of ``fires`` go to the same state
            cols, inv = np.unique(fires, axis=1, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
            for c in range(cols.shape[1]):
                if not cols[:, c].any():
                    continue
                tgt = nfa.closure([edges[k][1] for k in np.flatnonzero(cols[:, c])])
                if tgt not in ids:
                    ids[tgt] = len(order)
                    order.append(tgt)
                    if len(order) > MAX_STATES:
                        raise ValueError("from_regex: the pattern needs too many states")
                row[inv == c] = ids[tgt]
        rows.append(row)
        i += 1
    accepting = [k for k, s in enumerate(order) if final in s]
    return np.stack(rows), 0, accepting
