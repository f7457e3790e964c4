"""``TokenDFA`` (models/grammar.py): the three constructors against brute force, and the
constructor's validation."""

import itertools
import re
import time

import numpy as np
import pytest

from ray_amd.models.grammar import TokenDFA, padded_vocab, regex_to_byte_dfa


def _all_sequences(V, longest):
    for n in range(longest + 1):
        yield from itertools.product(range(V), repeat=n)


# ------------------------------------------------------------------------- from_choices
def test_choices_accept_exactly_the_choices():
    V, EOS = 6, 5
    choices = [[1, 2, 3], [1, 2], [4], [0, 0, 1], [1, 3]]  # [1, 2] is a prefix of [1, 2, 3]
    dfa = TokenDFA.from_choices(choices, V, EOS)
    assert dfa.vocab_size == V and dfa.start == 0 and dfa.next.dtype == np.int16
    want = {tuple(c) + (EOS,) for c in choices}
    got = {s for s in _all_sequences(V, 4) if dfa.accepts(s)}
    # beyond the choices only trailing repeats of EOS are accepted (EOS stays where it is)
    assert {s for s in got if s.count(EOS) == 1} == want
    assert all(s[: s.index(EOS) + 1] in want and set(s[s.index(EOS):]) == {EOS} for s in got)
    assert dfa.walk([1, 2]) >= 0 and dfa.next[dfa.walk([1, 2]), 3] >= 0  # children kept
    assert not dfa.accepts([]) and not dfa.accepts([1, 2]) and not dfa.accepts([1, EOS])
    assert dfa.walk([1, 9]) == -1 and dfa.walk([2]) == -1


def test_choices_errors():
    for bad in ([], [[1], [1]], [[]], [[1, 6]], [[-1]], [[1, 5, 2]]):
        with pytest.raises(ValueError):
            TokenDFA.from_choices(bad, 6, 5)


# ------------------------------------------------------------------- regex and byte DFA
ALPHABET = b"ab1_ \n"
MULTI = [b"ab", b"ba", b"aa", b"bb", b"a1", b"1a", b"11", b"ab1", b"b1_", b"aab", b"abab",
         b"a ", b" a", b"  ", b"\n\n", b"a\n", b"_a", b"__", b"1_1", b"bab", b"aaa", b"bbb",
         b"111", b"ab ", b"1 1", b"_ _", b"a_b", b"b_a", b"ba1", b"1ab", b"abb", b"bba",
         b"a1b", b" \n", b"\n ", b"aaaa", b"abba", b"1111", b"a_", b"_1"]
VOCAB = [bytes([i]) for i in range(256)] + MULTI + [b""] + [b"<eos>"]
EOS = len(VOCAB) - 1
EMPTY = len(VOCAB) - 2

PATTERNS = [r"ab", r"a|b1", r"a*b", r"(ab)+", r"a?b?1", r"[ab]{2}", r"[^a]b", r".a", r"\d\w\s",
            r"a{1,3}", r"(a|b)*1", r"[a-b0-9_]+", r"(?:a|ab)(1|_)?", r"\s*a", r"a\n|\x62{2,3}",
            r"[\d_]a|\.?b", r"(a{2}){1,2}", r"a{0,2}b"]


def _tokenisations(s, pieces):
    """Every way to write the bytes ``s`` as a sequence of vocabulary tokens."""
    if not s:
        yield ()
        return
    for n in range(1, len(s) + 1):
        for t in pieces.get(s[:n], ()):
            for rest in _tokenisations(s[n:], pieces):
                yield (t,) + rest


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regex_accepts_what_re_fullmatch_accepts(pattern):
    dfa = TokenDFA.from_regex(pattern, VOCAB, EOS)
    assert (dfa.next[:, EMPTY] == -1).all()  # the empty entry is never allowed
    pieces = {}
    for t, v in enumerate(VOCAB[:-2]):
        pieces.setdefault(v, []).append(t)
    rx = re.compile(pattern.encode())
    n_yes = 0
    for n in range(5):
        for s in itertools.product(ALPHABET, repeat=n):
            s = bytes(s)
            want = rx.fullmatch(s) is not None
            n_yes += want
            for toks in _tokenisations(s, pieces):
                assert dfa.accepts(toks + (EOS,)) == want, (pattern, s, toks)
                if want:  # and every prefix is alive, without EOS it is not accepted
                    assert dfa.walk(toks) >= 0 and not dfa.accepts(toks)
    assert n_yes > 0


@pytest.mark.parametrize("pattern,names", [
    (r"^a", "anchor"), (r"a$", "anchor"), (r"a*?", "lazy"), (r"(?=a)b", "group extension"),
    (r"(?P<x>a)", "group extension"), (r"\1", "escape"), (r"\bfoo", "escape"),
    (r"a{2,}", "counted"), (r"a{65}", "64"), (r"a{3,2}", "m <= n"), (r"(a", "unbalanced"),
    (r"a)", "unbalanced"), (r"[a", "unterminated"), (r"*a", "nothing to repeat"),
    (r"[[:alpha:]]", "POSIX"), (r"[z-a]", "reversed"), (r"a++", "possessive")])
def test_unsupported_constructs_are_named(pattern, names):
    with pytest.raises(ValueError, match=names):
        TokenDFA.from_regex(pattern, VOCAB, EOS)


def test_a_dead_end_branch_leaves_no_dead_end_state():
    # without the byte 'c' in any token, the branch "ac" can start and never finish
    vocab = [bytes([i]) if i != ord("c") else b"" for i in range(256)] + [b"ab", b"<eos>"]
    eos = len(vocab) - 1
    dfa = TokenDFA.from_regex(r"ac|ab|b", vocab, eos)
    q = dfa.walk([ord("a")])
    assert q >= 0 and sorted(np.flatnonzero(dfa.next[q] >= 0)) == [ord("b")]
    assert dfa.accepts([256, eos]) and dfa.accepts([ord("b"), eos])
    # a branch that can only die is cut at its first token
    dfa = TokenDFA.from_regex(r"cc|b", vocab, eos)
    assert sorted(np.flatnonzero(dfa.next[dfa.start] >= 0)) == [ord("b")]
    for s in range(dfa.n_states):  # the constructor's own guarantee, spelled out
        assert (dfa.next[s] >= 0).any()
    with pytest.raises(ValueError, match="no token sequence"):
        TokenDFA.from_regex(r"c+", vocab, eos)


def test_byte_dfa_directly_and_its_errors():
    trans = np.full((3, 256), -1)
    trans[0, ord("a")] = 1
    trans[1, ord("b")] = 2
    trans[2, ord("a")] = 1  # (ab)+
    dfa = TokenDFA.from_byte_dfa(VOCAB, trans, 0, [2], EOS)
    ab, abab = 256 + MULTI.index(b"ab"), 256 + MULTI.index(b"abab")
    assert dfa.accepts([ab, EOS]) and dfa.accepts([abab, ord("a"), ord("b"), EOS])
    assert not dfa.accepts([ord("a"), EOS]) and dfa.walk([256 + MULTI.index(b"ba")]) == -1
    with pytest.raises(ValueError):
        TokenDFA.from_byte_dfa(VOCAB, trans[:, :255], 0, [2], EOS)
    with pytest.raises(ValueError):
        TokenDFA.from_byte_dfa(VOCAB, trans + 5, 0, [2], EOS)
    with pytest.raises(ValueError):
        TokenDFA.from_byte_dfa(VOCAB, trans, 3, [2], EOS)
    with pytest.raises(ValueError):
        TokenDFA.from_byte_dfa(VOCAB, trans, 0, [7], EOS)


def test_byte_dfa_is_vectorised_over_a_real_vocabulary():
    rng = np.random.default_rng(0)
    V = 50257
    vocab = [bytes([i]) for i in range(256)] + \
        [bytes(rng.integers(97, 123, size=rng.integers(2, 9)).tolist()) for _ in range(V - 257)]
    vocab.append(b"<eos>")
    trans, start, acc = regex_to_byte_dfa(r"([a-z]{1,8} ){0,22}[a-z]{1,8}\.")
    assert 195 <= trans.shape[0] <= 215  # Q about 200
    t0 = time.perf_counter()
    dfa = TokenDFA.from_byte_dfa(vocab, trans, start, acc, V - 1)
    took = time.perf_counter() - t0
    print(f"from_byte_dfa: Q {trans.shape[0]}, V {V}: {took:.2f} s")
    assert took < 5  # "a few seconds"
    assert dfa.vocab_size == V and dfa.table().shape == (dfa.n_states, padded_vocab(V))
    word = [300, 301, ord(" "), 5000, ord("."), V - 1]
    assert dfa.accepts(word) == (len(vocab[300]) + len(vocab[301]) <= 8)


# ------------------------------------------------------------------------- constructor
def test_constructor_validation_and_pruning():
    EOS = 2
    ok = np.array([[1, -1, -1], [-1, 1, 1]])  # 0 -a-> 1 (accepting, loops on b)
    dfa = TokenDFA(ok, 0, EOS)
    assert dfa.n_states == 2 and dfa.accepts([0, 1, 1, EOS]) and not dfa.accepts([0])
    with pytest.raises(ValueError, match="outside"):
        TokenDFA(np.array([[2, -1, -1], [-1, 1, 1]]), 0, EOS)
    with pytest.raises(ValueError, match="outside"):
        TokenDFA(np.array([[-2, 1, -1], [-1, 1, 1]]), 0, EOS)
    with pytest.raises(ValueError, match="allows no token"):
        TokenDFA(np.array([[1, 2, -1], [-1, 1, 1], [-1, -1, -1]]), 0, EOS)
    with pytest.raises(ValueError, match="cannot reach"):  # state 2 loops for ever
        TokenDFA(np.array([[1, 2, -1], [-1, 1, 1], [2, -1, -1]]), 0, EOS)
    with pytest.raises(ValueError, match="start"):
        TokenDFA(ok, 2, EOS)
    with pytest.raises(ValueError, match="eos_token_id"):
        TokenDFA(ok, 0, 3)
    with pytest.raises(ValueError, match="integer table"):
        TokenDFA(ok.astype(np.float32), 0, EOS)
    # unreachable states (a dead end among them) are dropped, the rest renumbered
    dfa = TokenDFA(np.array([[-1, -1, -1], [2, -1, -1], [-1, 2, 2]]), 1, EOS)
    assert dfa.n_states == 2 and dfa.start == 0 and dfa.accepts([0, 1, EOS])
    t = dfa.table(offset=10)
    assert t.shape == (2, 8) and t.dtype == np.int16 and (t[:, 3:] == -1).all()
    assert t[0, 0] == 11 and t[1, 2] == 11 and t[0, 1] == -1
    with pytest.raises(ValueError, match="int16"):
        dfa.table(offset=32766)


def test_too_many_states():
    Q = 32768  # a chain: token 0 advances, the last state accepts
    nxt = np.full((Q, 2), -1)
    nxt[:-1, 0] = np.arange(1, Q)
    nxt[-1, 1] = Q - 1
    with pytest.raises(ValueError, match="32767"):
        TokenDFA(nxt, 0, 1)
    assert TokenDFA(nxt[1:] - (nxt[1:] >= 0), 0, 1).n_states == Q - 1
