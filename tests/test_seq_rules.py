"""``ref.seq_ban`` and ``ref.stop_check`` (the single definitions of banned sequences, no-repeat
n-grams and stop sequences) against independent scalar implementations, plain Python loops
over lists written from the rules: BIT EQUALITY on the whole logits buffer, exact equality on
every integer output. Then every rule alone on planted values, the boundaries (C < n, C == n
- 1, C == n, a full row, suffixes that straddle two segments), the skip rules and the
wrappers' argument errors (CPU).

``make_case`` / ``make_stop_case`` build the mixed batches the GPU test
(test_seq_rules_gpu.py) shares."""

import numpy as np
import pytest
import torch

from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

INF = float("inf")
Q, ML = rf.SEQ_MAX, rf.SEQ_MAX_LEN
NAMES = ("prompt", "prompt_len", "out", "n_out", "bad", "bad_len", "ngram")
STOP_NAMES = ("out", "n_out", "pos", "stops", "stop_len", "hit")
I32 = torch.int32


# ------------------------------------------------------------------ the scalar implementations
def _bits_of(t):
    """The logits as a numpy array of raw integers."""
    idt = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(idt).numpy().astype(np.int64) & ((1 << (8 * t.element_size())) - 1)


NEG_INF = {torch.bfloat16: 0xFF80, torch.float32: 0xFF800000}


def context_of(c, b):
    """The context of logits row b as a list, or None for a row the skip rules name (a row
    without a rule is not among them here)."""
    R, P = c["prompt"].shape
    cap = c["out"].shape[1]
    r = int(c["rows"][b]) if c.get("rows") is not None else b
    if c.get("active") is not None and not int(c["active"][b]):
        return None
    if not 0 <= r < R:
        return None
    pl, no = int(c["prompt_len"][r]), int(c["n_out"][r])
    ne, W = 0, 0
    if c.get("extra") is not None:
        ne, W = int(c["n_extra"][b]), c["extra"].shape[1]
    if not (0 <= pl <= P and 0 <= no <= cap and 0 <= ne <= W):
        return None
    if not 0 <= int(c["ngram"][r]) <= ML:
        return None
    ctx = c["prompt"][r, :pl].tolist() + c["out"][r, :no].tolist()
    if ne:
        ctx += c["extra"][b, :ne].tolist()
    return ctx


def banned_tokens(ctx, n, bad, bad_len):
    """The set of banned ids for one context: the two rules, as the issue states them."""
    C = len(ctx)
    res = set()
    for q in range(len(bad)):
        L = bad_len[q]
        if not 1 <= L <= ML or L - 1 > C:
            continue
        if ctx[C - (L - 1):] == bad[q][: L - 1]:
            res.add(bad[q][L - 1])
    if n >= 1:
        for i in range(0, C - n + 1):
            if ctx[i: i + n - 1] == ctx[C - n + 1: C]:
                res.add(ctx[i + n - 1])
    return res


def scalar_seq_ban(c, dtype):
    """The expected raw bits [B, Vs] of ``c["logits"]`` after the ban: plain loops."""
    bits = _bits_of(c["logits"]).copy()
    B, Vs = bits.shape
    V = c.get("vocab_size") or Vs
    for b in range(B):
        ctx = context_of(c, b)
        if ctx is None:
            continue
        r = int(c["rows"][b]) if c.get("rows") is not None else b
        for t in banned_tokens(ctx, int(c["ngram"][r]), c["bad"][r].tolist(),
                               c["bad_len"][r].tolist()):
            if 0 <= t < V:
                bits[b, t] = NEG_INF[dtype]
    return bits


def scalar_stop_check(c, max_span=None):
    """The expected ``(n_out, pos, hit, active, lens, done)`` as lists: plain loops."""
    out = c["out"].tolist()
    cap = c["out"].shape[1]
    res = {k: c[k].tolist() for k in ("n_out", "pos", "hit", "active", "lens", "done")}
    for r in range(len(out)):
        n, p = res["n_out"][r], res["pos"][r]
        if not (0 <= n <= cap and 0 <= p <= n):
            continue
        last = n if max_span is None else min(n, p + max_span)
        found = None
        for e in range(p + 1, last + 1):
            for q in range(Q):
                L = int(c["stop_len"][r, q])
                if 1 <= L <= ML and L <= e and out[r][e - L: e] == c["stops"][r, q, :L].tolist():
                    found = (e, q)
                    break
            if found:
                break
        if found:
            res["n_out"][r], res["hit"][r] = found
            res["active"][r], res["lens"][r], res["done"][r] = 0, ref.SLOT_INACTIVE, 1
            res["pos"][r] = found[0]
        else:
            res["pos"][r] = last
    return res


# ------------------------------------------------------------------ the shared cases
def make_case(V, B, seed=0, dtype=torch.bfloat16, width=70, window=5, pad=0):
    """A mixed batch for ``seq_ban`` as CPU tensors: B logits rows over R = B + 3 context rows
    of ``width`` columns. Histories with a period of 3, over six values and over the whole
    vocabulary, some ids negative or >= V; lengths from {0, 1, 2, 7, 33} and one row that fills
    prompt and output; ``ngram`` from {0, 1, 2, 3, 8, 4}; banned lists with a one-token entry,
    entries of 8, 3 and 2 tokens copied from the end of the row's own context (so they match
    and straddle its segments), one that does not match, two with a length out of range and one
    with an id >= V; rows without a rule, rows with a bad length, ``ngram``, ``rows`` index and
    an inactive row; ±inf and NaN patterns planted; ``pad`` more columns of NaN."""
    g = torch.Generator().manual_seed(seed * 7919 + V * 31 + B)
    R, W = B + 3, window

    def rint(lo, hi, shape):
        return torch.randint(lo, hi, shape, generator=g)

    def history(kind, n):
        if kind == 0:
            return (torch.arange(n) % 3 + int(rint(0, max(1, V - 2), (1,)))) % max(V, 3)
        if kind == 1:
            return rint(-1, 5, (n,)) * max(1, V // 6)
        return rint(-2, V + 2, (n,))

    lens = (0, 1, 2, 7, 33)
    prompt = torch.zeros(R, width, dtype=I32)
    out = torch.zeros(R, width, dtype=torch.int64)
    prompt_len = torch.tensor([lens[(r + 1) % 5] for r in range(R)], dtype=I32).clamp(max=width)
    n_out = torch.tensor([lens[(2 * r + 3) % 5] for r in range(R)], dtype=I32).clamp(max=width)
    prompt_len[0], n_out[0] = width, width  # the full row
    for r in range(R):
        prompt[r] = history(r % 3, width).to(I32)
        out[r] = history(r % 3 if r % 2 else (r + 1) % 3, width)
    ngram = torch.tensor([(0, 1, 2, 3, 8, 4)[r % 6] for r in range(R)], dtype=I32)
    rows = torch.arange(B, dtype=I32)
    if B > 1:
        rows = torch.randperm(R, generator=g)[:B].to(I32)
        rows[0] = 0
    active = torch.ones(B, dtype=torch.uint8)
    if B >= 5:
        rows[2], rows[3], active[4] = -1, R, 0
        rows[1] = rows[0]  # two logits rows share a context row
    extra = rint(-1, 5, (B, W)) * max(1, V // 6)
    n_extra = rint(0, W + 1, (B,)).to(I32)
    bad = rint(-1, V + 1, (R, Q, ML)).to(I32)
    bad_len = torch.zeros(R, Q, dtype=I32)
    first = {}
    for b in range(B):
        first.setdefault(int(rows[b]), b)
    for r in range(R):
        if r % 5 == 4:  # no banned sequence (and no rule at all where ngram is 0 too)
            bad_len[r, 1], bad_len[r, 2] = ML + 1, -1
            if r % 2:
                ngram[r] = 0
            continue
        b = first.get(r, 0)
        ctx = torch.cat([prompt[r, : int(prompt_len[r])].long(), out[r, : int(n_out[r])],
                         extra[b, : int(n_extra[b])]])
        bad_len[r, 0], bad[r, 0, 0] = 1, (r * 5) % V
        for q, L in ((1, 8), (2, 3), (7, 2)):  # the context's own end, then some token
            if len(ctx) >= L - 1:
                bad_len[r, q] = L
                bad[r, q, : L - 1] = ctx[len(ctx) - (L - 1):].to(I32)
                bad[r, q, L - 1] = (r * 7 + q) % V
        bad_len[r, 3] = 4  # random tokens: no match
        bad_len[r, 4], bad_len[r, 5] = ML + 1, -1  # unused
        bad_len[r, 6], bad[r, 6, 0] = 1, V  # an id out of range
    if R > 6:
        prompt_len[R - 1], n_out[R - 2], ngram[R - 3] = width + 1, -1, ML + 1
        ngram[R - 4] = -1
    if B >= 5:
        n_extra[B - 1] = W + 1
    x = (torch.randn(B, V, generator=g) * 4).to(dtype)
    idt = {torch.bfloat16: torch.int16, torch.float32: torch.int32}[dtype]
    nan = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA00005}[dtype]
    raw = x.view(idt)
    for b in range(B if V >= 16 else 0):  # NaN patterns, -inf, +inf: some under a ban
        at = rint(0, V, (6,))
        raw[b, at[:3]] = nan
        x[b, at[3]], x[b, at[4]] = INF, -INF
    if pad:
        x = torch.cat([x, torch.full((B, pad), nan, dtype=idt).view(dtype)], 1)
    return dict(logits=x, prompt=prompt, prompt_len=prompt_len, out=out, n_out=n_out, bad=bad,
                bad_len=bad_len, ngram=ngram, rows=rows, extra=extra, n_extra=n_extra,
                active=active, vocab_size=V)


def call(fn, c, logits=None):
    """``fn`` (``ref.seq_ban`` or ``rf.seq_ban``) on the case, IN PLACE on ``logits`` (default:
    a copy of the case's); returns the edited tensor."""
    x = c["logits"].clone() if logits is None else logits
    fn(x, *(c[k] for k in NAMES), rows=c.get("rows"), extra=c.get("extra"),
       n_extra=c.get("n_extra"), active=c.get("active"), vocab_size=c.get("vocab_size"))
    return x


def skipped_rows(c):
    """The logits rows that must keep their bytes, by the skip rules (rows without a rule
    among them)."""
    res = []
    for b in range(c["logits"].shape[0]):
        if context_of(c, b) is None:
            res.append(b)
            continue
        r = int(c["rows"][b])
        if int(c["ngram"][r]) == 0 and not any(1 <= L <= ML for L in c["bad_len"][r].tolist()):
            res.append(b)
    return res


def make_stop_case(R, seed=0, cap=40):
    """A mixed batch for ``stop_check``: outputs over five values (matches are common), spans
    ``n_out - pos`` of 0, 1, 9 and more, stop lists with lengths 0..8, two unused lengths, an
    entry copied from the row's own output so that it ends inside the span, a duplicate of it
    at a higher q, rows without stops, rows with ``n_out`` / ``pos`` out of range, and random
    ``active`` / ``lens`` / ``done`` (never read)."""
    g = torch.Generator().manual_seed(seed * 104729 + R)

    def rint(lo, hi, shape):
        return torch.randint(lo, hi, shape, generator=g)

    out = rint(0, 5, (R, cap))
    n_out = rint(0, cap + 1, (R,)).to(I32)
    span = torch.tensor([(1, 9, 0, 3, 40)[r % 5] for r in range(R)], dtype=I32)
    pos = (n_out - span).clamp(min=0)
    stops = rint(0, 5, (R, Q, ML)).to(I32)
    stop_len = torch.zeros(R, Q, dtype=I32)
    for r in range(R):
        if r % 4 == 3:
            continue  # no stops
        for q in range(Q):
            stop_len[r, q] = (3, 8, 0, 5, ML + 1, 2, -1, 4)[(q + r) % 8]
        n, p = int(n_out[r]), int(pos[r])
        if r % 3 == 0 and n > p:  # plant: ends at e inside the span, may begin before pos
            e = int(rint(p + 1, n + 1, (1,)))
            L = min(e, (2, 4, 8)[r % 3 if r % 9 else 2])
            for q in (5, 2):  # the same sequence twice: the lowest q wins
                stop_len[r, q] = L
                stops[r, q, :L] = out[r, e - L: e].to(I32)
    if R >= 5:
        n_out[R - 1], n_out[R - 2] = -1, cap + 1
        pos[R - 3] = -1
        pos[R - 4] = n_out[R - 4] + 1
    return dict(out=out, n_out=n_out, pos=pos, stops=stops, stop_len=stop_len,
                hit=torch.full((R,), -1, dtype=I32), active=rint(0, 2, (R,)).to(torch.uint8),
                lens=rint(0, 100, (R,)).to(I32), done=rint(0, 2, (R,)).to(torch.uint8))


def call_stop(fn, c, max_span=None, optional=True):
    """``fn`` (``ref.stop_check`` or ``rf.stop_check``) on a copy of the case; returns the
    dict of everything it may write."""
    d = {k: v.clone() for k, v in c.items()}
    kw = dict(active=d["active"], lens=d["lens"], done=d["done"]) if optional else {}
    if max_span is not None:
        kw["max_span"] = max_span
    fn(*(d[k] for k in STOP_NAMES), **kw)
    return {k: d[k].tolist() for k in ("n_out", "pos", "hit", "active", "lens", "done")}


# ------------------------------------------------------------------ reference == scalar loops
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,B", [(1, 1), (7, 5), (9, 12), (509, 5), (509, 23), (509, 67),
                                 (50257, 6)])
def test_seq_ban_reference_against_scalar_loops(V, B, dtype):
    c = make_case(V, B, dtype=dtype, pad=3)
    want = scalar_seq_ban(c, dtype)
    got = call(ref.seq_ban, c)
    assert got.dtype == dtype
    assert np.array_equal(_bits_of(got), want)
    before = _bits_of(c["logits"])
    assert np.array_equal(want[:, V:], before[:, V:])  # the NaN padding keeps its bytes
    skipped = skipped_rows(c)
    assert np.array_equal(want[skipped], before[skipped])
    if B == 67:
        assert len(skipped) >= 5
        assert (want != before).any(1).sum() > (B - len(skipped)) // 2
        assert int(c["prompt_len"][0]) == 70 and int(c["n_out"][0]) == 70


@pytest.mark.parametrize("max_span", [None, 0, 1, 4])
@pytest.mark.parametrize("R", [1, 5, 23, 67])
def test_stop_check_reference_against_scalar_loops(R, max_span):
    for seed in range(3):
        c = make_stop_case(R, seed)
        want = scalar_stop_check(c, max_span)
        assert call_stop(ref.stop_check, c, max_span) == want
        # without the optional outputs the others are the same
        bare = call_stop(ref.stop_check, c, max_span, optional=False)
        for k in ("n_out", "pos", "hit"):
            assert bare[k] == want[k]
        for k in ("active", "lens", "done"):
            assert bare[k] == c[k].tolist()
    if R == 67 and max_span is None:
        hits = sum(h >= 0 for h in want["hit"])
        assert 5 <= hits < R


# ------------------------------------------------------------------ seq_ban on planted values
def _ban(prompt, out, extra=None, ngram=0, bad=(), V=16, dtype=torch.float32, **kw):
    """One logits row of zeros over one context row; returns the case."""
    P, cap = max(len(prompt), 1) + 1, max(len(out), 1) + 1
    c = dict(logits=torch.zeros(1, V, dtype=dtype),
             prompt=torch.tensor([list(prompt) + [3] * (P - len(prompt))], dtype=I32),
             prompt_len=torch.tensor([len(prompt)], dtype=I32),
             out=torch.tensor([list(out) + [3] * (cap - len(out))]),
             n_out=torch.tensor([len(out)], dtype=I32),
             bad=torch.zeros(1, Q, ML, dtype=I32), bad_len=torch.zeros(1, Q, dtype=I32),
             ngram=torch.tensor([ngram], dtype=I32))
    for q, seq in enumerate(bad):
        c["bad"][0, q, : len(seq)] = torch.tensor(seq, dtype=I32)
        c["bad_len"][0, q] = len(seq)
    if extra is not None:
        c["extra"] = torch.tensor([list(extra) + [3]])
        c["n_extra"] = torch.tensor([len(extra)], dtype=I32)
    c.update(kw)
    return c


def _banned(c):
    """The banned ids of the single row, after checking the reference against the loops."""
    got = call(ref.seq_ban, c)
    assert np.array_equal(_bits_of(got), scalar_seq_ban(c, c["logits"].dtype))
    return sorted(torch.nonzero(got[0] == -INF).flatten().tolist())


def test_no_repeat_boundaries_and_segments():
    # n = 3 (the Hugging Face example): 1 2 3 1 2 -> 3
    assert _banned(_ban([1, 2, 3], [1, 2], ngram=3)) == [3]
    assert _banned(_ban([1, 2], [], ngram=3)) == []          # C == n - 1
    assert _banned(_ban([1], [], ngram=3)) == []             # C < n
    assert _banned(_ban([], [], ngram=3)) == []              # C == 0
    assert _banned(_ban([2, 2, 2], [], ngram=3)) == [2]      # C == n: one candidate, i = 0
    assert _banned(_ban([1, 2, 1], [], ngram=3)) == []       # C == n, no match
    # the suffix straddles prompt/out, then out/extra; the candidate straddles them too
    assert _banned(_ban([5, 6, 7, 5], [6], ngram=3)) == [7]
    assert _banned(_ban([5], [6, 7, 5], [6], ngram=3)) == [7]
    assert _banned(_ban([], [5, 6], [7, 5, 6], ngram=3)) == [7]
    assert _banned(_ban([5, 6, 7], [], [5, 6], ngram=3)) == [7]
    # several candidates ban several tokens; the last n-gram's own start is a candidate
    assert _banned(_ban([1, 2, 4, 1, 2, 5], [1, 2], ngram=3)) == [4, 5]
    assert _banned(_ban([9, 9], [9], ngram=2)) == [9]
    # n = 1 bans every context token; n = 8 needs seven equal tokens
    assert _banned(_ban([1, 5], [7], [2], ngram=1)) == [1, 2, 5, 7]
    seq = [1, 2, 3, 4, 5, 6, 7]
    assert _banned(_ban(seq + [8], seq[:3], seq[3:], ngram=8)) == [8]
    assert _banned(_ban(seq + [8], seq[:3], seq[3:6] + [9], ngram=8)) == []
    assert _banned(_ban(seq, [], ngram=8)) == []             # C == n - 1
    assert _banned(_ban(seq[:6] + seq[:1], [], ngram=2)) == [2]
    # ids below 0 and at or beyond V take part in the compare and are ignored as a ban
    assert _banned(_ban([-1, 16, 4, -1], [16], ngram=3)) == [4]
    assert _banned(_ban([4, -1, 16, 4], [-1], ngram=3)) == []
    assert _banned(_ban([], [2 ** 40, 5, 2 ** 40], ngram=2, V=8)) == [5]
    assert _banned(_ban([], [2 ** 32 + 5, 6, 5], ngram=2, V=8)) == []  # compared whole
    assert _banned(_ban([1, 9], [1], ngram=2, vocab_size=8)) == []


def test_banned_sequences():
    assert _banned(_ban([1], [], bad=[[4]])) == [4]                      # L = 1: always
    assert _banned(_ban([], [], bad=[[4], [4], [6]])) == [4, 6]          # C == 0, a duplicate
    assert _banned(_ban([1, 2], [3], bad=[[2, 3, 9]])) == [9]            # prompt/out
    assert _banned(_ban([1, 2], [3], [5], bad=[[2, 3, 5, 9]])) == [9]    # all three segments
    assert _banned(_ban([1, 2], [3], [5], bad=[[2, 3, 9]])) == []        # not at the end
    assert _banned(_ban([3], [], bad=[[2, 3, 9]])) == []                 # L - 1 > C
    assert _banned(_ban([2, 3], [], bad=[[2, 3, 9]])) == [9]             # L - 1 == C
    seq = [1, 2, 3, 4, 5, 6, 7]
    assert _banned(_ban(seq[:2], seq[2:5], seq[5:], bad=[seq + [8]])) == [8]  # L = 8
    assert _banned(_ban(seq[:2], seq[2:5], [6, 6], bad=[seq + [8]])) == []
    assert _banned(_ban([1], [], bad=[[16], [-1], [1, 16]])) == []       # ids out of range
    # a length out of range makes the entry unused; the others still act
    c = _ban([1], [], bad=[[4], [5], [6]])
    c["bad_len"][0, 0], c["bad_len"][0, 1] = ML + 1, -1
    assert _banned(c) == [6]
    # both rules together
    assert _banned(_ban([1, 2, 3, 1], [2], ngram=3, bad=[[1, 2, 7], [2, 8]])) == [3, 7, 8]


def test_seq_ban_skipped_rows_keep_nan_bytes_and_the_rest_of_the_row():
    u8 = torch.uint8
    for kw, kept in ((dict(active=torch.zeros(1, dtype=u8)), True),
                     (dict(rows=torch.tensor([1], dtype=I32)), True),
                     (dict(rows=torch.tensor([-1], dtype=I32)), True),
                     (dict(n_out=torch.tensor([9], dtype=I32)), True),
                     (dict(n_out=torch.tensor([-1], dtype=I32)), True),
                     (dict(prompt_len=torch.tensor([-1], dtype=I32)), True),
                     (dict(prompt_len=torch.tensor([9], dtype=I32)), True),
                     (dict(n_extra=torch.tensor([3], dtype=I32)), True),
                     (dict(n_extra=torch.tensor([-1], dtype=I32)), True),
                     (dict(ngram=torch.tensor([9], dtype=I32)), True),
                     (dict(ngram=torch.tensor([-1], dtype=I32)), True),
                     (dict(ngram=torch.tensor([0], dtype=I32),
                           bad_len=torch.zeros(1, Q, dtype=I32)), True),
                     (dict(), False)):
        c = _ban([1, 2], [1], [2], ngram=2, bad=[[4]], dtype=torch.bfloat16)
        c.update(kw)
        raw = c["logits"].view(torch.int16)
        raw[0, 1], raw[0, 4], raw[0, 5] = 0x7FA5, 0x7FA5, 0x7FA5
        got = call(ref.seq_ban, c).view(torch.int16)[0].tolist()
        assert np.array_equal(_bits_of(call(ref.seq_ban, c)), scalar_seq_ban(c, torch.bfloat16))
        assert got[5] == 0x7FA5  # no rule names token 5
        want = raw[0].tolist()
        if not kept:  # context 1 2 1 2: token 1 repeats the 2-gram, token 4 is banned
            want[1], want[4] = -128, -128  # 0xFF80
        assert got == want, kw


# ------------------------------------------------------------------ stop_check on planted values
def _stop(out, n_out, pos, stops, cap=12, **kw):
    c = dict(out=torch.tensor([list(out) + [0] * (cap - len(out))]),
             n_out=torch.tensor([n_out], dtype=I32), pos=torch.tensor([pos], dtype=I32),
             stops=torch.zeros(1, Q, ML, dtype=I32), stop_len=torch.zeros(1, Q, dtype=I32),
             hit=torch.tensor([-1], dtype=I32), active=torch.ones(1, dtype=torch.uint8),
             lens=torch.tensor([17], dtype=I32), done=torch.zeros(1, dtype=torch.uint8))
    for q, seq in stops.items():
        c["stops"][0, q, : len(seq)] = torch.tensor(seq, dtype=I32)
        c["stop_len"][0, q] = len(seq)
    c.update(kw)
    return c


def _stopped(c, max_span=None):
    got = call_stop(ref.stop_check, c, max_span)
    assert got == scalar_stop_check(c, max_span)
    return tuple(got[k][0] for k in ("n_out", "pos", "hit", "active", "lens", "done"))


def test_stop_check_rules():
    OFF, out = ref.SLOT_INACTIVE, [1, 2, 3, 4, 5, 6, 7, 8, 9, 1]
    miss = (10, 10, -1, 1, 17, 0)
    assert _stopped(_stop(out, 10, 9, {0: [9, 1]})) == (10, 10, 0, 0, OFF, 1)  # span 1
    assert _stopped(_stop(out, 10, 9, {0: [9, 2]})) == miss
    assert _stopped(_stop(out, 10, 1, {3: [4, 5]})) == (5, 5, 3, 0, OFF, 1)    # span 9
    # a match may begin before pos, but its end must be new
    assert _stopped(_stop(out, 10, 4, {0: [3, 4, 5]})) == (5, 5, 0, 0, OFF, 1)
    assert _stopped(_stop(out, 10, 5, {0: [3, 4, 5]})) == miss
    # a sequence longer than e is no match, even where the bytes before the row would fit
    assert _stopped(_stop([2, 3], 2, 0, {0: [0, 2, 3]})) == (2, 2, -1, 1, 17, 0)
    assert _stopped(_stop([2, 3], 2, 0, {0: [2, 3]})) == (2, 2, 0, 0, OFF, 1)
    # two sequences end at the same e: the lowest q; two ends in one span: the earliest
    assert _stopped(_stop(out, 10, 0, {5: [3], 2: [2, 3], 7: [1, 2, 3]})) == (3, 3, 2, 0, OFF, 1)
    assert _stopped(_stop(out, 10, 2, {1: [7, 8], 4: [5]})) == (5, 5, 4, 0, OFF, 1)
    assert _stopped(_stop(out, 10, 0, {0: [1]})) == (1, 1, 0, 0, OFF, 1)  # out[9] is later
    # the longest sequence; tokens are compared whole (int64 against int32)
    assert _stopped(_stop(out, 10, 7, {6: out[1:9]})) == (9, 9, 6, 0, OFF, 1)
    assert _stopped(_stop([2 ** 32 + 5], 1, 0, {0: [5]})) == (1, 1, -1, 1, 17, 0)
    # no stops, and pos == n_out: nothing but pos moves
    assert _stopped(_stop(out, 10, 3, {})) == miss
    assert _stopped(_stop(out, 7, 7, {0: [7]})) == (7, 7, -1, 1, 17, 0)
    # a length out of range is unused
    c = _stop(out, 10, 0, {0: [1], 1: [2]})
    c["stop_len"][0, 0], c["stop_len"][0, 1] = ML + 1, -1
    assert _stopped(c) == miss
    # rows out of range have nothing written
    for n, p in ((-1, 0), (13, 0), (5, -1), (5, 6)):
        assert _stopped(_stop(out, n, p, {0: [1]})) == (n, p, -1, 1, 17, 0)
    # active and done are never read: a row that is already retired is still cut
    c = _stop(out, 10, 6, {0: [8]}, active=torch.zeros(1, dtype=torch.uint8),
              done=torch.ones(1, dtype=torch.uint8), lens=torch.tensor([OFF], dtype=I32))
    assert _stopped(c) == (8, 8, 0, 0, OFF, 1)
    # max_span: pos advances as far as was checked
    assert _stopped(_stop(out, 10, 1, {0: [6]}), max_span=3) == (10, 4, -1, 1, 17, 0)
    assert _stopped(_stop(out, 10, 1, {0: [4]}), max_span=3) == (4, 4, 0, 0, OFF, 1)
    assert _stopped(_stop(out, 10, 1, {0: [2]}), max_span=0) == (10, 1, -1, 1, 17, 0)


# ------------------------------------------------------------------ the wrappers
def test_wrappers_use_the_reference_on_the_cpu_and_return_their_arguments():
    assert (rf.SEQ_MAX, rf.SEQ_MAX_LEN) == (8, 8)
    c = make_case(509, 9)
    x = c["logits"].clone()
    assert call(rf.seq_ban, c, x) is x
    assert np.array_equal(_bits_of(x), _bits_of(call(ref.seq_ban, c)))
    # a column slice of a wider buffer is edited in place, the rest keeps its bytes
    wide = torch.full((9, 640), float("nan"), dtype=torch.bfloat16)
    wide[:, 3: 512] = c["logits"]
    call(rf.seq_ban, c, wide[:, 3: 512])
    assert np.array_equal(_bits_of(wide[:, 3: 512]), _bits_of(x))
    assert wide[:, :3].isnan().all() and wide[:, 512:].isnan().all()
    s = make_stop_case(9)
    assert call_stop(rf.stop_check, s) == call_stop(ref.stop_check, s)
    d = {k: v.clone() for k, v in s.items()}
    res = rf.stop_check(*(d[k] for k in STOP_NAMES))
    assert res[0] is d["n_out"] and res[1] is d["pos"] and res[2] is d["hit"]


def test_seq_ban_argument_errors():
    c = make_case(9, 5)
    args = [c["logits"].clone()] + [c[k] for k in NAMES]
    kw = dict(rows=c["rows"], extra=c["extra"], n_extra=c["n_extra"], active=c["active"])
    rf.seq_ban(*args, **kw)  # the base call is fine

    def bad_args(i, t):
        a = list(args)
        a[i] = t
        with pytest.raises(ValueError):
            rf.seq_ban(*a, **kw)

    bad_args(0, args[0][0])  # not 2-D
    bad_args(0, torch.zeros(5, 9, dtype=I32))
    for i, t in enumerate(args[1:], 1):
        bad_args(i, t.to(torch.float64))  # dtype
        bad_args(i, t[:-1])  # rows
        bad_args(i, t.tolist())  # not a tensor
    bad_args(1, args[1][0])
    bad_args(3, args[3].to(I32))
    bad_args(5, args[5][:, :-1])  # fewer than SEQ_MAX sequences
    bad_args(5, args[5][:, :, :-1])
    bad_args(6, args[6][:, :-1])
    for name, t in (("rows", c["rows"][:-1]), ("rows", c["rows"].long()),
                    ("active", c["active"].bool()), ("active", c["active"][:-1]),
                    ("extra", c["extra"].to(I32)), ("extra", c["extra"][:-1]),
                    ("n_extra", c["n_extra"].long()), ("n_extra", None), ("extra", None),
                    ("vocab_size", 10), ("vocab_size", 0)):
        with pytest.raises(ValueError):
            rf.seq_ban(*args, **{**kw, name: t})
    with pytest.raises(ValueError):  # fewer context rows than logits rows, and no ``rows``
        rf.seq_ban(args[0], *(t[:3] for t in args[1:]), **{**kw, "rows": None})


def test_stop_check_argument_errors():
    c = make_stop_case(5)
    args = [c[k].clone() for k in STOP_NAMES]
    kw = dict(active=c["active"].clone(), lens=c["lens"].clone(), done=c["done"].clone())
    rf.stop_check(*args, **kw)

    def bad_args(i, t):
        a = list(args)
        a[i] = t
        with pytest.raises(ValueError):
            rf.stop_check(*a, **kw)

    for i, t in enumerate(args):
        bad_args(i, t.to(torch.float64))
        bad_args(i, t[:-1])
        bad_args(i, t.tolist())
    bad_args(0, args[0][0])
    bad_args(0, args[0][:, :0])
    bad_args(3, args[3][:, :-1])
    bad_args(4, args[4][:, :-1])
    bad_args(1, torch.zeros(10, dtype=I32)[::2])  # written in place: contiguous
    for name, t in (("active", c["active"].bool()), ("active", c["active"][:-1]),
                    ("lens", c["lens"].long()), ("done", c["done"].to(I32)),
                    ("max_span", -1), ("max_span", 1.5), ("max_span", True)):
        with pytest.raises(ValueError):
            rf.stop_check(*args, **{**kw, name: t})
