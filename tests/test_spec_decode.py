"""Speculative decoding on the CPU in fp32: the semantics of ``ref.spec_draft`` and
``ref.spec_accept`` (ops/csrc/spec.hip) against naive loops, ``GPT2.verify_step`` against
``decode_step`` fed the same tokens one at a time, and the engine with ``speculate=k``: a
request's tokens are those of ``generate`` on it alone for every k, every ``prefill_chunk``,
with prefixes and an EOS, with the n-gram drafter and with an oracle drafter that is right
four times out of five."""

import asyncio
import collections
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.serve.llm import GPT2EngineServer, build_gpt2_app

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
INACTIVE = -(1 << 30)

# (prompt length, max_new_tokens, temperature, top_k, top_p, seed): the mix, the prefixes and
# the schedules of test_gpt2_extend.py
MIX = [
    (1, 7, 0.0, None, None, 3),
    (39, 12, 0.8, 5, None, 11),
    (5, 29, 1.3, 50, 0.9, 2 ** 63 + 5),
    (17, 9, 0.8, None, 0.9, 7),
    (2, 21, 0.0, 5, None, 0),
    (30, 15, 1.3, None, None, -4),
    (11, 26, 0.8, 50, None, 123456789),
    (8, 17, 1.3, 5, 0.9, 42),
    (23, 22, 0.8, None, 1.0, 99),
]
PREFIXED = {1: 20, 3: 16, 5: 29, 8: 1}
SCHEDULES = {
    "s3_all_at_once": (3, [0] * 9),
    "s4_staggered": (4, [0, 0, 2, 2, 5, 5, 6, 6, 60]),
    "s1": (1, [0] * 9),
}


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


# ------------------------------------------------------------------ ref.spec_draft
def _naive_draft(tok0, hist, lens, n_out, max_new, active, k, lo, hi, win):
    """The definition, every candidate j tried; returns (win, n_win) without touching ``win``."""
    S, cap = hist.shape
    win, n_win = win.clone(), torch.zeros(S, dtype=torch.int32)
    for s in range(S):
        p = int(lens[s])
        if not int(active[s]) or p < 0 or p >= cap:
            continue
        seq = [int(t) for t in hist[s, :p]] + [int(tok0[s])]
        L = len(seq)
        win[s, 0] = tok0[s]
        found = None
        for n in range(hi, lo - 1, -1):
            js = [j for j in range(L) if j + n <= L - 1 and seq[j: j + n] == seq[L - n: L]]
            if n <= L - 1 and js:
                found = (max(js), n)
                break
        nd = 0
        if found is not None:
            j, n = found
            room = min(int(max_new[s]) - int(n_out[s]), cap - p)
            nd = max(min(k, room - 1), 0)
            drafts = []
            for i in range(1, nd + 1):
                q = j + n + i - 1
                drafts.append(seq[q] if q < L else drafts[q - L])  # draft q - L + 1, 1-based
            win[s, 1: 1 + nd] = torch.tensor(drafts, dtype=torch.int64)
        n_win[s] = 1 + nd
    return win, n_win


PLANTED_CAP = 16
# (hist[:p], tok0, room = max_new - n_out, active, the window for k 4 and ngram (2, 4))
PLANTED = [
    ([0, 1, 2, 3, 4], 5, 9, 1, [5]),                                # no match
    ([7, 8, 1, 2, 3, 7], 8, 9, 1, [8, 1, 2, 3, 7]),                 # a match only at j = 0
    ([7, 8, 1, 7, 8, 2, 5, 7], 8, 9, 1, [8, 2, 5, 7, 8]),           # two: the later one wins
    ([1, 2, 3, 9, 5, 2, 3, 4, 1, 2], 3, 9, 1, [3, 9, 5, 2, 3]),     # n 3 at j 0 beats n 2 at j 5
    ([4, 6, 6], 6, 9, 1, [6, 6, 6, 6, 6]),                          # period 1: runs on into itself
    ([3, 1, 2, 1], 2, 9, 1, [2, 1, 2, 1, 2]),                       # period 2
    ([7, 8, 1, 2, 3, 7], 8, 1, 1, [8]),                             # room 1
    ([7, 8, 1, 2, 3, 7], 8, 3, 1, [8, 1, 2]),                       # room 3: two drafts
    ([7, 8, 1, 2, 3, 7], 8, 9, 0, None),                            # inactive
    ([7, 8, 1] * 5, 7, 9, 1, [7]),                                  # p = cap - 1: room 1
]


def _planted(cap=PLANTED_CAP):
    S = len(PLANTED)
    g = torch.Generator().manual_seed(2)
    hist = torch.randint(0, 9, (S, cap), generator=g, dtype=torch.int32)  # stale past p
    lens, tok0, n_out, max_new, active = [], [], [], [], []
    for s, (h, t0, room, act, _) in enumerate(PLANTED):
        hist[s, : len(h)] = _i32(h)
        lens.append(len(h))
        tok0.append(t0)
        n_out.append(s)
        max_new.append(s + room)
        active.append(act)
    return (torch.tensor(tok0), hist, _i32(lens), _i32(n_out), _i32(max_new),
            torch.tensor(active, dtype=torch.uint8))


def test_reference_spec_draft_planted_cases():
    args = _planted()
    assert int(args[2][-1]) == PLANTED_CAP - 1
    win0 = torch.full((len(PLANTED), 5), -7, dtype=torch.int64)
    win, n_win = rf.spec_draft(*args, 4, 2, 4, win=win0.clone(),
                               n_win=torch.full((len(PLANTED),), -7, dtype=torch.int32))
    for s, case in enumerate(PLANTED):
        want = case[4]
        if want is None:
            assert int(n_win[s]) == 0 and torch.equal(win[s], win0[s]), s
            continue
        assert int(n_win[s]) == len(want), (s, win[s], n_win[s])
        assert win[s, : len(want)].tolist() == want, s
        assert (win[s, len(want):] == -7).all(), s  # nothing past the window is written
    nw, nn = _naive_draft(*args, 4, 2, 4, win0)
    assert torch.equal(win, nw) and torch.equal(n_win, nn)


def _random_draft_case(seed, cap=48):
    """Histories over a 3-token alphabet at lengths 0, 1, 2, 9, 40 and cap - 1, cap (out of
    range) and -1, with every kind of room, some slots inactive."""
    g = torch.Generator().manual_seed(seed)
    lens = [0, 1, 2, 9, 40] * 4 + [cap - 1, cap, -1, 40, 9]
    S = len(lens)
    hist = torch.randint(0, 3, (S, cap), generator=g, dtype=torch.int32)
    tok0 = torch.randint(0, 3, (S,), generator=g)
    n_out = torch.randint(0, 5, (S,), generator=g, dtype=torch.int32)
    max_new = n_out + torch.randint(-1, 12, (S,), generator=g, dtype=torch.int32)
    max_new[::3] += 20  # room for a full window
    active = torch.ones(S, dtype=torch.uint8)
    active[[7, S - 1]] = 0
    return tok0, hist, _i32(lens), n_out, max_new, active


@pytest.mark.parametrize("ngram", [(1, 1), (2, 4), (3, 8)])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_reference_spec_draft_against_loop(k, ngram):
    seen = collections.Counter()
    for seed in range(3):
        args = _random_draft_case(seed)
        win0 = torch.randint(-9, -1, (args[0].shape[0], k + 1),
                             generator=torch.Generator().manual_seed(seed))
        want_w, want_n = _naive_draft(*args, k, *ngram, win0)
        win, n_win = ref.spec_draft(*args, k, *ngram, win0.clone(),
                                    torch.zeros_like(want_n))
        assert torch.equal(n_win, want_n) and torch.equal(win, want_w)
        seen.update(n_win.tolist())
        # through the public name, allocating its outputs
        w2, n2 = rf.spec_draft(*args, k, *ngram)
        assert torch.equal(n2, want_n)
        for s in range(w2.shape[0]):
            assert torch.equal(w2[s, : int(n2[s])], want_w[s, : int(n2[s])])
    assert seen[0] and seen[1] and seen[k + 1]  # skipped, no draft, a full window


def test_spec_draft_checks():
    args = list(_planted())
    for k, lo, hi in ((0, 2, 4), (9, 2, 4), (4, 0, 4), (4, 3, 2), (4, 2, 9)):
        with pytest.raises(ValueError):
            rf.spec_draft(*args, k, lo, hi)
    with pytest.raises(ValueError):
        rf.spec_draft(args[0].int(), *args[1:], 4)
    with pytest.raises(ValueError):
        rf.spec_draft(args[0], args[1].long(), *args[2:], 4)
    with pytest.raises(ValueError):
        rf.spec_draft(*args[:2], args[2][:-1], *args[3:], 4)
    with pytest.raises(ValueError):
        rf.spec_draft(*args, 4, win=torch.zeros(len(PLANTED), 4, dtype=torch.int64))


# ------------------------------------------------------------------ ref.spec_accept
ACC_K, ACC_CAP, ACC_VP, ACC_EOS = 4, 12, 8, 99


def _accept_case():
    """One slot per line: (win, n_win, cand, n_out, max_new, lens, active), k = 4."""
    w = [10, 11, 12, 13, 14]
    rows = []
    for a in range(ACC_K + 1):  # every a: the first a drafts agree, draft a + 1 does not
        rows.append((w, 5, w[1: 1 + a] + [50] * (5 - a), 0, 9, 3, 1))
    rows += [
        (w, 3, w[1:] + [50], 2, 9, 3, 1),                   # n_win stops a at 2
        ([ACC_EOS, 11, 12, 13, 14], 5, w[1:] + [50], 0, 9, 3, 1),          # EOS as tok0
        ([10, 11, ACC_EOS, 13, 14], 5, [11, ACC_EOS, 13, 14, 50], 1, 9, 3, 1),  # accepted EOS
        ([10, 11, ACC_EOS, 13, 14], 5, [11, 40, 13, 14, 50], 1, 9, 3, 1),  # a rejected EOS
        (w, 5, w[1:] + [50], 4, 6, 3, 1),                   # max_new cuts inside the run: m 2
        (w, 5, w[1:] + [50], 4, 9, 3, 1),                   # ... and exactly at its end: m 5
        (w, 0, w[1:] + [50], 1, 9, 3, 1),                   # n_win 0 on an active slot
        (w, ACC_K + 2, w[1:] + [50], 1, 9, 3, 1),           # n_win k + 2
        (w, 5, w[1:] + [50], 1, 9, 3, 0),                   # inactive
        (w, 5, w[1:] + [50], 1, 9, INACTIVE, 0),            # inactive and pinned already
        (w, 5, w[1:] + [50], ACC_CAP, 99, 3, 1),            # n_out = cap
        (w, 5, w[1:] + [50], -1, 9, 3, 1),                  # n_out < 0
        (w, 5, w[1:] + [50], 0, 9, ACC_CAP, 1),             # lens = cap
        (w, 5, w[1:] + [50], ACC_CAP - 2, 99, 3, 1),        # cap - n_out cuts: m 2
        (w, 5, w[1:] + [50], 0, 99, ACC_CAP - 3, 1),        # cap - lens cuts: m 3
        (w, 1, [50] * 5, 0, 9, 3, 1),                       # no drafts: the plain step
    ]
    S = len(rows)
    g = torch.Generator().manual_seed(4)
    col = lambda i, dt: torch.tensor([r[i] for r in rows], dtype=dt)  # noqa: E731
    return dict(
        win=col(0, torch.int64), n_win=col(1, torch.int32), cand=col(2, torch.int64),
        logits_win=torch.randn(S, ACC_K + 1, ACC_VP, generator=g),
        lens=col(5, torch.int32), n_out=col(3, torch.int32), max_new=col(4, torch.int32),
        active=col(6, torch.uint8),
        out=torch.randint(-9, -1, (S, ACC_CAP), generator=g),
        hist=torch.randint(-9, -1, (S, ACC_CAP), generator=g, dtype=torch.int32),
        buf=torch.randn(S, ACC_VP, generator=g),
        n_drafted=torch.arange(S, dtype=torch.int32),
        n_accepted=torch.arange(S, dtype=torch.int32) * 2)
    # rows 0..4: a = 0..4


ACC_ORDER = ("win", "n_win", "cand", "logits_win", "lens", "n_out", "max_new", "active", "out",
             "hist", "buf", "n_drafted", "n_accepted")
# the number of tokens each slot of _accept_case emits (None: no write at all)
ACC_M = [1, 2, 3, 4, 5, 3, 1, 3, 2, 2, 5, None, None, None, None, None, None, None, 2, 3, 1]
ACC_STAYS = [1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1]


def _naive_accept(c, eos):
    """The definition, slot by slot, on a copy of the case."""
    c = {k: v.clone() for k, v in c.items()}
    S, W = c["win"].shape
    cap = c["out"].shape[1]
    for s in range(S):
        if not int(c["active"][s]):
            c["lens"][s] = INACTIVE
            continue
        nw, n, p, mx = (int(c[k][s]) for k in ("n_win", "n_out", "lens", "max_new"))
        if not (1 <= nw <= W and 0 <= n < cap and 0 <= p < cap):
            c["active"][s], c["lens"][s] = 0, INACTIVE
            continue
        a = 0
        for j in range(1, nw):
            if int(c["win"][s, j]) != int(c["cand"][s, j - 1]):
                break
            a = j
        emitted = []
        for t in c["win"][s, : a + 1].tolist():
            if len(emitted) >= max(1, min(mx - n, cap - n, cap - p)):
                break
            emitted.append(t)
            if t == eos:
                break
        m = len(emitted)
        for i, t in enumerate(emitted):
            c["out"][s, n + i] = t
            c["hist"][s, p + i] = t
        c["n_out"][s] += m
        c["lens"][s] += m
        c["n_drafted"][s] += nw - 1
        c["n_accepted"][s] += m - 1
        if emitted[-1] == eos or n + m >= mx:
            c["active"][s], c["lens"][s] = 0, INACTIVE
        else:
            c["buf"][s] = c["logits_win"][s, m - 1]
    return c


def test_reference_spec_accept_against_loop():
    c0 = _accept_case()
    want = _naive_accept(c0, ACC_EOS)
    got = {k: v.clone() for k, v in c0.items()}
    assert rf.spec_accept(*(got[k] for k in ACC_ORDER), eos_token_id=ACC_EOS) is None
    for k in ACC_ORDER:
        a, b = got[k], want[k]
        if a.is_floating_point():
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k
    assert len(ACC_M) == len(ACC_STAYS) == c0["win"].shape[0]
    for s, (m, stays) in enumerate(zip(ACC_M, ACC_STAYS)):
        assert int(got["active"][s]) == stays, s
        if not stays:
            assert int(got["lens"][s]) == INACTIVE, s
        keeps_buf = torch.equal(got["buf"][s].view(torch.int32), c0["buf"][s].view(torch.int32))
        if m is None:  # no write: out, hist, buf and the counts keep their bits
            for k in ("out", "hist", "n_out", "n_drafted", "n_accepted"):
                assert torch.equal(got[k][s], c0[k][s]), (s, k)
            assert keeps_buf, s
            continue
        n, p = int(c0["n_out"][s]), int(c0["lens"][s])
        assert int(got["n_out"][s]) == n + m, s
        assert got["out"][s, n: n + m].tolist() == c0["win"][s, :m].tolist(), s
        assert got["hist"][s, p: p + m].tolist() == c0["win"][s, :m].tolist(), s
        assert torch.equal(got["out"][s, n + m:], c0["out"][s, n + m:]), s
        assert int(got["n_accepted"][s]) == 2 * s + m - 1, s
        assert int(got["n_drafted"][s]) == s + int(c0["n_win"][s]) - 1, s
        if stays:
            assert int(got["lens"][s]) == p + m, s
            assert torch.equal(got["buf"][s].view(torch.int32),
                               c0["logits_win"][s, m - 1].view(torch.int32)), s
        else:
            assert keeps_buf, s
    # without an EOS the three EOS slots run on
    got = {k: v.clone() for k, v in c0.items()}
    rf.spec_accept(*(got[k] for k in ACC_ORDER))
    want = _naive_accept(c0, -1)
    assert torch.equal(got["n_out"], want["n_out"]) and torch.equal(got["active"], want["active"])
    assert got["n_out"][6:9].tolist() == [5, 6, 3] and got["active"][6:9].tolist() == [1, 1, 1]


def test_spec_accept_checks():
    c = _accept_case()
    args = [c[k] for k in ACC_ORDER]
    for i, bad in ((0, c["win"].int()), (2, c["cand"][:, :4]), (3, c["logits_win"][:, :4]),
                   (4, c["lens"].long()), (9, c["hist"][:, :5]), (10, c["buf"][:, :4]),
                   (7, c["active"].bool())):
        broken = list(args)
        broken[i] = bad
        with pytest.raises(ValueError):
            rf.spec_accept(*broken)


# ------------------------------------------------------------------ verify_step
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(11)
    return GPT2(CFG).eval()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, CFG.vocab_size, (m[0],), generator=g).tolist() for m in MIX]


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_verify_step_matches_decode_steps(model):
    g = torch.Generator().manual_seed(6)
    plens, n_win, W, Tmax = [5, 17, 9, 12], [5, 3, 0, 4], 5, 40
    ps = [torch.randint(0, CFG.vocab_size, (n,), generator=g).tolist() for n in plens]
    win = torch.randint(0, CFG.vocab_size, (4, W), generator=g)
    cache = KVCache(CFG, 4, Tmax)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    for s, p in enumerate(ps):
        model.prefill_into(torch.tensor([p]), [len(p)], cache, _i32([s]))
    cache.lens[3] = INACTIVE  # an idle slot with a window: nothing happens to it
    lens0, k0, v0 = cache.lens.clone(), cache.k.clone(), cache.v.clone()
    out = torch.full((4, W, CFG.padded_vocab), float("nan"))
    got = model.verify_step(win, _i32(n_win), cache, out=out)
    assert got.shape == (4, W, CFG.vocab_size) and got.data_ptr() == out.data_ptr()
    assert torch.equal(cache.lens, lens0)  # the accept kernel advances it, not the model
    for s in (0, 1):
        one = KVCache(CFG, 1, Tmax)
        model.prefill_into(torch.tensor([ps[s]]), [plens[s]], one, _i32([0]))
        for i in range(n_win[s]):
            want = model.decode_step(win[s, i: i + 1], one)
            assert _rel(got[s, i], want[0]) < 1e-4, (s, i)
        end = plens[s] + n_win[s]
        assert _rel(cache.k[:, s, :, :end], one.k[:, 0, :, :end]) < 1e-4
        assert _rel(cache.v[:, s, :, :end], one.v[:, 0, :, :end]) < 1e-4
        assert torch.isnan(cache.k[:, s, :, end:]).all()
        assert torch.isnan(cache.v[:, s, :, end:]).all()
    for s in (2, 3):  # n_win 0 and the idle slot: every bit as it was
        assert torch.equal(cache.k[:, s].view(torch.int32), k0[:, s].view(torch.int32))
        assert torch.equal(cache.v[:, s].view(torch.int32), v0[:, s].view(torch.int32))
    # without out: the same logits
    cache.k.copy_(k0)
    cache.v.copy_(v0)
    again = model.verify_step(win, _i32(n_win), cache)
    assert torch.equal(again[:2], got[:2])
    with pytest.raises(ValueError):
        model.verify_step(win[:3], _i32(n_win), cache)
    with pytest.raises(ValueError):
        model.verify_step(win, torch.tensor(n_win), cache)


# ------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def expected(model, prompts):
    """Every request through ``generate`` on its whole prompt alone, computed once."""
    return [model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3], top_p=m[4],
                           seeds=[m[5]])[0].tolist() for p, m in zip(prompts, MIX)]


@pytest.fixture(scope="module")
def eos(expected):
    """A token that ends some requests early: the commonest one past a request's start."""
    seen = collections.Counter(t for e in expected for t in e[1:-1])
    return seen.most_common(1)[0][0]


def _cut(tokens, eos):
    return tokens if eos is None or eos not in tokens else tokens[: tokens.index(eos) + 1]


class Oracle:
    """A drafter that knows the answers: it holds the full sequences (prompt + expected
    tokens) on the device, finds each slot's by matching ``hist[:p] + tok0`` against them,
    proposes the true continuation and corrupts draft i wherever ``(p + i) % 5 == 3``. torch
    ops only and no host read, so it is capturable."""

    def __init__(self, sequences, k, cap, vocab, device=None):
        self.k, self.vocab = k, vocab
        full = torch.full((len(sequences), cap + k + 1), -1, dtype=torch.int64)
        for r, seq in enumerate(sequences):
            full[r, : len(seq)] = torch.tensor(seq)
        self.full = full.to(device)
        self.pos = torch.arange(cap, device=device)
        self.ahead = torch.arange(1, k + 1, device=device)

    def __call__(self, tok0, hist, lens, n_out, max_new, active):
        S, cap = hist.shape
        ok = (active != 0) & (lens >= 0) & (lens < cap)
        p = lens.long().clamp(0, cap - 1)
        seq = hist.long().scatter(1, p.unsqueeze(1), tok0.unsqueeze(1))
        same = (seq.unsqueeze(1) == self.full[:, :cap].unsqueeze(0)) | \
            (self.pos.view(1, 1, cap) > p.view(S, 1, 1))
        known = same.all(-1)  # [S, R]
        idx = p.unsqueeze(1) + self.ahead  # the drafts' positions p + i
        drafts = self.full[known.long().argmax(1)].gather(1, idx)
        drafts = torch.where(idx % 5 == 3, (drafts + 1) % self.vocab, drafts)
        room = torch.minimum(max_new - n_out, cap - lens)
        nd = torch.where(known.any(1), (room - 1).clamp(0, self.k), torch.zeros_like(room))
        n_win = torch.where(ok, 1 + nd, torch.zeros_like(nd)).to(torch.int32)
        return torch.cat([tok0.unsqueeze(1), drafts], 1), n_win


def _engine(model, **kw):
    kw.setdefault("poll_every", 1)
    kw.setdefault("prefix_slots", len(PREFIXED))
    return GPT2Engine(model, **kw)


def _submit(eng, prompts, i, pids=None):
    m = MIX[i]
    toks, pid = prompts[i], None
    if pids is not None and i in PREFIXED:
        toks, pid = prompts[i][PREFIXED[i]:], pids[i]
    return eng.submit(toks, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                      prefix=pid)


def _drive(eng, prompts, arrivals, pids):
    pending = sorted(range(len(MIX)), key=lambda i: (arrivals[i], i))
    rid_of, got, events = {}, collections.defaultdict(list), []
    while pending or eng.has_work():
        while pending and (arrivals[pending[0]] <= eng.steps or not eng.has_work()):
            i = pending.pop(0)
            rid_of[_submit(eng, prompts, i, pids)] = i
        for rid, new, fin in eng.step():
            events.append((rid_of[rid], new, fin))
            got[rid_of[rid]].extend(new)
    return [got[i] for i in range(len(MIX))], events


@pytest.mark.parametrize("chunk", [None, 7])
@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_speculative_engine_matches_generate_alone(model, prompts, expected, eos, schedule, k,
                                                   chunk):
    S, arrivals = SCHEDULES[schedule]
    sequences = [p + e for p, e in zip(prompts, expected)]
    for oracle in (False, True):
        for end in (None, eos):
            drafter = Oracle(sequences, k, CFG.n_positions, CFG.vocab_size) if oracle else None
            eng = _engine(model, slots=S, prefill_chunk=chunk, speculate=k, drafter=drafter,
                          eos_token_id=end, poll_every=1 if oracle else 2)
            pids = {i: eng.add_prefix(prompts[i][:n]) for i, n in PREFIXED.items()}
            got, events = _drive(eng, prompts, arrivals, pids)
            want = [_cut(e, end) for e in expected]
            assert got == want, (oracle, end)
            for i in range(len(MIX)):
                fins = [fin for j, _, fin in events if j == i]
                assert fins.count(True) == 1 and fins[-1]
            assert not eng.has_work() and eng.num_active == 0 and eng.num_filling == 0
            stats = eng.spec_stats()
            assert stats["accepted"] <= stats["drafted"]
            if oracle:
                # four drafts in five are right and the fifth is wrong: some are accepted,
                # not all are, and a request needs fewer device steps than tokens
                assert 0 < stats["accepted"] < stats["drafted"], stats
                if schedule == "s1" and end is None:
                    assert eng.steps < sum(m[1] for m in MIX)
                    assert sum(len(g) for g in got) == sum(m[1] for m in MIX)
    if end is not None:
        assert any(len(w) < m[1] for w, m in zip(want, MIX))  # the EOS did cut a request


def test_oracle_acceptance_is_what_was_planted(model, prompts, expected):
    """One request, k = 4, no corrupted position inside its first windows: the accept rule
    takes exactly the drafts up to the first wrong one (an off-by-one here changes
    ``steps``)."""
    i, k = 2, 4  # prompt 5, 29 new tokens: positions 5 .. 33
    eng = GPT2Engine(model, slots=1, poll_every=1, speculate=k,
                     drafter=Oracle([prompts[i] + expected[i]], k, CFG.n_positions,
                                    CFG.vocab_size))
    _submit(eng, prompts, i)
    sizes = [len(new) for _, new, _ in iter(lambda: (eng.step() or [None])[0], None)]
    # tok0 at p, drafts at p + 1 .. p + 4, cut before the first position = 3 (mod 5) and at
    # max_new: p = 5: 5 6 7 | p = 8: 8 9 10 11 12 | p = 13: 13 14 15 16 17 | ...
    want, p, end = [], 5, 5 + 29
    while p < end:
        m = 1
        while m <= k and (p + m) % 5 != 3 and p + m < end:
            m += 1
        want.append(m)
        p += m
    assert sizes == want and eng.steps == len(want)
    assert eng.spec_stats()["accepted"] == 29 - len(want)


def test_speculate_zero_is_the_engine_without_it(model, prompts, expected):
    plain = GPT2Engine(model, slots=3, poll_every=2)
    zero = GPT2Engine(model, slots=3, poll_every=2, speculate=0, ngram=(1, 8))
    for eng in (plain, zero):
        rids = [_submit(eng, prompts, i) for i in range(len(MIX))]
        got = eng.run()
        assert [got[r] for r in rids] == expected
        assert not hasattr(eng, "hist") and not hasattr(eng, "logits_win")
        assert eng.spec_stats() == {"drafted": 0, "accepted": 0}
    assert plain.steps == zero.steps
    assert zero._ar.shape == plain._ar.shape  # noqa: SLF001  (the poll is as wide as it was)


def test_cancel_and_reuse_with_speculation(model, prompts, expected):
    eng = GPT2Engine(model, slots=1, poll_every=1, speculate=4, ngram=(1, 3))
    a = _submit(eng, prompts, 6)
    b = _submit(eng, prompts, 4)
    eng.step()
    assert eng.cancel(a) and not eng.cancel(a)
    assert eng.run() == {b: expected[4]}  # the slot's stale history does not reach b


def test_adapters_reach_the_verify_pass(prompts):
    """Requests on two adapters and on the base model share speculative steps: each gets the
    tokens of ``generate(..., adapters=[its adapter])`` on it alone."""
    from ray_amd.models.lora import LoRAStack, target_dims

    torch.manual_seed(11)
    m = GPT2(CFG).eval()
    stack = LoRAStack(CFG, 2, 4)
    g = torch.Generator().manual_seed(1)
    for i in range(2):
        state = {}
        for layer in range(CFG.n_layer):
            for t, (din, dout) in target_dims(CFG).items():
                state[f"h.{layer}.{t}.lora_A"] = torch.randn(4, din, generator=g) * 0.2
                state[f"h.{layer}.{t}.lora_B"] = torch.randn(dout, 4, generator=g) * 0.2
        stack.load(i, state, alpha=8.0)
    m.attach_lora(stack)
    rows = [(1, 0), (2, None), (4, 1), (6, 0)]  # (request of MIX, adapter)
    want = []
    for i, ad in rows:
        mx = MIX[i]
        want.append(m.generate(torch.tensor([prompts[i]]), mx[1], temperature=mx[2], top_k=mx[3],
                               top_p=mx[4], seeds=[mx[5]],
                               adapters=[-1 if ad is None else ad])[0].tolist())
    for drafter in (None, Oracle([prompts[i] + w for (i, _), w in zip(rows, want)], 4,
                                 CFG.n_positions, CFG.vocab_size)):
        eng = GPT2Engine(m, slots=3, poll_every=1, lora=stack, speculate=4, ngram=(1, 3),
                         drafter=drafter)
        rids = [eng.submit(prompts[i], MIX[i][1], temperature=MIX[i][2], top_k=MIX[i][3],
                           top_p=MIX[i][4], seed=MIX[i][5], adapter=ad) for i, ad in rows]
        got = eng.run()
        assert [got[r] for r in rids] == want
    assert eng.spec_stats()["accepted"] > 0


def test_constructor_checks(model):
    for kw in ({"speculate": -1}, {"speculate": 9}, {"speculate": 2.0}, {"speculate": True},
               {"speculate": 2, "ngram": (0, 4)}, {"speculate": 2, "ngram": (3, 2)},
               {"speculate": 2, "ngram": (2, 9)}, {"speculate": 2, "ngram": 3},
               {"ngram": (0, 4)}, {"drafter": lambda *a: None},
               {"speculate": 0, "drafter": lambda *a: None}):
        with pytest.raises(ValueError):
            GPT2Engine(model, slots=2, **kw)
    eng = GPT2Engine(model, slots=2, speculate=8, ngram=(1, 8))
    assert eng.hist.shape == (2, CFG.n_positions) and eng.win.shape == (2, 9)
    assert eng.logits_win.shape == (2, 9, CFG.padded_vocab)


# ------------------------------------------------------------------ serving
SEED = 11
REQUESTS = [
    {"prefix": "sys", "tokens": [5, 17, 300, 42, 8], "max_new_tokens": 12},
    {"prefix": "sys", "tokens": [7], "max_new_tokens": 9, "temperature": 0.8, "top_k": 20,
     "seed": 5},
    {"tokens": [3, 1, 4, 1, 5, 3, 1, 4], "max_new_tokens": 20, "temperature": 1.2, "top_p": 0.9},
    {"tokens": [9, 8, 7], "max_new_tokens": 6},
]
SYS = list(range(100, 137))


def test_serve_round_trip_with_speculation():
    torch.manual_seed(SEED)
    m = GPT2(CFG).eval()
    want = []
    for r in REQUESTS:
        toks = (SYS if "prefix" in r else []) + r["tokens"]
        want.append(m.generate(torch.tensor([toks]), r["max_new_tokens"],
                               temperature=r.get("temperature", 0.0), top_k=r.get("top_k"),
                               top_p=r.get("top_p"), seeds=[r.get("seed", SEED)])[0].tolist())
    app = build_gpt2_app(CFG, seed=SEED, continuous=True, slots=2, device="cpu",
                         prefixes={"sys": SYS}, prefill_chunk=8, speculate=4, ngram=(1, 3))
    assert app.deployment.func_or_class is GPT2EngineServer
    srv = GPT2EngineServer(*app.args, **app.kwargs)
    try:
        assert srv.engine.speculate == 4 and srv.engine.ngram == (1, 3)

        async def streamed(r):
            chunks = [c async for c in srv.stream(r)]
            assert chunks[-1].get("finished")
            return [t for c in chunks for t in c["tokens"]]

        async def calls():
            return await asyncio.gather(*(srv(r) for r in REQUESTS),
                                        *(streamed(r) for r in REQUESTS))

        got = asyncio.run(calls())
        assert got[:4] == [{"tokens": w} for w in want] and got[4:] == want
        assert not srv.engine.has_work()
    finally:
        srv.close()


def test_speculate_needs_the_continuous_app():
    with pytest.raises(ValueError):
        build_gpt2_app(CFG, speculate=4)
    with pytest.raises(ValueError):
        GPT2EngineServer(CFG, seed=SEED, slots=1, device="cpu", speculate=9)
    with pytest.raises(ValueError):
        GPT2EngineServer(CFG, seed=SEED, slots=1, device="cpu", speculate=2, ngram=(4, 2))
