"""Per-token log-probabilities on the CPU in fp32: ``reference.token_logprobs`` on planted
rows, ``GPT2.generate(logprobs=n)`` and ``GPT2.score`` against explicit loops, and the
engine's guarantee that a request's logprob entries are those of its own teacher-forced
sequence, whatever the schedule, with EOS, ``cancel``, a prefix, chunked prefill and
speculation."""

import collections
import dataclasses
import math

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
INF = float("inf")

# the request mix and the schedules of test_gpt2_engine.py
# (prompt length, max_new_tokens, temperature, top_k, top_p, seed)
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
SCHEDULES = {
    "s3_all_at_once": (3, [0] * 9),
    "s4_staggered": (4, [0, 0, 2, 2, 5, 5, 6, 6, 60]),
    "s1": (1, [0] * 9),
}
WANTS = [5, 0, 3, None, 5, 1, None, 2, 4]  # each request's logprobs=m (engine N = 5)
PREFIXED = {1: 20, 5: 29}  # request -> the length of its prompt that is a registered prefix


# ------------------------------------------------------------------ the reference
def planted_rows():
    """(logits [B, Vs], tok [B], vocab_size, top_n, want lp, want ids, want top values - lse
    as plain lists): the cases the GPU test runs through the kernel too."""
    x = torch.full((6, 12), -3.0)
    x[0, [2, 5, 9]] = 1.5                      # a three-way tie at the top: 2, 5, 9 in order
    x[0, 7] = 1.0
    x[1, :] = 0.25                             # all equal: index order
    x[2, :] = -INF                             # -inf entries below three finite ones
    x[2, [11, 0, 4]] = torch.tensor([2.0, 2.0, -1.0])
    x[3, 3] = 4.0                              # tok out of range
    x[4, [1, 6]] = torch.tensor([0.0, -0.0])   # -0 ties with +0
    x[5, 10] = 7.0                             # tok holds -inf
    x[5, 0] = -INF
    tok = torch.tensor([7, 11, 3, 12, 6, 0])
    return x, tok


def _lse(vals):
    m = max(vals)
    return m + math.log(sum(math.exp(v - m) for v in vals))


def test_reference_on_planted_rows():
    x, tok = planted_rows()
    lp, ids, tlp = ref.token_logprobs(x, tok, 4)
    assert lp.dtype == torch.float32 and ids.dtype == torch.int32 and tlp.dtype == torch.float32
    assert ids.tolist() == [[2, 5, 9, 7], [0, 1, 2, 3], [0, 11, 4, 1], [3, 0, 1, 2],
                            [1, 6, 0, 2], [10, 1, 2, 3]]
    lses = [_lse(r) for r in x.tolist()]
    assert lp[0].item() == pytest.approx(1.0 - lses[0], abs=1e-6)
    assert lp[1].item() == pytest.approx(-math.log(12), abs=1e-6)
    assert lp[2].item() == -INF            # a -inf logit
    assert math.isnan(lp[3].item())        # tok == V
    assert lp[4].item() == pytest.approx(0.0 - lses[4], abs=1e-6)
    assert lp[5].item() == -INF
    assert tlp[2].tolist()[3] == -INF and ids[2, 3].item() == 1  # the lowest -inf index
    for b in range(6):
        for j in range(4):
            want = x[b, ids[b, j]].item() - lses[b]
            assert tlp[b, j].item() == pytest.approx(want, abs=1e-6) or want == -INF
    # negative tok
    assert math.isnan(ref.token_logprobs(x[:1], torch.tensor([-1]))[0].item())
    # top_n = 0: empty tables
    lp0, ids0, tlp0 = ref.token_logprobs(x, tok, 0)
    assert torch.equal(lp0[:2], lp[:2]) and ids0.shape == (6, 0) and tlp0.shape == (6, 0)


def test_reference_small_vocab_pads():
    x = torch.tensor([[0.5], [2.0]])
    lp, ids, tlp = ref.token_logprobs(x, torch.tensor([0, 0]), 3)  # V = 1
    assert lp.tolist() == [0.0, 0.0]
    assert ids.tolist() == [[0, -1, -1]] * 2
    assert tlp.tolist() == [[0.0, -INF, -INF]] * 2
    x = torch.tensor([[1.0, 3.0, 2.0, 9.0]])
    lp, ids, tlp = ref.token_logprobs(x, torch.tensor([1]), 8, vocab_size=3)  # V < top_n
    lse = _lse([1.0, 3.0, 2.0])
    assert ids.tolist() == [[1, 2, 0, -1, -1, -1, -1, -1]]
    assert tlp[0, :3].tolist() == pytest.approx([3 - lse, 2 - lse, 1 - lse], abs=1e-6)
    assert tlp[0, 3:].tolist() == [-INF] * 5
    assert lp.item() == pytest.approx(3 - lse, abs=1e-6)


def test_reference_ignores_the_tail():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 20, generator=g)
    tok = torch.tensor([0, 9, 13])
    want = ref.token_logprobs(x[:, :14].contiguous(), tok, 5)
    y = x.clone()
    y[:, 14:] = torch.tensor([50.0, float("nan"), INF, 99.0, float("nan"), 1e30])
    got = ref.token_logprobs(y, tok, 5, vocab_size=14)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert math.isnan(ref.token_logprobs(y, torch.tensor([14, 0, 0]), 0, 14)[0][0].item())


def placement_case():
    """``(logits, tok, rows, cols, active, R, cap)``: rows 0 and 3 are written, every other
    row meets one skip condition."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, 33, generator=g)
    tok = torch.tensor([1, 2, 3, 4, 5, 6, 7, 8])
    rows = torch.tensor([2, 1, -1, 0, 3, 1, 1, 0], dtype=torch.int32)    # -1, 3: outside R = 3
    cols = torch.tensor([4, 0, 1, 0, 1, -1, 5, 2], dtype=torch.int32)    # -1, 5: outside cap = 5
    active = torch.tensor([1, 0, 1, 7, 1, 1, 1, 0], dtype=torch.uint8)   # rows 1, 7 inactive
    return x, tok, rows, cols, active, 3, 5


def fresh_tables(R, cap, n, device=None):
    return (torch.full((R, cap), 7.5, device=device),
            torch.full((R, cap, n), 77, dtype=torch.int32, device=device),
            torch.full((R, cap, n), -2.5, device=device))


@pytest.mark.parametrize("n", [0, 3])
def test_reference_placement_and_skips(n):
    x, tok, rows, cols, active, R, cap = placement_case()
    lp, ids, tlp = ref.token_logprobs(x, tok, n)
    out = fresh_tables(R, cap, n)
    assert rf.token_logprobs(x, tok, n, out=out, rows=rows, cols=cols, active=active) is out
    want = fresh_tables(R, cap, n)
    for b, (r, c) in ((0, (2, 4)), (3, (0, 0))):
        want[0][r, c], want[1][r, c], want[2][r, c] = lp[b], ids[b], tlp[b]
    for a, b in zip(out, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # without active: rows 1 and 7 land too
    out = fresh_tables(R, cap, n)
    rf.token_logprobs(x, tok, n, out=out, rows=rows, cols=cols)
    for b, (r, c) in ((1, (1, 0)), (7, (0, 2))):
        want[0][r, c], want[1][r, c], want[2][r, c] = lp[b], ids[b], tlp[b]
    for a, b in zip(out, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_argument_checks():
    x, tok, rows, cols, active, R, cap = placement_case()
    assert rf.LOGPROB_MAX_TOP == 8
    out = fresh_tables(R, cap, 2)
    for bad in (
        lambda: rf.token_logprobs(x[0], tok[:1]),
        lambda: rf.token_logprobs(x, tok, 9),
        lambda: rf.token_logprobs(x, tok, -1),
        lambda: rf.token_logprobs(x, tok, True),
        lambda: rf.token_logprobs(x, tok.int()),
        lambda: rf.token_logprobs(x, tok[:3]),
        lambda: rf.token_logprobs(x, tok, vocab_size=34),
        lambda: rf.token_logprobs(x.long(), tok),
        lambda: rf.token_logprobs(x, tok, 2, rows=rows, cols=cols),          # no out
        lambda: rf.token_logprobs(x, tok, 2, out=out, rows=rows),            # no cols
        lambda: rf.token_logprobs(x, tok, 2, out=out, rows=rows.long(), cols=cols),
        lambda: rf.token_logprobs(x, tok, 3, out=out, rows=rows, cols=cols),  # tables are n = 2
        lambda: rf.token_logprobs(x, tok, 2, out=out[:2], rows=rows, cols=cols),
        lambda: rf.token_logprobs(x, tok, 2, out=(out[0].double(),) + out[1:], rows=rows,
                                  cols=cols),
        lambda: rf.token_logprobs(x, tok, 2, out=(out[0].t(),) + out[1:], rows=rows, cols=cols),
        lambda: rf.token_logprobs(x, tok, 2, out=out, rows=rows, cols=cols,
                                  active=active.bool()),
    ):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------ generate and score
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(11)
    return GPT2(CFG).eval()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, CFG.vocab_size, (m[0],), generator=g).tolist() for m in MIX]


def _loop_logits(model, idx, lens, toks):
    """The logits every token of ``toks`` [B, n] was drawn from, by an explicit prefill +
    decode_step loop: [B, n, V]."""
    B, n = toks.shape
    cache = KVCache(CFG, B, max(lens) + n, idx.device, model.wte.dtype)
    logits = [model.prefill(idx, torch.tensor(lens, dtype=torch.int32), cache)]
    for t in range(n - 1):
        logits.append(model.decode_step(toks[:, t], cache).clone())
    return torch.stack(logits, 1)


@pytest.mark.parametrize("path", ["generator", "seeds"])
def test_generate_logprobs_match_an_explicit_loop(model, path):
    g = torch.Generator().manual_seed(3)
    lens = [9, 4, 13]
    idx = torch.randint(0, CFG.vocab_size, (3, 13), generator=g)
    if path == "generator":
        kw = dict(temperature=0.9, top_k=40)
        rnd = lambda: dict(generator=torch.Generator().manual_seed(8))  # noqa: E731
    else:
        kw = dict(temperature=[0.0, 0.8, 1.3], top_k=[0, 5, 0], top_p=[1.0, 1.0, 0.9])
        rnd = lambda: dict(seeds=[4, 5, 6])  # noqa: E731
    plain = model.generate(idx, 11, lens=lens, **kw, **rnd())
    toks, lp, ids, tlp = model.generate(idx, 11, lens=lens, logprobs=3, **kw, **rnd())
    assert torch.equal(toks, plain)  # the tokens are those of the call without logprobs
    assert lp.shape == (3, 11) and ids.shape == (3, 11, 3) and tlp.shape == (3, 11, 3)
    logits = _loop_logits(model, idx, lens, toks)
    want = ref.token_logprobs(logits.view(33, -1), toks.reshape(33), 3)
    for got, w in zip((lp, ids, tlp), want):
        assert torch.equal(got.reshape(w.shape), w)
    # n = 0: empty tables, the same values; a bad n
    toks0, lp0, ids0, tlp0 = model.generate(idx, 11, lens=lens, logprobs=0, **kw, **rnd())
    assert torch.equal(toks0, plain) and torch.equal(lp0, lp) and ids0.shape == (3, 11, 0)
    for bad in (9, -1, True, 2.0):
        with pytest.raises(ValueError):
            model.generate(idx, 2, logprobs=bad)


def test_generate_logprobs_with_eos(model):
    """A row that has emitted EOS keeps emitting it; its entries describe that token under
    the logits of the step, like every other entry."""
    idx = torch.tensor([[5, 6, 7]])
    plain = model.generate(idx, 8, temperature=1.0, seeds=[1])
    eos = plain[0, 2].item()
    toks, lp, _, _ = model.generate(idx, 8, temperature=1.0, seeds=[1], eos_token_id=eos,
                                    logprobs=1)
    assert toks[0, 2:].tolist() == [eos] * 6 and torch.isfinite(lp).all()


def test_score_against_fp64_log_softmax(model):
    g = torch.Generator().manual_seed(9)
    B, T = 3, 21
    idx = torch.randint(0, CFG.vocab_size, (B, T), generator=g)
    full = torch.log_softmax(model(idx).double(), -1)  # [B, T, V]
    want = torch.full((B, T), float("nan"), dtype=torch.float64)
    want[:, 1:] = full[:, :-1].gather(2, idx[:, 1:].unsqueeze(2)).squeeze(2)
    # fp32 logits carry about 1e-6 of rounding, a wrong position moves a value by order 1
    tol = 1e-4
    lp = model.score(idx)
    assert lp.shape == (B, T) and lp.dtype == torch.float32
    assert torch.isnan(lp[:, 0]).all()
    assert (lp[:, 1:].double() - want[:, 1:]).abs().max().item() < tol
    # ragged, with the top table, in chunks of 8 rows
    lens = [21, 1, 10]
    model.score_chunk = 8
    try:
        lp2, ids, tlp = model.score(idx, lens=lens, top_n=4)
    finally:
        del model.score_chunk
    for b, n in enumerate(lens):
        assert torch.isnan(lp2[b, n:]).all() and torch.isnan(lp2[b, 0])
        assert (ids[b, n:] == -1).all() and (ids[b, 0] == -1).all()
        assert torch.isnan(tlp[b, n:]).all()
        assert torch.equal(lp2[b, 1:n], lp[b, 1:n])  # a row's values do not depend on lens
        top = full[b, : n - 1].topk(4, -1)
        assert torch.equal(ids[b, 1:n].long(), top.indices)
        assert (tlp[b, 1:n].double() - top.values).abs().max().item() < tol if n > 1 else True
    # T = 1: nothing to score
    assert torch.isnan(model.score(idx[:, :1])).all()
    with pytest.raises(ValueError):
        model.score(idx, top_n=9)
    with pytest.raises(ValueError):
        model.score(idx, lens=[1, 2])


# ------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def expected(model, prompts):
    """Every request through ``generate`` alone, computed once."""
    return [model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3], top_p=m[4],
                           seeds=[m[5]])[0].tolist() for p, m in zip(prompts, MIX)]


@pytest.fixture(scope="module")
def eos(expected):
    """A token that ends some requests early: the commonest one past a request's start."""
    seen = collections.Counter(t for e in expected for t in e[1:-1])
    return seen.most_common(1)[0][0]


@pytest.fixture(scope="module")
def yardstick(model, prompts, expected):
    """``ref.token_logprobs`` (top 5) on a teacher-forced fp32 ``forward`` over prompt +
    output, per request: entry t describes ``expected[i][t]``. Computed once, never changed."""
    res = []
    for p, e in zip(prompts, expected):
        logits = model(torch.tensor([p + e]))[0, len(p) - 1: -1]
        res.append(tuple(t.clone() for t in ref.token_logprobs(logits, torch.tensor(e), 5)))
    return res


def _cut(toks, eos):
    return toks[: toks.index(eos) + 1] if eos is not None and eos in toks else toks


class Oracle:
    """test_spec_decode.py's drafter that knows the answers: it holds the full sequences on
    the device, finds each slot's by matching ``hist[:p] + tok0``, proposes the true
    continuation and corrupts draft i wherever ``(p + i) % 5 == 3``. Capturable."""

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


def _submit(eng, prompts, i, pids=None, logprobs=True):
    m = MIX[i]
    toks, pid = prompts[i], None
    if pids and i in pids:
        toks, pid = prompts[i][PREFIXED[i]:], pids[i]
    return eng.submit(toks, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                      prefix=pid, **({"logprobs": WANTS[i]} if logprobs else {}))


def _drive(eng, prompts, arrivals, pids=None, logprobs=True):
    """Submits request i when ``eng.steps`` has reached ``arrivals[i]``; returns per request
    index the tokens and the merged info (None for a request that asked for none)."""
    pending = sorted(range(len(MIX)), key=lambda i: (arrivals[i], i))
    rid_of, got, infos = {}, collections.defaultdict(list), {}
    while pending or eng.has_work():
        while pending and (arrivals[pending[0]] <= eng.steps or not eng.has_work()):
            i = pending.pop(0)
            rid_of[_submit(eng, prompts, i, pids, logprobs)] = i
        for ev in eng.step():
            i = rid_of[ev[0]]
            got[i].extend(ev[1])
            if logprobs:
                assert len(ev) == 4
                if ev[3] is None:
                    assert WANTS[i] is None
                    infos[i] = None
                    continue
                assert sorted(ev[3]) == ["logprobs", "top_ids", "top_logprobs"]
                # aligned with new_tokens
                assert all(len(v) == len(ev[1]) for v in ev[3].values())
                for k, v in ev[3].items():
                    infos.setdefault(i, {"logprobs": [], "top_ids": [],
                                         "top_logprobs": []})[k].extend(v)
    return [got[i] for i in range(len(MIX))], [infos.get(i) for i in range(len(MIX))]


def _check_infos(got, infos, yardstick):
    """Every request's entries against the teacher-forced yardstick, cut to the tokens it
    got (1e-3 absolute: fp32 summation order moves a value by about 1e-5, a wrong position,
    column or token by order 1 on this model) and to its own m."""
    for i, (toks, info) in enumerate(zip(got, infos)):
        m, n = WANTS[i], len(toks)
        if m is None:
            assert info is None
            continue
        lp, ids, tlp = yardstick[i]
        assert len(info["logprobs"]) == n
        assert torch.tensor(info["logprobs"]).sub(lp[:n]).abs().max().item() < 1e-3, i
        assert all(len(r) == m for r in info["top_ids"] + info["top_logprobs"])
        if m:
            assert info["top_ids"] == ids[:n, :m].tolist(), i
            assert torch.tensor(info["top_logprobs"]).sub(tlp[:n, :m]).abs().max().item() < 1e-3
            if MIX[i][2] == 0.0:  # a greedy request's token is the most likely one
                assert [r[0] for r in info["top_ids"]] == toks


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_engine_logprobs_match_teacher_forcing(model, prompts, expected, eos, yardstick,
                                               schedule):
    S, arrivals = SCHEDULES[schedule]
    for end in (None, eos):
        plain = GPT2Engine(model, slots=S, eos_token_id=end, poll_every=3)
        want, _ = _drive(plain, prompts, arrivals, logprobs=False)
        assert want == [_cut(e, end) for e in expected]
        eng = GPT2Engine(model, slots=S, eos_token_id=end, poll_every=3, logprobs=5)
        got, infos = _drive(eng, prompts, arrivals)
        assert got == want  # the tokens of the engine without logprobs
        assert eng.steps == plain.steps
        _check_infos(got, infos, yardstick)
    assert any(len(w) < m[1] for w, m in zip(want, MIX))  # the EOS did cut a request


@pytest.mark.parametrize("k", [0, 4])
def test_engine_logprobs_with_prefix_chunks_and_speculation(model, prompts, expected, eos,
                                                            yardstick, k):
    S, arrivals = SCHEDULES["s4_staggered"]
    sequences = [p + e for p, e in zip(prompts, expected)]
    for oracle in ((False, True) if k else (False,)):
        drafter = Oracle(sequences, k, CFG.n_positions, CFG.vocab_size) if oracle else None
        eng = GPT2Engine(model, slots=S, eos_token_id=eos, poll_every=2, prefix_slots=2,
                         prefill_chunk=7, speculate=k, drafter=drafter, logprobs=5)
        pids = {i: eng.add_prefix(prompts[i][:n]) for i, n in PREFIXED.items()}
        got, infos = _drive(eng, prompts, arrivals, pids)
        assert got == [_cut(e, eos) for e in expected]
        _check_infos(got, infos, yardstick)
        if oracle:
            stats = eng.spec_stats()
            assert 0 < stats["accepted"] < stats["drafted"], stats  # both branches ran


def test_engine_cancel_and_reuse(model, prompts, expected, yardstick):
    eng = GPT2Engine(model, slots=1, poll_every=2, logprobs=5)
    first = _submit(eng, prompts, 2)
    eng.step()
    assert eng.cancel(first)
    rid = _submit(eng, prompts, 4)  # takes over the slot and its tables
    toks, info = eng.run(logprobs=True)[rid]
    assert toks == expected[4]
    lp, ids, _ = yardstick[4]
    assert torch.tensor(info["logprobs"]).sub(lp).abs().max().item() < 1e-3
    assert info["top_ids"] == ids[:, : WANTS[4]].tolist()


def test_run_with_logprobs(model, prompts, expected, yardstick):
    eng = GPT2Engine(model, slots=3, logprobs=2)
    a = eng.submit(prompts[0], 7, logprobs=2)
    b = eng.submit(prompts[4], 21)
    res = eng.run(logprobs=True)
    assert res[a][0] == expected[0] and res[b] == (expected[4], None)
    assert res[a][1]["top_ids"] == yardstick[0][1][:, :2].tolist()
    eng.submit(prompts[0], 7, logprobs=0)
    assert eng.run() == {2: expected[0]}  # without the flag: tokens only


def test_submit_rejections_and_constructor(model, prompts):
    eng = GPT2Engine(model, slots=2, logprobs=3)
    for bad in (4, -1, True, 1.0, "2"):
        with pytest.raises(ValueError):
            eng.submit(prompts[0], 3, logprobs=bad)
    assert not eng.has_work()
    plain = GPT2Engine(model, slots=2)
    with pytest.raises(ValueError):
        plain.submit(prompts[0], 3, logprobs=0)
    with pytest.raises(ValueError):
        plain.run(logprobs=True)
    for bad in (9, -1, True, 2.5):
        with pytest.raises(ValueError):
            GPT2Engine(model, slots=2, logprobs=bad)


def test_logprobs_none_is_the_engine_without_them(model, prompts, expected):
    eng = GPT2Engine(model, slots=3, poll_every=2)
    for name in ("lp_hist", "top_ids_hist", "top_lp_hist", "_lp_out", "_win_rows"):
        assert not hasattr(eng, name)
    rid = eng.submit(prompts[0], 7)
    events = []
    while eng.has_work():
        events.extend(eng.step())
    assert all(len(ev) == 3 for ev in events)
    assert [t for ev in events for t in ev[1]] == expected[0] and events[0][0] == rid
    on = GPT2Engine(model, slots=3, poll_every=2, logprobs=0)
    assert on.lp_hist.shape == (3, CFG.n_positions) and on.top_ids_hist.shape[2] == 0
