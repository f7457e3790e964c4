"""Continuous batching (models/gpt2_engine.py) on the CPU in fp32: the slot ops'
semantics, and the guarantee that a request's tokens are those of ``generate`` on that
request alone, whenever it was admitted, in whichever slot, whoever shared its steps."""

import collections
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import functional as rf

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
INACTIVE = -(1 << 30)

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
assert sum(m[1] for m in MIX) == 158


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(11)
    return GPT2(CFG).eval()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, CFG.vocab_size, (m[0],), generator=g).tolist() for m in MIX]


@pytest.fixture(scope="module")
def expected(model, prompts):
    """Every request through ``generate`` alone, computed once."""
    return [model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3], top_p=m[4],
                           seeds=[m[5]])[0].tolist() for p, m in zip(prompts, MIX)]


def _engine(model, **kw):
    """Polls after every device step unless the test says otherwise: the step counts and
    the schedules below are stated in device steps."""
    kw.setdefault("poll_every", 1)
    return GPT2Engine(model, **kw)


def _cut(toks, eos):
    return toks[: toks.index(eos) + 1] if eos is not None and eos in toks else toks


def _submit(eng, prompts, i):
    m = MIX[i]
    return eng.submit(prompts[i], m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5])


def _drive(eng, prompts, arrivals):
    """Submits request i when ``eng.steps`` has reached ``arrivals[i]``; returns the
    tokens per request index and the raw events."""
    pending = sorted(range(len(MIX)), key=lambda i: (arrivals[i], i))
    rid_of, got, events = {}, collections.defaultdict(list), []
    while pending or eng.has_work():
        while pending and (arrivals[pending[0]] <= eng.steps or not eng.has_work()):
            i = pending.pop(0)
            rid_of[_submit(eng, prompts, i)] = i
        for rid, new, fin in eng.step():
            events.append((rid_of[rid], new, fin))
            got[rid_of[rid]].extend(new)
    return [got[i] for i in range(len(MIX))], events


SCHEDULES = {
    "s3_all_at_once": (3, [0] * 9),
    "s4_staggered": (4, [0, 0, 2, 2, 5, 5, 6, 6, 60]),  # the last long after the others
    "s1": (1, [0] * 9),
}


# ------------------------------------------------------------------ the two ops
def test_kv_insert_semantics():
    g = torch.Generator().manual_seed(0)
    Bn, Tp, H, D, S, Tmax = 5, 12, 2, 4, 4, 9
    qkv = torch.randn(Bn, Tp, 3, H, D, generator=g)
    k0 = torch.randn(S, H, Tmax, D, generator=g)
    v0 = torch.randn(S, H, Tmax, D, generator=g)
    k0[0, 0, 3] = float("nan")
    slots = torch.tensor([2, -1, 0, 4, 3], dtype=torch.int32)  # -1 and S: skipped
    lens = torch.tensor([5, 3, 0, 4, 40], dtype=torch.int32)   # 0: nothing; 40: clamps to 9
    k, v = k0.clone(), v0.clone()
    assert rf.kv_insert(qkv, k, v, slots, lens) is None
    wk, wv = k0.clone(), v0.clone()
    for b, s, n in ((0, 2, 5), (4, 3, 9)):
        wk[s, :, :n] = qkv[b, :n, 1].transpose(0, 1)
        wv[s, :, :n] = qkv[b, :n, 2].transpose(0, 1)
    assert torch.equal(k.view(torch.int32), wk.view(torch.int32))
    assert torch.equal(v.view(torch.int32), wv.view(torch.int32))
    # Tp < Tmax clamps to Tp
    k, v = k0.clone(), v0.clone()
    rf.kv_insert(qkv[:1, :3], k, v, torch.tensor([1], dtype=torch.int32),
                 torch.tensor([7], dtype=torch.int32))
    wk = k0.clone()
    wk[1, :, :3] = qkv[0, :3, 1].transpose(0, 1)
    assert torch.equal(k.view(torch.int32), wk.view(torch.int32))
    with pytest.raises(ValueError):
        rf.kv_insert(qkv, k, v, slots.long(), lens)
    with pytest.raises(ValueError):
        rf.kv_insert(qkv[:, :, :2], k, v, slots, lens)
    with pytest.raises(ValueError):
        rf.kv_insert(qkv, k, v[:, :1], slots, lens)


def test_slot_advance_semantics():
    assert rf.SLOT_INACTIVE == INACTIVE
    S, cap, eos = 5, 3, 9
    # slot 0: retires by count (max_new 2); 1: by EOS at its 2nd token; 2: idle throughout;
    # 3: max_new 10 > cap 3, stopped by the cap guard; 4: runs 3 tokens, retires by count
    lens = torch.tensor([4, 7, 50, 1, 2], dtype=torch.int32)
    n_out = torch.zeros(S, dtype=torch.int32)
    max_new = torch.tensor([2, 8, 5, 10, 3], dtype=torch.int32)
    active = torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8)
    out = torch.full((S, cap), -7, dtype=torch.int64)
    toks = [[1, 2, 3, 4, 5], [6, 9, 8, 1, 2], [3, 3, 3, 3, 3], [4, 4, 4, 4, 4]]
    want_active = [[1, 1, 0, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0]]
    want_n = [[1, 1, 0, 1, 1], [2, 2, 0, 2, 2], [2, 2, 0, 3, 3], [2, 2, 0, 3, 3]]
    want_lens = [[4, 7, INACTIVE, 1, 2], [INACTIVE, INACTIVE, INACTIVE, 2, 3],
                 [INACTIVE, INACTIVE, INACTIVE, 3, INACTIVE], [INACTIVE] * 5]
    for c in range(4):
        rf.slot_advance(torch.tensor(toks[c]), lens, n_out, max_new, active, out, eos)
        assert active.tolist() == want_active[c], c
        assert n_out.tolist() == want_n[c], c
        assert lens.tolist() == want_lens[c], c  # idle slots re-pinned on every call
        lens += 1  # what decode_step does
    assert out.tolist() == [[1, 6, -7], [2, 9, -7], [-7, -7, -7], [4, 1, 3], [5, 2, 3]]
    # without EOS slot 1 would have gone on
    lens = torch.tensor([7], dtype=torch.int32)
    n_out = torch.zeros(1, dtype=torch.int32)
    active = torch.ones(1, dtype=torch.uint8)
    out = torch.zeros(1, 4, dtype=torch.int64)
    for t in (6, 9, 8):
        rf.slot_advance(torch.tensor([t]), lens, n_out, torch.tensor([8], dtype=torch.int32),
                        active, out)
    assert out.tolist() == [[6, 9, 8, 0]] and active.tolist() == [1] and lens.tolist() == [7]
    with pytest.raises(ValueError):
        rf.slot_advance(torch.tensor([1]), lens.long(), n_out, n_out, active, out)
    with pytest.raises(ValueError):
        rf.slot_advance(torch.tensor([1]), lens, n_out, n_out, active.bool(), out)
    with pytest.raises(ValueError):
        rf.slot_advance(torch.tensor([1]), lens, n_out, n_out, active, out[0])


# ------------------------------------------------------------------ engine == generate alone
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_engine_matches_generate_alone(model, prompts, expected, schedule):
    S, arrivals = SCHEDULES[schedule]
    eng = _engine(model, slots=S)
    got, events = _drive(eng, prompts, arrivals)
    assert got == expected
    if schedule == "s1":
        assert eng.steps == sum(m[1] for m in MIX)  # admission and retirement cost no step
        assert [i for i, _, fin in events if fin] == list(range(len(MIX)))  # FIFO
    # events: finished exactly once, as the request's last event
    for i in range(len(MIX)):
        fins = [fin for j, _, fin in events if j == i]
        assert fins.count(True) == 1 and fins[-1]
    assert not eng.has_work() and eng.num_active == 0 and eng.num_queued == 0


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_engine_matches_generate_alone_with_eos(model, prompts, expected, schedule):
    interior = collections.Counter(t for e in expected for t in e[:-1])
    eos = interior.most_common(1)[0][0]
    want = [_cut(e, eos) for e in expected]
    assert sum(len(w) < len(e) for w, e in zip(want, expected)) >= 1  # some request hits it
    S, arrivals = SCHEDULES[schedule]
    eng = _engine(model, slots=S, eos_token_id=eos)
    got, _ = _drive(eng, prompts, arrivals)
    assert got == want
    if schedule == "s1":
        assert eng.steps == sum(len(w) for w in want)


def test_steps_when_everything_fits(model, prompts, expected):
    eng = _engine(model, slots=len(MIX))
    rids = [_submit(eng, prompts, i) for i in range(len(MIX))]
    assert eng.num_queued == len(MIX) and eng.num_active == 0
    got = eng.run()
    assert [got[r] for r in rids] == expected
    assert eng.steps == max(m[1] for m in MIX)


def test_poll_every(model, prompts, expected):
    eng = _engine(model, slots=4, poll_every=5)
    rids = [_submit(eng, prompts, i) for i in range(len(MIX))]
    got = eng.run()
    assert [got[r] for r in rids] == expected
    assert eng.steps % 5 == 0


def test_stale_slot_contents_do_not_matter(model, prompts, expected):
    eng = _engine(model, slots=2)
    eng.cache.k.fill_(float("nan"))
    eng.cache.v.fill_(float("nan"))
    rids = [_submit(eng, prompts, i) for i in range(len(MIX))]
    got = eng.run()
    assert [got[r] for r in rids] == expected


def test_stale_slot_contents_after_finished_requests(model, prompts, expected):
    eng = _engine(model, slots=2)
    first = [_submit(eng, prompts, i) for i in (0, 3)]
    got = eng.run()
    assert [got[r] for r in first] == [expected[0], expected[3]]
    eng.cache.k.fill_(float("nan"))
    eng.cache.v.fill_(float("nan"))
    second = [_submit(eng, prompts, i) for i in (1, 2, 4)]
    got = eng.run()
    assert [got[r] for r in second] == [expected[1], expected[2], expected[4]]


def test_cancel(model, prompts, expected):
    eng = _engine(model, slots=2)
    a, b, c, d = (_submit(eng, prompts, i) for i in (2, 6, 1, 4))  # a, b run; c, d queued
    got = collections.defaultdict(list)
    for _ in range(3):
        for rid, new, _fin in eng.step():
            got[rid].extend(new)
    assert eng.num_active == 2 and eng.num_queued == 2
    assert eng.cancel(c) and eng.cancel(b)  # one queued, one running
    assert not eng.cancel(b)
    assert eng.num_active == 1 and eng.num_queued == 1
    seen_b = list(got[b])
    steps = eng.steps
    while eng.has_work():
        for rid, new, _fin in eng.step():
            got[rid].extend(new)
    assert got[b] == seen_b and c not in got  # nothing more for either
    assert got[a] == expected[2] and got[d] == expected[4]
    # d took b's slot at once: both were done when the longer of them was
    assert eng.steps == max(MIX[2][1], steps + MIX[4][1])


@pytest.mark.parametrize("kwargs", [
    dict(tokens=[]),
    dict(tokens=[1, CFG.vocab_size]),
    dict(tokens=[-1]),
    dict(max_new_tokens=0),
    dict(tokens=[1] * 100, max_new_tokens=29),  # 129 > max_len 128
    dict(temperature=-0.5),
    dict(temperature=float("inf")),
    dict(temperature=float("nan")),
    dict(top_p=0.0),
    dict(top_p=1.5),
    dict(seed=2 ** 64),
    dict(seed=-2 ** 63 - 1),
])
def test_submit_rejections(model, kwargs):
    eng = _engine(model, slots=2)
    args = dict(tokens=[1, 2, 3], max_new_tokens=4)
    args.update(kwargs)
    with pytest.raises(ValueError):
        eng.submit(**args)
    assert eng.num_queued == 0 and not eng.has_work() and eng.step() == []


def test_constructor_checks(model):
    with pytest.raises(ValueError):
        _engine(model, slots=2, graph=True)  # no graphs on the CPU
    with pytest.raises(ValueError):
        _engine(model, slots=0)
    eng = _engine(model, slots=2, max_len=40)
    assert eng.cache.lens.tolist() == [INACTIVE, INACTIVE]
    with pytest.raises(ValueError):
        eng.submit([1] * 30, 11)
    eng.submit([1] * 30, 10)
