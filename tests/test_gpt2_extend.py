"""Extending cached sequences on the CPU in fp32: the semantics of ``ref.attn_extend`` and
``ref.kv_copy`` against naive loops, ``GPT2.extend_into`` against ``prefill_into``, and the
engine's shared prefixes and chunked prefill (models/gpt2_engine.py): a request's tokens are
those of ``generate`` on its whole prompt alone for every ``prefill_chunk``, with or
without a prefix, under every schedule."""

import collections
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
INACTIVE = -(1 << 30)

# (prompt length, max_new_tokens, temperature, top_k, top_p, seed): the mix of
# test_gpt2_engine.py
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
# requests submitted as (prefix = the first k tokens, continuation = the rest)
PREFIXED = {1: 20, 3: 16, 5: 29, 8: 1}
SCHEDULES = {
    "s3_all_at_once": (3, [0] * 9),
    "s4_staggered": (4, [0, 0, 2, 2, 5, 5, 6, 6, 60]),
    "s1": (1, [0] * 9),
}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ ref.attn_extend
def _naive_extend(qkv, k, v, slots, base, n_new, scale):
    """The definition, one query at a time; returns (out, k, v) without touching its inputs."""
    Bn, Tn, _, H, D = qkv.shape
    S, _, Tmax, _ = k.shape
    k, v = k.clone(), v.clone()
    out = torch.zeros(Bn, Tn, H, D)
    for b in range(Bn):
        s, b0, n = int(slots[b]), int(base[b]), int(n_new[b])
        if not (0 <= s < S and b0 >= 0 and 1 <= n <= Tn and b0 + n <= Tmax):
            continue
        for i in range(n):
            k[s, :, b0 + i] = qkv[b, i, 1]
            v[s, :, b0 + i] = qkv[b, i, 2]
        for i in range(n):
            for h in range(H):
                kk, vv = k[s, h, : b0 + i + 1], v[s, h, : b0 + i + 1]
                p = torch.softmax((kk @ qkv[b, i, 0, h]) * scale, 0)
                out[b, i, h] = p @ vv
    return out, k, v


def _extend_case(seed=0):
    g = torch.Generator().manual_seed(seed)
    Tn, H, D, S, Tmax = 6, 2, 8, 6, 19
    #        active  active(exact fit)  slot -1  slot S  base -1  n 0  n > Tn  base+n = Tmax+1
    slots = [4, 1, -1, S, 2, 3, 0, 5, 2]
    base = [3, Tmax - 5, 2, 2, -1, 4, 1, Tmax - 3, 0]
    n_new = [6, 5, 3, 3, 2, 0, Tn + 1, 4, 1]  # the last row: base 0, one token, active
    Bn = len(slots)
    qkv = torch.randn(Bn, Tn, 3, H, D, generator=g)
    k = torch.randn(S, H, Tmax, D, generator=g)
    v = torch.randn(S, H, Tmax, D, generator=g)
    # NaN past each slot's cached positions: an active row's, and everything of the idle ones
    cached = {4: 3, 1: Tmax - 5, 2: 0}
    for s in range(S):
        k[s, :, cached.get(s, 0):] = float("nan")
        v[s, :, cached.get(s, 0):] = float("nan")
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    return qkv, k, v, i32(slots), i32(base), i32(n_new)


def test_reference_attn_extend_against_loop():
    qkv, k0, v0, slots, base, n_new = _extend_case()
    D = qkv.shape[-1]
    want, wk, wv = _naive_extend(qkv, k0, v0, slots, base, n_new, D ** -0.5)
    k, v = k0.clone(), v0.clone()
    out = rf.attn_extend(qkv, k, v, slots, base, n_new)  # CPU tensors: the reference
    assert out.shape == want.shape and torch.isfinite(out).all()
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-6)
    active = [0, 1, 8]
    for b in range(qkv.shape[0]):
        n = int(n_new[b]) if b in active else 0
        assert (out[b, n:] == 0).all(), b
    # the caches: the appended positions bitwise, every other element its old bits (NaNs too)
    assert torch.equal(_bits(k), _bits(wk)) and torch.equal(_bits(v), _bits(wv))
    changed = _bits(k) != _bits(k0)
    where = torch.zeros_like(changed)
    for b in active:
        s, b0, n = int(slots[b]), int(base[b]), int(n_new[b])
        where[s, :, b0: b0 + n] = True
        assert torch.equal(k[s, :, b0: b0 + n], qkv[b, :n, 1].transpose(0, 1))
        assert torch.equal(v[s, :, b0: b0 + n], qkv[b, :n, 2].transpose(0, 1))
    assert not (changed & ~where).any()
    # base 0, one token: the output is the new V itself
    assert torch.equal(out[8, 0], qkv[8, 0, 2])
    # the same through the reference's own name and with an explicit scale
    k2, v2 = k0.clone(), v0.clone()
    same = ref.attn_extend(qkv, k2, v2, slots, base, n_new, D ** -0.5)
    assert torch.equal(same, out) and torch.equal(_bits(k2), _bits(k))


def test_attn_extend_checks():
    qkv, k, v, slots, base, n_new = _extend_case()
    with pytest.raises(ValueError):
        rf.attn_extend(qkv, k, v, slots.long(), base, n_new)
    with pytest.raises(ValueError):
        rf.attn_extend(qkv, k, v, slots, base[:-1], n_new)
    with pytest.raises(ValueError):
        rf.attn_extend(qkv[:, :, :2], k, v, slots, base, n_new)
    with pytest.raises(ValueError):
        rf.attn_extend(qkv, k, v[:, :1], slots, base, n_new)
    with pytest.raises(ValueError):
        rf.attn_extend(qkv, k, v, slots, base, n_new, scale=0.0)
    with pytest.raises(RuntimeError):
        rf.attn_extend(qkv.clone().requires_grad_(), k, v, slots, base, n_new)


# ------------------------------------------------------------------ ref.kv_copy
def test_reference_kv_copy_against_loop():
    g = torch.Generator().manual_seed(1)
    L, P, S, H, D, Tsrc, Tdst = 2, 3, 5, 2, 4, 11, 9
    sk = torch.randn(L, P, H, Tsrc, D, generator=g)
    sv = torch.randn(L, P, H, Tsrc, D, generator=g)
    dk0 = torch.randn(L, S, H, Tdst, D, generator=g)
    dv0 = torch.randn(L, S, H, Tdst, D, generator=g)
    dk0[:, 3] = float("nan")
    sk[:, 1, :, 7:] = float("nan")
    #           ok  ok(len 0)  src -1  src P  dst -1  dst S  len -1  len > min(Tsrc, Tdst)  exact fit
    src_rows = [1, 0, -1, P, 0, 0, 2, 2, 2]
    dst_rows = [3, 0, 1, 1, -1, S, 1, 1, 4]
    lens = [7, 0, 2, 2, 2, 2, -1, Tdst + 1, Tdst]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    wk, wv = dk0.clone(), dv0.clone()
    for b in (0, 8):
        wk[:, dst_rows[b], :, : lens[b]] = sk[:, src_rows[b], :, : lens[b]]
        wv[:, dst_rows[b], :, : lens[b]] = sv[:, src_rows[b], :, : lens[b]]
    dk, dv = dk0.clone(), dv0.clone()
    assert rf.kv_copy(sk, sv, dk, dv, i32(src_rows), i32(dst_rows), i32(lens)) is None
    assert torch.equal(_bits(dk), _bits(wk)) and torch.equal(_bits(dv), _bits(wv))
    assert torch.isfinite(dk[:, 3, :, :7]).all() and torch.isnan(dk[:, 3, :, 7:]).all()
    # the wider destination: Tsrc < Tdst
    dk, dv = dk0.clone(), dv0.clone()
    rf.kv_copy(dk0[:, :, :, :4].contiguous(), dv0[:, :, :, :4].contiguous(), dk, dv,
               i32([0, 1]), i32([2, 4]), i32([4, 5]))  # 5 > Tsrc 4: skipped
    wk = dk0.clone()
    wk[:, 2, :, :4] = dk0[:, 0, :, :4]
    assert torch.equal(_bits(dk), _bits(wk))
    with pytest.raises(ValueError):
        rf.kv_copy(sk, sv, dk, dv, i32([0]).long(), i32([0]), i32([1]))
    with pytest.raises(ValueError):
        rf.kv_copy(sk, sv[:, :, :1], dk, dv, i32([0]), i32([0]), i32([1]))
    with pytest.raises(ValueError):
        rf.kv_copy(sk[:1], sv[:1], dk, dv, i32([0]), i32([0]), i32([1]))


# ------------------------------------------------------------------ extend_into
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


def _whole(model, prompt, S=1, slot=0, max_len=64):
    cache = KVCache(CFG, S, max_len)
    logits = model.prefill_into(torch.tensor([prompt]), [len(prompt)], cache,
                                torch.tensor([slot], dtype=torch.int32))
    return logits, cache


@pytest.mark.parametrize("cut", [1, 13, 39])
def test_extend_into_matches_prefill_into(model, cut):
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, CFG.vocab_size, (40,), generator=g).tolist()
    want, wc = _whole(model, prompt)
    cache = KVCache(CFG, 1, 64)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    slot = torch.zeros(1, dtype=torch.int32)
    model.prefill_into(torch.tensor([prompt[:cut]]), [cut], cache, slot)
    cache.lens.fill_(INACTIVE)  # base is the argument, never cache.lens
    # right-padded by 3: the padding must change nothing
    idx = torch.tensor([prompt[cut:] + [0, 0, 0]])
    got = model.extend_into(idx, [40 - cut], cache, slot, torch.tensor([cut], dtype=torch.int32))
    assert got.shape == (1, CFG.vocab_size)
    assert cache.lens.tolist() == [40]
    assert _rel(got, want) < 1e-4
    assert _rel(cache.k[:, :, :, :40], wc.k[:, :, :, :40]) < 1e-4
    assert _rel(cache.v[:, :, :, :40], wc.v[:, :, :, :40]) < 1e-4
    assert torch.isnan(cache.k[:, :, :, 40:]).all()  # nothing past the sequence was written


def test_extend_into_ragged_rows_of_a_wider_cache(model):
    g = torch.Generator().manual_seed(4)
    pa = torch.randint(0, CFG.vocab_size, (40,), generator=g).tolist()
    pb = torch.randint(0, CFG.vocab_size, (23,), generator=g).tolist()
    (wa, ca), (wb, cb) = _whole(model, pa), _whole(model, pb)
    cache = KVCache(CFG, 5, 64)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    slots = torch.tensor([3, 0], dtype=torch.int32)  # not adjacent, not in order
    cuts = [13, 20]
    idx = torch.zeros(2, 13, dtype=torch.long)
    idx[0, :13], idx[1, :13] = torch.tensor(pa[:13]), torch.tensor(pb[:13])
    model.prefill_into(idx, [13, 13], cache, slots)
    # row b first catches up to its own cut alone, then both extend raggedly together
    model.extend_into(torch.tensor([pb[13:20]]), [7], cache, slots[1:],
                      torch.tensor([13], dtype=torch.int32))
    idx = torch.zeros(2, 27, dtype=torch.long)
    idx[0, :27], idx[1, :3] = torch.tensor(pa[13:]), torch.tensor(pb[20:])
    got = model.extend_into(idx, [27, 3], cache, slots, torch.tensor(cuts, dtype=torch.int32))
    assert cache.lens.tolist() == [23, 0, 0, 40, 0]
    assert _rel(got[0], wa[0]) < 1e-4 and _rel(got[1], wb[0]) < 1e-4
    assert _rel(cache.k[:, 3, :, :40], ca.k[:, 0, :, :40]) < 1e-4
    assert _rel(cache.v[:, 0, :, :23], cb.v[:, 0, :, :23]) < 1e-4
    assert torch.isnan(cache.k[:, [1, 2, 4]]).all()  # the other rows keep their bytes
    with pytest.raises(ValueError):
        model.extend_into(idx, [27, 3], cache, slots.long(), torch.tensor(cuts, dtype=torch.int32))


# ------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def expected(model, prompts):
    """Every request through ``generate`` on its whole prompt alone, computed once."""
    return [model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3], top_p=m[4],
                           seeds=[m[5]])[0].tolist() for p, m in zip(prompts, MIX)]


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


@pytest.mark.parametrize("chunk", [None, 1, 7, 16])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_engine_matches_generate_alone(model, prompts, expected, schedule, chunk):
    S, arrivals = SCHEDULES[schedule]
    eng = _engine(model, slots=S, prefill_chunk=chunk)
    pids = {i: eng.add_prefix(prompts[i][:k]) for i, k in PREFIXED.items()}
    got, events = _drive(eng, prompts, arrivals, pids)
    assert got == expected
    for i in range(len(MIX)):
        fins = [fin for j, _, fin in events if j == i]
        assert fins.count(True) == 1 and fins[-1]
    if schedule == "s1":  # filling costs no device step
        assert eng.steps == sum(m[1] for m in MIX)
    assert not eng.has_work() and eng.num_active == 0 and eng.num_filling == 0


def test_defaults_are_the_engine_without_the_options(model, prompts, expected):
    eng = GPT2Engine(model, slots=3, poll_every=1)
    assert eng.prefix_cache is None and eng.prefill_chunk is None
    with pytest.raises(ValueError):
        eng.add_prefix([1, 2, 3])  # a store of no rows is full
    rids = [_submit(eng, prompts, i) for i in range(len(MIX))]
    got = eng.run()
    assert [got[r] for r in rids] == expected


def test_filling_slot_bookkeeping(model, prompts, expected):
    eng = _engine(model, slots=2, prefill_chunk=8)
    a = _submit(eng, prompts, 4)   # 2 tokens: decoding after the first step
    b = _submit(eng, prompts, 1)   # 39 tokens: 5 chunks of 8
    c = _submit(eng, prompts, 0)   # queued behind them
    got = collections.defaultdict(list)
    for n in range(1, 5):
        events = eng.step()
        assert [rid for rid, _, _ in events] == [a]  # the filling slot yields no event
        got[a].extend(events[0][1])
        assert eng.num_active == 2 and eng.num_filling == 1 and eng.num_queued == 1
        assert eng._fill[1] == 8 * n  # noqa: SLF001  (the host keeps the base)
        assert eng.active.tolist() == [1, 0] and eng.cache.lens[1].item() <= INACTIVE + 1
    for rid, new, _ in eng.step():  # the fifth chunk completes b's prompt
        got[rid].extend(new)
    assert eng.num_filling == 0 and len(got[b]) == 1
    while eng.has_work():
        for rid, new, _ in eng.step():
            got[rid].extend(new)
    assert [got[a], got[b], got[c]] == [expected[4], expected[1], expected[0]]


def test_cancel_filling_request_frees_the_slot(model, prompts, expected):
    eng = _engine(model, slots=1, prefill_chunk=8)
    b = _submit(eng, prompts, 1)
    d = _submit(eng, prompts, 6)
    assert eng.step() == [] and eng.step() == []  # only a filling slot: no device step
    assert eng.steps == 0 and eng.num_filling == 1 and eng.has_work()
    assert eng.cancel(b) and not eng.cancel(b)
    assert eng.num_active == 0 and eng.num_filling == 0
    got = eng.run()
    assert got == {d: expected[6]}


def test_drop_prefix_while_in_use(model, prompts, expected):
    eng = _engine(model, slots=2, prefix_slots=1, prefill_chunk=7)
    pid = eng.add_prefix(prompts[1][:20])
    with pytest.raises(ValueError):
        eng.add_prefix([1, 2])  # the store is full
    running = eng.submit(prompts[1][20:], MIX[1][1], temperature=0.8, top_k=5, seed=11,
                         prefix=pid)
    eng.step()  # admitted: the slot has its copy
    queued = eng.submit(prompts[1][20:], MIX[1][1], temperature=0.8, top_k=5, seed=11,
                        prefix=pid)
    eng.drop_prefix(pid)
    with pytest.raises(ValueError):
        eng.drop_prefix(pid)
    with pytest.raises(ValueError):
        eng.submit([1], 2, prefix=pid)
    other = eng.add_prefix(prompts[5][:29])  # reuses the row while `running` still fills
    eng.prefix_cache.k.fill_(float("nan"))   # ... and nobody reads the store any more
    eng.prefix_cache.v.fill_(float("nan"))
    got = eng.run()
    # the queued one lost its prefix before admission and was prefilled whole
    assert got[running] == expected[1] and got[queued] == expected[1]
    assert other != pid


@pytest.mark.parametrize("bad", ["unknown", "too_long", "prefix_tokens", "prefix_len", "empty"])
def test_rejections_queue_nothing(model, bad):
    eng = _engine(model, slots=2, prefix_slots=1)
    if bad == "unknown":
        with pytest.raises(ValueError):
            eng.submit([1, 2], 3, prefix=0)
        with pytest.raises(ValueError):
            eng.submit([1, 2], 3, prefix="sys")
    elif bad == "too_long":
        pid = eng.add_prefix([1] * 100)
        with pytest.raises(ValueError):
            eng.submit([2] * 20, 9, prefix=pid)  # 100 + 20 + 9 = 129 > max_len 128
        eng.submit([2] * 20, 8, prefix=pid)
        assert eng.num_queued == 1
        return
    elif bad == "prefix_tokens":
        with pytest.raises(ValueError):
            eng.add_prefix([1, CFG.vocab_size])
        with pytest.raises(ValueError):
            eng.add_prefix([])
        eng.add_prefix([1])  # ... and the row is still free
    elif bad == "prefix_len":
        with pytest.raises(ValueError):
            eng.add_prefix([1] * 128)  # no room for a continuation
        eng.add_prefix([1] * 127)
    else:
        pid = eng.add_prefix([1, 2])
        with pytest.raises(ValueError):
            eng.submit([], 3, prefix=pid)  # the continuation is non-empty
    assert eng.num_queued == 0 and not eng.has_work() and eng.step() == []


def test_constructor_checks(model):
    with pytest.raises(ValueError):
        GPT2Engine(model, slots=2, prefix_slots=-1)
    with pytest.raises(ValueError):
        GPT2Engine(model, slots=2, prefill_chunk=0)
