"""ops/csrc/kv_slots.hip (``rf.kv_insert``, ``rf.slot_advance``) against the plain-torch
references, bit for bit, and the continuous-batching engine on the GPU in bf16:
``prefill_into`` against ``prefill``, captured against eager steps, the engine against
``generate`` on the same rows, and a request's tokens against its placement."""

import dataclasses
import functools

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

D = 64


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _bits(shape, g):
    """bf16 of random bit patterns: every kind of value, NaNs of every payload included."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32) \
        .to(torch.int16).view(torch.bfloat16)


# ------------------------------------------------------------------ kv_insert
@pytest.mark.parametrize("shape,slots,lens", [
    ((3, 128, 2, 5, 160), [4, 0, 2], [1, 37, 128]),
    ((4, 40, 2, 3, 24), [1, -1, 3, 0], [40, 5, 7, 0]),  # clamp to Tmax, two skipped rows
    ((2, 256, 12, 2, 256), [1, 0], [256, 200]),
    ((4, 130, 1, 4, 130), [3, 1, 0, 2], [63, 64, 65, 129]),  # the mover's 64-row block edge
])
def test_kv_insert_bitwise(cuda_device, shape, slots, lens):
    Bn, Tp, H, S, Tmax = shape
    g = torch.Generator().manual_seed(Bn * 1000 + Tp)
    qkv = torch.randn(Bn, Tp, 3, H, D, generator=g).bfloat16()
    qkv[0, 0, 1, 0, :3] = float("nan")
    qkv = qkv.to(cuda_device)
    k0, v0 = _bits((S, H, Tmax, D), g).to(cuda_device), _bits((S, H, Tmax, D), g).to(cuda_device)
    sl = torch.tensor(slots, dtype=torch.int32, device=cuda_device)
    ln = torch.tensor(lens, dtype=torch.int32, device=cuda_device)
    k, v, wk, wv = k0.clone(), v0.clone(), k0.clone(), v0.clone()
    ref.kv_insert(qkv, wk, wv, sl, ln)
    assert rf.kv_insert(qkv, k, v, sl, ln) is None
    assert torch.equal(k.view(torch.int16), wk.view(torch.int16))
    assert torch.equal(v.view(torch.int16), wv.view(torch.int16))
    # the reference did write what the table says, and only that
    changed = (wk.view(torch.int16) != k0.view(torch.int16)).any(-1).any(1)  # [S, Tmax]
    for s in range(S):
        n = max([min(l, Tp, Tmax) for x, l in zip(slots, lens) if x == s], default=0)
        assert not changed[s, n:].any()
        if n:
            assert torch.equal(wk[s, :, :n].view(torch.int16),
                               qkv[slots.index(s), :n, 1].transpose(0, 1).view(torch.int16))


# ------------------------------------------------------------------ slot_advance
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("S", [1, 5, 64, 200])
def test_slot_advance_exact(cuda_device, S, eos):
    cap = 6
    g = torch.Generator().manual_seed(S)
    host = dict(
        lens=torch.randint(0, 50, (S,), generator=g, dtype=torch.int32),
        n_out=torch.randint(0, cap + 1, (S,), generator=g, dtype=torch.int32),
        max_new=torch.randint(1, 9, (S,), generator=g, dtype=torch.int32),
        active=(torch.rand(S, generator=g) < 0.7).to(torch.uint8),
        out=torch.full((S, cap), -1, dtype=torch.int64),
    )
    if S >= 5:
        host["active"][:2] = 1
        host["n_out"][0] = cap  # the cap guard
        host["n_out"][1] = 0
    dev = {n: t.to(cuda_device) for n, t in host.items()}
    for call in range(4):
        tok = torch.randint(0, 6, (S,), generator=g)
        ref.slot_advance(tok, host["lens"], host["n_out"], host["max_new"], host["active"],
                         host["out"], eos)
        assert rf.slot_advance(tok.to(cuda_device), dev["lens"], dev["n_out"], dev["max_new"],
                               dev["active"], dev["out"], eos) is None
        for n in host:
            assert torch.equal(dev[n].cpu(), host[n]), (call, n)
        idle = host["active"] == 0
        assert (host["lens"][idle] == rf.SLOT_INACTIVE).all()
        host["lens"] += 1
        dev["lens"] += 1


# ------------------------------------------------------------------ model
def _cfg():
    return dataclasses.replace(GPT2Config.tiny(), n_embd=128, n_head=2, init_std=0.2)


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(0)
    return GPT2(_cfg()).eval().to(dev, torch.bfloat16)


# (prompt length, max_new_tokens, temperature, top_k, top_p, seed)
MIX = [(1, 24, 0.0, None, None, 3), (5, 9, 0.8, 5, None, 11), (17, 16, 1.3, 50, 0.9, 2),
       (40, 3, 0.8, None, 0.9, 7), (9, 20, 1.3, None, None, -4), (30, 12, 0.0, 5, None, 0)]


def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 512, (m[0],), generator=g).tolist() for m in MIX]


def _submit(eng, i):
    m = MIX[i]
    return eng.submit(_prompts()[i], m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5])


def _drive(eng, arrivals):
    """Submits request i once ``eng.steps`` has reached ``arrivals[i]``."""
    pending = sorted(arrivals, key=lambda i: (arrivals[i], i))
    rid_of, got = {}, {i: [] for i in arrivals}
    while pending or eng.has_work():
        while pending and (arrivals[pending[0]] <= eng.steps or not eng.has_work()):
            i = pending.pop(0)
            rid_of[_submit(eng, i)] = i
        for rid, new, _fin in eng.step():
            got[rid_of[rid]].extend(new)
    return got


def test_prefill_into_equals_prefill(cuda_device):
    model = _model(cuda_device)
    cfg = model.cfg
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, cfg.vocab_size, (2, 40), generator=g).to(cuda_device)
    lens = torch.tensor([17, 40], dtype=torch.int32, device=cuda_device)
    own = KVCache(cfg, 2, 64, cuda_device, torch.bfloat16)
    want = model.prefill(idx, lens, own)
    wide = KVCache(cfg, 4, 64, cuda_device, torch.bfloat16)
    wide.k.copy_(_bits(tuple(wide.k.shape), g))
    wide.v.copy_(_bits(tuple(wide.v.shape), g))
    wide.lens.fill_(rf.SLOT_INACTIVE)
    k0, v0, lens_ptr = wide.k.clone(), wide.v.clone(), wide.lens.data_ptr()
    slots = torch.tensor([2, 0], dtype=torch.int32, device=cuda_device)
    got = model.prefill_into(idx, lens, wide, slots)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert wide.lens.data_ptr() == lens_ptr  # written in place, never rebound
    assert wide.lens.tolist() == [40, rf.SLOT_INACTIVE, 17, rf.SLOT_INACTIVE]
    for c, c0, o in ((wide.k, k0, own.k), (wide.v, v0, own.v)):
        c, c0, o = c.view(torch.int16), c0.view(torch.int16), o.view(torch.int16)
        for b, (s, n) in enumerate(((2, 17), (0, 40))):
            assert torch.equal(c[:, s, :, :n], o[:, b, :, :n])
            assert torch.equal(c[:, s, :, n:], c0[:, s, :, n:])  # past lens: kept
        assert torch.equal(c[:, 1], c0[:, 1]) and torch.equal(c[:, 3], c0[:, 3])


def test_engine_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    arrivals = {0: 0, 1: 0, 2: 2, 3: 5, 4: 6, 5: 40}  # the last long after most finished
    eager = GPT2Engine(model, slots=4, max_len=96, graph=False, poll_every=1)
    graphed = GPT2Engine(model, slots=4, max_len=96, poll_every=1)
    assert eager._graph is None and graphed._graph is not None
    a, b = _drive(eager, arrivals), _drive(graphed, arrivals)
    assert a == b
    assert [len(a[i]) for i in range(len(MIX))] == [m[1] for m in MIX]
    assert eager.steps == graphed.steps


def test_engine_equals_generate_on_the_same_rows(cuda_device):
    model = _model(cuda_device)
    rows = [0, 1, 2, 3]
    prompts = _prompts()
    lens = [MIX[i][0] for i in rows]
    new = [MIX[i][1] for i in rows]
    idx = torch.zeros(len(rows), max(lens), dtype=torch.long)
    for b, i in enumerate(rows):
        idx[b, : lens[b]] = torch.tensor(prompts[i])
    out = model.generate(idx.to(cuda_device), max(new), lens=lens,
                         temperature=[MIX[i][2] for i in rows], top_k=[MIX[i][3] for i in rows],
                         top_p=[MIX[i][4] for i in rows], seeds=[MIX[i][5] for i in rows]).cpu()
    want = [out[b, : new[b]].tolist() for b in range(len(rows))]
    eng = GPT2Engine(model, slots=len(rows), max_len=max(lens) + max(new),
                     poll_every=1)
    rids = [_submit(eng, i) for i in rows]
    got = eng.run()
    assert [got[r] for r in rids] == want
    assert eng.steps == max(new)


def test_placement_invariance(cuda_device):
    model = _model(cuda_device)
    alone = GPT2Engine(model, slots=4, max_len=96, poll_every=1)
    rid = _submit(alone, 2)
    want = alone.run()[rid]
    busy = GPT2Engine(model, slots=4, max_len=96, poll_every=1)
    got = _drive(busy, {0: 0, 4: 0, 2: 7})  # admitted alone at step 7, two slots decoding
    assert got[2] == want and len(want) == MIX[2][1]
