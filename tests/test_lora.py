"""Per-row low-rank adapters on the CPU: ``ref.lora_add`` against a per-token fp64 loop,
``rf.lora_add``'s argument checks, the ``LoRAStack`` store, the model's passes with
``adapters`` against merged weights and against each other, ``generate`` and the engine
against ``generate`` on each request alone."""

import collections
import copy
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.models.lora import TARGETS, LoRAStack, target_dims
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
BF = torch.bfloat16
WEIGHT = {"c_attn": "c_attn_w", "c_proj": "c_proj_w", "c_fc": "c_fc_w", "mlp_proj": "mlp_proj_w"}


def _bits(shape, g, dtype):
    """Random bit patterns: every kind of value, NaNs of every payload included."""
    if dtype == BF:
        return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32) \
            .to(torch.int16).view(BF)
    return torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64) \
        .to(torch.int32).view(torch.float32)


def _raw(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _state(r, seed, alpha=None, std=0.2, targets=TARGETS, layers=None, cfg=CFG):
    g = torch.Generator().manual_seed(seed)
    state = {} if alpha is None else {"alpha": alpha}
    for layer in range(cfg.n_layer) if layers is None else layers:
        for t in targets:
            din, dout = target_dims(cfg)[t]
            state[f"h.{layer}.{t}.lora_A"] = torch.randn(r, din, generator=g) * std
            state[f"h.{layer}.{t}.lora_B"] = torch.randn(dout, r, generator=g) * std
    return state


# ------------------------------------------------------------------ ref.lora_add
def _loop(y, x, a, b, scale, idx, r_used=None):
    """Token by token in fp64; ``t`` rounded once to the input dtype (bf16 inputs only)."""
    out = y.clone()
    for bi in range(x.shape[0]):
        ad = int(idx[bi])
        if not 0 <= ad < a.shape[0]:
            continue
        r = a.shape[1] if r_used is None else r_used[ad]
        for i in range(x.shape[1]):
            t = a[ad, :r].double() @ x[bi, i].double()
            if x.dtype == BF:
                t = t.to(BF).double()
            d = b[ad, :, :r].double() @ t
            out[bi, i] = (y[bi, i].double() + float(scale[ad]) * d).to(y.dtype)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_reference_against_loop(dtype):
    g = torch.Generator().manual_seed(0)
    Bn, T, Din, Dout, R, NA = 7, 5, 24, 40, 16, 3
    x = torch.randn(Bn, T, Din, generator=g).to(dtype)
    a = (torch.randn(NA, R, Din, generator=g) * 0.3).to(dtype)
    b = (torch.randn(NA, Dout, R, generator=g) * 0.3).to(dtype)
    a[2, 4:], b[2, :, 4:] = 0, 0  # an r = 4 adapter, zero-padded to 16
    scale = torch.tensor([0.5, 2.0, 8.0])
    idx = torch.tensor([0, -1, 1, NA, 2, -2 ** 31, 1], dtype=torch.int32)
    y0 = torch.randn(Bn, T, Dout, generator=g).to(dtype)
    bad = [1, 3, 5]
    y0[bad] = _bits((3, T, Dout), g, dtype)
    y = y0.clone()
    assert ref.lora_add(y, x, a, b, scale, idx) is None
    assert torch.equal(_raw(y[bad]), _raw(y0[bad]))  # bytes kept, NaN payloads included
    # the padded adapter gives the unpadded r = 4 formula
    want = _loop(y0, x, a, b, scale, idx, r_used={0: R, 1: R, 2: 4})
    good = [0, 2, 4, 6]
    if dtype == BF:
        # fp32 against fp64 sums: t or y may land on the neighbouring bf16
        err = (y[good].double() - want[good].double()).abs()
        assert (err <= 2.0 ** -7 * want[good].double().abs() + 1e-3).all()
        assert (y[good] == want[good]).float().mean() > 0.95
    else:
        assert torch.allclose(y[good], want[good], rtol=1e-5, atol=1e-5)
    assert not torch.equal(y[good], y0[good])
    # the 2-D form is T = 1
    y2 = y0[:, 0].clone()
    ref.lora_add(y2, x[:, 0], a, b, scale, idx)
    assert torch.equal(_raw(y2[bad]), _raw(y0[bad, 0]))
    tol = 2.0 ** -7 if dtype == BF else 1e-5  # (the CPU matmul's sums depend on the shape)
    assert torch.allclose(y2[good].float(), y[good, 0].float(), rtol=tol, atol=tol)
    # and the bmm composition computes the same thing
    y3 = y0.clone()
    ref.lora_add_bmm(y3, x, a, b, scale, idx)
    assert torch.equal(_raw(y3[bad]), _raw(y0[bad]))
    tol = 3e-2 if dtype == BF else 1e-5
    assert torch.allclose(y3[good].float(), want[good].float(), rtol=tol, atol=tol)


def test_lora_add_checks():
    Bn, T, Din, Dout, R, NA = 2, 3, 8, 12, 4, 2
    g = torch.Generator().manual_seed(1)

    def args():
        return dict(y=torch.randn(Bn, T, Dout, generator=g), x=torch.randn(Bn, T, Din, generator=g),
                    a_stack=torch.randn(NA, R, Din, generator=g),
                    b_stack=torch.randn(NA, Dout, R, generator=g),
                    scale=torch.ones(NA), idx=torch.zeros(Bn, dtype=torch.int32))

    ok = args()
    y0 = ok["y"].clone()
    rf.lora_add(**ok)
    assert not torch.equal(ok["y"], y0)
    bad = {
        "x_shape": dict(x=torch.randn(Bn, T + 1, Din)),
        "x_dim": dict(x=torch.randn(Bn, Din)),
        "a_din": dict(a_stack=torch.randn(NA, R, Din + 1)),
        "b_rank": dict(b_stack=torch.randn(NA, Dout, R + 1)),
        "b_count": dict(b_stack=torch.randn(NA + 1, Dout, R)),
        "stack_dtype": dict(a_stack=torch.randn(NA, R, Din).to(BF)),
        "scale_dtype": dict(scale=torch.ones(NA, dtype=torch.float64)),
        "scale_shape": dict(scale=torch.ones(NA + 1)),
        "idx_dtype": dict(idx=torch.zeros(Bn, dtype=torch.int64)),
        "idx_shape": dict(idx=torch.zeros(Bn + 1, dtype=torch.int32)),
        "idx_list": dict(idx=[0, 0]),
        "idx_device": dict(idx=torch.zeros(Bn, dtype=torch.int32, device="meta")),
        "y_strided": dict(y=torch.randn(Bn, T, 2 * Dout)[:, :, ::2]),
        "x_grad": dict(x=torch.randn(Bn, T, Din, requires_grad=True)),
        "a_grad": dict(a_stack=torch.randn(NA, R, Din, requires_grad=True)),
    }
    for name, change in bad.items():
        kw = args()
        kw.update(change)
        y0 = kw["y"].clone()
        with pytest.raises(ValueError):
            rf.lora_add(**kw)
        assert torch.equal(kw["y"], y0), name


# ------------------------------------------------------------------ LoRAStack
def test_stack_load_and_clear():
    st = LoRAStack(CFG, 3, 10)
    C = CFG.n_embd
    assert st.rank == 16 and LoRAStack(CFG, 1, 33).rank == 48 and LoRAStack(CFG, 1, 64).rank == 64
    assert st.a["mlp_proj"].shape == (CFG.n_layer, 3, 16, 4 * C)
    assert st.b["c_attn"].shape == (CFG.n_layer, 3, 3 * C, 16)
    assert st.scale.dtype == torch.float32 and not any(t.any() for t in st.buffers())
    ptrs = [t.data_ptr() for t in st.buffers()]
    state = _state(4, 1, targets=("c_attn", "mlp_proj"), layers=[1])
    st.load(1, state, alpha=10)
    assert st.scale.tolist() == [0.0, 2.5, 0.0]  # alpha / r
    assert torch.equal(st.a["c_attn"][1, 1, :4], state["h.1.c_attn.lora_A"])
    assert torch.equal(st.b["mlp_proj"][1, 1, :, :4], state["h.1.mlp_proj.lora_B"])
    assert not st.a["c_attn"][1, 1, 4:].any() and not st.b["mlp_proj"][1, 1, :, 4:].any()
    # missing targets and layers, and the other slots, stay zero
    assert not st.a["c_fc"].any() and not st.b["c_proj"].any() and not st.a["c_attn"][0].any()
    assert not st.a["c_attn"][:, [0, 2]].any()
    st.load(2, dict(_state(10, 2), alpha=5.0))  # the dict's alpha; and no alpha at all: r / r
    st.load(0, _state(3, 3))
    assert st.scale.tolist() == [1.0, 2.5, 0.5]
    st.load(2, dict(_state(10, 2), alpha=5.0), alpha=20)  # the argument wins
    assert st.scale[2].item() == 2.0
    # a rejected load leaves the slot as it was
    before = [t.clone() for t in st.buffers()]
    good = _state(4, 5)
    for broken in (
        dict(good, **{"h.0.c_attn.lora_A": torch.zeros(4, C + 1)}),        # shape
        dict(good, **{"h.0.c_attn.lora_B": torch.zeros(3 * C, 5)}),        # two ranks
        dict(good, **{"h.9.c_attn.lora_A": torch.zeros(4, C)}),            # no such layer
        dict(good, **{"h.0.c_attn.lora_C": torch.zeros(4, C)}),            # no such key
        dict(good, **{"h.0.wte.lora_A": torch.zeros(4, C)}),               # no such target
        {"h.0.c_fc.lora_A": torch.zeros(4, C)},                            # A without B
        _state(11, 6),                                                     # rank > 10
        [("h.0.c_fc.lora_A", 0)],                                          # not a dict
    ):
        with pytest.raises(ValueError):
            st.load(1, broken)
    for slot in (3, -1, None, True):
        with pytest.raises(ValueError):
            st.load(slot, good)
        with pytest.raises(ValueError):
            st.clear(slot)
    assert all(torch.equal(a, b) for a, b in zip(st.buffers(), before))
    st.clear(1)
    assert st.scale.tolist() == [1.0, 0.0, 2.0] and not st.a["c_attn"][:, 1].any()
    assert st.a["c_attn"][:, 0].any() and st.b["c_fc"][:, 2].any()
    assert [t.data_ptr() for t in st.buffers()] == ptrs  # written in place, never rebound
    for bad in (dict(n_adapters=0, rank=4), dict(n_adapters=1, rank=0),
                dict(n_adapters=1, rank=65)):
        with pytest.raises(ValueError):
            LoRAStack(CFG, **bad)


# ------------------------------------------------------------------ the model
ALPHA = {0: 8.0, 1: 24.0}
RANK = {0: 4, 1: 16}


@pytest.fixture(scope="module")
def states():
    return {i: _state(RANK[i], 30 + i) for i in (0, 1)}


@pytest.fixture(scope="module")
def model(states):
    torch.manual_seed(11)
    m = GPT2(CFG).eval()
    stack = LoRAStack(CFG, 3, 16)  # adapter 2 stays a zero adapter
    for i, s in states.items():
        stack.load(i, s, alpha=ALPHA[i])
    m.attach_lora(stack)
    return m


@pytest.fixture(scope="module")
def merged(model, states):
    """Per adapter, a copy of the model with W += scale * B . A merged in fp32; -1: the base."""
    out = {-1: copy.deepcopy(model)}
    out[-1].attach_lora(None)
    for i, s in states.items():
        m = copy.deepcopy(out[-1])
        with torch.no_grad():
            for layer, blk in enumerate(m.h):
                for t in TARGETS:
                    w = getattr(blk, WEIGHT[t])
                    w += (ALPHA[i] / RANK[i]) * (s[f"h.{layer}.{t}.lora_B"] @
                                                 s[f"h.{layer}.{t}.lora_A"])
        out[i] = m
    return out


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _ids(*v):
    return torch.tensor(v, dtype=torch.int32)


def test_adapters_need_a_stack(model):
    bare = copy.deepcopy(model)
    bare.attach_lora(None)
    idx = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError):
        bare.prefill(idx, [3, 3], KVCache(CFG, 2, 8), adapters=_ids(0, 0))
    with pytest.raises(ValueError):
        bare.generate(idx, 2, adapters=0)
    for bad in (_ids(0), _ids(0, 0).long(), [0, 0]):
        with pytest.raises(ValueError):
            model.prefill(idx, [3, 3], KVCache(CFG, 2, 8), adapters=bad)
    for bad in (3, -2, [0], [0, 5]):
        with pytest.raises(ValueError):
            model.generate(idx, 2, adapters=bad)
    with pytest.raises(ValueError):
        model.attach_lora(LoRAStack(dataclasses.replace(CFG, n_embd=128), 1, 4))
    with pytest.raises(ValueError):
        model.attach_lora(LoRAStack(CFG, 1, 4, dtype=BF))


def test_no_op_cases_keep_the_bits(model):
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, CFG.vocab_size, (3, 20), generator=g)
    lens = [20, 7, 13]
    c0 = KVCache(CFG, 3, 32)
    want = model.prefill(idx, lens, c0)
    for ids in (_ids(-1, -1, -1), _ids(2, -1, 2)):  # the base model; a cleared adapter
        c = KVCache(CFG, 3, 32)
        got = model.prefill(idx, lens, c, adapters=ids)
        assert torch.equal(got, want) and torch.equal(c.k, c0.k) and torch.equal(c.v, c0.v)


def test_passes_match_merged_weights(model, merged):
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, CFG.vocab_size, (3, 20), generator=g)
    lens = [20, 7, 13]
    toks = torch.randint(0, CFG.vocab_size, (3, 3), generator=g)

    def run(m, rows, ids):
        n = len(rows)
        cache = KVCache(CFG, n, 32)
        out = [m.prefill(idx[rows], [lens[r] for r in rows], cache, adapters=ids)]
        for s in range(3):
            out.append(m.decode_step(toks[rows, s], cache, adapters=ids).clone())
        return out

    base = run(merged[-1], [0, 1, 2], None)
    for a in (0, 1):
        got = run(model, [0, 1, 2], _ids(a, a, a))
        want = run(merged[a], [0, 1, 2], None)
        assert _rel(got[0], base[0]) > 1e-2  # the adapter is seen to act
        for gl, wl in zip(got, want):
            assert _rel(gl, wl) < 1e-4
    mixed = run(model, [0, 1, 2], _ids(0, -1, 1))
    for row, a in enumerate((0, -1, 1)):
        want = run(merged[a], [row], None)
        for gl, wl in zip(mixed, want):
            assert _rel(gl[row], wl[0]) < 1e-4


@pytest.mark.parametrize("cut", [1, 13, 39])
def test_extend_into_matches_prefill_into(model, cut):
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, CFG.vocab_size, (40,), generator=g).tolist()
    slot, ad = torch.zeros(1, dtype=torch.int32), _ids(1)
    wc = KVCache(CFG, 1, 64)
    want = model.prefill_into(torch.tensor([prompt]), [40], wc, slot, adapters=ad)
    bc = KVCache(CFG, 1, 64)
    base = model.prefill_into(torch.tensor([prompt]), [40], bc, slot)
    assert _rel(base, want) > 1e-2 and _rel(bc.k[:, :, :, :40], wc.k[:, :, :, :40]) > 1e-2
    cache = KVCache(CFG, 1, 64)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    model.prefill_into(torch.tensor([prompt[:cut]]), [cut], cache, slot, adapters=ad)
    idx = torch.tensor([prompt[cut:] + [0, 0, 0]])  # right-padded by 3
    got = model.extend_into(idx, [40 - cut], cache, slot, _ids(cut), adapters=ad)
    assert cache.lens.tolist() == [40]
    assert _rel(got, want) < 1e-4
    assert _rel(cache.k[:, :, :, :40], wc.k[:, :, :, :40]) < 1e-4
    assert _rel(cache.v[:, :, :, :40], wc.v[:, :, :, :40]) < 1e-4
    assert torch.isnan(cache.k[:, :, :, 40:]).all() and torch.isnan(cache.v[:, :, :, 40:]).all()


# ------------------------------------------------------------------ generate and the engine
# (prompt length, max_new_tokens, temperature, top_k, top_p, seed): the mix of
# test_gpt2_extend.py; the adapter of request i is ADAPTER[i]
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
ADAPTER = [0, 1, None, 1, None, 0, 0, None, 1]
PREFIX = (5, 29)  # request 5 names a prefix (its first 29 tokens) bound to its adapter
SCHEDULES = {
    "s3_all_at_once": (3, [0] * 9),
    "s4_staggered": (4, [0, 0, 2, 2, 5, 5, 6, 6, 60]),
    "s1": (1, [0] * 9),
}


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, CFG.vocab_size, (m[0],), generator=g).tolist() for m in MIX]


def _alone(model, prompt, m, adapter):
    kw = {} if adapter == "none" else {"adapters": [adapter]}
    return model.generate(torch.tensor([prompt]), m[1], temperature=m[2], top_k=m[3], top_p=m[4],
                          seeds=[m[5]], **kw)[0].tolist()


@pytest.fixture(scope="module")
def expected(model, prompts):
    """Every request through ``generate`` alone with its adapter, computed once."""
    return [_alone(model, p, m, a) for p, m, a in zip(prompts, MIX, ADAPTER)]


@pytest.fixture(scope="module")
def expected_base(model, prompts):
    return [_alone(model, p, m, "none") for p, m in zip(prompts, MIX)]


def test_generate_rows_equal_generate_alone(model, prompts, expected, expected_base):
    rows = [1, 2, 3, 5]
    lens = [MIX[i][0] for i in rows]
    idx = torch.zeros(len(rows), max(lens), dtype=torch.long)
    for b, i in enumerate(rows):
        idx[b, : lens[b]] = torch.tensor(prompts[i])
    out = model.generate(idx, max(MIX[i][1] for i in rows), lens=lens,
                         temperature=[MIX[i][2] for i in rows], top_k=[MIX[i][3] for i in rows],
                         top_p=[MIX[i][4] for i in rows], seeds=[MIX[i][5] for i in rows],
                         adapters=[ADAPTER[i] for i in rows])
    for b, i in enumerate(rows):
        assert out[b, : MIX[i][1]].tolist() == expected[i]
    # the adapters change the tokens, the base rows keep theirs
    assert all((expected[i] != expected_base[i]) == (ADAPTER[i] is not None)
               for i in range(len(MIX)))
    # greedy without the device sampler takes adapters too
    i = 4
    got = model.generate(torch.tensor([prompts[i]]), 6, adapters=1)[0].tolist()
    assert got == _alone(model, prompts[i], (0, 6, 0.0, None, None, 0), 1)


def _submit(eng, prompts, i, pid=None):
    m = MIX[i]
    toks = prompts[i]
    if pid is not None and i == PREFIX[0]:
        toks = toks[PREFIX[1]:]
    else:
        pid = None
    return eng.submit(toks, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                      prefix=pid, adapter=ADAPTER[i])


def _drive(eng, prompts, arrivals, pid=None):
    pending = sorted(range(len(MIX)), key=lambda i: (arrivals[i], i))
    rid_of, got = {}, collections.defaultdict(list)
    while pending or eng.has_work():
        while pending and (arrivals[pending[0]] <= eng.steps or not eng.has_work()):
            i = pending.pop(0)
            rid_of[_submit(eng, prompts, i, pid)] = i
        for rid, new, _fin in eng.step():
            got[rid_of[rid]].extend(new)
    return [got[i] for i in range(len(MIX))]


@pytest.mark.parametrize("chunk", [None, 7])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_engine_matches_generate_alone(model, prompts, expected, schedule, chunk):
    S, arrivals = SCHEDULES[schedule]
    eng = GPT2Engine(model, slots=S, poll_every=1, prefix_slots=1, prefill_chunk=chunk,
                     lora=model.lora)
    i, k = PREFIX
    pid = eng.add_prefix(prompts[i][:k], adapter=ADAPTER[i])
    assert _drive(eng, prompts, arrivals, pid) == expected
    assert not eng.has_work() and eng.num_active == 0


def test_engine_defaults(model, prompts, expected_base):
    """A stack attached and no adapter named: the engine without ``lora``."""
    bare = copy.deepcopy(model)
    bare.attach_lora(None)
    arrivals = SCHEDULES["s4_staggered"][1]
    plain = GPT2Engine(bare, slots=4, poll_every=1)
    assert plain.lora is None and plain.adapter is None
    with_stack = GPT2Engine(model, slots=4, poll_every=1, lora=model.lora)
    assert with_stack.adapter.tolist() == [-1] * 4
    sub = lambda eng, i: eng.submit(prompts[i], MIX[i][1], temperature=MIX[i][2],  # noqa: E731
                                    top_k=MIX[i][3], top_p=MIX[i][4], seed=MIX[i][5])
    got = []
    for eng in (plain, with_stack):
        rids = [sub(eng, i) for i in range(len(MIX))]
        out = eng.run()
        got.append([out[r] for r in rids])
    assert got[0] == got[1] == expected_base
    assert with_stack.adapter.tolist() == [-1] * 4 and arrivals


def test_engine_rejections_queue_nothing(model, prompts):
    bare = copy.deepcopy(model)
    bare.attach_lora(None)
    plain = GPT2Engine(bare, slots=2, poll_every=1)
    with pytest.raises(ValueError):
        plain.submit([1, 2], 3, adapter=0)  # adapter without lora
    with pytest.raises(ValueError):
        plain.load_adapter(0, {})
    assert not plain.has_work()
    eng = GPT2Engine(model, slots=2, poll_every=1, prefix_slots=2, lora=model.lora)
    for bad in (3, -1, "0", 1.0, True):
        with pytest.raises(ValueError):
            eng.submit([1, 2], 3, adapter=bad)
        with pytest.raises(ValueError):
            eng.add_prefix([1, 2], adapter=bad)
    assert not eng.has_work() and not eng._prefixes and len(eng._prefix_free) == 2
    p0, pb = eng.add_prefix([5, 6, 7], adapter=0), eng.add_prefix([5, 6, 7])
    for pid, other in ((p0, 1), (pb, 0)):
        with pytest.raises(ValueError):
            eng.submit([1, 2], 3, prefix=pid, adapter=other)  # prefix / adapter mismatch
    assert not eng.has_work() and eng._next_rid == 0
    # in use: by a prefix, by a queued request, by a running one
    state = _state(4, 50)
    for call in (lambda: eng.unload_adapter(0), lambda: eng.load_adapter(0, state)):
        with pytest.raises(ValueError):
            call()
    rid = eng.submit([1, 2], 4, adapter=1)
    with pytest.raises(ValueError):
        eng.unload_adapter(1)
    eng.step()
    assert eng.num_active == 1
    with pytest.raises(ValueError):
        eng.load_adapter(1, state)
    assert len(eng.run()[rid]) + 1 == 4  # (the first step's token went to that step's events)
    eng.drop_prefix(p0)
    before = [t.clone() for t in model.lora.buffers()]
    with pytest.raises(ValueError):
        eng.load_adapter(2, {"h.0.c_fc.lora_Z": torch.zeros(1, 1)})  # a bad state: slot kept
    assert all(torch.equal(a, b) for a, b in zip(model.lora.buffers(), before))


def test_engine_live_load(model, prompts):
    """An adapter loaded into a running engine serves the next request that names it."""
    live = copy.deepcopy(model)  # its own stack: the module's stays as the fixtures built it
    eng = GPT2Engine(live, slots=2, poll_every=1, lora=live.lora)
    first = _submit(eng, prompts, 3)
    eng.step()
    state = _state(8, 60)
    eng.load_adapter(2, state, alpha=4)
    m = MIX[6]
    rid = eng.submit(prompts[6], m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                     adapter=2)
    got = eng.run()
    assert got[rid] == _alone(live, prompts[6], m, 2)
    assert got[rid] != _alone(live, prompts[6], m, "none")
    assert len(got[first]) == MIX[3][1] - 1
    eng.unload_adapter(2)  # nothing names it any more
    rid = eng.submit(prompts[6], m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                     adapter=2)
    assert eng.run()[rid] == _alone(live, prompts[6], m, "none")  # a zero adapter
