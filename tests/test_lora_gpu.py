"""ops/csrc/lora.hip (``rf.lora_add``) on the GPU: the operand layout with exact integer data,
the arithmetic against fp64, untouched rows and guards bit for bit, the invariance of a
token's bits against batch size, tile place and repetition, one capture serving changing
inputs and adapters; then the model and the engine in bf16 with adapters per row."""

import dataclasses
import functools

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.models.lora import LoRAStack
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops.graph_lock import CapturedStep

pytestmark = pytest.mark.gpu

NA = 3  # adapters; adapter 2 is an r = 4 adapter zero-padded to R
# (Bn, T, Din, Dout, R): the smallest shapes at which each part of the kernel can go wrong
SHAPES = [
    (1, 1, 64, 64, 16),        # the minimum
    (5, 37, 768, 2304, 16),    # a token tail inside the second tile
    (3, 1, 3072, 768, 64),     # the longest K and the largest R, in decode form
    (2, 130, 768, 3072, 32),   # three tiles with a 2-token tail
    (64, 1, 768, 768, 16),     # the engine's width
]
SCALES = [0.5, 2.0, 8.0]
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _bits(shape, g):
    """bf16 of random bit patterns: every kind of value, NaNs of every payload included."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32) \
        .to(torch.int16).view(BF)


def _idx(Bn):
    """All adapters mixed with -1 and n_adapters (the two kinds of row without one)."""
    pat = [1, 2, -1, 0, NA]
    return torch.tensor([pat[b % len(pat)] for b in range(Bn)], dtype=torch.int32)


def _pad_r4(a, b):
    """Adapter 2 as the loader leaves an r = 4 adapter: zero beyond rank 4."""
    a[2, 4:] = 0
    b[2, :, 4:] = 0
    return a, b


@functools.lru_cache(maxsize=None)
def _random_case(shape):
    """CPU inputs and the fp64 results of one shape, computed once: ``want`` with y ~ N(0,1),
    ``delta`` = the adapter term alone (the result with y = 0), ``slack`` = scale * |t64|.|B|^T."""
    Bn, T, Din, Dout, R = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(Bn, T, Din, generator=g).to(BF)
    y = torch.randn(Bn, T, Dout, generator=g).to(BF)
    a, b = _pad_r4((torch.randn(NA, R, Din, generator=g) * 0.05).to(BF),
                   (torch.randn(NA, Dout, R, generator=g) * 0.05).to(BF))
    scale = torch.tensor(SCALES)
    idx = _idx(Bn)
    ok = (idx >= 0) & (idx < NA)
    ic = idx.long().clamp(0, NA - 1)
    t64 = x.double() @ a.double()[ic].transpose(1, 2)          # no intermediate rounding
    sc = (scale.double()[ic] * ok).view(Bn, 1, 1)
    delta = sc * (t64 @ b.double()[ic].transpose(1, 2))
    slack = sc * (t64.abs() @ b.double()[ic].abs().transpose(1, 2))
    return dict(x=x, y=y, a=a, b=b, scale=scale, idx=idx, ok=ok, delta=delta, slack=slack)


def _run(dev, y, x, a, b, scale, idx):
    y = y.to(dev).clone()
    rf.lora_add(y, x.to(dev), a.to(dev), b.to(dev), scale.to(dev), idx.to(dev))
    return y.cpu()


# ------------------------------------------------------------------ layout, exact data
@pytest.mark.parametrize("shape", SHAPES)
def test_layout_exact_integers(cuda_device, shape):
    """Small integers, asymmetric in (r, k) and (n, r), y = 0. The fp32 sums of integers are
    exact in any order (|t| <= 4 * 3072, |sum_r| <= 64 * 2 * 2**14 < 2**24), so the two
    roundings the contract names are the only ones and the result is determined bit for bit:
    a row/column swap or a b_stack fragment out of the permuted k order cannot hide."""
    Bn, T, Din, Dout, R = shape
    k, r, n = torch.arange(Din), torch.arange(R), torch.arange(Dout)
    bi, ti, ai = torch.arange(Bn), torch.arange(T), torch.arange(NA)
    x = ((bi.view(-1, 1, 1) + 3 * ti.view(1, -1, 1) + 7 * k.view(1, 1, -1) +
          k.view(1, 1, -1) // 11) % 5 - 2).to(BF)
    a = ((ai.view(-1, 1, 1) + r.view(1, -1, 1) + 2 * k.view(1, 1, -1) +
          k.view(1, 1, -1) // 13) % 5 - 2).to(BF)
    b = ((2 * ai.view(-1, 1, 1) + 3 * n.view(1, -1, 1) + r.view(1, 1, -1) +
          n.view(1, -1, 1) // 7) % 5 - 2).to(BF)
    a, b = _pad_r4(a, b)
    scale = torch.tensor(SCALES)
    idx = _idx(Bn)
    ok = ((idx >= 0) & (idx < NA)).view(Bn, 1, 1)
    ic = idx.long().clamp(0, NA - 1)
    t = (x.double() @ a.double()[ic].transpose(1, 2)).to(BF).double()
    want = (scale.double()[ic].view(Bn, 1, 1) * (t @ b.double()[ic].transpose(1, 2))).to(BF)
    want = torch.where(ok, want, torch.zeros_like(want))
    assert want.abs().max() > 0
    got = _run(cuda_device, torch.zeros(Bn, T, Dout, dtype=BF), x, a, b, scale, idx)
    bad = (got.float() != want.float()).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, first at {bad[0].tolist()}"


# ------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("shape", SHAPES)
def test_against_fp64(cuda_device, shape):
    """|got - want| <= 2^-7 |want| + 2^-7 scale (|t64| . |B|^T): the two bf16 roundings (t and
    the final y) are at most 2^-8 relative each, and the factor 2 lets fp32 sums in another
    order land on the neighbouring bf16; the fp32 accumulation terms are three orders of
    magnitude smaller at K <= 3072. With y = 0, per-row relative norm error < 1e-2 as well.
    Measured on an MI355X: worst ratio to the bound 0.478, worst row error 2.98e-3."""
    c = _random_case(shape)
    eps = 2.0 ** -7
    for y in (c["y"], torch.zeros_like(c["y"])):
        want = y.double() + c["delta"]
        got = _run(cuda_device, y, c["x"], c["a"], c["b"], c["scale"], c["idx"]).double()
        bound = eps * want.abs() + eps * c["slack"]
        ratio = ((got - want).abs() / bound.clamp_min(1e-300))[c["ok"]]
        print(f"lora_add {shape} y={'0' if not y.any() else 'N(0,1)'}: "
              f"worst |err| / bound = {ratio.max().item():.3f}")
        assert torch.equal(got[~c["ok"]], y.double()[~c["ok"]])
        assert ratio.max().item() <= 1.0
        if not y.any():
            rows = c["ok"].nonzero().flatten()
            rel = ((got - want)[rows].flatten(1).norm(dim=1) /
                   want[rows].flatten(1).norm(dim=1))
            print(f"lora_add {shape}: worst row relative error = {rel.max().item():.2e}")
            assert rel.max().item() < 1e-2


# ------------------------------------------------------------------ untouched bytes
@pytest.mark.parametrize("shape", SHAPES)
def test_untouched_rows_and_guards(cuda_device, shape):
    Bn, T, Din, Dout, R = shape
    c = _random_case(shape)
    g = torch.Generator().manual_seed(3)
    guard, n = 64, Bn * T * Dout  # 128-byte guards keep y 16-byte aligned
    buf0 = _bits((guard + n + guard,), g)
    buf = buf0.to(cuda_device).clone()
    y = buf[guard: guard + n].view(Bn, T, Dout)
    dev = cuda_device
    rf.lora_add(y, c["x"].to(dev), c["a"].to(dev), c["b"].to(dev), c["scale"].to(dev),
                c["idx"].to(dev))
    got, was = buf.cpu().view(torch.int16), buf0.view(torch.int16)
    assert torch.equal(got[:guard], was[:guard]) and torch.equal(got[-guard:], was[-guard:])
    got, was = got[guard: guard + n].view(Bn, T, Dout), was[guard: guard + n].view(Bn, T, Dout)
    assert torch.equal(got[~c["ok"]], was[~c["ok"]])
    assert not torch.equal(got[c["ok"]], was[c["ok"]])  # and the others were written


# ------------------------------------------------------------------ invariance
def test_invariance_bitwise(cuda_device):
    shape = SHAPES[1]
    Bn, T, Din, Dout, R = shape
    c = _random_case(shape)
    dev = cuda_device
    args = [c[k].to(dev) for k in ("a", "b", "scale")]
    x, y0, idx = c["x"].to(dev), c["y"].to(dev), c["idx"].to(dev)
    full = y0.clone()
    rf.lora_add(full, x, *args, idx)
    again = y0.clone()
    rf.lora_add(again, x, *args, idx)
    assert torch.equal(full.view(torch.int16), again.view(torch.int16))
    for b in range(Bn):
        alone = y0[b: b + 1].clone()                 # the row as a batch of one
        rf.lora_add(alone, x[b: b + 1].contiguous(), *args, idx[b: b + 1].clone())
        assert torch.equal(alone.view(torch.int16), full[b: b + 1].view(torch.int16)), b
        toks = y0[b].clone().view(T, 1, Dout)        # each token as a row of its own, T = 1
        rf.lora_add(toks, x[b].contiguous().view(T, 1, Din), *args, idx[b: b + 1].repeat(T))
        assert torch.equal(toks.view(T, Dout).view(torch.int16), full[b].view(torch.int16)), b
        flat = y0[b].clone()                         # and in the 2-D form
        rf.lora_add(flat, x[b].contiguous(), *args, idx[b: b + 1].repeat(T))
        assert torch.equal(flat.view(torch.int16), full[b].view(torch.int16)), b


# ------------------------------------------------------------------ capture
def test_one_capture_serves_changing_inputs_and_adapters(cuda_device):
    dev = cuda_device
    cfg = _cfg()
    stack = LoRAStack(cfg, NA, 16, dev, BF)
    for i in range(NA):
        stack.load(i, _state(cfg, 4 if i == 2 else 16, seed=10 + i), alpha=SCALES[i] * 16)
    C, Bn = cfg.n_embd, 6
    a, b = stack.a["c_fc"][1], stack.b["c_fc"][1]
    g = torch.Generator().manual_seed(8)
    x = torch.randn(Bn, C, generator=g).to(dev, BF)
    y = torch.randn(Bn, 4 * C, generator=g).to(dev, BF)
    idx = _idx(Bn).to(dev)
    rf.lora_add(y.clone(), x, a, b, stack.scale, idx)  # warm-up
    step = CapturedStep(lambda: rf.lora_add(y, x, a, b, stack.scale, idx), dev)
    for r in range(4):
        x.copy_(torch.randn(Bn, C, generator=g))
        y.copy_(torch.randn(Bn, 4 * C, generator=g))
        idx.copy_(_idx(Bn).roll(r))
        if r == 2:
            stack.load(1, _state(cfg, 16, seed=77), alpha=4)  # in place: same addresses
        want = y.clone()
        rf.lora_add(want, x, a, b, stack.scale, idx)
        step.replay()
        assert torch.equal(y.view(torch.int16), want.view(torch.int16)), r


# ------------------------------------------------------------------ model and engine, bf16
def _cfg():
    return dataclasses.replace(GPT2Config.tiny(), n_embd=128, n_head=2, init_std=0.2)


def _state(cfg, r, seed, std=0.1):
    g = torch.Generator().manual_seed(seed)
    C = cfg.n_embd
    dims = {"c_attn": (C, 3 * C), "c_proj": (C, C), "c_fc": (C, 4 * C), "mlp_proj": (4 * C, C)}
    state = {}
    for layer in range(cfg.n_layer):
        for t, (din, dout) in dims.items():
            state[f"h.{layer}.{t}.lora_A"] = torch.randn(r, din, generator=g) * std
            state[f"h.{layer}.{t}.lora_B"] = torch.randn(dout, r, generator=g) * std
    return state


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(0)
    model = GPT2(_cfg()).eval().to(dev, BF)
    stack = LoRAStack(model.cfg, 2, 16, dev, BF)
    stack.load(0, _state(model.cfg, 16, seed=21), alpha=32)
    stack.load(1, _state(model.cfg, 4, seed=22), alpha=8)
    model.attach_lora(stack)
    return model


# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, adapter)
MIX = [(1, 24, 0.0, None, None, 3, 0), (5, 9, 0.8, 5, None, 11, None),
       (17, 16, 1.3, 50, 0.9, 2, 1), (40, 3, 0.8, None, 0.9, 7, 0),
       (9, 20, 1.3, None, None, -4, None), (30, 12, 0.0, 5, None, 0, 1)]


def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 512, (m[0],), generator=g).tolist() for m in MIX]


def _submit(eng, i):
    m = MIX[i]
    return eng.submit(_prompts()[i], m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                      adapter=m[6])


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


def _generate(model, rows, graph=False):
    prompts = _prompts()
    lens = [MIX[i][0] for i in rows]
    new = [MIX[i][1] for i in rows]
    idx = torch.zeros(len(rows), max(lens), dtype=torch.long)
    for b, i in enumerate(rows):
        idx[b, : lens[b]] = torch.tensor(prompts[i])
    out = model.generate(idx.to(model.wte.device), max(new), lens=lens,
                         temperature=[MIX[i][2] for i in rows], top_k=[MIX[i][3] for i in rows],
                         top_p=[MIX[i][4] for i in rows], seeds=[MIX[i][5] for i in rows],
                         adapters=[MIX[i][6] for i in rows], graph=graph).cpu()
    return [out[b, : new[b]].tolist() for b in range(len(rows))]


def test_adapters_act(cuda_device):
    """The adapters of this file's model change its tokens: the tests below compare runs
    that would also agree if no adapter were applied anywhere."""
    model = _model(cuda_device)
    rows = [0, 2, 5]
    with_ad = _generate(model, rows)
    idx = torch.zeros(len(rows), 30, dtype=torch.long)
    for b, i in enumerate(rows):
        idx[b, : MIX[i][0]] = torch.tensor(_prompts()[i])
    base = model.generate(idx.to(cuda_device), 24, lens=[MIX[i][0] for i in rows],
                          temperature=[MIX[i][2] for i in rows], top_k=[MIX[i][3] for i in rows],
                          top_p=[MIX[i][4] for i in rows], seeds=[MIX[i][5] for i in rows]).cpu()
    assert all(base[b, : MIX[i][1]].tolist() != with_ad[b] for b, i in enumerate(rows))


def test_generate_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    rows = [0, 1, 2, 3]
    assert _generate(model, rows, graph=True) == _generate(model, rows)


def test_engine_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    arrivals = {0: 0, 1: 0, 2: 2, 3: 5, 4: 6, 5: 40}  # the last long after most finished
    eager = GPT2Engine(model, slots=4, max_len=96, graph=False, poll_every=1, lora=model.lora)
    graphed = GPT2Engine(model, slots=4, max_len=96, poll_every=1, lora=model.lora)
    assert eager._graph is None and graphed._graph is not None
    a, b = _drive(eager, arrivals), _drive(graphed, arrivals)
    assert a == b
    assert [len(a[i]) for i in range(len(MIX))] == [m[1] for m in MIX]
    assert eager.steps == graphed.steps


def test_engine_equals_generate_on_the_same_rows(cuda_device):
    model = _model(cuda_device)
    rows = [0, 1, 2, 3]
    want = _generate(model, rows)
    lens = [MIX[i][0] for i in rows]
    new = [MIX[i][1] for i in rows]
    eng = GPT2Engine(model, slots=len(rows), max_len=max(lens) + max(new), poll_every=1,
                     lora=model.lora)
    rids = [_submit(eng, i) for i in rows]
    got = eng.run()
    assert [got[r] for r in rids] == want
    assert eng.steps == max(new)


def test_placement_invariance(cuda_device):
    """A request with adapter 1 admitted alone at step 7 beside two decoding requests with
    adapters 0 and -1."""
    model = _model(cuda_device)
    alone = GPT2Engine(model, slots=4, max_len=96, poll_every=1, lora=model.lora)
    rid = _submit(alone, 2)
    want = alone.run()[rid]
    busy = GPT2Engine(model, slots=4, max_len=96, poll_every=1, lora=model.lora)
    got = _drive(busy, {0: 0, 4: 0, 2: 7})
    assert got[2] == want and len(want) == MIX[2][1]
