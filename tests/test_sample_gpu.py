"""The HIP token sampler (ops/csrc/sample.hip) against the fp64 reference.

Acceptance rule (not token equality, which would hang on the summation order at interval
boundaries). With ``eps`` a bound on the kernel's error in the normalised CDF, the
candidate kept sets of a row are the strict set (value classes whose mass above is
< p - eps) and that set extended one value class at a time, from the top, over the classes
whose mass above lies in [p - eps, p + eps). The drawn token t is accepted iff for some
candidate set t is in it and u lies in [cdf_lo(t) - eps, cdf_hi(t) + eps] of that set's
fp64 CDF in index order. Top-k is decided on the stored values and is exact. Every row of
every launch is checked.

eps = 1e-5. The kernel has no floating-point addition chain at all: a weight is
exp((x - max) / T) rounded once to 2^-40 fixed point and every sum after that is an exact
integer sum, so the rounding of the sums is at most V * 2^-41 (2.3e-8 at V = 50257). What
remains is the fp32 weight itself: the argument (x - max) / T carries about three
roundings (1 / T, the product, the scaling to base 2 inside the exponential), a relative
weight error of about |arg| * 3 * 2^-24; over the tokens that carry all but 1e-6 of the
mass |arg| < 16, which gives 3e-6, below 1e-5.
"""

import dataclasses
import functools

import pytest
import torch

import ray_amd.models.gpt2 as gpt2_mod
from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

EPS = 1e-5
ROWS = 12
PARAMS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (1.3, 40, 0.95), (0.5, 1, 1.0),
          (1.0, 0, 0.01)]


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def accept(x, T, k, p, u, t, eps=EPS):
    """The acceptance rule for one row: x fp64 [V] stored values, the row's parameters,
    its uniform and the token the kernel drew. Returns None or the reason for refusal."""
    V = x.numel()
    if not 0 <= t < V:
        return f"token {t} outside [0, {V})"
    if T == 0:
        want = int((x == x.max()).nonzero()[0])
        return None if t == want else f"greedy: {t}, want {want}"
    xs, order = x.sort(descending=True)
    n_k = V
    if 0 < k < V:
        n_k = int((xs >= xs[k - 1]).sum())  # ties at the k-th value are kept
    xs, order = xs[:n_k], order[:n_k]
    ws = torch.exp(xs / T - xs[0] / T)
    total = ws.sum()
    before = (ws.cumsum(0) - ws) / total
    new_class = torch.ones(n_k, dtype=torch.bool)
    new_class[1:] = xs[1:] != xs[:-1]
    starts = new_class.nonzero().flatten()
    above = before[starts]  # normalised mass above each value class
    ends = torch.cat([starts[1:], torch.tensor([n_k])])
    if p >= 1:
        cands = [n_k]
    else:
        n_strict = int((above < p - eps).sum())  # classes; the top one always survives
        cands = [int(ends[max(n_strict, 1) - 1])]
        for c in range(max(n_strict, 1), int((above < p + eps).sum())):
            cands.append(int(ends[c]))
    rank = torch.empty(V, dtype=torch.long)
    rank[:] = V
    rank[order] = torch.arange(n_k)
    w = torch.zeros(V, dtype=torch.float64)
    w[order] = ws
    why = []
    for n in cands:
        if rank[t] >= n:
            why.append(f"token {t} (rank {int(rank[t])}) outside the {n} kept")
            continue
        wk = torch.where(rank < n, w, torch.zeros_like(w))
        tot = wk.sum()
        lo = float(wk[:t].sum() / tot)
        hi = lo + float(wk[t] / tot)
        if lo - eps <= u <= hi + eps:
            return None
        why.append(f"kept {n}: u {u:.9f} outside [{lo:.9f}, {hi:.9f}]")
    return "; ".join(why)


def _launch(x, params, seeds, steps, dev, done=None, eos=None, pad=0):
    """x [B, V] bf16 CPU; params: one (T, k, p) per row. Returns the tokens (CPU)."""
    B, V = x.shape
    if pad:
        buf = torch.full((B, V + pad), float("inf"), dtype=torch.bfloat16)
        buf[:, :V] = x
        lg = buf.to(dev)[:, :V]
    else:
        lg = x.to(dev)
    T = torch.tensor([q[0] for q in params], dtype=torch.float32, device=dev)
    k = torch.tensor([q[1] for q in params], dtype=torch.int32, device=dev)
    p = torch.tensor([q[2] for q in params], dtype=torch.float32, device=dev)
    return rf.sample_logits(lg, T, k, p, seeds.to(dev), steps.to(dev), done=done,
                            eos_token_id=eos).cpu()


def _check_rows(x, params, seeds, steps, toks, tag):
    u = ref.sample_uniform(seeds, steps, torch.float64)
    xd = x.double()
    bad = []
    for b in range(x.shape[0]):
        T, k, p = params[b]
        # (the parameters as the kernel holds them: fp32)
        why = accept(xd[b], float(torch.tensor(T, dtype=torch.float32)), k,
                     float(torch.tensor(p, dtype=torch.float32)), float(u[b]), int(toks[b]))
        if why:
            bad.append(f"{tag} row {b} {params[b]}: {why}")
    assert not bad, "\n".join(bad)


@functools.lru_cache(maxsize=None)
def _logits(V, scale, rows=ROWS):
    g = torch.Generator().manual_seed(V * 10 + scale)
    return (torch.randn(rows, V, generator=g) * scale).to(torch.bfloat16)


def _seeds(n, salt):
    return torch.arange(n, dtype=torch.int64) * 7919 + salt, \
        (torch.arange(n, dtype=torch.int32) * 13) % 1024


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("V", [50257, 1000, 65, 64, 2])
def test_kernel_against_fp64_rule(cuda_device, V, scale):
    x = _logits(V, scale)
    seeds, steps = _seeds(ROWS, V + scale)
    for i, q in enumerate(PARAMS):
        toks = _launch(x, [q] * ROWS, seeds + i, steps, cuda_device)
        assert toks.dtype == torch.int64 and toks.shape == (ROWS,)
        _check_rows(x, [q] * ROWS, seeds + i, steps, toks, f"V={V} x{scale}")
    mixed = [PARAMS[(b + scale) % len(PARAMS)] for b in range(ROWS)]
    toks = _launch(x, mixed, seeds, steps, cuda_device)
    _check_rows(x, mixed, seeds, steps, toks, f"V={V} x{scale} mixed")


@pytest.mark.parametrize("V", [8185, 8186])
def test_either_side_of_the_register_resident_limit(cuda_device, V):
    """Rows of up to 8185 logits stay in registers, longer ones are re-read per pass; an
    odd stride on top, so that the rows start at every offset inside a 16-byte slot."""
    x = _logits(V, 4)
    mixed = [PARAMS[b % len(PARAMS)] for b in range(ROWS)]
    seeds, steps = _seeds(ROWS, V)
    toks = _launch(x, mixed, seeds, steps, cuda_device, pad=47)
    _check_rows(x, mixed, seeds, steps, toks, f"V={V}")


def test_greedy_rows_with_a_planted_tie(cuda_device):
    for V in (50257, 65, 2):
        x = _logits(V, 1).clone()
        top = x.float().max() + 1
        want = []
        for b in range(ROWS):
            i, j = (b * 37) % V, (V - 1 - b * 5) % V
            x[b, i] = top
            x[b, j] = top
            want.append(min(i, j))
        seeds, steps = _seeds(ROWS, 3)
        toks = _launch(x, [(0.0, 5, 0.5)] * ROWS, seeds, steps, cuda_device)
        assert toks.tolist() == want, V


@pytest.mark.parametrize("B,V", [(1, 50257), (70, 1000)])
def test_slice_of_a_padded_buffer(cuda_device, B, V):
    """Rows at an odd stride (V + 47 elements: seven rows in eight start off a 16-byte
    boundary), the padding +inf: nothing outside the V columns may count."""
    x = _logits(V, 4, rows=B)
    params = [PARAMS[b % len(PARAMS)] for b in range(B)]
    seeds, steps = _seeds(B, 17)
    toks = _launch(x, params, seeds, steps, cuda_device, pad=47)
    _check_rows(x, params, seeds, steps, toks, f"padded B={B}")
    assert torch.equal(toks, _launch(x, params, seeds, steps, cuda_device))


def test_eos_fusion(cuda_device):
    V, B = 1000, 6
    x = _logits(V, 4, rows=B)
    params = [(0.0, 0, 1.0)] * B
    seeds, steps = _seeds(B, 1)
    free = _launch(x, params, seeds, steps, cuda_device)
    eos = int(free[2])
    want_tok = [eos if b in (0, 4) else int(free[b]) for b in range(B)]
    done = torch.zeros(B, dtype=torch.uint8)
    done[0] = done[4] = 1
    want_done = [1 if (b in (0, 4) or int(free[b]) == eos) else 0 for b in range(B)]
    d = done.to(cuda_device)
    toks = _launch(x, params, seeds, steps, cuda_device, done=d, eos=eos)
    assert toks.tolist() == want_tok
    assert d.cpu().tolist() == want_done and want_done[2] == 1 and sum(want_done) < B
    d2 = done.to(cuda_device)  # without an eos the flags are neither read nor written
    assert torch.equal(_launch(x, params, seeds, steps, cuda_device, done=d2, eos=None), free)
    assert torch.equal(d2.cpu(), done)


def test_bit_identity(cuda_device):
    x = _logits(50257, 4)
    params = [PARAMS[b % len(PARAMS)] for b in range(ROWS)]
    seeds, steps = _seeds(ROWS, 5)
    runs = [_launch(x, params, seeds, steps, cuda_device) for _ in range(5)]
    assert all(torch.equal(runs[0], r) for r in runs[1:])


# the frequency test of tests/test_sample_logits.py, on the kernel
CHI2_LOGITS = [0.0, 1.0, -0.5, 2.0, 0.25, -1.5, 1.5, 0.75]  # exact in bf16
CHI2_BOUND = 24.32  # the 0.001 upper quantile of chi-square with 7 degrees of freedom
CHI2_BASE = 1000
CHI2_ROWS = 4096


def test_frequencies_chi_square(cuda_device):
    n, dev = CHI2_ROWS, cuda_device
    toks = rf.sample_logits(
        torch.tensor(CHI2_LOGITS, dtype=torch.bfloat16, device=dev).repeat(n, 1),
        torch.ones(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
        torch.ones(n, device=dev),
        torch.arange(CHI2_BASE, CHI2_BASE + n, dtype=torch.int64, device=dev),
        torch.zeros(n, dtype=torch.int32, device=dev)).cpu()
    probs = torch.softmax(torch.tensor(CHI2_LOGITS, dtype=torch.float64), 0)
    counts = torch.bincount(toks, minlength=8).double()
    assert counts.numel() == 8
    stat = float(((counts - probs * n) ** 2 / (probs * n)).sum())
    print(f"chi-square over {n} kernel draws, seeds from {CHI2_BASE}: {stat:.3f}")
    assert stat < CHI2_BOUND


def test_dispatch(cuda_device):
    dev = cuda_device
    B, V = 3, 40
    x = _logits(64, 1, rows=B)[:, :V].contiguous()
    z = torch.zeros(B, dtype=torch.int32, device=dev)
    args = (torch.ones(B, device=dev), z, torch.ones(B, device=dev),
            torch.arange(B, dtype=torch.int64, device=dev), z)
    hip = rf.sample_logits(x.to(dev), *args)
    fp32 = rf.sample_logits(x.float().to(dev), *args)  # the reference, on the GPU
    assert hip.dtype == fp32.dtype == torch.int64 and hip.device.type == "cuda"
    assert torch.equal(hip, fp32)  # (40 tokens: no uniform lands within 1e-5 of an edge)
    with pytest.raises(ValueError):
        rf.sample_logits(x.to(dev), -args[0], *args[1:])
    with pytest.raises(ValueError):
        rf.sample_logits(x.to(dev), args[0].cpu(), *args[1:])


# ----------------------------------------------------------------------------- model
PROMPT_LENS = (1, 5, 17)
NEW = 16
ROW_PARAMS = dict(temperature=[0.8, 1.3, 0.0], top_k=[20, 0, 0], top_p=[0.9, 1.0, 0.7],
                  seeds=[3, 4, 5])


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(0)
    cfg = dataclasses.replace(GPT2Config.tiny(), init_std=0.2, n_embd=128, n_head=2)
    m = GPT2(cfg).eval().to(dev, torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size, (len(PROMPT_LENS), max(PROMPT_LENS)), generator=g)
    for b, n in enumerate(PROMPT_LENS):
        prompts[b, n:] = 0
    return m, prompts.to(dev)


def test_generate_graph_equals_eager_and_captures_the_sampler(cuda_device, monkeypatch):
    model, prompts = _model(cuda_device)
    lens = list(PROMPT_LENS)
    eager = model.generate(prompts, NEW, lens=lens, **ROW_PARAMS)
    assert eager.dtype == torch.int64 and eager.shape == (len(lens), NEW)
    greedy = model.generate(prompts, NEW, lens=lens)
    assert torch.equal(eager[2], greedy[2]) and not torch.equal(eager[0], greedy[0])

    steps, calls = [], []
    capture, sample = gpt2_mod._SeededSampler.capture, rf.sample_logits

    def recording_capture(self):
        steps.append(self)
        capture(self)

    def counting_sample(*a, **kw):
        calls.append(torch.cuda.is_current_stream_capturing())
        return sample(*a, **kw)

    monkeypatch.setattr(gpt2_mod._SeededSampler, "capture", recording_capture)
    monkeypatch.setattr(rf, "sample_logits", counting_sample)
    graph = model.generate(prompts, NEW, lens=lens, graph=True, **ROW_PARAMS)
    assert torch.equal(graph, eager)
    # the sampler ran once eagerly (the warm-up step) and once under capture; the other
    # NEW - 1 tokens came out of replays, with no launch from Python between them
    assert calls == [False, True]
    (step,) = steps
    assert step.graph is not None
    assert torch.equal(step.tok, graph[:, -1])  # the graph's static token buffer -> out
    assert int(step.col) == NEW


def test_generate_row_alone_equals_row_in_a_mixed_batch(cuda_device):
    model, prompts = _model(cuda_device)
    lens = list(PROMPT_LENS)
    mixed = model.generate(prompts, NEW, lens=lens, **ROW_PARAMS)
    for b, n in enumerate(PROMPT_LENS):
        alone = model.generate(prompts[b:b + 1, :n], NEW,
                               **{k: [v[b]] for k, v in ROW_PARAMS.items()})
        assert torch.equal(alone[0], mixed[b]), b
