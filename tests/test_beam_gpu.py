"""The beam-search kernels (ops/csrc/beam.hip) against ``ops/reference.py`` fed fp64 logits, and
``GPT2.generate(num_beams=...)`` captured, eager and through the reference (GPU)."""

import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

EOS = 13
PAD_V = 50304
STEPS = 3
MARGIN = 1e-4


def step_logits(G, W, V, step):
    """Seeded bf16 logits [G * W, V] (CPU) with a planted EOS column (the best of group 0's
    rows at step 1, far down otherwise), duplicated values inside every row, two equal top
    values at step 0 (two beams leave it with equal scores), a duplicated row afterwards and,
    at step 2, a last row that is constant but for eight columns (every candidate ties)."""
    x = torch.randn(G * W, V, generator=torch.Generator().manual_seed(1000 * step + 10 * W + G))
    x = (x * 3).to(torch.bfloat16)
    x[:, 2] = float("-inf")
    x[:, 11] = x[:, 4] = x.max(-1).values
    x[:, EOS] = -40.0
    if step == 0:
        x[:, 7] = x[:, 9] = x.max(-1).values + 1
    if step == 1:
        x[:W, EOS] = x[:W].max(-1).values + 1
    if step > 0 and W > 1:
        x[1] = x[0]
    if step == 2:
        x[-1, 8:] = 1.0
    return x


def margins_ok(x, score, W):
    """The test's condition on its inputs, from the fp64 reference alone: consecutive distinct
    values among each row's, and each group's, first 2W + 1 candidates differ by MARGIN."""
    lp = torch.log_softmax(x.double(), -1)
    n = min(2 * W + 1, x.shape[1])
    rows = (score.double().view(-1, 1) + lp).topk(n, -1).values
    for c in list(rows) + list(rows.view(-1, W * n).sort(-1, descending=True).values[:, :n]):
        d = (c[:-1] - c[1:])[torch.isfinite(c[1:])]
        if bool(((d != 0) & (d < MARGIN)).any()):
            return False
    return True


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("V", [17, 50257])
def test_beam_step_matches_reference(V, off, W, G):
    """Scores within 1e-5 per step taken: under 4e-6 for lp (the logprobs kernel's documented
    error against fp64) plus one fp32 rounding of a sum below 64, 2^-18 = 3.8e-6."""
    N = G * W
    buf = torch.zeros(N, PAD_V, dtype=torch.bfloat16, device="cuda")
    view = buf[:, off: off + V]
    got = rf.beam_state(G, W, STEPS + 1, EOS, 1.0, False, "cuda")
    want = ref.beam_state(G, W, STEPS + 1, EOS, 1.0, False)
    for step in range(STEPS):
        x = step_logits(G, W, V, step)
        assert margins_ok(x, want["score"], W)
        view.copy_(x)
        rf.beam_step(view, got)
        ref.beam_step(x.double(), want)
        for key in ("tok", "parent", "done", "step", "hyp_n"):
            assert got[key].cpu().tolist() == want[key].tolist(), (key, step)
        assert torch.equal(got["tok_hist"][: step + 1].cpu(), want["tok_hist"][: step + 1])
        assert torch.equal(got["par_hist"][: step + 1].cpu(), want["par_hist"][: step + 1])
        held = torch.arange(W).view(1, W) < want["hyp_n"].view(G, 1)
        for key in ("hyp_step", "hyp_par", "hyp_ord"):
            assert torch.equal(got[key].cpu()[held], want[key][held]), (key, step)
        tol = 1e-5 * (step + 1)
        for key, keep in (("score", slice(None)), ("hyp_score", held)):
            a, b = got[key].cpu()[keep], want[key][keep]
            fin = torch.isfinite(b)
            assert torch.equal(a[~fin], b[~fin]) and bool(((a[fin] - b[fin]).abs() <= tol).all())
    assert int(want["hyp_n"].sum()) > 0  # the planted EOS made hypotheses


@pytest.mark.parametrize("n", [1, 64, 65, 70])
def test_beam_kv_fork_bitwise(n):
    L, S, H, T, D = 2, 8, 2, 70, 64
    g = torch.Generator().manual_seed(n)
    k = torch.randn(L, S, H, T, D, generator=g).to(torch.bfloat16).cuda()
    v = torch.randn(L, S, H, T, D, generator=g).to(torch.bfloat16).cuda()
    # rows 1..3: a three-way fork of row 0; 4: itself; 5: out of range; 6: its parent is a
    # destination; 7: an inactive length
    parent = torch.tensor([0, 0, 0, 0, 4, 99, 1, 4], dtype=torch.int32, device="cuda")
    lens = torch.full((S,), n, dtype=torch.int32, device="cuda")
    lens[7] = rf.SLOT_INACTIVE
    wk, wv = k.clone(), v.clone()
    ref.beam_kv_fork(wk, wv, parent, lens)
    assert torch.equal(wk[:, 1, :, :n], k[:, 0, :, :n]) and not torch.equal(wk, k)
    rf.beam_kv_fork(k, v, parent, lens)
    assert torch.equal(k, wk) and torch.equal(v, wv)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("steps", [1, 9])
def test_beam_backtrace_exact(steps, R):
    G, W, V = 2, 3, 24
    st = ref.beam_state(G, W, 9, EOS, 0.7, False)
    for step in range(steps):
        x = torch.randn(G * W, V, generator=torch.Generator().manual_seed(step))
        if step in (2, 5):
            x[:W, EOS] = 5.0
        ref.beam_step(x, st)
    dev = {k: t.cuda() if isinstance(t, torch.Tensor) else t for k, t in st.items()}
    for a, b in zip(rf.beam_backtrace(dev, R), ref.beam_backtrace(st, R)):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b)
    assert steps == 1 or int(st["hyp_n"][0]) > 0


def test_generate_graph_eager_reference(monkeypatch):
    # tiny() with heads of 64, the size the cache kernels take: every op of the step is HIP
    cfg = dataclasses.replace(GPT2Config.tiny(), init_std=0.2, n_embd=128, n_head=2)
    torch.manual_seed(3)
    model = GPT2(cfg).to("cuda", torch.bfloat16).eval()
    idx = torch.randint(0, cfg.vocab_size, (2, 9), generator=torch.Generator().manual_seed(4))
    idx = idx.cuda()
    eos = int(model.generate(idx, 12)[0, 5])
    kw = dict(eos_token_id=eos, num_beams=3, num_return_sequences=3, lens=[9, 6])
    eager = model.generate(idx, 12, **kw)
    graph = model.generate(idx, 12, graph=True, **kw)
    for a, b in zip(eager, graph):
        assert torch.equal(a, b)
    assert int(eager[2].min()) < 12  # a hypothesis ended with EOS
    for name in ("beam_step", "beam_kv_fork", "beam_backtrace"):
        monkeypatch.setattr(rf, name, getattr(ref, name))
    want = model.generate(idx, 12, **kw)
    assert torch.equal(eager[0], want[0]) and torch.equal(eager[2], want[2])
    assert float((eager[1] - want[1]).abs().max()) < 1e-4
