"""Weight-only int8 (``GPT2.quantize_weights``) on the CPU reference path: the quantiser's
error bound, and a quantised model against a copy that holds the dequantised weights as its
parameters (same fp32 arithmetic, so exactly the same tokens and scores), through
``generate``, ``score``, the engine and serve.llm."""

import asyncio
import copy
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.serve.llm import build_gpt2_app

SEED = 11
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
PROMPTS = torch.tensor([[5, 17, 300, 42, 8, 99, 123], [7, 3, 1, 4, 1, 5, 9]])


def test_quantize_w8_bound_and_zero_rows():
    torch.manual_seed(0)
    w = torch.randn(24, 96) * torch.logspace(-3, 2, 24)[:, None]
    w[5] = 0
    q, s = rf.quantize_w8(w)
    assert q.dtype == torch.int8 and s.dtype == torch.float32
    err = (w.double() - q.double() * s.double()[:, None]).abs()
    assert (err <= s.double()[:, None] * (0.5 + 2.0 ** -10)).all()
    nz = torch.arange(24) != 5
    assert (q[nz].abs().amax(1) == 127).all()
    assert s[5] == 0 and (q[5] == 0).all()


@pytest.fixture(scope="module")
def models():
    """(quantised model, copy with the dequantised weights as parameters). The embedding keeps
    reading ``wte``, so ``wte`` is first put on its own int8 grid: both models embed alike."""
    torch.manual_seed(SEED)
    qm = GPT2(CFG).eval()
    with torch.no_grad():
        qm.wte.copy_(ref.dequant_w8(*rf.quantize_w8(qm.wte), torch.float32))
    plain = copy.deepcopy(qm)
    qm.quantize_weights()
    with torch.no_grad():
        for t in GPT2.W8_TARGETS:
            for blk, (q, s) in zip(plain.h, qm.w8[t]):
                getattr(blk, t + "_w").copy_(ref.dequant_w8(q, s, torch.float32))
        plain.wte.copy_(ref.dequant_w8(*qm.w8["wte"], torch.float32))
    assert torch.equal(plain.wte, qm.wte)
    assert not torch.equal(plain.h[0].c_fc_w, qm.h[0].c_fc_w)  # the linears did move
    return qm, plain


@pytest.mark.parametrize("kw", [{}, {"temperature": 0.9, "top_k": 20, "seeds": [3, 4]}],
                         ids=["greedy", "seeded"])
def test_generate_equals_dequantised_copy(models, kw):
    qm, plain = models
    assert torch.equal(qm.generate(PROMPTS, 12, **kw), plain.generate(PROMPTS, 12, **kw))


def test_score_equals_dequantised_copy_and_state_dict_is_unchanged(models):
    qm, plain = models
    a, ai, al = qm.score(PROMPTS, top_n=2)
    b, bi, bl = plain.score(PROMPTS, top_n=2)
    assert torch.equal(a[:, 1:], b[:, 1:]) and torch.equal(ai, bi)
    assert torch.equal(al[:, 1:], bl[:, 1:])
    assert qm.state_dict().keys() == plain.state_dict().keys()
    assert copy.deepcopy(qm).dequantize_weights().w8 is None


def test_engine_returns_generates_tokens(models):
    qm, _ = models
    reqs = [([5, 17, 300, 42], 10, 0.0, 0), ([9, 8, 7], 6, 0.9, 5)]
    want = [qm.generate(torch.tensor([t]), n, temperature=temp, seeds=[seed])[0].tolist()
            for t, n, temp, seed in reqs]
    eng = GPT2Engine(qm, slots=2, graph=False, poll_every=1)
    got = {}
    rid0 = eng.submit(reqs[0][0], reqs[0][1], temperature=reqs[0][2], seed=reqs[0][3])
    for _ in range(3):  # the second request arrives while the first decodes
        for ev in eng.step():
            got.setdefault(ev[0], []).extend(ev[1])
    rid1 = eng.submit(reqs[1][0], reqs[1][1], temperature=reqs[1][2], seed=reqs[1][3])
    for rid, toks in eng.run().items():
        got.setdefault(rid, []).extend(toks)
    assert [got[rid0], got[rid1]] == want


@pytest.mark.parametrize("continuous", [False, True])
def test_serve_int8(models, continuous):
    qm, _ = models
    with pytest.raises(ValueError):
        build_gpt2_app(config="tiny", weights="int4", device="cpu", continuous=continuous)
    app = build_gpt2_app(config=CFG, seed=SEED, weights="int8", device="cpu",
                         continuous=continuous)
    srv = app.deployment.func_or_class(*app.args, **app.kwargs)
    try:
        # the server's model is the seeded init, quantised: compare with that, made here
        torch.manual_seed(SEED)
        mine = GPT2(CFG).eval().quantize_weights()
        want = mine.generate(PROMPTS[:1], 8, seeds=[SEED])[0].tolist()
        req = {"tokens": PROMPTS[0].tolist(), "max_new_tokens": 8}
        if continuous:
            assert asyncio.run(srv(req)) == {"tokens": want}
        else:
            assert srv.model.w8 is not None
            assert srv._run([req]) == [want]
    finally:
        if continuous:
            srv.close()
