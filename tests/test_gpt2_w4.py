"""Weight-only MXFP4 (``GPT2.quantize_weights(fmt="mxfp4")``) on the CPU reference path: the
quantiser's format and error bound, a quantised model against a copy that holds the
dequantised weights as its parameters (same fp32 arithmetic, so exactly the same tokens),
serve.llm with both servers, and the rejected arguments."""

import asyncio
import copy
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.serve.llm import build_gpt2_app

SEED = 11
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
PROMPTS = torch.tensor([[5, 17, 300, 42, 8, 99, 123], [7, 3, 1, 4, 1, 5, 9]])
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def test_grid_weights_round_trip():
    # every code of both signs (with 6 in each block, so the block's exponent is the row's),
    # at several exponents
    exps = torch.tensor([-20.0, -3.0, 0.0, 1.0, 9.0])
    blk = torch.cat([GRID, -GRID, GRID.flip(0), -GRID.flip(0)])
    w = blk[None, :] * torch.exp2(exps)[:, None]
    q, s = rf.quantize_w4(w)
    assert q.dtype == torch.uint8 and q.shape == (5, 16)
    assert s.dtype == torch.uint8 and s.flatten().tolist() == (exps + 127).int().tolist()
    assert q[0, :4].tolist() == [0x10, 0x32, 0x54, 0x76]  # low nibble first
    assert torch.equal(ref.dequant_w4(q, s, torch.float32), w)


def test_quantiser_bound_ties_and_zero_block():
    torch.manual_seed(0)
    w = torch.randn(24, 96) * torch.logspace(-3, 2, 24)[:, None]
    w[5, 32:64] = 0
    # a block with amax 6 (e = 0) that holds the tie cases, and one with amax 6.5 (e = 1)
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    w[7, :32] = torch.tensor([6.0] + ties + [-t for t in ties] + [0.0] * 17)
    w[8, :32] = torch.tensor([6.5] + [0.0] * 31)
    q, s = rf.quantize_w4(w)
    dq = ref.dequant_w4(q, s, torch.float32)
    e = s.double() - 127
    amax = w.view(24, 3, 32).abs().amax(2).double()
    nz = amax > 0
    # e is the smallest exponent at which nothing saturates; the error is at most half the
    # largest grid step (2) times the scale
    assert (6 * torch.exp2(e)[nz] >= amax[nz]).all()
    assert (6 * torch.exp2(e - 1)[nz] < amax[nz]).all()
    err = (w - dq).double().view(24, 3, 32).abs()
    assert (err <= torch.exp2(e)[:, :, None]).all()
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert s[7, 0] == 127 and dq[7, 1:15].tolist() == want + [-v for v in want]
    assert s[8, 0] == 128 and dq[8, 0] == 6.0
    assert s[5, 1] == 127 and (q[5, 16:32] == 0).all()


@pytest.fixture(scope="module")
def models():
    """(quantised model, copy with the dequantised weights as parameters). The embedding keeps
    reading ``wte``, so ``wte`` is first put on its own MXFP4 grid: both models embed alike."""
    torch.manual_seed(SEED)
    qm = GPT2(CFG).eval()
    with torch.no_grad():
        qm.wte.copy_(ref.dequant_w4(*rf.quantize_w4(qm.wte), torch.float32))
    plain = copy.deepcopy(qm)
    qm.quantize_weights(fmt="mxfp4")
    with torch.no_grad():
        for t in GPT2.W8_TARGETS:
            for blk, (q, s) in zip(plain.h, qm.w8[t]):
                assert q.dtype == torch.uint8 and s.dtype == torch.uint8
                getattr(blk, t + "_w").copy_(ref.dequant_w4(q, s, torch.float32))
    assert torch.equal(ref.dequant_w4(*qm.w8["wte"], torch.float32), qm.wte)
    return qm, plain


@pytest.mark.parametrize("kw", [{}, {"temperature": 0.9, "top_k": 20, "seeds": [3, 4]}],
                         ids=["greedy", "seeded"])
def test_generate_equals_dequantised_copy(models, kw):
    qm, plain = models
    assert torch.equal(qm.generate(PROMPTS, 12, **kw), plain.generate(PROMPTS, 12, **kw))
    assert copy.deepcopy(qm).dequantize_weights().w8 is None


@pytest.mark.parametrize("continuous", [False, True])
def test_serve_mxfp4_with_int8_kv_cache(continuous):
    app = build_gpt2_app(config=CFG, seed=SEED, weights="mxfp4", kv_cache="int8", device="cpu",
                         continuous=continuous)
    srv = app.deployment.func_or_class(*app.args, **app.kwargs)
    try:
        # the server's model is the seeded init, quantised: compare with that, made here
        torch.manual_seed(SEED)
        mine = GPT2(CFG).eval().quantize_weights(fmt="mxfp4")
        want = mine.generate(PROMPTS[:1], 8, seeds=[SEED], kv_cache="int8")[0].tolist()
        req = {"tokens": PROMPTS[0].tolist(), "max_new_tokens": 8}
        if continuous:
            assert asyncio.run(srv(req)) == {"tokens": want}
        else:
            assert srv.model.w8["wte"][0].dtype == torch.uint8
            assert srv._run([req]) == [want]
    finally:
        if continuous:
            srv.close()


def test_bad_values_raise():
    q, s = rf.quantize_w4(torch.randn(32, 64))
    x = torch.randn(2, 64)
    with pytest.raises(ValueError):
        GPT2(CFG).quantize_weights(fmt="int4")
    with pytest.raises(ValueError):
        rf.quantize_w4(torch.randn(32, 48))
    for bq, bs in [(q.to(torch.int8), s), (q, s.float()), (q[:, :24], s), (q, s[:, :1]),
                   (q, s[:16]), (q[0], s)]:
        with pytest.raises(ValueError):
            rf.linear_w4(x, bq, bs)
        with pytest.raises(ValueError):
            rf.dequant_w4(bq, bs)
    with pytest.raises(ValueError):
        rf.linear_w4(torch.randn(2, 32), q, s)
