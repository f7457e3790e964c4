"""``rf.linear_w4`` / ``rf.dequant_w4`` (ops/csrc/linear_w4.hip) against fp64 on the GPU: the
fragment layout on integer data (exact), a derived per-element bound on random data, the
invariance of a row's bits, the dequantiser (nibble order and scale operand of the convert
instruction), and an MXFP4 tiny GPT-2."""

import copy
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _weights(g, N, K, s_lo, s_hi):
    """Random MXFP4 bytes on the GPU with scale bytes in [s_lo, s_hi] varying per block, all 16
    codes present and the extremes (+6, -6) at the first and last element; and dq in fp64."""
    q = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    q[0, 1:9] = torch.arange(8, dtype=torch.uint8) * 0x22 + 0x10  # codes 0..15
    q[0, 0] = (q[0, 0] & 0xF0) | 0x7
    q[-1, -1] = (q[-1, -1] & 0x0F) | 0xF0
    q = q.to(DEV)
    s = torch.randint(s_lo, s_hi + 1, (N, K // 32), generator=g).to(DEV, torch.uint8)
    return q, s, ref.dequant_w4(q, s, torch.float64)


def _ref64(x, dq, b):
    y = x.double() @ dq.t()
    return y if b is None else y + b.double()


@pytest.fixture
def skinny(monkeypatch):
    monkeypatch.setattr(rf, "W4_SKINNY_MAX_M", 1 << 20)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("K", [64, 192, 1600])
@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("M", [1, 33, 129])
def test_layout_exact_on_integers(skinny, M, N, K, splits, bias):
    # x is an integer in [-4, 4], an e2m1 value a multiple of 1/2 up to 6 and a scale 2^-2..2^2:
    # every product is a multiple of 1/8 of at most 4 * 24, so every partial sum is below
    # 1600 * 4 * 24 * 8 < 2^24 in units of 1/8 and the bias (an integer) keeps that: fp32 is
    # exact in any order and only the one rounding to bf16 is left
    g = torch.Generator().manual_seed(M * 7 + N + K + splits)
    x = torch.randint(-4, 5, (M, K), generator=g).to(DEV, torch.bfloat16)
    q, s, dq = _weights(g, N, K, 125, 129)
    b = torch.randint(-8, 9, (N,), generator=g).to(DEV, torch.bfloat16) if bias else None
    y = rf.linear_w4(x, q, s, b, splits=splits)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    assert torch.equal(y, _ref64(x, dq, b).float().bfloat16())


@pytest.mark.parametrize("M,N,K,wide", [(8, 2304, 768, 0), (8, 768, 3072, 0), (3, 512, 64, 640)])
def test_numerics_against_fp64(M, N, K, wide):
    g = torch.Generator().manual_seed(N + K)
    x = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
    q, s, dq = _weights(g, N, K, 100, 150)
    b = torch.randn(N, generator=g).to(DEV, torch.bfloat16)
    out = None
    if wide:
        buf = torch.full((M, wide), -7.5, device=DEV, dtype=torch.bfloat16)
        out = buf[:, :N]
    y = rf.linear_w4(x, q, s, b, out=out)
    want = _ref64(x, dq, b)
    # one bf16 rounding (2^-9 relative) and fp32 accumulation (at most K * 2^-24 of the
    # absolute sum), each doubled
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -23 * (x.double().abs() @ dq.abs().t())
    err = (y.double() - want).abs()
    print(f"M={M} N={N} K={K}: max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    if wide:
        assert y.data_ptr() == buf.data_ptr()
        assert (buf[:, N:] == -7.5).all()


def test_a_rows_bits_do_not_depend_on_the_batch():
    g = torch.Generator().manual_seed(5)
    N, K = 768, 3072
    x = torch.randn(37, K, generator=g).to(DEV, torch.bfloat16)
    q, s, _ = _weights(g, N, K, 100, 150)
    b = torch.randn(N, generator=g).to(DEV, torch.bfloat16)
    y = rf.linear_w4(x, q, s, b)
    for j in (0, 31, 36):
        assert torch.equal(rf.linear_w4(x[j:j + 1], q, s, b)[0], y[j]), j


@pytest.mark.parametrize("N,K", [(96, 64), (50304, 768)])
def test_dequant_exact(N, K):
    if N == 96:  # every byte value, so every code in both nibbles, at six scale bytes
        q = torch.arange(256, dtype=torch.uint8).repeat(12).view(96, 32).to(DEV)
        s = torch.tensor([100, 113, 126, 127, 128, 150], dtype=torch.uint8).repeat(32)
        s = s.view(96, 2).to(DEV)
        dq = ref.dequant_w4(q, s, torch.float64)
    else:
        q, s, dq = _weights(torch.Generator().manual_seed(N), N, K, 100, 150)
    got = rf.dequant_w4(q, s)
    assert got.dtype == torch.bfloat16 and torch.equal(got, ref.dequant_w4(q, s))
    assert torch.equal(got.double(), dq)  # and bf16 holds the value exactly


def _step_logits(model, idx, tok):
    """The logits of ``prefill`` and of one ``decode_step`` on ``tok``, fp32 on the CPU."""
    dev = model.wte.device
    cache = KVCache(model.cfg, idx.shape[0], idx.shape[1] + 1, dev, model.wte.dtype)
    a = model.prefill(idx.to(dev), [idx.shape[1]] * idx.shape[0], cache)
    b = model.decode_step(tok.to(dev), cache)
    return torch.cat([a, b]).float().cpu()


def test_quantised_tiny_model():
    cfg = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
    torch.manual_seed(3)
    gpu = GPT2(cfg).eval().to(DEV, torch.bfloat16)
    cpu = copy.deepcopy(gpu).float().cpu()  # the same (bf16-valued) parameters in fp32
    idx = torch.randint(0, cfg.vocab_size, (4, 24), generator=torch.Generator().manual_seed(1))
    tok = torch.randint(0, cfg.vocab_size, (4,), generator=torch.Generator().manual_seed(2))
    # the yardstick, from the existing path: what bf16 on the GPU costs the unquantised model
    yard = (_step_logits(gpu, idx, tok) - _step_logits(cpu, idx, tok)).abs().max().item()

    gpu.quantize_weights(fmt="mxfp4")
    cpu.w8 = {t: tuple(v.cpu() for v in e) if t == "wte" else [(q.cpu(), s.cpu()) for q, s in e]
              for t, e in gpu.w8.items()}  # the same MXFP4 weights on the fp32 reference path
    diff = (_step_logits(gpu, idx, tok) - _step_logits(cpu, idx, tok)).abs().max().item()
    print(f"unquantised bf16-vs-fp32 {yard:.5f}, quantised {diff:.5f}")
    assert diff <= 2 * yard

    kw = dict(temperature=0.8, top_k=20, seeds=0)
    eager = gpu.generate(idx.to(DEV), 12, **kw)
    assert torch.equal(gpu.generate(idx.to(DEV), 12, graph=True, **kw), eager)
