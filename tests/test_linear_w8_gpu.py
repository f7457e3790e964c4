"""``rf.linear_w8`` / ``rf.dequant_w8`` (ops/csrc/linear_w8.hip) against fp64 on the GPU: the
fragment layout on integer data (exact), a derived per-element bound on random data, the
invariance of a row's bits, the dequantiser, and a quantised tiny GPT-2."""

import copy
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.ops import functional as rf

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref64(x, q, s, b):
    y = (x.double() @ q.double().t()) * s.double()
    return y if b is None else y + b.double()


@pytest.fixture
def skinny(monkeypatch):
    monkeypatch.setattr(rf, "W8_SKINNY_MAX_M", 1 << 20)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("K", [32, 64, 96, 1600])
@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("M", [1, 33, 129])
def test_layout_exact_on_integers(skinny, M, N, K, splits, bias):
    # every partial sum is an integer below 4 * 127 * 1600 < 2^24 and s * acc + b a multiple
    # of 1/8 below 2^20: exact in fp32 in any order, so only the one rounding to bf16 is left
    g = torch.Generator().manual_seed(M * 7 + N + K + splits)
    x = torch.randint(-4, 5, (M, K), generator=g).to(DEV, torch.bfloat16)
    q = torch.randint(-127, 128, (N, K), generator=g).to(DEV, torch.int8)
    q[0, 0], q[-1, -1] = 127, -127
    s = (2.0 ** -(torch.arange(N) % 4).float()).to(DEV)
    b = torch.randint(-8, 9, (N,), generator=g).to(DEV, torch.bfloat16) if bias else None
    y = rf.linear_w8(x, q, s, b, splits=splits)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    assert torch.equal(y, _ref64(x, q, s, b).float().bfloat16())


@pytest.mark.parametrize("M,N,K,wide", [(8, 2304, 768, 0), (8, 768, 3072, 0), (3, 512, 64, 640)])
def test_numerics_against_fp64(M, N, K, wide):
    g = torch.Generator().manual_seed(N + K)
    x = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
    q = torch.randint(-127, 128, (N, K), generator=g).to(DEV, torch.int8)
    s = (torch.rand(N, generator=g) * 0.01 + 1e-4).to(DEV)
    b = torch.randn(N, generator=g).to(DEV, torch.bfloat16)
    out = None
    if wide:
        buf = torch.full((M, wide), -7.5, device=DEV, dtype=torch.bfloat16)
        out = buf[:, :N]
    y = rf.linear_w8(x, q, s, b, out=out)
    want = _ref64(x, q, s, b)
    # one bf16 rounding (2^-9 relative) and fp32 accumulation (at most K * 2^-24 of the
    # absolute sum), each doubled
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -23 * s.double() * (
        x.double().abs() @ q.double().abs().t())
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
    q = torch.randint(-127, 128, (N, K), generator=g).to(DEV, torch.int8)
    s = (torch.rand(N, generator=g) * 0.01 + 1e-4).to(DEV)
    b = torch.randn(N, generator=g).to(DEV, torch.bfloat16)
    y = rf.linear_w8(x, q, s, b)
    for j in (0, 31, 36):
        assert torch.equal(rf.linear_w8(x[j:j + 1], q, s, b)[0], y[j]), j


@pytest.mark.parametrize("N,K", [(96, 64), (50304, 768)])
def test_dequant_exact(N, K):
    g = torch.Generator().manual_seed(N)
    q = torch.randint(-127, 128, (N, K), generator=g).to(DEV, torch.int8)
    s = (torch.rand(N, generator=g) * 0.01).to(DEV)
    assert torch.equal(rf.dequant_w8(q, s), (q.float() * s[:, None]).bfloat16())


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

    gpu.quantize_weights()
    cpu.w8 = {t: tuple(v.cpu() for v in e) if t == "wte" else [(q.cpu(), s.cpu()) for q, s in e]
              for t, e in gpu.w8.items()}  # the same int8 weights on the fp32 reference path
    diff = (_step_logits(gpu, idx, tok) - _step_logits(cpu, idx, tok)).abs().max().item()
    print(f"unquantised bf16-vs-fp32 {yard:.5f}, quantised {diff:.5f}")
    assert diff <= 2 * yard

    kw = dict(temperature=0.8, top_k=20, seeds=0)
    eager = gpu.generate(idx.to(DEV), 12, **kw)
    assert torch.equal(gpu.generate(idx.to(DEV), 12, graph=True, **kw), eager)
