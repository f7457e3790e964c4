"""Per-block paths of the attention kernels: the LDS-staged whole-row output stores of the
forward and dQ kernels, the dK/dV stores, and the pairing of causal blocks in one workgroup,
at block counts where a store path or a pairing can go wrong (one block, one pair, an odd
count with an unpaired middle block, two pairs plus a middle block) and with neighbouring
heads' columns beside the head that is written (GPU only)."""

import functools

import pytest
import torch

from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu

B, D = 2, 64
SHAPES = [(T, H) for T in (128, 256, 384, 640) for H in (1, 3)]
GUARD = 4096  # sentinel elements on each side of a carved tensor (a multiple of 8: 16-B stores)


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"
    yield
    # hand the shared references and the allocator's cached blocks back, so the modules that
    # run after this one start from the same allocator state as without it
    _case.cache_clear()
    torch.cuda.empty_cache()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _case(T, H):
    """Inputs and the fp32 autograd reference of test_flash_attention_fwd_bwd, computed once
    per shape."""
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(9 + 1000 * T + H)
    qkv = torch.randn(B, T, 3, H, D, device=dev, generator=gen).bfloat16()
    g = torch.randn(B, T, H, D, device=dev, generator=gen)
    ref_in = qkv.float().requires_grad_()
    q, k, v = ref_in.permute(2, 0, 3, 1, 4).unbind(0)
    s = (q @ k.transpose(-1, -2)) * D ** -0.5
    mask = torch.ones(T, T, device=dev, dtype=torch.bool).triu(1)
    p = torch.softmax(s.masked_fill(mask, float("-inf")), -1)
    yr = (p @ v).transpose(1, 2)
    yr.backward(g)
    return qkv, g.bfloat16(), yr.detach(), ref_in.grad.detach()


def _carved(shape, dtype, dev):
    """A tensor of `shape` inside a larger sentinel-filled buffer: (whole buffer, view)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev, dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _raw_fwd_bwd(qkv, dout):
    """ra_attn_fwd / ra_attn_bwd on carved out / dqkv buffers → (out buffer, out, lse, dqkv
    buffer, dqkv)."""
    dev = qkv.device
    _, T, _, H, _ = qkv.shape
    L = _lib.lib()
    obuf, out = _carved((B, T, H, D), torch.bfloat16, dev)
    gbuf, dqkv = _carved((B, T, 3, H, D), torch.bfloat16, dev)
    lse = torch.empty(B, H, T, device=dev, dtype=torch.float32)
    delta = torch.empty_like(lse)
    _lib.check(L.ra_attn_fwd(ptr(qkv), ptr(out), ptr(lse), B, T, H, D, D ** -0.5, stream_ptr()),
               "attn_fwd")
    _lib.check(L.ra_attn_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv),
                             B, T, H, D, D ** -0.5, stream_ptr()), "attn_bwd")
    torch.cuda.synchronize()
    return obuf, out, lse, gbuf, dqkv


@pytest.mark.parametrize("T,H", SHAPES)
def test_attn_blocks_match_fp32_autograd(cuda_device, T, H):
    qkv, g, yr, gr = _case(T, H)
    x = qkv.clone().requires_grad_()
    y = rf.causal_attention_qkv(x)
    assert _rel(y, yr) < 1e-2
    y.backward(g)
    for i in range(3):
        assert _rel(x.grad[:, :, i], gr[:, :, i]) < 2e-2, i


@pytest.mark.parametrize("T,H", SHAPES)
def test_attn_blocks_stay_in_bounds_and_write_everything(cuda_device, T, H):
    qkv, g, yr, gr = _case(T, H)
    obuf, out, _, gbuf, dqkv = _raw_fwd_bwd(qkv, g)
    sentinel = torch.full((GUARD,), float("nan"), device=cuda_device,
                          dtype=torch.bfloat16).view(torch.int16)
    for buf in (obuf, gbuf):
        raw = buf.view(torch.int16)
        assert torch.equal(raw[:GUARD], sentinel)
        assert torch.equal(raw[-GUARD:], sentinel)
    assert torch.isfinite(out.float()).all()
    assert torch.isfinite(dqkv.float()).all()
    # the raw entry points computed the same thing as the reference
    assert _rel(out, yr) < 1e-2
    for i in range(3):
        assert _rel(dqkv[:, :, i], gr[:, :, i]) < 2e-2, i


@pytest.mark.parametrize("T,H", [(384, 3), (640, 1)])
def test_attn_blocks_deterministic(cuda_device, T, H):
    qkv, g, _, _ = _case(T, H)
    _, out1, lse1, _, dqkv1 = _raw_fwd_bwd(qkv, g)
    _, out2, lse2, _, dqkv2 = _raw_fwd_bwd(qkv, g)
    assert torch.equal(out1.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(lse1, lse2)
    assert torch.equal(dqkv1.view(torch.int16), dqkv2.view(torch.int16))
