"""Staging of the weight-gradient kernel (ops/csrc/wgrad.hip), checked exactly (GPU only).

Operands are integer-valued bf16 in [-8, 8] and M <= 1024, so every product (<= 64), every
partial sum and every slab sum (<= 2^16) is an integer below 2^24: exact in fp32 whatever
the summation order. The kernel's output therefore has to EQUAL the fp64 reference cast to
the sink's dtype (both casts round to nearest even) — one misplaced 16-byte chunk or one
token row staged twice cannot hide in a norm.
"""

import functools

import pytest
import torch

from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _ints(shape, seed, device, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(device=device, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, device):
    """(dY, X, fp64 dW reference, fp64 db reference), made once per shape and never written."""
    dy = _ints((M, N), 1000 + M + N, device)
    x = _ints((M, K), 2000 + M + K, device)
    return dy, x, dy.double().t() @ x.double(), dy.double().sum(0)


def _check_accumulate(dy, x, ref_w, ref_b, sdtype, accumulate, bias, seed=7):
    """wgrad_accumulate onto an integer sink == the fp64 reference in the sink's dtype."""
    N, K = ref_w.shape
    sink0 = _ints((N, K), seed, dy.device, sdtype)
    bsink0 = _ints((N,), seed + 1, dy.device, sdtype)
    sink, bsink = sink0.clone(), (bsink0.clone() if bias else None)
    assert rf._wgrad_hip_ok(dy, x, sink, bsink)
    rf.wgrad_accumulate(dy, x, sink, bsink, accumulate=accumulate)
    want_w = (ref_w + sink0.double() if accumulate else ref_w).to(sdtype)
    assert torch.equal(sink, want_w)
    if bias:
        want_b = (ref_b + bsink0.double() if accumulate else ref_b).to(sdtype)
        assert torch.equal(bsink, want_b)


@pytest.mark.parametrize("M", [64, 128, 192, 320])
def test_kstep_counts_ragged_tiles(cuda_device, M):
    """1, 2, 3 and 5 K-steps (no prefetch, both buffer parities, an odd tail) on tiles that
    are ragged in both directions, so the folded column clamp is live."""
    dy, x, ref_w, ref_b = _operands(M, 264, 136, cuda_device)
    _check_accumulate(dy, x, ref_w, ref_b, torch.float32, True, False)
    _check_accumulate(dy, x, ref_w, ref_b, torch.bfloat16, False, False)


def test_tiny_tile_every_column_clamped(cuda_device):
    """N = K = 8: one 16-byte chunk per row, every lane's column clamps to 0."""
    dy, x, ref_w, ref_b = _operands(64, 8, 8, cuda_device)
    _check_accumulate(dy, x, ref_w, ref_b, torch.float32, True, False)
    _check_accumulate(dy, x, ref_w, ref_b, torch.bfloat16, False, False)


@pytest.mark.parametrize("M,S", [(320, 2), (448, 3)])
def test_explicit_uneven_splits(cuda_device, M, S):
    """ra_wgrad in slab mode with uneven token ranges: slab s is the reference over tokens
    [64 floor(s nks / S), 64 floor((s + 1) nks / S)), and the slabs sum to the whole."""
    N, K = 520, 264
    dy, x, ref_w, _ = _operands(M, N, K, cuda_device)
    ws = torch.full((S, N, K), 7.0, device=cuda_device)
    rc = _lib.lib().ra_wgrad(ptr(dy), N, ptr(x), K, M, N, K, S, ptr(ws), None, 0, stream_ptr())
    assert rc == 0
    nks = M // 64
    for s in range(S):
        a, b = 64 * (s * nks // S), 64 * ((s + 1) * nks // S)
        want = (dy[a:b].double().t() @ x[a:b].double()).float()
        assert torch.equal(ws[s], want), f"slab {s}: tokens [{a}, {b})"
    assert torch.equal(ws.double().sum(0), ref_w)


def test_strided_rows_lm_head_stride(cuda_device):
    """Column slices of wider rows (ld > cols); dY with the LM head's row stride of 50304,
    the largest per-lane staging offsets the workload reaches."""
    wide_y = _ints((128, 50304), 31, cuda_device)
    wide_x = _ints((128, 1024), 32, cuda_device)
    dy, x = wide_y[:, -264:], wide_x[:, 512:648]
    assert dy.stride(0) == 50304 and x.stride(0) == 1024
    ref_w = dy.double().t() @ x.double()
    _check_accumulate(dy, x, ref_w, None, torch.float32, True, False)
    _check_accumulate(dy, x, ref_w, None, torch.bfloat16, False, False)


@pytest.mark.parametrize("M", [64, 192])  # one K-step: sink read-modify-write; three: slabs
@pytest.mark.parametrize("sdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("accumulate", [True, False])
def test_bias_gradient(cuda_device, M, sdtype, accumulate):
    """K = 520 is three k-tiles, so tiles with and without the fused bias sum exist."""
    dy, x, ref_w, ref_b = _operands(M, 264, 520, cuda_device)
    _check_accumulate(dy, x, ref_w, ref_b, sdtype, accumulate, True)


def test_token_tail(cuda_device):
    """M = 1000: the kernel takes 960 rows, the torch tail the other 40."""
    dy, x, ref_w, ref_b = _operands(1000, 264, 136, cuda_device)
    _check_accumulate(dy, x, ref_w, ref_b, torch.float32, True, True)


class _Strided:
    """The tensor attributes _wgrad_hip_ok reads, with a row stride no real buffer has."""

    def __init__(self, t, ld):
        self._t, self._ld = t, ld
        self.shape, self.dtype, self.is_cuda = t.shape, t.dtype, t.is_cuda

    def stride(self, i):
        return self._ld if i == 0 else 1

    def data_ptr(self):
        return self._t.data_ptr()


def test_offset_guard(cuda_device):
    """A row stride whose staging offsets do not fit 32 bits is refused on the host, before
    any launch (nothing is dereferenced), and _wgrad_hip_ok mirrors the condition."""
    dy, x, _, _ = _operands(64, 8, 8, cuda_device)
    out = torch.full((8, 8), 7.0, device=cuda_device)
    L = _lib.lib()
    big = 1 << 31
    assert L.ra_wgrad(ptr(dy), big, ptr(x), 8, 64, 8, 8, 1, ptr(out), None, 0, stream_ptr()) != 0
    assert L.ra_wgrad(ptr(dy), 8, ptr(x), big, 64, 8, 8, 1, ptr(out), None, 0, stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert rf._wgrad_hip_ok(dy, x, out)
    assert not rf._wgrad_hip_ok(_Strided(dy, big), x, out)
    assert not rf._wgrad_hip_ok(dy, _Strided(x, big), out)
    # the bound itself: (64 ld + cols) * 2 <= 2^32
    assert rf._wgrad_offsets_fit(50304, 50304)
    assert rf._wgrad_offsets_fit(((1 << 31) - 264) // 64, 264)
    assert not rf._wgrad_offsets_fit(((1 << 31) - 264) // 64 + 1, 264)
