"""The int8 K/V cache kernels (ops/csrc/attn_decode_q8.hip) on the GPU: the quantising
``kv_insert`` and the append of ``attn_decode`` bit for bit against the plain-torch reference
run on CPU copies (IEEE division, round half to even), the attention output against fp64
attention over the dequantised cache, and ``generate(kv_cache="int8")`` eager against graph.

Output bound as tests/test_attn_decode_gpu.py, |a - b| / |b| < 1e-2 per row: the reference
here is fp64 over the SAME dequantised cache, so what is left is the kernel's fp32 sums and
the bf16 rounding of the output (2^-9 per element), as there."""

import dataclasses
import functools

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

D, H = 64, 2
REL = 1e-2


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _same(a, b):  # bit for bit, NaN scales included
    return a.dtype == b.dtype and torch.equal(a.view(torch.int8), b.view(torch.int8))


# ------------------------------------------------------------------------------ kv_insert
S, TMAX_I = 4, 129


@pytest.mark.parametrize("Tp", [1, 7, 130])
@pytest.mark.parametrize("Bn", [1, 3])
def test_kv_insert_q8_bitwise(cuda_device, Bn, Tp):
    g = torch.Generator().manual_seed(100 * Bn + Tp)
    qkv = (torch.randn(Bn, Tp, 3, H, D, generator=g) * 3).bfloat16()
    qkv[0, 0, 1, 0] = 0  # an all-zero vector
    qkv[0, 0, 2, 1] = 0
    qkv[0, 0, 2, 1, 37] = -3.0  # a single -max element
    lens_vals = [0, 1, Tp, Tp + 5, TMAX_I + 1, 70]
    slot_vals = [2, -1, 0, S, 3, 1]
    for shift in range(6):
        lens = torch.tensor([lens_vals[(shift + i) % 6] for i in range(Bn)], dtype=torch.int32)
        slots = torch.tensor([slot_vals[(2 * shift + i) % 6] for i in range(Bn)],
                             dtype=torch.int32)
        cpu = [torch.full((S, H, TMAX_I, D), 0x5A, dtype=torch.int8) for _ in range(2)] + \
              [torch.full((S, H, TMAX_I), float("nan")) for _ in range(2)]
        gpu = [t.to(cuda_device) for t in cpu]
        ref.kv_insert(qkv, cpu[0], cpu[1], slots, lens, cpu[2], cpu[3])
        rf.kv_insert(qkv.to(cuda_device), gpu[0], gpu[1], slots.to(cuda_device),
                     lens.to(cuda_device), k_scale=gpu[2], v_scale=gpu[3])
        for name, a, b in zip(("k", "v", "k_scale", "v_scale"), gpu, cpu):
            assert _same(a.cpu(), b), (name, lens.tolist(), slots.tolist())


# ---------------------------------------------------------------------------- attn_decode
# the kernel's granularities: 16 rows per wave load, 64 per load index of a workgroup, 256
# per workgroup step
TMAX = 300
LENS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, TMAX - 1, -1, TMAX, rf.SLOT_INACTIVE)


@functools.lru_cache(maxsize=None)
def _decode_case():
    """CPU inputs (garbage bytes and NaN / Inf scales past lens[b]), the reference's caches
    after the call and the fp64 attention over them. Computed once, never modified."""
    g = torch.Generator().manual_seed(7)
    B = len(LENS)
    qkv = torch.randn(B, 3, H, D, generator=g).bfloat16()
    k, ks = ref.quantize_kv(torch.randn(B, H, TMAX, D, generator=g) * 2)
    v, vs = ref.quantize_kv(torch.randn(B, H, TMAX, D, generator=g) * 2)
    for b, n in enumerate(LENS):
        n = min(max(n, 0), TMAX)
        for q, s, bad in ((k, ks, float("nan")), (v, vs, float("inf"))):
            q[b, :, n:] = torch.randint(-128, 128, q[b, :, n:].shape, generator=g).to(torch.int8)
            s[b, :, n:] = bad
    lens = torch.tensor(LENS, dtype=torch.int32)
    after = [t.clone() for t in (k, v, ks, vs)]
    ref.attn_decode(qkv, after[0], after[1], lens, None, after[2], after[3])
    want = torch.zeros(B, H, D, dtype=torch.float64)
    for b, n in enumerate(LENS):
        if 0 <= n < TMAX:
            kd = after[0][b, :, : n + 1].double() * after[2][b, :, : n + 1, None].double()
            vd = after[1][b, :, : n + 1].double() * after[3][b, :, : n + 1, None].double()
            p = torch.softmax((qkv[b, 0].double().unsqueeze(1) @ kd.transpose(-1, -2)) * D ** -0.5,
                              -1)
            want[b] = (p @ vd).squeeze(1)
    return qkv, (k, v, ks, vs), lens, after, want


def _decode(dev, rows, splits):
    qkv, before, lens, _, _ = _decode_case()
    caches = [t[rows].to(dev) for t in before]
    out = rf.attn_decode(qkv[rows].to(dev), caches[0], caches[1], lens[rows].to(dev),
                         splits=splits, k_scale=caches[2], v_scale=caches[3])
    return out.cpu(), [t.cpu() for t in caches]


@pytest.mark.parametrize("splits", [1, 2, 3, None])
def test_attn_decode_q8(cuda_device, splits):
    qkv, _, lens, after, want = _decode_case()
    out, caches = _decode(cuda_device, slice(None), splits)
    assert out.dtype == torch.bfloat16 and not out.isnan().any()
    # the append bit for bit, every other byte and scale unchanged
    for name, a, b in zip(("k", "v", "k_scale", "v_scale"), caches, after):
        assert _same(a, b), name
    for b, n in enumerate(LENS):
        if not 0 <= n < TMAX:
            assert (out[b] == 0).all(), n
            continue
        err = ((out[b].double() - want[b]).norm() / want[b].norm()).item()
        print(f"splits={splits} len={n}: rel err {err:.2e}")
        assert err < REL, (n, err)
        if splits is not None:  # alone: the same bits as inside the batch
            alone, _ = _decode(cuda_device, slice(b, b + 1), splits)
            assert _same(alone[0], out[b]), n


# ---------------------------------------------------------------------------------- model
def test_generate_int8_cache_graph_equals_eager(cuda_device):
    cfg = dataclasses.replace(GPT2Config.tiny(), init_std=0.2, n_embd=128, n_head=2)
    torch.manual_seed(0)
    model = GPT2(cfg).eval().to(cuda_device, torch.bfloat16)
    prompts = torch.randint(0, cfg.vocab_size, (3, 20), generator=torch.Generator().manual_seed(1))
    kw = dict(lens=[3, 20, 11], temperature=[0.0, 0.9, 0.7], top_k=[0, 40, 0], seeds=[1, 2, 3],
              kv_cache="int8")
    eager = model.generate(prompts.to(cuda_device), 24, **kw)
    graph = model.generate(prompts.to(cuda_device), 24, graph=True, **kw)
    assert eager.shape == (3, 24) and torch.equal(eager, graph)
