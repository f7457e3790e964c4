"""The HIP decode-attention kernel (ops/csrc/attn_decode.hip) against the plain-torch
reference on fp32 CPU copies: ragged lengths, the in-place append, split-KV and its
run-to-run bit identity, inactive rows; then prefill / decode_step / generate of the
model on the GPU, teacher-forced against the fp32 CPU forward, and graph against eager.

Inputs are randn rounded to bf16; the caches past lens[b] are filled with NaN, so masking
by multiplying with zero fails. Error measure and bound as test_flash_attention_fwd_bwd:
|a - b| / |b| < 1e-2."""

import dataclasses
import functools

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

D = 64
REL = 1e-2


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(lens, H, Tmax, seed=0):
    """(qkv, k_cache, v_cache) bf16 on the CPU with NaN past lens[b], the fp32 reference
    output and the expected caches after the call. Computed once, never modified."""
    g = torch.Generator().manual_seed(seed + 1000 * H + Tmax)
    B = len(lens)
    qkv = torch.randn(B, 3, H, D, generator=g).bfloat16()
    kc = torch.randn(B, H, Tmax, D, generator=g).bfloat16()
    vc = torch.randn(B, H, Tmax, D, generator=g).bfloat16()
    for b, n in enumerate(lens):
        n = min(max(n, 0), Tmax)
        kc[b, :, n:] = float("nan")
        vc[b, :, n:] = float("nan")
    lens_t = torch.tensor(lens, dtype=torch.int32)
    want = ref.attn_decode(qkv.float(), kc.float(), vc.float(), lens_t)
    # the caches after the call: built from the bf16 originals (a round trip through fp32
    # may change a NaN's bit pattern)
    k_after, v_after = kc.clone(), vc.clone()
    for b, n in enumerate(lens):
        if 0 <= n < Tmax:
            k_after[b, :, n] = qkv[b, 1]
            v_after[b, :, n] = qkv[b, 2]
    return qkv, kc, vc, lens_t, want, k_after, v_after


def _run(case, dev, splits=None):
    qkv, kc, vc, lens, want, k_after, v_after = case
    kd, vd = kc.to(dev), vc.to(dev)
    out = rf.attn_decode(qkv.to(dev), kd, vd, lens.to(dev), splits=splits)
    assert out.shape == want.shape and out.dtype == torch.bfloat16
    return out.cpu(), kd.cpu(), vd.cpu()


def _check(case, got, tag=""):
    qkv, kc, vc, lens, want, k_after, v_after = case
    out, kd, vd = got
    Tmax = kc.shape[2]
    assert torch.isfinite(out.float()).all(), tag
    err = _rel(out, want)
    print(f"{tag} rel err {err:.2e}")
    assert err < REL, tag
    for b, n in enumerate(lens.tolist()):
        if 0 <= n < Tmax:
            assert _rel(out[b], want[b]) < REL, (tag, b, n)
            # the append: the new k, v bitwise at position lens[b]
            assert torch.equal(_bits(kd[b, :, n]), _bits(qkv[b, 1])), (tag, b)
            assert torch.equal(_bits(vd[b, :, n]), _bits(qkv[b, 2])), (tag, b)
            if n == 0:  # one key: the output is the new v itself
                assert torch.equal(_bits(out[b]), _bits(qkv[b, 2])), (tag, b)
        else:
            assert (out[b] == 0).all(), (tag, b)
    # every other cache element unchanged, the NaNs included
    assert torch.equal(_bits(kd), _bits(k_after)), tag
    assert torch.equal(_bits(vd), _bits(v_after)), tag


TMAX = 160
RAGGED = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, TMAX - 1)


@pytest.mark.parametrize("H", [1, 3])
def test_ragged_batch_and_append(cuda_device, H):
    case = _case(RAGGED, H, TMAX)
    _check(case, _run(case, cuda_device), f"ragged H={H}")
    _check(case, _run(case, cuda_device, splits=3), f"ragged H={H} splits=3")


@pytest.mark.parametrize("H", [1, 3])
def test_single_rows(cuda_device, H):
    for n in RAGGED:
        case = _case((n,), H, TMAX)
        _check(case, _run(case, cuda_device), f"single len={n} H={H}")


@pytest.mark.parametrize("n", [5, 200, 2047])
def test_splits(cuda_device, n):
    case = _case((n,), 2, 2048)
    for s in (1, 2, 7, 0):
        a = _run(case, cuda_device, splits=s)
        b = _run(case, cuda_device, splits=s)
        _check(case, a, f"len={n} splits={s}")
        for x, y in zip(a, b):  # two runs: the same bits
            assert torch.equal(_bits(x), _bits(y)), (n, s)
    auto = _lib.lib().ra_attn_decode_splits(1, 2, 2048)
    assert 1 <= auto <= 64
    print(f"len={n}: automatic splits = {auto}")


def test_splits_argument_is_checked(cuda_device):
    qkv, kc, vc, lens = (t.to(cuda_device) for t in _case((5,), 2, 2048)[:4])
    with pytest.raises(_lib.HipKernelError):
        rf.attn_decode(qkv, kc.clone(), vc.clone(), lens, splits=100000)
    with pytest.raises(ValueError):
        rf.attn_decode(qkv, kc.clone(), vc.clone(), lens.long())
    with pytest.raises(RuntimeError):
        rf.attn_decode(qkv.clone().requires_grad_(), kc.clone(), vc.clone(), lens)


@pytest.mark.parametrize("splits", [None, 1, 3])
def test_inactive_rows(cuda_device, splits):
    """lens[b] in {-1, Tmax} (and one active row between them). The caches are views into
    a larger allocation with canary rows on both sides: a broken guard shows as a changed
    canary or neighbour, not as a fault."""
    H, Tmax = 2, 96
    lens = (-1, 17, Tmax)
    case = _case(lens, H, Tmax, seed=3)
    qkv, kc, vc, lens_t, want, k_after, v_after = case
    B = len(lens)
    bigs = []
    for c in (kc, vc):
        big = torch.full((B + 2, H, Tmax, D), 1.5, dtype=torch.bfloat16)
        big[1:-1] = c
        bigs.append(big.to(cuda_device))
    kd, vd = bigs[0][1:-1], bigs[1][1:-1]
    out = rf.attn_decode(qkv.to(cuda_device), kd, vd, lens_t.to(cuda_device), splits=splits)
    _check(case, (out.cpu(), kd.cpu(), vd.cpu()), f"inactive splits={splits}")
    assert (out[0] == 0).all() and (out[2] == 0).all()
    for big in bigs:
        assert (big[0] == 1.5).all() and (big[-1] == 1.5).all()


# ----------------------------------------------------------------------------- model
PROMPT_LENS = (1, 5, 17, 40)
NEW = 24


def _configs():
    tiny = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
    # the same size of model with head_dim 64, the HIP kernel's (tiny() has head_dim 16,
    # which the reference serves)
    hd64 = dataclasses.replace(tiny, n_embd=128, n_head=2)
    return {"tiny": tiny, "hd64": hd64}


@functools.lru_cache(maxsize=None)
def _model(name):
    """The scaled-init fp32 CPU model (at the default init greedy decoding emits one
    constant token), its token sequence and its fp32 logits at every position."""
    torch.manual_seed(0)
    m = GPT2(_configs()[name]).eval()
    with torch.no_grad():
        for blk in m.h:
            blk.c_proj_w.mul_(2)
            blk.mlp_proj_w.mul_(2)
        g = torch.Generator().manual_seed(1)
        seq = torch.randint(0, m.cfg.vocab_size, (len(PROMPT_LENS), max(PROMPT_LENS) + NEW),
                            generator=g)
        logits = m(seq)
    return m, seq, logits


def _gpu_model(name, dev):
    m, seq, logits = _model(name)
    g = GPT2(m.cfg).eval()
    g.load_state_dict(m.state_dict())
    return g.to(dev, torch.bfloat16), seq, logits


@pytest.mark.parametrize("name", ["tiny", "hd64"])
def test_model_teacher_forced(cuda_device, name):
    """prefill (ragged) + 24 decode_steps fed a fixed token sequence: at every step the
    logits against the fp32 CPU full forward of the same weights at that position.

    Bound: both the bf16 GPU full ``forward`` and the cached path are bf16 pipelines with
    the same rounding points, only the accumulation order differs, so every step's error
    must be within 2x the error of that full forward against the same fp32 reference. The
    forward's error is the largest per-position |a - b| / |b| over the compared (row,
    position) pairs, measured here; both are printed."""
    model, seq, want = _gpu_model(name, cuda_device)
    B, T = len(PROMPT_LENS), max(PROMPT_LENS)
    rows = torch.arange(B)
    lens = torch.tensor(PROMPT_LENS)
    with torch.no_grad():
        full = model(seq.to(cuda_device)).float().cpu()
    fwd_errs = [_rel(full[b, n - 1 + t], want[b, n - 1 + t])
                for b, n in enumerate(PROMPT_LENS) for t in range(NEW + 1)]
    fwd_err = max(fwd_errs)
    prompts = seq[:, :T].clone()
    for b, n in enumerate(PROMPT_LENS):
        prompts[b, n:] = 0
    cache = KVCache(model.cfg, B, T + NEW, cuda_device, torch.bfloat16)
    cache.k.fill_(float("nan"))  # nothing past lens[b] may be read
    cache.v.fill_(float("nan"))
    logits = model.prefill(prompts.to(cuda_device), lens.to(cuda_device), cache)
    worst = 0.0
    for t in range(NEW + 1):
        got = logits.float().cpu()
        assert got.shape == (B, model.cfg.vocab_size)
        errs = [_rel(got[b], want[b, n - 1 + t]) for b, n in enumerate(PROMPT_LENS)]
        worst = max(worst, max(errs))
        assert max(errs) <= 2 * fwd_err, (t, errs, fwd_err)
        if t < NEW:
            logits = model.decode_step(seq[rows, lens + t].to(cuda_device), cache)
    print(f"{name}: full bf16 forward err {fwd_err:.3e} (mean {sum(fwd_errs) / len(fwd_errs):.3e}),"
          f" prefill + decode_step worst err {worst:.3e}")
    assert torch.equal(cache.lens.cpu(), (lens + NEW).int())


@pytest.mark.parametrize("name", ["tiny", "hd64"])
def test_generate_graph_equals_eager(cuda_device, name):
    model, seq, _ = _gpu_model(name, cuda_device)
    T = max(PROMPT_LENS)
    prompts = seq[:, :T].to(cuda_device)
    lens = list(PROMPT_LENS)
    eager = model.generate(prompts, NEW, lens=lens)
    graph = model.generate(prompts, NEW, lens=lens, graph=True)
    print(name, "distinct greedy tokens per row:", [len(set(r.tolist())) for r in eager])
    assert eager.dtype == torch.int64 and eager.shape == (len(lens), NEW)
    assert torch.equal(eager, graph)

    def sample(**kw):
        gen = torch.Generator(device=cuda_device).manual_seed(5)
        return model.generate(prompts, NEW, lens=lens, temperature=0.9, top_k=40,
                              generator=gen, **kw)

    s_eager, s_graph = sample(), sample(graph=True)
    assert torch.equal(s_eager, s_graph)
    assert not torch.equal(s_eager, eager)
    assert int(s_eager.max()) < model.cfg.vocab_size
