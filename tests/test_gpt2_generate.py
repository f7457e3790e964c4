"""GPT-2 generation with a KV cache on the CPU (fp32): greedy ``generate`` against the
recompute loop through ``forward``, ragged and single prompts, EOS fill, argument errors,
sampling, and the plain-torch decode-attention reference against a direct softmax."""

import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

PROMPT_LENS = (1, 5, 17, 40)
NEW = 24


def scaled_tiny(seed=0):
    """tiny() with a larger init so that the context matters: at the default init greedy
    decoding emits one constant token."""
    torch.manual_seed(seed)
    model = GPT2(dataclasses.replace(GPT2Config.tiny(), init_std=0.2))
    with torch.no_grad():
        for blk in model.h:
            blk.c_proj_w.mul_(2)
            blk.mlp_proj_w.mul_(2)
    return model.eval()


@pytest.fixture(scope="module")
def model():
    return scaled_tiny()


@pytest.fixture(scope="module")
def prompts(model):
    g = torch.Generator().manual_seed(1)
    T = max(PROMPT_LENS)
    idx = torch.randint(0, model.cfg.vocab_size, (len(PROMPT_LENS), T), generator=g)
    for b, n in enumerate(PROMPT_LENS):
        idx[b, n:] = 0  # right padding
    return idx


def _recompute(model, prompt, n_new):
    seq = prompt.clone().view(1, -1)
    with torch.no_grad():
        for _ in range(n_new):
            nxt = model(seq)[:, -1].argmax(-1)
            seq = torch.cat([seq, nxt[:, None]], 1)
    return seq[0, prompt.numel():]


@pytest.fixture(scope="module")
def recomputed(model, prompts):
    return torch.stack([_recompute(model, prompts[b, :n], NEW)
                        for b, n in enumerate(PROMPT_LENS)])


def test_greedy_equals_recompute_ragged_batch(model, prompts, recomputed):
    out = model.generate(prompts, NEW, lens=list(PROMPT_LENS))
    assert out.dtype == torch.int64 and out.shape == (len(PROMPT_LENS), NEW)
    print("distinct tokens per row:", [len(set(r.tolist())) for r in recomputed])
    assert max(len(set(r.tolist())) for r in recomputed) > 4  # the context matters
    assert torch.equal(out, recomputed)


@pytest.mark.parametrize("b", range(len(PROMPT_LENS)))
def test_greedy_equals_recompute_single(model, prompts, recomputed, b):
    n = PROMPT_LENS[b]
    out = model.generate(prompts[b:b + 1, :n], NEW)
    assert torch.equal(out[0], recomputed[b])


def test_lens_as_tensor_and_extra_padding(model, prompts, recomputed):
    wide = torch.nn.functional.pad(prompts, (0, 9), value=3)
    out = model.generate(wide, NEW, lens=torch.tensor(PROMPT_LENS))
    assert torch.equal(out, recomputed)


def test_eos_fill(model, prompts, recomputed):
    row = max(range(len(PROMPT_LENS)), key=lambda b: len(set(recomputed[b].tolist())))
    eos = int(recomputed[row, 3])
    out = model.generate(prompts, NEW, lens=list(PROMPT_LENS), eos_token_id=eos)
    for b in range(len(PROMPT_LENS)):
        want = recomputed[b].clone()
        hit = (want == eos).nonzero()
        if hit.numel():
            want[int(hit[0]):] = eos
        assert torch.equal(out[b], want), b
    assert (out[row, 3:] == eos).all()


def test_value_errors(model, prompts):
    cfg = model.cfg
    with pytest.raises(ValueError):
        model.generate(prompts, cfg.n_positions - max(PROMPT_LENS) + 1, lens=list(PROMPT_LENS))
    model.generate(prompts[:1, :5], cfg.n_positions - 5)  # exactly fits
    with pytest.raises(ValueError):
        model.generate(prompts[:, :0], 4)
    with pytest.raises(ValueError):
        model.generate(prompts, 4, lens=[1, 0, 3, 4])
    with pytest.raises(ValueError):
        model.generate(prompts, 4, lens=[1, 2, 3, max(PROMPT_LENS) + 1])
    with pytest.raises(ValueError):
        model.generate(prompts, 4, graph=True)  # CPU tensors


def test_sampling(model, prompts, recomputed):
    lens = list(PROMPT_LENS)
    k1 = model.generate(prompts, NEW, lens=lens, temperature=0.8, top_k=1,
                        generator=torch.Generator().manual_seed(3))
    assert torch.equal(k1, recomputed)  # top-1 sampling is greedy
    a = model.generate(prompts, NEW, lens=lens, temperature=1.5, top_k=20,
                       generator=torch.Generator().manual_seed(4))
    b = model.generate(prompts, NEW, lens=lens, temperature=1.5, top_k=20,
                       generator=torch.Generator().manual_seed(4))
    c = model.generate(prompts, NEW, lens=lens, temperature=1.5,
                       generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b)
    assert not torch.equal(a, recomputed) and not torch.equal(a, c)
    for t in (a, c):
        assert t.min() >= 0 and t.max() < model.cfg.vocab_size


def test_padded_vocab_is_never_produced():
    torch.manual_seed(2)
    cfg = dataclasses.replace(GPT2Config.tiny(), vocab_size=500, init_std=0.2)
    m = GPT2(cfg).eval()
    with torch.no_grad():
        m.wte[cfg.vocab_size:] = m.wte[: cfg.vocab_size].abs().max() * 4  # tempting columns
    idx = torch.randint(0, cfg.vocab_size, (3, 6))
    for kw in ({}, {"temperature": 2.0, "generator": torch.Generator().manual_seed(0)}):
        out = m.generate(idx, 16, **kw)
        assert out.max() < cfg.vocab_size


def test_prefill_and_decode_step_logits(model, prompts):
    """Teacher-forced: prefill + decode_step logits against the full forward's."""
    g = torch.Generator().manual_seed(7)
    B, steps = len(PROMPT_LENS), 6
    cont = torch.randint(0, model.cfg.vocab_size, (B, steps), generator=g)
    cache = KVCache(model.cfg, B, max(PROMPT_LENS) + steps, "cpu", torch.float32)
    lens = torch.tensor(PROMPT_LENS, dtype=torch.int32)
    logits = model.prefill(prompts, lens, cache)
    assert logits.shape == (B, model.cfg.vocab_size)
    for t in range(steps + 1):
        for b, n in enumerate(PROMPT_LENS):
            seq = torch.cat([prompts[b, :n], cont[b, :t]]).view(1, -1)
            with torch.no_grad():
                want = model(seq)[0, -1]
            torch.testing.assert_close(logits[b], want, atol=2e-5, rtol=1e-5)
        if t < steps:
            logits = model.decode_step(cont[:, t], cache)
    assert torch.equal(cache.lens, lens + steps)


def _direct(qkv, kc, vc, lens, scale):
    """Row by row: softmax over the first lens[b] cached rows plus the new one."""
    B, _, H, D = qkv.shape
    out = torch.zeros(B, H, D, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        if n < 0 or n >= kc.shape[2]:
            continue
        for h in range(H):
            k = torch.cat([kc[b, h, :n], qkv[b, 1, h][None]]).double()
            v = torch.cat([vc[b, h, :n], qkv[b, 2, h][None]]).double()
            p = torch.softmax((k @ qkv[b, 0, h].double()) * scale, 0)
            out[b, h] = p @ v
    return out


@pytest.mark.parametrize("D", [16, 64])
def test_reference_attn_decode(D):
    g = torch.Generator().manual_seed(D)
    H, Tmax = 3, 12
    lens = torch.tensor([0, 1, 5, Tmax - 1, -1, Tmax, Tmax + 7], dtype=torch.int32)
    B = lens.numel()
    qkv = torch.randn(B, 3, H, D, generator=g)
    kc, vc = torch.randn(B, H, Tmax, D, generator=g), torch.randn(B, H, Tmax, D, generator=g)
    for b in range(B):  # whatever lies past lens[b] must not matter
        n = max(int(lens[b]), 0)
        kc[b, :, n:] = float("nan")
        vc[b, :, n:] = float("nan")
    k0, v0 = kc.clone(), vc.clone()
    want = _direct(qkv, k0, v0, lens, D ** -0.5)
    out = rf.attn_decode(qkv, kc, vc, lens)  # CPU tensors: the reference
    assert out.shape == (B, H, D) and out.dtype == qkv.dtype
    torch.testing.assert_close(out.double(), want, atol=1e-5, rtol=1e-5)
    assert (out[4:] == 0).all()
    assert torch.equal(out[0], qkv[0, 2])  # one key: the new v itself
    for b in range(B):
        n = int(lens[b])
        ke, ve = k0[b].clone(), v0[b].clone()
        if 0 <= n < Tmax:
            ke[:, n], ve[:, n] = qkv[b, 1], qkv[b, 2]
        assert torch.equal(kc[b].view(torch.int32), ke.view(torch.int32)), b
        assert torch.equal(vc[b].view(torch.int32), ve.view(torch.int32)), b
    same = ref.attn_decode(qkv, k0, v0, lens, D ** -0.5)
    assert torch.equal(same, out)


def test_attn_decode_rejects_grad():
    qkv = torch.randn(1, 3, 2, 16, requires_grad=True)
    kc, vc = torch.zeros(1, 2, 4, 16), torch.zeros(1, 2, 4, 16)
    with pytest.raises(RuntimeError):
        rf.attn_decode(qkv, kc, vc, torch.zeros(1, dtype=torch.int32))
