"""The int8 K/V cache (``kv_cache="int8"``) on the CPU reference path: the quantiser's error
bound, ``generate`` against a hand-rolled ``prefill`` / ``decode_step`` loop, the engine
against ``generate``, every rejection, and both servers."""

import asyncio
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.serve.llm import build_gpt2_app

SEED = 11
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
PROMPTS = torch.tensor([[5, 17, 300, 42, 8, 99, 123], [7, 3, 1, 4, 1, 5, 9]])


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(SEED)
    return GPT2(CFG).eval()


def test_quantize_kv_bound_and_zero_vector():
    torch.manual_seed(0)
    x = torch.randn(5, 3, 9, 64) * torch.logspace(-3, 2, 9)[:, None]
    x[2, 1, 4] = 0
    q, s = ref.quantize_kv(x)
    assert q.dtype == torch.int8 and q.shape == x.shape and s.shape == x.shape[:-1]
    err = (x.double() - q.double() * s.double()[..., None]).abs()
    assert (err <= s.double()[..., None] * (0.5 + 2.0 ** -10)).all()
    assert s[2, 1, 4] == 0 and (q[2, 1, 4] == 0).all()
    assert (q.abs().amax(-1) == 127).sum() == s.numel() - 1


def test_generate_equals_prefill_decode_loop(model):
    lens = [7, 4]
    got = model.generate(PROMPTS, 10, lens=lens, kv_cache="int8")
    cache = KVCache(CFG, 2, 7 + 10, quant="int8")
    assert cache.k.dtype == torch.int8 and cache.k_scale.shape == cache.k.shape[:-1]
    logits = model.prefill(PROMPTS, lens, cache)
    want = []
    for _ in range(10):
        want.append(logits.argmax(-1))
        logits = model.decode_step(want[-1], cache)
    assert torch.equal(got, torch.stack(want, 1))
    hd = CFG.n_embd // CFG.n_head  # hd + 4 bytes per vector where bf16 takes 2 hd
    assert cache.nbytes() * 2 * hd == KVCache(CFG, 2, 17, dtype=torch.bfloat16).nbytes() * (hd + 4)


def test_engine_returns_generates_tokens(model):
    reqs = [([5, 17, 300, 42], 10, 0.0, 0), ([9, 8, 7], 6, 0.9, 5)]
    want = [model.generate(torch.tensor([t]), n, temperature=temp, seeds=[seed],
                           kv_cache="int8")[0].tolist() for t, n, temp, seed in reqs]
    eng = GPT2Engine(model, slots=2, graph=False, poll_every=1, kv_cache="int8")
    got = {}
    rid0 = eng.submit(reqs[0][0], reqs[0][1], temperature=reqs[0][2], seed=reqs[0][3])
    for _ in range(3):  # the second request arrives while the first decodes
        for ev in eng.step():
            got.setdefault(ev[0], []).extend(ev[1])
    rid1 = eng.submit(reqs[1][0], reqs[1][1], temperature=reqs[1][2], seed=reqs[1][3])
    for rid, toks in eng.run().items():
        got.setdefault(rid, []).extend(toks)
    assert [got[rid0], got[rid1]] == want


def _q8(*shape):
    return torch.zeros(*shape, 16, dtype=torch.int8), torch.zeros(*shape)


I32 = torch.zeros(2, dtype=torch.int32)
QKV1, QKVT = torch.zeros(2, 3, 2, 16), torch.zeros(2, 1, 3, 2, 16)
REJECTED = {
    "quant": lambda m: KVCache(CFG, 1, 8, quant="fp8"),
    "decode_no_scales": lambda m: rf.attn_decode(QKV1, _q8(2, 2, 8)[0], _q8(2, 2, 8)[0], I32),
    "decode_float_scales": lambda m: rf.attn_decode(
        QKV1, torch.zeros(2, 2, 8, 16), torch.zeros(2, 2, 8, 16), I32,
        k_scale=torch.zeros(2, 2, 8), v_scale=torch.zeros(2, 2, 8)),
    "decode_scale_shape": lambda m: rf.attn_decode(
        QKV1, _q8(2, 2, 8)[0], _q8(2, 2, 8)[0], I32, k_scale=torch.zeros(2, 2, 7),
        v_scale=torch.zeros(2, 2, 8)),
    "insert_no_scales": lambda m: rf.kv_insert(QKVT, _q8(2, 2, 8)[0], _q8(2, 2, 8)[0], I32, I32),
    "insert_float_scales": lambda m: rf.kv_insert(
        QKVT, torch.zeros(2, 2, 8, 16), torch.zeros(2, 2, 8, 16), I32, I32,
        k_scale=torch.zeros(2, 2, 8), v_scale=torch.zeros(2, 2, 8)),
    "attn_extend": lambda m: rf.attn_extend(QKVT, _q8(2, 2, 8)[0], _q8(2, 2, 8)[0], I32, I32,
                                            I32 + 1),
    "kv_copy": lambda m: rf.kv_copy(*[_q8(1, 2, 2, 8)[0] for _ in range(4)], I32, I32, I32),
    "beam_kv_fork": lambda m: rf.beam_kv_fork(_q8(1, 2, 2, 8)[0], _q8(1, 2, 2, 8)[0], I32, I32),
    "extend_into": lambda m: m.extend_into(PROMPTS[:, :2], [2, 2], KVCache(CFG, 2, 8, quant="int8"),
                                           I32, I32),
    "verify_step": lambda m: m.verify_step(PROMPTS[:, :2], I32 + 1,
                                           KVCache(CFG, 2, 8, quant="int8")),
    "generate_value": lambda m: m.generate(PROMPTS, 2, kv_cache="fp8"),
    "generate_beams": lambda m: m.generate(PROMPTS, 2, num_beams=2, eos_token_id=0,
                                           kv_cache="int8"),
    "engine_value": lambda m: GPT2Engine(m, slots=1, graph=False, kv_cache="fp8"),
    "engine_prefix": lambda m: GPT2Engine(m, slots=1, graph=False, kv_cache="int8",
                                          prefix_slots=1),
    "engine_chunk": lambda m: GPT2Engine(m, slots=1, graph=False, kv_cache="int8",
                                         prefill_chunk=4),
    "engine_speculate": lambda m: GPT2Engine(m, slots=1, graph=False, kv_cache="int8",
                                             speculate=2),
    "app_value": lambda m: build_gpt2_app(config="tiny", kv_cache="fp8", device="cpu"),
}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_rejected(model, name):
    with pytest.raises(ValueError):
        REJECTED[name](model)


@pytest.mark.parametrize("continuous", [False, True])
def test_serve_int8_cache(continuous):
    app = build_gpt2_app(config=CFG, seed=SEED, kv_cache="int8", weights="int8", device="cpu",
                         continuous=continuous)
    srv = app.deployment.func_or_class(*app.args, **app.kwargs)
    try:
        torch.manual_seed(SEED)
        mine = GPT2(CFG).eval().quantize_weights()
        want = mine.generate(PROMPTS[:1], 8, seeds=[SEED], kv_cache="int8")[0].tolist()
        req = {"tokens": PROMPTS[0].tolist(), "max_new_tokens": 8}
        if continuous:
            assert srv.engine.cache.quant == "int8"
            assert asyncio.run(srv(req)) == {"tokens": want}
        else:
            assert srv._run([req]) == [want]
    finally:
        if continuous:
            srv.close()
