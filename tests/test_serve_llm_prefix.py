"""serve.llm with shared prompt prefixes: an app built with ``prefixes={"sys": ...}`` answers
a ``{"prefix": "sys", "tokens": continuation}`` request with the tokens of the request that
carries the whole prompt, awaited or streamed, with and without ``prefill_chunk`` (CPU)."""

import asyncio
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.serve.llm import GPT2EngineServer, GPT2Server, build_gpt2_app

SEED = 11
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
SYS = list(range(100, 137))  # 37 tokens
OTHER = [4, 4, 9]
REQUESTS = [
    {"prefix": "sys", "tokens": [5, 17, 300, 42, 8], "max_new_tokens": 12},
    {"prefix": "sys", "tokens": [7], "max_new_tokens": 9, "temperature": 0.8, "top_k": 20,
     "seed": 5},
    {"prefix": "other", "tokens": [3, 1, 4, 1, 5], "max_new_tokens": 20, "temperature": 1.2,
     "top_p": 0.9},
    {"tokens": [9, 8, 7], "max_new_tokens": 6},  # no prefix: as before
]
PREFIXES = {"sys": SYS, "other": OTHER}


def _full(r):
    full = dict(r)
    full["tokens"] = PREFIXES.get(full.pop("prefix", None), []) + r["tokens"]
    return full


@pytest.fixture(scope="module")
def expected():
    """What the app without prefixes answers to the whole-prompt requests = ``generate`` on
    each alone (tests/test_serve_llm_engine.py checks that equality)."""
    torch.manual_seed(SEED)
    model = GPT2(CFG).eval()
    out = []
    for r in map(_full, REQUESTS):
        out.append(model.generate(torch.tensor([r["tokens"]]), r["max_new_tokens"],
                                  temperature=r.get("temperature", 0.0), top_k=r.get("top_k"),
                                  top_p=r.get("top_p"), seeds=[r.get("seed", SEED)])[0].tolist())
    return out


@pytest.fixture
def server():
    made = []

    def make(**kw):
        app = build_gpt2_app(CFG, seed=SEED, continuous=True, slots=2, device="cpu", **kw)
        assert app.deployment.func_or_class is GPT2EngineServer
        made.append(GPT2EngineServer(*app.args, **app.kwargs))
        return made[-1]

    yield make
    for srv in made:
        srv.close()


@pytest.mark.parametrize("chunk", [None, 8])
def test_prefixed_requests_answer_as_the_whole_prompt(server, expected, chunk):
    srv = server(prefixes=PREFIXES, prefill_chunk=chunk)
    assert srv.engine.prefix_slots == 2 and srv.engine.prefill_chunk == chunk

    async def streamed(r):
        chunks = [c async for c in srv.stream(r)]
        assert chunks[-1].get("finished") and not any(c.get("finished") for c in chunks[:-1])
        return [t for c in chunks for t in c["tokens"]]

    async def calls():
        return await asyncio.gather(*(srv(r) for r in REQUESTS), *(streamed(r) for r in REQUESTS),
                                    *(srv(_full(r)) for r in REQUESTS))

    got = asyncio.run(calls())
    n = len(REQUESTS)
    assert got[:n] == [{"tokens": e} for e in expected]
    assert got[n: 2 * n] == expected
    assert got[2 * n:] == got[:n]  # the un-prefixed whole-prompt requests, same app
    assert not srv.engine.has_work()


def test_unknown_prefix_is_a_per_request_error(server, expected):
    srv = server(prefixes={"sys": SYS})

    async def calls():
        bad = [srv({"prefix": "nope", "tokens": [1], "max_new_tokens": 3}),
               srv({"prefix": ["sys"], "tokens": [1], "max_new_tokens": 3}),
               srv({"prefix": "sys", "tokens": [], "max_new_tokens": 3}),
               srv({"prefix": "sys", "tokens": [1] * 80, "max_new_tokens": 12})]  # 129 > 128
        chunks = [c async for c in srv.stream({"prefix": "nope", "tokens": [1]})]
        return await asyncio.gather(srv(REQUESTS[0]), *bad), chunks

    (good, *errs), chunks = asyncio.run(calls())
    assert good == {"tokens": expected[0]}
    for e in errs:
        assert "error" in e and "tokens" not in e
    assert len(chunks) == 1 and "error" in chunks[0] and chunks[0]["finished"]
    assert not srv.engine.has_work()


def test_prefix_needs_the_continuous_app():
    with pytest.raises(ValueError):
        build_gpt2_app(CFG, prefixes={"sys": SYS})
    with pytest.raises(ValueError):
        build_gpt2_app(CFG, prefill_chunk=8)
    app = build_gpt2_app(CFG, seed=SEED, device="cpu")
    assert app.deployment.func_or_class is GPT2Server
    srv = GPT2Server(*app.args, **app.kwargs)
    got = asyncio.run(srv({"prefix": "sys", "tokens": [1, 2], "max_new_tokens": 3}))
    assert "error" in got and "tokens" not in got
    ok = asyncio.run(srv({"tokens": [1, 2], "max_new_tokens": 3}))
    assert len(ok["tokens"]) == 3
    # a continuous app without prefixes: every name is unknown
    eng = GPT2EngineServer(CFG, seed=SEED, slots=1, device="cpu")
    try:
        got = asyncio.run(eng({"prefix": "sys", "tokens": [1, 2], "max_new_tokens": 3}))
        assert "error" in got
        assert eng.engine.prefix_slots == 0 and eng.engine.prefill_chunk is None
    finally:
        eng.close()
