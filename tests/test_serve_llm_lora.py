"""serve.llm with low-rank adapters: an app built with ``adapters={"name": ...}`` answers a
``{"adapter": "name", ...}`` request with the tokens of ``generate(adapters=[id])`` on that
request alone, requests of two adapters and of the base model in flight together (CPU)."""

import asyncio
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.lora import LoRAStack, target_dims
from ray_amd.serve.llm import GPT2EngineServer, GPT2Server, build_gpt2_app

SEED = 11
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
SYS = list(range(100, 137))


def _state(r, seed, alpha=None):
    g = torch.Generator().manual_seed(seed)
    state = {} if alpha is None else {"alpha": alpha}
    for layer in range(CFG.n_layer):
        for t, (din, dout) in target_dims(CFG).items():
            state[f"h.{layer}.{t}.lora_A"] = torch.randn(r, din, generator=g) * 0.2
            state[f"h.{layer}.{t}.lora_B"] = torch.randn(dout, r, generator=g) * 0.2
    return state


ADAPTERS = {"fr": _state(8, 1, alpha=16), "de": _state(16, 2)}
IDS = {"fr": 0, "de": 1, None: -1}
REQUESTS = [
    {"adapter": "fr", "tokens": [5, 17, 300, 42, 8], "max_new_tokens": 12},
    {"adapter": "de", "tokens": [7], "max_new_tokens": 9, "temperature": 0.8, "top_k": 20,
     "seed": 5},
    {"tokens": [9, 8, 7], "max_new_tokens": 6},  # the base model, as before
    {"adapter": "de", "tokens": [3, 1, 4, 1, 5], "max_new_tokens": 20, "temperature": 1.2,
     "top_p": 0.9},
    {"adapter": "fr", "prefix": "sys", "tokens": [2, 7], "max_new_tokens": 8},
    {"prefix": "sys", "tokens": [2, 7], "max_new_tokens": 8},  # inherits the prefix's adapter
]


@pytest.fixture(scope="module")
def expected():
    torch.manual_seed(SEED)
    model = GPT2(CFG).eval()
    stack = LoRAStack(CFG, 2, 16)
    for name, state in ADAPTERS.items():
        stack.load(IDS[name], state)
    model.attach_lora(stack)
    out, base = [], []
    for r in REQUESTS:
        toks = (SYS if r.get("prefix") else []) + r["tokens"]
        kw = dict(temperature=r.get("temperature", 0.0), top_k=r.get("top_k"),
                  top_p=r.get("top_p"), seeds=[r.get("seed", SEED)])
        ad = "fr" if r.get("prefix") else r.get("adapter")
        out.append(model.generate(torch.tensor([toks]), r["max_new_tokens"],
                                  adapters=[IDS[ad]], **kw)[0].tolist())
        base.append(model.generate(torch.tensor([toks]), r["max_new_tokens"], **kw)[0].tolist())
    # the adapters are seen to act, so the comparisons below mean something
    assert all((o != b) == (r.get("adapter") is not None or "prefix" in r)
               for o, b, r in zip(out, base, REQUESTS))
    return out


@pytest.fixture
def server():
    made = []

    def make(**kw):
        app = build_gpt2_app(CFG, seed=SEED, continuous=True, slots=3, device="cpu", **kw)
        assert app.deployment.func_or_class is GPT2EngineServer
        made.append(GPT2EngineServer(*app.args, **app.kwargs))
        return made[-1]

    yield make
    for srv in made:
        srv.close()


def test_adapter_requests_answer_as_generate_alone(server, expected, tmp_path):
    path = str(tmp_path / "de.pt")
    torch.save(ADAPTERS["de"], path)  # one adapter from a file, one from a dict
    srv = server(adapters={"fr": ADAPTERS["fr"], "de": path},
                 prefixes={"sys": {"tokens": SYS, "adapter": "fr"}})
    assert srv.engine.lora.n_adapters == 2 and srv.engine.lora.rank == 16

    async def calls():
        return await asyncio.gather(*(srv(r) for r in REQUESTS))

    # six requests over three slots: two adapters and the base model share the steps
    assert asyncio.run(calls()) == [{"tokens": e} for e in expected]
    assert asyncio.run(srv(REQUESTS[0])) == {"tokens": expected[0]}


def test_unknown_adapter_is_a_per_request_error(server, expected):
    srv = server(adapters=ADAPTERS, prefixes={"sys": {"tokens": SYS, "adapter": "fr"}})

    async def calls():
        bad = [srv({"adapter": "nope", "tokens": [1], "max_new_tokens": 3}),
               srv({"adapter": 0, "tokens": [1], "max_new_tokens": 3}),
               srv({"adapter": "de", "prefix": "sys", "tokens": [1], "max_new_tokens": 3})]
        return await asyncio.gather(*bad, srv(REQUESTS[1]))

    *errs, good = asyncio.run(calls())
    for e in errs:
        assert "error" in e and "tokens" not in e
    assert good == {"tokens": expected[1]}
    assert asyncio.run(srv(REQUESTS[2])) == {"tokens": expected[2]}  # and the next is served
    assert not srv.engine.has_work()


def test_adapters_need_the_continuous_app():
    with pytest.raises(ValueError):
        build_gpt2_app(CFG, adapters=ADAPTERS)
    app = build_gpt2_app(CFG, seed=SEED, device="cpu")
    assert app.deployment.func_or_class is GPT2Server
    srv = GPT2Server(*app.args, **app.kwargs)
    got = asyncio.run(srv({"adapter": "fr", "tokens": [1, 2], "max_new_tokens": 3}))
    assert "error" in got and "tokens" not in got
    assert len(asyncio.run(srv({"tokens": [1, 2], "max_new_tokens": 3}))["tokens"]) == 3
    # a continuous app without adapters: every name is unknown, and there is no stack
    eng = GPT2EngineServer(CFG, seed=SEED, slots=1, device="cpu")
    try:
        assert "error" in asyncio.run(eng({"adapter": "fr", "tokens": [1, 2]}))
        assert eng.engine.lora is None and eng.engine.adapter is None
    finally:
        eng.close()
