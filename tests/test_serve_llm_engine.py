"""serve.llm with ``continuous=True``: requests enter and leave a ``GPT2Engine``
independently, a short request does not wait for a long one, results can be streamed, and
each request gets what ``generate`` returns for it alone (CPU)."""

import asyncio
import dataclasses

import pytest
import torch

import ray_amd as ray
from ray_amd import serve
from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.serve.llm import GPT2EngineServer, GPT2Server, build_gpt2_app

SEED = 11
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
REQUESTS = [
    {"tokens": [5, 17, 300, 42, 8, 99, 123], "max_new_tokens": 12},
    {"tokens": [7], "max_new_tokens": 5, "temperature": 0.0},
    {"tokens": list(range(20, 49)), "max_new_tokens": 9, "temperature": 0.8, "top_k": 20,
     "seed": 5},
    {"tokens": [3, 1, 4, 1, 5], "max_new_tokens": 30, "temperature": 1.2, "top_p": 0.9},
]
LONG = {"tokens": [9, 8, 7], "max_new_tokens": 100, "temperature": 0.9, "seed": 1}
LONG2 = {"tokens": [2, 2], "max_new_tokens": 100, "temperature": 0.9, "seed": 2}
SHORT = {"tokens": [1, 2, 3, 4], "max_new_tokens": 3}


def _alone(model, r):
    return model.generate(torch.tensor([r["tokens"]]), r["max_new_tokens"],
                          temperature=r.get("temperature", 0.0), top_k=r.get("top_k"),
                          top_p=r.get("top_p"), seeds=[r.get("seed", SEED)])[0].tolist()


@pytest.fixture(scope="module")
def expected():
    torch.manual_seed(SEED)
    model = GPT2(CFG).eval()
    return {id(r): _alone(model, r) for r in REQUESTS + [LONG, LONG2, SHORT]}


@pytest.fixture
def server():
    made = []

    def make(slots):
        made.append(GPT2EngineServer(CFG, seed=SEED, slots=slots, device="cpu"))
        return made[-1]

    yield make
    for srv in made:
        srv.close()


def test_concurrent_requests_and_a_bad_one(server, expected):
    srv = server(3)
    bad = {"tokens": [1] * 100, "max_new_tokens": 40}  # 140 > 128

    async def calls():
        return await asyncio.gather(*(srv(r) for r in REQUESTS), srv(bad),
                                    srv({"tokens": [], "max_new_tokens": 3}))

    *got, err1, err2 = asyncio.run(calls())
    assert got == [{"tokens": expected[id(r)]} for r in REQUESTS]
    for e in (err1, err2):
        assert "error" in e and "tokens" not in e
    assert not srv.engine.has_work()


def test_short_request_overtakes_a_running_long_one(server, expected):
    srv = server(2)
    order = []

    async def calls():
        stream = srv.stream(LONG)
        first = await stream.__anext__()  # the long request is running
        assert first["tokens"] and not first.get("finished")

        async def rest():
            toks = list(first["tokens"])
            async for chunk in stream:
                toks.extend(chunk["tokens"])
                last = chunk
            order.append("long")
            assert last.get("finished")
            return toks

        async def short():
            got = await srv(SHORT)
            order.append("short")
            return got

        return await asyncio.gather(rest(), short())

    long_toks, short_got = asyncio.run(calls())
    assert short_got == {"tokens": expected[id(SHORT)]}
    assert long_toks == expected[id(LONG)]
    assert order == ["short", "long"]  # static batching answers both at the end


def test_closing_a_stream_frees_its_slot(server, expected):
    srv = server(2)
    order = []

    async def calls():
        long_task = asyncio.ensure_future(srv(LONG))
        long_task.add_done_callback(lambda _: order.append("long"))
        stream = srv.stream(LONG2)
        first = await stream.__anext__()
        assert first["tokens"]
        await stream.aclose()  # the consumer goes away: both slots were taken until now
        got = await srv(SHORT)
        order.append("short")
        return got, await long_task

    short_got, long_got = asyncio.run(calls())
    assert short_got == {"tokens": expected[id(SHORT)]}
    assert long_got == {"tokens": expected[id(LONG)]}
    assert order == ["short", "long"]
    assert not srv.engine.has_work()


@pytest.fixture(scope="module")
def cluster():
    ray.init(num_cpus=4)
    serve.start(http_options={"port": 18143})
    yield
    serve.shutdown()
    ray.shutdown()


def test_through_a_cluster(cluster, expected):
    app = build_gpt2_app(CFG, seed=SEED, continuous=True, slots=4, device="cpu")
    h = serve.run(app, name="gpt2-engine", route_prefix=None)
    resps = [h.remote(r) for r in REQUESTS]
    assert [r.result() for r in resps] == [{"tokens": expected[id(r)]} for r in REQUESTS]
    bad = h.remote({"tokens": [], "max_new_tokens": 3}).result()
    assert "error" in bad and "tokens" not in bad
    chunks = list(h.options(method_name="stream", stream=True).remote(REQUESTS[3]))
    assert len(chunks) > 1 and chunks[-1].get("finished")
    assert not any(c.get("finished") for c in chunks[:-1])
    assert [t for c in chunks for t in c["tokens"]] == expected[id(REQUESTS[3])]


def test_default_app_is_unchanged():
    app = build_gpt2_app(CFG)
    assert app.deployment.func_or_class is GPT2Server
    assert build_gpt2_app(CFG, continuous=True).deployment.func_or_class is GPT2EngineServer
