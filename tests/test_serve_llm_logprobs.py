"""serve.llm with ``"logprobs": m`` in a request: both servers answer with the per-token
log-probabilities and the top-m alternatives of ``generate(..., logprobs=m)`` on that
request alone, streamed chunks carry the slice for their tokens, a bad value is that
request's error, and a request without the field gets the response it always got (CPU)."""

import asyncio
import dataclasses
import json

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.serve.llm import GPT2EngineServer, GPT2Server, build_gpt2_app

SEED = 11
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
REQUESTS = [
    {"tokens": [5, 17, 300, 42, 8, 99, 123], "max_new_tokens": 12, "logprobs": 2},
    {"tokens": [7], "max_new_tokens": 5, "temperature": 0.0},
    {"tokens": list(range(20, 49)), "max_new_tokens": 9, "temperature": 0.8, "top_k": 20,
     "seed": 5, "logprobs": 0},
    {"tokens": [3, 1, 4, 1, 5], "max_new_tokens": 30, "temperature": 1.2, "top_p": 0.9,
     "logprobs": 4},
]
TOL = 1e-3  # as in test_token_logprobs.py: summation order against a wrong position


@pytest.fixture(scope="module")
def expected():
    """Each request through ``generate`` alone: the response it should get."""
    torch.manual_seed(SEED)
    model = GPT2(CFG).eval()
    res = []
    for r in REQUESTS:
        m = r.get("logprobs")
        got = model.generate(torch.tensor([r["tokens"]]), r["max_new_tokens"],
                             temperature=r.get("temperature", 0.0), top_k=r.get("top_k"),
                             top_p=r.get("top_p"), seeds=[r.get("seed", SEED)], logprobs=m)
        if m is None:
            res.append({"tokens": got[0].tolist()})
        else:
            toks, lp, ids, tlp = (t[0].tolist() for t in got)
            res.append({"tokens": toks, "logprobs": lp,
                        "top_logprobs": [[[i, v] for i, v in zip(a, b)]
                                         for a, b in zip(ids, tlp)]})
    return res


def _same(got, want):
    """The response ``got`` is ``want``: tokens and ids exactly, values within TOL."""
    assert sorted(got) == sorted(want), (got.keys(), want.keys())
    assert got["tokens"] == want["tokens"]
    if "logprobs" in want:
        n = len(want["tokens"])
        assert len(got["logprobs"]) == n and len(got["top_logprobs"]) == n
        assert max(abs(a - b) for a, b in zip(got["logprobs"], want["logprobs"])) < TOL
        for ga, wa in zip(got["top_logprobs"], want["top_logprobs"]):
            assert [p[0] for p in ga] == [p[0] for p in wa]
            assert all(abs(p[1] - q[1]) < TOL for p, q in zip(ga, wa))
    json.dumps(got, allow_nan=False)  # nothing non-finite reaches the wire


def test_static_server_fields_and_errors(expected):
    srv = GPT2Server(CFG, seed=SEED, device="cpu")
    bad = [dict(REQUESTS[0], logprobs=9), dict(REQUESTS[0], logprobs=-1),
           dict(REQUESTS[0], logprobs=True), dict(REQUESTS[0], logprobs="3")]

    async def calls():
        return await asyncio.gather(*(GPT2Server._generate_batch(srv, r)
                                      for r in REQUESTS + bad))

    got = asyncio.run(calls())
    for g, w in zip(got, expected):
        _same(g, w)
    assert len(got[3]["top_logprobs"][0]) == 4 and len(got[0]["top_logprobs"][0]) == 2
    assert got[2]["top_logprobs"] == [[]] * 9  # m = 0: the chosen token's value only
    for e in got[4:]:
        assert "error" in e and "tokens" not in e  # and the batch-mates were answered
    # a greedy batch with one logprobs request goes through the sampled path and still
    # answers the greedy request with the response it always got
    greedy = {"tokens": [5, 17, 300, 42, 8, 99, 123], "max_new_tokens": 12}

    async def pair():
        return await asyncio.gather(GPT2Server._generate_batch(srv, greedy),
                                    GPT2Server._generate_batch(srv, REQUESTS[0]))

    a, b = asyncio.run(pair())
    assert a == {"tokens": expected[0]["tokens"]}
    _same(b, expected[0])


def test_non_finite_values_are_none():
    from ray_amd.serve.llm import _logprob_fields

    got = _logprob_fields([-1.5, float("-inf"), float("nan")], [[3, -1]] * 3,
                          [[-0.5, float("-inf")]] * 3, 2)
    assert got == {"logprobs": [-1.5, None, None],
                   "top_logprobs": [[[3, -0.5], [-1, None]]] * 3}


@pytest.fixture
def server():
    made = []

    def make(**kw):
        made.append(GPT2EngineServer(CFG, seed=SEED, device="cpu", **kw))
        return made[-1]

    yield make
    for srv in made:
        srv.close()


def test_engine_server_fields_streams_and_errors(expected):
    app = build_gpt2_app(CFG, seed=SEED, continuous=True, slots=3, device="cpu", logprobs=4)
    assert app.deployment.func_or_class is GPT2EngineServer
    srv = app.deployment.func_or_class(*app.args, **app.kwargs)
    try:
        assert srv.engine.logprobs == 4
        too_many = dict(REQUESTS[0], logprobs=5)

        async def calls():
            whole = await asyncio.gather(*(srv(r) for r in REQUESTS), srv(too_many),
                                         srv(dict(REQUESTS[1], logprobs=1.5)))
            chunks = [c async for c in srv.stream(REQUESTS[3])]
            plain = [c async for c in srv.stream(REQUESTS[1])]
            return whole, chunks, plain

        whole, chunks, plain = asyncio.run(calls())
        for g, w in zip(whole, expected):
            _same(g, w)
        for e in whole[4:]:
            assert "error" in e and "tokens" not in e
        # every chunk's fields are aligned with its own tokens; together they are the answer
        assert len(chunks) > 1 and chunks[-1].get("finished")
        for c in chunks:
            assert len(c["logprobs"]) == len(c["tokens"]) == len(c["top_logprobs"])
        joined = {k: [v for c in chunks for v in c[k]]
                  for k in ("tokens", "logprobs", "top_logprobs")}
        _same(joined, expected[3])
        # a request without the field: chunks of tokens only
        assert all(sorted(c) in (["tokens"], ["finished", "tokens"]) for c in plain)
        assert [t for c in plain for t in c["tokens"]] == expected[1]["tokens"]
        assert not srv.engine.has_work()
    finally:
        srv.close()


def test_engine_server_without_the_option(server, expected):
    srv = server(slots=2)
    assert srv.engine.logprobs is None

    async def calls():
        return await asyncio.gather(srv(REQUESTS[0]), srv(REQUESTS[1]))

    err, ok = asyncio.run(calls())
    assert "error" in err and "logprobs" in err["error"] and "tokens" not in err
    assert ok == expected[1]  # today's response, and the bad request touched nothing
    chunks = asyncio.run(_collect(srv.stream(REQUESTS[0])))
    assert len(chunks) == 1 and "error" in chunks[0] and chunks[0]["finished"]


async def _collect(agen):
    return [c async for c in agen]
