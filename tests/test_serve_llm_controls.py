"""serve.llm with the logit-processor fields in a request (``repetition_penalty``,
``presence_penalty``, ``frequency_penalty``, ``min_new_tokens``, ``logit_bias``): both servers
answer what ``generate(..., seeds=[seed], <same controls>)`` answers on that request alone, a
bad value is that request's error, and the continuous app without ``logit_processors=True``
rejects the fields with a clear error (CPU)."""

import asyncio
import dataclasses
import json

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.serve.llm import (GPT2EngineServer, GPT2Server, _request_controls,
                               build_gpt2_app)

SEED = 11
EOS = 300
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
REQUESTS = [
    {"tokens": [5, 17, 300, 42, 8, 99, 123], "max_new_tokens": 12, "repetition_penalty": 1.3,
     "frequency_penalty": 0.5},
    {"tokens": [7], "max_new_tokens": 5},
    {"tokens": list(range(20, 49)), "max_new_tokens": 9, "temperature": 0.8, "top_k": 20,
     "seed": 5, "logit_bias": {"31": 3.0, 40: float("-inf"), "7": -1.5}, "logprobs": 2},
    {"tokens": [3, 1, 4, 1, 5], "max_new_tokens": 30, "temperature": 1.2, "top_p": 0.9,
     "presence_penalty": 0.8, "repetition_penalty": 1},
]
WITH_EOS = {"tokens": [9, 9, 9], "max_new_tokens": 10, "min_new_tokens": 7, "temperature": 1.0,
            "seed": 3}
BAD = [{"repetition_penalty": 0}, {"repetition_penalty": "1.2"}, {"presence_penalty": [0.1]},
       {"frequency_penalty": float("inf")}, {"logit_bias": [[3, 1.0]]},
       {"logit_bias": {"x": 1.0}}, {"logit_bias": {"3.5": 1.0}}, {"logit_bias": {"512": 1.0}},
       {"logit_bias": {"3": None}}, {"logit_bias": {"3": 1.0, 3: 2.0}},
       {"logit_bias": {str(i): 1.0 for i in range(65)}}, {"min_new_tokens": -1},
       {"min_new_tokens": 13}, {"min_new_tokens": True}]
TOL = 1e-3


def _expected(model, r, eos=None):
    bias = r.get("logit_bias")
    got = model.generate(
        torch.tensor([r["tokens"]]), r["max_new_tokens"], temperature=r.get("temperature", 0.0),
        top_k=r.get("top_k"), top_p=r.get("top_p"), seeds=[r.get("seed", SEED)],
        eos_token_id=eos, logprobs=r.get("logprobs"),
        logit_bias=None if bias is None else {int(k): v for k, v in bias.items()},
        **{k: r.get(k) for k in ("repetition_penalty", "presence_penalty", "frequency_penalty",
                                 "min_new_tokens")})
    if r.get("logprobs") is None:
        toks = got[0].tolist()
        return {"tokens": toks[: toks.index(eos) + 1] if eos in toks else toks}
    toks, lp, ids, tlp = (t[0].tolist() for t in got)
    n = toks.index(eos) + 1 if eos in toks else len(toks)
    return {"tokens": toks[:n], "logprobs": lp[:n],
            "top_logprobs": [[[i, v] for i, v in zip(a, b)] for a, b in zip(ids[:n], tlp[:n])]}


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(SEED)
    return GPT2(CFG).eval()


def _same(got, want):
    assert sorted(got) == sorted(want), (got, want.keys())
    assert got["tokens"] == want["tokens"]
    if "logprobs" in want:
        assert max(abs(a - b) for a, b in zip(got["logprobs"], want["logprobs"])) < TOL
        for ga, wa in zip(got["top_logprobs"], want["top_logprobs"]):
            assert [p[0] for p in ga] == [p[0] for p in wa]
    json.dumps(got, allow_nan=False)


def test_field_parsing():
    r = dict(REQUESTS[2])
    assert _request_controls(CFG, r, 9, None) == {"logit_bias": {31: 3.0, 40: float("-inf"),
                                                                 7: -1.5}}
    assert _request_controls(CFG, REQUESTS[1], 5, None) == {}
    assert _request_controls(CFG, {"logit_bias": None, "repetition_penalty": None}, 5, None) == {}
    assert _request_controls(CFG, WITH_EOS, 10, EOS) == {"min_new_tokens": 7}
    with pytest.raises(ValueError, match="eos_token_id"):
        _request_controls(CFG, WITH_EOS, 10, None)
    with pytest.raises(ValueError, match="logit_processors=True"):
        _request_controls(CFG, REQUESTS[0], 12, None, enabled=False)
    for bad in BAD:
        with pytest.raises(ValueError):
            _request_controls(CFG, bad, 12, EOS)


def test_static_server_agrees_with_generate_and_errors_are_per_request(model):
    srv = GPT2Server(CFG, seed=SEED, device="cpu")
    bad = [dict(REQUESTS[0], **b) for b in BAD] + [WITH_EOS]  # (the static server has no EOS)

    async def calls():
        return await asyncio.gather(*(GPT2Server._generate_batch(srv, r)
                                      for r in REQUESTS + bad))

    got = asyncio.run(calls())
    for g, r in zip(got, REQUESTS):
        _same(g, _expected(model, r))
    assert got[0]["tokens"] != _expected(model, {k: v for k, v in REQUESTS[0].items()
                                                 if "penalty" not in k})["tokens"]
    assert 40 not in got[2]["tokens"]
    for e in got[len(REQUESTS):]:
        assert "error" in e and "tokens" not in e  # and the batch-mates were answered
    # an all-greedy batch with one controlled request takes the device-sampler path and
    # still answers the plain request with what it always got
    plain = {"tokens": [5, 17, 300, 42, 8, 99, 123], "max_new_tokens": 12}

    async def pair():
        return await asyncio.gather(GPT2Server._generate_batch(srv, plain),
                                    GPT2Server._generate_batch(srv, REQUESTS[0]))

    a, b = asyncio.run(pair())
    assert a == {"tokens": model.generate(torch.tensor([plain["tokens"]]), 12)[0].tolist()}
    _same(b, _expected(model, REQUESTS[0]))


def test_continuous_app_agrees_with_generate(model):
    app = build_gpt2_app(CFG, seed=SEED, continuous=True, slots=3, device="cpu", logprobs=2,
                         eos_token_id=EOS, logit_processors=True)
    srv = app.deployment.func_or_class(*app.args, **app.kwargs)
    try:
        assert srv.engine.ctl is not None
        bad = [dict(REQUESTS[0], **b) for b in BAD]

        async def calls():
            whole = await asyncio.gather(*(srv(r) for r in REQUESTS + [WITH_EOS] + bad))
            chunks = [c async for c in srv.stream(REQUESTS[3])]
            return whole, chunks

        whole, chunks = asyncio.run(calls())
        for g, r in zip(whole, REQUESTS + [WITH_EOS]):
            _same(g, _expected(model, r, EOS))
        assert EOS not in whole[4]["tokens"][:7]
        for e in whole[5:]:
            assert "error" in e and "tokens" not in e
        assert [t for c in chunks for t in c["tokens"]] == _expected(model, REQUESTS[3],
                                                                     EOS)["tokens"]
        assert not srv.engine.has_work()
    finally:
        srv.close()


def test_continuous_app_without_the_flag():
    srv = GPT2EngineServer(CFG, seed=SEED, device="cpu", slots=2)
    try:
        assert srv.engine.ctl is None

        async def calls():
            whole = await asyncio.gather(srv(REQUESTS[0]), srv(REQUESTS[1]))
            return whole, [c async for c in srv.stream(REQUESTS[3])]

        (err, ok), chunks = asyncio.run(calls())
        assert "error" in err and "logit_processors=True" in err["error"] and "tokens" not in err
        assert len(ok["tokens"]) == 5  # the bad request touched nothing
        assert len(chunks) == 1 and "error" in chunks[0] and chunks[0]["finished"]
    finally:
        srv.close()
