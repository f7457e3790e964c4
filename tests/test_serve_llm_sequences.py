"""serve.llm with ``"stop"``, ``"bad_words"`` and ``"no_repeat_ngram_size"`` in a request: both
servers answer what ``generate(..., seeds=[seed], <same rules>)`` answers on that request alone,
cut after its stop sequence or EOS; streamed chunks concatenate to it; a bad value, a field
the app was not built for and a grammar with a ban are that request's error and leave its
batch-mates unharmed (CPU)."""

import asyncio
import dataclasses
import json

import pytest
import torch
from test_gpt2_generate_sequences import cut, violations

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.serve.llm import GPT2EngineServer, GPT2Server, build_gpt2_app

SEED = 11
EOS = 7
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
V = CFG.vocab_size
TOL = 1e-3
FIELDS = ("stop", "bad_words", "no_repeat_ngram_size")
BASE = {"tokens": [5, 17], "max_new_tokens": 6}  # what the bad fields are added to
BAD = [{"stop": [[V]]}, {"stop": [[1]] * 9}, {"stop": [[]]}, {"stop": 3}, {"stop": "ab"},
       {"bad_words": [[-1]]}, {"bad_words": [list(range(9))]}, {"bad_words": [[1.5]]},
       {"no_repeat_ngram_size": 9}, {"no_repeat_ngram_size": True},
       {"no_repeat_ngram_size": "2"}, {"choices": [[3, 4]], "bad_words": [[3]]},
       {"choices": [[3, 4]], "no_repeat_ngram_size": 2}]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(SEED)
    return GPT2(CFG).eval()


def _generate(model, r, eos, **drop):
    kw = {k: r[k] for k in FIELDS if k in r and k not in drop}
    return model.generate(
        torch.tensor([r["tokens"]]), r["max_new_tokens"], temperature=r.get("temperature", 0.0),
        top_k=r.get("top_k"), top_p=r.get("top_p"), seeds=[r.get("seed", SEED)],
        eos_token_id=eos, logprobs=r.get("logprobs"), **kw)


@pytest.fixture(scope="module")
def requests(model):
    """The requests; the stops are taken from each request's own run under its bans, so that
    they act."""
    reqs = [
        {"tokens": [5, 17, 300, 42, 8, 99, 123], "max_new_tokens": 14, "no_repeat_ngram_size": 2},
        {"tokens": [7], "max_new_tokens": 5},
        {"tokens": list(range(20, 49)), "max_new_tokens": 16, "temperature": 0.8, "top_k": 20,
         "seed": 5, "logprobs": 2, "bad_words": [3, [4, 5]], "no_repeat_ngram_size": 1},
        {"tokens": [3, 1, 4, 1, 5], "max_new_tokens": 8, "temperature": 1.2, "top_p": 0.9},
        {"tokens": [9, 9], "max_new_tokens": 20, "temperature": 1.0, "seed": 2,
         "no_repeat_ngram_size": 3},
    ]
    for i, (end, n) in {0: (6, 2), 2: (5, 1), 3: (4, 3)}.items():
        got = _generate(model, reqs[i], EOS)
        toks = (got if reqs[i].get("logprobs") is None else got[0])[0].tolist()
        reqs[i]["stop"] = [[500, 501], toks[end - n: end]]
    first = _generate(model, reqs[4], EOS)[0].tolist()[0]
    reqs[4]["bad_words"] = [first]  # a bare token: the request's own first answer
    return reqs


def _expected(model, r, eos):
    """``generate`` on the request alone; ``eos`` as the server applies it to the request."""
    got = _generate(model, r, eos)
    stops = [[s] if isinstance(s, int) else s for s in r.get("stop", [])]
    if r.get("logprobs") is None:
        toks = got[0].tolist()
        return {"tokens": cut(toks, stops) if eos is not None else toks}
    toks, lp, ids, tlp = (t[0].tolist() for t in got)
    n = len(cut(toks, stops)) if eos is not None else len(toks)
    return {"tokens": toks[:n], "logprobs": lp[:n],
            "top_logprobs": [[[i, v] for i, v in zip(a, b)] for a, b in zip(ids[:n], tlp[:n])]}


def _same(got, want):
    assert sorted(got) == sorted(want), (got, want.keys())
    assert got["tokens"] == want["tokens"]
    if "logprobs" in want:
        assert max(abs(a - b) for a, b in zip(got["logprobs"], want["logprobs"])) < TOL
        for ga, wa in zip(got["top_logprobs"], want["top_logprobs"]):
            assert [p[0] for p in ga] == [p[0] for p in wa]
    json.dumps(got, allow_nan=False)


def _holds(r, toks):
    assert violations(r["tokens"], toks, r.get("bad_words", ()),
                      r.get("no_repeat_ngram_size", 0)) == []
    if "stop" in r and toks[-1] != EOS and len(toks) < r["max_new_tokens"]:
        assert toks[-len(r["stop"][1]):] == r["stop"][1]
        return 1
    return 0


def test_static_server(model, requests):
    srv = GPT2Server(CFG, seed=SEED, device="cpu", eos_token_id=EOS)
    bad = [dict(BASE, **b) for b in BAD]

    async def calls():
        return await asyncio.gather(*(GPT2Server._generate_batch(srv, r)
                                      for r in requests + bad))

    got = asyncio.run(calls())
    stopped = 0
    for g, r in zip(got, requests):
        # a request without a stop does not end at EOS on this server, whoever shares its batch
        _same(g, _expected(model, r, EOS if "stop" in r else None))
        stopped += _holds(r, g["tokens"])
    assert stopped == 3
    assert got[4]["tokens"] != _generate(model, requests[4], None, bad_words=1,
                                         no_repeat_ngram_size=1)[0].tolist()
    for e in got[len(requests):]:
        assert "error" in e and "tokens" not in e  # and the batch-mates were answered
    # a server without an EOS answers the bans, and says what a stop needs
    bare = GPT2Server(CFG, seed=SEED, device="cpu")

    async def pair():
        return await asyncio.gather(*(GPT2Server._generate_batch(bare, r)
                                      for r in (requests[0], requests[4], requests[1])))

    a, b, c = asyncio.run(pair())
    assert "eos_token_id" in a["error"]
    assert b == got[4] and c == got[1]


def test_continuous_app(model, requests):
    app = build_gpt2_app(CFG, seed=SEED, continuous=True, slots=3, device="cpu", logprobs=2,
                         eos_token_id=EOS, sequence_rules=True, grammar_states=16, speculate=2)
    srv = app.deployment.func_or_class(*app.args, **app.kwargs)
    try:
        bad = [dict(BASE, **b) for b in BAD]

        async def calls():
            whole = await asyncio.gather(*(srv(r) for r in requests + bad))
            chunks = [c async for c in srv.stream(requests[0])]
            return whole, chunks

        whole, chunks = asyncio.run(calls())
        stopped = 0
        for g, r in zip(whole, requests):
            _same(g, _expected(model, r, EOS))
            stopped += _holds(r, g["tokens"])
        assert stopped == 3
        for e in whole[len(requests):]:
            assert "error" in e and "tokens" not in e
        streamed = [t for c in chunks for t in c["tokens"]]
        assert streamed == whole[0]["tokens"] and chunks[-1]["finished"]
        assert not srv.engine.has_work()
        # a grammar goes with a stop
        ok = asyncio.run(srv(dict(BASE, choices=[[3, 4, 5, 6]], stop=[[4, 5]])))
        assert ok["tokens"] == [3, 4, 5]
    finally:
        srv.close()


def test_apps_without_the_option(requests):
    srv = GPT2EngineServer(CFG, seed=SEED, device="cpu", slots=2, eos_token_id=EOS)
    try:
        assert not hasattr(srv.engine, "seq")

        async def calls():
            return await asyncio.gather(srv(requests[0]), srv(requests[4]), srv(requests[1]))

        a, b, ok = asyncio.run(calls())
        assert "sequence_rules=True" in a["error"] and "sequence_rules=True" in b["error"]
        assert 1 <= len(ok["tokens"]) <= 5  # the bad requests touched nothing
    finally:
        srv.close()
    with pytest.raises(ValueError, match="continuous=True"):
        build_gpt2_app(CFG, sequence_rules=True)
