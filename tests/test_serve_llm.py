"""serve.llm: concurrent generation requests of different prompt lengths and different
``max_new_tokens`` go through ``@serve.batch`` into one ragged ``generate`` call, and each
gets exactly what an un-batched ``generate`` of the same seeded model returns (CPU)."""

import asyncio
import dataclasses

import pytest
import torch

import ray_amd as ray
from ray_amd import serve
from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.serve.llm import GPT2Server, build_gpt2_app

SEED = 11
# a larger init than tiny()'s default, at which greedy decoding emits one constant token
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
REQUESTS = [
    {"tokens": [5, 17, 300, 42, 8, 99, 123], "max_new_tokens": 12},
    {"tokens": [7], "max_new_tokens": 5, "temperature": 0.0},
    {"tokens": list(range(20, 49)), "max_new_tokens": 9},
]


@pytest.fixture(scope="module")
def expected():
    torch.manual_seed(SEED)
    model = GPT2(CFG).eval()
    return [model.generate(torch.tensor([r["tokens"]]), r["max_new_tokens"])[0].tolist()
            for r in REQUESTS]


@pytest.fixture(scope="module")
def cluster():
    ray.init(num_cpus=4)
    serve.start(http_options={"port": 18127})
    yield
    serve.shutdown()
    ray.shutdown()


def test_batched_requests_match_unbatched_generate(cluster, expected):
    app = build_gpt2_app(CFG, seed=SEED, max_batch_size=8, batch_wait_timeout_s=0.5)
    h = serve.run(app, name="gpt2", route_prefix=None)
    resps = [h.remote(r) for r in REQUESTS]
    got = [r.result() for r in resps]
    for g, want, req in zip(got, expected, REQUESTS):
        assert g == {"tokens": want}
        assert len(g["tokens"]) == req["max_new_tokens"]
    bad = h.remote({"tokens": [], "max_new_tokens": 3}).result()
    assert "error" in bad and "tokens" not in bad


def test_server_pads_and_cuts_each_row(expected):
    """The batch body itself, without a cluster: one ragged call, rows cut at their own
    max_new_tokens, a too-long request reported without failing the others."""
    srv = GPT2Server(CFG, seed=SEED, device="cpu")
    assert srv._run(REQUESTS) == expected
    long = {"tokens": [1] * 100, "max_new_tokens": 40, "temperature": 0.5}  # 140 > 128

    async def calls():
        one = await GPT2Server._generate_batch(srv, REQUESTS[0])
        two = await asyncio.gather(GPT2Server._generate_batch(srv, long),
                                   GPT2Server._generate_batch(srv, REQUESTS[1]))
        return one, two

    one, (a, b) = asyncio.run(calls())
    assert one == {"tokens": expected[0]}
    assert "error" in a and b == {"tokens": expected[1]}
