"""The token sampler's definition (``ref.sample_logits``, plain torch, CPU): the hash, every
rule on hand-made rows, the frequencies; ``GPT2.generate(seeds=...)`` through it, and
``serve.llm`` batching requests with their own sampling parameters into one call."""

import asyncio
import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.serve.llm import GPT2Server

INF = float("inf")


def _draw(rows, u, T=1.0, k=0, p=1.0, vocab_size=None, dtype=torch.float64):
    """``_sample_logits_u`` on a list of rows; scalars are broadcast over the rows."""
    x = torch.tensor(rows, dtype=torch.float32)
    B = x.shape[0]

    def col(v, dt):
        return torch.tensor(v if isinstance(v, list) else [v] * B, dtype=dt)

    return ref._sample_logits_u(x, col(T, torch.float32), col(k, torch.int32),
                                col(p, torch.float32), col(u, torch.float64), vocab_size,
                                dtype=dtype).tolist()


# ------------------------------------------------------------------------------- hash
def test_hash_known_answers():
    cases = [((0, 0), 0.8833107948303223), ((1, 0), 0.5665615200996399),
             ((0, 1), 0.4315279722213745), ((2 ** 63 + 5, 1023), 0.1936417818069458)]
    for (seed, step), want in cases:
        seed = seed - 2 ** 64 if seed >= 2 ** 63 else seed  # the same 64 bits as int64
        u = ref.sample_uniform(torch.tensor([seed]), torch.tensor([step], dtype=torch.int32))
        assert u.dtype == torch.float32 and float(u[0]) == want, (seed, step, float(u[0]))
    many = ref.sample_uniform(torch.arange(1000), torch.zeros(1000, dtype=torch.int32))
    assert many.min() >= 0 and many.max() < 1


# ------------------------------------------------------------------------------ rules
def test_greedy_tie_picks_lowest_index():
    assert _draw([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]], 0.99, T=0.0) == [1, 0]


def test_k1_is_the_maximum():
    row = [0.5, 2.0, -1.0, 1.9]
    assert _draw([row] * 3, [0.0, 0.5, 0.999999], k=1) == [1, 1, 1]


def test_ties_at_the_kth_value_are_kept():
    # k = 2, but three tokens tie at the second largest value: four are kept, equal mass
    # for the tied ones. w = e^0, e^-1, e^-1, e^-1 at indices 4, 0, 2, 5.
    row = [1.0, -3.0, 1.0, -9.0, 2.0, 1.0]
    e = torch.tensor([-1.0], dtype=torch.float64).exp().item()
    tot = 1 + 3 * e
    # index order of the kept: 0 (e), 2 (e), 4 (1), 5 (e)
    us = [0.5 * e / tot, 1.5 * e / tot, (2 * e + 0.5) / tot, (2 * e + 1 + 0.5 * e) / tot]
    assert _draw([row] * 4, us, k=2) == [0, 2, 4, 5]
    assert all(t in (0, 2, 4, 5) for t in _draw([row] * 64, [i / 64 for i in range(64)], k=2))


def test_k_off_for_k_le_0_and_k_ge_v():
    row = [0.0, 0.0, 0.0, 0.0]
    us = [0.1, 0.3, 0.6, 0.9]
    for k in (0, -3, 4, 100):
        assert _draw([row] * 4, us, k=k) == [0, 1, 2, 3], k
    assert _draw([row] * 4, us, k=3) == [0, 1, 2, 3]  # all tie at the 3rd value


def test_p1_is_off_and_tiny_p_keeps_the_top_class():
    row = [0.0, 2.0, -1.0, 2.0, 1.0]
    us = [i / 50 for i in range(50)]
    assert set(_draw([row] * 50, us, p=1.0)) == {0, 1, 2, 3, 4}
    got = _draw([row] * 50, us, p=1e-6)
    assert set(got) == {1, 3}  # exactly the top tie class, both members
    assert got[:25] == [1] * 25 and got[25:] == [3] * 25


def test_top_p_classes_stand_or_fall_together():
    # masses 0.4, 0.2, 0.2, 0.1, 0.1 (as logits: their logs). The mass strictly above the
    # 0.2 class is 0.4, above the 0.1 class 0.8.
    probs = [0.1, 0.2, 0.4, 0.2, 0.1]
    row = torch.tensor(probs, dtype=torch.float64).log().float().tolist()
    us = [i / 40 for i in range(40)]
    assert set(_draw([row] * 40, us, p=0.3)) == {2}
    assert set(_draw([row] * 40, us, p=0.41)) == {1, 2, 3}
    assert set(_draw([row] * 40, us, p=0.79)) == {1, 2, 3}
    assert set(_draw([row] * 40, us, p=0.81)) == {0, 1, 2, 3, 4}


def test_minus_inf_is_never_drawn():
    row = [-INF, 0.0, -INF, 0.0, -INF]
    us = [0.0, 0.25, 0.5, 0.75, 0.999999]
    for kw in ({}, {"k": 4}, {"p": 0.999}):
        assert set(_draw([row] * 5, us, **kw)) == {1, 3}, kw
    assert _draw([row], 0.5, T=0.0) == [1]


def test_columns_past_vocab_size_are_ignored():
    row = [0.0, 1.0, 0.0, INF, INF]
    us = [0.0, 0.3, 0.6, 0.999999]
    for kw in ({}, {"k": 2}, {"p": 0.5}, {"T": 0.0}):
        assert max(_draw([row] * 4, us, vocab_size=3, **kw)) < 3, kw
    assert _draw([row], 0.5, T=0.0, vocab_size=3) == [1]


def test_u_around_a_boundary():
    # w = 1/4, 1/2, 1/4 exactly (logits are logs of powers of two up to rounding of log 2,
    # which the fp64 run resolves far below the 1e-9 steps used here)
    row = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64).log().float().tolist()
    d = 1e-6
    assert _draw([row] * 4, [0.25 - d, 0.25 + d, 0.75 - d, 0.75 + d]) == [0, 1, 1, 2]
    assert _draw([row] * 2, [0.0, 1 - 2.0 ** -24]) == [0, 2]


def test_temperature_scales_the_logits():
    row = [0.0, 1.0]
    for T in (0.5, 2.0):
        p0 = 1 / (1 + torch.tensor(1.0 / T, dtype=torch.float64).exp().item())
        assert _draw([row] * 2, [p0 - 1e-6, p0 + 1e-6], T=T) == [0, 1]


def test_rows_are_independent():
    rows = [[0.0, 1.0, 2.0, 3.0], [3.0, 2.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    T, k, p, u = [0.0, 0.7, 1.0], [0, 2, 0], [1.0, 1.0, 0.6], [0.9, 0.9, 0.9]
    mixed = _draw(rows, u, T=T, k=k, p=p)
    alone = [_draw([rows[i]], [u[i]], T=[T[i]], k=[k[i]], p=[p[i]])[0] for i in range(3)]
    assert mixed == alone


# -------------------------------------------------------------------------- frequencies
CHI2_LOGITS = [0.0, 1.0, -0.5, 2.0, 0.25, -1.5, 1.5, 0.75]
CHI2_BOUND = 24.32  # the 0.001 upper quantile of chi-square with 7 degrees of freedom
CHI2_BASE = 1000    # seeds base..base+4095; the reference's statistic for it is printed
CHI2_ROWS = 4096


def chi2_inputs(device="cpu", dtype=torch.float32):
    n = CHI2_ROWS
    return (torch.tensor(CHI2_LOGITS, dtype=dtype, device=device).repeat(n, 1),
            torch.ones(n, dtype=torch.float32, device=device),
            torch.zeros(n, dtype=torch.int32, device=device),
            torch.ones(n, dtype=torch.float32, device=device),
            torch.arange(CHI2_BASE, CHI2_BASE + n, dtype=torch.int64, device=device),
            torch.zeros(n, dtype=torch.int32, device=device))


def chi2_statistic(tokens):
    probs = torch.softmax(torch.tensor(CHI2_LOGITS, dtype=torch.float64), 0)
    counts = torch.bincount(tokens.cpu(), minlength=8).double()
    assert counts.numel() == 8 and counts.sum() == CHI2_ROWS
    want = probs * CHI2_ROWS
    return float(((counts - want) ** 2 / want).sum())


def test_frequencies_chi_square():
    stat = chi2_statistic(ref.sample_logits(*chi2_inputs()))
    print(f"chi-square over {CHI2_ROWS} draws, seeds from {CHI2_BASE}: {stat:.3f}")
    assert stat < CHI2_BOUND


# ------------------------------------------------------------------------------ dispatch
def test_functional_checks_arguments():
    B, V = 2, 5
    lg = torch.zeros(B, V)
    ok = dict(temperature=torch.ones(B), top_k=torch.zeros(B, dtype=torch.int32),
              top_p=torch.ones(B), seeds=torch.zeros(B, dtype=torch.int64),
              steps=torch.zeros(B, dtype=torch.int32))
    assert rf.sample_logits(lg, **ok).dtype == torch.int64
    bad = [("temperature", torch.ones(B, dtype=torch.float64)), ("temperature", torch.ones(3)),
           ("temperature", -torch.ones(B)), ("top_k", torch.zeros(B, dtype=torch.int64)),
           ("top_p", torch.ones(B, 1)), ("seeds", torch.zeros(B, dtype=torch.int32)),
           ("steps", torch.zeros(B, dtype=torch.int64))]
    for name, value in bad:
        with pytest.raises(ValueError):
            rf.sample_logits(lg, **{**ok, name: value})
    with pytest.raises(ValueError):
        rf.sample_logits(torch.zeros(V), **ok)
    with pytest.raises(ValueError):
        rf.sample_logits(lg, vocab_size=V + 1, **ok)


def test_functional_eos_latch_on_the_reference_path():
    lg = torch.tensor([[0.0, 9.0, 0.0]] * 3)
    z = torch.zeros(3, dtype=torch.int32)
    done = torch.tensor([1, 0, 0], dtype=torch.uint8)
    T = torch.tensor([0.0, 0.0, 0.0])
    tok = rf.sample_logits(lg, T, z, torch.ones(3), torch.zeros(3, dtype=torch.int64), z,
                           done=done, eos_token_id=2)
    assert tok.tolist() == [2, 1, 1] and done.tolist() == [1, 0, 0]
    tok = rf.sample_logits(lg, T, z, torch.ones(3), torch.zeros(3, dtype=torch.int64), z,
                           done=done, eos_token_id=1)
    assert tok.tolist() == [1, 1, 1] and done.tolist() == [1, 1, 1]


# ------------------------------------------------------------------------------ generate
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
NEW = 12
PROMPTS = [[5, 17, 300, 42, 8, 99, 123], [7], list(range(20, 31))]
PARAMS = [dict(temperature=0.8, top_k=20, top_p=0.9, seed=3),
          dict(temperature=1.3, top_k=0, top_p=1.0, seed=4),
          dict(temperature=1.0, top_k=0, top_p=0.7, seed=5)]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(11)
    return GPT2(CFG).eval()


def _padded(prompts):
    lens = [len(p) for p in prompts]
    idx = torch.zeros(len(prompts), max(lens), dtype=torch.long)
    for b, p in enumerate(prompts):
        idx[b, : lens[b]] = torch.tensor(p)
    return idx, lens


def _gen(model, rows, new=NEW, **kw):
    idx, lens = _padded([PROMPTS[b] for b in rows])
    return model.generate(idx, new, lens=lens,
                          temperature=[PARAMS[b]["temperature"] for b in rows],
                          top_k=[PARAMS[b]["top_k"] for b in rows],
                          top_p=[PARAMS[b]["top_p"] for b in rows],
                          seeds=[PARAMS[b]["seed"] for b in rows], **kw)


@pytest.fixture(scope="module")
def batch_of_three(model):
    return _gen(model, [0, 1, 2])


def test_generate_same_seeds_same_tokens(model, batch_of_three):
    assert batch_of_three.dtype == torch.int64 and batch_of_three.shape == (3, NEW)
    assert torch.equal(_gen(model, [0, 1, 2]), batch_of_three)
    assert int(batch_of_three.max()) < CFG.vocab_size and int(batch_of_three.min()) >= 0


def test_generate_different_seeds_different_tokens(model):
    idx, lens = _padded(PROMPTS)
    a = model.generate(idx, NEW, lens=lens, temperature=1.0, seeds=1)
    b = model.generate(idx, NEW, lens=lens, temperature=1.0, seeds=2)
    c = model.generate(idx, NEW, lens=lens, temperature=1.0, seeds=[1, 1, 1])
    assert torch.equal(a, c)  # a scalar seed is that seed in every row
    assert all(not torch.equal(a[r], b[r]) for r in range(3))


def test_generate_row_alone_equals_row_in_a_mixed_batch(model, batch_of_three):
    for b in range(3):
        assert torch.equal(_gen(model, [b])[0], batch_of_three[b]), b


def test_generate_temperature_0_rows_equal_generate_without_seeds(model):
    idx, lens = _padded(PROMPTS)
    greedy = model.generate(idx, NEW, lens=lens)
    assert torch.equal(model.generate(idx, NEW, lens=lens, seeds=9), greedy)
    mixed = model.generate(idx, NEW, lens=lens, temperature=[0.0, 1.2, 0.0], top_p=[0.5, 0.9, None],
                           seeds=[1, 2, 3])
    assert torch.equal(mixed[0], greedy[0]) and torch.equal(mixed[2], greedy[2])
    assert not torch.equal(mixed[1], greedy[1])
    one = model.generate(idx, 1, lens=lens, seeds=0)
    assert torch.equal(one, greedy[:, :1])


def test_generate_eos_latches(model, batch_of_three):
    row = max(range(3), key=lambda b: len(set(batch_of_three[b].tolist())))
    eos = int(batch_of_three[row, 4])
    out = _gen(model, [0, 1, 2], eos_token_id=eos)
    for b in range(3):
        want = batch_of_three[b].clone()
        hit = (want == eos).nonzero()
        if hit.numel():
            want[int(hit[0]):] = eos
        assert torch.equal(out[b], want), b
    assert (out[row, 4:] == eos).all()


def test_generate_value_errors(model):
    idx, lens = _padded(PROMPTS)
    with pytest.raises(ValueError):
        model.generate(idx, 4, lens=lens, temperature=1.0, seeds=1,
                       generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="seeds"):
        model.generate(idx, 4, lens=lens, temperature=1.0, top_p=0.9)
    with pytest.raises(ValueError, match="seeds"):
        model.generate(idx, 4, lens=lens, temperature=[1.0, 0.5, 0.0])
    with pytest.raises(ValueError, match="seeds"):
        model.generate(idx, 4, lens=lens, temperature=1.0, top_k=[5, 5, 5])
    with pytest.raises(ValueError):
        model.generate(idx, 4, lens=lens, temperature=[1.0, -0.5, 0.0], seeds=1)
    with pytest.raises(ValueError):
        model.generate(idx, 4, lens=lens, temperature=[1.0, 0.5], seeds=1)
    with pytest.raises(ValueError):
        model.generate(idx, 4, lens=lens, temperature=1.0, seeds=[1, 2])


# --------------------------------------------------------------------------------- serve
SEED = 11
REQUESTS = [
    {"tokens": [5, 17, 300, 42, 8, 99, 123], "max_new_tokens": 12},
    {"tokens": [7], "max_new_tokens": 5, "temperature": 0.0},
    {"tokens": list(range(20, 49)), "max_new_tokens": 9},
]
SAMPLED = [
    {"tokens": PROMPTS[0], "max_new_tokens": 12, "temperature": 0.8, "top_p": 0.9, "seed": 3},
    {"tokens": PROMPTS[1], "max_new_tokens": 5, "temperature": 1.3, "top_p": 0.95, "seed": 4},
    {"tokens": PROMPTS[2], "max_new_tokens": 9, "temperature": 0.6, "top_p": 0.7, "seed": 5,
     "top_k": 30},
]


@pytest.fixture()
def server():
    srv = GPT2Server(CFG, seed=SEED, device="cpu")
    calls = []
    inner = srv.model.generate

    def counted(*a, **kw):
        calls.append(kw)
        return inner(*a, **kw)

    srv.model.generate = counted
    return srv, calls


def _serve(srv, reqs):
    async def go():
        return await asyncio.gather(*[GPT2Server._generate_batch(srv, r) for r in reqs])

    return asyncio.run(go())


def test_serve_mixed_parameters_are_one_generate_call(server):
    srv, calls = server
    got = _serve(srv, SAMPLED)
    assert len(calls) == 1, len(calls)
    assert calls[0]["seeds"] == [3, 4, 5]
    calls.clear()
    for r, g in zip(SAMPLED, got):
        alone = srv.model.generate(torch.tensor([r["tokens"]]), r["max_new_tokens"],
                                   temperature=r["temperature"], top_k=r.get("top_k"),
                                   top_p=r["top_p"], seeds=[r["seed"]])[0].tolist()
        assert g == {"tokens": alone}, r
        assert len(g["tokens"]) == r["max_new_tokens"]


def test_serve_greedy_rides_along_and_default_seed(server):
    srv, calls = server
    reqs = [REQUESTS[0], {"tokens": [9, 8, 7], "max_new_tokens": 6, "temperature": 1.1}]
    got = _serve(srv, reqs)
    assert len(calls) == 1
    assert calls[0]["seeds"] == [SEED, SEED] and calls[0]["temperature"] == [0.0, 1.1]
    calls.clear()
    greedy = srv.model.generate(torch.tensor([REQUESTS[0]["tokens"]]), 12)[0].tolist()
    assert got[0] == {"tokens": greedy}
    alone = srv.model.generate(torch.tensor([[9, 8, 7]]), 6, temperature=1.1, seeds=SEED)
    assert got[1] == {"tokens": alone[0].tolist()}


def test_serve_bad_sampled_requests_error_alone(server):
    srv, calls = server
    n_pos = CFG.n_positions
    long = {"tokens": [1] * 100, "max_new_tokens": 40, "temperature": 0.5, "seed": 1}
    reqs = [SAMPLED[0], long, {"tokens": [], "temperature": 0.7},
            {"tokens": [3, 4], "temperature": -1.0}, {"tokens": [3, 4], "top_p": 1.5},
            {"tokens": [3, CFG.vocab_size], "seed": 1}, SAMPLED[1]]
    got = _serve(srv, reqs)
    assert len(calls) == 1
    for g in got[1:6]:
        assert "error" in g and "tokens" not in g, g
    assert len(got[0]["tokens"]) == 12 and len(got[6]["tokens"]) == 5
    calls.clear()
    # a valid batch whose longest prompt and longest continuation do not fit together is
    # split, not refused
    a = {"tokens": [2] * (n_pos - 4), "max_new_tokens": 4, "temperature": 0.9, "seed": 8}
    b = {"tokens": [6, 5], "max_new_tokens": 30, "temperature": 0.9, "seed": 8}
    got = _serve(srv, [a, b])
    assert len(calls) == 2
    assert len(got[0]["tokens"]) == 4 and len(got[1]["tokens"]) == 30
    alone = srv.model.generate(torch.tensor([b["tokens"]]), 30, temperature=0.9, seeds=8)
    assert got[1]["tokens"] == alone[0].tolist()


def test_serve_all_greedy_batch_is_the_scalar_path(server):
    srv, calls = server
    torch.manual_seed(SEED)
    model = GPT2(CFG).eval()
    expected = [model.generate(torch.tensor([r["tokens"]]), r["max_new_tokens"])[0].tolist()
                for r in REQUESTS]
    assert srv._run(REQUESTS) == expected
    calls.clear()
    got = _serve(srv, REQUESTS)
    assert got == [{"tokens": e} for e in expected]
    assert len(calls) == 1 and calls[0].get("seeds") is None
