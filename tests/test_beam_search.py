"""Beam search on the CPU: ``ref.beam_step`` against a naive list implementation of its rules,
slot stability, ``GPT2.generate(num_beams=...)`` against greedy decoding and teacher-forced
scores, and the static Serve app with a mixed batch."""

import asyncio
import dataclasses

import numpy as np
import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.serve.llm import GPT2EngineServer, GPT2Server

EOS = 3
G = 2
STEPS = 4
CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)


def planted_logits(W, V, step):
    """Seeded fp64 logits [G * W, V] with what the rules must meet: a -inf column; at step 0 two
    equal top values in every row, so that two beams leave it with equal scores; afterwards
    two identical rows (with those scores: exact cross-beam ties) and, in group 0, an EOS
    column that is every row's second best, at step 2 its best (W = 1: at step 2 only)."""
    x = torch.randn(G * W, V, dtype=torch.float64, generator=torch.Generator().manual_seed(
        100 * W + V + step)) * 2
    x[:, 5] = float("-inf")
    x[:, EOS] = -30.0
    if step == 0:
        x[:, 7] = x[:, 9] = x.max(-1).values + 0.5
    elif W > 1:
        x[1] = x[0]
        x[:W, EOS] = x[:W].max(-1).values + (0.1 if step == 2 else -0.2)
    elif step == 2:
        x[:W, EOS] = x[:W].max(-1).values + 0.2
    return x


def naive_step(x, lp, st, ev):
    """The rules of ``ref.beam_step`` on Python lists; ``st``: score, hyp, n, done, t per
    group as lists; returns (tok, parent) and adds what the hypothesis table did to ``ev``."""
    W, K, V = st["W"], 2 * st["W"], len(x[0])
    tok, parent = [EOS] * (G * W), list(range(G * W))
    for g in range(G):
        if st["done"][g]:
            continue
        t, norm, hyp = st["t"][g], st["norm"], st["hyp"][g]
        cands = []
        for w in range(W):
            r = g * W + w
            top = sorted(range(V), key=lambda i: (-x[r][i], i))[:K]
            cands += [(np.float32(st["score"][r] + lp[r][i]), w, j, i) for j, i in enumerate(top)]
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        live = []
        for q, (val, w, _, i) in enumerate(cands[:K]):
            if i == EOS and q < W:
                ev.add("eos_low")
                new = (val / np.float32(norm[t + 1]), -len(st["all"][g]), t, g * W + w)
                st["all"][g].append(new)
                if len(hyp) == W:
                    ev.add("replace" if new[0] > min(hyp)[0] else "reject")
                    if new[0] > min(hyp)[0]:
                        hyp.remove(min(hyp))
                        hyp.append(new)
                else:
                    hyp.append(new)
            elif i == EOS:
                ev.add("eos_high")
            elif len(live) < W:
                live.append((val, w, i))
        free = [w for w in range(W) if w not in {c[1] for c in live}]
        taken = set()
        for val, w, i in live:
            s = w if w not in taken else free.pop(0)
            taken.add(w)
            tok[g * W + s], parent[g * W + s], st["score"][g * W + s] = i, g * W + w, val
        best = live[0][0] / np.float32(norm[t + 1])
        st["done"][g] = len(hyp) == W and (st["early"] or min(hyp)[0] >= best)
        st["t"][g] += 1
    return tok, parent


@pytest.mark.parametrize("penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("V", [17, 40])
@pytest.mark.parametrize("W", [1, 3, 8])
def test_reference_against_naive(W, V, early, penalty):
    st = ref.beam_state(G, W, STEPS, EOS, penalty, early)
    nv = {"W": W, "early": early, "norm": st["len_norm"].tolist(), "score": st["score"].tolist(),
          "hyp": [[] for _ in range(G)], "all": [[] for _ in range(G)], "done": [False] * G,
          "t": [0] * G}
    ev = set()
    for step in range(STEPS):
        x = planted_logits(W, V, step)
        m = x.max(-1, keepdim=True).values
        lp = (x - (m + torch.log(torch.exp(x - m).sum(-1, keepdim=True)))).to(torch.float32)
        before = list(nv["done"])
        tok, parent = naive_step(x.tolist(), lp.numpy(), nv, ev)
        ref.beam_step(x, st)
        assert st["tok"].tolist() == tok and st["parent"].tolist() == parent
        assert st["done"].tolist() == nv["done"]
        live = [r for r in range(G * W) if not before[r // W]]
        assert [st["score"][r].item() for r in live] == [nv["score"][r] for r in live]
        for g in range(G):
            n = min(int(st["hyp_n"][g]), W)
            got = {(st["hyp_score"][g, i].item(), st["hyp_step"][g, i].item(),
                    st["hyp_par"][g, i].item()) for i in range(n)}
            assert got == {(float(h[0]), h[2], h[3]) for h in nv["hyp"][g]}
        # slot stability: a surviving parent keeps its row, no row is both source and destination
        assert all(parent[p] == p for p in set(parent))
    assert "eos_low" in ev
    if W > 1:
        assert "eos_high" in ev
    if (W, V, early, penalty) == (8, 17, False, 0.0):
        assert {"reject", "replace"} <= ev  # a full table met a worse and a better hypothesis
    # the read-out: every group's best hypotheses, best first, as the naive tables hold them
    toks, scores, lens = ref.beam_backtrace(st, W)
    for g in range(G):
        if nv["done"][g]:
            want = sorted(nv["hyp"][g], key=lambda h: (-h[0], -h[1]))
            assert scores[g].tolist() == [float(h[0]) for h in want]
            assert lens[g].tolist() == [h[2] + 1 for h in want]
            assert all(toks[g, j, h[2]] == EOS for j, h in enumerate(want))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(11)
    return GPT2(CFG).eval()


@pytest.fixture(scope="module")
def prompts():
    return torch.randint(0, CFG.vocab_size, (2, 6), generator=torch.Generator().manual_seed(5))


def test_one_beam_is_greedy(model, prompts):
    greedy = model.generate(prompts, 10)
    eos = int(greedy[0, 4])  # a token that greedy decoding meets
    greedy = model.generate(prompts, 10, eos_token_id=eos)
    toks, scores, lens = model.generate(prompts, 10, eos_token_id=eos, num_beams=1,
                                        length_penalty=0.0)
    assert toks.shape == (2, 1, 10) and toks.dtype == torch.int64
    assert torch.equal(toks[:, 0], greedy)
    assert int(lens[0, 0]) == greedy[0].tolist().index(eos) + 1


@pytest.mark.parametrize("W", [2, 4])
def test_scores_are_teacher_forced(model, prompts, W):
    eos = int(model.generate(prompts, 10)[0, 4])
    toks, scores, lens = model.generate(prompts, 10, eos_token_id=eos, num_beams=W,
                                        length_penalty=1.0, num_return_sequences=W)
    assert toks.shape == (2, W, 10) and scores.dtype == torch.float32
    assert lens.dtype == torch.int32 and int(lens.min()) >= 1 and int(lens.min()) < 10
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    for b in range(2):
        for j in range(W):
            n = int(lens[b, j])
            full = torch.cat([prompts[b], toks[b, j, :n]])[None]
            lp = model.score(full)[0, prompts.shape[1]:].double().sum()
            assert abs(float(lp) / n - float(scores[b, j])) < 1e-4
            assert toks[b, j, n:].tolist() == [eos] * (10 - n)


def test_arguments(model, prompts):
    kw = dict(eos_token_id=EOS, num_beams=2)
    for bad in ({"seeds": 1}, {"temperature": 0.7}, {"top_k": 5}, {"top_p": 0.9},
                {"logprobs": 1}, {"repetition_penalty": 1.2}, {"logit_bias": {1: 1.0}},
                {"stop": [[4]]}, {"bad_words": [[4]]}, {"no_repeat_ngram_size": 2},
                {"generator": torch.Generator()}, {"num_beams": 9}, {"num_beams": 0},
                {"num_return_sequences": 3}, {"length_penalty": float("nan")},
                {"early_stopping": 1}, {"eos_token_id": None}):
        with pytest.raises(ValueError):
            model.generate(prompts, 4, **{**kw, **bad})
    # without num_beams the call is what it was: a tensor, the beam arguments unused
    plain = model.generate(prompts, 4, eos_token_id=EOS)
    assert torch.equal(plain, model.generate(prompts, 4, eos_token_id=EOS, length_penalty=2.0))
    with pytest.raises(ValueError):
        rf.beam_backtrace(rf.beam_state(1, 2, 4, EOS), 3)


def test_static_server_mixed_batch(model, prompts):
    eos = int(model.generate(prompts, 10)[0, 4])
    srv = GPT2Server(CFG, seed=11, device="cpu", eos_token_id=eos)
    p0, p1 = prompts[0].tolist(), prompts[1].tolist()[:4]
    beam = {"max_new_tokens": 10, "num_beams": 3, "num_return_sequences": 2}
    reqs = [dict(beam, tokens=p0), {"tokens": p0, "max_new_tokens": 5}, dict(beam, tokens=p1),
            dict(beam, tokens=p0, length_penalty=0.0, early_stopping=False),
            dict(beam, tokens=p0, temperature=0.5), dict(beam, tokens=p0, num_beams=9),
            {"tokens": p0, "length_penalty": 1.0}]

    async def calls():
        return await asyncio.gather(*(GPT2Server._generate_batch(srv, r) for r in reqs))

    got = asyncio.run(calls())
    for r, g in zip(reqs[:4], got[:4]):
        if "num_beams" not in r:
            assert g == {"tokens": model.generate(prompts[:1], 5)[0].tolist()}
            continue
        toks, scores, lens = model.generate(
            torch.tensor([r["tokens"]]), 10, eos_token_id=eos, num_beams=3,
            num_return_sequences=2, length_penalty=r.get("length_penalty", 1.0),
            early_stopping=r.get("early_stopping", True))
        want = [toks[0, j, : int(lens[0, j])].tolist() for j in range(2)]
        assert g["sequences"] == want and g["tokens"] == want[0]
        assert g["scores"] == pytest.approx(scores[0].tolist(), abs=1e-4)
    assert all("error" in g and "tokens" not in g for g in got[4:])
    # the continuous app answers a beam request with that request's error
    eng = GPT2EngineServer.__new__(GPT2EngineServer)  # the request is refused before the engine
    eng.cfg, eng._eos = CFG, eos
    chunks = GPT2EngineServer._chunks(eng, reqs[0])
    first = asyncio.run(chunks.__anext__())
    assert first[0] == "error" and "num_beams" in first[1]
