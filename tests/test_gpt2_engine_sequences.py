"""``GPT2Engine(sequence_rules=True)`` on the CPU (``graph=False``): every request's tokens, and
its logprobs, are those of ``generate(..., seeds=[seed], <same rules>)`` on it alone, cut after
the first EOS or the first completed stop sequence, through slot reuse, a prefix, chunked
prefill, ``cancel`` of a neighbour, logit processors, a grammar with ``stop``, every
``poll_every`` and speculative steps whose drafter is right or wrong; a stop in the middle of an
accepted window whose later token is EOS cuts the window; off (the default), the engine
rejects the fields, allocates nothing and does what it did."""

import dataclasses

import pytest
import torch
from test_gpt2_engine_controls import _Drafter
from test_gpt2_generate_sequences import cut, violations

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.models.grammar import TokenDFA

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
V, EOS = CFG.vocab_size, 7
# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, logprobs, bans, controls);
# prompt + max_new_tokens + SEQ_MAX < 512: a row always has an unbanned token
MIX = [
    (5, 14, 0.0, None, None, 3, 2, dict(no_repeat_ngram_size=2), dict()),
    (1, 9, 0.9, 20, None, 11, None, dict(), dict()),
    (12, 16, 1.2, None, 0.9, 2, 2, dict(no_repeat_ngram_size=1, bad_words=[[3], [4, 5]]),
     dict(repetition_penalty=1.3)),
    (30, 6, 0.0, None, None, 7, 0, dict(bad_words=[9, [1, 2, 3]]), dict()),
    (8, 12, 0.0, None, None, 5, 2, dict(), dict(presence_penalty=0.4)),
    (3, 11, 0.7, 50, None, -4, 1, dict(no_repeat_ngram_size=3), dict()),
    (9, 13, 0.0, None, None, 8, 2, dict(no_repeat_ngram_size=8), dict(logit_bias={EOS: 3.0})),
]
STOPPED = {0: (5, 2), 2: (7, 1), 4: (6, 3), 6: (4, 8)}  # request -> (the stop's end, its length)
PREFIXED = {2: 5, 3: 17}  # request -> how much of its prompt is a registered prefix
TOL = 1e-3  # fp32 summation order against a wrong position (as in test_token_logprobs.py)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(4)
    return GPT2(CFG).eval()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(6)
    return [torch.randint(0, V, (m[0],), generator=g).tolist() for m in MIX]


def _generate(model, p, m, **rules):
    return model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3], top_p=m[4],
                          seeds=[m[5]], eos_token_id=EOS, logprobs=2 if m[6] is None else m[6],
                          **rules, **m[8])


@pytest.fixture(scope="module")
def rules(model, prompts):
    """Every request's rules: its bans, and a stop sequence taken from its own run under them
    (so that it acts), beside one that never occurs."""
    res = []
    for i, (p, m) in enumerate(zip(prompts, MIX)):
        r = dict(m[7])
        if i in (0, 3, 5):  # what the request does without a rule is banned: the bans act
            bare = _generate(model, p, m)[0][0].tolist()
            r["bad_words"] = list(r.get("bad_words", [])) + [[bare[0]], [p[-1], bare[0]]]
        if i in STOPPED:
            end, n = STOPPED[i]
            toks = _generate(model, p, m, **r)[0][0].tolist()
            r["stop"] = [[500, 501], (p + toks)[len(p) + end - n: len(p) + end][-min(n, end):]]
        res.append(r)
    return res


@pytest.fixture(scope="module")
def expected(model, prompts, rules):
    res = []
    for p, m, r in zip(prompts, MIX, rules):
        got = _generate(model, p, m, **r)
        n = len(cut(got[0][0].tolist(), r.get("stop", ())))
        res.append(tuple(t[0, :n] for t in got))
    return res


def _engine(model, **kw):
    return GPT2Engine(model, eos_token_id=EOS, graph=False, logprobs=2, logit_processors=True,
                      sequence_rules=True, **kw)


def _submit(eng, prompts, rules, i, pids=None):
    m = MIX[i]
    toks, pid = prompts[i], None
    if pids and i in pids:
        toks, pid = prompts[i][PREFIXED[i]:], pids[i]
    return eng.submit(toks, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                      prefix=pid, logprobs=m[6], **rules[i], **m[8])


def _run(eng, prompts, rules, order=None, pids=None):
    rid_of = {_submit(eng, prompts, rules, i, pids): i for i in (order or range(len(MIX)))}
    return {rid_of[r]: v for r, v in eng.run(logprobs=True).items()}


def _check(got, expected, only=None):
    for i in (only or range(len(MIX))):
        toks, info = got[i]
        etoks, elp, eids, etlp = expected[i]
        assert toks == etoks.tolist(), i
        m = MIX[i][6]
        if m is None:
            assert info is None
            continue
        assert (torch.tensor(info["logprobs"]) - elp).abs().max().item() < TOL, i
        if m:
            assert info["top_ids"] == eids[:, :m].tolist(), i
            d = torch.tensor(info["top_logprobs"]) - etlp[:, :m]
            assert d.nan_to_num(0.0).abs().max().item() < TOL


def test_expectations_are_worth_checking(model, prompts, rules, expected):
    cuts = 0
    for i, (p, m, r, e) in enumerate(zip(prompts, MIX, rules, expected)):
        toks = e[0].tolist()
        assert violations(p, toks, r.get("bad_words", ()),
                          r.get("no_repeat_ngram_size", 0)) == []
        bare = _generate(model, p, m)[0][0].tolist()
        if not r:
            assert toks == cut(bare)
        if i in STOPPED and toks[-1] != EOS:
            cuts += 1
            assert len(toks) <= STOPPED[i][0] < m[1]
            assert any(toks[-len(s):] == s for s in r["stop"])
    assert cuts >= 3
    assert sum(e[0].tolist() != cut(_generate(model, p, m)[0][0].tolist())[: len(e[0])]
               for p, m, e in zip(prompts, MIX, expected)) >= 3  # the bans act


@pytest.mark.parametrize("slots,poll_every", [(1, 8), (2, 1), (7, 8), (3, 1)])
def test_engine_equals_generate_alone(model, prompts, rules, expected, slots, poll_every):
    """One slot: every request reuses it, after a request with other rules or none."""
    eng = _engine(model, slots=slots, poll_every=poll_every)
    _check(_run(eng, prompts, rules), expected)
    _check(_run(eng, prompts, rules, order=[6, 5, 4, 3, 2, 1, 0]), expected)  # stale tables
    hits = eng.seq.hit.tolist()
    assert all(-1 <= h <= 1 for h in hits) and (slots > 1 or hits == [1])


@pytest.mark.parametrize("speculate,drafter,poll_every", [
    (0, None, 8), (2, "right", 1), (2, "wrong", 8), (4, "right", 8), (4, "wrong", 1),
    (4, None, 8)])
def test_with_prefix_chunks_and_speculation(model, prompts, rules, expected, speculate, drafter,
                                            poll_every):
    # the drafter proposes the UNCUT run: what the sampler would go on to draw past the stop
    sequences = [p + _generate(model, p, m, **{k: v for k, v in r.items() if k != "stop"})[0][0]
                 .tolist() for p, m, r in zip(prompts, MIX, rules)]
    hook = None if drafter is None else _Drafter(sequences, speculate, CFG.n_positions, V,
                                                 drafter == "wrong")
    eng = _engine(model, slots=3, poll_every=poll_every, prefix_slots=2, prefill_chunk=3,
                  speculate=speculate, drafter=hook)
    pids = {i: eng.add_prefix(prompts[i][:n]) for i, n in PREFIXED.items()}
    _check(_run(eng, prompts, rules, pids=pids), expected)
    if drafter is not None:
        stats = eng.spec_stats()
        assert stats["drafted"] > 0
        assert (stats["accepted"] == 0) == (drafter == "wrong")


def test_a_stop_inside_an_accepted_window_before_its_eos(model, prompts):
    """Request 6 is biased towards EOS. Its uncut run is searched for an EOS at output index k
    whose window (k + 1 tokens per step, all accepted from a drafter that knows the run) also
    holds index k - 2; the stop is that token: ``spec_accept`` retires the slot at the EOS,
    ``stop_check`` still cuts it two tokens earlier."""
    W, m = 5, MIX[6]
    for seed in range(64):
        mm = m[:2] + (1.0,) + m[3:5] + (seed,) + m[6:8] + (dict(logit_bias={EOS: 4.0}),)
        toks = _generate(model, prompts[6], mm)[0][0].tolist()
        k = toks.index(EOS) if EOS in toks else -1
        if k >= 2 and (k - 2) // W == k // W and toks[k - 2] not in toks[: k - 2]:
            break
    else:
        pytest.fail("no seed puts an EOS where the case needs it")
    stop = [[toks[k - 2]]]
    want = _generate(model, prompts[6], mm, stop=stop)
    assert want[0][0].tolist() == toks[: k - 1] + [EOS] * (m[1] - k + 1)
    hook = _Drafter([prompts[6] + toks], W - 1, CFG.n_positions, V, False)
    eng = _engine(model, slots=2, poll_every=1, speculate=W - 1, drafter=hook)
    rid = eng.submit(prompts[6], m[1], temperature=1.0, seed=seed, logprobs=2, stop=stop,
                     logit_bias={EOS: 4.0})
    events = []
    while eng.has_work():
        events += eng.step()
    assert [e[0] for e in events] == [rid] * len(events) and events[-1][2]
    got = [t for e in events for t in e[1]]
    assert got == toks[: k - 1]
    lp = [x for e in events for x in e[3]["logprobs"]]
    assert (torch.tensor(lp) - want[1][0, : k - 1]).abs().max().item() < TOL
    # the whole window, the EOS included, was accepted; then it was cut
    assert eng.spec_stats()["accepted"] >= k - (k // W)
    assert eng.seq.hit.tolist().count(0) == 1 and eng.n_out.max().item() == k - 1
    assert len(events[-1][1]) == (k - 2) % W + 1


def test_cancel_of_a_neighbour(model, prompts, rules, expected):
    eng = _engine(model, slots=3, poll_every=1)
    rids = {i: _submit(eng, prompts, rules, i) for i in (0, 2, 5)}
    got = {i: [] for i in rids}
    for ev in eng.step():
        got[{v: k for k, v in rids.items()}[ev[0]]] += ev[1]
    assert eng.cancel(rids[2])
    rids[6] = _submit(eng, prompts, rules, 6)  # takes the cancelled request's slot
    got[6] = []
    while eng.has_work():
        for ev in eng.step():
            got[{v: k for k, v in rids.items()}[ev[0]]] += ev[1]
    for i in (0, 5, 6):
        assert got[i] == expected[i][0].tolist(), i


def test_a_grammar_with_stop(model):
    dfa = TokenDFA.from_choices([[3, 4, 5, 6, 9], [400, 9, 9, 9, 2]], V, EOS)
    p = [17, 4, 250]
    want = model.generate(torch.tensor([p]), 8, seeds=[1], eos_token_id=EOS, grammar=dfa,
                          stop=[[4, 5], [9, 9]])[0].tolist()
    assert len(cut(want, [[4, 5], [9, 9]])) == 3
    for speculate in (0, 2):
        eng = _engine(model, slots=2, grammar_states=dfa.n_states, speculate=speculate)
        gid = eng.add_grammar(dfa)
        rid = eng.submit(p, 8, seed=1, grammar=gid, stop=[[4, 5], [9, 9]])
        other = eng.submit(p, 8, seed=1, grammar=gid)
        got = eng.run()
        assert got[rid] == want[:3] and dfa.accepts(got[other])
        for kw in (dict(bad_words=[[1]]), dict(no_repeat_ngram_size=2)):
            with pytest.raises(ValueError, match="grammar"):
                eng.submit(p, 8, grammar=gid, **kw)
        eng.submit(p, 2, grammar=gid, no_repeat_ngram_size=0, bad_words=[])
        eng.run()


def test_off_by_default(model, prompts, rules):
    eng = GPT2Engine(model, slots=3, eos_token_id=EOS, graph=False, poll_every=2)
    assert not hasattr(eng, "seq")
    for kw in (dict(stop=[[1]]), dict(bad_words=[[1]]), dict(no_repeat_ngram_size=2)):
        with pytest.raises(ValueError, match="sequence_rules"):
            eng.submit(prompts[0], 4, **kw)
    assert eng.num_queued == 0
    on = GPT2Engine(model, slots=3, eos_token_id=EOS, graph=False, poll_every=2,
                    sequence_rules=True)
    res = []
    for e in (eng, on):
        rids = [e.submit(p, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5])
                for p, m in zip(prompts, MIX)]
        got = e.run()
        res.append(([got[r] for r in rids], e.steps))
    assert res[0] == res[1]  # on and unused: the same tokens in the same steps
    # a request that names no rule is untouched by its neighbours' rules
    rids = [on.submit(p, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                      **(rules[i] if i % 2 == 0 else {}))
            for i, (p, m) in enumerate(zip(prompts, MIX))]
    got = on.run()
    for i in (1, 3, 5):
        assert got[rids[i]] == res[0][0][i]


def test_rejections(model, prompts):
    eng = _engine(model, slots=2)
    for kw in (dict(stop=[[V]]), dict(stop=[[1]] * 9), dict(stop=[[]]), dict(bad_words=[[-1]]),
               dict(bad_words=[list(range(9))]), dict(no_repeat_ngram_size=9),
               dict(no_repeat_ngram_size=True), dict(no_repeat_ngram_size=-1), dict(stop=3),
               dict(bad_words=[[1.5]])):
        with pytest.raises(ValueError):
            eng.submit(prompts[0], 4, **kw)
    assert eng.num_queued == 0
    no_eos = GPT2Engine(model, slots=2, graph=False, sequence_rules=True)
    with pytest.raises(ValueError, match="eos_token_id"):
        no_eos.submit(prompts[0], 4, stop=[[1]])
    no_eos.submit(prompts[0], 4, bad_words=[[1]], no_repeat_ngram_size=2)
    assert len(no_eos.run()) == 1
