"""``GPT2Engine(grammar_states=N)`` on the CPU (``graph=False``): every request's tokens, and
its logprobs, are those of ``generate(..., seeds=[seed], grammar=dfa, <same controls>)`` on it
alone, cut after the first EOS, through slot reuse, a prefix, chunked prefill, an adapter,
``cancel`` of a neighbour, every ``poll_every`` and speculative steps whose drafter is right,
wrong, or proposes tokens the grammar forbids; every constrained output is a word of its
grammar; the pool's bookkeeping; off (the default), the engine rejects the field and
allocates nothing."""

import dataclasses

import numpy as np
import pytest
import torch
from test_gpt2_engine_controls import _Drafter

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.models.grammar import TokenDFA
from ray_amd.models.lora import LoRAStack
from ray_amd.ops import functional as rf

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
V, EOS = CFG.vocab_size, 7
VOCAB = [bytes([i]) for i in range(256)] + [bytes([97 + i % 26, 97 + i // 26 % 26])
                                            for i in range(V - 256)]
# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, logprobs, grammar, controls)
MIX = [
    (5, 14, 0.0, None, None, 3, 2, "words", dict(repetition_penalty=1.3, frequency_penalty=0.5)),
    (1, 9, 0.9, 20, None, 11, None, None, dict()),
    (12, 16, 1.2, None, 0.9, 2, 2, "codes", dict()),
    (30, 6, 0.0, None, None, 7, 0, "choices", dict(logit_bias={5: 4.0, 300: -2.0})),
    (8, 12, 0.0, None, None, 5, 2, None, dict(presence_penalty=0.4)),
    (3, 11, 0.7, 50, None, -4, 1, "words", dict()),
    (9, 13, 1.0, None, None, 8, 2, "choices", dict()),
]
PREFIXED = {2: 5, 3: 17}  # request -> how much of its prompt is a registered prefix
ADAPTER = {0: 0, 4: 1}    # request -> its adapter
TOL = 1e-3  # fp32 summation order against a wrong position (as in test_token_logprobs.py)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(4)
    return GPT2(CFG).eval()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(6)
    return [torch.randint(0, V, (m[0],), generator=g).tolist() for m in MIX]


@pytest.fixture(scope="module")
def grammars():
    return {"choices": TokenDFA.from_choices([[3, 4, 5], [3, 4], [400, 9, 9, 9, 2], [11],
                                              [400, 9, 300]], V, EOS),
            "words": TokenDFA.from_regex(r"([a-z]{1,4} ){2,4}[a-z]{1,6}\.", VOCAB, EOS),
            "codes": TokenDFA.from_regex(r"\d{3}-\d{4}|[A-F0-9]{6,12}", VOCAB, EOS)}


@pytest.fixture(scope="module")
def stack():
    g = torch.Generator().manual_seed(8)
    stack = LoRAStack(CFG, 2, 16, torch.device("cpu"), torch.float32)
    for t in list(stack.a.values()) + list(stack.b.values()):
        t.copy_(torch.randn(t.shape, generator=g) * 0.3)
    stack.scale.fill_(1.0)
    return stack


def _alone(model, stack, prompts, grammars, adapters=False):
    res = []
    for i, (p, m) in enumerate(zip(prompts, MIX)):
        ad = {}
        if adapters:
            model.attach_lora(stack)
            ad = {"adapters": [ADAPTER.get(i, -1)]}
        gr = {} if m[7] is None else {"grammar": grammars[m[7]]}
        try:
            got = model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3],
                                 top_p=m[4], seeds=[m[5]], eos_token_id=EOS,
                                 logprobs=2 if m[6] is None else m[6], **ad, **gr, **m[8])
        finally:
            model.attach_lora(None)
        toks = got[0][0].tolist()
        n = toks.index(EOS) + 1 if EOS in toks else len(toks)
        res.append(tuple(t[0, :n] for t in got))
    return res


@pytest.fixture(scope="module")
def expected(model, stack, prompts, grammars):
    return _alone(model, stack, prompts, grammars)


def _engine(model, grammars, **kw):
    kw.setdefault("grammar_states", sum(d.n_states for d in grammars.values()))
    eng = GPT2Engine(model, eos_token_id=EOS, graph=False, logprobs=2, logit_processors=True,
                     **kw)
    return eng, {name: eng.add_grammar(d) for name, d in grammars.items()}


def _submit(eng, gids, prompts, i, pids=None, adapters=False):
    m = MIX[i]
    toks, pid = prompts[i], None
    if pids and i in pids:
        toks, pid = prompts[i][PREFIXED[i]:], pids[i]
    return eng.submit(toks, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                      prefix=pid, logprobs=m[6], adapter=ADAPTER.get(i) if adapters else None,
                      grammar=None if m[7] is None else gids[m[7]], **m[8])


def _run(eng, gids, prompts, order=None, pids=None, adapters=False):
    rid_of = {_submit(eng, gids, prompts, i, pids, adapters): i
              for i in (order or range(len(MIX)))}
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
            # (-inf entries, the forbidden tokens of a short allowed set, are equal)
            d = torch.tensor(info["top_logprobs"]) - etlp[:, :m]
            assert d.nan_to_num(0.0).abs().max().item() < TOL
            assert torch.equal(torch.tensor(info["top_logprobs"]).isinf(), etlp[:, :m].isinf())


def test_expectations_are_worth_checking(model, prompts, grammars, expected):
    """Every constrained output is a word of its grammar or a cut prefix, differs from the
    unconstrained one, and some words finish inside ``max_new_tokens``."""
    finished = 0
    for p, m, e in zip(prompts, MIX, expected):
        bare = model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3], top_p=m[4],
                              seeds=[m[5]], eos_token_id=EOS, **m[8])[0].tolist()
        toks = e[0].tolist()
        if m[7] is None:
            assert toks == (bare[: bare.index(EOS) + 1] if EOS in bare else bare)
            continue
        dfa = grammars[m[7]]
        assert toks != bare[: len(toks)]
        if toks[-1] == EOS:
            finished += 1
            assert dfa.accepts(toks)
        else:
            assert len(toks) == m[1] and dfa.walk(toks) >= 0
    assert finished >= 3


@pytest.mark.parametrize("slots,poll_every", [(1, 8), (2, 1), (7, 8), (3, 1)])
def test_engine_equals_generate_alone(model, prompts, grammars, expected, slots, poll_every):
    """One slot: every request reuses it, after a request with another grammar or none."""
    eng, gids = _engine(model, grammars, slots=slots, poll_every=poll_every)
    _check(_run(eng, gids, prompts), expected)
    _check(_run(eng, gids, prompts, order=[6, 5, 4, 3, 2, 1, 0]), expected)  # stale states


@pytest.mark.parametrize("speculate,drafter", [(0, None), (2, "right"), (2, "wrong"),
                                               (4, "right"), (4, "wrong"), (4, None)])
def test_with_prefix_chunks_and_speculation(model, prompts, grammars, expected, speculate,
                                            drafter):
    sequences = [p + e[0].tolist() for p, e in zip(prompts, expected)]
    hook = None if drafter is None else _Drafter(sequences, speculate, CFG.n_positions, V,
                                                 drafter == "wrong")
    eng, gids = _engine(model, grammars, slots=3, poll_every=2, prefix_slots=2, prefill_chunk=3,
                        speculate=speculate, drafter=hook)
    pids = {i: eng.add_prefix(prompts[i][:n]) for i, n in PREFIXED.items()}
    _check(_run(eng, gids, prompts, pids=pids), expected)
    if drafter is not None:
        stats = eng.spec_stats()
        assert stats["drafted"] > 0
        if drafter == "wrong":
            assert stats["accepted"] == 0
        else:  # everything but the drafts past an EOS or the end
            assert stats["accepted"] > stats["drafted"] // 2


class _ForbiddenDrafter:
    """Proposes, for every slot, k tokens that the slot's grammar forbids at the first
    drafted position (it follows each slot's automaton on the host-side copy of the table);
    a slot without a grammar gets token 0."""

    def __init__(self, eng, k):
        self.eng, self.k = eng, k

    def __call__(self, tok0, hist, lens, n_out, max_new, active):
        eng, S = self.eng, tok0.shape[0]
        drafts = torch.zeros(S, self.k, dtype=torch.int64)
        for s in range(S):
            q = int(eng.gstate[s])
            if not active[s] or q < 0:
                continue
            q = int(eng.gtable[q, int(tok0[s])])  # tok0 came from masked logits: allowed
            assert q >= 0
            banned = np.flatnonzero(eng.gtable[q, :V].numpy() < 0)
            drafts[s] = int(banned[(s + int(n_out[s])) % len(banned)])
        room = torch.minimum(max_new - n_out, hist.shape[1] - lens)
        n_win = torch.where(active != 0, 1 + (room - 1).clamp(0, self.k),
                            torch.zeros_like(room)).to(torch.int32)
        return torch.cat([tok0.unsqueeze(1), drafts], 1), n_win


@pytest.mark.parametrize("speculate", [2, 4])
def test_forbidden_drafts_are_never_emitted(model, prompts, grammars, expected, speculate):
    eng, gids = _engine(model, grammars, slots=3, poll_every=2, speculate=speculate)
    eng._drafter = _ForbiddenDrafter(eng, speculate)
    constrained = [i for i, m in enumerate(MIX) if m[7] is not None]
    got = _run(eng, gids, prompts, order=constrained)
    _check(got, expected, only=constrained)
    stats = eng.spec_stats()
    assert stats["drafted"] > 0 and stats["accepted"] == 0


def test_with_adapters(model, stack, prompts, grammars):
    want = _alone(model, stack, prompts, grammars, adapters=True)
    bare = _alone(model, stack, prompts, grammars)
    assert any(w[0].tolist() != b[0].tolist() for w, b in zip(want, bare))
    eng, gids = _engine(model, grammars, slots=2, lora=stack)
    try:
        _check(_run(eng, gids, prompts, adapters=True), want)
    finally:
        model.attach_lora(None)


def test_cancel_of_a_neighbour_and_reuse(model, prompts, grammars, expected):
    eng, gids = _engine(model, grammars, slots=2, poll_every=2)
    first = _submit(eng, gids, prompts, 5)
    rid_of = {_submit(eng, gids, prompts, 0): 0}
    got = {0: ([], {"logprobs": [], "top_ids": [], "top_logprobs": []})}
    events = eng.step()  # both are running, each in its slot
    assert {ev[0] for ev in events} == {first, *rid_of}
    assert eng.cancel(first)
    rid_of.update({_submit(eng, gids, prompts, i): i for i in (2, 4, 6)})  # take its slot over
    while eng.has_work() or events:
        for rid, new, _, info in events:
            if rid != first:
                toks, acc = got.setdefault(rid_of[rid], ([], {k: [] for k in info}))
                toks.extend(new)
                for k, v in info.items():
                    acc[k].extend(v)
        events = eng.step() if eng.has_work() else []
    _check(got, expected, only=[0, 2, 4, 6])


def test_the_pool(model, grammars):
    words, codes, choices = grammars["words"], grammars["codes"], grammars["choices"]
    n = words.n_states + codes.n_states
    eng = GPT2Engine(model, slots=2, eos_token_id=EOS, graph=False, grammar_states=n)
    assert eng.gtable.shape == (n, 512) and eng.gtable.dtype == torch.int16
    assert eng.grammar_free == n
    a, b = eng.add_grammar(words), eng.add_grammar(codes)
    assert eng.grammar_free == 0
    before = eng.gtable.clone()
    with pytest.raises(ValueError, match="pool is full"):
        eng.add_grammar(choices)
    assert torch.equal(eng.gtable, before) and eng.grammar_free == 0
    rid = eng.submit([1, 2, 3], 20, grammar=a)
    with pytest.raises(ValueError, match="in use"):
        eng.drop_grammar(a)  # queued
    head = [t for ev in eng.step() if ev[0] == rid for t in ev[1]]
    with pytest.raises(ValueError, match="in use"):
        eng.drop_grammar(a)  # running
    eng.drop_grammar(b)
    assert eng.grammar_free == codes.n_states
    ptr = eng.gtable.data_ptr()
    c = eng.add_grammar(choices)  # first fit: the freed rows, in place
    assert eng.gtable.data_ptr() == ptr and eng._graph is None
    first = words.n_states
    assert torch.equal(eng.gtable[first: first + choices.n_states],
                       torch.from_numpy(choices.table(first)))
    assert torch.equal(eng.gtable[:first], before[:first])
    rid2 = eng.submit([4, 5], 8, grammar=c, temperature=1.0, seed=3)
    got = eng.run()
    assert words.walk(head + got[rid]) >= 0 and choices.accepts(got[rid2])
    eng.drop_grammar(a), eng.drop_grammar(c)
    assert eng.grammar_free == n and eng._gfree == [(0, n)]  # the ranges merged again
    for bad in (a, 99, None, True):
        with pytest.raises(ValueError, match="unknown grammar"):
            eng.drop_grammar(bad)
    with pytest.raises(ValueError, match="unknown grammar"):
        eng.submit([1], 4, grammar=a)
    with pytest.raises(ValueError, match="TokenDFA"):
        eng.add_grammar("words")
    with pytest.raises(ValueError, match="EOS"):
        eng.add_grammar(TokenDFA.from_choices([[1]], V, 9))
    assert not eng.has_work()


def test_off_by_default_and_rejections(model, prompts, grammars):
    eng = GPT2Engine(model, slots=2, graph=False, eos_token_id=EOS)
    assert not any(hasattr(eng, n) for n in ("gtable", "gstate", "gpos", "_grammars", "_gfree",
                                              "_g_rows", "_g_idx", "_g_n_extra"))
    with pytest.raises(ValueError, match="grammar_states="):
        eng.submit(prompts[0], 4, grammar=0)
    with pytest.raises(ValueError, match="grammar_states="):
        eng.add_grammar(grammars["choices"])
    assert not eng.has_work()
    with pytest.raises(ValueError, match="eos_token_id"):
        GPT2Engine(model, slots=1, graph=False, grammar_states=8)
    for bad in (-1, 32768, True, 2.5):
        with pytest.raises(ValueError, match="grammar_states"):
            GPT2Engine(model, slots=1, graph=False, eos_token_id=EOS, grammar_states=bad)
    on, gids = _engine(model, grammars, slots=2)
    with pytest.raises(ValueError, match="min_new_tokens"):
        on.submit(prompts[0], 8, grammar=gids["words"], min_new_tokens=2)
    with pytest.raises(ValueError, match="-inf"):
        on.submit(prompts[0], 8, grammar=gids["words"], logit_bias={3: float("-inf")})
    on.submit(prompts[0], 8, grammar=gids["words"], min_new_tokens=0, logit_bias={3: -1.0})
    on.submit(prompts[0], 8, min_new_tokens=2, logit_bias={3: float("-inf")})  # no grammar: fine
    assert on.num_queued == 2


def test_a_request_without_a_grammar_is_untouched(model, prompts, expected, grammars):
    """The engine with the pool but no request using it, and without the pool: the same
    tokens and the same number of device steps."""
    plain = [i for i, m in enumerate(MIX) if m[7] is None]
    res = []
    for states in (0, 40):
        eng = GPT2Engine(model, slots=2, eos_token_id=EOS, graph=False, logprobs=2,
                         logit_processors=True, grammar_states=states)
        rids = [eng.submit(prompts[i], MIX[i][1], temperature=MIX[i][2], top_k=MIX[i][3],
                           top_p=MIX[i][4], seed=MIX[i][5], **MIX[i][8]) for i in plain]
        got = eng.run()
        res.append(([got[r] for r in rids], eng.steps))
    assert res[0] == res[1]
    for toks, i in zip(res[0][0], plain):
        assert toks == expected[i][0].tolist()
    assert rf.GRAMMAR_NONE == -1 and rf.GRAMMAR_DEAD == -2
