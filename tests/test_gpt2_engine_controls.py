"""``GPT2Engine(logit_processors=True)`` on the CPU (``graph=False``): every request's tokens,
and its logprobs, are those of ``generate(..., seeds=[seed], <same controls>)`` on it alone,
cut after the first EOS: each request with other controls, neutral ones among them, through
slot reuse, a prefix, chunked prefill, an adapter, ``cancel`` and speculative steps whose
drafter is always right or always wrong. Off (the default), the engine rejects the fields
and allocates nothing."""

import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.models.lora import LoRAStack

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, logprobs, controls)
MIX = [
    (5, 14, 0.0, None, None, 3, 2, dict(repetition_penalty=1.3, frequency_penalty=0.5)),
    (1, 9, 0.9, 20, None, 11, None, dict()),
    (12, 16, 1.2, None, 0.9, 2, 2, dict(min_new_tokens=10, presence_penalty=0.6)),
    (30, 4, 0.0, None, None, 7, 0, dict(logit_bias={5: 4.0, 9: float("-inf"), 300: -2.0})),
    (8, 12, 0.0, None, None, 5, 2, dict(repetition_penalty=1.0, presence_penalty=0.0)),
    (3, 11, 0.7, 50, None, -4, 1, dict(repetition_penalty=0.8, min_new_tokens=11,
                                       logit_bias={i: 0.25 * i for i in range(64)})),
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
    return [torch.randint(0, CFG.vocab_size, (m[0],), generator=g).tolist() for m in MIX]


@pytest.fixture(scope="module")
def stack():
    """Two random adapters, strong enough to change the tokens."""
    g = torch.Generator().manual_seed(8)
    stack = LoRAStack(CFG, 2, 16, torch.device("cpu"), torch.float32)
    for t in list(stack.a.values()) + list(stack.b.values()):
        t.copy_(torch.randn(t.shape, generator=g) * 0.3)
    stack.scale.fill_(1.0)
    return stack


@pytest.fixture(scope="module")
def eos(model, prompts):
    """A token that some requests emit early when nothing holds it back."""
    out = model.generate(torch.tensor([prompts[2]]), 6, temperature=1.2, top_p=0.9, seeds=[2])
    return int(out[0, 3])


def _alone(model, stack, prompts, eos, adapters=False):
    res = []
    for i, (p, m) in enumerate(zip(prompts, MIX)):
        ad = {}
        if adapters:
            model.attach_lora(stack)
            ad = {"adapters": [ADAPTER.get(i, -1)]}
        try:
            got = model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3],
                                 top_p=m[4], seeds=[m[5]], eos_token_id=eos,
                                 logprobs=2 if m[6] is None else m[6], **ad, **m[7])
        finally:
            model.attach_lora(None)
        toks = got[0][0].tolist()
        n = toks.index(eos) + 1 if eos in toks else len(toks)
        res.append(tuple(t[0, :n] for t in got))
    return res


@pytest.fixture(scope="module")
def expected(model, stack, prompts, eos):
    return _alone(model, stack, prompts, eos)


def _run(eng, prompts, order=None, pids=None, adapters=False, controls=True):
    rid_of = {}
    for i in (order or range(len(MIX))):
        m = MIX[i]
        toks, pid = prompts[i], None
        if pids and i in pids:
            toks, pid = prompts[i][PREFIXED[i]:], pids[i]
        rid_of[eng.submit(toks, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                          prefix=pid, logprobs=m[6],
                          adapter=ADAPTER.get(i) if adapters else None,
                          **(m[7] if controls else {}))] = i
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
            assert (torch.tensor(info["top_logprobs"]) - etlp[:, :m]).abs().max().item() < TOL


def test_expectations_are_worth_checking(model, prompts, expected, eos):
    """The controls change what the requests emit, EOS cuts some of them, and the bans hold."""
    bare = [model.generate(torch.tensor([p]), m[1], temperature=m[2], top_k=m[3], top_p=m[4],
                           seeds=[m[5]], eos_token_id=eos)[0].tolist()
            for p, m in zip(prompts, MIX)]
    cut = [b[: b.index(eos) + 1] if eos in b else b for b in bare]
    differ = [e[0].tolist() != c for e, c in zip(expected, cut)]
    assert differ[0] and differ[2] and not differ[1] and not differ[4]
    assert any(len(c) < m[1] for c, m in zip(cut, MIX))
    assert eos not in expected[2][0][:10].tolist() and len(expected[5][0]) == 11
    assert 9 not in expected[3][0].tolist()


@pytest.mark.parametrize("slots", [1, 2, 6])
def test_engine_equals_generate_alone(model, prompts, expected, eos, slots):
    """One slot: every request reuses it, after a request with other controls."""
    eng = GPT2Engine(model, slots=slots, eos_token_id=eos, poll_every=3, graph=False,
                     logprobs=2, logit_processors=True)
    _check(_run(eng, prompts), expected)
    _check(_run(eng, prompts, order=[5, 4, 3, 2, 1, 0]), expected)  # the slots' tables are stale


@pytest.mark.parametrize("speculate,drafter", [(0, None), (2, "right"), (2, "wrong"),
                                               (4, "right"), (4, "wrong"), (4, None)])
def test_with_prefix_chunks_and_speculation(model, prompts, expected, eos, speculate, drafter):
    sequences = [p + e[0].tolist() for p, e in zip(prompts, expected)]
    hook = None if drafter is None else _Drafter(sequences, speculate, CFG.n_positions,
                                                 CFG.vocab_size, drafter == "wrong")
    eng = GPT2Engine(model, slots=3, eos_token_id=eos, poll_every=2, graph=False, prefix_slots=2,
                     prefill_chunk=3, speculate=speculate, drafter=hook, logprobs=2,
                     logit_processors=True)
    pids = {i: eng.add_prefix(prompts[i][:n]) for i, n in PREFIXED.items()}
    _check(_run(eng, prompts, pids=pids), expected)
    if drafter is not None:
        stats = eng.spec_stats()
        assert stats["drafted"] > 0
        if drafter == "wrong":
            assert stats["accepted"] == 0
        else:  # everything but the drafts past an EOS or the end
            assert stats["accepted"] > stats["drafted"] // 2


def test_with_adapters(model, stack, prompts, eos):
    want = _alone(model, stack, prompts, eos, adapters=True)
    bare = _alone(model, stack, prompts, eos)
    assert any(w[0].tolist() != b[0].tolist() for w, b in zip(want, bare))
    eng = GPT2Engine(model, slots=2, eos_token_id=eos, graph=False, lora=stack, logprobs=2,
                     logit_processors=True)
    try:
        _check(_run(eng, prompts, adapters=True), want)
    finally:
        model.attach_lora(None)


def test_cancel_and_reuse(model, prompts, expected, eos):
    eng = GPT2Engine(model, slots=1, eos_token_id=eos, poll_every=2, graph=False, logprobs=2,
                     logit_processors=True)
    m = MIX[5]
    first = eng.submit(prompts[5], m[1], temperature=m[2], top_k=m[3], seed=m[5], **m[7])
    eng.step()
    assert eng.cancel(first)
    got = _run(eng, prompts, order=[0, 4])  # they take over the slot and its tables
    _check(got, expected, only=[0, 4])


def test_off_by_default(model, prompts):
    eng = GPT2Engine(model, slots=2, graph=False, eos_token_id=7)
    assert eng.ctl is None
    assert not any(hasattr(eng, n) for n in ("_ctl_rows", "_ctl_idx", "_ctl_n_extra"))
    for kw in (dict(repetition_penalty=1.0), dict(presence_penalty=0.0),
               dict(frequency_penalty=0.1), dict(logit_bias={}), dict(min_new_tokens=0)):
        with pytest.raises(ValueError, match="logit_processors=True"):
            eng.submit(prompts[0], 4, **kw)
    assert not eng.has_work()
    on = GPT2Engine(model, slots=2, graph=False, eos_token_id=7, logit_processors=True)
    assert on.ctl.prompt.shape == (2, CFG.n_positions) and on.ctl.bias_ids.shape == (2, 64)
    for kw in (dict(repetition_penalty=0.0), dict(frequency_penalty=float("nan")),
               dict(logit_bias={512: 1.0}), dict(logit_bias={i: 1.0 for i in range(65)}),
               dict(min_new_tokens=5), dict(min_new_tokens=-1), dict(logit_bias=[1])):
        with pytest.raises(ValueError):
            on.submit(prompts[0], 4, **kw)
    assert not on.has_work()
    with pytest.raises(ValueError, match="eos_token_id"):
        GPT2Engine(model, slots=1, graph=False, logit_processors=True).submit(
            prompts[0], 4, min_new_tokens=2)


class _Drafter:
    """A drafter that knows the answers (test_token_logprobs.py's ``Oracle``): it finds each
    slot's sequence by matching ``hist[:p] + tok0`` and proposes the true continuation, or,
    ``wrong``, that continuation with every token off by one."""

    def __init__(self, sequences, k, cap, vocab, wrong):
        self.k, self.vocab, self.wrong = k, vocab, wrong
        full = torch.full((len(sequences), cap + k + 1), -1, dtype=torch.int64)
        for r, seq in enumerate(sequences):
            full[r, : len(seq)] = torch.tensor(seq)
        self.full = full
        self.pos = torch.arange(cap)
        self.ahead = torch.arange(1, k + 1)

    def __call__(self, tok0, hist, lens, n_out, max_new, active):
        S, cap = hist.shape
        ok = (active != 0) & (lens >= 0) & (lens < cap)
        p = lens.long().clamp(0, cap - 1)
        seq = hist.long().scatter(1, p.unsqueeze(1), tok0.unsqueeze(1))
        same = (seq.unsqueeze(1) == self.full[:, :cap].unsqueeze(0)) | \
            (self.pos.view(1, 1, cap) > p.view(S, 1, 1))
        known = same.all(-1)  # [S, R]
        drafts = self.full[known.long().argmax(1)].gather(1, p.unsqueeze(1) + self.ahead)
        if self.wrong:
            drafts = (drafts + 1) % self.vocab
        room = torch.minimum(max_new - n_out, cap - lens)
        nd = torch.where(known.any(1), (room - 1).clamp(0, self.k), torch.zeros_like(room))
        n_win = torch.where(ok, 1 + nd, torch.zeros_like(nd)).to(torch.int32)
        return torch.cat([tok0.unsqueeze(1), drafts], 1), n_win
