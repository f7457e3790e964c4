"""``GPT2.generate`` with the logit-processor controls (repetition / presence / frequency
penalties, logit bias, minimum length before EOS) on a tiny fp32 model on the CPU: the
tokens are those of a hand-written loop of ``prefill``, ``ref.logit_process``,
``ref.sample_logits`` and ``decode_step``; a row does not depend on its batch-mates; the
bans hold; the calls without ``seeds=`` raise; without controls nothing changes."""

import dataclasses

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache, checked_controls
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

CFG = dataclasses.replace(GPT2Config.tiny(), init_std=0.2)
NEW = 14
LENS = [9, 3, 6, 1]
KW = dict(temperature=[0.0, 0.9, 1.2, 0.0], top_k=[0, 20, 0, 0], top_p=[1.0, 1.0, 0.9, 1.0],
          seeds=[3, 4, 5, 6])
CONTROLS = dict(repetition_penalty=[1.3, 1.0, 0.8, 2.0], presence_penalty=[0.0, 0.4, 0.0, -0.2],
                frequency_penalty=[0.5, 0.0, 0.3, 0.0], min_new_tokens=[0, 6, 0, NEW],
                logit_bias=[None, {17: 2.5, 300: float("-inf")}, {}, {5: -1.0}])


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1)
    return GPT2(CFG).eval()


@pytest.fixture(scope="module")
def idx():
    return torch.randint(0, CFG.vocab_size, (4, 9), generator=torch.Generator().manual_seed(2))


@pytest.fixture(scope="module")
def plain(model, idx):
    return model.generate(idx, NEW, lens=LENS, **KW)


@pytest.fixture(scope="module")
def eos(plain):
    """A token the rows do emit, so that ``min_new_tokens`` and the EOS latch matter."""
    return int(plain[1, 2])


def _by_hand(model, idx, lens, new, eos, kw, controls):
    """The tokens, with nothing but the reference and the model's two passes."""
    B, T = idx.shape
    cache = KVCache(CFG, B, max(lens) + new, dtype=torch.float32)
    logits = model.prefill(idx, torch.tensor(lens, dtype=torch.int32), cache).clone()
    NB = rf.LOGIT_BIAS_MAX
    rows = [checked_controls(CFG.vocab_size, new, eos, **{k: v[b] for k, v in controls.items()})
            for b in range(B)]
    bias_ids = torch.zeros(B, NB, dtype=torch.int32)
    bias_vals = torch.zeros(B, NB)
    for b, r in enumerate(rows):
        for i, (t, v) in enumerate(r[4]):
            bias_ids[b, i], bias_vals[b, i] = t, v
    tables = (idx.to(torch.int32), torch.tensor(lens, dtype=torch.int32))
    params = (torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows]),
              torch.tensor([r[2] for r in rows]),
              torch.tensor([r[3] for r in rows], dtype=torch.int32), bias_ids, bias_vals,
              torch.tensor([len(r[4]) for r in rows], dtype=torch.int32))
    out = torch.zeros(B, new, dtype=torch.int64)
    done = torch.zeros(B, dtype=torch.bool)
    sample = [torch.tensor(kw["temperature"]), torch.tensor(kw["top_k"], dtype=torch.int32),
              torch.tensor(kw["top_p"]), torch.tensor(kw["seeds"])]
    for t in range(new):
        ref.logit_process(logits, *tables, out, torch.full((B,), t, dtype=torch.int32), *params,
                          eos_token_id=eos)
        tok = ref.sample_logits(logits, *sample, cache.lens)
        tok = torch.where(done, torch.full_like(tok, eos), tok)
        done |= tok == eos
        out[:, t] = tok
        if t + 1 < new:
            logits = model.decode_step(tok, cache).clone()
    return out


def test_generate_equals_the_hand_written_loop(model, idx, eos, plain):
    got = model.generate(idx, NEW, lens=LENS, eos_token_id=eos, **KW, **CONTROLS)
    want = _by_hand(model, idx, LENS, NEW, eos, KW, CONTROLS)
    assert torch.equal(got, want)
    assert not torch.equal(got, model.generate(idx, NEW, lens=LENS, eos_token_id=eos, **KW))
    # the bans: no EOS in a row's first min_new_tokens tokens, no token with a -inf bias
    assert eos not in got[1, :6].tolist() and eos not in got[3].tolist()
    assert 300 not in got[1].tolist()
    # with logprobs: the same tokens, and the values describe the processed logits, the
    # distribution the token was drawn from (the greedy rows' token is its top entry)
    toks, lp, ids, _ = model.generate(idx, NEW, lens=LENS, eos_token_id=eos, logprobs=2, **KW,
                                      **CONTROLS)
    assert torch.equal(toks, got) and torch.isfinite(lp).all()
    for b in (0, 3):
        n = toks[b].tolist().index(eos) + 1 if eos in toks[b].tolist() else NEW
        assert torch.equal(ids[b, :n, 0].long(), toks[b, :n])


def test_a_row_does_not_depend_on_its_batch_mates(model, idx, eos):
    whole = model.generate(idx, NEW, lens=LENS, eos_token_id=eos, **KW, **CONTROLS)
    for b in range(4):
        alone = model.generate(idx[b: b + 1, : LENS[b]], NEW, eos_token_id=eos,
                               **{k: [v[b]] for k, v in {**KW, **CONTROLS}.items()})
        assert torch.equal(alone[0], whole[b]), b
    # scalars are every row's value; a dict is every row's bias
    a = model.generate(idx, 5, lens=LENS, seeds=1, repetition_penalty=1.5, logit_bias={9: 1.0})
    b = model.generate(idx, 5, lens=LENS, seeds=1, repetition_penalty=[1.5] * 4,
                       logit_bias=[{9: 1.0}] * 4)
    assert torch.equal(a, b)


def test_without_controls_the_tokens_are_todays(model, idx, plain):
    calls = []
    real = rf.logit_process
    rf.logit_process = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        again = model.generate(idx, NEW, lens=LENS, **KW)
        assert not calls  # not one extra op
        neutral = model.generate(idx, NEW, lens=LENS, repetition_penalty=1.0, **KW)
        assert calls
    finally:
        rf.logit_process = real
    assert torch.equal(again, plain) and torch.equal(neutral, plain)


def test_the_calls_without_seeds_raise(model, idx):
    for k, v in (("repetition_penalty", 1.2), ("presence_penalty", 0.1),
                 ("frequency_penalty", 0.1), ("min_new_tokens", 2), ("logit_bias", {3: 1.0})):
        with pytest.raises(ValueError, match=f"{k} needs the device sampler: pass seeds="):
            model.generate(idx, 4, eos_token_id=7, **{k: v})


@pytest.mark.parametrize("bad", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
    dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
    dict(repetition_penalty="1"), dict(repetition_penalty=[1.0, 1.0]),
    dict(presence_penalty=float("inf")), dict(frequency_penalty=float("nan")),
    dict(logit_bias={3: float("inf")}), dict(logit_bias={3: float("nan")}),
    dict(logit_bias={512: 1.0}), dict(logit_bias={-1: 1.0}), dict(logit_bias={"3": 1.0}),
    dict(logit_bias=[(3, 1.0)] * 4), dict(logit_bias={i: 0.5 for i in range(65)}),
    dict(min_new_tokens=-1), dict(min_new_tokens=5), dict(min_new_tokens=1.0),
    dict(min_new_tokens=2, eos_token_id=None)])
def test_validation(model, idx, bad):
    kw = dict(seeds=1, eos_token_id=7)
    kw.update(bad)
    with pytest.raises(ValueError):
        model.generate(idx, 4, **kw)


def test_the_limits_are_accepted(model, idx):
    got = model.generate(idx, 4, seeds=1, eos_token_id=7, min_new_tokens=4,
                         logit_bias={i: -float("inf") for i in range(64)},
                         repetition_penalty=1e-3, presence_penalty=-5.0, frequency_penalty=5)
    assert got.shape == (4, 4) and (got >= 64).all() and (got != 7).all()
