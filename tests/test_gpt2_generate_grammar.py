"""``GPT2.generate(..., seeds=, grammar=)`` on a tiny fp32 model on the CPU: every constrained
row is a word of its grammar (or a prefix of one where ``max_new_tokens`` cuts it) under every
sampling setting; a greedy row equals a host loop that recomputes the forward, walks the
automaton and takes the lowest-index maximum among the allowed tokens; rows without a grammar
get what they got without the argument; logprobs describe the masked distribution; the
rejected combinations raise."""

import numpy as np
import pytest
import torch
from test_gpt2_generate import PROMPT_LENS, scaled_tiny

from ray_amd.models.grammar import TokenDFA

EOS = 7
NEW = 24
V = 512
VOCAB = [bytes([i]) for i in range(256)] + [bytes([97 + i % 26, 97 + i // 26 % 26])
                                            for i in range(V - 256)]


@pytest.fixture(scope="module")
def model():
    return scaled_tiny()


@pytest.fixture(scope="module")
def prompts(model):
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, V, (len(PROMPT_LENS), max(PROMPT_LENS)), generator=g)
    for b, n in enumerate(PROMPT_LENS):
        idx[b, n:] = 0
    return idx


@pytest.fixture(scope="module")
def grammars():
    return {"choices": TokenDFA.from_choices([[3, 4, 5], [3, 4], [400, 9, 9, 9, 2], [11],
                                              [400, 9, 300]], V, EOS),
            "words": TokenDFA.from_regex(r"([a-z]{1,4} ){2,4}[a-z]{1,6}\.", VOCAB, EOS),
            "codes": TokenDFA.from_regex(r"\d{3}-\d{4}|[A-F0-9]{6,12}", VOCAB, EOS),
            "long": TokenDFA.from_regex(r"(ab|cd)+x?", VOCAB, EOS)}


def word_or_prefix(dfa, toks, max_new):
    """Accepted up to and including the first EOS, or never finished: alive and cut."""
    toks = list(toks)
    if EOS in toks:
        n = toks.index(EOS) + 1
        return dfa.accepts(toks[:n]) and set(toks[n:]) <= {EOS}
    return len(toks) == max_new and dfa.walk(toks) >= 0


def _recompute_constrained(model, prompt, dfa, n_new):
    """Greedy, with nothing but ``forward`` and the automaton's table."""
    seq = prompt.clone().view(1, -1)
    q, out = dfa.start, []
    with torch.no_grad():
        for _ in range(n_new):
            if out and out[-1] == EOS:
                out.append(EOS)
                continue
            logits = model(seq)[0, -1, :V]
            allowed = torch.from_numpy(np.asarray(dfa.next[q]) >= 0)
            masked = torch.where(allowed, logits, torch.full_like(logits, float("-inf")))
            t = int(torch.nonzero(masked == masked.max())[0])
            out.append(t)
            q = int(dfa.next[q, t])
            seq = torch.cat([seq, torch.tensor([[t]])], 1)
    return out


def test_greedy_rows_equal_the_recompute_loop(model, prompts, grammars):
    names = ["choices", "words", "codes", "long"]
    gram = [grammars[n] for n in names]
    out = model.generate(prompts, NEW, lens=list(PROMPT_LENS), seeds=0, eos_token_id=EOS,
                         grammar=gram)
    for b, n in enumerate(PROMPT_LENS):
        want = _recompute_constrained(model, prompts[b, :n], gram[b], NEW)
        assert out[b].tolist() == want, names[b]
        assert word_or_prefix(gram[b], want, NEW)
    assert EOS not in out[3].tolist()  # "(ab|cd)+x?" can go on: max_new_tokens cuts it
    # one grammar for every row, and a single row: the same tokens
    one = model.generate(prompts, NEW, lens=list(PROMPT_LENS), seeds=0, eos_token_id=EOS,
                         grammar=gram[1])
    assert torch.equal(one[1], out[1])
    solo = model.generate(prompts[2:3, :17], NEW, seeds=[0], eos_token_id=EOS, grammar=[gram[2]])
    assert torch.equal(solo[0], out[2])


SETTINGS = [dict(temperature=0.0), dict(temperature=1.0), dict(temperature=1.5, top_k=3),
            dict(temperature=0.8, top_p=0.7), dict(temperature=2.0, top_k=40, top_p=0.95),
            dict(temperature=1.2, repetition_penalty=1.5, frequency_penalty=0.8),
            dict(temperature=0.0, presence_penalty=1.0, logit_bias={9: 5.0, 98: 3.0}),
            dict(temperature=1.0, top_p=0.5, repetition_penalty=0.7, min_new_tokens=0)]


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
def test_every_output_is_a_word_of_its_grammar(model, prompts, grammars, setting):
    kw = SETTINGS[setting]
    gram = [grammars["choices"], grammars["words"], None, grammars["codes"]]
    seeds = [10 * setting + b for b in range(4)]
    out = model.generate(prompts, NEW, lens=list(PROMPT_LENS), seeds=seeds, eos_token_id=EOS,
                         grammar=gram, **kw)
    bare = model.generate(prompts, NEW, lens=list(PROMPT_LENS), seeds=seeds, eos_token_id=EOS,
                          **kw)
    for b, dfa in enumerate(gram):
        if dfa is None:  # untouched by its batch-mates' grammars
            assert torch.equal(out[b], bare[b])
        else:
            assert word_or_prefix(dfa, out[b].tolist(), NEW), (b, out[b].tolist())
            assert not torch.equal(out[b], bare[b])
    # the finite grammars do finish
    assert EOS in out[0].tolist() and EOS in out[3].tolist()


def test_logprobs_are_those_of_the_masked_distribution(model, prompts, grammars):
    dfa = grammars["choices"]
    toks, lp, ids, tlp = model.generate(prompts[:2], 6, lens=[1, 5], seeds=[1, 2],
                                        temperature=[1.0, 0.0], eos_token_id=EOS,
                                        grammar=[dfa, None], logprobs=4)
    q = dfa.start
    for t in range(6):
        allowed = np.flatnonzero(dfa.next[q] >= 0)
        k = min(4, len(allowed))
        assert set(ids[0, t, :k].tolist()) <= set(allowed.tolist())
        assert torch.isinf(tlp[0, t, k:]).all() and (tlp[0, t, k:] < 0).all()
        # the allowed tokens' probabilities sum to one
        if len(allowed) <= 4:
            assert abs(float(tlp[0, t, :k].exp().sum()) - 1) < 1e-5
        assert lp[0, t] <= 0 and int(toks[0, t]) in allowed
        q = int(dfa.next[q, int(toks[0, t])])
        if int(toks[0, t]) == EOS:
            break
    bare = model.generate(prompts[:2], 6, lens=[1, 5], seeds=[1, 2], temperature=[1.0, 0.0],
                          eos_token_id=EOS, logprobs=4)
    for a, b in zip((toks, lp, ids, tlp), bare):
        assert torch.equal(a[1], b[1])


def test_argument_errors(model, prompts, grammars):
    dfa = grammars["choices"]
    kw = dict(lens=list(PROMPT_LENS), eos_token_id=EOS)
    with pytest.raises(ValueError, match="seeds="):
        model.generate(prompts, 4, grammar=dfa, **kw)
    with pytest.raises(ValueError, match="eos_token_id"):
        model.generate(prompts, 4, seeds=0, grammar=dfa, lens=list(PROMPT_LENS))
    with pytest.raises(ValueError, match="EOS"):
        model.generate(prompts, 4, seeds=0, grammar=dfa, lens=list(PROMPT_LENS), eos_token_id=8)
    with pytest.raises(ValueError, match="TokenDFA"):
        model.generate(prompts, 4, seeds=0, grammar=["choices", None, None, None], **kw)
    with pytest.raises(ValueError, match="entries"):
        model.generate(prompts, 4, seeds=0, grammar=[dfa, None], **kw)
    with pytest.raises(ValueError, match="tokens"):
        model.generate(prompts, 4, seeds=0, grammar=TokenDFA.from_choices([[1]], 100, EOS), **kw)
    with pytest.raises(ValueError, match="min_new_tokens"):
        model.generate(prompts, 4, seeds=0, grammar=[dfa, None, None, None],
                       min_new_tokens=[2, 0, 0, 0], **kw)
    with pytest.raises(ValueError, match="-inf"):
        model.generate(prompts, 4, seeds=0, grammar=[None, None, dfa, None],
                       logit_bias=[None, None, {3: float("-inf")}, None], **kw)
    # the same controls on the rows WITHOUT a grammar are fine
    out = model.generate(prompts, 4, seeds=0, grammar=[dfa, None, None, None],
                         min_new_tokens=[0, 2, 0, 0],
                         logit_bias=[None, None, {3: float("-inf")}, None], **kw)
    assert word_or_prefix(dfa, out[0].tolist(), 4)
    # all rows None: the call without the argument
    assert torch.equal(model.generate(prompts, 4, seeds=0, grammar=[None] * 4, **kw),
                       model.generate(prompts, 4, seeds=0, **kw))
