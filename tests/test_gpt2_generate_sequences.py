"""``GPT2.generate(..., seeds=, stop=, bad_words=, no_repeat_ngram_size=)`` on a tiny fp32 model
on the CPU: no output completes a banned sequence or repeats an n-gram, over prompt plus
output, under every sampling setting; a greedy row equals a host loop that recomputes the
forward and takes the lowest-index maximum among the tokens the scalar rules of
test_seq_rules.py leave; a row ends right after its first completed stop sequence and is
padded with EOS; a row's tokens do not depend on its batch-mates; logprobs describe the
banned distribution; the rejected values and combinations raise."""

import pytest
import torch
from test_gpt2_generate import PROMPT_LENS, scaled_tiny
from test_seq_rules import banned_tokens

from ray_amd.models.gpt2 import checked_grammar_sequences, checked_sequences
from ray_amd.models.grammar import TokenDFA
from ray_amd.ops import functional as rf

EOS = 7
NEW = 24  # prompt (<= 40) + NEW + SEQ_MAX < 512: a row always has an unbanned token
V = 512
B = len(PROMPT_LENS)
SAMPLING = [dict(), dict(temperature=0.9), dict(temperature=1.2, top_k=20),
            dict(temperature=[0.0, 0.8, 1.3, 0.7], top_p=[1.0, 0.9, 1.0, 0.8])]


@pytest.fixture(scope="module")
def model():
    return scaled_tiny()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, V, (B, max(PROMPT_LENS)), generator=g)
    for b, n in enumerate(PROMPT_LENS):
        idx[b, n:] = 0
    return idx


def _gen(model, prompts, new=NEW, **kw):
    kw.setdefault("seeds", [3, 4, 5, 6])
    return model.generate(prompts, new, lens=list(PROMPT_LENS), eos_token_id=EOS, **kw)


@pytest.fixture(scope="module")
def bare(model, prompts):
    return _gen(model, prompts).tolist()


def cut(toks, stops=()):
    """``toks`` after the first EOS or the first completed stop sequence, whichever ends
    earlier."""
    stops = [[s] if isinstance(s, int) else s for s in stops]
    for e in range(1, len(toks) + 1):
        if toks[e - 1] == EOS or any(len(s) <= e and toks[e - len(s): e] == list(s)
                                     for s in stops):
            return toks[:e]
    return toks


def violations(prompt, out, bads=(), n=0):
    """The output positions at which ``prompt + out`` completes a banned sequence or an n-gram
    that occurred before."""
    seq, res = list(prompt) + list(out), []
    bads = [[s] if isinstance(s, int) else s for s in bads]
    for e in range(len(prompt) + 1, len(seq) + 1):
        if any(len(s) <= e and seq[e - len(s): e] == list(s) for s in bads):
            res.append(e - len(prompt) - 1)
        if n and e >= n and any(seq[i: i + n] == seq[e - n: e] for i in range(e - n)):
            res.append(e - len(prompt) - 1)
    return res


def _rows(prompts):
    return [prompts[b, :n].tolist() for b, n in enumerate(PROMPT_LENS)]


@pytest.mark.parametrize("sampling", SAMPLING)
def test_no_banned_sequence_and_no_repeated_ngram(model, prompts, bare, sampling):
    free = _gen(model, prompts, **sampling).tolist()
    # per row: what the free run does is forbidden (its first token, a pair of its tokens, a
    # token after the prompt's last one) and n-grams of size 1, 2, 3 and off
    bads = [[free[b][0], free[b][2:4], [_rows(prompts)[b][-1], free[b][0]],
             [1, 2, 3, 4, 5, 6, 7, 8]] for b in range(B)]
    ngs = [1, 2, 3, 0]
    got = _gen(model, prompts, bad_words=bads, no_repeat_ngram_size=ngs, **sampling).tolist()
    for b, p in enumerate(_rows(prompts)):
        out = cut(got[b])
        assert set(got[b][len(out):]) <= {EOS}
        body = out[:-1] if out[-1] == EOS else out  # (EOS itself is a token like any other)
        assert violations(p, out, bads[b], ngs[b]) == [], (b, out)
        assert got[b][0] != free[b][0] and len(body) >= 1
        assert violations(p, cut(free[b]), bads[b], ngs[b]) != []
    # n = 1 over prompt and output: every token is new
    p0 = _rows(prompts)[0]
    assert len(set(p0 + cut(got[0]))) == len(p0) + len(cut(got[0]))


def _recompute(model, prompt, bads, n, n_new):
    """Greedy, with nothing but ``forward`` and the scalar rules."""
    seq, out = list(prompt), []
    with torch.no_grad():
        for _ in range(n_new):
            if out and out[-1] == EOS:
                out.append(EOS)
                continue
            logits = model(torch.tensor([seq]))[0, -1].clone()
            for t in banned_tokens(seq, n, [s + [0] * 8 for s in bads], [len(s) for s in bads]):
                logits[t] = float("-inf")
            out.append(int(logits.argmax()))
            seq.append(out[-1])
    return out


@pytest.mark.parametrize("n", [0, 2, 8])
def test_greedy_row_equals_a_host_loop(model, prompts, bare, n):
    for b in (1, 2):
        p = _rows(prompts)[b]
        bads = [[bare[b][0]], bare[b][1:3], [p[-1], bare[b][4]]]
        got = model.generate(torch.tensor([p]), 12, seeds=[0], eos_token_id=EOS, bad_words=bads,
                             no_repeat_ngram_size=n)[0].tolist()
        assert got == _recompute(model, p, bads, n, 12)
        assert got != bare[b][:12]


def test_a_row_ends_right_after_its_first_completed_stop(model, prompts, bare):
    # stops taken from the free output: a single token, a pair, the longest sequence, one that
    # never occurs; the tokens before the stop are the free run's (a stop bans nothing)
    stops = [[bare[0][3]], [bare[1][4:6], [509, 510]], [bare[2][2:10], bare[2][5:7]],
             [[509, 510]]]
    got = _gen(model, prompts, stop=stops).tolist()
    for b in range(B):
        want = cut(bare[b], stops[b])
        assert got[b][: len(want)] == want, b
        assert set(got[b][len(want):]) <= {EOS}
    assert len(cut(bare[2], [bare[2][5:7]])) == 7 and got[2][7:] == [EOS] * (NEW - 7)
    assert got[3] == bare[3]
    # one value for all rows; a bare int is a one-token sequence
    t = bare[1][2]
    got = _gen(model, prompts, stop=[t, [508, 509]]).tolist()
    for b in range(B):
        want = cut(bare[b], [[t], [508, 509]])
        assert got[b] == want + [EOS] * (NEW - len(want))
    # with the other rules: the stop cuts the banned run
    kw = dict(bad_words=[[bare[b][0]] for b in range(B)], no_repeat_ngram_size=2)
    free = _gen(model, prompts, **kw).tolist()
    stops = [[free[b][3:5]] for b in range(B)]
    got = _gen(model, prompts, stop=stops, **kw).tolist()
    for b in range(B):
        want = cut(free[b], stops[b])
        assert got[b] == want + [EOS] * (NEW - len(want)) and len(want) <= 5


def test_rows_do_not_depend_on_their_batch_mates(model, prompts, bare):
    kw = dict(temperature=[0.0, 0.8, 1.3, 0.7], top_k=[0, 20, 0, 5])
    stops = [None, [bare[1][3:5]], None, [[bare[3][1]]]]
    bads = [[[bare[0][0]]], None, [bare[2][0], bare[2][1:3]], None]
    ngs = [2, 0, 3, 0]
    lp = _gen(model, prompts, stop=stops, bad_words=bads, no_repeat_ngram_size=ngs, logprobs=2,
              **kw)
    got = lp[0].tolist()
    for b, p in enumerate(_rows(prompts)):
        alone = model.generate(torch.tensor([p]), NEW, seeds=[3 + b], eos_token_id=EOS,
                               temperature=kw["temperature"][b], top_k=kw["top_k"][b],
                               stop=stops[b], bad_words=bads[b], no_repeat_ngram_size=ngs[b],
                               logprobs=2)
        assert alone[0][0].tolist() == got[b], b
        n = len(cut(got[b], stops[b] or []))
        assert torch.allclose(alone[1][0, :n], lp[1][b, :n], atol=1e-4)
        assert alone[2][0, :n].tolist() == lp[2][b, :n].tolist()
    # a row without a rule gets what it got without the arguments, whoever shares the batch
    plain = _gen(model, prompts, **kw).tolist()
    only = _gen(model, prompts, stop=[None, None, None, [[5]]], **kw).tolist()
    assert only[:3] == plain[:3]
    assert got[1][: len(cut(got[1], stops[1]))] == cut(plain[1], stops[1])


def test_logprobs_describe_the_banned_distribution(model, prompts, bare):
    free = _gen(model, prompts, logprobs=3)
    top0 = free[2][:, 0, 0].tolist()  # the most likely first token of every row
    assert top0 == [r[0] for r in bare]
    got = _gen(model, prompts, logprobs=3, bad_words=[[t] for t in top0])
    for b in range(B):
        assert top0[b] not in got[2][b, 0].tolist()
        assert got[2][b, 0, 0] == free[2][b, 0, 1]  # the runner-up leads
        assert got[1][b, 0] > free[3][b, 0, 1]  # and gained of the banned token's mass


def test_checked_sequences():
    assert checked_sequences(V, EOS) is None
    assert checked_sequences(V, EOS, stop=[5, [1, 2]], bad_words=[(3,)]) == \
        ([[5], [1, 2]], [[3]], 0)
    assert checked_sequences(V, None, bad_words=[], no_repeat_ngram_size=8) == ([], [], 8)
    assert checked_sequences(V, EOS, stop=[list(range(8))] * 8)[0][7] == list(range(8))
    for kw in (dict(stop=[[1]] * 9), dict(bad_words=[1] * 9), dict(stop=[[]]),
               dict(bad_words=[list(range(9))]), dict(stop=[[V]]), dict(bad_words=[[-1]]),
               dict(bad_words=[[1, True]]), dict(stop=[[1.0]]), dict(stop=[True]),
               dict(stop=5), dict(bad_words="ab"), dict(bad_words=["ab"]),
               dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=-1),
               dict(no_repeat_ngram_size=True), dict(no_repeat_ngram_size=2.0)):
        with pytest.raises(ValueError):
            checked_sequences(V, EOS, **kw)
    with pytest.raises(ValueError, match="eos_token_id"):
        checked_sequences(V, None, stop=[[1]])
    assert (rf.SEQ_MAX, rf.SEQ_MAX_LEN) == (8, 8)


def test_rejections(model, prompts):
    for kw in (dict(stop=[[1]]), dict(bad_words=[[1]]), dict(no_repeat_ngram_size=2)):
        with pytest.raises(ValueError, match="seeds"):
            model.generate(prompts, 4, eos_token_id=EOS, **kw)
    with pytest.raises(ValueError, match="eos_token_id"):
        model.generate(prompts, 4, seeds=0, stop=[[1]])
    for kw in (dict(stop=[[V]]), dict(bad_words=[[1]] * 9), dict(no_repeat_ngram_size=9),
               dict(no_repeat_ngram_size=[1, 2]), dict(stop=[None, [[1]]]),
               dict(bad_words=[None, None, None, [[1, 2, 3, 4, 5, 6, 7, 8, 9]]])):
        with pytest.raises(ValueError):
            model.generate(prompts, 4, seeds=0, eos_token_id=EOS, **kw)
    dfa = TokenDFA.from_choices([[3, 4, 5], [11]], V, EOS)
    for kw in (dict(bad_words=[[1]]), dict(no_repeat_ngram_size=2),
               dict(bad_words=[None, None, None, [[1]]])):
        with pytest.raises(ValueError, match="grammar"):
            model.generate(prompts, 4, seeds=0, eos_token_id=EOS, grammar=dfa, **kw)
    # a grammar on one row, a ban on another: fine; so are stop and n = 0 with a grammar
    model.generate(prompts, 4, seeds=0, eos_token_id=EOS, grammar=[dfa, None, None, None],
                   bad_words=[None, [[1]], None, None], no_repeat_ngram_size=[0, 2, 0, 0])
    checked_grammar_sequences(dfa, ([[1]], [], 0))
    checked_grammar_sequences(None, ([[1]], [[2]], 3))
    checked_grammar_sequences(dfa, None)


def test_stop_with_a_grammar_leaves_a_prefix_of_a_word(model, prompts):
    dfa = TokenDFA.from_choices([[3, 4, 5, 6, 9], [400, 9, 9, 9, 2]], V, EOS)
    free = _gen(model, prompts, grammar=dfa, new=8).tolist()
    got = _gen(model, prompts, grammar=dfa, new=8, stop=[[4, 5], [9, 9]]).tolist()
    for b in range(B):
        want = cut(free[b], [[4, 5], [9, 9]])
        assert got[b] == want + [EOS] * (8 - len(want))
        assert want[-1] != EOS and dfa.walk(want) >= 0 and len(want) == 3
