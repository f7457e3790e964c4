"""The grammar kernels (ops/csrc/grammar.hip, ``rf.grammar_mask`` / ``rf.grammar_advance``)
against ``ref.grammar_mask`` / ``ref.grammar_advance`` computed on the CPU from the same
bytes: BIT EQUALITY on the whole buffer, padding and sentinels included (the reference itself
is checked bit for bit against scalar loops in test_grammar_mask.py, so there is no tolerance
anywhere). Then a row alone against the row in its batch, the window rows the speculative step
builds, every chunk size, one capture over changing inputs, and the bf16 engine and
``generate`` with grammars: graph == eager, token for token."""

import dataclasses
import functools

import pytest
import torch
from test_grammar_mask import (CAP, N_STATES, call, call_advance, make_advance_case, make_case,
                               skipped_rows)

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.models.grammar import TokenDFA
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.ops.graph_lock import CapturedStep

pytestmark = pytest.mark.gpu

VS = (1, 7, 9, 509, 50257)
BS = (1, 5, 67)


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _raw(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(V, B, seed=0):
    """The case and the reference's result on it: CPU tensors, computed once."""
    c = make_case(V, B, seed=seed)
    return c, call(ref.grammar_mask, c)


def _on(c, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in c.items()}


def _layouts(x):
    """``(name, buffer, view_of)``: the rows as a contiguous tensor, as ``[:, :V]`` of a
    buffer padded like the LM head's and as a slice that starts 3 elements in; the padding
    and the bytes before and after a sliced row hold NaN sentinels (0x7FA5)."""
    B, V = x.shape

    def sentinels(cols):
        return torch.full((B, cols), 0x7FA5, dtype=torch.int16).view(torch.bfloat16)

    yield "contiguous", x.clone(), lambda t: t
    wide = sentinels(-(-(V + 1) // 128) * 128)
    wide[:, :V] = x
    yield "padded", wide, lambda t: t[:, :V]
    odd = sentinels(V + 16)
    odd[:, 3: 3 + V] = x
    yield "sliced", odd, lambda t: t[:, 3: 3 + V]


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_kernel_bit_equal_to_the_reference(cuda_device, V, B):
    c, want = _case(V, B)
    d = _on(c, cuda_device)
    changed = (_raw(want) != _raw(c["logits"])).any(1)
    if B == 67:  # the case does exercise the bans and the skips
        skipped = skipped_rows(c)
        assert len(skipped) >= 5 and not changed[skipped].any()
        assert changed.sum() > (B - len(skipped)) // 2
    for (name, buf, view), (_, wbuf, _) in zip(_layouts(c["logits"]), _layouts(want)):
        for attempt in range(2):  # the same bits every run
            gbuf = buf.to(cuda_device)
            rows = view(gbuf)
            assert name == "contiguous" or B == 1 or not rows.is_contiguous()
            assert call(rf.grammar_mask, d, rows) is rows
            assert torch.equal(_raw(gbuf.cpu()), _raw(wbuf)), (V, B, name, attempt)


def test_every_alignment_and_chunk(cuda_device):
    """A row that starts 0..8 elements into a 16-byte slot, and the chunk sizes the launcher
    may choose: the same bytes."""
    V, B = 4099, 3
    c, want = _case(V, B, seed=5)
    d = _on(c, cuda_device)
    for start in range(9):
        buf = torch.full((B, V + 24), 0x7FA5, dtype=torch.int16).view(torch.bfloat16)
        wbuf = buf.clone()
        buf[:, start: start + V] = c["logits"]
        wbuf[:, start: start + V] = want
        for chunk in (0, 256, 512, 4096):
            gbuf = buf.to(cuda_device)
            rf.grammar_mask(gbuf[:, start: start + V], d["table"], d["state"], rows=d["rows"],
                            extra=d["extra"], n_extra=d["n_extra"], active=d["active"],
                            chunk=chunk)
            assert torch.equal(_raw(gbuf.cpu()), _raw(wbuf)), (start, chunk)


def test_a_row_alone_and_among_others(cuda_device):
    c, want = _case(50257, 67)
    live = [b for b in range(67) if b not in skipped_rows(c)]
    for b in (live[0], live[len(live) // 2], live[-1], 0):
        one = {k: v for k, v in c.items()}
        for k in ("logits", "rows", "extra", "n_extra", "active"):
            one[k] = c[k][b: b + 1]
        got = call(rf.grammar_mask, _on(one, cuda_device))
        assert torch.equal(_raw(got.cpu()), _raw(want[b: b + 1])), b


def test_window_rows_as_the_engine_builds_them(cuda_device):
    """S slots, W window rows each: row (s, j) has the slot's state, ``win[s]`` as its extra
    tokens, ``n_extra = j + 1``, and is live iff ``j < n_win[s]`` and the slot is active. A
    forbidden draft leaves its own row and every later row of the slot untouched."""
    S, W, V = 6, 5, 50257
    c, _ = _case(V, S, seed=3)
    g = torch.Generator().manual_seed(9)
    table = c["table"]
    state = torch.tensor([2, 5, 0, 9, ref.GRAMMAR_NONE, 11], dtype=torch.int32)
    win = torch.zeros(S, W, dtype=torch.int64)
    for s in range(S):  # allowed tokens all along, but for slot 5: its third is forbidden
        q = max(int(state[s]), 0)
        for j in range(W):
            # (targets >= 2: the states 0 and 1 of the case allow all tokens / one token)
            ok = table[q, :V] < 0 if s == 5 and j == 2 else table[q, :V] >= 2
            ids = torch.nonzero(ok).view(-1)
            win[s, j] = ids[int(torch.randint(0, len(ids), (1,), generator=g))]
            q = max(int(table[q, win[s, j]]), 0)
    n_win = torch.tensor([5, 1, 0, 3, 5, 5], dtype=torch.int32)
    slot_active = torch.tensor([1, 1, 1, 0, 1, 1], dtype=torch.uint8)
    live = (torch.arange(W).unsqueeze(0) < n_win.unsqueeze(1)) & slot_active.bool().unsqueeze(1)
    w = dict(c, state=state, rows=torch.arange(S, dtype=torch.int32).repeat_interleave(W),
             extra=win.unsqueeze(1).expand(S, W, W).reshape(S * W, W).contiguous(),
             n_extra=torch.arange(1, W + 1, dtype=torch.int32).repeat(S),
             active=live.to(torch.uint8).view(S * W),
             logits=(torch.randn(S * W, V, generator=g) * 4).to(torch.bfloat16))
    want = call(ref.grammar_mask, w)
    changed = (_raw(want) != _raw(w["logits"])).any(1).view(S, W)
    assert changed[0].all() and changed[1].tolist() == [True, False, False, False, False]
    assert not changed[2:5].any() and changed[5].tolist() == [True, True, False, False, False]
    buf = torch.full((S, W, 50304), float("nan"), dtype=torch.bfloat16)
    buf.view(S * W, -1)[:, :V] = w["logits"]
    gbuf = buf.to(cuda_device)
    call(rf.grammar_mask, _on(w, cuda_device), gbuf.view(S * W, -1)[:, :V])
    got = gbuf.cpu().view(S * W, -1)
    assert torch.equal(_raw(got[:, :V]), _raw(want)) and got[:, V:].isnan().all()


def test_other_inputs_take_the_reference(cuda_device):
    """fp32 logits, a window wider than the kernel walks, a misaligned table: same results."""
    c, want = _case(509, 5)
    d = _on(c, cuda_device)
    got = call(rf.grammar_mask, d, c["logits"].float().to(cuda_device))
    assert torch.equal(got.cpu().view(torch.int32), want.float().view(torch.int32))
    wide = dict(c, extra=torch.cat([c["extra"], torch.zeros(5, rf.GRAMMAR_MAX_WALK,
                                                            dtype=torch.int64)], 1))
    got = call(rf.grammar_mask, _on(wide, cuda_device))
    assert torch.equal(_raw(got.cpu()), _raw(want))
    shifted = torch.zeros(N_STATES + 1, 512, dtype=torch.int16, device=cuda_device)
    shifted.view(-1)[4: 4 + N_STATES * 512] = d["table"].view(-1)
    off = dict(d, table=shifted.view(-1)[4: 4 + N_STATES * 512].view(N_STATES, 512))
    assert off["table"].data_ptr() % 16 == 8
    assert torch.equal(_raw(call(rf.grammar_mask, off).cpu()), _raw(want))


@pytest.mark.parametrize("max_steps", (0, 1, 3, CAP + 2))
def test_advance_bit_equal_to_the_reference(cuda_device, max_steps):
    for V, R in ((9, 5), (509, 67), (50257, 67)):
        c = make_advance_case(V, R)
        want = call_advance(ref.grammar_advance, c, max_steps)
        got = call_advance(rf.grammar_advance, _on(c, cuda_device), max_steps)
        assert got[0].cpu().tolist() == want[0].tolist(), (V, R)
        assert got[1].cpu().tolist() == want[1].tolist(), (V, R)


def test_one_capture_serves_changing_inputs(cuda_device):
    dev, V, B = cuda_device, 50257, 5
    cases = [_case(V, B, seed=s) for s in (11, 12, 13)]
    static = _on(cases[0][0], dev)
    buf = torch.zeros(B, 50304, device=dev, dtype=torch.bfloat16)
    static["logits"] = buf[:, :V]
    adv = _on(make_advance_case(V, 8, seed=11), dev)
    adv["table"] = static["table"]

    def step():
        call(rf.grammar_mask, static, static["logits"])
        rf.grammar_advance(adv["state"], adv["pos"], adv["out"], adv["n_out"], adv["table"], 2)

    step()  # warm-up
    graph = CapturedStep(step, dev)
    for (c, want), s in zip(cases, (11, 12, 13)):
        for k, v in c.items():  # the logits, the states, the windows AND the table's contents
            if isinstance(v, torch.Tensor):
                static[k].copy_(v)
        a = make_advance_case(V, 8, seed=s)
        a["table"] = c["table"]
        for k in ("state", "pos", "out", "n_out"):
            adv[k].copy_(a[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_raw(buf[:, :V].cpu()), _raw(want))
        assert not buf[:, V:].any()
        ws, wp = call_advance(ref.grammar_advance, a, 2)
        assert adv["state"].cpu().tolist() == ws.tolist()
        assert adv["pos"].cpu().tolist() == wp.tolist()


# ------------------------------------------------------------------ the engine, generate
def _cfg():
    return dataclasses.replace(GPT2Config.tiny(), n_embd=128, n_head=2, n_positions=256,
                               init_std=0.2)


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(0)
    return GPT2(_cfg()).eval().to(dev, torch.bfloat16)


EOS = 7


@functools.lru_cache(maxsize=None)
def _grammars():
    V = _cfg().vocab_size
    vocab = [bytes([i]) for i in range(256)] + [bytes([97 + i % 26, 97 + i // 26 % 26])
                                                for i in range(V - 256)]
    vocab[EOS] = b""
    return (TokenDFA.from_choices([[3, 4, 5], [3, 4], [400, 9, 9, 9, 2], [11]], V, EOS),
            TokenDFA.from_regex(r"([a-z]{1,4} ){2,6}[a-z]+\.", vocab, EOS),
            TokenDFA.from_regex(r"\d{3}-\d{4}|[A-F0-9]{6,12}", vocab, EOS))


def _words_ok(dfa, toks, max_new):
    toks = list(toks)
    if EOS in toks:
        toks = toks[: toks.index(EOS) + 1]
        return dfa.accepts(toks)
    return len(toks) == max_new and dfa.walk(toks) >= 0


def test_generate_with_grammars_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    choices, words, codes = _grammars()
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 512, (4, 40), generator=g).to(cuda_device)
    kw = dict(lens=[40, 7, 22, 31], temperature=[0.0, 0.8, 1.3, 1.0], top_k=[0, 5, 0, 0],
              top_p=[1.0, 1.0, 0.9, 1.0], seeds=[4, 5, 6, 7], eos_token_id=EOS, logprobs=3,
              repetition_penalty=[1.0, 1.2, 1.0, 1.0])
    gram = [choices, words, None, codes]
    eager = model.generate(idx, 24, grammar=gram, **kw)
    graphed = model.generate(idx, 24, graph=True, grammar=gram, **kw)
    for a, b in zip(eager, graphed):
        a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
        assert torch.equal(a, b)
    plain = model.generate(idx, 24, graph=True, **kw)
    assert torch.equal(plain[0][2], graphed[0][2])  # the row without a grammar
    for b, dfa in enumerate(gram):
        if dfa is not None:
            assert _words_ok(dfa, graphed[0][b].tolist(), 24), b
            assert not torch.equal(plain[0][b], graphed[0][b])
    # logprobs are those of the masked distribution: a forbidden token never ranks
    q = choices.start
    for t, ids in zip(graphed[0][0].tolist(), graphed[2][0].tolist()):
        allowed = {i for i in range(choices.vocab_size) if choices.next[q, i] >= 0}
        assert set(ids[: len(allowed)]) <= allowed
        q = int(choices.next[q, t])
        if t == EOS:
            break


# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, continues the prefix,
# logprobs, grammar index or None, controls)
MIX = [(1, 24, 0.0, None, None, 3, True, 5, 1, dict(repetition_penalty=1.3)),
       (150, 9, 0.8, 5, None, 11, False, 2, None, dict()),
       (17, 16, 1.3, 50, 0.9, 2, True, None, 0, dict()),
       (70, 30, 0.8, None, 0.9, 7, True, 0, 2, dict(logit_bias={5: 4.0})),
       (9, 20, 1.3, None, None, -4, False, 5, None, dict(presence_penalty=0.5)),
       (130, 12, 1.0, None, None, 0, True, 3, 1, dict())]


def _drive(model, graph, speculate, grammars=True):
    g = torch.Generator().manual_seed(5)
    prefix = torch.randint(0, 512, (70,), generator=g).tolist()
    prompts = [torch.randint(0, 512, (m[0],), generator=g).tolist() for m in MIX]
    kw = {} if graph else {"graph": False}
    dfas = _grammars()
    eng = GPT2Engine(model, slots=3, max_len=256, poll_every=2, prefix_slots=1, prefill_chunk=64,
                     eos_token_id=EOS, speculate=speculate, logprobs=5, logit_processors=True,
                     grammar_states=sum(d.n_states for d in dfas) if grammars else 0, **kw)
    assert (eng._graph is not None) == graph
    gids = [eng.add_grammar(d) for d in dfas] if grammars else []
    pid = eng.add_prefix(prefix)
    rids = [eng.submit(p, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                       prefix=pid if m[6] else None, logprobs=m[7],
                       **({"grammar": gids[m[8]]} if grammars and m[8] is not None else {}),
                       **m[9])
            for p, m in zip(prompts, MIX)]
    got = eng.run(logprobs=True)
    assert not eng.has_work() and eng.num_filling == 0
    return [got[r] for r in rids]


@pytest.mark.parametrize("speculate", [0, 4])
def test_engine_with_grammars_graph_equals_eager(cuda_device, speculate):
    model = _model(cuda_device)
    graphed = _drive(model, True, speculate)
    eager = _drive(model, False, speculate)
    for (tg, ig), (te, ie), m in zip(graphed, eager, MIX):
        assert tg == te
        if m[7] is None:
            assert ig is None and ie is None
            continue
        assert ig["top_ids"] == ie["top_ids"]
        for k in ("logprobs", "top_logprobs"):  # (floats from the fp32 tables: == is bitwise)
            assert torch.equal(torch.tensor(ig[k], dtype=torch.float64),
                               torch.tensor(ie[k], dtype=torch.float64)), k
    # every constrained request is a word of its grammar, the others got what they always got
    plain = _drive(model, True, speculate, grammars=False)
    dfas = _grammars()
    for i, m in enumerate(MIX):
        if m[8] is None:
            assert plain[i][0] == graphed[i][0]
        else:
            assert _words_ok(dfas[m[8]], graphed[i][0], m[1]), i


def test_pool_rows_are_reused_without_a_new_capture(cuda_device):
    model = _model(cuda_device)
    choices, words, codes = _grammars()
    eng = GPT2Engine(model, slots=2, max_len=128, eos_token_id=EOS,
                     grammar_states=words.n_states + codes.n_states)
    graph, table = eng._graph, eng.gtable.data_ptr()
    assert graph is not None
    eng.add_grammar(words)
    b = eng.add_grammar(codes)
    r = eng.submit([1, 2, 3], 14, grammar=b, temperature=1.0, seed=2)
    assert _words_ok(codes, eng.run()[r], 14)
    with pytest.raises(ValueError, match="pool is full"):
        eng.add_grammar(choices)
    eng.drop_grammar(b)
    c = eng.add_grammar(choices)  # into the rows that held ``codes``
    r = eng.submit([1, 2, 3], 14, grammar=c, temperature=1.0, seed=2)
    assert _words_ok(choices, eng.run()[r], 14)
    assert eng._graph is graph and eng.gtable.data_ptr() == table
