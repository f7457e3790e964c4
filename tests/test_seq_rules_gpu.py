"""The sequence-rule kernels (ops/csrc/seq_rules.hip, ``rf.seq_ban`` and ``rf.stop_check``)
against ``ref.seq_ban`` / ``ref.stop_check`` computed on the CPU from the same bytes: BIT
EQUALITY on the whole logits buffer, padding and sentinels included, and exact equality of
every integer output (the references are checked against scalar loops in test_seq_rules.py,
so there is no tolerance anywhere). Then repeatability, a row alone against the row in its
batch, the window rows the speculative step builds, one capture over changing inputs, and
the bf16 engine and ``generate`` with all three rules: graph == eager bit for bit."""

import dataclasses
import functools

import pytest
import torch
from test_seq_rules import (NAMES, STOP_NAMES, call, call_stop, make_case, make_stop_case,
                            skipped_rows)

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.ops.graph_lock import CapturedStep

pytestmark = pytest.mark.gpu

VS = (1, 7, 9, 509, 50257)
BS = (1, 5, 67)
WIDTH = 1024  # the tables' width: one context row is full


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _raw(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(V, B, seed=0):
    """The case and the reference's result on it: CPU tensors, computed once."""
    c = make_case(V, B, seed=seed, width=WIDTH)
    return c, call(ref.seq_ban, c)


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
def test_seq_ban_bit_equal_to_the_reference(cuda_device, V, B):
    c, want = _case(V, B)
    d = _on(c, cuda_device)
    changed = (_raw(want) != _raw(c["logits"])).any(1)
    if B == 67:  # the case does exercise the rules and the skips
        skipped = skipped_rows(c)
        assert len(skipped) >= 5 and not changed[skipped].any()
        assert changed.sum() > (B - len(skipped)) // 2
        assert int(c["prompt_len"][0]) == WIDTH and int(c["n_out"][0]) == WIDTH
    for (name, buf, view), (_, wbuf, _) in zip(_layouts(c["logits"]), _layouts(want)):
        for attempt in range(2):  # the same bits every run
            gbuf = buf.to(cuda_device)
            rows = view(gbuf)
            assert name == "contiguous" or B == 1 or not rows.is_contiguous()
            assert call(rf.seq_ban, d, rows) is rows
            assert torch.equal(_raw(gbuf.cpu()), _raw(wbuf)), (V, B, name, attempt)


@pytest.mark.parametrize("max_span", [None, 1, 4])
@pytest.mark.parametrize("R", BS)
def test_stop_check_equal_to_the_reference(cuda_device, R, max_span):
    for seed in range(3):
        c = make_stop_case(R, seed)
        want = call_stop(ref.stop_check, c, max_span)
        for attempt in range(2):
            assert call_stop(rf.stop_check, _on(c, cuda_device), max_span) == want
        bare = call_stop(rf.stop_check, _on(c, cuda_device), max_span, optional=False)
        assert [bare[k] for k in ("n_out", "pos", "hit")] == \
            [want[k] for k in ("n_out", "pos", "hit")]
        assert [bare[k] for k in ("active", "lens", "done")] == \
            [c[k].tolist() for k in ("active", "lens", "done")]
    if R == 67 and max_span is None:
        assert 5 <= sum(h >= 0 for h in want["hit"]) < R


def test_a_row_alone_and_among_others(cuda_device):
    c, want = _case(50257, 67)
    live = [b for b in range(67) if b not in skipped_rows(c)]
    for b in (live[0], live[len(live) // 2], live[-1], 0):
        one = {k: v for k, v in c.items()}
        for k in ("logits", "rows", "extra", "n_extra", "active"):
            one[k] = c[k][b: b + 1]
        got = call(rf.seq_ban, _on(one, cuda_device))
        assert torch.equal(_raw(got.cpu()), _raw(want[b: b + 1])), b
    s = make_stop_case(67)
    want = call_stop(ref.stop_check, s)
    for r in (0, 3, 30, 66):
        one = {k: v[r: r + 1] for k, v in s.items()}
        got = call_stop(rf.stop_check, _on(one, cuda_device))
        assert all(got[k] == want[k][r: r + 1] for k in got), r


def test_window_rows_as_the_engine_builds_them(cuda_device):
    """S slots, W window rows each: row (s, j) has the slot's context, ``win[s]`` as its
    extra tokens, ``n_extra = j + 1``, and is active iff ``j < n_win[s]`` and the slot is."""
    S, W, V = 6, 5, 50257
    c, _ = _case(V, S, seed=3)
    g = torch.Generator().manual_seed(9)
    win = torch.randint(0, 5, (S, W), generator=g) * (V // 6)
    win[1] = win[1, 0]  # a window of one repeated token
    n_win = torch.tensor([5, 1, 0, 3, 5, 2], dtype=torch.int32)
    slot_active = torch.tensor([1, 1, 1, 0, 1, 1], dtype=torch.uint8)
    w = dict(c)
    for k in NAMES:  # one context row per slot
        w[k] = c[k][:S].clone()
    w["n_out"].clamp_(0, WIDTH), w["prompt_len"].clamp_(0, WIDTH)
    w["ngram"][0], w["ngram"][1], w["ngram"][4] = 2, 1, 3
    w["bad_len"][0, 2], w["bad"][0, 2, :3] = 3, torch.tensor([int(win[0, 0]), int(win[0, 1]), 77],
                                                            dtype=torch.int32)
    w["rows"] = torch.arange(S, dtype=torch.int32).repeat_interleave(W)
    w["extra"] = win.unsqueeze(1).expand(S, W, W).reshape(S * W, W).contiguous()
    w["n_extra"] = torch.arange(1, W + 1, dtype=torch.int32).repeat(S)
    live = (torch.arange(W).unsqueeze(0) < n_win.unsqueeze(1)) & slot_active.bool().unsqueeze(1)
    w["active"] = live.to(torch.uint8).view(S * W)
    w["logits"] = (torch.randn(S * W, V, generator=g) * 4).to(torch.bfloat16)
    want = call(ref.seq_ban, w)
    # the banned sequence's prefix is the window's first two tokens: row 1 of slot 0 only
    assert [bool(want[j, 77] == float("-inf")) for j in range(W)] == [False, True, False, False,
                                                                      False]
    buf = torch.full((S, W, 50304), float("nan"), dtype=torch.bfloat16)
    buf.view(S * W, -1)[:, :V] = w["logits"]
    gbuf = buf.to(cuda_device)
    call(rf.seq_ban, _on(w, cuda_device), gbuf.view(S * W, -1)[:, :V])
    got = gbuf.cpu().view(S * W, -1)
    assert torch.equal(_raw(got[:, :V]), _raw(want)) and got[:, V:].isnan().all()
    untouched = ~live.view(S * W)
    assert torch.equal(_raw(got[untouched, :V]), _raw(w["logits"][untouched]))
    assert (_raw(want[live.view(S * W)]) != _raw(w["logits"][live.view(S * W)])).any(1).sum() > 5


def test_other_inputs_take_the_reference(cuda_device):
    """fp32 logits: the same results."""
    c, _ = _case(509, 5)
    got = call(rf.seq_ban, _on(c, cuda_device), c["logits"].float().to(cuda_device))
    assert torch.equal(got.cpu().view(torch.int32),
                       call(ref.seq_ban, c, c["logits"].float()).view(torch.int32))


def test_one_capture_serves_changing_inputs(cuda_device):
    dev, V, B = cuda_device, 50257, 5
    cases = [_case(V, B, seed=s) for s in (11, 12, 13)]
    ruleless = {k: v.clone() if isinstance(v, torch.Tensor) else v
                for k, v in cases[1][0].items()}
    ruleless["ngram"].zero_(), ruleless["bad_len"].zero_()  # ruled rows become rule-free
    cases.append((ruleless, call(ref.seq_ban, ruleless)))
    stops = [make_stop_case(B + 3, seed=s, cap=WIDTH) for s in (1, 2, 3, 4)]
    static = _on(cases[0][0], dev)
    sstat = _on(stops[0], dev)
    buf = torch.zeros(B, 50304, device=dev, dtype=torch.bfloat16)
    static["logits"] = buf[:, :V]

    def step():
        call(rf.seq_ban, static, static["logits"])
        rf.stop_check(*(sstat[k] for k in STOP_NAMES), active=sstat["active"],
                      lens=sstat["lens"], done=sstat["done"])

    step()  # warm-up
    graph = CapturedStep(step, dev)
    for (c, want), s in zip(cases, stops):
        for k, v in c.items():
            if isinstance(v, torch.Tensor):
                static[k].copy_(v)
        for k, v in s.items():
            sstat[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_raw(buf[:, :V].cpu()), _raw(want))
        assert not buf[:, V:].any()
        swant = call_stop(ref.stop_check, s)
        assert {k: sstat[k].tolist() for k in swant} == swant
    assert torch.equal(_raw(cases[-1][1]), _raw(ruleless["logits"]))


# ------------------------------------------------------------------ the engine, generate
def _cfg():
    return dataclasses.replace(GPT2Config.tiny(), n_embd=128, n_head=2, n_positions=256,
                               init_std=0.2)


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(0)
    return GPT2(_cfg()).eval().to(dev, torch.bfloat16)


EOS = 7
# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, continues the prefix,
# logprobs, rules)
MIX = [(1, 24, 0.0, None, None, 3, True, 5, dict(no_repeat_ngram_size=2)),
       (150, 9, 0.8, 5, None, 11, False, 2, dict()),
       (17, 16, 1.3, 50, 0.9, 2, True, None, dict(no_repeat_ngram_size=1, stop=[[5], [6, 7]])),
       (70, 3, 0.8, None, 0.9, 7, True, 0, dict(bad_words=[[9], [1, 2]])),
       (9, 20, 1.3, None, None, -4, False, 5, dict(no_repeat_ngram_size=0)),
       (130, 12, 0.0, 5, None, 0, True, 3, dict(no_repeat_ngram_size=3, bad_words=[3, 4]))]


def _drive(model, graph, speculate, rules=True, stops=None):
    g = torch.Generator().manual_seed(5)
    prefix = torch.randint(0, 512, (70,), generator=g).tolist()
    prompts = [torch.randint(0, 512, (m[0],), generator=g).tolist() for m in MIX]
    kw = {} if graph else {"graph": False}
    eng = GPT2Engine(model, slots=3, max_len=256, poll_every=2, prefix_slots=1, prefill_chunk=64,
                     eos_token_id=EOS, speculate=speculate, logprobs=5, sequence_rules=rules,
                     **kw)
    assert (eng._graph is not None) == graph
    pid = eng.add_prefix(prefix)
    rids = []
    for i, (p, m) in enumerate(zip(prompts, MIX)):
        r = dict(m[8]) if rules else {}
        if stops and i in stops:
            r["stop"] = stops[i]
        rids.append(eng.submit(p, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                               prefix=pid if m[6] else None, logprobs=m[7], **r))
    got = eng.run(logprobs=True)
    assert not eng.has_work() and eng.num_filling == 0
    return [got[r] for r in rids]


@pytest.mark.parametrize("speculate", [0, 4])
def test_engine_with_rules_graph_equals_eager(cuda_device, speculate):
    model = _model(cuda_device)
    free = _drive(model, True, speculate)
    # stops taken from the runs themselves, so that they act: requests 0 and 5 end early
    t0, t5 = free[0][0], free[5][0]
    h0, h5 = max(1, len(t0) // 2), len(t5) // 2
    stops = {0: [t0[h0 - 1: h0 + 1]], 5: [[t5[h5]]]}
    graphed = _drive(model, True, speculate, stops=stops)
    eager = _drive(model, False, speculate, stops=stops)
    for (tg, ig), (te, ie), m in zip(graphed, eager, MIX):
        assert tg == te
        if m[7] is None:
            assert ig is None and ie is None
            continue
        assert ig["top_ids"] == ie["top_ids"]
        for k in ("logprobs", "top_logprobs"):  # (floats from the fp32 tables: == is bitwise)
            assert torch.equal(torch.tensor(ig[k], dtype=torch.float64),
                               torch.tensor(ie[k], dtype=torch.float64)), k
    assert len(graphed[0][0]) <= h0 + 1 and graphed[0][0] == t0[: len(graphed[0][0])]
    assert len(graphed[5][0]) <= h5 + 1 and graphed[5][0] == t5[: len(graphed[5][0])]
    assert len(graphed[0][0]) < len(t0) or len(graphed[5][0]) < len(t5)
    # the rules did act, and the requests without any got the tokens they always got
    plain = _drive(model, True, speculate, rules=False)
    assert [t for t, _ in plain] != [t for t, _ in free]
    for i in (1, 4):
        assert plain[i][0] == graphed[i][0]
    assert 9 not in graphed[3][0]
    body = [t for t in graphed[2][0] if t != EOS]
    assert len(set(body)) == len(body)  # n = 1


def test_generate_with_rules_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 512, (3, 40), generator=g).to(cuda_device)
    kw = dict(lens=[40, 7, 22], temperature=[0.0, 0.8, 1.3], top_k=[0, 5, 0],
              top_p=[1.0, 1.0, 0.9], seeds=[4, 5, 6], eos_token_id=EOS, logprobs=3)
    plain = model.generate(idx, 20, graph=True, **kw)
    rules = dict(no_repeat_ngram_size=[2, 0, 3], bad_words=[None, [[int(plain[0][1, 0])]], [11]])
    base = model.generate(idx, 20, graph=True, **kw, **rules)[0].tolist()
    rules["stop"] = [None, None, [[base[2][9]]]]  # row 2 ends at its tenth token at the latest
    eager = model.generate(idx, 20, **kw, **rules)
    graphed = model.generate(idx, 20, graph=True, **kw, **rules)
    for a, b in zip(eager, graphed):
        a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
        assert torch.equal(a, b)
    toks = graphed[0].tolist()
    assert not torch.equal(plain[0], graphed[0])
    assert toks[1][0] != int(plain[0][1, 0]) and 11 not in toks[2]
    assert toks[:2] == base[:2]
    n = min(i for i, t in enumerate(base[2]) if t in (base[2][9], EOS)) + 1
    assert n <= 10 and toks[2] == base[2][:n] + [EOS] * (20 - n)
