"""The logit-processor kernel (ops/csrc/logit_proc.hip, ``rf.logit_process``) against
``ref.logit_process`` computed on the CPU from the same bf16 bytes: BIT EQUALITY on the whole
buffer, padding and sentinels included (the reference itself is checked bit for bit against
scalar loops in test_logit_process.py, so there is no tolerance anywhere). Then
repeatability, a row alone against the row in its batch, the window rows the speculative
step builds, one capture over changing inputs, and the bf16 engine and ``generate`` with
controls: graph == eager bit for bit."""

import dataclasses
import functools

import pytest
import torch
from test_logit_process import NAMES, call, make_case, skipped_rows

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
    return c, call(ref.logit_process, c)


def _on(c, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in c.items()}


def _layouts(x):
    """``(name, buffer, view_of)``: the rows as a contiguous tensor, as ``[:, :V]`` of a
    buffer padded like the LM head's and as a slice that starts 3 elements in; the padding
    and the bytes before and after a sliced row hold NaN sentinels (0x7FA5: not the
    canonical NaN, so a rewrite would show)."""
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
    if B == 67:  # the case does exercise the rules and the skips
        skipped = skipped_rows(c)
        assert len(skipped) >= 5 and not changed[skipped].any()
        assert changed.sum() > (B - len(skipped)) // 2
        assert int(c["prompt_len"][0]) == WIDTH and int(c["n_out"][0]) == WIDTH
        assert want.isinf().any() and (V == 1 or want.isnan().any())
    for (name, buf, view), (_, wbuf, _) in zip(_layouts(c["logits"]), _layouts(want)):
        for attempt in range(2):  # the same bits every run
            gbuf = buf.to(cuda_device)
            rows = view(gbuf)
            assert name == "contiguous" or B == 1 or not rows.is_contiguous()
            assert call(rf.logit_process, d, rows) is rows
            assert torch.equal(_raw(gbuf.cpu()), _raw(wbuf)), (V, B, name, attempt)


def test_a_row_alone_and_among_others(cuda_device):
    c, want = _case(50257, 67)
    live = [b for b in range(67) if b not in skipped_rows(c)]
    for b in (live[0], live[len(live) // 2], live[-1], 0):
        one = {k: v for k, v in c.items()}
        for k in ("logits", "rows", "extra", "n_extra", "active"):
            one[k] = c[k][b: b + 1]
        got = call(rf.logit_process, _on(one, cuda_device))
        assert torch.equal(_raw(got.cpu()), _raw(want[b: b + 1])), b


def test_window_rows_as_the_engine_builds_them(cuda_device):
    """S slots, W window rows each: row (s, j) has the slot's context, ``win[s]`` as its
    extra tokens, ``n_extra = j + 1``, and is active iff ``j < n_win[s]`` and the slot is."""
    S, W, V = 6, 5, 50257
    c, _ = _case(V, S, seed=3)
    g = torch.Generator().manual_seed(9)
    win = torch.randint(0, 48, (S, W), generator=g) * 1000
    win[1] = win[1, 0]  # a window of one repeated token
    n_win = torch.tensor([5, 1, 0, 3, 5, 2], dtype=torch.int32)
    slot_active = torch.tensor([1, 1, 1, 0, 1, 1], dtype=torch.uint8)
    w = dict(c)
    for k in NAMES:  # one context row per slot
        w[k] = c[k][:S].clone()
    w["n_out"].clamp_(0, WIDTH), w["prompt_len"].clamp_(0, WIDTH), w["n_bias"].clamp_(0, 64)
    w["min_new"][0] = int(w["n_out"][0]) + 3  # the ban ends inside slot 0's window
    w["rows"] = torch.arange(S, dtype=torch.int32).repeat_interleave(W)
    w["extra"] = win.unsqueeze(1).expand(S, W, W).reshape(S * W, W).contiguous()
    w["n_extra"] = torch.arange(1, W + 1, dtype=torch.int32).repeat(S)
    live = (torch.arange(W).unsqueeze(0) < n_win.unsqueeze(1)) & slot_active.bool().unsqueeze(1)
    w["active"] = live.to(torch.uint8).view(S * W)
    w["logits"] = (torch.randn(S * W, V, generator=g) * 4).to(torch.bfloat16)
    want = call(ref.logit_process, w)
    eos = w["eos_token_id"]
    assert [bool(want[j, eos] == float("-inf")) for j in range(W)] == [True, True, False, False,
                                                                       False]
    buf = torch.full((S, W, 50304), float("nan"), dtype=torch.bfloat16)
    buf.view(S * W, -1)[:, :V] = w["logits"]
    gbuf = buf.to(cuda_device)
    call(rf.logit_process, _on(w, cuda_device), gbuf.view(S * W, -1)[:, :V])
    got = gbuf.cpu().view(S * W, -1)
    assert torch.equal(_raw(got[:, :V]), _raw(want)) and got[:, V:].isnan().all()
    untouched = ~live.view(S * W)
    assert torch.equal(_raw(got[untouched, :V]), _raw(w["logits"][untouched]))


def test_other_inputs_take_the_reference(cuda_device):
    """fp32 logits, and tables beyond the kernel's context limit: the same results."""
    c, _ = _case(509, 5)
    d = _on(c, cuda_device)
    got = call(rf.logit_process, d, c["logits"].float().to(cuda_device))
    assert torch.equal(got.cpu().view(torch.int32),
                       call(ref.logit_process, c, c["logits"].float()).view(torch.int32))
    long = dict(c)
    pad = rf.LOGIT_PROCESS_MAX_CONTEXT - WIDTH  # P + cap + W + NB + 1 is now past the limit
    long["prompt"] = torch.cat([c["prompt"], torch.zeros(8, pad, dtype=torch.int32)], 1)
    got = call(rf.logit_process, _on(long, cuda_device))
    assert torch.equal(_raw(got.cpu()), _raw(call(ref.logit_process, long)))


def test_one_capture_serves_changing_inputs(cuda_device):
    dev, V, B = cuda_device, 50257, 5
    cases = [_case(V, B, seed=s) for s in (11, 12, 13)]
    static = _on(cases[0][0], dev)
    buf = torch.zeros(B, 50304, device=dev, dtype=torch.bfloat16)
    static["logits"] = buf[:, :V]

    def step():
        call(rf.logit_process, static, static["logits"])

    step()  # warm-up
    graph = CapturedStep(step, dev)
    for c, want in cases:
        for k, v in c.items():
            if isinstance(v, torch.Tensor):
                static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_raw(buf[:, :V].cpu()), _raw(want))
        assert not buf[:, V:].any()


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
# logprobs, controls): the mix of test_logprobs_gpu.py with controls, neutral ones among them
MIX = [(1, 24, 0.0, None, None, 3, True, 5, dict(repetition_penalty=1.3, frequency_penalty=0.5)),
       (150, 9, 0.8, 5, None, 11, False, 2, dict()),
       (17, 16, 1.3, 50, 0.9, 2, True, None, dict(min_new_tokens=12, presence_penalty=0.7)),
       (70, 3, 0.8, None, 0.9, 7, True, 0, dict(logit_bias={5: 4.0, 9: float("-inf")})),
       (9, 20, 1.3, None, None, -4, False, 5, dict(repetition_penalty=1.0)),
       (130, 12, 0.0, 5, None, 0, True, 3,
        dict(repetition_penalty=0.8, logit_bias={i: -1.0 * i for i in range(64)},
             min_new_tokens=12))]


def _drive(model, graph, speculate, controls=True):
    g = torch.Generator().manual_seed(5)
    prefix = torch.randint(0, 512, (70,), generator=g).tolist()
    prompts = [torch.randint(0, 512, (m[0],), generator=g).tolist() for m in MIX]
    kw = {} if graph else {"graph": False}
    eng = GPT2Engine(model, slots=3, max_len=256, poll_every=2, prefix_slots=1, prefill_chunk=64,
                     eos_token_id=EOS, speculate=speculate, logprobs=5,
                     logit_processors=controls, **kw)
    assert (eng._graph is not None) == graph
    pid = eng.add_prefix(prefix)
    rids = [eng.submit(p, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                       prefix=pid if m[6] else None, logprobs=m[7], **(m[8] if controls else {}))
            for p, m in zip(prompts, MIX)]
    got = eng.run(logprobs=True)
    assert not eng.has_work() and eng.num_filling == 0
    return [got[r] for r in rids]


@pytest.mark.parametrize("speculate", [0, 4])
def test_engine_with_controls_graph_equals_eager(cuda_device, speculate):
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
    # the controls did act, and the requests without any got the tokens they always got
    plain = _drive(model, True, speculate, controls=False)
    assert [t for t, _ in plain] != [t for t, _ in graphed]
    for i in (1, 4):
        assert plain[i][0] == graphed[i][0]
    assert 9 not in graphed[3][0]  # the banned token
    for i in (2, 5):  # min_new_tokens 12: no EOS before the twelfth token
        assert EOS not in graphed[i][0][:12]


def test_generate_with_controls_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 512, (3, 40), generator=g).to(cuda_device)
    kw = dict(lens=[40, 7, 22], temperature=[0.0, 0.8, 1.3], top_k=[0, 5, 0],
              top_p=[1.0, 1.0, 0.9], seeds=[4, 5, 6], eos_token_id=EOS, logprobs=3)
    ctl = dict(repetition_penalty=[1.3, 1.0, 0.9], frequency_penalty=[0.5, 0.0, 0.0],
               presence_penalty=0.25, min_new_tokens=[0, 0, 15],
               logit_bias=[None, None, {11: float("-inf"), 3: 2.0}])
    eager = model.generate(idx, 20, **kw, **ctl)
    graphed = model.generate(idx, 20, graph=True, **kw, **ctl)
    for a, b in zip(eager, graphed):
        a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
        assert torch.equal(a, b)
    plain = model.generate(idx, 20, graph=True, **kw)
    assert not torch.equal(plain[0], graphed[0])
    assert EOS not in graphed[0][2, :15].tolist() and 11 not in graphed[0][2].tolist()
    assert torch.equal(graphed[2][0, :, 0].long(), graphed[0][0])  # the greedy row's top id
