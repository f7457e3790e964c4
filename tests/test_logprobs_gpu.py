"""The token-logprobs kernel (ops/csrc/logprobs.hip, ``rf.token_logprobs``) against
``ref.token_logprobs`` in fp64 on the stored bf16 values: ids exact (ties included), values
within ``4e-6 + |ref| * 2^-23``; bitwise repeatability, independence of a row from its
batch, byte-exact placement, one capture over changing inputs; then the bf16 engine with
``logprobs=5`` (graph == eager bit for bit, plain and speculative; accuracy against the fp32
model no worse than twice ``model.score``'s) and ``generate(seeds=, graph=True, logprobs=3)``.

The bound. The kernel evaluates ``lse`` and the differences in fp64 and rounds each result
to fp32 once: ``|lp| * 2^-24``, inside the ``|ref| * 2^-23`` term. What is left is the
relative error of the fixed-point sum, which is the error of ``lse``. A weight is
``exp2(a)``, ``a = (x - max) * log2(e)`` in fp32: the subtraction and the product round by
``2^-24`` each, so ``a`` is off by at most ``|a| * 2^-23`` and the weight by the factor
``ln 2 * |a| * 2^-23``; ``v_exp_f32`` and the scaling add about ``2^-22``. Weights below
``2^-41`` of the maximum's round to nothing, so ``|a| <= 41`` where it matters: at most
``41 * 0.693 * 2^-23 + 2^-22 = 3.6e-6`` relative for every term, hence for the sum. The
rounding to ``2^-40`` fixed point adds at most ``2^18 * 2^-41 = 1.2e-7`` of the maximum's
weight. Together under 4e-6, tighter than the 1e-5 the sampler's test allows for the same
sum. Worst observed on an MI355X: 1.49e-6 (profiles/r16/logprobs.md)."""

import dataclasses
import functools

import pytest
import torch
from test_token_logprobs import fresh_tables, placement_case, planted_rows

from ray_amd.models.gpt2 import GPT2, GPT2Config
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.ops.graph_lock import CapturedStep

pytestmark = pytest.mark.gpu

VS = (1, 7, 8, 9, 509, 50257)
BS = (1, 5, 67)
TOPS = (0, 1, 8)
WORST = {"ratio": 0.0, "abs": 0.0}  # the largest error seen, as a fraction of the bound


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def _case(V, B):
    """``randn * 4`` rounded to bf16 (at V 50257 the top 8 then hold ties), tokens in range
    but one, and the fp64 reference's top 8. CPU tensors, computed once."""
    g = torch.Generator().manual_seed(1000 * B + V)
    x = (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16)
    tok = torch.randint(0, V, (B,), generator=g)
    if B >= 5:
        tok[3] = V  # out of range: NaN
        tok[4] = int(x[4].float().argmin())
    want = ref.token_logprobs(x.double(), tok, 8)
    return x, tok, want


def _layouts(x, dev):
    """The rows as a contiguous tensor, as ``[:, :V]`` of a buffer padded like the LM head's
    (50304 wide for GPT-2's V) and as a slice that starts 3 elements in; the padding and the
    bytes before and after a sliced row hold NaN."""
    B, V = x.shape
    yield "contiguous", x.to(dev)
    wide = torch.full((B, -(-(V + 1) // 128) * 128), float("nan"), dtype=torch.bfloat16)
    wide[:, :V] = x
    yield "padded", wide.to(dev)[:, :V]
    odd = torch.full((B, V + 16), float("nan"), dtype=torch.bfloat16)
    odd[:, 3: 3 + V] = x
    yield "sliced", odd.to(dev)[:, 3: 3 + V]


def _check(got, want, n, what):
    lp, ids, tlp = (t.cpu() for t in got)
    wlp, wids, wtlp = want[0], want[1][:, :n], want[2][:, :n]
    assert lp.dtype == torch.float32 and ids.dtype == torch.int32 and tlp.dtype == torch.float32
    assert torch.equal(ids, wids), what
    for a, b in ((lp, wlp), (tlp, wtlp)):
        a = a.double()
        fin = torch.isfinite(b)
        assert torch.equal(a[~fin].nan_to_num(nan=12345.0), b[~fin].nan_to_num(nan=12345.0)), what
        if fin.any():
            err = (a[fin] - b[fin]).abs()
            bound = 4e-6 + b[fin].abs() * 2.0 ** -23
            ratio = (err / bound).max().item()
            if ratio > WORST["ratio"]:
                WORST.update(ratio=ratio, abs=err.max().item())
            assert ratio <= 1.0, (what, err.max().item())


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_kernel_against_fp64_reference(cuda_device, V, B):
    x, tok, want = _case(V, B)
    if V == 50257:  # the order rule is exercised: equal values inside the top 8
        top = x.double().sort(-1, descending=True).values[:, :8]
        assert (top[:, 1:] == top[:, :-1]).any()
    for name, rows in _layouts(x, cuda_device):
        assert name == "contiguous" or not rows.is_contiguous() or B == 1
        for n in TOPS:
            got = rf.token_logprobs(rows, tok.to(cuda_device), n)
            _check(got, want, n, (V, B, name, n))
            again = rf.token_logprobs(rows, tok.to(cuda_device), n)  # the same bits every run
            for a, b in zip(got, again):
                assert torch.equal(_bits(a), _bits(b)), (V, B, name, n)
    print(f"V {V} B {B}: worst error so far {WORST['abs']:.3e}, {WORST['ratio']:.3f} of the "
          "bound")


def test_vocab_size_ignores_the_tail(cuda_device):
    x, tok, want = _case(509, 5)
    wide = torch.cat([x, torch.full((5, 11), 300.0, dtype=torch.bfloat16)], 1)
    wide[:, 511] = float("nan")
    got = rf.token_logprobs(wide.to(cuda_device), tok.to(cuda_device), 8, vocab_size=509)
    _check(got, want, 8, "tail")


def test_planted_rows(cuda_device):
    x, tok = planted_rows()
    want = ref.token_logprobs(x.double(), tok, 4)
    got = rf.token_logprobs(x.to(cuda_device, torch.bfloat16), tok.to(cuda_device), 4)
    _check(got, want, 4, "planted")
    assert got[1].cpu().tolist()[:2] == [[2, 5, 9, 7], [0, 1, 2, 3]]
    # V = 1 and V < top_n: the (-1, -inf) padding
    one = rf.token_logprobs(x[:, :1].to(cuda_device, torch.bfloat16).contiguous(),
                            torch.zeros(6, dtype=torch.int64, device=cuda_device), 3)
    assert one[1].cpu().tolist() == [[0, -1, -1]] * 6
    assert one[2].cpu()[:, 1:].tolist() == [[float("-inf")] * 2] * 6
    assert one[0].cpu()[[0, 1, 3, 4]].tolist() == [0.0] * 4  # lse of one element: itself


def test_a_row_alone_and_among_others(cuda_device):
    x, tok, _ = _case(50257, 67)
    dev = cuda_device
    all_rows = rf.token_logprobs(x.to(dev), tok.to(dev), 8)
    for b, at in ((0, 41), (66, 5)):
        others = torch.roll(x, at - b, 0)  # row b sits at index `at`, among 66 others
        assert torch.equal(others[at], x[b])
        moved = rf.token_logprobs(others.to(dev), torch.roll(tok, at - b, 0).to(dev), 8)
        alone = rf.token_logprobs(x[b: b + 1].to(dev), tok[b: b + 1].to(dev), 8)
        # alone in a buffer whose row start is not 16-byte aligned
        odd = torch.zeros(1, 50257 + 8, dtype=torch.bfloat16)
        odd[:, 5: 5 + 50257] = x[b]
        shifted = rf.token_logprobs(odd.to(dev)[:, 5: 5 + 50257], tok[b: b + 1].to(dev), 8)
        for a, m, s, w in zip(alone, moved, shifted, all_rows):
            assert torch.equal(_bits(a[0]), _bits(w[b]))
            assert torch.equal(_bits(m[at]), _bits(w[b]))
            assert torch.equal(_bits(s[0]), _bits(w[b]))


@pytest.mark.parametrize("n", [0, 3])
def test_placement_and_skips_are_byte_exact(cuda_device, n):
    x, tok, rows, cols, active, R, cap = placement_case()
    dev = cuda_device
    xb = x.to(torch.bfloat16)
    dense = rf.token_logprobs(xb.to(dev), tok.to(dev), n)
    for act in (active, None):
        want = fresh_tables(R, cap, n)
        ref.token_logprobs(xb.float(), tok, n, None, want, rows, cols, act)
        out = fresh_tables(R, cap, n, dev)
        res = rf.token_logprobs(xb.to(dev), tok.to(dev), n, out=out, rows=rows.to(dev),
                                cols=cols.to(dev), active=None if act is None else act.to(dev))
        assert res is out
        # the kernel touches exactly the entries the reference touches (the fill values are
        # no results), writes the dense call's bits there and the reference's ids
        hit = [b for b in range(8) if (act is None or act[b]) and 0 <= rows[b] < R
               and 0 <= cols[b] < cap]
        assert hit == ([0, 3] if act is not None else [0, 1, 3, 7])
        for t, d, w, f in zip(out, dense, want, fresh_tables(R, cap, n)):
            t, expect = t.cpu(), f.clone()
            for b in hit:
                expect[rows[b], cols[b]] = d[b].cpu()
            assert torch.equal(_bits(t), _bits(expect))
            assert torch.equal(_bits(t) != _bits(f), _bits(w) != _bits(f))
            if t.dtype == torch.int32:
                assert torch.equal(t, w)


def test_argument_checks(cuda_device):
    dev = cuda_device
    x = torch.zeros(4, 64, device=dev, dtype=torch.bfloat16)
    tok = torch.zeros(4, dtype=torch.int64, device=dev)
    out = fresh_tables(3, 5, 2, dev)
    i32 = torch.zeros(4, dtype=torch.int32, device=dev)
    for bad in (
        lambda: rf.token_logprobs(x, tok, 9),
        lambda: rf.token_logprobs(x, tok.cpu()),
        lambda: rf.token_logprobs(x, tok.int()),
        lambda: rf.token_logprobs(x, tok, vocab_size=65),
        lambda: rf.token_logprobs(x, tok, 2, out=out, rows=i32.cpu(), cols=i32),
        lambda: rf.token_logprobs(x, tok, 2, out=out, rows=i32, cols=i32[:3]),
        lambda: rf.token_logprobs(x, tok, 2, out=(out[0].cpu(),) + out[1:], rows=i32, cols=i32),
        lambda: rf.token_logprobs(x, tok, 2, out=(out[0].t(),) + out[1:], rows=i32, cols=i32),
        lambda: rf.token_logprobs(x, tok, 2, out=(out[0], out[1].long(), out[2]), rows=i32,
                                  cols=i32),
        lambda: rf.token_logprobs(x, tok, 2, out=out, rows=i32, cols=i32, active=i32),
        lambda: rf.token_logprobs(x, tok, 1, out=out, rows=i32, cols=i32),
    ):
        with pytest.raises(ValueError):
            bad()
    # the library's own checks
    L = _lib.lib()
    assert L.ra_token_logprobs_max_top() == rf.LOGPROB_MAX_TOP
    lp = torch.zeros(4, device=dev)
    st = _lib.stream_ptr()
    args = lambda **kw: [kw.get("logits", x.data_ptr()), kw.get("stride", 64), tok.data_ptr(),  # noqa: E731
                         None, None, None, lp.data_ptr(), None, None, kw.get("B", 4),
                         kw.get("V", 64), kw.get("n", 0), kw.get("R", 4), 1, st]
    assert L.ra_token_logprobs(*args()) == 0
    for kw in (dict(B=0), dict(V=0), dict(V=(1 << 18) + 1), dict(stride=63), dict(n=9),
               dict(n=1), dict(R=3), dict(logits=x.data_ptr() + 1), dict(logits=None)):
        assert L.ra_token_logprobs(*args(**kw)) != 0, kw
    torch.cuda.synchronize()


def test_one_capture_serves_changing_inputs(cuda_device):
    dev = cuda_device
    B, V, R, cap, n = 6, 50257, 4, 7, 5
    g = torch.Generator().manual_seed(77)

    def inputs():
        return dict(x=(torch.randn(B, V, generator=g) * 4).to(torch.bfloat16),
                    tok=torch.randint(0, V, (B,), generator=g),
                    rows=torch.randint(-1, R + 1, (B,), generator=g, dtype=torch.int32),
                    cols=torch.randint(-1, cap + 1, (B,), generator=g, dtype=torch.int32),
                    active=torch.randint(0, 2, (B,), generator=g, dtype=torch.uint8))

    static = {k: v.to(dev) for k, v in inputs().items()}
    buf = torch.zeros(B, 50304, device=dev, dtype=torch.bfloat16)
    out = fresh_tables(R, cap, n, dev)

    def step():
        rf.token_logprobs(buf[:, :V], static["tok"], n, out=out, rows=static["rows"],
                          cols=static["cols"], active=static["active"])

    buf[:, :V].copy_(static["x"])
    step()  # warm-up
    graph = CapturedStep(step, dev)
    for _ in range(3):
        new = inputs()
        # distinct targets, so that the expectation does not depend on an order of writes
        new["rows"][:4] = torch.arange(4, dtype=torch.int32)
        new["cols"][4:] = -1
        for k, v in new.items():
            (buf[:, :V] if k == "x" else static[k]).copy_(v)
        for t, f in zip(out, fresh_tables(R, cap, n, dev)):
            t.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        dense = rf.token_logprobs(new["x"].to(dev), new["tok"].to(dev), n)
        want = fresh_tables(R, cap, n)
        for b in range(B):
            r, c = int(new["rows"][b]), int(new["cols"][b])
            if new["active"][b] and 0 <= r < R and 0 <= c < cap:
                for w, d in zip(want, dense):
                    w[r, c] = d[b].cpu()
        for t, w in zip(out, want):
            assert torch.equal(_bits(t.cpu()), _bits(w))


# ------------------------------------------------------------------ the engine, generate
def _cfg():
    return dataclasses.replace(GPT2Config.tiny(), n_embd=128, n_head=2, n_positions=256,
                               init_std=0.2)


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(0)
    return GPT2(_cfg()).eval().to(dev, torch.bfloat16)


# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, continues the prefix,
# logprobs): the mix of test_spec_gpu.py
MIX = [(1, 24, 0.0, None, None, 3, True, 5), (150, 9, 0.8, 5, None, 11, False, 2),
       (17, 16, 1.3, 50, 0.9, 2, True, None), (70, 3, 0.8, None, 0.9, 7, True, 0),
       (9, 20, 1.3, None, None, -4, False, 5), (130, 12, 0.0, 5, None, 0, True, 3)]
EOS = 7


def _drive(model, graph, speculate, logprobs=5):
    g = torch.Generator().manual_seed(5)
    prefix = torch.randint(0, 512, (70,), generator=g).tolist()
    prompts = [torch.randint(0, 512, (m[0],), generator=g).tolist() for m in MIX]
    kw = {} if graph else {"graph": False}
    eng = GPT2Engine(model, slots=3, max_len=256, poll_every=2, prefix_slots=1, prefill_chunk=64,
                     eos_token_id=EOS, speculate=speculate, logprobs=logprobs, **kw)
    assert (eng._graph is not None) == graph
    pid = eng.add_prefix(prefix)
    rids = [eng.submit(p, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                       prefix=pid if m[6] else None,
                       **({} if logprobs is None else {"logprobs": m[7]}))
            for p, m in zip(prompts, MIX)]
    got = eng.run(logprobs=logprobs is not None)
    assert not eng.has_work() and eng.num_filling == 0
    full = [(prefix if m[6] else []) + p for p, m in zip(prompts, MIX)]
    return [got[r] for r in rids], full


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("speculate", [0, 4])
def test_engine_logprobs_graph_equals_eager_and_are_accurate(cuda_device, speculate):
    """Graph == eager bit for bit, tokens those of the engine without logprobs, and against
    the fp32 model teacher-forced on prompt + output the engine's logprobs err at most twice
    as much as the bf16 ``model.score`` of the same sequence: both are bf16 roundings of one
    computation in another order (a wrong position, column or token errs by order 1)."""
    dev, cfg = cuda_device, _cfg()
    model = _model(dev)
    graphed, full = _drive(model, True, speculate)
    eager, _ = _drive(model, False, speculate)
    plain, _ = _drive(model, True, speculate, logprobs=None)
    assert [t for t, _ in graphed] == plain
    for (tg, ig), (te, ie), m in zip(graphed, eager, MIX):
        assert tg == te
        if m[7] is None:
            assert ig is None and ie is None
            continue
        assert ig["top_ids"] == ie["top_ids"] and all(len(r) == m[7] for r in ig["top_ids"])
        for k in ("logprobs", "top_logprobs"):  # (floats from the fp32 tables: == is bitwise)
            assert torch.equal(torch.tensor(ig[k], dtype=torch.float64),
                               torch.tensor(ie[k], dtype=torch.float64)), k
        assert len(ig["logprobs"]) == len(tg)
        if m[2] == 0.0 and m[7]:
            assert [r[0] for r in ig["top_ids"]] == tg
    m32 = GPT2(cfg).eval()
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    eng_lp, score_lp, want_lp = [], [], []
    for (toks, info), p in zip(graphed, full):
        if info is None:
            continue
        seq = torch.tensor([p + toks])
        want_lp.append(m32.score(seq)[0, len(p):].double())
        score_lp.append(model.score(seq.to(dev))[0, len(p):].double().cpu())
        eng_lp.append(torch.tensor(info["logprobs"], dtype=torch.float64))
    want = torch.cat(want_lp)
    e_eng, e_score = _rel(torch.cat(eng_lp), want), _rel(torch.cat(score_lp), want)
    print(f"speculate={speculate}: engine logprob rel err {e_eng:.3e}, model.score rel err "
          f"{e_score:.3e} over {want.numel()} tokens")
    assert torch.isfinite(want).all() and e_eng <= 2 * e_score, (e_eng, e_score)


def test_generate_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 512, (3, 40), generator=g).to(cuda_device)
    kw = dict(lens=[40, 7, 22], temperature=[0.0, 0.8, 1.3], top_k=[0, 5, 0],
              top_p=[1.0, 1.0, 0.9], seeds=[4, 5, 6], eos_token_id=EOS, logprobs=3)
    eager = model.generate(idx, 20, **kw)
    graphed = model.generate(idx, 20, graph=True, **kw)
    plain = model.generate(idx, 20, graph=True, **{**kw, "logprobs": None})
    assert torch.equal(graphed[0], plain)
    for a, b in zip(eager, graphed):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.isfinite(graphed[1]).all() and (graphed[2] >= 0).all()
    assert torch.equal(graphed[2][0, :, 0].long(), graphed[0][0])  # the greedy row
