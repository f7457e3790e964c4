"""The speculative-decoding kernels (ops/csrc/spec.hip: ``rf.spec_draft``, ``rf.spec_accept``)
bitwise against the plain-loop references, one capture of draft -> accept replayed over
changing inputs, ``GPT2.verify_step`` in bf16 against the fp32 model, and the engine with
``speculate=4``: graph run == eager run == second graph run.

Equality with the non-speculative engine is not asserted here: the verify pass and
``decode_step`` round bf16 in different orders, as chunked prefill already does
(test_attn_extend_gpu.py); tests/test_spec_decode.py asserts it in fp32."""

import dataclasses
import functools

import pytest
import torch

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache
from ray_amd.models.gpt2_engine import GPT2Engine
from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref
from ray_amd.ops.graph_lock import CapturedStep

pytestmark = pytest.mark.gpu

INACTIVE = -(1 << 30)
CAP = 300
PS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 299)  # around the 256-lane stride and the end
KS = (1, 4, 8)
NGRAMS = ((1, 1), (2, 4), (3, 8))


@pytest.fixture(scope="module", autouse=True)
def _need_lib(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


# ------------------------------------------------------------------ spec_draft
@functools.lru_cache(maxsize=None)
def _draft_case(S, seed=0):
    """S slots over a 3-token alphabet, slot s at p = PS[s % 10] (every p for S >= 10), ``hist``
    random from p on (stale contents), every kind of room, a few slots inactive or out of
    range. CPU tensors, computed once."""
    g = torch.Generator().manual_seed(100 * S + seed)
    lens = _i32([PS[(s + seed) % len(PS)] for s in range(S)])
    hist = torch.randint(0, 3, (S, CAP), generator=g, dtype=torch.int32)
    for s in range(S):
        hist[s, int(lens[s]):] = torch.randint(0, 1000, (CAP - int(lens[s]),), generator=g,
                                               dtype=torch.int32)
    tok0 = torch.randint(0, 3, (S,), generator=g)
    n_out = torch.randint(0, 5, (S,), generator=g, dtype=torch.int32)
    max_new = n_out + torch.randint(-1, 12, (S,), generator=g, dtype=torch.int32)
    max_new[::3] += 20
    active = torch.ones(S, dtype=torch.uint8)
    if S > 4:
        active[3] = 0
        lens[4] = CAP  # out of range: skipped like an inactive slot
    if S > 20:
        active[[11, 40]] = 0
        lens[17], lens[18] = -1, INACTIVE
    return tok0, hist, lens, n_out, max_new, active


def _run_draft(args, k, ngram, dev, win0):
    win, n_win = rf.spec_draft(*(t.to(dev) for t in args), k, *ngram, win=win0.to(dev),
                               n_win=torch.full((args[0].shape[0],), -7, dtype=torch.int32,
                                                device=dev))
    return win.cpu(), n_win.cpu()


@pytest.mark.parametrize("S", [1, 5, 67])
def test_spec_draft_bitwise(cuda_device, S):
    seen = set()
    for seed in range(10 if S == 1 else 2):  # S 1: one p per call
        args = _draft_case(S, seed)
        for k in KS:
            win0 = torch.full((S, k + 1), -7, dtype=torch.int64)
            for ngram in NGRAMS:
                want_w, want_n = ref.spec_draft(*args, k, *ngram, win0.clone(),
                                                torch.zeros(S, dtype=torch.int32))
                got_w, got_n = _run_draft(args, k, ngram, cuda_device, win0)
                assert torch.equal(got_n, want_n), (S, seed, k, ngram, got_n, want_n)
                assert torch.equal(got_w, want_w), (S, seed, k, ngram)
                again_w, again_n = _run_draft(args, k, ngram, cuda_device, win0)
                assert torch.equal(again_w, got_w) and torch.equal(again_n, got_n)
                seen.update(want_n.tolist())
    assert {1, 2} <= seen and (S == 1 or 0 in seen) and 9 in seen


# (hist[:p], tok0, room, active, the window for k 4 and ngram (2, 4)): the planted cases of
# tests/test_spec_decode.py
PLANTED = [
    ([0, 1, 2, 3, 4], 5, 9, 1, [5]),                                # no match
    ([7, 8, 1, 2, 3, 7], 8, 9, 1, [8, 1, 2, 3, 7]),                 # a match only at j = 0
    ([7, 8, 1, 7, 8, 2, 5, 7], 8, 9, 1, [8, 2, 5, 7, 8]),           # two: the later one wins
    ([1, 2, 3, 9, 5, 2, 3, 4, 1, 2], 3, 9, 1, [3, 9, 5, 2, 3]),     # n 3 at j 0 beats n 2 at j 5
    ([4, 6, 6], 6, 9, 1, [6, 6, 6, 6, 6]),                          # period 1
    ([3, 1, 2, 1], 2, 9, 1, [2, 1, 2, 1, 2]),                       # period 2
    ([7, 8, 1, 2, 3, 7], 8, 1, 1, [8]),                             # room 1
    ([7, 8, 1, 2, 3, 7], 8, 3, 1, [8, 1, 2]),                       # room 3
    ([7, 8, 1, 2, 3, 7], 8, 9, 0, None),                            # inactive
    ([7, 8, 1] * 5, 7, 9, 1, [7]),                                  # p = cap - 1
    # a long match that ends in the first wave's lanes beats a later, shorter one in another's
    ([1, 2, 3, 4] + [0] * 364 + [9, 3, 4] + [5] * 80 + [1, 2, 3], 4, 9, 1, [4, 0, 0, 0, 0]),
]


def test_spec_draft_planted_cases(cuda_device):
    for cap in (16, 500):
        cases = [c for c in PLANTED if len(c[0]) < cap and (cap == 16 or c[4] != [7])]
        S = len(cases)
        hist = torch.randint(0, 9, (S, cap), generator=torch.Generator().manual_seed(2),
                             dtype=torch.int32)
        for s, c in enumerate(cases):
            hist[s, : len(c[0])] = _i32(c[0])
        args = (torch.tensor([c[1] for c in cases]), hist, _i32([len(c[0]) for c in cases]),
                _i32(list(range(S))), _i32([s + c[2] for s, c in enumerate(cases)]),
                torch.tensor([c[3] for c in cases], dtype=torch.uint8))
        win0 = torch.full((S, 5), -7, dtype=torch.int64)
        win, n_win = _run_draft(args, 4, (2, 4), cuda_device, win0)
        for s, c in enumerate(cases):
            if c[4] is None:
                assert int(n_win[s]) == 0 and (win[s] == -7).all(), s
                continue
            assert win[s, : int(n_win[s])].tolist() == c[4], (cap, s, win[s], n_win[s])
            assert (win[s, len(c[4]):] == -7).all(), s
        want_w, want_n = ref.spec_draft(*args, 4, 2, 4, win0.clone(),
                                        torch.zeros(S, dtype=torch.int32))
        assert torch.equal(win, want_w) and torch.equal(n_win, want_n)


# ------------------------------------------------------------------ spec_accept
ACC_K, ACC_CAP, ACC_EOS = 4, 12, 99
ACC_ORDER = ("win", "n_win", "cand", "logits_win", "lens", "n_out", "max_new", "active", "out",
             "hist", "buf", "n_drafted", "n_accepted")


def _rand_bits(shape, g):
    """bf16 of random bit patterns: every kind of value, NaNs of every payload included."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32) \
        .to(torch.int16).view(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _accept_case(Vp, copies=1):
    """The edge cases of tests/test_spec_decode.py, one slot per line: (win, n_win, cand,
    n_out, max_new, lens, active), k = 4; ``copies`` times over with other logits."""
    w = [10, 11, 12, 13, 14]
    rows = [(w, 5, w[1: 1 + a] + [50] * (5 - a), 0, 9, 3, 1) for a in range(ACC_K + 1)]
    rows += [
        (w, 3, w[1:] + [50], 2, 9, 3, 1),                   # n_win stops a at 2
        ([ACC_EOS, 11, 12, 13, 14], 5, w[1:] + [50], 0, 9, 3, 1),          # EOS as tok0
        ([10, 11, ACC_EOS, 13, 14], 5, [11, ACC_EOS, 13, 14, 50], 1, 9, 3, 1),  # accepted EOS
        ([10, 11, ACC_EOS, 13, 14], 5, [11, 40, 13, 14, 50], 1, 9, 3, 1),  # a rejected EOS
        (w, 5, w[1:] + [50], 4, 6, 3, 1),                   # max_new cuts inside the run
        (w, 5, w[1:] + [50], 4, 9, 3, 1),                   # ... and exactly at its end
        (w, 0, w[1:] + [50], 1, 9, 3, 1),                   # n_win 0 on an active slot
        (w, ACC_K + 2, w[1:] + [50], 1, 9, 3, 1),           # n_win k + 2
        (w, 5, w[1:] + [50], 1, 9, 3, 0),                   # inactive
        (w, 5, w[1:] + [50], 1, 9, INACTIVE, 0),            # inactive and pinned already
        (w, 5, w[1:] + [50], ACC_CAP, 99, 3, 1),            # n_out = cap
        (w, 5, w[1:] + [50], -1, 9, 3, 1),                  # n_out < 0
        (w, 5, w[1:] + [50], 0, 9, ACC_CAP, 1),             # lens = cap
        (w, 5, w[1:] + [50], 0, 9, -1, 1),                  # lens < 0
        (w, 5, w[1:] + [50], ACC_CAP - 2, 99, 3, 1),        # cap - n_out cuts
        (w, 5, w[1:] + [50], 0, 99, ACC_CAP - 3, 1),        # cap - lens cuts
        (w, 1, [50] * 5, 0, 9, 3, 1),                       # no drafts: the plain step
    ]
    rows = rows * copies
    S = len(rows)
    g = torch.Generator().manual_seed(4 + Vp)
    col = lambda i, dt: torch.tensor([r[i] for r in rows], dtype=dt)  # noqa: E731
    return dict(
        win=col(0, torch.int64), n_win=col(1, torch.int32), cand=col(2, torch.int64),
        logits_win=_rand_bits((S, ACC_K + 1, Vp), g),
        lens=col(5, torch.int32), n_out=col(3, torch.int32), max_new=col(4, torch.int32),
        active=col(6, torch.uint8),
        out=torch.randint(-9, -1, (S, ACC_CAP), generator=g),
        hist=torch.randint(-9, -1, (S, ACC_CAP), generator=g, dtype=torch.int32),
        buf=_rand_bits((S, Vp), g),
        n_drafted=torch.arange(S, dtype=torch.int32),
        n_accepted=torch.arange(S, dtype=torch.int32) * 2)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.is_floating_point() else t


def _accept_both(case, dev, eos=ACC_EOS, rows=None):
    """(reference result on the CPU, kernel result) for the slots ``rows`` of ``case``."""
    pick = (lambda t: t) if rows is None else (lambda t: t[rows].contiguous())
    want = {k: pick(v).clone() for k, v in case.items()}
    ref.spec_accept(*(want[k] for k in ACC_ORDER), eos)
    got = {k: pick(v).to(dev) for k, v in case.items()}
    assert rf.spec_accept(*(got[k] for k in ACC_ORDER), eos_token_id=eos) is None
    return want, {k: v.cpu() for k, v in got.items()}


# 512: one pass of the 16-byte copy; 50304: GPT-2's padded rows, several passes and a ragged
# last one; 509 and 1004: no multiple of the 8-element vector, so rows start off 16-byte
# boundaries and move element by element
@pytest.mark.parametrize("Vp", [512, 50304, 509, 1004])
def test_spec_accept_bitwise(cuda_device, Vp):
    case = _accept_case(Vp)
    for eos in (ACC_EOS, None):
        want, got = _accept_both(case, cuda_device, eos)
        for k in ACC_ORDER:
            assert torch.equal(_bits(got[k]), _bits(want[k])), (Vp, eos, k)
    kept = [s for s in range(case["win"].shape[0]) if int(want["active"][s])]
    assert len(kept) >= 9
    for s in kept:  # (eos None) a surviving slot holds the logits at its new position
        m = int(want["n_out"][s]) - int(case["n_out"][s])
        assert torch.equal(_bits(got["buf"][s]), _bits(case["logits_win"][s, m - 1])), s
    gone = [s for s in range(case["win"].shape[0]) if not int(want["active"][s])]
    assert torch.equal(_bits(got["buf"][gone]), _bits(case["buf"][gone]))


def test_spec_accept_batch_mate_independence(cuda_device):
    case = _accept_case(512, copies=3)  # 66 slots
    S = case["win"].shape[0]
    assert S == 66
    _, wide = _accept_both(case, cuda_device)
    for s in (0, 4, 7, 9, 20, 43, 65):
        _, alone = _accept_both(case, cuda_device, rows=[s])
        for k in ACC_ORDER:
            assert torch.equal(_bits(alone[k][0]), _bits(wide[k][s])), (s, k)


def test_spec_kernels_argument_checks(cuda_device):
    d = _draft_case(5)
    args = [t.to(cuda_device) for t in d]
    with pytest.raises(ValueError):
        rf.spec_draft(*args, 9)
    with pytest.raises(ValueError):
        rf.spec_draft(*args, 4, 3, 2)
    with pytest.raises(ValueError):
        rf.spec_draft(args[0], args[1].cpu(), *args[2:], 4)
    with pytest.raises(ValueError):
        rf.spec_draft(*args, 4, win=torch.zeros(5, 10, dtype=torch.int64,
                                                 device=cuda_device)[:, ::2])
    c = {k: v.to(cuda_device) for k, v in _accept_case(512).items()}
    for name, bad in (("buf", c["buf"].t().contiguous().t()), ("lens", c["lens"].long()),
                      ("cand", c["cand"].cpu()), ("logits_win", c["logits_win"][:, :, :504])):
        with pytest.raises(ValueError):
            rf.spec_accept(*(bad if k == name else c[k] for k in ACC_ORDER))


# ------------------------------------------------------------------ one capture, many inputs
def test_one_capture_serves_changing_inputs(cuda_device):
    dev, S, k, Vp = cuda_device, 5, 4, 512
    g = torch.Generator().manual_seed(8)

    def inputs(seed):
        tok0, hist, lens, n_out, max_new, active = _draft_case(S, seed)
        lens = lens.clamp(max=CAP - 1)
        return dict(tok0=tok0, hist=hist, lens=lens, n_out=n_out, max_new=max_new, active=active,
                    cand=torch.randint(0, 3, (S, k + 1), generator=g),
                    logits_win=_rand_bits((S, k + 1, Vp), g), buf=_rand_bits((S, Vp), g),
                    out=torch.randint(-9, -1, (S, CAP), generator=g))

    def step(t):
        win, n_win = rf.spec_draft(t["tok0"], t["hist"], t["lens"], t["n_out"], t["max_new"],
                                   t["active"], k, 1, 3, win=t["win"], n_win=t["n_win"])
        rf.spec_accept(win, n_win, t["cand"], t["logits_win"], t["lens"], t["n_out"],
                       t["max_new"], t["active"], t["out"], t["hist"], t["buf"], t["n_drafted"],
                       t["n_accepted"], 2)

    def fresh(host):
        t = {k_: v.clone() for k_, v in host.items()}
        t.update(win=torch.zeros(S, k + 1, dtype=torch.int64), n_win=torch.zeros(S).int(),
                 n_drafted=torch.zeros(S).int(), n_accepted=torch.zeros(S).int())
        return t

    static = {k_: v.to(dev) for k_, v in fresh(inputs(0)).items()}
    step(static)  # warm-up
    graph = CapturedStep(lambda: step(static), dev)
    accepted = 0
    for seed in (3, 4, 5):
        want = fresh(inputs(seed))
        for name, v in want.items():
            static[name].copy_(v)
        step(want)  # CPU tensors: the references
        graph.replay()
        torch.cuda.synchronize()
        for name in want:
            assert torch.equal(_bits(static[name].cpu()), _bits(want[name])), (seed, name)
        accepted += int(want["n_accepted"].sum())
    assert accepted > 0


# ------------------------------------------------------------------ verify_step
def _cfg():
    return dataclasses.replace(GPT2Config.tiny(), n_embd=128, n_head=2, n_positions=256,
                               init_std=0.2)


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(0)
    return GPT2(_cfg()).eval().to(dev, torch.bfloat16)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def test_verify_step_against_fp32_model(cuda_device):
    """The window through ``verify_step`` and, token by token, through ``decode_step``: both are
    bf16 roundings of one computation in another order, so against the fp32 model the verify
    path may err at most twice as much as the decode path (one more rounding order per
    layer; a wrong position or mask errs by orders of magnitude more)."""
    dev, cfg = cuda_device, _cfg()
    model = _model(dev)
    m32 = GPT2(cfg).eval()
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    g = torch.Generator().manual_seed(9)
    plens, n_win, W, Tmax = [150, 17, 64, 9], [9, 5, 0, 9], 9, 200
    ps = [torch.randint(0, 512, (n,), generator=g).tolist() for n in plens]
    win = torch.randint(0, 512, (4, W), generator=g)
    # the yardstick: each row alone through the fp32 decode path
    want = torch.zeros(4, W, cfg.vocab_size)
    for s in (0, 1):
        c32 = KVCache(cfg, 1, Tmax)
        m32.prefill_into(torch.tensor([ps[s]]), [plens[s]], c32, _i32([0]))
        for i in range(n_win[s]):
            want[s, i] = m32.decode_step(win[s, i: i + 1], c32)[0]

    def prefilled():
        cache = KVCache(cfg, 4, Tmax, dev, torch.bfloat16)
        cache.k.fill_(float("nan"))
        cache.v.fill_(float("nan"))
        for s, p in enumerate(ps):
            model.prefill_into(torch.tensor([p], device=dev), [len(p)], cache,
                               _i32([s]).to(dev))
        cache.lens[3] = INACTIVE
        return cache

    cache = prefilled()
    lens0, k0 = cache.lens.clone(), cache.k.clone()
    out = torch.zeros(4, W, cfg.padded_vocab, device=dev, dtype=torch.bfloat16)
    got = model.verify_step(win.to(dev), _i32(n_win).to(dev), cache, out=out).float().cpu()
    assert torch.equal(cache.lens, lens0)
    dec = torch.zeros_like(want)
    for s in (0, 1):
        one = KVCache(cfg, 1, Tmax, dev, torch.bfloat16)
        model.prefill_into(torch.tensor([ps[s]], device=dev), [plens[s]], one, _i32([0]).to(dev))
        for i in range(n_win[s]):
            dec[s, i] = model.decode_step(win[s, i: i + 1].to(dev), one)[0].float().cpu()
        end = plens[s] + n_win[s]
        assert torch.isfinite(cache.k[:, s, :, :end].float()).all()
        assert torch.isnan(cache.k[:, s, :, end:].float()).all()  # nothing past the window
    for s in (0, 1):
        e_dec = _rel(dec[s, : n_win[s]], want[s, : n_win[s]])
        e_ver = _rel(got[s, : n_win[s]], want[s, : n_win[s]])
        print(f"row {s}: decode_step rel err {e_dec:.3e}, verify_step rel err {e_ver:.3e}")
        assert e_ver <= 2 * e_dec, (s, e_ver, e_dec)
    for s in (2, 3):  # n_win 0 and an idle slot: untouched
        assert torch.equal(cache.k[:, s].view(torch.int16), k0[:, s].view(torch.int16))


# ------------------------------------------------------------------ engine
# (prompt length, max_new_tokens, temperature, top_k, top_p, seed, continues the prefix):
# the mix of test_attn_extend_gpu.py
MIX = [(1, 24, 0.0, None, None, 3, True), (150, 9, 0.8, 5, None, 11, False),
       (17, 16, 1.3, 50, 0.9, 2, True), (70, 3, 0.8, None, 0.9, 7, True),
       (9, 20, 1.3, None, None, -4, False), (130, 12, 0.0, 5, None, 0, True)]
EOS = 7


class Oracle:
    """The drafter of tests/test_spec_decode.py: proposes the continuation of whichever known
    sequence starts with ``hist[:p] + tok0`` and corrupts draft i where ``(p + i) % 5 == 3``.
    torch ops only, no host read: capturable."""

    def __init__(self, sequences, k, cap, vocab, device):
        self.k, self.vocab = k, vocab
        full = torch.full((len(sequences), cap + k + 1), -1, dtype=torch.int64)
        for r, seq in enumerate(sequences):
            full[r, : len(seq)] = torch.tensor(seq)
        self.full = full.to(device)
        self.pos = torch.arange(cap, device=device)
        self.ahead = torch.arange(1, k + 1, device=device)

    def __call__(self, tok0, hist, lens, n_out, max_new, active):
        S, cap = hist.shape
        ok = (active != 0) & (lens >= 0) & (lens < cap)
        p = lens.long().clamp(0, cap - 1)
        seq = hist.long().scatter(1, p.unsqueeze(1), tok0.unsqueeze(1))
        same = (seq.unsqueeze(1) == self.full[:, :cap].unsqueeze(0)) | \
            (self.pos.view(1, 1, cap) > p.view(S, 1, 1))
        known = same.all(-1)
        idx = p.unsqueeze(1) + self.ahead
        drafts = self.full[known.long().argmax(1)].gather(1, idx)
        drafts = torch.where(idx % 5 == 3, (drafts + 1) % self.vocab, drafts)
        room = torch.minimum(max_new - n_out, cap - lens)
        nd = torch.where(known.any(1), (room - 1).clamp(0, self.k), torch.zeros_like(room))
        n_win = torch.where(ok, 1 + nd, torch.zeros_like(nd)).to(torch.int32)
        return torch.cat([tok0.unsqueeze(1), drafts], 1), n_win


def _drive(model, graph, sequences=None):
    g = torch.Generator().manual_seed(5)
    prefix = torch.randint(0, 512, (70,), generator=g).tolist()
    prompts = [torch.randint(0, 512, (m[0],), generator=g).tolist() for m in MIX]
    kw = {} if graph else {"graph": False}
    if sequences is not None:
        kw["drafter"] = Oracle(sequences, 4, 256, 512, model.wte.device)
    eng = GPT2Engine(model, slots=3, max_len=256, poll_every=2, prefix_slots=1, prefill_chunk=64,
                     eos_token_id=EOS, speculate=4, **kw)
    assert (eng._graph is not None) == graph
    pid = eng.add_prefix(prefix)
    rids = [eng.submit(p, m[1], temperature=m[2], top_k=m[3], top_p=m[4], seed=m[5],
                       prefix=pid if m[6] else None) for p, m in zip(prompts, MIX)]
    got = eng.run()
    assert not eng.has_work() and eng.num_filling == 0
    full = [(prefix if m[6] else []) + p for p, m in zip(prompts, MIX)]
    return [got[r] for r in rids], full, eng


def test_speculative_engine_graph_equals_eager(cuda_device):
    model = _model(cuda_device)
    (graphed, _, _), (eager, full, _), (again, _, _) = (_drive(model, gr)
                                                       for gr in (True, False, True))
    assert graphed == eager and graphed == again
    for toks, m in zip(graphed, MIX):
        assert EOS not in toks[:-1]
        assert len(toks) == m[1] or (toks[-1] == EOS and len(toks) < m[1])
    # an oracle built from the eager run's own output: drafts are made, checked and kept
    sequences = [p + t for p, t in zip(full, eager)]
    for graph in (True, False):
        toks, _, eng = _drive(model, graph, sequences)
        stats = eng.spec_stats()
        print(f"oracle graph={graph}: {stats}, steps {eng.steps}")
        assert stats["drafted"] > 0 and 0 <= stats["accepted"] <= stats["drafted"]
        for t, m in zip(toks, MIX):
            assert EOS not in t[:-1]
            assert len(t) == m[1] or (t[-1] == EOS and len(t) < m[1])
