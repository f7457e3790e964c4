"""``ref.logit_process`` (the single definition of the repetition / presence / frequency
penalties, logit bias and the minimum length before EOS) bit for bit against an independent
scalar implementation, Python loops over ``numpy.float32`` scalars in the same operation
order with the store's rounding done by hand on the bits; then every rule alone on planted
values, the skip rules, the ``min_new`` boundary and the wrapper's argument errors (CPU).

``make_case`` builds the mixed batches the GPU test (test_logit_process_gpu.py) shares."""

import numpy as np
import pytest
import torch

from ray_amd.ops import functional as rf
from ray_amd.ops import reference as ref

INF = float("inf")
NAMES = ("prompt", "prompt_len", "out", "n_out", "repetition", "presence", "frequency",
         "min_new", "bias_ids", "bias_vals", "n_bias")


# ------------------------------------------------------------------ the scalar implementation
def _bits_of(t):
    """The logits as a numpy array of raw integers."""
    idt = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(idt).numpy().astype(np.int64) & ((1 << (8 * t.element_size())) - 1)


def _load(bits, dtype):
    u = int(bits) << 16 if dtype == torch.bfloat16 else int(bits)
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def _store(x, dtype):
    """``x`` (numpy.float32) rounded once to ``dtype``, nearest even, as raw bits; NaN gives
    the canonical quiet NaN."""
    u = int(np.array([x], dtype=np.float32).view(np.uint32)[0])
    if dtype == torch.float32:
        return 0x7FC00000 if x != x else u
    if x != x:
        return 0x7FC0
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def scalar_logit_process(c, dtype):
    """The expected raw bits [B, Vs] of ``c["logits"]`` after processing: plain loops."""
    f32 = np.float32
    bits = _bits_of(c["logits"]).copy()
    B, Vs = bits.shape
    V = c.get("vocab_size") or Vs
    R, P = c["prompt"].shape
    cap, NB = c["out"].shape[1], c["bias_ids"].shape[1]
    host = {k: c[k].tolist() for k in NAMES}
    rows = c["rows"].tolist() if c.get("rows") is not None else list(range(B))
    active = c["active"].tolist() if c.get("active") is not None else [1] * B
    extra = c["extra"].tolist() if c.get("extra") is not None else None
    n_extra = c["n_extra"].tolist() if extra is not None else [0] * B
    W = c["extra"].shape[1] if extra is not None else 0
    eos = c.get("eos_token_id")
    with np.errstate(all="ignore"):
        for b in range(B):
            r = rows[b]
            if not active[b] or not 0 <= r < R:
                continue
            pl, no, nb = host["prompt_len"][r], host["n_out"][r], host["n_bias"][r]
            if not (0 <= pl <= P and 0 <= no <= cap and 0 <= nb <= NB and 0 <= n_extra[b] <= W):
                continue
            rp, pp, fp = (f32(host[k][r]) for k in ("repetition", "presence", "frequency"))
            mn = host["min_new"][r]
            if rp == 1 and pp == 0 and fp == 0 and nb == 0 and mn == 0:
                continue
            generated = host["out"][r][:no] + (extra[b][: n_extra[b]] if extra else [])
            seen = host["prompt"][r][:pl] + generated
            bias = {}
            for i in range(nb):
                bias.setdefault(host["bias_ids"][r][i], host["bias_vals"][r][i])
            ban = eos is not None and len(generated) < mn
            named = set(seen) | set(bias) | ({eos} if ban else set())
            for v in named:
                if not 0 <= v < V:
                    continue
                x = _load(bits[b, v], dtype)
                if v in seen:
                    x = f32(x / rp) if x > 0 else f32(x * rp)
                n = generated.count(v)
                if n:
                    x = f32(x - f32(fp * f32(n)))
                    x = f32(x - pp)
                if v in bias:
                    x = f32(x + f32(bias[v]))
                if ban and v == eos:
                    x = f32(-INF)
                bits[b, v] = _store(x, dtype)
    return bits


# ------------------------------------------------------------------ the shared cases
LENS = (0, 1, 63, 64, 65)


def make_case(V, B, seed=0, dtype=torch.bfloat16, width=70, window=5, pad=0):
    """A mixed batch as CPU tensors: B logits rows over R = B + 3 context rows of ``width``
    columns. Lengths from {0, 1, 63, 64, 65} and one row at the full width; histories of one
    repeated token, of distinct tokens and of 50 colliding values, some ids negative or
    >= V; bias lists of 0, 1 and LOGIT_BIAS_MAX entries with a duplicate id, an id out of
    range and a -inf value; neutral rows, rows with a bad length, a bad ``rows`` index and
    an inactive row; ±0, ±inf and NaN planted on named tokens; ``pad`` more columns of NaN."""
    g = torch.Generator().manual_seed(seed * 7919 + V * 31 + B)
    NB, R, W = rf.LOGIT_BIAS_MAX, B + 3, window

    def rint(lo, hi, shape):
        return torch.randint(lo, hi, shape, generator=g)

    def history(kind, n):
        if kind == 0:
            return torch.full((n,), int(rint(0, V, (1,))))
        if kind == 1:  # all distinct, from -1 up: one negative id, ids >= V when V is small
            span = max(n + 2, min(V + 2, 4 * n + 2))
            return torch.randperm(span, generator=g)[:n] - 1
        return rint(-2, 48, (n,)) * max(1, V // 50) if V >= 50 else rint(-2, 48, (n,))

    prompt = torch.zeros(R, width, dtype=torch.int32)
    out = torch.zeros(R, width, dtype=torch.int64)
    prompt_len = torch.tensor([LENS[(r + 1) % 5] for r in range(R)], dtype=torch.int32)
    n_out = torch.tensor([LENS[(2 * r + 3) % 5] for r in range(R)], dtype=torch.int32)
    prompt_len[0], n_out[0] = width, width  # the full row
    prompt_len.clamp_(max=width), n_out.clamp_(max=width)
    for r in range(R):
        prompt[r] = history(r % 3, width).to(torch.int32)
        out[r] = history((r + 1) % 3, width)
    rep = torch.tensor([(1.0, 1.3, 0.7, 2.5)[r % 4] for r in range(R)])
    pres = torch.tensor([(0.0, 0.5, -0.25)[r % 3] for r in range(R)])
    freq = torch.tensor([(0.5, 0.0, 0.1, -0.3, 0.0)[r % 5] for r in range(R)])
    n_bias = torch.tensor([(0, 1, NB)[r % 3] for r in range(R)], dtype=torch.int32)
    bias_ids = rint(-1, V + 1, (R, NB)).to(torch.int32)
    bias_vals = torch.randn(R, NB, generator=g) * 3
    for r in range(R):
        bias_ids[r, 0] = int(out[r, 0].clamp(-1, V))  # a bias on a token of the history
        bias_ids[r, 5], bias_ids[r, 9] = bias_ids[r, 2], bias_ids[r, 2]  # duplicates
        bias_ids[r, 7], bias_ids[r, 8] = V, -1
        bias_vals[r, 3] = -INF
    min_new = torch.tensor([(0, 1, 10 ** 6, 64)[r % 4] for r in range(R)], dtype=torch.int32)
    for r in range(4, R, 5):  # all neutral
        rep[r], pres[r], freq[r], n_bias[r], min_new[r] = 1.0, 0.0, 0.0, 0, 0
    if R > 6:
        prompt_len[R - 1], n_out[R - 2], n_bias[R - 3] = width + 1, -1, NB + 1
    rows = torch.arange(B, dtype=torch.int32)
    if B > 1:
        rows = torch.randperm(R, generator=g)[:B].to(torch.int32)
        rows[0] = 0
    active = torch.ones(B, dtype=torch.uint8)
    if B >= 5:
        rows[2], rows[3], active[4] = -1, R, 0
        rows[1] = rows[0]  # two logits rows share a context row
    extra = rint(-2, 48, (B, W))
    n_extra = rint(0, W + 1, (B,)).to(torch.int32)
    if B >= 5:
        n_extra[B - 1] = W + 1
    eos = V // 2
    x = (torch.randn(B, V, generator=g) * 4).to(dtype)
    plant = torch.tensor([0.0, -0.0, INF, -INF, float("nan")], dtype=dtype)
    for b in range(B):
        r = int(rows[b].clamp(0, R - 1))
        named = torch.cat([prompt[r, : int(prompt_len[r].clamp(0, width))].long(),
                           out[r, : int(n_out[r].clamp(0, width))],
                           bias_ids[r, : int(n_bias[r].clamp(0, NB))].long()])
        named = named[(named >= 0) & (named < V)].unique()
        pick = named[torch.randperm(len(named), generator=g)[:5]]
        x[b, pick] = plant[: len(pick)]
    if pad:
        x = torch.cat([x, torch.full((B, pad), float("nan"), dtype=dtype)], 1)
    return dict(logits=x, prompt=prompt, prompt_len=prompt_len, out=out, n_out=n_out,
                repetition=rep, presence=pres, frequency=freq, min_new=min_new,
                bias_ids=bias_ids, bias_vals=bias_vals, n_bias=n_bias, rows=rows, extra=extra,
                n_extra=n_extra, active=active, eos_token_id=eos, vocab_size=V)


def call(fn, c, logits=None):
    """``fn`` (``ref.logit_process`` or ``rf.logit_process``) on the case, IN PLACE on
    ``logits`` (default: a copy of the case's); returns the edited tensor."""
    x = c["logits"].clone() if logits is None else logits
    fn(x, *(c[k] for k in NAMES), rows=c.get("rows"), extra=c.get("extra"),
       n_extra=c.get("n_extra"), active=c.get("active"), eos_token_id=c.get("eos_token_id"),
       vocab_size=c.get("vocab_size"))
    return x


def skipped_rows(c):
    """The logits rows that must keep their bytes, by the skip rules."""
    R, P = c["prompt"].shape
    cap, NB, W = c["out"].shape[1], c["bias_ids"].shape[1], c["extra"].shape[1]
    res = []
    for b, r in enumerate(c["rows"].tolist()):
        bad = not c["active"][b] or not 0 <= r < R or not 0 <= c["n_extra"][b] <= W
        if not bad:
            bad = not (0 <= c["prompt_len"][r] <= P and 0 <= c["n_out"][r] <= cap
                       and 0 <= c["n_bias"][r] <= NB)
            bad = bad or (c["repetition"][r] == 1 and c["presence"][r] == 0
                          and c["frequency"][r] == 0 and c["n_bias"][r] == 0
                          and c["min_new"][r] == 0)
        if bad:
            res.append(b)
    return res


# ------------------------------------------------------------------ reference == scalar loops
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,B", [(1, 1), (7, 5), (9, 12), (509, 5), (509, 23), (50257, 6)])
def test_reference_against_scalar_loops(V, B, dtype):
    c = make_case(V, B, dtype=dtype, pad=3)
    want = scalar_logit_process(c, dtype)
    got = call(ref.logit_process, c)
    assert got.dtype == dtype
    assert np.array_equal(_bits_of(got), want)
    before = _bits_of(c["logits"])
    assert np.array_equal(want[:, V:], before[:, V:])  # the NaN padding keeps its bytes
    skipped = skipped_rows(c)
    assert np.array_equal(want[skipped], before[skipped])
    if B >= 12:
        assert len(skipped) >= 4 and len(skipped) < B
        assert (want != before).any(1).sum() > (B - len(skipped)) // 2


def test_reference_is_used_on_the_cpu_and_returns_its_argument():
    c = make_case(509, 9)
    x = c["logits"].clone()
    res = rf.logit_process(x, *(c[k] for k in NAMES), rows=c["rows"], extra=c["extra"],
                           n_extra=c["n_extra"], active=c["active"],
                           eos_token_id=c["eos_token_id"])
    assert res is x
    assert np.array_equal(_bits_of(x), _bits_of(call(ref.logit_process, c)))
    # a column slice of a wider buffer is edited in place, the rest keeps its bytes
    wide = torch.full((9, 640), float("nan"), dtype=torch.bfloat16)
    wide[:, 3: 512] = c["logits"]
    call(rf.logit_process, c, wide[:, 3: 512])
    assert np.array_equal(_bits_of(wide[:, 3: 512]), _bits_of(x))
    assert wide[:, :3].isnan().all() and wide[:, 512:].isnan().all()


# ------------------------------------------------------------------ the rules on planted values
def _tiny(V=8, **kw):
    """One logits row over one context row: prompt [1, 2], output [2, 3, 3], all neutral."""
    c = dict(logits=torch.tensor([[4.0, 2.0, -2.0, 1.0, -1.0, 0.5, 3.0, -3.0]])[:, :V],
             prompt=torch.tensor([[1, 2, 7, 7]], dtype=torch.int32),
             prompt_len=torch.tensor([2], dtype=torch.int32),
             out=torch.tensor([[2, 3, 3, 6, 6]]), n_out=torch.tensor([3], dtype=torch.int32),
             repetition=torch.ones(1), presence=torch.zeros(1), frequency=torch.zeros(1),
             min_new=torch.zeros(1, dtype=torch.int32),
             bias_ids=torch.zeros(1, 4, dtype=torch.int32), bias_vals=torch.zeros(1, 4),
             n_bias=torch.zeros(1, dtype=torch.int32))
    for k, v in kw.items():
        c[k] = v if k in ("eos_token_id", "vocab_size") or isinstance(v, torch.Tensor) \
            else torch.tensor(v, dtype=c[k].dtype)
    return c


def test_each_rule_alone_and_all_together():
    x0 = _tiny()["logits"][0].tolist()
    rep = call(ref.logit_process, _tiny(repetition=[2.0]))[0].tolist()
    assert rep == [4.0, 1.0, -4.0, 0.5, -1.0, 0.5, 3.0, -3.0]  # prompt and output tokens
    pres = call(ref.logit_process, _tiny(presence=[0.5]))[0].tolist()
    assert pres == [4.0, 2.0, -2.5, 0.5, -1.0, 0.5, 3.0, -3.0]  # output tokens only, once
    freq = call(ref.logit_process, _tiny(frequency=[0.25]))[0].tolist()
    assert freq == [4.0, 2.0, -2.25, 0.5, -1.0, 0.5, 3.0, -3.0]  # per occurrence
    bias = call(ref.logit_process, _tiny(bias_ids=[[5, 0, 5, 0]], n_bias=[3],
                                         bias_vals=[[1.0, -INF, 9.0, 2.0]]))[0].tolist()
    assert bias == [-INF, 2.0, -2.0, 1.0, -1.0, 1.5, 3.0, -3.0]  # the lowest index of id 5
    ban = call(ref.logit_process, _tiny(min_new=[4], eos_token_id=4))[0].tolist()
    assert ban == [4.0, 2.0, -2.0, 1.0, -INF, 0.5, 3.0, -3.0]
    assert call(ref.logit_process, _tiny(min_new=[4]))[0].tolist() == x0  # no EOS: no ban
    everything = call(ref.logit_process, _tiny(
        repetition=[2.0], presence=[0.5], frequency=[0.25], min_new=[4], eos_token_id=3,
        bias_ids=[[2, 1, 0, 0]], bias_vals=[[1.0, 1.0, 0.0, 0.0]], n_bias=[2]))[0].tolist()
    # token 2: -2 * 2 - 0.25 - 0.5 + 1; token 1: 2 / 2 + 1; token 3 (EOS): banned
    assert everything == [4.0, 2.0, -3.75, -INF, -1.0, 0.5, 3.0, -3.0]


def test_ids_out_of_range_are_ignored_and_neutral_rows_keep_nan_bytes():
    x0 = _tiny()["logits"]
    got = call(ref.logit_process, _tiny(
        repetition=[2.0], prompt=[[-1, 8, 9, 7]], out=[[-5, 8, 2 ** 40, 6, 6]],
        bias_ids=[[8, -1, 0, 0]], bias_vals=[[5.0, 5.0, 0.0, 0.0]], n_bias=[2], min_new=[9],
        eos_token_id=8))
    assert torch.equal(got, x0)
    # vocab_size: the columns at and beyond it are not tokens
    got = call(ref.logit_process, _tiny(repetition=[2.0], prompt=[[6, 7, 1, 1]], vocab_size=6))
    assert got[0].tolist() == [4.0, 2.0, -4.0, 0.5, -1.0, 0.5, 3.0, -3.0]
    # a signalling-NaN pattern: kept by a neutral row, by an inactive one, by a row whose
    # context is out of range; made canonical where a rule names it
    for kw, kept in ((dict(), True),
                     (dict(repetition=[2.0], active=torch.zeros(1, dtype=torch.uint8)), True),
                     (dict(repetition=[2.0], rows=torch.tensor([1], dtype=torch.int32)), True),
                     (dict(repetition=[2.0], n_out=[6]), True),
                     (dict(repetition=[2.0], prompt_len=[-1]), True),
                     (dict(repetition=[2.0]), False)):
        c = _tiny(**kw)
        c["logits"] = c["logits"].to(torch.bfloat16)
        raw = c["logits"].view(torch.int16)
        raw[0, 2], raw[0, 5] = 0x7FA5, 0x7FA5  # token 2 is in the history, token 5 is not
        got = call(ref.logit_process, c).view(torch.int16)[0].tolist()
        assert got[5] == 0x7FA5
        assert got[2] == (0x7FA5 if kept else 0x7FC0), kw
        assert kept == (got == raw[0].tolist())


def test_min_new_boundary():
    # three generated tokens: EOS is banned at min_new 4 (3 == 4 - 1), free at 3
    assert call(ref.logit_process, _tiny(min_new=[4], eos_token_id=0))[0, 0] == -INF
    assert call(ref.logit_process, _tiny(min_new=[3], eos_token_id=0))[0, 0] == 4.0
    # the window's tokens count as generated
    kw = dict(eos_token_id=0, extra=torch.tensor([[5, 5, 5]]))
    for n_extra, banned in ((0, True), (1, True), (2, False)):
        c = _tiny(min_new=[5], n_extra=torch.tensor([n_extra], dtype=torch.int32), **kw)
        assert (call(ref.logit_process, c)[0, 0] == -INF) == banned
    # and are penalised as such
    c = _tiny(frequency=[1.0], n_extra=torch.tensor([2], dtype=torch.int32), **kw)
    assert call(ref.logit_process, c)[0, 5] == 0.5 - 2.0


def test_duplicates_are_edited_once():
    # token 3 occurs in the prompt, three times in the output, twice in the bias list and
    # is the banned EOS's neighbour: one division, one subtraction of 3 * f, one bias
    c = _tiny(repetition=[2.0], frequency=[0.5], prompt=[[3, 3, 3, 3]], prompt_len=[4],
              out=[[3, 3, 3, 0, 0]], bias_ids=[[3, 3, 0, 0]], bias_vals=[[0.25, 8.0, 0.0, 0.0]],
              n_bias=[2])
    assert call(ref.logit_process, c)[0].tolist() == [4.0, 2.0, -2.0, 0.5 - 1.5 + 0.25, -1.0, 0.5,
                                                       3.0, -3.0]


# ------------------------------------------------------------------ argument errors
def test_wrapper_argument_errors():
    c = make_case(9, 5)
    args = [c["logits"].clone()] + [c[k] for k in NAMES]
    kw = dict(rows=c["rows"], extra=c["extra"], n_extra=c["n_extra"], active=c["active"],
              eos_token_id=4)
    rf.logit_process(*args, **kw)  # the base call is fine
    assert rf.LOGIT_BIAS_MAX == 64

    def bad_args(i, t):
        a = list(args)
        a[i] = t
        with pytest.raises(ValueError):
            rf.logit_process(*a, **kw)

    bad_args(0, args[0][0])  # not 2-D
    bad_args(0, torch.zeros(5, 9, dtype=torch.int32))
    for i, t in enumerate(args[1:], 1):
        wrong = torch.float64 if t.dtype != torch.float64 else torch.int32
        bad_args(i, t.to(wrong))  # dtype
        bad_args(i, t[:-1])  # rows
        bad_args(i, t.tolist())  # not a tensor
    bad_args(1, args[1][0])
    bad_args(3, args[3][0])
    bad_args(9, torch.zeros(8, 65, dtype=torch.int32))  # NB > LOGIT_BIAS_MAX
    bad_args(10, args[10][:, :-1])
    for name, t in (("rows", c["rows"][:-1]), ("rows", c["rows"].long()),
                    ("active", c["active"].bool()), ("active", c["active"][:-1]),
                    ("extra", c["extra"].to(torch.int32)), ("extra", c["extra"][:-1]),
                    ("n_extra", c["n_extra"].long()), ("n_extra", None), ("extra", None),
                    ("eos_token_id", 1.5), ("eos_token_id", True), ("vocab_size", 10),
                    ("vocab_size", 0)):
        with pytest.raises(ValueError):
            rf.logit_process(*args, **{**kw, name: t})
    with pytest.raises(ValueError):  # fewer context rows than logits rows, and no ``rows``
        rf.logit_process(args[0], *(t[:3] for t in args[1:]), **{**kw, "rows": None})
