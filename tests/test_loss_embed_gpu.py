"""Loss and embedding kernels (ops/csrc/xent.hip, embed.hip, linear.hip) against plain fp64
references: ra_xent_fused, ra_xent_fwd / ra_xent_bwd, ra_embed_bwd, ra_scale_bf16 and
ra_scaled_accum, called through their raw entry points and checked per element.

Every reference is computed once, in fp64 torch, on the kernel's own bf16 / fp32 inputs widened
to double. Everything a kernel writes is carved out of a larger NaN-filled allocation (GUARD
elements each side). Units: U = 2^-24 is one fp32 rounding (half an ulp, relative), H = 2^-9 is
the unit the bf16 results are counted in; one bf16 rounding (8 significant bits, unit roundoff
2^-8) is at most 2 H. Every bound below is TWICE the derived count, except the embedding's,
which is the order-independent summation bound itself.

ra_xent_fused (512 lanes, NV 16-byte vectors per lane, D = NV*8 + 6 + 8 additions deep: NV*8
sequential per lane, 6 wave levels, 8 wave partials):
  loss, in units of U * S with S = max(1, |lse|, |x_t|). With m the row maximum, s the sum of
  e_j = exp2(fma(x_j, log2e, -fl(m log2e))) and p the softmax, the derived count is
      D                       additions feeding s (relative to s, so absolute in ln s)
    + 5                       exp2 (1 ulp = 2), m + ln s (1), lse - x_t (2)
    + |m| / S                 the rounding of m * log2e, common to every e_j
    + 2 E / S                 fma rounding and the fp32 log2e on each exponent argument,
                              weighted by p_j: E = sum_j p_j (m - x_j)  (<= ln V)
    + 4 |ln s| / S            __logf = v_log_f32 (1 ulp) times fp32 ln 2
  dlogits off the target: e_j is rounded to bf16, multiplied by c = inv_count / s and rounded to
  bf16 again: 2 roundings = 4 H of |ref|; the fp32 error of e_j and c next to them is below
  (|m| + 2 |x_j - m| + D) U < 2^-15, i.e. 0.02 H. Bound 8 H. A reference of exactly 0 (-inf
  columns, padding, ignored rows) must be met exactly. The inputs keep the smallest non-zero
  |reference| a normal bf16 (asserted on the reference).
  dlogits at the target: one bf16 rounding of (exp(x_t - lse) - 1) * inv_count, 2 H |ref|,
  plus the fp32 chain as an absolute term inv_count * U * (p_t (S * count_loss + 3 |x_t - lse|
  + 2) + 2): the kernel's lse error, the subtraction, __expf, then the -1 and the multiply.

ra_xent_fwd (256 lanes, `it` = ceil(ceil(V / 8) / 256) + 1 online iterations per lane, then 6
wave and 3 block merges): the factors exp(x - m1) exp(m1 - m2) ... of one element telescope to
|x - M|, each __expf costs 3 |arg| + 2, and an element passes at most it + 9 exps, it + 9
multiplies and 8 it + 9 additions: count = 11 it + 36 + 3 + (3 E + 2 |ln s|) / S for loss (S
as above) and for lse (S = max(1, |lse|)).
ra_xent_bwd, fed the reference's lse rounded to fp32: one bf16 rounding (2 H |ref|) plus
g * U * (p_j (|lse| + 3 |x_j - lse| + 4) + onehot), g = grad_out * inv_count.

ra_embed_bwd: exact inputs (eighths) must give torch.equal results; for random inputs an
element fed by n additions is within n U (|sink_old| + sum |dx rows|) in any order, n = rows of
the token + 1, or B + 1 for a position.

ra_scale_bf16 is one fp32 multiply and one rounding: bit-equal to torch's. ra_scaled_accum: the
multiply-add, fused or not, is within 2 U (|sink| + |g src|); a bf16 sink rounds once more.

Worst figures on an MI355X (each test prints its own with pytest -s):
ra_xent_fused loss 2.3 units against derived counts of 35 (NV = 2) to 148 (NV = 16), at most
0.065 of the count; dlogits off the target 3.9 H (two roundings: 4), at the target 0.43 of the
bound. ra_xent_fwd loss 2.0 / lse 1.9 units against counts from 61; ra_xent_bwd 0.50 of its
bound. ra_embed_bwd 0.50 (tokens) / 0.20 (positions) of the summation bound. ra_scaled_accum
0.50 (fp32 sink: one rounding, the multiply-add is fused) and 0.996 (bf16 sink: among 4.2e6
elements one sits just above a power of two, where a rounding is worth its full 2^-8).

Before xent_fwd_kernel skipped an all -inf step, as online_merge does, every row of
test_xent_fwd_bwd_minus_inf_first_in_a_lane, and the -inf rows of test_xent_fwd_bwd_elements,
came back NaN: a lane whose first 8 columns (or first tail column) were all -inf computed
exp(-inf - -inf).
"""

import functools
import math

import numpy as np
import pytest
import torch

from ray_amd.ops import _lib
from ray_amd.ops import functional as rf
from ray_amd.ops._lib import ptr, stream_ptr

gpu = pytest.mark.gpu

U = 2.0 ** -24   # one fp32 rounding, relative to its operands
H = 2.0 ** -9    # the unit of the bf16 results: one bf16 rounding is at most 2 of them
GUARD = 4096     # sentinel elements on each side of a carved buffer (a multiple of 8)
BIG8 = 2048 * 256 * 8  # elements one full ra_grid(…, 256) pass of 8-wide bf16 threads covers


def f32(x):
    """x as the kernel receives it: rounded to float32, widened back to double."""
    return float(np.float32(x))


@pytest.fixture(scope="module")
def dev(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"
    yield cuda_device
    # hand the shared inputs and the allocator's cached blocks back, so the modules that run
    # after this one start from the same allocator state as without it
    _xent_inputs.cache_clear()
    _embed_inputs.cache_clear()
    _flat_inputs.cache_clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------
# the references, written once (fp64 torch; work on any device)

def xent_ref(logits, targets, V, ignore_index, scale):
    """Cross-entropy of the real columns [0, V) of `logits` [N, Vp], per row, in fp64 ->
    dict: loss [N], lse [N], dl [N, Vp] = (softmax - onehot) * scale (0 on columns >= V and on
    ignored rows), and what the error budgets need: ign, onehot, xt, m, p, E."""
    x = logits[:, :V].double()
    N, Vp = logits.shape
    lse = torch.logsumexp(x, 1)
    ign = (targets == ignore_index) | (targets < 0) | (targets >= V)
    tc = torch.where(ign, torch.zeros_like(targets), targets)
    xt = x.gather(1, tc[:, None])[:, 0]
    p = (x - lse[:, None]).exp()
    onehot = torch.zeros_like(x, dtype=torch.bool)
    onehot[~ign, tc[~ign]] = True
    dl = torch.zeros(N, Vp, dtype=torch.float64, device=logits.device)
    dl[:, :V] = (p - onehot.double()) * scale
    dl[ign] = 0.0
    m = x.max(1).values
    E = torch.where(p > 0, p * (m[:, None] - x), torch.zeros_like(p)).sum(1)
    full = torch.zeros(N, Vp, dtype=torch.bool, device=logits.device)
    full[:, :V] = onehot
    return {"loss": torch.where(ign, torch.zeros_like(lse), lse - xt), "lse": lse, "dl": dl,
            "ign": ign, "onehot": full, "xt": torch.where(ign, torch.zeros_like(xt), xt),
            "m": m, "p": p, "E": E}


def embed_ref(dx, sid, perm, wte_old, wpe_old, B, T, V):
    """wte[sid[n]] += dx[perm[n]] for the ids inside [0, V); wpe[t] += sum_b dx[b * T + t].
    fp64 in, fp64 out -> (wte, wpe, rows per token [V])."""
    ok = (sid >= 0) & (sid < V)
    wte = wte_old.clone().index_add_(0, sid[ok], dx[perm[ok]])
    wpe = wpe_old.clone()
    wpe[:T] += dx.view(B, T, -1).sum(0)
    cnt = torch.zeros(V, dtype=torch.int64, device=dx.device).index_add_(
        0, sid[ok], torch.ones_like(sid[ok]))
    return wte, wpe, cnt


def units(got, ref, scale):
    """|got - ref| per element in units of `scale` (inf where scale is 0 and the values
    differ; NaN where got is NaN, which fails every `<=`)."""
    err = (got.double() - ref).abs()
    zero = torch.zeros_like(err)
    return torch.where(scale > 0, err / scale, torch.where(err == 0, zero, zero + math.inf))


def worst(t):
    """max of a possibly empty tensor, NaN if any element is NaN."""
    return float(t.max()) if t.numel() else 0.0


# ------------------------------------------------------------------------------------------
# helpers

_ITYPE = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def bits(t):
    return t.view(_ITYPE[t.dtype])


def carved(src, dtype=None):
    """`src` (a tensor, or an element count to leave NaN-filled) copied into the middle of a
    larger NaN-filled allocation -> (whole buffer, view shaped like src)."""
    if isinstance(src, int):
        n, device, shape = src, torch.device("cuda", 0), (src,)
    else:
        n, device, dtype, shape = src.numel(), src.device, dtype or src.dtype, src.shape
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=device, dtype=dtype)
    view = buf[GUARD:GUARD + n].view(shape)
    if not isinstance(src, int):
        view.copy_(src)
    return buf, view


def guards_intact(buf):
    nan = int(bits(torch.full((1,), float("nan"), dtype=buf.dtype))[0])
    raw = bits(buf)
    return bool((raw[:GUARD] == nan).all()) and bool((raw[-GUARD:] == nan).all())


def all_nan_bits(t):
    nan = int(bits(torch.full((1,), float("nan"), dtype=t.dtype))[0])
    return bool((bits(t) == nan).all())


def note(key, *vals):
    """Print each figure before it is asserted on (pytest -s shows the head-room)."""
    print(f"[loss_embed] {key}: " + " ".join(f"{x:.3g}" for x in vals))


# ------------------------------------------------------------------------------------------
# cross-entropy cases, shared by the fused and the two-pass kernels

# (Vp, V): the padded widths at which ra_xent_fused changes its register-count instantiation
# (NV = 2 up to 8192, 4 up to 16384, 8 up to 32768, 13 up to 53248, 16 up to 65536), each with
# V = Vp, a partial last vector, and several all-padding vectors
XENT_FUSED = [(8, 8), (8, 7), (8, 1)] + [
    (Vp, Vp - d) for Vp in (4096, 4104, 8192, 8200, 16392, 32776, 53256, 65536)
    for d in (0, 1, 7, 47)] + [(50304, 50257)]
XENT_FUSED.sort()
# the two-pass kernels also get: V < 8 (tail loop only), fewer than 256 vectors (idle lanes),
# every V % 8 with two lanes on their second vector
XENT_TWO_PASS = XENT_FUSED + [(8, 5), (8, 3), (512, 509), (1024, 1024)] + [
    (2064, 2048 + r) for r in range(1, 8)]
XENT_N = 16
# (ignore_index, inv_count)
XENT_VARIANTS = [(-100, 1.0 / 7.0), (3, 1.0)]


def fused_nv(Vp):
    per = (Vp // 8 + 511) // 512
    return next(nv for nv in (2, 4, 8, 13, 16) if per <= nv)


def xent_targets(V, Vp, variant):
    """16 targets, one per row: 12 from the edge columns that exist (first, either side of the
    first vector boundary, last, last column of the last full vector, either side of the
    k = 1 boundary of the fused kernel, two inner ones), rotated per variant so that the same
    column meets another kind of row, and 4 that select nothing at rows 3, 7, 11, 15."""
    edge = [0, 7, 8, V - 1, V // 8 * 8 - 1, 4095, 4096, V // 2, V // 3]
    valid = list(dict.fromkeys(t for t in edge if 0 <= t < V))
    valid = valid[3 * variant % len(valid):] + valid[:3 * variant % len(valid)]
    ignore_index = XENT_VARIANTS[variant][0]
    # the ignore index (3 is a real column wherever V > 3), and guards: t >= V and t < 0
    dead = [[ignore_index, V, -1, 2 ** 40], [ignore_index, -100, Vp, V + 5]][variant]
    out = []
    for i in range(XENT_N):
        out.append(dead[i // 4] if i % 4 == 3 else valid[(i - i // 4) % len(valid)])
    return out


def xent_inputs_host(Vp, V, variant):
    """bf16 logits [16, Vp] and int64 targets from a CPU generator. Row i has character
    i % 7: 0 3 * randn; 1, 2 row 0 shifted by +60, -60; 3 the target dominates
    (p_t ~ 1 - 1e-3); 4 another column (the last one, or the first) dominates (loss ~ 40);
    5 constant; 6 -inf in column 0, in columns 8..15 and in every ~10th column (never the
    whole row, never the target). Padding columns hold NaN and +3e38 in turn."""
    gen = torch.Generator().manual_seed(1000 * Vp + 10 * V + variant)
    ignore_index = XENT_VARIANTS[variant][0]
    t = torch.tensor(xent_targets(V, Vp, variant), dtype=torch.int64)
    x = 3.0 * torch.randn(XENT_N, V, generator=gen)
    for i in range(XENT_N):
        ti = int(t[i])
        live = ti != ignore_index and 0 <= ti < V
        ch = i % 7
        if ch == 1:
            x[i] = x[0] + 60.0
        elif ch == 2:
            x[i] = x[0] - 60.0
        elif ch == 3 and live and V > 1:
            others = torch.cat([x[i, :ti], x[i, ti + 1:]]).bfloat16().double()
            x[i, ti] = float(torch.logsumexp(others, 0)) + math.log(999.0)
        elif ch == 4 and live and V > 1:
            x[i, V - 1 if ti != V - 1 else 0] = x[i, ti] + 40.0
        elif ch == 5:
            x[i] = 0.5
        elif ch == 6:
            keep = ti if live else V - 1
            dead = torch.rand(V, generator=gen) < 0.1
            dead[0] = True
            dead[8:16] = True
            dead[keep] = False
            x[i, dead] = -math.inf
    logits = torch.empty(XENT_N, Vp)
    logits[:, :V] = x
    pad = torch.arange(V, Vp)
    logits[:, V:] = torch.where((pad - V) % 2 == 0, math.nan, 3e38)
    return logits.bfloat16(), t


@functools.lru_cache(maxsize=None)
def _xent_inputs(Vp, V, variant):
    d = torch.device("cuda", 0)
    return tuple(x.to(d) for x in xent_inputs_host(Vp, V, variant))


def loss_scale(r):
    one = torch.ones_like(r["lse"])
    return torch.maximum(one, torch.maximum(r["lse"].abs(), r["xt"].abs()))


def fused_loss_count(r, Vp):
    """The derived rounding count of the fused kernel's loss, per row (module docstring)."""
    S = loss_scale(r)
    D = fused_nv(Vp) * 8 + 6 + 8
    return D + 5 + (r["m"].abs() + 2 * r["E"] + 4 * (r["lse"] - r["m"]).abs()) / S


def fwd_count(r, V, S):
    it = -(-(-(-V // 8)) // 256) + 1  # ceil(ceil(V / 8) / 256) vector iterations + the tail
    return 11 * it + 36 + 3 + (3 * r["E"] + 2 * (r["lse"] - r["m"]).abs()) / S


def check_normal(r, V):
    """The smallest non-zero |dlogit| of the reference is a normal bf16."""
    nz = r["dl"][:, :V].abs()
    nz = nz[nz > 0]
    assert nz.numel() == 0 or float(nz.min()) >= 2.0 ** -126


def check_fused(out, loss, r, V, Vp, inv, tag):
    """dlogits `out` [N, Vp] bf16 and `loss` [N] of ra_xent_fused against the reference `r`
    -> worst figures as fractions of their bounds (loss, off-target, target)."""
    check_normal(r, V)
    ign, hot = r["ign"], r["onehot"]
    S, cnt = loss_scale(r), fused_loss_count(r, Vp)
    # loss: exactly 0 on ignored rows (scale 0 there), else within twice the count
    ul = units(loss, r["loss"], torch.where(ign, torch.zeros_like(S), U * S * 2 * cnt))
    raw = units(loss, r["loss"], torch.where(ign, torch.zeros_like(S), U * S))
    note(f"xent_fused loss units/count {tag}", worst(raw), float(cnt.min()))
    assert worst(ul) <= 1.0, (tag, ul.tolist())
    # off the target: 8 H of |ref|; a reference of 0 (padding, -inf columns, ignored rows) is
    # to be met exactly
    ud = units(out, r["dl"], 8 * H * r["dl"].abs())
    ud = torch.where(hot, torch.zeros_like(ud), ud)
    note(f"xent_fused dlogits off-target H {tag}", 8 * worst(ud))
    assert worst(ud) <= 1.0, (tag, ud.max(1).values.tolist())
    assert not out[:, V:].any() and not out[ign].any() and not loss[ign].any(), tag
    # the target column, patched from the fp32 logit
    live = ~ign
    got_t, ref_t = out[hot].double(), r["dl"][hot]
    pt = (r["xt"] - r["lse"]).exp()[live]
    fp32 = inv * U * (pt * (S[live] * cnt[live] + 3 * (r["xt"] - r["lse"])[live].abs() + 2) + 2)
    ut = units(got_t, ref_t, 2 * (2 * H * ref_t.abs() + fp32))
    note(f"xent_fused dlogits target {tag}", worst(ut))
    assert worst(ut) <= 1.0, (tag, ut.tolist())
    return worst(ul), worst(ud), worst(ut)


def check_two_pass_fwd(loss, lse, r, V, tag):
    ign = r["ign"]
    S, Sl = loss_scale(r), torch.maximum(torch.ones_like(r["lse"]), r["lse"].abs())
    ul = units(loss, r["loss"], torch.where(ign, torch.zeros_like(S),
                                            U * S * 2 * fwd_count(r, V, S)))
    ue = units(lse, r["lse"], U * Sl * 2 * fwd_count(r, V, Sl))
    note(f"xent_fwd loss/lse units {tag}",
         worst(units(loss, r["loss"], torch.where(ign, torch.zeros_like(S), U * S))),
         worst(units(lse, r["lse"], U * Sl)), float(fwd_count(r, V, Sl).min()))
    assert worst(ul) <= 1.0 and worst(ue) <= 1.0, (tag, ul.tolist(), ue.tolist())
    assert not loss[ign].any(), tag
    return worst(ul), worst(ue)


def check_two_pass_bwd(dl, r, x, V, g, tag, lse_err=0.0):
    """lse_err: absolute error bound [N, 1] of the lse the kernel was fed, beyond its rounding
    to fp32."""
    check_normal(r, V)
    p, lse = r["p"], r["lse"][:, None]
    fp32 = torch.zeros_like(r["dl"])
    arg = torch.where(p > 0, (x[:, :V].double() - lse).abs(), torch.zeros_like(p))
    fp32[:, :V] = g * (U * (p * (lse.abs() + 3 * arg + 4) + r["onehot"][:, :V].double())
                       + p * lse_err)
    fp32[r["ign"]] = 0.0
    ud = units(dl, r["dl"], 2 * (2 * H * r["dl"].abs() + fp32))
    note(f"xent_bwd dl {tag}", worst(ud))
    assert worst(ud) <= 1.0, (tag, ud.max(1).values.tolist())
    assert not dl[:, V:].any() and not dl[r["ign"]].any(), tag
    return worst(ud)


# ------------------------------------------------------------------------------------------
# embedding cases

# name -> (B, T, runs): run lengths over the sorted positions, windows of 32. An int is a run
# of one token (the k-th run is token 2k + 1, so every even row of the table never occurs);
# ("neg", n) / ("big", n) are runs of one id below 0 / at or above V.
EMBED_LAYOUTS = {
    "distinct": (5, 8, [1] * 40),
    "one_token_7_windows": (8, 25, [200]),
    "run_0_32": (7, 10, [32, 1, 1, 36]),
    "run_0_33": (7, 10, [33, 1, 36]),
    "run_31_33": (7, 10, [1] * 31 + [2, 37]),
    "run_30_98": (4, 27, [1] * 30 + [68] + [1] * 10),
    "edge_to_edge": (4, 33, [20, 44, 64, 4]),
    "edge_to_edge_short": (7, 11, [10, 22, 40, 5]),
    "ends_at_last_row": (3, 25, [1] * 5 + [70]),
    "rows_5": (1, 5, [2, 3]),
    "rows_1": (1, 1, [1]),
    "one_batch_row": (1, 70, [3, 40, 27]),
    "rows_400": (8, 50, [5, 390, 5]),
    "out_of_range": (8, 25, [("neg", 36), ("neg", 4), 10, 50, 40, ("big", 25), ("big", 35)]),
}
EMBED_C = [8, 72, 768, 1024, 1032, 1600]


def embed_ids(name):
    """-> (sorted ids [rows] ascending, V) of a layout."""
    B, T, runs = EMBED_LAYOUTS[name]
    V = 2 * len(runs) + 2
    ids, neg, big = [], -3 * len(runs), V
    for k, run in enumerate(runs):
        if isinstance(run, int):
            ids += [2 * k + 1] * run
        elif run[0] == "neg":
            ids += [neg] * run[1]
            neg += 2
        else:
            ids += [big] * run[1]
            big += 7
    assert len(ids) == B * T and ids == sorted(ids)
    return torch.tensor(ids, dtype=torch.int64), V


def embed_inputs_host(name, C, exact):
    """dx bf16 [rows, C], sorted ids, a random perm of the rows, fp32 prefills of the token
    sink [V, C] and the position sink [T + 3, C]. exact: dx in eighths within +-2 and
    prefills in eighths within +-64, so that every fp32 sum is exact in any order."""
    B, T, _ = EMBED_LAYOUTS[name]
    rows = B * T
    sid, V = embed_ids(name)
    gen = torch.Generator().manual_seed(7000 + 13 * rows + C + exact)
    perm = torch.randperm(rows, generator=gen)
    if exact:
        dx = torch.randint(-16, 17, (rows, C), generator=gen) / 8.0
        wte = torch.randint(-512, 513, (V, C), generator=gen) / 8.0
        wpe = torch.randint(-512, 513, (T + 3, C), generator=gen) / 8.0
    else:
        dx = torch.randn(rows, C, generator=gen)
        wte = torch.randn(V, C, generator=gen)
        wpe = torch.randn(T + 3, C, generator=gen)
    return dx.bfloat16(), sid, perm, wte, wpe


@functools.lru_cache(maxsize=None)
def _embed_inputs(name, C, exact):
    d = torch.device("cuda", 0)
    return tuple(x.to(d) for x in embed_inputs_host(name, C, exact))


def _run_embed(dx, sid, perm, wte0, wpe0, B, T, C, V):
    """One raw launch on carved copies of the sinks and a carved, NaN-filled workspace."""
    L = _lib.lib()
    b = {"wte": carved(wte0), "wpe": carved(wpe0),
         "work": carved(max(int(L.ra_embed_bwd_work(max(B, 1), max(T, 1), max(C, 8))), 8),
                        torch.float32)}
    b["rc"] = L.ra_embed_bwd(ptr(dx), ptr(sid), ptr(perm), ptr(b["work"][1]), ptr(b["wte"][1]),
                             ptr(b["wpe"][1]), B, T, C, V, stream_ptr())
    torch.cuda.synchronize()
    return b


# ------------------------------------------------------------------------------------------
# flat inputs of ra_scale_bf16 / ra_scaled_accum

FLAT_SIZES = [8, BIG8 + 8 * 777]


def flat_inputs_host(n):
    """src, sink (fp32): randn times a log-spaced scale 1e-4 .. 10, shuffled, so that every
    grid-stride pass sees the whole range; every 17th src exactly 0."""
    gen = torch.Generator().manual_seed(500 + n)
    scale = torch.logspace(-4, 1, n)[torch.randperm(n, generator=gen)]
    src = torch.randn(n, generator=gen) * scale
    src[::17] = 0.0
    sink = torch.randn(n, generator=gen) * scale[torch.randperm(n, generator=gen)]
    return src, sink


@functools.lru_cache(maxsize=None)
def _flat_inputs(n):
    d = torch.device("cuda", 0)
    return tuple(x.to(d) for x in flat_inputs_host(n))


# ------------------------------------------------------------------------------------------
# 1. the references themselves, against torch in double on the CPU (no GPU needed)

def test_xent_reference_matches_torch_cpu():
    assert [fused_nv(Vp) for Vp in (8, 8192, 8200, 16392, 32776, 50304, 53256, 65536)] == \
        [2, 2, 4, 8, 13, 13, 16, 16]
    assert len(XENT_FUSED) == 36 and len(set(XENT_TWO_PASS)) == len(XENT_TWO_PASS)
    F = torch.nn.functional
    for Vp, V in [(8, 8), (8, 7), (8, 1), (2064, 2051), (4104, 4097), (8200, 8153)]:
        for variant, (ignore_index, inv) in enumerate(XENT_VARIANTS):
            logits, t = xent_inputs_host(Vp, V, variant)
            r = xent_ref(logits, t, V, ignore_index, f32(inv))
            # the table holds what it says: edge targets, an ignored row, guards on both sides
            tl = t.tolist()
            assert {0, V - 1} <= set(tl) and ignore_index in tl and int(r["ign"].sum()) >= 4
            assert any(x >= V for x in tl) and any(x < 0 and x != ignore_index for x in tl)
            assert bool(logits[:, V:].isnan().any()) == (Vp - V > 0)
            assert torch.isfinite(r["lse"]).all() and torch.isfinite(r["dl"]).all()
            check_normal(r, V)
            live = ~r["ign"]
            if V > 1:
                pt = (r["xt"] - r["lse"]).exp()
                rows = torch.arange(XENT_N)
                assert worst(((1 - pt)[live & (rows % 7 == 3)] - 1e-3).abs()) < 2e-4
                assert worst((r["loss"][live & (rows % 7 == 4)] - 40).abs()) < 0.5
                assert worst((r["loss"][live & (rows % 7 == 5)] - math.log(V)).abs()) < 1e-12
                assert V < 64 or logits[6, :V].isinf().sum() >= 9
            # torch takes no out-of-range targets: hand it the ignore index there
            tt = torch.where(r["ign"], torch.full_like(t, -100), t)
            x = logits[:, :V].double().requires_grad_()
            rows_loss = F.cross_entropy(x, tt, reduction="none", ignore_index=-100)
            (rows_loss.sum() * f32(inv)).backward()
            assert torch.allclose(r["loss"], rows_loss.detach(), rtol=1e-12, atol=1e-12)
            assert torch.allclose(r["dl"][:, :V], x.grad, rtol=1e-10, atol=1e-300)
            assert not r["dl"][:, V:].any() and not r["dl"][r["ign"]].any()


def test_embed_reference_matches_torch_cpu():
    for name, C, exact in [("out_of_range", 8, True), ("run_30_98", 72, False),
                           ("one_token_7_windows", 8, False), ("rows_1", 8, True),
                           ("edge_to_edge", 72, True)]:
        B, T, runs = EMBED_LAYOUTS[name]
        dx, sid, perm, wte0, wpe0 = embed_inputs_host(name, C, exact)
        V = wte0.shape[0]
        assert sorted(perm.tolist()) == list(range(B * T))
        wte, wpe, cnt = embed_ref(dx.double(), sid, perm, wte0.double(), wpe0.double(), B, T, V)
        # the same sums spelled as a loop over the rows, and as sum(0)
        want = wte0.double().clone()
        for n in range(B * T):
            if 0 <= int(sid[n]) < V:
                want[int(sid[n])] += dx[int(perm[n])].double()
        assert torch.allclose(wte, want, rtol=1e-13, atol=1e-13)
        assert torch.equal(cnt, torch.bincount(sid[(sid >= 0) & (sid < V)], minlength=V))
        assert torch.equal(wte[::2], wte0.double()[::2])  # even tokens never occur
        pos = wpe0.double().clone()
        pos[:T] += dx.double().view(B, T, C).sum(0)
        assert torch.allclose(wpe, pos, rtol=1e-13, atol=1e-13)
        assert torch.equal(wpe[T:], wpe0.double()[T:])
        if exact:  # the exact cases are exact in fp32 too
            assert torch.equal(wte.float().double(), wte) and torch.equal(wpe.float().double(), wpe)


# ------------------------------------------------------------------------------------------
# 2. ra_xent_fused

def _run_fused(logits, t, inv, N, V, Vp, ignore_index):
    """One raw launch on a carved copy of the logits -> dict of (buffer, view) pairs."""
    b = {"x": carved(logits), "loss": carved(max(N, 1), torch.float32)}
    inv_t = torch.tensor([inv], device=logits.device, dtype=torch.float32)
    b["rc"] = _lib.lib().ra_xent_fused(ptr(b["x"][1]), ptr(t), ptr(inv_t), ptr(b["loss"][1]), N,
                                       V, Vp, ignore_index, stream_ptr())
    torch.cuda.synchronize()
    return b


@gpu
@pytest.mark.parametrize("Vp,V", XENT_FUSED)
def test_xent_fused_elements(dev, Vp, V):
    for variant, (ignore_index, inv) in enumerate(XENT_VARIANTS):
        tag = f"Vp={Vp} V={V} NV={fused_nv(Vp)} ignore={ignore_index}"
        logits, t = _xent_inputs(Vp, V, variant)
        r = xent_ref(logits, t, V, ignore_index, f32(inv))
        b = _run_fused(logits, t, inv, XENT_N, V, Vp, ignore_index)
        assert b["rc"] == 0, tag
        check_fused(b["x"][1], b["loss"][1], r, V, Vp, f32(inv), tag)
        assert guards_intact(b["x"][0]) and guards_intact(b["loss"][0]), tag
        # the same input again: the same bits
        b2 = _run_fused(logits, t, inv, XENT_N, V, Vp, ignore_index)
        assert torch.equal(bits(b["x"][0]), bits(b2["x"][0])), tag
        assert torch.equal(bits(b["loss"][0]), bits(b2["loss"][0])), tag


@gpu
def test_xent_fused_all_rows_ignored(dev):
    Vp, V = 8200, 8153
    logits, _ = _xent_inputs(Vp, V, 0)
    logits = logits[:5]
    t = torch.tensor([-100, -100, V, -1, -100], device=dev)
    b = _run_fused(logits, t, 1.0, 5, V, Vp, -100)
    assert b["rc"] == 0
    assert not bits(b["x"][1]).any() and not bits(b["loss"][1]).any()
    assert guards_intact(b["x"][0]) and guards_intact(b["loss"][0])


@gpu
@pytest.mark.parametrize("N,V,Vp", [(4, 65544, 65544), (4, 12, 12), (4, 4097, 4096), (0, 8, 8),
                                    (4, 65537, 65544)])
def test_xent_fused_rejects_before_launch(dev, N, V, Vp):
    logits = torch.ones(4, Vp, device=dev).bfloat16()
    t = torch.zeros(4, dtype=torch.int64, device=dev)
    b = _run_fused(logits, t, 1.0, N, V, Vp, -100)
    assert b["rc"] != 0
    assert torch.equal(bits(b["x"][1]), bits(logits)) and all_nan_bits(b["loss"][0])
    assert guards_intact(b["x"][0])


# ------------------------------------------------------------------------------------------
# 3. ra_xent_fwd / ra_xent_bwd

GOUT = 1.5


def _run_two_pass(logits, t, r, N, V, Vp, ignore_index, inv):
    """ra_xent_fwd, then ra_xent_bwd fed the reference's lse (rounded to fp32)."""
    L = _lib.lib()
    d = logits.device
    b = {"loss": carved(N, torch.float32), "lse": carved(N, torch.float32),
         "dl": carved(N * Vp, torch.bfloat16)}
    rc1 = L.ra_xent_fwd(ptr(logits), ptr(t), ptr(b["loss"][1]), ptr(b["lse"][1]), N, V, Vp,
                        ignore_index, stream_ptr())
    lse32 = r["lse"].float()
    gout = torch.tensor([GOUT], device=d, dtype=torch.float32)
    rc2 = L.ra_xent_bwd(ptr(logits), ptr(t), ptr(lse32), ptr(gout), inv, ptr(b["dl"][1]), N, V,
                        Vp, ignore_index, stream_ptr())
    torch.cuda.synchronize()
    b["rc"] = (rc1, rc2)
    b["dl"] = (b["dl"][0], b["dl"][1].view(N, Vp))
    return b


@gpu
@pytest.mark.parametrize("Vp,V", XENT_TWO_PASS)
def test_xent_fwd_bwd_elements(dev, Vp, V):
    for variant, (ignore_index, inv) in enumerate(XENT_VARIANTS):
        tag = f"Vp={Vp} V={V} ignore={ignore_index}"
        logits, t = _xent_inputs(Vp, V, variant)
        g = f32(GOUT) * f32(inv)
        r = xent_ref(logits, t, V, ignore_index, g)
        b = _run_two_pass(logits, t, r, XENT_N, V, Vp, ignore_index, inv)
        assert b["rc"] == (0, 0), tag
        check_two_pass_fwd(b["loss"][1], b["lse"][1], r, V, tag)
        check_two_pass_bwd(b["dl"][1], r, logits, V, g, tag)
        for k in ("loss", "lse", "dl"):
            assert guards_intact(b[k][0]), (tag, k)


def xent_inf_inputs_host(Vp, V):
    """8 rows whose -inf columns are the first thing a lane of xent_fwd_kernel sees: a whole
    aligned group of 8 (lane l starts at columns 8 l .. 8 l + 7), or the tail column
    V // 8 * 8 + l of a lane l that has no full vector (V < 64), or of a lane whose only
    vector is -inf too. Row 0 has all of them, each other row one. Targets are finite
    columns."""
    gen = torch.Generator().manual_seed(31 * Vp + V)
    x = 3.0 * torch.randn(8, V, generator=gen)
    V8 = V // 8
    spots = [[8 * g + j for j in range(8)]
             for g in dict.fromkeys((0, 5, 255, V8 - 1)) if 0 <= g < min(V8, 256)]
    spots += [[c] for c in range(V8 * 8 + V8, V)][:3]  # tail columns of lanes >= V8
    if V8 <= 256 and V % 8 and V8:  # lane 0: its only vector, then its tail column
        spots.append(spots[0] + [V8 * 8])
    t = torch.empty(8, dtype=torch.int64)
    for i in range(8):
        dead = torch.zeros(V, dtype=torch.bool)
        for cols in (spots if i == 0 else [spots[(i - 1) % len(spots)]]):
            dead[cols] = True
        live = (~dead).nonzero()[:, 0]
        t[i] = live[(7 * i) % live.numel()]
        x[i, dead] = -math.inf
    logits = torch.zeros(8, Vp)
    logits[:, :V] = x
    return logits.bfloat16(), t


@gpu
@pytest.mark.parametrize("Vp,V", [(8, 5), (16, 13), (32, 29), (2064, 2051), (4104, 4099),
                                  (50304, 50257)])
def test_xent_fwd_bwd_minus_inf_first_in_a_lane(dev, Vp, V):
    tag = f"Vp={Vp} V={V}"
    logits, t = (x.to(dev) for x in xent_inf_inputs_host(Vp, V))
    assert logits[:, :V].isinf().any(1).all() and not logits[:, :V].isinf().all(1).any()
    r = xent_ref(logits, t, V, -100, f32(GOUT))
    assert torch.isfinite(r["loss"]).all()
    b = _run_two_pass(logits, t, r, 8, V, Vp, -100, 1.0)
    assert b["rc"] == (0, 0), tag
    check_two_pass_fwd(b["loss"][1], b["lse"][1], r, V, tag)
    check_two_pass_bwd(b["dl"][1], r, logits, V, f32(GOUT), tag)
    # the public op: finite, and the mean of the same rows
    x = logits.clone().requires_grad_()
    loss = rf.cross_entropy(x, t, V)
    loss.backward()
    torch.cuda.synchronize()
    want = float(r["loss"].mean())
    assert abs(float(loss) - want) <= 1e-5 * max(1.0, abs(want)), (tag, float(loss), want)
    # its backward reads the forward kernel's own lse
    r8 = xent_ref(logits, t, V, -100, 1.0 / 8.0)
    Sl = torch.maximum(torch.ones_like(r8["lse"]), r8["lse"].abs())
    check_two_pass_bwd(x.grad, r8, logits, V, 1.0 / 8.0, tag + " rf.cross_entropy",
                       lse_err=(U * Sl * fwd_count(r8, V, Sl))[:, None])


# ------------------------------------------------------------------------------------------
# 4. ra_embed_bwd

@gpu
@pytest.mark.parametrize("C", EMBED_C)
@pytest.mark.parametrize("name", sorted(EMBED_LAYOUTS))
def test_embed_bwd_exact(dev, name, C):
    B, T, _ = EMBED_LAYOUTS[name]
    dx, sid, perm, wte0, wpe0 = _embed_inputs(name, C, True)
    V = wte0.shape[0]
    wte, wpe, _ = embed_ref(dx.double(), sid, perm, wte0.double(), wpe0.double(), B, T, V)
    b = _run_embed(dx, sid, perm, wte0, wpe0, B, T, C, V)
    assert b["rc"] == 0
    # both sinks whole: rows of tokens that do not occur and position rows >= T included
    assert torch.equal(b["wte"][1], wte.float()), (name, C)
    assert torch.equal(b["wpe"][1], wpe.float()), (name, C)
    for k in ("wte", "wpe", "work"):
        assert guards_intact(b[k][0]), (name, C, k)


@gpu
@pytest.mark.parametrize("C", [72, 1600])
@pytest.mark.parametrize("name", ["one_token_7_windows", "run_30_98", "rows_400", "out_of_range",
                                  "edge_to_edge"])
def test_embed_bwd_random_values_and_same_bits_twice(dev, name, C):
    B, T, _ = EMBED_LAYOUTS[name]
    dx, sid, perm, wte0, wpe0 = _embed_inputs(name, C, False)
    V = wte0.shape[0]
    d64 = dx.double()
    wte, wpe, cnt = embed_ref(d64, sid, perm, wte0.double(), wpe0.double(), B, T, V)
    ok = (sid >= 0) & (sid < V)
    mag_w = wte0.double().abs().index_add_(0, sid[ok], d64[perm[ok]].abs())
    mag_p = wpe0.double().abs()
    mag_p[:T] += d64.abs().view(B, T, C).sum(0)
    b = _run_embed(dx, sid, perm, wte0, wpe0, B, T, C, V)
    assert b["rc"] == 0
    uw = units(b["wte"][1], wte, U * mag_w * (cnt[:, None] + 1))
    up = units(b["wpe"][1][:T], wpe[:T], U * mag_p[:T] * (B + 1))
    note(f"embed_bwd wte/wpe fraction of n U sum|x| {name} C={C}", worst(uw), worst(up))
    assert worst(uw) <= 1.0 and worst(up) <= 1.0, (name, C, worst(uw), worst(up))
    assert torch.equal(bits(b["wpe"][1][T:]), bits(wpe0[T:]))
    assert torch.equal(bits(b["wte"][1][cnt == 0]), bits(wte0[cnt == 0]))
    b2 = _run_embed(dx, sid, perm, wte0, wpe0, B, T, C, V)
    for k in ("wte", "wpe"):
        assert guards_intact(b[k][0]), (name, C, k)
        assert torch.equal(bits(b[k][0]), bits(b2[k][0])), (name, C, k)


@gpu
@pytest.mark.parametrize("name,C", [("run_30_98", 1032), ("one_token_7_windows", 72)])
def test_embedding_backward_sorts_and_scatters_exactly(dev, name, C):
    """The same exact case through rf.embedding(...).backward: the wrapper's stable sort."""
    B, T, _ = EMBED_LAYOUTS[name]
    dx, sid, perm, wte0, wpe0 = _embed_inputs(name, C, True)
    V = wte0.shape[0]
    idx = torch.empty_like(sid)
    idx[perm] = sid
    wte = torch.zeros(V, C, device=dev).bfloat16()
    wpe = torch.zeros(T + 3, C, device=dev).bfloat16()
    (wb, wv), (pb, pv) = carved(wte0), carved(wpe0)
    wte._ra_grad, wte._ra_direct_grad = wv, True
    wpe._ra_grad, wpe._ra_direct_grad = pv, True
    wte.requires_grad_()
    wpe.requires_grad_()
    x = rf.embedding(idx.view(B, T), wte, wpe)
    x.backward(dx.view(B, T, C))
    torch.cuda.synchronize()
    want_w, want_p, _ = embed_ref(dx.double(), sid, perm, wte0.double(), wpe0.double(), B, T, V)
    assert torch.equal(wv, want_w.float()) and torch.equal(pv, want_p.float())
    assert guards_intact(wb) and guards_intact(pb)
    assert wte.grad is None and wpe.grad is None


@gpu
@pytest.mark.parametrize("B,T,C,V", [(4, 27, 12, 24), (0, 27, 8, 24), (4, 0, 8, 24),
                                     (4, 27, 0, 24), (4, 27, 8, 0), (-1, 27, 8, 24),
                                     (4, 27, -8, 24), (4, 27, 8, -3)])
def test_embed_bwd_rejects_before_launch(dev, B, T, C, V):
    dx, sid, perm, wte0, wpe0 = _embed_inputs("run_30_98", 72, True)
    b = _run_embed(dx, sid, perm, wte0, wpe0, B, T, C, V)
    assert b["rc"] != 0
    assert torch.equal(bits(b["wte"][1]), bits(wte0)) and torch.equal(bits(b["wpe"][1]), bits(wpe0))
    assert all_nan_bits(b["work"][0])


# ------------------------------------------------------------------------------------------
# 5. ra_scale_bf16, ra_scaled_accum

GSCALE = 0.37


@gpu
@pytest.mark.parametrize("n", FLAT_SIZES)
def test_scale_bf16_is_one_multiply_one_rounding(dev, n):
    L = _lib.lib()
    x0 = _flat_inputs(n)[0].bfloat16()
    g = torch.tensor([GSCALE], device=dev)
    xb, x = carved(x0)
    assert L.ra_scale_bf16(ptr(x), n, ptr(g), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits((x0.float() * g).bfloat16()))
    assert not torch.equal(bits(x), bits(x0)) and guards_intact(xb)
    # n % 8 != 0 is refused on the host, before any launch
    xb, x = carved(x0)
    assert L.ra_scale_bf16(ptr(x), n - 4, ptr(g), stream_ptr()) != 0
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(x0))


@gpu
@pytest.mark.parametrize("n", FLAT_SIZES)
@pytest.mark.parametrize("use_g", [True, False], ids=["g", "g_null"])
@pytest.mark.parametrize("sink_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_scaled_accum_elements(dev, sink_dtype, use_g, n):
    L = _lib.lib()
    src, sink0 = _flat_inputs(n)
    sink0 = sink0.to(sink_dtype)
    g = torch.tensor([GSCALE], device=dev)
    gv = f32(GSCALE) if use_g else 1.0
    is32 = 1 if sink_dtype == torch.float32 else 0
    ref = sink0.double() + gv * src.double()
    # multiply and add, fused or not: 2 U of the operands; a bf16 sink rounds the sum once more
    mag = sink0.double().abs() + (gv * src.double()).abs()
    bound = 2 * U * mag if is32 else 2 * U * mag * (1 + 2 * H) + 2 * H * ref.abs()
    (sb, sink), (rb, s) = carved(sink0), carved(src)
    assert L.ra_scaled_accum(ptr(s), ptr(sink), n, is32, ptr(g) if use_g else None,
                             stream_ptr()) == 0
    torch.cuda.synchronize()
    u = units(sink, ref, bound)
    note(f"scaled_accum fraction of bound {str(sink_dtype)[6:]} n={n}", worst(u))
    assert worst(u) <= 1.0
    assert torch.equal(bits(s), bits(src)) and guards_intact(sb) and guards_intact(rb)
    assert not torch.equal(bits(sink), bits(sink0))
    # n % 4 != 0 is refused on the host, before any launch
    sb, sink = carved(sink0)
    assert L.ra_scaled_accum(ptr(src), ptr(sink), n - 2, is32, ptr(g), stream_ptr()) != 0
    torch.cuda.synchronize()
    assert torch.equal(bits(sink), bits(sink0))
