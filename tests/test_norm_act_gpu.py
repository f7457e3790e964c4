"""LayerNorm, GELU, bias/residual, ReLU and column-sum kernels (ops/csrc/layernorm.hip, gelu.hip,
colsum_stage1/2 in common.h) against plain fp64 references, called through their raw entry
points and checked per element, per row statistic and per column sum.

Every reference is computed once, in fp64 torch, on the kernel's own bf16 / fp32 inputs widened
to double. Everything a kernel writes, and everything a buffer load could over-read, is carved
out of a larger NaN-filled allocation (GUARD elements each side). Units: U = 2^-24 is one fp32
rounding (relative), H = 2^-9; one bf16 rounding is at most 2 H. A bound that is a COUNT of
roundings along a chain is asserted at TWICE the count. Bounds that are exhaustive as they stand
are used as they are: the order-independent summation bound, a final bf16 rounding (2 H |ref|),
and chains of one or two operations (ra_bias_residual, xout).

LayerNorm forward (one wave per row, lane holds VPL x 4 values, VPL = the instantiated vector
count: ceil(D / 256) rounded up to 1..8, 12 or 16). A value passes n1 = 4 VPL + 6 additions (4 VPL
in its lane, 6 wave levels). With A = mean_j |x_j| of the row:
  mean   |err| <= e_mean = U A (n1 + 2)        n1 additions, the rounded 1 / D, the multiply.
         On grid rows (eighths, |x| <= 2) every partial sum is exact: (2 U + U^2) |mean|, as is.
  rstd   the squares d^2 = (x - mu)^2 carry 3 roundings, pass n1 additions, then 1 / D, the
         multiply and + eps: var + eps is within (n1 + 6) U relative, PLUS e_mean^2 absolute
         (sum (x - mu)^2 / D = var + (mu - mean)^2 exactly; this is what a constant row at 100
         sees: var = 0, eps = 1e-5). rsqrtf is 1 ulp = 2 U:
         e_rs = U ((n1 + 6) / 2 + 2) + e_mean^2 / (2 (var + eps)), relative.
  y      xh = (x - mu) rs: |xh| (e_rs + 2 U) + rstd e_mean; then * g, + b (2 more roundings):
         E_y = |xh g| (e_rs + 4 U) + |g| rstd e_mean + U |b|, absolute: it scales with
         |xh g| + |b| and with A rstd (= |mean| rstd on an ill-conditioned row), never with
         |y_ref|, which cancels where xh g = -b. Bound 2 (2 H |y_ref| + E_y (1 + 2 H)).
  xout   h + (rbias + skip): two fp32 additions, one bf16 rounding:
         2 H |ref| + (2 U + U^2)(|h| + |rbias| + |skip|)(1 + 2 H), as is; grid inputs bit-equal.
         y / mean / rstd of the residual form are checked against LayerNorm of the xout it wrote.

LayerNorm backward, fed mean / rstd with absolute error e_mean and relative error e_rs (the raw
entry gets the reference's, rounded to fp32: U |mean| and U; end to end the forward's own, above).
wd = dy g, c1 = mean_j wd, c2 = mean_j wd xh, M1 = mean_j |wd|, M2 = mean_j |wd xh|:
  e_xh = rstd e_mean + |xh| (e_rs + 2 U)
  e_c1 = U (n1 + 3) M1                          product, n1 additions, 1 / D, multiply
  e_c2 = U (n1 + 4) M2 + mean_j |wd| e_xh
  o = (wd - c1 - xh c2) rs + dres, T = |wd| + |c1| + |xh c2|:
  e_o  = rstd (e_c1 + |xh| e_c2 + |c2| e_xh) + (5 U + e_rs) T rstd + U |dres|
  dx   bound 2 (2 H |dx_ref| + e_o (1 + 2 H)).
  dgamma / dbeta / dbias: a column sum of N terms in ANY order is within n U sum |terms|, n =
  N + 4 (the waves' turns at the LDS row) + the column-sum levels ceil(P / 4 S) + 3 + S + 1 (the
  sink's own value, part of sum |terms| when accumulating). Added to it, twice the terms' own
  error: |dy| e_xh + U |dy xh| for dgamma, 0 for dbeta, e_o for dbias, whose reference is the
  column sum of the UNROUNDED o (the kernel sums its fp32 o[j], not the bf16 dx). A bf16 sink
  rounds once more: bound (1 + 2 H) + 2 H |ref|.

GELU (tanh form through exp2 and rcp), u = h + bias (U |u|), k0 = sqrt(2 / pi), k1 = 0.044715:
  z = k0 (u + k1 u^3): e_z = U k0 (4 |u| + 10 k1 |u|^3) (u's error through 1 + 3 k1 u^2, the
  cube's 3 products and its constant, the addition, k0 and its product)
  e = exp2(fl(2 log2e) z): relative rho = 2 e_z + 2 U |2 z| + 2 U (the constant, the product,
  1 ulp of v_exp_f32); e + 1 rounds (U), v_rcp_f32 is 1 ulp (2 U), so r = 1 / (e + 1) is within
  rho e / (e + 1) + 3 U; with 2 r = 1 - t and e / (e + 1) = (1 + t) / 2:
  e_t = (1 - t)(rho (1 + t) / 2 + 3 U) + U |t|, ABSOLUTE: in the negative tail (u <~ -4) t = -1
  + tiny, 1 - 2 r cancels completely and the result keeps only this absolute accuracy; where
  exp2 overflows or underflows t is exactly +-1 and e_t <= U.
  y = 0.5 u (1 + t): E_y = 0.5 |u| (e_t + U (1 + t)) + 2 U |y_ref|; bound 2 (2 H |y_ref| + E_y
  (1 + 2 H)).
  gelu' = 0.5 (1 + t) + 0.5 u (1 - t^2) dz, dz = k0 (1 + 3 k1 u^2):
  e_s = 2 |t| e_t + U (1 - t^2 and its square), e_dz = U k0 (3 + 24 k1 u^2),
  B = 0.5 u (1 - t^2) dz: e_B = 0.5 |u| (e_s dz + (1 - t^2) e_dz) + 3 U |B|,
  e_dg = 0.5 (e_t + U (1 + t)) + e_B + U |gelu'|; dh = dy gelu': e_dh = |dy| e_dg + U |dh_ref|,
  bound 2 (2 H |dh_ref| + e_dh (1 + 2 H)). dbias as above with n = N + column-sum levels + 1 and
  per-term error e_dh. The v1 fallback bwd_colpart_kernel runs only when one row chunk reaches
  2 GiB; that is out of this module's reach and stays untested here.

ra_bias_residual: res + h + bias is two fp32 additions and one rounding: 2 H |ref| + (2 U + U^2)
(|res| + |h| + |bias|)(1 + 2 H), as is. ra_colsum_bf16 / ra_colsum: exact terms, the summation
bound alone. ra_bias_relu_fwd: one addition, one rounding; ra_relu_bwd_bias: dh equals
where(y > 0, dy, 0) exactly, dbias within the summation bound with n = N + 256 / F8 (LDS) +
ceil(P / 32) + 2 + 16 + 1 (colsum_final_kernel's two accumulators, their sum, 16 row lanes, sink).

Worst figures on an MI355X, as fractions of the bounds above (each test prints its own with
pytest -s). LayerNorm forward: mean 0.033, rstd 0.10, y 0.498 (the bf16 rounding alone is worth
0.5 of a doubled bound). xout 0.996 (a hard bound: a value just above a power of two rounds by
its full 2^-8). LayerNorm backward through the raw entry: dx 0.498, the sinks 0.996 (bf16 sinks,
again the final rounding). End to end through rf.layer_norm / layer_norm_fork /
residual_layer_norm, the widths 2304 .. 5120 included: y 0.497, dx 0.497, dgamma 0.992, dbeta
0.996, dbias 0.988. bias_gelu y 0.498, dh 0.498, dbias 0.995. bias_residual 0.996, colsum_bf16
0.996, bias_relu y 0.996 and dbias 0.996, ra_colsum 0.95. No element exceeded a bound, so no
kernel arithmetic changed; the one defect is the dispatch hole the width test covers (before
LN_DISPATCH rounded a vector count of 9..11 up to 12 and 13..15 up to 16, rf.layer_norm raised
at D = 2304, 2560 and 3328; at D = 5120 the rows now go through fp32 torch).
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
GUARD = 4096     # sentinel elements on each side of a carved buffer
EPS = 1e-5
K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
BF16, F32 = torch.bfloat16, torch.float32


def f32(x):
    """x as the kernel receives it: rounded to float32, widened back to double."""
    return float(np.float32(x))


@pytest.fixture(scope="module")
def dev(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"
    yield cuda_device
    _ln_inputs.cache_clear()
    _act_inputs.cache_clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------
# the references, written once (fp64 torch; work on any device)

def ln_ref(x, g, b, eps):
    """LayerNorm of the rows of x [N, D] (fp64) -> mean [N], rstd [N], xh [N, D], y [N, D]."""
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = ((d * d).mean(1) + eps).rsqrt()
    xh = d * rstd[:, None]
    return mean, rstd, xh, xh * g + b


def ln_bwd_ref(dy, x, g, mean, rstd, dres):
    """-> dx [N, D], dgamma [D], dbeta [D], colsum(dx) [D]; dres may be None."""
    xh = (x - mean[:, None]) * rstd[:, None]
    wd = dy * g
    c1 = wd.mean(1, keepdim=True)
    c2 = (wd * xh).mean(1, keepdim=True)
    dx = (wd - c1 - xh * c2) * rstd[:, None]
    if dres is not None:
        dx = dx + dres
    return dx, (dy * xh).sum(0), dy.sum(0), dx.sum(0)


def gelu_ref(u):
    """tanh-form GELU and its derivative, through sig = 1 / (1 + exp(-2 z)) = (1 + tanh z) / 2
    so that the negative tail keeps its relative accuracy -> (y, dy/du)."""
    z = K0 * (u + K1 * u ** 3)
    sig = 1.0 / (1.0 + torch.exp(-2.0 * z))
    cosig = 1.0 / (1.0 + torch.exp(2.0 * z))
    dz = K0 * (1.0 + 3.0 * K1 * u * u)
    return u * sig, sig + 2.0 * u * sig * cosig * dz


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
# the error budgets of the module docstring

def ln_vpl(D):
    """Vectors per lane of the instantiation LN_DISPATCH runs for a row of D."""
    c = (D + 255) // 256
    return c if c <= 8 else 12 if c <= 12 else 16 if c <= 16 else c


def ln_stat_budget(x, rstd, D):
    """-> (e_mean absolute [N], e_rs relative [N]) of the forward kernel's statistics."""
    n1 = 4 * ln_vpl(D) + 6
    e_mean = U * (n1 + 2) * x.abs().mean(1)
    e_rs = U * ((n1 + 6) / 2 + 2) + e_mean ** 2 * rstd ** 2 / 2
    return e_mean, e_rs


def ln_y_budget(xh, g, b, rstd, e_mean, e_rs):
    return ((xh * g).abs() * (e_rs[:, None] + 4 * U) + g.abs() * (rstd * e_mean)[:, None]
            + U * b.abs())


def ln_bwd_budget(dy, x, g, mean, rstd, dres, e_mean, e_rs, D):
    """-> e_o [N, D] (the fp32 error of dx before its rounding) and the per-term errors of the
    dgamma terms [N, D]."""
    n1 = 4 * ln_vpl(D) + 6
    rs, em, er = rstd[:, None], e_mean[:, None], e_rs[:, None]
    xh = (x - mean[:, None]) * rs
    wd = dy * g
    c1 = wd.mean(1, keepdim=True)
    c2 = (wd * xh).mean(1, keepdim=True)
    e_xh = rs * em + xh.abs() * (er + 2 * U)
    e_c1 = U * (n1 + 3) * wd.abs().mean(1, keepdim=True)
    e_c2 = U * (n1 + 4) * (wd * xh).abs().mean(1, keepdim=True) \
        + (wd.abs() * e_xh).mean(1, keepdim=True)
    T = wd.abs() + c1.abs() + (xh * c2).abs()
    e_o = rs * (e_c1 + xh.abs() * e_c2 + c2.abs() * e_xh) + (5 * U + er) * T * rs
    if dres is not None:
        e_o = e_o + U * dres.abs()
    return e_o, dy.abs() * e_xh + U * (dy * xh).abs()


def gelu_budget(u):
    """-> (E_y, e_dg): absolute fp32 errors of gelu(u) and gelu'(u) before any bf16 rounding."""
    a = u.abs()
    z = K0 * (u + K1 * u ** 3)
    t = torch.tanh(z)
    y, dg = gelu_ref(u)
    e_z = U * K0 * (4 * a + 10 * K1 * a ** 3)
    rho = 2 * e_z + 2 * U * (2 * z).abs() + 2 * U
    e_t = (1 - t) * (rho * (1 + t) / 2 + 3 * U) + U * t.abs()
    e_y = 0.5 * a * (e_t + U * (1 + t)) + 2 * U * y.abs()
    dz = K0 * (1 + 3 * K1 * u * u)
    e_s = 2 * t.abs() * e_t + U
    e_dz = U * K0 * (3 + 24 * K1 * u * u)
    B = 0.5 * u * (1 - t * t) * dz
    e_B = 0.5 * a * (e_s * dz + (1 - t * t) * e_dz) + 3 * U * B.abs()
    return e_y, 0.5 * (e_t + U * (1 + t)) + e_B + U * dg.abs()


def colsum_levels(P):
    """Additions a partial row passes in colsum_stage1 / colsum_stage2."""
    S = min(max((P + 15) // 16, 1), 32)
    return -(-P // (4 * S)) + 3 + S


def rounded(ref, fp32_err):
    """Bound of a bf16 result whose fp32 value is within fp32_err (a count) of ref."""
    return 2 * (2 * H * ref.abs() + fp32_err * (1 + 2 * H))


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
    print(f"[norm_act] {key}: " + " ".join(f"{x:.3g}" for x in vals))


# The four sink modes (bf16 sink?, accumulate?) and each entry's own encoding of them.
MODES = [(False, False), (False, True), (True, False), (True, True)]


def ln_flags(bf16, acc):      # ra_layernorm_bwd, ra_colsum: bit0 bf16, bit1 accumulate
    return (1 if bf16 else 0) | (2 if acc else 0)


def sink_flags(bf16, acc):    # ra_bias_gelu_bwd, ra_colsum_bf16, ra_relu_bwd_bias
    return (1 if acc else 0) | (0 if bf16 else 2)


def make_sink(n, bf16, acc, seed):
    """A carved sink: NaN to be overwritten (any read of it shows), or non-zero values to be
    accumulated into -> (buffer, view, old values or None)."""
    dtype = BF16 if bf16 else F32
    if not acc:
        return carved(n, dtype) + (None,)
    gen = torch.Generator().manual_seed(seed)
    old = (0.5 + torch.rand(n, generator=gen)).to(dtype).to("cuda:0")
    return carved(old) + (old,)


def check_sink(sink, ref_sum, abs_sum, err_sum, n, bf16, tag):
    """A column sum in `sink` = (buffer, view, old): within n U sum |terms| + twice the terms'
    own error, one more rounding for a bf16 sink -> worst fraction of the bound."""
    buf, view, old = sink
    old64 = torch.zeros_like(ref_sum) if old is None else old.double()
    total = ref_sum + old64
    bound = n * U * (abs_sum + old64.abs()) + 2 * err_sum
    if bf16:
        bound = bound * (1 + 2 * H) + 2 * H * total.abs()
    u = units(view, total, bound)
    assert worst(u) <= 1.0, (tag, worst(u), int(u.argmax()))
    assert guards_intact(buf), tag
    return worst(u)


# ------------------------------------------------------------------------------------------
# LayerNorm inputs: the three families

def ln_inputs_host(N, D, fam):
    """x, g, b, dy, dres, skip, rbias (bf16) from a CPU generator.
    a: randn. b: rows i % 6 = 0, 2, 3, 5 have mean +100, -8, +8, -100 and a spread of up to
    3 bf16 ulps at that magnitude; rows 1 and 4 are exactly constant (100 and -8).
    c: eighths within +-2 with g = 1, b = 0 (every fp32 partial sum of a row is exact)."""
    gen = torch.Generator().manual_seed(100003 * N + 17 * D + ord(fam))
    g = 1.0 + 0.5 * torch.randn(D, generator=gen)
    b = 0.5 * torch.randn(D, generator=gen)
    skip = 0.25 * torch.randn(N, D, generator=gen)
    rbias = 0.25 * torch.randn(D, generator=gen)
    if fam == "a":
        x = torch.randn(N, D, generator=gen)
    elif fam == "b":
        m = torch.tensor([100.0, 100.0, -8.0, 8.0, -8.0, -100.0])[torch.arange(N) % 6]
        ulp = 2.0 ** (torch.floor(torch.log2(m.abs())) - 7)
        k = torch.randint(-3, 4, (N, D), generator=gen).double()
        k[(torch.arange(N) % 3) == 1] = 0.0
        x = m[:, None] + ulp[:, None] * k
    else:
        x = torch.randint(-16, 17, (N, D), generator=gen) / 8.0
        skip = torch.randint(-16, 17, (N, D), generator=gen) / 8.0
        rbias = torch.randint(-16, 17, (D,), generator=gen) / 8.0
        g, b = torch.ones(D), torch.zeros(D)
    dy = torch.randn(N, D, generator=gen)
    dres = torch.randn(N, D, generator=gen)
    return tuple(t.to(BF16) for t in (x, g, b, dy, dres, skip, rbias))


@functools.lru_cache(maxsize=8)
def _ln_inputs(N, D, fam):
    d = torch.device("cuda", 0)
    return tuple(t.to(d) for t in ln_inputs_host(N, D, fam))


def check_ln_fwd(y, mean, rstd, x, g, b, D, fam, tag):
    """Outputs of a forward launch against LayerNorm of x (bf16, the row the kernel
    normalised) -> worst fractions (mean, rstd, y)."""
    x64, g64, b64 = x.double(), g.double(), b.double()
    rm, rr, xh, ry = ln_ref(x64, g64, b64, f32(EPS))
    e_mean, e_rs = ln_stat_budget(x64, rr, D)
    um = units(mean, rm, 2 * e_mean)
    ur = units(rstd, rr, 2 * e_rs * rr)
    uy = units(y, ry, rounded(ry, ln_y_budget(xh, g64, b64, rr, e_mean, e_rs)))
    note(f"ln_fwd mean/rstd/y {tag}", worst(um), worst(ur), worst(uy))
    assert worst(um) <= 1.0 and worst(ur) <= 1.0, (tag, um.tolist(), ur.tolist())
    assert worst(uy) <= 1.0, (tag, uy.max(1).values.tolist())
    if fam == "c":
        assert worst(units(mean, rm, (2 * U + U * U) * rm.abs())) <= 1.0, tag
    return worst(um), worst(ur), worst(uy)


def _run_ln_fwd(x, g, b, res=None):
    """One raw launch; res = (skip, rbias or None) selects the residual form."""
    N, D = x.shape
    L = _lib.lib()
    o = {"y": carved(N * D, BF16), "mean": carved(N, F32), "rstd": carved(N, F32)}
    if res is None:
        o["rc"] = L.ra_layernorm_fwd(ptr(x), ptr(g), ptr(b), ptr(o["y"][1]), ptr(o["mean"][1]),
                                     ptr(o["rstd"][1]), N, D, EPS, stream_ptr())
    else:
        o["xout"] = carved(N * D, BF16)
        o["rc"] = L.ra_residual_layernorm_fwd(
            ptr(x), ptr(res[1]), ptr(res[0]), ptr(o["xout"][1]), ptr(g), ptr(b), ptr(o["y"][1]),
            ptr(o["mean"][1]), ptr(o["rstd"][1]), N, D, EPS, stream_ptr())
    torch.cuda.synchronize()
    return o


# ------------------------------------------------------------------------------------------
# activation inputs

def act_inputs_host(N, F):
    """h [N, F], bias [F], dy [N, F], res [N, F] (bf16): u = h + bias is dense in [-12, 12];
    columns 0..5 have bias 0 and h cycling through +0, -0, 16, -16, 64, -64."""
    gen = torch.Generator().manual_seed(7919 * N + F)
    h = 24.0 * torch.rand(N, F, generator=gen) - 12.0
    bias = 0.5 * torch.randn(F, generator=gen)
    special = torch.tensor([0.0, -0.0, 16.0, -16.0, 64.0, -64.0])
    r, c = torch.meshgrid(torch.arange(N), torch.arange(6), indexing="ij")
    bias[:6] = 0.0
    h[:, :6] = special[(r + c) % 6]
    dy = torch.randn(N, F, generator=gen)
    res = torch.randn(N, F, generator=gen)
    return tuple(t.to(BF16) for t in (h, bias, dy, res))


@functools.lru_cache(maxsize=8)
def _act_inputs(N, F):
    d = torch.device("cuda", 0)
    return tuple(t.to(d) for t in act_inputs_host(N, F))


# ------------------------------------------------------------------------------------------
# 0. the references themselves, against torch in double on the CPU (no GPU needed)

def test_ln_reference_matches_torch_cpu():
    Fn = torch.nn.functional
    assert [ln_vpl(D) for D in (4, 256, 260, 2048, 2304, 3072, 3328, 4096, 5120)] == \
        [1, 1, 2, 8, 12, 12, 16, 16, 20]
    for N, D, fam in [(5, 260, "a"), (7, 64, "b"), (3, 1280, "c"), (6, 4, "a")]:
        x, g, b, dy, dres, _, _ = (t.double() for t in ln_inputs_host(N, D, fam))
        eps = f32(EPS)
        mean, rstd, xh, y = ln_ref(x, g, b, eps)
        if fam == "b":  # the rows are what the docstring says
            assert bool((x[1] == 100.0).all()) and bool((x[4] == -8.0).all())
            assert float(rstd[1]) == float(rstd[4]) and abs(float(rstd[1]) * eps ** 0.5 - 1) < 1e-12
            assert 0 < float((x[0] - 100).abs().max()) <= 1.5
            assert 0 < float((x[2] + 8).abs().max()) <= 3 / 16
        xr, gr, br = (t.clone().requires_grad_() for t in (x, g, b))
        yt = Fn.layer_norm(xr, (D,), gr, br, eps)
        assert torch.allclose(y, yt.detach(), rtol=1e-12, atol=1e-12)
        assert torch.allclose(mean, x.mean(1), rtol=1e-12, atol=1e-12)
        assert torch.allclose(rstd, (x.var(1, unbiased=False) + eps).rsqrt(), rtol=1e-12, atol=0)
        (yt * dy).sum().backward()
        dx, dg, db, cs = ln_bwd_ref(dy, x, g, mean, rstd, None)
        scale = float(xr.grad.abs().max())
        assert torch.allclose(dx, xr.grad, rtol=1e-12, atol=1e-12 * scale)
        assert torch.allclose(dg, gr.grad, rtol=1e-12, atol=1e-12 * float(gr.grad.abs().max()))
        assert torch.allclose(db, br.grad, rtol=1e-12, atol=1e-12)
        dx2, _, _, cs2 = ln_bwd_ref(dy, x, g, mean, rstd, dres)
        assert torch.allclose(dx2, xr.grad + dres, rtol=1e-12, atol=1e-12 * scale)
        assert torch.allclose(cs2, dx2.sum(0), rtol=1e-12, atol=1e-12)


def test_gelu_reference_matches_torch_cpu():
    Fn = torch.nn.functional
    h, bias, _, _ = act_inputs_host(37, 520)
    u = (h.double() + bias.double())
    assert float(u.min()) < -11.9 and float(u.max()) > 11.9
    assert {0.0, 16.0, -16.0, 64.0, -64.0} <= set(u[:, :6].flatten().tolist())
    assert bool(torch.signbit(h[:, :6]).any()) and bool((h[:, :6] == 0).any())
    ur = u.clone().requires_grad_()
    yt = Fn.gelu(ur, approximate="tanh")
    yt.sum().backward()
    y, dg = gelu_ref(u)
    assert torch.isfinite(y).all() and torch.isfinite(dg).all()
    # torch forms 1 + tanh(z), which cancels in the tail: absolute 1e-12 there
    assert torch.allclose(y, yt.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dg, ur.grad, rtol=1e-12, atol=1e-12)
    e_y, e_dg = gelu_budget(u)
    assert torch.isfinite(e_y).all() and torch.isfinite(e_dg).all()
    # the tail is where the budget is absolute: far above 2 H |ref| there
    tail = u < -6
    assert bool((e_y[tail] > 100 * y[tail].abs()).all())


def test_wide_rows_take_the_fp32_branch_cpu():
    """D > 4096: the LayerNorm helpers compute in fp32 torch, each result rounded once; the
    same bounds as the kernels' hold (checked here on the CPU, and on the GPU below)."""
    N, D = 5, 5120
    x, g, b, dy, dres, _, _ = ln_inputs_host(N, D, "b")
    x2, y, mean, rstd = rf._ln_forward(x, g, b, EPS)
    check_ln_fwd(y, mean, rstd, x, g, b, D, "b", "cpu D=5120")
    dx, dg, db, _ = rf._ln_backward(dy, x2, g, b, mean, rstd, dres=dres)
    _check_ln_grads(dx, dg, db, None, dy, x, g, dres, D, "cpu D=5120", end_to_end=True)


def _check_ln_grads(dx, dg, db, dbias, dy, x, g, dres, D, tag, end_to_end):
    """bf16 dx / dgamma / dbeta / dbias (freshly written) against the reference on x."""
    N = x.shape[0]
    x64, g64, dy64 = x.double(), g.double(), dy.double()
    dr64 = None if dres is None else dres.double()
    mean, rstd, xh, _ = ln_ref(x64, g64, torch.zeros_like(g64), f32(EPS))
    if end_to_end:
        e_mean, e_rs = ln_stat_budget(x64, rstd, D)
    else:
        e_mean, e_rs = U * mean.abs(), U * torch.ones_like(rstd)
    rdx, rdg, rdb, rcs = ln_bwd_ref(dy64, x64, g64, mean, rstd, dr64)
    e_o, e_g = ln_bwd_budget(dy64, x64, g64, mean, rstd, dr64, e_mean, e_rs, D)
    ux = units(dx, rdx, rounded(rdx, e_o))
    assert worst(ux) <= 1.0, (tag, ux.max(1).values.tolist())
    n = N + 4 + colsum_levels(min(512, (N + 7) // 8)) + 1
    fr = [worst(ux)]
    for name, got, ref, mag, err in (("dgamma", dg, rdg, (dy64 * xh).abs().sum(0), e_g.sum(0)),
                                     ("dbeta", db, rdb, dy64.abs().sum(0), 0 * rdb),
                                     ("dbias", dbias, rcs, rdx.abs().sum(0), e_o.sum(0))):
        if got is not None:
            bound = (n * U * mag + 2 * err) * (1 + 2 * H) + 2 * H * ref.abs()
            u = units(got, ref, bound)
            assert worst(u) <= 1.0, (tag, name, worst(u))
            fr.append(worst(u))
    note(f"ln grads dx/dgamma/dbeta[/dbias] {tag}", *fr)
    return fr


# ------------------------------------------------------------------------------------------
# 1. ra_layernorm_fwd, ra_residual_layernorm_fwd

LN_FWD_N = [1, 3, 4, 5, 37]
LN_FWD_D = [4, 64, 256, 260, 768, 1024, 1280, 1600, 2048, 3072, 4092, 4096]


@gpu
@pytest.mark.parametrize("D", LN_FWD_D)
def test_layernorm_fwd_elements(dev, D):
    for N in LN_FWD_N:
        for fam in "abc":
            tag = f"N={N} D={D} {fam}"
            x, g, b, _, _, _, _ = _ln_inputs(N, D, fam)
            xb, xv = carved(x)
            o = _run_ln_fwd(xv, g, b)
            assert o["rc"] == 0, tag
            check_ln_fwd(o["y"][1].view(N, D), o["mean"][1], o["rstd"][1], x, g, b, D, fam, tag)
            for k in ("y", "mean", "rstd"):
                assert guards_intact(o[k][0]), (tag, k)
            assert torch.equal(bits(xv), bits(x)) and guards_intact(xb), tag


@gpu
@pytest.mark.parametrize("D", LN_FWD_D)
def test_residual_layernorm_fwd_elements(dev, D):
    for N in LN_FWD_N:
        for fam in "abc":
            for use_rbias in (True, False):
                tag = f"N={N} D={D} {fam} rbias={use_rbias}"
                h, g, b, _, _, skip, rbias = _ln_inputs(N, D, fam)
                rb = rbias if use_rbias else None
                o = _run_ln_fwd(h, g, b, res=(skip, rb))
                assert o["rc"] == 0, tag
                xout = o["xout"][1].view(N, D)
                parts = [h.double(), skip.double()] + ([rbias.double()] if use_rbias else [])
                ref = sum(parts)
                mag = sum(p.abs() for p in parts)
                ux = units(xout, ref, 2 * H * ref.abs() + (2 * U + U * U) * mag * (1 + 2 * H))
                note(f"residual xout {tag}", worst(ux))
                assert worst(ux) <= 1.0, tag
                if fam == "c":
                    assert torch.equal(xout.double(), ref), tag
                # the kernel normalises the bf16 values it wrote
                check_ln_fwd(o["y"][1].view(N, D), o["mean"][1], o["rstd"][1], xout, g, b, D,
                             fam, tag)
                for k in ("y", "xout", "mean", "rstd"):
                    assert guards_intact(o[k][0]), (tag, k)


@gpu
@pytest.mark.parametrize("D", [6, 4100, 5120])
def test_layernorm_raw_entries_refuse_before_launch(dev, D):
    """D % 4 != 0 and D > 4096 return an error code and write nothing."""
    L = _lib.lib()
    N = 5
    x = torch.ones(N, D, device=dev, dtype=BF16)
    g = torch.ones(D, device=dev, dtype=BF16)
    stat = torch.ones(N, device=dev)
    o = _run_ln_fwd(x, g, g)
    r = _run_ln_fwd(x, g, g, res=(x, g))
    assert o["rc"] != 0 and r["rc"] != 0
    for k in ("y", "mean", "rstd"):
        assert all_nan_bits(o[k][0]) and all_nan_bits(r[k][0]), k
    assert all_nan_bits(r["xout"][0])
    dx, dg, work = carved(N * D, BF16), carved(D, F32), carved(3 * 40 * D, F32)
    rc = L.ra_layernorm_bwd(ptr(x), ptr(x), ptr(g), ptr(stat), ptr(stat), None, ptr(dx[1]),
                            ptr(dg[1]), ptr(dg[1]), None, ptr(work[1]), N, D, 0, stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and all_nan_bits(dx[0]) and all_nan_bits(dg[0]) and all_nan_bits(work[0])


# ------------------------------------------------------------------------------------------
# 2. ra_layernorm_bwd

# v1: guarded columns, a prefetched row pair up to VPL = 8; N = 4100 / 8200 reach the second
# and third grid-stride iteration of some waves (512 blocks x 4 waves x 2 rows = 4096)
LN_BWD_V1 = [(N, D) for D in (4, 260, 1280, 1600, 2048, 4096) for N in (1, 5, 8, 9, 37)] + \
    [(4100, 260), (8200, 260)]
# v2: unguarded columns, a ring of 2 rows through buffer resources
LN_BWD_V2 = [(N, D) for D in (256, 512, 768, 1024) for N in (1, 5, 37, 4099)] + [(8197, 256)]


def _run_ln_bwd(dy, x, g, mean32, rstd32, dres, sinks, N, D, flags):
    """One raw launch on carved copies of every input and a carved, NaN-filled workspace;
    sinks = (dg, db, dbias or None) as make_sink gives them."""
    L = _lib.lib()
    o = {"in": [carved(t) for t in (dy, x, mean32, rstd32)] +
         ([carved(dres)] if dres is not None else []),
         "dx": carved(N * D, BF16), "work": carved(int(L.ra_layernorm_bwd_work(N, D)), F32)}
    i = o["in"]
    o["rc"] = L.ra_layernorm_bwd(
        ptr(i[0][1]), ptr(i[1][1]), ptr(g), ptr(i[2][1]), ptr(i[3][1]),
        ptr(i[4][1]) if dres is not None else None, ptr(o["dx"][1]), ptr(sinks[0][1]),
        ptr(sinks[1][1]), ptr(sinks[2][1]) if sinks[2] is not None else None, ptr(o["work"][1]),
        N, D, flags, stream_ptr())
    torch.cuda.synchronize()
    return o


@gpu
@pytest.mark.parametrize("N,D", LN_BWD_V1 + LN_BWD_V2)
def test_layernorm_bwd_elements(dev, N, D):
    P = min(512, (N + 7) // 8)
    assert int(_lib.lib().ra_layernorm_bwd_work(N, D)) == 3 * P * D + 3 * 32 * D
    n = N + 4 + colsum_levels(P) + 1
    for fam in "ab":
        x, g, _, dy, dres_all, _, _ = _ln_inputs(N, D, fam)
        x64, g64, dy64 = x.double(), g.double(), dy.double()
        mean, rstd, xh, _ = ln_ref(x64, g64, torch.zeros_like(g64), f32(EPS))
        mean32, rstd32 = mean.float(), rstd.float()
        e_mean, e_rs = U * mean.abs(), U * torch.ones_like(rstd)
        for dres in (None, dres_all):
            dr64 = None if dres is None else dres.double()
            rdx, rdg, rdb, rcs = ln_bwd_ref(dy64, x64, g64, mean, rstd, dr64)
            e_o, e_g = ln_bwd_budget(dy64, x64, g64, mean, rstd, dr64, e_mean, e_rs, D)
            dx_bound = rounded(rdx, e_o)
            cols = [(rdg, (dy64 * xh).abs().sum(0), e_g.sum(0)),
                    (rdb, dy64.abs().sum(0), torch.zeros_like(rdb)),
                    (rcs, rdx.abs().sum(0), e_o.sum(0))]
            first = None
            for with_dbias in (False, True):
                for bf16, acc in MODES:
                    tag = (f"N={N} D={D} {fam} dres={dres is not None} dbias={with_dbias} "
                           f"bf16={bf16} acc={acc}")
                    sinks = [make_sink(D, bf16, acc, 10 + k) for k in range(3)]
                    spare = sinks[2]
                    spare_bits = bits(spare[0]).clone()
                    o = _run_ln_bwd(dy, x, g, mean32, rstd32, dres,
                                    (sinks[0], sinks[1], spare if with_dbias else None), N, D,
                                    ln_flags(bf16, acc))
                    assert o["rc"] == 0, tag
                    dx = o["dx"][1].view(N, D)
                    if first is None:
                        ux = units(dx, rdx, dx_bound)
                        assert worst(ux) <= 1.0, (tag, ux.max(1).values.tolist())
                        first, fr = bits(o["dx"][0]).clone(), [worst(ux)]
                    else:  # the sinks' mode and the third slab do not touch dx
                        assert torch.equal(bits(o["dx"][0]), first), tag
                    assert guards_intact(o["dx"][0]) and guards_intact(o["work"][0]), tag
                    for buf, _ in o["in"]:
                        assert guards_intact(buf), tag
                    for k in range(3 if with_dbias else 2):
                        fr.append(check_sink(sinks[k], *cols[k], n, bf16, tag + f" sink{k}"))
                    if not with_dbias:  # passed nowhere: untouched
                        assert torch.equal(bits(spare[0]), spare_bits), tag
            note(f"ln_bwd dx, then sinks N={N} D={D} {fam} dres={dres is not None}",
                 fr[0], max(fr[1:]))
        # the same inputs again: the same bits (the waves and the column sums add in a fixed order)
        runs = []
        for _ in range(2):
            sinks = [make_sink(D, False, True, 10 + k) for k in range(3)]
            o = _run_ln_bwd(dy, x, g, mean32, rstd32, dres_all, sinks, N, D, ln_flags(False, True))
            runs.append([bits(o["dx"][0]).clone()] + [bits(s[0]).clone() for s in sinks])
        assert all(torch.equal(p, q) for p, q in zip(*runs)), (N, D, fam)


# ------------------------------------------------------------------------------------------
# 3. end to end: the forward's own statistics feed the backward

def _rf_case(dev, which, N, D, fam):
    """One of the three public forms, forward and backward -> checks y, dx and the bf16
    parameter gradients against the composed budgets."""
    tag = f"rf.{which} N={N} D={D} {fam}"
    x0, g0, b0, dy, dres, skip0, rbias0 = _ln_inputs(N, D, fam)
    g, b = g0.clone().requires_grad_(), b0.clone().requires_grad_()
    if which == "layer_norm":
        x = x0.clone().requires_grad_()
        y = rf.layer_norm(x, g, b, EPS)
        y.backward(dy)
        xin, grads_x, dr, drb = x0, [x.grad], None, None
    elif which == "layer_norm_fork":
        x = x0.clone().requires_grad_()
        xs, y = rf.layer_norm_fork(x, g, b, EPS)
        torch.autograd.backward([xs, y], [dres, dy])
        assert torch.equal(bits(xs.detach()), bits(x0)), tag
        xin, grads_x, dr, drb = x0, [x.grad], dres, None
    else:
        h, skip = x0.clone().requires_grad_(), skip0.clone().requires_grad_()
        rbias = rbias0.clone().requires_grad_()
        xo, y = rf.residual_layer_norm(h, rbias, skip, g, b, EPS)
        torch.autograd.backward([xo, y], [dres, dy])
        parts = [x0.double(), skip0.double(), rbias0.double()]
        ref = sum(parts)
        bound = 2 * H * ref.abs() + (2 * U + U * U) * sum(p.abs() for p in parts) * (1 + 2 * H)
        assert worst(units(xo.detach(), ref, bound)) <= 1.0, tag
        xin, grads_x, dr, drb = xo.detach(), [h.grad, skip.grad], dres, rbias.grad
    torch.cuda.synchronize()
    x64, g64, b64 = xin.double(), g0.double(), b0.double()
    mean, rstd, xh, ry = ln_ref(x64, g64, b64, f32(EPS))
    e_mean, e_rs = ln_stat_budget(x64, rstd, D)
    uy = units(y.detach(), ry, rounded(ry, ln_y_budget(xh, g64, b64, rstd, e_mean, e_rs)))
    note(f"y {tag}", worst(uy))
    assert worst(uy) <= 1.0, (tag, uy.max(1).values.tolist())
    for gx in grads_x:
        _check_ln_grads(gx, g.grad, b.grad, drb, dy, xin, g0, dr, D, tag, end_to_end=True)


RF_FORMS = ["layer_norm", "layer_norm_fork", "residual_layer_norm"]


@gpu
@pytest.mark.parametrize("which", RF_FORMS)
@pytest.mark.parametrize("D", [768, 1600])
def test_rf_layer_norm_forms_end_to_end(dev, D, which):
    for fam in "ab":
        _rf_case(dev, which, 37, D, fam)


@gpu
@pytest.mark.parametrize("which", RF_FORMS)
@pytest.mark.parametrize("D", [2304, 2560, 3328, 5120])
def test_rf_layer_norm_widths_between_instantiations(dev, D, which):
    """ceil(D / 256) in 9..11 and 13..15 has no instantiation of its own and runs the next one
    up (12, 16); D > 4096 computes in fp32 torch. Neither raises; both meet the same bounds."""
    for fam in "ab":
        _rf_case(dev, which, 5, D, fam)


# ------------------------------------------------------------------------------------------
# 4. ra_bias_gelu_fwd / ra_bias_gelu_bwd

ACT_F = [8, 64, 520, 3072]
ACT_N = [1, 2, 3, 31, 33, 37, 100]
ACT_CASES = [(N, F) for F in ACT_F for N in ACT_N] + [(8200, 64)]


def test_act_cases_reach_the_chunk_edges():
    """parts_for: P = 1, 2, 4 and 257 with odd and even rows per chunk."""
    def parts(N, F):
        bx = (F // 8 + 63) // 64
        return min(max(-(-8192 // bx), 256), max((N + 31) // 32, 1))
    got = {N: (parts(N, 64), -(-N // parts(N, 64))) for N in ACT_N + [8200]}
    assert got == {1: (1, 1), 2: (1, 2), 3: (1, 3), 31: (1, 31), 33: (2, 17), 37: (2, 19),
                   100: (4, 25), 8200: (257, 32)}


def _colsum_n(N, F):
    P = int(_lib.lib().ra_colsum_parts(N, F))
    return N + colsum_levels(P) + 1


@gpu
@pytest.mark.parametrize("N,F", ACT_CASES)
def test_bias_gelu_fwd_bwd_elements(dev, N, F):
    L = _lib.lib()
    h, bias, dy, _ = _act_inputs(N, F)
    u = h.double() + bias.double()
    ry, rdg = gelu_ref(u)
    e_y, e_dg = gelu_budget(u)
    yb, y = carved(N * F, BF16)
    assert L.ra_bias_gelu_fwd(ptr(h), ptr(bias), ptr(y), N, F, stream_ptr()) == 0
    torch.cuda.synchronize()
    uy = units(y.view(N, F), ry, rounded(ry, e_y))
    assert worst(uy) <= 1.0, (N, F, uy.max(1).values.tolist())
    assert guards_intact(yb) and bool(torch.isfinite(y).all())
    rdh = dy.double() * rdg
    e_dh = dy.double().abs() * e_dg + U * rdh.abs()
    dh_bound = rounded(rdh, e_dh)
    n = _colsum_n(N, F)
    fr, first = [], None
    for bf16, acc in MODES:
        tag = f"N={N} F={F} bf16={bf16} acc={acc}"
        sink = make_sink(F, bf16, acc, 3)
        ins = [carved(t) for t in (dy, h)]  # a chunk's buffer resource ends inside these
        dhb, dh = carved(N * F, BF16)
        wb, work = carved(int(L.ra_colsum_work(N, F)), F32)
        rc = L.ra_bias_gelu_bwd(ptr(ins[0][1]), ptr(ins[1][1]), ptr(bias), ptr(dh), ptr(sink[1]),
                                ptr(work), N, F, sink_flags(bf16, acc), stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, tag
        if first is None:
            ud = units(dh.view(N, F), rdh, dh_bound)
            assert worst(ud) <= 1.0, (tag, ud.max(1).values.tolist())
            first = bits(dhb).clone()
        assert torch.equal(bits(dhb), first), tag  # also: a second run gives the same bits
        assert guards_intact(dhb) and guards_intact(wb) and bool(torch.isfinite(dh).all()), tag
        fr.append(check_sink(sink, rdh.sum(0), rdh.abs().sum(0), e_dh.sum(0), n, bf16, tag))
        if (bf16, acc) == MODES[0]:
            keep = bits(sink[0]).clone()
    sink = make_sink(F, *MODES[0], 3)
    wb, work = carved(int(L.ra_colsum_work(N, F)), F32)
    dhb, dh = carved(N * F, BF16)
    assert L.ra_bias_gelu_bwd(ptr(ins[0][1]), ptr(ins[1][1]), ptr(bias), ptr(dh), ptr(sink[1]),
                              ptr(work), N, F, sink_flags(*MODES[0]), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(sink[0]), keep) and torch.equal(bits(dhb), first)
    note(f"bias_gelu y / dh / dbias N={N} F={F}", worst(uy), worst(ud), max(fr))


# ------------------------------------------------------------------------------------------
# 5. ra_bias_residual, ra_colsum_bf16

@gpu
@pytest.mark.parametrize("N,F", ACT_CASES)
def test_bias_residual_and_colsum_bf16(dev, N, F):
    L = _lib.lib()
    h, bias, dy, res = _act_inputs(N, F)
    for use_bias in (True, False):
        parts = [res.double(), h.double()] + ([bias.double().expand(N, F)] if use_bias else [])
        ref, mag = sum(parts), sum(p.abs() for p in parts)
        yb, y = carved(N * F, BF16)
        assert L.ra_bias_residual(ptr(h), ptr(bias) if use_bias else None, ptr(res), ptr(y), N, F,
                                  stream_ptr()) == 0
        torch.cuda.synchronize()
        uy = units(y.view(N, F), ref, 2 * H * ref.abs() + (2 * U + U * U) * mag * (1 + 2 * H))
        assert worst(uy) <= 1.0 and guards_intact(yb), (N, F, use_bias, worst(uy))
        # eighths: the fp32 sum is exact, one rounding is left
        gen = torch.Generator().manual_seed(N + F)
        gh, gr = ((torch.randint(-64, 65, (N, F), generator=gen) / 8.0).to(BF16).to(dev)
                  for _ in range(2))
        gb = (torch.randint(-64, 65, (F,), generator=gen) / 8.0).to(BF16).to(dev)
        yb, y = carved(N * F, BF16)
        assert L.ra_bias_residual(ptr(gh), ptr(gb) if use_bias else None, ptr(gr), ptr(y), N, F,
                                  stream_ptr()) == 0
        torch.cuda.synchronize()
        exact = gh.double() + gr.double() + (gb.double() if use_bias else 0.0)
        assert torch.equal(bits(y.view(N, F)), bits(exact.float().to(BF16))) and guards_intact(yb)
    n = _colsum_n(N, F)
    x64 = dy.double()
    fr = []
    for bf16, acc in MODES:
        tag = f"colsum_bf16 N={N} F={F} bf16={bf16} acc={acc}"
        sink = make_sink(F, bf16, acc, 5)
        xb, xv = carved(dy)
        wb, work = carved(int(L.ra_colsum_work(N, F)), F32)
        assert L.ra_colsum_bf16(ptr(xv), ptr(sink[1]), ptr(work), N, F, sink_flags(bf16, acc),
                                stream_ptr()) == 0, tag
        torch.cuda.synchronize()
        fr.append(check_sink(sink, x64.sum(0), x64.abs().sum(0), torch.zeros(F, device=dev,
                                                                             dtype=torch.float64),
                             n, bf16, tag))
        assert guards_intact(wb) and guards_intact(xb), tag
    note(f"bias_residual y / colsum_bf16 N={N} F={F}", worst(uy), max(fr))


# ------------------------------------------------------------------------------------------
# 6. ra_bias_relu_fwd / ra_relu_bwd_bias

def _relu_parts(N, F):
    rpi = 256 // (F // 8)
    rpb = max(-(-(-(-N // 512)) // rpi) * rpi, rpi)
    return -(-N // rpb), rpi


def test_relu_cases_reach_both_row_walks():
    assert [_relu_parts(N, F)[0] for N, F in ((1, 32), (7, 2048), (1000, 32), (1000, 64),
                                              (1000, 2048))] == [1, 7, 16, 32, 500]


@gpu
@pytest.mark.parametrize("F", [32, 64, 256, 2048])
@pytest.mark.parametrize("N", [1, 7, 33, 1000])
def test_bias_relu_fwd_bwd_elements(dev, N, F):
    L = _lib.lib()
    gen = torch.Generator().manual_seed(31 * N + F)
    h = torch.randn(N, F, generator=gen).to(BF16).to(dev)
    bias = (0.5 * torch.randn(F, generator=gen)).to(BF16).to(dev)
    h[:, 0] = -bias[0]  # h + bias = 0
    dy = torch.randn(N, F, generator=gen).to(BF16).to(dev)
    ref = (h.double() + bias.double()).clamp_min(0.0)
    yb, y = carved(N * F, BF16)
    assert L.ra_bias_relu_fwd(ptr(h), ptr(bias), ptr(y), N, F, stream_ptr()) == 0
    torch.cuda.synchronize()
    bound = 2 * H * ref.abs() + U * (h.double().abs() + bias.double().abs()) * (1 + 2 * H)
    uy = units(y.view(N, F), torch.where(ref > 0, ref, 0 * ref), torch.where(ref > 0, bound, 0 * ref))
    assert worst(uy) <= 1.0 and guards_intact(yb), (N, F, worst(uy))
    # backward on a y of its own: positives, +0 and -0
    yin = y.view(N, F).clone()
    yin[:, 1], yin[:, 2] = 0.0, -0.0
    assert bool(torch.signbit(yin[:, 2]).all()) and not bool(torch.signbit(yin[:, 1]).any())
    rdh = torch.where(yin > 0, dy, torch.zeros_like(dy))
    P, rpi = _relu_parts(N, F)
    assert int(L.ra_relu_bwd_work(N, F)) == P * F
    n = N + rpi + -(-P // 32) + 2 + 16 + 1
    fr = []
    for bf16, acc in MODES:
        tag = f"relu N={N} F={F} bf16={bf16} acc={acc}"
        sink = make_sink(F, bf16, acc, 9)
        dhb, dh = carved(N * F, BF16)
        wb, work = carved(P * F, F32)
        assert L.ra_relu_bwd_bias(ptr(dy), ptr(yin), ptr(dh), ptr(sink[1]), ptr(work), N, F,
                                  sink_flags(bf16, acc), stream_ptr()) == 0, tag
        torch.cuda.synchronize()
        assert torch.equal(dh.view(N, F), rdh) and guards_intact(dhb) and guards_intact(wb), tag
        fr.append(check_sink(sink, rdh.double().sum(0), rdh.double().abs().sum(0),
                             torch.zeros(F, device=dev, dtype=torch.float64), n, bf16, tag))
    note(f"bias_relu y / dbias N={N} F={F} P={P}", worst(uy), max(fr))


@gpu
@pytest.mark.parametrize("N,F", [(7, 12), (7, 24), (7, 4104), (0, 64), (-1, 64)])
def test_relu_bwd_bias_refuses_before_launch(dev, N, F):
    L = _lib.lib()
    if F % 8 or 256 % (F // 8):
        assert int(L.ra_relu_bwd_work(N, F)) == -1
    t = torch.ones(8, 4104, device=dev, dtype=BF16)
    dhb, dh = carved(t.numel(), BF16)
    sb, sink = carved(4104, F32)
    wb, work = carved(8 * 4104, F32)
    assert L.ra_relu_bwd_bias(ptr(t), ptr(t), ptr(dh), ptr(sink), ptr(work), N, F, 2,
                              stream_ptr()) != 0
    torch.cuda.synchronize()
    assert all_nan_bits(dhb) and all_nan_bits(sb) and all_nan_bits(wb)


# ------------------------------------------------------------------------------------------
# 7. ra_colsum

@gpu
@pytest.mark.parametrize("D", [4, 64, 260])
@pytest.mark.parametrize("P", [1, 16, 17, 512, 513])
def test_colsum_partials(dev, P, D):
    """S = 1 (P <= 16), S = 2, the cap S = 32, and a last stage-1 split that is partial."""
    L = _lib.lib()
    gen = torch.Generator().manual_seed(P * 1000 + D)
    part = torch.randn(P, D, generator=gen).to(dev)
    p64 = part.double()
    n = colsum_levels(P) + 1
    fr = []
    for bf16, acc in MODES:
        tag = f"colsum P={P} D={D} bf16={bf16} acc={acc}"
        sink = make_sink(D, bf16, acc, 21)
        pb, pv = carved(part)
        sb, scratch = carved(32 * D, F32)
        assert L.ra_colsum(ptr(pv), ptr(scratch), ptr(sink[1]), P, D, ln_flags(bf16, acc),
                           stream_ptr()) == 0, tag
        torch.cuda.synchronize()
        fr.append(check_sink(sink, p64.sum(0), p64.abs().sum(0), torch.zeros_like(p64[0]), n,
                             bf16, tag))
        assert guards_intact(sb) and guards_intact(pb), tag
    note(f"colsum P={P} D={D}", max(fr))
