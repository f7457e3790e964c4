"""Optimizer kernels (ops/csrc/optim.hip) against one plain fp64 reference.

Gradient clipping, flat AdamW (plain, W^T-refreshing, scalar fp32), SGD-momentum: every value
check is per element, in units of 2^-24 (one fp32 rounding) of the operands the kernel
actually combined, so a wrong decay group, bias correction or gradient scale (thousands of
units) cannot hide behind a tensor norm.

Every hyper-parameter enters the reference as its float32 value widened to double: the kernels
receive floats, and 1 - float32(0.9) is 4 fp32 ulps away from 0.1.

Bias corrections: the entry points form 1/(1 - powf(b, t)) in fp32. Where 1 - b^t is small
that subtraction amplifies powf's half-ulp rounding by b^t / (1 - b^t): 500 x for b2 = 0.999
at t = 2 (up to 1.5e-5 relative in the correction, 6.6e-6 with glibc's powf). That is the entry point's documented fp32 host
arithmetic, not element math, so the element-math cases keep b^t / (1 - b^t) < 10
(betas (0.9, 0.95) at t = 1, 2, 37; (0.9, 0.999) at t = 1 and 1000) and the trajectory tests
(rtol 1e-4) carry b2 = 0.999 through t = 2, 3, 4.

Worst figures on an MI355X (budget 32 units; each test prints its own with pytest -s):
ra_adamw_flat_dev p 5.0 / m 2.4 / v 3.8 units, ra_adamw_flat_wt 3.7 / 1.7 / 3.2,
ra_adamw_f32 7.0 / 2.3 / 3.5, ra_sgd_flat p 2.0 / buf 2.7; clip norm 4.7e-8 relative (fp32),
3.7e-8 (bf16), against a bound of 1e-5.
"""

import functools
import math

import numpy as np
import pytest
import torch

from ray_amd.ops import _lib
from ray_amd.ops._lib import ptr, stream_ptr

gpu = pytest.mark.gpu

U = 2.0 ** -24  # one fp32 rounding, relative to its operands
K = 32          # per-element budget in those units: the chain has < 16 fp32 roundings
GUARD = 4096    # sentinel elements on each side of a carved buffer (a multiple of 8)
BIG1D = 2048 * 256 * 4  # elements one full ra_grid(…, 256) pass of float4 threads covers
BIGSUM = 1024 * 256 * 4  # elements one pass of the fixed 1024-block sum-of-squares grid covers


def f32(x):
    """x as the kernel receives it: rounded to float32, widened back to double."""
    return float(np.float32(x))


@pytest.fixture(scope="module")
def dev(cuda_device):
    assert _lib.available(), "libray_amd_hip.so must load on a GPU box"
    yield cuda_device
    # hand the shared inputs and the allocator's cached blocks back, so the modules that run
    # after this one start from the same allocator state as without it
    _elem_inputs.cache_clear()
    _clip_inputs.cache_clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------
# the reference, written once (fp64 torch; works on any device)

def rbc(b, t):
    """1 / (1 - b^t) of the float32 beta."""
    return 1.0 / (1.0 - f32(b) ** t)


def adam_ref(p, g, m, v, *, sc, lr, b1, b2, eps, wd, n_decay, rbc1, rbc2):
    """One AdamW step on fp64 tensors -> (p', m', v', upd, gr)."""
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    gr = g * sc
    m2 = b1 * m + (1.0 - b1) * gr
    v2 = b2 * v + (1.0 - b2) * gr * gr
    upd = (m2 * rbc1) / ((v2 * rbc2).sqrt() + eps)
    decay = torch.ones_like(p)
    decay[:n_decay] = 1.0 - lr * wd
    return p * decay - lr * upd, m2, v2, upd, gr


def sgd_ref(p, g, buf, *, sc, lr, mom, wd):
    """One SGD-momentum step on fp64 tensors -> (p', buf')."""
    lr, mom, wd = f32(lr), f32(mom), f32(wd)
    gr = g * sc + wd * p
    b2 = mom * buf + gr
    return p - lr * b2, b2


def clip_norm_ref(g, pre_scale):
    return math.sqrt(float((g.double() ** 2).sum())) * f32(pre_scale)


def clip_scale_ref(norm, max_norm, pre_scale):
    max_norm, pre_scale = f32(max_norm), f32(pre_scale)
    if max_norm > 0.0 and norm > max_norm:
        return pre_scale * (max_norm / (norm + f32(1e-6)))
    return pre_scale


def units(got, ref, scale):
    """max over elements of |got - ref| in units of 2^-24 * scale (inf where scale is 0 and
    the values differ; NaN where got is NaN, which fails every `<=`)."""
    err = (got.double() - ref).abs()
    bound = U * scale
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, float("inf")))
    return float(r.max())


def adam_units(p, m, v, ref, p_old, m_old, *, lr, b1):
    """(p, m, v) errors in the issue's units: p against |p_old| + lr |upd|, m against
    |b1 m_old| + |(1 - b1) gr|, v against v_ref."""
    p_ref, m_ref, v_ref, upd, gr = ref
    lr, b1 = f32(lr), f32(b1)
    return (units(p, p_ref, p_old.abs() + lr * upd.abs()),
            units(m, m_ref, (b1 * m_old).abs() + ((1.0 - b1) * gr).abs()),
            units(v, v_ref, v_ref))


# ------------------------------------------------------------------------------------------
# helpers

_ITYPE = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def bits(t):
    return t.view(_ITYPE[t.dtype])


def carved(src, dtype=None):
    """`src` (a tensor, or a length to leave NaN-filled) copied into the middle of a larger
    NaN-filled allocation -> (whole buffer, view)."""
    if isinstance(src, int):
        n, device = src, torch.device("cuda", 0)
    else:
        n, device, dtype = src.numel(), src.device, dtype or src.dtype
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=device, dtype=dtype)
    view = buf[GUARD:GUARD + n]
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
    print(f"[optim] {key}: " + " ".join(f"{x:.3g}" for x in vals))


# ------------------------------------------------------------------------------------------
# 1. the reference itself, on the CPU path of FlatAdamW (no GPU needed)

class _Small(torch.nn.Module):
    """2-D weights and 1-D parameters whose sizes are no multiples of 64: padding exists."""

    def __init__(self):
        super().__init__()
        mk = lambda *s: torch.nn.Parameter(torch.randn(*s))  # noqa: E731
        self.w1, self.b1 = mk(37, 20), mk(37)
        self.w2, self.b2 = mk(5, 37), mk(5)
        self.w3, self.b3 = mk(130, 3), mk(130)
        self.s = mk(1)


def _padding_mask(flat):
    pad = torch.ones(flat.numel, dtype=torch.bool, device=flat.device)
    for (_, p), off in zip(flat.order, flat.offsets):
        pad[off:off + p.numel()] = False
    return pad


def _write_grads(flat, gen, norm_target, pre_scale):
    """Fresh random gradients in the parameters' own views, sized so that the pre-scaled
    global norm is ~norm_target; padding gradients stay 0."""
    n_real = sum(p.numel() for _, p in flat.order)
    amp = norm_target / (pre_scale * math.sqrt(n_real))
    for _, p in flat.order:
        g = torch.randn(p.shape, generator=gen) * amp
        p._ra_grad.copy_(g.to(p._ra_grad.device))


class _Traj:
    """The fp64 reference carried along a FlatAdamW trajectory."""

    def __init__(self, flat, opt):
        self.flat, self.opt = flat, opt
        self.p = flat.p32.double().clone()
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.t = 0
        self.norm = None

    def step(self, lr=None, sc=None, g=None):
        """Advance by the gradient `g` (default: what flat.g holds now, so call it before an
        optimizer that clears the gradient). `sc`: use this gradient scale instead of the
        fp64 clip scale."""
        o = self.opt
        g = self.flat.g.double() if g is None else g
        self.t += 1
        self.norm = clip_norm_ref(g, o.grad_scale)
        if sc is None:
            sc = clip_scale_ref(self.norm, o.max_grad_norm or 0.0, o.grad_scale)
        self.p_old, self.m_old = self.p, self.m
        self.ref = adam_ref(self.p, g, self.m, self.v, sc=sc, lr=o.lr if lr is None else lr,
                            b1=o.b1, b2=o.b2, eps=o.eps, wd=o.wd, n_decay=self.flat.n_decay,
                            rbc1=rbc(o.b1, self.t), rbc2=rbc(o.b2, self.t))
        self.p, self.m, self.v = self.ref[:3]


def _close(got, ref):
    # the constants test_flat_adamw_matches_torch uses for a 5-step trajectory: the clip
    # scale's 1e-5 relative error feeds every element
    return torch.allclose(got.double(), ref, atol=1e-5, rtol=1e-4)


def test_reference_matches_flat_adamw_cpu_path():
    from ray_amd.parallel.flat import FlatAdamW, FlatParams

    torch.manual_seed(5)
    flat = FlatParams(_Small(), dtype=torch.float32)
    assert not flat.p32.is_cuda and flat.numel > sum(p.numel() for p in flat.params())
    opt = FlatAdamW(flat, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1,
                    max_grad_norm=1.0, grad_scale=0.25)
    ref = _Traj(flat, opt)
    gen = torch.Generator().manual_seed(6)
    pad = _padding_mask(flat)
    for target in (3.0, 0.3, 2.0):  # clipped, not clipped, clipped
        _write_grads(flat, gen, target, opt.grad_scale)
        ref.step()
        opt.step()
        assert abs(float(opt.last_norm) - ref.norm) <= 1e-5 * ref.norm
        assert (ref.norm > 1.0) == (target > 1.0)
        assert _close(flat.p32, ref.p) and _close(opt.m, ref.m) and _close(opt.v, ref.v)
        assert not flat.p32[pad].any() and not opt.m[pad].any() and not opt.v[pad].any()
    # the trajectory moved: the comparison above is not between two untouched buffers
    assert float((ref.p - ref.p_old).abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------
# 2. AdamW element math through ra_adamw_flat_dev

SIZES = [BIG1D + 4 * 777, 4, 1028]
# (step, betas, eps, wd): FlatAdamW's defaults, then the RLlib learner's settings
STEPS = {1: (1, (0.9, 0.95), 1e-8, 0.1), 2: (2, (0.9, 0.95), 1e-8, 0.1),
         37: (37, (0.9, 0.95), 1e-8, 0.1), 1000: (1000, (0.9, 0.999), 1e-7, 0.0)}
LR = 3e-3
GSCALE = 0.37


def _elem_inputs_host(n):
    """p, g, m, v (fp32) and the mask of padding-like elements, from a CPU generator: the
    same values on every machine.
    g: randn times a log-spaced scale 1e-4 .. 10 (shuffled, so every grid-stride iteration
    sees the whole range), every 17th exactly 0. Two blocks have g = m = v = 0 as alignment
    padding does: [256, 320) with p = 0 too, and the last 64 elements with live p."""
    gen = torch.Generator().manual_seed(77 + n)
    scale = torch.logspace(-4, 1, n)[torch.randperm(n, generator=gen)]
    g = torch.randn(n, generator=gen) * scale
    g[::17] = 0.0
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * scale * 0.5
    v = (torch.randn(n, generator=gen) * scale) ** 2
    zero = torch.zeros(n, dtype=torch.bool)
    if n >= 1028:
        zero[256:320] = True
        p[256:320] = 0.0
        zero[n - 64:] = True
        for t in (g, m, v):
            t[zero] = 0.0
    return p, g, m, v, zero


@functools.lru_cache(maxsize=None)
def _elem_inputs(n):
    d = torch.device("cuda", 0)
    return tuple(t.to(d) for t in _elem_inputs_host(n))


def _run_adamw(entry, p0, g0, m0, v0, *, n_decay, lr, betas, eps, wd, step, gscale, flags,
               hyper=None, with_p16=True, n=None):
    """One raw launch on carved copies of the inputs -> dict of (buffer, view) pairs."""
    L = _lib.lib()
    b = {"p": carved(p0), "g": carved(g0), "m": carved(m0), "v": carved(v0),
         "p16": carved(p0.numel(), torch.bfloat16)}
    n = p0.numel() if n is None else n
    args = [ptr(b["p"][1]), ptr(b["p16"][1]) if with_p16 else None, ptr(b["g"][1]),
            ptr(b["m"][1]), ptr(b["v"][1]), n, n_decay, lr, betas[0], betas[1], eps, wd, step,
            ptr(gscale), flags]
    if entry == "ra_adamw_flat_dev":
        args.append(ptr(hyper))
    b["rc"] = getattr(L, entry)(*args, stream_ptr())
    torch.cuda.synchronize()
    return b


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("step", sorted(STEPS))
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_adamw_flat_dev_elements(dev, flags, step, n):
    t, betas, eps, wd = STEPS[step]
    p0, g0, m0, v0, zero = _elem_inputs(n)
    if t == 1:
        m0, v0 = torch.zeros_like(m0), torch.zeros_like(v0)
    gk = g0 if flags & 1 else g0.bfloat16()
    gscale = torch.tensor([GSCALE], device=dev)
    p64, g64, m64, v64 = (x.double() for x in (p0, gk, m0, v0))
    half = n // 2 // 4 * 4
    decays = sorted({0, 4, half, n}) if wd else [half]
    for use_hyper in (False, True):
        if use_hyper:
            # the host lr / step are deliberately wrong: the kernel must read the device ones
            hyper = torch.tensor([LR, 1.0 / (1.0 - f32(betas[0]) ** t),
                                  1.0 / (1.0 - f32(betas[1]) ** t), 0.0], device=dev)
            lr_arg, step_arg = 7.0 * LR, t + 5
            rbc1, rbc2 = float(hyper[1]), float(hyper[2])
        else:
            hyper, lr_arg, step_arg = None, LR, t
            rbc1, rbc2 = rbc(betas[0], t), rbc(betas[1], t)
        for with_p16 in (True, False):
            for nd in decays:
                tag = f"flags={flags} step={t} n={n} hyper={use_hyper} p16={with_p16} nd={nd}"
                ref = adam_ref(p64, g64, m64, v64, sc=f32(GSCALE), lr=LR, b1=betas[0],
                               b2=betas[1], eps=eps, wd=wd, n_decay=nd, rbc1=rbc1, rbc2=rbc2)
                b = _run_adamw("ra_adamw_flat_dev", p0, gk, m0, v0, n_decay=nd, lr=lr_arg,
                               betas=betas, eps=eps, wd=wd, step=step_arg, gscale=gscale,
                               flags=flags, hyper=hyper, with_p16=with_p16)
                assert b["rc"] == 0, tag
                p, m, v, g, p16 = (b[k][1] for k in ("p", "m", "v", "g", "p16"))
                up, um, uv = adam_units(p, m, v, ref, p64, m64, lr=LR, b1=betas[0])
                note(f"adamw_flat_dev units p/m/v flags={flags} step={t}", up, um, uv)
                assert up <= K and um <= K and uv <= K, (tag, up, um, uv)
                # both sides of the decay boundary, explicitly: within the bound of the right
                # group's reference, and outside the bound of the wrong group's wherever the
                # two references are further apart than the bounds
                lo, hi = max(nd - 4, 0), min(nd + 4, n)
                if wd and lo < hi:
                    s = slice(lo, hi)
                    bound = K * U * (p64[s].abs() + f32(LR) * ref[3][s].abs())
                    idx = torch.arange(lo, hi, device=dev)
                    wrong = p64[s] * torch.where(idx < nd, 1.0, 1.0 - f32(LR) * f32(wd)) \
                        - f32(LR) * ref[3][s]
                    differs = (wrong - ref[0][s]).abs() > 2 * bound
                    assert ((p[s].double() - ref[0][s]).abs() <= bound).all(), tag
                    assert ((p[s].double() - wrong).abs() > bound)[differs].all(), tag
                    assert differs.any(), tag
                # padding-like elements: untouched state, no NaN
                assert torch.isfinite(p).all() and torch.isfinite(m).all() \
                    and torch.isfinite(v).all(), tag
                if zero.any():
                    assert not m[zero].any() and not v[zero].any(), tag
                    assert torch.equal(bits(p[256:320]), bits(p0[256:320])), tag
                    if nd < n or not wd:
                        assert torch.equal(bits(p[n - 64:]), bits(p0[n - 64:])), tag
                # the bf16 mirror rounds the kernel's own p32 to nearest even
                if with_p16:
                    assert torch.equal(bits(p16), bits(p.bfloat16())), tag
                else:
                    assert all_nan_bits(b["p16"][0]), tag
                # ZERO clears the gradient in the same pass; without it g is not written
                if flags & 2:
                    assert not bits(g).any(), tag
                else:
                    assert torch.equal(bits(g), bits(gk)), tag
                for k in ("p", "g", "m", "v", "p16"):
                    assert guards_intact(b[k][0]), (tag, k)


@gpu
@pytest.mark.parametrize("n,nd", [(1030, 512), (1028, 2), (1027, 0), (1028, 1027)])
def test_adamw_flat_dev_rejects_unaligned_sizes_before_launch(dev, n, nd):
    p0, g0, m0, v0, _ = _elem_inputs(1032)
    gscale = torch.tensor([GSCALE], device=dev)
    for flags in range(4):
        gk = g0 if flags & 1 else g0.bfloat16()
        b = _run_adamw("ra_adamw_flat_dev", p0, gk, m0, v0, n_decay=nd, lr=LR,
                       betas=(0.9, 0.95), eps=1e-8, wd=0.1, step=3, gscale=gscale, flags=flags,
                       n=n)
        assert b["rc"] != 0
        for k, src in (("p", p0), ("g", gk), ("m", m0), ("v", v0)):
            assert torch.equal(bits(b[k][1]), bits(src)), k
        assert all_nan_bits(b["p16"][0])


# ------------------------------------------------------------------------------------------
# 3. ra_grad_clip

CLIP_SIZES = [(torch.bfloat16, BIGSUM + 4 * 333), (torch.bfloat16, 4),
              (torch.float32, BIGSUM + 4 * 333), (torch.float32, 4),
              (torch.float32, 1), (torch.float32, 1027), (torch.float32, BIGSUM + 3)]


@functools.lru_cache(maxsize=None)
def _clip_inputs(dtype, n):
    """A unit-scale gradient; where n is no multiple of 4 the last (up to) 3 elements, which
    only the scalar tail loop reads, are 100: dropping one moves the norm far beyond 1e-5."""
    gen = torch.Generator().manual_seed(300 + n)
    g = torch.randn(n, generator=gen)
    if n % 4:
        g[-3:] = 100.0
    return g.to(dtype).to(torch.device("cuda", 0))


def _run_clip(g, n, max_norm, pre_scale):
    L = _lib.lib()
    gb, gv = carved(g)
    work = torch.full((L.ra_norm_parts(),), float("nan"), device=g.device)
    out = torch.full((2,), float("nan"), device=g.device)
    rc = L.ra_grad_clip(ptr(gv), n, 1 if g.dtype == torch.bfloat16 else 0, max_norm, pre_scale,
                        ptr(work), ptr(out[:1]), ptr(out[1:]), stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(gb) and torch.equal(bits(gv), bits(g))
    return rc, out[0].item(), out[1].item(), work


@gpu
@pytest.mark.parametrize("dtype,n", CLIP_SIZES, ids=lambda x: str(x).replace("torch.", ""))
def test_grad_clip_norm_and_scale(dev, dtype, n):
    g = _clip_inputs(dtype, n)
    raw = clip_norm_ref(g, 1.0)  # of the stored (bf16-rounded) values, exact in fp32
    third = 1.0 / 3.0
    # (max_norm, pre_scale, scale must be exactly pre_scale)
    cases = [(0.0, 1.0, True), (0.0, third, True)]
    for ps in (1.0, 0.125, third):
        cases += [(2.0 * raw * ps, ps, True), (0.5 * raw * ps, ps, False)]
    # pre_scale alone decides the branch: raw norm above max_norm, scaled norm below it
    cases.append((0.5 * raw, 0.125, True))
    for max_norm, ps, exact in cases:
        tag = f"{dtype} n={n} max_norm={max_norm} pre_scale={ps}"
        rc, sc, norm, work = _run_clip(g, n, max_norm, ps)
        assert rc == 0, tag
        want = raw * f32(ps)
        rel = abs(norm - want) / want
        note(f"grad_clip norm rel err {str(dtype)[6:]}", rel)
        # non-negative summands: (longest addition chain + sqrt + multiply) x 2^-24, the
        # chain being 5 + 6 + 4 + 4 + 8 adds at these sizes — well under 100 x 6e-8
        assert rel <= 1e-5, (tag, norm, want)
        sc_ref = clip_scale_ref(norm, max_norm, ps)  # at the kernel's own norm_out
        assert abs(sc - sc_ref) <= 4 * float(np.spacing(np.float32(sc_ref))), (tag, sc, sc_ref)
        if exact:
            assert sc == f32(ps), tag
        else:
            assert abs(sc / f32(ps) - 0.5) < 1e-4, tag
        # the work buffer's previous contents (NaN) do not matter and all of it is written
        assert torch.isfinite(work).all(), tag
        assert abs(math.sqrt(float(work.double().sum())) - raw) <= 1e-5 * raw, tag


@gpu
@pytest.mark.parametrize("n", [1027, 6, 1])
def test_grad_clip_rejects_unaligned_bf16_before_launch(dev, n):
    g = _clip_inputs(torch.bfloat16, 1028)
    rc, sc, norm, work = _run_clip(g, n, 1.0, 1.0)
    assert rc != 0
    assert math.isnan(sc) and math.isnan(norm) and all_nan_bits(work)


# ------------------------------------------------------------------------------------------
# 4. FlatAdamW end to end, plain path, built as the RLlib learner builds it

def _check_flat_step(flat, opt, ref, pad, zero_grad, g_before):
    assert abs(float(opt.last_norm) - ref.norm) <= 1e-5 * ref.norm
    assert _close(flat.p32, ref.p) and _close(opt.m, ref.m) and _close(opt.v, ref.v)
    assert torch.equal(bits(flat.p16), bits(flat.p32.bfloat16()))
    for (_, p), off in zip(flat.order, flat.offsets):
        assert p.data_ptr() == flat.p16.data_ptr() + 2 * off and p.dtype == torch.bfloat16
    for t in (flat.p32, flat.p16, opt.m, opt.v):
        assert not bits(t)[pad].any()
    if zero_grad:
        assert not bits(flat.g).any()
    else:
        assert torch.equal(bits(flat.g), bits(g_before))


@gpu
@pytest.mark.parametrize("device_hyper", [False, True], ids=["host_lr", "device_hyper"])
@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep_g", "zero_g"])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])
def test_flat_adamw_learner_configuration(dev, grad_dtype, zero_grad, device_hyper):
    from ray_amd.parallel.flat import FlatAdamW, FlatParams

    torch.manual_seed(5)
    flat = FlatParams(_Small().to(dev), dtype=torch.bfloat16, grad_dtype=grad_dtype)
    assert flat.pt16 is None and flat.p16 is not flat.p32
    opt = FlatAdamW(flat, lr=5e-3, betas=(0.9, 0.999), eps=1e-7, weight_decay=0.01,
                    max_grad_norm=1.0, grad_scale=0.25, zero_grad=zero_grad)
    if device_hyper:
        opt.use_device_hyper()
    ref = _Traj(flat, opt)
    pad = _padding_mask(flat)
    gen = torch.Generator().manual_seed(6)
    lrs = (5e-3, 2e-3, 8e-3, 1e-3)
    for t, target in enumerate((3.0, 0.3, 2.0, 0.6), start=1):  # clipped or not, in turn
        if not zero_grad:
            flat.zero_grad()
        _write_grads(flat, gen, target, opt.grad_scale)
        g_before = flat.g.clone()
        if device_hyper:
            # a changing schedule that only reaches the kernel through device memory
            opt.set_device_hyper(lrs[t - 1], t)
            ref.step(lr=lrs[t - 1])
        else:
            ref.step()
        opt.step()
        torch.cuda.synchronize()
        assert (ref.norm > 1.0) == (target > 1.0)
        _check_flat_step(flat, opt, ref, pad, zero_grad, g_before)
    assert float((ref.p - flat.p32.double()).abs().max()) < float((ref.p - ref.p_old).abs().max())


# ------------------------------------------------------------------------------------------
# 5. ra_adamw_flat_wt through FlatParams(transpose=...)

WT_SHAPES = [(37, 8), (130, 68), (64, 64), (72, 4), (200, 132), (128, 256)]


class _WtModule(torch.nn.Module):
    def __init__(self, big):
        super().__init__()
        mk = lambda *s: torch.nn.Parameter(torch.randn(*s))  # noqa: E731
        for i, s in enumerate(WT_SHAPES):
            setattr(self, f"l{i}_w", mk(*s))
        self.plain2d = mk(10, 7)  # decayed, not transposed: the 1-D pass starts inside decay
        self.bias_a, self.bias_b = mk(37), mk(130)
        self.big = mk(big)


@gpu
@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep_g", "zero_g"])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])
def test_adamw_wt_matches_reference_and_stays_inside_its_tiles(dev, grad_dtype, zero_grad):
    from ray_amd.parallel.flat import FlatAdamW, FlatParams

    torch.manual_seed(11)
    mod = _WtModule(BIG1D + 4 * 100).to(dev)
    flat = FlatParams(mod, dtype=torch.bfloat16, grad_dtype=grad_dtype,
                      transpose=lambda n, p: n.endswith("_w"))
    assert flat.pt16 is not None
    wt = [(n, p) for n, p in flat.order if n.endswith("_w")]
    assert [tuple(p.shape) for _, p in wt] == WT_SHAPES[::-1]
    assert flat.names[len(wt)] == "plain2d" and flat.n_wt < flat.n_decay < flat.numel
    assert flat.wt_tiles == sum(-(-r // 64) * -(-c // 64) for r, c in WT_SHAPES)
    opt = FlatAdamW(flat, lr=5e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1,
                    max_grad_norm=1.0, grad_scale=0.25, zero_grad=zero_grad)
    pad = _padding_mask(flat)
    wt_pad = pad.clone()
    wt_pad[flat.n_wt:] = False  # the padding between tiled weights: no pass covers it
    assert int(wt_pad.sum()) == sum(-k % 64 for k in (r * c for r, c in WT_SHAPES))
    # sentinels wherever a store that runs past R or C would land
    nan = float("nan")
    flat.pt16[wt_pad[:flat.n_wt]] = nan
    for t in (flat.p32, flat.p16, opt.m, opt.v):
        t[wt_pad] = nan
    before = [bits(t)[wt_pad].clone() for t in (flat.p32, flat.p16, opt.m, opt.v)]
    ref = _Traj(flat, opt)
    ref.p[wt_pad] = 0.0
    real = ~pad
    gen = torch.Generator().manual_seed(12)
    for t, target in ((1, 3.0), (2, 0.4)):
        if not zero_grad:
            flat.zero_grad()
        _write_grads(flat, gen, target, opt.grad_scale)
        g_before = flat.g.clone()
        g64 = flat.g.double()
        opt.step()
        torch.cuda.synchronize()
        # the clip in front of the kernel, then the kernel against its own gradient scale
        sc = float(opt._scale)
        norm = clip_norm_ref(g64, opt.grad_scale)
        sc_ref = clip_scale_ref(norm, 1.0, opt.grad_scale)
        assert abs(float(opt.last_norm) - norm) <= 1e-5 * norm
        assert abs(sc - sc_ref) <= 2e-5 * sc_ref and (sc_ref < 0.25) == (t == 1)
        if t == 1:
            # one step from known state: the per-element bounds of the plain kernel's test
            ref.step(sc=sc, g=g64)
            up, um, uv = adam_units(flat.p32[real], opt.m[real], opt.v[real],
                                    tuple(x[real] for x in ref.ref), ref.p_old[real],
                                    ref.m_old[real], lr=opt.lr, b1=opt.b1)
            note(f"adamw_flat_wt units p/m/v g={str(grad_dtype)[6:]}", up, um, uv)
            assert up <= K and um <= K and uv <= K, (up, um, uv)
        else:
            ref.step(g=g64)
        for got, want in ((flat.p32, ref.p), (opt.m, ref.m), (opt.v, ref.v)):
            assert _close(got[real], want[real])
        # both sides of where the tiles hand over to the 1-D pass, and of the decay boundary
        for edge in (flat.n_wt, flat.n_decay):
            s = slice(edge - 64, edge + 64)
            keep = real[s]
            assert _close(flat.p32[s][keep], ref.p[s][keep])
        # mirrors: p16 of the kernel's own p32, W^T of the kernel's own p16
        assert torch.equal(bits(flat.p16[real]), bits(flat.p32[real].bfloat16()))
        for name, p in wt:
            assert p._ra_wt_view.shape == p.shape[::-1]
            assert torch.equal(bits(p._ra_wt_view.contiguous()),
                               bits(p.detach().t().contiguous())), name
        # nothing landed outside the weights' own elements
        assert all_nan_bits(flat.pt16[wt_pad[:flat.n_wt]])
        for tns, old in zip((flat.p32, flat.p16, opt.m, opt.v), before):
            assert torch.equal(bits(tns)[wt_pad], old)
        tail_pad = pad & ~wt_pad
        for tns in (flat.p32, flat.p16, opt.m, opt.v):
            assert not bits(tns)[tail_pad].any()
        if zero_grad:
            assert not bits(flat.g).any()
        else:
            assert torch.equal(bits(flat.g), bits(g_before))


@gpu
def test_adamw_wt_falls_back_beyond_the_segment_table(dev):
    from ray_amd.parallel.flat import FlatAdamW, FlatParams

    torch.manual_seed(13)
    mod = torch.nn.Module()
    mod.ws = torch.nn.ParameterList(
        [torch.nn.Parameter(torch.randn(4, 4)) for _ in range(_lib.lib().ra_wt_max_segments() + 1)])
    mod.to(dev)
    flat = FlatParams(mod, dtype=torch.bfloat16, transpose=lambda n, p: True)
    assert flat.pt16 is None and flat.wt_table is None
    assert not any(hasattr(p, "_ra_wt_view") for p in flat.params())
    opt = FlatAdamW(flat, lr=5e-3, weight_decay=0.1, max_grad_norm=1.0, grad_scale=0.25)
    ref = _Traj(flat, opt)
    pad = _padding_mask(flat)
    _write_grads(flat, torch.Generator().manual_seed(14), 3.0, opt.grad_scale)
    g_before = flat.g.clone()
    opt.step()
    torch.cuda.synchronize()
    ref.step(sc=float(opt._scale), g=g_before.double())
    up, um, uv = adam_units(flat.p32, opt.m, opt.v, ref.ref, ref.p_old, ref.m_old,
                            lr=opt.lr, b1=opt.b1)
    assert up <= K and um <= K and uv <= K, (up, um, uv)
    _check_flat_step(flat, opt, ref, pad, False, g_before)


# ------------------------------------------------------------------------------------------
# 6. the exports nothing else calls: ra_sgd_flat, ra_adamw_f32, ra_adamw_flat

@gpu
@pytest.mark.parametrize("n", [1028, BIG1D + 4 * 777])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("mom", [0.0, 0.9])
def test_sgd_flat_elements(dev, mom, wd, n):
    L = _lib.lib()
    p0, g0, buf0, _, _ = _elem_inputs(n)
    gk = g0.bfloat16()
    lr = 1e-2
    gscale = torch.tensor([GSCALE], device=dev)
    p64, g64, b64 = p0.double(), gk.double(), buf0.double()
    for use_scale in (True, False):
        sc = f32(GSCALE) if use_scale else 1.0
        p_ref, b_ref = sgd_ref(p64, g64, b64, sc=sc, lr=lr, mom=mom, wd=wd)
        # every term the kernel adds, by magnitude: cancellation cannot shrink the bound
        terms = (g64 * sc).abs() + (f32(wd) * p64).abs() + (f32(mom) * b64).abs()
        for with_p16 in (True, False):
            tag = f"mom={mom} wd={wd} n={n} gscale={use_scale} p16={with_p16}"
            (pb, p), (gb, g), (bb, buf) = carved(p0), carved(gk), carved(buf0)
            hb, p16 = carved(n, torch.bfloat16)
            rc = L.ra_sgd_flat(ptr(p), ptr(p16) if with_p16 else None, ptr(g), ptr(buf), n, lr,
                               mom, wd, ptr(gscale) if use_scale else None, stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, tag
            ub = units(buf, b_ref, terms)
            up = units(p, p_ref, p64.abs() + f32(lr) * terms)
            note("sgd_flat units p/buf", up, ub)
            assert up <= K and ub <= K, (tag, up, ub)
            if with_p16:
                assert torch.equal(bits(p16), bits(p.bfloat16())), tag
            else:
                assert all_nan_bits(hb), tag
            assert torch.equal(bits(g), bits(gk)), tag
            for x in (pb, gb, bb, hb):
                assert guards_intact(x), tag
    # n % 4 != 0 is refused on the host, before any launch
    (_, p), (_, g), (_, buf) = carved(p0), carved(gk), carved(buf0)
    assert L.ra_sgd_flat(ptr(p), None, ptr(g), ptr(buf), n - 2, lr, mom, wd, None,
                         stream_ptr()) != 0
    torch.cuda.synchronize()
    for got, src in ((p, p0), (g, gk), (buf, buf0)):
        assert torch.equal(bits(got), bits(src))


@gpu
@pytest.mark.parametrize("n,nd", [(1028, 512), (1027, 515), (2048 * 256 + 777, 2048 * 256 + 1),
                                  (2048 * 256 + 777, 0), (1028, 1028)])
@pytest.mark.parametrize("step", sorted(STEPS))
def test_adamw_f32_elements(dev, step, n, nd):
    t, betas, eps, wd = STEPS[step]
    p0, g0, m0, v0, _ = _elem_inputs(n)
    if t == 1:
        m0, v0 = torch.zeros_like(m0), torch.zeros_like(v0)
    gscale = torch.tensor([GSCALE], device=dev)
    p64, g64, m64, v64 = (x.double() for x in (p0, g0, m0, v0))
    for use_scale in (True, False):
        sc = f32(GSCALE) if use_scale else 1.0
        tag = f"step={t} n={n} nd={nd} gscale={use_scale}"
        ref = adam_ref(p64, g64, m64, v64, sc=sc, lr=LR, b1=betas[0], b2=betas[1], eps=eps,
                       wd=wd, n_decay=nd, rbc1=rbc(betas[0], t), rbc2=rbc(betas[1], t))
        (pb, p), (gb, g), (mb, m), (vb, v) = (carved(x) for x in (p0, g0, m0, v0))
        rc = _lib.lib().ra_adamw_f32(ptr(p), ptr(g), ptr(m), ptr(v), n, nd, LR, betas[0],
                                     betas[1], eps, wd, t, ptr(gscale) if use_scale else None,
                                     stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, tag
        up, um, uv = adam_units(p, m, v, ref, p64, m64, lr=LR, b1=betas[0])
        note(f"adamw_f32 units p/m/v step={t}", up, um, uv)
        assert up <= K and um <= K and uv <= K, (tag, up, um, uv)
        if wd and 0 < nd < n:
            # the element on each side of an n_decay that is no multiple of 4
            s = slice(nd - 1, nd + 1)
            bound = K * U * (p64[s].abs() + f32(LR) * ref[3][s].abs())
            assert ((p[s].double() - ref[0][s]).abs() <= bound).all(), tag
        assert torch.equal(bits(g), bits(g0)), tag
        for x in (pb, gb, mb, vb):
            assert guards_intact(x), tag


@gpu
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_adamw_flat_is_adamw_flat_dev_without_hyper(dev, flags):
    n = BIG1D + 4 * 777
    p0, g0, m0, v0, _ = _elem_inputs(n)
    gk = g0 if flags & 1 else g0.bfloat16()
    gscale = torch.tensor([GSCALE], device=dev)
    kw = dict(n_decay=n // 2 // 4 * 4, lr=LR, betas=(0.9, 0.95), eps=1e-8, wd=0.1, step=37,
              gscale=gscale, flags=flags)
    a = _run_adamw("ra_adamw_flat", p0, gk, m0, v0, **kw)
    b = _run_adamw("ra_adamw_flat_dev", p0, gk, m0, v0, hyper=None, **kw)
    assert a["rc"] == 0 and b["rc"] == 0
    for k in ("p", "g", "m", "v", "p16"):
        assert torch.equal(bits(a[k][0]), bits(b[k][0])), k
    assert not torch.equal(bits(a["p"][1]), bits(p0))
