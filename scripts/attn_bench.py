"""Time the HIP flash attention against torch SDPA (aotriton on ROCm) at GPT-2 shape.

python scripts/attn_bench.py [--B 16 --T 1024 --H 12]
python scripts/attn_bench.py --sweep [--shape 0]   forward and backward timed separately over a
    constant-token sweep (B*T fixed, T doubling): the block count stays, the tiles per block
    double, so a linear fit splits each time into a per-tile and a per-block part. With
    --shape I only that shape runs (one process per shape under a kernel trace gives the same
    split per kernel).
"""

import argparse
import json

import torch
import torch.nn.functional as F

from ray_amd.ops import functional as rf


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


SWEEP = ((64, 1024), (32, 2048), (16, 4096))  # (B, T): B*T = 65536 tokens


def block_cost_fit(shapes, ms):
    """Least-squares t = a * tiles + b over the sweep. With 128-row blocks and 64-row tiles a
    block sweeps T/128 + 1 tiles on average; the block count B*H*T/128 is the same for every
    shape. Returns (per-tile ms at the first shape, per-block ms, per-block share there)."""
    xs = [T / 128 + 1 for _, T in shapes]
    n = len(xs)
    mx, my = sum(xs) / n, sum(ms) / n
    a = sum((x - mx) * (y - my) for x, y in zip(xs, ms)) / sum((x - mx) ** 2 for x in xs)
    b = my - a * mx
    return a * xs[0], b, b / ms[0]


def sweep(a):
    from ray_amd.ops import _lib
    from ray_amd.ops._lib import ptr, stream_ptr

    H, D = a.H, 64
    shapes = SWEEP if a.shape is None else (SWEEP[a.shape],)
    res = {"H": H, "shapes": [], "fwd_ms": [], "bwd_ms": []}
    L = _lib.lib()
    for B, T in shapes:
        torch.manual_seed(0)
        qkv = torch.randn(B, T, 3, H, D, device="cuda", dtype=torch.bfloat16)
        dout = torch.randn(B, T, H, D, device="cuda", dtype=torch.bfloat16)
        out = torch.empty_like(dout)
        lse = torch.empty(B, H, T, device="cuda", dtype=torch.float32)
        delta = torch.empty_like(lse)
        dqkv = torch.empty_like(qkv)
        st = stream_ptr()

        def fwd():
            _lib.check(L.ra_attn_fwd(ptr(qkv), ptr(out), ptr(lse), B, T, H, D, D ** -0.5, st))

        def bwd():
            _lib.check(L.ra_attn_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(delta),
                                     ptr(dqkv), B, T, H, D, D ** -0.5, st))

        res["shapes"].append([B, T])
        res["fwd_ms"].append(round(timeit(fwd, a.iters), 4))
        res["bwd_ms"].append(round(timeit(bwd, a.iters), 4))
    if len(shapes) > 1:
        for k in ("fwd", "bwd"):
            tile, blk, share = block_cost_fit(shapes, res[k + "_ms"])
            res[k + "_fit"] = {"per_tile_ms": round(tile, 4), "per_block_ms": round(blk, 4),
                               "per_block_share": round(share, 3)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--shape", type=int, default=None, choices=range(len(SWEEP)))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.sweep:
        return sweep(a)
    B, T, H, D = a.B, a.T, a.H, 64
    dev = "cuda"
    qkv = torch.randn(B, T, 3, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    g = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16)
    flops_fwd = 4 * B * H * T * T * D / 2  # causal
    res = {}

    def ours_fwd():
        with torch.no_grad():
            rf.causal_attention_qkv(qkv)

    def ours_fb():
        y = rf.causal_attention_qkv(qkv)
        y.backward(g)

    def sdpa(x):
        q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)
        return F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2)

    def sdpa_fwd():
        with torch.no_grad():
            sdpa(qkv)

    def sdpa_fb():
        sdpa(qkv).backward(g)

    for name, fn in (("ours_fwd", ours_fwd), ("ours_fwd_bwd", ours_fb), ("sdpa_fwd", sdpa_fwd),
                     ("sdpa_fwd_bwd", sdpa_fb)):
        ms = timeit(fn)
        mult = 1 if name.endswith("fwd") else 3.5  # bwd = 2.5x fwd flops
        res[name] = {"ms": round(ms, 4), "tflops": round(mult * flops_fwd / ms / 1e9, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
