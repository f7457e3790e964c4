"""Embedding backward at the GPT-2 bench shape (B 64, T 1024, C 768, V 50304): the HIP
kernels (ops/csrc/embed.hip, with the torch.sort that feeds them) vs torch's index_add_ +
batch-sum into fp32 sinks, for uniform-random token ids (~1.3 rows per token, the
benchmark's data) and for skewed ones (Zipf-like: the most frequent token fills ~8 % of the
batch, ~5000 rows)."""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_amd.ops._lib import check, lib, ptr, stream_ptr  # noqa: E402


def timed(fn, iters=20):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    B, T, C, V = 64, 1024, 768, 50304
    torch.manual_seed(0)
    dx = torch.randn(B * T, C, device="cuda").bfloat16()
    wte = torch.zeros(V, C, device="cuda")
    wpe = torch.zeros(1024, C, device="cuda")
    L = lib()
    work = torch.empty(L.ra_embed_bwd_work(B, T, C), device="cuda")
    p = 1.0 / torch.arange(1, 50258, device="cuda", dtype=torch.float64)
    ids = {"uniform": torch.randint(0, 50257, (B * T,), device="cuda"),
           "skewed": torch.multinomial(p / p.sum(), B * T, replacement=True)}
    out = {}
    for name, idx in ids.items():
        def hip():
            sid, perm = torch.sort(idx, stable=True)
            check(L.ra_embed_bwd(ptr(dx), ptr(sid), ptr(perm), ptr(work), ptr(wte), ptr(wpe),
                                 B, T, C, V, stream_ptr()), "embed_bwd")

        def ref():
            wte.index_add_(0, idx, dx.to(torch.float32))
            wpe[:T].add_(dx.view(B, T, C).float().sum(0))

        # same batch twice: the same bits, and the torch reference's values
        wte.zero_()
        hip()
        a = wte.clone()
        wte.zero_()
        hip()
        same = torch.equal(a, wte)
        wte.zero_()
        ref()
        err = float((a - wte).abs().max() / wte.abs().max())
        out[name] = {"max_rows_per_token": int(torch.bincount(idx).max()),
                     "hip_ms": round(timed(hip), 4), "torch_ms": round(timed(ref), 4),
                     "repeat_bitwise": same, "rel_err_vs_torch": err}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
