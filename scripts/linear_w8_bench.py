#!/usr/bin/env python
"""Weight-only int8 linears (ops/csrc/linear_w8.hip through ``rf.linear_w8``).

    python scripts/linear_w8_bench.py [--part kernel|decode|trace] [--out FILE.jsonl]

kernel: ``rf.linear_w8`` through its skinny kernel and through its dequantise + library GEMM
path, and ``F.linear`` on the bf16 weight, at the GPT-2 small and XL layer shapes and LM heads
for M in 1..512. Each path is captured 20 times in one HIP graph; device events around
alternating replays, a warm-up, median of ``--repeats`` blocks, microseconds per call. This
is what ``W8_SKINNY_MAX_M`` is set from. Also the skinny kernel with one split against its
automatic split count at M = 8.

decode: ``GPT2.generate(graph=True)`` with bf16 and with int8 weights on one model, the two
alternated; the step time is the wall-time difference of a long and a short call over the
difference of their token counts, which takes the prompt pass and the capture out.

trace: M = 8 skinny calls only, for a kernel trace (weight bytes over kernel time).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402

SHAPES = [("small c_attn", 2304, 768), ("small c_proj", 768, 768), ("small c_fc", 3072, 768),
          ("small mlp_proj", 768, 3072), ("small lm_head", 50304, 768),
          ("xl c_attn", 4800, 1600), ("xl c_proj", 1600, 1600), ("xl c_fc", 6400, 1600),
          ("xl mlp_proj", 1600, 6400), ("xl lm_head", 50304, 1600)]
MS = (1, 8, 32, 64, 128, 256, 512)
GRAPH_CALLS = 20


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            fn()
    return g.replay


def block_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters / GRAPH_CALLS


def time_paths(paths, seconds, repeats):
    reps = {n: graphed(fn) for n, fn in paths.items()}
    iters = {n: max(3, int(seconds * 1e6 / (block_us(r, 3) * GRAPH_CALLS)) + 1)
             for n, r in reps.items()}
    times = {n: [] for n in reps}
    for _ in range(repeats):
        for n, r in reps.items():  # alternate the paths
            times[n].append(block_us(r, iters[n]))
    return {n: sorted(t)[len(t) // 2] for n, t in times.items()}


def with_max_m(v, fn):
    def call():
        old, rf.W8_SKINNY_MAX_M = rf.W8_SKINNY_MAX_M, v
        try:
            return fn()
        finally:
            rf.W8_SKINNY_MAX_M = old
    return call


def kernel_part(a, emit):
    dev = torch.device("cuda")
    L = _lib.lib()
    for name, N, K in SHAPES:
        g = torch.Generator().manual_seed(N + K)
        w = (torch.randn(N, K, generator=g) * 0.02).to(dev, torch.bfloat16)
        q, s = rf.quantize_w8(w)
        wd = rf.dequant_w8(q, s)
        auto = L.ra_linear_w8_splits(N, K)
        for M in MS:
            x = torch.randn(M, K, generator=g).to(dev, torch.bfloat16)
            paths = {"skinny": with_max_m(1 << 30, lambda: rf.linear_w8(x, q, s)),
                     "dequant": with_max_m(0, lambda: rf.linear_w8(x, q, s)),
                     "bf16": lambda: F.linear(x, w)}
            if M == 8 and auto > 1:
                paths["skinny_s1"] = with_max_m(1 << 30, lambda: rf.linear_w8(x, q, s, splits=1))
            # same results first: against the library GEMM on the dequantised weight
            diff = float((paths["skinny"]().float() - F.linear(x, wd).float()).abs().max())
            emit({"part": "kernel", "shape": name, "N": N, "K": K, "M": M, "splits": auto,
                  "max_abs_diff_vs_dequant_gemm": diff,
                  "us": time_paths(paths, a.seconds, a.repeats)})


def trace_part(a, emit):
    dev = torch.device("cuda")
    for name, N, K in SHAPES:
        g = torch.Generator().manual_seed(N + K)
        q, s = rf.quantize_w8((torch.randn(N, K, generator=g) * 0.02).to(dev, torch.bfloat16))
        x = torch.randn(8, K, generator=g).to(dev, torch.bfloat16)
        for _ in range(50):
            rf.linear_w8(x, q, s)
        torch.cuda.synchronize()
        emit({"part": "trace", "shape": name, "weight_bytes": N * K, "calls": 50})


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def decode_part(a, emit):
    dev = torch.device("cuda")
    for cname in a.configs:
        torch.manual_seed(0)
        model = GPT2(getattr(GPT2Config, cname)()).to(dev, torch.bfloat16).eval()
        for B in a.slots:
            idx = torch.randint(0, model.cfg.vocab_size, (B, 32),
                                generator=torch.Generator().manual_seed(B)).to(dev)
            times = {(w, n): [] for w in ("bf16", "int8") for n in (a.short, a.long)}
            for rep in range(a.repeats + 1):  # the first round warms up
                for w in ("bf16", "int8"):
                    model.quantize_weights() if w == "int8" else model.dequantize_weights()
                    for n in (a.short, a.long):
                        t = wall(lambda: model.generate(idx, n, graph=True, seeds=0))
                        if rep:
                            times[(w, n)].append(t)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            step = {w: (med[(w, a.long)] - med[(w, a.short)]) / (a.long - a.short) * 1e3
                    for w in ("bf16", "int8")}
            emit({"part": "decode", "config": cname, "slots": B, "step_ms": step,
                  "int8_vs_bf16": step["bf16"] / step["int8"]})
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "decode", "trace"), default="kernel")
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", nargs="*", default=["small", "xl"])
    ap.add_argument("--slots", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--short", type=int, default=32)
    ap.add_argument("--long", type=int, default=160)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_w8_bench needs a GPU: timings are device timings")
    fh = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    {"kernel": kernel_part, "decode": decode_part, "trace": trace_part}[a.part](a, emit)


if __name__ == "__main__":
    main()
