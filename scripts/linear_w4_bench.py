#!/usr/bin/env python
"""Weight-only MXFP4 linears (ops/csrc/linear_w4.hip through ``rf.linear_w4``) against the
int8 ones and bf16; the timing harness is ``linear_w8_bench.py``'s.

    python scripts/linear_w4_bench.py [--part kernel|decode] [--out FILE.jsonl]

kernel: the skinny kernels of ``rf.linear_w4`` and ``rf.linear_w8`` and ``F.linear`` on the
bf16 weight at the GPT-2 small and XL layer shapes and LM heads, M = 1, 8, 64, microseconds per
call. ``warm``: 20 back-to-back calls in one HIP graph, so a weight that fits the last-level
cache is served from it. ``cold``: every call in the graph follows a fill of a 512 MB buffer
(twice the last-level cache), and the same graph of fills alone is subtracted.

decode: ``GPT2.generate(graph=True)`` with bf16, int8 and MXFP4 weights on one model, the
three alternated; step time as in ``linear_w8_bench.py``.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from linear_w8_bench import SHAPES, time_paths, wall  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402

MS = (1, 8, 64)
FLUSH_BYTES = 512 << 20


def kernel_part(a, emit):
    dev = torch.device("cuda")
    L = _lib.lib()
    flush = torch.empty(FLUSH_BYTES, device=dev, dtype=torch.uint8)
    for name, N, K in SHAPES:
        g = torch.Generator().manual_seed(N + K)
        w = (torch.randn(N, K, generator=g) * 0.02).to(dev, torch.bfloat16)
        q8, s8 = rf.quantize_w8(w)
        q4, s4 = rf.quantize_w4(w)
        w4 = rf.dequant_w4(q4, s4)
        for M in MS:
            x = torch.randn(M, K, generator=g).to(dev, torch.bfloat16)
            calls = {"mxfp4": lambda: rf.linear_w4(x, q4, s4),
                     "int8": lambda: rf.linear_w8(x, q8, s8), "bf16": lambda: F.linear(x, w)}
            # same results first: against the library GEMM on the dequantised weight
            diff = float((calls["mxfp4"]().float() - F.linear(x, w4).float()).abs().max())
            warm = time_paths(calls, a.seconds, a.repeats)
            cold = {"flush": lambda: flush.fill_(1)}
            for n, fn in calls.items():
                cold[n] = lambda fn=fn: (flush.fill_(1), fn())
            cold = time_paths(cold, a.seconds, a.repeats)
            emit({"part": "kernel", "shape": name, "N": N, "K": K, "M": M,
                  "splits": {"mxfp4": L.ra_linear_w4_splits(N, K),
                             "int8": L.ra_linear_w8_splits(N, K)},
                  "max_abs_diff_vs_dequant_gemm": diff, "warm_us": warm, "flush_us": cold["flush"],
                  "cold_us": {n: cold[n] - cold["flush"] for n in calls}})


def decode_part(a, emit):
    dev = torch.device("cuda")
    fmts = ("bf16", "int8", "mxfp4")
    for cname in a.configs:
        torch.manual_seed(0)
        model = GPT2(getattr(GPT2Config, cname)()).to(dev, torch.bfloat16).eval()
        for B in a.slots:
            idx = torch.randint(0, model.cfg.vocab_size, (B, 32),
                                generator=torch.Generator().manual_seed(B)).to(dev)
            times = {(w, n): [] for w in fmts for n in (a.short, a.long)}
            for rep in range(a.repeats + 1):  # the first round warms up
                for w in fmts:
                    model.dequantize_weights() if w == "bf16" else model.quantize_weights(fmt=w)
                    for n in (a.short, a.long):
                        t = wall(lambda: model.generate(idx, n, graph=True, seeds=0))
                        if rep:
                            times[(w, n)].append(t)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            step = {w: (med[(w, a.long)] - med[(w, a.short)]) / (a.long - a.short) * 1e3
                    for w in fmts}
            emit({"part": "decode", "config": cname, "slots": B, "step_ms": step,
                  "mxfp4_vs_int8": step["int8"] / step["mxfp4"],
                  "mxfp4_vs_bf16": step["bf16"] / step["mxfp4"]})
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "decode"), default="kernel")
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", nargs="*", default=["small", "xl"])
    ap.add_argument("--slots", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--short", type=int, default=32)
    ap.add_argument("--long", type=int, default=160)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_w4_bench needs a GPU: timings are device timings")
    fh = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    {"kernel": kernel_part, "decode": decode_part}[a.part](a, emit)


if __name__ == "__main__":
    main()
