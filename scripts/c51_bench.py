#!/usr/bin/env python
"""C51 projection loss, forward + backward, at DQN update sizes: the fused HIP kernel
(ops/csrc/c51.hip through ``rf.c51_loss``) vs the plain-torch reference path
(``ref.c51_loss``, ~25 small launches) on the GPU.

    python scripts/c51_bench.py [--out profiles/r7/c51_bench.md]

Device events around alternating blocks of the two paths in one process; every case gets a
warm-up and at least ``--seconds`` of timed work per path and repeat; the table reports the
median and the spread (min..max) of ``--repeats`` repeats.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402
from ray_amd.ops import reference as ref  # noqa: E402

SHAPES = [(32, 6, 51), (512, 6, 51), (32, 18, 51)]


def make_inputs(B, A, K, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = (2 * torch.randn(B, A, K, generator=g)).to(dev).requires_grad_()
    rest = [torch.randint(0, A, (B,), generator=g), 2 * torch.randn(B, A, K, generator=g),
            2 * torch.randn(B, A, K, generator=g), 4 * torch.randn(B, generator=g),
            torch.full((B,), 0.99), (torch.rand(B, generator=g) < 0.1).float(),
            0.2 + 0.8 * torch.rand(B, generator=g)]
    return [logits] + [t.to(dev) for t in rest]


def step(fn, args):
    args[0].grad = None
    fn(*args, -10.0, 10.0)[0].backward()


def block_us(fn, args, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step(fn, args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r7", "c51_bench.md"))
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("c51_bench needs a GPU: timings are device-event timings")
    _lib.lib()
    dev = torch.device("cuda")
    paths = {"fused": rf.c51_loss, "reference": ref.c51_loss}
    rows = []
    for B, A, K in SHAPES:
        args = make_inputs(B, A, K, dev)
        # same results first: faster and different is not faster
        lf, cf, _ = rf.c51_loss(*args, -10.0, 10.0)
        lr_, cr = ref.c51_loss(*args, -10.0, 10.0)[:2]
        max_ce_diff = float((cf - cr).abs().max())
        iters = {}
        for name, fn in paths.items():  # warm-up + block length for >= --seconds
            block_us(fn, args, 20)
            iters[name] = max(50, int(a.seconds * 1e6 / block_us(fn, args, 100)) + 1)
        times = {n: [] for n in paths}
        for _ in range(a.repeats):
            for name, fn in paths.items():  # alternate the two paths
                times[name].append(block_us(fn, args, iters[name]))
        rec = {"B": B, "A": A, "K": K, "max_ce_diff": max_ce_diff,
               "loss_diff": float((lf - lr_).detach().abs())}
        for n, t in times.items():
            t = sorted(t)
            rec[n] = {"median_us": t[len(t) // 2], "min_us": t[0], "max_us": t[-1],
                      "iters": iters[n]}
        rec["speedup_median"] = rec["reference"]["median_us"] / rec["fused"]["median_us"]
        rec["speedup_worst"] = rec["reference"]["min_us"] / rec["fused"]["max_us"]
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    lines = ["# C51 projection loss: fused HIP kernel vs plain-torch reference (fwd + bwd)", "",
             f"`scripts/c51_bench.py` on {torch.cuda.get_device_name(0)}: device events, the two "
             f"paths alternated in one process, >= {a.seconds:g} s of timed work per path and "
             f"repeat, median (min..max) of {a.repeats} repeats, microseconds per forward + "
             "backward. `worst` = slowest fused repeat against the fastest reference repeat.", "",
             "| B | A | K | fused us | reference us | speed-up (median) | worst | max abs ce diff |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        f, q = r["fused"], r["reference"]
        lines.append(
            f"| {r['B']} | {r['A']} | {r['K']} | {f['median_us']:.1f} ({f['min_us']:.1f}.."
            f"{f['max_us']:.1f}) | {q['median_us']:.1f} ({q['min_us']:.1f}..{q['max_us']:.1f}) | "
            f"{r['speedup_median']:.2f}x | {r['speedup_worst']:.2f}x | {r['max_ce_diff']:.2e} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
