#!/usr/bin/env python
"""Beam search: the kernels (ops/csrc/beam.hip through ``rf.beam_step`` and
``rf.beam_kv_fork``) against the usual torch composition, how many beams fork per step, and
what ``GPT2.generate(num_beams=...)`` delivers end to end.

    python scripts/beam_bench.py [--out profiles/r20/beam.md]

Kernel part, (G, W) = (1, 4), (8, 4), (8, 8). ``beam_step`` on V = 50257 bf16 logits (randn x 4)
as the [:, :V] view of a [G * W, 50304] buffer: ``hip`` is one call (two launches), ``torch``
is ``log_softmax`` in fp32, ``topk(2W)`` per row, the add of the scores, ``topk(2W)`` over the
group and the gathers of token, parent and score for the first W (no EOS handling, no
hypothesis table, no slot placement: it does less than the kernels). ``beam_kv_fork`` on a
GPT-2 small cache (12 layers, 12 heads of 64) of G * W rows with ``len`` cached positions and
0, 1 or W - 1 forking beams per group: ``hip`` is one call, ``torch`` is ``index_select`` of K
and of V by ``parent`` into a second cache (what a cache re-ordered every step costs whatever
forks). ``beam_backtrace`` reads out W hypotheses per group from a history of 1023 steps with
random back pointers (no torch counterpart: its column repeats the kernel's). 20 calls of one
path captured in one HIP graph and replayed, device events around blocks of replays, a warm-up
and at least ``--seconds`` of timed work per path and repeat, the paths alternated, median
(min..max) of ``--repeats``, microseconds per call. (The EOS column is -inf and the state has
room for 2^20 steps, so that no timed call meets a finished group.)

End to end: GPT-2 small, bf16, random-init weights, G = 8 prompts of 128 tokens, 128 new tokens,
``graph=True``: ``num_beams`` 4 and 8 against the sampled ``seeds=`` path at batch G * W, wall
time around synchronised calls, the paths alternated, median (min..max) of ``--repeats`` after
one warm-up; tokens/s counts G * W * 128 decoded rows on both. ``forks``: the share of (step,
beam) pairs whose beam moved to another cache row, from the search's own ``par_hist``."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "r20", "beam.md"))
ap.add_argument("--seconds", type=float, default=0.2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-kernel", dest="kernel", action="store_false")
ap.add_argument("--no-generate", dest="generate", action="store_false")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402

V, VPAD, EOS = 50257, 50304, 50256
SHAPES = ((1, 4), (8, 4), (8, 8))
GRAPH_CALLS = 20


def block_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def stats(t):
    t = sorted(t)
    return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}


def time_graphed(paths, seconds, repeats):
    reps = {}
    for name, fn in paths.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(GRAPH_CALLS):
                fn()
        reps[name] = g.replay
    iters = {}
    for name, fn in reps.items():
        block_us(fn, 5)
        iters[name] = max(5, int(seconds * 1e6 / block_us(fn, 10)) + 1)
    times = {n: [] for n in reps}
    for _ in range(repeats):
        for name, fn in reps.items():
            times[name].append(block_us(fn, iters[name]) / GRAPH_CALLS)
    return {n: stats(t) for n, t in times.items()}


def kernel_part(a, dev):
    rows = []
    for G, W in SHAPES:
        N, K = G * W, 2 * W
        g = torch.Generator().manual_seed(N)
        buf = torch.zeros(N, VPAD, dtype=torch.bfloat16)
        buf[:, :V] = (torch.randn(N, V, generator=g) * 4).bfloat16()
        buf[:, EOS] = float("-inf")
        logits = buf.to(dev)[:, :V]
        st = rf.beam_state(G, W, 1 << 20, EOS, 1.0, True, dev)
        st["score"].copy_(torch.randn(N, generator=g).to(dev))

        def torch_step():
            lp, tok = torch.log_softmax(logits.float(), -1).topk(K, -1)
            cand = (st["score"].view(N, 1) + lp).view(G, W * K)
            val, at = cand.topk(K, -1)
            return tok.view(G, W * K).gather(1, at)[:, :W], (at // K)[:, :W], val[:, :W]

        rec = {"op": "beam_step", "G": G, "W": W,
               "device_us": time_graphed({"hip": lambda: rf.beam_step(logits, st),
                                          "torch": torch_step}, a.seconds, a.repeats)}
        rec["speedup"] = rec["device_us"]["torch"]["median"] / rec["device_us"]["hip"]["median"]
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        bt = rf.beam_state(G, W, 1023, EOS, 1.0, True, dev)  # a full history, random pointers
        bt["step"].fill_(1023)
        bt["par_hist"].copy_((torch.randint(0, W, (1023, N), generator=g) +
                              torch.arange(N) // W * W).to(dev))
        rec = {"op": "beam_backtrace, 1023 steps", "G": G, "W": W,
               "device_us": time_graphed({"hip": lambda: rf.beam_backtrace(bt, W)}, a.seconds,
                                         a.repeats)}
        rec["device_us"]["torch"], rec["speedup"] = rec["device_us"]["hip"], 1.0
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        for length in (128, 1000):
            shape = (12, N, 12, length + 24, 64)
            k = torch.randn(shape, device=dev, dtype=torch.bfloat16)
            v, k2, v2 = torch.randn_like(k), torch.empty_like(k), torch.empty_like(k)
            lens = torch.full((N,), length, dtype=torch.int32, device=dev)
            for forks in sorted({0, 1, W - 1}):
                parent = torch.arange(N, dtype=torch.int32).view(G, W).clone()
                parent[:, W - forks:] = parent[:, :1]  # the last `forks` beams continue beam 0
                parent = parent.view(N).to(dev)
                index = parent.long()

                def gather():
                    torch.index_select(k, 1, index, out=k2)
                    torch.index_select(v, 1, index, out=v2)

                rec = {"op": "beam_kv_fork", "G": G, "W": W, "len": length, "forks": forks,
                       "device_us": time_graphed(
                           {"hip": lambda: rf.beam_kv_fork(k, v, parent, lens), "torch": gather},
                           a.seconds, a.repeats)}
                rec["speedup"] = rec["device_us"]["torch"]["median"] / \
                    rec["device_us"]["hip"]["median"]
                print(json.dumps(rec), flush=True)
                rows.append(rec)
            del k, v, k2, v2
            torch.cuda.empty_cache()
    return rows


def generate_part(a, dev):
    torch.manual_seed(0)
    model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    G, T, NEW = 8, 128, 128
    idx = torch.randint(0, V, (G, T), generator=torch.Generator().manual_seed(1)).to(dev)
    kept = {}
    backtrace = rf.beam_backtrace

    def keep_state(state, R):  # the search's own history, for the fork count
        kept["par_hist"] = state["par_hist"].clone()
        return backtrace(state, R)

    rows = []
    for W in (4, 8):
        wide = idx.repeat_interleave(W, 0)
        paths = {"beams": lambda: model.generate(idx, NEW, eos_token_id=EOS, num_beams=W,
                                                 graph=True),
                 "sampled": lambda: model.generate(wide, NEW, temperature=0.8, top_k=50,
                                                   seeds=list(range(G * W)), graph=True)}
        rf.beam_backtrace = keep_state
        paths["beams"]()
        rf.beam_backtrace = backtrace
        moved = kept["par_hist"][1:] != torch.arange(G * W, device=dev)
        runs = {n: [] for n in paths}
        paths["sampled"]()
        for _ in range(a.repeats):
            for n, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                runs[n].append(G * W * NEW / (time.perf_counter() - t0))
        rec = {"W": W, "G": G, "forks_per_step_and_beam": float(moved.float().mean()),
               "tok_per_s": {n: stats(r) for n, r in runs.items()}}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def cell(s, fmt=".1f"):
    return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("beam_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    krows = kernel_part(a, dev) if a.kernel else []
    grows = generate_part(a, dev) if a.generate else []
    lines = ["# Beam search: beam_step, beam_kv_fork, generate(num_beams=...)", "",
             f"`scripts/beam_bench.py` on {torch.cuda.get_device_name(0)}; method in its docstring.",
             ""]
    if krows:
        lines += ["## One call", "", "| op | G | W | len | forks | hip device us | torch device us | "
                  "torch / hip |", "|---|---|---|---|---|---|---|---|"]
        for r in krows:
            dv = r["device_us"]
            lines.append(f"| {r['op']} | {r['G']} | {r['W']} | {r.get('len', '')} | "
                         f"{r.get('forks', '')} | {cell(dv['hip'], '.2f')} | {cell(dv['torch'])} | "
                         f"{r['speedup']:.1f}x |")
    if grows:
        lines += ["", "## generate, GPT-2 small bf16 (random init), 8 prompts x 128, 128 new, "
                  "graph=True", "", "| num_beams | beams rows/s | sampled rows/s at batch G * W | "
                  "forks per (step, beam) |", "|---|---|---|---|"]
        for r in grows:
            lines.append(f"| {r['W']} | {cell(r['tok_per_s']['beams'], '.0f')} | "
                         f"{cell(r['tok_per_s']['sampled'], '.0f')} | "
                         f"{r['forks_per_step_and_beam']:.3f} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
