#!/usr/bin/env python
"""Per-row low-rank adapters: ``rf.lora_add`` (ops/csrc/lora.hip) against the torch
composition, and what an attached adapter stack costs the GPT-2 engine.

    python scripts/lora_bench.py [--out profiles/r13/lora.md]

Kernel part. GPT-2 small's four adapted linears (Din -> Dout: c_attn 768 -> 2304, c_proj
768 -> 768, c_fc 768 -> 3072, mlp_proj 3072 -> 768), R 16 and 64, three adapters mixed with
base rows (``idx`` cycles 0, 1, -1, 2), at (Bn, T) = (8, 1), (64, 1), (8, 128), (8, 1024).
``hip`` is ``rf.lora_add``, ``bmm`` the sync-free composition ``ref.lora_add_bmm``
(``index_select`` of the stacks by the clamped ids, two ``bmm``, the rows without an adapter
masked out). Both are captured in one HIP graph (20 calls per replay) and timed with device
events around alternating blocks in one process, a warm-up and at least ``--seconds`` of timed
work per path and repeat, median (min..max) of ``--repeats``.

Engine part: GPT-2 small, bf16, S = 64, ``poll_every`` 8, the request mix of
profiles/r10/engine.md (``--requests`` seeded requests, prompts 16..128, ``max_new_tokens``
uniform in 16..256, temperature 0.8, top-k 50), all queued at t0: (a) no stack attached, (b)
a rank-16 stack of four adapters attached and every request on the base model, (c) the
requests spread over the four adapters. Wall time around synchronised calls, the paths
alternated, median (min..max) of ``--repeats`` after a warm-up run. ``--package-root DIR
--base-only`` runs (a) alone on another checkout of the package (the parent commit), for the
check that the engine without a stack has not moved."""
import argparse
import json
import os
import sys
import time


def _root():
    for i, v in enumerate(sys.argv):
        if v == "--package-root":
            return os.path.abspath(sys.argv[i + 1])
        if v.startswith("--package-root="):
            return os.path.abspath(v.split("=", 1)[1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


sys.path.insert(0, _root())

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402
from ray_amd.ops import reference as ref  # noqa: E402

C = 768
LINEARS = [("c_attn", C, 3 * C), ("c_proj", C, C), ("c_fc", C, 4 * C), ("mlp_proj", 4 * C, C)]
SHAPES = [(8, 1), (64, 1), (8, 128), (8, 1024)]
RANKS = [16, 64]
NA = 3
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


def time_graphed(paths, seconds, repeats):
    """Device microseconds per call of each path, captured, the paths alternated."""
    replays = {n: graphed(fn) for n, fn in paths.items()}
    iters = {}
    for name, fn in replays.items():  # warm-up + block length for >= seconds
        block_us(fn, 5)
        iters[name] = max(5, int(seconds * 1e6 / block_us(fn, 10)) + 1)
    times = {n: [] for n in paths}
    for _ in range(repeats):
        for name, fn in replays.items():
            times[name].append(block_us(fn, iters[name]) / GRAPH_CALLS)
    return {n: stats(t) for n, t in times.items()}


def kernel_part(a, dev):
    rows = []
    g = torch.Generator().manual_seed(0)
    for R in RANKS:
        for name, din, dout in LINEARS:
            As = (torch.randn(NA, R, din, generator=g) * 0.05).bfloat16().to(dev)
            Bs = (torch.randn(NA, dout, R, generator=g) * 0.05).bfloat16().to(dev)
            # small scales: the timed calls add to y in place thousands of times
            scale = torch.tensor([1e-3, -1e-3, 5e-4], device=dev)
            for Bn, T in SHAPES:
                x = torch.randn(Bn, T, din, generator=g).bfloat16().to(dev)
                y0 = torch.randn(Bn, T, dout, generator=g).bfloat16().to(dev)
                idx = torch.tensor([(0, 1, -1, 2)[b % 4] for b in range(Bn)], dtype=torch.int32,
                                   device=dev)
                # same results first: faster and different is not faster
                big = torch.tensor([0.5, 2.0, 8.0], device=dev)
                outs = []
                for fn in (rf.lora_add, ref.lora_add_bmm):
                    y = y0.clone()
                    fn(y, x, As, Bs, big, idx)
                    outs.append(y.float())
                rel = ((outs[0] - outs[1]).norm() / outs[1].norm()).item()
                y = y0.clone()
                paths = {"hip": lambda: rf.lora_add(y, x, As, Bs, scale, idx),
                         "bmm": lambda: ref.lora_add_bmm(y, x, As, Bs, scale, idx)}
                rec = {"linear": name, "R": R, "Bn": Bn, "T": T, "rel_diff": rel,
                       "device_us": time_graphed(paths, a.seconds, a.repeats)}
                print(json.dumps(rec), flush=True)
                rows.append(rec)
    return rows


# ------------------------------------------------------------------ the engine
def make_requests(n, vocab):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(16, 129, (n,), generator=g).tolist()
    new = torch.randint(16, 257, (n,), generator=g).tolist()
    return [{"tokens": torch.randint(0, vocab, (L,), generator=g).tolist(), "new": m, "seed": i}
            for i, (L, m) in enumerate(zip(lens, new))]


def run_engine(eng, reqs, adapters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, r in enumerate(reqs):
        kw = {} if adapters is None else {"adapter": i % adapters}
        eng.submit(r["tokens"], r["new"], temperature=0.8, top_k=50, seed=r["seed"], **kw)
    got = {}
    while eng.has_work():
        for rid, new, _fin in eng.step():
            got.setdefault(rid, []).extend(new)
    torch.cuda.synchronize()
    return {"wall": time.perf_counter() - t0, "tokens": [got[k] for k in sorted(got)]}


def engine_part(a, dev):
    torch.manual_seed(0)
    model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    reqs = make_requests(a.requests, model.cfg.vocab_size)
    requested = sum(r["new"] for r in reqs)
    max_len = max(len(r["tokens"]) for r in reqs) + max(r["new"] for r in reqs)
    paths = {}
    eng = GPT2Engine(model, slots=64, max_len=max_len, poll_every=8)  # captured without a stack
    paths["(a) no stack"] = lambda: run_engine(eng, reqs, None)
    if not a.base_only:
        from ray_amd.models.lora import LoRAStack, target_dims

        stack = LoRAStack(model.cfg, 4, 16, dev, torch.bfloat16)
        g = torch.Generator().manual_seed(2)
        for i in range(4):
            state = {}
            for layer in range(model.cfg.n_layer):
                for t, (din, dout) in target_dims(model.cfg).items():
                    state[f"h.{layer}.{t}.lora_A"] = torch.randn(16, din, generator=g) * 0.02
                    state[f"h.{layer}.{t}.lora_B"] = torch.randn(dout, 16, generator=g) * 0.02
            stack.load(i, state, alpha=32)
        leng = GPT2Engine(model, slots=64, max_len=max_len, poll_every=8, lora=stack)
        paths["(b) stack attached, all requests base"] = lambda: run_engine(leng, reqs, None)
        paths["(c) requests over four adapters"] = lambda: run_engine(leng, reqs, 4)
    first = {n: fn() for n, fn in paths.items()}  # warm-up
    runs = {n: [] for n in paths}
    for _ in range(a.repeats):
        for n, fn in paths.items():
            runs[n].append(fn())
    rows = []
    for n, rs in runs.items():
        rec = {"path": n, "requested_tokens": requested,
               "tok_per_s": stats([requested / r["wall"] for r in rs]),
               "same_as_a": sum(x == y for x, y in zip(first[n]["tokens"],
                                                       first["(a) no stack"]["tokens"]))
               / len(reqs),
               "repeatable": all(r["tokens"] == first[n]["tokens"] for r in rs)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "lora.md"))
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--no-engine", dest="engine", action="store_false")
    ap.add_argument("--no-kernels", dest="kernels", action="store_false")
    ap.add_argument("--package-root", default=None, help="time this checkout of the package")
    ap.add_argument("--base-only", action="store_true", help="engine row (a) alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    krows = kernel_part(a, dev) if a.kernels and not a.base_only else []
    torch.cuda.empty_cache()
    erows = engine_part(a, dev) if a.engine else []

    def cell(s, fmt=".1f"):
        return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"

    lines = ["# Per-row low-rank adapters: lora.hip and the GPT-2 engine", "",
             f"`scripts/lora_bench.py` on {torch.cuda.get_device_name(0)}.", ""]
    if krows:
        lines += [
            "## lora_add, GPT-2 small's four linears, three adapters mixed with base rows", "",
            "Device microseconds per call, both paths captured in a HIP graph (20 calls per "
            f"replay), device events around alternating blocks, >= {a.seconds:g} s of timed work "
            f"per path and repeat, median (min..max) of {a.repeats} repeats. `bmm` is "
            "`ref.lora_add_bmm`. `rel diff`: relative norm of the two paths' difference on "
            "one call with scales 0.5, 2, 8 (bf16 outputs).", "",
            "| linear | R | Bn | T | hip us | bmm us | hip vs bmm | rel diff |",
            "|---|---|---|---|---|---|---|---|"]
        for r in krows:
            dv = r["device_us"]
            lines.append(f"| {r['linear']} | {r['R']} | {r['Bn']} | {r['T']} | "
                         f"{cell(dv['hip'], '.2f')} | {cell(dv['bmm'], '.2f')} | "
                         f"{dv['bmm']['median'] / dv['hip']['median']:.2f}x | "
                         f"{r['rel_diff']:.1e} |")
    if erows:
        lines += ["", "## The engine with and without an adapter stack, GPT-2 small bf16, S 64",
                  "", f"{a.requests} requests (prompts 16..128, max_new_tokens uniform in "
                  f"16..256, {erows[0]['requested_tokens']} requested tokens, temperature 0.8, "
                  "top-k 50, a seed each), all queued at t0, `poll_every` 8. Wall time around "
                  f"synchronised calls, the paths alternated, median (min..max) of {a.repeats} "
                  "repeats after one warm-up run. `same tokens`: share of requests whose tokens "
                  "equal row (a)'s.", "",
                  "| path | requested tokens/s | same tokens | repeatable |", "|---|---|---|---|"]
        for r in erows:
            lines.append(f"| {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{r['same_as_a']:.2f} | {r['repeatable']} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
