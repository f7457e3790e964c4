#!/usr/bin/env python
"""Continuous batching: the two slot kernels (ops/csrc/kv_slots.hip) against their torch
compositions, and ``GPT2Engine`` against static batching through ``generate``.

    python scripts/gpt2_engine_bench.py [--out profiles/r10/engine.md]

Kernel part. ``kv_insert``: 12 layers of GPT-2-small K/V (H = 12, D = 64) of Bn prompts of
T positions into random slots of a 64-slot, 1024-position cache; ``hip`` is 12
``rf.kv_insert`` calls, ``indexed`` the composition ``cache.k[i, slots, :, :n] = ...`` (two
``index_put_`` per layer with the slot ids on the device). ``slot_advance``: one
``rf.slot_advance`` call against the same bookkeeping written as torch ops
(``ref.slot_advance`` on the GPU). Device events around alternating blocks of the paths in
one process, a warm-up and at least ``--seconds`` of timed work per path and repeat, median
(min..max) of ``--repeats``; ``call`` is eager calls (host launch work included), ``device``
20 calls captured in one HIP graph and replayed.

End-to-end part: GPT-2 small, bf16, ``--requests`` seeded requests (prompt lengths 16..128,
``max_new_tokens`` uniform in 16..256, temperature 0.8, top-k 50), all queued at t0. Static:
chunks of 8 and of 64 in arrival order through ``generate(seeds=..., graph=True)``, a
request complete when its chunk's call returns. Engine: S = 8 and 64, ``poll_every`` 1 and
8, built (cache, capture) once outside the timed window as a server builds it, a request
complete when its ``finished`` event arrives. Wall time around synchronised calls, the
paths alternated, median (min..max) of ``--repeats``."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402
from ray_amd.ops import reference as ref  # noqa: E402

H, D, LAYERS = 12, 64, 12
CACHE_SLOTS, CACHE_T = 64, 1024
INSERT_SHAPES = [(1, 128), (8, 128), (8, 1024)]
ADVANCE_S = [8, 64]
ADVANCE_CAP = 1 << 20  # columns per slot: no slot fills up inside a timed block
GRAPH_CALLS = 20


def block_us(fn, iters, prep=None):
    if prep is not None:
        prep()
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


def time_paths(paths, seconds, repeats, in_graph=False, prep=None, max_iters=None):
    if in_graph:
        if max_iters is not None:
            max_iters //= GRAPH_CALLS
        res = time_paths({n: graphed(fn) for n, fn in paths.items()}, seconds, repeats,
                         prep=prep, max_iters=max_iters)
        return {n: {k: v / GRAPH_CALLS for k, v in s.items()} for n, s in res.items()}
    iters = {}
    for name, fn in paths.items():  # warm-up + block length for >= seconds
        block_us(fn, 10, prep)
        iters[name] = max(20, int(seconds * 1e6 / block_us(fn, 50, prep)) + 1)
        if max_iters is not None:
            iters[name] = min(iters[name], max_iters)
    times = {n: [] for n in paths}
    for _ in range(repeats):
        for name, fn in paths.items():  # alternate the paths
            times[name].append(block_us(fn, iters[name], prep))
    return {n: stats(t) for n, t in times.items()}


def insert_part(a, dev):
    g = torch.Generator().manual_seed(0)
    kc = torch.zeros(LAYERS, CACHE_SLOTS, H, CACHE_T, D, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    rows = []
    for Bn, T in INSERT_SHAPES:
        qkv = torch.randn(Bn, T, 3, H, D, generator=g).bfloat16().to(dev)
        slots = torch.randperm(CACHE_SLOTS, generator=g)[:Bn].to(dev)
        slots32 = slots.to(torch.int32)
        lens = torch.full((Bn,), T, dtype=torch.int32, device=dev)

        def hip():
            for i in range(LAYERS):
                rf.kv_insert(qkv, kc[i], vc[i], slots32, lens)

        def indexed():
            for i in range(LAYERS):
                kc[i, slots, :, :T] = qkv[:, :, 1].transpose(1, 2)
                vc[i, slots, :, :T] = qkv[:, :, 2].transpose(1, 2)

        # same results first: faster and different is not faster
        outs = []
        for fn in (hip, indexed):
            kc.zero_()
            vc.zero_()
            fn()
            outs.append((kc.clone(), vc.clone()))
        same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        del outs
        paths = {"hip": hip, "indexed": indexed}
        rec = {"Bn": Bn, "T": T, "same": bool(same),
               "us": time_paths(paths, a.seconds, a.repeats),
               "device_us": time_paths(paths, a.seconds, a.repeats, in_graph=True)}
        moved = 2 * 2 * LAYERS * Bn * T * H * D * 2  # K and V, read and written
        rec["hip_GBps"] = moved / rec["device_us"]["hip"]["median"] * 1e-3
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def advance_part(a, dev):
    rows = []
    for S in ADVANCE_S:
        g = torch.Generator().manual_seed(S)
        tok = torch.randint(0, 50256, (S,), generator=g).to(dev)  # never the EOS id below
        lens = torch.full((S,), 100, dtype=torch.int32, device=dev)
        n_out = torch.zeros(S, dtype=torch.int32, device=dev)
        max_new = torch.full((S,), 1 << 30, dtype=torch.int32, device=dev)
        active = torch.ones(S, dtype=torch.uint8, device=dev)
        active[::4] = 0  # a quarter of the slots idle
        out = torch.zeros(S, ADVANCE_CAP, dtype=torch.int64, device=dev)
        paths = {"hip": lambda: rf.slot_advance(tok, lens, n_out, max_new, active, out, 50256),
                 "torch": lambda: ref.slot_advance(tok, lens, n_out, max_new, active, out, 50256)}
        rec = {"S": S, "device_us": time_paths(paths, a.seconds, a.repeats, in_graph=True,
                                               prep=n_out.zero_, max_iters=ADVANCE_CAP // 2)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del out
    return rows


# ------------------------------------------------------------------ end to end
def make_requests(n, vocab):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(16, 129, (n,), generator=g).tolist()
    new = torch.randint(16, 257, (n,), generator=g).tolist()
    return [{"tokens": torch.randint(0, vocab, (L,), generator=g).tolist(), "new": m, "seed": i}
            for i, (L, m) in enumerate(zip(lens, new))]


def run_static(model, reqs, chunk, dev, temp, top_k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done, toks, steps, rows = [], [], 0, 0
    for c in range(0, len(reqs), chunk):
        part = reqs[c: c + chunk]
        lens = [len(r["tokens"]) for r in part]
        new = max(r["new"] for r in part)
        idx = torch.zeros(len(part), max(lens), dtype=torch.long)
        for b, r in enumerate(part):
            idx[b, : lens[b]] = torch.tensor(r["tokens"])
        out = model.generate(idx.to(dev), new, lens=lens, temperature=temp, top_k=top_k,
                             seeds=[r["seed"] for r in part], graph=True).cpu()
        t = time.perf_counter() - t0
        done += [t] * len(part)
        toks += [out[b, : r["new"]].tolist() for b, r in enumerate(part)]
        steps += new
        rows += new * len(part)
    return {"wall": time.perf_counter() - t0, "done": done, "tokens": toks, "steps": steps,
            "row_steps": rows}


def run_engine(eng, reqs, temp, top_k):
    steps0 = eng.steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [eng.submit(r["tokens"], r["new"], temperature=temp, top_k=top_k, seed=r["seed"])
            for r in reqs]
    got, fin = {}, {}
    while eng.has_work():
        for rid, new, finished in eng.step():
            got.setdefault(rid, []).extend(new)
            if finished:
                fin[rid] = time.perf_counter() - t0
    torch.cuda.synchronize()
    steps = eng.steps - steps0
    return {"wall": time.perf_counter() - t0, "done": [fin[r] for r in rids],
            "tokens": [got[r] for r in rids], "steps": steps, "row_steps": steps * eng.slots}


def e2e_part(a, dev):
    torch.manual_seed(0)
    model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    reqs = make_requests(a.requests, model.cfg.vocab_size)
    requested = sum(r["new"] for r in reqs)
    max_len = max(len(r["tokens"]) for r in reqs) + max(r["new"] for r in reqs)
    temp, top_k = 0.8, 50
    paths = {}
    for chunk in (8, 64):
        paths[f"static {chunk}"] = lambda chunk=chunk: run_static(model, reqs, chunk, dev, temp,
                                                                  top_k)
    for S in (8, 64):
        for pe in (1, 8):
            eng = GPT2Engine(model, slots=S, max_len=max_len, poll_every=pe)
            paths[f"engine S={S} poll_every={pe}"] = lambda eng=eng: run_engine(eng, reqs, temp,
                                                                                top_k)
    first = {n: fn() for n, fn in paths.items()}  # warm-up
    runs = {n: [] for n in paths}
    for _ in range(a.repeats):
        for n, fn in paths.items():
            runs[n].append(fn())
    rows = []
    for n, rs in runs.items():
        done = [sorted(r["done"]) for r in rs]
        rec = {"path": n, "requested_tokens": requested, "max_len": max_len,
               "tok_per_s": stats([requested / r["wall"] for r in rs]),
               "mean_done_s": stats([sum(d) / len(d) for d in done]),
               "p95_done_s": stats([d[int(0.95 * (len(d) - 1))] for d in done]),
               "steps": rs[0]["steps"], "occupancy": requested / rs[0]["row_steps"],
               "same_as_static_8": sum(x == y for x, y in zip(first[n]["tokens"],
                                                             first["static 8"]["tokens"]))
               / len(reqs),
               "repeatable": all(r["tokens"] == first[n]["tokens"] for r in rs)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "engine.md"))
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--no-e2e", dest="e2e", action="store_false")
    ap.add_argument("--no-kernels", dest="kernels", action="store_false")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpt2_engine_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    irows = insert_part(a, dev) if a.kernels else []
    arows = advance_part(a, dev) if a.kernels else []
    torch.cuda.empty_cache()
    erows = e2e_part(a, dev) if a.e2e else []

    def cell(s, fmt=".1f"):
        return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"

    lines = ["# Continuous batching: slot kernels and the GPT-2 engine", "",
             f"`scripts/gpt2_engine_bench.py` on {torch.cuda.get_device_name(0)}.", ""]
    if irows:
        lines += [
            "## kv_insert, 12 layers (H = 12, D = 64, bf16, 64-slot x 1024-position cache)", "",
            f"Device events, the paths alternated in one process, >= {a.seconds:g} s of timed work "
            f"per path and repeat, median (min..max) of {a.repeats} repeats, microseconds per 12 "
            "layers. `call`: eager calls from Python; `device`: captured in one HIP graph and "
            "replayed. `indexed` is `cache.k[i, slots, :, :n] = ...` (and V). GB/s: K/V bytes "
            "read plus written over the hip device median.", "",
            "| Bn | T | hip call us | indexed call us | hip device us | indexed device us | "
            "hip vs indexed (device) | hip GB/s | same bits |",
            "|---|---|---|---|---|---|---|---|---|"]
        for r in irows:
            u, dv = r["us"], r["device_us"]
            lines.append(f"| {r['Bn']} | {r['T']} | {cell(u['hip'])} | {cell(u['indexed'])} | "
                         f"{cell(dv['hip'], '.2f')} | {cell(dv['indexed'], '.2f')} | "
                         f"{dv['indexed']['median'] / dv['hip']['median']:.2f}x | "
                         f"{r['hip_GBps']:.0f} | {r['same']} |")
    if arows:
        lines += ["", "## slot_advance, one call", "",
                  "Both paths captured in a HIP graph (20 calls per replay), microseconds per "
                  "call; `torch` is the same bookkeeping as torch ops (`ref.slot_advance`).", "",
                  "| S | hip device us | torch device us | hip vs torch |", "|---|---|---|---|"]
        for r in arows:
            dv = r["device_us"]
            lines.append(f"| {r['S']} | {cell(dv['hip'], '.2f')} | {cell(dv['torch'], '.2f')} | "
                         f"{dv['torch']['median'] / dv['hip']['median']:.1f}x |")
    if erows:
        lines += ["", "## Engine against static batching, GPT-2 small bf16", "",
                  f"{a.requests} requests (prompts 16..128, max_new_tokens uniform in 16..256, "
                  f"{erows[0]['requested_tokens']} requested tokens, temperature 0.8, top-k 50, a "
                  f"seed each), all queued at t0; cache capacity {erows[0]['max_len']} for every "
                  "path. Wall time around synchronised calls, the paths alternated, median "
                  f"(min..max) of {a.repeats} repeats after one warm-up run. Completion times "
                  "count from t0. Occupancy: requested tokens over steps x width. `same tokens`: "
                  "share of requests whose tokens equal the static-8 run's (bf16: another "
                  "prefill shape or decode width can flip a near-tie).", "",
                  "| path | requested tokens/s | mean completion s | p95 completion s | "
                  "device steps | occupancy | same tokens | repeatable |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in erows:
            lines.append(f"| {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{cell(r['mean_done_s'], '.2f')} | {cell(r['p95_done_s'], '.2f')} | "
                         f"{r['steps']} | {r['occupancy']:.2f} | {r['same_as_static_8']:.2f} | "
                         f"{r['repeatable']} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
