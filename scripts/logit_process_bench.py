#!/usr/bin/env python
"""Logit processors: the kernel (ops/csrc/logit_proc.hip through ``rf.logit_process``)
against a plain-torch composition of the same rules, what ``GPT2Engine(...,
logit_processors=True)`` costs end to end, and how often greedy requests still loop.

    python scripts/logit_process_bench.py [--out profiles/r17/logit_process.md]

Kernel part: V = 50257 bf16 logits (randn x 4) as the [:, :V] view of a [B, 50304] buffer,
B 1 / 8 / 64 / 320 (320 = 64 slots x 5 window rows of a speculative step), every row with
its own context of 128 or 1000 tokens (half prompt, half output, random ids; tables 1024
wide), ``repetition`` 1.3, ``presence`` 0.2, ``frequency`` 0.5 and three bias entries.
``hip`` is one ``rf.logit_process`` call, ``torch`` the dense composition
``ref.logit_process`` (scatter / scatter_add / scatter_reduce over [B, V] tables, then
``where``): the same bits, checked first. 20 calls of one path captured in one HIP graph
and replayed, device events around blocks of replays, a warm-up and at least ``--seconds``
of timed work per path and repeat, the paths alternated, median (min..max) of
``--repeats``, microseconds per call.

Engine part: GPT-2 small, bf16, the request mix of scripts/gpt2_engine_bench.py
(``--requests`` seeded requests, prompts 16..128, ``max_new_tokens`` uniform in 16..256,
temperature 0.8, top-k 50, all queued at t0) at S 8 and S 64 with ``poll_every`` 8:
``logit_processors=False``, on with every request neutral, on with ``repetition_penalty=1.3,
frequency_penalty=0.5`` on every request, and the same with ``speculate=4``. Engines built
once outside the timed window, wall time around synchronised runs, the paths alternated,
median (min..max) of ``--repeats`` after one warm-up run.

Loops: the greedy requests of scripts/gpt2_spec_bench.py part (d) (64 prompts, each followed
by 64 tokens of its own greedy continuation, 256 new tokens, temperature 0): the share of
requests whose output ends in a repeated cycle (its last 32 tokens have a period <= 16),
without and with ``repetition_penalty=1.3``. One number, random-init weights.

``--repo PATH`` imports ``ray_amd`` from another checkout and ``--engine-json FILE`` dumps the
engine rows: with ``--cases none`` that measures the engine without the argument on another
commit, and ``--parent-json FILE`` puts such rows beside this commit's in the write-up."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "r17", "logit_process.md"))
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--requests", type=int, default=256)
ap.add_argument("--cases", default="all", choices=["all", "none"])
ap.add_argument("--no-kernel", dest="kernel", action="store_false")
ap.add_argument("--no-engine", dest="engine", action="store_false")
ap.add_argument("--no-loops", dest="loops", action="store_false")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--engine-json")
ap.add_argument("--parent-json", action="append", default=[])
ap.add_argument("--resources", help="the kernel's VGPR / scratch / LDS line, for the write-up")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.repo))

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402
from ray_amd.ops import reference as ref  # noqa: E402

V, VPAD, WIDTH = 50257, 50304, 1024
BATCHES = (1, 8, 64, 320)
CONTEXTS = (128, 1000)
GRAPH_CALLS = 20
CONTROLS = {"repetition_penalty": 1.3, "frequency_penalty": 0.5}


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
    """fn captured GRAPH_CALLS times back to back in one HIP graph: a replay costs the
    device time of the calls without the host's per-call launch work."""
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
    reps = {n: graphed(fn) for n, fn in paths.items()}
    iters = {}
    for name, fn in reps.items():  # warm-up + block length for >= seconds
        block_us(fn, 5)
        iters[name] = max(5, int(seconds * 1e6 / block_us(fn, 10)) + 1)
    times = {n: [] for n in reps}
    for _ in range(repeats):
        for name, fn in reps.items():  # alternate the paths
            times[name].append(block_us(fn, iters[name]) / GRAPH_CALLS)
    return {n: stats(t) for n, t in times.items()}


def kernel_part(a, dev):
    rows = []
    i32, f32 = torch.int32, torch.float32
    for B in BATCHES:
        for ctx in CONTEXTS:
            g = torch.Generator().manual_seed(B * 7 + ctx)
            x = (torch.randn(B, V, generator=g) * 4).bfloat16()
            tables = [torch.randint(0, V, (B, WIDTH), generator=g).to(i32),
                      torch.full((B,), ctx // 2, dtype=i32),
                      torch.randint(0, V, (B, WIDTH), generator=g),
                      torch.full((B,), ctx - ctx // 2, dtype=i32),
                      torch.full((B,), 1.3), torch.full((B,), 0.2), torch.full((B,), 0.5),
                      torch.zeros(B, dtype=i32),
                      torch.randint(0, V, (B, rf.LOGIT_BIAS_MAX), generator=g).to(i32),
                      torch.randn(B, rf.LOGIT_BIAS_MAX, generator=g).to(f32),
                      torch.full((B,), 3, dtype=i32)]
            tables = [t.to(dev) for t in tables]
            bufs = {}
            for name in ("hip", "torch"):
                buf = torch.zeros(B, VPAD, dtype=torch.bfloat16)
                buf[:, :V] = x
                bufs[name] = buf.to(dev)[:, :V]
            paths = {"hip": lambda: rf.logit_process(bufs["hip"], *tables),
                     "torch": lambda: ref.logit_process(bufs["torch"], *tables)}
            # same results first: faster and different is not faster
            paths["hip"](), paths["torch"]()
            rec = {"B": B, "context": ctx,
                   "bit_equal": bool(torch.equal(bufs["hip"].view(torch.int16),
                                                 bufs["torch"].view(torch.int16))),
                   "edited": int((bufs["hip"].cpu() != x).sum())}
            rec["device_us"] = time_graphed(paths, a.seconds, a.repeats)
            rec["speedup"] = rec["device_us"]["torch"]["median"] / rec["device_us"]["hip"]["median"]
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    return rows


def make_requests(n, vocab):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(16, 129, (n,), generator=g).tolist()
    new = torch.randint(16, 257, (n,), generator=g).tolist()
    return [{"tokens": torch.randint(0, vocab, (L,), generator=g).tolist(), "new": m, "seed": i}
            for i, (L, m) in enumerate(zip(lens, new))]


def run_engine(eng, reqs, controls, temperature=0.8, top_k=50):
    steps0 = eng.steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [eng.submit(r["tokens"], r["new"], temperature=temperature, top_k=top_k,
                       seed=r["seed"], **controls) for r in reqs]
    got = {}
    while eng.has_work():
        for ev in eng.step():
            got.setdefault(ev[0], []).extend(ev[1])
    torch.cuda.synchronize()
    return {"wall": time.perf_counter() - t0, "tokens": [got[r] for r in rids],
            "steps": eng.steps - steps0}


def engine_part(a, dev, model):
    reqs = make_requests(a.requests, model.cfg.vocab_size)
    requested = sum(r["new"] for r in reqs)
    max_len = max(len(r["tokens"]) for r in reqs) + max(r["new"] for r in reqs)
    cases = [("off", {}, {})]
    if a.cases == "all":
        on = {"logit_processors": True}
        cases = [("logit_processors=False", {"logit_processors": False}, {}),
                 ("on, neutral requests", on, {}),
                 ("on, repetition 1.3 + frequency 0.5", on, CONTROLS),
                 ("speculate=4", {"speculate": 4}, {}),
                 ("speculate=4, on, repetition 1.3 + frequency 0.5", dict(on, speculate=4),
                  CONTROLS)]
    rows = []
    for S in (8, 64):
        paths = {}
        for name, kw, ctl in cases:
            eng = GPT2Engine(model, slots=S, max_len=max_len, poll_every=8, **kw)
            paths[name] = lambda eng=eng, ctl=ctl: run_engine(eng, reqs, ctl)
        first = {n: fn() for n, fn in paths.items()}  # warm-up
        runs = {n: [] for n in paths}
        for _ in range(a.repeats):
            for n, fn in paths.items():
                runs[n].append(fn())
        for n, rs in runs.items():
            # the engine without controls at the same ``speculate``
            ref_name = "speculate=4" if n.startswith("speculate") else cases[0][0]
            rec = {"S": S, "path": n, "requested_tokens": requested,
                   "tok_per_s": stats([requested / r["wall"] for r in rs]),
                   "emitted": sum(len(t) for t in rs[0]["tokens"]), "steps": rs[0]["steps"],
                   "same_tokens": sum(x == y for x, y in zip(first[n]["tokens"],
                                                             first[ref_name]["tokens"]))
                   / len(reqs),
                   "repeatable": all(r["tokens"] == first[n]["tokens"] for r in rs)}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
        del paths
        torch.cuda.empty_cache()
    return rows


def ends_in_cycle(toks, tail=32, max_period=16):
    t = toks[-tail:]
    return len(t) == tail and any(all(t[i] == t[i - p] for i in range(p, tail))
                                  for p in range(1, max_period + 1))


def loops_part(a, dev, model):
    n = min(a.requests, 64)
    base = make_requests(n, model.cfg.vocab_size)
    lens = [len(r["tokens"]) for r in base]
    reqs = []
    for c in range(0, n, 16):  # each prompt followed by 64 tokens of its greedy continuation
        part = base[c: c + 16]
        idx = torch.zeros(len(part), max(lens[c: c + 16]), dtype=torch.long)
        for b, r in enumerate(part):
            idx[b, : len(r["tokens"])] = torch.tensor(r["tokens"])
        out = model.generate(idx.to(dev), 64, lens=lens[c: c + 16], temperature=0.0, seeds=0,
                             graph=True).cpu()
        reqs += [{"tokens": r["tokens"] + out[b].tolist(), "new": 256, "seed": r["seed"]}
                 for b, r in enumerate(part)]
    max_len = max(len(r["tokens"]) for r in reqs) + 256
    eng = GPT2Engine(model, slots=64, max_len=max_len, logit_processors=True)
    rec = {"requests": len(reqs)}
    for name, ctl in (("plain", {}), ("repetition_penalty=1.3", {"repetition_penalty": 1.3})):
        toks = run_engine(eng, reqs, ctl, temperature=0.0, top_k=None)["tokens"]
        rec[name] = sum(ends_in_cycle(t) for t in toks) / len(toks)
    print(json.dumps(rec), flush=True)
    return rec


def cell(s, fmt=".1f"):
    return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("logit_process_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    krows = kernel_part(a, dev) if a.kernel and a.cases == "all" else []
    torch.cuda.empty_cache()
    model = None
    if a.engine or a.loops:
        torch.manual_seed(0)
        model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    erows = engine_part(a, dev, model) if a.engine else []
    if a.engine_json:
        os.makedirs(os.path.dirname(a.engine_json) or ".", exist_ok=True)
        with open(a.engine_json, "w") as fh:
            json.dump(erows, fh)
    if a.cases != "all":
        return
    loops = loops_part(a, dev, model) if a.loops else None
    prows = []
    for i, path in enumerate(a.parent_json):
        with open(path) as fh:
            prows += [dict(r, path=f"parent commit, process {i + 1}") for r in json.load(fh)]

    lines = ["# Logit processors: penalties, logit bias, minimum length", "",
             f"`scripts/logit_process_bench.py` on {torch.cuda.get_device_name(0)}.", ""]
    if a.resources:
        lines += ["## The kernel's resources", "", a.resources, ""]
    if krows:
        lines += [f"## One call, V = {V} bf16 (a view of a [B, {VPAD}] buffer)", "",
                  f"Every row with its own context of `context` tokens (half prompt, half output, "
                  f"random ids, tables {WIDTH} wide), repetition 1.3, presence 0.2, frequency 0.5, "
                  f"three bias entries. {GRAPH_CALLS} calls of one path captured in one HIP graph "
                  f"and replayed, device events, the paths alternated, >= {a.seconds:g} s of timed "
                  f"work per path and repeat, median (min..max) of {a.repeats} repeats, "
                  "microseconds per call. `torch`: `ref.logit_process`, the dense composition "
                  "(scatter, scatter_add and scatter_reduce into [B, V] tables, then `where`). "
                  "`edited`: elements of the buffer the first call changed.", "",
                  "| B | context | hip device us | torch device us | torch / hip | bit equal | "
                  "edited |", "|---|---|---|---|---|---|---|"]
        for r in krows:
            dv = r["device_us"]
            lines.append(f"| {r['B']} | {r['context']} | {cell(dv['hip'], '.2f')} | "
                         f"{cell(dv['torch'])} | {r['speedup']:.1f}x | {r['bit_equal']} | "
                         f"{r['edited']} |")
    if erows:
        lines += ["", "## Engine, GPT-2 small bf16, poll_every 8", "",
                  f"{a.requests} requests (prompts 16..128, max_new_tokens uniform in 16..256, "
                  f"{erows[0]['requested_tokens']} requested tokens, temperature 0.8, top-k 50, a "
                  "seed each), all queued at t0. Wall time around synchronised runs, the paths "
                  f"alternated, median (min..max) of {a.repeats} repeats after one warm-up run. "
                  "`same tokens`: share of requests whose tokens equal those of the engine "
                  "without controls at the same `speculate`. `parent commit`: this script with "
                  "`--repo` on a checkout of the parent and `--cases none`, in processes of "
                  "their own.",
                  "", "| S | path | requested tokens/s | vs off | device steps | same tokens | "
                  "repeatable |", "|---|---|---|---|---|---|---|"]
        for r in prows:
            lines.append(f"| {r['S']} | {r['path']} | {cell(r['tok_per_s'], '.0f')} | | "
                         f"{r['steps']} | | {r['repeatable']} |")
        for r in erows:
            base = next(x for x in erows if x["S"] == r["S"]
                        and x["path"] == "logit_processors=False")
            lines.append(f"| {r['S']} | {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{r['tok_per_s']['median'] / base['tok_per_s']['median']:.3f}x | "
                         f"{r['steps']} | {r['same_tokens']:.2f} | {r['repeatable']} |")
    if loops:
        lines += ["", "## Greedy loops", "",
                  f"{loops['requests']} greedy requests (the prompts of scripts/gpt2_spec_bench.py "
                  "part (d): a random prompt followed by 64 tokens of its own greedy continuation, "
                  "256 new tokens). Share whose output ends in a repeated cycle (the last 32 "
                  f"tokens have a period <= 16): {loops['plain']:.2f} without controls, "
                  f"{loops['repetition_penalty=1.3']:.2f} with `repetition_penalty=1.3`. One "
                  "number on random-init weights, not a statement about real text."]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
