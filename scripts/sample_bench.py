#!/usr/bin/env python
"""The device-side token sampler (ops/csrc/sample.hip through ``rf.sample_logits``) against
the reference composition (``ref.sample_logits``, plain torch) on the same GPU, and
``GPT2.generate`` with the ``generator`` path against the ``seeds`` path.

    python scripts/sample_bench.py [--out profiles/r9/sample.md]

Sampler part: V = 50257 bf16 logits (randn x 4) as the [:, :V] view of a [B, 50304] buffer,
every row with the same (T, k, p). ``hip`` is one ``rf.sample_logits`` call, ``reference``
one ``ref.sample_logits`` call, ``pick`` (where top-p is off) the ``GPT2._pick`` chain of
the ``generator`` path. Device events around alternating blocks of the paths in one
process, a warm-up and at least ``--seconds`` of timed work per path and repeat, median
(min..max) of ``--repeats``; once as eager calls (host launch work included) and once as
20 calls captured in one HIP graph and replayed (device time; ``pick`` draws from a
generator and is not captured).

End-to-end part: GPT-2 small, bf16, a 128-token prompt and 128 new tokens at temperature
0.8, top-k 50; wall time around a synchronised call, the four paths alternated, median of
``--repeats``.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402
from ray_amd.ops import reference as ref  # noqa: E402

V, VPAD = 50257, 50304
BATCHES = (1, 8, 64)
PARAMS = [(1.0, 0, 1.0), (0.8, 50, 1.0), (1.0, 0, 0.9), (0.8, 50, 0.95)]
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


def time_paths(paths, seconds, repeats, in_graph=False):
    if in_graph:
        res = time_paths({n: graphed(fn) for n, fn in paths.items()}, seconds, repeats)
        return {n: {k: v / GRAPH_CALLS for k, v in s.items()} for n, s in res.items()}
    iters = {}
    for name, fn in paths.items():  # warm-up + block length for >= seconds
        block_us(fn, 10)
        iters[name] = max(20, int(seconds * 1e6 / block_us(fn, 50)) + 1)
    times = {n: [] for n in paths}
    for _ in range(repeats):
        for name, fn in paths.items():  # alternate the paths
            times[name].append(block_us(fn, iters[name]))
    return {n: stats(t) for n, t in times.items()}


def sampler_part(a, dev):
    rows = []
    for B in BATCHES:
        g = torch.Generator().manual_seed(B)
        buf = torch.zeros(B, VPAD, dtype=torch.bfloat16)
        buf[:, :V] = (torch.randn(B, V, generator=g) * 4).bfloat16()
        lg = buf.to(dev)[:, :V]
        seeds = torch.arange(B, dtype=torch.int64, device=dev)
        steps = torch.full((B,), 130, dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        for T, k, p in PARAMS:
            Tt = torch.full((B,), T, device=dev)
            kt = torch.full((B,), k, dtype=torch.int32, device=dev)
            pt = torch.full((B,), p, device=dev)
            paths = {
                "hip": lambda: rf.sample_logits(lg, Tt, kt, pt, seeds, steps, validate=False),
                "reference": lambda: ref.sample_logits(lg, Tt, kt, pt, seeds, steps),
            }
            # same results first: faster and different is not faster
            o = {n: fn() for n, fn in paths.items()}
            rec = {"B": B, "T": T, "k": k, "p": p,
                   "tokens_equal_reference": float((o["hip"] == o["reference"]).float().mean())}
            rec["device_us"] = {}
            for n in list(paths):  # one path per capture
                rec["device_us"].update(time_paths({n: paths[n]}, a.seconds, a.repeats,
                                                   in_graph=True))
            if p >= 1:
                paths["pick"] = lambda: GPT2._pick(lg, T, k or None, gen)
            rec["us"] = time_paths(paths, a.seconds, a.repeats)
            rec["speedup_call"] = rec["us"]["reference"]["median"] / rec["us"]["hip"]["median"]
            rec["speedup_device"] = (rec["device_us"]["reference"]["median"]
                                     / rec["device_us"]["hip"]["median"])
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    return rows


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def e2e_part(a, dev):
    torch.manual_seed(0)
    model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    rows = []
    kw = dict(temperature=0.8, top_k=50)
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        idx = torch.randint(0, model.cfg.vocab_size, (B, a.prompt), generator=g).to(dev)

        def gen_path(graph):
            gen = torch.Generator(device=dev).manual_seed(1)
            return model.generate(idx, a.new, generator=gen, graph=graph, **kw)

        paths = {"generator eager": lambda: gen_path(False),
                 "generator graph": lambda: gen_path(True),
                 "seeds eager": lambda: model.generate(idx, a.new, seeds=1, **kw),
                 "seeds graph": lambda: model.generate(idx, a.new, seeds=1, graph=True, **kw)}
        outs = {n: wall(fn)[1] for n, fn in paths.items()}  # warm-up
        times = {n: [] for n in paths}
        for _ in range(a.repeats):
            for n, fn in paths.items():
                times[n].append(wall(fn)[0])
        rec = {"B": B, "prompt": a.prompt, "new": a.new,
               "seeds_graph_equals_eager": bool(torch.equal(outs["seeds eager"],
                                                            outs["seeds graph"])),
               "tok_per_s": {n: stats([B * a.new / x for x in t]) for n, t in times.items()}}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r9", "sample.md"))
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--no-e2e", dest="e2e", action="store_false")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    srows = sampler_part(a, dev)
    erows = e2e_part(a, dev) if a.e2e else []

    def cell(s, fmt=".1f"):
        return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"

    lines = ["# Device-side token sampler", "",
             f"`scripts/sample_bench.py` on {torch.cuda.get_device_name(0)}.", "",
             f"## One call, V = {V} bf16 (a view of a [B, {VPAD}] buffer)", "",
             f"Device events, the paths alternated in one process, >= {a.seconds:g} s of timed "
             f"work per path and repeat, median (min..max) of {a.repeats} repeats, microseconds "
             "per call. `call`: eager calls from Python, host launch work included; `device`: "
             f"{GRAPH_CALLS} calls captured in one HIP graph and replayed, per call. `reference` "
             "is `ref.sample_logits` on the GPU, `pick` the `GPT2._pick` chain of the "
             "`generator` path (no top-p). `same`: share of rows where hip and reference drew "
             "the same token.", "",
             "| B | T | k | p | hip call us | reference call us | pick call us | hip vs ref "
             "(call) | hip device us | reference device us | hip vs ref (device) | same |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in srows:
        u, dv = r["us"], r["device_us"]
        lines.append(f"| {r['B']} | {r['T']} | {r['k']} | {r['p']} | {cell(u['hip'])} | "
                     f"{cell(u['reference'])} | {cell(u['pick']) if 'pick' in u else 'n/a'} | "
                     f"{r['speedup_call']:.1f}x | {cell(dv['hip'], '.2f')} | "
                     f"{cell(dv['reference'], '.1f')} | {r['speedup_device']:.1f}x | "
                     f"{r['tokens_equal_reference']:.2f} |")
    if erows:
        lines += ["", "## generate, GPT-2 small bf16, temperature 0.8, top-k 50", "",
                  f"{a.prompt}-token prompt, {a.new} new tokens; wall time around a synchronised "
                  f"call, paths alternated, tokens/s as median (min..max) of {a.repeats} "
                  "repeats.", "",
                  "| B | generator eager | generator graph | seeds eager | seeds graph | "
                  "seeds graph vs generator graph | seeds graph == seeds eager |",
                  "|---|---|---|---|---|---|---|"]
        for r in erows:
            t = r["tok_per_s"]
            lines.append(
                f"| {r['B']} | " + " | ".join(cell(t[n], ".0f") for n in
                                              ("generator eager", "generator graph",
                                               "seeds eager", "seeds graph"))
                + f" | {t['seeds graph']['median'] / t['generator graph']['median']:.2f}x"
                + f" | {r['seeds_graph_equals_eager']} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
