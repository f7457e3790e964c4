#!/usr/bin/env python
"""GPT-2 decoding: the HIP decode-attention kernel (ops/csrc/attn_decode.hip through
``rf.attn_decode``) against SDPA on the same cache, and ``GPT2.generate`` (KV cache, eager
and graph) against the recompute loop through ``forward(idx)``.

    python scripts/gpt2_decode_bench.py [--out profiles/r8/gpt2_decode.md]

Kernel part: GPT-2-small heads (H = 12, D = 64), every row holding Tcache positions.
``hip`` is one ``rf.attn_decode`` call (append + attention, automatic split count);
``sdpa`` appends with ``index_copy_`` and calls ``scaled_dot_product_attention`` on the
cache, whose capacity is exactly the Tcache + 1 valid positions (the host knows the
length here, which spares the baseline a mask); ``reference`` is ``ref.attn_decode`` on the
GPU. Device events around alternating blocks of the paths in one process, a warm-up and at
least ``--seconds`` of timed work per path and repeat, median (min..max) of ``--repeats``;
once as eager calls (host launch work included) and once as 20 calls captured in one HIP
graph and replayed (device time).

End-to-end part: GPT-2 small, bf16, a 128-token prompt and 128 new tokens, greedy; wall
time around a synchronised call, the three paths alternated, median of ``--repeats``.
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
from ray_amd.ops import reference as ref  # noqa: E402

H, D = 12, 64
SHAPES = [(1, 1023), (8, 1023), (64, 1023), (64, 127)]
SWEEP = (1, 2, 4, 8, 16, 32)


def make_inputs(B, Tc, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3, H, D, generator=g).bfloat16().to(dev)
    kc = torch.randn(B, H, Tc + 1, D, generator=g).bfloat16().to(dev)
    vc = torch.randn(B, H, Tc + 1, D, generator=g).bfloat16().to(dev)
    lens = torch.full((B,), Tc, dtype=torch.int32, device=dev)
    return qkv, kc, vc, lens


def sdpa_on_cache(qkv, kc, vc, lens, pos):
    kc.index_copy_(2, pos, qkv[:, 1].unsqueeze(2))
    vc.index_copy_(2, pos, qkv[:, 2].unsqueeze(2))
    return F.scaled_dot_product_attention(qkv[:, 0].unsqueeze(2), kc, vc).squeeze(2)


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


GRAPH_CALLS = 20


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


def kernel_part(a, dev):
    rows = []
    L = _lib.lib()
    for B, Tc in SHAPES:
        qkv, kc, vc, lens = make_inputs(B, Tc, dev)
        pos = torch.tensor([Tc], device=dev)
        paths = {
            "hip": lambda: rf.attn_decode(qkv, kc, vc, lens),
            "sdpa": lambda: sdpa_on_cache(qkv, kc, vc, lens, pos),
            "reference": lambda: ref.attn_decode(qkv, kc, vc, lens),
        }
        # same results first: faster and different is not faster
        o = {n: fn().float() for n, fn in paths.items()}
        diff = float((o["hip"] - o["sdpa"]).abs().max())
        rec = {"B": B, "Tcache": Tc, "splits": L.ra_attn_decode_splits(B, H, Tc + 1),
               "max_abs_diff_vs_sdpa": diff, "us": time_paths(paths, a.seconds, a.repeats)}
        fast = {n: paths[n] for n in ("hip", "sdpa")}
        rec["device_us"] = time_paths(fast, a.seconds, a.repeats, in_graph=True)
        kv_bytes = 2 * B * H * (Tc + 1) * D * 2
        rec["hip_GBps"] = kv_bytes / rec["device_us"]["hip"]["median"] * 1e-3
        rec["speedup_median"] = rec["us"]["sdpa"]["median"] / rec["us"]["hip"]["median"]
        rec["device_speedup_median"] = (rec["device_us"]["sdpa"]["median"]
                                        / rec["device_us"]["hip"]["median"])
        if a.sweep:
            sw = {f"S{s}": (lambda s=s: rf.attn_decode(qkv, kc, vc, lens, splits=s))
                  for s in SWEEP if s <= (Tc + 32) // 32}
            rec["sweep_us"] = {n: v["median"] for n, v in
                               time_paths(sw, a.seconds / 4, a.repeats, in_graph=True).items()}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def recompute(model, idx, new):
    seq = idx
    with torch.no_grad():
        for _ in range(new):
            nxt = model(seq)[:, -1].argmax(-1)
            seq = torch.cat([seq, nxt[:, None]], 1)
    return seq[:, idx.shape[1]:]


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
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        idx = torch.randint(0, model.cfg.vocab_size, (B, a.prompt), generator=g).to(dev)
        paths = {"eager": lambda: model.generate(idx, a.new),
                 "recompute": lambda: recompute(model, idx, a.new)}
        if a.graph:
            paths["graph"] = lambda: model.generate(idx, a.new, graph=True)
        outs = {n: wall(fn)[1] for n, fn in paths.items()}  # warm-up
        times = {n: [] for n in paths}
        for _ in range(a.repeats):
            for n, fn in paths.items():
                times[n].append(wall(fn)[0])
        rec = {"B": B, "prompt": a.prompt, "new": a.new,
               "graph_equals_eager": bool(torch.equal(outs["eager"], outs["graph"]))
               if a.graph else None,
               "tokens_equal_recompute": float((outs["eager"] == outs["recompute"]).float().mean()),
               "tok_per_s": {n: stats([B * a.new / x for x in t]) for n, t in times.items()}}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r8", "gpt2_decode.md"))
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="also time explicit split counts")
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--no-graph", dest="graph", action="store_false")
    ap.add_argument("--no-e2e", dest="e2e", action="store_false")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpt2_decode_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    krows = kernel_part(a, dev)
    erows = e2e_part(a, dev) if a.e2e else []

    def cell(s, fmt=".1f"):
        return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"

    lines = ["# GPT-2 decoding: HIP decode attention and KV-cache generation", "",
             f"`scripts/gpt2_decode_bench.py` on {torch.cuda.get_device_name(0)}.", "",
             "## Decode attention, one call (H = 12, D = 64, bf16)", "",
             f"Device events, the paths alternated in one process, >= {a.seconds:g} s of timed "
             f"work per path and repeat, median (min..max) of {a.repeats} repeats, microseconds "
             "per call (append + attention). `call`: eager calls from Python, host launch work "
             f"included; `device`: {GRAPH_CALLS} calls captured in one HIP graph and replayed, "
             "per call. GB/s: K/V bytes of the valid positions over the hip device median.", "",
             "| B | Tcache | splits | hip call us | sdpa-on-cache call us | reference call us | "
             "hip vs sdpa (call) | hip device us | sdpa device us | hip vs sdpa (device) | "
             "hip GB/s | max abs diff |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in krows:
        u, dv = r["us"], r["device_us"]
        lines.append(f"| {r['B']} | {r['Tcache']} | {r['splits']} | {cell(u['hip'])} | "
                     f"{cell(u['sdpa'])} | {cell(u['reference'])} | {r['speedup_median']:.2f}x | "
                     f"{cell(dv['hip'], '.2f')} | {cell(dv['sdpa'], '.2f')} | "
                     f"{r['device_speedup_median']:.2f}x | "
                     f"{r['hip_GBps']:.0f} | {r['max_abs_diff_vs_sdpa']:.1e} |")
    if a.sweep:
        lines += ["", "Explicit split counts, hip device median us (graph replay):", ""]
        for r in krows:
            lines.append(f"- B={r['B']} Tcache={r['Tcache']} (automatic: {r['splits']}): " +
                         ", ".join(f"{k}={v:.2f}" for k, v in r["sweep_us"].items()))
    if erows:
        lines += ["", "## generate, GPT-2 small bf16, greedy", "",
                  f"{a.prompt}-token prompt, {a.new} new tokens; wall time around a synchronised "
                  f"call, paths alternated, tokens/s as median (min..max) of {a.repeats} repeats. "
                  "`recompute` is the loop through `forward(idx)`. `same tokens`: share of "
                  "positions where the cached path and the recompute loop agree (bf16, random "
                  "weights: near-ties can flip).", "",
                  "| B | eager tok/s | graph tok/s | recompute tok/s | eager vs recompute | "
                  "graph vs recompute | graph == eager | same tokens |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in erows:
            t = r["tok_per_s"]
            gr = t.get("graph")
            lines.append(
                f"| {r['B']} | {cell(t['eager'], '.0f')} | "
                f"{cell(gr, '.0f') if gr else 'n/a'} | {cell(t['recompute'], '.0f')} | "
                f"{t['eager']['median'] / t['recompute']['median']:.2f}x | "
                + (f"{gr['median'] / t['recompute']['median']:.2f}x" if gr else "n/a")
                + f" | {r['graph_equals_eager']} | {r['tokens_equal_recompute']:.2f} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
