#!/usr/bin/env python
"""Per-token log-probabilities: the kernel (ops/csrc/logprobs.hip through
``rf.token_logprobs``) against the usual torch composition, and what ``GPT2Engine(...,
logprobs=N)`` costs end to end.

    python scripts/logprobs_bench.py [--out profiles/r16/logprobs.md]

Kernel part: V = 50257 bf16 logits (randn x 4) as the [:, :V] view of a [B, 50304] buffer,
B 1 / 8 / 64 / 576 (576 = 64 slots x 9 window rows of a speculative step), top_n 0 / 5 / 8.
``hip`` is one ``rf.token_logprobs`` call, ``torch`` the composition ``log_softmax`` in fp32,
``gather`` and ``topk``: a timing baseline only, its tie order is not the reference's. 20
calls of one path captured in one HIP graph and replayed, device events around blocks of
replays, a warm-up and at least ``--seconds`` of timed work per path and repeat, the paths
alternated, median (min..max) of ``--repeats``, microseconds per call.

Engine part: GPT-2 small, bf16, the request mix of scripts/gpt2_engine_bench.py
(``--requests`` seeded requests, prompts 16..128, ``max_new_tokens`` uniform in 16..256,
temperature 0.8, top-k 50, all queued at t0) at S 8 and S 64 with ``poll_every`` 8:
``logprobs=None``, ``logprobs=0``, ``logprobs=5`` (every request asking for 5) and
``speculate=4`` without and with ``logprobs=5``. Engines built once outside the timed
window, wall time around synchronised runs, the paths alternated, median (min..max) of
``--repeats`` after one warm-up run.

``--repo PATH`` imports ``ray_amd`` from another checkout and ``--engine-json FILE`` dumps the
engine rows: with ``--cases none`` that measures ``logprobs=None`` on another commit, and
``--parent-json FILE`` puts such rows beside this commit's in the write-up."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "r16", "logprobs.md"))
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--requests", type=int, default=256)
ap.add_argument("--cases", default="all", choices=["all", "none"])
ap.add_argument("--no-kernel", dest="kernel", action="store_false")
ap.add_argument("--no-engine", dest="engine", action="store_false")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--engine-json")
ap.add_argument("--parent-json")
ap.add_argument("--worst-error", help="the GPU test's worst observed error, for the write-up")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.repo))

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402

V, VPAD = 50257, 50304
BATCHES = (1, 8, 64, 576)
TOPS = (0, 5, 8)
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


def torch_composition(logits, tok, n):
    lsm = torch.log_softmax(logits.float(), -1)
    lp = lsm.gather(1, tok.unsqueeze(1)).squeeze(1)
    if not n:
        return lp, None, None
    top = lsm.topk(n, -1)
    return lp, top.indices, top.values


def kernel_part(a, dev):
    rows = []
    for B in BATCHES:
        g = torch.Generator().manual_seed(B)
        buf = torch.zeros(B, VPAD, dtype=torch.bfloat16)
        buf[:, :V] = (torch.randn(B, V, generator=g) * 4).bfloat16()
        lg = buf.to(dev)[:, :V]
        tok = torch.randint(0, V, (B,), generator=g).to(dev)
        for n in TOPS:
            paths = {"hip": lambda: rf.token_logprobs(lg, tok, n),
                     "torch": lambda: torch_composition(lg, tok, n)}
            # same results first: faster and different is not faster
            h, t = paths["hip"](), paths["torch"]()
            rec = {"B": B, "top_n": n,
                   "max_abs_diff": float((h[0] - t[0]).abs().max()),
                   "ids_equal_topk": 1.0 if not n else
                   float((h[1].long() == t[1]).float().mean())}
            rec["device_us"] = time_graphed(paths, a.seconds, a.repeats)
            rec["speedup"] = rec["device_us"]["torch"]["median"] / rec["device_us"]["hip"]["median"]
            # the row is read twice, the second time from L2: HBM traffic is one read
            rec["hip_GBps"] = B * V * 2 / rec["device_us"]["hip"]["median"] * 1e-3
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    return rows


def make_requests(n, vocab):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(16, 129, (n,), generator=g).tolist()
    new = torch.randint(16, 257, (n,), generator=g).tolist()
    return [{"tokens": torch.randint(0, vocab, (L,), generator=g).tolist(), "new": m, "seed": i}
            for i, (L, m) in enumerate(zip(lens, new))]


def run_engine(eng, reqs, want):
    steps0 = eng.steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kw = {} if want is None else {"logprobs": want}
    rids = [eng.submit(r["tokens"], r["new"], temperature=0.8, top_k=50, seed=r["seed"], **kw)
            for r in reqs]
    got, n_lp = {}, 0
    while eng.has_work():
        for ev in eng.step():
            got.setdefault(ev[0], []).extend(ev[1])
            if want is not None:
                n_lp += len(ev[3]["logprobs"])
    torch.cuda.synchronize()
    return {"wall": time.perf_counter() - t0, "tokens": [got[r] for r in rids],
            "steps": eng.steps - steps0, "n_lp": n_lp}


def engine_part(a, dev):
    torch.manual_seed(0)
    model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    reqs = make_requests(a.requests, model.cfg.vocab_size)
    requested = sum(r["new"] for r in reqs)
    max_len = max(len(r["tokens"]) for r in reqs) + max(r["new"] for r in reqs)
    cases = [("logprobs=None", {}, None)]
    if a.cases == "all":
        cases += [("logprobs=0", {"logprobs": 0}, 0), ("logprobs=5", {"logprobs": 5}, 5),
                  ("speculate=4", {"speculate": 4}, None),
                  ("speculate=4 logprobs=5", {"speculate": 4, "logprobs": 5}, 5)]
    rows = []
    for S in (8, 64):
        paths = {}
        for name, kw, want in cases:
            eng = GPT2Engine(model, slots=S, max_len=max_len, poll_every=8, **kw)
            paths[name] = lambda eng=eng, want=want: run_engine(eng, reqs, want)
        first = {n: fn() for n, fn in paths.items()}  # warm-up
        runs = {n: [] for n in paths}
        for _ in range(a.repeats):
            for n, fn in paths.items():
                runs[n].append(fn())
        for n, rs in runs.items():
            ref_name = "speculate=4" if n.startswith("speculate") else "logprobs=None"
            rec = {"S": S, "path": n, "requested_tokens": requested,
                   "tok_per_s": stats([requested / r["wall"] for r in rs]),
                   "steps": rs[0]["steps"], "logprob_entries": rs[0]["n_lp"],
                   "same_tokens": sum(x == y for x, y in zip(first[n]["tokens"],
                                                             first[ref_name]["tokens"]))
                   / len(reqs),
                   "repeatable": all(r["tokens"] == first[n]["tokens"] for r in rs)}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
        del paths
        torch.cuda.empty_cache()
    return rows


def cell(s, fmt=".1f"):
    return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("logprobs_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    krows = kernel_part(a, dev) if a.kernel and a.cases == "all" else []
    torch.cuda.empty_cache()
    erows = engine_part(a, dev) if a.engine else []
    if a.engine_json:
        os.makedirs(os.path.dirname(a.engine_json) or ".", exist_ok=True)
        with open(a.engine_json, "w") as fh:
            json.dump(erows, fh)
    if a.cases != "all":
        return
    prows = []
    if a.parent_json:
        with open(a.parent_json) as fh:
            prows = json.load(fh)

    lines = ["# Per-token log-probabilities", "",
             f"`scripts/logprobs_bench.py` on {torch.cuda.get_device_name(0)}.", ""]
    if a.worst_error:
        lines += ["## Accuracy", "",
                  "`tests/test_logprobs_gpu.py`, kernel against `ref.token_logprobs` in fp64 on the "
                  "stored bf16 values (V 1..50257, B 1 / 5 / 67, three layouts, ties in the top 8): "
                  f"ids exact, worst observed value error {a.worst_error}.", ""]
    if krows:
        lines += [f"## One call, V = {V} bf16 (a view of a [B, {VPAD}] buffer)", "",
                  f"{GRAPH_CALLS} calls of one path captured in one HIP graph and replayed, device "
                  f"events, the paths alternated, >= {a.seconds:g} s of timed work per path and "
                  f"repeat, median (min..max) of {a.repeats} repeats, microseconds per call. "
                  "`torch`: `log_softmax` in fp32, `gather`, `topk` (a timing baseline: its tie "
                  "order is not the reference's; `ids = topk`: share of top ids where the two "
                  "agree). GB/s: one read of the rows over the hip median.", "",
                  "| B | top_n | hip device us | torch device us | torch / hip | hip GB/s | "
                  "max abs diff of lp | ids = topk |", "|---|---|---|---|---|---|---|---|"]
        for r in krows:
            dv = r["device_us"]
            lines.append(f"| {r['B']} | {r['top_n']} | {cell(dv['hip'], '.2f')} | "
                         f"{cell(dv['torch'])} | {r['speedup']:.1f}x | {r['hip_GBps']:.0f} | "
                         f"{r['max_abs_diff']:.2e} | {r['ids_equal_topk']:.4f} |")
    if erows:
        lines += ["", "## Engine, GPT-2 small bf16, poll_every 8", "",
                  f"{a.requests} requests (prompts 16..128, max_new_tokens uniform in 16..256, "
                  f"{erows[0]['requested_tokens']} requested tokens, temperature 0.8, top-k 50, a "
                  "seed each), all queued at t0. Wall time around synchronised runs, the paths "
                  f"alternated, median (min..max) of {a.repeats} repeats after one warm-up run. "
                  "`same tokens`: share of requests whose tokens equal those of the engine "
                  "without logprobs (of `speculate=4` for the speculative rows). `parent commit`: "
                  "this script with `--repo` on a checkout of the parent, in a run of its own.",
                  "", "| S | path | requested tokens/s | vs logprobs=None | device steps | "
                  "logprob entries | same tokens | repeatable |", "|---|---|---|---|---|---|---|---|"]
        for r in prows:
            lines.append(f"| {r['S']} | parent commit | {cell(r['tok_per_s'], '.0f')} | | "
                         f"{r['steps']} | | | {r['repeatable']} |")
        for r in erows:
            base = next(x for x in erows if x["S"] == r["S"] and x["path"] == "logprobs=None")
            lines.append(f"| {r['S']} | {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{r['tok_per_s']['median'] / base['tok_per_s']['median']:.3f}x | "
                         f"{r['steps']} | {r['logprob_entries']} | {r['same_tokens']:.2f} | "
                         f"{r['repeatable']} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
