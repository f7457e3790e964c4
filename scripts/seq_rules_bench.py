#!/usr/bin/env python
"""Sequence rules: the kernels (ops/csrc/seq_rules.hip through ``rf.seq_ban`` and
``rf.stop_check``) against their plain-torch references, what ``GPT2Engine(...,
sequence_rules=True)`` costs end to end, and how often greedy requests still loop.

    python scripts/seq_rules_bench.py [--out profiles/r19/seq_rules.md]

Kernel part: ``seq_ban`` on V = 50257 bf16 logits (randn x 4) as the [:, :V] view of a
[B, 50304] buffer, B 1 / 8 / 64 / 576 (576 = 64 slots x 9 window rows of a speculative step),
every row with its own context of 128 or 1000 tokens (half prompt, half output, ids drawn from
64 values so that n-grams do repeat; tables 1024 wide), ``ngram`` 3 and four banned sequences
of 1, 2, 4 and 8 tokens, the first three taken from the end of the row's context.
``stop_check`` on the same rows' outputs with a span of 1 and of 9 new tokens and four stop
sequences per row. ``hip`` is one call of the kernel, ``torch`` the reference
(``ref.seq_ban``: gathers over the [B, P + cap] context and a scatter into a [B, V] mask;
``ref.stop_check``: gathers over [R, cap, 8]): the same results, checked first. 20 calls of
one path captured in one HIP graph and replayed, device events around blocks of replays, a
warm-up and at least ``--seconds`` of timed work per path and repeat, the paths alternated,
median (min..max) of ``--repeats``, microseconds per call. (``stop_check`` rewrites its own
inputs: ``pos`` is reset by a copy inside the graph, on both paths.)

Engine part: GPT-2 small, bf16, the request mix of scripts/gpt2_engine_bench.py
(``--requests`` seeded requests, prompts 16..128, ``max_new_tokens`` uniform in 16..256,
temperature 0.8, top-k 50, all queued at t0) at S 8 and S 64 with ``poll_every`` 8:
``sequence_rules=False``, on with no request naming a rule, on with
``no_repeat_ngram_size=3`` and one stop sequence on every request, and the last two with
``speculate=4``. Engines built once outside the timed window, wall time around synchronised
runs, the paths alternated, median (min..max) of ``--repeats`` after one warm-up run.

Loops: the greedy requests of scripts/logit_process_bench.py (64 prompts, each followed by 64
tokens of its own greedy continuation, 256 new tokens, temperature 0): the share of requests
whose output ends in a repeated cycle (its last 32 tokens have a period <= 16), without a
rule and with ``no_repeat_ngram_size=3``.

``--repo PATH`` imports ``ray_amd`` from another checkout and ``--engine-json FILE`` dumps the
engine rows: with ``--cases none`` that measures the engine without the argument on another
commit, and ``--parent-json FILE`` puts such rows beside this commit's in the write-up."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "r19", "seq_rules.md"))
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
ap.add_argument("--resources", help="the kernels' VGPR / scratch / LDS line, for the write-up")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.repo))

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402
from ray_amd.ops import reference as ref  # noqa: E402

V, VPAD, WIDTH = 50257, 50304, 1024
BATCHES = (1, 8, 64, 576)
CONTEXTS = (128, 1000)
GRAPH_CALLS = 20
RULES = {"no_repeat_ngram_size": 3, "stop": [[11, 12]]}


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
    i32, Q, ML = torch.int32, rf.SEQ_MAX, rf.SEQ_MAX_LEN
    for B in BATCHES:
        for ctx in CONTEXTS:
            g = torch.Generator().manual_seed(B * 7 + ctx)
            x = (torch.randn(B, V, generator=g) * 4).bfloat16()
            pl, no = ctx // 2, ctx - ctx // 2
            prompt = (torch.randint(0, 64, (B, WIDTH), generator=g) * 700).to(i32)
            out = torch.randint(0, 64, (B, WIDTH), generator=g) * 700
            bad = torch.randint(0, V, (B, Q, ML), generator=g).to(i32)
            bad_len = torch.zeros(B, Q, dtype=i32)
            for q, L in enumerate((1, 2, 4, 8)):
                bad_len[:, q] = L
                if L in (2, 4):  # the context's own end, then some token
                    bad[:, q, : L - 1] = out[:, no - (L - 1): no].to(i32)
            tables = [t.to(dev) for t in (
                prompt, torch.full((B,), pl, dtype=i32), out, torch.full((B,), no, dtype=i32),
                bad, bad_len, torch.full((B,), 3, dtype=i32))]
            bufs = {}
            for name in ("hip", "torch"):
                buf = torch.zeros(B, VPAD, dtype=torch.bfloat16)
                buf[:, :V] = x
                bufs[name] = buf.to(dev)[:, :V]
            paths = {"hip": lambda: rf.seq_ban(bufs["hip"], *tables),
                     "torch": lambda: ref.seq_ban(bufs["torch"], *tables)}
            # same results first: faster and different is not faster
            paths["hip"](), paths["torch"]()
            rec = {"op": "seq_ban", "B": B, "context": ctx,
                   "equal": bool(torch.equal(bufs["hip"].view(torch.int16),
                                             bufs["torch"].view(torch.int16))),
                   "edited": int((bufs["hip"].cpu() != x).sum())}
            rec["device_us"] = time_graphed(paths, a.seconds, a.repeats)
            rec["speedup"] = rec["device_us"]["torch"]["median"] / rec["device_us"]["hip"]["median"]
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            for span in (1, 9):
                stops = torch.randint(0, 64, (B, Q, ML), generator=g).to(i32) * 700
                stop_len = torch.zeros(B, Q, dtype=i32)
                stop_len[:, :4] = torch.tensor([1, 2, 4, 8], dtype=i32)
                n_out0 = tables[3]
                pos0 = (n_out0 - span).clamp(min=0)
                st = {}
                for name in ("hip", "torch"):
                    st[name] = dict(n_out=n_out0.clone(), pos=pos0.clone(),
                                    hit=torch.full((B,), -1, dtype=i32, device=dev),
                                    active=torch.ones(B, dtype=torch.uint8, device=dev),
                                    lens=torch.zeros(B, dtype=i32, device=dev))
                stops, stop_len = stops.to(dev), stop_len.to(dev)

                def run(fn, s):
                    s["n_out"].copy_(n_out0), s["pos"].copy_(pos0)  # a call rewrites them
                    fn(tables[2], s["n_out"], s["pos"], stops, stop_len, s["hit"],
                       active=s["active"], lens=s["lens"])

                paths = {"hip": lambda: run(rf.stop_check, st["hip"]),
                         "torch": lambda: run(ref.stop_check, st["torch"])}
                paths["hip"](), paths["torch"]()
                rec = {"op": "stop_check", "B": B, "context": ctx, "span": span,
                       "equal": all(torch.equal(st["hip"][k], st["torch"][k]) for k in st["hip"]),
                       "edited": int((st["hip"]["hit"] >= 0).sum())}
                rec["device_us"] = time_graphed(paths, a.seconds, a.repeats)
                rec["speedup"] = rec["device_us"]["torch"]["median"] / \
                    rec["device_us"]["hip"]["median"]
                print(json.dumps(rec), flush=True)
                rows.append(rec)
    return rows


def make_requests(n, vocab):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(16, 129, (n,), generator=g).tolist()
    new = torch.randint(16, 257, (n,), generator=g).tolist()
    return [{"tokens": torch.randint(0, vocab, (L,), generator=g).tolist(), "new": m, "seed": i}
            for i, (L, m) in enumerate(zip(lens, new))]


def run_engine(eng, reqs, rules, temperature=0.8, top_k=50):
    steps0 = eng.steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [eng.submit(r["tokens"], r["new"], temperature=temperature, top_k=top_k,
                       seed=r["seed"], **rules) for r in reqs]
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
        on = {"sequence_rules": True, "eos_token_id": 50256}
        off = {"eos_token_id": 50256}
        cases = [("sequence_rules=False", off, {}),
                 ("on, no request names a rule", on, {}),
                 ("on, no_repeat_ngram_size=3 + one stop", on, RULES),
                 ("speculate=4", dict(off, speculate=4), {}),
                 ("speculate=4, on, no request names a rule", dict(on, speculate=4), {}),
                 ("speculate=4, on, no_repeat_ngram_size=3 + one stop", dict(on, speculate=4),
                  RULES)]
    rows = []
    for S in (8, 64):
        paths = {}
        for name, kw, rules in cases:
            eng = GPT2Engine(model, slots=S, max_len=max_len, poll_every=8, **kw)
            paths[name] = lambda eng=eng, rules=rules: run_engine(eng, reqs, rules)
        first = {n: fn() for n, fn in paths.items()}  # warm-up
        runs = {n: [] for n in paths}
        for _ in range(a.repeats):
            for n, fn in paths.items():
                runs[n].append(fn())
        for n, rs in runs.items():
            # the engine without rules at the same ``speculate``
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
    eng = GPT2Engine(model, slots=64, max_len=max_len, sequence_rules=True)
    rec = {"requests": len(reqs)}
    for name, rules in (("plain", {}), ("no_repeat_ngram_size=3", {"no_repeat_ngram_size": 3})):
        toks = run_engine(eng, reqs, rules, temperature=0.0, top_k=None)["tokens"]
        rec[name] = sum(ends_in_cycle(t) for t in toks)
    print(json.dumps(rec), flush=True)
    return rec


def cell(s, fmt=".1f"):
    return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("seq_rules_bench needs a GPU: timings are device timings")
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

    lines = ["# Sequence rules: stop sequences, banned sequences, no-repeat n-grams", "",
             f"`scripts/seq_rules_bench.py` on {torch.cuda.get_device_name(0)}.", ""]
    if a.resources:
        lines += ["## The kernels' resources", "", a.resources, ""]
    if krows:
        lines += [f"## One call, V = {V} bf16 (a view of a [B, {VPAD}] buffer)", "",
                  f"Every row with its own context of `context` tokens (half prompt, half output, "
                  f"ids from 64 values, tables {WIDTH} wide), `ngram` 3, banned sequences of 1, 2, "
                  f"4 and 8 tokens; `stop_check` with stops of 1, 2, 4 and 8 tokens over `span` "
                  f"new tokens. {GRAPH_CALLS} calls of one path captured in one HIP graph and "
                  f"replayed, device events, the paths alternated, >= {a.seconds:g} s of timed "
                  f"work per path and repeat, median (min..max) of {a.repeats} repeats, "
                  "microseconds per call. `torch`: the reference of ops/reference.py. `edited`: "
                  "logits the first call banned, or rows it stopped.", "",
                  "| op | B | context | span | hip device us | torch device us | torch / hip | "
                  "equal | edited |", "|---|---|---|---|---|---|---|---|---|"]
        for r in krows:
            dv = r["device_us"]
            lines.append(f"| {r['op']} | {r['B']} | {r['context']} | {r.get('span', '')} | "
                         f"{cell(dv['hip'], '.2f')} | {cell(dv['torch'])} | {r['speedup']:.1f}x | "
                         f"{r['equal']} | {r['edited']} |")
    if erows:
        lines += ["", "## Engine, GPT-2 small bf16, poll_every 8", "",
                  f"{a.requests} requests (prompts 16..128, max_new_tokens uniform in 16..256, "
                  f"{erows[0]['requested_tokens']} requested tokens, temperature 0.8, top-k 50, a "
                  "seed each), all queued at t0. Wall time around synchronised runs, the paths "
                  f"alternated, median (min..max) of {a.repeats} repeats after one warm-up run. "
                  "`same tokens`: share of requests whose tokens equal those of the engine "
                  "without rules at the same `speculate`. `parent commit`: this script with "
                  "`--repo` on a checkout of the parent and `--cases none`, in processes of "
                  "their own.",
                  "", "| S | path | requested tokens/s | vs off | device steps | same tokens | "
                  "repeatable |", "|---|---|---|---|---|---|---|"]
        for r in prows:
            lines.append(f"| {r['S']} | {r['path']} | {cell(r['tok_per_s'], '.0f')} | | "
                         f"{r['steps']} | | {r['repeatable']} |")
        for r in erows:
            base = next(x for x in erows if x["S"] == r["S"]
                        and x["path"] == "sequence_rules=False")
            lines.append(f"| {r['S']} | {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{r['tok_per_s']['median'] / base['tok_per_s']['median']:.3f}x | "
                         f"{r['steps']} | {r['same_tokens']:.2f} | {r['repeatable']} |")
    if loops:
        lines += ["", "## Greedy loops", "",
                  f"{loops['requests']} greedy requests (the prompts of "
                  "scripts/logit_process_bench.py: a random prompt followed by 64 tokens of its own "
                  "greedy continuation, 256 new tokens). Requests whose output ends in a repeated "
                  f"cycle (the last 32 tokens have a period <= 16): {loops['plain']} without a "
                  f"rule, {loops['no_repeat_ngram_size=3']} with `no_repeat_ngram_size=3`. Counts "
                  "on random-init weights, not a statement about real text."]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
