#!/usr/bin/env python
"""Grammar-constrained decoding: the kernels (ops/csrc/grammar.hip through ``rf.grammar_mask``
and ``rf.grammar_advance``) against a plain-torch composition, the chunk size of the mask
kernel, and what ``GPT2Engine(..., grammar_states=N)`` costs end to end.

    python scripts/grammar_bench.py [--out profiles/r18/grammar.md]

Kernel part: V = 50257 bf16 logits (randn x 4) as the [:, :V] view of a [B, 50304] buffer,
B 1 / 8 / 64 / 576 (576 = 64 slots x 9 window rows of a speculative step at ``speculate=8``),
a table of 64 states whose rows allow a ``sparse`` (0.1 %) or a ``nearly full`` (99 %) set of
tokens, every row in a state of its own. ``hip`` is one ``rf.grammar_mask`` call, ``torch``
the composition ``logits.masked_fill_(table[state][:, :V] < 0, -inf)``: the same bits, checked
first. 20 calls of one path captured in one HIP graph and replayed, device events around
blocks of replays, a warm-up and at least ``--seconds`` of timed work per path and repeat,
the paths alternated, median (min..max) of ``--repeats``, microseconds per call. The chunk
sweep runs the same call with ``chunk=`` 256 .. 8192 slots per workgroup and 0, the
launcher's rule. ``rf.grammar_advance`` is timed the same way at R 64 and 576 context rows
with ``max_steps`` 1 and 9.

Engine part: GPT-2 small, bf16, the request mix of scripts/gpt2_engine_bench.py
(``--requests`` seeded requests, prompts 16..128, ``max_new_tokens`` uniform in 16..256,
temperature 0.8, top-k 50, all queued at t0) at S 8 and S 64 with ``poll_every`` 8 and an
``eos_token_id``: ``grammar_states=0``, the pool on with no request using it, and every
request under a regex grammar over a synthetic byte vocabulary (256 single bytes, then
two- to four-letter strings), and the same three under ``speculate=4``. Engines built once
outside the timed window, wall time around synchronised runs, the paths alternated, median
(min..max) of ``--repeats`` after one warm-up run; the rate counts EMITTED tokens, since a
grammar ends a request where its word ends.

``--repo PATH`` imports ``ray_amd`` from another checkout and ``--engine-json FILE`` dumps the
engine rows: with ``--cases none`` that measures the engine without the argument on another
commit, and ``--parent-json FILE`` puts such rows beside this commit's in the write-up."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "r18", "grammar.md"))
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--requests", type=int, default=256)
ap.add_argument("--cases", default="all", choices=["all", "none"])
ap.add_argument("--no-kernel", dest="kernel", action="store_false")
ap.add_argument("--no-engine", dest="engine", action="store_false")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--engine-json")
ap.add_argument("--kernel-json")
ap.add_argument("--parent-json", action="append", default=[])
ap.add_argument("--resources", help="the kernels' VGPR / scratch line, for the write-up")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.repo))

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402

V, VPAD, VT, N_STATES = 50257, 50304, 50264, 64
BATCHES = (1, 8, 64, 576)
DENSITIES = (("sparse", 0.001), ("nearly full", 0.99))
CHUNKS = (0, 256, 512, 1024, 2048, 8192)
GRAPH_CALLS = 20
EOS = 50256
# at least 41 words of 2..4-letter tokens: most requests are cut by max_new_tokens, so the
# constrained paths emit about what the others do
PATTERN = r"([a-z]{1,8} ){40,64}[a-z]{1,8}\."


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


def make_table(p, g):
    nxt = torch.randint(0, N_STATES, (N_STATES, VT), generator=g)
    allowed = torch.rand(N_STATES, VT, generator=g) < p
    t = torch.where(allowed, nxt, torch.full_like(nxt, -1)).to(torch.int16)
    t[:, V:] = -1
    return t


def kernel_part(a, dev):
    mask_rows, chunk_rows, adv_rows = [], [], []
    ninf = float("-inf")
    for B in BATCHES:
        for dname, p in DENSITIES:
            g = torch.Generator().manual_seed(B * 7 + int(p * 1000))
            x = (torch.randn(B, V, generator=g) * 4).bfloat16()
            table = make_table(p, g).to(dev)
            state = torch.randint(0, N_STATES, (B,), generator=g).to(torch.int32).to(dev)
            bufs = {}
            for name in ("hip", "torch"):
                buf = torch.zeros(B, VPAD, dtype=torch.bfloat16)
                buf[:, :V] = x
                bufs[name] = buf.to(dev)[:, :V]
            paths = {"hip": lambda: rf.grammar_mask(bufs["hip"], table, state),
                     "torch": lambda: bufs["torch"].masked_fill_(
                         table[state.long()][:, :V] < 0, ninf)}
            # same results first: faster and different is not faster
            paths["hip"](), paths["torch"]()
            rec = {"B": B, "allowed": dname,
                   "bit_equal": bool(torch.equal(bufs["hip"].view(torch.int16),
                                                 bufs["torch"].view(torch.int16))),
                   "banned": int((bufs["hip"].cpu().view(torch.int16) != x.view(torch.int16))
                                 .sum())}
            rec["device_us"] = time_graphed(paths, a.seconds, a.repeats)
            rec["speedup"] = rec["device_us"]["torch"]["median"] / rec["device_us"]["hip"]["median"]
            print(json.dumps(rec), flush=True)
            mask_rows.append(rec)
            sweep = {f"chunk {c}": (lambda c=c: rf.grammar_mask(bufs["hip"], table, state,
                                                                chunk=c)) for c in CHUNKS}
            rec = {"B": B, "allowed": dname, "auto": _lib.lib().ra_grammar_mask_chunk(B, V),
                   "device_us": time_graphed(sweep, a.seconds / 2, a.repeats)}
            print(json.dumps(rec), flush=True)
            chunk_rows.append(rec)
    for R in (64, 576):
        g = torch.Generator().manual_seed(R)
        table = make_table(0.99, g).to(dev)
        out = torch.randint(0, V, (R, 256), generator=g).to(dev)
        n_out = torch.full((R,), 200, dtype=torch.int32, device=dev)
        state0 = torch.randint(0, N_STATES, (R,), generator=g).to(torch.int32).to(dev)
        state, pos = state0.clone(), torch.zeros(R, dtype=torch.int32, device=dev)
        for steps in (1, 9):
            def fn(steps=steps):
                # (each call starts from the same rows: the walk is the timed work)
                state.copy_(state0)
                pos.zero_()
                rf.grammar_advance(state, pos, out, n_out, table, steps)

            def reset():
                state.copy_(state0)
                pos.zero_()

            t = time_graphed({"advance": fn, "reset only": reset}, a.seconds / 2, a.repeats)
            rec = {"R": R, "max_steps": steps, "device_us": t}
            print(json.dumps(rec), flush=True)
            adv_rows.append(rec)
    return {"mask": mask_rows, "chunk": chunk_rows, "advance": adv_rows}


def byte_vocab(g):
    """50257 entries: the 256 single bytes, lower-case strings of 2..4 letters, EOS last."""
    words = [bytes(torch.randint(97, 123, (int(n),), generator=g).tolist())
             for n in torch.randint(2, 5, (V - 257,), generator=g)]
    return [bytes([i]) for i in range(256)] + words + [b""]


def make_requests(n, vocab):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(16, 129, (n,), generator=g).tolist()
    new = torch.randint(16, 257, (n,), generator=g).tolist()
    return [{"tokens": torch.randint(0, vocab, (L,), generator=g).tolist(), "new": m, "seed": i}
            for i, (L, m) in enumerate(zip(lens, new))]


def run_engine(eng, reqs, extra, temperature=0.8, top_k=50):
    steps0 = eng.steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [eng.submit(r["tokens"], r["new"], temperature=temperature, top_k=top_k,
                       seed=r["seed"], **extra) for r in reqs]
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
    cases = [("off", {}, False)]
    dfa = None
    if a.cases == "all":
        from ray_amd.models.grammar import TokenDFA

        t0 = time.perf_counter()
        dfa = TokenDFA.from_regex(PATTERN, byte_vocab(torch.Generator().manual_seed(2)), EOS)
        print(json.dumps({"grammar_states": dfa.n_states,
                          "build_s": round(time.perf_counter() - t0, 2)}), flush=True)
        on = {"grammar_states": dfa.n_states}
        cases = [("grammar_states=0", {}, False),
                 ("pool on, no request uses it", on, False),
                 ("every request under the regex", on, True),
                 ("speculate=4", {"speculate": 4}, False),
                 ("speculate=4, pool on, no request uses it", dict(on, speculate=4), False),
                 ("speculate=4, every request under the regex", dict(on, speculate=4), True)]
    rows = []
    for S in (8, 64):
        paths = {}
        for name, kw, use in cases:
            eng = GPT2Engine(model, slots=S, max_len=max_len, poll_every=8, eos_token_id=EOS,
                             **kw)
            extra = {"grammar": eng.add_grammar(dfa)} if use else {}
            paths[name] = lambda eng=eng, extra=extra: run_engine(eng, reqs, extra)
        first = {n: fn() for n, fn in paths.items()}  # warm-up
        runs = {n: [] for n in paths}
        for _ in range(a.repeats):
            for n, fn in paths.items():
                runs[n].append(fn())
        for (n, rs), (_, _, use) in zip(runs.items(), cases):
            # the engine without the pool at the same ``speculate``
            ref_name = "speculate=4" if n.startswith("speculate") else cases[0][0]
            emitted = sum(len(t) for t in rs[0]["tokens"])
            rec = {"S": S, "path": n, "requested_tokens": requested, "emitted": emitted,
                   "tok_per_s": stats([emitted / r["wall"] for r in rs]),
                   "steps": rs[0]["steps"],
                   "same_tokens": sum(x == y for x, y in zip(first[n]["tokens"],
                                                             first[ref_name]["tokens"]))
                   / len(reqs),
                   "repeatable": all(r["tokens"] == first[n]["tokens"] for r in rs)}
            if use:  # every output is a word of the grammar, or a prefix cut by max_new_tokens
                rec["words"] = sum(
                    dfa.accepts(t) if t[-1] == EOS else
                    (len(t) == r["new"] and dfa.walk(t) >= 0)
                    for t, r in zip(rs[0]["tokens"], reqs)) / len(reqs)
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
        raise SystemExit("grammar_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    k = kernel_part(a, dev) if a.kernel and a.cases == "all" else None
    if k and a.kernel_json:
        os.makedirs(os.path.dirname(a.kernel_json) or ".", exist_ok=True)
        with open(a.kernel_json, "w") as fh:
            json.dump(k, fh)
    torch.cuda.empty_cache()
    erows = []
    if a.engine:
        torch.manual_seed(0)
        model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
        erows = engine_part(a, dev, model)
    if a.engine_json:
        os.makedirs(os.path.dirname(a.engine_json) or ".", exist_ok=True)
        with open(a.engine_json, "w") as fh:
            json.dump(erows, fh)
    if a.cases != "all":
        return
    prows = []
    for i, path in enumerate(a.parent_json):
        with open(path) as fh:
            prows += [dict(r, path=f"parent commit, process {i + 1}") for r in json.load(fh)]

    lines = ["# Grammar-constrained decoding: the token-DFA kernels", "",
             f"`scripts/grammar_bench.py` on {torch.cuda.get_device_name(0)}.", ""]
    if a.resources:
        lines += ["## The kernels' resources", "", a.resources, ""]
    if k:
        lines += [f"## `grammar_mask`, V = {V} bf16 (a view of a [B, {VPAD}] buffer)", "",
                  f"A table of {N_STATES} states x {VT} int16, every row in a state of its own; "
                  "`sparse` allows 0.1 % of the tokens, `nearly full` 99 %. "
                  f"{GRAPH_CALLS} calls of one path captured in one HIP graph and replayed, device "
                  f"events, the paths alternated, >= {a.seconds:g} s of timed work per path and "
                  f"repeat, median (min..max) of {a.repeats} repeats, microseconds per call. "
                  "`torch`: `logits.masked_fill_(table[state][:, :V] < 0, -inf)`. `banned`: "
                  "elements of the buffer the first call changed.", "",
                  "| B | allowed | hip device us | torch device us | torch / hip | bit equal | "
                  "banned |", "|---|---|---|---|---|---|---|"]
        for r in k["mask"]:
            dv = r["device_us"]
            lines.append(f"| {r['B']} | {r['allowed']} | {cell(dv['hip'], '.2f')} | "
                         f"{cell(dv['torch'])} | {r['speedup']:.1f}x | {r['bit_equal']} | "
                         f"{r['banned']} |")
        lines += ["", "## The chunk: 16-byte slots of a row per workgroup", "",
                  "The same call with `chunk=`; 0 is the launcher's rule (`auto`: what it chose). "
                  "A row has 6283 slots; a workgroup is one wave with 4 slots in flight per "
                  "lane, 256 per pass. Microseconds per call, median (min..max).", "",
                  "| B | allowed | auto | " + " | ".join(f"chunk {c}" for c in CHUNKS) + " |",
                  "|---|---|---|" + "---|" * len(CHUNKS)]
        for r in k["chunk"]:
            lines.append(f"| {r['B']} | {r['allowed']} | {r['auto']} | " + " | ".join(
                cell(r["device_us"][f"chunk {c}"], ".2f") for c in CHUNKS) + " |")
        lines += ["", "## `grammar_advance`", "",
                  "R context rows, 200 tokens each to consume, the `nearly full` table. A timed "
                  "call resets `state` and `pos` (two small copies, `reset only`) and advances.",
                  "", "| R | max_steps | reset + advance us | reset only us |", "|---|---|---|---|"]
        for r in k["advance"]:
            lines.append(f"| {r['R']} | {r['max_steps']} | "
                         f"{cell(r['device_us']['advance'], '.2f')} | "
                         f"{cell(r['device_us']['reset only'], '.2f')} |")
    if erows:
        lines += ["", "## Engine, GPT-2 small bf16, poll_every 8", "",
                  f"{a.requests} requests (prompts 16..128, max_new_tokens uniform in 16..256, "
                  f"{erows[0]['requested_tokens']} requested tokens, temperature 0.8, top-k 50, a "
                  f"seed each, eos_token_id {EOS}), all queued at t0. The grammar: `{PATTERN}` over "
                  "a synthetic byte vocabulary (256 single bytes, then random lower-case strings "
                  "of 2..4 letters). Wall time around synchronised runs, the paths alternated, "
                  f"median (min..max) of {a.repeats} repeats after one warm-up run; tokens/s "
                  "counts emitted tokens. `same tokens`: share of requests whose tokens equal "
                  "those of the engine without the pool at the same `speculate`. `words`: share "
                  "of outputs that are a word of the grammar, or a prefix of one cut by "
                  "`max_new_tokens`. `parent commit`: this script with `--repo` on a checkout of "
                  "the parent and `--cases none`, in processes of their own.",
                  "", "| S | path | emitted tokens/s | vs off | emitted | device steps | same "
                  "tokens | words | repeatable |", "|---|---|---|---|---|---|---|---|---|"]
        for r in prows:
            lines.append(f"| {r['S']} | {r['path']} | {cell(r['tok_per_s'], '.0f')} | | "
                         f"{r['emitted']} | {r['steps']} | | | {r['repeatable']} |")
        for r in erows:
            base = next(x for x in erows if x["S"] == r["S"] and x["path"] == "grammar_states=0")
            words = f"{r['words']:.2f}" if "words" in r else ""
            lines.append(f"| {r['S']} | {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{r['tok_per_s']['median'] / base['tok_per_s']['median']:.3f}x | "
                         f"{r['emitted']} | {r['steps']} | {r['same_tokens']:.2f} | {words} | "
                         f"{r['repeatable']} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
