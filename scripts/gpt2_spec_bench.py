#!/usr/bin/env python
"""Speculative decoding in the GPT-2 engine: what a speculative step costs and when it pays.

    python scripts/gpt2_spec_bench.py [--parts abcde] [--out profiles/r14/spec.md]
    python scripts/gpt2_spec_bench.py --parts e --tree <checkout of another commit>

(a) The two kernels of ops/csrc/spec.hip against the same decisions written as torch ops
    (``torch_draft`` / ``torch_accept`` below: no host read either), S 8 / 64, the slots at
    position 128 / 1000 of a 1024-position history, k 4, n-grams 2..4, GPT-2's 50304 logits
    columns. All paths captured in a HIP graph (20 calls per replay), device events around
    alternating blocks, median (min..max) of ``--repeats``.
(b) The captured device step, GPT-2 small bf16, every slot decoding at positions 64..: the
    plain step (``speculate=0``) against the speculative step for k 2 / 4 / 8 at S 1 / 8 / 64,
    from this one tree. ``full``: a drafter that always fills the window (with tokens the
    sampler rejects, so every step emits one token and no slot finishes), the most a step
    can cost; ``ngram``: the default drafter, whose windows are as long as its matches.
    Device events around blocks of graph replays. Break-even: a speculative step emits
    1 + (accepted drafts) tokens, so it pays when the mean number of accepted drafts per
    step exceeds t_spec / t_plain - 1.
(c) Engine tokens/s on the request mix of scripts/gpt2_engine_bench.py (256 requests, prompts
    16..128, 16..256 new tokens, temperature 0.8, top-k 50), ``poll_every`` 8, with an oracle
    drafter: it knows what the engine will emit (from a first run with the same k) and
    corrupts a draft with probability 1 - q, decided by a hash of the position.
(d) The same with the n-gram drafter on greedy requests whose prompt already holds the start
    of their own continuation (the prompt plus 64 tokens of its greedy continuation, so a
    loop the model has entered is in the history from the first step).
(e) Tokens/s of the engine WITHOUT the argument, for a comparison of ``speculate=0`` against
    another commit: run part e from both trees (``--tree``) and compare the ranges.

Wall time around synchronised calls for (c)-(e), the paths alternated, median (min..max) of
``--repeats`` after a warm-up run."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "r14", "spec.md"))
ap.add_argument("--parts", default="abcd")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose ray_amd is measured (default: this one)")
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--requests", type=int, default=256)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402

GRAPH_CALLS = 20
INACTIVE = -(1 << 30)


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


def time_paths(paths, seconds, repeats, prep=None, max_iters=None):
    """us per call of each path: warm-up, then ``repeats`` alternating blocks of >= seconds."""
    iters = {}
    for name, fn in paths.items():
        block_us(fn, 5, prep)
        iters[name] = max(10, int(seconds * 1e6 / block_us(fn, 20, prep)) + 1)
        if max_iters is not None:
            iters[name] = min(iters[name], max_iters)
    times = {n: [] for n in paths}
    for _ in range(repeats):
        for name, fn in paths.items():
            times[name].append(block_us(fn, iters[name], prep))
    return {n: stats(t) for n, t in times.items()}


# ------------------------------------------------------------------ (a) the kernels
def torch_draft(tok0, hist, lens, n_out, max_new, active, k, lo, hi, win, n_win):
    """``rf.spec_draft`` as torch ops on the device, no host read."""
    S, cap = hist.shape
    dev = hist.device
    ok = (active != 0) & (lens >= 0) & (lens < cap)
    p = lens.long().clamp(0, cap - 1)
    seq = hist.long().scatter(1, p.unsqueeze(1), tok0.unsqueeze(1))
    e = torch.arange(1, cap + 1, device=dev)  # a candidate's end j + n
    run = torch.ones(S, cap, dtype=torch.bool, device=dev)
    m = torch.zeros(S, cap, dtype=torch.long, device=dev)
    for i in range(hi):
        a = seq[:, (e - 1 - i).clamp(min=0)]
        b = seq.gather(1, (p - i).clamp(min=0).unsqueeze(1))
        run = run & (e - 1 - i >= 0).unsqueeze(0) & (i < p).unsqueeze(1) & (a == b)
        m += run
    key = torch.where((e.unsqueeze(0) <= p.unsqueeze(1)) & (m > 0), (m << 23) | e, 0)
    key = key.max(1).values
    start = key & ((1 << 23) - 1)
    room = torch.minimum(max_new - n_out, cap - lens).long()
    nd = torch.where((key >> 23) >= lo, (room - 1).clamp(0, k), torch.zeros_like(room))
    ext = torch.cat([seq, seq.new_zeros(S, k)], 1)  # seq running on into the drafts
    cols = [tok0]
    for i in range(1, k + 1):
        d = ext.gather(1, (start + i - 1).unsqueeze(1))
        ext.scatter_(1, (p + i).unsqueeze(1), d)
        cols.append(d.squeeze(1))
    col = torch.arange(k + 1, device=dev).unsqueeze(0)
    win.copy_(torch.where(ok.unsqueeze(1) & (col <= nd.unsqueeze(1)), torch.stack(cols, 1), win))
    n_win.copy_(torch.where(ok, 1 + nd, torch.zeros_like(nd)))


def torch_accept(win, n_win, cand, logits_win, lens, n_out, max_new, active, out, hist, buf,
                 n_drafted, n_accepted, eos):
    """``rf.spec_accept`` as torch ops on the device, no host read."""
    S, W = win.shape
    cap = out.shape[1]
    dev = win.device
    col = torch.arange(W, device=dev).unsqueeze(0)
    nw, n, p = n_win.long(), n_out.long(), lens.long()
    good = (active != 0) & (nw >= 1) & (nw <= W) & (n >= 0) & (n < cap) & (p >= 0) & (p < cap)
    agree = (win[:, 1:] == cand[:, :-1]) & (col[:, 1:] < nw.unsqueeze(1))
    a = agree.long().cumprod(1).sum(1)
    lim = torch.minimum(max_new.long() - n, cap - torch.maximum(n, p)).clamp(min=1)
    m = torch.minimum(a + 1, lim)
    first = torch.where((win == eos) & (col < m.unsqueeze(1)), col, W).min(1).values
    hit = (first < W) & good
    m = torch.where(good, torch.where(first < W, first + 1, m), torch.zeros_like(m))
    mask = col < m.unsqueeze(1)
    for table, at in ((out, n), (hist, p)):
        at0 = at.clamp(0, cap - 1).unsqueeze(1)
        # the columns that are not written all point at column `at`, with one value
        idx = torch.where(mask, at.unsqueeze(1) + col, at0)
        rest = torch.where((m > 0).unsqueeze(1), win[:, :1].to(table.dtype), table.gather(1, at0))
        table.scatter_(1, idx, torch.where(mask, win.to(table.dtype), rest))
    n_out += m.int()
    lens += m.int()
    n_drafted += torch.where(good, nw - 1, 0).int()
    n_accepted += torch.where(good, m - 1, 0).int()
    stay = good & ~hit & (n + m < max_new)
    active.copy_(stay)
    lens.masked_fill_(~stay, INACTIVE)
    row = logits_win[torch.arange(S, device=dev), (m - 1).clamp(min=0)]
    buf.copy_(torch.where(stay.unsqueeze(1), row, buf))


def kernel_part(a, dev):
    rows = []
    k, lo, hi, cap, Vp = 4, 2, 4, 1024, 50304
    for S in (8, 64):
        for p0 in (128, 1000):
            g = torch.Generator().manual_seed(S + p0)
            hist = torch.randint(0, 50257, (S, cap), generator=g, dtype=torch.int32)
            tok0 = torch.randint(0, 50257, (S,), generator=g)
            for s in range(0, S, 2):  # every other slot has seen its last 3 tokens before
                hist[s, 40:42] = hist[s, p0 - 2: p0]
                hist[s, 42] = tok0[s]
            base = dict(tok0=tok0, hist=hist, lens=torch.full((S,), p0, dtype=torch.int32),
                        n_out=torch.zeros(S, dtype=torch.int32),
                        max_new=torch.full((S,), 1 << 20, dtype=torch.int32),
                        active=torch.ones(S, dtype=torch.uint8))
            base["active"][::4] = 0
            st = {n: t.to(dev) for n, t in base.items()}
            wins = {n: (torch.zeros(S, k + 1, dtype=torch.int64, device=dev),
                        torch.zeros(S, dtype=torch.int32, device=dev)) for n in ("hip", "torch")}
            dargs = [st[n] for n in ("tok0", "hist", "lens", "n_out", "max_new", "active")]
            draft = {"hip": lambda: rf.spec_draft(*dargs, k, lo, hi, *wins["hip"]),
                     "torch": lambda: torch_draft(*dargs, k, lo, hi, *wins["torch"])}
            for fn in draft.values():
                fn()
            same_d = all(torch.equal(x, y) for x, y in zip(wins["hip"], wins["torch"]))
            rec = {"S": S, "p": p0, "draft_same": bool(same_d),
                   "mean_n_win": float(wins["hip"][1].float().mean()),
                   "draft_us": time_paths({n: graphed(f) for n, f in draft.items()}, a.seconds,
                                          a.repeats)}
            # accept: the cand agree with half of each window
            win, n_win = wins["hip"]
            cand = torch.cat([win[:, 1:3], win[:, 3:] + 1, win[:, :1]], 1)
            fixed = dict(win=win, n_win=n_win, cand=cand, max_new=st["max_new"],
                         logits_win=torch.randn(S, k + 1, Vp, device=dev).bfloat16())
            acap = 1 << 16
            state0 = dict(lens=st["lens"], n_out=st["n_out"], active=st["active"],
                          out=torch.zeros(S, acap, dtype=torch.int64, device=dev),
                          hist=torch.zeros(S, acap, dtype=torch.int32, device=dev),
                          buf=torch.zeros(S, Vp, device=dev, dtype=torch.bfloat16),
                          n_drafted=torch.zeros(S, dtype=torch.int32, device=dev),
                          n_accepted=torch.zeros(S, dtype=torch.int32, device=dev))
            states = {n: {k_: v.clone() for k_, v in state0.items()} for n in ("hip", "torch")}

            def call(fn, t, *tail):
                fn(fixed["win"], fixed["n_win"], fixed["cand"], fixed["logits_win"], t["lens"],
                   t["n_out"], fixed["max_new"], t["active"], t["out"], t["hist"], t["buf"],
                   t["n_drafted"], t["n_accepted"], *tail)

            accept = {"hip": lambda: call(rf.spec_accept, states["hip"]),
                      "torch": lambda: call(torch_accept, states["torch"], -1)}

            def reset():
                for t in states.values():
                    for n in ("lens", "n_out", "active"):
                        t[n].copy_(state0[n])

            for fn in accept.values():
                fn()
            same_a = all(torch.equal(states["hip"][n], states["torch"][n]) for n in state0)
            reset()
            rec["accept_same"] = bool(same_a)
            rec["accept_us"] = time_paths({n: graphed(f) for n, f in accept.items()}, a.seconds,
                                          a.repeats, prep=reset,
                                          max_iters=(acap - p0) // (GRAPH_CALLS * (k + 1)) - 2)
            rec["draft_us"] = {n: {q: v / GRAPH_CALLS for q, v in s.items()}
                               for n, s in rec["draft_us"].items()}
            rec["accept_us"] = {n: {q: v / GRAPH_CALLS for q, v in s.items()}
                                for n, s in rec["accept_us"].items()}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            del states, state0, fixed
    return rows


# ------------------------------------------------------------------ (b) the step
class FullWindow:
    """Always a full window, of tokens the sampler does not draw (tok0 + 1 + i: a match is a
    1-in-50257 accident), so a step costs its most and emits one token."""

    def __init__(self, k, vocab, dev):
        self.k, self.vocab = k, vocab
        self.ahead = torch.arange(k + 1, device=dev).unsqueeze(0)

    def __call__(self, tok0, hist, lens, n_out, max_new, active):
        cap = hist.shape[1]
        room = torch.minimum(max_new - n_out, cap - lens)
        ok = (active != 0) & (lens >= 0) & (lens < cap)
        n_win = torch.where(ok, 1 + (room - 1).clamp(0, self.k), torch.zeros_like(room))
        return (tok0.unsqueeze(1) + self.ahead) % self.vocab, n_win


def step_part(a, dev, model):
    rows = []
    V = model.cfg.vocab_size
    for S in (1, 8, 64):
        g = torch.Generator().manual_seed(S)
        prompts = [torch.randint(0, V, (64,), generator=g).tolist() for _ in range(S)]
        engines = {"plain": GPT2Engine(model, slots=S, max_len=1024, speculate=0)}
        for k in (2, 4, 8):
            engines[f"k={k} full"] = GPT2Engine(model, slots=S, max_len=1024, speculate=k,
                                                drafter=FullWindow(k, V, dev))
            engines[f"k={k} ngram"] = GPT2Engine(model, slots=S, max_len=1024, speculate=k)
        for eng in engines.values():  # every slot decoding, far from its end
            for i, p in enumerate(prompts):
                eng.submit(p, 960, temperature=0.8, top_k=50, seed=i)
            eng._admit()       # noqa: SLF001
            eng._fill_round()  # noqa: SLF001
        # 25 warm-up steps and 3 blocks of <= 60: no slot reaches its 960 tokens unless nearly
        # every draft is accepted (still_active tells)
        paths = {n: eng._graph.replay for n, eng in engines.items()}  # noqa: SLF001
        us = time_paths(paths, a.seconds, a.repeats, max_iters=60)
        rec = {"S": S, "step_us": us,
               "still_active": {n: int(e.active.sum()) for n, e in engines.items()},
               "stats": {n: e.spec_stats() for n, e in engines.items() if n != "plain"}}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del engines, paths
        torch.cuda.empty_cache()
    return rows


# ------------------------------------------------------------------ (c) (d) (e) end to end
def make_requests(n, vocab):
    """The mix of scripts/gpt2_engine_bench.py."""
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(16, 129, (n,), generator=g).tolist()
    new = torch.randint(16, 257, (n,), generator=g).tolist()
    return [{"tokens": torch.randint(0, vocab, (L,), generator=g).tolist(), "new": m, "seed": i}
            for i, (L, m) in enumerate(zip(lens, new))]


def run_engine(eng, reqs, temp, top_k):
    steps0 = eng.steps
    stats0 = eng.spec_stats() if hasattr(eng, "spec_stats") else {"drafted": 0, "accepted": 0}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [eng.submit(r["tokens"], r["new"], temperature=temp, top_k=top_k, seed=r["seed"])
            for r in reqs]
    got = {}
    while eng.has_work():
        for rid, new, _ in eng.step():
            got.setdefault(rid, []).extend(new)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st = eng.spec_stats() if hasattr(eng, "spec_stats") else stats0
    return {"wall": wall, "tokens": [got[r] for r in rids], "steps": eng.steps - steps0,
            "drafted": st["drafted"] - stats0["drafted"],
            "accepted": st["accepted"] - stats0["accepted"]}


class Oracle:
    """Knows the sequences (found by a slot's first 16 tokens: the prompts are random and at
    least that long), proposes their continuation and corrupts a draft with probability
    1 - q, decided by a hash of its position. torch ops only: capturable. ``q`` 0 knows
    nothing: every draft is wrong."""

    def __init__(self, sequences, k, cap, vocab, q, dev):
        self.k, self.vocab, self.keep = k, vocab, int(q * 1024)
        full = torch.zeros(len(sequences), cap + k + 1, dtype=torch.int64)
        for r, seq in enumerate(sequences):
            full[r, : len(seq)] = torch.tensor(seq)
        self.full = full.to(dev)
        self.head = self.full[:, :16].contiguous()
        self.ahead = torch.arange(1, k + 1, device=dev).unsqueeze(0)

    def __call__(self, tok0, hist, lens, n_out, max_new, active):
        cap = hist.shape[1]
        ok = (active != 0) & (lens >= 0) & (lens < cap)
        r = (hist[:, :16].long().unsqueeze(1) == self.head.unsqueeze(0)).all(-1).long().argmax(1)
        pos = lens.long().clamp(0, cap - 1).unsqueeze(1) + self.ahead
        drafts = self.full[r].gather(1, pos)
        wrong = ((pos * 2654435761) >> 7) % 1024 >= self.keep
        drafts = torch.where(wrong, (drafts + 1) % self.vocab, drafts)
        room = torch.minimum(max_new - n_out, cap - lens)
        n_win = torch.where(ok, 1 + (room - 1).clamp(0, self.k), torch.zeros_like(room))
        return torch.cat([tok0.unsqueeze(1), drafts], 1), n_win


def measure(paths, repeats, requested_of):
    first = {n: fn() for n, fn in paths.items()}  # warm-up
    runs = {n: [] for n in paths}
    for _ in range(repeats):
        for n, fn in paths.items():
            runs[n].append(fn())
    rows = []
    for n, rs in runs.items():
        req = requested_of(n)
        emitted = sum(len(t) for t in rs[0]["tokens"])
        rec = {"path": n, "tokens": emitted,
               "tok_per_s": stats([req / r["wall"] for r in rs]), "steps": rs[0]["steps"],
               "drafted": rs[0]["drafted"], "accepted": rs[0]["accepted"],
               # a slot's step emits 1 + (accepted drafts) tokens
               "accepted_per_slot_step": rs[0]["accepted"] / max(emitted - rs[0]["accepted"], 1),
               "repeatable": all(r["tokens"] == first[n]["tokens"] for r in rs)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows, first


def oracle_part(a, dev, model):
    reqs = make_requests(a.requests, model.cfg.vocab_size)
    requested = sum(r["new"] for r in reqs)
    max_len = max(len(r["tokens"]) for r in reqs) + max(r["new"] for r in reqs)
    V, k = model.cfg.vocab_size, 4
    paths, first_tokens = {}, {}
    for S in (8, 64):
        plain = GPT2Engine(model, slots=S, max_len=max_len, speculate=0)
        paths[f"S={S} plain"] = lambda e=plain: run_engine(e, reqs, 0.8, 50)
        # what the speculative engine emits, from a run whose drafts are all wrong
        blind = GPT2Engine(model, slots=S, max_len=max_len, speculate=k,
                           drafter=Oracle([r["tokens"] for r in reqs], k, max_len, V, 0.0, dev))
        toks = run_engine(blind, reqs, 0.8, 50)["tokens"]
        first_tokens[S] = toks
        paths[f"S={S} k={k} q=0"] = lambda e=blind: run_engine(e, reqs, 0.8, 50)
        seqs = [r["tokens"] + t for r, t in zip(reqs, toks)]
        for q in (0.5, 0.8, 1.0):
            eng = GPT2Engine(model, slots=S, max_len=max_len, speculate=k,
                             drafter=Oracle(seqs, k, max_len, V, q, dev))
            paths[f"S={S} k={k} q={q}"] = lambda e=eng: run_engine(e, reqs, 0.8, 50)
    rows, first = measure(paths, a.repeats, lambda n: requested)
    for r in rows:
        S = int(r["path"].split()[0][2:])
        r["same_as_q0"] = sum(x == y for x, y in zip(first[r["path"]]["tokens"],
                                                    first_tokens[S])) / len(reqs)
    return rows, requested


def ngram_part(a, dev, model):
    n = min(a.requests, 64)
    base = make_requests(n, model.cfg.vocab_size)
    # each prompt followed by 64 tokens of its own greedy continuation
    idx_lens = [len(r["tokens"]) for r in base]
    reqs = []
    for c in range(0, n, 16):
        part = base[c: c + 16]
        idx = torch.zeros(len(part), max(idx_lens[c: c + 16]), dtype=torch.long)
        for b, r in enumerate(part):
            idx[b, : len(r["tokens"])] = torch.tensor(r["tokens"])
        out = model.generate(idx.to(dev), 64, lens=idx_lens[c: c + 16], temperature=0.0,
                             seeds=0, graph=True).cpu()
        reqs += [{"tokens": r["tokens"] + out[b].tolist(), "new": 256, "seed": r["seed"]}
                 for b, r in enumerate(part)]
    requested = sum(r["new"] for r in reqs)
    max_len = max(len(r["tokens"]) for r in reqs) + 256
    paths = {}
    for S in (8, 64):
        for k in (0, 4, 8):
            eng = GPT2Engine(model, slots=S, max_len=max_len, speculate=k)
            paths[f"S={S} " + (f"k={k} ngram 2..4" if k else "plain")] = \
                lambda e=eng: run_engine(e, reqs, 0.0, None)
    rows, _ = measure(paths, a.repeats, lambda n_: requested)
    return rows, len(reqs), requested


def default_part(a, dev, model):
    reqs = make_requests(a.requests, model.cfg.vocab_size)
    requested = sum(r["new"] for r in reqs)
    max_len = max(len(r["tokens"]) for r in reqs) + max(r["new"] for r in reqs)
    paths = {}
    for S in (8, 64):
        eng = GPT2Engine(model, slots=S, max_len=max_len)  # no speculate argument at all
        paths[f"S={S} engine, no argument"] = lambda e=eng: run_engine(e, reqs, 0.8, 50)
    rows, _ = measure(paths, a.repeats, lambda n: requested)
    return rows


def cell(s, fmt=".1f"):
    return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("gpt2_spec_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    lines = ["# Speculative decoding: the kernels, the step and the engine", "",
             f"`scripts/gpt2_spec_bench.py --parts {a.parts}` on {torch.cuda.get_device_name(0)}, "
             f"tree `{os.path.relpath(os.path.abspath(a.tree))}`. Median (min..max) of "
             f"{a.repeats} repeats everywhere.", ""]
    if "a" in a.parts:
        rows = kernel_part(a, dev)
        lines += ["## (a) spec_draft and spec_accept against torch ops", "",
                  "k 4, n-grams 2..4, a 1024-position history, 50304 logits columns; a quarter of "
                  "the slots idle, every other active slot has a match. Microseconds per call "
                  "inside a HIP graph of 20 calls.", "",
                  "| S | p | draft hip | draft torch | torch / hip | accept hip | accept torch | "
                  "torch / hip | same results |", "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            d, c = r["draft_us"], r["accept_us"]
            lines.append(f"| {r['S']} | {r['p']} | {cell(d['hip'], '.2f')} | "
                         f"{cell(d['torch'], '.1f')} | "
                         f"{d['torch']['median'] / d['hip']['median']:.0f}x | "
                         f"{cell(c['hip'], '.2f')} | {cell(c['torch'], '.1f')} | "
                         f"{c['torch']['median'] / c['hip']['median']:.0f}x | "
                         f"{r['draft_same'] and r['accept_same']} |")
        lines.append("")
    model = None
    if set(a.parts) & set("bcde"):
        torch.manual_seed(0)
        model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    if "b" in a.parts:
        rows = step_part(a, dev, model)
        lines += ["## (b) the captured step, GPT-2 small bf16", "",
                  "Every slot decoding (prompt 64, sampling with temperature 0.8 and top-k 50). "
                  "Microseconds per graph replay, device events around blocks of up to 60 replays. "
                  "Break-even: the mean number of accepted drafts per step above which the "
                  "speculative step emits tokens faster than the plain one, t_spec / t_plain - 1.",
                  "", "| S | path | step us | vs plain | break-even accepted drafts per slot and "
                  "step |",
                  "|---|---|---|---|---|"]
        for r in rows:
            t0 = r["step_us"]["plain"]["median"]
            for n, s in r["step_us"].items():
                ratio = s["median"] / t0
                lines.append(f"| {r['S']} | {n} | {cell(s, '.0f')} | {ratio:.2f}x | "
                             + ("" if n == "plain" else f"{ratio - 1:.2f}") + " |")
        lines.append("")
    if "c" in a.parts:
        rows, requested = oracle_part(a, dev, model)
        lines += ["## (c) engine tokens/s with an oracle drafter, k 4", "",
                  f"{a.requests} requests ({requested} requested tokens), all queued at t0, "
                  "`poll_every` 8. q: the probability that the oracle leaves a draft as it knows "
                  "it. `same tokens`: the share of requests whose tokens equal the q = 0 run's, "
                  "which is where the oracle's knowledge comes from. With random-init weights "
                  "the logits are nearly flat, and another admission round or window length "
                  "reorders bf16 sums enough to flip a token (profiles/r10/engine.md has the same "
                  "column); from there on the oracle drafts a continuation that is no longer the "
                  "request's and its drafts are rejected. So read the tokens/s against the "
                  "acceptance a row REACHED, not against q.", "",
                  "| path | requested tokens/s | vs plain | device steps | accepted / drafted | "
                  "accepted drafts per slot and step | same tokens | repeatable |",
                  "|---|---|---|---|---|---|---|---|"]
        plain = {r["path"].split()[0]: r["tok_per_s"]["median"] for r in rows
                 if r["path"].endswith("plain")}
        for r in rows:
            lines.append(f"| {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{r['tok_per_s']['median'] / plain[r['path'].split()[0]]:.2f}x | "
                         f"{r['steps']} | {r['accepted']} / {r['drafted']} | "
                         f"{r['accepted_per_slot_step']:.2f} | {r['same_as_q0']:.2f} | "
                         f"{r['repeatable']} |")
        lines.append("")
    if "d" in a.parts:
        rows, n, requested = ngram_part(a, dev, model)
        lines += ["## (d) engine tokens/s with the n-gram drafter", "",
                  f"{n} greedy requests of 256 new tokens ({requested} requested tokens); each "
                  "prompt is a random prompt followed by 64 tokens of its own greedy continuation. "
                  "The weights are the random init: what the model repeats, and so what the "
                  "drafter finds, says nothing about real text.", "",
                  "| path | requested tokens/s | vs plain | device steps | accepted / drafted | "
                  "accepted drafts per slot and step | repeatable |",
                  "|---|---|---|---|---|---|---|"]
        plain = {r["path"].split()[0]: r["tok_per_s"]["median"] for r in rows
                 if r["path"].endswith("plain")}
        for r in rows:
            lines.append(f"| {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{r['tok_per_s']['median'] / plain[r['path'].split()[0]]:.2f}x | "
                         f"{r['steps']} | {r['accepted']} / {r['drafted']} | "
                         f"{r['accepted_per_slot_step']:.2f} | {r['repeatable']} |")
        lines.append("")
    if "e" in a.parts:
        rows = default_part(a, dev, model)
        lines += ["## (e) the engine without the argument", "",
                  "The request mix of (c), `poll_every` 8. Run from two trees to compare them.", "",
                  "| path | requested tokens/s | device steps |", "|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['path']} | {cell(r['tok_per_s'], '.0f')} | {r['steps']} |")
        lines.append("")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
