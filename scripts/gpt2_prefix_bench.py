#!/usr/bin/env python
"""Shared prefixes and chunked prefill: ``rf.attn_extend`` and ``rf.kv_copy`` against their
torch compositions, and ``GPT2Engine`` with the two options against itself without them.

    python scripts/gpt2_prefix_bench.py [--out profiles/r11/prefix.md]

Kernel part, timed as in ``gpt2_engine_bench.py`` (device events around alternating blocks
of the paths, a warm-up and at least ``--seconds`` of timed work per path and repeat, median
(min..max) of ``--repeats``; ``device`` is 20 calls captured in one HIP graph and replayed).
``attn_extend``: one layer, H = 12, D = 64, a 64-slot x 1024-position cache, Bn rows with
``base`` cached positions and ``n_new`` new tokens each. ``hip`` is one ``rf.attn_extend``
call (append launch + attention launch); ``torch`` is the composition on the same cache with
slots, base and n_new on the device: an indexed copy of the new K/V into the cache, a gather
of the cache rows, a materialised [Bn, 1, Tn, Tmax] mask and SDPA. ``kv_copy``: 12 layers of
T positions of Bn rows from a 4-row store into a 64-slot cache; ``hip`` is one ``rf.kv_copy``
call, ``indexed`` is ``dst[:, rows, :, :T] = src[:, srcs, :, :T]`` for K and for V.

Engine part: GPT-2 small, bf16, S = 64, wall time around synchronised calls, the paths
alternated, median (min..max) of ``--repeats`` after one warm-up run. Prefix: ``--requests``
requests that share one 512-token prefix (continuations 16..64 tokens, ``max_new_tokens``
16..64, temperature 0.8, top-k 50), all queued at t0, submitted with ``prefix=`` against
submitted with their full prompts; time to first token counts from t0. Chunked prefill: 32
requests decoding (32-token prompts, 160 new tokens) when eight 768-token prompts arrive,
``prefill_chunk`` None against 128; the gap is the longest time between two ``step()``
returns that delivered tokens for one of the 32."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gpt2_engine_bench import stats, time_paths  # noqa: E402
from ray_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402

H, D, LAYERS = 12, 64, 12
CACHE_SLOTS, CACHE_T = 64, 1024
EXTEND_SHAPES = [(1, 512, 32), (8, 512, 32), (8, 0, 512), (1, 896, 128)]
COPY_SHAPES = [(1, 512), (8, 512)]


def extend_part(a, dev):
    g = torch.Generator().manual_seed(0)
    kc = torch.randn(CACHE_SLOTS, H, CACHE_T, D, generator=g).bfloat16().to(dev)
    vc = torch.randn(CACHE_SLOTS, H, CACHE_T, D, generator=g).bfloat16().to(dev)
    t = torch.arange(CACHE_T, device=dev).view(1, 1, 1, CACHE_T)
    rows = []
    for Bn, base, n in EXTEND_SHAPES:
        qkv = torch.randn(Bn, n, 3, H, D, generator=g).bfloat16().to(dev)
        slots = torch.randperm(CACHE_SLOTS, generator=g)[:Bn].to(dev)
        slots32 = slots.to(torch.int32)
        base_t = torch.full((Bn,), base, dtype=torch.int32, device=dev)
        n_t = torch.full((Bn,), n, dtype=torch.int32, device=dev)
        i = torch.arange(n, device=dev)

        def hip():
            return rf.attn_extend(qkv, kc, vc, slots32, base_t, n_t)

        def composed():
            pos = base_t.long().view(Bn, 1) + i  # [Bn, Tn]
            kc[slots.view(Bn, 1), :, pos] = qkv[:, :, 1]
            vc[slots.view(Bn, 1), :, pos] = qkv[:, :, 2]
            mask = t <= pos.view(Bn, 1, n, 1)
            y = F.scaled_dot_product_attention(qkv[:, :, 0].transpose(1, 2), kc[slots], vc[slots],
                                               attn_mask=mask)
            return y.transpose(1, 2)

        a_out, b_out = hip().float(), composed().float()
        rel = ((a_out - b_out).norm() / b_out.norm()).item()
        paths = {"hip": hip, "torch": composed}
        rec = {"Bn": Bn, "base": base, "n_new": n, "rel_diff": rel,
               "us": time_paths(paths, a.seconds, a.repeats),
               "device_us": time_paths(paths, a.seconds, a.repeats, in_graph=True)}
        kv_bytes = 2 * Bn * H * (base + n) * D * 2  # K and V rows the queries attend over
        rec["hip_GBps"] = kv_bytes / rec["device_us"]["hip"]["median"] * 1e-3
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def copy_part(a, dev):
    g = torch.Generator().manual_seed(1)
    sk = torch.randn(LAYERS, 4, H, CACHE_T, D, generator=g).bfloat16().to(dev)
    sv = torch.randn(LAYERS, 4, H, CACHE_T, D, generator=g).bfloat16().to(dev)
    dk = torch.zeros(LAYERS, CACHE_SLOTS, H, CACHE_T, D, dtype=torch.bfloat16, device=dev)
    dv = torch.zeros_like(dk)
    rows = []
    for Bn, T in COPY_SHAPES:
        dst = torch.randperm(CACHE_SLOTS, generator=g)[:Bn].to(dev)
        src = torch.randint(0, 4, (Bn,), generator=g).to(dev)
        dst32, src32 = dst.to(torch.int32), src.to(torch.int32)
        lens = torch.full((Bn,), T, dtype=torch.int32, device=dev)

        def hip():
            rf.kv_copy(sk, sv, dk, dv, src32, dst32, lens)

        def indexed():
            dk[:, dst, :, :T] = sk[:, src, :, :T]
            dv[:, dst, :, :T] = sv[:, src, :, :T]

        outs = []
        for fn in (hip, indexed):
            dk.zero_()
            dv.zero_()
            fn()
            outs.append((dk.clone(), dv.clone()))
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


# ------------------------------------------------------------------ engine
def drive(eng, submit_first, submit_later=None, later_after=0, watch=None):
    """Runs the engine dry. ``submit_first()`` / ``submit_later()`` return request ids; the
    second is called after ``later_after`` ``step()`` calls. ``watch``: ids of the first group
    whose delivery gaps are measured from the moment the second group is submitted."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = list(submit_first())
    got, first_tok, calls, step_s = {}, {}, 0, []
    last_seen, gap = None, 0.0
    while eng.has_work():
        if submit_later is not None and calls == later_after:
            rids += list(submit_later())
            submit_later = None
            last_seen = time.perf_counter()
        before = time.perf_counter()
        events = eng.step()
        calls += 1
        now = time.perf_counter()
        step_s.append(now - before)
        for rid, new, _fin in events:
            if new and rid not in first_tok:
                first_tok[rid] = now - t0
            got.setdefault(rid, []).extend(new)
        if last_seen is not None and watch and any(rid in watch and new for rid, new, _ in events):
            gap = max(gap, now - last_seen)
            last_seen = now
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"wall": wall, "tokens": [got[r] for r in rids],
            "ttft": [first_tok[r] for r in rids], "gap": gap,
            "median_step": sorted(step_s)[len(step_s) // 2]}


def repeat_paths(paths, repeats):
    first = {n: fn() for n, fn in paths.items()}  # warm-up
    runs = {n: [] for n in paths}
    for _ in range(repeats):
        for n, fn in paths.items():
            runs[n].append(fn())
    return first, runs


def prefix_part(a, model, dev):
    vocab = model.cfg.vocab_size
    g = torch.Generator().manual_seed(2)
    prefix = torch.randint(0, vocab, (512,), generator=g).tolist()
    lens = torch.randint(16, 65, (a.requests,), generator=g).tolist()
    new = torch.randint(16, 65, (a.requests,), generator=g).tolist()
    conts = [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lens]
    eng = GPT2Engine(model, slots=64, max_len=640, prefix_slots=1)
    pid = eng.add_prefix(prefix)

    def submit(with_prefix):
        return [eng.submit(c if with_prefix else prefix + c, m, temperature=0.8, top_k=50, seed=i,
                           prefix=pid if with_prefix else None)
                for i, (c, m) in enumerate(zip(conts, new))]

    paths = {"full prompts": lambda: drive(eng, lambda: submit(False)),
             "prefix=": lambda: drive(eng, lambda: submit(True))}
    first, runs = repeat_paths(paths, a.repeats)
    rows = []
    for n, rs in runs.items():
        rec = {"path": n, "requested_tokens": sum(new),
               "tok_per_s": stats([sum(new) / r["wall"] for r in rs]),
               "mean_ttft_s": stats([sum(r["ttft"]) / len(r["ttft"]) for r in rs]),
               "same_as_full": sum(x == y for x, y in zip(first[n]["tokens"],
                                                          first["full prompts"]["tokens"]))
               / a.requests,
               "repeatable": all(r["tokens"] == first[n]["tokens"] for r in rs)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def chunk_part(a, model, dev):
    vocab = model.cfg.vocab_size
    g = torch.Generator().manual_seed(3)
    short = [torch.randint(0, vocab, (32,), generator=g).tolist() for _ in range(32)]
    long_ = [torch.randint(0, vocab, (768,), generator=g).tolist() for _ in range(8)]
    total = 32 * 160 + 8 * 32
    paths = {}
    for chunk in (None, 128):
        eng = GPT2Engine(model, slots=64, max_len=1024, prefill_chunk=chunk)
        watch = set()

        def first(eng=eng, watch=watch):
            rids = [eng.submit(p, 160, temperature=0.8, top_k=50, seed=i)
                    for i, p in enumerate(short)]
            watch.clear()
            watch.update(rids)
            return rids

        def later(eng=eng):
            return [eng.submit(p, 32, temperature=0.8, top_k=50, seed=100 + i)
                    for i, p in enumerate(long_)]

        paths[f"prefill_chunk={chunk}"] = lambda eng=eng, first=first, later=later, watch=watch: \
            drive(eng, first, later, later_after=4, watch=watch)
    first_runs, runs = repeat_paths(paths, a.repeats)
    rows = []
    for n, rs in runs.items():
        rec = {"path": n, "requested_tokens": total,
               "max_gap_ms": stats([r["gap"] * 1e3 for r in rs]),
               "median_step_ms": stats([r["median_step"] * 1e3 for r in rs]),
               "tok_per_s": stats([total / r["wall"] for r in rs]),
               "same_as_unchunked": sum(x == y for x, y in zip(
                   first_runs[n]["tokens"], first_runs["prefill_chunk=None"]["tokens"])) / 40,
               "repeatable": all(r["tokens"] == first_runs[n]["tokens"] for r in rs)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r11", "prefix.md"))
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--no-e2e", dest="e2e", action="store_false")
    ap.add_argument("--no-kernels", dest="kernels", action="store_false")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpt2_prefix_bench needs a GPU: timings are device timings")
    _lib.lib()
    dev = torch.device("cuda")
    xrows = extend_part(a, dev) if a.kernels else []
    crows = copy_part(a, dev) if a.kernels else []
    torch.cuda.empty_cache()
    prows = krows = []
    if a.e2e:
        torch.manual_seed(0)
        model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
        prows = prefix_part(a, model, dev)
        torch.cuda.empty_cache()
        krows = chunk_part(a, model, dev)

    def cell(s, fmt=".1f"):
        return f"{s['median']:{fmt}} ({s['min']:{fmt}}..{s['max']:{fmt}})"

    lines = ["# Shared prefixes and chunked prefill: attn_extend, kv_copy and the engine", "",
             f"`scripts/gpt2_prefix_bench.py` on {torch.cuda.get_device_name(0)}.", ""]
    timing = (f"Device events, the paths alternated in one process, >= {a.seconds:g} s of timed "
              f"work per path and repeat, median (min..max) of {a.repeats} repeats, microseconds. "
              "`call`: eager calls from Python; `device`: captured in one HIP graph and replayed.")
    if xrows:
        lines += ["## attn_extend, one layer (H = 12, D = 64, bf16, 64-slot x 1024-position cache)",
                  "", timing + " `torch`: indexed copy of the new K/V, gather of the cache rows, "
                  "materialised mask, SDPA, every index on the device. GB/s: bytes of the K and V "
                  "rows attended over (base + n_new per row) over the hip device median. "
                  "`rel diff`: |hip - torch| / |torch| of the bf16 outputs.", "",
                  "| Bn | base | n_new | hip call us | torch call us | hip device us | "
                  "torch device us | hip vs torch (device) | hip K/V GB/s | rel diff |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for r in xrows:
            u, dv = r["us"], r["device_us"]
            lines.append(f"| {r['Bn']} | {r['base']} | {r['n_new']} | {cell(u['hip'])} | "
                         f"{cell(u['torch'])} | {cell(dv['hip'], '.2f')} | "
                         f"{cell(dv['torch'], '.2f')} | "
                         f"{dv['torch']['median'] / dv['hip']['median']:.2f}x | "
                         f"{r['hip_GBps']:.0f} | {r['rel_diff']:.1e} |")
    if crows:
        lines += ["", "## kv_copy, 12 layers (4-row store into a 64-slot cache, 1024 positions)", "",
                  timing + " `indexed`: `dst[:, rows, :, :T] = src[:, srcs, :, :T]` for K and V. "
                  "GB/s: K/V bytes read plus written over the hip device median.", "",
                  "| Bn | T | hip call us | indexed call us | hip device us | indexed device us | "
                  "hip vs indexed (device) | hip GB/s | same bits |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in crows:
            u, dv = r["us"], r["device_us"]
            lines.append(f"| {r['Bn']} | {r['T']} | {cell(u['hip'])} | {cell(u['indexed'])} | "
                         f"{cell(dv['hip'], '.2f')} | {cell(dv['indexed'], '.2f')} | "
                         f"{dv['indexed']['median'] / dv['hip']['median']:.2f}x | "
                         f"{r['hip_GBps']:.0f} | {r['same']} |")
    if prows:
        lines += ["", "## Engine with and without the prefix cache, GPT-2 small bf16, S = 64", "",
                  f"{a.requests} requests sharing one 512-token prefix (continuations 16..64 tokens, "
                  f"max_new_tokens 16..64, {prows[0]['requested_tokens']} requested tokens, "
                  "temperature 0.8, top-k 50, a seed each), all queued at t0, one engine. Wall time "
                  f"around synchronised calls, the paths alternated, median (min..max) of {a.repeats} "
                  "repeats after one warm-up run. Time to first token counts from t0. `same "
                  "tokens`: share of requests whose tokens equal the full-prompt run's (bf16: the "
                  "two paths attend through different kernels and a near-tie may flip).", "",
                  "| path | requested tokens/s | mean time to first token s | same tokens | "
                  "repeatable |", "|---|---|---|---|---|"]
        for r in prows:
            lines.append(f"| {r['path']} | {cell(r['tok_per_s'], '.0f')} | "
                         f"{cell(r['mean_ttft_s'], '.3f')} | {r['same_as_full']:.2f} | "
                         f"{r['repeatable']} |")
    if krows:
        lines += ["", "## Chunked prefill, GPT-2 small bf16, S = 64, poll_every 8", "",
                  "32 requests decoding (32-token prompts, 160 new tokens each) when eight "
                  "768-token prompts (32 new tokens each) arrive after the fourth `step()`. `gap`: "
                  "the longest time between two `step()` returns that delivered tokens for one of "
                  "the 32, from the arrival on, milliseconds; `step`: the median duration of a "
                  "`step()` call of the run (8 device steps and a poll, mostly without any "
                  "prefill). Same timing rules as above.", "",
                  "| path | largest gap ms | median step ms | requested tokens/s | same tokens | "
                  "repeatable |", "|---|---|---|---|---|---|"]
        for r in krows:
            lines.append(f"| {r['path']} | {cell(r['max_gap_ms'], '.1f')} | "
                         f"{cell(r['median_step_ms'], '.1f')} | {cell(r['tok_per_s'], '.0f')} | {r['same_as_unchunked']:.2f} | "
                         f"{r['repeatable']} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
