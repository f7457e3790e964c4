#!/usr/bin/env python
"""The int8 K/V cache (ops/csrc/attn_decode_q8.hip) against the bf16 cache.

    python scripts/kv_q8_bench.py [--part decode|insert|engine|drift] [--out FILE.jsonl]
                                  [--tree DIR] [--kv-cache none int8]

decode: ``rf.attn_decode`` at H = 12, Tmax = 1024 on an int8 and on a bf16 cache holding the
same values, over 12 layers' caches in turn as a decode step reads them (so no call finds the
previous call's cache in the last-level cache). The 12 calls are captured in one HIP graph;
device events around alternating replays, a warm-up, median (min..max) of ``--repeats``
blocks, microseconds per call. GB/s: the K/V bytes and scales a call must read over that.

insert: ``rf.kv_insert`` over 12 layers into a 64-slot, 1024-position cache, int8 against
bf16, measured the same way; microseconds per 12 layers.

engine: ``GPT2Engine`` (GPT-2 small bf16, ``poll_every`` 8) on the request mix of
scripts/gpt2_engine_bench.py at S = 8 and S = 64, once per ``--kv-cache`` value, the engines
alternated; requested tokens per second of wall time, and the cache's bytes. ``--tree DIR``
imports ``ray_amd`` from another checkout (with ``--kv-cache none`` one that does not know
the option), for a comparison between commits in separate processes.

drift: for information only, the largest difference between the logits of one decode step on
the int8 and on the bf16 cache, GPT-2 small with the seeded random init after a 64-token
prompt. Random weights say nothing about the quality of generated text.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("decode", "insert", "engine", "drift"), default="decode")
ap.add_argument("--out", default=None)
ap.add_argument("--tree", default=os.path.dirname(HERE))
ap.add_argument("--kv-cache", nargs="*", default=["none", "int8"], choices=("none", "int8"))
ap.add_argument("--seconds", type=float, default=0.2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--requests", type=int, default=256)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
sys.path.append(HERE)

import torch  # noqa: E402

from ray_amd.models.gpt2 import GPT2, GPT2Config, KVCache  # noqa: E402
from ray_amd.models.gpt2_engine import GPT2Engine  # noqa: E402
from ray_amd.ops import _lib  # noqa: E402
from ray_amd.ops import functional as rf  # noqa: E402
from ray_amd.ops import reference as ref  # noqa: E402

H, D, LAYERS, TMAX = 12, 64, 12, 1024
DECODE_SHAPES = [(1, 1023), (8, 1023), (64, 1023), (64, 127)]
INSERT_SHAPES = [(1, 128), (8, 128), (8, 1024)]
INSERT_SLOTS = 64


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


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


def time_paths(paths, a, per):
    """Microseconds per ``per``-th of a call of each path, the paths alternated."""
    reps = {n: graphed(fn) for n, fn in paths.items()}
    iters = {n: max(5, int(a.seconds * 1e6 / block_us(r, 5)) + 1) for n, r in reps.items()}
    times = {n: [] for n in reps}
    for _ in range(a.repeats):
        for n, r in reps.items():
            times[n].append(block_us(r, iters[n]) / per)
    return {n: stats(t) for n, t in times.items()}


def quantised(x):
    """``ref.quantize_kv`` layer by layer (its fp32 temporaries are 4x the bf16 cache)."""
    q = torch.empty(x.shape, dtype=torch.int8, device=x.device)
    s = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    for i in range(x.shape[0]):
        q[i], s[i] = ref.quantize_kv(x[i])
    return q, s


def decode_part(a, emit):
    dev = torch.device("cuda")
    for B, T in DECODE_SHAPES:
        g = torch.Generator(device=dev).manual_seed(B + T)
        kc = torch.randn(LAYERS, B, H, TMAX, D, generator=g, device=dev, dtype=torch.bfloat16)
        vc = torch.randn(LAYERS, B, H, TMAX, D, generator=g, device=dev, dtype=torch.bfloat16)
        (kq, ks), (vq, vs) = quantised(kc), quantised(vc)
        qkv = torch.randn(B, 3, H, D, generator=g, device=dev, dtype=torch.bfloat16)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)

        def bf16():
            for i in range(LAYERS):
                rf.attn_decode(qkv, kc[i], vc[i], lens)

        def int8():
            for i in range(LAYERS):
                rf.attn_decode(qkv, kq[i], vq[i], lens, k_scale=ks[i], v_scale=vs[i])

        diff = float((rf.attn_decode(qkv, kq[0], vq[0], lens, k_scale=ks[0], v_scale=vs[0]).float()
                      - rf.attn_decode(qkv, kc[0], vc[0], lens).float()).abs().max())
        us = time_paths({"bf16": bf16, "int8": int8}, a, LAYERS)
        keys = B * H * (T + 1) * 2
        emit({"part": "decode", "B": B, "Tcache": T, "us": us,
              "splits": _lib.lib().ra_attn_decode_splits(B, H, TMAX),
              "bf16_GBps": keys * 2 * D / us["bf16"]["median"] * 1e-3,
              "int8_GBps": keys * (D + 4) / us["int8"]["median"] * 1e-3,
              "int8_vs_bf16": us["bf16"]["median"] / us["int8"]["median"],
              "max_abs_out_diff": diff})
        del kc, vc, kq, vq, ks, vs
        torch.cuda.empty_cache()


def insert_part(a, emit):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    shape = (LAYERS, INSERT_SLOTS, H, TMAX, D)
    kc = torch.zeros(shape, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    kq = torch.zeros(shape, dtype=torch.int8, device=dev)
    vq = torch.zeros_like(kq)
    ks = torch.zeros(shape[:-1], dtype=torch.float32, device=dev)
    vs = torch.zeros_like(ks)
    for Bn, T in INSERT_SHAPES:
        qkv = torch.randn(Bn, T, 3, H, D, generator=g).bfloat16().to(dev)
        slots = torch.randperm(INSERT_SLOTS, generator=g)[:Bn].to(dev, torch.int32)
        lens = torch.full((Bn,), T, dtype=torch.int32, device=dev)

        def bf16():
            for i in range(LAYERS):
                rf.kv_insert(qkv, kc[i], vc[i], slots, lens)

        def int8():
            for i in range(LAYERS):
                rf.kv_insert(qkv, kq[i], vq[i], slots, lens, k_scale=ks[i], v_scale=vs[i])

        us = time_paths({"bf16": bf16, "int8": int8}, a, 1)
        vectors = 2 * LAYERS * Bn * T * H
        emit({"part": "insert", "Bn": Bn, "T": T, "us_12_layers": us,
              "bf16_GBps": vectors * 4 * D / us["bf16"]["median"] * 1e-3,
              "int8_GBps": vectors * (3 * D + 4) / us["int8"]["median"] * 1e-3,
              "int8_vs_bf16": us["bf16"]["median"] / us["int8"]["median"]})


def engine_part(a, emit):
    from gpt2_engine_bench import make_requests, run_engine

    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    reqs = make_requests(a.requests, model.cfg.vocab_size)
    requested = sum(r["new"] for r in reqs)
    max_len = max(len(r["tokens"]) for r in reqs) + max(r["new"] for r in reqs)
    for S in (8, 64):
        engines = {kv: GPT2Engine(model, slots=S, max_len=max_len, poll_every=8,
                                  **({} if kv == "none" else {"kv_cache": kv}))
                   for kv in a.kv_cache}
        runs = {kv: [] for kv in engines}
        for rep in range(a.repeats + 1):  # the first round warms up
            for kv, eng in engines.items():
                r = run_engine(eng, reqs, 0.8, 50)
                if rep:
                    runs[kv].append(requested / r["wall"])
        for kv, eng in engines.items():
            c = eng.cache
            nbytes = sum(t.numel() * t.element_size()
                         for t in (c.k, c.v, getattr(c, "k_scale", None),
                                   getattr(c, "v_scale", None)) if t is not None)
            emit({"part": "engine", "tree": a.tree, "S": S, "kv_cache": kv, "max_len": max_len,
                  "requested_tokens": requested, "tok_per_s": stats(runs[kv]),
                  "cache_bytes": nbytes})
        del engines
        torch.cuda.empty_cache()


def drift_part(a, emit):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = GPT2(GPT2Config.small()).to(dev, torch.bfloat16).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (8, 64),
                        generator=torch.Generator().manual_seed(1)).to(dev)
    lens = torch.full((8,), 64, dtype=torch.int32, device=dev)
    logits = {}
    for quant in (None, "int8"):
        cache = KVCache(model.cfg, 8, 128, dev, torch.bfloat16, quant=quant)
        tok = model.prefill(idx, lens, cache).argmax(-1)  # (the prompt pass reads no cache)
        logits[quant] = model.decode_step(tok, cache).float()
    emit({"part": "drift", "max_abs_logit_diff": float((logits["int8"] - logits[None]).abs().max()),
          "max_abs_logit": float(logits[None].abs().max()),
          "argmax_equal_rows": int((logits["int8"].argmax(-1) == logits[None].argmax(-1)).sum()),
          "rows": 8})


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("kv_q8_bench needs a GPU: timings are device timings")
    fh = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    {"decode": decode_part, "insert": insert_part, "engine": engine_part,
     "drift": drift_part}[a.part](a, emit)


if __name__ == "__main__":
    main()
