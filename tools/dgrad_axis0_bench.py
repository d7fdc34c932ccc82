#!/usr/bin/env python3
"""Same-process A/B of the two routes of the backward of an AXIS-0 layer with respect to its input, dx = g @ dequantize(W_q, axis=0) (needs an MI355X):
ops.gemm_dgrad_axis0 — the fused kernel hqq_hip_gemm_dgrad_axis0 — against the route it replaces, ops.dequantize(axis=0) + torch.matmul(g, W) (what
HQQLinear._matmul_hip(transpose=False) has always run for such a layer).

    python tools/dgrad_axis0_bench.py [--out FILE.json] [--reps 7] [--window-ms 40] [--rows 1,16,...]

Shapes: int4 group_size 64 fp16 at (N, K) = (4096, 4096), (11008, 4096), (4096, 11008); M in 1, 2, 4, 8, 16, 32, 64, 128, 256, 1024.
The timing protocol is tools/dgrad_bench.py's.  Every layer exists in enough copies (random packed bytes, random meta) to exceed the 256 MB
last-level cache, and consecutive calls take consecutive copies: as in a model, a layer's packed bytes come from HBM.  Each route is captured ONCE per
(shape, M) as a HIP graph of one call per copy, so the timed window holds device time and no Python; a repetition replays that graph until `window-ms`
have passed (replay count fixed from a probe), timed with device events.  After a warm-up of both routes, `reps` repetitions ALTERNATE between them.
Reported per case: the median and the spread (max - min) of each route in microseconds per call, the ratio old / new of the medians, the largest
difference of the two outputs, and the peak of torch.cuda.max_memory_allocated over one eager call of each route above what was allocated before it
(the old route's transient weight shows there).  Last line: the largest M up to which the kernel is at least 10 % faster on every shape at every
measured M (0 if it is not at M = 1) — the value for ops.DGRAD_AXIS0_ROUTE_MAX_M."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(4, torch.float16, 4096, 4096), (4, torch.float16, 11008, 4096), (4, torch.float16, 4096, 11008)]
ROWS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 1024]
GS = 64
CACHE_BYTES = 320 << 20


def make_layers(nbits, dt, N, K, gen):
    per = 8 // nbits
    one = N // per * K + 2 * 2 * (N * K // GS)
    n = -(-CACHE_BYTES // one)
    layers = []
    for _ in range(n):
        Wq = torch.randint(0, 256, (N // per, K), dtype=torch.uint8, device="cuda", generator=gen)
        s = (torch.rand(N * K // GS, device="cuda", generator=gen) * 0.004 + 0.001).to(dt)
        z = (torch.rand(N * K // GS, device="cuda", generator=gen) * (2 ** nbits - 1)).to(dt)
        layers.append((Wq, s, z))
    return layers


def capture(fn, layers):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # eager first: libraries have picked their kernels
        for L in layers:
            fn(L)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for L in layers:
            fn(L)
    return g


def time_replays(g, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)   # ms


def peak_above(fn, L):
    """bytes one eager call holds at its peak above what was allocated when it started"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(L)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/dgrad_axis0_bench.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--rows", default=",".join(str(m) for m in ROWS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dgrad_axis0_bench: needs the GPU")
    from hqq_amd import ops
    Ms = [int(m) for m in a.rows.split(",")]
    gen = torch.Generator(device="cuda").manual_seed(20251)
    rows = []
    for nbits, dt, N, K in CASES:
        layers = make_layers(nbits, dt, N, K, gen)
        for M in Ms:
            x = torch.randn(M, N, device="cuda", dtype=dt, generator=gen)
            y_new = torch.empty(M, K, device="cuda", dtype=dt)
            y_old = torch.empty(M, K, device="cuda", dtype=dt)

            def new(L):
                ops.gemm_dgrad_axis0(x, L[0], L[1], L[2], N, K, GS, nbits, out=y_new)

            def old(L):
                W = ops.dequantize(L[0], L[1], L[2], N, K, GS, nbits, 0)
                torch.matmul(x, W, out=y_old)

            peak = {"new": peak_above(new, layers[0]), "old": peak_above(old, layers[0])}
            graphs = {"new": capture(new, layers), "old": capture(old, layers)}
            torch.cuda.synchronize()
            diff = float((y_new.float() - y_old.float()).abs().max())   # both hold the last copy's output
            n_rep = {r: max(1, int(a.window_ms / max(time_replays(g, 2) / 2, 1e-3))) for r, g in graphs.items()}   # (probe = second warm-up)
            us = {"new": [], "old": []}
            for _ in range(a.reps):   # interleaved
                for r in ("new", "old"):
                    us[r].append(time_replays(graphs[r], n_rep[r]) * 1e3 / (n_rep[r] * len(layers)))
            med = {r: statistics.median(v) for r, v in us.items()}
            row = {"nbits": nbits, "dtype": str(dt).replace("torch.", ""), "N": N, "K": K, "M": M, "copies": len(layers),
                   "new_us": round(med["new"], 2), "new_spread_us": round(max(us["new"]) - min(us["new"]), 2),
                   "old_us": round(med["old"], 2), "old_spread_us": round(max(us["old"]) - min(us["old"]), 2),
                   "old_over_new": round(med["old"] / med["new"], 3), "max_abs_diff": diff,
                   "new_peak_bytes": peak["new"], "old_peak_bytes": peak["old"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del graphs
        del layers
        torch.cuda.empty_cache()
    wins = [M for M in Ms if all(r["old_over_new"] >= 1.10 for r in rows if r["M"] == M)]
    cut = 0
    for M in Ms:   # the largest M up to which every measured M wins; 0 if the first does not
        if M in wins:
            cut = M
        else:
            break
    res = {"tool": "dgrad_axis0_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "window_ms": a.window_ms, "group_size": GS,
           "rows": rows, "wins_by_10_percent_on_every_shape": wins, "DGRAD_AXIS0_ROUTE_MAX_M": cut}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wins_by_10_percent_on_every_shape": wins, "DGRAD_AXIS0_ROUTE_MAX_M": cut}))


if __name__ == "__main__":
    main()
