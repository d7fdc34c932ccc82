#!/usr/bin/env python3
"""Same-process A/B of the two routes HQQLinearLoRA.merge_and_quantize has for the merged weight of a quantised layer (needs an MI355X):
ops.lora_merge — the fused kernel hqq_hip_lora_merge — against the torch composition the wrapper runs with HQQLinearLoRA.fused_merge = False,
`W = dequantize(W_q); W += (torch.matmul(A, B) * scaling).t().to(W.dtype)`.

    python tools/lora_merge_bench.py [--out FILE.json] [--reps 7] [--window-ms 40]

Shapes: int4 group_size 64 fp16 at (N, K) = (4096, 4096), (11008, 4096), (4096, 11008); axis 1 and 0; an fp32 adapter of rank 8 and 64.
Merge alone — the timing protocol of tools/dgrad_bench.py: every layer exists in enough copies (random packed bytes, random meta) to exceed the 256 MB
last-level cache, consecutive calls take consecutive copies; each route is captured ONCE per case as a HIP graph of one call per copy, so the timed
window holds device time and no Python; a repetition replays that graph until `window-ms` have passed (replay count fixed from a probe), timed with
device events; after a warm-up of both routes, `reps` repetitions ALTERNATE between them.
Merge + the quantise that follows (ops.quantize on the merged weight: what merge_and_quantize does next) — eager calls over the copies between two
device events, the same alternation; the solver takes milliseconds per layer, so the host's share of such a call does not show.
Peak transient memory: torch.cuda.max_memory_allocated() over one eager call of each route, above what was allocated before the call (the merged
weight itself, 2 N K bytes, is part of both).
Reported per case: median and spread (max - min) of each route in microseconds per call, the ratio composed / fused of the medians, the two peaks
in MiB, and whether the two merged weights have the same bits (a library GEMM sums in its own order: a handful of last-bit differences is expected)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]
RANKS = [8, 64]
NBITS, GS, DT = 4, 64, torch.float16
SCALING = 2.0
CACHE_BYTES = 320 << 20


def make_layers(N, K, gen):
    one = N * K // 2 + 2 * 2 * (N * K // GS)
    n = -(-CACHE_BYTES // one)
    layers = []
    for _ in range(n):
        Wq = torch.randint(0, 256, (N * K // 2,), dtype=torch.uint8, device="cuda", generator=gen)
        s = (torch.rand(N * K // GS, device="cuda", generator=gen) * 0.004 + 0.001).to(DT)
        z = (torch.rand(N * K // GS, device="cuda", generator=gen) * (2 ** NBITS - 1)).to(DT)
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


def timed(run, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)   # ms


def ab(runs, calls_per_run, reps, window_ms):
    """runs: {route: callable}; alternating repetitions -> {route: [us per call]}"""
    n_rep = {r: max(1, int(window_ms / max(timed(f, 2) / 2, 1e-3))) for r, f in runs.items()}   # (probe = second warm-up)
    us = {r: [] for r in runs}
    for _ in range(reps):
        for r, f in runs.items():
            us[r].append(timed(f, n_rep[r]) * 1e3 / (n_rep[r] * calls_per_run))
    return us


def peak_mib(fn, L):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(L)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return round(peak / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/lora_merge_bench.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="only the first so many shapes (a rehearsal)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_merge_bench: needs the GPU")
    from hqq_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(20251)
    rows = []
    for N, K in SHAPES[:a.shapes]:
        layers = make_layers(N, K, gen)
        for axis in (1, 0):
            for r in RANKS:
                A = (torch.randn(K, r, device="cuda", generator=gen) * 0.05)
                B = (torch.randn(r, N, device="cuda", generator=gen) * 0.05)
                w_new = torch.empty(N, K, device="cuda", dtype=DT)

                def fused(L, out=None):
                    return ops.lora_merge(L[0], L[1], L[2], N, K, GS, NBITS, axis, A, B, SCALING, out=out)

                def composed(L):
                    W = ops.dequantize(L[0], L[1], L[2], N, K, GS, NBITS, axis)
                    W += (torch.matmul(A, B) * SCALING).t().to(W.dtype)
                    return W

                def fused_q(L):
                    return ops.quantize(fused(L), nbits=NBITS, group_size=GS, axis=axis)

                def composed_q(L):
                    return ops.quantize(composed(L), nbits=NBITS, group_size=GS, axis=axis)

                differing = int((fused(layers[-1]).view(torch.int16) != composed(layers[-1]).view(torch.int16)).sum())
                peaks = {"fused": peak_mib(fused, layers[0]), "composed": peak_mib(composed, layers[0]),
                         "fused_q": peak_mib(fused_q, layers[0]), "composed_q": peak_mib(composed_q, layers[0])}
                graphs = {"fused": capture(lambda L: fused(L, out=w_new), layers), "composed": capture(composed, layers)}
                torch.cuda.synchronize()
                us = ab({k: g.replay for k, g in graphs.items()}, len(layers), a.reps, a.window_ms)
                del graphs
                few = layers[:4]
                for f in (fused_q, composed_q):   # warm-up
                    f(few[0])
                us_q = ab({"fused_q": lambda: [fused_q(L) for L in few], "composed_q": lambda: [composed_q(L) for L in few]}, len(few), a.reps,
                          a.window_ms)
                us.update(us_q)
                med = {k: statistics.median(v) for k, v in us.items()}
                row = {"N": N, "K": K, "axis": axis, "r": r, "copies": len(layers)}
                for k in ("fused", "composed", "fused_q", "composed_q"):
                    row[k + "_us"] = round(med[k], 1)
                    row[k + "_spread_us"] = round(max(us[k]) - min(us[k]), 1)
                    row[k + "_peak_mib"] = peaks[k]
                row["composed_over_fused"] = round(med["composed"] / med["fused"], 2)
                row["composed_q_over_fused_q"] = round(med["composed_q"] / med["fused_q"], 3)
                row["merged_weight_mib"] = round(2 * N * K / 2 ** 20, 1)
                row["fused_write_gb_s"] = round(2 * N * K / (med["fused"] * 1e-6) / 1e9, 1)   # the merged weight's bytes over the fused call's time
                row["elements_differing"] = differing
                rows.append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
        del layers
        torch.cuda.empty_cache()
    res = {"tool": "lora_merge_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "window_ms": a.window_ms,
           "nbits": NBITS, "group_size": GS, "dtype": str(DT).replace("torch.", ""), "adapter_dtype": "float32", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
