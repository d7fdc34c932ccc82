"""Same-process A/B of the decode routes of an AXIS-0 layer (needs the GPU; prints one JSON line).

On one level matrix per shape (fp16, group_size 64, int4 and int2, the Llama-2-7B linear shapes, M in {1, 4, 16}) it times
  axis0   hqq_hip_gemv_axis0 on the axis-0 container + [1, N K / 64] meta (the new kernel, csrc/gemv_axis0.hip)
  deq_mm  today's axis-0 route: hqq_hip_dequantize(axis = 0) into an fp16 [N, K] + torch.matmul
  axis1   hqq_hip_gemv on the axis-1 layout of the same bytes (the container is identical; the meta is [N K / 64] per-row groups)
Each variant is captured as one hipGraph of `calls` launches that rotate over enough copies of the layer to exceed the 256 MB
infinity cache, so the bytes come from HBM; a replay is timed with device events.  GB/s use the algorithmic bytes of SURVEY.md
section 8(d): packed weights + fp16 scale and zero + x + y (0.5625 B/param at int4), against 8 TB/s.

    python tools/axis0_decode_bench.py [--out FILE] [--iters 5]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hqq_amd import ops  # noqa: E402

HBM_TBS = 8.0
SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]   # (N, K): q/k/v/o, gate/up, down of Llama-2-7B


def alg_bytes(N, K, gs, nbits, M):
    return N * K * nbits // 8 + 2 * 2 * (N * K // gs) + 2 * M * K + 2 * M * N


def time_graph(fn, calls: int, iters: int) -> float:
    """µs per call: `calls` launches of fn(i) captured in one graph, the median of `iters` timed replays"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(3):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(calls):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / calls)
    del g
    return sorted(ts)[len(ts) // 2]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--nbits", type=int, nargs="*", default=[4, 2])
    ap.add_argument("--M", type=int, nargs="*", default=[1, 4, 16])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("axis0_decode_bench: needs the GPU")
    dev, gs, dt = torch.device("cuda"), 64, torch.float16
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for nbits in args.nbits:
        per = 8 // nbits
        for N, K in SHAPES:
            C = N * K // gs
            packed_bytes = N * K // per
            copies = max(2, min(64, math.ceil(512e6 / (packed_bytes + 4 * C))))
            L = torch.randint(0, 2 ** nbits, (gs, C), device=dev, dtype=torch.uint8, generator=gen)
            P = ops.pack(nbits, L)                               # the axis-0 container: [gs / per, C] bytes == the axis-1 [N / per, K]
            del L
            Ws = [P.clone() for _ in range(copies)]
            s0 = [(torch.rand(1, C, device=dev, generator=gen) * 0.004 + 0.001).to(dt) for _ in range(copies)]
            z0 = [(torch.rand(1, C, device=dev, generator=gen) * (2 ** nbits - 1)).to(dt) for _ in range(copies)]
            W1 = [w.view(N // per, K) for w in Ws]
            for M in args.M:
                x = torch.randn(M, K, device=dev, generator=gen).to(dt)
                y = torch.empty(M, N, device=dev, dtype=dt)
                f_a0 = lambda i: ops.gemv_axis0(x, Ws[i % copies], s0[i % copies], z0[i % copies], None, N, K, gs, nbits, out=y)   # noqa: E731

                def f_dm(i):
                    W = ops.dequantize(Ws[i % copies], s0[i % copies].reshape(-1), z0[i % copies].reshape(-1), N, K, gs, nbits, 0)
                    return torch.matmul(x, W.t())

                f_a1 = lambda i: ops.gemv(x, W1[i % copies], s0[i % copies].reshape(-1), z0[i % copies].reshape(-1), None, N, K, gs, nbits, out=y, opts=0)   # noqa: E731
                # same numbers from the new kernel and today's route (same weights, fp32 vs library accumulation)
                ref = f_dm(0)
                got = f_a0(0).clone()
                err = float((got.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-6))
                calls = 4 * copies
                t_a0, t_dm, t_a1 = (time_graph(f, calls, args.iters) for f in (f_a0, f_dm, f_a1))
                B = alg_bytes(N, K, gs, nbits, M)
                rows.append({"nbits": nbits, "N": N, "K": K, "M": M, "gs": gs, "copies": copies,
                             "us_axis0": round(t_a0, 2), "us_dequant_matmul": round(t_dm, 2), "us_axis1_gemv": round(t_a1, 2),
                             "speedup_vs_dequant_matmul": round(t_dm / t_a0, 2), "ratio_axis0_over_axis1": round(t_a0 / t_a1, 2),
                             "alg_bytes": B, "GBs_axis0": round(B / t_a0 / 1e3, 1), "GBs_axis1": round(B / t_a1 / 1e3, 1),
                             "hbm_frac_axis0": round(B / t_a0 / 1e3 / (HBM_TBS * 1e3), 3), "max_rel_diff_vs_dequant_matmul": err})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            del Ws, s0, z0, W1, P
            torch.cuda.empty_cache()
    res = {"tool": "axis0_decode_bench", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "hbm_TBs": HBM_TBS,
           "faster_than_dequant_matmul_everywhere": all(r["us_axis0"] < r["us_dequant_matmul"] for r in rows), "rows": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
