#!/usr/bin/env python3
"""Fused against composed route of HQQExperts on one mixture-of-experts block (needs an MI355X).

Shapes: `mixtral` — Mixtral-8x7B's experts (E 8, k 2, H 4096, I 14336) — and `qwen3moe` — Qwen3-30B-A3B-like (E 64, k 8, H 2048, I 768).  Configurations:
int4 group_size 64 and int2 group_size 16, fp16.  T in {1, 2, 4, 8, 16}.  Routing: `random` (k distinct experts per token) and `same` (every token on
the same k experts).  The stacks hold random levels, scales and zero-points (nothing is quantised: the time does not depend on the values); the routing
changes from call to call over a fixed cycle of 8 seeded routings, so that a call does not find the previous call's experts in the caches.

    python tools/moe_bench.py [--shapes mixtral,qwen3moe] [--configs 4:64,2:16] [--passes 2] [--limit 240] [--out profiles/moe_bench.json] [--md profiles/moe_summary.md]
        The driver.  EVERY (shape, configuration, route) measurement runs in a process of its own under its own time limit (--limit seconds) and times all
        T and both routings: per point a warm-up over the routing cycle, then calls for at least --window seconds between device synchronisations (host
        clock).  The two routes are alternated `passes` times so that the spread shows.  A child that is killed by a signal or runs into its limit ends
        the whole run (nothing further is started on the GPU); the tables then say what was not measured.
    python tools/moe_bench.py --route fused|composed --shape mixtral --config 4:64     one measurement, one JSON line (what the driver starts)

Bytes: a call needs the packed levels and the constants of the experts it selects, 3 H I (1 / per + 4 / group_size) bytes each.  `GB/s` in the tables is
that over the DISTINCT experts of the call, per call time (both launches); T k experts' bytes (what is read when no two waves share a line in a cache) is in the JSON as `pair_bytes`.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"mixtral": dict(E=8, k=2, H=4096, I=14336), "qwen3moe": dict(E=64, k=8, H=2048, I=768)}
ROUTES = ("composed", "fused")
TS = (1, 2, 4, 8, 16)
ROUTINGS = ("random", "same")
CYCLE = 8


def expert_bytes(H, I, nbits, gs):
    return 3 * H * I // (8 // nbits) + 3 * (H * I // gs) * 4


def build(shape, nbits, gs):
    import torch
    from hqq_amd.core.moe import HQQExperts
    from hqq_amd.core.quantize import BaseQuantizeConfig
    s = SHAPES[shape]
    E, H, I = s["E"], s["H"], s["I"]
    g = torch.Generator(device="cuda").manual_seed(20261)
    per, maxv = 8 // nbits, 2 ** nbits - 1
    stacks, meta = {}, {}
    for role, (N, K) in (("gate", (I, H)), ("up", (I, H)), ("down", (H, I))):
        R = N * K // gs
        stacks[role, "W_q"] = torch.randint(0, 256, (E, R // per, gs), device="cuda", dtype=torch.uint8, generator=g)
        stacks[role, "scale"] = (0.01 * (1.0 + 0.5 * torch.rand((E, R, 1), device="cuda", generator=g))).half()
        stacks[role, "zero"] = (maxv / 2 + 0.5 * torch.randn((E, R, 1), device="cuda", generator=g)).half()
        meta[role] = {"nbits": nbits, "group_size": gs, "shape": torch.Size((N, K)), "axis": 1, "packing": f"{nbits}bit_u8", "unpack_view_dtype": torch.uint8,
                      "view_as_float": False}
    return HQQExperts.from_stacks(stacks, meta, BaseQuantizeConfig(nbits=nbits, group_size=gs, axis=1), compute_dtype=torch.float16, device="cuda")


def routings(kind, T, E, k, gen):
    import torch
    out = []
    for i in range(CYCLE):
        if kind == "same":
            idx = ((torch.arange(k) + i * k) % E).repeat(T, 1)
        else:
            idx = torch.stack([torch.randperm(E, generator=gen)[:k] for _ in range(T)])
        w = torch.rand((T, k), generator=gen) + 0.25
        out.append((idx.to(torch.int64).cuda().contiguous(), (w / w.sum(-1, keepdim=True)).float().cuda().contiguous()))
    return out


def worker(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench: needs the GPU")
    nbits, gs = (int(v) for v in a.config.split(":"))
    s = SHAPES[a.shape]
    q = build(a.shape, nbits, gs)
    fwd = q.forward_fused if a.route == "fused" else q.forward_composed
    gen = torch.Generator().manual_seed(7)
    points = []
    with torch.no_grad():
        for T in TS:
            x = (torch.randn((T, s["H"]), generator=gen) * 0.5).half().cuda()
            assert a.route != "fused" or q.fused_covers(x, torch.zeros((T, s["k"]), dtype=torch.int64, device="cuda"))
            for kind in ROUTINGS:
                cyc = routings(kind, T, s["E"], s["k"], gen)
                for idx, w in cyc:
                    fwd(x, idx, w)
                torch.cuda.synchronize()
                n, t0 = 0, time.perf_counter()
                while True:
                    for idx, w in cyc:
                        fwd(x, idx, w)
                    n += CYCLE
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if dt >= a.window:
                        break
                distinct = statistics.mean(len(set(idx.reshape(-1).tolist())) for idx, _ in cyc)
                eb = expert_bytes(s["H"], s["I"], nbits, gs)
                points.append({"T": T, "routing": kind, "us": round(dt / n * 1e6, 2), "calls": n, "distinct_bytes": int(distinct * eb), "pair_bytes": T * s["k"] * eb})
    print(json.dumps({"shape": a.shape, "config": a.config, "route": a.route, "device": torch.cuda.get_device_name(0), "window_s": a.window, "points": points}), flush=True)


def run_child(cmd, limit):
    """(result dict | None, note): a child that was killed or timed out returns (None, why) and the caller stops starting work"""
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, f"ran into its limit of {limit} s"
    if p.returncode != 0:
        return None, f"exit status {p.returncode}: {(p.stderr or p.stdout)[-300:].strip()}"
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]), ""


def cutoff(res):
    """the largest T <= 16 such that, at it and at every smaller measured T, the fused route's median time is at least 10 % ahead of composed
    (composed / fused >= 1.1) on every measured shape, configuration and routing; 0 when not even T = 1 qualifies; None when nothing was measured"""
    ok = None
    for T in TS:
        ratios = []
        for key, routes in res["cases"].items():
            for kind in ROUTINGS:
                f, c = routes.get("fused", {}).get(f"{T}:{kind}"), routes.get("composed", {}).get(f"{T}:{kind}")
                if not f or not c:
                    return ok
                ratios.append(statistics.median(c) / statistics.median(f))
        if min(ratios) < 1.1:
            return ok if ok is not None else 0
        ok = T
    return ok


def markdown(res) -> str:
    out = ["# Routed expert kernel against the composed route (one MoE block)", "",
           f"`tools/moe_bench.py` on {res.get('device', 'an MI355X')}: `HQQExperts.forward_fused` (two launches, `csrc/moe.hip`) against `HQQExperts.forward_composed` "
           "(HF's loop over the experts hit, `ops.forward` per expert and role), fp16, random stacks.  Every (shape, configuration, route) is a process of its own; "
           f"per point a warm-up over a cycle of {CYCLE} routings, then calls for at least {res['window']} s between device synchronisations.  Cells: microseconds "
           f"per call of each of the {res['passes']} alternating passes; speed-up = median composed / median fused; GB/s = packed levels + constants of the call's "
           "DISTINCT experts over the fused call time (both launches).", ""]
    for key, routes in res["cases"].items():
        shape, config = key.split("/")
        s = SHAPES[shape]
        out += [f"## {shape} (E {s['E']}, k {s['k']}, H {s['H']}, I {s['I']}), int{config.split(':')[0]} group_size {config.split(':')[1]}", "",
                "| T | routing | composed us | fused us | speed-up | fused GB/s (distinct experts) |", "|---|---|---|---|---|---|"]
        for T in TS:
            for kind in ROUTINGS:
                c, f = routes.get("composed", {}).get(f"{T}:{kind}"), routes.get("fused", {}).get(f"{T}:{kind}")
                cell = lambda v: ", ".join(f"{x:.1f}" for x in v) if v else "not measured"
                ratio = f"{statistics.median(c) / statistics.median(f):.2f}" if c and f else "not measured"
                b = res["bytes"].get(key, {}).get(f"{T}:{kind}")
                gbs = f"{b / (statistics.median(f) * 1e-6) / 1e9:.0f}" if f and b else "not measured"
                out.append(f"| {T} | {kind} | {cell(c)} | {cell(f)} | {ratio} | {gbs} |")
        out.append("")
    co = cutoff(res)
    out += ["## Cut-off", "",
            "Rule: `ops.MOE_ROUTE_MAX_T` is the largest T <= 16 such that, at it and at every smaller measured T, the fused route is at least 10 % ahead of the "
            "composed route (median composed / median fused >= 1.1) on every measured shape, configuration and routing.", "",
            f"Measured cut-off: {'not measured' if co is None else co}.", ""]
    if res.get("stopped"):
        out += [f"The run was stopped: {res['stopped']}  Nothing was started after it; cells above say what was not measured.", ""]
    return "\n".join(out)


def driver(a):
    shapes, configs = a.shapes.split(","), a.configs.split(",")
    res = {"tool": "moe_bench", "passes": a.passes, "window": a.window, "cases": {f"{s}/{c}": {} for s in shapes for c in configs}, "bytes": {}, "stopped": ""}
    plan = [(s, c, r) for _ in range(a.passes) for s in shapes for c in configs for r in ROUTES]
    for s, c, r in plan:
        got, why = run_child([sys.executable, os.path.abspath(__file__), "--route", r, "--shape", s, "--config", c, "--window", str(a.window)], a.limit)
        if got is None:
            res["stopped"] = f"{s} / {c} / {r}: {why}."
            break
        res["device"] = got["device"]
        for p in got["points"]:
            res["cases"][f"{s}/{c}"].setdefault(r, {}).setdefault(f"{p['T']}:{p['routing']}", []).append(p["us"])
            res["bytes"].setdefault(f"{s}/{c}", {})[f"{p['T']}:{p['routing']}"] = p["distinct_bytes"]
            res.setdefault("pair_bytes", {}).setdefault(f"{s}/{c}", {})[f"{p['T']}:{p['routing']}"] = p["pair_bytes"]
        print(json.dumps({"done": [s, c, r]}), flush=True)
    res["cutoff"] = cutoff(res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))
    print(json.dumps({"written": a.out, "stopped": res["stopped"], "cutoff": res["cutoff"]}))
    return 1 if res["stopped"] else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=ROUTES, default=None)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="mixtral")
    ap.add_argument("--config", default="4:64")
    ap.add_argument("--shapes", default="mixtral,qwen3moe")
    ap.add_argument("--configs", default="4:64,2:16")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default="profiles/moe_bench.json")
    ap.add_argument("--md", default="profiles/moe_summary.md")
    a = ap.parse_args()
    if a.route:
        worker(a)
        return 0
    return driver(a)


if __name__ == "__main__":
    sys.exit(main())
