#!/usr/bin/env python3
"""Decode attention per KV-head group (gqa_attention="group", csrc/attn_gqa.hip) against the per-head kernels ("heads") on grouped-query shapes (needs an
MI355X).  The house method of tools/kvq_bench.py: every leg runs in a PROCESS OF ITS OWN, the driver goes through all legs twice, alternating the modes, and the
tables give medians over both passes with min - max.  Nothing here decides a route: the feature is opt-in and the default does not depend on these numbers.

    python tools/gqa_attn_bench.py [--parts attn,sweep,step] [--shapes 32x8,28x4,64x8] [--formats dense,q8,q4] [--models llama,qwen3]
                                   [--out profiles/gqa_attn_bench.json] [--md profiles/gqa_attn_summary.md]
        the driver: starts the legs below one after another, merges them into the JSON record (parts that were not run keep what the file held) and renders
        the tables; what the record does not hold is listed as not measured
    python tools/gqa_attn_bench.py --leg attn --mode heads|group --shape 32x8 --format dense|q8|q4
        the attention launch alone, fp16, head_dim 128, B = 1 / 8 / 16 at 256 / 1024 / 4096 / 16384 visible positions (the cache holds exactly that many):
        "heads" is ops.attn_decode_batched / ops.attn_decode_kvq_batched with ops.attn_splits, "group" ops.attn_decode_gqa_batched / _gqa_kvq_batched with
        ops.attn_gqa_splits.  Timed over a ROTATION of independent caches — as many as a 32-layer model holds, fewer where 32 do not fit in `--rotation-gib` — a
        captured graph of one rotation replayed between two HIP events; us per launch (a split call includes its merging launch).
    python tools/gqa_attn_bench.py --leg sweep --shape 32x8 --format dense|q8|q4
        the grouped launch at every split count in 1, 2, 4, 8, 16, 32, 64 that the context allows (S <= positions): what ops.attn_gqa_splits' rule is read off
    python tools/gqa_attn_bench.py --leg step --mode heads|group --model llama|qwen3
        the whole captured decode step of a random-weight model, int4 group_size 64, `--blocks` decoder blocks: "llama" is Llama-3-8B-shaped (hidden 4096, 32 / 8
        heads of 128, intermediate 14336, vocab 128256 — the Llama-family dense case, which pays one more launch per block under "group"), "qwen3" Qwen3-8B-shaped
        (hidden 4096, 32 / 8 heads of 128, intermediate 12288, vocab 151936; qk_norm="fused").  GraphedGreedyDecoder(attention="hip", gqa_attention=mode),
        B = 1 / 8 / 16 after prompts of 256 / 3000 tokens on a cache of 4096: ms per step of `--steps` timed graph replays (benchmark_batch).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("heads", "group")
FORMATS = ("dense", "q8", "q4")
SHAPES = ("32x8", "28x4", "64x8")
MODELS = ("llama", "qwen3")
HD, GS = 128, 64
POSITIONS = (256, 1024, 4096, 16384)
BATCHES = (1, 8, 16)
CONTEXTS = (256, 3000)
SWEEP = (1, 2, 4, 8, 16, 32, 64)


def _shape(s):
    h, k = s.split("x")
    return int(h), int(k)


def kv_bytes(fmt: str, B: int, n_kv: int, n: int) -> int:
    """the bytes of K and V of n visible positions of B sequences (what a launch that reads each row once must read)"""
    row = HD * 2 if fmt == "dense" else HD * int(fmt[1]) // 8 + 2 * 2 * (HD // GS)
    return 2 * B * n_kv * n * row


def _caches(torch, ops, fmt, B, n_kv, n, copies, g):
    out = []
    for _ in range(copies):
        if fmt == "dense":
            out.append(tuple(torch.randn(B, n_kv, n, HD, device="cuda", generator=g, dtype=torch.float16) for _ in range(2)))
            continue
        bufs = ops.kv_alloc(B, n_kv, n, HD, int(fmt[1]), GS, torch.float16, "cuda")
        for b in range(B):   # (row by row: the dense source of one sequence is a transient)
            k, v = (torch.randn(1, n_kv, n, HD, device="cuda", generator=g, dtype=torch.float16) for _ in range(2))
            ops.kv_quantize(k, v, tuple(t[b:b + 1] for t in bufs), start=0)
        out.append(bufs)
    return out


def _time_rotation(torch, rotation, copies, reps):
    rotation()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rotation()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rotation()
    replays = max(2, 200 // copies)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(round(e0.elapsed_time(e1) * 1e3 / (replays * copies), 2))
    return us


def _launcher(ops, mode, fmt, q, o, pos, splits, ws):
    if fmt == "dense":
        fn = ops.attn_decode_gqa_batched if mode == "group" else ops.attn_decode_batched
        return lambda c: fn(q, c[0], c[1], pos, o, HD ** -0.5, splits=splits, workspace=ws)
    fn = ops.attn_decode_gqa_kvq_batched if mode == "group" else ops.attn_decode_kvq_batched
    return lambda c: fn(q, c, pos, o, HD ** -0.5, HD, splits=splits, workspace=ws)


def leg_attn(a, sweep: bool):
    import torch
    from hqq_amd import ops
    n_heads, n_kv = _shape(a.shape)
    g = torch.Generator(device="cuda").manual_seed(7)
    out = {}
    for B in BATCHES:
        for n in POSITIONS:
            per = kv_bytes(a.format, B, n_kv, n)
            copies = max(1, min(32, int(a.rotation_gib * (1 << 30)) // max(per, 1)))
            q = (torch.randn(B, n_heads * HD, device="cuda", generator=g) * 0.5).half()
            o = torch.empty_like(q)
            pos = torch.full((B,), n - 1, dtype=torch.int64, device="cuda")
            caches = _caches(torch, ops, a.format, B, n_kv, n, copies, g)
            rule = ops.attn_gqa_splits(n, B, n_kv) if (sweep or a.mode == "group") else ops.attn_splits(n)
            point = {"bytes": per, "caches": copies, "rule": rule}
            for S in ([s for s in SWEEP if s <= n] if sweep else [rule]):
                ws = ops.attn_workspace_batched("cuda", B, n_heads, HD, S)
                launch = _launcher(ops, "group" if sweep else a.mode, a.format, q, o, pos, S, ws)
                us = _time_rotation(torch, lambda: [launch(c) for c in caches], copies, a.reps)
                if sweep:
                    point.setdefault("us_by_splits", {})[str(S)] = us
                else:
                    point.update({"us": us, "splits": S})
            out[f"B{B}-n{n}"] = point
            del caches
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"points": out, "device": torch.cuda.get_device_name(0)}), flush=True)


def leg_step(a):
    import torch
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    if a.model == "llama":
        from transformers import LlamaConfig as Cfg, LlamaForCausalLM as Model
        cfg = Cfg(hidden_size=4096, intermediate_size=14336, num_hidden_layers=a.blocks, num_attention_heads=32, num_key_value_heads=8, vocab_size=128256,
                  max_position_embeddings=4096)
        opt_in = {}
    else:
        from transformers import Qwen3Config as Cfg, Qwen3ForCausalLM as Model
        cfg = Cfg(hidden_size=4096, intermediate_size=12288, num_hidden_layers=a.blocks, num_attention_heads=32, num_key_value_heads=8, head_dim=128, vocab_size=151936,
                  max_position_embeddings=4096)
        opt_in = {"qk_norm": "fused"}
    dflt = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    torch.manual_seed(20250)
    try:
        with torch.device("cuda"):
            model = Model(cfg).eval()
    finally:
        torch.set_default_dtype(dflt)
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=torch.float16, device="cuda")
    prepare_for_inference(model, backend="hip")
    group_llama_projections(model)
    out = {}
    for B in BATCHES:
        dec = GraphedGreedyDecoder(model, max_cache_len=4096, attention="hip", gqa_attention=a.mode, **opt_in)
        assert dec.variant is not None and dec.gqa_grouped == (a.mode == "group")
        for T in CONTEXTS:
            ids = torch.randint(0, 32000, (B, T), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
            dec.benchmark_batch(ids, new_tokens=a.steps, warmup=a.warmup)   # warm-up: captures the graphs
            ms = [round(dec.benchmark_batch(ids, new_tokens=a.steps, warmup=a.warmup)["ms_per_step"], 4) for _ in range(a.reps)]
            step = dec.step if B == 1 else dec._batch[B]["step"]
            assert step is not None and step.gqa_attention == a.mode, "the fused step must serve both modes"
            out[f"B{B}-T{T}"] = {"ms": ms}
        del dec
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"points": out, "device": torch.cuda.get_device_name(0)}), flush=True)


def _child(a, leg, **kw):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--blocks", str(a.blocks), "--reps", str(a.reps), "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--rotation-gib", str(a.rotation_gib)]
    for k, v in kw.items():
        cmd += ["--" + k, v]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        raise SystemExit(f"gqa_attn_bench: leg {leg} {kw} failed (rc={res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    print(leg, kw, "done", flush=True)
    return json.loads(lines[-1][len("RESULT "):])


def _stat(vals):
    return statistics.median(vals), min(vals), max(vals)


def markdown(res) -> str:
    rows = ["# Decode attention per KV-head group against per query head", "",
            f"`tools/gqa_attn_bench.py` on {res.get('device', '?')}.  Every leg in a process of its own; two passes that alternate the modes; per leg {res.get('reps', '?')} "
            "repetitions; medians over both passes with min - max.  `\"group\"` is opt-in (`gqa_attention=\"group\"`) and the default does not change whatever these "
            "numbers are.  A ratio below 1 means `\"group\"` is faster; every ratio is against `\"heads\"` measured in the same run."]
    missing = []
    attn = res.get("attn", {})
    if attn:
        rows += ["", "## The attention launch alone", "",
                 f"fp16, head_dim {HD}, quantised caches at group size {GS}; the cache holds exactly the visible positions.  `\"heads\"`: `ops.attn_decode_batched` / "
                 "`ops.attn_decode_kvq_batched` with `ops.attn_splits`; `\"group\"`: `ops.attn_decode_gqa_batched` / `ops.attn_decode_gqa_kvq_batched` with "
                 f"`ops.attn_gqa_splits`.  Timed over a rotation of independent caches (as many as a 32-layer model holds, fewer where 32 do not fit in "
                 f"{res.get('rotation_gib', '?')} GiB), a captured graph of one rotation replayed between two HIP events; us per launch, merging launch included.", "",
                 "| heads | cache | B | positions | caches | heads: splits | us (min - max) | group: splits | us (min - max) | group / heads |", "|---|---|---|---|---|---|---|---|---|---|"]
    for shape in SHAPES:
        for fmt in FORMATS:
            legs = attn.get(f"{shape}-{fmt}")
            if not legs or not all(legs.get(m) for m in MODES):
                missing.append(f"the attention launch, {shape} heads, {fmt} cache")
                continue
            for B in BATCHES:
                for n in POSITIONS:
                    key = f"B{B}-n{n}"
                    st = {m: _stat([v for p in legs[m] for v in p[key]["us"]]) for m in MODES}
                    p0 = {m: legs[m][0][key] for m in MODES}
                    rows.append(f"| {shape.replace('x', ' / ')} | {fmt} | {B} | {n} | {p0['heads']['caches']} | {p0['heads']['splits']} | {st['heads'][0]:.1f} ({st['heads'][1]} - "
                                f"{st['heads'][2]}) | {p0['group']['splits']} | {st['group'][0]:.1f} ({st['group'][1]} - {st['group'][2]}) | {st['group'][0] / st['heads'][0]:.2f} |")
    sweep = res.get("sweep", {})
    if sweep:
        rows += ["", "## The split count of the grouped launch", "",
                 "The grouped launch at every split count the context allows; us per launch (median over both passes).  `rule` is what `ops.attn_gqa_splits` returns "
                 "for the point and `best` the fastest split count measured; `rule / best` is the time at the rule's count over the time at the best "
                 "(a rule value between two measured counts is compared at the nearest measured count at or below it).", "",
                 "| heads | cache | B | positions | " + " | ".join(f"S={s}" for s in SWEEP) + " | best | rule | rule / best |", "|---|---|---|---|" + "---|" * (len(SWEEP) + 3)]
    for shape in SHAPES:
        for fmt in FORMATS:
            passes = sweep.get(f"{shape}-{fmt}")
            if not passes:
                missing.append(f"the splits sweep, {shape} heads, {fmt} cache")
                continue
            for B in BATCHES:
                for n in POSITIONS:
                    key = f"B{B}-n{n}"
                    med = {int(s): statistics.median([v for p in passes for v in p[key]["us_by_splits"][s]]) for s in passes[0][key]["us_by_splits"]}
                    best = min(med, key=med.get)
                    rule = passes[0][key]["rule"]
                    at = max(s for s in med if s <= rule)
                    rows.append(f"| {shape.replace('x', ' / ')} | {fmt} | {B} | {n} | " + " | ".join(f"{med[s]:.1f}" if s in med else "-" for s in SWEEP) +
                                f" | {best} | {rule} | {med[at] / med[best]:.2f} |")
    step = res.get("step", {})
    if step:
        rows += ["", "## The whole captured decode step", "",
                 f"Random-weight models, int4 group_size 64, {res.get('blocks', '?')} decoder blocks, `GraphedGreedyDecoder(attention=\"hip\", max_cache_len=4096)`: ms per step "
                 f"of {res.get('steps', '?')} timed graph replays after {res.get('warmup', '?')} warm-up steps (`benchmark_batch`, HIP events).  `llama`: Llama-3-8B-shaped, the "
                 "Llama-family dense case that pays one more launch per block under `\"group\"`; `qwen3`: Qwen3-8B-shaped (`qk_norm=\"fused\"`), the same launches either way.", "",
                 "| model | B | context | heads: ms (min - max) | group: ms (min - max) | group / heads |", "|---|---|---|---|---|---|"]
    for model in MODELS:
        legs = step.get(model)
        if not legs or not all(legs.get(m) for m in MODES):
            missing.append(f"the whole captured step, {model}")
            continue
        for B in BATCHES:
            for T in CONTEXTS:
                key = f"B{B}-T{T}"
                st = {m: _stat([v for p in legs[m] for v in p[key]["ms"]]) for m in MODES}
                rows.append(f"| {model} | {B} | {T} | {st['heads'][0]:.3f} ({st['heads'][1]} - {st['heads'][2]}) | {st['group'][0]:.3f} ({st['group'][1]} - {st['group'][2]}) | "
                            f"{st['group'][0] / st['heads'][0]:.3f} |")
    rows += ["", "## Not measured", ""] + ([f"- {m}" for m in missing] or ["- nothing of the plan is missing"])
    if res.get("notes"):
        rows += ["", "## Notes", ""] + [f"- {n}" for n in res["notes"]]
    rows.append("")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=("attn", "sweep", "step"))
    ap.add_argument("--mode", default="heads", choices=MODES)
    ap.add_argument("--shape", default="32x8")
    ap.add_argument("--format", default="dense", choices=FORMATS)
    ap.add_argument("--model", default="llama", choices=MODELS)
    ap.add_argument("--parts", default="attn,sweep,step")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--formats", default=",".join(FORMATS))
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--out", default="profiles/gqa_attn_bench.json")
    ap.add_argument("--md", default="profiles/gqa_attn_summary.md")
    ap.add_argument("--render-only", action="store_true", help="render --md from --out without running anything")
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rotation-gib", type=float, default=8.0)
    ap.add_argument("--leg-timeout", type=int, default=900)
    ap.add_argument("--note", action="append", default=[], help="a line for the record's Notes section")
    a = ap.parse_args()
    if a.leg in ("attn", "sweep"):
        return leg_attn(a, a.leg == "sweep")
    if a.leg == "step":
        return leg_step(a)
    out = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
    md = a.md if os.path.isabs(a.md) else os.path.join(ROOT, a.md)
    res = {}
    if os.path.exists(out):
        with open(out) as fh:
            res = json.load(fh)

    def save():
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
        with open(md, "w") as fh:
            fh.write(markdown(res))

    if a.render_only:
        res["notes"] = a.note or res.get("notes", [])
        return save()
    res.update({"tool": "gqa_attn_bench", "reps": a.reps, "notes": a.note or res.get("notes", [])})
    parts = a.parts.split(",")
    pairs = [(s, f) for s in a.shapes.split(",") for f in a.formats.split(",")]
    if "attn" in parts:
        res["rotation_gib"] = a.rotation_gib
        for s, f in pairs:
            res.setdefault("attn", {})[f"{s}-{f}"] = {m: [] for m in MODES}
        for _ in range(2):   # two passes, the modes alternating
            for s, f in pairs:
                for m in MODES:
                    r = _child(a, "attn", mode=m, shape=s, format=f)
                    res["device"] = r["device"]
                    res["attn"][f"{s}-{f}"][m].append(r["points"])
                save()
    if "sweep" in parts:
        for s, f in pairs:
            res.setdefault("sweep", {})[f"{s}-{f}"] = []
        for _ in range(2):
            for s, f in pairs:
                r = _child(a, "sweep", shape=s, format=f)
                res["device"] = r["device"]
                res["sweep"][f"{s}-{f}"].append(r["points"])
                save()
    if "step" in parts:
        res.update({"blocks": a.blocks, "steps": a.steps, "warmup": a.warmup})
        for mdl in a.models.split(","):
            res.setdefault("step", {})[mdl] = {m: [] for m in MODES}
        for _ in range(2):
            for mdl in a.models.split(","):
                for m in MODES:
                    r = _child(a, "step", mode=m, model=mdl)
                    res["device"] = r["device"]
                    res["step"][mdl][m].append(r["points"])
                save()
    save()
    print(markdown(res))


if __name__ == "__main__":
    main()
