#!/usr/bin/env python3
"""The quantised KV cache against the dense one (needs an MI355X): the decode-attention launch alone, and the whole decode step at a long context.  Every leg
runs in a PROCESS OF ITS OWN, and the driver goes through all legs twice, alternating the formats (pass 1: dense, q8, q4; pass 2 the same again), so that no
format inherits another's allocator state or clocks.

    python tools/kvq_bench.py [--parts attn,step] [--out profiles/kvq_bench.json] [--md profiles/kvq_summary.md] [--blocks 32] [--context 3000] [--reps 3]
        the driver: starts the legs below one after another, merges them into the JSON record (parts that were not run keep what the file held) and renders the table
    python tools/kvq_bench.py --leg attn --format dense|q8|q4
        the attention launch alone on the 7B head shape (32 query and 32 kv heads of 128, fp16): ops.attn_decode_batched on a dense cache, or
        ops.attn_decode_kvq_batched on a quantised one (group size 64), at 1024 / 4096 / 16384 visible positions (the cache holds exactly that many; the split count
        is ops.attn_splits' for that length), B = 1 and 16.  A decode step runs this launch once per layer on that layer's own cache, so the launch is timed over
        a ROTATION of independent caches — as many as a 32-layer model has, fewer where 32 do not fit in 8 GiB — never twice in a row on bytes the last call left
        in the caches of the chip.  A captured graph of one rotation, replayed; HIP events; us per launch and the GB/s of the bytes the format must read
        (levels and meta, or dense rows, of the visible positions of K and V: counted from the shapes).  Prints one JSON line.
    python tools/kvq_bench.py --leg step --format dense|q8|q4
        the 7B-shaped random-weight model (hidden 4096, 32 heads of 128, intermediate 11008, vocab 32000, fp16, linears int4 group_size 64; `--blocks` decoder
        blocks), GraphedGreedyDecoder(attention="hip", kv_cache=...) with a cache of 4096 positions after a prompt of `--context` tokens: tok/s of
        `--steps` timed graph replays (GraphedGreedyDecoder.benchmark), `--reps` times; the cache's device bytes; prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS = ("dense", "q8", "q4")
HEADS, KV_HEADS, HD, GS = 32, 32, 128, 64
POSITIONS = (1024, 4096, 16384)
BATCHES = (1, 16)
ROTATION_BYTES = 8 << 30


def kv_bytes(fmt: str, B: int, n: int) -> int:
    """the bytes of K and V one attention launch must read for n visible positions of B sequences"""
    row = HD * 2 if fmt == "dense" else HD * int(fmt[1]) // 8 + 2 * 2 * (HD // GS)
    return 2 * B * KV_HEADS * n * row


def leg_attn(a):
    import torch
    from hqq_amd import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    out = {}
    for B in BATCHES:
        for n in POSITIONS:
            per = kv_bytes(a.format, B, n)
            copies = max(1, min(32, ROTATION_BYTES // max(per, 1)))
            q = (torch.randn(B, HEADS * HD, device="cuda", generator=g) * 0.5).half()
            o = torch.empty_like(q)
            pos = torch.full((B,), n - 1, dtype=torch.int64, device="cuda")
            splits = ops.attn_splits(n)
            ws = ops.attn_workspace_batched("cuda", B, HEADS, HD, splits)
            caches = []
            for _ in range(copies):
                if a.format == "dense":
                    caches.append(tuple(torch.randn(B, KV_HEADS, n, HD, device="cuda", generator=g, dtype=torch.float16) for _ in range(2)))
                else:
                    bufs = ops.kv_alloc(B, KV_HEADS, n, HD, int(a.format[1]), GS, torch.float16, "cuda")
                    for b in range(B):   # (row by row: the dense source of one sequence is a transient)
                        k, v = (torch.randn(1, KV_HEADS, n, HD, device="cuda", generator=g, dtype=torch.float16) for _ in range(2))
                        ops.kv_quantize(k, v, tuple(t[b:b + 1] for t in bufs), start=0)
                    caches.append(bufs)

            def rotation():
                for c in caches:
                    if a.format == "dense":
                        ops.attn_decode_batched(q, c[0], c[1], pos, o, HD ** -0.5, splits=splits, workspace=ws)
                    else:
                        ops.attn_decode_kvq_batched(q, c, pos, o, HD ** -0.5, HD, splits=splits, workspace=ws)

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
            replays = max(2, 400 // copies)
            for _ in range(2):
                graph.replay()
            torch.cuda.synchronize()
            us = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(replays):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / (replays * copies))
            out[f"B{B}-n{n}"] = {"us": [round(v, 2) for v in us], "bytes": per, "caches": copies, "splits": splits}
            del caches
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"leg": "attn", "format": a.format, "points": out, "device": torch.cuda.get_device_name(0)}), flush=True)


def leg_step(a):
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=a.blocks, num_attention_heads=HEADS, num_key_value_heads=KV_HEADS, vocab_size=32000,
                      max_position_embeddings=4096)
    dflt = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    torch.manual_seed(20250)
    try:
        with torch.device("cuda"):
            model = LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(dflt)
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=torch.float16, device="cuda")
    prepare_for_inference(model, backend="hip")
    group_llama_projections(model)
    dec = GraphedGreedyDecoder(model, max_cache_len=4096, attention="hip", kv_cache=None if a.format == "dense" else a.format)
    ids = torch.randint(0, 32000, (1, a.context), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    toks = dec.generate(ids, 16)[0, a.context:].tolist()
    assert dec.step is not None and dec.step.kv_bits == (None if a.format == "dense" else int(a.format[1])), "the fused step must serve every format"
    dec.benchmark(ids, new_tokens=a.steps, warmup=a.warmup)   # warm-up: captures the graphs
    reps = [dec.benchmark(ids, new_tokens=a.steps, warmup=a.warmup)["tok_s"] for _ in range(a.reps)]
    print("RESULT " + json.dumps({"leg": "step", "format": a.format, "tok_s": [round(v, 2) for v in reps], "tokens": toks, "kv_cache_bytes": dec.kv_cache_bytes,
                                  "device": torch.cuda.get_device_name(0)}), flush=True)


def _child(a, leg, fmt):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--format", fmt, "--blocks", str(a.blocks), "--reps", str(a.reps), "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--context", str(a.context)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        raise SystemExit(f"kvq_bench: leg {leg} {fmt} failed (rc={res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    print(lines[-1], flush=True)
    return json.loads(lines[-1][len("RESULT "):])


def _med(vals):
    return round(statistics.median(vals), 2)


def markdown(res) -> str:
    rows = ["# Quantised KV cache (8 / 4 bits) against the dense cache", "",
            f"`tools/kvq_bench.py` on {res.get('device', '?')}.  Every leg in a process of its own; two passes that alternate the formats; per leg {res['reps']} repetitions.  "
            "The feature is opt-in (`GraphedGreedyDecoder(kv_cache=\"q8\" / \"q4\")`): no route depends on these numbers."]
    if "attn" in res:
        rows += ["", "## The attention launch alone", "",
                 "7B head shape (32 query and 32 kv heads of 128, fp16), group size 64; the cache holds exactly the visible positions; `ops.attn_splits` picks the "
                 "split count.  Timed over a rotation of independent caches (as many as a 32-layer model has, fewer where 32 do not fit in 8 GiB), a captured graph "
                 "of one rotation replayed between two HIP events.  us per launch (median over both passes; min - max); GB/s = the bytes the format must read "
                 "(levels and meta, or dense rows, of K and V: counted from the shapes) over that time.", "",
                 "| B | positions | format | bytes read | caches | us per launch | spread | GB/s | time / dense |", "|---|---|---|---|---|---|---|---|---|"]
        for B in BATCHES:
            for n in POSITIONS:
                key = f"B{B}-n{n}"
                base = None
                for fmt in FORMATS:
                    pts = [p[key] for p in res["attn"][fmt]]
                    us = [v for p in pts for v in p["us"]]
                    m = _med(us)
                    base = m if fmt == "dense" else base
                    rows.append(f"| {B} | {n} | {fmt} | {pts[0]['bytes'] / 2 ** 20:.1f} MiB | {pts[0]['caches']} | {m} | {min(us)} - {max(us)} | "
                                f"{pts[0]['bytes'] / (m * 1e-6) / 1e9:.0f} | {m / base:.2f} |")
    if "step" in res:
        rows += ["", "## The whole decode step at a long context", "",
                 f"The 7B-shaped random-weight model ({res['blocks']} decoder blocks, hidden 4096, 32 heads of 128, intermediate 11008, vocab 32000, fp16, linears int4 "
                 f"group_size 64), `GraphedGreedyDecoder(attention=\"hip\", max_cache_len=4096)`, one sequence after a prompt of {res['context']} tokens: tok/s of "
                 f"{res['steps']} timed graph replays after {res['warmup']} warm-up steps (`GraphedGreedyDecoder.benchmark`, HIP events).", "",
                 "| format | tok/s, pass 1 | tok/s, pass 2 | median | spread (max - min) | tok/s / dense | KV cache bytes | of dense |", "|---|---|---|---|---|---|---|---|"]
        dense = res["step"]["dense"]
        dm = statistics.median([v for p in dense for v in p["tok_s"]])
        for fmt in FORMATS:
            p = res["step"][fmt]
            allv = p[0]["tok_s"] + p[1]["tok_s"]
            rows.append(f"| {fmt} | {', '.join(map(str, p[0]['tok_s']))} | {', '.join(map(str, p[1]['tok_s']))} | {_med(allv)} | {round(max(allv) - min(allv), 2)} | "
                        f"{statistics.median(allv) / dm:.3f} | {p[0]['kv_cache_bytes'] / 2 ** 20:.0f} MiB | {p[0]['kv_cache_bytes'] / dense[0]['kv_cache_bytes']:.3f} |")
        same = {fmt: res["step"][fmt][0]["tokens"] == dense[0]["tokens"] for fmt in ("q8", "q4")}
        rows += ["", f"The first 16 greedy tokens equal the dense run's: q8 {same['q8']}, q4 {same['q4']} (random weights: near-flat logits, so a quantised cache may "
                     "well pick other tokens; the tests state what is guaranteed)."]
    if res.get("notes"):
        rows += ["", "## Notes", ""] + [f"- {n}" for n in res["notes"]]
    rows.append("")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=("attn", "step"))
    ap.add_argument("--format", default="dense", choices=FORMATS)
    ap.add_argument("--parts", default="attn,step")
    ap.add_argument("--out", default="profiles/kvq_bench.json")
    ap.add_argument("--md", default=None)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--context", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--leg-timeout", type=int, default=600)
    ap.add_argument("--note", action="append", default=[], help="a line for the record's Notes section")
    a = ap.parse_args()
    if a.leg == "attn":
        return leg_attn(a)
    if a.leg == "step":
        return leg_step(a)
    out = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
    res = {}
    if os.path.exists(out):
        with open(out) as fh:
            res = json.load(fh)
    res.update({"tool": "kvq_bench", "reps": a.reps, "notes": a.note or res.get("notes", [])})
    parts = a.parts.split(",")
    if "step" in parts:
        res.update({"blocks": a.blocks, "context": a.context, "steps": a.steps, "warmup": a.warmup})
    for part in parts:
        res[part] = {fmt: [] for fmt in FORMATS}
    for _ in range(2):   # two passes, the formats alternating
        for part in parts:
            for fmt in FORMATS:
                r = _child(a, part, fmt)
                res["device"] = r.pop("device")
                res[part][fmt].append(r["points"] if part == "attn" else r)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
