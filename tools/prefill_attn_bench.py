#!/usr/bin/env python3
"""The prefill with prefill_attention="hip" (ops.attn_prefill / ops.attn_prefill_kvq, csrc/attn_prefill.hip) against the default prefill — HF's attention function
on the whole static cache, the parent behaviour — measured in the same run (needs an MI355X).  The house method of tools/gqa_attn_bench.py: every leg runs in a
PROCESS OF ITS OWN, the driver goes through all legs twice, alternating the modes, and the table gives medians over both passes with min - max.  Nothing here
decides a route: the feature is opt-in and the default stays "model" whatever these numbers are.

    python tools/prefill_attn_bench.py [--models 7b,llama3] [--formats dense,q8,q4] [--prompts 128,512,2048,8192] [--blocks 32]
                                       [--out profiles/prefill_attn_bench.json] [--md profiles/prefill_attn_summary.md]
        the driver: starts the legs below one after another, merges them into the JSON record (what was not run keeps what the file held) and renders the table;
        what the record does not hold is listed as not measured
    python tools/prefill_attn_bench.py --leg --mode model|hip|rest --model 7b|llama3 --format dense|q8|q4
        one leg: a random-weight model, fp16, linears int4 group_size 64, `--blocks` decoder blocks — "7b": Llama-2-7B-shaped (hidden 4096, 32 / 32 heads of 128,
        intermediate 11008, vocab 32000), "llama3": Llama-3-8B-shaped (hidden 4096, 32 / 8 heads of 128, intermediate 14336, vocab 128256) — and, for every prompt
        length T and max_cache_len in (the next power of two above T, 16384), the time of ONE prefill call (GraphedGreedyDecoder._prefill into a reset cache: the
        model's forward, the cache write included) between two HIP events, `--reps` times after a warm-up call; ms.
        mode "model": the default route.  "hip": prefill_attention="hip".  "rest": the "hip" route with the attention op replaced by one that launches nothing —
        the prefill WITHOUT its attention (the projections, the rotary embedding, the cache write, the mask, the MLP and the head remain).  The attention's share of
        a route is (route - rest) / route: for the default route that is SDPA over the whole cache and, on a quantised cache, the full-length dequantisation of
        every layer; for "hip" it is the kernel alone.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("model", "hip", "rest")
FORMATS = ("dense", "q8", "q4")
MODELS = ("7b", "llama3")
PROMPTS = (128, 512, 2048, 8192)
BIG = 16384
SHAPES = {"7b": dict(intermediate_size=11008, num_key_value_heads=32, vocab_size=32000), "llama3": dict(intermediate_size=14336, num_key_value_heads=8, vocab_size=128256)}


def cache_lens(T: int):
    """the next power of two above the prompt, and 16384"""
    n = 1
    while n <= T:
        n *= 2
    return sorted({n, BIG})


def leg(a):
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd import ops
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    cfg = LlamaConfig(hidden_size=4096, num_hidden_layers=a.blocks, num_attention_heads=32, max_position_embeddings=BIG, **SHAPES[a.model])
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
    if a.mode == "rest":   # the attention op launches nothing: its output buffer comes back as allocated
        def nothing(q, *args, **kw):
            return torch.empty(q.shape[0], q.shape[1], q.shape[2], dtype=q.dtype, device=q.device)
        ops.attn_prefill = ops.attn_prefill_kvq = nothing
    out = {}
    for T in [int(t) for t in a.prompts.split(",")]:
        ids = torch.randint(0, 32000, (1, T), device="cuda", generator=torch.Generator(device="cuda").manual_seed(T))
        for L in cache_lens(T):
            dec = GraphedGreedyDecoder(model, max_cache_len=L, prefill_attention="model" if a.mode == "model" else "hip",
                                       **({} if a.format == "dense" else {"kv_cache": a.format}))
            assert dec.prefill_hip == (a.mode != "model")
            cache = dec._new_cache()
            ms = []
            with torch.no_grad():
                for i in range(a.reps + 1):
                    cache.reset()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    dec._prefill(ids, cache)
                    e1.record()
                    torch.cuda.synchronize()
                    if i:   # (the first call is the warm-up: lazy initialisation of the cache, the kernels' LDS limits)
                        ms.append(round(e0.elapsed_time(e1), 3))
            out[f"T{T}-L{L}"] = {"ms": ms}
            del dec, cache
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"points": out, "device": torch.cuda.get_device_name(0)}), flush=True)


def _child(a, **kw):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--blocks", str(a.blocks), "--reps", str(a.reps), "--prompts", a.prompts]
    for k, v in kw.items():
        cmd += ["--" + k, v]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        raise SystemExit(f"prefill_attn_bench: leg {kw} failed (rc={res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    print(kw, "done", flush=True)
    return json.loads(lines[-1][len("RESULT "):])


def _stat(vals):
    return statistics.median(vals), min(vals), max(vals)


def markdown(res) -> str:
    rows = ["# The prefill with `prefill_attention=\"hip\"` against the default prefill", "",
            f"`tools/prefill_attn_bench.py` on {res.get('device', '?')}.  Every leg in a process of its own; two passes that alternate the modes; per leg "
            f"{res.get('reps', '?')} repetitions after a warm-up call; medians over both passes with min - max.  Random-weight models, fp16, linears int4 group_size 64, "
            f"{res.get('blocks', '?')} decoder blocks (`7b`: Llama-2-7B-shaped, 32 / 32 heads of 128; `llama3`: Llama-3-8B-shaped, 32 / 8 heads of 128).  One prefill "
            "call of `GraphedGreedyDecoder` (the model's forward into a reset static cache) between two HIP events; ms.  `model` is the default route — the parent "
            "behaviour, measured in the same run —, `hip` is `prefill_attention=\"hip\"`, and `rest` the prefill without its attention (the op launches nothing).  "
            "`share` is the attention's share of a route, (route - rest) / route: SDPA over the whole cache plus, on a quantised cache, the full-length "
            "dequantisation of every layer for `model`; the kernel for `hip`.  `hip / model` below 1 means `\"hip\"` is faster.  The feature is opt-in and the default "
            "stays `\"model\"` whatever these numbers are.  "
            "`attn / block` is (route - rest) / decoder blocks, the attention's time per block in ms: with few blocks the embedding and the head weigh on `share` "
            "far more than they do in a whole model, and this column does not depend on them.", "",
            "| model | cache | prompt | max_cache_len | model: ms (min - max) | share | attn / block | hip: ms (min - max) | share | attn / block | rest: ms | hip / model |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    missing = []
    legs = res.get("legs", {})
    for mdl in MODELS:
        for fmt in FORMATS:
            mine = legs.get(f"{mdl}-{fmt}")
            if not mine or not all(mine.get(m) for m in MODES):
                missing.append(f"{mdl}, {fmt} cache")
                continue
            for key in mine["model"][0]:
                if not all(key in p for m in MODES for p in mine[m]):
                    continue
                st = {m: _stat([v for p in mine[m] for v in p[key]["ms"]]) for m in MODES}
                T, L = key[1:].split("-L")
                share = {m: max(0.0, (st[m][0] - st["rest"][0]) / st[m][0]) for m in ("model", "hip")}
                per = {m: max(0.0, st[m][0] - st["rest"][0]) / max(1, int(res.get("blocks", 1))) for m in ("model", "hip")}
                rows.append(f"| {mdl} | {fmt} | {T} | {L} | {st['model'][0]:.2f} ({st['model'][1]} - {st['model'][2]}) | {share['model']:.0%} | {per['model']:.3f} | "
                            f"{st['hip'][0]:.2f} ({st['hip'][1]} - {st['hip'][2]}) | {share['hip']:.0%} | {per['hip']:.3f} | {st['rest'][0]:.2f} | {st['hip'][0] / st['model'][0]:.2f} |")
    rows += ["", "## Not measured", ""] + ([f"- {m}" for m in missing] or ["- nothing of the plan is missing"])
    if res.get("notes"):
        rows += ["", "## Notes", ""] + [f"- {n}" for n in res["notes"]]
    rows.append("")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--mode", default="model", choices=MODES)
    ap.add_argument("--model", default="llama3", choices=MODELS)
    ap.add_argument("--format", default="dense", choices=FORMATS)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--formats", default=",".join(FORMATS))
    ap.add_argument("--prompts", default=",".join(map(str, PROMPTS)))
    ap.add_argument("--out", default="profiles/prefill_attn_bench.json")
    ap.add_argument("--md", default="profiles/prefill_attn_summary.md")
    ap.add_argument("--render-only", action="store_true", help="render --md from --out without running anything")
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=900)
    ap.add_argument("--note", action="append", default=[], help="a line for the record's Notes section")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
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
    res.update({"tool": "prefill_attn_bench", "reps": a.reps, "blocks": a.blocks, "notes": a.note or res.get("notes", [])})
    pairs = [(m, f) for m in a.models.split(",") for f in a.formats.split(",")]
    for m, f in pairs:
        res.setdefault("legs", {})[f"{m}-{f}"] = {mode: [] for mode in MODES}
    for _ in range(2):   # two passes, the modes alternating
        for m, f in pairs:
            for mode in MODES:
                r = _child(a, mode=mode, model=m, format=f)
                res["device"] = r["device"]
                res["legs"][f"{m}-{f}"][mode].append(r["points"])
            save()
    save()
    print(markdown(res))


if __name__ == "__main__":
    main()
