#!/usr/bin/env python3
"""What a speculative step costs: the captured verify step of GraphedGreedyDecoder(speculate="ngram") at 4, 8 and 16 rows against the plain one-row step, on the
random Llama-2-7B-shaped model of bench.py's end-to-end leg (32 blocks, hidden 4096, intermediate 11008, vocab 32000, fp16, every decoder linear int4 gs 64,
seed 20250), attention="hip", at a short and a long context.  The ratio of the two step times is the mean number of tokens a step must commit for speculation to
break even; the attention launches' share of the long-context step is what the second set of legs is about: the same verify step with verify_attention="tile"
(ops.attn_decode_tiled, the kernel that reads each key once for all rows) beside verify_attention="rows" (ops.attn_decode_shared), measured in the same run.  How many
tokens a step DOES commit depends on the text: a random model's greedy output loops, so the tokens per step recorded here are not representative, and no speed
claim on real text follows from this file.  Needs an MI355X.

    python tools/spec_decode_bench.py [--out FILE.json] [--md FILE.md] [--steps 64] [--warmup 8]

Every leg (the plain step, the verify step at one row count with one attention kernel) runs in a process of its own; two passes that alternate the legs.  The
record is rewritten after every leg, so a run that is cut short keeps what it measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (4, 8, 16)
CONTEXTS = (256, 3000)
KINDS = ("rows", "tile")      # FusedLlamaStep's verify_attention; a leg's name is the kind + the row count
LEGS = ("plain",) + tuple(f"{k}{r}" for r in ROWS for k in KINDS)
CACHE_LEN = 4096


def build(blocks: int):
    """bench.py's end-to-end model (the same config, seed and quantisation), with room for the long context"""
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=blocks, num_attention_heads=32, num_key_value_heads=32, vocab_size=32000,
                      max_position_embeddings=CACHE_LEN)
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
    return model


def attention_ms(step, T: int, R: int, reps: int = 20) -> float:
    """the step's attention launches alone — per block the step's own verify attention (ops.attn_decode_shared or ops.attn_decode_tiled, and the merging launch) on
    the block's own cache tensors, rows at T .. T + R - 1 —
    as ONE captured graph of all blocks, replayed `reps` times between two HIP events: ms per step's worth of attention"""
    import torch
    from hqq_amd import ops
    from hqq_amd.utils.generation import kv_bucket
    pos = torch.arange(T, T + R, device="cuda")
    splits = ops.attn_splits(kv_bucket(T + R - 1, "hip", CACHE_LEN))   # (the split count the step itself takes at these positions)
    ws = ops.attn_workspace_batched("cuda", R, step.n_heads, step.hd, splits)

    def run():
        for b in step.blocks:
            step._verify_attn(b["qr"], b["kc"], b["vc"], pos, step.att, b["attn"].scaling, splits=splits, workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def leg(a):
    import torch
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = build(a.blocks)
    out = {"leg": a.leg, "device": torch.cuda.get_device_name(0), "points": {}}
    gx = torch.Generator(device="cuda").manual_seed(1)
    for T in CONTEXTS:
        ids = torch.randint(0, 32000, (1, T), device="cuda", generator=gx)
        if a.leg == "plain":
            dec = GraphedGreedyDecoder(model, max_cache_len=CACHE_LEN, attention="hip")
            dec.benchmark(ids, new_tokens=a.steps, warmup=a.warmup)   # captures the graphs
            ms = [dec.benchmark(ids, new_tokens=a.steps, warmup=a.warmup)["ms_per_token"] for _ in range(a.reps)]
            assert dec.step is not None
            out["points"][str(T)] = {"ms_per_step": [round(v, 4) for v in ms]}
        else:
            kind, R = a.leg[:4], int(a.leg[4:])
            dec = GraphedGreedyDecoder(model, max_cache_len=CACHE_LEN, attention="hip", speculate="ngram", draft_rows=R, verify_attention=kind)
            dec.benchmark_speculative(ids, steps=a.steps, warmup=a.warmup)
            ms = [dec.benchmark_speculative(ids, steps=a.steps, warmup=a.warmup)["ms_per_step"] for _ in range(a.reps)]
            att = [attention_ms(dec._spec["step"], T, R) for _ in range(a.reps)]
            dec.generate(ids, 128)
            assert dec.speculating and dec._spec["step"].verify_attention == kind
            out["points"][str(T)] = {"ms_per_step": [round(v, 4) for v in ms], "attention_ms": [round(v, 4) for v in att], "random_model_stats": dict(dec.spec_stats)}
        del dec
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def _child(a, name):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--blocks", str(a.blocks), "--reps", str(a.reps), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        raise SystemExit(f"spec_decode_bench: leg {name} failed (rc={res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    print(lines[-1], flush=True)
    return json.loads(lines[-1][len("RESULT "):])


def _all(res, name, T, key):
    return [v for p in res["legs"][name] for v in p[str(T)][key]]


def markdown(res) -> str:
    rows = ["# Speculative greedy decode by prompt lookup: what a step costs", "",
            f"`tools/spec_decode_bench.py` on one MI355X (torch names it `{res['device']}`).  The model is `bench.py`'s end-to-end model: a random-init Llama-2-7B-shaped `LlamaForCausalLM` "
            f"({res['blocks']} blocks, fp16, seed 20250, every decoder linear int4 gs 64), `GraphedGreedyDecoder(attention=\"hip\", max_cache_len={CACHE_LEN})`.  "
            f"Every leg in a process of its own, two passes that alternate the legs, {res['reps']} repetitions per leg and context; a repetition is {res['steps']} "
            f"replays of the captured step between two HIP events after {res['warmup']} warm-up replays.  The verify step is timed in the frozen state "
            "(`benchmark_speculative`: propose, the R-row step, the rows' argmax and accept all run at the prompt's end, nothing is committed), the plain step by "
            "`benchmark` (its position advances by one per replay).", "",
            "The feature is opt-in and no route depends on these numbers.  **Break-even** is the verify step's time over the plain step's: the mean number of "
            "tokens a speculative step must commit to match plain decoding.  A step commits between 1 and R tokens; how many is a property of the text.", "",
            "| context | step | ms / step (median) | min - max | break-even tokens / step | attention launches, ms | share of the step |", "|---|---|---|---|---|---|---|"]
    for T in CONTEXTS:
        base = statistics.median(_all(res, "plain", T, "ms_per_step"))
        v = _all(res, "plain", T, "ms_per_step")
        rows.append(f"| {T} | plain, 1 row | {base:.3f} | {min(v):.3f} - {max(v):.3f} | 1.00 | | |")
        for R in ROWS:
            for kind in KINDS:
                v = _all(res, f"{kind}{R}", T, "ms_per_step")
                m = statistics.median(v)
                av = _all(res, f"{kind}{R}", T, "attention_ms")
                at = statistics.median(av)
                rows.append(f"| {T} | verify, {R} rows, `\"{kind}\"` | {m:.3f} | {min(v):.3f} - {max(v):.3f} | **{m / base:.2f}** | {at:.3f} ({min(av):.3f} - {max(av):.3f}) | "
                            f"{100 * at / m:.0f} % |")
    rows += ["", "## Tokens per step on this model: NOT representative", "",
             "The weights are random and so are the prompts: the greedy output is whatever near-flat logits give — a loop the drafts then follow, or tokens that never "
             "occurred before, of which no draft is confirmed (1.00 tokens per step: every step costs the break-even factor above and commits one token).  The "
             "figures say nothing about real text.  128 new tokens after the prompt, `ngram_max=3`.", "",
             "| context | rows | attention | steps | tokens | tokens / step |", "|---|---|---|---|---|---|"]
    for T in CONTEXTS:
        for R in ROWS:
            for kind in KINDS:
                s = res["legs"][f"{kind}{R}"][0][str(T)]["random_model_stats"]
                rows.append(f"| {T} | {R} | {kind} | {s['steps']} | {s['tokens']} | {s['tokens'] / max(1, s['steps']):.2f} |")
    if res.get("notes"):
        rows += ["", "## Notes", ""] + [f"- {n}" for n in res["notes"]]
    rows.append("")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=LEGS)
    ap.add_argument("--out", default="profiles/spec_decode_bench.json")
    ap.add_argument("--md", default=None)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--leg-timeout", type=int, default=600)
    ap.add_argument("--note", action="append", default=[], help="a line for the record's Notes section")
    a = ap.parse_args()
    if a.leg is not None:
        return leg(a)
    out = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
    res = {"tool": "spec_decode_bench", "blocks": a.blocks, "reps": a.reps, "steps": a.steps, "warmup": a.warmup, "contexts": list(CONTEXTS), "notes": a.note,
           "legs": {name: [] for name in LEGS}}
    for _ in range(2):   # two passes, the legs alternating
        for name in LEGS:
            r = _child(a, name)
            res["device"] = r["device"]
            res["legs"][name].append(r["points"])
            with open(out, "w") as fh:
                json.dump(res, fh, indent=1)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
