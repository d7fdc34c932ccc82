#!/usr/bin/env python3
"""Same-process A/B of the two decode routes of a model quantised along AXIS 0 (needs an MI355X): GraphedGreedyDecoder(axis0="model") — the model's
own forward, every linear a hqq_hip_gemv_axis0 call between HF's eager glue — against axis0="fused" — llama_fused's step with q|k|v and gate|up
(+ SiLU * up) as one grouped axis-0 launch each.  The model is bench.py's end-to-end shape (a random-init Llama-2-7B-shaped LlamaForCausalLM: 32 blocks,
hidden 4096, intermediate 11008, vocab 32000, fp16, seed 20250) with every decoder linear int4, group_size 64, axis 0.

    python tools/axis0_step_bench.py [--out FILE.json] [--reps 5] [--steps 64] [--warmup 8] [--blocks 32]
        After one warm-up benchmark of each route, `reps` repetitions ALTERNATE between the two decoders (both kept alive, same process): each
        repetition times `steps` replays of the captured step with HIP events.  Reported: every repetition, the median and the spread (max - min) per
        route, and whether "fused" beats "model" by more than the larger spread.  Then generate_batch at B = 8 and B = 16 through the batched axis-0 step
        (aggregate tokens per second, same alternation against the batch-1 routes: decoding the prompts one after another IS the batch-1 rate).
    python tools/axis0_step_bench.py --trace model|fused [--tokens N]
        a stream-ordered decode (no graph: replays are not listed in a kernel trace) of N new tokens, to be run as the program after `--` of
        `rocprofv3 --kernel-trace --stats --output-format csv`, under a time limit of its own
    python tools/axis0_step_bench.py --launches STATS_N1.csv STATS_N2.csv --dtokens D
        launches per decode step from two such traces that differ by D decode steps (prefill and set-up cancel): (calls_2 - calls_1) / D per kernel
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(blocks: int):
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=blocks, num_attention_heads=32, num_key_value_heads=32, vocab_size=32000,
                      max_position_embeddings=2048)
    dflt = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    torch.manual_seed(20250)
    try:
        with torch.device("cuda"):
            model = LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(dflt)
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=0), compute_dtype=torch.float16, device="cuda")
    prepare_for_inference(model, backend="hip")
    return model


def summarise(vals):
    return {"reps": [round(v, 2) for v in vals], "median": round(statistics.median(vals), 2), "spread": round(max(vals) - min(vals), 2)}


def launches(stats_a: str, stats_b: str, dtokens: int) -> dict:
    def calls(path):
        out = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                out[row["Name"]] = out.get(row["Name"], 0) + int(float(row["Calls"]))
        return out
    a, b = calls(stats_a), calls(stats_b)
    per = {k: (b.get(k, 0) - a.get(k, 0)) / dtokens for k in sorted(set(a) | set(b)) if b.get(k, 0) != a.get(k, 0)}
    return {"launches_per_step": round(sum(per.values()), 2), "by_kernel": {k: round(v, 2) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/axis0_step_bench.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--attention", default="sdpa", choices=("sdpa", "hip"))
    ap.add_argument("--trace", choices=("model", "fused"), default=None)
    ap.add_argument("--tokens", type=int, default=8)
    ap.add_argument("--launches", nargs=2, metavar="STATS_CSV", default=None)
    ap.add_argument("--dtokens", type=int, default=8)
    a = ap.parse_args()
    if a.launches:
        print(json.dumps(launches(a.launches[0], a.launches[1], a.dtokens), indent=1))
        return
    if not torch.cuda.is_available():
        raise SystemExit("axis0_step_bench: needs the GPU")
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    t0 = time.perf_counter()
    model = build(a.blocks)
    t_build = time.perf_counter() - t0
    gx = torch.Generator(device="cuda").manual_seed(1)
    if a.trace:
        dec = GraphedGreedyDecoder(model, max_cache_len=256, axis0=a.trace, attention=a.attention)
        out = dec.generate(torch.randint(0, 32000, (1, 16), device="cuda", generator=gx), a.tokens, use_graph=False)
        torch.cuda.synchronize()
        print(json.dumps({"trace": a.trace, "tokens": a.tokens, "decode_steps": a.tokens - 1, "fused_axis0": dec.fused_axis0, "step": dec.step is not None,
                          "shape": list(out.shape)}))
        return
    ids = torch.randint(0, 32000, (16, 16), device="cuda", generator=gx)
    decs = {r: GraphedGreedyDecoder(model, max_cache_len=256, axis0=r, attention=a.attention) for r in ("model", "fused")}
    assert decs["fused"].fused_axis0 and not decs["model"].fused_axis0 and not decs["model"].fused, "the fused axis-0 step must serve this model"
    # same tokens from both routes before anything is timed
    same = bool(torch.equal(decs["model"].generate(ids[:1], 24), decs["fused"].generate(ids[:1], 24)))
    for d in decs.values():   # warm-up: builds the step, captures the graphs
        d.benchmark(ids[:1], new_tokens=a.steps, warmup=a.warmup)
    single = {"model": [], "fused": []}
    for _ in range(a.reps):   # interleaved
        for r in ("model", "fused"):
            single[r].append(decs[r].benchmark(ids[:1], new_tokens=a.steps, warmup=a.warmup)["tok_s"])
    res = {"tool": "axis0_step_bench", "device": torch.cuda.get_device_name(0),
           "model": f"random-init Llama-2-7B-shaped LlamaForCausalLM ({a.blocks} blocks, hidden 4096, intermediate 11008, vocab 32000, fp16, seed 20250), "
                    "every decoder linear int4 gs 64 axis 0", "attention": a.attention, "steps": a.steps, "warmup": a.warmup, "prompt_tokens": 16,
           "build_s": round(t_build, 1), "same_tokens_24": same, "batch1_tok_s": {r: summarise(v) for r, v in single.items()}, "batched": []}
    b1 = res["batch1_tok_s"]
    res["batch1_speedup_median"] = round(b1["fused"]["median"] / b1["model"]["median"], 3)
    res["fused_faster_beyond_spread"] = bool(b1["fused"]["median"] - b1["model"]["median"] > max(b1["fused"]["spread"], b1["model"]["spread"]))
    print(json.dumps({"batch1_tok_s": b1, "speedup": res["batch1_speedup_median"]}), flush=True)
    dec = decs["fused"]
    for B in (8, 16):
        covered = llama_fused.supports_axis0_batch(model, B)
        dec.benchmark_batch(ids[:B], new_tokens=a.steps, warmup=a.warmup)   # warm-up: builds the B-row state, captures its graphs
        rows, seq = [], []
        for _ in range(a.reps):   # interleaved with sequential decoding's rate: the "model" route at batch 1 (what generate_batch falls back to)
            seq.append(decs["model"].benchmark(ids[:1], new_tokens=a.steps, warmup=a.warmup)["tok_s"])
            rows.append(dec.benchmark_batch(ids[:B], new_tokens=a.steps, warmup=a.warmup)["tok_s"])
        rb, sq = summarise(rows), summarise(seq)
        res["batched"].append({"B": B, "covered": covered, "batched_step": B in dec._batch, "aggregate_tok_s": rb, "sequential_model_route_tok_s": sq,
                               "ratio_vs_sequential": round(rb["median"] / sq["median"], 3), "ratio_vs_fused_batch1": round(rb["median"] / b1["fused"]["median"], 3)})
        print(json.dumps(res["batched"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
