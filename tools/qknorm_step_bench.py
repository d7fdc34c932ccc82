#!/usr/bin/env python3
"""Same-process A/B of the two decode routes of a Qwen3 model (needs an MI355X): GraphedGreedyDecoder(qk_norm="model") — the model's own forward, the
fused linears between HF's eager glue — against qk_norm="fused" — llama_fused's step with hqq_hip_qknorm_rope_cache_batched (per-head q_norm / k_norm,
rotary embedding and cache write in one launch) in rope_cache's place.  The model is random-weight and Qwen3-8B-shaped: hidden 4096, 36 blocks, 32 / 8
heads, head_dim 128, intermediate 12288, vocab 151936, fp16, seed 20250, every decoder linear int4, group_size 64, axis 1.

    python tools/qknorm_step_bench.py [--out FILE.json] [--md FILE.md] [--reps 5] [--steps 64] [--warmup 8] [--blocks 36] [--attention sdpa|hip]
        After one warm-up benchmark of each route, `reps` repetitions ALTERNATE between the two decoders (both kept alive, same process): each
        repetition times `steps` replays of the captured step with HIP events (GraphedGreedyDecoder.benchmark).  Reported: every repetition, the median
        and the spread (max - min) per route, whether both routes emit the same 24 tokens, and whether "fused" beats "model" by more than the larger
        spread.  --md writes the table as Markdown (profiles/qknorm_step_summary.md is such a file).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(blocks: int):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    cfg = Qwen3Config(hidden_size=4096, intermediate_size=12288, num_hidden_layers=blocks, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
                      vocab_size=151936, max_position_embeddings=2048)
    dflt = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    torch.manual_seed(20250)
    try:
        with torch.device("cuda"):
            model = Qwen3ForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(dflt)
    g = torch.Generator(device="cuda").manual_seed(20251)
    for blk in model.model.layers:   # (the all-ones default would make the head norms' weights invisible to the same-tokens check)
        for nrm in (blk.self_attn.q_norm, blk.self_attn.k_norm):
            nrm.weight.data = (1 + 0.1 * torch.randn(128, device="cuda", generator=g)).half()
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=torch.float16, device="cuda")
    prepare_for_inference(model, backend="hip")
    group_llama_projections(model)
    return model


def summarise(vals):
    return {"reps": [round(v, 2) for v in vals], "median": round(statistics.median(vals), 2), "spread": round(max(vals) - min(vals), 2)}


def markdown(res) -> str:
    b1 = res["batch1_tok_s"]
    rows = ["# Qwen3 models through the fused decode step (opt-in)", "",
            f"`tools/qknorm_step_bench.py` on {res['device']}: {res['model']}.", "",
            f"Both routes in one process, alternating, after a warm-up of each; {res['steps']} timed graph replays per repetition after {res['warmup']} "
            f"warm-up steps, a prompt of {res['prompt_tokens']} tokens, attention = `{res['attention']}`, glue = `{res['glue']}`.  tok/s from HIP events "
            "(`GraphedGreedyDecoder.benchmark`).", "",
            "| route | tok/s, every repetition | median | spread (max - min) |", "|---|---|---|---|"]
    for r in ("model", "fused"):
        rows.append(f"| `qk_norm=\"{r}\"` | {', '.join(str(v) for v in b1[r]['reps'])} | {b1[r]['median']} | {b1[r]['spread']} |")
    rows += ["", f"Median ratio fused / model: {res['batch1_speedup_median']}.  Fused ahead by more than the larger spread: {res['fused_faster_beyond_spread']}.  "
                 f"The two routes emitted the same 24 greedy tokens: {res['same_tokens_24']}.", ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/qknorm_step_bench.json")
    ap.add_argument("--md", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=36)
    ap.add_argument("--attention", default="sdpa", choices=("sdpa", "hip"))
    ap.add_argument("--glue", default="auto", choices=("auto", "folded", "kernels"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qknorm_step_bench: needs the GPU")
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    t0 = time.perf_counter()
    model = build(a.blocks)
    t_build = time.perf_counter() - t0
    ids = torch.randint(0, 151936, (1, 16), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    decs = {r: GraphedGreedyDecoder(model, max_cache_len=256, qk_norm=r, attention=a.attention, glue=a.glue) for r in ("model", "fused")}
    assert decs["fused"].fused_qk_norm and not decs["model"].fused_qk_norm and not decs["model"].fused, "the fused Qwen3 step must serve this model"
    same = bool(torch.equal(decs["model"].generate(ids, 24), decs["fused"].generate(ids, 24)))   # before anything is timed
    assert decs["fused"].step is not None and decs["model"].step is None
    for d in decs.values():   # warm-up: builds the step, captures the graphs
        d.benchmark(ids, new_tokens=a.steps, warmup=a.warmup)
    single = {"model": [], "fused": []}
    for _ in range(a.reps):   # interleaved
        for r in ("model", "fused"):
            single[r].append(decs[r].benchmark(ids, new_tokens=a.steps, warmup=a.warmup)["tok_s"])
    res = {"tool": "qknorm_step_bench", "device": torch.cuda.get_device_name(0),
           "model": f"random-init Qwen3-8B-shaped Qwen3ForCausalLM ({a.blocks} blocks, hidden 4096, 32 / 8 heads, head_dim 128, intermediate 12288, vocab 151936, "
                    "fp16, seed 20250), every decoder linear int4 gs 64 axis 1", "attention": a.attention, "glue": a.glue, "folded": bool(decs["fused"].step.folded),
           "steps": a.steps, "warmup": a.warmup, "prompt_tokens": 16, "build_s": round(t_build, 1), "same_tokens_24": same,
           "batch1_tok_s": {r: summarise(v) for r, v in single.items()}}
    b1 = res["batch1_tok_s"]
    res["batch1_speedup_median"] = round(b1["fused"]["median"] / b1["model"]["median"], 3)
    res["fused_faster_beyond_spread"] = bool(b1["fused"]["median"] - b1["model"]["median"] > max(b1["fused"]["spread"], b1["model"]["spread"]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
