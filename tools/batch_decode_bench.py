#!/usr/bin/env python3
"""Aggregate decode rate of GraphedGreedyDecoder.generate_batch on the random Llama-2-7B-shaped model of bench.py's end-to-end leg (32 blocks, hidden 4096,
intermediate 11008, vocab 32000, fp16, every decoder linear int4 gs 64, seed 20250): for B = 1, 2, 4, 8, 16 the batched step's time (HIP events over the
replays of its captured graph), the aggregate tokens per second, the ratio to the batch-1 decoder (glue="auto" and glue="kernels") and the 7B
linear stack's bytes over the step time.  Needs an MI355X.

    python tools/batch_decode_bench.py [--out FILE.json] [--steps 64] [--warmup 8]
    python tools/batch_decode_bench.py --trace B [--tokens N]   # a stream-ordered decode of B prompts, for rocprofv3 --kernel-trace (graph replays are not listed)
"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from transformers import LlamaConfig, LlamaForCausalLM  # noqa: E402

from hqq_amd.backends.hip import group_llama_projections  # noqa: E402
from hqq_amd.core.quantize import BaseQuantizeConfig  # noqa: E402
from hqq_amd.utils import llama_fused  # noqa: E402
from hqq_amd.utils.generation import GraphedGreedyDecoder  # noqa: E402
from hqq_amd.utils.model import quantize_model  # noqa: E402
from hqq_amd.utils.patching import prepare_for_inference  # noqa: E402

BATCHES = (1, 2, 4, 8, 16)


def build():
    """bench.py's end-to-end model: the same config, seed and quantisation"""
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=32, vocab_size=32000,
                      max_position_embeddings=2048)
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


def linear_bytes(model) -> int:
    """packed levels + scale + zero of every decoder linear: what one decode step streams from HBM for the linears"""
    n = 0
    for lins in llama_fused._decoder_linears(model):
        for L in lins:
            n += L.W_q.numel() * L.W_q.element_size() + L.scale.numel() * L.scale.element_size() + L.zero.numel() * L.zero.element_size()
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/batch_decode_bench.json")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--trace", type=int, default=0, help="B: decode B prompts stream-ordered (no graph) for a kernel trace, then exit")
    ap.add_argument("--tokens", type=int, default=8)
    a = ap.parse_args()
    t0 = time.perf_counter()
    model = build()
    t_build = time.perf_counter() - t0
    gx = torch.Generator(device="cuda").manual_seed(1)
    if a.trace:
        dec = GraphedGreedyDecoder(model, max_cache_len=256, glue="kernels")
        prompts = [torch.randint(0, 32000, (1, 16), device="cuda", generator=gx) for _ in range(a.trace)]
        out = dec.generate_batch(prompts, a.tokens, use_graph=False)
        torch.cuda.synchronize()
        print(json.dumps({"trace_batch": a.trace, "tokens": a.tokens, "batched_step": a.trace in dec._batch, "shapes": [list(o.shape) for o in out]}))
        return
    ids = torch.randint(0, 32000, (max(BATCHES), 16), device="cuda", generator=gx)
    nbytes = linear_bytes(model)
    res = {"model": "random-init Llama-2-7B-shaped LlamaForCausalLM (bench.py's end-to-end model: 32 blocks, hidden 4096, intermediate 11008, vocab 32000, fp16, "
                    "seed 20250), every decoder linear int4 gs 64", "linear_stack_bytes": nbytes, "steps": a.steps, "warmup": a.warmup, "prompt_tokens": 16,
           "build_s": round(t_build, 1), "batch1": {}, "batched": []}
    for glue in ("auto", "kernels"):
        dec = GraphedGreedyDecoder(model, max_cache_len=256, glue=glue)
        r = dec.benchmark(ids[:1], new_tokens=a.steps, warmup=a.warmup)
        res["batch1"][glue] = {"ms_per_token": round(r["ms_per_token"], 4), "tok_s": round(r["tok_s"], 2), "folded": bool(dec.step is not None and dec.step.folded)}
        del dec
        torch.cuda.empty_cache()
    for B in BATCHES:
        dec = GraphedGreedyDecoder(model, max_cache_len=256)
        r = dec.benchmark_batch(ids[:B], new_tokens=a.steps, warmup=a.warmup)
        ms = r["ms_per_step"]
        res["batched"].append({
            "B": B, "route": "batch-1 generate (glue auto)" if B == 1 else "FusedLlamaBatchStep (glue kernels, M = B linears)", "covered": llama_fused.supports_batch(model, B),
            "ms_per_step": round(ms, 4), "tok_s": round(r["tok_s"], 2),
            "ratio_vs_batch1_auto": round(r["tok_s"] / res["batch1"]["auto"]["tok_s"], 3), "ratio_vs_batch1_kernels": round(r["tok_s"] / res["batch1"]["kernels"]["tok_s"], 3),
            "linear_bytes_per_step_time_TBps": round(nbytes / (ms * 1e-3) / 1e12, 3)})
        print(json.dumps(res["batched"][-1]), flush=True)
        del dec
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
