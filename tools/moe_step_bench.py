#!/usr/bin/env python3
"""A/B of the MoE decode routes and of the router launch (needs an MI355X).  Every leg runs in a PROCESS OF ITS OWN, and the driver goes through all legs
twice, alternating the routes (pass 1: model, fused, ...; pass 2 the same again), so that no route inherits another's allocator state or clocks.

    python tools/moe_step_bench.py [--out FILE.json] [--md FILE.md] [--blocks 2] [--reps 3] [--steps 64] [--warmup 8] [--shapes mixtral,qwen3_moe] [--note TEXT]
        the driver: starts the legs below one after another and writes the record (profiles/moe_step_summary.md is such a file)
    python tools/moe_step_bench.py --leg step --shape mixtral|qwen3_moe --route model|fused
        one decode route of a random-weight model of the shape: GraphedGreedyDecoder(moe="model") — the model's own forward, HF's router and glue around
        HQQExperts' two launches — or moe="fused" (with qk_norm="fused" for Qwen3-MoE) — llama_fused's step with hqq_hip_moe_router.  `reps` repetitions of
        `steps` timed graph replays (GraphedGreedyDecoder.benchmark, HIP events); prints one JSON line with the tok/s of every repetition and 16 greedy tokens.
    python tools/moe_step_bench.py --leg router --shape mixtral|qwen3_moe --route kernel|torch
        the router alone at 1 and 16 rows: ops.moe_router against the torch chain it replaces (F.linear, softmax, topk, sum, div; Qwen3-MoE: the cast), both
        as eager launches from Python and as a captured graph of 50 calls (HIP events around `reps` x 20 replays); prints one JSON line, us per call.

Shapes (random weights, fp16, experts and attention linears int4 group_size 64 axis 1, `--blocks` decoder blocks — 2 by default, so that construction fits in
host and device memory and in a few minutes; the real models have 32 and 48):
    mixtral     Mixtral-8x7B's block: hidden 4096, 32 / 8 heads of 128, 8 experts of 14336, top-2, router 8 x 4096, vocab 32000
    qwen3_moe   a Qwen3-MoE-30B-like block: hidden 2048, 32 / 4 heads of 128, 128 experts of 768, top-8, norm_topk_prob, router 128 x 2048, vocab 151936
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "mixtral": dict(hidden=4096, heads=32, kv=8, hd=128, experts=8, inter=14336, top_k=2, vocab=32000),
    "qwen3_moe": dict(hidden=2048, heads=32, kv=4, hd=128, experts=128, inter=768, top_k=8, vocab=151936),
}


def build(shape: str, blocks: int):
    import torch
    from transformers import MixtralConfig, MixtralForCausalLM, Qwen3MoeConfig, Qwen3MoeForCausalLM
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    s = SHAPES[shape]
    common = dict(hidden_size=s["hidden"], num_hidden_layers=blocks, num_attention_heads=s["heads"], num_key_value_heads=s["kv"], head_dim=s["hd"],
                  num_experts_per_tok=s["top_k"], vocab_size=s["vocab"], max_position_embeddings=2048)
    dflt = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    torch.manual_seed(20251)
    try:
        with torch.device("cuda"):
            if shape == "mixtral":
                model = MixtralForCausalLM(MixtralConfig(intermediate_size=s["inter"], num_local_experts=s["experts"], **common)).eval()
            else:
                model = Qwen3MoeForCausalLM(Qwen3MoeConfig(intermediate_size=s["inter"], moe_intermediate_size=s["inter"], num_experts=s["experts"],
                                                           norm_topk_prob=True, **common)).eval()
    finally:
        torch.set_default_dtype(dflt)
    g = torch.Generator(device="cuda").manual_seed(20252)
    for blk in model.model.layers:   # (transformers initialises the Qwen3-MoE router to zeros: every logit would tie)
        blk.mlp.gate.weight.data = (torch.randn(blk.mlp.gate.weight.shape, device="cuda", generator=g) * 0.02).half()
    qc = BaseQuantizeConfig(nbits=4, group_size=64, axis=1)
    quantize_model(model, qc, compute_dtype=torch.float16, device="cuda", expert_config=qc)
    prepare_for_inference(model, backend="hip")
    return model


def leg_step(a):
    import torch
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = build(a.shape, a.blocks)
    kw = {} if a.route == "model" else (dict(moe="fused", qk_norm="fused") if a.shape == "qwen3_moe" else dict(moe="fused"))
    dec = GraphedGreedyDecoder(model, max_cache_len=256, **kw)
    assert dec.fused_moe == (a.route == "fused") and not dec.fused, "the fused MoE step must serve this model when asked, and only then"
    ids = torch.randint(0, SHAPES[a.shape]["vocab"], (1, 16), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    toks = dec.generate(ids, 16)[0, 16:].tolist()
    assert (dec.step is not None) == (a.route == "fused")
    dec.benchmark(ids, new_tokens=a.steps, warmup=a.warmup)   # warm-up: captures the graphs
    reps = [dec.benchmark(ids, new_tokens=a.steps, warmup=a.warmup)["tok_s"] for _ in range(a.reps)]
    print("RESULT " + json.dumps({"leg": "step", "shape": a.shape, "route": a.route, "tok_s": [round(v, 2) for v in reps], "tokens": toks,
                                  "device": torch.cuda.get_device_name(0)}), flush=True)


def leg_router(a):
    import torch
    import torch.nn.functional as F
    from hqq_amd import ops
    s = SHAPES[a.shape]
    g = torch.Generator(device="cuda").manual_seed(3)
    W = (torch.randn(s["experts"], s["hidden"], device="cuda", generator=g) * 0.02).half()
    k, qwen = s["top_k"], a.shape == "qwen3_moe"
    out = {}
    for T in (1, 16):
        x = torch.randn(T, s["hidden"], device="cuda", generator=g).half()
        idx, wts = torch.empty(T, k, dtype=torch.int64, device="cuda"), torch.empty(T, k, device="cuda")

        def kernel():
            ops.moe_router(x, W, k, renorm=True, round_weights=qwen, idx=idx, weights=wts)

        def chain():   # MixtralTopKRouter.forward / Qwen3MoeTopKRouter.forward
            logits = F.linear(x, W)
            probs = F.softmax(logits, dtype=torch.float, dim=-1)
            v, i = torch.topk(probs, k, dim=-1)
            v /= v.sum(dim=-1, keepdim=True)
            return v.to(logits.dtype) if qwen else v, i

        fn = kernel if a.route == "kernel" else chain
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        eager, graphed = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(300):
                fn()
            e1.record()
            torch.cuda.synchronize()
            eager.append(e0.elapsed_time(e1) * 1e3 / 300)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(50):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            graphed.append(e0.elapsed_time(e1) * 1e3 / 1000)
        out[str(T)] = {"eager_us": [round(v, 2) for v in eager], "graph_us": [round(v, 2) for v in graphed]}
    print("RESULT " + json.dumps({"leg": "router", "shape": a.shape, "route": a.route, "rows": out, "device": torch.cuda.get_device_name(0)}), flush=True)


def _child(a, leg, shape, route):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--shape", shape, "--route", route, "--blocks", str(a.blocks), "--reps", str(a.reps),
           "--steps", str(a.steps), "--warmup", str(a.warmup)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        raise SystemExit(f"moe_step_bench: leg {leg} {shape} {route} failed (rc={res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    print(lines[-1], flush=True)
    return json.loads(lines[-1][len("RESULT "):])


def _med(vals):
    return round(statistics.median(vals), 2)


def markdown(res) -> str:
    rows = ["# Mixtral and Qwen3-MoE through the fused decode step (opt-in), and the router launch", "",
            f"`tools/moe_step_bench.py` on {res['device']}.  Every leg in a process of its own; two passes that alternate the routes; per leg {res['reps']} repetitions.  "
            f"Random-weight fp16 models of {res['blocks']} decoder blocks (the real models have 32 and 48), experts and attention linears int4, group_size 64, axis 1:",
            "", "- `mixtral`: Mixtral-8x7B's block — hidden 4096, 32 / 8 heads of 128, 8 experts of 14336, top-2, vocab 32000",
            "- `qwen3_moe`: a Qwen3-MoE-30B-like block — hidden 2048, 32 / 4 heads of 128, 128 experts of 768, top-8, norm_topk_prob, vocab 151936", "",
            "## Decode step", "",
            f"tok/s of {res['steps']} timed graph replays after {res['warmup']} warm-up steps (`GraphedGreedyDecoder.benchmark`, HIP events), prompt of 16 tokens, attention "
            "`sdpa`.  With so few blocks the lm_head and the front of the step weigh far more than in the real models: the ratio says what the step saves per block "
            "only together with the block count.", "",
            "| shape | route | tok/s, pass 1 | tok/s, pass 2 | median | spread (max - min) |", "|---|---|---|---|---|---|"]
    for shape, st in res["step"].items():
        for route in ("model", "fused"):
            p = st[route]
            allv = p[0] + p[1]
            rows.append(f"| {shape} | `moe=\"{route}\"` | {', '.join(map(str, p[0]))} | {', '.join(map(str, p[1]))} | {_med(allv)} | {round(max(allv) - min(allv), 2)} |")
        rows.append(f"| {shape} | fused / model (medians) | | | {st['speedup_median']} | beyond the larger spread: {st['fused_faster_beyond_spread']}; same 16 tokens: {st['same_tokens_16']} |")
    rows += ["", "## Router launch", "",
             "`ops.moe_router` (one launch) against the torch chain it replaces (`F.linear`, `softmax`, `topk`, `sum`, `div`; Qwen3-MoE: the cast), us per call, "
             "median over both passes.  eager: 300 calls from Python between two HIP events (host-bound for the chain); graph: a captured graph of 50 calls, replayed 20 times.", "",
             "| shape | rows | kernel, eager | torch, eager | kernel, graph | torch, graph | torch / kernel (graph) |", "|---|---|---|---|---|---|---|"]
    for shape, rt in res["router"].items():
        for T in ("1", "16"):
            ke, te, kg, tg = (_med(rt[r][0][T][m] + rt[r][1][T][m]) for r, m in (("kernel", "eager_us"), ("torch", "eager_us"), ("kernel", "graph_us"), ("torch", "graph_us")))
            rows.append(f"| {shape} | {T} | {ke} | {te} | {kg} | {tg} | {round(tg / kg, 2)} |")
    if res.get("notes"):
        rows += ["", "## Notes", ""] + [f"- {n}" for n in res["notes"]]
    rows.append("")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=("step", "router"))
    ap.add_argument("--shape", default="mixtral", choices=tuple(SHAPES))
    ap.add_argument("--route", default="fused", choices=("model", "fused", "kernel", "torch"))
    ap.add_argument("--out", default="profiles/moe_step_bench.json")
    ap.add_argument("--md", default=None)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--leg-timeout", type=int, default=600)
    ap.add_argument("--shapes", default="mixtral,qwen3_moe")
    ap.add_argument("--note", action="append", default=[], help="a line for the record's Notes section (what else was measured around this run)")
    a = ap.parse_args()
    if a.leg == "step":
        return leg_step(a)
    if a.leg == "router":
        return leg_router(a)
    shapes = a.shapes.split(",")
    res = {"tool": "moe_step_bench", "blocks": a.blocks, "reps": a.reps, "steps": a.steps, "warmup": a.warmup, "notes": a.note, "step": {}, "router": {}}
    for shape in shapes:
        res["router"][shape] = {"kernel": [], "torch": []}
        res["step"][shape] = {"model": [], "fused": []}
    tokens = {}
    for _ in range(2):   # two passes, the routes alternating
        for shape in shapes:
            for route in ("torch", "kernel"):
                r = _child(a, "router", shape, route)
                res["router"][shape][route].append(r["rows"])
                res["device"] = r["device"]
            for route in ("model", "fused"):
                r = _child(a, "step", shape, route)
                res["step"][shape][route].append(r["tok_s"])
                tokens[shape, route] = r["tokens"]
    for shape in shapes:
        st = res["step"][shape]
        m, f = st["model"][0] + st["model"][1], st["fused"][0] + st["fused"][1]
        st["speedup_median"] = round(statistics.median(f) / statistics.median(m), 3)
        st["fused_faster_beyond_spread"] = bool(statistics.median(f) - statistics.median(m) > max(max(m) - min(m), max(f) - min(f)))
        st["same_tokens_16"] = tokens[shape, "model"] == tokens[shape, "fused"]
    with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
