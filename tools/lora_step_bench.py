#!/usr/bin/env python3
"""Decode rate of a model whose LoRA adapters are still adapters, route by route (needs an MI355X).  The model is random-weight and Llama-2-7B-shaped
(hidden 4096, 32 blocks, 32 heads of 128, intermediate 11008, vocab 32000, fp16, seed 20260), every decoder linear int4, group_size 64, quantised
along axis 1 or axis 0, with adapters of rank 16 or 64 on all seven linears of every block, in fp32 or fp16 (lora_B = 0.02 randn: LoRA's own
initialiser zeroes it).

Routes:
    default   GraphedGreedyDecoder(model): the model's own forward, graph-replayed — what serves an adapted model without the opt-in (the baseline)
    fused     GraphedGreedyDecoder(model, lora="fused" [, axis0="fused"]): the fused step with lora_shrink + lora_expand behind each base launch
    ceiling   the same base WITHOUT adapters through the fused step with glue="kernels" (axis 0: axis0="fused"): what the adapters cost on top of
    merged    PeftUtils.merge_lora, then the decoder's default for a merged model (axis 0: axis0="fused"): another model (re-quantised), for scale

    python tools/lora_step_bench.py [--cases axis1:16:f32,axis1:64:f16,...] [--passes 2] [--steps 256] [--warmup 16] [--blocks 32]
                                    [--out profiles/lora_step_bench.json] [--md profiles/lora_step_summary.md] [--limit 240] [--profile DIR]
        The driver.  EVERY (case, route) measurement runs in a process of its own under its own time limit (--limit seconds): warm-up, then `steps`
        graph replays timed between device synchronisations (HIP events, GraphedGreedyDecoder.benchmark).  The routes are alternated `passes` times
        so that the spread shows.  ceiling does not depend on rank or adapter dtype: it is measured once per axis and pass.  A child that is killed
        by a signal or runs into its limit ends the whole run (nothing further is started on the GPU); the tables then say what was not measured.
        --profile DIR: additionally ONE run of the fused route of the first case under `rocprofv3 --kernel-trace --stats` (a run of its own), from
        which the two new kernels' rows are taken.
    python tools/lora_step_bench.py --route ROUTE --case axis1:16:f32 ...      one measurement, one JSON line (what the driver starts)
"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUTES = ("default", "fused", "ceiling", "merged")
ALL_CASES = [f"axis{a}:{r}:{d}" for a in (1, 0) for r in (16, 64) for d in ("f32", "f16")]
TAGS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def parse_case(c):
    a, r, d = c.split(":")
    return int(a[-1]), int(r), d


def build(axis: int, rank: int, ldt: str, route: str, blocks: int):
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.peft import PeftUtils, is_hqq_lora_layer
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=blocks, num_attention_heads=32, num_key_value_heads=32, vocab_size=32000,
                      max_position_embeddings=2048)
    dflt = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    torch.manual_seed(20260)
    try:
        with torch.device("cuda"):
            model = LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(dflt)
    qcfg = BaseQuantizeConfig(nbits=4, group_size=64, axis=axis)
    quantize_model(model, qcfg, compute_dtype=torch.float16, device="cuda")
    if route != "ceiling":
        PeftUtils.add_lora(model, {t: {"r": rank, "lora_alpha": 2 * rank, "dropout": 0.0} for t in TAGS})
        g = torch.Generator(device="cuda").manual_seed(20261)
        for m in model.modules():
            if is_hqq_lora_layer(m):
                m.lora_B.data = 0.02 * torch.randn(m.lora_B.shape, device="cuda", generator=g)
        if ldt == "f16":
            PeftUtils.cast_lora_weights(model, torch.float16)
        if route == "merged":
            PeftUtils.merge_lora(model, {t: qcfg for t in TAGS})
    prepare_for_inference(model, backend="hip")
    if axis == 1:
        group_llama_projections(model)
    return model.eval()


def worker(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lora_step_bench: needs the GPU")
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    axis, rank, ldt = parse_case(a.case)
    t0 = time.perf_counter()
    model = build(axis, rank, ldt, a.route, a.blocks)
    t_build = time.perf_counter() - t0
    kw = {"default": {}, "fused": dict(lora="fused"), "ceiling": dict(glue="kernels"), "merged": {}}[a.route]
    if axis == 0 and a.route != "default":
        kw = dict(kw, axis0="fused")
        kw.pop("glue", None)
    dec = GraphedGreedyDecoder(model, max_cache_len=512, **kw)
    ids = torch.randint(0, 32000, (1, 16), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    res = dec.benchmark(ids, new_tokens=a.steps, warmup=a.warmup)
    torch.cuda.synchronize()
    step = dec.step
    if a.route == "default":
        assert step is None
    elif a.route == "fused":
        assert step is not None and step.lora, "the lora step must serve this model"
    else:
        assert step is not None and not step.lora
    print(json.dumps({"case": a.case, "route": a.route, "tok_s": round(res["tok_s"], 2), "ms_per_token": round(res["ms_per_token"], 4), "steps": a.steps,
                      "warmup": a.warmup, "blocks": a.blocks, "build_s": round(t_build, 1), "device": torch.cuda.get_device_name(0),
                      "step": None if step is None else {"lora": bool(step.lora), "folded": bool(step.folded), "axis0": bool(step.axis0)}}), flush=True)


def child_cmd(a, case, route, steps=None):
    return [sys.executable, os.path.abspath(__file__), "--route", route, "--case", case, "--steps", str(steps or a.steps), "--warmup", str(a.warmup),
            "--blocks", str(a.blocks)]


def run_child(cmd, limit):
    """(result dict | None, note): a child that was killed or timed out returns (None, why) and the caller stops starting work"""
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, f"ran into its limit of {limit} s"
    if p.returncode != 0:
        return None, f"exit status {p.returncode}: {(p.stderr or p.stdout)[-300:].strip()}"
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line), ""


def kernel_rows(directory):
    """the rows of the two new kernels in rocprofv3's kernel stats CSV(s) under `directory`"""
    import csv
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            rows += [r for r in csv.DictReader(fh) if "lora_shrink_kernel" in r.get("Name", "") or "lora_expand_kernel" in r.get("Name", "")]
    return rows


def markdown(res) -> str:
    out = ["# Un-merged LoRA adapters in the fused decode step (opt-in)", "",
           f"`tools/lora_step_bench.py` on {res.get('device', 'an MI355X')}: random-weight Llama-2-7B-shaped model ({res['blocks']} blocks, hidden 4096, 32 heads of 128, "
           "intermediate 11008, vocab 32000, fp16), every decoder linear int4, group_size 64; adapters on all seven linears of every block.", "",
           f"Every figure is one process of its own: {res['warmup']} warm-up steps, then {res['steps']} graph replays timed between device synchronisations; "
           f"tok/s of each of the {res['passes']} alternating passes.  `default` is the model's own forward (the behaviour without the opt-in), `fused` is "
           "`lora=\"fused\"`, `ceiling` the same base without adapters through the fused step with the separate glue kernels, `merged` the re-quantised merged model.", "",
           "| case (axis : rank : adapter dtype) | default | fused | ceiling | merged | fused / default (medians) |", "|---|---|---|---|---|---|"]
    for case, routes in res["cases"].items():
        def cell(r):
            v = res["ceiling"].get(case.split(":")[0]) if r == "ceiling" else routes.get(r)
            return ", ".join(str(x) for x in v) if v else "not measured"
        d, f = routes.get("default"), routes.get("fused")
        ratio = f"{statistics.median(f) / statistics.median(d):.2f}" if d and f else "not measured"
        out.append(f"| {case} | {cell('default')} | {cell('fused')} | {cell('ceiling')} | {cell('merged')} | {ratio} |")
    out.append("")
    if res.get("stopped"):
        out += [f"The run was stopped: {res['stopped']}  Nothing was started after it; cells above say what was not measured.", ""]
    if res.get("kernels"):
        out += ["Kernel times of the two new kernels (`rocprofv3 --kernel-trace --stats`, a run of its own on the first case, fused route):", "",
                "| kernel | calls | average ns | min ns | max ns |", "|---|---|---|---|---|"]
        for k in res["kernels"]:
            out.append(f"| `{k.get('Name', '?')[:90]}` | {k.get('Calls', '?')} | {k.get('AverageNs', '?')} | {k.get('MinNs', '?')} | {k.get('MaxNs', '?')} |")
        out.append("")
    elif "kernels" in res:
        out += ["Kernel times of the two new kernels: not measured.", ""]
    return "\n".join(out)


def driver(a):
    cases = a.cases.split(",") if a.cases else ALL_CASES
    res = {"tool": "lora_step_bench", "blocks": a.blocks, "steps": a.steps, "warmup": a.warmup, "passes": a.passes, "cases": {c: {} for c in cases},
           "ceiling": {}, "stopped": ""}
    plan = []
    for p in range(a.passes):
        seen_axis = set()
        for c in cases:
            for r in a.routes.split(","):
                if r == "ceiling":
                    if c.split(":")[0] in seen_axis:
                        continue
                    seen_axis.add(c.split(":")[0])
                plan.append((c, r))
    for c, r in plan:
        got, why = run_child(child_cmd(a, c, r), a.limit)
        if got is None:
            res["stopped"] = f"{c} / {r}: {why}."
            break
        res["device"] = got["device"]
        (res["ceiling"].setdefault(c.split(":")[0], []) if r == "ceiling" else res["cases"][c].setdefault(r, [])).append(got["tok_s"])
        print(json.dumps(got), flush=True)
    if a.profile and not res["stopped"]:
        os.makedirs(a.profile, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.profile, "--"] + child_cmd(a, cases[0], "fused", steps=32)
        got, why = run_child(cmd, a.limit * 2)
        res["kernels"] = kernel_rows(a.profile) if got is not None else []
        if got is None:
            res["stopped"] = f"profile run: {why}."
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))
    print(json.dumps({"written": a.out, "stopped": res["stopped"]}))
    return 1 if res["stopped"] else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=ROUTES, default=None)
    ap.add_argument("--case", default=ALL_CASES[0])
    ap.add_argument("--cases", default=None)
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default="profiles/lora_step_bench.json")
    ap.add_argument("--md", default=None)
    ap.add_argument("--profile", default=None)
    a = ap.parse_args()
    if a.route:
        return worker(a)
    sys.exit(driver(a))


if __name__ == "__main__":
    main()
