#!/usr/bin/env python3
"""What serving several LoRA adapters over one quantised base costs, measured three ways (needs an MI355X).  The model of (ii) and (iii) is
tools/lora_step_bench.py's: random-weight, Llama-2-7B-shaped (hidden 4096, 32 blocks, 32 heads of 128, intermediate 11008, vocab 32000, fp16, seed 20260),
every decoder linear int4, group_size 64, axis 1, adapters of rank 16 in fp16 on all seven linears of every block (lora_B = 0.02 randn).

Legs:
    kernels   (i) the price of routing.  The adapter launches of ONE decoder block at 7B shapes — q|k|v (K 4096 -> 3 x 4096), o (4096 -> 4096), gate|up
              (4096 -> 2 x 11008), down (11008 -> 4096): four shrink + four expand launches — captured once in a graph that holds 32 such blocks and replayed;
              `single` is ops.lora_shrink + ops.lora_expand, `routed` ops.lora_shrink_routed + ops.lora_expand_routed on a bank of 4 adapters with UNIFORM slots
              (every row adapter 0).  Rank 16 and 64 (fp16 adapters), B = 1 / 8 / 16.  us per block.
    step      (ii) the batched decode step at B = 8 / 16: `bank` — GraphedGreedyDecoder(lora="fused", lora_bank=bank), the SAME captured graphs timed with 1, 4
              and B distinct adapters among the rows (only step.slots is rewritten in between); `single` — today's lora="fused" step, one adapter for all rows.
              ms per step and aggregate tok/s.  The bank leg also reports the wall time of generate_batch on a mixed batch (B prompts of 16 tokens, 64 new
              tokens, 4 distinct adapters, kept state), for (iii).
    statusquo (iii) a mixed batch without the bank: B = 8 prompts under 4 distinct adapters, per adapter PeftUtils.load_lora_weights(file) (the decoder's
              fingerprint changes: step and graphs are rebuilt) + generate_batch of that adapter's prompts, 64 new tokens.  Total wall time, first round (with the
              first captures) and second round (every adapter loaded again: rebuilt again).

    python tools/lora_bank_bench.py [--passes 2] [--legs kernels,step,statusquo] [--out profiles/lora_bank_bench.json] [--md profiles/lora_bank_summary.md]
        The driver: every measurement in a process of its own under its own time limit (--limit), the legs alternated `passes` times so that the spread shows.  A
        child that is killed or runs into its limit ends the whole run (nothing further is started on the GPU); the tables then say what was not measured.
    python tools/lora_bank_bench.py --leg kernels --kind routed --rank 16 --batch 8        one measurement, one JSON line (what the driver starts)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
H, I = 4096, 11008
GROUPS = ((H, (H, H, H)), (H, (H,)), (H, (I, I)), (I, (H,)))   # (K, the N of each adapted member): q|k|v, o, gate|up, down
BANK_N = 16       # adapters in the step legs' bank (B = 16 rows can each take another one)
NEW, PROMPT = 64, 16


def kernels_worker(a):
    import torch
    from hqq_amd import ops
    dev, dt, B, r, na = "cuda", torch.float16, a.batch, a.rank, 4
    g = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    slots = torch.zeros(B, dtype=torch.int64, device=dev)
    work = []
    for K, Ns in GROUPS:
        x = rnd(B, K).to(dt)
        banks = [((rnd(na, K, r) / K ** 0.5).to(dt), (0.02 * rnd(na, r, N)).to(dt), torch.full((na,), 2.0, device=dev)) for N in Ns]
        ys = [rnd(B, N).to(dt) for N in Ns]
        ws = ops.lora_decode_workspace(dev, B, K, [r] * len(Ns))
        if a.kind == "routed":
            work.append(lambda x=x, banks=banks, ys=ys, ws=ws: ops.lora_apply_routed(x, banks, slots, ys, workspace=ws))
        else:
            one = [(A[0].contiguous(), Bm[0].contiguous(), 2.0) for A, Bm, _ in banks]
            work.append(lambda x=x, one=one, ys=ys, ws=ws: ops.lora_apply(x, one, ys, workspace=ws))
    blocks = 32

    def model_pass():
        for _ in range(blocks):
            for f in work:
                f()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model_pass()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        model_pass()
    for _ in range(a.warmup):
        graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (a.steps * blocks)
    print(json.dumps({"leg": "kernels", "kind": a.kind, "rank": r, "batch": B, "us_per_block": round(us, 2), "launches_per_block": 2 * len(GROUPS),
                      "steps": a.steps, "device": torch.cuda.get_device_name(0)}), flush=True)


def adapter_params(model, seed):
    """one adapter for the model's wrappers, as PeftUtils.save_lora_weights would write it ("parameters"), on the wrappers' device"""
    import torch
    from hqq_amd.core.peft import is_hqq_lora_layer
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = {}
    for name, m in model.named_modules():
        if is_hqq_lora_layer(m):
            out[name] = {"lora_A": (torch.randn(m.lora_A.shape, device="cuda", generator=g) / m.in_features ** 0.5).to(m.lora_A.dtype),
                         "lora_B": (0.02 * torch.randn(m.lora_B.shape, device="cuda", generator=g)).to(m.lora_B.dtype), "scaling": float(m.scaling), "bias": None}
    return out


def step_worker(a):
    import torch
    from lora_step_bench import build
    from hqq_amd.core.peft import LoRABank
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    B = a.batch
    model = build(1, 16, "f16", "fused", a.blocks)
    ids = torch.randint(0, 32000, (B, PROMPT), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    res = {"leg": "step", "kind": a.kind, "batch": B, "blocks": a.blocks, "steps": a.steps, "device": torch.cuda.get_device_name(0)}
    if a.kind == "single":
        dec = GraphedGreedyDecoder(model, max_cache_len=512, lora="fused")
        r = dec.benchmark_batch(ids, new_tokens=a.steps, warmup=a.warmup)
        assert dec._batch[B]["step"].lora and dec._batch[B]["step"].lora_bank is None
        res["ms_per_step"] = {"1": round(r["ms_per_step"], 4)}
    else:
        first = adapter_params(model, 100)
        bank = LoRABank.from_params(model, [first] * BANK_N)
        for i in range(1, BANK_N):
            bank.set(i, adapter_params(model, 100 + i))
        res["bank_bytes"] = bank.nbytes
        dec = GraphedGreedyDecoder(model, max_cache_len=512, lora="fused", lora_bank=bank)
        res["ms_per_step"] = {}
        for distinct in (1, 4, B):
            slots = [i % distinct for i in range(B)]
            dec.generate_batch(list(ids), 3, adapters=slots)
            st = dec._batch[B]
            assert st["step"].lora_bank is bank and st["step"].slots.tolist() == slots
            res["ms_per_step"][str(distinct)] = round(dec._timed_steps(st, PROMPT + 2, a.steps, a.warmup), 4)
        mixed = [i % 4 for i in range(B)]
        dec.generate_batch(list(ids), NEW, adapters=mixed)   # (every cache bucket of the run has its graph now)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.generate_batch(list(ids), NEW, adapters=mixed)
        torch.cuda.synchronize()
        res["mixed_batch_wall_s"] = round(time.perf_counter() - t0, 3)
    res["tok_s"] = {k: round(B * 1e3 / v, 1) for k, v in res["ms_per_step"].items()}
    print(json.dumps(res), flush=True)


def statusquo_worker(a):
    import torch
    from lora_step_bench import build
    from hqq_amd.core.peft import PeftUtils
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    B, distinct = a.batch, 4
    model = build(1, 16, "f16", "fused", a.blocks)
    ids = torch.randint(0, 32000, (B, PROMPT), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with tempfile.TemporaryDirectory() as d:
        files = []
        for i in range(distinct):
            files.append(os.path.join(d, f"adapter{i}.pt"))
            torch.save({"peft_config": model.peft_config, "parameters": {k: {n: (t.cpu() if hasattr(t, "cpu") else t) for n, t in v.items()}
                                                                         for k, v in adapter_params(model, 100 + i).items()}}, files[-1])
        dec = GraphedGreedyDecoder(model, max_cache_len=512, lora="fused")
        rounds = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, f in enumerate(files):
                PeftUtils.load_lora_weights(model, f)
                mine = [ids[b] for b in range(B) if b % distinct == i]
                dec.generate_batch(mine, NEW)
            torch.cuda.synchronize()
            rounds.append(round(time.perf_counter() - t0, 3))
    print(json.dumps({"leg": "statusquo", "batch": B, "distinct": distinct, "blocks": a.blocks, "new_tokens": NEW, "wall_s_first_round": rounds[0],
                      "wall_s_second_round": rounds[1], "device": torch.cuda.get_device_name(0)}), flush=True)


# a record kept by hand (the code it measured is gone): appended to every summary the driver writes
FIRST_DESIGN = """
## The design that was not kept: a walk over the distinct adapters inside one workgroup

The routed kernels were first built the other way the grid can be cut: workgroup (slice, layer) staged x once, listed the distinct adapters among the rows' slots in LDS
and walked them one after the other, each row's `fmaf` predicated on the adapter being walked.  Same bits, same tests passed.  Measured once, in processes of their own as
above (rank 64 for the kernels, the same model and bank for the step), before it was replaced:

| | walk inside the workgroup | grid dimension over rows (kept; tables above) |
|---|---|---|
| (i) rank 64, B = 8, uniform slots: us per block, routed (single: 116.7) | 143.6 | 135.8 |
| (ii) B = 8: ms per step with 1 / 4 / 8 distinct adapters | 6.09 / 10.48 / 16.14 | 6.02 / 5.86 / 5.90 |
| (iii) mixed `generate_batch`, B = 8, 4 adapters: s | 0.94 | 0.63 |

The shrink grid at 7B shapes is 16 slices x at most 3 layers — a fraction of the device's compute units — so serialising the adapters inside those few workgroups made the
launch grow with every further adapter, while a grid dimension runs them side by side on units that were idle.  What the grid dimension costs is the workgroups that find
no adapter to serve (at uniform slots all but one in B), which is table (i)'s 1.03-1.26x.
"""


def run_child(args, limit):
    cmd = [sys.executable, os.path.abspath(__file__)] + [str(x) for x in args]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, f"ran into its limit of {limit} s"
    if p.returncode != 0:
        return None, f"exit status {p.returncode}: {(p.stderr or p.stdout)[-300:].strip()}"
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]), ""


def spread(v):
    return f"{statistics.median(v):.4g} ({min(v):.4g}–{max(v):.4g})" if v else "not measured"


def markdown(res) -> str:
    out = ["# Several LoRA adapters over one quantised base: what the bank costs", "",
           f"`tools/lora_bank_bench.py` on {res.get('device', 'an MI355X')}; every figure is the median of {res['passes']} alternating passes, each in a process of its own, "
           "with (min–max).", "",
           "## (i) The routed launches against the existing ones at uniform slots", "",
           "The adapter launches of one decoder block at 7B shapes (four shrink + four expand launches over q|k|v, o, gate|up, down; fp16 adapters), from a captured graph "
           f"of 32 blocks replayed {res['steps_kernels']} times.  `routed` reads a bank of 4 adapters, every row adapter 0.  The 32 blocks of the graph read the same "
           "tensors, so both sides run cache-warm.  us per block.", "",
           "| rank | B | single | routed | routed / single (medians) |", "|---|---|---|---|---|"]
    for key, kinds in res["kernels"].items():
        s, r = kinds.get("single", []), kinds.get("routed", [])
        ratio = f"{statistics.median(r) / statistics.median(s):.3f}" if s and r else "not measured"
        rank, B = key.split(":")
        out.append(f"| {rank} | {B} | {spread(s)} | {spread(r)} | {ratio} |")
    out += ["", "## (ii) The batched decode step with 1, 4 and B distinct adapters", "",
            f"Random-weight Llama-2-7B-shaped model ({res['blocks']} blocks, int4, group_size 64, axis 1, fp16; adapters of rank 16 in fp16 on all seven linears), a bank of "
            f"{BANK_N} adapters.  `bank` times the same captured graphs after rewriting `step.slots`; `single` is the existing `lora=\"fused\"` step (one adapter for all rows).  "
            "ms per step.", "",
            "| B | single (1 adapter) | bank, 1 distinct | bank, 4 distinct | bank, B distinct |", "|---|---|---|---|---|"]
    for B, kinds in res["step"].items():
        bank = kinds.get("bank", {})
        out.append(f"| {B} | {spread(kinds.get('single', {}).get('1', []))} | {spread(bank.get('1', []))} | {spread(bank.get('4', []))} | {spread(bank.get(B, []))} |")
    out += ["", "## (iii) A mixed batch: the bank against the status quo", "",
            f"8 prompts of {PROMPT} tokens under 4 distinct adapters, {NEW} new tokens each.  Status quo: per adapter `PeftUtils.load_lora_weights` (which makes the decoder "
            "rebuild its step and graphs) + `generate_batch` of that adapter's two prompts; total wall time of a first round and of a second round over the same four files.  "
            "Bank: one `generate_batch(prompts, adapters=...)` on kept state.  Seconds.", "",
            "| | wall time |", "|---|---|",
            f"| status quo, first round | {spread(res['statusquo'].get('first', []))} |",
            f"| status quo, second round | {spread(res['statusquo'].get('second', []))} |",
            f"| bank, one mixed `generate_batch` (B = 8) | {spread(res['bank_wall'])} |", ""]
    if res.get("stopped"):
        out += [f"The run was stopped: {res['stopped']}  Nothing was started after it; cells above say what was not measured.", ""]
    return "\n".join(out) + FIRST_DESIGN


def driver(a):
    legs = a.legs.split(",")
    res = {"tool": "lora_bank_bench", "passes": a.passes, "blocks": a.blocks, "steps_kernels": a.steps * 4, "steps": a.steps, "kernels": {}, "step": {},
           "statusquo": {}, "bank_wall": [], "stopped": ""}
    plan = []
    for _ in range(a.passes):
        if "kernels" in legs:
            plan += [("kernels", kind, rank, B) for rank in (16, 64) for B in (1, 8, 16) for kind in ("single", "routed")]
        if "step" in legs:
            plan += [("step", kind, 16, B) for B in (8, 16) for kind in ("single", "bank")]
        if "statusquo" in legs:
            plan.append(("statusquo", "single", 16, 8))
    for leg, kind, rank, B in plan:
        steps = a.steps * 4 if leg == "kernels" else a.steps
        got, why = run_child(["--leg", leg, "--kind", kind, "--rank", rank, "--batch", B, "--steps", steps, "--warmup", a.warmup, "--blocks", a.blocks],
                             60 if leg == "kernels" else a.limit)
        if got is None:
            res["stopped"] = f"{leg} / {kind} / rank {rank} / B {B}: {why}."
            break
        res["device"] = got["device"]
        print(json.dumps(got), flush=True)
        if leg == "kernels":
            res["kernels"].setdefault(f"{rank}:{B}", {}).setdefault(kind, []).append(got["us_per_block"])
        elif leg == "step":
            for k, v in got["ms_per_step"].items():
                res["step"].setdefault(str(B), {}).setdefault(kind, {}).setdefault(k, []).append(v)
            if kind == "bank" and B == 8:
                res["bank_wall"].append(got["mixed_batch_wall_s"])
            if "bank_bytes" in got:
                res["bank_bytes"] = got["bank_bytes"]
        else:
            res["statusquo"].setdefault("first", []).append(got["wall_s_first_round"])
            res["statusquo"].setdefault("second", []).append(got["wall_s_second_round"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))
    print(json.dumps({"written": a.out, "stopped": res["stopped"]}))
    return 1 if res["stopped"] else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("kernels", "step", "statusquo"), default=None)
    ap.add_argument("--kind", choices=("single", "routed", "bank"), default="routed")
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--legs", default="kernels,step,statusquo")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default="profiles/lora_bank_bench.json")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if a.leg:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("lora_bank_bench: needs the GPU")
        return {"kernels": kernels_worker, "step": step_worker, "statusquo": statusquo_worker}[a.leg](a)
    sys.exit(driver(a))


if __name__ == "__main__":
    main()
