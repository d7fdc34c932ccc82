#!/usr/bin/env python3
"""Write tests/golden/lora_merge_*.npz: what the REFERENCE (mobiusml/hqq) computes when a LoRA adapter is merged into a quantised layer and the
result is quantised again (hqq/core/peft.py:167-190), on the CPU at fp16.

    HQQ_REFERENCE=<checkout of mobiusml/hqq> python tests/golden/make_merge_golden.py

HQQLinearLoRA.merge_and_quantize itself cannot run without a CUDA device (its `HQQLinear(None, quant_config)` takes the constructor's default device,
"cuda"), so the script runs its three statements on the reference's own functions:
  base weight   Quantizer.dequantize of the seeded layer Quantizer.quantize produced (compute dtype fp16, meta cast as HQQLinear.cuda casts it) — what the
                identity pushed through the forward returns
  merge         `W += (torch.matmul(lora_A, lora_B) * scaling).t().to(W.dtype)`, verbatim
  re-quantise   Quantizer.quantize(W, **weight_quant_params, device="cpu", compute_dtype=float16)
The adapter's values are multiples of 1/64 below 1/4 in magnitude and r <= 8: every product and every partial sum of A @ B is exact in fp32, so the
GEMM's summation order cannot matter and the file pins ONE result.  The script asserts that (the float64 product equals the float32 one) before it
writes anything.

Each file holds arrays only: the packed layer (W_q, scale, zero in fp16), its dequantised weight, lora_A / lora_B (fp32), scaling, bias, the merged
weight (fp16), and the re-quantised W_q / scale / zero as Quantizer.quantize returned them (fp32 meta), plus nbits / group_size / axis / shape.
tests/test_lora_merge_cpu.py and tests/test_lora_merge_gpu.py read them without the reference.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _import_reference  # noqa: E402
from _merge_cases import exact_adapter  # noqa: E402

# name -> (nbits, axis, N, K, group_size, r, lora_alpha, seed)
CASES = {
    "lora_merge_4b_axis1_32x128": (4, 1, 32, 128, 64, 8, 16, 11),
    "lora_merge_2b_axis0_32x128": (2, 0, 32, 128, 64, 4, 8, 12),
}


def main():
    Quantizer, _, BaseQuantizeConfig, _ = _import_reference()
    for name, (nbits, axis, N, K, gs, r, alpha, seed) in CASES.items():
        wq = BaseQuantizeConfig(nbits=nbits, group_size=gs, axis=axis)["weight_quant_params"]
        torch.manual_seed(seed)
        W0 = (torch.randn(N, K) * 0.02).half()
        W_q0, meta0 = Quantizer.quantize(W0, device="cpu", compute_dtype=torch.float16, **wq)
        meta0["scale"], meta0["zero"] = meta0["scale"].half(), meta0["zero"].half()   # HQQLinear.cuda: the meta in the compute dtype
        base = Quantizer.dequantize(W_q0, meta0).clone()
        assert base.dtype == torch.float16 and tuple(base.shape) == (N, K)

        A, B = exact_adapter(K, N, r, seed + 100)
        A, B = A / 4, B / 4           # multiples of 1/64 below 1/4
        scaling = alpha / r
        P32 = torch.matmul(A, B)
        assert torch.equal(P32.double(), torch.matmul(A.double(), B.double())), "A @ B is not exact in fp32"
        bias = (torch.randn(N) * 0.1).half()

        W = base.clone()
        W += (torch.matmul(A, B) * scaling).t().to(W.dtype)   # peft.py:179-183
        merged = W.clone()
        W_q1, meta1 = Quantizer.quantize(W, device="cpu", compute_dtype=torch.float16, **wq)   # peft.py:188

        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(
            path, nbits=np.int64(nbits), axis=np.int64(axis), group_size=np.int64(gs), shape=np.array([N, K], np.int64),
            W_q=W_q0.numpy(), scale=meta0["scale"].reshape(-1).numpy(), zero=meta0["zero"].reshape(-1).numpy(), base=base.numpy(),
            lora_A=A.numpy(), lora_B=B.numpy(), scaling=np.float64(scaling), lora_alpha=np.int64(alpha), bias=bias.numpy(), merged=merged.numpy(),
            merged_W_q=W_q1.numpy(), merged_scale=meta1["scale"].reshape(-1).float().numpy(), merged_zero=meta1["zero"].reshape(-1).float().numpy())
        print(f"  {name}.npz  {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
