#!/usr/bin/env python3
"""One SHA-256 of the output bytes per case of the MFMA-tile attention family (csrc/attn_tile.hip, attn_gqa.hip, attn_prefill.hip), on a GPU:
    python tools/attn_bits.py > bits.txt
Run on two trees and compare the lists: it pins a refactor of those kernels (same bits as before), not a contract — the contract is the GPU suite's.
The inputs are the suite's case builders (tests/_tile_cases.py, _gqa_cases.py, _prefill_cases.py), seeded on the CPU.  The cases are the smallest at which the
kernels can go wrong: head_dim 64 / 128 / 256 x fp16 / bf16, a cache of 104 positions, 70 visible keys (a share ends inside a 32-key block, off a multiple of 16).
  tiled    5 rows, one of them at position 1 (at 3 splits its later shares are empty), 8 query heads over 2 KV heads, 1 and 3 splits
  grouped  2 sequences (70 and 41 keys), 8 query heads over 2 KV heads, 1 and 3 splits, on the dense, the 8-bit and the 4-bit cache
  prompt   21 rows at pos0 = 3: two tiles, the last of 5 rows, on the dense, the 8-bit and the 4-bit cache"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _gqa_cases as gc      # noqa: E402
import _prefill_cases as pc  # noqa: E402
import _tile_cases as tc     # noqa: E402
from hqq_amd import ops      # noqa: E402

L, HEADS, DEV = 104, (8, 2), "cuda"


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def gpu(t: dict) -> dict:
    return {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in t.items()}


def packed(K: torch.Tensor, V: torch.Tensor, hd: int, nbits: int):
    """K, V [B, n_kv, L, hd] quantised whole into six fresh buffers"""
    bufs = ops.kv_alloc(K.shape[0], K.shape[1], K.shape[2], hd, nbits, ops.kv_group_size(hd), K.dtype, K.device)
    ops.kv_quantize(K, V, bufs, 0)
    return bufs


def main() -> None:
    for hd in tc.HDS:
        for dt in tc.DTS:
            sc = hd ** -0.5
            qscale = 0.25 if hd == 256 else 1.0
            for S in (1, 3):
                case = tc.Case("random", dt, hd, L, (69, 1, 33, 68, 50), S, heads=HEADS, seed=11, qscale=qscale)
                t = gpu(tc.build(case, "cpu", fill=0.0))
                out = torch.full_like(t["q"], float("nan"))
                ops.attn_decode_tiled(t["q"], t["K"], t["V"], t["pos"], out, sc, splits=S)
                print(f"tiled   {dt} hd{hd} S{S} dense {sha(out)}")
            for S in (1, 3):
                case = gc.Case("random", dt, hd, L, HEADS, (69, 40), S, seed=12)
                t = gpu(gc.build(case, "cpu", fill=0.0))
                for fmt in ("dense", "q8", "q4"):
                    out = torch.full_like(t["q"], float("nan"))
                    if fmt == "dense":
                        ops.attn_decode_gqa_batched(t["q"], t["K"], t["V"], t["pos"], out, sc, splits=S)
                    else:
                        ops.attn_decode_gqa_kvq_batched(t["q"], packed(t["K"], t["V"], hd, int(fmt[1])), t["pos"], out, sc, hd, splits=S)
                    print(f"grouped {dt} hd{hd} S{S} {fmt} {sha(out)}")
            case = pc.Case(dt, hd, L, HEADS, 3, 21, seed=13)
            t = gpu(pc.build(case, "cpu", fill=0.0))
            for fmt in ("dense", "q8", "q4"):
                if fmt == "dense":
                    out = pc.prefill(t)
                else:
                    out = pc.prefill_kvq(t, packed(t["K"][None], t["V"][None], hd, int(fmt[1])))
                print(f"prompt  {dt} hd{hd} S1 {fmt} {sha(out)}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
