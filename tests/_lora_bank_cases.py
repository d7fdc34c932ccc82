"""Shared by tests/test_lora_routed_gpu.py and tests/test_lora_bank_cpu.py: the cases that pin the routed adapter kernels of csrc/lora_decode.hip
(hqq_hip_lora_shrink_routed, hqq_hip_lora_expand_routed) — shapes, banks of stacked adapters, slot patterns.  Nothing here imports GPU code.

The reference of every check on these cases is the EXISTING pair (ops.lora_shrink + ops.lora_expand) on one row with one adapter, bit for bit: the routed
kernels promise that pair's bits per row, so no tolerance appears anywhere.  The shapes are _lora_decode_cases' edges that the routing could disturb:
  three      K 520 (three 256-k slices at r <= 64, the last of 8 k); layers (r, N) = (8, 64), (17, 264) — a rank that is no power of two, two expand tiles with
             a ragged second one —, (3, 8)
  four       the same with (64, 256): the most layers a call takes, and a rank that fills the column stride
  r130       K 1040, r 130, N 64: the 1024-k slices of ranks above 128 (one whole slice and one of 16 k)
  r128       K 1040, r 128, N 64: the 512-k slices of ranks 65 .. 128 (two whole slices and one of 16 k)
A bank holds 3 adapters; activations x adapters run over _lora_decode_cases.PAIRS.
Slot patterns (one int64 per row; anything outside [0, 3) names no adapter):
  M 1        [2]
  M 5        [0, 1, 2, 0, 1] (every adapter, two of them twice), [1, 1, 1, 1, 1] (uniform: the existing M-row call is the reference too),
             [2, -1, 0, 3, -7] (the documented -1, the first index past the bank, another negative)
  M 16       the three adapters interleaved, two -1 and one 2**40 among them
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import torch

import _lora_decode_cases as D

N_ADAPTERS = 3
PAIRS = D.PAIRS

SHAPES = {
    # name: (K, ((r, N), ...))
    "three": (520, ((8, 64), (17, 264), (3, 8))),
    "four": (520, ((8, 64), (17, 264), (3, 8), (64, 256))),
    "r130": (1040, ((130, 64),)),
    "r128": (1040, ((128, 64),)),
}

SLOTS = {
    "M1": [2],
    "M5-all": [0, 1, 2, 0, 1],
    "M5-uniform": [1, 1, 1, 1, 1],
    "M5-invalid": [2, -1, 0, 3, -7],
    "M16": [0, 1, 2, -1, 1, 0, 2, 2 ** 40, 2, 1, 0, -1, 0, 2, 1, 0],
}
assert len(SLOTS["M16"]) == 16 and SLOTS["M16"].count(-1) == 2 and SLOTS["M16"].count(2 ** 40) == 1 and {0, 1, 2} <= set(SLOTS["M16"])


def valid(slot: int) -> bool:
    return 0 <= slot < N_ADAPTERS


@dataclass(frozen=True)
class Case:
    shape: str
    dt: torch.dtype
    ldt: torch.dtype
    slots: str

    @property
    def id(self) -> str:
        return f"{self.shape}-{str(self.dt)[6:]}x{str(self.ldt)[6:]}-{self.slots}"

    @property
    def K(self) -> int:
        return SHAPES[self.shape][0]

    @property
    def layers(self) -> tuple:
        return SHAPES[self.shape][1]

    @property
    def M(self) -> int:
        return len(SLOTS[self.slots])


CASES = [Case(sh, dt, ldt, sl) for sh in SHAPES for dt, ldt in PAIRS for sl in SLOTS]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES) == 80


@functools.lru_cache(maxsize=None)
def inputs(case_id: str):
    """(x [M, K] in T, [(A [3, K, r], B [3, r, N] in L, scaling fp32 [3], y0 [M, N] in T)]) as CPU tensors; computed once, shared, never modified.
    x ~ N(0, 1), A ~ N(0, 1 / K), B ~ N(0, 0.05^2), y0 ~ N(0, 1); the scalings differ per adapter and layer and are no powers of two"""
    case = BY_ID[case_id]
    g = torch.Generator().manual_seed(2000 + sum(map(ord, case.shape)))
    x = torch.randn(case.M, case.K, generator=g).to(case.dt)
    layers = []
    for l, (r, N) in enumerate(case.layers):
        A = (torch.randn(N_ADAPTERS, case.K, r, generator=g) / case.K ** 0.5).to(case.ldt)
        B = (torch.randn(N_ADAPTERS, r, N, generator=g) * 0.05).to(case.ldt)
        s = torch.tensor([1.25 + 0.75 * a + 0.3 * l for a in range(N_ADAPTERS)], dtype=torch.float32)
        layers.append((A, B, s, torch.randn(case.M, N, generator=g).to(case.dt)))
    return x, layers
