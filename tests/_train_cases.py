"""Shared by tests/test_train_cpu.py and tests/test_train_gpu.py: the cases that pin the TRAINING path's gradients — HQQLinear's autograd route
(hqq_hip_gemm_dgrad where HQQLinear._dgrad_kernel_ok sends it, dequantise + matmul elsewhere) and HQQLinearLoRA — against float64, element by
element, with bounds derived from the arithmetic each route documents.  Nothing here imports GPU code.

Layer weights (layer_weight): 0.02 randn, +0.08 on the first third of the output rows, -0.08 on the second third.  Every group of those rows lies on
one side of 0, where the solver emits what hand-built meta never held: zero-points below 0 (a positive group: zero = -min * scale) and above the
largest level (a negative one).  zero_point_kinds() reads the premise off the built meta; the GPU file asserts it for every axis-1 layer (an axis-0
group is a column of the flat [gs, -1] view and strides over all thirds of the rows: there only the finiteness of the meta is asserted).

Shapes (N, K, gs): (96, 192, 64) an odd number of the dgrad kernel's 64-wide k tiles, N / per = 24 packed rows for 2-bit (a ragged 32-row step);
(128, 256, 32) two groups inside one 64-wide k tile.  Rows: 1, R, R + 1 with R = ops.DGRAD_ROUTE_MAX_M as the module has it (the GPU file reads
it, nothing patches it), a 3-D input (2, R // 2, K) and a zero-row input.

References: plain float64 functions of tensors (ref_dx, ref_lora).

Bounds (every compared element has its own, computed in float64 from absolute values; nothing is fitted to a result):
  a contraction of length n accumulated in fp32, in ANY order, is within gamma(n) = n 2^-24 / (1 - n 2^-24) times the sum of absolute products
  (products of two fp16 / bf16 values are exact in fp32; fp32 products cost one of the n roundings, as in the textbook bound);
  a rounding to a dtype T is within U[T] / 2 of the value rounded (U = 2^-10 fp16, 2^-7 bf16, 2^-23 fp32), plus one smallest subnormal of T;
  an error E already on an operand propagates through its absolute co-factor (mm_bound).
No term carries a multiplier; the arithmetic modelled is, per route:
  bare layer        x.grad = round_T(sum_n go W) — one rounding, one contraction over N (both the dgrad kernel and dequantise + matmul)
  wrapper, x.grad   round_T(round_T(sum_n go W) + round_T(lora part)) — three roundings (dgrad result, cast of the LoRA branch, autograd's add)
  wrapper, adapters with R the train dtype, every product rounded once to R (for fp32 that rounding is the "fp32 u on the result"):
                    xd = round_R(x m), h = round_R(xd A), gl = round_R(go s), B.grad = round_R(h^T gl), dh = round_R(gl B^T),
                    A.grad = round_R(xd^T dh), lora part of x.grad = round_R(round_R(dh A^T) m), bias.grad = round_R(sum_rows go)
"""
from __future__ import annotations

import torch

SHAPES = [(96, 192, 64), (128, 256, 32)]
NBITS_ALL = [8, 4, 2, 3, 1]
NBITS_KERNEL = (8, 4, 2)                       # what hqq_hip_gemm_dgrad serves (axis 1)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
U = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
SUBNORMAL = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149, torch.float64: 0.0}
LORA_R, LORA_ALPHA = 8, 16
P_DROP = 0.25


def gamma(n: int) -> float:
    """the error constant of an fp32 contraction of length n, any summation order"""
    return n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def layer_weight(N: int, K: int, seed: int) -> torch.Tensor:
    """the nn.Linear(K, N) weight of a case, float32"""
    W = 0.02 * torch.randn(N, K, generator=torch.Generator().manual_seed(seed))
    W[:N // 3] += 0.08
    W[N // 3:2 * (N // 3)] -= 0.08
    return W


def one_signed_groups(W: torch.Tensor, gs: int, axis: int):
    """(a group lies wholly above 0, a group lies wholly below 0) in the quantiser's own grouping: [-1, gs] along axis 1, [gs, -1] along axis 0"""
    G = W.reshape(-1, gs) if axis == 1 else W.reshape(gs, -1).t()
    return bool((G > 0).all(1).any()), bool((G < 0).all(1).any())


def zero_point_kinds(zero: torch.Tensor, nbits: int):
    """(some zero-point is negative, some zero-point is above the largest level)"""
    z = zero.double()
    return bool((z < 0).any()), bool((z > 2 ** nbits - 1).any())


def row_forms(R: int, K: int):
    """name -> input shape: 1, R and R + 1 rows, the 3-D input and the zero-row input"""
    return {"1": (1, K), "R": (R, K), "R+1": (R + 1, K), "3d": (2, R // 2, K), "0": (0, K)}


def randn(shape, seed: int, dtype=torch.float32, scale: float = 1.0) -> torch.Tensor:
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def lora_init(K: int, N: int, seed: int):
    """seeded adapters, lora_B non-zero (a trained state)"""
    return {"lora_A": randn((K, LORA_R), seed, scale=0.05), "lora_B": randn((LORA_R, N), seed + 1, scale=0.05)}


def drop_mask(shape, seed: int, dtype) -> torch.Tensor:
    """a fixed dropout mask divided by (1 - p), in the dtype the wrapper multiplies in: the check does not depend on a generator's stream"""
    keep = torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) >= P_DROP
    return (keep.float() / (1.0 - P_DROP)).to(dtype)


# ---- float64 references ------------------------------------------------------------------------------------------------------------------
def ref_dx(go: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """dx = go @ W for go [*, N], W [N, K] = layer.dequantize()"""
    return go.double() @ W.double()


def ref_lora(x, go, W, A, B, s: float, mask=None) -> dict:
    """the gradients of y = x W^T + ((x m) A) B s (+ bias) for grad_output go; 2-D x [M, K] and go [M, N]; mask m [M, K] or None"""
    x, go, W, A, B = (t.double() for t in (x, go, W, A, B))
    m = torch.ones_like(x) if mask is None else mask.double()
    xd = x * m
    dh = (go @ B.t()) * s
    x_lora = (dh @ A.t()) * m
    return {"A": xd.t() @ dh, "B": (xd @ A).t() @ go * s, "bias": go.sum(0), "x_base": go @ W, "x_lora": x_lora, "x": go @ W + x_lora}


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------
def rounded(val: torch.Tensor, E, dt) -> torch.Tensor:
    """|round_dt(v') - v| for |v' - v| <= E"""
    return (U[dt] / 2) * (val.abs() + E) + E + SUBNORMAL[dt]


def mm_bound(A, EA, B, EB, dt) -> torch.Tensor:
    """|round_dt(fp32 contraction of A' B') - A B| for |A' - A| <= EA, |B' - B| <= EB (float64 tensors or 0.0)"""
    A, B = A.double(), B.double()
    aA, aB = A.abs() + EA, B.abs() + EB
    zA, zB = torch.zeros_like(A) + EA, torch.zeros_like(B) + EB
    E = gamma(A.shape[-1]) * (aA @ aB) + zA @ aB + A.abs() @ zB
    return rounded(A @ B, E, dt)


def bound_dx(go: torch.Tensor, W: torch.Tensor, dt) -> torch.Tensor:
    """bare layer: one rounding to the compute dtype plus gamma(N) sum_n |go| |W|"""
    return mm_bound(go, 0.0, W, 0.0, dt)


def bound_lora(x, go, W, A, B, s: float, dt, train_dt, mask=None) -> dict:
    """the bounds of ref_lora's entries for compute dtype dt and adapters in train_dt, following the module docstring's chain step by step"""
    x, go, W, A, B = (t.double() for t in (x, go, W, A, B))
    Rt = train_dt
    m = torch.ones_like(x) if mask is None else mask.double()
    xd = x * m
    E_xd = rounded(xd, 0.0, Rt) if mask is not None else torch.zeros_like(xd)   # (x.to(train dtype) is exact: fp16 / bf16 -> fp32, or the same dtype)
    h = xd @ A
    E_h = mm_bound(xd, E_xd, A, 0.0, Rt)
    gl = go * s
    E_gl = rounded(gl, 0.0, Rt)
    dh = gl @ B.t()
    E_dh = mm_bound(gl, E_gl, B.t(), 0.0, Rt)
    dxd = dh @ A.t()
    E_dxd = mm_bound(dh, E_dh, A.t(), 0.0, Rt)
    x_lora = dxd * m
    E_xl = rounded(x_lora, E_dxd * m, Rt) if mask is not None else E_dxd
    E_cast = rounded(x_lora, E_xl, dt)                        # rounding 2: the LoRA branch cast to the compute dtype
    x_base = go @ W
    E_base = bound_dx(go, W, dt)                              # rounding 1: the dgrad result
    ones = torch.ones(1, go.shape[0], dtype=torch.float64)
    return {"A": mm_bound(xd.t(), E_xd.t(), dh, E_dh, Rt), "B": mm_bound(h.t(), E_h.t(), gl, E_gl, Rt),
            "bias": mm_bound(ones, 0.0, go, 0.0, Rt)[0], "x_base": E_base,
            "x": rounded(x_base + x_lora, E_base + E_cast, dt)}   # rounding 3: autograd's add of the two branches


def within(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor):
    """(all inside, the worst ratio |got - want| / bound) on the host in float64"""
    r = ((got.double().cpu() - want).abs() / bound)
    return bool((r <= 1.0).all()) and bool(torch.isfinite(got.double()).all()), float(r.max()) if r.numel() else 0.0
