"""The LoRA merge kernel's contract restated on the CPU, and the cases the GPU tests run (tests/test_lora_merge_cpu.py, tests/test_lora_merge_gpu.py).

`merged_reference` is include/hqq_hip.h's definition of hqq_hip_lora_merge in torch float32 elementwise ops: the rank-r product is a loop over j with a
separate `*` and `+` (each a materialised fp32 tensor: no fused multiply-add, no matmul, no addcmul), then the roundings of the torch statements it
stands for — `(A @ B * scaling).t().to(W.dtype)` added to W.  Everything is compared with torch.equal: there is no tolerance to choose.

Case shapes are the smallest at which the kernel (tile 64 n x 128 k, 8 k per thread, j staged in chunks of 32) can go wrong:
  48 x 192, group_size 64   two k tiles, the second half empty; a partial n tile; every bit width and both axes
  40 x 72, group_size 8     partial tiles on both edges; 8-element runs that are exactly one group (axis 1)
  136 x 200, group_size 8   3 x 2 tiles, both edges partial; 200 = 128 + 72
  24 x 100, group_size 20   K no multiple of 8: scalar stores, a 4-element last run, rows that start off 16 bytes, runs that cross a group edge
  25 x 100, 3-bit, gs 20    13 packed rows x 20: the slab edges (260, 520, ...) fall inside 8-element runs
ranks 1, 3, 17 (odd, below a chunk), 64 (two full chunks), 256 (the largest; eight chunks); 33 would add nothing over 17 + 64.
"""
import itertools

import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
PACK_DTYPE = {8: torch.uint8, 4: torch.uint8, 3: torch.int32, 2: torch.uint8, 1: torch.uint8}
PER = {8: 1, 4: 2, 3: 10, 2: 4, 1: 8}


def merged_reference(W, A, B, scaling, L, T):
    """W [N, K] in T (the base weight: dequantize()'s bits, or a dense weight), A [K, r], B [r, N] in L, scaling a number -> the merged [N, K] in T.
    CPU tensors."""
    assert W.dtype == T and A.dtype == L and B.dtype == L and not W.is_cuda
    A32, B32 = A.float(), B.float()
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=F32)
    for j in range(A.shape[1]):
        prod = A32[:, j:j + 1] * B32[j:j + 1, :]      # fmul_rn, materialised
        acc = acc + prod                               # fadd_rn
    m = acc.to(L)                                      # the matmul's result in the adapter's dtype
    s = (m.float() * torch.tensor(float(scaling), dtype=F32)).to(L)   # * scaling: an fp32 product, rounded to the adapter's dtype
    d = s.t().to(T)                                    # .t().to(W.dtype)
    return (W.float() + d.float()).to(T)               # W += d: one rounding in T


def packed_elements(nbits, N, K, gs, axis):
    """element count of the reference's container for a [N, K] weight"""
    groups = N * K // gs
    urows, ucols = (groups, gs) if axis == 1 else (gs, groups)
    prow = (urows + 9) // 10 if nbits == 3 else urows // PER[nbits]
    return prow * ucols


def synthetic_layer(nbits, N, K, gs, axis, T, seed):
    """a container of random levels with meta that dequantises to weights of about N(0, 0.02^2)'s spread: zero near the middle level, scale so that the
    level range spans +-3.5 sigma.  CPU tensors (W_q, scale, zero); scale / zero flat, N K / gs elements in T."""
    g = torch.Generator().manual_seed(seed)
    n = packed_elements(nbits, N, K, gs, axis)
    if nbits == 3:
        W_q = torch.randint(0, 1 << 30, (n,), generator=g, dtype=torch.int32)
    else:
        W_q = torch.randint(0, 256, (n,), generator=g, dtype=torch.int32).to(torch.uint8)
    top = float(2 ** nbits - 1)
    groups = N * K // gs
    zero = (top / 2 + (torch.rand(groups, generator=g) - 0.5) * max(top / 4, 0.5)).to(T)
    scale = (0.14 / top * (1 + 0.2 * torch.rand(groups, generator=g))).to(T)
    return W_q, scale, zero


def adapter(K, N, r, L, seed):
    """entries of about 0.05 in magnitude, random (no sum of them is exact)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K, r, generator=g) * 0.05).to(L), (torch.randn(r, N, generator=g) * 0.05).to(L)


RANKS = [1, 3, 17, 64, 256]
DTYPES = [(T, L) for T in (F16, BF16) for L in (F32, F16, BF16)]

# (nbits, axis, N, K, group_size, r, T, L); nbits 0: the dense base
CASES = []
# every bit width and axis at the main shape and at the edge shape
for nbits, axis in itertools.product((8, 4, 3, 2, 1), (0, 1)):
    CASES.append((nbits, axis, 48, 192, 64, 17, F16, F32))
    CASES.append((nbits, axis, 40, 72, 8, 3, BF16 if axis else F16, F16 if axis else BF16))
# every rank x every dtype pair: int4 axis 1 at the main shape, and the dense base at the edge shape
for r, (T, L) in itertools.product(RANKS, DTYPES):
    CASES.append((4, 1, 48, 192, 64, r, T, L))
    CASES.append((0, 0, 40, 72, 0, r, T, L))
# several tiles each way, both edges partial
for nbits, axis in ((4, 1), (4, 0), (2, 1), (0, 0)):
    CASES.append((nbits, axis, 136, 200, 8 if nbits else 0, 64, F16, F32))
# K no multiple of 8; runs that cross a group edge / a slab edge
for nbits, axis, N in ((4, 1, 24), (4, 0, 24), (8, 1, 24), (3, 1, 25), (3, 0, 25), (0, 0, 24)):
    CASES.append((nbits, axis, N, 100, 20 if nbits else 0, 17, BF16, F32))


def case_id(c):
    nbits, axis, N, K, gs, r, T, L = c
    base = "dense" if nbits == 0 else f"{nbits}b-axis{axis}-gs{gs}"
    return f"{base}-{N}x{K}-r{r}-{str(T)[6:]}-{str(L)[6:]}"


def exact_adapter(K, N, r, seed):
    """adapter values whose every product and partial sum is exact in fp32 (multiples of 1/16 up to 15/16 in magnitude, r <= 8: products are multiples of
    2^-8 below 1, sums of 8 stay below 8): the order of a GEMM's summation cannot matter, so a library matmul and the kernel's loop agree bit for bit"""
    assert r <= 8
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-15, 16, (K, r), generator=g).float() / 16
    B = torch.randint(-15, 16, (r, N), generator=g).float() / 16
    return A, B
