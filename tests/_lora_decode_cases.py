"""Shared by tests/test_lora_decode_cpu.py and tests/test_lora_decode_gpu.py: the cases that pin the two kernels of csrc/lora_decode.hip
(hqq_hip_lora_shrink, hqq_hip_lora_expand), their inputs and the host references.  Nothing here imports GPU code.

What the kernels compute, for a group of layers l that read the same rows x[M, K] (include/hqq_hip.h), T the compute dtype:
    t_l[m, j] = sum_k x[m, k] A_l[k, j]            fp32
    u_l[m, n] = s_l sum_j t_l[m, j] B_l[j, n]      fp32
    y_l[m, n] = rnd_T(y0_l[m, n] + rnd_T(u_l[m, n]))

Edge families: ONE axis at its edge, the others small (M 2, K 520, r 8, N 64, one layer) — not a cross product.  The sizes follow from the kernels'
constants, restated below with their source lines:
  K       8 (less than one 16-byte load per row beyond the first); one slice exactly; one slice +- 8; several slices with a ragged last one (3 slices + 72);
          11008; the same around the 512- and 1024-k slices of the larger ranks
  r       1, 2, 3, 8, 16, 17, 64, 255, 256, and 65 / 128 / 129 where the slice size changes
  N       8; one expand tile exactly; one tile +- 8; several tiles with a ragged last one (2 tiles + 72)
  M       1, 2, 5, 16, and 4 / 8 / 9: either side of the row counts at which the kernels carry more accumulators
  groups  one layer; three layers of different r_l, N_l, s_l; four (the most a call takes)
  dtypes  fp16 x fp32, fp16 x fp16, bf16 x bf16, bf16 x fp32 (activations x adapters): every pair at the base shape, rotating over the other cases
Every shape is run as a CONSTRUCTED case (exact bits) and as a RANDN case (float64 with a derived bound).

Constructed cases.  x, A, B are small dyadic numbers given by index formulas (cx, ca, cb: quarters, quarters, halves; functions of the indices: linear with a
coefficient that is no multiple of the modulus, so that neighbouring rows and columns always differ, plus a product term that breaks the period), s a power of two, x scaled by a power of two 2^-e per case.  Every product x A is a multiple of
q1 = 2^-(4 + e), every product t B a multiple of q2 = 2^-(5 + e); exactness() checks that the sum of ABSOLUTE products of every output stays below
2^24 q — then every partial sum, in any order and with or without fused multiply-adds, is a multiple of q below 2^24 q and exact in fp32 — and that
|u| stays below T's largest finite number.  The expected bits are ((y0.float() + u.to(T).float()).to(T)) with u exact: each step rounds once, exactly
as the kernel's two statements do, so there is no tolerance.

Randn cases.  The reference is float64 on the same (already rounded) inputs: y64 = y0 + s x A B.  Bound per element, nothing fitted to a result:
  shrink: t^ is a contraction of length K accumulated in fp32 in some order (products of two inputs are exact or fused), so
          |t^ - t| <= K 2^-24 sum_k |x A|  to first order;
  expand: the sum over r terms adds r roundings, the product with s one more, and the error of t^ passes through |B|:
          |u^ - u| <= (K + r + 1) 2^-24 sum |s x A B|; two more units cover the second-order terms, hence (K + r + 3);
  rnd_T(u^) is within 2^-p |u| of u^ (p = 11 fp16, 8 bf16: half a unit in the last place, relative), plus T's smallest subnormal;
  the add rounds once more: within 2^-p (|y0| + |u|).
  bound = (K + r + 3) 2^-24 sum |s x A B| + 2^-p |u| + 2^-p (|y0| + |u|) + subnormal_T
For fp16 / bf16 adapters the kernels keep t and u in fp32 where the reference rounds them to the adapter's dtype: the bound is about the VALUE, which is
the same; HQQLinearLoRA.forward itself would miss it.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch

# ---- the kernels' constants, restated ----------------------------------------------------------------------------------------------------------
THREADS = 256        # threads per workgroup of both kernels (lora_decode.hip:42 LD_THREADS)
KC = 256             # k per staged chunk of x (lora_decode.hip:43 LD_KC)
EN = 256             # columns per expand workgroup (lora_decode.hip:44 LD_EN)
MAX_R = 256          # lora_decode.hip:45 LD_MAX_R
MAX_M = 16           # lora_decode.hip:46 LD_MAX_M = HQQ_GEMV_MAX_M (include/hqq_hip.h:110)
MAX_GROUP = 4        # HQQ_GEMV_MAX_GROUP (include/hqq_hip.h:112)
ROW_STEPS = (1, 4, 8, 16)   # accumulators per thread (lora_decode.hip:53 ld_rows)


def kslice(r: int) -> int:
    """k per slice (lora_decode.hip:50 ld_kslice)"""
    return 256 if r <= 64 else (512 if r <= 128 else 1024)


def slices(K: int, r: int) -> int:
    """lora_decode.hip:51 ld_slices"""
    return -(-K // kslice(r))


def workspace_bytes(M: int, K: int, rs) -> int:
    """[layer][slice][M][r_l] fp32, rounded up to 16 bytes (lora_decode.hip ld_workspace_bytes)"""
    return (sum(slices(K, r) * M * r for r in rs) * 4 + 15) & ~15


F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
PAIRS = [(F16, F32), (F16, F16), (BF16, BF16), (BF16, F32)]       # (activations, adapters)
P_BITS = {F16: 11, BF16: 8}
SUBNORMAL = {F16: 2.0 ** -24, BF16: 2.0 ** -133}
FMAX = {F16: 65504.0, BF16: float(torch.finfo(BF16).max)}


@dataclass(frozen=True)
class Case:
    name: str
    kind: str            # "constructed" | "randn"
    dt: torch.dtype
    ldt: torch.dtype
    M: int
    K: int
    layers: tuple        # ((r, N, s), ...)

    @property
    def id(self) -> str:
        return f"{self.kind}-{self.name}-{str(self.dt)[6:]}x{str(self.ldt)[6:]}"


BASE = dict(M=2, K=520, layers=((8, 64, 2.0),))
THREE = ((8, 64, 2.0), (17, 264, 0.5), (3, 8, 4.0))
FOUR = THREE + ((64, 256, 1.0),)


def _shapes():
    out = []
    for K in (8, 256, 248, 264, 840, 11008):
        out.append((f"K{K}", dict(BASE, K=K)))
    for r, Ks in ((128, (512, 520)), (256, (1024, 1032))):
        for K in Ks:
            out.append((f"K{K}-r{r}", dict(BASE, K=K, layers=((r, 64, 2.0),))))
    out.append(("K11008-r64", dict(BASE, K=11008, layers=((64, 64, 2.0),))))
    for r in (1, 2, 3, 8, 16, 17, 64, 65, 128, 129, 255, 256):
        out.append((f"r{r}", dict(BASE, layers=((r, 64, 2.0),))))
    for N in (8, 256, 248, 264, 584):
        out.append((f"N{N}", dict(BASE, layers=((8, N, 2.0),))))
    for M in (1, 2, 4, 5, 8, 9, 16):
        out.append((f"M{M}", dict(BASE, M=M, layers=((17, 264, 2.0),))))
    out.append(("group3", dict(BASE, M=5, K=840, layers=THREE)))
    out.append(("group4", dict(BASE, M=2, K=264, layers=FOUR)))
    return out


def _cases():
    out = []
    for kind in ("constructed", "randn"):
        for dt, ldt in PAIRS:
            out.append(Case("base", kind, dt, ldt, **BASE))
            out.append(Case("group3-base", kind, dt, ldt, M=5, K=840, layers=THREE))
        for i, (name, kw) in enumerate(_shapes()):
            dt, ldt = PAIRS[i % len(PAIRS)]
            layers = kw["layers"]
            if kind == "randn":   # (randn cases need no power of two)
                layers = tuple((r, N, s * 1.25) for r, N, s in layers)
            out.append(Case(name, kind, dt, ldt, kw["M"], kw["K"], layers))
    return out


CASES = _cases()
CONSTRUCTED = [c for c in CASES if c.kind == "constructed"]
RANDN = [c for c in CASES if c.kind == "randn"]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES) <= 300


# ---- constructed inputs --------------------------------------------------------------------------------------------------------------------------
def cx(m, k):
    """x[m, k] before scaling: quarters in [-1, 1]"""
    return ((m * 7 + k * 2 + (m * k) % 5) % 9 - 4) / 4.0


def ca(k, j, l):
    """A_l[k, j]: quarters in [-3/4, 3/4]"""
    return ((k * 3 + j * 5 + (k * j) % 11 + 3 * l) % 7 - 3) / 4.0


def cb(j, n, l):
    """B_l[j, n]: halves in [-1, 1]"""
    return ((j * 3 + n * 2 + (j * n) % 7 + 2 * l) % 5 - 2) / 2.0


def cy(m, n, l):
    """y0_l[m, n]: eighths in [-2, 2]"""
    return ((m * 5 + n * 3 + (m * n) % 7 + l) % 33 - 16) / 8.0


def _grid(f, rows, cols, *a):
    i, j = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), indexing="ij")
    return f(i, j, *a).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _constructed(case: Case):
    x = _grid(cx, case.M, case.K)
    layers = [(_grid(ca, case.K, r, l), _grid(cb, r, N, l), s, _grid(cy, case.M, N, l)) for l, (r, N, s) in enumerate(case.layers)]
    # e: x is scaled by 2^-e so that |u| stays within 2^12 (every dtype's largest finite number is far above; y0 still matters in the sum)
    top = max(float(np.abs(s * ((x @ A) @ B)).max()) for A, B, s, _ in layers)
    e = 0
    while top / 2 ** e > 2 ** 12:
        e += 1
    return x / 2 ** e, layers, e


def constructed_arrays(case: Case):
    """(x, [(A, B, s, y0)], e) as float64 arrays (shared: not to be modified); every value is exactly representable in fp16 and bf16"""
    return _constructed(case)


def exactness(case: Case):
    """for a constructed case: (largest sum of |x A| in units of q1, largest sum of |t B| in units of q2, largest |u| / T's largest finite number);
    the first two must stay below 2^24, the third below 1"""
    x, layers, e = constructed_arrays(case)
    q1, q2 = 2.0 ** -(4 + e), 2.0 ** -(5 + e)
    w1 = w2 = w3 = 0.0
    for A, B, s, _ in layers:
        w1 = max(w1, float((np.abs(x) @ np.abs(A)).max()) / q1)
        w2 = max(w2, float(((np.abs(x) @ np.abs(A)) @ np.abs(B)).max()) / q2)
        w3 = max(w3, float(np.abs(s * ((x @ A) @ B)).max()) / FMAX[case.dt])
    return w1, w2, w3


def _finish(y0: torch.Tensor, u64: np.ndarray, dt) -> torch.Tensor:
    """the kernels' two statements on an exact u: rnd_T(y0 + rnd_T(u)), through fp32 as the kernel goes"""
    u = torch.from_numpy(u64).to(F32)
    assert torch.equal(u.double(), torch.from_numpy(u64)), "u is not exact in fp32"
    return (y0.float() + u.to(dt).float()).to(dt)


def constructed_expected(case: Case, displace=None):
    """expected outputs [y_l] of a constructed case.  displace (for the sensitivity checks, layer 0 only): ("A_row", k) — row k of A replaced by row
    k + 1 (cyclic); ("B_col", n) — column n of B replaced by column n + 1 (cyclic); ("slice", i) — the partial t of K slice i replaced by that of
    slice i + 1 (cyclic; by zero where there is one slice)"""
    x, layers, _ = constructed_arrays(case)
    out = []
    for l, (A, B, s, y0) in enumerate(layers):
        r = A.shape[1]
        if displace is not None and l == 0 and displace[0] == "A_row":
            A = A.copy()
            A[displace[1]] = _grid(ca, case.K, r, l)[(displace[1] + 1) % case.K]
        if displace is not None and l == 0 and displace[0] == "B_col":
            B = B.copy()
            B[:, displace[1]] = _grid(cb, r, B.shape[1], l)[:, (displace[1] + 1) % B.shape[1]]
        ks, S = kslice(r), slices(case.K, r)
        parts = [x[:, i * ks:(i + 1) * ks] @ A[i * ks:(i + 1) * ks] for i in range(S)]
        if displace is not None and l == 0 and displace[0] == "slice":
            i = displace[1]
            parts[i] = parts[(i + 1) % S] if S > 1 else np.zeros_like(parts[i])
        t = sum(parts)
        out.append(_finish(torch.from_numpy(y0).to(case.dt), s * (t @ B), case.dt))
    return out


# ---- randn inputs --------------------------------------------------------------------------------------------------------------------------------
def randn_arrays(case: Case):
    """(x in T, [(A, B in L, s, y0 in T)]) as CPU tensors; x ~ N(0, 1), A ~ N(0, 1 / K), B ~ N(0, 0.05^2), y0 ~ N(0, 1)"""
    g = torch.Generator().manual_seed(1000 + sum(map(ord, case.name)))
    x = torch.randn(case.M, case.K, generator=g).to(case.dt)
    layers = []
    for r, N, s in case.layers:
        A = (torch.randn(case.K, r, generator=g) / case.K ** 0.5).to(case.ldt)
        B = (torch.randn(r, N, generator=g) * 0.05).to(case.ldt)
        layers.append((A, B, s, torch.randn(case.M, N, generator=g).to(case.dt)))
    return x, layers


def reference64(x, A, B, s, y0):
    """(y64, bound) of one layer: the float64 value on the given inputs and the derived bound of this file's head, per element"""
    dt = y0.dtype
    K, r = A.shape
    xd, Ad, Bd, yd = x.double(), A.double(), B.double(), y0.double()
    u = float(s) * ((xd @ Ad) @ Bd)
    absum = abs(float(s)) * ((xd.abs() @ Ad.abs()) @ Bd.abs())
    half = 2.0 ** -P_BITS[dt]
    bound = (K + r + 3) * 2.0 ** -24 * absum + half * u.abs() + half * (yd.abs() + u.abs()) + SUBNORMAL[dt]
    return yd + u, bound


@functools.lru_cache(maxsize=None)
def inputs(case_id: str):
    """(x, [(A, B, s, y0)]) of a case as CPU tensors in its dtypes; computed once, shared, never modified"""
    case = BY_ID[case_id]
    if case.kind == "randn":
        return randn_arrays(case)
    x, layers, _ = constructed_arrays(case)
    to = lambda a, dt: torch.from_numpy(a).to(dt)   # noqa: E731
    xt = to(x, case.dt)
    assert torch.equal(xt.double(), torch.from_numpy(x))
    return xt, [(to(A, case.ldt), to(B, case.ldt), s, to(y0, case.dt)) for A, B, s, y0 in layers]


@functools.lru_cache(maxsize=None)
def expected(case_id: str):
    """constructed: [y_l] expected bits; randn: [(y64_l, bound_l)].  Computed once, shared, never modified"""
    case = BY_ID[case_id]
    if case.kind == "constructed":
        return constructed_expected(case)
    x, layers = inputs(case_id)
    return [reference64(x, A, B, s, y0) for A, B, s, y0 in layers]


def emulate_fp32(x, A, B, s, y0):
    """the kernels' arithmetic in numpy float32 with ANOTHER summation order (the BLAS's blocked order over all of K at once, no K slices): what the
    bound must hold for whatever the order is"""
    dt = y0.dtype
    t = x.float().numpy() @ A.float().numpy()
    u = np.float32(s) * (t @ B.float().numpy())
    return (y0.float() + torch.from_numpy(u).to(dt).float()).to(dt)
