"""Shared by tests/test_kvq_cpu.py, tests/test_kvq_gpu.py and tests/test_kvq_step_gpu.py: a numpy restatement of the quantised KV cache's row format
(include/hqq_hip.h, csrc/kv_cache.hip) — quantise, pack, unpack and dequantise in the compute dtype —, the rows the tests run it on, and the error bound of
a round trip.

A row of head_dim values in the compute dtype T is viewed as [head_dim / gs, gs] and quantised as Quantizer.quantize(optimize=False, round_zero=False) does
(hqq/core/quantize.py:102-154), in float32:
    denom = max - min; scale = (1 / denom) * max_v (Tensor.__rtruediv__: reciprocal, then the product); scale = 1 where |denom| <= 1e-4; scale = min(scale, 2e4);
    zero = -min * scale; level = clip(rint(w * scale + zero), 0, max_v), product and sum rounded separately; stored scale = 1 / scale
and scale / zero are then cast to T.  8 bits: byte i is level i; 4 bits: byte i is level[i] << 4 | level[i + head_dim / 2].  Dequantisation is
round_T(round_T(q - zero) * scale).  bf16 values travel as raw uint16 (numpy has no bfloat16), fp16 as np.float16.
"""
from __future__ import annotations

import numpy as np

F16, BF16 = 1, 2
UNIT = {F16: 2.0 ** -11, BF16: 2.0 ** -8}   # unit roundoff of T: half an ulp relative, 11 and 8 significant bits

# (head_dim, gs): 64 with 32, 128 with 64 and with 32, one 256 case
SHAPES = ((64, 32), (128, 64), (128, 32), (256, 64))


def bf16_round(a32: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bits (uint16), round to nearest even; a NaN stays a NaN"""
    x = np.ascontiguousarray(a32, np.float32).view(np.uint32)
    nan = (x & 0x7FFFFFFF) > 0x7F800000
    r = ((x.astype(np.uint64) + 0x7FFF + ((x >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(nan, ((x >> 16) | 0x40).astype(np.uint16), r)


def to_cd(a32: np.ndarray, code: int) -> np.ndarray:
    """float32 -> T, one rounding (fp16: np.float16; bf16: raw uint16)"""
    with np.errstate(over="ignore"):
        return np.asarray(a32, np.float32).astype(np.float16) if code == F16 else bf16_round(a32)


def from_cd(a: np.ndarray, code: int) -> np.ndarray:
    """T -> float32, exact"""
    if code == F16:
        return np.asarray(a).view(np.float16).astype(np.float32)
    return (np.asarray(a).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def quantize_rows(x_cd: np.ndarray, code: int, nbits: int, gs: int):
    """rows [R, head_dim] of T -> (levels [R, head_dim] uint8, scale [R, head_dim / gs] of T, zero likewise)"""
    R, hd = x_cd.shape
    max_v = np.float32(2 ** nbits - 1)
    w = from_cd(x_cd, code).reshape(R, hd // gs, gs)
    one = np.float32(1.0)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        mn, mx = w.min(axis=2, keepdims=True), w.max(axis=2, keepdims=True)
        denom = (mx - mn).astype(np.float32)
        sc = ((one / denom).astype(np.float32) * max_v).astype(np.float32)
        sc = np.where(np.abs(denom) <= np.float32(1e-4), one, sc)
        sc = np.where(sc > np.float32(2e4), np.float32(2e4), sc).astype(np.float32)
        ze = ((-mn) * sc).astype(np.float32)
        q = (w * sc).astype(np.float32)
        q = (q + ze).astype(np.float32)
        q = np.clip(np.rint(q), 0, max_v)
        inv = (one / sc).astype(np.float32)
    return q.reshape(R, hd).astype(np.uint8), to_cd(inv[..., 0], code), to_cd(ze[..., 0], code)


def pack_rows(levels: np.ndarray, nbits: int) -> np.ndarray:
    """levels [R, head_dim] -> the stored bytes [R, head_dim * nbits / 8]"""
    if nbits == 8:
        return levels.astype(np.uint8).copy()
    half = levels.shape[1] // 2
    return ((levels[:, :half].astype(np.uint8) << 4) | levels[:, half:].astype(np.uint8)).astype(np.uint8)


def unpack_rows(packed: np.ndarray, nbits: int) -> np.ndarray:
    if nbits == 8:
        return packed.astype(np.uint8).copy()
    return np.concatenate([packed >> 4, packed & 0xF], axis=1).astype(np.uint8)


def dequantize_rows(levels: np.ndarray, scale_cd: np.ndarray, zero_cd: np.ndarray, code: int, gs: int) -> np.ndarray:
    """round_T(round_T(q - zero) * scale) -> rows [R, head_dim] of T.  fp16: each op exact in float64, rounded once to fp16 (what v_sub_f16 / v_mul_f16 give);
    bf16: each op in float32, then rounded to bf16 (how torch evaluates a bf16 elementwise op)"""
    R, hd = levels.shape
    q = levels.reshape(R, hd // gs, gs)
    with np.errstate(over="ignore", invalid="ignore"):
        if code == F16:
            z = np.asarray(zero_cd).view(np.float16).astype(np.float64)[..., None]
            s = np.asarray(scale_cd).view(np.float16).astype(np.float64)[..., None]
            d = (q.astype(np.float64) - z).astype(np.float16)
            return (d.astype(np.float64) * s).astype(np.float16).reshape(R, hd)
        z, s = from_cd(zero_cd, code)[..., None], from_cd(scale_cd, code)[..., None]
        d = from_cd(bf16_round((q.astype(np.float32) - z).astype(np.float32)), code)
        return bf16_round((d * s).astype(np.float32)).reshape(R, hd)


def special_rows(hd: int, gs: int, nbits: int, code: int, seed: int = 0) -> np.ndarray:
    """rows of T whose groups exercise every branch of the rule: random, a constant group, a range below 1e-4, a group that hits the 2e4 clamp (a range just above
    1e-4: max_v / range > 2e4), negative-only and positive-only groups — one kind per row, the kind in group g only, the other groups random"""
    rng = np.random.default_rng(seed)
    G = hd // gs
    kinds = ("random", "constant", "tiny", "clamp", "negative", "positive")
    rows = []
    for kind in kinds:
        for g in range(G):
            r = rng.standard_normal(hd).astype(np.float32)
            seg = slice(g * gs, (g + 1) * gs)
            if kind == "constant":
                r[seg] = 0.75
            elif kind == "tiny":      # neighbours of 2^-8 in T, one ulp apart (fp16 2^-18, bf16 2^-15): a range below 1e-4 that is not 0
                r[seg] = 2.0 ** -8 + rng.integers(0, 2, gs) * (2.0 ** -18 if code == F16 else 2.0 ** -15)
                r[g * gs], r[g * gs + 1] = 2.0 ** -8, 2.0 ** -8 + (2.0 ** -18 if code == F16 else 2.0 ** -15)
            elif kind == "clamp":     # range 3 * 2^-13 = 3.7e-4 (three bf16 ulps at 2^-6): above 1e-4, and max_v / range > 2e4 at both widths (15 / 3.7e-4 = 4.1e4)
                r[seg] = 2.0 ** -6 + rng.integers(0, 4, gs) * 2.0 ** -13
                r[g * gs], r[g * gs + 1] = 2.0 ** -6, 2.0 ** -6 + 3 * 2.0 ** -13
            elif kind == "negative":
                r[seg] = -np.abs(r[seg]) - 0.5
            elif kind == "positive":
                r[seg] = np.abs(r[seg]) + 0.5
            rows.append(r)
        if kind == "random":
            rows = rows[:1] + [rng.standard_normal(hd).astype(np.float32) * 4.0 for _ in range(3)]
    x = np.stack(rows)
    return to_cd(x, code)


def roundtrip_bound(x32: np.ndarray, gs: int, nbits: int, code: int) -> np.ndarray:
    """|x - dequant(quant(x))| <= this, element by element, where no scale is clamped (group range > max(1e-4, max_v / 2e4)) and nothing leaves T's normal range.
    With h = 1 / scale the step (float32), u = UNIT[T], the stored scale h (1 + e1), the stored zero z0 (1 + e2) (z0 = -min * scale), d = (q - z)(1 + e3) and
    out = d s (1 + e4), every |e| <= u:
        out = [(q - z0) - z0 e2] h (1 + e1)(1 + e3)(1 + e4),      x = (q - z0) h + r, |r| <= h / 2 (x lies inside [min, max]: no level is clipped)
        |out - x| <= h / 2 + |q - z0| h ((1 + u)^3 - 1) + |z0| h u (1 + u)^3,       |q - z0| h <= |x| + h / 2,      |z0| h = |min| (1 + O(2^-23))
    plus the float32 roundings of scale, zero, the product and the sum inside the level computation: each at most 2^-23 relative on a quantity of at most
    max_v + |z0| levels, i.e. (max_v + |z0|) h 2^-21 in all, which moves x by that much before rint and can add as much to r."""
    R, hd = x32.shape
    w = x32.reshape(R, hd // gs, gs).astype(np.float64)
    u = UNIT[code]
    max_v = 2 ** nbits - 1
    mn, mx = w.min(axis=2, keepdims=True), w.max(axis=2, keepdims=True)
    h = (mx - mn) / max_v
    a = (1 + u) ** 3
    z0h = np.abs(mn)
    b = h / 2 + (np.abs(w) + h / 2) * (a - 1) + z0h * u * a + (max_v * h + z0h) * 2.0 ** -21 * 2
    return b.reshape(R, hd)
