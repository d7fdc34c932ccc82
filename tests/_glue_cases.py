"""Float64 restatements, bands, cases and checks of the decode step's base glue kernels (csrc/block.hip: add_rmsnorm, rope_cache, silu_mul, token_prologue,
argmax_advance; element arithmetic csrc/block_math.h) — tests/test_glue_cpu.py proves them on the host, tests/test_glue_gpu.py holds the kernels to them.
numpy only: nothing here runs on a device, and no torch op stands on the reference side.  16-bit values travel as uint16 bit patterns; T = "fp16" | "bf16".

Double rounding.  For a + b and a * b of two values of T, the float64 result rounded ONCE to T (what this file computes) has the bits of both evaluations
the kernels use: fp32 arithmetic then one round-to-nearest-even to T (El<true>, torch's bf16 ops), and native half arithmetic (El<false>).  Reason: rounding
the exact sum / product of two p-bit numbers first to a format of q >= 2 p + 2 significand bits and then to p bits equals rounding once (Figueroa, "When is
double rounding innocuous?", 1995); fp32 has q = 24 >= 2 * 11 + 2 = 24 for fp16 and >= 2 * 8 + 2 for bf16, float64 has q = 53.  So add, mul, rope_pair, the
residual add and every copy have ONE expected bit pattern: no tolerance.  (The argument covers +, * only: a float64 -> T CONVERSION of an arbitrary value
through fp32 is not innocuous, which is why round_f16 / round_bf16 round float64 directly.)

Bands stand only where a transcendental sits in the chain; every figure is derived here or measured by tools/glue_ulp.hip (output: profiles/glue_ulp.txt).

SiLU.  The kernel forms s32 = fl(x / fl(1 + e^)), e^ = expf(-x) = e (1 + t), |t| <= EXPF_ULPS 2^-23 (an error of E ulps is at most E 2^-23 relative).
  1 + e^ = (1 + e)(1 + t e / (1 + e)), e / (1 + e) < 1: relative error below EXPF_ULPS 2^-23;  the rounding of 1 + e^: 2^-24 relative;  the division: block.hip is
  built with -O3 -std=c++17 -ffp-contract=off and nothing else (csrc/Makefile: no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt), so hipcc's default
  correctly rounded fp32 division holds: half an ulp of the quotient.  A relative error rho is at most 2 rho 2^23 ulps (|s| < 2 * 2^23 ulp(s)), hence
      |s32 - s| <= SILU_BAND_ULPS ulp32(s),   SILU_BAND_ULPS = 1.01 (2 EXPF_ULPS + 1 + 0.5),   ulp32 floored at 2^-149
  (1.01: the products of two of these terms, below 2^-45 relative, and the float64 reference's own 2^-52).  A result e^ below 2^-126 may carry any error up to
  2^-126 without changing fl(1 + e^) = 1; the tool reports the subnormal results of expf apart (ulp floored at 2^-149), and EXPF_SEEN_ULPS is the worst of all.  Where s is exactly +-0 the
  kernel's quotient is exact too (0 / y; x / inf): no band, the sign is compared.
  fp32 range: where exp(-x) rounds to +inf in fp32, the formula gives x / inf: -0 for a finite x < 0 (gates below about -88.72), NaN for x = -inf.  This is the
  rule of torch's own fp32 formula x / (1 + exp(-x)) (tests/test_glue_cpu.py holds it to torch's CPU result), not a concession to the kernel: HF computes SiLU
  in fp32 whatever T, so a bf16 gate of -89, whose exact SiLU -2e-37 is a normal bf16 number, gives -0 there too.
  A gate pattern is DECIDED when T(s - band) and T(s + band) have the same bits; the kernel must give those bits.  Otherwise either of the two is allowed.

RMSNorm.  The kernel forms r^ = rsqrtf(fl(fl(S^ / H) + eps)), S^ an fp32 sum of the H squares (each exact in fp32: 2 * 11 <= 24 bits) in an order of its own:
  |S^ - S| <= (H - 1) 2^-24 S (all terms non-negative);  / H and + eps: 2^-24 each, not amplified (both terms positive);  so the argument is within (H + 1) 2^-24
  and r within (H + 1) 2^-25 relative;  rsqrtf within RSQRTF_ULPS 2^-23 relative;  and the fp32 product x * r^ that is rounded to T was rounded to fp32 first
  (El::r_prod): 2^-24 relative, as if r had moved by that much.  Together
      delta(H) = 1.01 ((H + 1) 2^-25 + RSQRTF_ULPS 2^-23 + 2^-24)
  and the kernel's output lies, in T's ordering, between the reference evaluated at r (1 - delta) and at r (1 + delta): T(x r) is monotone in r, and so is the
  product with a fixed weight.  Where every partial sum is exact in fp32 (the dispatch-edge cases) the reference takes / H and + eps in numpy float32 and the
  first term drops out.  An element is DECIDED when both ends have the same bits.
"""
from __future__ import annotations

import math

import numpy as np

F16, BF16 = "fp16", "bf16"
TYPES = (F16, BF16)
_FMT = {F16: (11, -14, 0x7C00, 0x7E00), BF16: (8, -126, 0x7F80, 0x7FC0)}   # significand bits, exponent of the smallest normal number, +inf, a quiet NaN

# tools/glue_ulp.hip on an MI355X, block.hip's flags; its output is profiles/glue_ulp.txt
EXPF_SEEN_ULPS = 0.9670     # profiles/glue_ulp.txt: the worst of all four EXPF figures (normal results 0.7760 fp16 / 0.7605 bf16; results below 2^-126 0.9670 / 0.8017)
RSQRTF_SEEN_ULPS = 0.8598   # profiles/glue_ulp.txt: 0.8598 over the 2^22 sampled arguments, 0.6382 over the cases' own 154
EXPF_ULPS = math.ceil(EXPF_SEEN_ULPS * 4) / 4      # the sweep is exhaustive over the kernel's arguments: the seen error is the bound, rounded up to the next 0.25 ulp
RSQRTF_ULPS = 2.0 * RSQRTF_SEEN_ULPS               # the sweep is sampled: twice the seen error
SILU_BAND_ULPS = 1.01 * (2.0 * EXPF_ULPS + 1.5)
FP32_OVER = (2.0 - 2.0 ** -24) * 2.0 ** 127        # float64 values from here on round to +inf in fp32


def rms_delta(H, exact_sum=False):
    return 1.01 * ((0.0 if exact_sum else (H + 1) * 2.0 ** -25) + RSQRTF_ULPS * 2.0 ** -23 + 2.0 ** -24)


# ---- bit patterns <-> float64 ----------------------------------------------------------------------------------------------------------------------------
def widen(bits, T):
    """the float64 value of every bit pattern (exact)"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    if T == F16:
        return b.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):   # (a signalling NaN pattern widens to a quiet one: the value is not used as a payload)
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _round(x, T):
    p, emin, inf, nan = _FMT[T]
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    fin = np.isfinite(a)
    a0 = np.where(fin, a, 0.0)
    _, ex = np.frexp(a0)                                          # a0 = m 2^ex, m in [0.5, 1)
    e = np.maximum(ex.astype(np.int64) - 1, emin)                 # exponent of the binade; subnormals share the smallest normal's quantum
    scaled = np.ldexp(a0, (-(e - (p - 1))).astype(np.int32))      # a0 in units of its quantum: exact (a power of two)
    n = np.rint(scaled)                                           # ties to even
    bits = np.where(a0 == 0.0, 0, ((e - emin) << (p - 1)) + n.astype(np.int64))   # n = 2^p carries into the exponent field by itself
    bits = np.minimum(bits, inf)                                  # overflow to infinity
    bits = np.where(fin, bits, np.where(np.isnan(x), nan, inf))
    return (bits | (np.signbit(x).astype(np.int64) << 15)).astype(np.uint16)


def round_f16(x64):
    """float64 -> fp16 bits: round to nearest even, subnormals, overflow to inf, NaN, the sign of zero kept"""
    return _round(x64, F16)


def round_bf16(x64):
    """float64 -> bf16 bits, as round_f16"""
    return _round(x64, BF16)


def rnd(x64, T):
    return _round(x64, T)


def is_nan(bits, T):
    return (np.asarray(bits, dtype=np.uint16) & 0x7FFF) > _FMT[T][2]


def is_finite(bits, T):
    return (np.asarray(bits, dtype=np.uint16) & 0x7FFF) < _FMT[T][2]


def same(a, b, T):
    """bit equality; any NaN equals any NaN (payloads are not compared), the sign of zero is compared"""
    a, b = np.asarray(a, dtype=np.uint16), np.asarray(b, dtype=np.uint16)
    return (a == b) | (is_nan(a, T) & is_nan(b, T))


def order_key(bits):
    """T's ordering on non-NaN patterns as integers: -0 directly below +0"""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int32)
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -1 - mag, mag)


def ulp32(x64):
    """the fp32 ulp at |x|, floored at 2^-149"""
    _, ex = np.frexp(np.abs(np.where(np.isfinite(x64), x64, 1.0)))
    return np.ldexp(1.0, np.maximum(ex.astype(np.int32) - 24, -149))


def all_patterns():
    return np.arange(65536, dtype=np.uint16)


def sentinel(shape, salt=0):
    """a per-element fill no kernel output reproduces by accident: finite values in [2, 4) of either format, different from slot to slot"""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt)
    return (0x4000 + ((i * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(0x3FF))).astype(np.uint16).reshape(shape)


def bits_of(values, T):
    return rnd(np.asarray(values, dtype=np.float64), T)


def max_finite(T):
    return np.uint16(_FMT[T][2] - 1)


def random_finite(n, T, rng):
    """random finite patterns: the exponent field uniform over T's whole range (log-uniform magnitudes, subnormals included), random signs"""
    p = _FMT[T][0]
    n_exp = _FMT[T][2] >> (p - 1)
    return ((rng.integers(0, 2, n) << 15) | (rng.integers(0, n_exp, n) << (p - 1)) | rng.integers(0, 1 << (p - 1), n)).astype(np.uint16)


# ---- element arithmetic (csrc/block_math.h) ----------------------------------------------------------------------------------------------------------------
def add(a, b, T):
    with np.errstate(all="ignore"):
        return rnd(widen(a, T) + widen(b, T), T)


def mul(a, b, T):
    with np.errstate(all="ignore"):
        return rnd(widen(a, T) * widen(b, T), T)


def neg(a):
    return np.asarray(a, dtype=np.uint16) ^ np.uint16(0x8000)


def rope_pair(x1, x2, c1, c2, s1, s2, T, rule=None):
    """block_math.h rope_pair: q * cos + rotate_half(q) * sin, rotate_half = cat(-x2, x1); three roundings per output, the negation exact.
    rule: a deliberately wrong variant (tests of the tests)"""
    if rule == "cos_i_both":
        c2, s2 = c1, s1
    if rule == "flip_rotate_half":
        return add(mul(x1, c1, T), mul(x2, s1, T), T), add(mul(x2, c2, T), mul(neg(x1), s2, T), T)
    return add(mul(x1, c1, T), mul(neg(x2), s1, T), T), add(mul(x2, c2, T), mul(x1, s2, T), T)


# ---- silu_mul ------------------------------------------------------------------------------------------------------------------------------------------------
def silu64(gate, T):
    """s = x / (1 + exp(-x)) in float64 with the formula's fp32 range (header)"""
    x = widen(gate, T)
    with np.errstate(all="ignore"):
        e = np.exp(-x)
        e = np.where(e >= FP32_OVER, np.inf, e)
        return x / (1.0 + e)


def silu_bounds(gate, T, band=None):
    """(lo, hi) bits of T(silu(gate)): T(s - band), T(s + band); equal where the pattern is decided"""
    band = SILU_BAND_ULPS if band is None else band
    s = silu64(gate, T)
    with np.errstate(all="ignore"):
        w = np.where(np.isfinite(s) & (s != 0.0), band * ulp32(s), 0.0)
        return rnd(np.where(w > 0, s - w, s), T), rnd(np.where(w > 0, s + w, s), T)   # (-0) + 0 would lose the sign


def silu_ref(gate, up, T, rule=None):
    """T(T(s) * up), s rounded from float64"""
    if rule == "sigmoid_rounded":    # x * sigmoid(x) with sigmoid rounded to T (a wrong rule)
        x = widen(gate, T)
        with np.errstate(all="ignore"):
            S = mul(gate, rnd(1.0 / (1.0 + np.exp(-x)), T), T)
    else:
        S = rnd(silu64(gate, T), T)
    return mul(S, up, T)


def check_silu_gate(got, gate, T, sign=False):
    """got = the kernel's T(silu(gate)) (up = 1.0; sign: up = -1.0, an exact sign flip).  Decided patterns equal, the others one of the two neighbours.
    Returns the number of undecided patterns."""
    lo, hi = silu_bounds(gate, T)
    if sign:
        lo, hi = neg(lo), neg(hi)
    ok = same(got, lo, T) | same(got, hi, T)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, f"silu {T}: {bad.size} gate patterns outside the band, first gate 0x{int(np.ravel(gate)[bad[0]]):04x}: got 0x{int(np.ravel(got)[bad[0]]):04x}, " \
                          f"want 0x{int(np.ravel(lo)[bad[0]]):04x}..0x{int(np.ravel(hi)[bad[0]]):04x}"
    return int(np.count_nonzero(lo != hi))


def silu_fixed_gates(T):
    """the gates of the product sweep: zeros, the smallest subnormals, ones, the fp32-range edge, large arguments, the ends of T"""
    vals = bits_of([0.0, -0.0, 1.0, -1.0, -5.0, -17.0, -20.0, -89.0, 11.0, 88.0, np.inf], T)
    return np.concatenate([vals, np.array([0x0001, 0x8001, max_finite(T), max_finite(T) | 0x8000, _FMT[T][2] | 0x8000], dtype=np.uint16)])   # 16


def expect_equal(got, want, T, what, exact=False):
    """whole-buffer comparison; exact: NaN payloads too (copies)"""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got == want) if exact else same(got, want, T)
    bad = np.flatnonzero(~ok.ravel())
    assert bad.size == 0, f"{what} ({T}): {bad.size} of {got.size} elements differ, first at flat index {int(bad[0])}: got 0x{int(got.ravel()[bad[0]]):04x}, " \
                          f"want 0x{int(want.ravel()[bad[0]]):04x}"


# ---- rope_cache ------------------------------------------------------------------------------------------------------------------------------------------------
def rope_ref(q, k, v, cos, sin, pos, k_cache, v_cache, n_heads, n_kv, hd, T, rule=None):
    """rope_cache_batched on bit patterns: q [B, n_heads hd], k / v [B, n_kv hd], cos / sin [B, hd], pos B ints, caches [B, n_kv, L, hd] as they stand before
    the call.  Returns (q_out, k_cache, v_cache) after it: a position outside [0, L) writes nothing."""
    B, half, L = q.shape[0], hd // 2, k_cache.shape[2]

    def rot(x, heads):
        x = x.reshape(B, heads, hd)
        c, s = cos.reshape(B, 1, hd), sin.reshape(B, 1, hd)
        o1, o2 = rope_pair(x[..., :half], x[..., half:], c[..., :half], c[..., half:], s[..., :half], s[..., half:], T, rule)
        return np.concatenate([o1, o2], axis=-1)

    q_out = rot(q, n_heads).reshape(B, n_heads * hd)
    k_rot = rot(k, n_kv)
    kc, vc = k_cache.copy(), v_cache.copy()
    for b in range(B):
        if 0 <= int(pos[b]) < L:
            kc[b, :, int(pos[b]), :] = k_rot[b]
            vc[b, :, int(pos[b]), :] = v[b].reshape(n_kv, hd)
    return q_out, kc, vc


def rope_cos_values(T):
    """the factors of the product sweep: 1, two rotary values, the smallest subnormal, the largest finite value, -0, inf, NaN"""
    return np.concatenate([bits_of([1.0, 0.5403, -0.9900], T), np.array([0x0001, max_finite(T), 0x8000, _FMT[T][2], _FMT[T][3]], dtype=np.uint16)])


def add_partners(T):
    """the second operands of the sum sweeps: zeros, the smallest subnormal and normal numbers (subnormal sums), +-1 and a neighbour (cancellation: every first
    operand meets itself), the largest finite values (overflow to inf), inf (inf - inf)"""
    p = _FMT[T][0]
    return np.concatenate([bits_of([0.0, -0.0, 1.0, -1.0], T),
                           np.array([0x0001, 1 << (p - 1), int(bits_of([1.0], T)[0]) + 1, max_finite(T), max_finite(T) | 0x8000, _FMT[T][2]], dtype=np.uint16)])


def rotary_rows(positions, hd, T, base=10000.0):
    """cos / sin [len(positions), hd] of a real rotary embedding, from float64 numpy, rounded to T (both halves the same, as HF builds them)"""
    inv = base ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    ang = np.asarray(positions, dtype=np.float64)[:, None] * inv[None, :]
    ang = np.concatenate([ang, ang], axis=1)
    return rnd(np.cos(ang), T), rnd(np.sin(ang), T)


def sweep_operands(T, kind):
    """(a, b): the operand pairs of the exhaustive sweeps, as the GPU test forms them — every pattern of a against each partner — and 65,536 random pairs"""
    partners = rope_cos_values(T) if kind == "mul" else add_partners(T)
    a = np.tile(all_patterns(), partners.size)
    b = np.repeat(partners, 65536)
    rng = np.random.default_rng(7 if kind == "mul" else 11)
    return np.concatenate([a, random_finite(65536, T, rng)]), np.concatenate([b, random_finite(65536, T, rng)])


# ---- add_rmsnorm ---------------------------------------------------------------------------------------------------------------------------------------------
def rmsnorm_ref(h, delta, w, eps, T, exact_sum=False, rule=None):
    """h [rows, H], delta [rows, H] or None, w [H] as bits.  Returns (h after the residual add, lo, hi, arg32): the output evaluated at r (1 - delta(H)) and
    r (1 + delta(H)) (header), and the fp32 argument var + eps of rsqrtf, row by row."""
    rows, H = h.shape
    hn = add(h, delta, T) if delta is not None else np.asarray(h, dtype=np.uint16).copy()
    x = widen(hn, T)
    eps32 = np.float32(0.0 if rule == "no_eps" else eps)
    div = H - 1 if rule == "div_h_minus_1" else H
    with np.errstate(all="ignore"):
        S = (x * x).sum(axis=1)                                   # float64
        if exact_sum:                                             # S exact in fp32 in any order: the kernel's own / H and + eps, in numpy float32
            arg = (S.astype(np.float32) / np.float32(div) + eps32).astype(np.float64)
        else:
            arg = S / div + np.float64(eps32)
        r = 1.0 / np.sqrt(arg)
        d = rms_delta(H, exact_sum)
        lo = mul(w[None, :], rnd(x * (r * (1.0 - d))[:, None], T), T)
        hi = mul(w[None, :], rnd(x * (r * (1.0 + d))[:, None], T), T)
        arg32 = arg.astype(np.float32)
    return hn, lo, hi, arg32


def check_rmsnorm(got, lo, hi, T, what="add_rmsnorm"):
    """got between lo and hi in T's ordering (NaN where an end is NaN).  Returns the share of decided elements."""
    got = np.asarray(got, dtype=np.uint16)
    nan_end = is_nan(lo, T) | is_nan(hi, T)
    kl, kh, kg = order_key(lo), order_key(hi), order_key(got)
    inside = ~is_nan(got, T) & (kg >= np.minimum(kl, kh)) & (kg <= np.maximum(kl, kh))
    both_nan = is_nan(lo, T) & is_nan(hi, T)
    ok = np.where(both_nan, is_nan(got, T), nan_end | inside)     # one end NaN (an overflow to inf met a zero weight at that end only): anything goes
    bad = np.flatnonzero(~ok.ravel())
    assert bad.size == 0, f"{what} ({T}): {bad.size} of {got.size} elements outside the interval, first at flat index {int(bad[0])}: got 0x{int(got.ravel()[bad[0]]):04x}, " \
                          f"between 0x{int(lo.ravel()[bad[0]]):04x} and 0x{int(hi.ravel()[bad[0]]):04x}"
    return float(np.mean(same(lo, hi, T)))


RMS_EDGE_H = (8, 64, 4088, 4096, 4104, 8192, 8200, 16392)   # either side of the kernel's register-resident / two-chunk / re-read dispatch (H <= 4096, <= 8192, beyond)
RMS_EPS = (1e-5, 1e-6)
# random rows: the H for which tests/test_glue_cpu.py counts >= 90 % decided elements (delta(H) grows with H; fp16's rounding midpoints lie 8 times as dense)
RMS_RANDOM_H = {F16: (8, 136, 520), BF16: (8, 520, 4104)}
RMS_RANDOM_ROWS = 3


def _weights(H, T, rng):
    return rnd(1.0 + 0.1 * rng.standard_normal(H), T)


def rms_edge_case(H, rows, eps, T):
    """values from {+-1/4 .. +-4}, row i scaled by 2^-i within that set (a cross-row mix-up shows): every partial sum of the squares is a multiple of 2^-4 below
    2^24 2^-4, exact in fp32 in any order.  With the larger eps the row arrives as h + delta, two halves that add exactly."""
    rng = np.random.default_rng(1000 * H + 10 * rows + (1 if eps == RMS_EPS[0] else 2) + (0 if T == F16 else 5))
    mags = np.array([[4.0, 2.0, 1.0], [2.0, 1.0, 0.5], [1.0, 0.5, 0.25]])[:rows]
    v = np.stack([rng.choice(mags[i], H) * rng.choice([-1.0, 1.0], H) for i in range(rows)])
    w = _weights(H, T, rng)
    if eps == RMS_EPS[0]:
        return bits_of(v / 2, T), bits_of(v / 2, T), w
    return bits_of(v, T), None, w


def rms_random_case(H, T, seed=0):
    """|x| log-uniform in [2^-12, 2^12], random signs, as h + delta with delta a tenth of h's size"""
    rng = np.random.default_rng(77 * H + seed + (0 if T == F16 else 3))
    x = np.exp2(rng.uniform(-12.0, 12.0, (RMS_RANDOM_ROWS, H))) * rng.choice([-1.0, 1.0], (RMS_RANDOM_ROWS, H))
    d = 0.1 * np.exp2(rng.uniform(-12.0, 12.0, (RMS_RANDOM_ROWS, H))) * rng.choice([-1.0, 1.0], (RMS_RANDOM_ROWS, H))
    return bits_of(x, T), bits_of(d, T), _weights(H, T, rng)


def rms_arguments():
    """every fp32 argument var + eps the cases above give rsqrtf (tools/glue_ulp.hip measures it on them)"""
    out = []
    for T in TYPES:
        for H in RMS_EDGE_H:
            for rows in (1, 3):
                for eps in RMS_EPS:
                    h, d, w = rms_edge_case(H, rows, eps, T)
                    out.append(rmsnorm_ref(h, d, w, eps, T, exact_sum=True)[3])
        for H in RMS_RANDOM_H[T]:
            h, d, w = rms_random_case(H, T)
            out.append(rmsnorm_ref(h, d, w, RMS_EPS[0], T)[3])
        for eps in RMS_EPS:
            h, w = rms_special_rows(T)
            out.append(rmsnorm_ref(h, None, w, eps, T)[3])
    out = np.concatenate(out).astype(np.float32)
    return out[np.isfinite(out)]                                  # (the special rows with an inf / a NaN have no finite argument)


# ---- token_prologue ------------------------------------------------------------------------------------------------------------------------------------------
def prologue_ref(tok, pos, embed, cos_tab, sin_tab, L, T, rule=None):
    """block.hip's rule: h = embed[clamp(tok)], cos / sin = row clamp(pos) of the tables (clamp: below 0 -> 0, beyond the end -> the last row), and
    mask[i] = 0 if i <= pos else -inf with the RAW position.  tok / pos: B Python ints.  Returns (h, cos, sin, mask), cos / sin None without tables."""
    vocab = embed.shape[0]
    t = [min(max(int(x), 0), vocab - 1) for x in tok]
    pr = [min(max(int(x), 0), L - 1) for x in pos]
    h = embed[t]
    cos = cos_tab[pr] if cos_tab is not None else None
    sin = sin_tab[pr] if sin_tab is not None else None
    ninf = np.uint16(_FMT[T][2] | 0x8000)
    i = np.arange(L)
    mask = np.stack([np.where((i < int(p)) if rule == "mask_lt" else (i <= int(p)), np.uint16(0), ninf) for p in pos]).astype(np.uint16)
    return h, cos, sin, mask


# ---- argmax_advance ------------------------------------------------------------------------------------------------------------------------------------------
def argmax_ref(values, rule=None):
    """torch.argmax's rule written out, on a list of Python floats: the first NaN if there is one; otherwise the first index of the greatest value
    (-0 == +0; all -inf: index 0)"""
    best_i, best = 0, values[0]
    if best != best:
        return 0
    for i in range(1, len(values)):
        v = values[i]
        if v != v:
            return i
        if v > best or (rule == "last_tie" and v == best):
            best_i, best = i, v
    return best_i


def argmax_cases(n, T):
    """[(name, logits bits [n], expected index)] — the expected index by construction; argmax_ref must agree (tests/test_glue_cpu.py).
    Indices sit on the kernel's 1024-thread stride and on the levels of its LDS tree."""
    rng = np.random.default_rng(n)
    low = bits_of(-1.0 - rng.random(n), T)                        # every other logit: in (-2, -1]
    one, two, pinf, ninf, nan = (int(x) for x in bits_of([1.0, 2.0, np.inf, -np.inf, np.nan], T))
    out = []
    for i in sorted({j for j in (0, 1, 511, 512, 1023, 1024, n - 1024, n - 1) if 0 <= j < n}):
        x = low.copy(); x[i] = one
        out.append((f"max@{i}", x, i))
    pairs = sorted({(a, b) for a, b in ((0, 1024), (1, 1025), (511, 1535), (511, 512), (0, 512), (1023, 1024), (0, n - 1), (n - 1025, n - 1)) if 0 <= a < b < n})
    for a, b in pairs:
        x = low.copy(); x[a] = one; x[b] = one
        out.append((f"tie@{a},{b}", x, a))
        if a > 0:                                                 # NaN pair, a +inf at a lower index: the first NaN wins over it
            x = low.copy(); x[a] = nan; x[b] = nan | 0x8000; x[a - 1] = pinf
            out.append((f"nan@{a},{b}", x, a))
        elif n > 2:
            x = low.copy(); x[a] = nan; x[b] = nan                # NaN at 0 and b, +inf between
            x[1] = pinf
            out.append((f"nan@{a},{b}", x, a))
    z = np.where(rng.integers(0, 2, n) == 1, 0x8000, 0).astype(np.uint16); z[0] = 0x8000
    out.append(("zeros", z, 0))
    out.append(("all-ninf", np.full(n, ninf, dtype=np.uint16), 0))
    if n >= 2:
        x = low.copy(); x[(n - 1) // 2] = pinf; x[n - 1] = pinf
        out.append(("two-pinf", x, (n - 1) // 2))
        x = low.copy(); x[n - 1] = two; x[0] = one
        out.append(("greater-later", x, n - 1))
    return out


ARGMAX_N = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 32000, 151936)


# ---- the cases both halves of the tests build (inputs only; the expectation comes from the *_ref functions) ------------------------------------------------
ROPE_ARITH = dict(n_heads=256, n_kv=256, hd=128, L=4)   # 16,384 rotary pairs per row on the q path and as many on the k path


def rope_arith_case(kind, T):
    """kind "mul": every pattern of x1 (x2 = 0, sin[i] = 0: o1 = x1 * cos[i] and nothing else) against each of rope_cos_values, on the q path and on the k path;
    "add": every pattern of x1 against each of add_partners as x2 with cos = sin = 1 (o1 = x1 - x2, o2 = x2 + x1);  "random": 65,536 random finite pairs per
    path, cos / sin with DIFFERENT halves (values in [-1, 1] in two rows, random finite patterns in two), two positions outside the cache;  "rotary": real
    rotary rows of positions 0, 1, 1000.  v: every pattern (NaN payloads included) in every pair of rows.  Returns the arguments of rope_ref."""
    g = ROPE_ARITH
    n_heads, n_kv, hd, L = g["n_heads"], g["n_kv"], g["hd"], g["L"]
    half, per = hd // 2, g["n_heads"] * hd // 2
    chunks = all_patterns().reshape(4, n_heads, half)
    rng = np.random.default_rng({"mul": 1, "add": 2, "random": 3, "rotary": 4}[kind] + (0 if T == F16 else 10))
    one = bits_of([1.0], T)[0]
    if kind in ("mul", "add"):
        partners = rope_cos_values(T) if kind == "mul" else add_partners(T)
        P = partners.size
        B = 4 * P
        q, k = np.zeros((B, n_heads, hd), dtype=np.uint16), np.zeros((B, n_kv, hd), dtype=np.uint16)
        cos, sin = np.zeros((B, hd), dtype=np.uint16), np.zeros((B, hd), dtype=np.uint16)
        for b in range(B):
            c, j = b % 4, b // 4
            q[b, :, :half], k[b, :, :half] = chunks[c], chunks[(c + 2) % 4]
            if kind == "mul":
                cos[b, :half], cos[b, half:], sin[b, half:] = partners[j], partners[(j + 5) % P], partners[(j + 3) % P]
            else:
                q[b, :, half:], k[b, :, half:] = partners[j], partners[j]
                cos[b], sin[b] = one, one
        pos = [b % L for b in range(B)]
    elif kind == "random":
        B = 4
        q, k = random_finite(B * n_heads * hd, T, rng).reshape(B, n_heads, hd), random_finite(B * n_kv * hd, T, rng).reshape(B, n_kv, hd)
        cos = np.concatenate([bits_of(rng.uniform(-1, 1, (2, hd)), T), random_finite(2 * hd, T, rng).reshape(2, hd)])
        sin = np.concatenate([bits_of(rng.uniform(-1, 1, (2, hd)), T), random_finite(2 * hd, T, rng).reshape(2, hd)])
        pos = [0, L - 1, L, -1]
    else:
        B = 3
        q, k = bits_of(rng.standard_normal((B, n_heads, hd)), T), bits_of(rng.standard_normal((B, n_kv, hd)), T)
        cos, sin = rotary_rows([0, 1, 1000], hd, T)
        pos = [0, 1, 2]
    assert per * 4 == 65536
    v = np.resize(all_patterns(), B * n_kv * hd).reshape(B, n_kv * hd)
    return dict(q=q.reshape(B, -1), k=k.reshape(B, -1), v=v, cos=cos, sin=sin, pos=pos, n_heads=n_heads, n_kv=n_kv, hd=hd, L=L)


ROPE_GEOMETRIES = ((1, 1, 2), (3, 1, 6), (5, 5, 64), (7, 1, 96), (9, 3, 256))   # (n_heads, n_kv, hd): the smallest; an odd half; ...; more than one workgroup, ragged last
ROPE_POSITIONS = ((1, 0), (16, 0), (16, 15), (16, 16), (16, -1), (16, 2 ** 40))  # (L, pos)


def rope_geometry_case(n_heads, n_kv, hd, L, positions, T):
    """random finite q / k / v and cos / sin in [-1, 1] with different halves, one row per position"""
    B = len(positions)
    rng = np.random.default_rng(n_heads * 1000 + hd + L + B + (0 if T == F16 else 7))
    q, k, v = (random_finite(B * h * hd, T, rng).reshape(B, h * hd) for h in (n_heads, n_kv, n_kv))
    cos, sin = bits_of(rng.uniform(-1, 1, (B, hd)), T), bits_of(rng.uniform(-1, 1, (B, hd)), T)
    return dict(q=q, k=k, v=v, cos=cos, sin=sin, pos=list(positions), n_heads=n_heads, n_kv=n_kv, hd=hd, L=L)


def rope_caches(c, salt=0):
    """the sentinel-filled caches a rope case starts from"""
    B = c["q"].shape[0]
    shape = (B, c["n_kv"], c["L"], c["hd"])
    return sentinel(shape, 1 + salt), sentinel(shape, 77 + salt)


def rope_expect(c, k_cache, v_cache, T, rule=None):
    return rope_ref(c["q"], c["k"], c["v"], c["cos"], c["sin"], c["pos"], k_cache, v_cache, c["n_heads"], c["n_kv"], c["hd"], T, rule)


def rms_special_rows(T, H=64):
    """(h [4, H], w): an all-zero row of mixed signs (eps alone under the root: +-0 out, by IEEE's sign rules), a row with one +inf (r = 0: NaN there, +-0
    elsewhere), a row with one NaN (NaN everywhere), and a row of |x| in [2^-10, 2^-8] whose mean square is of eps's size (1e-5)"""
    rng = np.random.default_rng(5 if T == F16 else 6)
    x = rng.standard_normal((4, H))
    h = bits_of(x, T)
    h[0] = np.where(rng.integers(0, 2, H) == 1, 0x8000, 0)
    h[1, H // 3] = _FMT[T][2]
    h[2, H - 1] = _FMT[T][3]
    h[3] = bits_of(np.exp2(rng.uniform(-10, -8, H)) * rng.choice([-1.0, 1.0], H), T)
    return h, _weights(H, T, rng)


PROLOGUE_TABLES = ((8192, 8), (64, 2056), (16, 4104))   # all 65,536 patterns as [8192, 8]; 257 16-byte chunks per row: one workgroup, a stride remainder of 1;
#                                                          513 chunks: the grid of block.hip's token_prologue_run is 2 workgroups (513 / 256), remainder 1
PROLOGUE_L = (1, 96, 300)
PROLOGUE_HD = (2, 48, 300)


def prologue_tokens(vocab):
    return [0, vocab - 1, -1, vocab, 2 ** 40]


def prologue_positions(L):
    return [0, L - 1, L, -3]


def prologue_tables(vocab, H, L, hd, T):
    """(embed [vocab, H], cos_tab, sin_tab [L, hd]) of arbitrary patterns, NaN payloads included: the kernel copies"""
    embed = all_patterns().reshape(vocab, H) if vocab * H == 65536 else (np.arange(vocab * H, dtype=np.uint64) * np.uint64(40503) % np.uint64(65536)).astype(np.uint16).reshape(vocab, H)
    rng = np.random.default_rng(vocab + L * 7 + hd)
    return embed, rng.integers(0, 65536, (L, hd)).astype(np.uint16), rng.integers(0, 65536, (L, hd)).astype(np.uint16)


if __name__ == "__main__":   # python tests/_glue_cases.py FILE: the RMSNorm cases' rsqrtf arguments as raw float32, for tools/glue_ulp.hip
    import sys
    rms_arguments().tofile(sys.argv[1])
