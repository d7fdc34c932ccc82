"""Cases, host model and error bounds of the router kernel's tests (csrc/moe_router.hip; tests/test_moe_router_cpu.py, tests/test_moe_router_gpu.py).

What the kernel states (include/hqq_hip.h, hqq_hip_moe_router), T the compute dtype, rnd = round to T:
    l = fp32(rnd(x . W_e));  p = exp(l - max l) / sum_e exp(l - max l) in fp32, the sum in ascending e;  sel = the k largest l, descending, equal logits by
    ascending e;  w = p[sel], / sum_s p[sel_s] with renorm, rounded to T with round_weights.

Two host models.
  reference (float64): l64 = x . W_e in float64, unrounded; ref_select(l64, k); ref_weights(logits, idx, ...) = the softmax, gather and renormalisation in
      float64 on GIVEN logits of T.  The weights are a function of the rounded logits, so the reference takes the logits the code under test returned (which
      are checked against l64 on their own) and checks the arithmetic that follows them.
  restatement (float32, model32): rounding for rounding what the kernel does.  Products of two T values are exact in fp32, so fma(x, w, acc) rounds once, as
      acc + (x * w) does here: lane i of 64 adds the elements of the 8-element chunks i, i + 64, ... in ascending index into one accumulator, and the 64
      partial sums are added as a balanced binary tree in lane order.  Its logits are the kernel's bit for bit; its weights differ from the kernel's by what
      two implementations of exp differ by.  It carries the NaN rule (a NaN logit compares as the largest, NaNs by ascending id) and -0 == +0.

Bounds (derived here, not fitted to a kernel's output).  u = 2^-24.
  logits: |l_kernel - l64| <= gamma_H * sum_i |x_i W_ei| + half an ulp of T at |l64| + that,  gamma_H = H u / (1 - H u): an fp32 sum of H exact products
      in any order (Higham, Accuracy and Stability, section 3.1), then one rounding to T.
  selection: a row's ordered selection is decided when every gap between neighbours among its k + 1 largest l64 exceeds twice the largest logit bound among
      them (`margin_ok`); the k-th / (k+1)-th gap is one of these gaps, the others fix the ORDER inside the selection.  Every random case is built so that all of
      its rows satisfy this: a row that does not is drawn again from the case's generator, so no row is ever left out of a check.
  weights: with d = l - max (one fp32 subtraction, relative error u, hence a relative error |d| u in exp), exp within EXP_ULPS ulps (2 u EXP_ULPS relative),
      E - 1 additions of non-negative terms ((E - 1) u), one division (u):   rel_p = 2 (2 u EXP_ULPS + dmax u) + (E - 1) u + u,  dmax = max l - min l of the row.
      With renorm: numerator rel_p, denominator rel_p + (k - 1) u, one division: rel_w = 2 rel_p + k u.  First-order terms; the products of two of them are
      below 2^-40 and covered by the factor 1.01.  With round_weights: + half an ulp of T at the bounded value.  + 2^-126 for a probability that underflows.
  EXP_ULPS: the documentation a ROCm 7 installation carries (share/doc under the ROCm prefix) states no ulp bound for expf, so the error of the
      device function was MEASURED: expf, compiled with the flags of csrc/moe_router.hip, on an MI355X, against float64 exp, over every argument the kernel
      can form from these cases' logits — d = a - b for a, b on the grid of T is a multiple of 2^-24 in [-2^7, 0] here — sampled as 2^22 uniformly spaced
      values in [-32, 0], 2^22 in [-1, 0] and 2^20 log-uniform ones in [-88, -2^-20] (tools/expf_ulp.hip).  Largest error seen: EXP_SEEN_ULPS; twice that is allowed.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

U32 = 2.0 ** -24
EXP_SEEN_ULPS = 0.85    # measured as described above: 0.8436 ulps, at d = -0.108516693
EXP_ULPS = 2.0 * EXP_SEEN_ULPS
MANT = {torch.float16: 11, torch.bfloat16: 8}          # significand bits of T
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126}   # exponent of T's smallest normal number


@dataclass(frozen=True)
class Case:
    kind: str            # "random" | "integer" | "tie_all" | "top_equal"
    E: int
    k: int
    H: int
    T: int
    dt: torch.dtype
    renorm: bool = True
    round_w: bool = False
    seed: int = 0

    @property
    def id(self):
        return (f"{self.kind}-E{self.E}-k{self.k}-H{self.H}-T{self.T}-{'bf16' if self.dt == torch.bfloat16 else 'fp16'}"
                f"{'-renorm' if self.renorm else ''}{'-round' if self.round_w else ''}")


ES, KS, HS, TS = (1, 4, 8, 60, 128, 256), (1, 2, 8), (8, 64, 136, 2048), (1, 3, 16)
DTYPES = (torch.float16, torch.bfloat16)
PAIRS = [(E, k) for E in ES for k in KS if k <= E]   # 15


def _grid(kind):
    """every (E, k) pair in both dtypes; H, T_, renorm and round_weights cycle with different periods so that every value meets every dtype and both flags"""
    out = []
    for i, (E, k) in enumerate(PAIRS):
        for j, dt in enumerate(DTYPES):
            n = 2 * i + j
            out.append(Case(kind, E, k, HS[(i + j) % 4], TS[(i + 2 * j) % 3], dt, renorm=(n % 3 != 2), round_w=(n % 4 in (1, 2)), seed=101 + 7 * n))
    return out


RANDOM = _grid("random")
INTEGER = _grid("integer")[::3]
# closed forms with exactly representable weights: all E logits equal (k = 1, 2 for any E: p / (p + p) = 1/2; any power-of-two k where E is a power of two: p = 1 / E
# is a power of two and every sum is exact), and k equal logits at 0 over E - k at -200 (exp(-200) = 0 in fp32: den = k, p = 1 / k exactly, with and without renorm)
TIE_ALL = [Case("tie_all", E, k, H, T, dt) for (E, k, H, T, dt) in (
    (1, 1, 8, 1, torch.float16), (4, 2, 64, 3, torch.bfloat16), (8, 8, 136, 16, torch.float16), (60, 2, 2048, 3, torch.float16), (60, 1, 64, 1, torch.bfloat16),
    (128, 8, 64, 16, torch.bfloat16), (256, 2, 136, 3, torch.float16), (256, 8, 8, 1, torch.bfloat16))]
TOP_EQUAL = [Case("top_equal", E, k, H, T, dt, renorm=rn, round_w=rw) for (E, k, H, T, dt, rn, rw) in (
    (4, 1, 8, 3, torch.float16, True, False), (8, 2, 64, 16, torch.bfloat16, False, True), (60, 8, 136, 3, torch.float16, True, True),
    (128, 2, 2048, 1, torch.bfloat16, True, False), (256, 8, 64, 16, torch.float16, False, False), (60, 2, 8, 1, torch.bfloat16, True, False))]
CLOSED = INTEGER + TIE_ALL + TOP_EQUAL
BY_ID = {c.id: c for c in RANDOM + CLOSED}
assert len(BY_ID) == len(RANDOM) + len(CLOSED)


# ---- number formats -----------------------------------------------------------------------------------------------------------------------------------------------
def half_ulp(v: torch.Tensor, dt) -> torch.Tensor:
    """half the spacing of T at magnitude v (float64), at least half the subnormal spacing"""
    e = torch.floor(torch.log2(v.double().abs().clamp_min(2.0 ** MIN_EXP[dt]))).clamp_min(MIN_EXP[dt])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dt])


def rnd(v: torch.Tensor, dt) -> torch.Tensor:
    """fp32 -> T -> fp32 (round to nearest even, the conversion torch makes)"""
    return v.float().to(dt).float()


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------------------------------------
def logits64(x, W):
    return x.double() @ W.double().t()


def logit_bound(x, W, dt):
    """[T, E]: how far the kernel's logit may lie from logits64"""
    H = x.shape[1]
    gamma = H * U32 / (1.0 - H * U32)
    acc = gamma * (x.double().abs() @ W.double().abs().t())
    return acc + half_ulp(logits64(x, W).abs() + acc, dt)


def ref_select(l, k):
    """[T, k] int64: the k largest of each row in descending order, equal values by ascending id (a stable sort keeps the ascending ids of equal values)"""
    return torch.sort(l.double(), dim=-1, descending=True, stable=True).indices[:, :k].contiguous()


def margin_ok(l64, bound, k):
    """[T] bool: every gap between neighbours among the row's min(k + 1, E) largest logits exceeds twice the largest bound among them"""
    n = min(k + 1, l64.shape[1])
    top = torch.sort(l64, dim=-1, descending=True, stable=True)
    v, b = top.values[:, :n], torch.gather(bound, 1, top.indices[:, :n])
    if n == 1:
        return torch.ones(l64.shape[0], dtype=torch.bool)
    return ((v[:, :-1] - v[:, 1:]).min(dim=-1).values > 2.0 * b.max(dim=-1).values)


def smallest_gap_in_ulps(logits, k, dt):
    """the smallest k-th / (k+1)-th gap over the rows of `logits` (of T), in ulps of T at the k-th logit's magnitude (inf where k == E)"""
    l = logits.double()
    if k >= l.shape[1]:
        return float("inf")
    v = torch.sort(l, dim=-1, descending=True).values
    return float(((v[:, k - 1] - v[:, k]) / (2.0 * half_ulp(torch.maximum(v[:, k - 1].abs(), v[:, k].abs()), dt))).min())


def ref_weights(logits, idx, renorm):
    """float64 [T, k]: softmax of the given logits (of T), gathered at idx, renormalised; NOT rounded (weight_bound accounts for round_weights)"""
    p = torch.softmax(logits.double(), dim=-1)
    w = torch.gather(p, 1, idx)
    return w / w.sum(-1, keepdim=True) if renorm else w


def weight_bound(logits, w64, E, k, renorm, round_dt=None):
    """[T, k]: how far fp32 weights computed from `logits` may lie from ref_weights(logits, ...)"""
    l = logits.double()
    dmax = (l.max(-1).values - l.min(-1).values).unsqueeze(-1)
    rel_p = 2.0 * (2.0 * U32 * EXP_ULPS + dmax * U32) + (E - 1) * U32 + U32
    rel = (2.0 * rel_p + k * U32) if renorm else rel_p
    b = 1.01 * rel * w64 + 2.0 ** -126
    if round_dt is not None:
        b = b + half_ulp(w64 + b, round_dt)
    return b


# ---- the float32 restatement --------------------------------------------------------------------------------------------------------------------------------------
def logits32(x, W):
    """[T, E] float32: the kernel's sums before the rounding to T, in the kernel's order"""
    T, H = x.shape
    E = W.shape[0]
    prod = x.float()[:, None, :] * W.float()[None, :, :]          # exact
    iters = -(-(H // 8) // 64)
    prod = torch.nn.functional.pad(prod, (0, iters * 512 - H)).view(T, E, iters, 64, 8)
    acc = torch.zeros((T, E, 64), dtype=torch.float32)
    for it in range(iters):
        for j in range(8):
            acc = acc + prod[:, :, it, :, j]
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def select32(l, k):
    """the stated order on fp32 logits: NaN first (by ascending id), then descending value with -0 == +0, equal values by ascending id"""
    rows = []
    for row in l.tolist():
        rows.append(sorted(range(len(row)), key=lambda e: (0, 0.0, e) if math.isnan(row[e]) else (1, -row[e] + 0.0, e))[:k])
    return torch.tensor(rows, dtype=torch.int64)


def softmax32(l, idx, renorm, round_dt):
    l = l.float()
    m = torch.where(torch.isnan(l), torch.full_like(l, float("-inf")), l).max(-1, keepdim=True).values
    ex = torch.exp(l - m)
    den = torch.zeros(l.shape[0], dtype=torch.float32)
    for e in range(l.shape[1]):
        den = den + ex[:, e]
    p = torch.gather(ex, 1, idx) / den[:, None]
    if renorm:
        s = torch.zeros(l.shape[0], dtype=torch.float32)
        for j in range(idx.shape[1]):
            s = s + p[:, j]
        p = p / s[:, None]
    return rnd(p, round_dt) if round_dt is not None else p


def model32(x, W, k, renorm=True, round_w=False):
    """-> (idx [T, k] int64, weights [T, k] float32, logits [T, E] of T)"""
    dt = x.dtype
    l = logits32(x, W).to(dt)
    idx = select32(l.float(), k)
    return idx, softmax32(l, idx, renorm, dt if round_w else None), l


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------------
def _draw_row(g, H, dt):
    return (torch.randn((1, H), generator=g) * 0.5).to(dt)


@functools.lru_cache(maxsize=None)
def build(case: Case):
    """-> dict: x [T, H], W [E, H] of T; for the closed forms also "idx" (exact), "logits" (exact, of T) and "w" (exact float32) or None where the weights are
    only bounded.  Built once per case and shared: callers do not modify it."""
    g = torch.Generator().manual_seed(case.seed)
    E, k, H, T, dt = case.E, case.k, case.H, case.T, case.dt
    out = {"case": case, "redrawn": 0}
    if case.kind == "random":
        W = (torch.randn((E, H), generator=g) * (2.0 / math.sqrt(H))).to(dt)
        rows = []
        for _ in range(T):
            for attempt in range(2000):
                r = _draw_row(g, H, dt)
                if bool(margin_ok(logits64(r, W), logit_bound(r, W, dt), k)[0]):
                    break
                out["redrawn"] += 1
            else:
                raise RuntimeError(f"{case.id}: no row with a decided selection in 2000 draws")
            rows.append(r)
        out["x"], out["W"] = torch.cat(rows), W
        return out
    if case.kind == "integer":      # every product a multiple of 1/4, every sum below 2^13: exact in fp32 in any order
        x = torch.randint(-2, 3, (T, H), generator=g).to(dt)
        W = (torch.randint(-4, 5, (E, H), generator=g).float() / 4.0).to(dt)
    elif case.kind == "tie_all":    # every expert has the same row: E equal logits per token
        x = torch.randint(-2, 3, (T, H), generator=g).to(dt)
        W = (torch.randint(-4, 5, (1, H), generator=g).float() / 4.0).to(dt).expand(E, H).contiguous()
    else:                           # top_equal: l = 0 for k chosen experts, -200 for the rest (x = e_c for a column c that moves with the row)
        x = torch.zeros((T, H), dtype=dt)
        W = torch.randint(-4, 5, (E, H), generator=g).float() / 4.0
        chosen = torch.randperm(E, generator=g)[:k]
        cols = [(5 * t + 3) % H for t in range(T)]
        for t, c in enumerate(cols):
            x[t, c] = 1.0
        W[:, cols] = -200.0
        W[chosen[:, None], torch.tensor(cols)[None, :]] = 0.0
        W = W.to(dt)
    l = rnd(logits64(x, W).float(), dt)     # exact sums (representable in fp32), rounded once
    out["x"], out["W"], out["logits"] = x, W, l.to(dt)
    out["idx"] = ref_select(l, k)
    exact = case.kind == "top_equal" or (case.kind == "tie_all" and (k <= 2 or (E & (E - 1)) == 0))
    out["w"] = None
    if exact:
        w = torch.full((T, k), 1.0 / k, dtype=torch.float32)
        out["w"] = rnd(w, dt) if case.round_w else w
    return out
