"""Shared by tests/test_tile_cpu.py and tests/test_tile_gpu.py: the cases, the fp64 reference, the error band and a host emulation for the verify step's tiled
decode attention (csrc/attn_tile.hip, hqq_hip_attn_decode_tiled; ops.attn_decode_tiled): R <= 16 queries of one sequence, row i over keys [0, pos[i]], each key
read once for all rows.  Every expected value is fp64 attention over the same tensors (reference_rows), never another kernel's output.

The closed forms are _attn_cases' (one key decides the output), per ROW here.  All rows of a head share one query direction, q[i, h] = f_i qg[h] with f_i in
{1, 2} — what _attn_cases.Bed does for the query heads of a GQA group —, so a needle key C qg[h] serves every row exactly.  They stay exact under this kernel
although it rounds its probabilities to T: a needle's p is exp(0) = 1 and rounds to 1, every other p is below e^-100 and rounds to 0 (in fp32 already, or on the
way to T), and V is an integer of at most 7 bits.
  tier     key a <= min(pos) holds 32 qg, key pos[t] holds 64 qg (both exact in fp16 and bf16): rows i >= t give V[pos[t]] bit for bit, rows i < t give V[a]
           bit for bit — the per-row causal edge, for every t in 0 .. R - 1
  needle   one needle, the rows ending at n_max, for every n_max from 1 to 2 KB + 33 (KB = kb(hd): the keys a workgroup covers per pass, waves x 32), at the
           places `places` picks relative to KB and 32: a needle in the last block (earlier blocks rescaled by alpha = 0), in the first (no rescale), in a block
           only some rows see.  A row that does not see the needle is held to the band below
  twin     the same key in two different blocks, waves and shares: (V[a] + V[b]) / 2, within one ulp of T
  flat     K = 0, V zero but for one key j*: row i gives V[j*] / (pos[i] + 1) within _attn_cases' flat bound — the per-row count of the denominator, n_max <= 1025
  splits   S in (2, 3, 7, 16) on a cache of 2048: needles at the first and the last key of every non-empty share of [0, n_max), rows whose position lies in an
           earlier share than the last (their later shares are empty), n_max < S
Random cases (randn q, K, V; NaN from n_max on) catch a mis-weighted rescale: the closed forms only ever rescale by 0 or 1.

THE BAND, derived (u32 = 2^-24, u_T = 2^-SIG_BITS, per element d of row i and head h; w_j = the exact softmax weights, o_d = sum_j w_j v_jd):
  scores   the kernel's s_j is hd exact products (two T values) summed in fp32 in an order the MFMA does not promise (hd - 1 additions), the scaling multiply (1),
           and the subtraction of the maximum (|s - m| <= 2 max |s|: 2):  |s^_j - m^ - (s_j - m)| <= delta = (hd + 2) u32 scaling max_j sum_d |q_d k_jd|.
           The common m^ cancels between numerator and denominator.
  exp      expf under -ffp-contract=off, the function and flags _router_cases.EXP_ULPS was measured with: relative eps_exp = 2 u32 EXP_ULPS.
  weights  w^_j / w_j lies within e^(+-2 delta) (1 +- eps_exp) / (1 -+ eps_exp), so sum_j |w^_j - w_j| |v_jd| <= vmax_d ((e^(2 delta) - 1) + 2 eps_exp) to first
           order; the statement of the kernel's contract allows 2 (e^(2 delta) - 1), which also covers the second-order products.
  P to T   the numerator's probabilities are rounded to T (the denominator sums the fp32 ones): sum_j w_j rho_j v_jd, |rho_j| <= u_T: u_T vmax_d.  A probability
           below T's smallest normal number rounds with an ABSOLUTE error of half the subnormal spacing, 2^(MIN_EXP - SIG_BITS), relative to a row sum >= 1 (the
           key with the largest score contributes exactly 1; p <= 1 always, and a block's p is rescaled by alpha <= 1 afterwards): n_vis 2^(MIN_EXP - SIG_BITS) vmax_d.
  c_acc    fp32 roundings in l and O, each relative to a partial sum bounded by (sum |p v|) <= l vmax_d, counted from the kernel:
             per block a wave takes (nbw = ceil(ceil(chunk / 32) / waves) of them): O: the rescale by alpha (1) + the MFMA's sum of 32 products onto the accumulator
             (32); l: the rescale (1), the lane's 8 probabilities (7), the two shuffle additions (2), the addition onto l (1): 44
             the merge of the waves: per wave one fmaf onto the numerator and one onto the denominator (waves x 2), the weights exp(m_w - m): the subtraction (1) and
             expf (2 EXP_ULPS), numerator against denominator: 2 (2 EXP_ULPS + 1)
             S == 1: the division (1).  S > 1, attn_combine_kernel (csrc/block.hip): per share two fmaf (2 S), its weights __expf(m_s - m): 2 (2 FAST_EXP_ULPS + 1),
             the division (1)
  output   one rounding to T: u_T |ref| (+ half a subnormal spacing of T)
  |got - ref| <= vmax_d (2 (e^(2 delta) - 1) + 2 eps_exp + u_T + n_vis 2^(MIN_EXP - SIG_BITS) + c_acc u32) + u_T |ref| + 2^(MIN_EXP - SIG_BITS)
  vmax_d = the largest visible |V[j, d]| of the row.
  So that the band cannot hide a failure, every random case satisfies (checked on the CPU): the terms other than u_T vmax_d + u_T |ref| sum to less than
  u_T vmax_d — the band is less than twice the rounding of P and of the output.  With randn queries at hd = 256 in fp16 delta alone breaks this
  (4 delta ~ 8e-4 > 2^-11), so the hd = 256 cases draw their queries at a quarter of the scale: the case changes, not the band.
  FAST_EXP_ULPS: __expf's error was measured as _router_cases describes for expf (tools/expf_ulp.hip built with -DEXPF_FN=__expf and the flags of csrc/block.hip,
  on an MI355X, the same 2^22 + 2^22 + 2^20 arguments over [-88, 0]): largest error among results that are normal fp32 numbers FAST_EXP_SEEN_ULPS; twice that is
  allowed.  Below 2^-126 the intrinsic flushes to zero: an absolute 2^-126, which no term above can see.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

from _attn_cases import C_NEEDLE, CODE, DT, SIG_BITS, bits, coded_values, flat_row, reference, ulp  # noqa: F401  (reference: the one-row fp64 attention, which test_tile_cpu holds reference_rows to)
from _router_cases import EXP_ULPS

U32 = 2.0 ** -24
MIN_EXP = {"f16": -14, "bf16": -126}
FAST_EXP_SEEN_ULPS = 61.6    # measured as described above: 61.5331 ulps, at d = -84.5764084 (the error grows with |d|: the argument is scaled by log2 e in fp32 first)
FAST_EXP_ULPS = 2.0 * FAST_EXP_SEEN_ULPS
WAVES, BLOCK, MAX_ROWS = 8, 32, 16
HEADS = 8                    # probes per closed-form launch: n_heads = n_kv = 8, one place per head
HDS = (64, 128, 256)
DTS = ("f16", "bf16")
FLAT_MAX_N = 1025
SPLITS = (2, 3, 7, 16)


def kb(hd: int) -> int:
    """the keys a workgroup covers per pass of its waves (TILE_WAVES x 32 in csrc/attn_tile.hip; the same for every head size)"""
    return WAVES * BLOCK


def sweep_max_n(hd: int) -> int:
    return 2 * kb(hd) + 33


def shares(n: int, S: int):
    """[k0, k1) of every share, as the kernel cuts them: chunk = ceil(n / S); k1 <= k0 is an empty share"""
    chunk = (n + S - 1) // S
    return [(s * chunk, min(s * chunk + chunk, n)) for s in range(S)]


def places(n: int, hd: int):
    """_attn_cases.places relative to this kernel's units: key 0, n - 1, n - 2, the middle, and both sides of the last multiple of 32 and of KB below n"""
    m1 = (n - 1) // BLOCK * BLOCK
    m4 = (n - 1) // kb(hd) * kb(hd)
    return tuple(min(max(p, 0), n - 1) for p in (0, n - 1, n - 2, n // 2, m1 - 1, m1, m4 - 1, m4))


def _fill(seq, k=HEADS):
    seq = list(seq)
    return tuple(seq[i % len(seq)] for i in range(k))


@dataclass(frozen=True)
class Case:
    kind: str            # "tier" | "needle" | "twin" | "flat" | "random"
    dt: str
    hd: int
    L: int
    pos: tuple           # the rows' positions
    S: int = 1
    a: tuple = ()        # per KV head: the 32-needle (tier, needle, twin) or j* (flat)
    b: tuple = ()        # per KV head: the 64-needle (tier) or the second 32-needle (twin)
    heads: tuple = (HEADS, HEADS)
    seed: int = 0
    qscale: float = 1.0

    @property
    def id(self):
        p = self.pos
        ps = f"{p[0]}..{p[-1]}" if list(p) == list(range(p[0], p[0] + len(p))) else ".".join(map(str, p))
        return f"{self.kind}-{self.dt}-hd{self.hd}-h{self.heads[0]}.{self.heads[1]}-R{len(p)}-p{ps}-s{self.S}-a{'.'.join(map(str, self.a))}-b{'.'.join(map(str, self.b))}"

    @property
    def n_max(self):
        return max(self.pos) + 1


def _ending_at(n: int, R: int):
    return tuple(range(max(0, n - R), n))


# ---- the grid -----------------------------------------------------------------------------------------------------------------------------------
TIER_R, TIER_P0 = 16, 57                    # rows 57 .. 72: the tile is full and its positions straddle the block edge at 64
TIER_A = (0, 1, 31, 32, 33, 55, 56, 40)     # all <= min(pos)


def tier_cases(dt: str, hd: int):
    pos = tuple(range(TIER_P0, TIER_P0 + TIER_R))
    out = [Case("tier", dt, hd, 128, pos, S, TIER_A, (pos[t],) * HEADS) for S in (1, 2) for t in range(TIER_R)]
    # three rows at scattered, unsorted positions: the needle of row t at pos[t] is seen by the rows at or beyond it, whatever their index
    pos = (300, 45, 170)
    out += [Case("tier", dt, hd, 320, pos, S, _fill((0, 44, 7, 32)), (pos[t],) * HEADS) for S in (1, 3) for t in range(3)]
    return out


def sweep_cases(dt: str, hd: int, R: int = 5):
    L = sweep_max_n(hd) + 63
    return [Case("needle", dt, hd, L, _ending_at(n, R), 1, places(n, hd), places(n, hd)) for n in range(1, sweep_max_n(hd) + 1)]


def twin_cases(dt: str, hd: int):
    """a, b <= min(pos): block 0 and block 1 (two waves), block 0 and block 8 (one wave, two passes), either side of a share's edge, far apart"""
    n, K = 700, kb(hd)
    pos = _ending_at(n, 4)
    a = (0, 3, 31, 5, 100, K - 1, K, 17)
    b = (32, K + 3, 300, 600, 613, 2 * K - 1, 2 * K, 690)
    assert max(a + b) <= min(pos)
    return [Case("twin", dt, hd, 704, pos, S, a, b) for S in (1, 2, 3)]


def flat_cases(dt: str, hd: int):
    out = []
    for n in (1, 2, 5, 31, 32, 33, 64, 255, 256, 257, 545, 1024, 1025):
        pos = _ending_at(n, 4)
        lo = min(pos)
        j = _fill((0, lo, lo // 2, max(lo - 1, 0), min(31, lo), min(32, lo), min(256, lo), lo // 3))
        for S in ((1,) if n < 64 else (1, 3)):
            out.append(Case("flat", dt, hd, FLAT_MAX_N, pos, S, j, j))
    return out


def split_cases(dt: str, hd: int, S: int):
    out = []
    for n in (2048, 1500):
        live = [(k0, k1) for k0, k1 in shares(n, S) if k0 < k1]
        probes = [p for k0, k1 in live for p in (k0, k1 - 1)]
        # rows in the first share, in a middle one, at the end, unsorted: the later shares of the early rows are empty
        pos = (n - 1, live[0][1] - 1, live[len(live) // 2][0], 5, n - 2, live[-1][0])
        for i in range(0, len(probes), HEADS):
            a = _fill(probes[i:i + HEADS])
            out.append(Case("needle", dt, hd, 2048, pos, S, a, a))
    n = S - 1                                  # n_max < S: chunk = 1, the shares from n_max on are empty
    out.append(Case("needle", dt, hd, 2048, _ending_at(n, 3), S, _fill(range(n)), _fill(range(n))))
    return out


RANDOM_RS = (1, 2, 3, 8, 15, 16)
RANDOM_HEADS = ((4, 4), (8, 2))
RANDOM_L = 2048


def random_cases():
    """every (hd, heads, dtype) at every first position p0 in (0, 31, 32, 1023, L - R); R cycles with a period coprime to the others so that every R meets every
    hd, dtype and p0; above 1024 visible keys the splits cycle through (2, 3, 4, 1).  Once a non-consecutive, unsorted pos."""
    out, n = [], 0
    for hd in HDS:
        for heads in RANDOM_HEADS:
            for dt in DTS:
                for ip, p0 in enumerate((0, 31, 32, 1023, None)):
                    R = RANDOM_RS[(n + ip) % 6]
                    p = RANDOM_L - R if p0 is None else p0
                    S = 1 if p + R <= 1024 else (2, 3, 4, 1)[n % 4]
                    out.append(Case("random", dt, hd, RANDOM_L, tuple(range(p, p + R)), S, heads=heads, seed=n, qscale=0.25 if hd == 256 else 1.0))
                    n += 1
    out.append(Case("random", "f16", 128, RANDOM_L, (900, 17, 1033, 64, 63, 1500, 0), 3, heads=(8, 2), seed=997))
    out.append(Case("random", "bf16", 64, RANDOM_L, (40, 2047, 5, 1024), 1, heads=(4, 4), seed=998))
    return out


def closed_cases(dt: str, hd: int):
    out = tier_cases(dt, hd) + twin_cases(dt, hd) + flat_cases(dt, hd)
    for S in SPLITS:
        out += split_cases(dt, hd, S)
    return out


# ---- the tensors --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _base(dt: str, hd: int, L: int, n_kv: int, flat: bool, device: str):
    """(qg [n_kv, hd] of T, K, V [n_kv, L, hd] of T): shared by the closed-form cases of one bed; callers clone before they patch"""
    T = DT[dt]
    g = torch.Generator(device=device).manual_seed(7000 * hd + 10 * CODE[dt] + L)
    qg = torch.randn(n_kv, hd, device=device, generator=g).to(T)
    if flat:
        return qg, torch.zeros(n_kv, L, hd, dtype=T, device=device), torch.zeros(n_kv, L, hd, dtype=T, device=device)
    return qg, torch.randn(n_kv, L, hd, device=device, generator=g).to(T), coded_values(n_kv, L, hd, device).to(T)


def build(case: Case, device, fill=float("nan")):
    """-> dict q [R, n_heads * hd], K, V [n_kv, L, hd] of T (rows from n_max on hold `fill`), pos int64 [R]; for the closed forms also qg"""
    T, hd, L = DT[case.dt], case.hd, case.L
    n_heads, n_kv = case.heads
    R = len(case.pos)
    device = str(device)
    assert 1 <= R <= MAX_ROWS and all(0 <= p < L for p in case.pos)
    out = {"case": case, "pos": torch.tensor(case.pos, dtype=torch.int64, device=device)}
    if case.kind == "random":
        g = torch.Generator(device=device).manual_seed(31 * case.seed + 5)
        q = (torch.randn(R, n_heads * hd, device=device, generator=g) * case.qscale).to(T)
        K = torch.randn(n_kv, L, hd, device=device, generator=g).to(T)
        V = torch.randn(n_kv, L, hd, device=device, generator=g).to(T)
    else:
        assert n_heads == n_kv == HEADS
        qg, K0, V0 = _base(case.dt, hd, L, n_kv, case.kind == "flat", device)
        f = torch.tensor([1.0 + (i % 2) for i in range(R)], device=device).view(R, 1, 1)
        q = (qg.float().view(1, n_kv, hd) * f).to(T).reshape(R, n_kv * hd).contiguous()
        K, V = K0.clone(), V0.clone()
        hidx = torch.arange(n_kv, device=device)
        a = torch.tensor(case.a, dtype=torch.int64, device=device)
        b = torch.tensor(case.b, dtype=torch.int64, device=device)
        if case.kind == "flat":
            V[hidx, a] = flat_row(n_kv, hd, device).to(T)
        else:
            lo, hi = (qg.float() * C_NEEDLE).to(T), (qg.float() * 2 * C_NEEDLE).to(T)
            assert torch.equal(lo.double(), qg.double() * C_NEEDLE) and torch.equal(hi.double(), qg.double() * 2 * C_NEEDLE)
            K[hidx, a] = lo
            if case.kind == "twin":
                K[hidx, b] = lo
            elif case.kind == "tier":
                K[hidx, b] = hi
        out["qg"], out["V0"] = qg, V0
    n_max = case.n_max
    K[:, n_max:] = fill
    V[:, n_max:] = fill
    out["q"], out["K"], out["V"] = q, K, V
    return out


# ---- the fp64 reference ----------------------------------------------------------------------------------------------------------------------------
def reference_rows(q, K, V, pos, scaling: float):
    """fp64 softmax attention of R rows q [R, n_heads * hd] over K / V [n_kv, L, hd], row i over keys [0, pos[i]]: (out [R, n_heads, hd], scores [R, n_heads,
    n_max] with -inf on the masked keys).  Only the first n_max = max(pos) + 1 cache rows are read."""
    n_kv, _, hd = K.shape
    R = q.shape[0]
    n = int(pos.max()) + 1
    qq = q.double().view(R, n_kv, -1, hd)
    s = torch.einsum("rkgd,kjd->rkgj", qq, K[:, :n].double()) * scaling
    hidden = torch.arange(n, device=q.device).view(1, 1, 1, n) > pos.view(R, 1, 1, 1)
    s = s.masked_fill(hidden, -math.inf)
    o = torch.einsum("rkgj,kjd->rkgd", torch.softmax(s, -1), V[:, :n].double())
    return o.reshape(R, -1, hd), s.reshape(R, -1, n)


# ---- the band ----------------------------------------------------------------------------------------------------------------------------------------
def c_acc(n_max: int, S: int) -> float:
    chunk = -(-n_max // S)
    nbw = -(-(-(-chunk // BLOCK)) // WAVES)
    c = nbw * 44 + 2 * WAVES + 2 * (2 * EXP_ULPS + 1)
    return c + (1 if S == 1 else 2 * S + 2 * (2 * FAST_EXP_ULPS + 1) + 1)


def band(t, ref, scaling: float):
    """(tol, rest, lead): tol [R, n_heads, hd] as derived above; rest = the terms other than lead = u_T vmax_d and u_T |ref| (the band condition: rest < lead)"""
    case = t["case"]
    q, K, V, pos = t["q"], t["K"], t["V"], t["pos"]
    n_kv, _, hd = K.shape
    R, n = q.shape[0], case.n_max
    uT, sub = 2.0 ** -SIG_BITS[case.dt], 2.0 ** (MIN_EXP[case.dt] - SIG_BITS[case.dt])
    hidden = torch.arange(n, device=q.device).view(1, 1, 1, n) > pos.view(R, 1, 1, 1)
    A = torch.einsum("rkgd,kjd->rkgj", q.double().view(R, n_kv, -1, hd).abs(), K[:, :n].double().abs()).masked_fill(hidden, 0.0).amax(-1)   # [R, n_kv, rep]
    delta = ((hd + 2) * U32 * scaling * A).reshape(R, -1, 1)
    rep = A.shape[2]
    vmax = V[:, :n].double().abs().cummax(dim=1).values[:, pos].permute(1, 0, 2).repeat_interleave(rep, 1)   # [R, n_heads, hd]: the largest |V[j, d]| over j <= pos[i]
    n_vis = (pos + 1).double().view(R, 1, 1)
    eps_exp = 2 * U32 * EXP_ULPS
    rest = vmax * (2 * torch.expm1(2 * delta) + 2 * eps_exp + n_vis * sub + c_acc(n, case.S) * U32) + sub
    lead = uT * vmax
    return lead + uT * ref.abs() + rest, rest, lead


# ---- verdicts ------------------------------------------------------------------------------------------------------------------------------------------
def expected(t):
    """the closed form per (row, head) as fp64 [R, n_heads, hd], and exact [R, n_heads] bool: where it holds (a needle row that does not see its needle has none)"""
    case = t["case"]
    R, dev = len(case.pos), t["q"].device
    pos = t["pos"].view(R, 1)
    hidx = torch.arange(HEADS, device=dev)
    a = torch.tensor(case.a, dtype=torch.int64, device=dev)
    b = torch.tensor(case.b, dtype=torch.int64, device=dev)
    if case.kind == "flat":
        assert int(a.max()) <= min(case.pos)
        cf = flat_row(HEADS, case.hd, dev).double().view(1, HEADS, -1) / (pos + 1).double().view(R, 1, 1)
        return cf, torch.ones(R, HEADS, dtype=torch.bool, device=dev)
    Va, Vb = t["V0"][hidx, a].double(), t["V0"][hidx, b].double()
    if case.kind == "twin":
        return ((Va + Vb) / 2).view(1, HEADS, -1).expand(R, HEADS, case.hd), torch.ones(R, HEADS, dtype=torch.bool, device=dev)
    if case.kind == "tier":
        assert max(case.a) <= min(case.pos)
        sees = pos >= b.view(1, HEADS)
        return torch.where(sees.unsqueeze(-1), Vb.view(1, HEADS, -1), Va.view(1, HEADS, -1)), torch.ones(R, HEADS, dtype=torch.bool, device=dev)
    sees = pos >= a.view(1, HEADS)
    return Va.view(1, HEADS, -1).expand(R, HEADS, case.hd), sees


def closed_form_bad(t, ref):
    """[R, n_heads] bool: does the fp64 reference miss the closed form where one holds?  tier / needle / twin: rounded to T the same bits; flat: 1e-12 relative"""
    case = t["case"]
    cf, holds = expected(t)
    T = DT[case.dt]
    if case.kind == "flat":
        return ((ref - cf).abs() > 1e-12 * cf.abs()).any(-1) & holds
    return ((cf.to(T).double() != cf).any(-1) | (bits(ref.to(T)) != bits(cf.to(T))).any(-1)) & holds


def kernel_bad(t, got, ref, scaling: float):
    """[R, n_heads] bool: is the output [R, n_heads * hd] outside the case's bound around the fp64 reference?  (A NaN compares false: bad.)"""
    case = t["case"]
    T = DT[case.dt]
    got = got.view(ref.shape)
    err = (got.double() - ref).abs()
    in_band = (err <= band(t, ref, scaling)[0]).all(-1)
    if case.kind == "random":
        return ~in_band
    _, holds = expected(t)
    if case.kind == "twin":
        ok = (err <= ulp(ref, case.dt)).all(-1)
    elif case.kind == "flat":
        ok = (err <= ref.abs() * (2.0 ** -SIG_BITS[case.dt] + 2.0 ** -22)).all(-1)
    else:
        ok = (bits(got) == bits(ref.to(T))).all(-1)
    return ~torch.where(holds, ok, in_band)


def run(cases, device, kernel=None):
    """every case: the fp64 reference against its closed form and, with kernel(t) -> out [R, n_heads * hd], the kernel against the reference.  The verdicts
    stay on the device and are read back once.  Returns the ids of the failing (case, row, head) triples."""
    flags = []
    for case in cases:
        t = build(case, device)
        scaling = case.hd ** -0.5
        ref, _ = reference_rows(t["q"], t["K"], t["V"], t["pos"], scaling)
        f = torch.zeros(2, MAX_ROWS, max(HEADS, case.heads[0]), dtype=torch.bool, device=device)
        R, nh = len(case.pos), case.heads[0]
        if case.kind != "random":
            f[0, :R, :nh] = closed_form_bad(t, ref)
        if kernel is not None:
            f[1, :R, :nh] = kernel_bad(t, kernel(t), ref, scaling)
        flags.append(f)
    flags = torch.stack(flags).cpu()
    names = ("the fp64 reference misses the closed form", "the kernel misses the fp64 reference")
    return [f"{cases[i].id} row {r} head {h}: {names[c]}" for i, c, r, h in flags.nonzero().tolist()]


def summary(bad, what):
    return f"{what}: {len(bad)} failures, first: " + "; ".join(bad[:6])


def margins(t):
    """fp64, over the whole un-patched bed: (the 32-needle's score minus the largest background score, the 64-needle's minus the 32-needle's), each at its least
    over the heads, for the rows with f = 1 (a row with f = 2 doubles both, and both are positive)"""
    case = t["case"]
    qg = t["qg"].double()
    K0 = _base(case.dt, case.hd, case.L, HEADS, False, str(t["q"].device))[1].double()
    scaling = case.hd ** -0.5
    bg = torch.einsum("hd,hjd->hj", qg, K0).amax(-1) * scaling
    nd = (qg * qg).sum(-1) * C_NEEDLE * scaling
    return float((nd - bg).min()), float(nd.min())


# ---- the host emulation ------------------------------------------------------------------------------------------------------------------------------
def emulate(t, order: str):
    """what the kernel states, on the host: fp32 scores, blocks of 32 keys, a running (m, l, O) per row, P rounded to T for the product with V, fp32 accumulation;
    order "waves": the blocks of a share dealt round-robin to 8 accumulators merged in order (the kernel's), "serial": one accumulator over the blocks in
    descending order.  The shares are merged as attn_combine_kernel merges them.  -> out [R, n_heads * hd] of T"""
    case = t["case"]
    T, hd, S = DT[case.dt], case.hd, case.S
    q, K, V, pos = t["q"], t["K"], t["V"], t["pos"]
    n_kv = K.shape[0]
    R, n = q.shape[0], case.n_max
    rep = case.heads[0] // n_kv
    scaling = torch.tensor(hd ** -0.5, dtype=torch.float32)
    qf = q.float().view(R, n_kv, rep, hd)
    ninf = torch.tensor(-math.inf)

    def fresh():
        return [torch.full((R, n_kv, rep), -math.inf), torch.zeros(R, n_kv, rep), torch.zeros(R, n_kv, rep, hd)]

    def fold(acc, j0, j1):
        m, l, O = acc
        s = torch.einsum("rkgd,kjd->rkgj", qf, K[:, j0:j1].float()) * scaling
        s = torch.where(torch.arange(j0, j1).view(1, 1, 1, -1) > pos.view(R, 1, 1, 1), ninf, s)
        m_new = torch.maximum(m, s.amax(-1))
        m_sub = torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)
        alpha = torch.exp(m - m_sub)
        p = torch.exp(s - m_sub.unsqueeze(-1))
        acc[0], acc[1] = m_new, l * alpha + p.sum(-1)
        acc[2] = O * alpha.unsqueeze(-1) + torch.einsum("rkgj,kjd->rkgd", p.to(T).float(), V[:, j0:j1].float())

    def merge(parts):
        mm = torch.stack([a[0] for a in parts]).amax(0)
        num, den = torch.zeros_like(parts[0][2]), torch.zeros_like(parts[0][1])
        for m, l, O in parts:
            w = torch.where(l > 0, torch.exp(m - mm), torch.zeros_like(l))
            num, den = num + w.unsqueeze(-1) * O, den + w * l
        return [mm, den, num]

    recs = []
    for k0, k1 in shares(n, S):
        blocks = [(j, min(j + BLOCK, k1)) for j in range(k0, k1, BLOCK)]
        if order == "waves":
            accs = [fresh() for _ in range(WAVES)]
            for i, (j0, j1) in enumerate(blocks):
                fold(accs[i % WAVES], j0, j1)
            recs.append(merge(accs))
        else:
            acc = fresh()
            for j0, j1 in reversed(blocks):
                fold(acc, j0, j1)
            recs.append(acc)
    m, l, O = merge(recs) if S > 1 else recs[0]
    return (O / l.unsqueeze(-1)).to(T).reshape(R, -1)


# ---- the raw C-ABI call (argument checks) ----------------------------------------------------------------------------------------------------------------
def call(lib, t, out, rows=None, S=None, ws_ptr=0, ws_bytes=0) -> int:
    case = t["case"]
    n_heads, n_kv = case.heads
    st = torch.cuda.current_stream().cuda_stream
    return lib.hqq_hip_attn_decode_tiled(t["q"].data_ptr(), t["K"].data_ptr(), t["V"].data_ptr(), t["pos"].data_ptr(), len(case.pos) if rows is None else rows,
                                         out.data_ptr(), n_heads, n_kv, case.hd, case.L, case.hd ** -0.5, CODE[case.dt], case.S if S is None else S, ws_ptr, ws_bytes, st)
