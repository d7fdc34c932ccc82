"""Shared by tests/test_gqa_attn_cpu.py and tests/test_gqa_attn_gpu.py: the cases, the fp64 reference and the verdicts for the grouped-query decode attention
(csrc/attn_gqa.hip, hqq_hip_attn_decode_gqa_batched / _gqa_kvq_batched; ops.attn_decode_gqa*): B sequences, sequence b over keys [0, pos[b]], the G = n_heads /
n_kv query heads of a KV group as the rows of one MFMA query tile.  Every expected value is fp64 attention over the same tensors, never another kernel's output.

The kernel runs the tile kernel's body (csrc/attn_tile_core.h), so ONE SEQUENCE of a case is a problem of tests/_tile_cases.py seen transposed — its rows are the
G heads of a group, its heads the n_kv KV heads, every row at the sequence's position (tile_view) — and the fp64 reference (_tile_cases.reference_rows) and the
band (_tile_cases.band, unchanged: the arithmetic is the tile kernel's term by term) are taken per sequence through that view.  The band's condition stays in
force for every random case (rest < lead, checked on the CPU); head_dim 256 draws its queries at a quarter of the scale, as there.

Closed forms (one key decides the output), the heads of a group as the rows: q[kvh G + u] = f_u qg[kvh], f_u in {1, 2}
  needle   key a holds 32 qg[kvh]: every head of the group gives V[a] bit for bit
  twin     keys a != b both hold 32 qg[kvh]: (V[a] + V[b]) / 2 within one ulp of T
  flat     K = 0, V zero but for key j*: V[j*] / (pos + 1) within _attn_cases' flat bound
  ident    the one form that tells the heads of a group APART: K = 0 but for G keys j_u, distinct per head, K[j_u] = 64 e_(d_u) with d_u distinct per head, and
           head u queries 64 e_(d_u).  Its score is 4096 / sqrt(hd) >= 256 at j_u and exactly 0 at every other key (a zero row, or another head's direction), so
           head u returns V[j_u] bit for bit: the other keys weigh e^-256 each, which vanishes against half an ulp of any nonzero 7-bit integer V in fp64 and, where
           V[j_u, d] = 0, leaves less than 2047 * 127 * e^-256 — below half of T's smallest subnormal in both dtypes (test_gqa_attn_cpu checks the fp64 reference
           rounded to T against V[j_u]).  A swapped or repeated head-to-row mapping returns another head's V[j_u'] and fails this form and no other.
Random cases (randn q, K, V; NaN beyond each sequence's position) catch a mis-weighted rescale.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

import _tile_cases as tc
from _attn_cases import C_NEEDLE, CODE, DT, SIG_BITS, bits, coded_values, flat_row, ulp  # noqa: F401

HEADS = ((4, 2), (8, 2), (7, 1), (16, 1), (8, 8))     # G = 2, 4, 7, 16 and the degenerate 1
HDS = (64, 128, 256)
DTS = ("f16", "bf16")
SPLITS = (1, 2, 3, 7, 16)
L_BIG = 2048
IDENT_C = 64.0
# ragged, unsorted positions: 0, 31, 32, 255, 256, 257, 1023 and L - 1 all occur, in batches of 3 and of 1
POS3 = ((257, 0, 1023), (31, L_BIG - 1, 32), (255, 256, 5), (1023, 1500, 64))
POS1 = ((L_BIG - 1,), (1023,), (0,), (300,), (32,), (256,))


@dataclass(frozen=True)
class Case:
    kind: str            # "needle" | "twin" | "flat" | "ident" | "random"
    dt: str
    hd: int
    L: int
    heads: tuple         # (n_heads, n_kv)
    pos: tuple           # one position per sequence
    S: int = 1
    seed: int = 0

    @property
    def id(self):
        return f"{self.kind}-{self.dt}-hd{self.hd}-h{self.heads[0]}.{self.heads[1]}-p{'.'.join(map(str, self.pos))}-s{self.S}-seed{self.seed}"

    @property
    def G(self):
        return self.heads[0] // self.heads[1]

    @property
    def qscale(self):
        return 0.25 if self.hd == 256 else 1.0


def _cycle(seq, i):
    return seq[i % len(seq)]


def closed_cases(dt: str, hd: int):
    """every head shape x every kind, the positions and splits cycling with periods coprime to each other so that every split meets every kind and head shape;
    flat stays within FLAT_MAX_N keys, twin needs two keys and ident G of them (their position lists leave the short sequences out)"""
    out, n = [], 0
    for ih, heads in enumerate(HEADS):
        G = heads[0] // heads[1]
        for kind in ("needle", "twin", "flat", "ident"):
            for rep in range(3):
                pos = _cycle(POS3, n) if rep < 2 else _cycle(POS1, n)
                if kind == "flat":
                    pos = tuple(min(p, tc.FLAT_MAX_N - 1) for p in pos)
                if kind == "twin":
                    pos = tuple(max(p, 1) for p in pos)
                if kind == "ident":
                    pos = tuple(max(p, 31) for p in pos)     # (>= 16 keys for the heads' own)
                out.append(Case(kind, dt, hd, L_BIG, heads, pos, _cycle(SPLITS, n + rep), seed=n))
                n += 1
    # n < S on purpose: one visible key, sixteen shares
    out.append(Case("needle", dt, hd, L_BIG, (8, 2), (0, 2, 1), 16, seed=n))
    out.append(Case("flat", dt, hd, L_BIG, (16, 1), (0,), 7, seed=n + 1))
    return out


def random_cases():
    """every (head shape, hd, dtype): a ragged batch of 3 and a single sequence, splits cycling through SPLITS (n < S occurs: position 0 under S > 1)"""
    out, n = [], 0
    for heads in HEADS:
        for hd in HDS:
            for dt in DTS:
                out.append(Case("random", dt, hd, L_BIG, heads, _cycle(POS3, n), _cycle(SPLITS, n), seed=100 + n))
                out.append(Case("random", dt, hd, L_BIG, heads, _cycle(POS1, n), _cycle(SPLITS, n + 2), seed=500 + n))
                n += 1
    out.append(Case("random", "f16", 128, 320, (8, 2), (319, 0, 31), 3, seed=901))      # a short cache, L - 1
    return out


# ---- the tensors --------------------------------------------------------------------------------------------------------------------------------------
def _probe(n: int, hd: int, i: int):
    return tc.places(n, hd)[i % 8]


def ident_keys(case: Case, b: int, kvh: int):
    """(j_u, d_u) for u < G: the key and the direction of head u of group kvh in sequence b, both distinct within the group"""
    G, n = case.G, case.pos[b] + 1
    stride = n // G
    assert stride >= 1
    off = (7 * kvh + 3 * b + case.seed) % stride
    return [u * stride + off for u in range(G)], [(4 * u + kvh) % case.hd for u in range(G)]


def build(case: Case, device, fill=float("nan")):
    """-> dict q [B, n_heads * hd], K, V [B, n_kv, L, hd] of T (sequence b's rows beyond pos[b] hold `fill`), pos int64 [B]; for the closed forms also V0 (V before
    the fill) and the probes a, b [B, n_kv]"""
    T, hd, L = DT[case.dt], case.hd, case.L
    n_heads, n_kv = case.heads
    B, G = len(case.pos), case.G
    device = str(device)
    assert n_heads == n_kv * G and 1 <= G <= 16 and all(0 <= p < L for p in case.pos)
    g = torch.Generator(device=device).manual_seed(7919 * case.seed + 13 * hd + CODE[case.dt])
    out = {"case": case, "pos": torch.tensor(case.pos, dtype=torch.int64, device=device)}
    if case.kind == "random":
        q = (torch.randn(B, n_heads * hd, device=device, generator=g) * case.qscale).to(T)
        K = torch.randn(B, n_kv, L, hd, device=device, generator=g).to(T)
        V = torch.randn(B, n_kv, L, hd, device=device, generator=g).to(T)
    else:
        qg = torch.randn(B, n_kv, hd, device=device, generator=g).to(T)
        f = torch.tensor([1.0 + (u % 2) for u in range(G)], device=device).view(1, 1, G, 1)
        q = (qg.float().view(B, n_kv, 1, hd) * f).to(T).reshape(B, n_heads * hd).contiguous()
        V = torch.stack([coded_values(n_kv, L + 5 * B, hd, device)[:, 5 * b:5 * b + L] for b in range(B)]).to(T)   # (sequence b: the code of key j + 5 b)
        K = torch.randn(B, n_kv, L, hd, device=device, generator=g).to(T)
        a = torch.zeros(B, n_kv, dtype=torch.int64, device=device)
        bb = torch.zeros(B, n_kv, dtype=torch.int64, device=device)
        if case.kind in ("flat", "ident"):
            K.zero_()
        if case.kind == "flat":
            V.zero_()
        for b in range(B):
            n = case.pos[b] + 1
            for kvh in range(n_kv):
                ia = _probe(n, hd, kvh + 3 * b + case.seed)
                ib = _probe(n, hd, kvh + 3 * b + case.seed + 3)
                if ib == ia:
                    ib = (ia + max(1, n // 2)) % n
                a[b, kvh], bb[b, kvh] = ia, ib
                if case.kind == "flat":
                    V[b, kvh, ia] = flat_row(n_kv, hd, device)[kvh].to(T)
                elif case.kind == "ident":
                    js, ds = ident_keys(case, b, kvh)
                    for u, (j, d) in enumerate(zip(js, ds)):
                        K[b, kvh, j, d] = IDENT_C
                        q[b, (kvh * G + u) * hd:(kvh * G + u + 1) * hd] = 0
                        q[b, (kvh * G + u) * hd + d] = IDENT_C
                else:
                    lo = (qg[b, kvh].float() * C_NEEDLE).to(T)
                    assert torch.equal(lo.double(), qg[b, kvh].double() * C_NEEDLE)
                    K[b, kvh, ia] = lo
                    if case.kind == "twin":
                        assert ib != ia
                        K[b, kvh, ib] = lo
        out["a"], out["b"], out["V0"] = a, bb, V.clone()
    for b, p in enumerate(case.pos):
        K[b, :, p + 1:] = fill
        V[b, :, p + 1:] = fill
    out["q"], out["K"], out["V"] = q, K, V
    return out


# ---- one sequence as a problem of _tile_cases ----------------------------------------------------------------------------------------------------------------
def to_rows(x, n_kv: int, G: int, hd: int):
    """[n_heads (* hd)] of one sequence, head kvh G + u -> the tile's [G rows, n_kv heads, hd]"""
    return x.reshape(n_kv, G, hd).permute(1, 0, 2).contiguous()


def to_heads(x):
    """the tile's [G, n_kv, hd] -> [n_heads, hd]"""
    return x.permute(1, 0, 2).reshape(-1, x.shape[-1])


def tile_view(t, b: int):
    """sequence b as _tile_cases sees it: rows = the G heads of a group, heads = the KV heads (n_heads = n_kv there), every row at pos[b], the same splits"""
    case = t["case"]
    n_kv, G = case.heads[1], case.G
    tcase = tc.Case("random", case.dt, case.hd, case.L, (case.pos[b],) * G, case.S, heads=(n_kv, n_kv), seed=case.seed, qscale=case.qscale)
    return {"case": tcase, "q": to_rows(t["q"][b], n_kv, G, case.hd).reshape(G, n_kv * case.hd), "K": t["K"][b], "V": t["V"][b],
            "pos": t["pos"][b:b + 1].expand(G).contiguous()}


def reference(t):
    """fp64 attention -> [B, n_heads, hd]"""
    case = t["case"]
    return torch.stack([to_heads(tc.reference_rows(v["q"], v["K"], v["V"], v["pos"], case.hd ** -0.5)[0]) for v in (tile_view(t, b) for b in range(len(case.pos)))])


def band(t, ref):
    """_tile_cases.band per sequence, unchanged -> (tol, rest, lead), each [B, n_heads, hd]"""
    case = t["case"]
    n_kv, G, hd = case.heads[1], case.G, case.hd
    outs = []
    for b in range(len(case.pos)):
        tol, rest, lead = tc.band(tile_view(t, b), to_rows(ref[b], n_kv, G, hd), hd ** -0.5)
        outs.append([to_heads(x.expand(G, n_kv, hd)) for x in (tol, rest, lead)])
    return tuple(torch.stack([o[i] for o in outs]) for i in range(3))


# ---- verdicts ------------------------------------------------------------------------------------------------------------------------------------------------
def expected(t):
    """the closed form as fp64 [B, n_heads, hd]"""
    case = t["case"]
    B, (n_heads, n_kv), G, hd = len(case.pos), case.heads, case.G, case.hd
    dev = t["q"].device
    bi = torch.arange(B, device=dev).view(B, 1)
    ki = torch.arange(n_kv, device=dev).view(1, n_kv)
    if case.kind == "flat":
        cf = flat_row(n_kv, hd, dev).double().view(1, n_kv, hd) / (t["pos"] + 1).double().view(B, 1, 1)
        return cf.repeat_interleave(G, 1)
    V0 = t["V0"].double()
    if case.kind == "ident":
        cf = torch.empty(B, n_heads, hd, dtype=torch.float64, device=dev)
        for b in range(B):
            for kvh in range(n_kv):
                for u, j in enumerate(ident_keys(case, b, kvh)[0]):
                    cf[b, kvh * G + u] = V0[b, kvh, j]
        return cf
    Va = V0[bi, ki, t["a"]]
    if case.kind == "twin":
        Va = (Va + V0[bi, ki, t["b"]]) / 2
    return Va.repeat_interleave(G, 1)


def closed_form_bad(t, ref):
    """[B, n_heads] bool: does the fp64 reference miss the closed form?  needle / ident / twin: rounded to T the same bits (twin's mean of two 7-bit integers is
    exact in T); flat: 1e-12 relative"""
    case = t["case"]
    cf = expected(t)
    T = DT[case.dt]
    if case.kind == "flat":
        return ((ref - cf).abs() > 1e-12 * cf.abs()).any(-1)
    return (cf.to(T).double() != cf).any(-1) | (bits(ref.to(T)) != bits(cf.to(T))).any(-1)


def kernel_bad(t, got, ref):
    """[B, n_heads] bool: is the output [B, n_heads * hd] outside the case's bound around the fp64 reference?  (A NaN compares false: bad.)"""
    case = t["case"]
    T = DT[case.dt]
    got = got.view(ref.shape)
    err = (got.double() - ref).abs()
    if case.kind == "random":
        return ~(err <= band(t, ref)[0]).all(-1)
    if case.kind == "twin":
        return ~(err <= ulp(ref, case.dt)).all(-1)
    if case.kind == "flat":
        return ~(err <= ref.abs() * (2.0 ** -SIG_BITS[case.dt] + 2.0 ** -22)).all(-1)
    return ~(bits(got) == bits(ref.to(T))).all(-1)


def run(cases, device, kernel=None):
    """every case: the fp64 reference against its closed form and, with kernel(t) -> out [B, n_heads * hd], the kernel against the reference.  The verdicts stay
    on the device and are read back once.  Returns the ids of the failing (case, sequence, head) triples."""
    flags = []
    for case in cases:
        t = build(case, device)
        ref = reference(t)
        f = torch.zeros(2, 3, 16, dtype=torch.bool, device=device)
        B, nh = len(case.pos), case.heads[0]
        if case.kind != "random":
            f[0, :B, :nh] = closed_form_bad(t, ref)
        if kernel is not None:
            f[1, :B, :nh] = kernel_bad(t, kernel(t), ref)
        flags.append(f)
    flags = torch.stack(flags).cpu()
    names = ("the fp64 reference misses the closed form", "the kernel misses the fp64 reference")
    return [f"{cases[i].id} sequence {b} head {h}: {names[c]}" for i, c, b, h in flags.nonzero().tolist()]


def summary(bad, what):
    return f"{what}: {len(bad)} failures, first: " + "; ".join(bad[:6])


# ---- the raw C-ABI call (argument checks) --------------------------------------------------------------------------------------------------------------------
def call(lib, t, out, *, heads=None, hd=None, S=None, ws_ptr=0, ws_bytes=0, q_ptr=None, k_ptr=None) -> int:
    case = t["case"]
    n_heads, n_kv = case.heads if heads is None else heads
    st = torch.cuda.current_stream().cuda_stream
    return lib.hqq_hip_attn_decode_gqa_batched(t["q"].data_ptr() if q_ptr is None else q_ptr, t["K"].data_ptr() if k_ptr is None else k_ptr, t["V"].data_ptr(),
                                               t["pos"].data_ptr(), len(case.pos), out.data_ptr(), n_heads, n_kv, case.hd if hd is None else hd, case.L,
                                               case.hd ** -0.5, CODE[case.dt], case.S if S is None else S, ws_ptr, ws_bytes, st)
