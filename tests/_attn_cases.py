"""Shared by tests/test_attn_keys_cpu.py and tests/test_attn_keys_gpu.py: inputs for the decode-attention kernels (csrc/block.hip,
attn_decode_kernel / attn_combine_kernel) in which ONE key decides the output, the grid of visible-key counts, needle places and split
counts they run at, the fp64 reference, and the raw C-ABI calls.

With randn inputs one key carries about 1 / n of the output: above roughly a thousand keys a kernel that drops, duplicates or mis-weights a
key stays inside any tolerance that admits fp16 rounding.  Here the fp64 result has a closed form that every such error changes grossly:

  needle   background keys are randn (scores small but not zero), the key at the needle position is C q: the softmax puts all but e^-100 of
           its mass there, and the output is V[needle] BIT FOR BIT.  C = 32 is a power of two, so C q is exact in fp16 and bf16, and the
           needle's score C |q|^2 / sqrt(hd) exceeds every background score by more than 100 (checked by the CPU file for every bed): a
           share without the needle merges with e^(m_s - m) = 0.  A background score that phase 2 leaves un-exponentiated is O(1), not
           e^-100, and shows through its V row.
  twin     two keys at different places hold the same C q: each gets exactly half, the output is T((V[a] + V[b]) / 2) — exactly
           representable (|V| <= 127, so the mean has at most 8 significant bits) — within one ulp of T.  A needle counted twice, or
           counted in the sum but not in the output, passes `needle` and fails here.
  flat     K = 0: every score is 0, p = 1 / n.  V is 0 except at one key j*, which holds powers of two: the output is V[j*] / n, one fp32
           division and one rounding to T away from exact: |got - want| <= |want| (2^-23 + 2^-p + their product) < |want| (2^-p + 2^-22),
           p = 11 (fp16) or 8 (bf16) significant bits.  It resolves ONE key too many or too few in the sum (a relative 1 / n) only while
           1 / n is above that bound — to n of about 1000 in fp16 and 128 in bf16 — and is therefore not run above n = 1025; a dropped
           or misplaced j* is caught at any n.

V is position-coded: V[kvh, j, d] = ((37 j + 11 d + 53 kvh) mod 127 + 1) * (-1)^(d + kvh), a nonzero integer of at most 7 bits (exact in
bf16) that differs between neighbouring keys and neighbouring heads in every element; never 0, so the residual softmax mass cannot become a
relative error of 1 in the reference itself.

One launch probes one place per KV head (n_kv == n_heads outside the GQA cases: each head reads its own cache rows).  Cache rows beyond the
visible keys are NaN.  Every case checks its closed form against fp64 softmax attention over the same tensors — that is all the CPU file
runs — and the GPU result is compared with that fp64 result, never with another kernel's output."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

F16, BF16 = 1, 2
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f16": F16, "bf16": BF16}
SIG_BITS = {"f16": 11, "bf16": 8}      # significant bits of T

C_NEEDLE = 32.0
HEADS = 8                              # probes per launch
HDS = (64, 128, 256)                   # the head sizes the entry points accept
MAX_L, MAX_SPLITS = 30000, 64          # attn_decode_run's limits
FLAT_MAX_N = 1025
LONG_NS = (1024, 1025, 2048, 4001, 8191, 20000, 29999, 30000)
SPLITS = (2, 3, 7, 8, 16, 64)


def step(hd: int) -> int:
    """keys per pass of the eight waves in phases 1 and 3 (STEP in attn_decode_kernel): 64, 32, 16"""
    return 8 * (512 // hd)


def sweep_max_n(hd: int) -> int:
    return 2 * 4 * step(hd) + step(hd) + 1


def split_ns(S: int):
    return sorted({n for n in (1, 2, S - 1, S, S + 1, 37, 1025, 4001, 20000) if n >= 1})


def shares(n: int, S: int):
    """[k0, k1) of every share, as the kernel cuts them: chunk = ceil(n / S); k1 <= k0 is an empty share"""
    chunk = (n + S - 1) // S
    return [(s * chunk, min(s * chunk + chunk, n)) for s in range(S)]


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Launch:
    kind: str            # "needle" | "twin" | "flat"
    n: int               # visible keys: pos = n - 1
    S: int               # splits
    a: tuple             # per KV head: the needle (needle, twin) or j* (flat)
    b: tuple             # per KV head: the second needle (twin); == a otherwise

    @property
    def id(self):
        return f"{self.kind}-n{self.n}-s{self.S}-" + ".".join(str(x) if x == y else f"{x}+{y}" for x, y in zip(self.a, self.b))


def _fill(seq, k=HEADS):
    seq = list(seq)
    return tuple(seq[i % len(seq)] for i in range(k))


def places(n: int, hd: int):
    """key 0, n - 1, n - 2, the middle, and both sides of the last multiple of STEP and of 4 STEP below n"""
    st = step(hd)
    m1 = (n - 1) // st * st
    m4 = (n - 1) // (4 * st) * (4 * st)
    return tuple(min(max(p, 0), n - 1) for p in (0, n - 1, n - 2, n // 2, m1 - 1, m1, m4 - 1, m4))


def _one_workgroup(n: int, hd: int, flat: bool):
    a = places(n, hd)
    out = [Launch("needle", n, 1, a, a)]
    if n >= 2:
        b = tuple(a[(i + 3) % HEADS] for i in range(HEADS))
        out.append(Launch("twin", n, 1, a, tuple(y if y != x else (x + 1) % n for x, y in zip(a, b))))
    if flat and n <= FLAT_MAX_N:
        out.append(Launch("flat", n, 1, a, a))
    return out


def sweep_launches(hd: int):
    """every n from 1 to 2 * 4 STEP + STEP + 1: every residue of the 4-unrolled loops and of their tails, the wave and sub-row of the last key varying"""
    return [l for n in range(1, sweep_max_n(hd) + 1) for l in _one_workgroup(n, hd, True)]


def long_launches(hd: int):
    return [l for n in LONG_NS for l in _one_workgroup(n, hd, False)]


def split_launches(hd: int, S: int):
    """per n: a needle at the first and at the last key of every non-empty share; twins in two different shares; flat scores up to FLAT_MAX_N"""
    out = []
    for n in split_ns(S):
        live = [(k0, k1) for k0, k1 in shares(n, S) if k0 < k1]
        probes = [p for k0, k1 in live for p in (k0, k1 - 1)]
        for i in range(0, len(probes), HEADS):
            a = _fill(probes[i:i + HEADS])
            out.append(Launch("needle", n, S, a, a))
        if len(live) >= 2:
            ns = len(live)
            pa, pb = [], []
            for t in range(HEADS):
                i, j = (t * 5) % ns, (t * 3 + 1) % ns
                if i == j:
                    j = (i + 1) % ns
                pa.append(live[i][0])
                pb.append(live[j][1] - 1)
            out.append(Launch("twin", n, S, tuple(pa), tuple(pb)))
        if n <= FLAT_MAX_N:
            a = _fill(probes[::max(1, len(probes) // HEADS)])
            out.append(Launch("flat", n, S, a, a))
    return out


# ---- the tensors ----------------------------------------------------------------------------------------------------------------------
def coded_values(n_kv: int, L: int, hd: int, device):
    kvh = torch.arange(n_kv, device=device).view(-1, 1, 1)
    j = torch.arange(L, device=device).view(1, -1, 1)
    d = torch.arange(hd, device=device).view(1, 1, -1)
    return (((37 * j + 11 * d + 53 * kvh) % 127 + 1) * (1 - 2 * ((d + kvh) % 2))).float()


def flat_row(n_kv: int, hd: int, device):
    """what V[j*] holds in a flat case: +-2^0 .. 2^7 (V[j*] / n stays a normal fp16 number for every n <= FLAT_MAX_N)"""
    kvh = torch.arange(n_kv, device=device).view(-1, 1)
    d = torch.arange(hd, device=device).view(1, -1)
    return (2.0 ** ((d + 3 * kvh) % 8) * (1 - 2 * ((d + kvh) % 2))).float()


def reference(q, K, V, n: int, scaling: float):
    """fp64 softmax attention of q [n_heads, hd] over the first n rows of K / V [n_kv, L, hd] (any dtype); returns (out [n_heads, hd], scores)"""
    n_kv, hd = K.shape[0], K.shape[-1]
    qq = q.double().view(n_kv, -1, hd)
    s = torch.matmul(qq, K[:, :n].double().transpose(1, 2)) * scaling
    return torch.matmul(torch.softmax(s, -1), V[:, :n].double()).view(-1, hd), s.view(-1, n)


class Bed:
    """q and the caches of one (dtype, head size, cache length), patched in place per launch and restored after it.  Launches must come with
    n descending: the rows from n on are turned to NaN and stay so.  `mirror`: fp64 copies of the caches kept in step with every patch,
    which the reference then reads (on the CPU, converting 8 x 30000 x 256 values per launch would take most of the time)."""

    def __init__(self, dt: str, hd: int, L: int, device, *, heads: int = HEADS, rep: int = 1, flat: bool = False, mirror: bool = False, seed: int = 0):
        assert hd in HDS and 1 <= L <= MAX_L
        self.dt, self.T, self.hd, self.L, self.n_kv, self.rep, self.flat, self.device = dt, DT[dt], hd, L, heads, rep, flat, device
        self.n_heads, self.scaling = heads * rep, hd ** -0.5
        g = torch.Generator(device=device).manual_seed(1000 * hd + 10 * CODE[dt] + seed)
        qg = torch.randn(heads, hd, device=device, generator=g).to(self.T)
        # the query heads of a group: the group's q times 1 or 2 — different bits, the same needle (its score only grows)
        f = torch.tensor([1.0 + (r % 2) for r in range(rep)], device=device).view(1, rep, 1)
        self.q = (qg.view(heads, 1, hd).float() * f).to(self.T).reshape(self.n_heads, hd).contiguous()
        if flat:
            self.kc = torch.zeros(heads, L, hd, dtype=self.T, device=device)
            self.vc = torch.zeros(heads, L, hd, dtype=self.T, device=device)
            self.patch = flat_row(heads, hd, device).to(self.T)
        else:
            self.kc = torch.randn(heads, L, hd, device=device, generator=g).to(self.T)
            self.vc = coded_values(heads, L, hd, device).to(self.T)
            self.patch = (qg.float() * C_NEEDLE).to(self.T)
            assert torch.equal(self.patch.double(), qg.double() * C_NEEDLE) and bool((self.vc != 0).all())
        self.target = self.vc if flat else self.kc
        self.k64 = self.kc.double() if mirror else None
        self.v64 = self.vc.double() if mirror else None
        self.target64 = self.v64 if flat else self.k64
        self.visible = L
        self.hidx = torch.arange(heads, device=device)
        self._saved = None

    def shrink(self, n: int):
        assert 1 <= n <= self.visible, "launches of a bed come with n descending"
        if n < self.visible:
            self.kc[:, n:self.visible] = float("nan")
            self.vc[:, n:self.visible] = float("nan")
            self.visible = n

    def apply(self, a, b):
        """a, b: int64 [n_kv] on the device.  Puts the patch row at a, then at b; returns nothing — restore() undoes it"""
        assert self._saved is None
        sa = self.target[self.hidx, a].clone()
        self.target[self.hidx, a] = self.patch
        sb = self.target[self.hidx, b].clone()
        self.target[self.hidx, b] = self.patch
        self._saved = (a, b, sa, sb)
        if self.target64 is not None:
            self.target64[self.hidx, a] = self.patch.double()
            self.target64[self.hidx, b] = self.patch.double()

    def restore(self):
        a, b, sa, sb = self._saved
        self.target[self.hidx, b] = sb
        self.target[self.hidx, a] = sa
        if self.target64 is not None:
            self.target64[self.hidx, b] = sb.double()
            self.target64[self.hidx, a] = sa.double()
        self._saved = None

    def reference(self, n: int):
        K, V = (self.kc, self.vc) if self.k64 is None else (self.k64, self.v64)
        return reference(self.q, K, V, n, self.scaling)

    def closed_form(self, kind: str, n: int, a, b):
        """fp64 [n_heads, hd]: V[a] (needle), (V[a] + V[b]) / 2 (twin), V[j*] / n (flat), the same for every query head of a group"""
        if kind == "flat":
            cf = self.patch.double() / n
        else:
            cf = (self.vc[self.hidx, a].double() + self.vc[self.hidx, b].double()) / 2
        return cf.repeat_interleave(self.rep, 0)


def bits(t):
    return t.contiguous().view(torch.int16)


def ulp(x, dt: str):
    """one unit in the last place of T at |x| (fp64 in, fp64 out; x != 0 and normal in T)"""
    _, e = torch.frexp(x)                       # |x| = m 2^e, m in [0.5, 1): ulp = 2^(e - 1 - (p - 1))
    return torch.ldexp(torch.ones_like(x), e - SIG_BITS[dt])


def closed_form_bad(bed: Bed, kind: str, n: int, a, b, ref):
    """per query head: does the fp64 reference miss the closed form?  needle / twin: rounded to T they are the same bits; flat: 1e-12 relative"""
    cf = bed.closed_form(kind, n, a, b)
    if kind == "flat":
        return ((ref - cf).abs() > 1e-12 * cf.abs()).any(-1)
    assert kind in ("needle", "twin")
    return (cf.to(bed.T).double() != cf).any(-1) | (bits(ref.to(bed.T)) != bits(cf.to(bed.T))).any(-1)


def kernel_bad(bed: Bed, kind: str, got, ref):
    """per query head: is the kernel's output [n_heads, hd] outside the kind's bound around the fp64 reference?"""
    if kind == "needle":
        return (bits(got) != bits(ref.to(bed.T))).any(-1)
    err = (got.double() - ref).abs()
    if kind == "twin":
        tol = ulp(ref, bed.dt)
    else:
        tol = ref.abs() * (2.0 ** -SIG_BITS[bed.dt] + 2.0 ** -22)
    return ~(err <= tol).all(-1)                 # (a NaN compares false: bad)


# ---- the calls (device) -----------------------------------------------------------------------------------------------------------------
def workspace_bytes(lib, n_heads: int, hd: int, S: int) -> int:
    return int(lib.hqq_hip_attn_decode_workspace_bytes(n_heads, hd, S))


def call(lib, *, rope: bool, dt: str, q, kc, vc, pos, out, S: int, ws_ptr, ws_bytes, k=None, v=None, cos=None, sin=None, batch=None) -> int:
    """the C entry point itself (the batch-1 one, or with `batch` the *_batched one); returns its return code"""
    st = torch.cuda.current_stream().cuda_stream
    hd, L = kc.shape[-1], kc.shape[-2]
    n_kv = kc.shape[-3]
    n_heads = q.numel() // hd // (batch or 1)
    tail = (n_heads, n_kv, hd, L, hd ** -0.5, CODE[dt], S, ws_ptr, ws_bytes, st)
    p = lambda t: t.data_ptr()   # noqa: E731
    if rope:
        head = (p(q), p(k), p(v), p(cos), p(sin), p(pos))
        if batch:
            return lib.hqq_hip_rope_attn_decode_batched(*head, batch, p(kc), p(vc), p(out), *tail)
        return lib.hqq_hip_rope_attn_decode(*head, p(kc), p(vc), p(out), *tail)
    if batch:
        return lib.hqq_hip_attn_decode_batched(p(q), p(kc), p(vc), p(pos), batch, p(out), *tail)
    return lib.hqq_hip_attn_decode(p(q), p(kc), p(vc), p(pos), p(out), *tail)


def unit_angles(hd: int, T, device, batch: int = 1):
    """cos = 1, sin = 0: the rotary embedding returns its input bit for bit (x * 1 + rotate_half(x) * 0), the closed forms stay exact"""
    return torch.ones(batch, hd, dtype=T, device=device), torch.zeros(batch, hd, dtype=T, device=device)


def run(bed: Bed, launches, kernel=None):
    """Every launch of the list on the bed, n descending.  kernel(bed, launch, pos_tensor) -> (out [n_heads, hd], extra_bad bool[] or None)
    runs the entry point under test on the patched bed; None: the construction alone (the CPU file).
    Returns the ids of the failing (launch, query head) pairs.  The per-launch verdicts stay on the device as bool tensors and are read back
    once, after the last launch: a read-back per launch would synchronise some 17000 times and take most of the GPU file's runtime."""
    launches = sorted(launches, key=lambda l: -l.n)
    A = torch.tensor([l.a for l in launches], dtype=torch.int64).to(bed.device)
    B = torch.tensor([l.b for l in launches], dtype=torch.int64).to(bed.device)
    N = torch.tensor([[l.n - 1] for l in launches], dtype=torch.int64).to(bed.device)
    flags = []
    for i, l in enumerate(launches):
        assert (l.kind == "flat") == bed.flat and all(0 <= x < l.n for x in l.a + l.b)
        bed.shrink(l.n)
        bed.apply(A[i], B[i])
        extra = None
        if kernel is not None:
            got, extra = kernel(bed, l, N[i])
        ref, _ = bed.reference(l.n)
        f = [closed_form_bad(bed, l.kind, l.n, A[i], B[i], ref)]
        if kernel is not None:
            f.append(kernel_bad(bed, l.kind, got, ref))
            f.append(extra.expand(bed.n_heads) if extra is not None else torch.zeros_like(f[0]))
        flags.append(torch.stack(f))
        bed.restore()
    flags = torch.stack(flags).cpu()             # [launches, checks, n_heads]
    names = ("the fp64 reference misses the closed form", "the kernel misses the fp64 reference", "the rotary form's cache row is not the new key / value")
    bad = []
    for i, c, h in flags.nonzero().tolist():
        bad.append(f"{launches[i].id} head {h}: {names[c]}")
    return bad


def summary(bad, what):
    return f"{what}: {len(bad)} failures, first: " + "; ".join(bad[:6])


def needle_margin(bed: Bed):
    """fp64, over the whole bed: (the needle's score minus the largest background score) per query head at its least"""
    s_bg = torch.matmul(bed.q.double().view(bed.n_kv, -1, bed.hd), bed.kc.double().transpose(1, 2)).amax(-1) * bed.scaling
    s_nd = (bed.q.double().view(bed.n_kv, -1, bed.hd) * bed.patch.double().view(bed.n_kv, 1, bed.hd)).sum(-1) * bed.scaling
    return float((s_nd - s_bg).min())


def off_needle_mass(bed: Bed, n: int, place: int):
    """fp64: the softmax mass the reference leaves off a needle at `place`, the largest over the heads (from the scores, not as 1 - p)"""
    a = torch.full((bed.n_kv,), place, dtype=torch.int64, device=bed.device)
    bed.apply(a, a)
    _, s = bed.reference(n)
    bed.restore()
    s = s - s[:, place:place + 1]
    s[:, place] = -math.inf
    return float(torch.exp(s).sum(-1).max())
