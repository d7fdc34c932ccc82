"""Cases, host model and error bound of the routed expert kernel's tests (csrc/moe.hip; tests/test_moe_cpu.py, tests/test_moe_gpu.py).

Host model.  `model()` restates the fused arithmetic of include/hqq_hip.h (hqq_hip_moe_*) with every dot product taken in fp64 and every rounding the
kernel makes, T the compute dtype, rnd = round to T:
    g = rnd(x . Wg_e), u = rnd(x . Wu_e);  a = rnd(rnd(silu32(g)) * u);  d = rnd(a . Wd_e)
    out[t]: acc = 0; for the token's slots in ascending (expert id, slot): acc = rnd(acc + rnd(fp32(d) * w[t, s]))
Where the dot products are exact in fp32 (the closed-form cases) the kernel must return these bits; elsewhere it may differ by what fp32 accumulation
costs, which `bound()` derives.

Closed-form cases.  x in {-1, 0, 1}; gate / up weights (q - z) * s with integer zero-points and power-of-two scales, so that every term of x . W is a
multiple of s below 2^24 s in sum: exact in fp32 in any order.  a = silu(g) * u is an arbitrary number of T, so the down weights have ONE non-zero
level difference per output row (q = z elsewhere; its column moves with the row over every group and slab): a[j] * (q - z) * s has at most 11 + 4 bits —
the "sum" is one exact term.

Bound for random inputs (derived here, not fitted to a kernel's output).  u = 2^-24, eps = unit roundoff of T (2^-11 fp16, 2^-8 bf16), eta = half the
subnormal spacing of T (2^-25 fp16; 0 for bf16, whose subnormals lie below anything these cases reach).
  (1) An fp32 sum of K products, each product exact (two numbers of T multiply exactly in fp32, and fma(x, w, acc) then rounds once like an add), taken in
      ANY order, is within gamma_K * sum |x_k w_k| of the exact sum, gamma_K = K u / (1 - K u)  (Higham, Accuracy and Stability, section 3.1).
  (2) If |p - q| <= r and q is the model's pre-rounding value, |rnd(p) - rnd(q)| <= r + eps (|p| + |q|) + 2 eta <= r + eps (2 |q| + r) + 2 eta =: R(|q|, r).
  (3) silu(x) = x sigmoid(x) has |silu'| <= 1.1 everywhere; its fp32 evaluation (expf, one add, one division) is within 8 u |silu| of the true value on
      either side (a few ulp each for expf and the division; 8 is generous and still 2^13 times below eps).
Propagation, with D. the radius of the kernel's value around the model's:
      Dg = R(|g64|, gamma_H sum|x Wg|), Du alike;  Ds = R(|silu(g)|, 1.1 Dg + 8 u |silu(g)|)
      Da = R(|s u|, |s| Du + |u| Ds + Ds Du)
      Dd = R(|d64|, sum_j Da_j |Wd_nj| + gamma_I sum_j (|a_j| + Da_j) |Wd_nj|)         (Da = 0 when the model is fed the kernel's own a)
      Dp = R(|d w|, |w| Dd + u |d w|)                                                    (the fp32 product d * w rounds once in fp32)
      Dacc_i = R(|acc_{i-1} + p_i|, Dacc_{i-1} + Dp_i)
The composed route (per-expert kernels that accumulate in fp32, torch's elementwise ops) has the same structure: the same bound holds for it.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

U32 = 2.0 ** -24
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
ETA = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
ROLES = ("gate", "up", "down")


@dataclass(frozen=True)
class Case:
    kind: str        # "closed" | "random"
    nbits: int
    gs: int
    dt: torch.dtype
    T: int
    k: int
    E: int = 4
    H: int = 128
    I: int = 192
    seed: int = 0

    @property
    def id(self):
        return f"{self.kind}-int{self.nbits}g{self.gs}-{'bf16' if self.dt == torch.bfloat16 else 'fp16'}-T{self.T}-k{self.k}-E{self.E}"


CONFIGS = ((4, 64), (2, 16))
DTYPES = (torch.float16, torch.bfloat16)


def _cases(kind):
    out = [Case(kind, nb, gs, dt, T, k, seed=7 + 13 * i) for i, (nb, gs, dt, T, k) in enumerate(
        (nb, gs, dt, T, k) for nb, gs in CONFIGS for dt in DTYPES for T in (1, 3, 16) for k in (1, 2))]
    out.append(Case(kind, 4, 64, torch.float16, 2, 8, E=8, seed=5))   # every expert hit
    return out


CLOSED, RANDOM = _cases("closed"), _cases("random")
BY_ID = {c.id: c for c in CLOSED + RANDOM}


# ---- packing and dequantising on the host (the BitPack layout: slab 0 most significant) ---------------------------------------------------------------
def pack(levels: torch.Tensor, nbits: int) -> torch.Tensor:
    """[R, gs] integer levels -> [R / per, gs] uint8"""
    per = 8 // nbits
    step = levels.shape[0] // per
    out = torch.zeros((step, levels.shape[1]), dtype=torch.int32)
    for s in range(per):
        out |= levels[s * step:(s + 1) * step].to(torch.int32) << (nbits * (per - 1 - s))
    return out.to(torch.uint8)


def dequant(levels: torch.Tensor, scale: torch.Tensor, zero: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Quantizer.dequantize on levels [R, gs] with scale / zero [R, 1] of T: two roundings in T"""
    return ((levels.to(scale.dtype) - zero) * scale).reshape(N, K)


def routing(case: Case, g: torch.Generator):
    idx = torch.stack([torch.randperm(case.E, generator=g)[:case.k] for _ in range(case.T)]).to(torch.int64)
    if case.k == case.E:
        idx[0] = torch.arange(case.E - 1, -1, -1)                  # every expert, descending
    elif case.k >= 2:
        idx[0, :2] = torch.tensor([case.E - 1, 0])                  # a token whose slots are in descending expert order
        if case.T >= 3:
            idx[2, :2] = torch.tensor([1, 1])                       # the same expert twice: ties go by ascending slot
    w = torch.rand((case.T, case.k), generator=g, dtype=torch.float32) + 0.25
    w = w / w.sum(-1, keepdim=True)
    return idx, w


def build(case: Case):
    """-> dict: x [T, H] of T, idx, w, levels / scale / zero per role ([E, R, gs] uint8, [E, R, 1] of T), W per role ([E, N, K] of T, dequantised)"""
    g = torch.Generator().manual_seed(case.seed)
    E, H, I, gs, dt = case.E, case.H, case.I, case.gs, case.dt
    maxv = 2 ** case.nbits - 1
    shapes = {"gate": (I, H), "up": (I, H), "down": (H, I)}
    out = {"case": case}
    if case.kind == "closed":
        out["x"] = torch.randint(-1, 2, (case.T, H), generator=g).to(dt)
    else:
        out["x"] = (torch.randn((case.T, H), generator=g) * 0.5).to(dt)
    out["idx"], out["w"] = routing(case, g)
    if case.kind == "closed":
        out["w"] = (torch.randint(1, 8, (case.T, case.k), generator=g).float() / 8.0)   # three bits: d * w stays an exact fp32 product either way
    for role in ROLES:
        N, K = shapes[role]
        R = N * K // gs
        q = torch.randint(0, maxv + 1, (E, R, gs), generator=g).to(torch.uint8)
        if case.kind == "closed":
            z = torch.randint(maxv // 2, maxv // 2 + 2, (E, R, 1), generator=g).to(dt)
            s = torch.where(torch.randint(0, 2, (E, R, 1), generator=g) == 0, 2.0 ** -5, 2.0 ** -6).to(dt)
            if role == "down":   # one non-zero level difference per output row
                q = z.to(torch.uint8).expand(E, R, gs).clone().reshape(E, N, K)
                for e in range(E):
                    rows = torch.arange(N)
                    cols = (rows * 37 + 11 * e + 5) % K
                    zz = q[e, rows, cols].to(torch.int32)
                    delta = torch.randint(1, maxv // 2 + 1, (N,), generator=g, dtype=torch.int32) * (torch.randint(0, 2, (N,), generator=g, dtype=torch.int32) * 2 - 1)
                    q[e, rows, cols] = (zz + delta).clamp(0, maxv).to(torch.uint8)
                q = q.reshape(E, R, gs)
        else:
            z = (maxv / 2 + 0.5 * torch.randn((E, R, 1), generator=g)).to(dt)
            s = (0.02 * (1.0 + 0.5 * torch.rand((E, R, 1), generator=g))).to(dt)
        out[role] = {"levels": q, "scale": s, "zero": z, "W": torch.stack([dequant(q[e], s[e], z[e], N, K) for e in range(E)])}
    return out


def stacks(data):
    """{(role, kind): tensor [E, ...]} for HQQExperts.from_stacks, and the per-role meta"""
    c = data["case"]
    st, meta = {}, {}
    shapes = {"gate": (c.I, c.H), "up": (c.I, c.H), "down": (c.H, c.I)}
    for role in ROLES:
        d = data[role]
        st[role, "W_q"] = torch.stack([pack(d["levels"][e], c.nbits) for e in range(c.E)])
        st[role, "scale"], st[role, "zero"] = d["scale"].clone(), d["zero"].clone()
        meta[role] = {"nbits": c.nbits, "group_size": c.gs, "shape": torch.Size(shapes[role]), "axis": 1, "packing": f"{c.nbits}bit_u8",
                      "unpack_view_dtype": torch.uint8, "view_as_float": False}
    return st, meta


def quant_config(case: Case):
    from hqq_amd.core.quantize import BaseQuantizeConfig
    return BaseQuantizeConfig(nbits=case.nbits, group_size=case.gs, axis=1)


def experts(data, device="cpu"):
    from hqq_amd.core.moe import HQQExperts
    st, meta = stacks(data)
    return HQQExperts.from_stacks(st, meta, quant_config(data["case"]), compute_dtype=data["case"].dt, device=device)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------
def slot_order(idx_row):
    """the order in which a token's slots are combined: ascending (expert id, slot)"""
    return sorted(range(len(idx_row)), key=lambda s: (int(idx_row[s]), s))


def _silu(g: torch.Tensor) -> torch.Tensor:
    """rnd(silu32(g)): torch's SiLU on a tensor of T computes x / (1 + exp(-x)) in fp32 and rounds once"""
    return torch.nn.functional.silu(g.float()).to(g.dtype)


def model_a(data, dot=None):
    """a [T, k, I] of T.  dot(x [K], W [N, K]) -> the pre-rounding sums (default: fp64)"""
    dot = dot or (lambda x, W: W.double() @ x.double())
    c = data["case"]
    a = torch.zeros((c.T, c.k, c.I), dtype=c.dt)
    for t in range(c.T):
        for s in range(c.k):
            e = int(data["idx"][t, s])
            g = dot(data["x"][t], data["gate"]["W"][e]).to(c.dt)
            u = dot(data["x"][t], data["up"]["W"][e]).to(c.dt)
            a[t, s] = _silu(g) * u
    return a


def model_down(data, a, dot=None, idx=None, w=None):
    """out [T, H] of T from a [T, k, I]"""
    dot = dot or (lambda x, W: W.double() @ x.double())
    c = data["case"]
    idx = data["idx"] if idx is None else idx
    w = data["w"] if w is None else w
    out = torch.zeros((c.T, c.H), dtype=c.dt)
    for t in range(c.T):
        for s in slot_order(idx[t]):
            d = dot(a[t, s], data["down"]["W"][int(idx[t, s])]).to(c.dt)
            p = (d.float() * w[t, s]).to(c.dt)          # an fp32 product, rounded to T
            out[t] = out[t] + p                          # an add in T
    return out


def model(data, dot=None):
    a = model_a(data, dot)
    return a, model_down(data, a, dot)


def fp32_dot(perm_seed: int):
    """dot products the way SOME fp32 kernel takes them: exact products, a sequential fp32 sum in a random order"""
    import numpy as np

    def dot(x, W):
        p = (W.float() * x.float()).numpy()             # exact in fp32: two numbers of T
        order = np.random.default_rng(perm_seed + W.shape[1]).permutation(W.shape[1])
        return torch.from_numpy(np.cumsum(p[:, order], axis=1, dtype=np.float32)[:, -1].copy())
    return dot


# ---- the bound ------------------------------------------------------------------------------------------------------------------------------------------
def _gamma(K):
    return K * U32 / (1.0 - K * U32)


def _R(q_abs, r, dt):
    return r + EPS[dt] * (2.0 * q_abs + r) + 2.0 * ETA[dt]


def bound_a(data):
    """Da [T, k, I] (fp64): the radius of a kernel's a around model_a's"""
    c = data["case"]
    Da = torch.zeros((c.T, c.k, c.I), dtype=torch.float64)
    for t in range(c.T):
        x = data["x"][t].double()
        for s in range(c.k):
            e = int(data["idx"][t, s])
            Wg, Wu = data["gate"]["W"][e].double(), data["up"]["W"][e].double()
            g64, u64 = Wg @ x, Wu @ x
            Dg = _R(g64.abs(), _gamma(c.H) * (Wg.abs() @ x.abs()), c.dt)
            Du = _R(u64.abs(), _gamma(c.H) * (Wu.abs() @ x.abs()), c.dt)
            gm, um = g64.to(c.dt), u64.to(c.dt)
            sil = torch.nn.functional.silu(gm.double()).abs()
            Ds = _R(sil, 1.1 * Dg + 8 * U32 * sil, c.dt)
            sm = _silu(gm).double().abs()
            Da[t, s] = _R(sm * um.double().abs(), sm * Du + um.double().abs() * Ds + Ds * Du, c.dt)
    return Da


def bound_out(data, a, Da=None):
    """Dout [T, H] (fp64): the radius of a kernel's output around model_down(a)'s; Da = None: the kernel was fed this very a"""
    c = data["case"]
    out = torch.zeros((c.T, c.H), dtype=torch.float64)
    for t in range(c.T):
        acc = torch.zeros(c.H, dtype=c.dt)
        Dacc = torch.zeros(c.H, dtype=torch.float64)
        for s in slot_order(data["idx"][t]):
            Wd = data["down"]["W"][int(data["idx"][t, s])].double()
            av = a[t, s].double()
            da = torch.zeros_like(av) if Da is None else Da[t, s]
            d64 = Wd @ av
            Dd = _R(d64.abs(), Wd.abs() @ da + _gamma(c.I) * (Wd.abs() @ (av.abs() + da)), c.dt)
            d = d64.to(c.dt)
            w = float(data["w"][t, s])
            dw = (d.double() * w).abs()
            Dp = _R(dw, abs(w) * Dd + U32 * dw, c.dt)
            p = (d.float() * data["w"][t, s]).to(c.dt)
            Dacc = _R((acc.double() + p.double()).abs(), Dacc + Dp, c.dt)
            acc = acc + p
        out[t] = Dacc
    return out
