"""Shared by tests/test_prefill_attn_cpu.py and tests/test_prefill_attn_gpu.py: the shapes, the tile slicing and the calls for the prompt's causal attention
(csrc/attn_prefill.hip, hqq_hip_attn_prefill / hqq_hip_attn_prefill_kvq; ops.attn_prefill / ops.attn_prefill_kvq): T rows of one sequence at positions
pos0 .. pos0 + T - 1, row t over keys [0, pos0 + t], 16 consecutive rows of a query head per workgroup.

Nothing is derived here.  A prompt is a stack of _tile_cases' tiles: tile j of a case is the _tile_cases.Case with pos = (pos0 + 16 j, ...) and S = 1, and the
expected values, the band (c_acc(n_max, 1), n_max the TILE's) and the verdict are _tile_cases' reference_rows / band on that tile's view of the tensors.  K and V
are _tile_cases.build's (randn, `fill` from pos0 + T on); the queries are randn at the scale _tile_cases uses for the head size (a quarter at hd = 256, where
delta alone would break the band condition).  The cache is never longer than 512 positions.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

import _tile_cases as tc
from _tile_cases import CODE, DT, DTS, HDS, bits  # noqa: F401

TILE = tc.MAX_ROWS           # rows of a query tile
HEADS = tc.RANDOM_HEADS      # (4, 4) and (8, 2)
SWEEP_T = (1, 15, 16, 17, 31, 32, 33, 49)     # tile edges, 32-key block edges (with the pos0 below), a padded last tile
SWEEP_P0 = (0, 5, 16, 37)
SWEEP_L = 128
LONG_T, LONG_L = 273, 320    # 273 keys: 9 blocks of 32, so wave 0 of the last tiles gets two
FULL = (47, 49, 96)          # (pos0, T, L): pos0 + T == L
DEEP = (239, 273, 512)       # (pos0, T, L): up to 512 keys, 16 blocks — every one of the 8 waves gets two — and again pos0 + T == L


@dataclass(frozen=True)
class Case:
    dt: str
    hd: int
    L: int
    heads: tuple
    pos0: int
    T: int
    seed: int = 0

    @property
    def id(self):
        return f"{self.dt}-hd{self.hd}-h{self.heads[0]}.{self.heads[1]}-L{self.L}-p{self.pos0}-T{self.T}"

    @property
    def n(self):
        """1 + the last position of the prompt: nothing from here on may be read"""
        return self.pos0 + self.T

    @property
    def qscale(self):
        return 0.25 if self.hd == 256 else 1.0


def cases(dt: str, hd: int):
    """the whole cross product of the sweep for both head layouts, the long prompt, the prompt that fills its cache and the deep one"""
    out, seed = [], 0
    for heads in HEADS:
        for T in SWEEP_T:
            for p0 in SWEEP_P0:
                out.append(Case(dt, hd, SWEEP_L, heads, p0, T, seed))
                seed += 1
        out.append(Case(dt, hd, LONG_L, heads, 0, LONG_T, seed))
        out.append(Case(dt, hd, FULL[2], heads, FULL[0], FULL[1], seed + 1))
        out.append(Case(dt, hd, DEEP[2], heads, DEEP[0], DEEP[1], seed + 2))
        seed += 3
    return out


def tiles(case: Case):
    """[(j, the positions of tile j's rows)]"""
    return [(j, tuple(range(case.pos0 + TILE * j, case.pos0 + min(TILE * j + TILE, case.T)))) for j in range(-(-case.T // TILE))]


def build(case: Case, device, fill=float("nan")):
    """-> dict q [T, n_heads, hd] (dense), K, V [n_kv, L, hd] of the case's dtype (rows from pos0 + T on hold `fill`), pos int64 [T]"""
    device = str(device)
    kv = tc.build(tc.Case("random", case.dt, case.hd, case.L, (case.n - 1,), 1, heads=case.heads, seed=case.seed), device, fill)
    g = torch.Generator(device=device).manual_seed(977 * case.seed + 13)
    q = (torch.randn(case.T, case.heads[0], case.hd, device=device, generator=g) * case.qscale).to(DT[case.dt])
    return {"case": case, "q": q, "K": kv["K"], "V": kv["V"], "pos": torch.arange(case.pos0, case.n, dtype=torch.int64, device=device)}


def tile_view(t, j: int, pos):
    """tile j as _tile_cases sees a verify step: its Case (S = 1) and the tile's rows of q as [r, n_heads * hd] against the same K and V"""
    case = t["case"]
    r0 = TILE * j
    q = t["q"][r0:r0 + len(pos)].reshape(len(pos), -1).contiguous()
    return {"case": tc.Case("random", case.dt, case.hd, case.L, tuple(pos), 1, heads=case.heads, seed=case.seed, qscale=case.qscale), "q": q, "K": t["K"], "V": t["V"],
            "pos": torch.tensor(pos, dtype=torch.int64, device=q.device)}


def reference(t):
    """fp64 attention of all T rows at once: [T, n_heads, hd] (computed once per case; the tiles slice it)"""
    case = t["case"]
    return tc.reference_rows(t["q"].reshape(case.T, -1), t["K"], t["V"], t["pos"], case.hd ** -0.5)[0]


def outside_band(t, got, ref):
    """[T, n_heads] bool: tile by tile, is `got` [T, n_heads, hd] outside _tile_cases.band (c_acc(n_max of the tile, 1)) around ref?  (A NaN compares false: outside.)"""
    case = t["case"]
    bad = torch.ones(case.T, case.heads[0], dtype=torch.bool, device=got.device)
    for j, pos in tiles(case):
        rows = slice(TILE * j, TILE * j + len(pos))
        tol = tc.band(tile_view(t, j, pos), ref[rows], case.hd ** -0.5)[0]
        bad[rows] = ~((got[rows].double() - ref[rows]).abs() <= tol).all(-1)
    return bad


# ---- the calls ---------------------------------------------------------------------------------------------------------------------------------------------
def prefill(t, q=None, K=None, V=None):
    from hqq_amd import ops
    case = t["case"]
    out = torch.full((case.T, case.heads[0], case.hd), float("nan"), dtype=DT[case.dt], device=t["q"].device)
    return ops.attn_prefill(t["q"] if q is None else q, t["K"] if K is None else K, t["V"] if V is None else V, case.pos0, out=out, scaling=case.hd ** -0.5)


def tiled(t, j: int, pos):
    """ops.attn_decode_tiled on tile j's queries with their positions and splits = 1: [r, n_heads, hd]"""
    from hqq_amd import ops
    v = tile_view(t, j, pos)
    out = torch.full_like(v["q"], float("nan"))
    return ops.attn_decode_tiled(v["q"], v["K"], v["V"], v["pos"], out, t["case"].hd ** -0.5, splits=1).view(len(pos), t["case"].heads[0], t["case"].hd)


def quantised(t, nbits: int, gs: int, beyond: str = "zero"):
    """the six buffers [1, n_kv, L, .] holding positions [0, pos0 + T) of K and V quantised (ops.kv_quantize); from pos0 + T on zeros, or (beyond = "nan") NaN
    scales and zeros over levels of 0xFF"""
    from hqq_amd import ops
    case = t["case"]
    K, V = t["K"], t["V"]
    bufs = ops.kv_alloc(1, K.shape[0], case.L, case.hd, nbits, gs, K.dtype, K.device)
    ops.kv_quantize(K[None, :, :case.n], V[None, :, :case.n], bufs, 0)
    if beyond == "nan":
        for b in bufs:
            b[:, :, case.n:] = 0xFF if b.dtype == torch.uint8 else float("nan")
    return bufs


def prefill_kvq(t, bufs, q=None):
    from hqq_amd import ops
    case = t["case"]
    out = torch.full((case.T, case.heads[0], case.hd), float("nan"), dtype=DT[case.dt], device=t["q"].device)
    return ops.attn_prefill_kvq(t["q"] if q is None else q, bufs, case.pos0, case.hd, out=out, scaling=case.hd ** -0.5)


def call(lib, t, out, pos0=None, T=None, L=None, qrs=None, qhs=None, q_ptr=None, hd=None, n_kv=None) -> int:
    """the raw C-ABI call of the dense entry (argument checks)"""
    case = t["case"]
    q = t["q"]
    return lib.hqq_hip_attn_prefill(q.data_ptr() if q_ptr is None else q_ptr, q.stride(0) if qrs is None else qrs, q.stride(1) if qhs is None else qhs,
                                    t["K"].data_ptr(), t["V"].data_ptr(), case.pos0 if pos0 is None else pos0, case.T if T is None else T, out.data_ptr(),
                                    case.heads[0], case.heads[1] if n_kv is None else n_kv, case.hd if hd is None else hd, case.L if L is None else L,
                                    case.hd ** -0.5, CODE[case.dt], torch.cuda.current_stream().cuda_stream)


def call_kvq(lib, t, bufs, nbits, gs, out, pos0=None, T=None, qrs=None) -> int:
    case = t["case"]
    q = t["q"]
    return lib.hqq_hip_attn_prefill_kvq(nbits, q.data_ptr(), q.stride(0) if qrs is None else qrs, q.stride(1), *(b.data_ptr() for b in bufs),
                                        case.pos0 if pos0 is None else pos0, case.T if T is None else T, out.data_ptr(), case.heads[0], case.heads[1], case.hd, gs,
                                        case.L, case.hd ** -0.5, CODE[case.dt], torch.cuda.current_stream().cuda_stream)
