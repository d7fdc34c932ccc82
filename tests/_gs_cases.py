"""Shared by tests/test_group_size_cpu.py and tests/test_group_size_gpu.py: the cases that pin the GENERIC group-size bodies of the fused forward
kernels (every group_size but 64; 8- and 1-bit always), the constructed layers whose output has a closed form, and the host references.

What is pinned is ONE axis: which (zero, scale) a kernel reads for the 16 k-values a lane owns.  The generic bodies compute that index per lane —
gemv_kernel.inc:119-131 (`goff = (k0 / gs) * 2`, `row_off` per slab), gemv_mfma.hip:185 (`g = (kb * 64 + c * 16) / gs`), gemm.hip:116 and :297
(`(k0 + wk * 16) / gs`, `(k0 + c * 16) / gs`) — and the route table of include/hqq_hip.h promises them for every group_size % 16 == 0.

The K and group_size values follow from the kernels' own constants, restated below with their source lines, never from a model's shapes.
Families of cases and the edge each exists for:
  ROWWISE (gemv_kernel.inc, GS64 == false), 8/4/2/1-bit fp16 and 4/2-bit bf16, every M of 1..4:
    gs 16 / 32 / 48     several groups inside one 64-k block, an edge at every residue of the 16-k lane chunk (mod 32, 48)
    gs 48 / 80 / 96     no power of two: the division k0 / gs is a real division, edges drift against the lanes
    gs 128 / 256        the reference's other stock sizes (several lanes, a quarter step)
    gs 1024 / 2048      one group per wave load (GV_KSTEP) / per unit (GV_UNIT): every lane of a load reads the same pair
    gs == K             one group per row (16, 48, 80, 96, 192…; 3088 and 4144 span units): the index is 0 for every lane
    K < GV_KSTEP        lanes past K (K = 16 … 960; K % 64 != 0 at 16, 48, 80, 240, 2064 …): their group index lies past the row
    K == GV_KSTEP       exactly one load, no tail
    GV_UNIT + 16 j      a second unit whose first load is ragged and whose second is dead
    > 2 GV_UNIT + tail  the ring of GV_NF units wraps
    > 3 GV_UNIT         few rows: the workgroup's waves share one row (the K-split of launch_gemv_f16, `nunits >= WPG`)
    N                   one packed row; 7 / 13 packed rows (a ragged workgroup of GV_WAVES rows); 8195 packed rows: a wave takes a second row
  ROWWISE under OPT_FACTORED, 4/2-bit, M in 5, 8, 9, 16 (launches of 8): the randn layer only (its arithmetic is not the exact one)
  MFMA16 (gemv_mfma.hip, GS64 == false), 8/4/2/1-bit fp16, M in 5, 8, 9, 16:
    K = 64              one block; K = 192, 320, 576: an odd number of blocks (a half-dead unit); 35 … 48 blocks: every K slice an uneven share
    gs 48 / 96          K a multiple of 192
    N                   one packed row, 21 and 37 packed rows (ragged 16-row tiles), 65557 packed rows: a workgroup takes a second tile
  GEMM_TILE (gemm.hip), 4/2-bit fp16, M in 17, 100 (a ragged M tile), 129 (one M tile and a row), N one ragged N tile, K one tile and several,
    default / OPT_GEMM_CLASSIC / OPT_GEMM_REGTILE; the register-tile kernel itself only runs from 256 workgroup tiles on (gemm.hip:490), so four
    REGTILE cases have 32644 packed rows
  grouped launches (hqq_hip_gemv_grouped) of three layers of different N, gs 128 and gs 16, on ROWWISE and MFMA16

Constructed layers (closed form in fp64; every weight, product and partial sum a multiple of 2^-q below 2^24 2^-q, so fp32 accumulation is exact
in ANY order and the expected bits need no tolerance):
  scale  levels 1, zero 0, scale[r] = code(r) / 16          -> W[n, k] = code(n G + k // gs) / 16
  zero   levels 0, scale 2^-4, zero[r] = code(r)            -> W[n, k] = -code(n G + k // gs) / 16
  level  zero 0, level (3 n + 5 k) mod 2^nbits, scale 1 — or the power of two 2^-e that keeps the all-ones sum of a long row finite in fp16
code(r) = 1 + (r + 17 layer) mod 61 over the FLAT group index r = n G + g: injective over any 61 consecutive groups (a wrong group of the same
or a neighbouring row) — and, checked by the CPU file for every case, over the same group of the other slab rows a packed row holds.  The codes
are sixteenths so that the all-ones sum of the longest row stays below fp16's largest number.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

# ---- the kernels' constants, restated ------------------------------------------------------------------------------------------------
LANE_K = 16                      # k-values a lane owns per load: 16 packed bytes (gemv_kernel.inc:65 LANE_BYTES; gemv_mfma.hip:22-23; gemm.hip:104)
GV_KSTEP = 1024                  # k per wave load of the row-per-wave kernel (gemv_shared.h:14)
GV_U = 2                         # loads per unit (gemv_shared.h:16, :21)
GV_NF = 2                        # units of the ring (gemv_shared.h:19, :22)
GV_UNIT = GV_KSTEP * GV_U        # k per unit (gemv_shared.h:23)
GV_WAVES = 4                     # rows (waves) per workgroup (gemv_shared.h:8, :13)
GV_EXACT_MAX_M = 4               # gemv_shared.h:26
GM_BLOCK = 64                    # the 64-k block of gemv_mfma.hip (:155 `nb = K >> 6`)
GM_UB = 2                        # blocks per unit (gemv_mfma.hip:40)
GM_ROWS = 16                     # packed rows per tile (gemv_mfma.hip:168)
GB_K = 64                        # K tile of both kernels of gemm.hip (:26)
GB_N = 128                       # output features per tile of the staged kernel (gemm.hip:26); 128 tokens per M tile below 1536 tiles (:493)
RT_ROWS = 128                    # packed rows per tile of the register-tile kernel (gemm.hip:234, :258)
RT_MIN_TILES = 256               # ... which runs from this many workgroup tiles of 256 tokens on (gemm.hip:490)
CUS = 256                        # compute units of an MI355X (the launch rules below only need "at least 16")

PER = {8: 1, 4: 2, 2: 4, 1: 8}
ROUTE_ROWWISE, ROUTE_MFMA16, ROUTE_GEMM_TILE = 1, 5, 8          # include/hqq_hip.h HQQ_ROUTE_*
OPT_FACTORED, OPT_META_SCALABLE, OPT_GEMM_REGTILE, OPT_GEMM_CLASSIC = 1, 2, 16, 32
WANT_ROUTE = {"rowwise": ROUTE_ROWWISE, "mfma16": ROUTE_MFMA16, "gemm_tile": ROUTE_GEMM_TILE}
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f16": 1, "bf16": 2}
P_CODE = 61                      # the prime of code(): 61 / 16 and 61 are exact in bf16 (8 significant bits) and fp16
Q_CODE = 4                       # codes are multiples of 2^-4
KINDS = ("scale", "zero", "level")


def gm_ks(nbits: int, K: int, tiles: int) -> int:
    """K slices (waves) per tile of gemv_mfma.hip (gm_launch, :328-335)"""
    nb = K // GM_BLOCK
    ks = -(-CUS * 8 // tiles)
    ks = min(ks, max(nb // GM_UB, 1))
    return max(1, min(ks, min(32 // PER[nbits], 16)))


def gm_slices(nbits: int, K: int, tiles: int):
    """[kb0, kb1) of every wave, in blocks (gemv_mfma.hip:157-158)"""
    nb, ks = K // GM_BLOCK, gm_ks(nbits, K, tiles)
    return [(nb * w // ks, nb * (w + 1) // ks) for w in range(ks)]


def gm_grid_cap(nbits: int, K: int, tiles: int) -> int:
    """workgroups of a launch at most (gemv_mfma.hip:337-340): beyond it a workgroup takes a second tile"""
    return CUS * max(16 // gm_ks(nbits, K, tiles), 1)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    route: str                # "rowwise" | "mfma16" | "gemm_tile"
    nbits: int
    dt: str                   # "f16" | "bf16"
    opts: int
    M: int
    Ns: tuple
    K: int
    gs: int
    bias: bool = False

    @property
    def grouped(self):
        return len(self.Ns) > 1

    @property
    def G(self):
        return self.K // self.gs

    @property
    def per(self):
        return PER[self.nbits]

    @property
    def factored(self):
        return self.route == "rowwise" and bool(self.opts & OPT_FACTORED)

    @property
    def id(self):
        bits = [self.route, f"{self.nbits}b", self.dt, f"M{self.M}", "N" + "+".join(map(str, self.Ns)), f"K{self.K}", f"gs{self.gs}"]
        for bit, name in ((OPT_FACTORED, "factored"), (OPT_GEMM_REGTILE, "regtile"), (OPT_GEMM_CLASSIC, "classic")):
            if self.opts & bit:
                bits.append(name)
        if self.bias:
            bits.append("bias")
        return "-".join(bits)


# (K, gs) of the row-per-wave kernel: shorter than a load | exactly one | one unit and a ragged tail | more than two units and a tail | the K-split
ROWWISE_KGS = [(16, 16), (48, 16), (48, 48), (80, 80), (96, 32), (96, 48), (96, 96), (240, 16), (240, 48), (240, 80), (256, 128), (256, 256), (480, 96),
               (960, 48), (960, 80), (1024, 16), (1024, 32), (1024, 128), (1024, 256), (1024, 1024),
               (2096, 16), (2080, 32), (2064, 48), (2080, 80), (2112, 96), (2176, 128), (2304, 256), (3072, 1024), (3088, 3088),
               (4144, 16), (4128, 48), (4160, 80), (4128, 96), (4224, 128), (4352, 256), (5120, 1024), (6144, 2048), (4144, 4144),
               (8240, 16), (8240, 80), (8256, 96), (8320, 128)]
ROWWISE_COMBOS = [(8, "f16"), (4, "f16"), (2, "f16"), (1, "f16"), (4, "bf16"), (2, "bf16")]
ROWWISE_ROWS = (1, 7, 13)        # packed rows: N == per; ragged workgroups of GV_WAVES rows
ROWWISE_ROWS_SECOND = 2 * CUS * 4 * GV_WAVES + 3   # more rows than the largest grid has waves (launch_gemv_f16: at most 4 workgroups per CU)
FACTORED_KGS = [(48, 16), (240, 48), (240, 80), (480, 96), (1024, 32), (1024, 1024), (2064, 48), (2176, 128)]

# (K, gs) of the 16-row-tile kernel, K % 64 == 0: one block | an odd number | every slice (16, 8 or 4 waves) an uneven share
MFMA_KGS = [(64, 16), (64, 32), (192, 48), (192, 96), (192, 192), (320, 16), (320, 80), (320, 320), (576, 32), (576, 48), (576, 96), (768, 128), (768, 256),
            (2368, 16), (2368, 32), (2496, 48), (2496, 96), (2240, 80), (2432, 128), (2304, 256), (3072, 1024), (4096, 2048)]
MFMA_MS = (5, 8, 9, 16)
MFMA_ROWS = (1, 21, 37)
MFMA_ROWS_SECOND = CUS * 16 * GM_ROWS + 21          # K = 64: one wave per tile, 16 workgroups per CU

# (K, gs) of the output-tile kernels, K % GB_K == 0: one K tile | several
GEMM_KGS = [(64, 16), (64, 32), (128, 128), (192, 48), (192, 96), (192, 192), (256, 256), (320, 80), (576, 48), (768, 128)]
GEMM_MS = (17, 100, 129)
GEMM_ROWS = 20                                       # packed rows: one ragged N tile of either kernel, N % (4 per) == 0
GEMM_ROWS_REGTILE = (RT_MIN_TILES - 1) * RT_ROWS + 4   # 256 tiles of the register-tile kernel, the last one ragged


def _rowwise_cases():
    out = []
    for c, (nbits, dt) in enumerate(ROWWISE_COMBOS):
        for i, (K, gs) in enumerate(ROWWISE_KGS):
            j = i + c
            out.append(Case("rowwise", nbits, dt, 0, 1 + j % GV_EXACT_MAX_M, (ROWWISE_ROWS[(j // 4 + i) % 3] * PER[nbits],), K, gs, bias=j % 2 == 1))
    # a wave's second row, once per dtype
    out += [Case("rowwise", 4, "f16", 0, 2, (ROWWISE_ROWS_SECOND * 2,), 240, 48, bias=True),
            Case("rowwise", 2, "bf16", 0, 3, (ROWWISE_ROWS_SECOND * 4,), 96, 32)]
    for i, (K, gs) in enumerate(FACTORED_KGS):
        for b, nbits in enumerate((4, 2)):
            out.append(Case("rowwise", nbits, "f16", OPT_FACTORED, MFMA_MS[(i + b) % 4], (ROWWISE_ROWS[(i + b) % 3] * PER[nbits],), K, gs, bias=(i + b) % 2 == 1))
    out += [Case("rowwise", 4, "f16", 0, 3, (14, 2, 26), 2176, 128, bias=True),
            Case("rowwise", 2, "bf16", 0, 4, (28, 4, 52), 2096, 16),
            Case("rowwise", 8, "f16", 0, 1, (7, 13), 240, 16)]
    return out


def _mfma_cases():
    out = []
    for c, nbits in enumerate((8, 4, 2, 1)):
        for i, (K, gs) in enumerate(MFMA_KGS):
            j = i + c
            out.append(Case("mfma16", nbits, "f16", 0, MFMA_MS[j % 4], (MFMA_ROWS[(j // 4 + i) % 3] * PER[nbits],), K, gs, bias=j % 2 == 1))
    out += [Case("mfma16", 4, "f16", 0, 5, (MFMA_ROWS_SECOND * 2,), 64, 16, bias=True),
            Case("mfma16", 4, "f16", 0, 9, (42, 2, 74), 768, 128, bias=True),
            Case("mfma16", 2, "f16", 0, 16, (84, 148, 4), 320, 16),
            Case("mfma16", 1, "f16", 0, 5, (8, 168), 192, 48)]
    return out


def _gemm_cases():
    out = []
    for b, nbits in enumerate((4, 2)):
        for i, (K, gs) in enumerate(GEMM_KGS):
            for v, opts in enumerate((0, OPT_GEMM_REGTILE, OPT_GEMM_CLASSIC)):
                j = i + b + v
                out.append(Case("gemm_tile", nbits, "f16", opts, GEMM_MS[j % 3], (GEMM_ROWS * PER[nbits],), K, gs, bias=j % 2 == 1))
    out += [Case("gemm_tile", 4, "f16", OPT_GEMM_REGTILE, 17, (GEMM_ROWS_REGTILE * 2,), 64, 16, bias=True),
            Case("gemm_tile", 4, "f16", OPT_GEMM_REGTILE, 17, (GEMM_ROWS_REGTILE * 2,), 64, 32),
            Case("gemm_tile", 4, "f16", OPT_GEMM_REGTILE, 17, (GEMM_ROWS_REGTILE * 2,), 192, 48),
            Case("gemm_tile", 2, "f16", OPT_GEMM_REGTILE, 17, (GEMM_ROWS_REGTILE * 4,), 64, 16, bias=True)]
    return out


CASES = _rowwise_cases() + _mfma_cases() + _gemm_cases()
assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}


def reaches_regtile(c: Case) -> bool:
    """the register-tile kernel itself serves the call (gemm.hip:490)"""
    return c.route == "gemm_tile" and bool(c.opts & OPT_GEMM_REGTILE) and -(-c.M // 256) * -(-(c.Ns[0] // c.per) // RT_ROWS) >= RT_MIN_TILES


# ---- rounding to the compute dtype ---------------------------------------------------------------------------------------------------
def _bf16_bits(a32: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(a32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def round_dt(a64: np.ndarray, dt: str) -> np.ndarray:
    """fp64 -> the nearest value of the dtype (ties to even), ONE rounding, returned as fp64.  bf16 goes through float32, which must hold the value
    exactly (the callers' values are short dyadic numbers; the randn path rounds float32 values)."""
    a64 = np.asarray(a64, np.float64)
    if dt == "f16":
        with np.errstate(over="ignore"):
            return a64.astype(np.float16).astype(np.float64)
    a32 = a64.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a64), "bf16 rounding needs a float32-exact value"
    return (_bf16_bits(a32).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def raw(a64: np.ndarray, dt: str) -> np.ndarray:
    """values of the dtype -> what the oracle takes (np.float16 / raw bf16 bits)"""
    if dt == "f16":
        return np.asarray(a64).astype(np.float16)
    return (np.ascontiguousarray(a64, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def tensor(a64: np.ndarray, dt: str) -> torch.Tensor:
    """values of the dtype -> a torch tensor of it (exact)"""
    r = raw(a64, dt)
    return torch.from_numpy(r) if dt == "f16" else torch.from_numpy(r.view(np.int16)).view(torch.bfloat16)


# ---- constructed layers --------------------------------------------------------------------------------------------------------------
def code(r):
    return 1 + np.asarray(r) % P_CODE


def level_shift(c: Case) -> int:
    """e of the level-coded layer's scale 2^-e: 0 (scale 1) unless the all-ones sum of a row, K (2^nbits - 1), would pass 2^15"""
    e = 0
    while c.K * (2 ** c.nbits - 1) >= 2 ** (15 + e):
        e += 1
    return e


def coded_layer(c: Case, kind: str, li: int = 0):
    """layer li of the case: levels U [N G, gs] uint8, scale / zero [N G] and the closed-form weights W [N, K], all fp64 values exact in the dtype;
    q: every weight is a multiple of 2^-q"""
    N, K, gs, G = c.Ns[li], c.K, c.gs, c.G
    R = N * G
    cd = code(np.arange(R, dtype=np.int64) + 17 * li).astype(np.float64)
    if kind == "scale":
        U = np.ones((R, gs), np.uint8)
        scale, zero, q = cd / 2 ** Q_CODE, np.zeros(R), Q_CODE
        W = np.repeat(scale.reshape(N, G), gs, axis=1)
    elif kind == "zero":
        U = np.zeros((R, gs), np.uint8)
        scale, zero, q = np.full(R, 2.0 ** -Q_CODE), cd, Q_CODE
        W = np.repeat(-(cd / 2 ** Q_CODE).reshape(N, G), gs, axis=1)
    else:
        q = level_shift(c)
        n, k = np.arange(N, dtype=np.int64).reshape(N, 1), np.arange(K, dtype=np.int64).reshape(1, K)
        lv = (3 * n + 5 * k) % (2 ** c.nbits)
        U = lv.astype(np.uint8).reshape(R, gs)
        scale, zero = np.full(R, 2.0 ** -q), np.zeros(R)
        W = lv.astype(np.float64) / 2 ** q
    return U, scale, zero, W, q


def coded_bias(c: Case, li: int = 0):
    """quarters in [-3/4, 3/4]: exact in both dtypes"""
    return None if not c.bias else ((np.arange(c.Ns[li]) + li) % 7 - 3) / 4.0


# ---- activations ---------------------------------------------------------------------------------------------------------------------
def edges(c: Case):
    """the k at which a kernel's own structure changes: loads and units of the row-per-wave kernel, the first block of every wave's K slice of
    the 16-row-tile kernel, the K tiles of the output-tile kernels; a case of another table's own route brings its rule along as own_edges()"""
    own = getattr(c, "own_edges", None)
    if own is not None and own() is not None:
        return own()
    if c.route == "rowwise":
        return list(range(GV_KSTEP, c.K, GV_KSTEP))
    if c.route == "mfma16":
        tiles = sum(-(-(N // c.per) // GM_ROWS) for N in c.Ns)
        return [kb0 * GM_BLOCK for kb0, _ in gm_slices(c.nbits, c.K, tiles)[1:]]
    return list(range(GB_K, c.K, GB_K))


def probe_groups(c: Case):
    """every group of a row up to 64 of them; beyond: the first two, the last two and the groups either side of every edge"""
    G = c.G
    if G <= 64:
        return list(range(G))
    g = {0, 1, G - 2, G - 1}
    for e in edges(c):
        g |= {(e - 1) // c.gs, e // c.gs}
    return sorted(g)


def activations(c: Case, family: str) -> np.ndarray:
    """x of one family, [rows, K] of zeros and ones: "onehot" (the first and the last k of every probed group), "group" (ones over exactly one group
    per row), "ones" (one row)"""
    gs = c.gs
    if family == "ones":
        return np.ones((1, c.K))
    groups = probe_groups(c)
    if family == "group":
        X = np.zeros((len(groups), c.K))
        for i, g in enumerate(groups):
            X[i, g * gs:(g + 1) * gs] = 1.0
        return X
    ks = sorted({k for g in groups for k in (g * gs, (g + 1) * gs - 1)})
    X = np.zeros((len(ks), c.K))
    X[np.arange(len(ks)), ks] = 1.0
    return X


FAMILIES = ("onehot", "group", "ones")


def launch_index(c: Case, rows: int) -> np.ndarray:
    """which row of a probe set of `rows` rows every row of its whole launches of M rows is (the last launch is filled from the top)"""
    return np.arange(-(-rows // c.M) * c.M) % rows


def launches(c: Case, X: np.ndarray) -> np.ndarray:
    """the rows of X as whole launches of M rows: [n_launches, M, K] (the last launch is filled from the top)"""
    return np.take(X, launch_index(c, X.shape[0]), axis=0).reshape(-1, c.M, c.K)


def expected(c: Case, W: np.ndarray, X: np.ndarray, bias) -> np.ndarray:
    """the closed form of x @ W^T in fp64, rounded ONCE to the dtype, plus one more rounding for the bias add (include/hqq_hip.h: "fp32 accumulation,
    one rounding to dtype (+ one for the bias add)"); fp64 values of the dtype"""
    y = round_dt(X @ W.T, c.dt)
    return y if bias is None else round_dt(y + np.asarray(bias).reshape(1, -1), c.dt)


def exact_in_fp32(W: np.ndarray, X: np.ndarray, q: int) -> bool:
    """every product x w is a multiple of 2^-q and the absolute sum of a row's products stays below 2^24 2^-q: every partial sum, in any order, is
    such a multiple below that bound — a float32 holds it exactly"""
    Wq = W * 2.0 ** q
    return bool(np.array_equal(Wq, np.rint(Wq)) and np.array_equal(X, np.rint(X)) and (np.abs(X) @ np.abs(Wq).T).max() < 2 ** 24)


# ---- the randn layer -----------------------------------------------------------------------------------------------------------------
def random_layer(c: Case, li: int = 0):
    """_random_layer of tests/test_hip_parity.py (scale in [0.001, 0.005], zero in [0, 2^nbits - 1]), x ~ N(0, 1), a N(0, 1) bias where the case has one"""
    N, K, gs, dt = c.Ns[li], c.K, c.gs, DT[c.dt]
    g = torch.Generator().manual_seed(1000 * c.nbits + K + gs + 7 * li + c.M)
    R = N * K // gs
    U = torch.randint(0, 2 ** c.nbits, (R, gs), generator=g, dtype=torch.uint8)
    s = (torch.rand(R, 1, generator=g) * 0.004 + 0.001).to(dt)
    z = (torch.rand(R, 1, generator=g) * (2 ** c.nbits - 1)).to(dt)
    b = torch.randn(N, generator=g).to(dt) if c.bias else None
    return U, s, z, b


def random_x(c: Case):
    return torch.randn(c.M, c.K, generator=torch.Generator().manual_seed(c.K + c.M)).to(DT[c.dt])


def reference_weights(oracle, c: Case, P, s, z, li: int = 0):
    """Quantizer.dequantize on the host, values of the dtype as float32: the oracle for fp16; for bf16 the two-rounding restatement of
    tests/test_axis0_decode_gpu.py::_ref_weights on the axis-1 layout (float32 carries more than twice bf16's bits: each op rounds once)"""
    N = c.Ns[li]
    if c.dt == "f16":
        return oracle.dequantize(c.nbits, P, s.numpy(), z.numpy(), N, c.K, c.gs, 1).astype(np.float32)
    U = oracle.unpack(c.nbits, P)[:N * c.K // c.gs].astype(np.float32)   # (the slice drops the 3-bit container's padding rows; a no-op at the byte widths)
    s32, z32 = s.float().numpy().reshape(-1, 1), z.float().numpy().reshape(-1, 1)
    rb = lambda a: (_bf16_bits(a).astype(np.uint32) << 16).view(np.float32)   # noqa: E731
    return rb(rb(U - z32) * s32).reshape(N, c.K)


def reference_forward(oracle, c: Case, Wd32, x, b):
    """oracle.matmul: double accumulation, one rounding (+ one for the bias); float32 values of the dtype"""
    f = lambda t: raw(t.float().numpy(), c.dt)   # noqa: E731
    yo, _ = oracle.matmul(f(x), raw(Wd32, c.dt), None if b is None else f(b), CODE[c.dt])
    return yo.astype(np.float32) if c.dt == "f16" else (yo.astype(np.uint32) << 16).view(np.float32)
