"""Shared by tests/test_gs64_cpu.py and tests/test_gs64_gpu.py: the cases that pin the group_size = 64 bodies of the fused forward kernels — the
production setting, which tests/_gs_cases.py ("every group_size but 64") leaves out.  The instrument is that file's: constructed layers whose
output has a closed form that fp32 accumulation reproduces exactly in any summation order (coded_layer, kinds scale / zero / level), probed with
one-hot rows, one-group indicators and all ones placed at the k where each kernel's structure changes.  Everything is imported from there, with gs = 64.

What is pinned is which (zero, scale) pair meets which 64 k-values where a kernel does its own arithmetic.  The K, N and M values follow from the
kernels' constants, restated below with their source lines.  Routes (include/hqq_hip.h HQQ_ROUTE_*) and the edge each family reaches:

  ROWWISE       gemv_kernel.inc GS64 body via gemv.hip:111-172; 4/2-bit fp16 and bf16 take it (MZ slab-pair load, gemv_kernel.inc:86, :100-110);
                8- and 1-bit are dispatched to the GENERIC body even at gs 64 (gemv.hip:209, :212) and are pinned on the same K values.
                K 64 (one group, 31 of 32 meta lanes dead) | 960 (< one wave load) | 1024 (one load) | 1088 (second load holds one group) |
                2048 (one unit = 32 groups: a full MZ pair load) | 2112 (second unit whose meta lanes run past the row's end) | 4096 (nsteps == WPG:
                not xp2) | 4160 (xp2, gemv.hip:130; three units: the ring of GV_NF = 2 wraps) | 6208 (four units: ksplit with few rows, the ring wraps twice with 1027 packed rows) | 8256 (ksplit, 5 units)
                packed rows 1 / 7 / 13; 8195 (a wave's second row); 1027 packed rows, M = 1, 4-bit fp16, K 2112: the 8-wave grid (gemv.hip:114-118)
                FACTORED (M 5, 8, 9, 16; GS64 && !EXACT: the non-MZ GS64 branch, gemv_kernel.inc:111-118): the randn layer only
  ROWWISE_W3S   gemv_w3s.hip (the same kernel text, NBITS = 3, PER = 2, MZ): fp16 and bf16, the same K edges (xp2 in both dtypes, gemv_w3s.hip:64)
  GEMV3_ROWS    gemv3.hip: K 64 (G = 1) | 128 | 1024 (one unit = 16 groups) | 1088 | 4160; N so that N G % 10 != 0, step % G != 0, a row straddles a
                slab boundary and (where G allows it: G = 1, 2, 16) another row starts exactly on one
  GEMV3_SLABS   gemv3s.hip forced with OPT_GEMV3_SLABS: K 1024 (G = 16 = S3_ROWS: a row change in every task) | 1088 | 2112; N so that step % 16 != 0
                (a ragged last task), N G % 10 != 0, step % G != 0 (a slab starts mid-row); the same layers through OPT_GEMV3_ROWWISE give the same bits
  MFMA16        gemv_mfma.hip GS64 body (4/2-bit, gemv_mfma.hip:171-179; 8/1-bit: the generic body, :349, :352): K 64 | 192 | 320 (odd block count) |
                2240 / 2368 / 2496 (35 / 37 / 39 blocks: every K slice an uneven share); packed rows 1 / 21 / 37; 65557 (a workgroup's second tile)
  SKINNY        skinny.hip: 8/4/2-bit and the 3-bit stream layout, fp16 / bf16; M 5, 16, 17, 33, 48, 64 (mt 1..4); K 512 (two chunks) | 768 (odd chunk count
                against a ring of 2) | 1280 | 4096 (16 chunks = SK_MAX_CPS) | 4352 (17: the cap forces a second split); packed rows 1 / 31 / 33 / 65;
                narrow tile by the shape rule and OPT_SKINNY_WIDE; the plan's own split, OPT_SKINNY_KS(2), (chunks / 2) and (1)
  GEMM_PIPE     gemm_pipe.hip: 8/4/2-bit and the stream layout, fp16 / bf16; M 65, 128, 129, 257; K 128 | 384 | 640 | 2048; tiles forced narrow, wide
                and 256-token (not at 2 bits); OPT_SKINNY_KS 2 and 3 on the short K; packed rows 4 / 60 / 68 / 132; one hybrid plan (HYBRID below)
  GEMM_TILE     gemm.hip GS64: 4/2-bit fp16; M 17, 100, 129; K 64 | 192 | 576; default, OPT_GEMM_CLASSIC, OPT_GEMM_REGTILE (one case reaches the kernel)
  grouped launches of three layers of different N on every decode route and on GEMM_PIPE

3-bit layers: levels U [N G, 64] packed by oracle.pack(3, U) into the reference container int32 [ceil(N G / 10), 64] (BitPack.pack_3bit_32); the
stream layout is oracle.w3s_pack_np of that container, made on the host — the device pack kernel is not trusted here.  The level kind is
(3 n + 5 k) mod 8 (coded_layer's rule at nbits = 3).

group_index() below restates, per route, which flat meta index r a kernel pairs with (output row n, 64-k group g) and which container word its
levels come from; tests/test_gs64_cpu.py shows that it reproduces the closed-form W for every case and that each MUTANT of it is caught.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

import _gs_cases as gc
from _gs_cases import CUS, GV_EXACT_MAX_M, GV_KSTEP, GV_NF, GV_U, GV_UNIT, GV_WAVES, GM_BLOCK, GM_ROWS, GB_K, RT_MIN_TILES, RT_ROWS

GS = 64
# ---- the kernels' constants, restated ------------------------------------------------------------------------------------------------
GV_UNIT_GROUPS = GV_UNIT // GS       # 32 groups per unit: `GV_KSTEP * U / 64` (gemv_kernel.inc:84, :86, :107)
GV_WG_PER_CU = 4                     # gemv_shared.h:10-11
G3_UNIT_GROUPS = 16                  # gemv3.hip:35 (G3_U = 4 loads of four groups), :126 `nunits = (G + 15) >> 4`
S3_ROWS = 16                         # packed rows per task (gemv3s.hip:34)
G3S_MIN_BYTES = 19 << 20             # packed bytes from which GEMV3_SLABS serves unforced (gemv3.hip:319)
SK_KC, SK_BLK, SK_MAX_CPS = 256, 4, 16   # skinny.hip:82, :83, :93
SK_ROWS = {"wide": 64, "narrow": 32}     # packed rows per panel: 16 SK_RG (skinny.hip:60, :76, :81)
SK_BPW = {"wide": 2, "narrow": 1}        # blocks per wave and chunk: SK_BLK / SK_SPLIT (skinny.hip:63, :73, :85)
SK_NARROW_MAX_PROWS = 2048           # skinny.hip:773-781 (x 4 at 2 bits; never at 8 bits, never under OPT_SKINNY_WIDE)
WS_COUNTER_BYTES = 256 << 10         # hqq_common.h:163
GD_K = 64                            # k per step of gemm_pipe.hip (:36)

PER = {8: 1, 4: 2, 2: 4, 1: 8}
(ROUTE_ROWWISE, ROUTE_ROWWISE_W3S, ROUTE_GEMV3_ROWS, ROUTE_GEMV3_SLABS, ROUTE_MFMA16, ROUTE_SKINNY, ROUTE_GEMM_PIPE, ROUTE_GEMM_TILE) = range(1, 9)
WANT_ROUTE = {"rowwise": 1, "rowwise_w3s": 2, "gemv3_rows": 3, "gemv3_slabs": 4, "mfma16": 5, "skinny": 6, "gemm_pipe": 7, "gemm_tile": 8}
GEMM_ROUTES = ("gemm_pipe", "gemm_tile")             # served by hqq_hip_gemm; the others by hqq_hip_gemv (include/hqq_hip.h:104)
ROW_PER_WAVE = ("rowwise", "rowwise_w3s", "gemv3_rows")
OPT_FACTORED, OPT_META_SCALABLE, OPT_GEMV3_ROWWISE, OPT_GEMV3_SLABS, OPT_GEMM_REGTILE, OPT_GEMM_CLASSIC = 1, 2, 4, 8, 16, 32
OPT_GEMM_NARROW, OPT_GEMM_WIDE, OPT_GEMM_NOHYBRID, OPT_SKINNY_WIDE, OPT_W3S = 64, 128, 256, 512, 1024


def OPT_KS(n: int) -> int:
    return int(n) << 24


@dataclass(frozen=True)
class Case64(gc.Case):
    layout: str = "u8"           # "u8": the byte containers | "c3": the reference's 3-bit container | "w3s": the 3-bit stream layout
    variants: tuple = (0,)       # option bits OR-ed onto opts, one run each: every one must give the closed form's bits
    note: str = ""               # the variant the case claims to reach (proved by tests/test_gs64_cpu.py)

    @property
    def per(self):
        return {"u8": PER.get(self.nbits), "c3": 10, "w3s": 2}[self.layout]

    def own_edges(self):
        """the k at which the structure of a route that _gs_cases.edges() does not know changes (None: its rule holds)"""
        step = {"rowwise_w3s": GV_KSTEP,               # loads and units of the row-per-wave kernel, as "rowwise"
                "gemv3_rows": G3_UNIT_GROUPS * GS,     # units of 16 groups
                "gemv3_slabs": S3_ROWS * GS,           # a task's 16 packed rows = 16 groups of a row
                "skinny": SK_KC,                       # chunks; every split edge (a multiple of cps chunks) is one of them
                "gemm_pipe": GD_K}.get(self.route)     # steps; every split edge (a multiple of kps steps) is one of them
        return None if step is None else list(range(step, self.K, step))

    @property
    def base_opts(self):
        return self.opts | (OPT_W3S if self.layout == "w3s" else 0)

    @property
    def id(self):
        bits = [self.route, f"{self.nbits}b" + ("" if self.layout == "u8" else self.layout), self.dt, f"M{self.M}", "N" + "+".join(map(str, self.Ns)), f"K{self.K}"]
        for bit, name in ((OPT_FACTORED, "factored"), (OPT_GEMM_REGTILE, "regtile"), (OPT_GEMM_CLASSIC, "classic"), (OPT_GEMV3_SLABS, "slabs")):
            if self.opts & bit:
                bits.append(name)
        if self.bias:
            bits.append("bias")
        if self.note:
            bits.append(self.note)
        return "-".join(bits)


def C(route, nbits, dt, M, Ns, K, opts=0, bias=False, layout="u8", variants=(0,), note=""):
    return Case64(route, nbits, dt, opts, M, tuple(Ns), K, GS, bias, layout, tuple(variants), note)


# ---- launch rules, restated ----------------------------------------------------------------------------------------------------------
def gv_launch(c, M=None):
    """launch_gemv_f16 (gemv.hip:111-172) / launch_w3s (gemv_w3s.hip:48-100) on a 256-CU device: waves per workgroup, xp2, ksplit and whether a
    wave takes a second row (the grid holds at most CUS * WG_PER_CU workgroups; registers can only lower that)"""
    M = c.M if M is None else M
    prow = sum(N // c.per for N in c.Ns)
    f16_exact = c.dt == "f16" and not c.factored
    eight_ok = (c.layout == "w3s" and c.dt == "f16") or (c.layout == "u8" and f16_exact and c.nbits in (4, 2))   # GS64 && EXACT && !BF16 (gemv.hip:114; 8-bit is compiled GS64 = false); gemv_w3s.hip:51
    wpg = GV_WAVES
    if eight_ok and M == 1 and len(c.Ns) == 1 and prow <= CUS * 8 and prow * 2 > CUS * 8 and c.K >= GV_UNIT:
        wpg = 8
    wg_per_cu = GV_WG_PER_CU * GV_WAVES // wpg
    nsteps = -(-c.K // GV_KSTEP)
    nunits = -(-nsteps // GV_U)
    gs64_body = c.layout == "w3s" or (c.nbits in (4, 2))
    xp2 = nsteps > wpg and gs64_body and (c.layout == "w3s" or f16_exact)
    ksplit = nunits >= wpg and prow * 4 <= CUS * wg_per_cu * wpg
    tiles = prow if ksplit else -(-prow // wpg)
    return dict(wpg=wpg, xp2=xp2, ksplit=ksplit, nunits=nunits, second_row=tiles > CUS * wg_per_cu, wraps=(not ksplit) and nunits > GV_NF)


def sk_tile(c, extra=0):
    """sk_takes_narrow (skinny.hip:776-782)"""
    nb = 4 if c.layout == "w3s" else c.nbits        # (the stream layout: two slabs per packed row, like the 4-bit container; skinny.hip:95, :778)
    if ((c.base_opts | extra) & OPT_SKINNY_WIDE) or c.nbits == 8:
        return "wide"
    prows = sum(N // c.per for N in c.Ns)
    return "narrow" if prows <= (4 if nb == 2 else 1) * SK_NARROW_MAX_PROWS else "wide"


def sk_choose(c, extra=0):
    """sk_choose (skinny.hip:645-660): (tile, panels, ks, cps)"""
    tile = sk_tile(c, extra)
    panels = sum(-(-(N // c.per) // SK_ROWS[tile]) for N in c.Ns)
    nchunks = c.K // SK_KC
    forced = (c.base_opts | extra) >> 24
    ks = 1 if (panels * 16 >= CUS * 9 and nchunks <= SK_MAX_CPS) else -(-CUS // panels)
    if tile == "wide":
        if panels >= 48:
            ks = min(ks, max(nchunks // 8, 1))
    elif ks > 1:
        ks = min(CUS // panels, max(nchunks // 4, 1))
    ks = min(ks, nchunks // 2)
    ks = min(max(ks, 1), 16)
    if 1 <= forced <= nchunks:
        ks = forced
    cps = min(-(-nchunks // ks), SK_MAX_CPS)
    return tile, panels, -(-nchunks // cps), cps


def sk_ks_from_workspace(c, nbytes, extra=0):
    """the split a launch makes, read back from hqq_hip_gemv_workspace_bytes (sk_part_bytes, skinny.hip:661-663; 0 bytes: one split)"""
    if nbytes == 0:
        return 1
    tile, panels, _, _ = sk_choose(c, extra)
    unit = panels * SK_ROWS[tile] * c.per * 16 * (-(-c.M // 16)) * 4
    assert (nbytes - WS_COUNTER_BYTES) % unit == 0
    return (nbytes - WS_COUNTER_BYTES) // unit


def gemm_plan(L, c, extra=0, M=None, N=None):
    """hqq_hip_gemm_plan: dict(nw, bm, n_tiles, m_tiles, ks, kps, full, wgs), or None when another kernel serves the shape"""
    out = (ctypes.c_int * 8)()
    rc = L.hqq_hip_gemm_plan(c.nbits, c.M if M is None else M, c.Ns[0] if N is None else N, c.K, GS, gc.CODE[c.dt], c.base_opts | extra, out)
    return None if rc else dict(zip(("nw", "bm", "n_tiles", "m_tiles", "ks", "kps", "full", "wgs"), list(out)))


def g3_props(N, G):
    """the 3-bit container of an N-row layer with G groups per row (gemv3.hip:6-9, gemv3s.hip:6-11)"""
    R = N * G
    step = -(-R // 10)
    starts = [t * step for t in range(1, 10) if t * step < R]
    return dict(R=R, step=step, pad=10 * step - R, covered=G <= step, straddle=any(s % G for s in starts), exact=any(s % G == 0 for s in starts),
                step_mod_g=step % G, ragged_task=step % S3_ROWS != 0)


def g3_pick(G, slabs=False):
    """the smallest even N (even: the same levels also go through the stream layout) whose container has padding rows, step % G != 0, a row that
    straddles a slab boundary and — where some N below 400 allows it — a row that starts exactly on one; for the slab-sharing kernel a ragged
    last task as well"""
    for want_exact, first in ((True, 12), (True, 11), (False, 12), (False, 11)):   # (G = 65: an even N has N G % 10 == 0 — that case takes an odd N)
        for N in range(first, 400, 2):
            p = g3_props(N, G)
            if p["covered"] and p["pad"] and (G == 1 or (p["step_mod_g"] and p["straddle"])) and (p["exact"] or not want_exact) and (p["ragged_task"] or not slabs):
                return N
    raise AssertionError(G)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
ROWWISE_K = (64, 960, 1024, 1088, 2048, 2112, 4096, 4160, 6208, 8256)
ROWWISE_COMBOS = gc.ROWWISE_COMBOS
ROWWISE_ROWS = gc.ROWWISE_ROWS
ROWWISE_ROWS_SECOND = gc.ROWWISE_ROWS_SECOND
ROWS_8WAVE = 1027                   # more than 4 CUS, at most 8 CUS packed rows (gemv.hip:116); also more than CUS * 16 / 4: no ksplit (gemv.hip:156)
FACTORED_K = (64, 1088, 2112, 4160)
G3_ROWS_K = (64, 128, 1024, 1088, 4160)
G3_SLABS_K = (1024, 1088, 2112)
MFMA_K = (64, 192, 320, 2240, 2368, 2496)
MFMA_MS, MFMA_ROWS, MFMA_ROWS_SECOND = gc.MFMA_MS, gc.MFMA_ROWS, gc.MFMA_ROWS_SECOND
SKINNY_COMBOS = [(8, "u8", "f16"), (4, "u8", "f16"), (2, "u8", "f16"), (3, "w3s", "f16"), (8, "u8", "bf16"), (4, "u8", "bf16"), (2, "u8", "bf16"), (3, "w3s", "bf16")]
SKINNY_MS = (5, 16, 17, 33, 48, 64)
SKINNY_K = (512, 768, 1280, 4096, 4352)
SKINNY_ROWS = (1, 31, 33, 65)
PIPE_MS = (65, 128, 129, 257)
PIPE_K = (128, 384, 640, 2048)
PIPE_ROWS = (4, 60, 68, 132)
GEMM_MS, GEMM_K, GEMM_ROWS, GEMM_ROWS_REGTILE = gc.GEMM_MS, (64, 192, 576), gc.GEMM_ROWS, gc.GEMM_ROWS_REGTILE
# a hybrid plan of the pipelined GEMM (full > 0) on a 256-CU device: (nbits, M, N, K), 11 M weights; plan 8 waves x 128 tokens, 29 x 9 tiles, 256 of
# them whole, the other 5 — token tile 8, i.e. token row 1024 alone — split 3 ways.  It is the smallest N K that hqq_hip_gemm_plan reported over
# nbits 8 / 4 / 2, M in 257, 385, 513, 641, 769, 1025, K = 2048, 2176 .. 8192 and N K <= 32 Mi; that it is the smallest of all shapes is NOT asserted
# (tests/test_gs64_cpu.py asserts that it is a hybrid, and that the compared rows reach a split tile)
HYBRID = (8, 1025, 3588, 3072)


def _rowwise_cases():
    out = []
    for ci, (nbits, dt) in enumerate(ROWWISE_COMBOS):
        for i, K in enumerate(ROWWISE_K):
            j = i + ci
            out.append(C("rowwise", nbits, dt, 1 + j % GV_EXACT_MAX_M, (ROWWISE_ROWS[(j // 4 + i) % 3] * PER[nbits],), K, bias=j % 2 == 1))
    out += [C("rowwise", 4, "f16", 2, (ROWWISE_ROWS_SECOND * 2,), 64, bias=True, note="second_row"),
            C("rowwise", 2, "bf16", 3, (ROWWISE_ROWS_SECOND * 4,), 64, note="second_row"),
            C("rowwise", 4, "f16", 1, (ROWS_8WAVE * 2,), 2112, bias=True, note="wave8"),
            C("rowwise", 4, "f16", 2, (ROWS_8WAVE * 2,), 6208, note="ring_wraps"),
            C("rowwise", 4, "f16", 3, (14, 2, 26), 2112, bias=True),
            C("rowwise", 2, "bf16", 4, (28, 4, 52), 1088),
            C("rowwise", 8, "f16", 1, (7, 13, 1), 4160),
            C("rowwise", 1, "f16", 2, (8, 104, 56), 2112, bias=True)]
    for i, K in enumerate(FACTORED_K):
        for b, nbits in enumerate((4, 2)):
            out.append(C("rowwise", nbits, "f16", MFMA_MS[(i + b) % 4], (ROWWISE_ROWS[(i + b) % 3] * PER[nbits],), K, opts=OPT_FACTORED, bias=(i + b) % 2 == 1))
    return out


def _w3s_cases():
    out = []
    for ci, dt in enumerate(("f16", "bf16")):
        for i, K in enumerate(ROWWISE_K):
            j = i + 2 * ci
            out.append(C("rowwise_w3s", 3, dt, 1 + j % 4, (ROWWISE_ROWS[(j // 4 + i) % 3] * 2,), K, bias=j % 2 == 1, layout="w3s"))
    out.append(C("rowwise_w3s", 3, "f16", 3, (14, 2, 26), 2112, bias=True, layout="w3s"))
    return out


def _g3_cases():
    out = []
    for i, K in enumerate(G3_ROWS_K):
        for r in range(2 if K in (1088, 4160) else 1):
            out.append(C("gemv3_rows", 3, "f16", 1 + (2 * i + r) % 4, (g3_pick(K // GS),), K, bias=(i + r) % 2 == 1, layout="c3"))
    out.append(C("gemv3_rows", 3, "f16", 2, (g3_pick(17), g3_pick(17) + 10, 20), 1088, bias=True, layout="c3"))
    for i, K in enumerate(G3_SLABS_K):
        for r in range(2 if K == 1088 else 1):
            out.append(C("gemv3_slabs", 3, "f16", 1 + (i + 2 * r) % 4, (g3_pick(K // GS, True),), K, opts=OPT_GEMV3_SLABS, bias=(i + r) % 2 == 0, layout="c3"))
    out.append(C("gemv3_slabs", 3, "f16", 4, (g3_pick(17, True), g3_pick(17, True) + 6, 24), 1088, opts=OPT_GEMV3_SLABS, layout="c3"))
    return out


def _mfma_cases():
    out = []
    for ci, nbits in enumerate((8, 4, 2, 1)):
        for i, K in enumerate(MFMA_K):
            j = i + ci
            out.append(C("mfma16", nbits, "f16", MFMA_MS[j % 4], (MFMA_ROWS[(j // 4 + i) % 3] * PER[nbits],), K, bias=j % 2 == 1))
    out += [C("mfma16", 4, "f16", 5, (MFMA_ROWS_SECOND * 2,), 64, bias=True, note="second_tile"),
            C("mfma16", 4, "f16", 9, (42, 2, 74), 2368, bias=True),
            C("mfma16", 2, "f16", 16, (84, 148, 4), 320)]
    return out


def _skinny_variants(nbits, K):
    n = K // SK_KC
    v = [0, OPT_KS(2), OPT_KS(n // 2), OPT_KS(1)]
    if nbits != 8:
        v += [OPT_SKINNY_WIDE, OPT_SKINNY_WIDE | OPT_KS(2)]
    return tuple(dict.fromkeys(v))


def _skinny_cases():
    out = []
    for ci, (nbits, layout, dt) in enumerate(SKINNY_COMBOS):
        per = 2 if layout == "w3s" else PER[nbits]
        for i, K in enumerate(SKINNY_K):
            j = i + ci
            out.append(C("skinny", nbits, dt, SKINNY_MS[j % 6], (SKINNY_ROWS[(j // 2 + i) % 4] * per,), K, bias=j % 2 == 1, layout=layout, variants=_skinny_variants(nbits, K)))
    out += [C("skinny", 4, "f16", 17, (62, 2, 130), 768, bias=True, variants=_skinny_variants(4, 768)),
            C("skinny", 3, "bf16", 33, (66, 130, 2), 1280, layout="w3s", variants=_skinny_variants(3, 1280)),
            C("skinny", 2, "f16", 48, (124, 4, 260), 4352, variants=_skinny_variants(2, 4352))]
    return out


def _pipe_variants(nbits, K):
    v = [0, OPT_GEMM_NARROW, OPT_GEMM_WIDE] + ([OPT_GEMM_NARROW | OPT_GEMM_WIDE] if nbits != 2 else [])
    if K < 2048:
        v += [OPT_KS(2), OPT_KS(3), OPT_GEMM_WIDE | OPT_KS(2)]
    return tuple(v)


def _pipe_cases():
    out = []
    for ci, (nbits, layout, dt) in enumerate(SKINNY_COMBOS):
        per = 2 if layout == "w3s" else PER[nbits]
        for i, K in enumerate(PIPE_K):
            j = i + ci
            out.append(C("gemm_pipe", nbits, dt, PIPE_MS[j % 4], (PIPE_ROWS[(j // 4 + i) % 4] * per,), K, bias=j % 2 == 1, layout=layout, variants=_pipe_variants(nbits, K)))
    out += [C("gemm_pipe", 4, "f16", 129, (120, 8, 264), 640, bias=True, variants=(0, OPT_KS(2))),
            C("gemm_pipe", 3, "bf16", 65, (136, 8, 264), 384, layout="w3s", variants=(0, OPT_KS(3)))]
    if HYBRID:
        nbits, M, N, K = HYBRID
        out.append(C("gemm_pipe", nbits, "f16", M, (N,), K, bias=True, note="hybrid"))
    return out


def _gemm_cases():
    out = []
    for b, nbits in enumerate((4, 2)):
        for i, K in enumerate(GEMM_K):
            for v, opts in enumerate((0, OPT_GEMM_REGTILE, OPT_GEMM_CLASSIC)):
                j = i + b + v
                out.append(C("gemm_tile", nbits, "f16", GEMM_MS[j % 3], (GEMM_ROWS * PER[nbits],), K, opts=opts, bias=j % 2 == 1))
    out.append(C("gemm_tile", 4, "f16", 17, (GEMM_ROWS_REGTILE * 2,), 64, opts=OPT_GEMM_REGTILE, bias=True, note="regtile_kernel"))
    return out


CASES = _rowwise_cases() + _w3s_cases() + _g3_cases() + _mfma_cases() + _skinny_cases() + _pipe_cases() + _gemm_cases()
assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}


# ---- packing -------------------------------------------------------------------------------------------------------------------------
def pack_layer(oracle, c, U, N):
    """the levels U [N G, 64] as the case's layout: (what the kernel reads, the reference container or None)"""
    U = np.ascontiguousarray(U, np.uint8)
    if c.layout == "u8":
        return oracle.pack(c.nbits, U).reshape(N // c.per, c.K), None
    P = oracle.pack(3, U)
    assert P.dtype == np.int32 and P.shape == (-(-N * c.G // 10), GS)
    if c.layout == "c3":
        return P, P
    return oracle.w3s_pack_np(P, N, c.K).view(np.int32).reshape(N // 2, c.K // 16 * 3), P


def unpack_layer(oracle, c, Wq, N):
    """the inverse, through the oracle: levels [N G, 64]"""
    if c.layout == "u8":
        return oracle.unpack(c.nbits, Wq.reshape(-1, GS) if c.nbits == 8 else Wq.reshape(N // c.per, c.K)).reshape(N * c.G, GS)
    P = Wq if c.layout == "c3" else oracle.w3s_unpack_np(Wq.view(np.uint32), N, c.K)
    return oracle.unpack(3, P)[:N * c.G]


# ---- the kernels' group index, restated ----------------------------------------------------------------------------------------------
MUTANTS = {
    # name: (route family it perturbs, what is wrong)
    "unit_edge_off_by_one": "rowwise: a unit's first group is 31 u, not 32 u (gemv_kernel.inc:107)",
    "ragged_end_next_row": "rowwise: the consumer of a ragged row's last group takes the lane behind it — the next row's first group (gemv_kernel.inc:102, :335)",
    "mz_wrong_half": "rowwise MZ: slab s reads the other half of its slab pair (gemv_kernel.inc:104, :335)",
    "slice_edge_off_by_one": "mfma16: a K slice's first block index is kb0 - 1 for every wave but the first (gemv_mfma.hip:157, :172)",
    "split_last_chunk_dropped": "skinny: c1 = c0 + cps - 1 in the last, ragged split (skinny.hip:320)",
    "split_last_chunk_twice": "skinny: the last split starts one chunk early (skinny.hip:320)",
    "lds_stride_even": "skinny: the reader strides the constants by cps * SK_BLK, the writer by cps * SK_BLK + 1 (skinny.hip:321, :479)",
    "second_wave_first_blocks": "skinny: the second wave of a row group takes the first wave's blocks' constants (skinny.hip:311)",
    "pipe_last_split_short": "gemm_pipe: the last split runs kps steps back from the end of K instead of from ks * kps (gemm_pipe.hip:273-274)",
    "slab_after_row_change": "gemv3_rows: a group behind the slab boundary keeps the first slab (gemv3.hip:171)",
    "task_no_row_change": "gemv3_slabs: groups behind a task's row change are added to the first row (gemv3s.hip:10-11)",
    "k_tile_off_by_one": "gemm_tile: the K tile's group is (k0 - 64) / 64 from the second tile on (gemm.hip:116, :297)",
}


def group_index(c, li=0, mutant=None, extra=0, plan=None):
    """For layer li of the case: idx [N, G] — the flat meta index the kernel pairs with (row n, group g), -1 where it reads nothing (a buffer load's
    range check returns 0) —, src [N, G] — the flat index of the level row (of unpack(container)) it dequantises there, -1 for zeros —, row [N, G] —
    the output row the products are added to — and mult [G], how often group g's products are counted.  mutant: one of MUTANTS."""
    N, G, per = c.Ns[li], c.G, c.per
    n = np.arange(N, dtype=np.int64).reshape(N, 1)
    g = np.arange(G, dtype=np.int64).reshape(1, G)
    row = np.broadcast_to(n, (N, G)).copy()
    mult = np.ones(G)
    R = N * G
    if c.route in ("rowwise", "rowwise_w3s", "mfma16", "skinny", "gemm_pipe", "gemm_tile"):
        rps = N // per
        p, s = n % rps, n // rps
        src = (n * G + g) + 0 * g
        gg = g + 0 * n                                        # the group the kernel's own decomposition of k arrives at
        if c.route in ("rowwise", "rowwise_w3s") and (c.layout == "w3s" or c.nbits in (4, 2)) and not c.factored:
            u, l = g // GV_UNIT_GROUPS, g % GV_UNIT_GROUPS    # unit, fetching lane (gemv_kernel.inc:84 m_lane, :335 the consumer's source lane)
            base = (31 if mutant == "unit_edge_off_by_one" else GV_UNIT_GROUPS) * u
            l = l + (1 if mutant == "ragged_end_next_row" else 0) * ((g == G - 1) & (G % GV_UNIT_GROUPS != 0))
            half = (s & 1) ^ (1 if mutant == "mz_wrong_half" else 0)
            idx = (p + (s - (s & 1)) * rps) * G + base + l + half * rps * G      # gemv_kernel.inc:103-107
        elif c.route == "mfma16" and c.nbits in (4, 2):
            tiles = sum(-(-(Nl // per) // GM_ROWS) for Nl in c.Ns)
            sl = gc.gm_slices(c.nbits, c.K, tiles)
            kb0 = np.zeros(G, np.int64)
            for w, (a, b) in enumerate(sl):
                kb0[a:b] = a - (1 if mutant == "slice_edge_off_by_one" and w else 0)
                gg[:, a:b] = kb0[a:b] + (np.arange(a, b) - a)
            idx = (p + s * rps) * G + gg                      # gemv_mfma.hip:172-176
        elif c.route == "skinny":
            tile, panels, ks, cps = sk_choose(c, extra)
            nch = G // SK_BLK
            chunk, blk = g // SK_BLK, g % SK_BLK
            split = chunk // cps
            c0 = split * cps
            if mutant == "split_last_chunk_twice":
                c0 = c0 - (split == ks - 1) * (split > 0)
            local = (g // SK_BLK - c0) * SK_BLK + (blk % SK_BPW[tile] if mutant == "second_wave_first_blocks" else blk)
            if mutant == "split_last_chunk_dropped" and nch % cps:
                mult[(nch - 1) * SK_BLK:] = 0
            if mutant == "split_last_chunk_twice" and ks > 1:
                mult[(ks - 1) * cps * SK_BLK - SK_BLK:(ks - 1) * cps * SK_BLK] = 2
            rs = (p % SK_ROWS[tile]) * per + s                # LDS row of (packed row, slab): skinny.hip:479
            if mutant == "lds_stride_even":
                q = rs * (cps * SK_BLK) + local
                rs2, local2 = q // (cps * SK_BLK + 1), q % (cps * SK_BLK + 1)
                p2, s2 = p - p % SK_ROWS[tile] + rs2 // per, rs2 % per
                idx = np.where((local2 < cps * SK_BLK) & (p2 < rps), (p2 + s2 * rps) * G + c0 * SK_BLK + local2, -1)
            else:
                idx = (p + s * rps) * G + c0 * SK_BLK + local  # skinny.hip:462, :479
        elif c.route == "gemm_pipe":
            nk = G
            ksn, kps = (plan["ks"], plan["kps"]) if plan else (1, nk)
            step = g
            split = step // kps
            kt0 = split * kps
            if mutant == "pipe_last_split_short" and ksn > 1 and nk % kps:
                kt0 = np.where(split == ksn - 1, nk - kps, kt0)
                mult[nk - kps:(ksn - 1) * kps] = 2
            idx = (p + s * rps) * G + kt0 + (step - split * kps)   # gemm_pipe.hip:273-274
        elif c.route == "gemm_tile":
            kt = g - (1 if mutant == "k_tile_off_by_one" else 0) * (g > 0)
            idx = (p + s * rps) * G + kt                      # gemm.hip:116, :297 with gs = 64 = GB_K
        else:                                                 # the generic body at gs = 64: goff = k0 / gs (gemv_kernel.inc:122-126; gemv_mfma.hip:185)
            idx = (p + s * rps) * G + g
        idx = np.where((idx >= 0) & (idx < R), idx, -1) + 0 * src
        return idx, src, row, mult
    # the reference's 3-bit container: group row r = n G + g sits in slab r / step at packed row r - slab * step
    step = -(-R // 10)
    r = n * G + g
    if c.route == "gemv3_rows":
        s0 = (n * G) // step                                  # gemv3.hip:164-172
        s = s0 + (0 if mutant == "slab_after_row_change" else 1) * (r >= (s0 + 1) * step)
        pk = r - s * step
        src = np.where(pk < step, s * step + pk, -1)          # a packed row past the container: the range check's zeros
        return r + 0 * g, src, row, mult
    # gemv3_slabs: task j, slab t, packed rows 16 j .. 16 j + 15 -> groups g0 .. of row n0, then of row n0 + 1 (gemv3s.hip:9-11)
    t = r // step
    pk = r - t * step
    p0 = pk - pk % S3_ROWS
    n0 = (p0 + t * step) // G
    if mutant == "task_no_row_change":
        row = np.where(n0 < n, n0, n) + 0 * g
    return r + 0 * g, r + 0 * g, row, mult


def restated_weights(c, kind, li=0, mutant=None, extra=0, plan=None, oracle=None):
    """W_eff [N, K]: what the restated kernel contracts with x — levels from where it reads them, (zero, scale) from the index it computes"""
    U, s, z, W, q = gc.coded_layer(c, kind, li)
    N, G = c.Ns[li], c.G
    idx, src, row, mult = group_index(c, li, mutant, extra, plan)
    lev = np.where(src.reshape(N, G, 1) >= 0, U[np.maximum(src, 0)].astype(np.float64), 0.0)          # [N, G, 64]
    zz = np.where(idx >= 0, z[np.maximum(idx, 0)], 0.0).reshape(N, G, 1)
    ss = np.where(idx >= 0, s[np.maximum(idx, 0)], 0.0).reshape(N, G, 1)
    w = (lev - zz) * ss * mult.reshape(1, G, 1)
    out = np.zeros((N, G, GS))
    np.add.at(out, (row, np.broadcast_to(np.arange(G).reshape(1, G), (N, G))), w)
    return out.reshape(N, c.K)
