"""CPU side of the group_size = 64 cases (tests/_gs64_cases.py): every case takes the route its table names and reaches the launch variant it claims
(asked of the library's planner where it answers — hqq_hip_forward_route, hqq_hip_gemv_workspace_bytes, hqq_hip_gemm_plan; without a device the library
assumes 256 compute units, an MI355X's, so these are the plans the GPU file runs — and derived from the restated launch rules otherwise); the packed
bytes and 3-bit words, in both layouts, dequantise on the host to the closed-form W and every expected output is exact in fp32 in any summation
order; the codes separate every probed group from its neighbours; the probes cover every group or every edge; and the host restatement of each
kernel's group index (_gs64_cases.group_index) reproduces the closed form while each deliberately wrong variant of it is caught:

  mutant                     caught by (case, run)
  unit_edge_off_by_one       rowwise-4b-f16-M3-N2-K2112
  ragged_end_next_row        rowwise-4b-f16-M1-N14-K1088
  mz_wrong_half              rowwise-4b-f16-M2-N2-K64-bias
  slice_edge_off_by_one      mfma16-4b-f16-M5-N42-K2240
  split_last_chunk_dropped   skinny-4b-f16-M17-N66-K768, OPT_SKINNY_KS(2)
  split_last_chunk_twice     skinny-4b-f16-M17-N66-K768, OPT_SKINNY_KS(2)
  lds_stride_even            skinny-4b-f16-M17-N66-K768, OPT_SKINNY_KS(2)
  second_wave_first_blocks   skinny-4b-f16-M17-N66-K768, OPT_SKINNY_WIDE
  pipe_last_split_short      gemm_pipe-4b-f16-M129-N120-K384, OPT_SKINNY_KS(2)
  slab_after_row_change      gemv3_rows-3bc3-f16-M3-N12-K128-bias
  task_no_row_change         gemv3_slabs-3bc3-f16-M1-N12-K1024-slabs-bias
  k_tile_off_by_one          gemm_tile-4b-f16-M100-N40-K192-bias
"""
import ctypes

import numpy as np
import pytest

import _gs_cases as gc
import _gs64_cases as g64
from _gs_cases import FAMILIES, KINDS
from _gs64_cases import CASES, GS

CATCHES = {
    "unit_edge_off_by_one": ("rowwise-4b-f16-M3-N2-K2112", 0),
    "ragged_end_next_row": ("rowwise-4b-f16-M1-N14-K1088", 0),
    "mz_wrong_half": ("rowwise-4b-f16-M2-N2-K64-bias", 0),
    "slice_edge_off_by_one": ("mfma16-4b-f16-M5-N42-K2240", 0),
    "split_last_chunk_dropped": ("skinny-4b-f16-M17-N66-K768", g64.OPT_KS(2)),
    "split_last_chunk_twice": ("skinny-4b-f16-M17-N66-K768", g64.OPT_KS(2)),
    "lds_stride_even": ("skinny-4b-f16-M17-N66-K768", g64.OPT_KS(2)),
    "second_wave_first_blocks": ("skinny-4b-f16-M17-N66-K768", g64.OPT_SKINNY_WIDE),
    "pipe_last_split_short": ("gemm_pipe-4b-f16-M129-N120-K384", g64.OPT_KS(2)),
    "slab_after_row_change": ("gemv3_rows-3bc3-f16-M3-N12-K128-bias", 0),
    "task_no_row_change": ("gemv3_slabs-3bc3-f16-M1-N12-K1024-slabs-bias", 0),
    "k_tile_off_by_one": ("gemm_tile-4b-f16-M100-N40-K192-bias", 0),
}


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    return _C.lib()


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _layer_case(c, li):
    return c if not c.grouped else g64.C(c.route, c.nbits, c.dt, c.M, (c.Ns[li],), c.K, c.opts, c.bias, c.layout, c.variants, c.note)


def _by(route):
    return [c for c in CASES if c.route == route]


# ---- routes --------------------------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_route_the_table_names(L):
    from hqq_amd import ops
    assert (ops.ROUTE_ROWWISE, ops.ROUTE_ROWWISE_W3S, ops.ROUTE_GEMV3_ROWS, ops.ROUTE_GEMV3_SLABS, ops.ROUTE_MFMA16, ops.ROUTE_SKINNY, ops.ROUTE_GEMM_PIPE,
            ops.ROUTE_GEMM_TILE) == tuple(range(1, 9))
    assert (ops.OPT_FACTORED, ops.OPT_META_SCALABLE, ops.OPT_GEMV3_ROWWISE, ops.OPT_GEMV3_SLABS, ops.OPT_GEMM_REGTILE, ops.OPT_GEMM_CLASSIC, ops.OPT_GEMM_NARROW,
            ops.OPT_GEMM_WIDE, ops.OPT_GEMM_NOHYBRID, ops.OPT_SKINNY_WIDE, ops.OPT_W3S) == (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
    assert ops.OPT_SKINNY_KS(3) == g64.OPT_KS(3)
    for c in CASES:
        want, dt = g64.WANT_ROUTE[c.route], gc.CODE[c.dt]
        assert c.gs == GS and c.K % GS == 0 and c.K <= 8256, c.id
        for extra in c.variants:
            for meta in {0, g64.OPT_META_SCALABLE if c.dt == "f16" else 0}:
                opts = c.base_opts | extra | meta
                assert ops.route(gc.DT[c.dt], c.M, tuple(c.Ns), c.K, GS, c.nbits, opts) == want, (c.id, opts, L.hqq_hip_last_error())
                for N in c.Ns:   # the per-layer calls a grouped case is compared with
                    assert L.hqq_hip_forward_route(c.nbits, 1, _i64([N]), c.M, c.K, GS, dt, opts) == want, (c.id, N, opts)
        if c.route in g64.ROW_PER_WAVE and c.M > 1:   # M = 1 is compared with row 0 of M rows: the same route
            assert ops.route(gc.DT[c.dt], 1, tuple(c.Ns), c.K, GS, c.nbits, c.base_opts) == want, c.id
        if c.route == "gemv3_slabs":   # the same layers through the row-per-wave kernel; unforced they are far below the slab kernel's 19 MB
            o = (c.base_opts & ~g64.OPT_GEMV3_SLABS)
            assert ops.route(gc.DT[c.dt], c.M, tuple(c.Ns), c.K, GS, 3, o | g64.OPT_GEMV3_ROWWISE) == g64.ROUTE_GEMV3_ROWS
            assert ops.route(gc.DT[c.dt], c.M, tuple(c.Ns), c.K, GS, 3, o) == g64.ROUTE_GEMV3_ROWS
            assert sum(-(-N * c.G // 10) * 256 for N in c.Ns) < g64.G3S_MIN_BYTES
        if c.layout == "c3" and c.G != 65:   # ... and through the stream layout (the GPU file compares the three; G = 65 needs an odd N for its padding rows)
            assert all(N % 2 == 0 for N in c.Ns) and ops.route(gc.DT[c.dt], c.M, tuple(c.Ns), c.K, GS, 3, g64.OPT_W3S) == g64.ROUTE_ROWWISE_W3S, c.id
        assert all(N * c.K <= 32 << 20 for N in c.Ns), c.id


def test_the_table_holds_what_the_issue_lists():
    rw = [c for c in _by("rowwise") if not c.factored]
    for combo in g64.ROWWISE_COMBOS:
        cs = [c for c in rw if (c.nbits, c.dt) == combo and not c.grouped]
        assert {c.M for c in cs} == {1, 2, 3, 4} and {c.K for c in cs} >= set(g64.ROWWISE_K), combo
        assert {c.Ns[0] // c.per for c in cs} >= set(g64.ROWWISE_ROWS), combo
    for nbits in (8, 1):   # the ragged-unit K values at the two widths that take the generic body
        assert {1088, 2112, 4160, 6208} <= {c.K for c in rw if c.nbits == nbits}
    assert {c.M for c in _by("rowwise") if c.factored} == set(g64.MFMA_MS) and {c.nbits for c in _by("rowwise") if c.factored} == {4, 2}
    for dt in ("f16", "bf16"):
        cs = [c for c in _by("rowwise_w3s") if c.dt == dt and not c.grouped]
        assert {c.M for c in cs} == {1, 2, 3, 4} and {c.K for c in cs} == set(g64.ROWWISE_K) and {c.Ns[0] // 2 for c in cs} == set(g64.ROWWISE_ROWS)
        assert all(N % 2 == 0 for c in cs for N in c.Ns)
    assert {c.K for c in _by("gemv3_rows")} == set(g64.G3_ROWS_K) and {c.M for c in _by("gemv3_rows")} == {1, 2, 3, 4}
    assert {c.K for c in _by("gemv3_slabs")} == set(g64.G3_SLABS_K) and {c.M for c in _by("gemv3_slabs")} == {1, 2, 3, 4}
    for nbits in (8, 4, 2, 1):
        cs = [c for c in _by("mfma16") if c.nbits == nbits and not c.grouped]
        assert {c.M for c in cs} == set(g64.MFMA_MS) and {c.K for c in cs} >= set(g64.MFMA_K) and {c.Ns[0] // c.per for c in cs} >= set(g64.MFMA_ROWS), nbits
    for (nbits, layout, dt) in g64.SKINNY_COMBOS:
        cs = [c for c in _by("skinny") if (c.nbits, c.layout, c.dt) == (nbits, layout, dt) and not c.grouped]
        assert {c.K for c in cs} == set(g64.SKINNY_K) and len({c.M for c in cs}) >= 5 and len({c.Ns[0] // c.per for c in cs}) >= 3, (nbits, layout, dt)
        cs = [c for c in _by("gemm_pipe") if (c.nbits, c.layout, c.dt) == (nbits, layout, dt) and not c.grouped and not c.note]
        assert {c.K for c in cs} == set(g64.PIPE_K) and {c.M for c in cs} == set(g64.PIPE_MS) and {c.Ns[0] // c.per for c in cs} <= set(g64.PIPE_ROWS), (nbits, layout, dt)
    assert {c.M for c in _by("skinny")} == set(g64.SKINNY_MS) and {-(-c.M // 16) for c in _by("skinny")} == {1, 2, 3, 4}
    assert {c.Ns[0] // c.per for c in _by("skinny") if not c.grouped} == set(g64.SKINNY_ROWS)
    assert {c.Ns[0] // c.per for c in _by("gemm_pipe") if not c.grouped and not c.note} == set(g64.PIPE_ROWS)
    for nbits in (4, 2):
        for opts in (0, g64.OPT_GEMM_REGTILE, g64.OPT_GEMM_CLASSIC):
            cs = [c for c in _by("gemm_tile") if c.nbits == nbits and c.opts == opts and not c.note]
            assert {c.M for c in cs} == set(g64.GEMM_MS) and {c.K for c in cs} == set(g64.GEMM_K)
            assert all(c.K % 128 for c in cs)       # the default route reaches the output-tile kernel because the pipelined one does not cover K
    for r in ("rowwise", "rowwise_w3s", "gemv3_rows", "gemv3_slabs", "mfma16", "skinny", "gemm_pipe"):
        assert any(c.grouped and len(set(c.Ns)) == 3 for c in _by(r)), r
    assert all(N % 8 == 0 for c in CASES if c.nbits == 1 for N in c.Ns)
    assert 200 < len(CASES) < 400


# ---- reached variants ----------------------------------------------------------------------------------------------------------------
def test_row_per_wave_launches_reach_the_variants_they_claim():
    for route in ("rowwise", "rowwise_w3s"):
        cs = [c for c in _by(route) if not c.factored]
        for c in cs:
            v = g64.gv_launch(c)
            assert v["second_row"] == (c.note == "second_row") and (v["wpg"] == 8) == (c.note == "wave8"), (c.id, v)
            assert v["wraps"] == (c.K in (4160, 6208, 8256) and not v["ksplit"]), (c.id, v)   # three units and more against a ring of GV_NF = 2
        gs64 = [c for c in cs if c.layout == "w3s" or c.nbits in (4, 2)]
        for dt in ("f16", "bf16"):
            sel = [c for c in gs64 if c.dt == dt]
            xp2 = {c.K for c in sel if g64.gv_launch(c)["xp2"]}
            assert xp2 == ({4160, 6208, 8256} if (dt == "f16" or route == "rowwise_w3s") else set()), (route, dt, xp2)   # gemv.hip:130 (fp16 only); gemv_w3s.hip:64
            assert any(c.K == 4096 and not g64.gv_launch(c)["xp2"] for c in sel)                               # nsteps == WPG: one pass
            assert {c.K for c in sel if g64.gv_launch(c)["ksplit"]} >= {6208, 8256}                            # nunits >= WPG, few rows
            assert all(not g64.gv_launch(c)["ksplit"] for c in sel if c.K <= 4160)
    w8 = [c for c in _by("rowwise") if c.note == "wave8"]
    assert len(w8) == 1 and w8[0].nbits == 4 and w8[0].M == 1 and w8[0].dt == "f16" and 4 * g64.CUS < w8[0].Ns[0] // 2 <= 8 * g64.CUS and w8[0].K >= g64.GV_UNIT
    wr = [c for c in _by("rowwise") if c.note == "ring_wraps"]
    assert wr and all(g64.gv_launch(c)["wraps"] and g64.gv_launch(c)["xp2"] and g64.gv_launch(c, M=1)["wpg"] == 8 for c in wr)
    assert {c.dt for c in _by("rowwise") if c.note == "second_row"} == {"f16", "bf16"}
    # meta lanes past a ragged row's end: G % 32 != 0 — the next row's groups, or past the tensor for the last row of the last slab (every n is compared)
    assert {c.G % g64.GV_UNIT_GROUPS for c in _by("rowwise")} >= {0, 1, 15, 16, 17}


def test_three_bit_container_cases_reach_their_edges():
    for c in _by("gemv3_rows") + _by("gemv3_slabs"):
        for N in c.Ns[:1] if c.grouped else c.Ns:
            p = g64.g3_props(N, c.G)
            assert p["covered"] and p["pad"], (c.id, p)
            if c.G > 1:
                assert p["step_mod_g"] and p["straddle"], (c.id, p)
            if c.route == "gemv3_slabs":
                assert p["ragged_task"] and c.G >= g64.S3_ROWS, (c.id, p)
    # a row that starts exactly on a slab boundary needs t step = 0 (mod G) for a t in 1..9 with step != 0 (mod G): never at the prime G = 17; at G = 65
    # padding rows need an odd N, then step = (13 N + 1) / 2 is no multiple of 13 and t = 5 fails, t = 13 is no slab; at G = 33 no N below 400 has it
    assert {c.G for c in _by("gemv3_rows") if not c.grouped and g64.g3_props(c.Ns[0], c.G)["exact"]} == {1, 2, 16}
    assert {c.G for c in _by("gemv3_slabs") if not c.grouped and g64.g3_props(c.Ns[0], c.G)["exact"]} == {16}
    assert any(c.G == g64.S3_ROWS for c in _by("gemv3_slabs")) and any(c.G == g64.S3_ROWS + 1 for c in _by("gemv3_slabs"))


def test_mfma_cases_reach_their_edges():
    mf = [c for c in _by("mfma16") if not c.grouped]
    for nbits in (8, 4, 2, 1):
        uneven = 0
        for c in (c for c in mf if c.nbits == nbits):
            tiles = -(-(c.Ns[0] // c.per) // g64.GM_ROWS)
            n = [b - a for a, b in gc.gm_slices(nbits, c.K, tiles)]
            assert min(n) >= 1
            if c.K >= 2240:
                assert len(n) == min(32 // c.per, 16) and len(set(n)) > 1, (c.id, n)   # the most waves a tile gets, every slice an uneven share
                uneven += 1
            if c.K == 320:
                assert sum(n) == 5 and any(v % 2 for v in n)                           # an odd number of blocks: a half-dead unit
        assert uneven == 3, nbits
    big = [c for c in mf if c.note == "second_tile"]
    assert big and all(-(-(c.Ns[0] // c.per) // g64.GM_ROWS) > gc.gm_grid_cap(c.nbits, c.K, -(-(c.Ns[0] // c.per) // g64.GM_ROWS)) for c in big)


def test_skinny_launches_split_as_restated_and_reach_their_edges(L):
    seen = set()
    for c in _by("skinny"):
        for extra in c.variants:
            tile, panels, ks, cps = g64.sk_choose(c, extra)
            nbytes = L.hqq_hip_gemv_workspace_bytes(c.nbits, len(c.Ns), _i64(c.Ns), c.M, c.K, GS, gc.CODE[c.dt], c.base_opts | extra)
            assert g64.sk_ks_from_workspace(c, nbytes, extra) == ks, (c.id, extra, nbytes, (tile, panels, ks, cps))
            assert tile == ("wide" if (extra & g64.OPT_SKINNY_WIDE) or c.nbits == 8 else "narrow"), (c.id, extra)
            nch = c.K // g64.SK_KC
            forced = extra >> 24
            if not forced and not c.grouped and panels == 1 and ks > 1:
                seen.add("own split of a one-panel layer")
            if forced == 2 and nch % 2 and ks == 2 and nch % cps:
                seen.add("a ragged last split")
            if forced == nch // 2 and forced > 1 and cps in (2, 3) and ks == forced:
                seen.add("two chunks per split")
            if forced == 1:
                seen.add("one split" if ks == 1 else "the cap forces a second split")
                assert (ks, cps) == ((1, nch) if nch <= g64.SK_MAX_CPS else (2, g64.SK_MAX_CPS)), (c.id, ks, cps)
            if cps == g64.SK_MAX_CPS and ks == 1:
                seen.add("16 chunks in one split")
            seen.add(tile)
            seen.add((tile, -(-c.M // 16)))
            if nch % 2 and cps % 2:
                seen.add("an odd chunk count against the ring of 2")
    assert seen >= {"own split of a one-panel layer", "a ragged last split", "two chunks per split", "one split", "the cap forces a second split",
                    "16 chunks in one split", "narrow", "wide", "an odd chunk count against the ring of 2"} | {(t, m) for t in ("narrow", "wide") for m in (1, 2, 3, 4)}, seen
    # packed rows 31 / 33 / 65: a ragged narrow panel, a panel and a row (narrow), a panel and a row (wide)
    rows = {c.Ns[0] // c.per for c in _by("skinny") if not c.grouped}
    assert 31 < g64.SK_ROWS["narrow"] < 33 < g64.SK_ROWS["wide"] < 65 and rows == {1, 31, 33, 65}


def test_pipelined_plans_reach_their_edges(L):
    seen = set()
    for c in _by("gemm_pipe"):
        assert not c.grouped or L.hqq_hip_gemm_grouped_covers(c.nbits, len(c.Ns), _i64(c.Ns), c.M, c.K, GS, gc.CODE[c.dt], c.base_opts) == 1, c.id
        for N in c.Ns:
            for extra in c.variants:
                p = g64.gemm_plan(L, c, extra, N=N)
                assert p is not None, (c.id, extra)
                nk = c.K // g64.GD_K
                both = extra & g64.OPT_GEMM_NARROW and extra & g64.OPT_GEMM_WIDE
                if both:
                    assert (p["nw"], p["bm"]) == (8, 256) and c.nbits != 2
                    seen.add("256-token tile")
                elif extra & g64.OPT_GEMM_NARROW:
                    assert (p["nw"], p["bm"]) == (4, 128)
                    seen.add("narrow")
                elif extra & g64.OPT_GEMM_WIDE and c.nbits != 2:   # (2-bit layers keep the 4-wave tile: gemm_pipe.hip:613)
                    assert (p["nw"], p["bm"]) == (8, 128)
                    seen.add("wide")
                forced = extra >> 24
                if forced:
                    kps = -(-nk // forced)
                    kps += kps & 1
                    assert (p["kps"], p["ks"]) == (kps, -(-nk // kps)) and p["full"] == 0, (c.id, extra, p)   # gemm_pipe.hip:574-576
                    if p["ks"] > 1 and nk % p["kps"]:
                        seen.add("a ragged last split")
                    if p["ks"] > 1 and (p["kps"] // 2) % 2:
                        seen.add("an odd number of step pairs per split")
                    seen.add(("forced", forced, p["ks"]))
                elif p["ks"] > 1:
                    assert p["kps"] >= 16 and c.K >= 2048, (c.id, p)
                    seen.add("hybrid" if p["full"] else "unforced split")
                if c.note == "hybrid":
                    assert p["full"] > 0 and p["full"] % 256 == 0 and p["ks"] > 1 and p["n_tiles"] * p["m_tiles"] > p["full"], p
                    # the split tiles are the ids from `full` on, token tile mt = tile / n_tiles (gemm_pipe.hip:263-266): the rows the GPU file compares —
                    # every row of every launch, gc.launch_index — include token rows of a split tile, each carrying a probe
                    split_rows = {m for t in range(p["full"], p["n_tiles"] * p["m_tiles"]) for m in range(t // p["n_tiles"] * p["bm"], min((t // p["n_tiles"] + 1) * p["bm"], c.M))}
                    whole_rows = {m for t in range(p["full"]) for m in range(t // p["n_tiles"] * p["bm"], min((t // p["n_tiles"] + 1) * p["bm"], c.M))}
                    for fam in FAMILIES:
                        idx = gc.launch_index(c, gc.activations(c, fam).shape[0])
                        assert split_rows and whole_rows and split_rows | whole_rows == set(range(c.M)) and len(idx) % c.M == 0 and len(idx) >= c.M, (fam, sorted(split_rows)[:3])
                ragged = (N // c.per) % (16 * p["nw"])
                seen.add("ragged feature tile" if ragged else "whole feature tile")
                seen.add("ragged token tile" if c.M % p["bm"] else "whole token tile")
    assert seen >= {"256-token tile", "narrow", "wide", "a ragged last split", "an odd number of step pairs per split", "unforced split", "hybrid",
                    "ragged feature tile", "ragged token tile", "whole token tile", ("forced", 2, 2), ("forced", 3, 3)}, seen
    assert g64.HYBRID is not None and g64.HYBRID[2] * g64.HYBRID[3] <= 32 << 20


def test_output_tile_cases_reach_their_kernels(L):
    gm = _by("gemm_tile")
    for c in gm:
        assert g64.gemm_plan(L, c) is None, c.id                              # not the pipelined kernel
        assert gc.reaches_regtile(c) == (c.note == "regtile_kernel"), c.id
        assert (c.Ns[0] // c.per) % (gc.GB_N // c.per) and (c.Ns[0] // c.per) % g64.RT_ROWS and c.K % g64.GB_K == 0, c.id   # ragged N tiles
    assert any(gc.reaches_regtile(c) for c in gm)
    assert any(c.M % 128 for c in gm) and any(c.M > 128 for c in gm)


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def _exact_in_dtype(a, dt):
    a = np.asarray(a, np.float64)
    if dt == "bf16" and not np.array_equal(a.astype(np.float32).astype(np.float64), a):
        return False
    return np.array_equal(gc.round_dt(a, dt), a)


@pytest.mark.parametrize("route,nbits,layout,dt", sorted({(c.route, c.nbits, c.layout, c.dt) for c in CASES}))
def test_closed_forms_are_what_the_packed_layers_dequantise_to_and_exact(oracle, route, nbits, layout, dt):
    """per case, layer and kind: meta and weights exact in the dtype; the packed bytes (3-bit: the container AND the stream layout) unpack to the levels
    and dequantise, through the oracle, to the closed-form W; every partial sum of every activation family is a float32-exact dyadic number; expected()
    equals the correctly rounded fp64 product of the dequantised weights"""
    for c in CASES:
        if (c.route, c.nbits, c.layout, c.dt) != (route, nbits, layout, dt) or c.factored:
            continue
        assert gc.level_shift(c) >= 0 and c.K * (2 ** c.nbits - 1) < 2 ** (15 + gc.level_shift(c))
        for li in range(len(c.Ns)):
            N = c.Ns[li]
            for kind in KINDS:
                U, s, z, W, q = gc.coded_layer(c, kind, li)
                for a in (s, z, W):
                    assert _exact_in_dtype(a, c.dt), (c.id, kind)
                assert int(U.max()) < 2 ** c.nbits
                if kind == "level":
                    n, k = np.arange(N).reshape(N, 1), np.arange(c.K).reshape(1, c.K)
                    assert np.array_equal(U.reshape(N, c.K), (3 * n + 5 * k) % 2 ** c.nbits)
                Wq, P = g64.pack_layer(oracle, c, U, N)
                assert np.array_equal(g64.unpack_layer(oracle, c, Wq, N), U), (c.id, kind, "unpack")
                if c.layout == "w3s":   # the stream layout restores the container bit for bit, padding rows included
                    assert np.array_equal(oracle.w3s_unpack_np(Wq.view(np.uint32), N, c.K), P) and Wq.size * 4 == N * c.K * 3 // 8
                cont = Wq if c.layout == "u8" else P
                Ud = g64.unpack_layer(oracle, c, Wq, N)
                cont2 = oracle.pack(c.nbits, Ud) if c.layout == "u8" else oracle.pack(3, Ud)    # (dequantise what the kernel's own bytes unpack to)
                assert np.array_equal(np.asarray(cont2).reshape(-1), np.asarray(cont).reshape(-1))
                Wd = oracle.from_cd(oracle.dequantize(c.nbits, cont2, gc.raw(s, c.dt), gc.raw(z, c.dt), N, c.K, GS, gc.CODE[c.dt]), gc.CODE[c.dt])
                assert np.array_equal(Wd.astype(np.float64), W), (c.id, kind)
                b = gc.coded_bias(c, li)
                assert b is None or _exact_in_dtype(b, c.dt)
                for fam in FAMILIES:
                    X = gc.activations(c, fam)
                    assert gc.exact_in_fp32(W, X, q), (c.id, kind, fam)
                    want = gc.expected(_layer_case(c, li), W, X, b)
                    assert _exact_in_dtype(want, c.dt) and np.isfinite(want).all()
                    y16 = gc.round_dt(X @ W.T, c.dt)
                    assert np.array_equal(want, y16 if b is None else gc.round_dt(y16 + b.reshape(1, -1), c.dt)), (c.id, kind, fam)
                    if fam == "onehot" and b is None:   # a one-hot row reads one weight: the output IS the code, no rounding at all
                        assert np.array_equal(want, X @ W.T)


def test_probes_cover_every_group_or_every_edge():
    for c in CASES:
        groups = gc.probe_groups(c)
        if c.G <= 64:
            assert groups == list(range(c.G))
        else:
            assert {0, 1, c.G - 2, c.G - 1} <= set(groups) and gc.edges(c), c.id
            for e in gc.edges(c):
                assert {(e - 1) // GS, e // GS} <= set(groups)
        if c.route == "skinny":    # every split edge of every variant is a chunk edge, hence probed on both sides
            for extra in c.variants:
                _, _, ks, cps = g64.sk_choose(c, extra)
                assert all(s * cps * g64.SK_KC in [0] + gc.edges(c) for s in range(ks))
        X = gc.activations(c, "onehot")
        assert X.sum(axis=1).tolist() == [1.0] * X.shape[0] and {int(k) for k in X.argmax(axis=1)} == {k for g in groups for k in (g * GS, (g + 1) * GS - 1)}
        Xg = gc.activations(c, "group")
        assert Xg.shape[0] == len(groups) and (Xg.sum(axis=1) == GS).all()
        La = gc.launches(c, X)
        assert La.shape[1:] == (c.M, c.K) and np.array_equal(La.reshape(-1, c.K)[:X.shape[0]], X)
        # every row of every launch carries a probe and is compared (token tiles 2.., the ragged token tile, row tiles 2..4 of the skinny kernel included)
        for fam in FAMILIES:
            Xf = gc.activations(c, fam)
            idx = gc.launch_index(c, Xf.shape[0])
            assert len(idx) == -(-Xf.shape[0] // c.M) * c.M and set(idx.tolist()) == set(range(Xf.shape[0])), (c.id, fam)
            assert np.array_equal(gc.launches(c, Xf).reshape(-1, c.K), Xf[idx]) and (Xf[idx].sum(axis=1) > 0).all()
        if X.shape[0] >= c.M:      # the rows of one launch are distinct wherever the probe set has enough rows
            assert all(len({r.tobytes() for r in launch}) == c.M for launch in La[:-1])


# ---- injectivity ---------------------------------------------------------------------------------------------------------------------
def test_codes_separate_every_probed_group_from_the_groups_a_wrong_index_would_reach():
    for c in CASES:
        for li, N in enumerate(c.Ns):
            G = c.G
            assert G < gc.P_CODE or G % gc.P_CODE, c.id            # neighbours in the same row: any two groups less than 61 apart differ (code is 1 + r mod 61) ...
            d = [G]                                                 # ... the same group of the next row
            if c.layout == "c3":
                step = -(-N * G // 10)
                d += [t * step for t in range(1, 10)]               # the ten group rows that share a packed word
            else:
                d += [s * (N // c.per) * G for s in range(1, c.per)]   # the same group of the other slab rows of the packed row
            for v in d:
                assert v % gc.P_CODE, (c.id, N, v)
        assert len({(17 * li) % gc.P_CODE for li in range(len(c.Ns))}) == len(c.Ns)
    for nbits in (8, 4, 3, 2, 1):   # the level code: a = 3, b = 5 odd -> the next k and the next row carry another level at every width
        assert 3 % 2 ** nbits and 5 % 2 ** nbits


# ---- the restated group index and its mutants --------------------------------------------------------------------------------------------
def _runs(L, c):
    for extra in c.variants:
        yield extra, (g64.gemm_plan(L, c, extra) if c.route == "gemm_pipe" else None)


def test_the_restated_group_index_reproduces_the_closed_form(L):
    n = 0
    for c in CASES:
        if c.factored or max(c.Ns) * c.K > 1 << 20:
            continue
        for li in range(len(c.Ns)):
            for extra, plan in _runs(L, _layer_case(c, li)) if c.route == "gemm_pipe" else [(e, None) for e in c.variants]:
                for kind in ("scale", "level"):
                    W = gc.coded_layer(c, kind, li)[3]
                    assert np.array_equal(g64.restated_weights(c, kind, li, None, extra, plan), W), (c.id, li, extra, kind)
                    n += 1
    assert n > 500


@pytest.mark.parametrize("mutant", sorted(g64.MUTANTS))
def test_every_mutant_of_the_group_index_is_caught(L, mutant):
    cid, extra = CATCHES[mutant]
    c = g64.BY_ID[cid]
    assert extra == 0 or extra in c.variants, (cid, extra)
    plan = g64.gemm_plan(L, c, extra) if c.route == "gemm_pipe" else None
    caught = []
    for kind in KINDS:
        W = gc.coded_layer(c, kind)[3]
        Wm = g64.restated_weights(c, kind, 0, mutant, extra, plan)
        for fam in FAMILIES:
            X = gc.activations(c, fam)
            if not np.array_equal(gc.expected(c, Wm, X, gc.coded_bias(c)), gc.expected(c, W, X, gc.coded_bias(c))):
                caught.append((kind, fam))
    assert caught, (mutant, cid)
    assert any(fam == "onehot" for _, fam in caught), (mutant, caught)      # ... and named: a one-hot row gives the group and the row
    assert set(CATCHES) == set(g64.MUTANTS)
