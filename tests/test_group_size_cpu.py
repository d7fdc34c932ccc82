"""CPU side of the generic group-size cases (tests/_gs_cases.py): the planner gives every case the route the table claims and asks for no
workspace; the closed forms are what the packed bytes dequantise to and exact as claimed; the grid reaches the edges its docstring names; the
codes tell neighbouring groups and the slabs of a packed row apart."""
import ctypes

import numpy as np
import pytest
import torch

import _gs_cases as gc
from _gs_cases import CASES, FAMILIES, KINDS


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    return _C.lib()


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _layer_case(c, li):
    return c if not c.grouped else gc.Case(c.route, c.nbits, c.dt, c.opts, c.M, (c.Ns[li],), c.K, c.gs, c.bias)


# ---- routes --------------------------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_route_the_table_claims_and_needs_no_workspace(L):
    from hqq_amd import ops
    assert (ops.ROUTE_ROWWISE, ops.ROUTE_MFMA16, ops.ROUTE_GEMM_TILE) == (gc.ROUTE_ROWWISE, gc.ROUTE_MFMA16, gc.ROUTE_GEMM_TILE)
    assert (ops.OPT_FACTORED, ops.OPT_META_SCALABLE, ops.OPT_GEMM_REGTILE, ops.OPT_GEMM_CLASSIC) == (gc.OPT_FACTORED, gc.OPT_META_SCALABLE, gc.OPT_GEMM_REGTILE, gc.OPT_GEMM_CLASSIC)
    for c in CASES:
        want, dt = gc.WANT_ROUTE[c.route], gc.CODE[c.dt]
        assert c.gs != 64 and c.gs % gc.LANE_K == 0 and c.K % c.gs == 0, c.id
        for opts in {c.opts, c.opts | (gc.OPT_META_SCALABLE if c.dt == "f16" else 0)}:
            assert ops.route(gc.DT[c.dt], c.M, tuple(c.Ns), c.K, c.gs, c.nbits, opts) == want, (c.id, opts, L.hqq_hip_last_error())
            if c.route == "gemm_tile":
                assert not c.grouped
                assert L.hqq_hip_gemm_workspace_bytes(c.nbits, c.M, c.Ns[0], c.K, c.gs, dt, opts) == 0, c.id
                assert L.hqq_hip_forward_workspace_bytes(c.nbits, c.M, c.Ns[0], c.K, c.gs, dt, opts) == 0, c.id
            else:
                assert L.hqq_hip_gemv_workspace_bytes(c.nbits, len(c.Ns), _i64(c.Ns), c.M, c.K, c.gs, dt, opts) == 0, c.id
                for N in c.Ns:   # the per-layer calls a grouped case is compared with
                    assert L.hqq_hip_forward_route(c.nbits, 1, _i64([N]), c.M, c.K, c.gs, dt, opts) == want, (c.id, N)


def test_the_table_holds_what_the_route_table_allows():
    by = lambda r: [c for c in CASES if c.route == r]   # noqa: E731
    exact = [c for c in by("rowwise") if not c.factored]
    assert {(c.nbits, c.dt) for c in exact} == set(gc.ROWWISE_COMBOS)
    for combo in gc.ROWWISE_COMBOS:
        assert {c.M for c in exact if (c.nbits, c.dt) == combo and not c.grouped} == {1, 2, 3, 4}, combo
    assert {c.M for c in by("rowwise") if c.factored} == set(gc.MFMA_MS) and all(c.M > 4 for c in by("rowwise") if c.factored)
    for nbits in (8, 4, 2, 1):
        assert {c.M for c in by("mfma16") if c.nbits == nbits and not c.grouped} == set(gc.MFMA_MS), nbits
    assert {(c.nbits, c.dt) for c in by("gemm_tile")} == {(4, "f16"), (2, "f16")}
    for nbits in (4, 2):
        for opts in (0, gc.OPT_GEMM_REGTILE, gc.OPT_GEMM_CLASSIC):
            assert {c.M for c in by("gemm_tile") if c.nbits == nbits and c.opts == opts} >= ({17} if opts == gc.OPT_GEMM_REGTILE else set()) | set(gc.GEMM_MS)
    assert all(N % 8 == 0 for c in CASES if c.nbits == 1 for N in c.Ns)
    for r in ("rowwise", "mfma16"):   # a grouped launch of different N at gs 128 and at gs 16
        grouped = [c for c in by(r) if c.grouped]
        assert {128, 16} <= {c.gs for c in grouped} and all(len(set(c.Ns)) == len(c.Ns) >= 2 for c in grouped)


# ---- grid reach ----------------------------------------------------------------------------------------------------------------------
def test_the_grid_reaches_the_edges_it_names():
    rw = [c for c in CASES if c.route == "rowwise" and not c.factored and not c.grouped]
    for combo in gc.ROWWISE_COMBOS:
        cs = [c for c in rw if (c.nbits, c.dt) == combo]
        gss = {c.gs for c in cs}
        assert {16, 32, 48, 80, 96, 128, 256, gc.GV_KSTEP, gc.GV_UNIT} <= gss, combo
        # every residue of a group edge against the lane chunks of a 64-k block that gs % 16 == 0 allows: edges at 16, 32, 48 (mod 64)
        res = {(g * c.gs) % gc.GM_BLOCK for c in cs for g in range(1, c.G)}
        assert res == {0, 16, 32, 48}, (combo, res)
        # ... and an odd / even 16-k chunk on either side of an edge (the lane's k0 / 16)
        assert {(g * c.gs // gc.LANE_K) % 2 for c in cs for g in range(1, c.G)} == {0, 1}
        assert any(c.gs == c.K and c.K & (c.K - 1) for c in cs) and any(c.gs == c.K == gc.LANE_K for c in cs)
        assert any(c.gs == c.K and c.K > gc.GV_UNIT for c in cs)                                   # one group spans units
        assert any(c.K < gc.GV_KSTEP and c.K % 64 for c in cs) and any(c.K == gc.GV_KSTEP for c in cs)
        assert any(gc.GV_UNIT < c.K < gc.GV_UNIT + gc.GV_KSTEP and (c.K - gc.GV_UNIT) % gc.LANE_K == 0 for c in cs)
        assert any(c.K > gc.GV_NF * gc.GV_UNIT and c.K % gc.GV_UNIT for c in cs)
        assert any(c.K > 3 * gc.GV_UNIT and c.Ns[0] // c.per * 4 <= 16 * 16 for c in cs)            # the K-split: nunits >= GV_WAVES, few rows
        assert {c.Ns[0] // c.per for c in cs} >= set(gc.ROWWISE_ROWS) and 1 in gc.ROWWISE_ROWS
    for dt in ("f16", "bf16"):
        assert any(c.dt == dt and c.Ns[0] // c.per > gc.CUS * 4 * gc.GV_WAVES for c in rw)          # a wave's second row
    mf = [c for c in CASES if c.route == "mfma16" and not c.grouped]
    for nbits in (8, 4, 2, 1):
        cs = [c for c in mf if c.nbits == nbits]
        assert {16, 32, 48, 80, 96, 128, 256} <= {c.gs for c in cs} and all(c.K % 192 == 0 for c in cs if c.gs in (48, 96))
        assert any(0 < (g * c.gs) % gc.GM_BLOCK for c in cs for g in range(1, c.G))               # an edge inside a 64-k block
        assert any(c.K == gc.GM_BLOCK for c in cs) and any(c.K // gc.GM_BLOCK % 2 == 1 and c.K > gc.GM_BLOCK for c in cs)
        assert any(c.gs == c.K and c.K & (c.K - 1) for c in cs)
        shares = {}
        for c in cs:
            sl = gc.gm_slices(nbits, c.K, -(-(c.Ns[0] // c.per) // gc.GM_ROWS))
            n = [b - a for a, b in sl]
            # gm_launch gives a tile at most K / 128 waves: no slice is ever empty, and a one-block slice exists only at K = 64
            assert min(n) >= 1 and (min(n) >= 2 or c.K == gc.GM_BLOCK), c.id
            shares[c.id] = n
        cap = min(32 // gc.PER[nbits], 16)
        assert any(len(n) == cap and len(set(n)) > 1 for n in shares.values()), nbits          # the most waves a tile gets, uneven shares
        assert any(len(n) == 1 and n[0] == 1 for n in shares.values())                          # one block
        assert any(1 in {v % 2 for v in n} and 0 in {v % 2 for v in n} for n in shares.values())   # whole units and a half-dead one side by side
        assert {c.Ns[0] // c.per for c in cs} >= set(gc.MFMA_ROWS)
    big = [c for c in mf if -(-(c.Ns[0] // c.per) // gc.GM_ROWS) > gc.gm_grid_cap(c.nbits, c.K, -(-(c.Ns[0] // c.per) // gc.GM_ROWS))]
    assert big, "a workgroup of the 16-row-tile kernel takes a second tile"
    gm = [c for c in CASES if c.route == "gemm_tile"]
    for nbits in (4, 2):
        for opts in (0, gc.OPT_GEMM_REGTILE, gc.OPT_GEMM_CLASSIC):
            cs = [c for c in gm if c.nbits == nbits and c.opts == opts]
            assert any(c.K == gc.GB_K for c in cs) and any(c.K > 2 * gc.GB_K for c in cs)
            assert any(0 < (g * c.gs) % gc.GB_K for c in cs for g in range(1, c.G))
            assert all(c.K % gc.GB_K == 0 and c.Ns[0] % (4 * c.per) == 0 for c in cs)
        rt = [c for c in gm if c.nbits == nbits and gc.reaches_regtile(c)]
        assert rt and any(c.gs < gc.GB_K for c in rt), "the register-tile kernel itself runs, with a group edge inside its K tile"
        assert all((c.Ns[0] // c.per) % (gc.GB_N // c.per) and (c.Ns[0] // c.per) % gc.RT_ROWS for c in gm if c.nbits == nbits)   # ragged N tiles
    assert 100 < len(CASES) < 600


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def _exact_in_dtype(a, dt):
    a = np.asarray(a, np.float64)
    if dt == "bf16" and not np.array_equal(a.astype(np.float32).astype(np.float64), a):
        return False
    return np.array_equal(gc.round_dt(a, dt), a)


@pytest.mark.parametrize("route,nbits,dt", sorted({(c.route, c.nbits, c.dt) for c in CASES}))
def test_closed_forms_are_what_the_packed_bytes_dequantise_to_and_exact(oracle, route, nbits, dt):
    """per case, layer and kind: meta and weights exact in the dtype; oracle.dequantize of the packed bytes IS the closed-form W; every partial sum of
    every activation family a float32-exact dyadic number; expected() equals the correctly rounded fp64 product computed from the dequantised weights"""
    for c in CASES:
        if (c.route, c.nbits, c.dt) != (route, nbits, dt) or c.factored:
            continue
        for li in range(len(c.Ns)):
            for kind in KINDS:
                U, s, z, W, q = gc.coded_layer(c, kind, li)
                for a in (s, z, W):
                    assert _exact_in_dtype(a, c.dt), (c.id, kind)
                assert int(U.max()) < 2 ** c.nbits
                N = c.Ns[li]
                P = oracle.pack(c.nbits, U)
                assert P.shape == (N // c.per, c.K) or P.size == N // c.per * c.K
                Wd = oracle.from_cd(oracle.dequantize(c.nbits, P, gc.raw(s, c.dt), gc.raw(z, c.dt), N, c.K, c.gs, gc.CODE[c.dt]), gc.CODE[c.dt])
                assert np.array_equal(Wd.astype(np.float64), W), (c.id, kind)
                b = gc.coded_bias(c, li)
                assert b is None or _exact_in_dtype(b, c.dt)
                for fam in FAMILIES:
                    X = gc.activations(c, fam)
                    assert gc.exact_in_fp32(W, X, q), (c.id, kind, fam)
                    want = gc.expected(_layer_case(c, li), W, X, b)
                    y = X @ Wd.astype(np.float64).T
                    assert _exact_in_dtype(want, c.dt) and np.isfinite(want).all()
                    y16 = gc.round_dt(y, c.dt)
                    assert np.array_equal(want, y16 if b is None else gc.round_dt(y16 + b.reshape(1, -1), c.dt)), (c.id, kind, fam)
                    if fam == "onehot" and b is None:   # a one-hot row reads one weight: the output IS the code, no rounding at all
                        assert np.array_equal(want, y)


def test_probes_cover_every_group_or_every_edge():
    for c in CASES:
        groups = gc.probe_groups(c)
        if c.G <= 64:
            assert groups == list(range(c.G))
        else:
            assert {0, 1, c.G - 2, c.G - 1} <= set(groups)
            for e in gc.edges(c):
                assert {(e - 1) // c.gs, e // c.gs} <= set(groups)
            assert gc.edges(c), c.id
        X = gc.activations(c, "onehot")
        assert X.sum(axis=1).tolist() == [1.0] * X.shape[0] and {int(k) for k in X.argmax(axis=1)} == {k for g in groups for k in (g * c.gs, (g + 1) * c.gs - 1)}
        Xg = gc.activations(c, "group")
        assert Xg.shape[0] == len(groups) and (Xg.sum(axis=1) == c.gs).all()
        La = gc.launches(c, X)
        assert La.shape[1:] == (c.M, c.K) and np.array_equal(La.reshape(-1, c.K)[:X.shape[0]], X)


# ---- injectivity ---------------------------------------------------------------------------------------------------------------------
def test_codes_tell_neighbouring_groups_and_the_slabs_of_a_packed_row_apart():
    r = np.arange(4 * gc.P_CODE)
    cd = gc.code(r)
    assert cd.min() == 1 and cd.max() == gc.P_CODE
    for w in range(1, gc.P_CODE):   # any two groups less than 61 apart carry different codes
        assert (cd[w:] != cd[:-w]).all()
    for c in CASES:
        for li, N in enumerate(c.Ns):
            rps = N // c.per
            # the same group of another slab row of the packed row (a wrong row_off / slab stride), and of the next packed row
            for d in [s * rps * c.G for s in range(1, c.per)] + [c.G]:
                assert d % gc.P_CODE, (c.id, N, d)
        # layers of a grouped launch: the same (row, group) of another layer carries another code
        assert len({(17 * li) % gc.P_CODE for li in range(len(c.Ns))}) == len(c.Ns)
    # the level code: a = 3, b = 5 odd -> the next k and the next row carry another level at every width
    for nbits in (8, 4, 2, 1):
        assert 3 % 2 ** nbits and 5 % 2 ** nbits


def test_rounding_helpers():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 65504.0, 3.8125, -0.75])
    assert gc.round_dt(a, "bf16").tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 65536.0, 3.8125, -0.75]
    assert gc.round_dt(np.array([2049.0, 2051.0]), "f16").tolist() == [2048.0, 2052.0]
    for dt in ("f16", "bf16"):
        t = gc.tensor(np.array([3.8125, -0.75, 61.0]), dt)
        assert t.dtype == gc.DT[dt] and t.double().tolist() == [3.8125, -0.75, 61.0]
    assert torch.equal(gc.tensor(np.array([1.5]), "bf16"), torch.tensor([1.5], dtype=torch.bfloat16))
