"""Host-side half of the workspace-contract tests (tests/test_workspace_contract_gpu.py): every case of the shared table really is what the
GPU file means it to be — the intended route, a workspace with a body behind the counter head, more than one K split where a split is
forced, a hybrid plan where one is asked for.  Pure host arithmetic of libhqq_hip.so: no device needed."""
import pytest

import _ws_cases as W


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    return _C.lib()


@pytest.mark.parametrize("c", W.CASES + W.MIXED, ids=lambda c: c.id)
def test_case_takes_its_route_and_parks_sums(L, c):
    assert W.route(L, c) == W.WANT_ROUTE[c.kind], L.hqq_hip_last_error()
    need = W.need(L, c)
    assert need > W.HEAD and need % 16 == 0
    if c.kind == "pipe" and not c.grouped:
        # what the plan parks is what the query asks for: K splits x split tiles x (tokens x packed rows x slabs) fp32 sums behind the head
        nw, bm, n_tiles, m_tiles, ks, kps, full, wgs = W.gemm_plan(L, c)
        assert ks > 1
        per = W._per(c.nbits, bool(c.opts & W.W3S))
        assert need == W.HEAD + ks * (n_tiles * m_tiles - full) * bm * 16 * nw * per * 4
        if c.opts >> 24:
            assert 1 < ks <= c.opts >> 24 and ks * kps >= c.K // 64 > (ks - 1) * kps
        if c.opts & (W.NARROW | W.WIDE) and c.nbits != 2:
            assert (nw, bm) == {W.NARROW: (4, 128), W.WIDE: (8, 128), W.NARROW | W.WIDE: (8, 256)}[c.opts & (W.NARROW | W.WIDE)]
        assert (full > 0) == c.hybrid
        if c.hybrid:
            assert full % 256 == 0 and n_tiles * m_tiles > full


@pytest.mark.parametrize("c", [c for c in W.CASES if c.kind == "skinny"], ids=lambda c: c.id)
def test_skinny_cases_split_k_as_they_say(L, c):
    """the query's size is K splits x panels x one fp32 tile per (panel row, slab, 16-row m-tile): a forced split count is honoured, and the
    counters of every (panel, row group) fit the head"""
    per = W._per(c.nbits, bool(c.opts & W.W3S))
    body = W.need(L, c) - W.HEAD
    nchunks = c.K // 256
    fits = []
    for rows in ((64,) if c.opts & W.SKINNY_WIDE else (32, 64)):   # which tile serves an unforced launch is the planner's tuning, not contract
        panels = sum((N // per + rows - 1) // rows for N in c.Ns)
        tile = rows * per * 16 * ((c.M + 15) // 16) * 4
        ks, rest = divmod(body, panels * tile)
        ok = rest == 0 and 2 <= ks <= nchunks and panels * (rows // 16) * 4 <= W.HEAD
        if ok and c.opts >> 24:
            cps = -(-nchunks // (c.opts >> 24))
            ok = ks == -(-nchunks // cps)
        fits.append(ok)
    assert any(fits), (c.id, body)


def test_the_skinny_grid_reaches_every_edge_it_names():
    sk = [c for c in W.CASES if c.kind == "skinny"]
    assert {(c.M + 15) // 16 for c in sk} == {1, 2, 3, 4}
    assert {(c.nbits, c.dt) for c in sk} == {(b, d) for b in (8, 4, 3, 2) for d in ("f16", "bf16")}
    assert any(c.opts & W.SKINNY_WIDE for c in sk) and any(not c.opts & W.SKINNY_WIDE for c in sk)
    assert any((c.K // 256) % (c.opts >> 24) for c in sk if c.opts >> 24)                  # a split count that does not divide K / 256
    assert any(c.opts >> 24 == c.K // 256 // 2 for c in sk)
    assert any(len(c.Ns) == 3 and len(set(c.Ns)) == 3 for c in sk)
    assert any(c.bias for c in sk) and any(not c.bias for c in sk)


@pytest.mark.parametrize("c", [c for c in W.CASES if c.kind == "gemv3s"], ids=lambda c: c.id)
def test_gemv3s_query_counts_the_tasks(L, c):
    """ten slabs x two segments x M fp32 sums per task of sixteen packed rows"""
    tasks = sum(-(-(-(-N * (c.K // 64) // 10)) // 16) for N in c.Ns)
    assert W.need(L, c) == W.HEAD + tasks * 10 * 2 * c.M * 4


def test_the_gemv3s_grid_reaches_every_edge_it_names():
    g3 = [c for c in W.CASES if c.kind == "gemv3s"]
    assert {c.M for c in g3} == {1, 2, 3, 4}
    G = lambda c: c.K // 64                                                                # noqa: E731
    assert any(G(c) % 16 == 0 for c in g3) and any(G(c) % 16 for c in g3)
    assert any((c.Ns[0] * G(c)) % 10 for c in g3)                                          # a padded last slab
    assert any((-(-c.Ns[0] * G(c) // 10)) % 16 for c in g3)                                # a ragged last task
    assert any(len(c.Ns) == 2 for c in g3) and any(c.opts & W.META_SCALABLE for c in g3)


def test_the_pipe_grid_reaches_every_edge_it_names(L):
    pp = [c for c in W.CASES if c.kind == "pipe"]
    assert {c.M for c in pp if not c.hybrid} == {65, 128, 200, 640}
    assert {(c.nbits, c.dt) for c in pp} >= {(b, d) for b in (8, 4, 3, 2) for d in ("f16", "bf16")}
    assert any(c.hybrid for c in pp) and any(len(c.Ns) == 3 for c in pp)
    assert {c.opts & (W.NARROW | W.WIDE) for c in pp} == {0, W.NARROW, W.WIDE, W.NARROW | W.WIDE}
    assert any(c.opts >> 24 for c in pp) and any(not c.opts >> 24 for c in pp)


@pytest.mark.parametrize("c", [c for c in W.CASES + W.MIXED if c.kind == "axis0" and c.grouped], ids=lambda c: c.id)
def test_axis0_grouped_query_is_the_head_plus_the_members_bodies(L, c):
    """include/hqq_hip.h: "the counter head (untouched) plus the sum of the layers' partial-sum areas" """
    bodies = [int(L.hqq_hip_gemv_axis0_workspace_bytes(c.nbits, c.M, N, c.K, c.gs_eff, W.CODE[c.dt])) - W.HEAD for N in c.Ns]
    assert all(b > 0 for b in bodies)
    assert W.need(L, c) == W.HEAD + sum(bodies)


def test_the_axis0_grid_reaches_every_edge_it_names():
    a0 = [c for c in W.CASES if c.kind == "axis0"]
    assert {(c.nbits, c.dt) for c in a0} == {(8, "f16"), (4, "f16"), (2, "f16"), (1, "f16"), (4, "bf16"), (2, "bf16")}
    assert {c.M for c in a0} == {1, 3, 16} and {c.gs for c in a0} == {16, 64, 128, None}
    assert {len(c.Ns) for c in a0 if c.grouped} >= {2, 3} and any(c.flags & W.BLOCK_SILU for c in a0)


@pytest.mark.parametrize("c", W.ATTN_CASES, ids=lambda c: c.id)
def test_attention_cases_need_a_record_buffer(L, c):
    assert W.attn_need(L, c) == len(c.pos) * c.n_heads * c.splits * (c.hd + 2) * 4 > 0
    assert all(0 <= p < c.L for p in c.pos) and c.n_heads % c.n_kv == 0


def test_the_attention_grid_reaches_every_edge_it_names():
    at = W.ATTN_CASES
    assert {c.splits for c in at} == {3, 8, 16} and {c.hd for c in at} == {64, 128, 256}
    assert {(c.rope, c.batched) for c in at} == {(r, b) for r in (False, True) for b in (False, True)}
    assert any(c.n_heads != c.n_kv for c in at)
    assert any(max(c.pos) < c.splits for c in at) and any(c.L - 1 in c.pos for c in at) and any(len(set(c.pos)) > 2 for c in at)
