"""CPU tests of the route planner (hqq_hip_forward_route, include/hqq_hip.h "Routes"): every host-side query of the library, and the Python
predicates over it, follow from the one route the planner gives a call."""
import ctypes
import itertools

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    return _C.lib()


F16, BF16, F32 = 1, 2, 0
W3S, FACTORED = 1024, 1
MS = [1, 2, 4, 5, 8, 9, 16, 17, 32, 64, 65, 128, 2048, 2561]
NS = [4096, 11008, 1024, 333, 176]
KS = [4096, 11008, 28672, 4160, 176]
CASES = [(4, 0), (2, 0), (8, 0), (1, 0), (3, 0), (3, W3S)]
SPLIT_K_ROUTES = (6, 4, 7)   # HQQ_ROUTE_SKINNY, _GEMV3_SLABS, _GEMM_PIPE: the kernels that park partial sums


def _route(L, nbits, Ns, M, K, gs, dt, opts):
    return L.hqq_hip_forward_route(nbits, len(Ns), (ctypes.c_int64 * len(Ns))(*Ns), M, K, gs, dt, opts)


def test_route_codes_match_the_python_names(L):
    from hqq_amd import ops
    assert (ops.ROUTE_ROWWISE, ops.ROUTE_SKINNY, ops.ROUTE_GEMM_PIPE, ops.ROUTE_GEMM_TILE) == (1, 6, 7, 8)
    assert _route(L, 4, [4096], 1, 4096, 64, F16, 0) == ops.ROUTE_ROWWISE
    assert _route(L, 3, [4096], 1, 4096, 64, F16, W3S) == ops.ROUTE_ROWWISE_W3S
    assert _route(L, 4, [4096], 8, 4096, 128, F16, 0) == ops.ROUTE_MFMA16
    assert _route(L, 4, [4096], 32, 4096, 64, F16, 0) == ops.ROUTE_SKINNY
    assert _route(L, 4, [4096, 1024, 1024], 8, 4096, 64, F16, 0) == ops.ROUTE_SKINNY
    assert _route(L, 4, [4096, 1024, 1024], 8, 4096 + 256, 64, F16, 0) == ops.ROUTE_SKINNY
    assert _route(L, 4, [4096, 333], 8, 4096, 64, F16, 0) == -4                         # 333 rows are no 4-bit layer: the group is refused whole
    assert b"needs N % 2 == 0" in L.hqq_hip_last_error()
    assert _route(L, 4, [4096], 512, 4096, 64, F16, 0) == ops.ROUTE_GEMM_PIPE
    assert _route(L, 4, [4096], 512, 4096, 128, F16, 0) == ops.ROUTE_GEMM_TILE
    assert _route(L, 3, [4096], 1, 4096, 64, F16, 0) in (ops.ROUTE_GEMV3_ROWS, ops.ROUTE_GEMV3_SLABS)
    assert _route(L, 3, [8192], 2, 28672, 64, F16, 0) == ops.ROUTE_GEMV3_SLABS          # 19 MB and more of packed weights
    assert _route(L, 3, [4096], 1, 4096, 64, F16, 4) == ops.ROUTE_GEMV3_ROWS            # HQQ_OPT_GEMV3_ROWWISE


def test_refusals_carry_the_launch_errors(L):
    P = 4096   # aligned and never read: each of these calls is refused before anything launches
    for nbits, M, N, K, gs, dt, opts, code, text in [
            (5, 1, 64, 64, 64, F16, 0, -4, b"not covered"),
            (4, 1, 64, 64, 64, F16, 1 << 15, -2, b"unknown option bits"),
            (4, 1, 64, 64, 64, F16, W3S, -2, b"3-bit layout"),
            (4, 8, 64, 176, 16, F16, 0, -4, b"K % 64 == 0"),
            (2, 8, 4096, 4096, 128, BF16, 0, -4, b"bf16 covers"),
            (3, 8, 4096, 4096, 64, F16, 0, -4, b"nbits=3 not covered by the fused GEMM"),
            (3, 2, 8, 4096, 64, F16, 0, -4, b"fewer than 10 output rows"),
            (4, 512, 4096, 4096, 128, BF16, 0, -4, b"fp16 only"),
            (4, 512, 4096, 4000, 64, F16, 0, -2, b"bad M/N/K/group_size")]:
        assert _route(L, nbits, [N], M, K, gs, dt, opts) == code
        assert text in L.hqq_hip_last_error()
        assert L.hqq_hip_forward(nbits, P, P, P, P, None, P, M, N, K, gs, dt, opts, None, 0, None) == code
        assert text in L.hqq_hip_last_error()
    # a group the pipelined GEMM cannot take whole
    Ns = (ctypes.c_int64 * 2)(4096, 333)
    assert _route(L, 4, [4096, 333], 128, 4096, 64, F16, 0) == -4 and b"every layer of the group" in L.hqq_hip_last_error()
    assert L.hqq_hip_gemm_grouped_covers(4, 2, Ns, 128, 4096, 64, F16, 0) == 0


@pytest.mark.parametrize("nbits,layout", CASES)
def test_every_query_follows_from_the_route(L, nbits, layout):
    out = (ctypes.c_int * 8)()
    for dt, gs, mode, K, N, M in itertools.product((F16, BF16, F32), (64, 128), (0, FACTORED), KS, NS, MS):
        opts = mode | layout
        r = _route(L, nbits, [N], M, K, gs, dt, opts)
        N1 = (ctypes.c_int64 * 1)(N)
        fwd_ws = L.hqq_hip_forward_workspace_bytes(nbits, M, N, K, gs, dt, opts)
        assert fwd_ws == 0 or r in SPLIT_K_ROUTES, (nbits, M, N, K, gs, dt, opts, r)
        # the decode entry plans the same call the same way where hqq_hip_forward sends it there
        if 0 < r < 7:
            assert L.hqq_hip_gemv_workspace_bytes(nbits, 1, N1, M, K, gs, dt, opts) == fwd_ws
        # the GEMM entry: its plan, its workspace and the grouped query agree with the route
        gemm_pipe = L.hqq_hip_gemm_plan(nbits, M, N, K, gs, dt, opts, out) == 0
        assert gemm_pipe == (L.hqq_hip_gemm_grouped_covers(nbits, 1, N1, M, K, gs, dt, opts) == 1)
        assert (L.hqq_hip_gemm_workspace_bytes(nbits, M, N, K, gs, dt, opts) > 0) <= gemm_pipe
        if r >= 7:
            assert gemm_pipe == (r == 7)
            assert L.hqq_hip_gemm_grouped_workspace_bytes(nbits, 1, N1, M, K, gs, dt, opts) == fwd_ws
        # the speed hint: the decode rows always; beyond, the skinny route, or the pipelined one while it wins
        if not layout and dt != F32:
            pf = L.hqq_hip_forward_prefers_fused(nbits, M, N, K, gs, dt)
            r0 = _route(L, nbits, [N], M, K, gs, dt, 0)
            assert pf == 1 if M <= 16 else (pf == 1) <= (r0 in (6, 7))


@pytest.mark.parametrize("nbits,layout", CASES)
def test_python_wrappers_ask_the_query(L, nbits, layout):
    from hqq_amd import ops
    from hqq_amd.utils.llama_fused import batch_covers
    w3s = bool(layout)
    for dtype, dt in ((torch.float16, F16), (torch.bfloat16, BF16)):
        for gs, K, N, M in itertools.product((64, 128), KS, NS, MS):
            r = _route(L, nbits, [N], M, K, gs, dt, layout)
            assert ops.route(dtype, M, (N,), K, gs, nbits, layout) == r
            assert ops.skinny_covers(dtype, M, N, K, gs, nbits, w3s) == (r == ops.ROUTE_SKINNY)
            if not w3s:
                assert ops.decode_covers(dtype, M, N, K, gs, nbits) == (M <= 16 and 0 < r < 7 and not (r == ops.ROUTE_SKINNY and dtype == torch.bfloat16))
            assert batch_covers(dtype, M, [(N, K, gs, nbits, w3s)] * 2) == (0 < r < 7)
            assert ops.gemm_grouped_covers(dtype, [N, N], M, K, gs, nbits, layout) == (_route(L, nbits, [N, N], max(M, 65), K, gs, dt, layout) == 7)
