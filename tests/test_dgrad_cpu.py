"""CPU tests of the backward-through-weights entry point (hqq_hip_gemm_dgrad, include/hqq_hip.h): the symbols, the coverage answer on a hand-written
table, and the refusal of every uncovered call before anything launches."""
import pytest
import torch

F32, F16, BF16 = 0, 1, 2
UNSUPPORTED = -4

# (nbits, M, N, K, group_size, dtype) -> covered
COVERED = [
    (4, 1, 64, 128, 64, F16),
    (8, 17, 16, 64, 16, F16),
    (2, 130, 64, 256, 256, BF16),
    (4, 33, 11008, 4096, 64, F16),
    (2, 65, 4096, 11008, 64, BF16),
    (8, 3, 48, 192, 16, BF16),
    (2, 17, 96, 192, 16, F16),      # 24 packed rows: a multiple of 8, not of 16
]
# each coverage rule broken once
REFUSED = [
    (3, 8, 64, 128, 64, F16, b"3-bit"),
    (1, 8, 64, 128, 64, F16, b"1-bit"),
    (4, 8, 64, 96, 32, F16, b"K % 64 == 0"),
    (4, 8, 24, 128, 64, F16, b"N % 16 == 0"),
    (4, 8, 64, 192, 24, F16, b"group_size % 16 == 0"),
    (4, 8, 64, 128, 64, F32, b"fp32"),
    (4, 0, 64, 128, 64, F16, b"at least 1 row"),
]


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    return _C.lib()


def test_symbols_load_and_abi_is_unchanged(L):
    from hqq_amd import _C
    assert "hqq_hip_gemm_dgrad" in _C.SYMBOLS and "hqq_hip_gemm_dgrad_covers" in _C.SYMBOLS
    assert hasattr(L, "hqq_hip_gemm_dgrad") and hasattr(L, "hqq_hip_gemm_dgrad_covers")
    assert L.hqq_hip_abi_version() == 9 and _C.ABI_VERSION == 9


def test_covers_table(L):
    from hqq_amd import ops
    TD = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
    for nbits, M, N, K, gs, dt in COVERED:
        assert L.hqq_hip_gemm_dgrad_covers(nbits, M, N, K, gs, dt) == 1, (nbits, M, N, K, gs, dt)
        assert ops.gemm_dgrad_covers(TD[dt], M, N, K, gs, nbits) is True
    for nbits, M, N, K, gs, dt, _ in REFUSED:
        assert L.hqq_hip_gemm_dgrad_covers(nbits, M, N, K, gs, dt) == 0, (nbits, M, N, K, gs, dt)
        assert ops.gemm_dgrad_covers(TD[dt], M, N, K, gs, nbits) is False


def test_uncovered_calls_are_refused_before_any_launch(L):
    P = 4096   # aligned and never read: each of these calls is refused before anything launches
    for nbits, M, N, K, gs, dt, text in REFUSED:
        assert L.hqq_hip_gemm_dgrad(nbits, P, P, P, P, P, M, N, K, gs, dt, None) == UNSUPPORTED, (nbits, M, N, K, gs, dt)
        assert text in L.hqq_hip_last_error(), L.hqq_hip_last_error()
    # null pointers are fine for a refused call
    assert L.hqq_hip_gemm_dgrad(3, None, None, None, None, None, 8, 64, 128, 64, F16, None) == UNSUPPORTED


def test_route_cut_off_is_declared():
    from hqq_amd import ops
    from hqq_amd.core.quantize import HQQLinear
    assert isinstance(ops.DGRAD_ROUTE_MAX_M, int) and ops.DGRAD_ROUTE_MAX_M >= 0
    assert HQQLinear.fused_backward is True
