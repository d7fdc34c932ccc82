"""CPU tests of the axis-0 backward-through-weights entry point (hqq_hip_gemm_dgrad_axis0, include/hqq_hip.h): the symbols, the coverage answer on a
hand-written table, the refusal of every uncovered call before anything launches, the declared routing cut-off, and the index map the kernel rests
on — which constant an element uses and which rows a container byte holds —, proved on the host against the reference's own statement of
Quantizer.dequantize(axis=0).  (Quantizer.quantize / dequantize themselves run on the GPU only here; the CPU oracle's quantize_axis0 restates the
quantiser, and the GPU file checks the same map against the real layer.)"""
import inspect

import numpy as np
import pytest
import torch

F32, F16, BF16 = 0, 1, 2
UNSUPPORTED, SHAPE = -4, -2

# (nbits, M, N, K, group_size, dtype) -> covered
COVERED = [
    (4, 1, 128, 128, 32, F16),
    (2, 17, 96, 192, 32, F16),       # 24 packed rows, Nr = 3
    (8, 3, 192, 64, 16, BF16),
    (4, 130, 64, 256, 64, BF16),     # group_size = N: one meta row
    (4, 33, 11008, 4096, 64, F16),   # Nr = 172
    (2, 65, 4096, 11008, 64, BF16),
    (8, 1 << 20, 256, 128, 16, F16),
    (2, 5, 3648, 64, 16, F16),       # Nr = 228: past the LDS staging, served by global loads
]
# each coverage rule broken once
REFUSED = [
    (3, 8, 128, 128, 32, F16, UNSUPPORTED, b"3-bit"),
    (1, 8, 128, 128, 32, F16, UNSUPPORTED, b"1-bit"),
    (4, 8, 128, 128, 32, F32, UNSUPPORTED, b"fp32"),
    (4, 8, 96, 128, 64, F16, UNSUPPORTED, b"N % group_size == 0"),
    (4, 8, 96, 128, 24, F16, UNSUPPORTED, b"group_size % 16 == 0"),
    (4, 8, 128, 96, 32, F16, UNSUPPORTED, b"K % 64 == 0"),
    (2, 8, 48, 128, 16, F16, UNSUPPORTED, b"N % 32 == 0"),          # N % (8 per): a lane contracts 8 packed rows
    (4, 0, 128, 128, 32, F16, UNSUPPORTED, b"at least 1 row"),
    (8, 8, 1 << 17, 1 << 16, 64, F16, SHAPE, b"size overflow"),     # N K = 2^33 packed bytes
    (2, 8, 1 << 17, 1 << 17, 64, F16, SHAPE, b"size overflow"),     # N K / 4 = 2^32 packed bytes: one past 32-bit offsets
    (4, 1 << 31, 128, 128, 32, F16, SHAPE, b"size overflow"),       # M past a 32-bit row count
]


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    return _C.lib()


def test_symbols_load_and_abi_is_unchanged(L):
    from hqq_amd import _C
    assert "hqq_hip_gemm_dgrad_axis0" in _C.SYMBOLS and "hqq_hip_gemm_dgrad_axis0_covers" in _C.SYMBOLS
    assert hasattr(L, "hqq_hip_gemm_dgrad_axis0") and hasattr(L, "hqq_hip_gemm_dgrad_axis0_covers")
    assert L.hqq_hip_abi_version() == 9 and _C.ABI_VERSION == 9


def test_covers_table(L):
    from hqq_amd import ops
    TD = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
    for nbits, M, N, K, gs, dt in COVERED:
        assert L.hqq_hip_gemm_dgrad_axis0_covers(nbits, M, N, K, gs, dt) == 1, (nbits, M, N, K, gs, dt)
        assert ops.gemm_dgrad_axis0_covers(TD[dt], M, N, K, gs, nbits) is True
    for nbits, M, N, K, gs, dt, _, _ in REFUSED:
        assert L.hqq_hip_gemm_dgrad_axis0_covers(nbits, M, N, K, gs, dt) == 0, (nbits, M, N, K, gs, dt)
        assert ops.gemm_dgrad_axis0_covers(TD[dt], M, N, K, gs, nbits) is False
    # group_size None is one group of N rows
    assert ops.gemm_dgrad_axis0_covers(torch.float16, 5, 64, 256, None, 4) is True
    assert ops.gemm_dgrad_axis0_covers(torch.float16, 5, 72, 256, None, 4) is False   # 72 % 16 != 0


def test_uncovered_calls_are_refused_before_any_launch(L):
    P = 4096   # aligned and never read: each of these calls is refused before anything launches
    for nbits, M, N, K, gs, dt, rc, text in REFUSED:
        assert L.hqq_hip_gemm_dgrad_axis0(nbits, P, P, P, P, P, M, N, K, gs, dt, None) == rc, (nbits, M, N, K, gs, dt)
        assert text in L.hqq_hip_last_error(), L.hqq_hip_last_error()
    # null pointers are fine for a refused call, and refused (nothing launched) on a covered one; so is a misaligned pointer
    assert L.hqq_hip_gemm_dgrad_axis0(3, None, None, None, None, None, 8, 128, 128, 32, F16, None) == UNSUPPORTED
    for hole in range(5):
        ptrs = [P] * 5
        ptrs[hole] = None
        assert L.hqq_hip_gemm_dgrad_axis0(4, *ptrs, 8, 128, 128, 32, F16, None) == SHAPE and b"null" in L.hqq_hip_last_error()
        ptrs[hole] = P + 8
        assert L.hqq_hip_gemm_dgrad_axis0(4, *ptrs, 8, 128, 128, 32, F16, None) == -6 and b"aligned" in L.hqq_hip_last_error()


def test_route_cut_off_is_declared():
    from hqq_amd import ops
    from hqq_amd.core.quantize import HQQLinear
    assert isinstance(ops.DGRAD_AXIS0_ROUTE_MAX_M, int) and ops.DGRAD_AXIS0_ROUTE_MAX_M >= 0
    assert HQQLinear.fused_backward is True and hasattr(HQQLinear, "_dgrad_axis0_kernel_ok")
    src = inspect.getsource(ops)
    at = src.index("\nDGRAD_AXIS0_ROUTE_MAX_M =")
    comment = src[src.rindex("\n\n", 0, at):at]
    assert "profiles/dgrad_axis0_summary.md" in comment and all(l.startswith("#") for l in comment.strip().splitlines())
    assert ops.gemm_dgrad.__name__ == "gemm_dgrad" and ops.DGRAD_ROUTE_MAX_M == 16   # the axis-1 route keeps its name and cut-off


def _bf16_round(a32):
    u = np.ascontiguousarray(a32, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


SHAPES = [(128, 128, 32), (96, 192, 32), (192, 64, 16), (64, 256, None), (256, 128, 16), (3648, 64, 16)]   # tests/test_dgrad_axis0_gpu.py


@pytest.mark.parametrize("N,K,gs", SHAPES)
@pytest.mark.parametrize("nbits", [8, 4, 2])
@pytest.mark.parametrize("code", [F16, BF16])
def test_index_map_on_the_host(oracle, nbits, code, N, K, gs):
    """element (n, k) of dequantize(axis=0) is (U[n, k] - zero.flat[(n % Nr) K + k]) * scale.flat[same], rounded per op; byte [p, k] of the container
    viewed [N / per, K] holds rows p + slab N / per, slab 0 in the most significant bits"""
    g = gs or N
    Nr, per = N // g, 8 // nbits
    W = 0.02 * torch.randn(N, K, generator=torch.Generator().manual_seed(N + K + nbits)).numpy()
    q = oracle.quantize_axis0(W, nbits=nbits, group_size=g)
    Uq = q["Wq"]                                                    # [gs, N K / gs]: the quantiser's own grouping
    s = oracle.from_cd(oracle.to_cd(q["scale"], code), code)        # [1, N K / gs] in the compute dtype, as float32
    z = oracle.from_cd(oracle.to_cd(q["zero"], code), code)
    assert s.shape == (1, Nr * K) and Uq.shape == (g, Nr * K)

    def deq(u, zz, ss):   # (W_q - zero) * scale, one rounding per op in the compute dtype
        if code == F16:
            return ((u.astype(np.float16) - zz.astype(np.float16)) * ss.astype(np.float16)).astype(np.float32)
        return _bf16_round(_bf16_round(u.astype(np.float32) - zz) * ss)

    want = deq(Uq, z, s).reshape(N, K)                               # Quantizer.dequantize: broadcast over the [gs, C] view, then .reshape(shape)
    U = Uq.reshape(N, K)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    idx = (n % Nr) * K + k
    got = deq(U, z.reshape(-1)[idx], s.reshape(-1)[idx])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(idx)) == Nr * K
    # the container: BitPack of the [gs, C] view is the [N / per, K] byte array of rows p + slab N / per
    B = oracle.pack(nbits, Uq)
    assert B.size == (N // per) * K
    B = B.reshape(N // per, K)
    for slab in range(per):
        assert np.array_equal((B >> (8 - nbits * (slab + 1))) & (2 ** nbits - 1), U[slab * N // per:(slab + 1) * N // per])
    # every slab of byte [p, k] shares the meta element (p % Nr, k): N / per is a multiple of Nr
    assert (N // per) % Nr == 0
    p = np.arange(N // per)
    for slab in range(per):
        assert np.array_equal((p + slab * (N // per)) % Nr, p % Nr)
