"""CPU side of the axis-0 kernel for 17..256 rows (hqq_hip_gemm_axis0): argument checks before any launch, workspace sizes as host arithmetic,
the Python coverage predicate, and the names of the decode kernel that keep their 16-row limit."""
import torch

P16 = 16   # a 16-byte aligned stand-in pointer: every call below must be refused before anything touches it
HEAD = 256 << 10   # the decode workspace's counter head (csrc/hqq_common.h), left untouched by this kernel


def _L():
    from hqq_amd import _C
    return _C.lib()


def _call(nbits=4, M=32, N=256, K=1024, gs=64, dtype=1, opts=0, ws_bytes=1 << 30, x=P16, ws=P16):
    return _L().hqq_hip_gemm_axis0(nbits, x, P16, P16, P16, None, P16, M, N, K, gs, dtype, opts, ws, ws_bytes, None)


def _ws(nbits, M, N, K, gs, dtype):
    return _L().hqq_hip_gemm_axis0_workspace_bytes(nbits, M, N, K, gs, dtype)


def _err():
    return _L().hqq_hip_last_error()


def test_bad_arguments_are_refused_before_any_launch():
    assert _call(M=16) == -4 and b"not covered" in _err()                    # the decode kernel's rows
    assert _call(M=257) == -4 and b"not covered" in _err()                   # past the cap
    assert _call(M=0) == -2
    assert _call(nbits=3) == -4 and b"not covered" in _err()                 # 3-bit containers
    assert _call(dtype=0) == -4 and b"not covered" in _err()                 # fp32
    assert _call(nbits=8, dtype=2) == -4 and b"not covered" in _err()        # bf16 covers 4 / 2 bits
    assert _call(nbits=1, dtype=2) == -4 and b"not covered" in _err()
    assert _call(nbits=5) == -1 and _call(dtype=7) == -3
    assert _call(gs=48) == -4 and b"not covered" in _err()                   # group_size does not divide N = 256
    assert _call(gs=40, N=320) == -4 and b"not covered" in _err()            # group_size % 16 != 0
    assert _call(K=1000) == -4 and b"not covered" in _err()                  # K % 64 != 0
    assert _call(opts=1 << 15) == -2 and b"option" in _err()                 # unknown option bits
    assert _call(x=24) == -6                                                 # misaligned activation
    assert _call(ws_bytes=0) == -5 and _call(ws=None) == -5                  # the workspace is never optional
    assert _call(ws_bytes=_ws(4, 32, 256, 1024, 64, 1) - 1) == -5            # one byte short
    assert _call(N=1 << 23, K=1024) == -2 and b"size overflow" in _err()     # (N / 2) * K packed bytes: one past 32-bit offsets
    assert _call(M=256, N=1 << 22, K=1 << 16, gs=16, nbits=1) == -2 and b"size overflow" in _err()   # 2^22 columns x 2^16: packed bytes, meta and 256 rows of partial sums are all past 32-bit offsets
    assert b"hqq_hip_gemm_axis0" in _err()


def test_workspace_is_host_arithmetic():
    one = _ws(4, 17, 4096, 4096, 64, 1)
    assert one > HEAD
    assert _ws(4, 17, 4096, 4096, 64, 2) == one                              # the plan does not look at the dtype
    # non-decreasing in M over the whole range
    sizes = [_ws(4, M, 4096, 4096, 64, 1) for M in range(17, 257)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and all(s > HEAD for s in sizes)
    # within one 64-row pass count the partial-sum area is proportional to M
    for lo, hi in [(17, 64), (65, 128), (129, 192), (193, 256)]:
        per_row = (_ws(4, lo, 4096, 4096, 64, 1) - HEAD) // lo
        assert per_row > 0 and per_row % (4 * 4096) == 0
        for M in range(lo, hi + 1):
            assert _ws(4, M, 4096, 4096, 64, 1) - HEAD == per_row * M, M
    # 64 rows of a 4096 x 4096 int4 layer: the partial sums are no larger than the packed weights
    assert _ws(4, 64, 4096, 4096, 64, 1) - HEAD <= 4096 * 4096 // 2
    # uncovered configurations need nothing (the call itself refuses them)
    for args in [(3, 32, 4096, 4096, 64, 1), (4, 16, 4096, 4096, 64, 1), (4, 257, 4096, 4096, 64, 1), (4, 0, 4096, 4096, 64, 1),
                 (4, 32, 4096, 4096, 64, 0), (4, 32, 4096, 4000, 64, 1), (4, 32, 4000, 4096, 64, 1), (8, 32, 4096, 4096, 64, 2),
                 (1, 32, 4096, 4096, 64, 2), (4, 32, 256, 1024, 48, 1), (4, 32, 320, 1024, 40, 1), (4, 32, 1 << 23, 1024, 64, 1)]:
        assert _ws(*args) == 0, args


def test_gemm_axis0_covers_truth_table():
    from hqq_amd import ops
    assert ops.GEMM_AXIS0_MAX_M == 256 and 16 <= ops.AXIS0_GEMM_ROUTE_MAX_M <= ops.GEMM_AXIS0_MAX_M
    f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32
    yes = [(f16, 17, 4096, 4096, 64, 4), (f16, 256, 4096, 4096, 64, 8), (f16, 33, 256, 1024, 16, 1), (f16, 64, 256, 1024, None, 2),
           (bf16, 65, 4096, 11008, 64, 4), (bf16, 100, 1024, 8192, 128, 2), (f16, 256, 8192, 28672, 64, 4), (f16, 17, 96, 128, 48, 4)]
    no = [(f16, 16, 4096, 4096, 64, 4), (f16, 1, 4096, 4096, 64, 4), (f16, 257, 4096, 4096, 64, 4), (f16, 0, 4096, 4096, 64, 4),
          (f16, 32, 4096, 4096, 64, 3), (f32, 32, 4096, 4096, 64, 4), (bf16, 32, 4096, 4096, 64, 8), (bf16, 32, 4096, 4096, 64, 1),
          (f16, 32, 4096, 4096, 48, 4), (f16, 32, 4096, 4096, 8, 4), (f16, 32, 4096, 4032 + 32, 64, 4), (f16, 32, 100, 1024, None, 4)]
    no += [(f16, 32, 1 << 23, 1024, 64, 4), (f16, 256, 1 << 22, 1 << 16, 16, 1)]   # past 32-bit offsets
    yes += [(f16, 256, 256000, 4096, 64, 4)]                                          # a vocabulary-sized layer stays within them
    for args in yes:
        assert ops.gemm_axis0_covers(*args), args
    for args in no:
        assert not ops.gemm_axis0_covers(*args), args
    # the library agrees on every case (its workspace query is 0 exactly where it refuses)
    code = {f16: 1, bf16: 2, f32: 0}
    for dt, M, N, K, gs, nb in yes + no:
        got = _ws(nb, M, N, K, N if gs is None else gs, code[dt]) > 0
        assert got == ops.gemm_axis0_covers(dt, M, N, K, gs, nb), (dt, M, N, K, gs, nb)


def test_the_decode_kernels_names_keep_their_row_limit():
    from hqq_amd import ops
    assert not ops.decode_axis0_covers(torch.float16, 17, 4096, 4096, 64, 4)
    assert not ops.axis0_grouped_covers(torch.float16, 17, [4096, 4096], 4096, 64, 4)
    L = _L()
    assert L.hqq_hip_gemv_axis0(4, P16, P16, P16, P16, None, P16, 17, 256, 1024, 64, 1, 0, P16, 1 << 30, None) == -4 and b"not covered" in _err()
    assert L.hqq_hip_gemv_axis0_workspace_bytes(4, 17, 4096, 4096, 64, 1) == 0
    assert L.hqq_hip_abi_version() == 9
