"""CPU side of the axis-0 decode kernel (hqq_hip_gemv_axis0): argument checks before any launch, workspace sizes as host arithmetic,
the Python coverage predicate, the layout identity the kernel rests on, and the refusals of the code that reads axis-1 meta."""
import ctypes

import numpy as np
import pytest
import torch

P16 = 16   # a 16-byte aligned stand-in pointer: every call below must be refused before anything touches it


def _L():
    from hqq_amd import _C
    return _C.lib()


def _call(nbits=4, M=1, N=256, K=1024, gs=64, dtype=1, opts=0, ws_bytes=1 << 30, x=P16, ws=P16):
    return _L().hqq_hip_gemv_axis0(nbits, x, P16, P16, P16, None, P16, M, N, K, gs, dtype, opts, ws, ws_bytes, None)


def _err():
    return _L().hqq_hip_last_error()


def test_bad_arguments_are_refused_before_any_launch():
    assert _call(opts=1 << 15) == -2 and b"option" in _err()                 # unknown option bits
    assert _call(nbits=3) == -4 and b"not covered" in _err()                 # 3-bit containers
    assert _call(dtype=0) == -4 and b"not covered" in _err()                 # fp32
    assert _call(nbits=8, dtype=2) == -4 and b"not covered" in _err()        # bf16 covers 4 / 2 bits
    assert _call(nbits=5) == -1 and _call(dtype=7) == -3
    assert _call(gs=48) == -4 and b"not covered" in _err()                   # group_size does not divide N = 256
    assert _call(gs=40, N=320) == -4 and b"not covered" in _err()            # group_size % 16 != 0
    assert _call(K=1000) == -4 and b"not covered" in _err()                  # K % 64 != 0
    assert _call(M=17) == -4 and b"not covered" in _err()                    # more rows than the decode kernel takes
    assert _call(M=0) == -2
    assert _call(N=1 << 23, K=1024) == -2 and b"size overflow" in _err()     # (N / 2) * K packed bytes: one past 32-bit offsets
    assert _call(x=24) == -6                                                 # misaligned activation
    assert _call(ws_bytes=0) == -5 and _call(ws=None) == -5                  # the workspace is never optional


def test_workspace_is_host_arithmetic():
    L = _L()
    head = 256 << 10   # the decode workspace's counter head (csrc/hqq_common.h), left untouched by this kernel
    one = L.hqq_hip_gemv_axis0_workspace_bytes(4, 1, 4096, 4096, 64, 1)
    assert one > head and (one - head) % (4 * 4096) == 0
    # the K split depends on the shape only: the partial sums grow with the rows, the split count stays
    assert L.hqq_hip_gemv_axis0_workspace_bytes(4, 16, 4096, 4096, 64, 1) - head == 16 * (one - head)
    assert L.hqq_hip_gemv_axis0_workspace_bytes(4, 1, 4096, 4096, 64, 2) == one
    # uncovered configurations need nothing (the call itself refuses them)
    for args in [(3, 1, 4096, 4096, 64, 1), (4, 17, 4096, 4096, 64, 1), (4, 1, 4096, 4096, 64, 0), (4, 1, 4096, 4000, 64, 1), (4, 1, 4000, 4096, 64, 1)]:
        assert L.hqq_hip_gemv_axis0_workspace_bytes(*args) == 0, args


def test_decode_axis0_covers_truth_table():
    from hqq_amd import ops
    f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32
    yes = [(f16, 1, 4096, 4096, 64, 4), (f16, 16, 4096, 4096, 64, 8), (f16, 7, 256, 1024, 16, 1), (f16, 1, 256, 1024, None, 2),
           (bf16, 4, 4096, 11008, 64, 4), (bf16, 1, 1024, 8192, 128, 2), (f16, 1, 8192, 28672, 64, 4), (f16, 2, 96, 128, 48, 4)]
    no = [(f16, 17, 4096, 4096, 64, 4), (f16, 0, 4096, 4096, 64, 4), (f16, 1, 4096, 4096, 64, 3), (f32, 1, 4096, 4096, 64, 4),
          (bf16, 1, 4096, 4096, 64, 8), (bf16, 1, 4096, 4096, 64, 1), (f16, 1, 4096, 4096, 48, 4), (f16, 1, 4096, 4096, 8, 4),
          (f16, 1, 4096, 4032 + 32, 64, 4), (f16, 1, 100, 1024, None, 4)]
    for args in yes:
        assert ops.decode_axis0_covers(*args), args
    for args in no:
        assert not ops.decode_axis0_covers(*args), args
    # the library agrees on every case (its workspace query is 0 exactly where it refuses)
    code = {f16: 1, bf16: 2, f32: 0}
    for dt, M, N, K, gs, nb in yes + no:
        got = _L().hqq_hip_gemv_axis0_workspace_bytes(nb, M, N, K, N if gs is None else gs, code[dt]) > 0
        assert got == ops.decode_axis0_covers(dt, M, N, K, gs, nb), (dt, M, N, K, gs, nb)


@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("gs", [16, 64, 128, None])
def test_axis0_container_holds_the_axis1_bytes(oracle, nbits, gs):
    """BitPack of the level matrix viewed as [gs, N K / gs] (axis 0) and as [N K / gs, gs] (axis 1) gives the same bytes: the axis-0 kernel
    streams the axis-1 kernels' weight layout and only indexes the meta differently"""
    N, K = 256, 192
    g = gs or N
    L = np.random.default_rng(nbits * 1000 + g).integers(0, 2 ** nbits, (N, K), dtype=np.uint8)
    a0 = oracle.pack(nbits, L.reshape(g, -1))
    a1 = oracle.pack(nbits, L.reshape(-1, g))
    assert a0.tobytes() == a1.tobytes()
    # and byte n K + k (n < N / per) holds W[n + j N / per, k] in slab j, slab 0 most significant
    per = 8 // nbits
    B = a0.reshape(N // per, K)
    for j in range(per):
        assert np.array_equal((B >> (8 - nbits * (j + 1))) & (2 ** nbits - 1), L[j * N // per:(j + 1) * N // per])


def test_code_that_reads_axis1_meta_refuses_axis0_layers():
    from hqq_amd import shard
    W = torch.zeros(128, 64, dtype=torch.uint8)
    s = torch.ones(1, 128 * 128 // 64, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="axis 1"):
        shard.shard_packed(W, s, s, None, 128, 128, 64, 4, 0, 2, axis=0)
    with pytest.raises(NotImplementedError, match="axis 1"):
        shard.ShardedHQQForward(W, s, s, None, 128, 128, 64, 4, axis=0)
