"""The backward-through-weights kernel (hqq_hip_gemm_dgrad, csrc/gemm_dgrad.hip) on the GPU: bit-exact one-hot rows against the dequantise kernel,
the double-accumulated oracle on reference-exact weights, full-size layers, row independence, determinism, bounds, graph capture, and the autograd
route of HQQLinear onto it."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CODE = {torch.float16: 1, torch.bfloat16: 2}
COMBOS = [(8, torch.float16), (4, torch.float16), (2, torch.float16), (4, torch.bfloat16), (2, torch.bfloat16)]
# (N, K, gs): an even / odd number of 16-row n tiles per slab, an odd number of 64-wide k tiles, several groups per lane range of 64 k (gs 16),
# one group per row (gs = K)
SHAPES = [(64, 128, 64), (96, 192, 16), (128, 256, 128), (64, 256, 256)]
BARS = {torch.float16: dict(rtol=1e-3, atol=1e-3), torch.bfloat16: dict(rtol=2.0 ** -7, atol=2e-3)}   # tests/test_axis0_gemm_gpu.py


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from hqq_amd import ops as o
    assert o.is_available(), "libhqq_hip.so must load on the GPU box (no fallback)"
    return o


def _bf16_round(a32: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), returned as float32"""
    u = np.ascontiguousarray(a32, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def _raw(a32: np.ndarray, dt):
    """float32 values of the dtype -> what the oracle takes (np.float16 / raw bf16 bits)"""
    return a32.astype(np.float16) if dt == torch.float16 else (np.ascontiguousarray(a32, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _ref_weights(oracle, nbits, P, s, z, N, K, gs, dt):
    """Quantizer.dequantize of an axis-1 layer on the host: unpack the [N, K] level matrix, (U - zero) * scale per group of gs along k with one
    rounding to the compute dtype per op.  Returns float32 values of the dtype."""
    U = oracle.unpack(nbits, P).reshape(N, K // gs, gs)
    s32, z32 = s.float().numpy().reshape(N, K // gs, 1), z.float().numpy().reshape(N, K // gs, 1)
    if dt == torch.float16:
        W = ((U.astype(np.float16) - z32.astype(np.float16)) * s32.astype(np.float16)).astype(np.float32)
    else:
        W = _bf16_round(_bf16_round(U.astype(np.float32) - z32) * s32)
    return W.reshape(N, K)


@functools.lru_cache(maxsize=4)
def _layer(oracle, nbits, dt, N, K, gs, seed):
    """one layer per configuration, built once: packed bytes [N / per, K] + meta on the device, the reference-exact weights on the host (read-only).
    Random levels; positive scales that keep the weights of the order of 1e-2 at every width; zero-points over the whole level range, for bf16 some
    far below one level (q - z must still round once)."""
    g = torch.Generator().manual_seed(seed)
    C = N * K // gs
    U = torch.randint(0, 2 ** nbits, (N, K), generator=g, dtype=torch.uint8).numpy()
    s = ((torch.rand(C, generator=g) * 0.004 + 0.001) * (16.0 / 2 ** nbits if nbits == 8 else 1.0)).to(dt)
    z = (torch.rand(C, generator=g) * (2 ** nbits - 1)).to(dt)
    if dt == torch.bfloat16:
        z[::5] = 0.00836
        z[1::11] = 2.0 ** -12
    P = oracle.pack(nbits, U)
    assert P.shape == (N * nbits // 8, K)
    Wd = _ref_weights(oracle, nbits, P, s, z, N, K, gs, dt)
    return torch.from_numpy(np.ascontiguousarray(P)).cuda(), s.cuda(), z.cuda(), Wd


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("N,K,gs", SHAPES)
@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_one_hot_rows_are_the_dequantised_weight_bit_for_bit(ops, oracle, nbits, dt, N, K, gs):
    """g = I (M = N rows): dx is every row of every slab at every k, one exact product each; the host weights say the same"""
    P, s, z, Wd = _layer(oracle, nbits, dt, N, K, gs, seed=nbits + N + K + gs)
    W = ops.dequantize(P, s, z, N, K, gs, nbits)
    assert torch.equal(W.float().cpu(), torch.from_numpy(Wd))
    dx = ops.gemm_dgrad(torch.eye(N, dtype=dt, device="cuda"), P, s, z, N, K, gs, nbits)
    assert dx.dtype == dt and tuple(dx.shape) == (N, K)
    assert torch.equal(_bits(dx), _bits(W))
    for M in (17, 65):   # the same rows at the edges of the 16-row tiles of a zero matrix
        rows = sorted({r for r in (0, 15, 16, 17, M - 1) if r < M})
        ns = [(7 * r + 3) % N for r in rows]
        g = torch.zeros(M, N, dtype=dt, device="cuda")
        g[rows, ns] = 1
        want = torch.zeros(M, K, dtype=dt, device="cuda")
        want[rows] = W[ns]
        assert torch.equal(_bits(ops.gemm_dgrad(g, P, s, z, N, K, gs, nbits)), _bits(want)), M


def _want(oracle, g, Wd, dt):
    yo, _ = oracle.matmul(_raw(g.float().numpy(), dt), _raw(np.ascontiguousarray(Wd.T), dt), None, CODE[dt])
    return torch.from_numpy(yo.astype(np.float32)) if dt == torch.float16 else torch.from_numpy((yo.astype(np.uint32) << 16).view(np.float32))


def _check_vs_oracle(ops, oracle, nbits, dt, N, K, gs, Ms, seed):
    P, s, z, Wd = _layer(oracle, nbits, dt, N, K, gs, seed)
    g = torch.randn(max(Ms), N, generator=torch.Generator().manual_seed(seed + 1)).to(dt)
    want = _want(oracle, g, Wd, dt)   # (the oracle's rows are independent: its first M rows are its answer for g[:M])
    for M in Ms:
        dx = ops.gemm_dgrad(g[:M].cuda(), P, s, z, N, K, gs, nbits)
        assert dx.dtype == dt and tuple(dx.shape) == (M, K)
        torch.testing.assert_close(dx.float().cpu(), want[:M], **BARS[dt], msg=lambda m: f"M={M}: {m}")


@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_dgrad_vs_oracle(ops, oracle, nbits, dt):
    """every ragged and full last row tile, one and several 64-row blocks, on (N, K) = (128, 256), gs 64"""
    _check_vs_oracle(ops, oracle, nbits, dt, 128, 256, 64, [1, 15, 16, 17, 33, 65, 130], seed=nbits * 10 + 1)


@pytest.mark.parametrize("nbits,dt,N,K,M", [(4, torch.float16, 11008, 4096, 33), (2, torch.bfloat16, 4096, 11008, 65)])
def test_dgrad_full_size_vs_oracle(ops, oracle, nbits, dt, N, K, M):
    """full-size layers: 32-bit offsets at real shapes"""
    _check_vs_oracle(ops, oracle, nbits, dt, N, K, 64, [M], seed=N + K + nbits)


@pytest.mark.parametrize("nbits,dt", [(4, torch.float16), (2, torch.bfloat16)])
def test_rows_are_independent_and_calls_deterministic(ops, oracle, nbits, dt):
    N, K, gs = 128, 256, 64
    P, s, z, _ = _layer(oracle, nbits, dt, N, K, gs, seed=nbits * 10 + 1)
    g = torch.randn(130, N, generator=torch.Generator().manual_seed(5)).to(dt).cuda()
    full = ops.gemm_dgrad(g, P, s, z, N, K, gs, nbits)
    assert torch.equal(_bits(full), _bits(ops.gemm_dgrad(g, P, s, z, N, K, gs, nbits)))
    for M in (1, 16, 17, 64, 65, 129):
        assert torch.equal(_bits(ops.gemm_dgrad(g[:M], P, s, z, N, K, gs, nbits)), _bits(full[:M])), M


def test_output_stays_inside_its_rows(ops, oracle):
    """the output is the middle of a sentinel-filled buffer: the rows either side are untouched (M = 17: a ragged second tile)"""
    N, K, gs, M = 128, 256, 64, 17
    P, s, z, _ = _layer(oracle, 4, torch.float16, N, K, gs, seed=41)
    g = torch.randn(M, N, generator=torch.Generator().manual_seed(6)).to(torch.float16).cuda()
    buf = torch.full((M + 64, K), 777.0, dtype=torch.float16, device="cuda")
    out = buf[32:32 + M]
    got = ops.gemm_dgrad(g, P, s, z, N, K, gs, 4, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:32] == 777.0).all()) and bool((buf[32 + M:] == 777.0).all())
    assert torch.equal(_bits(out), _bits(ops.gemm_dgrad(g, P, s, z, N, K, gs, 4)))


def test_uncovered_calls_raise(ops, oracle):
    P, s, z, _ = _layer(oracle, 4, torch.float16, 128, 256, 64, seed=41)
    with pytest.raises(NotImplementedError):
        ops.gemm_dgrad(torch.zeros(0, 128, dtype=torch.float16, device="cuda"), P, s, z, 128, 256, 64, 4)


def test_graph_capture_replays_the_eager_result(ops, oracle):
    N, K, gs, M = 128, 256, 64, 33
    P, s, z, _ = _layer(oracle, 4, torch.float16, N, K, gs, seed=41)
    g = torch.randn(M, N, generator=torch.Generator().manual_seed(7)).to(torch.float16).cuda()
    eager = ops.gemm_dgrad(g, P, s, z, N, K, gs, 4)
    out = torch.zeros(M, K, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemm_dgrad(g, P, s, z, N, K, gs, 4, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))


# ---- the autograd route of HQQLinear ----
def _hqq_layer(nbits, bias, dt=torch.float16):
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    torch.manual_seed(nbits + int(bias))
    return HQQLinear(torch.nn.Linear(256, 128, bias=bias), BaseQuantizeConfig(nbits=nbits, group_size=64), compute_dtype=dt, device="cuda")


def _backward(layer, x0):
    x = x0.clone().requires_grad_(True)
    y = layer(x)
    y.retain_grad()
    y.float().square().sum().backward()
    return x.grad, y.grad


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", [(5, 256), (2, 9, 256)])
def test_autograd_takes_the_fused_kernel_when_routed(ops, monkeypatch, shape, bias):
    from hqq_amd.core.quantize import HQQLinear
    monkeypatch.setattr(ops, "DGRAD_ROUTE_MAX_M", 1 << 30)
    layer = _hqq_layer(4, bias)
    if bias:
        layer.bias = layer.bias.detach().requires_grad_(True)   # (HQQLinear keeps its bias as a plain tensor: a leaf here)
    x0 = torch.randn(*shape, generator=torch.Generator().manual_seed(8)).to(torch.float16).cuda()
    xg, go = _backward(layer, x0)
    m = layer.meta
    assert tuple(xg.shape) == shape and xg.dtype == torch.float16
    assert torch.equal(_bits(xg), _bits(ops.gemm_dgrad(go, layer.W_q, m["scale"], m["zero"], 128, 256, 64, 4)))
    want = (go.double() @ layer.dequantize().double()).float()
    torch.testing.assert_close(xg.float(), want, **BARS[torch.float16])
    if bias:   # the bias gradient path is unchanged
        assert torch.equal(layer.bias.grad, go.reshape(-1, 128).sum(0))
    # the switch: the same call with the route off is dequantise + matmul, bit for bit
    monkeypatch.setattr(HQQLinear, "fused_backward", False)
    xg_off, go_off = _backward(layer, x0)
    assert torch.equal(_bits(go_off), _bits(go))
    assert torch.equal(_bits(xg_off), _bits(torch.matmul(go, layer.dequantize())))


def test_autograd_keeps_todays_route_for_3bit_layers(ops, monkeypatch):
    monkeypatch.setattr(ops, "DGRAD_ROUTE_MAX_M", 1 << 30)
    layer = _hqq_layer(3, False)
    x0 = torch.randn(5, 256, generator=torch.Generator().manual_seed(9)).to(torch.float16).cuda()
    xg, go = _backward(layer, x0)
    assert torch.equal(_bits(xg), _bits(torch.matmul(go, layer.dequantize())))
