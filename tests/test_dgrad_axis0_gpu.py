"""The backward-through-weights kernel of axis-0 layers (hqq_hip_gemm_dgrad_axis0, csrc/gemm_dgrad_axis0.hip) on the GPU, test for test what
tests/test_dgrad_gpu.py asks of the axis-1 kernel: bit-exact one-hot rows against the dequantise kernel and a host restatement of
Quantizer.dequantize(axis=0), the double-accumulated oracle, full-size layers, row independence, determinism, bounds, graph capture, the autograd
route of HQQLinear onto it, and one LoRA training step merged back into an axis-0 layer."""
import functools

import _train_cases as tc
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

CODE = {torch.float16: 1, torch.bfloat16: 2}
COMBOS = [(8, torch.float16), (4, torch.float16), (2, torch.float16), (4, torch.bfloat16), (2, torch.bfloat16)]   # tests/test_dgrad_gpu.py
BARS = {torch.float16: dict(rtol=1e-3, atol=1e-3), torch.bfloat16: dict(rtol=2.0 ** -7, atol=2e-3)}   # tests/test_dgrad_gpu.py
# (N, K, gs) -> Nr = N / gs meta rows: the smallest shapes that reach each way the meta walk can go wrong
SHAPES = [
    (128, 128, 32),     # Nr = 4: a lane's 8 packed rows wrap the meta rows twice
    (96, 192, 32),      # Nr = 3: the wrap is aligned with nothing; an odd number of k tiles; 2-bit: 24 packed rows, a ragged 32-row step
    (192, 64, 16),      # Nr = 12: the wrap falls inside a lane's 8 rows at some steps only; a single k tile
    (64, 256, None),    # Nr = 1: every row reads meta row 0
    (256, 128, 16),     # Nr = 16: no wrap inside a lane
    (3648, 64, 16),     # Nr = 228: the smallest layer whose meta slab does not fit the LDS staging (Nr <= 227; N % 32 == 0 for 2 bits): global loads
]


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


def _ref_weights(U, s, z, N, K, gs, dt):
    """Quantizer.dequantize of an axis-0 layer on the host, as the reference states it: the level matrix viewed [gs, N K / gs], (U - zero) * scale with
    zero / scale [1, N K / gs] broadcast down the rows, one rounding to the compute dtype per op, .reshape(N, K).  Returns float32 values of the dtype."""
    Uv = U.reshape(gs, -1)
    s32, z32 = s.float().numpy().reshape(1, -1), z.float().numpy().reshape(1, -1)
    if dt == torch.float16:
        W = ((Uv.astype(np.float16) - z32.astype(np.float16)) * s32.astype(np.float16)).astype(np.float32)
    else:
        W = _bf16_round(_bf16_round(Uv.astype(np.float32) - z32) * s32)
    return W.reshape(N, K)


@functools.lru_cache(maxsize=4)
def _layer(oracle, nbits, dt, N, K, gs, seed):
    """one layer per configuration, built once: packed bytes [N / per, K] + meta [N K / gs] on the device, the reference-exact weights on the host
    (read-only).  Levels, scales and zero-points as tests/test_dgrad_gpu.py builds them: random levels over the full range; zero-points over the whole
    level range, for bf16 some far below one level (q - z must still round once).  gs: the resolved group size (N for group_size=None)."""
    g = torch.Generator().manual_seed(seed)
    C = N * K // gs
    U = torch.randint(0, 2 ** nbits, (N, K), generator=g, dtype=torch.uint8).numpy()
    s = ((torch.rand(C, generator=g) * 0.004 + 0.001) * (16.0 / 2 ** nbits if nbits == 8 else 1.0)).to(dt)
    z = (torch.rand(C, generator=g) * (2 ** nbits - 1)).to(dt)
    if dt == torch.bfloat16:
        z[::5] = 0.00836
        z[1::11] = 2.0 ** -12
    P = oracle.pack(nbits, U.reshape(gs, -1))   # BitPack of the quantiser's [gs, N K / gs] view: the [N / per, K] byte array
    assert P.size == N * nbits // 8 * K
    Wd = _ref_weights(U, s, z, N, K, gs, dt)
    return torch.from_numpy(np.ascontiguousarray(P)).reshape(N * nbits // 8, K).cuda(), s.cuda(), z.cuda(), Wd


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("N,K,gs", SHAPES)
@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_one_hot_rows_are_the_dequantised_weight_bit_for_bit(ops, oracle, nbits, dt, N, K, gs):
    """g = I (M = N rows): dx is every row of every slab at every k, one exact product each; the host weights say the same"""
    P, s, z, Wd = _layer(oracle, nbits, dt, N, K, gs or N, seed=nbits + N + K + (gs or 0))
    W = ops.dequantize(P, s, z, N, K, gs or N, nbits, 0)
    assert torch.equal(W.float().cpu(), torch.from_numpy(Wd))
    dx = ops.gemm_dgrad_axis0(torch.eye(N, dtype=dt, device="cuda"), P, s, z, N, K, gs, nbits)
    assert dx.dtype == dt and tuple(dx.shape) == (N, K)
    assert torch.equal(_bits(dx), _bits(W))
    for M in (17, 65):   # the same rows at the edges of the 16-row tiles of a zero matrix
        rows = sorted({r for r in (0, 15, 16, 17, M - 1) if r < M})
        ns = [(7 * r + 3) % N for r in rows]
        g = torch.zeros(M, N, dtype=dt, device="cuda")
        g[rows, ns] = 1
        want = torch.zeros(M, K, dtype=dt, device="cuda")
        want[rows] = W[ns]
        assert torch.equal(_bits(ops.gemm_dgrad_axis0(g, P, s, z, N, K, gs, nbits)), _bits(want)), M


@pytest.mark.parametrize("nbits,dt", [(8, torch.bfloat16), (4, torch.float16)])   # (8-bit bf16: covered, and in no other case of this file)
def test_the_largest_staged_layer(ops, oracle, nbits, dt):
    """Nr = 227 = 3632 / 16: the last layer whose meta slab is staged in LDS (its two slabs end 160 bytes short of the 64 KiB buffer); SHAPES holds
    Nr = 228, the first on the other side.  (3632 % 32 != 0: no 2-bit layer has this size)"""
    N, K, gs = 3632, 64, 16
    P, s, z, Wd = _layer(oracle, nbits, dt, N, K, gs, seed=nbits + N)
    W = ops.dequantize(P, s, z, N, K, gs, nbits, 0)
    assert torch.equal(W.float().cpu(), torch.from_numpy(Wd))
    assert torch.equal(_bits(ops.gemm_dgrad_axis0(torch.eye(N, dtype=dt, device="cuda"), P, s, z, N, K, gs, nbits)), _bits(W))


def _want(oracle, g, Wd, dt):
    yo, _ = oracle.matmul(_raw(g.float().numpy(), dt), _raw(np.ascontiguousarray(Wd.T), dt), None, CODE[dt])
    return torch.from_numpy(yo.astype(np.float32)) if dt == torch.float16 else torch.from_numpy((yo.astype(np.uint32) << 16).view(np.float32))


def _check_vs_oracle(ops, oracle, nbits, dt, N, K, gs, Ms, seed):
    P, s, z, Wd = _layer(oracle, nbits, dt, N, K, gs, seed)
    g = torch.randn(max(Ms), N, generator=torch.Generator().manual_seed(seed + 1)).to(dt)
    want = _want(oracle, g, Wd, dt)   # (the oracle's rows are independent: its first M rows are its answer for g[:M])
    for M in Ms:
        dx = ops.gemm_dgrad_axis0(g[:M].cuda(), P, s, z, N, K, gs, nbits)
        assert dx.dtype == dt and tuple(dx.shape) == (M, K)
        torch.testing.assert_close(dx.float().cpu(), want[:M], **BARS[dt], msg=lambda m: f"M={M}: {m}")


@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_dgrad_vs_oracle(ops, oracle, nbits, dt):
    """every ragged and full last row tile, one and several 64-row blocks, on (N, K) = (128, 128), gs 32"""
    _check_vs_oracle(ops, oracle, nbits, dt, 128, 128, 32, [1, 15, 16, 17, 33, 65, 130], seed=nbits * 10 + 1)


@pytest.mark.parametrize("nbits,dt,N,K,M", [(4, torch.float16, 11008, 4096, 33), (2, torch.bfloat16, 4096, 11008, 65)])
def test_dgrad_full_size_vs_oracle(ops, oracle, nbits, dt, N, K, M):
    """full-size layers: 32-bit offsets at real shapes; 11008 / 64 = 172 meta rows, a multiple of neither 8 nor 32"""
    _check_vs_oracle(ops, oracle, nbits, dt, N, K, 64, [M], seed=N + K + nbits)


@pytest.mark.parametrize("nbits,dt", [(4, torch.float16), (2, torch.bfloat16)])
def test_rows_are_independent_and_calls_deterministic(ops, oracle, nbits, dt):
    N, K, gs = 128, 128, 32
    P, s, z, _ = _layer(oracle, nbits, dt, N, K, gs, seed=nbits * 10 + 1)
    g = torch.randn(130, N, generator=torch.Generator().manual_seed(5)).to(dt).cuda()
    full = ops.gemm_dgrad_axis0(g, P, s, z, N, K, gs, nbits)
    assert torch.equal(_bits(full), _bits(ops.gemm_dgrad_axis0(g, P, s, z, N, K, gs, nbits)))
    for M in (1, 16, 17, 64, 65, 129):
        assert torch.equal(_bits(ops.gemm_dgrad_axis0(g[:M], P, s, z, N, K, gs, nbits)), _bits(full[:M])), M


def test_output_stays_inside_its_rows(ops, oracle):
    """the output is the middle of a sentinel-filled buffer: the rows either side are untouched (M = 17: a ragged second tile)"""
    N, K, gs, M = 128, 128, 32, 17
    P, s, z, _ = _layer(oracle, 4, torch.float16, N, K, gs, seed=41)
    g = torch.randn(M, N, generator=torch.Generator().manual_seed(6)).to(torch.float16).cuda()
    buf = torch.full((M + 64, K), 777.0, dtype=torch.float16, device="cuda")
    out = buf[32:32 + M]
    got = ops.gemm_dgrad_axis0(g, P, s, z, N, K, gs, 4, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:32] == 777.0).all()) and bool((buf[32 + M:] == 777.0).all())
    assert torch.equal(_bits(out), _bits(ops.gemm_dgrad_axis0(g, P, s, z, N, K, gs, 4)))


def test_uncovered_and_malformed_calls_raise(ops, oracle):
    P, s, z, _ = _layer(oracle, 4, torch.float16, 128, 128, 32, seed=41)
    with pytest.raises(NotImplementedError):
        ops.gemm_dgrad_axis0(torch.zeros(0, 128, dtype=torch.float16, device="cuda"), P, s, z, 128, 128, 32, 4)
    g = torch.zeros(3, 128, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):   # the meta count of another group size
        ops.gemm_dgrad_axis0(g, P, s, z, 128, 128, 64, 4)
    with pytest.raises(ValueError):   # an output of the wrong size
        ops.gemm_dgrad_axis0(g, P, s, z, 128, 128, 32, 4, out=torch.empty(3, 64, dtype=torch.float16, device="cuda"))


def test_graph_capture_replays_the_eager_result(ops, oracle):
    N, K, gs, M = 128, 128, 32, 33
    P, s, z, _ = _layer(oracle, 4, torch.float16, N, K, gs, seed=41)
    g = torch.randn(M, N, generator=torch.Generator().manual_seed(7)).to(torch.float16).cuda()
    eager = ops.gemm_dgrad_axis0(g, P, s, z, N, K, gs, 4)
    out = torch.zeros(M, K, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemm_dgrad_axis0(g, P, s, z, N, K, gs, 4, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))


# ---- the autograd route of HQQLinear ----
class _Spy:
    """ops.gemm_dgrad_axis0 with its behaviour kept: counts the calls"""

    def __init__(self, fn):
        self.fn, self.n = fn, 0

    def __call__(self, *a, **kw):
        self.n += 1
        return self.fn(*a, **kw)


@pytest.fixture
def spy(ops, monkeypatch):
    s = _Spy(ops.gemm_dgrad_axis0)
    monkeypatch.setattr(ops, "gemm_dgrad_axis0", s)
    return s


def _hqq_layer(nbits, bias, dt=torch.float16, N=128, K=256, gs=32, vaf=False):
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    torch.manual_seed(nbits + int(bias))
    cfg = BaseQuantizeConfig(nbits=nbits, group_size=gs, axis=0, view_as_float=vaf)
    return HQQLinear(nn.Linear(K, N, bias=bias), cfg, compute_dtype=dt, device="cuda")


def _backward(layer, x0):
    x = x0.clone().requires_grad_(True)
    y = layer(x)
    y.retain_grad()
    y.float().square().sum().backward()
    return x.grad, y.grad


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", [(5, 256), (2, 9, 256)])
def test_autograd_takes_the_fused_kernel_when_routed(ops, spy, monkeypatch, shape, bias):
    from hqq_amd.core.quantize import HQQLinear
    monkeypatch.setattr(ops, "DGRAD_AXIS0_ROUTE_MAX_M", 1 << 30)
    layer = _hqq_layer(4, bias)
    if bias:
        layer.bias = layer.bias.detach().requires_grad_(True)   # (HQQLinear keeps its bias as a plain tensor: a leaf here)
    x0 = torch.randn(*shape, generator=torch.Generator().manual_seed(8)).to(torch.float16).cuda()
    xg, go = _backward(layer, x0)
    assert spy.n == 1
    m = layer.meta
    assert tuple(xg.shape) == shape and xg.dtype == torch.float16
    assert torch.equal(_bits(xg), _bits(spy.fn(go, layer.W_q, m["scale"], m["zero"], 128, 256, 32, 4)))
    want = (go.double() @ layer.dequantize().double()).float()
    torch.testing.assert_close(xg.float(), want, **BARS[torch.float16])
    if bias:   # the bias gradient path is unchanged
        assert torch.equal(layer.bias.grad, go.reshape(-1, 128).sum(0))
    # the switch: the same call with the route off is dequantise + matmul, bit for bit
    monkeypatch.setattr(HQQLinear, "fused_backward", False)
    xg_off, go_off = _backward(layer, x0)
    assert spy.n == 1
    assert torch.equal(_bits(go_off), _bits(go))
    assert torch.equal(_bits(xg_off), _bits(torch.matmul(go, layer.dequantize())))


def test_autograd_views_a_float_container_back(ops, spy, monkeypatch):
    monkeypatch.setattr(ops, "DGRAD_AXIS0_ROUTE_MAX_M", 1 << 30)
    layer, plain = _hqq_layer(4, False, vaf=True), _hqq_layer(4, False)
    assert layer.W_q.dtype == torch.float16 and plain.W_q.dtype == torch.uint8
    x0 = torch.randn(5, 256, generator=torch.Generator().manual_seed(8)).to(torch.float16).cuda()
    xg, go = _backward(layer, x0)
    xg_plain, go_plain = _backward(plain, x0)
    assert spy.n == 2 and torch.equal(_bits(go), _bits(go_plain)) and torch.equal(_bits(xg), _bits(xg_plain))


@pytest.mark.parametrize("what", ["3bit", "N % gs != 0", "reference-named backends"])
def test_autograd_keeps_todays_route_elsewhere(ops, spy, monkeypatch, what):
    monkeypatch.setattr(ops, "DGRAD_AXIS0_ROUTE_MAX_M", 1 << 30)
    if what == "3bit":
        layer, K = _hqq_layer(3, False), 256
    elif what == "N % gs != 0":
        layer, K = _hqq_layer(4, False, N=96, K=192, gs=64), 192
    else:
        layer, K = _hqq_layer(4, False), 256
    x0 = torch.randn(5, K, generator=torch.Generator().manual_seed(9)).to(torch.float16).cuda()
    if what == "reference-named backends":
        for name in ("forward_pytorch_backprop", "forward_aten_backprop"):
            x = x0.clone().requires_grad_(True)
            y = getattr(layer, name)(x)
            y.retain_grad()
            y.float().square().sum().backward()
            assert torch.equal(_bits(x.grad), _bits(torch.matmul(y.grad, layer.dequantize())))
    else:
        xg, go = _backward(layer, x0)
        assert torch.equal(_bits(xg), _bits(torch.matmul(go, layer.dequantize())))
    assert spy.n == 0


def test_the_cut_off_splits_the_rows(ops, spy):
    """with the cut-off as the module has it: R rows take the kernel (where R >= 1), R + 1 rows keep dequantise + matmul"""
    R = ops.DGRAD_AXIS0_ROUTE_MAX_M
    layer = _hqq_layer(4, False)
    for rows, calls in ((R, 1 if R >= 1 else 0), (R + 1, 0)):
        if rows == 0:
            continue
        before = spy.n
        x0 = torch.randn(rows, 256, generator=torch.Generator().manual_seed(10)).to(torch.float16).cuda()
        xg, go = _backward(layer, x0)
        assert spy.n - before == calls, (rows, R)
        torch.testing.assert_close(xg.float(), (go.double() @ layer.dequantize().double()).float(), **BARS[torch.float16])


# ---- training: one LoRA step on an axis-0 layer, merged back ----
@pytest.mark.parametrize("dn", list(tc.DTYPES))
def test_lora_step_on_an_axis0_layer_and_merge(ops, spy, monkeypatch, dn):
    from hqq_amd.core.peft import HQQLinearLoRA
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    monkeypatch.setattr(ops, "DGRAD_AXIS0_ROUTE_MAX_M", 1 << 30)
    dt, N, K, gs, M = tc.DTYPES[dn], 128, 256, 32, 9
    cfg = BaseQuantizeConfig(nbits=4, group_size=gs, axis=0)
    lin = nn.Linear(K, N, bias=False)
    lin.weight.data = tc.layer_weight(N, K, seed=N + 4)
    layer = HQQLinear(lin, cfg, compute_dtype=dt, device="cuda")
    lora = HQQLinearLoRA(layer, {"r": tc.LORA_R, "lora_alpha": tc.LORA_ALPHA, "lora_init": tc.lora_init(K, N, 11)})
    S = tc.LORA_ALPHA / tc.LORA_R
    W = layer.dequantize().double().cpu()
    x0, t = tc.randn((M, K), 21, dt).cuda(), tc.randn((M, N), 22).cuda()
    x = x0.clone().requires_grad_(True)
    y = lora(x)
    y.retain_grad()
    (y.float() * t).sum().backward()
    assert spy.n == 1                                             # the wrapper inherits the wrapped layer's route
    A, B = lora.lora_A.detach().cpu(), lora.lora_B.detach().cpu()
    args = (x0.cpu(), y.grad.cpu(), W, A, B, S)
    ref, bnd = tc.ref_lora(*args), tc.bound_lora(*args, dt, torch.float32)
    for name, got in (("A", lora.lora_A.grad), ("B", lora.lora_B.grad), ("x", x.grad)):
        ok, worst = tc.within(got, ref[name], bnd[name])
        assert ok, f"{name}.grad: worst |error| / bound = {worst:.3f}"
    assert layer.W_q.grad is None
    # one optimiser step, then the merge: the new layer is the quantised composition of base weight + adapter, again an axis-0 layer
    torch.optim.SGD([lora.lora_A, lora.lora_B], lr=0.05).step()
    assert not torch.equal(lora.lora_A.detach().cpu(), A) and not torch.equal(lora.lora_B.detach().cpu(), B)
    merged = lora.merge_and_quantize(cfg)
    Wm = layer.dequantize()
    Wm += (torch.matmul(lora.lora_A.data, lora.lora_B.data) * S).t().to(dt)
    want = HQQLinear.from_weights(Wm, None, cfg, compute_dtype=dt, device="cuda")
    assert type(merged) is HQQLinear and merged.meta["axis"] == 0 and torch.equal(merged.W_q, want.W_q)
    for key in ("scale", "zero"):
        assert torch.equal(_bits(merged.meta[key].reshape(-1)), _bits(want.meta[key].reshape(-1))), key
    with torch.no_grad():
        ym = merged(x0)
    torch.testing.assert_close(ym.float(), (x0.double() @ merged.dequantize().double().t()).float(), **BARS[dt])
    before = spy.n
    xm = x0.clone().requires_grad_(True)
    merged(xm).float().mul(t).sum().backward()                     # and the merged layer trains on through the same route
    assert spy.n == before + 1 and bool(torch.isfinite(xm.grad).all())
