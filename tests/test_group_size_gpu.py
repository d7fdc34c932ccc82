"""The generic group-size bodies of the fused forward kernels on the GPU (cases, constructed layers and references: tests/_gs_cases.py; what the
CPU side proves about them: tests/test_group_size_cpu.py).  Every case goes through hqq_amd.ops and the C ABI.

Coded layers: the output bits must EQUAL the closed form — a wrong group index shows as another group's code.  The randn layer: the one-hot
columns equal the dequantise kernel's, and the result meets the bars the project already uses for the same quantity (named where applied)."""
import numpy as np
import pytest
import torch

import _gs_cases as gc
from _gs_cases import CASES, FAMILIES, KINDS

pytestmark = pytest.mark.gpu

EXACT_CASES = [c for c in CASES if not c.factored]
ids = lambda cs: [c.id for c in cs]   # noqa: E731


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from hqq_amd import ops as o
    assert o.is_available(), "libhqq_hip.so must load on the GPU box (no fallback)"
    return o


def _device_layer(oracle, c, U, s, z, b, N):
    """(W_q, scale, zero, bias, N) as the entry points take them; U uint8 [N G, gs] on the host, the rest tensors of the dtype"""
    P = oracle.pack(c.nbits, np.ascontiguousarray(U)).reshape(N // c.per, c.K)
    return (torch.from_numpy(P).cuda(), s.reshape(-1, 1).cuda(), z.reshape(-1, 1).cuda(), None if b is None else b.cuda(), N)


def _call(ops, c, layers, x, opts, grouped=None):
    """one launch: x [M, K] through the case's entry point; the outputs of its layers"""
    if c.route == "gemm_tile":
        Wq, s, z, b, N = layers[0]
        return [ops.gemm(x, Wq, s, z, b, N, c.K, c.gs, c.nbits, opts=opts)]
    if c.grouped if grouped is None else grouped:
        return ops.gemv_grouped(x, layers, c.K, c.gs, c.nbits, opts=opts)
    return [ops.gemv(x, Wq, s, z, b, N, c.K, c.gs, c.nbits, opts=opts) for (Wq, s, z, b, N) in layers]


def _rows(ops, c, layers, X, opts, grouped=None):
    """the rows of X [rows, K] (host, fp64 values of the dtype) in launches of M: per layer [rows, N]"""
    La = gc.tensor(gc.launches(c, X), c.dt).cuda()
    outs = [_call(ops, c, layers, La[i], opts, grouped) for i in range(La.shape[0])]
    return [torch.cat([o[li] for o in outs])[:X.shape[0]] for li in range(len(layers))]


def _mismatch(c, y, want, what):
    bad = (y != want).nonzero()
    r, n = (int(v) for v in bad[0])
    return f"{c.id} {what}: {bad.shape[0]} of {y.numel()} outputs differ; first at row {r}, n {n} (packed row {n % (y.shape[1] // c.per)}, slab {n // (y.shape[1] // c.per)}): got {float(y[r, n])}, want {float(want[r, n])}"


@pytest.mark.parametrize("c", EXACT_CASES, ids=ids(EXACT_CASES))
def test_coded_layers_equal_their_closed_form(ops, oracle, c):
    """scale-, zero- and level-coded layers x one-hot rows, group indicators and all ones: torch.equal with the fp64 closed form rounded once (+ once
    for the bias), with opts as the case has them and with OPT_META_SCALABLE where the meta check accepts every layer; a grouped launch also
    equals its per-layer calls bit for bit"""
    for kind in KINDS:
        host = [gc.coded_layer(c, kind, li) for li in range(len(c.Ns))]
        layers = []
        for li, (U, s, z, W, q) in enumerate(host):
            b = gc.coded_bias(c, li)
            layers.append(_device_layer(oracle, c, U, gc.tensor(s, c.dt), gc.tensor(z, c.dt), None if b is None else gc.tensor(b, c.dt), c.Ns[li]))
        variants = [c.opts]
        if c.dt == "f16" and all(ops.meta_scalable(s, z, N, c.K, c.gs, c.nbits) for (_, s, z, _, N) in layers):
            variants.append(c.opts | gc.OPT_META_SCALABLE)
        for fam in FAMILIES:
            X = gc.activations(c, fam)
            wants = [gc.tensor(gc.expected(c, host[li][3], X, gc.coded_bias(c, li)), c.dt).cuda() for li in range(len(layers))]
            for opts in variants:
                ys = _rows(ops, c, layers, X, opts)
                for li, (y, want) in enumerate(zip(ys, wants)):
                    assert y.dtype == want.dtype and y.shape == want.shape
                    assert torch.equal(y, want), _mismatch(c, y, want, f"{kind}-coded layer {li}, {fam}, opts {opts}")
            if c.grouped:
                for y, y1 in zip(ys, _rows(ops, c, layers, X, variants[-1], grouped=False)):
                    assert torch.equal(y, y1), _mismatch(c, y, y1, f"{kind}-coded, {fam}: grouped vs per-layer")


@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
def test_the_three_op_form_runs_on_coded_layers(ops, nbits):
    """the coded layers pass hqq_hip_meta_check at every width (integer zeros up to 61, scales of at most 61 / 16), so the test above runs the
    three-op rebuild of the row-per-wave kernel on all three kinds of every fp16 case"""
    c = next(c for c in EXACT_CASES if c.route == "rowwise" and c.dt == "f16" and c.nbits == nbits)
    for kind in KINDS:
        _, s, z, _, _ = gc.coded_layer(c, kind)
        assert ops.meta_scalable(gc.tensor(s, "f16").cuda(), gc.tensor(z, "f16").cuda(), c.Ns[0], c.K, c.gs, nbits), (c.id, kind)


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_randn_layer_against_the_fp64_reference(ops, oracle, c):
    """_random_layer's meta and randn x against dequantise + double-accumulated matmul on the host; one-hot rows against the dequantise kernel's
    columns; grouped == per-layer, M = 1 == row 0 of M rows (row-per-wave kernel), the same call twice == the same bits"""
    host = [gc.random_layer(c, li) for li in range(len(c.Ns))]
    layers = [_device_layer(oracle, c, U.numpy(), s, z, b, c.Ns[li]) for li, (U, s, z, b) in enumerate(host)]
    x = gc.random_x(c)
    xd = x.cuda()
    ys = _call(ops, c, layers, xd, c.opts)
    Wdevs = []
    for li, ((U, s, z, b), (Wq, sd, zd, bd, N), y) in enumerate(zip(host, layers, ys)):
        Wd = gc.reference_weights(oracle, c, oracle.pack(c.nbits, U.numpy()), s, z, li)
        want = torch.from_numpy(gc.reference_forward(oracle, c, Wd, x, b))
        got = y.float().cpu()
        assert y.dtype == gc.DT[c.dt] and tuple(y.shape) == (c.M, N)
        err = (got.double() - want.double()).abs()
        print(f"{c.id} layer {li}: max abs err {float(err.max()):.3e}, max |y| {float(want.abs().max()):.3e}")
        if c.factored:
            # the bound of tests/test_round3_gpu.py::test_factored_arithmetic_against_the_reference_outputs: at most 2^-8 from the reference's
            # y, at most max(2, outputs / 200) of them beyond rtol = atol = 1e-3
            beyond = int((err > 1e-3 + 1e-3 * want.double().abs()).sum())
            assert float(err.max()) <= 2 ** -8 + 1e-6 and beyond <= max(2, y.numel() // 200), (c.id, float(err.max()), beyond)
        elif c.dt == "bf16":     # tests/test_axis0_decode_gpu.py::_check_vs_oracle
            torch.testing.assert_close(got, want, rtol=2.0 ** -7, atol=2e-3)
        elif c.route == "gemm_tile":   # tests/test_hip_parity.py::test_gemm_vs_oracle
            torch.testing.assert_close(got, want, rtol=1e-3, atol=2e-3)
        else:                    # tests/test_hip_parity.py::test_gemv_vs_oracle; 8-bit: ::test_gemv_8bit_1bit_vs_oracle
            torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3 * (16 if c.nbits == 8 else 1))
        if not c.factored:
            # the fused kernel's weights ARE the dequantise kernel's: y[n] = W[n, k] for a one-hot row, at the first and last k of every probed group
            Wdevs.append(ops.dequantize(Wq, sd.reshape(-1), zd.reshape(-1), N, c.K, c.gs, c.nbits))
            assert np.array_equal(Wdevs[-1].float().cpu().numpy(), Wd), (c.id, "dequantise kernel vs host")
    for li, (y, y2) in enumerate(zip(ys, _call(ops, c, layers, xd, c.opts))):
        assert torch.equal(y, y2), (c.id, li, "the same call twice")
    if c.grouped:
        for li, (y, y1) in enumerate(zip(ys, _call(ops, c, layers, xd, c.opts, grouped=False))):
            assert torch.equal(y, y1), _mismatch(c, y, y1, f"randn layer {li}: grouped vs per-layer")
    if c.route == "rowwise" and c.M > 1 and not c.factored:
        for li, (y, y1) in enumerate(zip(ys, _call(ops, c, layers, xd[:1].contiguous(), c.opts))):
            assert torch.equal(y[:1], y1), _mismatch(c, y[:1], y1, f"randn layer {li}: M = 1 vs row 0 of M = {c.M}")
    if not c.factored:
        X = gc.activations(c, "onehot")
        ks = torch.from_numpy(X.argmax(axis=1)).cuda()
        nobias = [(Wq, s, z, None, N) for (Wq, s, z, _, N) in layers]
        for li, y in enumerate(_rows(ops, c, nobias, X, c.opts)):
            cols = Wdevs[li][:, ks].t().contiguous()
            assert torch.equal(y, cols), _mismatch(c, y, cols, f"randn layer {li}: one-hot rows vs dequantise columns")
