"""The group_size = 64 bodies of the fused forward kernels on the GPU (cases, constructed layers, packing and the restated launch rules:
tests/_gs64_cases.py; what the CPU side proves about them: tests/test_gs64_cpu.py).  Every call goes through hqq_amd.ops and the C ABI.

Coded layers: the output bits must EQUAL the closed form, for every option variant of the case (forced tiles and K splits included) and with
OPT_META_SCALABLE where the meta check accepts every layer — a wrong group index shows as another group's code, and the failure names case, kind,
family, row, n, packed row and slab.  3-bit: the container kernels and the stream-layout kernel give the same bits on the same coded levels.
The randn layer: the dequantise kernel's weights equal the host's, the one-hot columns equal the dequantise kernel's, and the result meets the bar the
project already uses for the same route (named where applied); the same call twice gives the same bits on every variant."""
import numpy as np
import pytest
import torch

import _gs_cases as gc
import _gs64_cases as g64
from _gs_cases import FAMILIES, KINDS
from _gs64_cases import CASES, GS

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
    """(W_q, scale, zero, bias, N) as the entry points take them, in the case's layout, and the reference container of a 3-bit layer (host)"""
    Wq, P = g64.pack_layer(oracle, c, U, N)
    return (torch.from_numpy(np.ascontiguousarray(Wq)).cuda(), s.reshape(-1, 1).cuda(), z.reshape(-1, 1).cuda(), None if b is None else b.cuda(), N), P


def _call(ops, c, layers, x, opts, grouped=None):
    """one launch: x [M, K] through the case's entry point; the outputs of its layers"""
    grouped = c.grouped if grouped is None else grouped
    if c.route in g64.GEMM_ROUTES:
        if grouped:
            return ops.gemm_grouped(x, layers, c.K, GS, c.nbits, opts=opts)
        return [ops.gemm(x, Wq, s, z, b, N, c.K, GS, c.nbits, opts=opts) for (Wq, s, z, b, N) in layers]
    if grouped:
        return ops.gemv_grouped(x, layers, c.K, GS, c.nbits, opts=opts)
    return [ops.gemv(x, Wq, s, z, b, N, c.K, GS, c.nbits, opts=opts) for (Wq, s, z, b, N) in layers]


def _rows(ops, c, layers, X, opts, grouped=None):
    """the rows of X [rows, K] (host, fp64 values of the dtype) in whole launches of M: per layer EVERY row of every launch, [n_launches M, N] — row i
    is row gc.launch_index(c, rows)[i] of X (the last launch is filled from the top, and those rows are compared like the others)"""
    La = gc.tensor(gc.launches(c, X), c.dt).cuda()
    outs = [_call(ops, c, layers, La[i], opts, grouped) for i in range(La.shape[0])]
    return [torch.cat([o[li] for o in outs]) for li in range(len(layers))]


def _mismatch(c, y, want, what):
    bad = (y != want).nonzero()
    r, n = (int(v) for v in bad[0])
    N = y.shape[1]
    if c.layout == "c3":
        step = -(-N * c.G // 10)
        where = f"first group row {n * c.G}: slab {n * c.G // step}, packed row {n * c.G % step}"
    else:
        where = f"packed row {n % (N // c.per)}, slab {n // (N // c.per)}"
    return f"{c.id} {what}: {bad.shape[0]} of {y.numel()} outputs differ; first at launch {r // c.M}, row {r % c.M}, n {n} ({where}): got {float(y[r, n])}, want {float(want[r, n])}"


def _meta_ok(ops, c, layers):
    if c.dt != "f16":
        return False
    if c.layout == "w3s":
        return all(ops.w3s_meta_scalable(s, z, N, c.K) for (_, s, z, _, N) in layers)
    return all(ops.meta_scalable(s, z, N, c.K, GS, c.nbits) for (_, s, z, _, N) in layers)


def _stream_twin(oracle, c, layers, conts):
    """the same levels and meta in the 3-bit stream layout (made on the host), for the row-per-wave stream kernel"""
    out = []
    for (Wq, s, z, b, N), P in zip(layers, conts):
        W3 = oracle.w3s_pack_np(P, N, c.K).view(np.int32).reshape(N // 2, c.K // 16 * 3)
        out.append((torch.from_numpy(np.ascontiguousarray(W3)).cuda(), s, z, b, N))
    return out


@pytest.mark.parametrize("c", EXACT_CASES, ids=ids(EXACT_CASES))
def test_coded_layers_equal_their_closed_form(ops, oracle, c):
    """scale-, zero- and level-coded layers x one-hot rows, group indicators and all ones: torch.equal with the fp64 closed form rounded once (+ once
    for the bias), for every option variant of the case and with OPT_META_SCALABLE where the meta check accepts every layer; a grouped launch also
    equals its per-layer calls bit for bit; a 3-bit container case also equals the stream-layout kernel (and the forced row-per-wave kernel) on the same levels"""
    for kind in KINDS:
        host = [gc.coded_layer(c, kind, li) for li in range(len(c.Ns))]
        layers, conts = [], []
        for li, (U, s, z, W, q) in enumerate(host):
            b = gc.coded_bias(c, li)
            L, P = _device_layer(oracle, c, U, gc.tensor(s, c.dt), gc.tensor(z, c.dt), None if b is None else gc.tensor(b, c.dt), c.Ns[li])
            layers.append(L)
            conts.append(P)
        variants = [c.base_opts | extra for extra in c.variants]
        if _meta_ok(ops, c, layers):
            variants += [v | g64.OPT_META_SCALABLE for v in variants]
        twin = c.layout == "c3" and all(N % 2 == 0 for N in c.Ns)
        for fam in FAMILIES:
            X = gc.activations(c, fam)
            idx = gc.launch_index(c, X.shape[0])   # every row of every launch is held to the closed form of the probe it carries
            wants = [gc.tensor(gc.expected(c, host[li][3], X, gc.coded_bias(c, li))[idx], c.dt).cuda() for li in range(len(layers))]
            for opts in variants:
                ys = _rows(ops, c, layers, X, opts)
                for li, (y, want) in enumerate(zip(ys, wants)):
                    assert y.dtype == want.dtype and y.shape == want.shape
                    assert torch.equal(y, want), _mismatch(c, y, want, f"{kind}-coded layer {li}, {fam}, opts {opts:#x}")
            if c.grouped:
                for y, y1 in zip(ys, _rows(ops, c, layers, X, variants[-1], grouped=False)):
                    assert torch.equal(y, y1), _mismatch(c, y, y1, f"{kind}-coded, {fam}: grouped vs per-layer")
            if twin:
                cw = g64.C("rowwise_w3s", 3, c.dt, c.M, c.Ns, c.K, bias=c.bias, layout="w3s")
                for y, y3 in zip(ys, _rows(ops, cw, _stream_twin(oracle, c, layers, conts), X, g64.OPT_W3S)):
                    assert torch.equal(y, y3), _mismatch(c, y, y3, f"{kind}-coded, {fam}: container kernel vs stream-layout kernel")
            if c.route == "gemv3_slabs":
                o = (c.base_opts & ~g64.OPT_GEMV3_SLABS) | g64.OPT_GEMV3_ROWWISE
                for y, y1 in zip(ys, _rows(ops, c, layers, X, o)):
                    assert torch.equal(y, y1), _mismatch(c, y, y1, f"{kind}-coded, {fam}: slab-sharing vs row-per-wave kernel")


@pytest.mark.parametrize("nbits,layout", [(8, "u8"), (4, "u8"), (3, "c3"), (3, "w3s"), (2, "u8"), (1, "u8")])
def test_the_three_op_form_runs_on_coded_layers(ops, nbits, layout):
    """the coded layers pass the meta check at every width and in both 3-bit layouts (integer zeros up to 61, scales of at most 61 / 16), so the test
    above runs the three-op rebuild on all three kinds of every fp16 case"""
    c = next(c for c in EXACT_CASES if c.dt == "f16" and c.nbits == nbits and c.layout == layout)
    for kind in KINDS:
        _, s, z, _, _ = gc.coded_layer(c, kind)
        assert _meta_ok(ops, c, [(None, gc.tensor(s, "f16").cuda(), gc.tensor(z, "f16").cuda(), None, c.Ns[0])]), (c.id, kind)


def _ulp_f16(t):
    """tests/test_hip_parity.py::ulp_f16: the spacing of fp16 numbers at |t|"""
    return torch.pow(2.0, torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -14))) - 10)


def _check_bar(c, extra, got, want, b):
    """the bar the project already uses for the route, named"""
    err = (got.double() - want.double()).abs()
    if c.factored:
        # tests/test_round3_gpu.py::test_factored_arithmetic_against_the_reference_outputs: at most 2^-8 from the reference's y, at most
        # max(2, outputs / 200) of them beyond rtol = atol = 1e-3
        beyond = int((err > 1e-3 + 1e-3 * want.double().abs()).sum())
        assert float(err.max()) <= 2 ** -8 + 1e-6 and beyond <= max(2, got.numel() // 200), (c.id, float(err.max()), beyond)
    elif c.dt == "bf16" and c.route == "gemm_pipe" and c.layout == "u8":
        # tests/test_gemm_pipe_gpu.py::test_pipelined_gemm_bf16: one bf16 ulp of the matmul result before the bias add
        bound = 2.0 ** -7 * (want.abs() + (0 if b is None else b.float().abs()[None, :])) + 2e-3
        assert bool(((got - want).abs() <= bound).all()), (c.id, hex(extra), float(err.max()), float(((got - want).abs() - bound).max()))
    elif c.dt == "bf16":
        # tests/test_hip_parity.py::test_gemv_bf16_vs_oracle, ::test_skinny_gemm_bf16_vs_oracle; tests/test_w3s_gpu.py::test_w3s_gemv_bf16_vs_oracle,
        # ::test_w3s_skinny_gemm_vs_oracle, ::test_w3s_pipelined_gemm_vs_oracle
        torch.testing.assert_close(got, want, rtol=2.0 ** -7, atol=2e-3, msg=lambda m: f"{c.id} opts {extra:#x}: {m}")
    elif c.layout == "w3s":     # tests/test_w3s_gpu.py::test_w3s_gemv_vs_oracle, ::test_w3s_skinny_gemm_vs_oracle, ::test_w3s_pipelined_gemm_vs_oracle
        torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3)
    elif c.layout == "c3":      # tests/test_hip_parity.py::test_gemv_3bit_vs_oracle, ::test_gemv_3bit_slab_sharing_kernel
        torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3)
    elif c.route == "skinny":   # tests/test_hip_parity.py::test_skinny_gemm_vs_oracle (assert_forward_parity: 1e-3 + 1e-3 |ref| + one fp16 ulp of ref)
        tol = 1e-3 + 1e-3 * want.abs() + _ulp_f16(want)
        assert not bool(((got - want).abs() > tol).any()), (c.id, extra, float(err.max()))
    elif c.note == "hybrid":    # tests/test_gemm_pipe_gpu.py::test_hybrid_plan_full_rounds_whole_last_round_split (an 8-bit layer: |y| up to 100, two fp16 roundings with the bias)
        torch.testing.assert_close(got, want, rtol=2e-3, atol=2e-3 * float(want.abs().max()) / 4 + 2e-3)
    elif c.route == "gemm_pipe" and extra & (g64.OPT_GEMM_NARROW | g64.OPT_GEMM_WIDE):   # tests/test_gemm_pipe_gpu.py::test_every_tile_shape_forced
        torch.testing.assert_close(got, want, rtol=2e-3, atol=2e-3)
    elif c.route in g64.GEMM_ROUTES:   # tests/test_gemm_pipe_gpu.py::test_pipelined_gemm_vs_oracle; tests/test_hip_parity.py::test_gemm_vs_oracle
        torch.testing.assert_close(got, want, rtol=1e-3, atol=2e-3)
    else:                       # tests/test_hip_parity.py::test_gemv_vs_oracle; 8-bit: ::test_gemv_8bit_1bit_vs_oracle
        torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3 * (16 if c.nbits == 8 else 1))


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_randn_layer_against_the_fp64_reference(ops, oracle, c):
    """_random_layer's meta and randn x against dequantise + double-accumulated matmul on the host, on every option variant, each run twice (the same
    bits, the split-K variants included); the dequantise kernel's weights against the host's; one-hot rows against the dequantise kernel's columns;
    grouped == per-layer where the group does not change the K split; M = 1 == row 0 of M rows on the row-per-wave kernels"""
    host = [gc.random_layer(c, li) for li in range(len(c.Ns))]
    if c.dt == "bf16" and not (c.route == "gemm_pipe" and c.layout == "u8"):
        # these routes' bf16 bar (rtol 2^-7, atol 2e-3) is one bf16 ulp of the RESULT; with a N(0, 1) bias a last-bit flip of bf16(acc) between fp32 and double
        # accumulation survives the add as one ulp of |acc| <= |y| + |bias|, which only the pipelined route's bar allows for.  The randn layer therefore runs
        # without the bias here; the bias add itself is pinned bit for bit by the coded layers above.
        host = [(U, s, z, None) for (U, s, z, _) in host]
    layers, conts = [], []
    for li, (U, s, z, b) in enumerate(host):
        L, P = _device_layer(oracle, c, U.numpy(), s, z, b, c.Ns[li])
        layers.append(L)
        conts.append(P)
    x = gc.random_x(c)
    xd = x.cuda()
    refs, Wdevs = [], []
    for li, ((U, s, z, b), (Wq, sd, zd, bd, N)) in enumerate(zip(host, layers)):
        cont = conts[li] if conts[li] is not None else oracle.pack(c.nbits, U.numpy())   # the reference container: [N G / per, 64] bytes, [ceil(N G / 10), 64] words
        Wd = gc.reference_weights(oracle, c, cont, s, z, li)
        refs.append(torch.from_numpy(gc.reference_forward(oracle, c, Wd, x, b)))
        if not c.factored:
            # the fused kernels' weights ARE the dequantise kernel's (of the reference container), which are the host's
            Wdevs.append(ops.dequantize(Wq if c.layout == "u8" else torch.from_numpy(cont).cuda(), sd.reshape(-1), zd.reshape(-1), N, c.K, GS, c.nbits))
            assert np.array_equal(Wdevs[-1].float().cpu().numpy(), Wd), (c.id, "dequantise kernel vs host")
    for extra in c.variants:
        opts = c.base_opts | extra
        ys = _call(ops, c, layers, xd, opts)
        for li, (y, want) in enumerate(zip(ys, refs)):
            assert y.dtype == gc.DT[c.dt] and tuple(y.shape) == (c.M, c.Ns[li])
            got = y.float().cpu()
            _check_bar(c, extra, got, want, host[li][3])
        for li, (y, y2) in enumerate(zip(ys, _call(ops, c, layers, xd, opts))):
            assert torch.equal(y, y2), (c.id, li, hex(opts), "the same call twice")
    ys = _call(ops, c, layers, xd, c.base_opts)
    if c.grouped and c.route in g64.ROW_PER_WAVE + ("mfma16",):   # (the skinny, slab-sharing and pipelined kernels choose their split for the group's width)
        for li, (y, y1) in enumerate(zip(ys, _call(ops, c, layers, xd, c.base_opts, grouped=False))):
            assert torch.equal(y, y1), _mismatch(c, y, y1, f"randn layer {li}: grouped vs per-layer")
    if c.route in g64.ROW_PER_WAVE and c.M > 1 and not c.factored:
        for li, (y, y1) in enumerate(zip(ys, _call(ops, c, layers, xd[:1].contiguous(), c.base_opts))):
            assert torch.equal(y[:1], y1), _mismatch(c, y[:1], y1, f"randn layer {li}: M = 1 vs row 0 of M = {c.M}")
    if not c.factored:
        X = gc.activations(c, "onehot")
        ks = torch.from_numpy(X.argmax(axis=1)[gc.launch_index(c, X.shape[0])]).cuda()   # the k of every row of every launch
        nobias = [(Wq, s, z, None, N) for (Wq, s, z, _, N) in layers]
        for extra in c.variants:
            for li, y in enumerate(_rows(ops, c, nobias, X, c.base_opts | extra)):
                cols = Wdevs[li][:, ks].t().contiguous()
                assert torch.equal(y, cols), _mismatch(c, y, cols, f"randn layer {li}, opts {c.base_opts | extra:#x}: one-hot rows vs dequantise columns")
