"""The axis-0 kernel for 17..256 rows (hqq_hip_gemm_axis0, csrc/gemm_axis0.hip) on the GPU: against the double-accumulated oracle on reference-exact
weights, bit-exact one-hot rows against the dequantise kernel, row independence, determinism, graph capture, the caller-owned workspace, the routing of
ops.forward(axis=0), the reference's axis-0 fixtures through HQQLinear, and a tiny HF Llama quantised along axis 0 end to end."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

COMBOS = [(8, torch.float16), (4, torch.float16), (2, torch.float16), (1, torch.float16), (4, torch.bfloat16), (2, torch.bfloat16)]
CODE = {torch.float16: 1, torch.bfloat16: 2}
ROWS = [17, 31, 32, 33, 48, 64, 65, 129, 256]   # first tile edge + 1, every ragged last tile, a full pass, a second pass of one row, the cap
HEAD = 256 << 10   # the workspace's counter head (csrc/hqq_common.h)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from hqq_amd import ops as o
    assert o.is_available(), "libhqq_hip.so must load on the GPU box (no fallback)"
    return o


# ---- the construction of test_axis0_decode_gpu.py (copied: test modules do not import each other) ----
def _bf16_round(a32: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), returned as float32"""
    u = np.ascontiguousarray(a32, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def _ref_weights(oracle, nbits, P, s, z, N, K, dt):
    """Quantizer.dequantize of an axis-0 layer on the host: unpack the [gs, N K / gs] level matrix, (U - zero) * scale per column with one
    rounding to the compute dtype per op, reshape to [N, K].  Returns float32 values of the dtype."""
    U = oracle.unpack(nbits, P)
    s32, z32 = s.float().numpy().reshape(1, -1), z.float().numpy().reshape(1, -1)
    if dt == torch.float16:
        W = ((U.astype(np.float16) - z32.astype(np.float16)) * s32.astype(np.float16)).astype(np.float32)
    else:
        W = _bf16_round(_bf16_round(U.astype(np.float32) - z32) * s32)
    return W.reshape(N, K)


def _raw(a32: np.ndarray, dt):
    """float32 values of the dtype -> what the oracle takes (np.float16 / raw bf16 bits)"""
    return a32.astype(np.float16) if dt == torch.float16 else (np.ascontiguousarray(a32, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _random_layer(N, K, gs, nbits, dt, seed):
    g = torch.Generator().manual_seed(seed)
    C = N * K // gs
    U = torch.randint(0, 2 ** nbits, (gs, C), generator=g, dtype=torch.uint8).numpy()
    s = (torch.rand(C, generator=g) * 0.004 + 0.001).to(dt)
    z = (torch.rand(C, generator=g) * (2 ** nbits - 1)).to(dt)
    if dt == torch.bfloat16:
        z[::5] = 0.00836   # zero-points far below one level: q - z must still round once
        z[1::11] = 2.0 ** -12
    return U, s.reshape(1, -1), z.reshape(1, -1)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=4)
def _layer(oracle, nbits, dt, N, K, gs, seed):
    """one layer per configuration, built once: packed bytes + meta on the device and the reference-exact weights on the host (read-only)"""
    gs_eff = N if gs is None else gs
    U, s, z = _random_layer(N, K, gs_eff, nbits, dt, seed)
    P = oracle.pack(nbits, U)
    return _dev(P), s.cuda(), z.cuda(), _raw(_ref_weights(oracle, nbits, P, s, z, N, K, dt), dt)


def _check_vs_oracle(ops, oracle, nbits, dt, N, K, gs, Ms, with_bias, seed):
    P, s, z, Wd = _layer(oracle, nbits, dt, N, K, gs, seed)
    # The bias holds multiples of 1/8 in [-0.25, 0.25].  The output is round(round(y) + bias) and the bar is rtol |want| + atol on the FINAL value, while
    # fp32 against double accumulation may move round(y) by one ulp of y when y sits at a rounding tie: at most 2^-10 |y| in fp16, 2^-7 |y| in bf16.
    # (a) |y| <= |want| + |bias|, so that flip stays inside the bar down to want = 0 when 2^-10 |bias| <= 1e-3 (fp16: |bias| <= 1.02) and
    #     2^-7 |bias| <= 2e-3 (bf16: |bias| <= 0.256).  A larger bias cancels outputs of its own size to ~0 somewhere in the 65536 outputs of a 256-row
    #     call: bf16, nbits 4, gs 64, M 256, row 188, column 33 with a bias of -0.375 has round(y) either side of 1.0, 2^-7 apart, against a bar of
    #     2^-7 * 0.617 + 2e-3.
    # (b) a bias with bits below the result's ulp makes round(y) + bias itself a tie, and ties-to-even then sends the two neighbouring round(y) in
    #     opposite directions: two ulps from a one-ulp flip.  Seen at (fp16, nbits 8, gs 128, M 129, row 101, column 80) with a uniform bias: the dot
    #     product is 4.65820282 against the tie 4.658203125, the bias -0.380859375; this kernel and dequantise + torch.matmul both give 4.28125, the
    #     oracle 4.2734375.  Multiples of 1/8 are multiples of every result's ulp here (|y| < 128), so the bias add is exact or a plain half-way case.
    bias = (torch.randint(-2, 3, (N,), generator=torch.Generator().manual_seed(seed + 2)) / 8).to(dt) if with_bias else None
    xs = torch.randn(max(Ms), K, generator=torch.Generator().manual_seed(seed + 1)).to(dt)
    yo, _ = oracle.matmul(_raw(xs.float().numpy(), dt), Wd, None if bias is None else _raw(bias.float().numpy(), dt), CODE[dt])
    want = torch.from_numpy(yo.astype(np.float32)) if dt == torch.float16 else torch.from_numpy((yo.astype(np.uint32) << 16).view(np.float32))
    for M in Ms:   # (the oracle's rows are independent: its first M rows are its answer for x[:M])
        y = ops.gemm_axis0(xs[:M].cuda(), P, s, z, None if bias is None else bias.cuda(), N, K, gs, nbits)
        assert y.dtype == dt and tuple(y.shape) == (M, N)
        if dt == torch.float16:   # fp32 accumulation vs the double-accumulated oracle on identical weights
            torch.testing.assert_close(y.float().cpu(), want[:M], rtol=1e-3, atol=1e-3, msg=lambda m: f"M={M}: {m}")
        else:                     # bf16 outputs: within one bf16 ulp
            torch.testing.assert_close(y.float().cpu(), want[:M], rtol=2.0 ** -7, atol=2e-3, msg=lambda m: f"M={M}: {m}")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("gs", [16, 64, 128, None])
@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_gemm_axis0_vs_oracle(ops, oracle, nbits, dt, gs, bias):
    """every row count of ROWS on N = 256, K = 1024"""
    _check_vs_oracle(ops, oracle, nbits, dt, 256, 1024, gs, ROWS, bias, seed=nbits * 100 + (gs or 7))


def test_gemm_axis0_ragged_packed_rows_and_two_units(ops, oracle):
    """(N, K, gs) = (96, 128, 48) at 4 bits: P = 24 packed rows per class (a ragged tile), K holds 2 units (fewer than any split target)"""
    _check_vs_oracle(ops, oracle, 4, torch.float16, 96, 128, 48, [17, 65], True, seed=48)


@pytest.mark.parametrize("nbits,dt,N,K,M", [(4, torch.float16, 4096, 4096, 33), (2, torch.bfloat16, 11008, 4096, 65)])
def test_gemm_axis0_full_size_vs_oracle(ops, oracle, nbits, dt, N, K, M):
    """full-size layers: 32-bit offsets and the plan at real shapes"""
    _check_vs_oracle(ops, oracle, nbits, dt, N, K, 64, [M], True, seed=N + K + nbits)


HOT_ROWS = [0, 15, 16, 17, 31, 32, 47, 63, 64]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("nbits,dt", COMBOS)
@pytest.mark.parametrize("NK,gs", [((256, 1024), 64), ((256, 1024), None), ((4096, 4096), 64)])
def test_one_hot_rows_are_the_dequantised_weights(ops, oracle, nbits, dt, NK, gs, bias):
    """e_k at rows HOT_ROWS of a 65-row zero matrix: row i is column k of ops.dequantize(axis=0) bit for bit (plus the bias, rounded once), every
    other row exactly zero (or exactly the bias)"""
    N, K = NK
    gs_eff = N if gs is None else gs
    P, s, z, _ = _layer(oracle, nbits, dt, N, K, gs, 11 + nbits)
    Wdev = ops.dequantize(P, s.reshape(-1), z.reshape(-1), N, K, gs_eff, nbits, 0)
    ks = [0, 63, 64, 127, 128, K // 2 - 1, K // 2, K - 64, K - 1]
    b = torch.randn(N, generator=torch.Generator().manual_seed(3)).to(dt).cuda() if bias else None
    e = torch.zeros(65, K, dtype=dt, device="cuda")
    for i, k in zip(HOT_ROWS, ks):
        e[i, k] = 1.0
    ye = ops.gemm_axis0(e, P, s, z, b, N, K, gs, nbits)
    rest = torch.zeros(N, dtype=dt, device="cuda") if b is None else b
    for i in range(65):
        if i in HOT_ROWS:
            k = ks[HOT_ROWS.index(i)]
            assert torch.equal(ye[i], Wdev[:, k] if b is None else Wdev[:, k] + b), (i, k)
        else:
            assert torch.equal(ye[i], rest), i


@pytest.mark.parametrize("M", [40, 100])
@pytest.mark.parametrize("nbits,dt", [(4, torch.float16), (2, torch.bfloat16)])
def test_rows_are_independent_within_a_call(ops, oracle, nbits, dt, M):
    N, K, gs = 256, 1024, 64
    P, s, z, _ = _layer(oracle, nbits, dt, N, K, gs, 21 + nbits)
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    b = torch.randn(N, generator=g).to(dt).cuda()
    y = ops.gemm_axis0(x, P, s, z, b, N, K, gs, nbits)
    perm = torch.randperm(M, generator=g).cuda()
    assert torch.equal(ops.gemm_axis0(x[perm].contiguous(), P, s, z, b, N, K, gs, nbits), y[perm])
    for keep in (0, 16, M // 2, M - 1):   # all rows but one replaced by other data
        x2 = (torch.randn(M, K, generator=g) * 3).to(dt).cuda()
        x2[keep] = x[keep]
        assert torch.equal(ops.gemm_axis0(x2, P, s, z, b, N, K, gs, nbits)[keep], y[keep]), keep


def test_deterministic_and_graph_capturable(ops, oracle):
    N, K, gs, nbits = 4096, 4096, 64, 4
    P, s, z, _ = _layer(oracle, nbits, torch.float16, N, K, gs, 5)
    x = torch.randn(80, K, device="cuda", dtype=torch.float16)
    b = torch.randn(N, device="cuda", dtype=torch.float16)
    y1 = ops.gemm_axis0(x, P, s, z, b, N, K, gs, nbits)
    y2 = ops.gemm_axis0(x, P, s, z, b, N, K, gs, nbits)
    assert torch.equal(y1, y2)
    # inside torch.cuda.graph capture, with the workspace reserved by an eager call of the same size on a side stream
    xs = x[:40].clone()
    out = torch.empty(40, N, device="cuda", dtype=torch.float16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gemm_axis0(xs, P, s, z, b, N, K, gs, nbits, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemm_axis0(xs, P, s, z, b, N, K, gs, nbits, out=out)
    xs.copy_(x[40:80])
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    # (the eager bits of the same 40-row call: the K split, hence the order of the sum, is a function of the shape and the number of 64-row passes)
    assert torch.equal(out, ops.gemm_axis0(x[40:80].contiguous(), P, s, z, b, N, K, gs, nbits))


@pytest.mark.parametrize("nbits,dt,M", [(4, torch.float16, 33), (2, torch.bfloat16, 130)])
def test_caller_owned_workspace(ops, oracle, nbits, dt, M):
    """the raw ABI on a buffer of exactly workspace_bytes: the counter head is left as it was, the output is ops.gemm_axis0's"""
    from hqq_amd import _C
    L = _C.lib()
    N, K, gs = 256, 1024, 64
    P, s, z, _ = _layer(oracle, nbits, dt, N, K, gs, 31 + nbits)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(dt).cuda()
    b = torch.randn(N, generator=torch.Generator().manual_seed(M + 1)).to(dt).cuda()
    want = ops.gemm_axis0(x, P, s, z, b, N, K, gs, nbits)
    need = int(L.hqq_hip_gemm_axis0_workspace_bytes(nbits, M, N, K, gs, CODE[dt]))
    assert need > HEAD
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    pattern = (torch.arange(HEAD, device="cuda") % 251).to(torch.uint8)
    ws[:HEAD] = pattern
    ws[HEAD:] = 0xA5   # stale partial sums must not matter
    y = torch.empty(M, N, dtype=dt, device="cuda")
    rc = L.hqq_hip_gemm_axis0(nbits, x.data_ptr(), P.data_ptr(), s.data_ptr(), z.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, gs, CODE[dt], 0,
                              ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _C.last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws[:HEAD], pattern)
    assert torch.equal(y, want)
    # one byte less is refused before any launch
    assert L.hqq_hip_gemm_axis0(nbits, x.data_ptr(), P.data_ptr(), s.data_ptr(), z.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, gs, CODE[dt], 0,
                                ws.data_ptr(), need - 1, torch.cuda.current_stream().cuda_stream) == -5


def _count(monkeypatch, hops, names):
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(hops, n)

        def counting(*a, _real=real, _n=n, **k):
            calls[_n] += 1
            return _real(*a, **k)

        monkeypatch.setattr(hops, n, counting)
    return calls


def test_forward_axis0_routing(ops, oracle, monkeypatch):
    """which kernel ops.forward(axis=0) takes, with the cut-off set to 64 for the test (the route's code runs whatever value was measured) and at the
    shipped value of ops.AXIS0_GEMM_ROUTE_MAX_M"""
    from hqq_amd import ops as hops
    N, K, gs, nbits = 256, 1024, 64, 4
    P, s, z, _ = _layer(oracle, nbits, torch.float16, N, K, gs, 41)
    Wd = hops.dequantize(P, s.reshape(-1), z.reshape(-1), N, K, gs, nbits, 0)
    b = torch.randn(N, generator=torch.Generator().manual_seed(42)).half().cuda()
    shipped = hops.AXIS0_GEMM_ROUTE_MAX_M
    calls = _count(monkeypatch, hops, ["gemm_axis0", "gemv_axis0", "dequantize"])

    def run(M, bias=None, with_out=False, **kw):
        for n in calls:
            calls[n] = 0
        x = torch.randn(M, K, device="cuda", dtype=torch.float16)
        out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float16) if with_out else None
        y = hops.forward(x, P, s, z, bias, N, K, gs, nbits, out=out, axis=0, **kw)
        if with_out:
            assert y.data_ptr() == out.data_ptr()
        want = x.float() @ Wd.float().t()
        torch.testing.assert_close(y.float(), want if bias is None else want + bias.float(), rtol=2e-3, atol=2e-3)
        return dict(calls)

    new, old, decode = {"gemm_axis0": 1, "gemv_axis0": 0, "dequantize": 0}, {"gemm_axis0": 0, "gemv_axis0": 0, "dequantize": 1}, \
        {"gemm_axis0": 0, "gemv_axis0": 1, "dequantize": 0}
    monkeypatch.setattr(hops, "AXIS0_GEMM_ROUTE_MAX_M", 64)
    assert run(18) == new
    assert run(18, bias=b, with_out=True) == new          # the caller's buffer, with a bias
    assert run(64) == new
    assert run(65) == old                                  # cut-off + 1
    assert run(65, bias=b, with_out=True) == old
    assert run(18, library_gemm=True) == old
    assert run(257) == old
    assert run(16) == decode
    assert run(16, library_gemm=True) == decode
    x3 = torch.randn(2, 9, K, device="cuda", dtype=torch.float16)   # leading dimensions are kept
    assert tuple(hops.forward(x3, P, s, z, None, N, K, gs, nbits, axis=0).shape) == (2, 9, N)
    monkeypatch.setattr(hops, "AXIS0_GEMM_ROUTE_MAX_M", 256)
    assert run(256) == new and run(257) == old
    # the shipped value: 16 means the measured default is the old route (the kernel is opt-in)
    monkeypatch.setattr(hops, "AXIS0_GEMM_ROUTE_MAX_M", shipped)
    assert run(18) == (new if shipped >= 18 else old)
    if 17 <= shipped + 1 <= 256:
        assert run(shipped + 1) == old
    assert run(16) == decode


@pytest.mark.parametrize("nbits,dt,M", [(4, torch.float16, 40), (8, torch.float16, 129), (2, torch.bfloat16, 100)])
def test_general_bias_is_one_more_rounding_of_the_rounded_output(ops, oracle, nbits, dt, M):
    """an arbitrary (randn) bias: the output is round(round(acc) + bias) — the call without a bias, plus the bias, rounded once — bit for bit"""
    N, K, gs = 256, 1024, 64
    P, s, z, _ = _layer(oracle, nbits, dt, N, K, gs, 51 + nbits)
    g = torch.Generator().manual_seed(M + nbits)
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    b = (torch.randn(N, generator=g) * 3).to(dt).cuda()
    y0 = ops.gemm_axis0(x, P, s, z, None, N, K, gs, nbits)
    want = (y0.float() + b.float()).to(dt)   # (the fp32 sum of two fp16 / bf16 values is exact or rounds harmlessly: 24 bits against 11 / 8, one rounding to dt)
    assert torch.equal(ops.gemm_axis0(x, P, s, z, b, N, K, gs, nbits), want)


@pytest.mark.parametrize("nbits", [4, 2, 8])
def test_hqqlinear_axis0_fixture_takes_the_gemm_kernel(ops, nbits, monkeypatch):
    """HQQLinear(axis=0) on the reference's fixture, x tiled to 24 rows: within 1e-3 of the reference's output rows, through hqq_hip_gemm_axis0"""
    from hqq_amd import ops as hops
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    g = load_golden(f"quant_axis0_{nbits}b_128x256")
    lin = torch.nn.Linear(256, 128, bias=False)
    lin.weight.data = torch.from_numpy(g["W"]).clone()
    layer = HQQLinear(lin, BaseQuantizeConfig(nbits=nbits, group_size=64, axis=0), compute_dtype=torch.float16, device="cuda")
    x0 = torch.from_numpy(g["x_f32"]).half().reshape(-1, 256)
    reps = -(-24 // x0.shape[0])
    x = x0.repeat(reps, 1)[:24].contiguous().cuda()
    want = torch.from_numpy(g["y_f16"].astype(np.float32)).reshape(-1, 128).repeat(reps, 1)[:24]
    shipped = hops.AXIS0_GEMM_ROUTE_MAX_M
    calls = _count(monkeypatch, hops, ["gemm_axis0", "dequantize"])
    monkeypatch.setattr(hops, "AXIS0_GEMM_ROUTE_MAX_M", 256)   # the route through the kernel, whatever cut-off was measured
    with torch.no_grad():
        y = layer(x)
    assert calls == {"gemm_axis0": 1, "dequantize": 0}
    torch.testing.assert_close(y.float().cpu(), want, rtol=1e-3, atol=1e-3)
    monkeypatch.setattr(hops, "AXIS0_GEMM_ROUTE_MAX_M", shipped)   # and at the shipped cut-off
    calls.update(gemm_axis0=0, dequantize=0)
    with torch.no_grad():
        y = layer(x)
    assert calls["gemm_axis0"] == (1 if shipped >= 24 else 0)
    torch.testing.assert_close(y.float().cpu(), want, rtol=1e-3, atol=1e-3)
    # and the kernel itself on the layer's tensors, whatever the default route is
    m = layer.meta
    y2 = hops.gemm_axis0(x, layer.W_q, m["scale"], m["zero"], None, 128, 256, 64, nbits)
    torch.testing.assert_close(y2.float().cpu(), want, rtol=1e-3, atol=1e-3)


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=128)
    return LlamaForCausalLM(cfg).half().cuda().eval()


@pytest.mark.parametrize("nbits", [4, 2])
def test_tiny_llama_short_prompt_takes_the_gemm_kernel(nbits, monkeypatch):
    from hqq_amd import ops as hops
    from hqq_amd.backends.hip import HQQLinearHIP
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQBackend, HQQLinear
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    model = _tiny_llama()
    quantize_model(model, BaseQuantizeConfig(nbits=nbits, group_size=64, axis=0), compute_dtype=torch.float16, device="cuda")
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(1)).cuda()
    prompt = torch.randint(0, 512, (1, 20), generator=torch.Generator().manual_seed(2)).cuda()
    HQQLinear.set_backend(HQQBackend.PYTORCH_FORWARD)
    try:
        with torch.no_grad():
            dense = model(ids).logits.float()
            want = model.generate(prompt, max_new_tokens=8, min_new_tokens=8, do_sample=False)
    finally:
        HQQLinear.set_backend(HQQBackend.HIP)
    prepare_for_inference(model, backend="hip")
    assert sum(isinstance(m, HQQLinearHIP) for m in model.modules()) == 14
    calls = _count(monkeypatch, hops, ["gemm_axis0", "dequantize"])
    monkeypatch.setattr(hops, "AXIS0_GEMM_ROUTE_MAX_M", 256)   # the route through the kernel, whatever cut-off was measured
    with torch.no_grad():
        out = model(ids).logits.float()            # 18 rows
    assert calls == {"gemm_axis0": 14, "dequantize": 0}
    torch.testing.assert_close(out, dense, rtol=2e-3, atol=2e-3)
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    calls.update(gemm_axis0=0, dequantize=0)
    assert torch.equal(dec.generate(prompt, 8, use_graph=False), want)   # a 20-row prefill through the kernel, then one-row steps
    assert calls == {"gemm_axis0": 14, "dequantize": 0}
