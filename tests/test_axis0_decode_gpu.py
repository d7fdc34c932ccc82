"""The axis-0 decode kernel (hqq_hip_gemv_axis0, csrc/gemv_axis0.hip) on the GPU: against the double-accumulated oracle on reference-exact
weights, bit-exact one-hot columns against the dequantise kernel, determinism, graph capture, the reference's axis-0 fixtures through HQQLinear,
and a tiny HF Llama quantised along axis 0 end to end."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

COMBOS = [(8, torch.float16), (4, torch.float16), (2, torch.float16), (1, torch.float16), (4, torch.bfloat16), (2, torch.bfloat16)]
CODE = {torch.float16: 1, torch.bfloat16: 2}


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


def _ref_weights(oracle, nbits, P, s, z, N, K, dt):
    """Quantizer.dequantize of an axis-0 layer on the host: unpack the [gs, N K / gs] level matrix, (U - zero) * scale per column with one
    rounding to the compute dtype per op (numpy's float16 ops round once; bf16 through float32 + an explicit round to nearest even — both exact
    restatements: float32 carries more than twice the bits of either format), reshape to [N, K].  Returns float32 values of the dtype."""
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


def _check_vs_oracle(ops, oracle, nbits, dt, N, K, gs, M, with_bias, seed):
    gs_eff = N if gs is None else gs
    U, s, z = _random_layer(N, K, gs_eff, nbits, dt, seed)
    P = oracle.pack(nbits, U)
    Wd = _ref_weights(oracle, nbits, P, s, z, N, K, dt)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed + 1)).to(dt)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(seed + 2)).to(dt) if with_bias else None
    yo, _ = oracle.matmul(_raw(x.float().numpy(), dt), _raw(Wd, dt), None if bias is None else _raw(bias.float().numpy(), dt), CODE[dt])
    want = torch.from_numpy(yo.astype(np.float32)) if dt == torch.float16 else torch.from_numpy((yo.astype(np.uint32) << 16).view(np.float32))
    y = ops.gemv_axis0(x.cuda(), torch.from_numpy(P).cuda(), s.cuda(), z.cuda(), None if bias is None else bias.cuda(), N, K, gs, nbits)
    assert y.dtype == dt and tuple(y.shape) == (M, N)
    if dt == torch.float16:   # fp32 accumulation vs the double-accumulated oracle on identical weights: the bar of test_gemv_vs_oracle
        torch.testing.assert_close(y.float().cpu(), want, rtol=1e-3, atol=1e-3)
    else:                     # bf16 outputs: within one bf16 ulp (the bar of the bf16 decode tests)
        torch.testing.assert_close(y.float().cpu(), want, rtol=2.0 ** -7, atol=2e-3)
    return U, P, s, z


def test_reference_weights_helper_matches_the_fixtures(oracle):
    """the host restatement used below reproduces the reference's own dequantised axis-0 weights bit for bit"""
    for nbits in (4, 2, 8):
        g = load_golden(f"quant_axis0_{nbits}b_128x256")
        P = g["Wq_packed"]
        W = _ref_weights(oracle, nbits, P, torch.from_numpy(g["scale_f16"]), torch.from_numpy(g["zero_f16"]), 128, 256, torch.float16)
        assert np.array_equal(W.astype(np.float16).view(np.uint16), g["Wdeq_f16"].view(np.uint16)), nbits


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M", [1, 2, 3, 4, 7, 16])
@pytest.mark.parametrize("gs", [16, 64, 128, None])
@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_gemv_axis0_vs_oracle(ops, oracle, nbits, dt, gs, M, bias):
    _check_vs_oracle(ops, oracle, nbits, dt, 256, 1024, gs, M, bias, seed=nbits * 100 + (gs or 7) + M)


SHAPES_7B = [(4096, 4096), (11008, 4096), (4096, 11008)]


# (the 235 M-weight host reference of the 70B down projection is built for one fp16 and one bf16 width only)
LLAMA_CASES = [(nb, dt, NK) for nb, dt in COMBOS for NK in SHAPES_7B + [(1024, 8192)]] + \
              [(4, torch.float16, (8192, 28672)), (2, torch.bfloat16, (8192, 28672))]


@pytest.mark.parametrize("nbits,dt,NK", LLAMA_CASES)
def test_gemv_axis0_llama_shapes_vs_oracle(ops, oracle, nbits, dt, NK):
    """every Llama-2-7B linear shape and the 70B k/v and down projections (K = 28672), one row, with a bias"""
    _check_vs_oracle(ops, oracle, nbits, dt, NK[0], NK[1], 64, 1, True, seed=NK[0] + NK[1] + nbits)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("nbits,dt", COMBOS)
@pytest.mark.parametrize("NK,gs", [((256, 1024), 64), ((4096, 4096), 64), ((1024, 8192), 128), ((256, 1024), None)])
def test_one_hot_columns_are_the_dequantised_weights(ops, oracle, nbits, dt, NK, gs):
    """e_k at the first and last k of K-chunks and at K - 1 gives column k of ops.dequantize(axis=0) bit for bit"""
    N, K = NK
    gs_eff = N if gs is None else gs
    U, s, z = _random_layer(N, K, gs_eff, nbits, dt, seed=11 + nbits)
    P = _dev(oracle.pack(nbits, U))
    s, z = s.cuda(), z.cuda()
    Wdev = ops.dequantize(P, s.reshape(-1), z.reshape(-1), N, K, gs_eff, nbits, 0)
    ks = sorted({0, 63, 64, 127, 128, K // 2 - 1, K // 2, K - 64, K - 1})
    e = torch.zeros(len(ks), K, dtype=dt, device="cuda")
    for i, k in enumerate(ks):
        e[i, k] = 1.0
    ye = ops.gemv_axis0(e, P, s, z, None, N, K, gs, nbits)
    for i, k in enumerate(ks):
        assert torch.equal(ye[i], Wdev[:, k]), k


def test_deterministic_and_graph_capturable(ops, oracle):
    N, K, gs, nbits = 4096, 4096, 64, 4
    U, s, z = _random_layer(N, K, gs, nbits, torch.float16, seed=5)
    P, s, z = _dev(oracle.pack(nbits, U)), s.cuda(), z.cuda()
    x = torch.randn(16, K, device="cuda", dtype=torch.float16)
    b = torch.randn(N, device="cuda", dtype=torch.float16)
    y1 = ops.gemv_axis0(x, P, s, z, b, N, K, gs, nbits)
    y2 = ops.gemv_axis0(x, P, s, z, b, N, K, gs, nbits)
    assert torch.equal(y1, y2)
    # rows are independent of the batch they come in (the K split is a function of the shape)
    assert torch.equal(ops.gemv_axis0(x[3:4], P, s, z, b, N, K, gs, nbits), y1[3:4])
    # inside torch.cuda.graph capture, with the workspace reserved by the eager calls above
    xs = x[:2].clone()
    out = torch.empty(2, N, device="cuda", dtype=torch.float16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gemv_axis0(xs, P, s, z, b, N, K, gs, nbits, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemv_axis0(xs, P, s, z, b, N, K, gs, nbits, out=out)
    xs.copy_(x[5:7])
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, y1[5:7])


@pytest.mark.parametrize("nbits", [4, 2, 8])
def test_hqqlinear_axis0_fixture_takes_the_decode_kernel(ops, nbits, monkeypatch):
    """HQQLinear(axis=0) on the reference's fixture: output within 1e-3 of the reference's, through hqq_hip_gemv_axis0 and no torch.matmul"""
    from hqq_amd import ops as hops
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    g = load_golden(f"quant_axis0_{nbits}b_128x256")
    lin = torch.nn.Linear(256, 128, bias=False)
    lin.weight.data = torch.from_numpy(g["W"]).clone()
    layer = HQQLinear(lin, BaseQuantizeConfig(nbits=nbits, group_size=64, axis=0), compute_dtype=torch.float16, device="cuda")
    calls = {"axis0": 0, "matmul": 0}
    real_axis0, real_matmul = hops.gemv_axis0, torch.matmul

    def counting_axis0(*a, **k):
        calls["axis0"] += 1
        return real_axis0(*a, **k)

    def counting_matmul(*a, **k):
        calls["matmul"] += 1
        return real_matmul(*a, **k)

    monkeypatch.setattr(hops, "gemv_axis0", counting_axis0)
    monkeypatch.setattr(torch, "matmul", counting_matmul)
    x = torch.from_numpy(g["x_f32"]).half().cuda()
    with torch.no_grad():
        y = layer(x)
    assert calls == {"axis0": 1, "matmul": 0}
    torch.testing.assert_close(y.float().cpu(), torch.from_numpy(g["y_f16"].astype(np.float32)), rtol=1e-3, atol=1e-3)


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=128)
    return LlamaForCausalLM(cfg).half().cuda().eval()


@pytest.mark.parametrize("nbits", [4, 2])
def test_tiny_llama_quantised_along_axis0(nbits):
    from hqq_amd.backends.hip import HQQLinearHIP, group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQBackend, HQQLinear
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    model = _tiny_llama()
    quantize_model(model, BaseQuantizeConfig(nbits=nbits, group_size=64, axis=0), compute_dtype=torch.float16, device="cuda")
    qs = [m for m in model.modules() if isinstance(m, HQQLinear)]
    assert len(qs) == 14 and all(q.meta["axis"] == 0 for q in qs)
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(1)).cuda()
    HQQLinear.set_backend(HQQBackend.PYTORCH_FORWARD)
    try:
        with torch.no_grad():
            dense = model(ids).logits.float()
            dense_one = model(ids[:, :1]).logits.float()
            want = model.generate(ids[:1, :5], max_new_tokens=8, min_new_tokens=8, do_sample=False)
    finally:
        HQQLinear.set_backend(HQQBackend.HIP)
    prepare_for_inference(model, backend="hip")
    assert sum(isinstance(m, HQQLinearHIP) for m in model.modules()) == 14                 # none skipped
    assert all(m.axis == 0 for m in model.modules() if isinstance(m, HQQLinearHIP))
    with torch.no_grad():
        out = model(ids).logits.float()            # 18 rows: dequantise + matmul, as HQQLinear runs them
        one = model(ids[:, :1]).logits.float()     # 2 rows: the axis-0 decode kernel
    torch.testing.assert_close(out, dense, rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(one, dense_one, rtol=2e-3, atol=2e-3)
    assert group_llama_projections(model) == 0     # the grouped kernels read axis-1 meta
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    assert not dec.fused                           # the fused decode step reads axis-1 meta: the model's own forward serves
    assert torch.equal(dec.generate(ids[:1, :5], 8, use_graph=False), want)
