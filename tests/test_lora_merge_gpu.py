"""The LoRA merge on the GPU: hqq_hip_lora_merge against its contract restated on the CPU (tests/_merge_cases.py), bit for bit; the layer and model
level merges (HQQLinearLoRA.merge_and_quantize, PeftUtils.merge_lora) against the torch composition and against the reference's recorded result."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import _merge_cases as mc
from conftest import load_golden

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
GOLDENS = ["lora_merge_4b_axis1_32x128", "lora_merge_2b_axis0_32x128"]


@pytest.fixture(scope="module")
def ops():
    from hqq_amd import ops
    assert ops.is_available()
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run_case(ops, c, B_zero=False):
    """the kernel's output, the base weight it should have used (dequantize()'s bits, or the dense weight), and the adapter, for one case"""
    nbits, axis, N, K, gs, r, T, L = c
    seed = 1000 * nbits + 100 * axis + N + K + r
    A, B = mc.adapter(K, N, r, L, seed)
    if B_zero:
        B = torch.zeros_like(B)
    if nbits == 0:
        W = (torch.randn(N, K, generator=torch.Generator().manual_seed(seed + 1)) * 0.02).to(T)
        got = ops.lora_merge_dense(W.cuda(), A.cuda(), B.cuda(), 1.7)
        return got, W, A, B
    W_q, scale, zero = mc.synthetic_layer(nbits, N, K, gs, axis, T, seed + 1)
    W_q, scale, zero = W_q.cuda(), scale.cuda(), zero.cuda()
    W = ops.dequantize(W_q, scale, zero, N, K, gs, nbits, axis)
    got = ops.lora_merge(W_q, scale, zero, N, K, gs, nbits, axis, A.cuda(), B.cuda(), 1.7)
    return got, W.cpu(), A, B


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_kernel_matches_the_restated_contract(ops, case):
    nbits, axis, N, K, gs, r, T, L = case
    assert ops.lora_merge_covers(T, L, N, K, gs, nbits, axis, r)     # every case is one the kernel serves: none is skipped
    got, W, A, B = _run_case(ops, case)
    assert got.dtype == T and tuple(got.shape) == (N, K)
    want = mc.merged_reference(W, A, B, 1.7, L, T)
    assert float((want.float() - W.float()).abs().max()) > 0         # the adapter moved the weights
    assert torch.equal(_bits(got.cpu()), _bits(want))


@pytest.mark.parametrize("case", [c for c in mc.CASES if c[5] == 17], ids=mc.case_id)
def test_zero_adapter_gives_the_dequantised_weights(ops, case):
    got, W, _, _ = _run_case(ops, case, B_zero=True)
    assert torch.equal(_bits(got.cpu()), _bits(W))


def test_two_calls_give_the_same_bits_and_out_is_honoured(ops):
    N, K, gs, r = 136, 200, 8, 64
    W_q, scale, zero = (t.cuda() for t in mc.synthetic_layer(4, N, K, gs, 1, F16, 5))
    A, B = (t.cuda() for t in mc.adapter(K, N, r, F32, 6))
    first = ops.lora_merge(W_q, scale, zero, N, K, gs, 4, 1, A, B, 0.5)
    guard = torch.full((N * K + 64,), float("nan"), dtype=F16, device="cuda")
    out = guard[32:32 + N * K]
    again = ops.lora_merge(W_q, scale, zero, N, K, gs, 4, 1, A, B, 0.5, out=out)
    assert again.data_ptr() == out.data_ptr() and torch.equal(_bits(again), _bits(first))
    assert bool(torch.isnan(guard[:32]).all()) and bool(torch.isnan(guard[32 + N * K:]).all())    # nothing outside [N, K] is written
    with pytest.raises(NotImplementedError):
        ops.lora_merge(W_q, scale, zero, N, K, gs, 4, 1, torch.zeros(K, 257, device="cuda"), torch.zeros(257, N, device="cuda"), 0.5)
    with pytest.raises(NotImplementedError):
        ops.lora_merge(W_q, scale.float(), zero.float(), N, K, gs, 4, 1, A, B, 0.5)
    with pytest.raises(ValueError):
        ops.lora_merge(W_q, scale[:-1], zero[:-1], N, K, gs, 4, 1, A, B, 0.5)
    with pytest.raises(ValueError):
        ops.lora_merge(W_q[:-1], scale, zero, N, K, gs, 4, 1, A, B, 0.5)


def test_flat_indices_past_32_bits(ops):
    """65600 x 65536 int4: N K > 2^32, so the flat element index, the slab / container split and the meta index leave 32 bits (the kernel divides in 64 bits
    there).  B = 0 must give dequantize()'s bits everywhere; with an adapter, the rows at the start, around flat index 2^31 and 2^32, and at the end match
    the restated contract."""
    N, K, gs, r = 65600, 65536, 64, 3
    g = torch.Generator(device="cuda").manual_seed(3)
    W_q = torch.randint(0, 256, (N * K // 2,), generator=g, dtype=torch.uint8, device="cuda")
    zero = (7.5 + torch.rand(N * K // gs, generator=g, device="cuda") * 2 - 1).half()
    scale = (0.01 * (1 + 0.2 * torch.rand(N * K // gs, generator=g, device="cuda"))).half()
    A, B = (t.cuda() for t in mc.adapter(K, N, r, F32, 4))
    W = ops.dequantize(W_q, scale, zero, N, K, gs, 4, 1)
    out = ops.lora_merge(W_q, scale, zero, N, K, gs, 4, 1, A, torch.zeros_like(B), 2.0)
    assert torch.equal(_bits(out), _bits(W))
    ops.lora_merge(W_q, scale, zero, N, K, gs, 4, 1, A, B, 2.0, out=out)
    rows = torch.tensor([0, 1, 32767, 32768, 32799, 32800, 65535, 65536, 65598, 65599])   # 32768 K = 2^31, 32800: the slab edge, 65536 K = 2^32
    want = mc.merged_reference(W[rows.cuda()].cpu(), A.cpu(), B[:, rows.cuda()].cpu(), 2.0, F32, F16)
    assert torch.equal(_bits(out[rows.cuda()].cpu()), _bits(want))


# ---- the layer: HQQLinearLoRA.merge_and_quantize -------------------------------------------------------------------------------------------------
def _same_layer(a, b):
    assert a.W_q.dtype == b.W_q.dtype and torch.equal(a.W_q, b.W_q)
    for key in ("scale", "zero"):
        assert a.meta[key].dtype == b.meta[key].dtype and torch.equal(_bits(a.meta[key].reshape(-1)), _bits(b.meta[key].reshape(-1))), key
    assert (a.bias is None) == (b.bias is None)
    if a.bias is not None:
        assert a.bias.dtype == b.bias.dtype and torch.equal(a.bias, b.bias)
    assert a.compute_dtype == b.compute_dtype and a.meta["shape"] == b.meta["shape"] and a.meta["axis"] == b.meta["axis"]


def _count_calls(monkeypatch, ops, name):
    calls, fn = [], getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(1), fn(*a, **k))[1])
    return calls


@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("T", [F16, BF16], ids=["float16", "bfloat16"])
def test_layer_merge_equals_the_quantised_composition(ops, monkeypatch, axis, T):
    from hqq_amd.core.peft import HQQLinearLoRA
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    N, K, r = 96, 192, 8
    cfg = BaseQuantizeConfig(nbits=4, group_size=64, axis=axis)
    torch.manual_seed(20 + axis)
    lin = nn.Linear(K, N, bias=True)
    lin.weight.data.normal_(0, 0.02)
    layer = HQQLinear(lin, cfg, compute_dtype=T, device="cuda")
    A, B = mc.adapter(K, N, r, F32, 30 + axis)
    wrapper = HQQLinearLoRA(layer, {"r": r, "lora_alpha": 12, "lora_init": {"lora_A": A, "lora_B": B}})
    wrapper.scaling = nn.Parameter(torch.tensor(1.5, device="cuda"), requires_grad=False)     # as load_state_dict can leave it
    calls = _count_calls(monkeypatch, ops, "lora_merge")
    new = wrapper.merge_and_quantize(cfg)
    assert calls == [1] and type(new) is HQQLinear and new.ready and new.compute_dtype == T and new.W_q.is_cuda

    W = mc.merged_reference(layer.dequantize().cpu(), A, B, 1.5, F32, T)
    want = HQQLinear.from_weights(W.cuda(), wrapper.bias.data.clone(), cfg, compute_dtype=T, device="cuda")
    _same_layer(new, want)
    assert new.bias.data_ptr() != wrapper.bias.data_ptr()
    assert not torch.equal(new.W_q, layer.W_q)                       # and the adapter changed the layer


def _golden_wrapper(g, bias=True):
    """the reference's packed layer and adapter of a fixture, as an HQQLinearLoRA over an HQQLinear on the GPU"""
    from hqq_amd.core.peft import HQQLinearLoRA
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    N, K = (int(v) for v in g["shape"])
    cfg = BaseQuantizeConfig(nbits=int(g["nbits"]), group_size=int(g["group_size"]), axis=int(g["axis"]))
    lin = nn.Linear(K, N, bias=bias)
    if bias:
        lin.bias.data = torch.from_numpy(g["bias"]).float()
    layer = HQQLinear(lin, cfg, compute_dtype=F16, device="cuda")
    layer.W_q = nn.Parameter(torch.from_numpy(g["W_q"]).cuda().reshape(layer.W_q.shape), requires_grad=False)
    for key in ("scale", "zero"):
        layer.meta[key] = torch.from_numpy(g[key]).cuda().reshape(layer.meta[key].shape)
    assert np.array_equal(layer.dequantize().cpu().numpy().view(np.uint16), g["base"].view(np.uint16))
    r = g["lora_A"].shape[1]
    init = {"lora_A": torch.from_numpy(g["lora_A"]), "lora_B": torch.from_numpy(g["lora_B"])}
    wrapper = HQQLinearLoRA(layer, {"r": r, "lora_alpha": int(g["lora_alpha"]), "lora_init": init})
    assert wrapper.scaling == float(g["scaling"])
    return wrapper, cfg


@pytest.mark.parametrize("name", GOLDENS)
def test_layer_merge_reproduces_the_reference(ops, monkeypatch, name):
    """the reference's own merge statements and Quantizer.quantize, recorded on the CPU: packed bytes and meta of the re-quantised layer"""
    g = load_golden(name)
    wrapper, cfg = _golden_wrapper(g)
    calls = _count_calls(monkeypatch, ops, "lora_merge")
    new = wrapper.merge_and_quantize(cfg)
    assert calls == [1]
    assert np.array_equal(new.W_q.cpu().numpy().reshape(-1), g["merged_W_q"].reshape(-1))
    for key in ("scale", "zero"):    # HQQLinear.cuda casts the solver's fp32 meta to the compute dtype
        want = torch.from_numpy(g["merged_" + key]).half()
        assert torch.equal(_bits(new.meta[key].reshape(-1).cpu()), _bits(want)), key
    assert torch.equal(new.bias.cpu(), torch.from_numpy(g["bias"])) and new.bias.dtype == F16


@pytest.mark.parametrize("name", GOLDENS)
def test_forced_composition_gives_the_same_layer(ops, monkeypatch, name):
    """fused_merge = False: the torch statements (a library GEMM); on inputs whose sums are exact its summation order cannot matter"""
    from hqq_amd.core.peft import HQQLinearLoRA
    g = load_golden(name)
    wrapper, cfg = _golden_wrapper(g)
    fused = wrapper.merge_and_quantize(cfg)
    calls = _count_calls(monkeypatch, ops, "lora_merge")
    monkeypatch.setattr(HQQLinearLoRA, "fused_merge", False)
    composed = wrapper.merge_and_quantize(cfg)
    assert calls == []
    _same_layer(fused, composed)
    # outside the kernel's coverage the composition serves without the switch: an fp32 adapter of rank 257 is merged, not refused
    monkeypatch.setattr(HQQLinearLoRA, "fused_merge", True)
    wide = HQQLinearLoRA(wrapper.linear_layer, {"r": 257, "lora_alpha": 257})
    wide.lora_B.data.normal_(0, 0.01)
    assert type(wide.merge_and_quantize(cfg)).__name__ == "HQQLinear" and calls == []


def test_wrapped_nn_linear_takes_the_dense_kernel(ops, monkeypatch):
    from hqq_amd.core.peft import HQQLinearLoRA
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    N, K, r = 40, 128, 8
    cfg = BaseQuantizeConfig(nbits=4, group_size=64, axis=1)
    torch.manual_seed(40)
    lin = nn.Linear(K, N, bias=False)
    lin.weight.data.normal_(0, 0.02)
    lin = lin.half().cuda()
    W0 = lin.weight.data.clone()
    A, B = mc.exact_adapter(K, N, r, 41)
    wrapper = HQQLinearLoRA(lin, {"r": r, "lora_alpha": 16, "lora_init": {"lora_A": A / 4, "lora_B": B / 4}})
    calls = _count_calls(monkeypatch, ops, "lora_merge_dense")
    new = wrapper.merge_and_quantize(cfg)
    assert calls == [1] and new.bias is None and new.compute_dtype == F16
    assert torch.equal(lin.weight.data, W0)                          # the wrapped layer is left as it was
    want = HQQLinear.from_weights(mc.merged_reference(W0.cpu(), A / 4, B / 4, 2.0, F32, F16).cuda(), None, cfg, compute_dtype=F16, device="cuda")
    _same_layer(new, want)
    monkeypatch.setattr(HQQLinearLoRA, "fused_merge", False)
    _same_layer(wrapper.merge_and_quantize(cfg), want)
    assert calls == [1]


# ---- the model: train -> merge -> prepare_for_inference -> the fused, graph-replayed decode ---------------------------------------------------------
def test_merged_model_decodes_through_the_fused_step(ops, monkeypatch):
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.peft import HQQLinearLoRA, PeftUtils, is_hqq_lora_layer
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    torch.manual_seed(0)
    hf = LlamaForCausalLM(LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                                      vocab_size=512, max_position_embeddings=128)).half().cuda().eval()
    qcfg = BaseQuantizeConfig(nbits=4, group_size=64, axis=1)
    model = quantize_model(hf, qcfg, compute_dtype=F16, device="cuda")
    tags = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    lora = {"r": 8, "lora_alpha": 16, "dropout": 0.0}
    PeftUtils.add_lora(model, {t: (dict(lora) if t in ("self_attn.q_proj", "self_attn.v_proj", "mlp.down_proj") else None) for t in tags})
    wrapped = [n for n, m in model.named_modules() if is_hqq_lora_layer(m)]
    assert len(wrapped) == 6
    assert not llama_fused.supports(model)                           # a model that carries wrappers is not served by the fused step
    for i, n in enumerate(wrapped):   # a trained state whose sums are exact, so that the composition's GEMM and the kernel's loop must agree
        m = model.get_submodule(n)
        A, B = mc.exact_adapter(m.in_features, m.out_features, 8, 50 + i)
        m.lora_A.data, m.lora_B.data = (A / 16).cuda(), (B / 16).cuda()
    twin = copy.deepcopy(model)
    before = {n: model.get_submodule(n).linear_layer.W_q.clone() for n in wrapped}

    calls = _count_calls(monkeypatch, ops, "lora_merge")
    PeftUtils.merge_lora(model, {t: qcfg for t in tags})
    assert len(calls) == 6
    assert not any(is_hqq_lora_layer(m) for m in model.modules()) and not hasattr(model, "peft_config")
    monkeypatch.setattr(HQQLinearLoRA, "fused_merge", False)
    for n in wrapped:   # the copy: layer by layer through the composition
        parent, _, child = n.rpartition(".")
        setattr(twin.get_submodule(parent), child, twin.get_submodule(n).merge_and_quantize(qcfg))
    assert len(calls) == 6
    for n in wrapped:
        a, b = model.get_submodule(n), twin.get_submodule(n)
        assert type(a) is HQQLinear and type(b) is HQQLinear
        assert torch.equal(a.W_q, b.W_q) and torch.equal(a.meta["scale"], b.meta["scale"]) and torch.equal(a.meta["zero"], b.meta["zero"])
        assert not torch.equal(a.W_q, before[n])

    ids = torch.randint(0, 512, (1, 6), generator=torch.Generator().manual_seed(3)).cuda()
    toks = []
    for m in (model, twin):
        prepare_for_inference(m, backend="hip")
        group_llama_projections(m)
        assert not any(is_hqq_lora_layer(x) or type(x) is HQQLinear for x in m.modules())    # every linear went to the inference layer
        assert llama_fused.supports(m)
        dec = GraphedGreedyDecoder(m, max_cache_len=64)
        assert dec.fused
        toks.append(dec.generate(ids, 8, use_graph=True))
        assert dec.graph is not None
    assert toks[0].shape[-1] == 6 + 8 and torch.equal(toks[0], toks[1])
