"""CPU tests of the LoRA merge (hqq_hip_lora_merge, include/hqq_hip.h; HQQLinearLoRA.merge_and_quantize / PeftUtils.merge_lora): the restated contract
against the reference's recorded merge, the coverage answer at its edges, the refusal of bad calls before anything launches, and merge_lora's
bookkeeping on a toy module tree."""
import numpy as np
import pytest
import torch
from torch import nn

import _merge_cases as mc
from conftest import load_golden

F32, F16, BF16 = 0, 1, 2
NBITS_ERR, SHAPE, DTYPE, UNSUPPORTED = -1, -2, -3, -4
GOLDENS = ["lora_merge_4b_axis1_32x128", "lora_merge_2b_axis0_32x128"]


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    return _C.lib()


@pytest.mark.parametrize("name", GOLDENS)
def test_restated_contract_reproduces_the_reference_merge(name):
    """merged_reference (a j loop of separate fp32 `*` and `+`) on the reference's dequantised weight == the reference's own
    `W += (A @ B * scaling).t().to(W.dtype)`, bit for bit: the adapter's sums are exact, so the loop and the library matmul must agree"""
    g = load_golden(name)
    A, B = torch.from_numpy(g["lora_A"]), torch.from_numpy(g["lora_B"])
    assert torch.equal(torch.matmul(A.double(), B.double()), torch.matmul(A, B).double())
    got = mc.merged_reference(torch.from_numpy(g["base"]), A, B, float(g["scaling"]), torch.float32, torch.float16)
    assert np.array_equal(got.numpy().view(np.uint16), g["merged"].view(np.uint16))
    assert not np.array_equal(g["merged"], g["base"])


def test_reference_rounds_where_the_contract_says():
    """each rounding of merged_reference matters on ordinary (inexact) inputs: dropping any one of them changes bits, so the GPU comparison pins them all"""
    T, Ld = torch.float16, torch.float16
    W = (torch.randn(48, 192, generator=torch.Generator().manual_seed(1)) * 0.02).to(T)
    A, B = mc.adapter(192, 48, 17, Ld, 2)
    want = mc.merged_reference(W, A, B, 1.7, Ld, T)
    P = torch.matmul(A.float(), B.float())
    no_m = (W.float() + (P * 1.7).to(Ld).t().float()).to(T)                       # without round_L of the matmul's result
    one_round = (W.float() + (P.to(Ld).float() * 1.7).t()).to(T)                  # without round_L / round_T of the scaled product
    assert not torch.equal(no_m, want) and not torch.equal(one_round, want)
    assert torch.equal(mc.merged_reference(W, A, torch.zeros_like(B), 1.7, Ld, T), W)


def test_symbols_load_and_abi_is_unchanged(L):
    from hqq_amd import _C
    assert "hqq_hip_lora_merge" in _C.SYMBOLS and "hqq_hip_lora_merge_covers" in _C.SYMBOLS
    assert hasattr(L, "hqq_hip_lora_merge") and hasattr(L, "hqq_hip_lora_merge_covers")
    assert L.hqq_hip_abi_version() == 9 and _C.ABI_VERSION == 9


def test_covers_at_its_edges(L):
    from hqq_amd import ops
    cov = L.hqq_hip_lora_merge_covers
    for r, want in ((0, 0), (1, 1), (256, 1), (257, 0)):
        assert cov(4, 48, 192, 64, 1, F16, F32, r) == want, r
        assert cov(0, 48, 192, 0, 0, BF16, F16, r) == want, r
        assert ops.lora_merge_covers(torch.float16, torch.float32, 48, 192, 64, 4, 1, r) is bool(want)
    for nbits in (8, 4, 3, 2, 1):
        for axis in (0, 1):
            for T in (F16, BF16):
                for Ld in (F32, F16, BF16):
                    assert cov(nbits, 48, 192, 64, axis, T, Ld, 8) == 1, (nbits, axis, T, Ld)
            assert cov(nbits, 48, 192, 64, axis, F32, F32, 8) == 0        # an fp32 compute dtype
            assert cov(nbits, 40, 72, 8, axis, F16, F32, 8) == 1          # the edge shape of the GPU tests
    assert cov(0, 48, 192, 0, 0, F32, F32, 8) == 0
    assert cov(5, 48, 192, 64, 1, F16, F32, 8) == 0 and cov(6, 48, 192, 64, 1, F16, F32, 8) == 0   # no container of their own
    assert cov(4, 48, 192, 64, 2, F16, F32, 8) == 0                       # axis
    assert cov(4, 48, 192, 7, 1, F16, F32, 8) == 0                        # N K not divisible by the group size
    assert cov(4, 25, 100, 20, 1, F16, F32, 8) == 0                       # 125 unpacked rows do not pack in pairs ...
    assert cov(3, 25, 100, 20, 1, F16, F32, 8) == 1                       # ... but do in tens
    assert cov(4, 48, 192, 64, 1, F16, 3, 8) == 0                         # a uint8 adapter
    assert ops.lora_merge_covers(torch.float32, torch.float32, 48, 192, 64, 4, 1, 8) is False
    assert ops.lora_merge_covers(torch.float16, torch.float32, 48, 192, None, 4, 1, 8) is False
    assert ops.lora_merge_covers(torch.float16, torch.float32, 48, 192, 0, 0, 0, 8) is True
    # every case the GPU test compares is one the kernel serves
    for c in mc.CASES:
        nbits, axis, N, K, gs, r, T, Ld = c
        assert ops.lora_merge_covers(T, Ld, N, K, gs, nbits, axis, r), mc.case_id(c)


def test_bad_calls_are_refused_before_any_launch(L):
    P = 4096   # aligned and never read: each of these calls is refused before anything launches
    call = L.hqq_hip_lora_merge
    for args, rc, text in (
            ((4, P, P, P, P, P, 1.0, P, 48, 192, 64, 1, F16, F32, 0, None), UNSUPPORTED, b"rank 0"),
            ((4, P, P, P, P, P, 1.0, P, 48, 192, 64, 1, F16, F32, 257, None), UNSUPPORTED, b"rank 257"),
            ((4, P, P, P, P, P, 1.0, P, 48, 192, 64, 1, F32, F32, 8, None), UNSUPPORTED, b"fp32"),
            ((0, P, None, None, P, P, 1.0, P, 48, 192, 0, 0, F32, F32, 8, None), UNSUPPORTED, b"fp32"),
            ((5, P, P, P, P, P, 1.0, P, 48, 192, 64, 1, F16, F32, 8, None), NBITS_ERR, b"nbits=5"),
            ((4, P, P, P, P, P, 1.0, P, 48, 192, 64, 1, 3, F32, 8, None), DTYPE, b"dtype 3"),
            ((4, P, P, P, P, P, 1.0, P, 48, 192, 64, 1, F16, 3, 8, None), DTYPE, b"adapter dtype 3"),
            ((4, P, P, P, P, P, 1.0, P, 48, 192, 7, 1, F16, F32, 8, None), SHAPE, b"group_size=7"),
            ((4, P, P, P, P, P, 1.0, P, 48, 192, 64, 2, F16, F32, 8, None), SHAPE, b"bad axis 2"),
            ((4, P, P, P, P, P, 1.0, P, 25, 100, 20, 1, F16, F32, 8, None), SHAPE, b"not packable"),
            ((4, P, P, P, P, P, 1.0, P, 0, 192, 64, 1, F16, F32, 8, None), SHAPE, b"bad N / K"),
            ((4, None, P, P, P, P, 1.0, P, 48, 192, 64, 1, F16, F32, 8, None), SHAPE, b"null"),
            ((4, P, None, P, P, P, 1.0, P, 48, 192, 64, 1, F16, F32, 8, None), SHAPE, b"null"),
            ((0, P, None, None, P, None, 1.0, P, 48, 192, 0, 0, F16, F32, 8, None), SHAPE, b"null"),
            ((4, P, P, P, P + 2, P, 1.0, P, 48, 192, 64, 1, F16, F32, 8, None), -6, b"aligned"),      # an fp32 adapter off its element size
            ((4, P, P, P, P, P, 1.0, P + 1, 48, 192, 64, 1, F16, F16, 8, None), -6, b"aligned")):
        assert call(*args) == rc, args
        assert text in L.hqq_hip_last_error(), (args, L.hqq_hip_last_error())
    # null pointers are fine for a call that is refused for its configuration
    assert call(4, None, None, None, None, None, 1.0, None, 48, 192, 64, 1, F16, F32, 300, None) == UNSUPPORTED


def test_ops_validate_their_arguments_without_a_gpu():
    from hqq_amd import ops
    W_q = torch.zeros(24 * 192, dtype=torch.uint8)
    s = z = torch.zeros(48 * 192 // 64, dtype=torch.float16)
    A, B = torch.zeros(192, 8), torch.zeros(8, 48)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lora_merge(W_q, s, z, 48, 192, 64, 4, 1, A, B, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lora_merge_dense(torch.zeros(48, 192, dtype=torch.float16), A, B, 1.0)


# ---- PeftUtils.merge_lora on a toy tree: which wrappers are replaced, under which names, and when peft_config goes ----
class _Marker(nn.Module):
    def __init__(self, wrapper, cfg):
        super().__init__()
        object.__setattr__(self, "of", wrapper)   # (not registered as a submodule: the wrapper has left the tree)
        self.cfg = cfg


def _toy():
    class Attn(nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj, self.k_proj, self.v_proj = nn.Linear(8, 4), nn.Linear(8, 4, bias=False), nn.Linear(8, 4)

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.self_attn = Attn()
            self.mlp = nn.Sequential(nn.Linear(4, 4))

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = nn.ModuleList([Block(), Block()])
    return Toy()


def test_merge_lora_replaces_the_tagged_wrappers_only(monkeypatch):
    from hqq_amd.core.peft import HQQLinearLoRA, PeftUtils, is_hqq_lora_layer, patch_linear_merge_peft
    monkeypatch.setattr(HQQLinearLoRA, "merge_and_quantize", lambda self, cfg: _Marker(self, cfg))
    lora = {"r": 2, "lora_alpha": 4}
    model = _toy()
    PeftUtils.add_lora(model, {"self_attn.q_proj": dict(lora), "self_attn.k_proj": dict(lora), "self_attn.v_proj": dict(lora)})
    wrappers = {n: m for n, m in model.named_modules() if is_hqq_lora_layer(m)}
    assert len(wrappers) == 6
    qcfg, vcfg = {"weight_quant_params": {"nbits": 4}}, {"weight_quant_params": {"nbits": 2}}

    # q_proj and v_proj are merged, each with its own config; k_proj (mapped to None) stays; untagged linears are not touched
    PeftUtils.merge_lora(model, {"self_attn.q_proj": qcfg, "self_attn.k_proj": None, "self_attn.v_proj": vcfg})
    for i in range(2):
        attn = model.layers[i].self_attn
        assert isinstance(attn.q_proj, _Marker) and attn.q_proj.of is wrappers[f"layers.{i}.self_attn.q_proj"] and attn.q_proj.cfg is qcfg
        assert isinstance(attn.v_proj, _Marker) and attn.v_proj.cfg is vcfg
        assert attn.k_proj is wrappers[f"layers.{i}.self_attn.k_proj"]
        assert isinstance(model.layers[i].mlp[0], nn.Linear)
        assert attn.q_proj.name == f"layers.{i}.self_attn.q_proj" and attn.k_proj.name == f"layers.{i}.self_attn.k_proj"   # autoname_modules ran
    assert hasattr(model, "peft_config")          # two wrappers are left
    # a tag no wrapper carries changes nothing
    PeftUtils.merge_lora(model, {"mlp.0": qcfg})
    assert isinstance(model.layers[0].mlp[0], nn.Linear) and hasattr(model, "peft_config")
    # the last wrappers go, and peft_config with them
    PeftUtils.merge_lora(model, {"self_attn.k_proj": qcfg})
    assert not any(is_hqq_lora_layer(m) for m in model.modules()) and not hasattr(model, "peft_config")
    assert all(isinstance(model.layers[i].self_attn.k_proj, _Marker) for i in range(2))

    w = HQQLinearLoRA(nn.Linear(8, 4), dict(lora))
    assert patch_linear_merge_peft(w, None) is w and isinstance(patch_linear_merge_peft(w, qcfg), _Marker)


def test_merge_refuses_an_inference_only_layer_and_reads_scaling_once():
    from hqq_amd.backends.hip import HQQLinearHIP
    from hqq_amd.core.peft import HQQLinearLoRA
    assert HQQLinearLoRA.fused_merge is True
    w = HQQLinearLoRA(nn.Linear(8, 4), {"r": 2, "lora_alpha": 4})
    for s in (2.0, 2, torch.tensor(2.0, dtype=torch.float16), nn.Parameter(torch.tensor(2.0), requires_grad=False)):
        w.scaling = s
        assert w._scaling_float() == 2.0 and type(w._scaling_float()) is float
    hip = HQQLinearHIP.__new__(HQQLinearHIP)
    nn.Module.__init__(hip)
    w.linear_layer = hip
    with pytest.raises(NotImplementedError, match="before prepare_for_inference"):
        w.merge_and_quantize({"weight_quant_params": {"nbits": 4}})
