"""LoRA over quantised linears on the GPU (hqq_amd/core/peft.py): the wrapper's arithmetic in the reference's operation order, its gradients against a
torch-only replica, and PeftUtils on a tiny HF Llama — freeze, one backward step, save / load of the adapter file."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

BARS = dict(rtol=1e-3, atol=1e-3)   # fp16 against fp32-accumulated references: tests/test_axis0_gemm_gpu.py


def _wrapped(train_bias=False):
    from hqq_amd.core.peft import HQQLinearLoRA
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    torch.manual_seed(3)
    layer = HQQLinear(nn.Linear(256, 128, bias=True), BaseQuantizeConfig(nbits=4, group_size=64), compute_dtype=torch.float16, device="cuda")
    bias = layer.bias.clone()
    init = {"lora_A": torch.randn(256, 8) * 0.05, "lora_B": torch.randn(8, 128) * 0.05}
    lora = HQQLinearLoRA(layer, {"r": 8, "lora_alpha": 16, "dropout": 0.0, "lora_init": init, "train_bias": train_bias})
    return layer, lora, bias, init


def test_wrapper_arithmetic_in_the_reference_order():
    layer, lora, bias, init = _wrapped()
    assert layer.bias is None and torch.equal(lora.bias.data, bias) and not lora.bias.requires_grad   # the bias moved to the wrapper
    assert lora.scaling == 2.0 and lora.lora_A.dtype == torch.float32 and tuple(lora.lora_A.shape) == (256, 8) and tuple(lora.lora_B.shape) == (8, 128)
    x = torch.randn(5, 256, generator=torch.Generator().manual_seed(4)).half().cuda()
    with torch.no_grad():
        y = lora(x)
        want = layer(x)
        want += ((x.float() @ init["lora_A"].cuda()) @ init["lora_B"].cuda() * 2.0).to(x.dtype)
        want += bias
    assert y.dtype == torch.float16 and torch.equal(y, want)
    assert set(lora.state_dict()) == {"lora_A", "lora_B", "scaling", "bias"}


@pytest.mark.parametrize("routed", [False, True])
def test_gradients_match_a_torch_only_replica(monkeypatch, routed):
    """the replica: an nn.Linear holding layer.dequantize(), the same A / B.  The loss is linear in y with fixed coefficients, so that both sides
    back-propagate the same grad_output and differ by accumulation order only."""
    from hqq_amd import ops
    if routed:
        monkeypatch.setattr(ops, "DGRAD_ROUTE_MAX_M", 1 << 30)
    layer, lora, bias, init = _wrapped()
    W = layer.dequantize()
    x0 = torch.randn(2, 5, 256, generator=torch.Generator().manual_seed(5)).half().cuda()
    t = torch.randn(2, 5, 128, generator=torch.Generator().manual_seed(6)).half().cuda()

    x = x0.clone().requires_grad_(True)
    (lora(x).float() * t.float()).sum().backward()
    assert layer.W_q.grad is None and not layer.W_q.requires_grad and lora.bias.grad is None

    lin = nn.Linear(256, 128, bias=True).half().cuda()
    lin.weight.data, lin.bias.data = W.clone(), bias.clone()
    A, B = init["lora_A"].cuda().requires_grad_(True), init["lora_B"].cuda().requires_grad_(True)
    xr = x0.clone().requires_grad_(True)
    yr = lin(xr) + ((xr.float() @ A) @ B * 2.0).to(torch.float16)
    (yr.float() * t.float()).sum().backward()

    torch.testing.assert_close(lora.lora_A.grad, A.grad, **BARS)
    torch.testing.assert_close(lora.lora_B.grad, B.grad, **BARS)
    torch.testing.assert_close(x.grad.float(), xr.grad.float(), **BARS)
    assert x.grad.dtype == torch.float16 and lora.lora_A.grad.dtype == torch.float32


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=128)
    return LlamaForCausalLM(cfg).half().cuda().eval()


def _quantised_llama():
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    return quantize_model(_tiny_llama(), BaseQuantizeConfig(nbits=4, group_size=64), compute_dtype=torch.float16, device="cuda")


def test_peft_utils_on_a_tiny_llama(tmp_path):
    from hqq_amd.core.peft import PeftUtils, is_hqq_lora_layer
    cfg = {"r": 8, "lora_alpha": 16, "dropout": 0.0}
    peft_config = {"self_attn.q_proj": dict(cfg), "self_attn.k_proj": None, "self_attn.v_proj": dict(cfg), "self_attn.o_proj": None,
                   "mlp.gate_proj": None, "mlp.up_proj": None, "mlp.down_proj": None}
    model = _quantised_llama()
    PeftUtils.add_lora(model, peft_config)
    assert model.peft_config is peft_config
    wrapped = sorted(n for n, m in model.named_modules() if is_hqq_lora_layer(m))
    assert wrapped == sorted(f"model.layers.{i}.self_attn.{p}" for i in range(2) for p in ("q_proj", "v_proj"))
    want_trainable = sorted(f"{n}.{w}" for n in wrapped for w in ("lora_A", "lora_B"))
    assert sorted(n for n, p in model.named_parameters() if p.requires_grad) == want_trainable

    torch.manual_seed(7)
    for n in wrapped:   # a trained state: lora_B starts at zero
        m = model.get_submodule(n)
        m.lora_B.data = torch.randn_like(m.lora_B) * 0.05
    ids = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(8)).cuda()
    loss = model(input_ids=ids).logits.float().square().mean()
    loss.backward()
    with_grad = sorted(n for n, p in model.named_parameters() if p.grad is not None)
    assert with_grad == want_trainable
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n

    PeftUtils.cast_lora_weights(model, torch.float16)
    with torch.no_grad():
        logits = model(input_ids=ids).logits
    f = str(tmp_path / "lora.pt")
    PeftUtils.save_lora_weights(model, f)
    fresh = _quantised_llama()
    PeftUtils.load_lora_weights(fresh, f)
    assert sorted(n for n, m in fresh.named_modules() if is_hqq_lora_layer(m)) == wrapped
    with torch.no_grad():
        again = fresh(input_ids=ids).logits
    assert torch.equal(again, logits)
