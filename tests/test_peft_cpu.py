"""CPU tests of hqq_amd.core.peft against what the reference writes (tests/golden/make_lora_golden.py): the adapter's state dict key by key, and a
reference-written v0.2 weights file loaded through PeftUtils.load_lora_weights on a stub model."""
import os

import torch
from torch import nn

from conftest import GOLDEN


def _linear(i, o, bias):
    return nn.Linear(i, o, bias=bias)


class Attn(nn.Module):
    def __init__(self):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = _linear(64, 32, True), _linear(64, 32, False), _linear(64, 32, False)

    def forward(self, x):
        return self.q_proj(x) + self.k_proj(x) + self.v_proj(x)


class Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn = Attn()


class Stub(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([Block(), Block()])


def test_module_imports_without_a_gpu():
    from hqq_amd.core import peft
    assert {"HQQLinearLoRA", "PeftUtils", "is_hqq_lora_layer", "autoname_modules"} <= set(dir(peft))


def test_state_dict_matches_the_reference_key_by_key():
    from hqq_amd.core.peft import HQQLinearLoRA
    want = torch.load(os.path.join(GOLDEN, "lora_state_dict.pt"), map_location="cpu", weights_only=True)
    torch.manual_seed(1)
    layer = HQQLinearLoRA(_linear(64, 32, True), {"r": 4, "lora_alpha": 8, "dropout": 0.0})
    got = layer.state_dict()
    assert list(got) == list(want) == ["lora_A", "lora_B", "scaling", "bias"]
    for k in ("lora_A", "lora_B", "bias"):
        assert type(got[k]) is type(want[k]) and got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    assert isinstance(got["scaling"], float) and got["scaling"] == want["scaling"] == 2.0
    assert layer.linear_layer.bias is None and not layer.bias.requires_grad      # the bias moved into the wrapper, frozen
    assert layer.lora_A.requires_grad and layer.lora_B.requires_grad
    # zero B; Kaiming-uniform A (a = sqrt 5) on the [in, r] tensor: torch takes the second dimension as fan-in, so the bound is 1 / sqrt(r)
    assert bool((layer.lora_B.data == 0).all()) and 0.0 < float(layer.lora_A.data.abs().max()) <= 1.0 / 4 ** 0.5
    # the reference's own state dict loads (cast to the compute dtype, the wrapped layer's parameter dtype here)
    layer.load_state_dict(want)
    assert torch.equal(layer.lora_A.data, want["lora_A"]) and torch.equal(layer.lora_B.data, want["lora_B"]) and torch.equal(layer.bias.data, want["bias"].data)
    # forward: the reference's operation order
    x = torch.randn(3, 64)
    y = layer(x)
    ref = layer.linear_layer(x)
    ref += (torch.matmul(torch.matmul(x, want["lora_A"]), want["lora_B"]) * 2.0).to(x.dtype)
    ref += want["bias"].data
    assert torch.equal(y, ref)


def test_reference_written_weights_file_loads():
    from hqq_amd.core.peft import HQQLinearLoRA, PeftUtils, is_hqq_lora_layer
    path = os.path.join(GOLDEN, "lora_weights_v02.pt")
    data = torch.load(path, map_location="cpu", weights_only=True)
    assert set(data) == {"peft_config", "parameters"}
    model = Stub()
    PeftUtils.load_lora_weights(model, path)     # no adapters yet: the v0.2 file creates them from its own peft_config
    assert model.peft_config == data["peft_config"]
    wrapped = sorted(n for n, m in model.named_modules() if is_hqq_lora_layer(m))
    assert wrapped == sorted(data["parameters"]) == ["layers.0.self_attn.q_proj", "layers.0.self_attn.v_proj", "layers.1.self_attn.q_proj", "layers.1.self_attn.v_proj"]
    assert isinstance(model.layers[0].self_attn.k_proj, nn.Linear)   # its tag carries None
    for name in wrapped:
        layer, sd = model.get_submodule(name), data["parameters"][name]
        assert isinstance(layer, HQQLinearLoRA) and layer.name == name
        assert torch.equal(layer.lora_A.data, sd["lora_A"].float()) and torch.equal(layer.lora_B.data, sd["lora_B"].float())
        assert layer.scaling == sd["scaling"] == 2.0
        assert (layer.bias is None) == (sd["bias"] is None)
        if layer.bias is not None:
            assert torch.equal(layer.bias.data, sd["bias"].data.float())
    trainable = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    assert trainable == sorted(f"{n}.{w}" for n in wrapped for w in ("lora_A", "lora_B"))


def test_save_then_load_round_trips(tmp_path):
    from hqq_amd.core.peft import PeftUtils, is_hqq_lora_layer
    torch.manual_seed(2)
    a = Stub()
    cfg = {"r": 4, "lora_alpha": 8, "dropout": 0.0}
    PeftUtils.add_lora(a, {"self_attn.q_proj": dict(cfg), "self_attn.k_proj": None, "self_attn.v_proj": dict(cfg)})
    for m in a.modules():
        if is_hqq_lora_layer(m):
            m.lora_B.data = torch.randn_like(m.lora_B) * 0.1
    f = str(tmp_path / "lora.pt")
    PeftUtils.save_lora_weights(a, f)
    saved = torch.load(f, map_location="cpu", weights_only=True)
    ref = torch.load(os.path.join(GOLDEN, "lora_weights_v02.pt"), map_location="cpu", weights_only=True)
    assert set(saved) == set(ref) and sorted(saved["parameters"]) == sorted(ref["parameters"]) and saved["peft_config"] == ref["peft_config"]
    for name in ref["parameters"]:
        assert list(saved["parameters"][name]) == list(ref["parameters"][name])
    b = Stub()
    PeftUtils.load_lora_weights(b, f)
    for name in ref["parameters"]:
        la, lb = a.get_submodule(name), b.get_submodule(name)
        assert torch.equal(la.lora_A, lb.lora_A) and torch.equal(la.lora_B, lb.lora_B)
