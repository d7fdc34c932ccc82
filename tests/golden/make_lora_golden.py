#!/usr/bin/env python3
"""Write tests/golden/lora_state_dict.pt and tests/golden/lora_weights_v02.pt: what the REFERENCE (mobiusml/hqq) writes for LoRA adapters.

  lora_state_dict.pt    HQQLinearLoRA.state_dict() of one adapter (in 64, out 32, r 4, lora_alpha 8, a frozen bias, a non-zero lora_init)
  lora_weights_v02.pt   PeftUtils.save_lora_weights() of a two-block stub model with adapters on q_proj / v_proj: the v0.2 file
                        {"peft_config": ..., "parameters": {module_name: state_dict}}
tests/test_peft_cpu.py checks key names, shapes, dtypes and `scaling` against the first and loads the second through
hqq_amd.core.peft.PeftUtils.load_lora_weights, without the reference: the reference is needed only to regenerate the files.
The wrapped linears are plain nn.Linear on the CPU carrying a `compute_dtype` attribute (the reference reads it from HQQ layers; its branch for
other layers refers to an undefined name).

    HQQ_REFERENCE=<checkout of mobiusml/hqq> python tests/golden/make_lora_golden.py
"""
import os
import sys
import types

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"]


def _linear(i, o, bias):
    lin = nn.Linear(i, o, bias=bias)
    lin.compute_dtype = torch.float16
    return lin


class Attn(nn.Module):
    def __init__(self):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = _linear(64, 32, True), _linear(64, 32, False), _linear(64, 32, False)


class Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn = Attn()


class Stub(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([Block(), Block()])


class StubBase:
    """the two calls PeftUtils makes on a base class (hqq/models/base.py), over the stub model"""
    @classmethod
    def setup_model(cls, model):
        model.linear_tags = TAGS

    @classmethod
    def patch_linearlayers(cls, model, patch_fct, patch_params, verbose=True):
        for blk in model.layers:
            for tag in TAGS:
                parent = blk.self_attn
                child = tag.split(".")[-1]
                setattr(parent, child, patch_fct(getattr(parent, child), patch_params[tag]))


def main():
    ref = os.environ.get("HQQ_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set HQQ_REFERENCE to a checkout of mobiusml/hqq")
    stub = types.ModuleType("termcolor")   # hard import at hqq/core/quantize.py:13
    stub.colored = lambda t, *a, **k: t
    sys.modules.setdefault("termcolor", stub)
    sys.path.insert(0, ref)
    from hqq.core.peft import HQQLinearLoRA, PeftUtils

    torch.manual_seed(0)
    init = {"lora_A": torch.randn(64, 4) * 0.1, "lora_B": torch.randn(4, 32) * 0.1}
    one = HQQLinearLoRA(_linear(64, 32, True), {"r": 4, "lora_alpha": 8, "dropout": 0.0, "lora_init": init})
    torch.save(one.state_dict(), os.path.join(HERE, "lora_state_dict.pt"))

    model = Stub()
    model.base_class = StubBase
    cfg = {"r": 4, "lora_alpha": 8, "dropout": 0.0}
    PeftUtils.add_lora(model, {"self_attn.q_proj": dict(cfg), "self_attn.k_proj": None, "self_attn.v_proj": dict(cfg)}, verbose=False)
    for m in model.modules():
        if isinstance(m, HQQLinearLoRA):   # trained values: lora_B starts at zero
            m.lora_B.data = torch.randn_like(m.lora_B) * 0.1
    PeftUtils.cast_lora_weights(model, torch.float16, verbose=False)
    PeftUtils.save_lora_weights(model, os.path.join(HERE, "lora_weights_v02.pt"), verbose=False)
    for f in ("lora_state_dict.pt", "lora_weights_v02.pt"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
