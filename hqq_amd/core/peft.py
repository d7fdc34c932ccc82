"""LoRA adapters over quantised linears: the host mirror of hqq/core/peft.py.

`HQQLinearLoRA` wraps a linear (an `HQQLinear`, or any module with `in_features` / `out_features` / `bias`) and adds the trainable low-rank
pair lora_A [in, r], lora_B [r, out]: y = linear(x) + ((x @ A) @ B * scaling).to(x.dtype) (+ bias), in the reference's operation order.  The base layer
stays frozen; its gradient with respect to the input runs through HQQLinear's autograd route (fused `hqq_hip_gemm_dgrad` where HQQLinear routes it there,
`hqq_hip_gemm_dgrad_axis0` for a layer quantised along axis 0, dequantise + matmul elsewhere): the wrapper inherits the route from the layer it wraps
and holds no routing of its own.  `PeftUtils` adds the adapters to a whole model, casts them, and saves / loads them in the reference's v0.2 file format
({"peft_config": ..., "parameters": {module_name: state_dict}}), so that adapter files travel both ways.

Linears are found by qualified-name suffix ("tag"), exactly as `hqq_amd.utils.model.quantize_model` finds them; there is no model zoo and no base class.

`HQQLinearLoRA.merge_and_quantize` / `PeftUtils.merge_lora` fold a trained adapter back into a freshly quantised `HQQLinear` (peft.py:167-190, 396-404,
452-461): base weight + ((A @ B) * scaling)^T in one launch (`ops.lora_merge`, csrc/lora_merge.hip) where the kernel covers the layer, the reference's
torch statements elsewhere; the HIP quantiser takes it from there.  A merged model is an ordinary quantised model again: prepare_for_inference and the
fused decode step apply.

Not covered (the reference's experimental paths): HQQLinearLoRAWithFakeQuant, HQQLinearGroupedProj, and training through or merging from HQQLinearHIP
(backends/hip.py), which stays inference-only.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor, float16, float32, nn


def _get_dense_param(in_features: int, out_features: int, device="cuda", trainable: bool = True, dtype: torch.dtype = float32) -> nn.Parameter:
    """a trainable [in, out] matrix with nn.Linear's initialisation (peft.py:14-28)"""
    W = nn.Linear(in_features, out_features, bias=False).weight.data.t().to(dtype).to(device).contiguous()
    return nn.Parameter(W, requires_grad=trainable)


class HQQLinearLoRA(nn.Module):
    """peft.py:32-224.  peft_config: r, lora_alpha, and optionally dropout (0), train_dtype (fp32), train_bias (False),
    lora_init ({"lora_A": [in, r], "lora_B": [r, out]})."""

    def __init__(self, linear_layer: nn.Module, peft_config: dict):
        super().__init__()
        self.device = linear_layer.device if hasattr(linear_layer, "device") else next(linear_layer.parameters()).device
        self.train_dtype = peft_config.get("train_dtype", torch.float)

        self.linear_layer = linear_layer
        self.in_features = linear_layer.in_features
        self.out_features = linear_layer.out_features

        # the bias moves from the wrapped layer into the wrapper
        self.bias = None if linear_layer.bias is None else linear_layer.bias.clone()
        self.linear_layer.bias = None
        self.train_bias = peft_config.get("train_bias", False)
        if self.bias is not None:
            self.bias = nn.Parameter(self.bias, requires_grad=self.train_bias)
            if self.train_bias:
                self.bias.data = self.bias.data.to(self.train_dtype)
        elif self.train_bias:
            self.bias = nn.Parameter(torch.zeros((self.out_features,), device=self.device, dtype=self.train_dtype), requires_grad=True)

        p_drop = peft_config.get("dropout", 0.0)
        self.peft_drop = nn.Dropout(p=p_drop) if p_drop > 0.0 else nn.Identity()

        self.peft_config = peft_config
        self.lora_alpha = peft_config["lora_alpha"]
        self.r = peft_config["r"]
        self.scaling = self.lora_alpha / self.r
        self.lora_A = _get_dense_param(self.in_features, self.r, device=self.device, trainable=True, dtype=self.train_dtype)
        self.lora_B = _get_dense_param(self.r, self.out_features, device=self.device, trainable=True, dtype=self.train_dtype)
        if "lora_init" in peft_config:
            init = peft_config["lora_init"]
            assert (init["lora_A"].shape[0], init["lora_B"].shape[1]) == (self.in_features, self.out_features), (
                f"Invalid init LoRA weight shapes. Expected: lora_A: {self.in_features} x r , lora_B: r x {self.out_features})")
            self.lora_A.data = init["lora_A"].to(device=self.device, dtype=self.train_dtype)
            self.lora_B.data = init["lora_B"].to(device=self.device, dtype=self.train_dtype)
        else:   # as the original LoRA implementation
            nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))
            nn.init.zeros_(self.lora_B)

        # compute dtype: what load_state_dict casts to (inference)
        if hasattr(self.linear_layer, "compute_dtype"):
            self.compute_dtype = self.linear_layer.compute_dtype
        else:
            fp = [p for p in self.linear_layer.parameters() if p.is_floating_point()]
            self.compute_dtype = fp[0].dtype if fp else self.train_dtype

    def forward_lora(self, x: Tensor) -> Tensor:   # in lora_A's dtype
        return torch.matmul(torch.matmul(self.peft_drop(x.to(self.lora_A.dtype)), self.lora_A), self.lora_B) * self.scaling

    def forward(self, x: Tensor) -> Tensor:
        x_dtype = x.dtype
        # the reference's operations in its order, out of place: with a gradient flowing, HQQLinear's output is a view made inside its autograd
        # function, which autograd does not allow to be modified in place
        out = self.linear_layer(x)
        if self.train_bias:
            out = out + (self.forward_lora(x) + self.bias).to(x_dtype)
        else:
            out = out + self.forward_lora(x).to(x_dtype)
            if self.bias is not None:
                out = out + self.bias
        return out

    # merge_and_quantize builds the merged weight in ONE launch (ops.lora_merge for a wrapped HQQLinear, ops.lora_merge_dense for a wrapped nn.Linear)
    # wherever ops.lora_merge_covers says so.  HQQLinearLoRA.fused_merge = False keeps the torch composition everywhere (the counterpart of
    # HQQLinear.fused_backward).
    fused_merge = True

    def _scaling_float(self) -> float:
        """`scaling` as load_state_dict can leave it (a number, a tensor, a parameter), read once"""
        s = self.scaling
        return float(s.detach().float().item()) if isinstance(s, Tensor) else float(s)

    def _base_weight(self) -> Tensor:
        """the wrapped layer's [out, in] weight, a tensor of its own: what the reference obtains by pushing an identity through the forward (peft.py:169-176)
        for whatever linear it wraps; here the two kinds of linear a model holds are read directly"""
        from .quantize import HQQLinear
        if isinstance(self.linear_layer, HQQLinear):
            return self.linear_layer.dequantize()
        if isinstance(self.linear_layer, nn.Linear):
            return self.linear_layer.weight.data.clone()
        raise NotImplementedError(f"hqq_amd: merging into a wrapped {type(self.linear_layer).__name__} is not covered (HQQLinear or nn.Linear)")

    def _merged_weight_fused(self, scaling: float) -> Optional[Tensor]:
        """base weight + adapter through hqq_hip_lora_merge, or None where the kernel does not cover the layer"""
        from .. import ops
        from .quantize import HQQLinear, Quantizer
        ll, A, B = self.linear_layer, self.lora_A.data, self.lora_B.data
        if not (A.is_cuda and B.is_cuda and A.dtype == B.dtype):
            return None
        if isinstance(ll, HQQLinear):
            meta = ll.meta
            if not (ll.ready and meta.get("packing")) or not ll.W_q.is_cuda:
                return None
            N, K = meta["shape"]
            axis = meta["axis"]
            gs = meta["group_size"] if meta["group_size"] else (K if axis == 1 else N)
            nbits = Quantizer._packing_bits[meta["packing"]]
            scale, zero = meta["scale"].reshape(-1), meta["zero"].reshape(-1)
            if scale.numel() != (N * K) // gs or zero.numel() != scale.numel() or scale.dtype != zero.dtype:   # (channel_wise=False: one pair per tensor)
                return None
            if not ops.lora_merge_covers(scale.dtype, A.dtype, N, K, gs, nbits, axis, self.r):
                return None
            W_q = ll.W_q.view(meta["unpack_view_dtype"]) if meta["view_as_float"] else ll.W_q
            return ops.lora_merge(W_q, scale, zero, N, K, gs, nbits, axis, A, B, scaling)
        if isinstance(ll, nn.Linear):
            W = ll.weight.data
            if not W.is_cuda or not ops.lora_merge_covers(W.dtype, A.dtype, W.shape[0], W.shape[1], 0, 0, 0, self.r):
                return None
            return ops.lora_merge_dense(W, A, B, scaling)
        return None

    def merge_and_quantize(self, quant_config: dict):
        """peft.py:167-190: the base weight, `W += (A @ B * scaling).t().to(W.dtype)`, `HQQLinear(None, quant_config).quantize(W, **quant_config)`; the new
        layer's bias is a clone of the wrapper's (or None).  Deliberately different from the reference: the new layer takes the wrapped layer's compute
        dtype and device (the reference's HQQLinear(None, quant_config) falls back to fp16 / "cuda" whatever the layer was), and the bias is cast to that
        compute dtype (a trained bias is in train_dtype)."""
        from ..backends.hip import HQQLinearHIP
        from .quantize import HQQLinear
        if isinstance(self.linear_layer, HQQLinearHIP):
            raise NotImplementedError("hqq_amd: a wrapped HQQLinearHIP is inference-only (its container may be re-laid out): merge the adapters before "
                                      "prepare_for_inference")
        scaling = self._scaling_float()
        W = self._merged_weight_fused(scaling) if HQQLinearLoRA.fused_merge else None
        if W is None:   # outside the kernel's coverage (an fp32 compute dtype, r > 256, a CPU layer, ...) or switched off: the same torch statements
            W = self._base_weight()
            W += (torch.matmul(self.lora_A.data, self.lora_B.data) * scaling).t().to(W.dtype)
        new_layer = HQQLinear(None, {"offload_meta": False, **quant_config}, compute_dtype=self.compute_dtype, device=self.device)
        new_layer.bias = None if self.bias is None else self.bias.data.clone().to(device=self.device, dtype=self.compute_dtype)
        wq = dict(quant_config["weight_quant_params"])
        if wq.get("group_size") is None:   # one group per row / column, as HQQLinear.initialize resolves it
            wq["group_size"] = self.in_features if wq.get("axis") == 1 else self.out_features
        new_layer.quantize(W, wq, quant_config.get("scale_quant_params"), quant_config.get("zero_quant_params"))
        return new_layer

    def cast(self, dtype: torch.dtype = float16):
        self.lora_A.data = self.lora_A.data.to(dtype)
        self.lora_B.data = self.lora_B.data.to(dtype)
        if self.bias is not None:
            self.bias.data = self.bias.data.to(dtype)
        if isinstance(self.scaling, nn.Parameter):
            self.scaling.data = self.scaling.data.to(dtype)
        elif isinstance(self.scaling, Tensor):
            self.scaling = self.scaling.to(dtype)
        return self

    def state_dict(self, *args, **kwargs):
        return {"lora_A": self.lora_A.data, "lora_B": self.lora_B.data, "scaling": self.scaling, "bias": self.bias}

    def load_state_dict(self, state_dict, *args, **kwargs):
        to = dict(device=self.device, dtype=self.compute_dtype)
        self.lora_A.data = state_dict["lora_A"].data.to(**to)
        self.lora_B.data = state_dict["lora_B"].data.to(**to)
        if state_dict["bias"] is not None:
            if self.bias is None:   # (the reference fails on None.data here; a file that carries a bias gets it)
                self.bias = nn.Parameter(state_dict["bias"].data.to(**to), requires_grad=self.train_bias)
            else:
                self.bias.data = state_dict["bias"].data.to(**to)
        scaling = state_dict["scaling"]
        if isinstance(scaling, nn.Parameter):
            self.scaling = nn.Parameter(scaling.data.to(**to), requires_grad=scaling.requires_grad)
        elif isinstance(scaling, Tensor):
            self.scaling = scaling.to(**to)
        elif isinstance(scaling, (int, float)):
            self.scaling = scaling


_HQQ_LORA_CLASSES = [HQQLinearLoRA]
_HQQ_LORA_MAPPING = {"default": HQQLinearLoRA}


def is_hqq_lora_layer(layer) -> bool:
    return type(layer) in _HQQ_LORA_CLASSES


def autoname_modules(model: nn.Module) -> None:
    for name, module in model.named_modules():
        module.name = name


def _is_linear(mod: nn.Module) -> bool:
    from .quantize import HQQLinear   # (imported late: this module loads without the native library)
    return isinstance(mod, (nn.Linear, HQQLinear))


def patch_linear_add_peft(layer: nn.Module, patch_params: Optional[dict]) -> nn.Module:
    if not patch_params:
        return layer
    lora_type = patch_params.get("lora_type", "default")
    if lora_type not in _HQQ_LORA_MAPPING:
        raise NotImplementedError(f"hqq_amd: lora_type {lora_type!r} is not covered (only 'default')")
    return _HQQ_LORA_MAPPING[lora_type](layer, patch_params)


def patch_linear_merge_peft(layer: nn.Module, quant_config: Optional[dict]) -> nn.Module:
    """peft.py:396-404: the merged, re-quantised layer, or the wrapper itself where no quant config is given"""
    if not quant_config:
        return layer
    return layer.merge_and_quantize(quant_config)


def _lora_layers(model: nn.Module):
    return [(name, mod) for name, mod in model.named_modules() if is_hqq_lora_layer(mod)]


class PeftUtils:
    """peft.py:414-555 without the model zoo: the linears are the modules whose qualified name ends with a key of peft_config."""

    @classmethod
    def add_lora(cls, model: nn.Module, peft_config: Dict[str, Optional[dict]], base_class=None, verbose: bool = False) -> None:
        for param in model.parameters():
            param.requires_grad = False
        tags = list(peft_config)
        todo = []
        for name, mod in model.named_modules():
            if _is_linear(mod):
                tag = next((t for t in tags if name.endswith(t)), None)
                if tag is not None and peft_config.get(tag):
                    todo.append((name, tag))
        for name, tag in todo:
            parent_name, _, child = name.rpartition(".")
            parent = model.get_submodule(parent_name) if parent_name else model
            setattr(parent, child, patch_linear_add_peft(getattr(parent, child), peft_config[tag]))
            if verbose:
                print(f"lora {name}")
        autoname_modules(model)
        model.peft_config = peft_config

    @classmethod
    def merge_lora(cls, model: nn.Module, merge_lora_params: Dict[str, Optional[dict]], base_class=None, verbose: bool = False) -> None:
        """peft.py:452-461: every HQQLinearLoRA whose qualified name ends with a key of merge_lora_params that maps to a quant config is replaced in its
        parent by the merged HQQLinear; a key mapped to None (or a wrapper no key matches) stays.  model.peft_config goes once no wrapper is left."""
        tags = list(merge_lora_params)
        todo = []
        for name, mod in _lora_layers(model):
            tag = next((t for t in tags if name.endswith(t)), None)
            if tag is not None and merge_lora_params.get(tag):
                todo.append((name, tag))
        for name, tag in todo:
            parent_name, _, child = name.rpartition(".")
            parent = model.get_submodule(parent_name) if parent_name else model
            setattr(parent, child, patch_linear_merge_peft(getattr(parent, child), merge_lora_params[tag]))
            if verbose:
                print(f"merged {name}")
        autoname_modules(model)
        if not _lora_layers(model) and hasattr(model, "peft_config"):
            del model.peft_config
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    @classmethod
    def cast_lora_weights(cls, model: nn.Module, dtype: torch.dtype, base_class=None, verbose: bool = False) -> None:
        for _, layer in _lora_layers(model):
            layer.cast(dtype)

    @classmethod
    def save_lora_weights(cls, model: nn.Module, filename: str, base_class=None, verbose: bool = False) -> None:
        autoname_modules(model)
        params = {layer.name: layer.state_dict() for _, layer in _lora_layers(model)}
        torch.save({"peft_config": model.peft_config, "parameters": params}, filename)

    @classmethod
    def load_lora_weights(cls, model: nn.Module, filename: str, base_class=None, verbose: bool = False) -> None:
        lora_data = torch.load(filename, map_location="cpu", weights_only=True)
        if ("peft_config" in lora_data) and ("parameters" in lora_data):   # v0.2: the adapters are created where the model has none
            params = lora_data["parameters"]
            if not hasattr(model, "peft_config"):
                cls.add_lora(model=model, peft_config=lora_data["peft_config"])
        else:                                                               # v0.1: the bare {module_name: state_dict}
            if not hasattr(model, "peft_config"):
                raise Exception("Using older version of lora weights. LoRa modules should be manually added in this case.")
            params = lora_data
        autoname_modules(model)
        for _, layer in _lora_layers(model):
            layer.load_state_dict(params[layer.name])


class LoRABank:
    """Several adapters for ONE adapted model, stacked per wrapper so that the fused decode step can pick one per batch row on the device
    (ops.lora_shrink_routed / ops.lora_expand_routed; llama_fused.FusedLlamaStep(lora=True, lora_bank=bank)).

    `model` already carries its HQQLinearLoRA wrappers (PeftUtils.add_lora).  Every adapter is a {module_name: state_dict} dictionary keyed by
    autoname_modules names — what PeftUtils.save_lora_weights writes as "parameters" (v0.2), or the bare v0.1 dictionary.  Per wrapper the bank holds
    A [n, K, r] and B [n, r, N] in `dtype` (default: the dtype of the wrapper's lora_A) and scaling float32 [n] — float32(float(scaling)), the value the
    one-adapter kernels are passed as a host float — all on the wrapper's device.  Refused, each with a ValueError that names the layer and the adapter's
    index: an adapter that lacks a wrapped layer, lora_A / lora_B of another shape than the wrapper's [K, r] / [r, N] (one rank per layer across the
    bank), a bias that is not None, lora_A and lora_B of different dtypes.

    The tensors are allocated once: set() and activate() copy in place, so a decode step or a captured graph built on the bank stays valid whatever
    is loaded into it later.  activate(model, i) makes the WRAPPERS hold adapter i (or no adapter: i = -1 zeroes lora_B), which is how the model's own
    forward — the prefill, the composed decode route — runs under an adapter of the bank; the wrappers are left holding the last adapter activated."""

    def __init__(self, model: nn.Module, adapters, dtype: Optional[torch.dtype] = None):
        autoname_modules(model)
        self.names = [name for name, _ in _lora_layers(model)]
        if not self.names:
            raise ValueError("hqq_amd: LoRABank needs a model that carries HQQLinearLoRA wrappers (PeftUtils.add_lora)")
        adapters = list(adapters)
        if not adapters:
            raise ValueError("hqq_amd: LoRABank needs at least one adapter")
        self.n = len(adapters)
        self._layers = {}
        self._host_scaling = {name: [0.0] * self.n for name in self.names}   # the float32 values of the scaling tensors, as Python floats (activate reads these)
        for name, w in _lora_layers(model):
            dt = w.lora_A.dtype if dtype is None else dtype
            K, r, N = w.in_features, w.r, w.out_features
            dev = w.lora_A.device
            self._layers[name] = (torch.empty(self.n, K, r, dtype=dt, device=dev), torch.empty(self.n, r, N, dtype=dt, device=dev),
                                  torch.empty(self.n, dtype=float32, device=dev))
        for i, params in enumerate(adapters):
            self.set(i, params)

    @staticmethod
    def _params(file_or_params) -> dict:
        """the {module_name: state_dict} dictionary of a file PeftUtils.save_lora_weights wrote (v0.2, or the bare v0.1 form), or of such a dictionary"""
        data = file_or_params
        if not isinstance(data, dict):
            data = torch.load(data, map_location="cpu", weights_only=True)
        if ("peft_config" in data) and ("parameters" in data):
            data = data["parameters"]
        return data

    @classmethod
    def from_files(cls, model: nn.Module, filenames, dtype: Optional[torch.dtype] = None) -> "LoRABank":
        return cls(model, [cls._params(f) for f in filenames], dtype)

    @classmethod
    def from_params(cls, model: nn.Module, parameters, dtype: Optional[torch.dtype] = None) -> "LoRABank":
        return cls(model, [cls._params(p) for p in parameters], dtype)

    @staticmethod
    def _scaling(s) -> float:
        return float(s.detach().float().item()) if isinstance(s, Tensor) else float(s)

    def set(self, i: int, file_or_params) -> None:
        """adapter `i` <- the file or dictionary, copied into the bank's tensors in place (their addresses stay: no step or graph is invalidated)"""
        if not 0 <= int(i) < self.n:
            raise ValueError(f"hqq_amd: LoRABank.set: adapter index {i} outside 0 .. {self.n - 1}")
        params = self._params(file_or_params)
        checked = []
        for name in self.names:
            A_bank, B_bank, _ = self._layers[name]
            sd = params.get(name) if isinstance(params, dict) else None
            if not isinstance(sd, dict) or any(k not in sd for k in ("lora_A", "lora_B", "scaling")):
                raise ValueError(f"hqq_amd: LoRABank: adapter {i} has no entry for the adapted layer {name!r}")
            A, B = sd["lora_A"], sd["lora_B"]
            A, B = getattr(A, "data", A), getattr(B, "data", B)
            if tuple(A.shape) != tuple(A_bank.shape[1:]) or tuple(B.shape) != tuple(B_bank.shape[1:]):
                raise ValueError(f"hqq_amd: LoRABank: adapter {i}, layer {name!r}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} where the wrapper has "
                                 f"{tuple(A_bank.shape[1:])} / {tuple(B_bank.shape[1:])} (one rank per layer across the bank)")
            if sd.get("bias") is not None:
                raise ValueError(f"hqq_amd: LoRABank: adapter {i}, layer {name!r} carries a bias, which the routed kernels do not serve")
            if A.dtype != B.dtype:
                raise ValueError(f"hqq_amd: LoRABank: adapter {i}, layer {name!r}: lora_A is {A.dtype} and lora_B {B.dtype} (mixed dtypes)")
            checked.append((name, A, B, self._scaling(sd["scaling"])))
        for name, A, B, s in checked:   # (nothing is written before the whole adapter has been accepted)
            A_bank, B_bank, sc = self._layers[name]
            A_bank[i].copy_(A)
            B_bank[i].copy_(B)
            sc[i] = s
            self._host_scaling[name][i] = float(torch.tensor(s, dtype=float32))

    def layer(self, name: str):
        """(A [n, K, r], B [n, r, N], scaling float32 [n]) of the wrapper called `name`"""
        return self._layers[name]

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for ts in self._layers.values() for t in ts)

    def pointers(self) -> tuple:
        """the addresses of the bank's tensors and n: what a decoder keeps its step and graphs by"""
        return (self.n,) + tuple(t.data_ptr() for name in self.names for t in self._layers[name])

    def scaling_key(self, i: int):
        """adapter i's scalings over the bank's layers as a hashable value (None for -1): what a captured forward of the WRAPPERS depends on beyond the
        tensors activate() rewrites in place — `scaling` is a Python float there, a constant of the capture"""
        return None if int(i) < 0 else tuple(self._host_scaling[name][int(i)] for name in self.names)

    def activate(self, model: nn.Module, i: int) -> None:
        """the model's wrappers <- adapter i, in place (lora_A.data.copy_, lora_B.data.copy_, scaling as a Python float); i = -1: lora_B <- 0, the base
        model.  The wrappers are left holding it."""
        i = int(i)
        if not -1 <= i < self.n:
            raise ValueError(f"hqq_amd: LoRABank.activate: adapter index {i} outside -1 .. {self.n - 1}")
        wrappers = dict(_lora_layers(model))
        if sorted(wrappers) != sorted(self.names):
            raise ValueError("hqq_amd: LoRABank.activate: the model's wrappers are not the ones the bank was stacked for")
        for name in self.names:
            w = wrappers[name]
            A_bank, B_bank, sc = self._layers[name]
            if i < 0:
                w.lora_B.data.zero_()
                continue
            w.lora_A.data.copy_(A_bank[i])
            w.lora_B.data.copy_(B_bank[i])
            w.scaling = self._host_scaling[name][i]
