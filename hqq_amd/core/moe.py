"""HQQExperts — the fused experts module of a mixture-of-experts block, quantised (the reference patches Mixtral's per-expert linears:
hqq/models/hf/mixtral.py; transformers 5 keeps the experts of every MoE family in ONE module of two 3-D parameters instead).

The module it replaces has `gate_up_proj [E, 2I, H]`, `down_proj [E, H, I]`, `act_fn` and `forward(hidden_states, top_k_index, top_k_weights)`
(MixtralExperts, Qwen2MoeExperts, Qwen3MoeExperts, OlmoeExperts, PhimoeExperts, DeepseekV3NaiveMoe's experts).  Every expert's gate, up and down
slice is quantised on its own by the call HQQLinear makes (Quantizer.quantize), so expert e's W_q / scale / zero are what HQQLinear gives for a linear
holding that slice; they are kept in one dense, expert-major buffer per role and kind (`gate_W_q [E, ...]`, `gate_scale`, `gate_zero`, the same for
`up` and `down`), which is what lets a kernel reach expert e at base + e * stride.

Two routes.  Composed: HF's own loop, with the quantised linear in place of F.linear — any configuration, any number of rows, CPU tensors too (a CPU
tensor meets the reference's dequantise formula in torch ops; GPU tensors go through hqq_amd.ops.forward).  Fused: hqq_amd.ops.moe_forward, two
launches, no host read of the routing — the one a graph can capture.  `HQQExperts.fused` (class attribute) = None: fused where ops.moe_covers holds and
the token count is at most ops.MOE_ROUTE_MAX_T, else composed; True: fused or an error; False: always composed.
The composed route reads the routing on the host, so a graph capture of the module needs the fused route: at most ops.MOE_ROUTE_MAX_T tokens, or
`HQQExperts.fused = True` (up to ops.MOE_MAX_T tokens; slower than composing where profiles/moe_summary.md says so).
"""
from __future__ import annotations

import copy
from typing import Union

import torch
from torch import Tensor, float16, nn

from .. import ops
from .quantize import HQQLinear, Quantizer

ROLES = ("gate", "up", "down")
_KINDS = ("W_q", "scale", "zero")
_DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


def is_experts_module(mod) -> bool:
    """the parameter layout of transformers' fused experts modules: gate_up_proj [E, 2I, H], down_proj [E, H, I], act_fn"""
    gu, dn = getattr(mod, "gate_up_proj", None), getattr(mod, "down_proj", None)
    return (isinstance(gu, (nn.Parameter, Tensor)) and isinstance(dn, (nn.Parameter, Tensor)) and gu.dim() == 3 and dn.dim() == 3 and hasattr(mod, "act_fn")
            and gu.shape[0] == dn.shape[0] and gu.shape[1] == 2 * dn.shape[2] and gu.shape[2] == dn.shape[1])


def _is_silu(act) -> bool:
    if isinstance(act, nn.SiLU) or act is torch.nn.functional.silu:
        return True
    return type(act).__name__ in ("SiLUActivation", "SiLU")


def _dequantize_host(W_q: Tensor, meta: dict) -> Tensor:
    """Quantizer.dequantize for CPU tensors, as the reference states it (quantize.py:183-199): unpack, (W_q - zero) * scale in the compute dtype, reshape"""
    nbits = Quantizer._packing_bits[meta["packing"]]
    if nbits == 3:
        raise NotImplementedError("hqq_amd: the 3-bit container has no host dequantise in HQQExperts; move the module to the GPU")
    if meta["view_as_float"]:
        W_q = W_q.view(meta["unpack_view_dtype"])
    per = 8 // nbits
    mask = (1 << nbits) - 1
    W_r = torch.cat([(W_q >> (nbits * (per - 1 - s))) & mask for s in range(per)], dim=0).to(meta["scale"].dtype)   # slab 0 most significant (bitpack.py)
    return ((W_r - meta["zero"]) * meta["scale"]).reshape(meta["shape"])


class HQQExperts(nn.Module):
    fused: Union[bool, None] = None   # class-wide route override, like HQQLinear.fused_backward

    def __init__(self, experts_module: Union[nn.Module, None], quant_config: Union[dict, None], compute_dtype: torch.dtype = float16, device: str = "cuda",
                 solver_dtype: torch.dtype = torch.float32, del_orig: bool = True):
        super().__init__()
        self.compute_dtype = compute_dtype
        self.device = device
        self.solver_dtype = solver_dtype
        self.quant_config = copy.deepcopy(quant_config)
        self.act_fn = nn.SiLU()
        self.num_experts = self.hidden_dim = self.intermediate_dim = None
        self.layer_meta = None   # role -> the non-tensor entries of Quantizer.quantize's meta (the same for every expert of the role)
        for role in ROLES:
            for kind in _KINDS:
                self.register_buffer(f"{role}_{kind}", None)
        self.ready = False
        if experts_module is not None:
            self._quantize(experts_module, del_orig)

    # ---- construction -------------------------------------------------------------------------------------------------------------------------------
    def _quantize(self, mod: nn.Module, del_orig: bool) -> None:
        if not is_experts_module(mod):
            raise ValueError("hqq_amd: HQQExperts takes a module with gate_up_proj [E, 2I, H], down_proj [E, H, I] and act_fn")
        if not _is_silu(mod.act_fn):
            raise NotImplementedError(f"hqq_amd: HQQExperts covers SiLU experts, not {type(mod.act_fn).__name__}")
        gu, dn = mod.gate_up_proj.data, mod.down_proj.data
        E, I, H = int(dn.shape[0]), int(dn.shape[2]), int(dn.shape[1])
        self.num_experts, self.hidden_dim, self.intermediate_dim = E, H, I
        # as HQQLinear.initialize: quantised scale / zero and meta offloading are deprecated in the reference and ignored
        self.quant_config["scale_quant_params"] = None
        self.quant_config["zero_quant_params"] = None
        self.quant_config.pop("offload_meta", None)
        self.layer_meta = {}
        stacks = {}
        for e in range(E):
            slices = {"gate": gu[e, :I], "up": gu[e, I:], "down": dn[e]}
            for role in ROLES:   # three separate layers: the solver's early stop is global per layer
                W = slices[role]
                wq = dict(self.quant_config["weight_quant_params"])
                if wq["group_size"] is None:
                    wq["group_size"] = int(W.shape[1]) if wq["axis"] == 1 else int(W.shape[0])
                W_q, meta = Quantizer.quantize(W, device=self.device, compute_dtype=self.compute_dtype, solver_dtype=self.solver_dtype, **wq)
                meta.update({"quant_scale": False, "quant_zero": False, "compute_dtype": self.compute_dtype})
                W_q, meta = Quantizer.cuda(W_q, meta, self.device)   # scale / zero in the compute dtype, as HQQLinear.cuda leaves them
                if e == 0:
                    self.layer_meta[role] = {k: v for k, v in meta.items() if not isinstance(v, Tensor)}
                    for kind, t in (("W_q", W_q), ("scale", meta["scale"]), ("zero", meta["zero"])):
                        stacks[role, kind] = torch.empty((E,) + tuple(t.shape), dtype=t.dtype, device=t.device)
                for kind, t in (("W_q", W_q), ("scale", meta["scale"]), ("zero", meta["zero"])):
                    stacks[role, kind][e].copy_(t)
        for (role, kind), t in stacks.items():
            setattr(self, f"{role}_{kind}", t)
        if del_orig:
            mod.gate_up_proj = None
            mod.down_proj = None
        self.ready = True

    @classmethod
    def from_stacks(cls, stacks: dict, layer_meta: dict, quant_config: dict, compute_dtype: torch.dtype = float16, device: str = "cuda"):
        """an HQQExperts over stacks that exist already — {(role, kind): tensor [E, ...]} with the per-role meta of Quantizer.quantize (no tensors) —
        nothing quantised again: what load_state_dict does, for a caller that holds the tensors"""
        self = cls(None, quant_config, compute_dtype=compute_dtype, device=device)
        self.layer_meta = {r: dict(layer_meta[r]) for r in ROLES}
        for r in ROLES:
            self.layer_meta[r].update({"quant_scale": False, "quant_zero": False, "compute_dtype": compute_dtype})
            for kind in _KINDS:
                t = stacks[r, kind]
                t = t.to(compute_dtype) if torch.is_floating_point(t) and kind != "W_q" else t
                setattr(self, f"{r}_{kind}", t.to(device).contiguous())
        H, I = (int(v) for v in self.layer_meta["down"]["shape"])
        self.num_experts, self.hidden_dim, self.intermediate_dim = int(self.down_W_q.shape[0]), H, I
        self.ready = True
        return self

    def extra_repr(self) -> str:
        if not self.ready:
            return ""
        m = self.layer_meta["gate"]
        return f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, intermediate_dim={self.intermediate_dim}, nbits={m['nbits']}, group_size={m['group_size']}"

    # ---- per-expert views ---------------------------------------------------------------------------------------------------------------------------
    def _meta(self, e: int, role: str) -> dict:
        m = dict(self.layer_meta[role])
        m["scale"], m["zero"] = getattr(self, role + "_scale")[e], getattr(self, role + "_zero")[e]
        return m

    def expert_linear(self, e: int, role: str) -> HQQLinear:
        """expert e's gate / up / down as an HQQLinear that SHARES this module's storage (views of the stacks; nothing re-quantised): for tests, export and
        dequantize().  An in-place edit through it edits the expert."""
        if role not in ROLES or not 0 <= e < self.num_experts:
            raise ValueError(f"hqq_amd: expert_linear takes an expert 0 .. {self.num_experts - 1} and one of {ROLES}")
        cfg = copy.deepcopy(self.quant_config)
        cfg["offload_meta"] = False
        layer = HQQLinear(None, cfg, compute_dtype=self.compute_dtype, device=self.device, initialize=False)
        layer.W_q = nn.Parameter(getattr(self, role + "_W_q")[e], requires_grad=False)
        layer.meta = self._meta(e, role)
        layer.bias = None
        layer.out_features, layer.in_features = (int(v) for v in layer.meta["shape"])
        layer.axis, layer.channel_wise = layer.meta["axis"], True
        layer.in_gpu = layer.W_q.is_cuda
        layer._hip_opts = 0   # (the three-op rebuild is a per-layer premise nobody checked here: the four-op form serves)
        layer._w3s = None
        layer.ready = True
        return layer

    def dequantize(self, e: int, role: str) -> Tensor:
        W_q, m = getattr(self, role + "_W_q")[e], self._meta(e, role)
        return Quantizer.dequantize(W_q, m) if W_q.is_cuda else _dequantize_host(W_q, m)

    def _linear(self, x: Tensor, e: int, role: str) -> Tensor:
        """F.linear(x, expert e's weight) on the quantised layer"""
        W_q = getattr(self, role + "_W_q")[e]
        if not x.is_cuda:
            return nn.functional.linear(x, _dequantize_host(W_q, self._meta(e, role)))
        m = self.layer_meta[role]
        N, K = (int(v) for v in m["shape"])
        if not m["packing"]:
            return nn.functional.linear(x, self.dequantize(e, role))
        if m["view_as_float"]:
            W_q = W_q.view(m["unpack_view_dtype"])
        scale, zero = getattr(self, role + "_scale")[e], getattr(self, role + "_zero")[e]
        if x.dtype != scale.dtype or x.dtype not in (torch.float16, torch.bfloat16) or not m["group_size"]:
            return nn.functional.linear(x, self.dequantize(e, role))
        return ops.forward(x, W_q, scale, zero, None, N, K, m["group_size"], Quantizer._packing_bits[m["packing"]], opts=0, axis=m["axis"])

    # ---- forward ------------------------------------------------------------------------------------------------------------------------------------
    def fused_covers(self, hidden_states: Tensor, top_k_index: Tensor) -> bool:
        """the call is one ops.moe_forward serves: ops.moe_covers for the shapes, and a layout the kernel reads (byte containers, no view_as_float)"""
        g = self.layer_meta["gate"]
        if not (hidden_states.is_cuda and hidden_states.dim() == 2 and top_k_index.dim() == 2 and self.gate_W_q.is_cuda):
            return False
        if any(self.layer_meta[r]["view_as_float"] or self.layer_meta[r]["packing"] not in ("4bit_u8", "2bit_u8") or self.layer_meta[r]["packing"] != g["packing"]
               or self.layer_meta[r]["group_size"] != g["group_size"] or self.layer_meta[r]["axis"] != 1 for r in ROLES):
            return False
        if hidden_states.dtype != self.gate_scale.dtype:
            return False
        return ops.moe_covers(hidden_states.dtype, int(hidden_states.shape[0]), int(top_k_index.shape[1]), self.num_experts, self.hidden_dim,
                              self.intermediate_dim, g["group_size"], Quantizer._packing_bits[g["packing"]], 1)

    def forward(self, hidden_states: Tensor, top_k_index: Tensor, top_k_weights: Tensor) -> Tensor:
        want = HQQExperts.fused
        if want is not False:
            ok = self.fused_covers(hidden_states, top_k_index)
            if want is True and not ok:
                raise NotImplementedError("hqq_amd: HQQExperts.fused = True, and this call is outside what the routed expert kernel covers (ops.moe_covers)")
            if ok and (want is True or hidden_states.shape[0] <= ops.MOE_ROUTE_MAX_T):
                return self.forward_fused(hidden_states, top_k_index, top_k_weights)
        return self.forward_composed(hidden_states, top_k_index, top_k_weights)

    def forward_fused(self, hidden_states: Tensor, top_k_index: Tensor, top_k_weights: Tensor, a: Union[Tensor, None] = None) -> Tensor:
        g = self.layer_meta["gate"]
        # routers that hand the weights over in the compute dtype (Qwen3-MoE): fp16 / bf16 -> fp32 is exact, and the product of two 11- / 8-bit
        # significands is exact in fp32, so rnd(fp32(d) * fp32(w)) is HF's rnd(d * w)
        w = top_k_weights if top_k_weights.dtype == torch.float32 else top_k_weights.float()
        return ops.moe_forward(hidden_states.contiguous(), top_k_index.contiguous(), w.contiguous(),
                               (self.gate_W_q, self.gate_scale, self.gate_zero), (self.up_W_q, self.up_scale, self.up_zero),
                               (self.down_W_q, self.down_scale, self.down_zero), self.num_experts, self.hidden_dim, self.intermediate_dim,
                               g["group_size"], Quantizer._packing_bits[g["packing"]], a=a)

    def forward_composed(self, hidden_states: Tensor, top_k_index: Tensor, top_k_weights: Tensor) -> Tensor:
        """MixtralExperts.forward statement for statement; the two F.linear calls (gate and up are one there, chunked after) on the quantised layers"""
        final_hidden_states = torch.zeros_like(hidden_states)
        with torch.no_grad():
            expert_mask = torch.nn.functional.one_hot(top_k_index, num_classes=self.num_experts)
            expert_mask = expert_mask.permute(2, 1, 0)
            expert_hit = torch.greater(expert_mask.sum(dim=(-1, -2)), 0).nonzero()

        for expert_idx in expert_hit:
            expert_idx = expert_idx[0]
            if expert_idx == self.num_experts:
                continue
            e = int(expert_idx)
            top_k_pos, token_idx = torch.where(expert_mask[expert_idx])
            current_state = hidden_states[token_idx]
            gate, up = self._linear(current_state, e, "gate"), self._linear(current_state, e, "up")
            current_hidden_states = self.act_fn(gate) * up
            current_hidden_states = self._linear(current_hidden_states, e, "down")
            current_hidden_states = current_hidden_states * top_k_weights[token_idx, top_k_pos, None]
            final_hidden_states.index_add_(0, token_idx, current_hidden_states.to(final_hidden_states.dtype))

        return final_hidden_states

    # HF calls .to() / .half() / ... on whole models; packed weights and their constants must not be touched (HQQLinear does the same)
    def to(self, *args, **kwargs):
        return self

    def half(self, *args, **kwargs):
        return self

    def bfloat16(self, *args, **kwargs):
        return self

    def float(self, *args, **kwargs):
        return self

    def double(self, *args, **kwargs):
        return self

    # ---- state: the nine stacks are plain buffers; the configuration travels as extra state ---------------------------------------------------------
    def get_extra_state(self):
        if not self.ready:
            return {}
        enc = lambda v: (str(v).replace("torch.", "") if isinstance(v, torch.dtype) else (list(v) if isinstance(v, torch.Size) else v))
        return {"quant_config": copy.deepcopy(self.quant_config), "compute_dtype": enc(self.compute_dtype),
                "layer_meta": {r: {k: enc(v) for k, v in self.layer_meta[r].items()} for r in ROLES}}

    def set_extra_state(self, state):
        if not state:
            return
        self.quant_config = copy.deepcopy(state["quant_config"])
        self.compute_dtype = _DTYPES[state["compute_dtype"]]
        self.layer_meta = {}
        for r in ROLES:
            m = dict(state["layer_meta"][r])
            m["shape"] = torch.Size(m["shape"])
            for k in ("compute_dtype", "unpack_view_dtype"):
                if isinstance(m.get(k), str):
                    m[k] = getattr(torch, m[k])
            self.layer_meta[r] = m
        H, I = (int(v) for v in self.layer_meta["down"]["shape"])
        self.hidden_dim, self.intermediate_dim = H, I

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # an empty shell has no buffer to copy into: adopt the tensors (on this module's device), then the extra state
        for role in ROLES:
            for kind in _KINDS:
                key = f"{prefix}{role}_{kind}"
                if key in state_dict:
                    setattr(self, f"{role}_{kind}", state_dict.pop(key).to(self.device).contiguous())
                elif strict:
                    missing_keys.append(key)
        extra = prefix + "_extra_state"
        if extra in state_dict:
            self.set_extra_state(state_dict.pop(extra))
        elif strict:
            missing_keys.append(extra)
        if self.down_W_q is not None and self.layer_meta is not None:
            self.num_experts = int(self.down_W_q.shape[0])
            self.ready = True
