"""A quantised static KV cache for HF models (opt-in: GraphedGreedyDecoder(kv_cache="q8" / "q4"), HFGenerator likewise).

The format is this library's own (include/hqq_hip.h, csrc/kv_cache.hip): every (sequence, kv head, position) row of head_dim values — keys after the rotary
embedding, and values — is quantised by itself as Quantizer.quantize(row.view(head_dim // gs, gs), nbits, group_size=gs, axis=1, optimize=False) when it is
written, and never touched again.  transformers' QuantizedCache(backend="hqq") has the same role upstream with another schedule: it keeps a full-precision
residual window, re-quantises the whole cache every residual_length steps and dequantises it into a fresh tensor on every step.

QuantizedStaticCache is the COMPOSED route: a transformers Cache of static layers (StaticLayer's protocol: a device counter of written positions, static shapes,
no host synchronisation, so the model's own forward stays graph-capturable with it) whose update() writes the incoming rows with ops.kv_quantize and returns the
full-length dequantised tensors of ops.kv_dequantize.  One rule throughout: every attended key and value is the stored, dequantised one, the prompt's included.
It holds only the six quantised buffers per layer; the dense tensors are per-layer transients.  It serves any model the dense StaticCache serves.
Under GraphedGreedyDecoder(prefill_attention="hip") a prefill sets the layers' packed_prefill flag for its duration: update() then quantises as always and
dequantises nothing, and the attention reads the six buffers itself (ops.attn_prefill_kvq) — the rule above holds, without the full-length tensors.
The FUSED route (llama_fused.FusedLlamaStep on such a cache) reads the same buffers with ops.rope_kvq_cache_batched and ops.attn_decode_kvq_batched.
"""
from __future__ import annotations

import torch
from transformers.cache_utils import Cache, StaticLayer

from .. import ops

KV_CACHE_BITS = {"q8": 8, "q4": 4}


def kv_cache_bits(kv_cache) -> int | None:
    """the decoders' `kv_cache` keyword as a bit width: None (the dense StaticCache), "q8" -> 8, "q4" -> 4; anything else is a ValueError"""
    if kv_cache is None:
        return None
    if not isinstance(kv_cache, str) or kv_cache not in KV_CACHE_BITS:
        raise ValueError("kv_cache: None, 'q8' or 'q4'")
    return KV_CACHE_BITS[kv_cache]


def check_kv_group_size(kv_cache, kv_group_size) -> None:
    """the decoders' `kv_group_size` keyword: None (ops.kv_group_size's default), or 32 / 64 together with a quantised cache; anything else is a ValueError"""
    if kv_group_size is None:
        return
    if kv_cache is None:
        raise ValueError("kv_group_size goes with kv_cache='q8' or 'q4'")
    if isinstance(kv_group_size, bool) or kv_group_size not in (32, 64):
        raise ValueError("kv_group_size: None, 32 or 64")


class QuantizedStaticLayer(StaticLayer):
    """StaticLayer with the six quantised buffers (`bufs`: kq, k_scale, k_zero, vq, v_scale, v_zero) in the place of keys / values, which stay None"""

    def __init__(self, max_cache_len: int, nbits: int, group_size: int | None = None, **kwargs):
        super().__init__(max_cache_len=max_cache_len)
        self.nbits, self.group_size = int(nbits), group_size
        self.bufs = None
        self.packed_prefill = False   # set for the duration of a prefill_attention="hip" prefill (utils/prefill_attn.py): update() then dequantises nothing

    def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        self.dtype, self.device = key_states.dtype, key_states.device
        self.batch_size, self.num_heads = key_states.shape[:2]
        self.k_head_dim = self.v_head_dim = hd = int(key_states.shape[-1])
        if value_states.shape[-1] != hd:
            raise ValueError("hqq_amd: the quantised KV cache needs keys and values of one head_dim")
        if self.group_size is None:
            self.group_size = ops.kv_group_size(hd)
        self.bufs = ops.kv_alloc(self.batch_size, self.num_heads, self.max_cache_len, hd, self.nbits, self.group_size, self.dtype, self.device)
        self.cumulative_length = self.cumulative_length.to(self.device)
        if not torch.compiler.is_compiling():
            for t in self.bufs + (self.cumulative_length,):
                torch._dynamo.mark_static_address(t)
        self.is_initialized = True

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
        """the incoming rows quantised into positions cumulative_length .. + T - 1 (read on the device), then the whole cache dequantised: what the layer attends.
        Under packed_prefill the rows are quantised the same way and handed back as they came: the prefill's attention function (prefill_attn.hip_prefill_attention)
        does not look at them — it reads this layer's `bufs` through ops.attn_prefill_kvq, so what is attended is still the stored, dequantised row"""
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        ops.kv_quantize(key_states, value_states, self.bufs, start=self.cumulative_length.view(1))
        self.cumulative_length.add_(key_states.shape[-2])
        if self.packed_prefill:
            return key_states, value_states
        return ops.kv_dequantize(self.bufs, self.k_head_dim)

    def reset(self) -> None:
        if self.is_initialized:
            for t in self.bufs:
                t.zero_()
        self.cumulative_length.zero_()

    def offload(self):
        raise NotImplementedError("hqq_amd: the quantised KV cache is not offloaded")

    prefetch = offload

    def reorder_cache(self, beam_idx: torch.LongTensor) -> None:
        if self.is_initialized:
            for t in self.bufs:
                t.copy_(t.index_select(0, beam_idx.to(t.device)))

    def copy_row(self, b: int, src: "QuantizedStaticLayer", n: int) -> None:
        """the first n positions of src's sequence 0 into this layer's sequence b (generate_batch: a prefilled prompt into its row of the B-row cache)"""
        for d, s in zip(self.bufs, src.bufs):
            d[b, :, :n].copy_(s[0, :, :n])

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.bufs) if self.is_initialized else 0


class QuantizedStaticCache(Cache):
    """QuantizedStaticCache(config, max_cache_len, nbits, group_size=None): a StaticCache whose layers hold 8- or 4-bit rows (module docstring).  group_size None:
    ops.kv_group_size(head_dim).  Models with sliding-window or linear-attention layers are refused (the dense StaticCache serves them)."""

    def __init__(self, config, max_cache_len: int, nbits: int, group_size: int | None = None, **kwargs):
        from transformers.cache_utils import get_layer_types_and_kwargs
        if nbits not in (8, 4):
            raise ValueError("hqq_amd: QuantizedStaticCache takes nbits 8 or 4")
        if group_size is not None and group_size not in (32, 64):
            raise ValueError("hqq_amd: QuantizedStaticCache takes group_size None, 32 or 64")
        if max_cache_len < 1 or max_cache_len > ops.KV_MAX_LEN:
            raise ValueError(f"hqq_amd: QuantizedStaticCache holds 1 .. {ops.KV_MAX_LEN} positions")
        layer_types, _ = get_layer_types_and_kwargs(config.get_text_config(decoder=True))
        if any(t != "full_attention" for t in layer_types):
            raise ValueError("hqq_amd: QuantizedStaticCache serves full-attention layers only")
        self.nbits, self.group_size = int(nbits), group_size
        super().__init__(layers=[QuantizedStaticLayer(max_cache_len, nbits, group_size) for _ in layer_types])

    @property
    def nbytes(self) -> int:
        """the device bytes of every layer's six buffers"""
        return sum(lay.nbytes for lay in self.layers)
