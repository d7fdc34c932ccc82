"""The prefill's attention through ops.attn_prefill (opt-in: GraphedGreedyDecoder(prefill_attention="hip"), HFGenerator likewise).

The model's own prefill hands HF's attention function the whole static cache — max_cache_len positions under a [T, max_cache_len] mask, and on a
kv_cache.QuantizedStaticCache a full-length dequantised copy of it per layer.  hip_prefill(model, cache, pos0) is a context manager that, for the duration of ONE
forward of the model, makes every attention module call hip_prefill_attention instead: the function is registered with transformers' AttentionInterface under the
name NAME (the SDPA mask function under the same name, so that the model builds the mask it would have built), and config._attn_implementation is switched to NAME
and restored in `finally` — the decode steps with attention="sdpa" read the config.

The hook sits where HF calls its attention function: q | k | v, the biases, q / k-norm, the rotary embedding and the cache write have happened, so the one kernel
serves every family (Llama, Mistral, Qwen2, Qwen3, Mixtral, Qwen3-MoE), axis 0 and adapters.  llama_fused.supports_prefill_attention is the coverage rule.
"""
from __future__ import annotations

from contextlib import contextmanager

from .. import ops

NAME = "hqq_hip_prefill"

_active = None   # (cache, pos0) inside hip_prefill, None outside


def hip_prefill_attention(module, query, key, value, attention_mask, scaling=None, **kwargs):
    """HF's attention-function signature: query [1, H, T, hd] (any strides with hd dense), key / value what the cache layer's update() returned.  The mask is
    ignored: row t stands at position pos0 + t and attends over keys [0, pos0 + t] of the layer's cache, which update() has just written.  A dense StaticCache
    hands its tensors [1, n_kv, L, hd] over as key / value; a QuantizedStaticLayer under packed_prefill hands the new rows back, and its six buffers are read
    through module.layer_idx.  Returns (out [1, T, H, hd], None)."""
    if _active is None:
        raise RuntimeError(f"hqq_amd: the attention function '{NAME}' serves a prefill inside prefill_attn.hip_prefill only")
    cache, pos0 = _active
    if query.dim() != 4 or query.shape[0] != 1:
        raise ValueError("hqq_amd: prefill_attention='hip' serves one sequence per forward")
    _, H, T, hd = query.shape
    q = query[0].transpose(0, 1)   # [T, H, hd] through the strides, no copy
    scaling = module.scaling if scaling is None else scaling
    layer = cache.layers[module.layer_idx]
    if getattr(layer, "packed_prefill", False):
        out = ops.attn_prefill_kvq(q, layer.bufs, pos0, hd, scaling=scaling)
    else:
        out = ops.attn_prefill(q, key, value, pos0, scaling=scaling)
    return out.view(1, T, H, hd), None


def _register() -> None:
    from transformers import AttentionInterface, AttentionMaskInterface
    from transformers.masking_utils import sdpa_mask
    if NAME not in AttentionInterface._global_mapping:
        AttentionInterface.register(NAME, hip_prefill_attention)
        AttentionMaskInterface.register(NAME, sdpa_mask)


@contextmanager
def hip_prefill(model, cache, pos0: int = 0):
    """one prefill forward of `model` into `cache` attends through ops.attn_prefill / ops.attn_prefill_kvq, its rows at positions pos0 ..: the config's attention
    implementation and the quantised layers' packed_prefill flag are set here and put back whatever the forward does"""
    global _active
    _register()
    cfg = model.config
    was, was_active = cfg._attn_implementation, _active
    packed = [lay for lay in cache.layers if hasattr(lay, "packed_prefill")]
    try:
        cfg._attn_implementation = NAME
        for lay in packed:
            lay.packed_prefill = True
        _active = (cache, int(pos0))
        yield
    finally:
        _active = was_active
        for lay in packed:
            lay.packed_prefill = False
        cfg._attn_implementation = was
