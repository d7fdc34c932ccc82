"""CPU side of the opt-in fused decode step for Qwen3 models (per-head q_norm / k_norm in front of the rotary embedding): the architecture predicate of
its own, the `qk_norm` keyword of the generation front ends, and hqq_hip_qknorm_rope_cache_batched's argument checks, made before any launch."""
import pytest
import torch

P16 = 16    # a stand-in pointer: every call below must be refused before anything touches it


def _tiny_qwen3(**kw):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    torch.manual_seed(0)
    args = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128, vocab_size=512,
                max_position_embeddings=128)
    args.update(kw)
    return Qwen3ForCausalLM(Qwen3Config(**args))


def test_qk_norm_arch_supported_takes_qwen3_and_only_qwen3():
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.utils import llama_fused
    model = _tiny_qwen3()
    assert llama_fused.qk_norm_arch_supported(model)
    assert llama_fused.qk_norm_arch_supported(_tiny_qwen3().half()) and llama_fused.qk_norm_arch_supported(_tiny_qwen3().bfloat16())
    # the Llama predicate and everything built on it keep refusing it: the step is opt-in
    assert not llama_fused.arch_supported(model) and not llama_fused.supports(model) and not llama_fused.supports_batch(model, 2)
    # its linears are nn.Linear: the architecture is served, this model is not
    assert not llama_fused.supports_qk_norm(model) and not llama_fused.supports_qk_norm_batch(model, 2)
    assert not llama_fused.supports_qk_norm(model.half())
    llama = LlamaForCausalLM(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, vocab_size=64,
                                         max_position_embeddings=64))
    assert llama_fused.arch_supported(llama) and not llama_fused.qk_norm_arch_supported(llama)
    assert not llama_fused.qk_norm_arch_supported(_tiny_qwen3(attention_bias=True))
    assert not llama_fused.qk_norm_arch_supported(_tiny_qwen3(layer_types=["full_attention", "sliding_attention"], use_sliding_window=True, sliding_window=16,
                                                              max_window_layers=1))
    m = _tiny_qwen3()
    m.config.layer_types = ["full_attention", "sliding_attention"]
    assert not llama_fused.qk_norm_arch_supported(m)
    m = _tiny_qwen3()
    m.config.sliding_window = 16
    assert not llama_fused.qk_norm_arch_supported(m)
    m = _tiny_qwen3()
    del m.model.layers[1].self_attn.k_norm
    assert not llama_fused.qk_norm_arch_supported(m)
    m = _tiny_qwen3()
    m.config.model_type = "qwen3_moe"
    assert not llama_fused.qk_norm_arch_supported(m)
    m = _tiny_qwen3()
    m.model.layers[0].self_attn.q_norm.weight.data = torch.ones(64)   # a norm over something other than head_dim
    assert not llama_fused.qk_norm_arch_supported(m)
    m = _tiny_qwen3()
    m.model.layers[0].self_attn.q_norm.half()   # not the compute dtype
    assert not llama_fused.qk_norm_arch_supported(m)
    m = _tiny_qwen3()
    m.model.layers[0].self_attn.sinks = torch.zeros(4)
    assert not llama_fused.qk_norm_arch_supported(m)
    assert not llama_fused.qk_norm_arch_supported(_tiny_qwen3(hidden_act="gelu"))
    assert not llama_fused.qk_norm_arch_supported(object()) and not llama_fused.supports_qk_norm(object())


def test_generation_front_ends_reject_an_unknown_qk_norm_value():
    from hqq_amd.utils.generation import GraphedGreedyDecoder, HFGenerator
    model = _tiny_qwen3()
    for bad in ("bad", "auto", "Fused", "", None, True):
        with pytest.raises(ValueError, match="qk_norm"):
            GraphedGreedyDecoder(model, max_cache_len=32, qk_norm=bad)
        with pytest.raises(ValueError, match="qk_norm"):
            HFGenerator(model, tokenizer=None, max_new_tokens=8, qk_norm=bad)


def _call(q=P16, k=P16, v=P16, qw=P16, kw=P16, q_eps=1e-6, k_eps=1e-6, cos=P16, sin=P16, pos=P16, batch=1, q_out=P16, kc=P16, vc=P16, n_heads=4, n_kv=2, hd=128,
          L=16, dtype=1):
    from hqq_amd import _C
    return _C.lib().hqq_hip_qknorm_rope_cache_batched(q, k, v, qw, kw, q_eps, k_eps, cos, sin, pos, batch, q_out, kc, vc, n_heads, n_kv, hd, L, dtype, None)


def test_bad_arguments_are_refused_before_any_launch():
    from hqq_amd import _C
    err = _C.lib().hqq_hip_last_error
    for name in ("q", "k", "v", "qw", "kw", "cos", "sin", "pos", "q_out", "kc", "vc"):   # a null pointer, whichever it is
        assert _call(**{name: None}) == -2 and b"qknorm_rope_cache" in err(), name
    assert _call(hd=127) == -2 and _call(hd=1) == -2 and _call(hd=0) == -2              # an odd head_dim has no rotary pairs
    assert _call(hd=96) == -4 and b"head_dim 96 not covered" in err()                    # even, but no kernel for it
    assert _call(hd=512) == -4
    assert _call(batch=0) == -2 and b"batch" in err()
    assert _call(batch=65536) == -2
    assert _call(dtype=0) == -4 and b"fp16 / bf16 only" in err()                         # fp32
    assert _call(dtype=7) == -4
    assert _call(n_heads=0) == -2 and _call(n_kv=0) == -2 and _call(L=0) == -2
    assert _call(q_eps=-1.0) == -2 and _call(k_eps=float("nan")) == -2
    assert _call(n_heads=1 << 24, hd=128) == -2 and _call(L=1 << 31) == -2               # extents beyond 32 bits
