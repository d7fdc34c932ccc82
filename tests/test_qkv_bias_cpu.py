"""CPU side of the opt-in fused decode step for Qwen2 / Qwen2.5 models (biases on q_proj / k_proj / v_proj): the architecture predicate of its own, the
`qkv_bias` keyword of the generation front ends, and hqq_hip_bias_rope_cache_batched's argument checks, made before any launch."""
import pytest
import torch

P16 = 16    # a stand-in pointer: every call below must be refused before anything touches it


def _tiny_qwen2(**kw):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(0)
    args = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
                max_position_embeddings=128)
    args.update(kw)
    return Qwen2ForCausalLM(Qwen2Config(**args))


def test_qkv_bias_arch_supported_takes_qwen2_and_only_qwen2():
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen3Config, Qwen3ForCausalLM
    from hqq_amd.utils import llama_fused
    model = _tiny_qwen2()
    assert all(t == "full_attention" for t in model.config.layer_types) and model.config.sliding_window is None   # what the config is expected to give
    assert llama_fused.qkv_bias_arch_supported(model)
    assert llama_fused.qkv_bias_arch_supported(_tiny_qwen2().half()) and llama_fused.qkv_bias_arch_supported(_tiny_qwen2().bfloat16())
    # the Llama and Qwen3 predicates and everything built on them keep refusing it: the step is opt-in
    assert not llama_fused.arch_supported(model) and not llama_fused.qk_norm_arch_supported(model)
    assert not llama_fused.supports(model) and not llama_fused.supports_batch(model, 2) and not llama_fused.supports_qk_norm(model)
    # its linears are nn.Linear: the architecture is served, this model is not
    assert not llama_fused.supports_qkv_bias(model) and not llama_fused.supports_qkv_bias_batch(model, 2)
    assert not llama_fused.supports_qkv_bias(model.half())
    # a sliding-window layer
    assert not llama_fused.qkv_bias_arch_supported(_tiny_qwen2(use_sliding_window=True, sliding_window=16, max_window_layers=1,
                                                               layer_types=["full_attention", "sliding_attention"]))
    m = _tiny_qwen2()
    m.config.layer_types = ["full_attention", "sliding_attention"]
    assert not llama_fused.qkv_bias_arch_supported(m)
    m = _tiny_qwen2()
    m.model.layers[1].self_attn.sliding_window = 16
    assert not llama_fused.qkv_bias_arch_supported(m)
    # other architectures
    llama = LlamaForCausalLM(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, vocab_size=64,
                                         max_position_embeddings=64))
    assert llama_fused.arch_supported(llama) and not llama_fused.qkv_bias_arch_supported(llama)
    qwen3 = Qwen3ForCausalLM(Qwen3Config(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, head_dim=64,
                                         vocab_size=64, max_position_embeddings=64))
    assert llama_fused.qk_norm_arch_supported(qwen3) and not llama_fused.qkv_bias_arch_supported(qwen3)
    m = _tiny_qwen2()
    m.config.model_type = "qwen2_moe"
    assert not llama_fused.qkv_bias_arch_supported(m)
    # biases anywhere but on q, k and v — or missing there
    m = _tiny_qwen2()
    m.model.layers[1].self_attn.k_proj.bias = None
    assert not llama_fused.qkv_bias_arch_supported(m)
    for name in ("q_proj", "v_proj"):
        m = _tiny_qwen2()
        setattr(getattr(m.model.layers[0].self_attn, name), "bias", None)
        assert not llama_fused.qkv_bias_arch_supported(m), name
    m = _tiny_qwen2()
    m.model.layers[0].self_attn.o_proj.bias = torch.nn.Parameter(torch.zeros(256))
    assert not llama_fused.qkv_bias_arch_supported(m)
    m = _tiny_qwen2()
    m.model.layers[1].mlp.down_proj.bias = torch.nn.Parameter(torch.zeros(256))
    assert not llama_fused.qkv_bias_arch_supported(m)
    # head norms, sinks, another activation
    m = _tiny_qwen2()
    m.model.layers[0].self_attn.q_norm = torch.nn.Identity()
    assert not llama_fused.qkv_bias_arch_supported(m)
    m = _tiny_qwen2()
    m.model.layers[0].self_attn.sinks = torch.zeros(4)
    assert not llama_fused.qkv_bias_arch_supported(m)
    assert not llama_fused.qkv_bias_arch_supported(_tiny_qwen2(hidden_act="gelu"))
    assert not llama_fused.qkv_bias_arch_supported(object()) and not llama_fused.supports_qkv_bias(object())


def test_generation_front_ends_reject_an_unknown_qkv_bias_value():
    from hqq_amd.utils.generation import GraphedGreedyDecoder, HFGenerator
    model = _tiny_qwen2()
    for bad in ("x", "auto", "Fused", "", None, True):
        with pytest.raises(ValueError, match="qkv_bias"):
            GraphedGreedyDecoder(model, max_cache_len=32, qkv_bias=bad)
        with pytest.raises(ValueError, match="qkv_bias"):
            HFGenerator(model, tokenizer=None, max_new_tokens=8, qkv_bias=bad)


def _call(q=P16, k=P16, v=P16, qb=P16, kb=P16, vb=P16, cos=P16, sin=P16, pos=P16, batch=1, q_out=P16, kc=P16, vc=P16, n_heads=4, n_kv=2, hd=128, L=16, dtype=1):
    from hqq_amd import _C
    return _C.lib().hqq_hip_bias_rope_cache_batched(q, k, v, qb, kb, vb, cos, sin, pos, batch, q_out, kc, vc, n_heads, n_kv, hd, L, dtype, None)


def test_bad_arguments_are_refused_before_any_launch():
    from hqq_amd import _C
    err = _C.lib().hqq_hip_last_error
    for name in ("qb", "kb", "vb", "q", "k", "v", "cos", "sin", "pos", "q_out", "kc", "vc"):   # a null pointer, whichever it is: all three biases are required
        assert _call(**{name: None}) == -2 and b"bias_rope_cache" in err(), name
    assert _call(hd=127) == -2 and b"bias_rope_cache" in err()                           # an odd head_dim has no rotary pairs
    assert _call(hd=1) == -2 and _call(hd=0) == -2
    assert _call(batch=0) == -2 and b"batch" in err()
    assert _call(batch=65536) == -2 and b"batch" in err()
    assert _call(dtype=0) == -4 and b"fp16 / bf16 only" in err()                         # fp32
    assert _call(dtype=7) == -4
    assert _call(n_heads=0) == -2 and _call(n_kv=0) == -2 and _call(L=0) == -2
    assert _call(n_heads=1 << 24, hd=128) == -2 and _call(L=1 << 31) == -2               # extents beyond 32 bits
    assert _call(n_heads=1 << 32) == -2 and _call(hd=1 << 32) == -2
