"""CPU side of the grouped axis-0 decode launch (hqq_hip_gemv_axis0_grouped) and of the opt-in fused step for axis-0 models: argument checks
before any launch, the workspace size as host arithmetic, the Python coverage predicate tied to the workspace query, the `axis0` keyword of the
generation front ends, and supports_axis0 on models the step does not serve."""
import ctypes
import itertools

import pytest
import torch

P16 = 16    # a 16-byte aligned stand-in pointer: every call below must be refused before anything touches it
HEAD = 256 << 10   # the decode workspace's counter head (csrc/hqq_common.h)
SILU = 4    # HQQ_BLOCK_SILU


def _L():
    from hqq_amd import _C
    return _C.lib()


def _err():
    return _L().hqq_hip_last_error()


def _call(nbits=4, Ns=(256, 256), M=1, K=1024, gs=64, dtype=1, opts=0, flags=0, ws_bytes=1 << 30, x=P16, ws=P16, n=None):
    n = len(Ns) if n is None else n
    VP = ctypes.c_void_p * max(len(Ns), 1)
    ptrs = VP(*([P16] * len(Ns)))
    Nc = (ctypes.c_int64 * max(len(Ns), 1))(*Ns)
    return _L().hqq_hip_gemv_axis0_grouped(nbits, n, x, ptrs, ptrs, ptrs, None, ptrs, Nc, M, K, gs, dtype, opts, flags, ws, ws_bytes, None)


def _bytes(nbits, Ns, M, K, gs, dtype, flags=0):
    return _L().hqq_hip_gemv_axis0_grouped_workspace_bytes(nbits, len(Ns), (ctypes.c_int64 * len(Ns))(*Ns), M, K, gs, dtype, flags)


def test_bad_arguments_are_refused_before_any_launch():
    assert _call(Ns=(256,), n=0) == -2 and b"n_layers" in _err()                       # an empty group
    assert _call(Ns=(256, 256, 256, 256)) == -2 and b"n_layers" in _err()              # more than three layers
    assert _call(M=17) == -4 and b"not covered" in _err()                              # more rows than the decode kernel takes
    assert _call(M=0) == -2
    assert _call(nbits=3) == -4 and b"not covered" in _err()                           # 3-bit containers
    assert _call(nbits=5) == -1
    assert _call(dtype=0) == -4 and b"not covered" in _err()                           # fp32
    assert _call(dtype=7) == -3
    assert _call(nbits=8, dtype=2) == -4 and b"not covered" in _err()                  # bf16 covers 4 / 2 bits
    assert _call(Ns=(256, 288, 256)) == -4 and b"not covered" in _err()                # one member's N is not a multiple of group_size
    assert _call(Ns=(256, 256), gs=40) == -4 and b"not covered" in _err()              # group_size % 16 != 0
    assert _call(K=1000) == -4 and b"not covered" in _err()                            # K % 64 != 0
    assert _call(opts=1 << 15) == -2 and b"option" in _err()                           # unknown option bits
    assert _call(Ns=(256, 256, 256), flags=SILU) == -4 and b"HQQ_BLOCK_SILU" in _err()  # SiLU * up takes gate and up only
    assert _call(Ns=(512, 256), flags=SILU) == -4 and b"HQQ_BLOCK_SILU" in _err()      # ... of equal N
    assert _call(Ns=(256,), flags=SILU) == -4 and b"HQQ_BLOCK_SILU" in _err()
    for flags in (1, 2, 8, 1 | SILU, 16, 1 << 31):                                     # NORM / RESID / ROPE and unknown bits are not served here
        assert _call(flags=flags) == -4 and b"flags" in _err(), flags
    assert _call(x=24) == -6                                                           # misaligned activation
    need = _bytes(4, (256, 256), 1, 1024, 64, 1)
    assert need > HEAD
    assert _call(ws_bytes=need - 1) == -5 and b"workspace" in _err()                   # one byte short
    assert _call(ws_bytes=0) == -5 and _call(ws=None) == -5                            # the workspace is never optional
    assert _call(Ns=(256, 1 << 23), K=1024) == -2 and b"size overflow" in _err()


def test_workspace_is_the_head_plus_the_members_areas():
    L = _L()
    for nbits, dt, M, K, gs, Ns in [(4, 1, 1, 4096, 64, (4096, 4096, 4096)), (4, 1, 16, 4096, 64, (11008, 11008)), (2, 2, 5, 8192, 128, (8192, 1024, 1024)),
                                    (8, 1, 3, 1024, 16, (256,)), (1, 1, 2, 1024, 256, (256, 256)), (4, 2, 7, 256, 64, (256, 512, 64))]:
        want = HEAD + sum(L.hqq_hip_gemv_axis0_workspace_bytes(nbits, M, N, K, gs, dt) - HEAD for N in Ns)
        assert _bytes(nbits, Ns, M, K, gs, dt) == want, (nbits, dt, M, K, gs, Ns)
    # SiLU * up changes the reduce, not the partial sums
    assert _bytes(4, (11008, 11008), 1, 4096, 64, 1, SILU) == _bytes(4, (11008, 11008), 1, 4096, 64, 1)
    # a group of one is the single-layer call's workspace
    assert _bytes(4, (4096,), 1, 4096, 64, 1) == L.hqq_hip_gemv_axis0_workspace_bytes(4, 1, 4096, 4096, 64, 1)
    # refused calls need nothing
    assert _bytes(4, (4096, 4000), 1, 4096, 64, 1) == 0 and _bytes(4, (4096, 4096, 4096), 1, 4096, 64, 1, SILU) == 0
    assert _bytes(4, (4096,), 1, 4096, 64, 1, 1) == 0


def test_axis0_grouped_covers_truth_table():
    from hqq_amd import ops
    f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32
    yes = [(f16, 1, (4096, 4096, 4096), 4096, 64, 4, 0), (f16, 16, (11008, 11008), 4096, 64, 4, SILU), (bf16, 5, (8192, 1024, 1024), 8192, 128, 2, 0),
           (f16, 1, (256,), 1024, 16, 8, 0), (f16, 2, (256, 256), 1024, None, 1, SILU), (bf16, 1, (512, 128, 128), 1024, 64, 4, 0)]
    no = [(f16, 1, (), 4096, 64, 4, 0), (f16, 1, (256,) * 4, 1024, 64, 4, 0), (f16, 17, (256, 256), 1024, 64, 4, 0), (f16, 1, (256, 256), 1024, 64, 3, 0),
          (f32, 1, (256, 256), 1024, 64, 4, 0), (bf16, 1, (256, 256), 1024, 64, 8, 0), (f16, 1, (256, 288), 1024, 64, 4, 0),
          (f16, 1, (256, 256, 256), 1024, 64, 4, SILU), (f16, 1, (512, 256), 1024, 64, 4, SILU), (f16, 1, (256, 256), 1024, 64, 4, 1),
          (f16, 1, (256, 256), 1024, 64, 4, 8 | SILU), (f16, 1, (512, 256), 1024, None, 4, 0), (f16, 1, (256, 256), 1000, 64, 4, 0)]
    for args in yes:
        assert ops.axis0_grouped_covers(*args), args
    for args in no:
        assert not ops.axis0_grouped_covers(*args), args


def test_axis0_grouped_covers_agrees_with_the_workspace_query():
    """the library's workspace query is 0 exactly where the call is refused: the Python predicate says the same for every input of the grid"""
    from hqq_amd import ops
    code = {torch.float16: 1, torch.bfloat16: 2, torch.float32: 0}
    groups = [(256,), (256, 256), (512, 128, 128), (256, 288), (4096, 4096, 4096), (11008, 11008), (8192, 1024, 1024), (100, 100), (256,) * 4, (512, 256)]
    checked = 0
    for dt, M, Ns, K, gs, nbits, flags in itertools.product(code, (0, 1, 5, 16, 17), groups, (1024, 4096, 1000), (16, 64, 128, 48, None), (8, 4, 3, 2, 1),
                                                             (0, SILU, 1, 2 | SILU)):
        if gs is None and len(set(Ns)) != 1:
            assert not ops.axis0_grouped_covers(dt, M, Ns, K, gs, nbits, flags)   # one group per column cannot be shared by layers of different N
            continue
        if len(Ns) > 3:   # (the query is not handed more sizes than it reads: n_layers is checked first)
            assert not ops.axis0_grouped_covers(dt, M, Ns, K, gs, nbits, flags) and _bytes(nbits, Ns, M, K, gs or Ns[0], code[dt], flags) == 0
            continue
        got = _bytes(nbits, Ns, M, K, Ns[0] if gs is None else gs, code[dt], flags) > 0
        assert got == ops.axis0_grouped_covers(dt, M, Ns, K, gs, nbits, flags), (dt, M, Ns, K, gs, nbits, flags)
        checked += 1
    assert checked > 10000


def test_wrapper_refuses_bad_groups_on_the_host():
    from hqq_amd import ops
    x = torch.zeros(1, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="1..3 layers"):
        ops.gemv_axis0_grouped(x, [], 64, 64, 4)
    with pytest.raises(ValueError, match="1..3 layers"):
        ops.gemv_axis0_grouped(x, [(None, None, None, None, 64)] * 4, 64, 64, 4)


def _tiny_cfg(**kw):
    from transformers import LlamaConfig
    base = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, vocab_size=64,
                max_position_embeddings=64)
    base.update(kw)
    return LlamaConfig(**base)


def test_generation_front_ends_reject_an_unknown_axis0_value():
    from transformers import LlamaForCausalLM
    from hqq_amd.utils.generation import GraphedGreedyDecoder, HFGenerator
    model = LlamaForCausalLM(_tiny_cfg())
    for bad in ("auto", "Fused", "", None, True):
        with pytest.raises(ValueError, match="axis0"):
            GraphedGreedyDecoder(model, max_cache_len=32, axis0=bad)
        with pytest.raises(ValueError, match="axis0"):
            HFGenerator(model, tokenizer=None, max_new_tokens=8, axis0=bad)


def test_supports_axis0_is_false_for_models_the_step_does_not_serve():
    from transformers import LlamaForCausalLM
    from hqq_amd.utils import llama_fused
    plain = LlamaForCausalLM(_tiny_cfg())   # unquantised: nn.Linear everywhere
    assert llama_fused.arch_supported(plain)
    assert not llama_fused.supports_axis0(plain) and not llama_fused.supports_axis0_batch(plain, 4)
    assert not llama_fused.supports_axis0(plain.half())
    # every architecture arch_supported refuses is refused here too, before any layer is looked at
    refused = [LlamaForCausalLM(_tiny_cfg(attention_bias=True)), LlamaForCausalLM(_tiny_cfg(mlp_bias=True))]
    odd = LlamaForCausalLM(_tiny_cfg())
    odd.config.model_type = "qwen3"
    refused.append(odd)
    for name in ("residual_multiplier", "embedding_multiplier", "logits_scaling", "attention_multiplier"):
        m = LlamaForCausalLM(_tiny_cfg())
        setattr(m.config, name, 0.5)
        refused.append(m)
    m = LlamaForCausalLM(_tiny_cfg())
    m.config.sliding_window = 16
    refused.append(m)
    m = LlamaForCausalLM(_tiny_cfg())
    m.model.layers[0].self_attn.q_norm = torch.nn.Identity()
    refused.append(m)
    m = LlamaForCausalLM(_tiny_cfg(hidden_act="gelu"))
    refused.append(m)
    for m in refused:
        assert not llama_fused.arch_supported(m)
        assert not llama_fused.supports_axis0(m) and not llama_fused.supports_axis0_batch(m, 2)
    assert not llama_fused.supports_axis0(object())
    # the batch bound is the decode kernel's row limit, whatever the model
    assert not llama_fused.supports_axis0_batch(plain, 0) and not llama_fused.supports_axis0_batch(plain, 17)
