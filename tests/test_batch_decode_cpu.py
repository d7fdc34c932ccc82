"""CPU tests of batched decoding: the *_batched entry points of csrc/block.hip reject bad arguments before anything is launched, the rule of which
batches the fused linears serve (llama_fused.batch_covers) is a pure function of the shapes, and the host-side bookkeeping of
GraphedGreedyDecoder.generate_batch (length check, cache bucket, per-row EOS) runs without a device."""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

F32, F16, BF16 = 0, 1, 2
SHAPE, UNSUPPORTED, ALIGN = -2, -4, -6


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        _C.build()
    return _C.lib()


P = ctypes.c_void_p(16)      # aligned, never dereferenced: every call below fails its argument checks first
MIS = ctypes.c_void_p(24)    # not 16-byte aligned


def _attn(L, rope, batch=2, hd=128, cache_len=256, q=P, k_cache=P, dtype=F16):
    if rope:
        return L.hqq_hip_rope_attn_decode_batched(q, P, P, P, P, P, batch, k_cache, P, P, 8, 2, hd, cache_len, 0.1, dtype, 1, None, 0, None)
    return L.hqq_hip_attn_decode_batched(q, k_cache, P, P, batch, P, 8, 2, hd, cache_len, 0.1, dtype, 1, None, 0, None)


@pytest.mark.parametrize("rope", [False, True])
def test_batched_attention_rejects_bad_arguments_before_launching(L, rope):
    assert _attn(L, rope, batch=0) == SHAPE and b"batch" in L.hqq_hip_last_error()
    assert _attn(L, rope, batch=-3) == SHAPE
    assert _attn(L, rope, batch=70000) == SHAPE
    assert _attn(L, rope, hd=96) == UNSUPPORTED and b"head_dim" in L.hqq_hip_last_error()
    assert _attn(L, rope, q=MIS) == ALIGN
    assert _attn(L, rope, k_cache=MIS) == ALIGN
    assert _attn(L, rope, cache_len=30001) == SHAPE
    assert _attn(L, rope, dtype=F32) == UNSUPPORTED
    # splits > 1 needs the records of batch * n_heads heads
    need = L.hqq_hip_attn_decode_workspace_bytes(2 * 8, 128, 4)
    assert need == 2 * 8 * 4 * 130 * 4
    assert L.hqq_hip_attn_decode_batched(P, P, P, P, 2, P, 8, 2, 128, 256, 0.1, F16, 4, P, need - 4, None) == SHAPE
    assert b"workspace" in L.hqq_hip_last_error()


def test_batched_glue_rejects_bad_arguments_before_launching(L):
    # rope_cache_batched: batch, dtype, shapes
    rc = L.hqq_hip_rope_cache_batched(P, P, P, P, P, P, 0, P, P, P, 8, 2, 128, 256, F16, None)
    assert rc == SHAPE and b"batch" in L.hqq_hip_last_error()
    assert L.hqq_hip_rope_cache_batched(P, P, P, P, P, P, 2, P, P, P, 8, 2, 127, 256, F16, None) == SHAPE
    assert L.hqq_hip_rope_cache_batched(P, P, P, P, P, P, 2, P, P, P, 8, 2, 128, 256, F32, None) == UNSUPPORTED
    # token_prologue_batched
    assert L.hqq_hip_token_prologue_batched(P, P, 0, P, 100, 4096, None, None, 1, 0, P, None, None, None, F16, None) == SHAPE
    assert L.hqq_hip_token_prologue_batched(P, P, 2, MIS, 100, 4096, None, None, 1, 0, P, None, None, None, F16, None) == ALIGN
    assert L.hqq_hip_token_prologue_batched(P, P, 2, P, 100, 4096, None, None, 1, 0, MIS, None, None, None, F16, None) == ALIGN
    assert L.hqq_hip_token_prologue_batched(P, P, 2, P, 100, 4100, None, None, 1, 0, P, None, None, None, F16, None) == SHAPE
    assert L.hqq_hip_token_prologue_batched(P, P, 2, P, 100, 4096, None, None, 1, 0, P, None, None, None, F32, None) == UNSUPPORTED
    # argmax_advance_batched
    assert L.hqq_hip_argmax_advance_batched(P, 0, 100, F16, P, None, None, None) == SHAPE
    assert L.hqq_hip_argmax_advance_batched(P, 2, 0, F16, P, None, None, None) == SHAPE
    assert L.hqq_hip_argmax_advance_batched(None, 2, 100, F16, P, None, None, None) == SHAPE
    assert L.hqq_hip_argmax_advance_batched(P, 2, 100, F32, P, None, None, None) == UNSUPPORTED


def test_batched_entry_points_are_declared_and_bound(L):
    from hqq_amd import _C
    for name in ("hqq_hip_token_prologue_batched", "hqq_hip_rope_cache_batched", "hqq_hip_attn_decode_batched", "hqq_hip_rope_attn_decode_batched",
                 "hqq_hip_argmax_advance_batched"):
        assert name in _C.SYMBOLS and hasattr(L, name)


def _tiny_shapes(nbits=4, gs=64, w3s=False):
    # the tiny Llama of the GPU tests (hidden 256, intermediate 512): q k v o gate up down as (N, K, group_size, nbits, w3s)
    return [(256, 256, gs, nbits, w3s)] * 4 + [(512, 256, gs, nbits, w3s)] * 2 + [(256, 512, gs, nbits, w3s)]


def _llama7b_shapes(nbits=4, w3s=False):
    return [(4096, 4096, 64, nbits, w3s)] * 4 + [(11008, 4096, 64, nbits, w3s)] * 2 + [(4096, 11008, 64, nbits, w3s)]


def test_batch_coverage_rule():
    from hqq_amd import ops
    from hqq_amd.utils.llama_fused import batch_covers
    f16, bf16 = torch.float16, torch.bfloat16
    # fp16 4-bit gs 64 on the tiny shapes: the decode kernels up to 16 rows; K = 256 is not a skinny shape, so 17 is out
    assert all(batch_covers(f16, B, _tiny_shapes()) for B in range(1, 17))
    assert not batch_covers(f16, 17, _tiny_shapes())
    assert not batch_covers(f16, 0, _tiny_shapes())
    # FACTORED mode: the row-per-wave kernel's 8 rows outside the skinny kernel
    assert batch_covers(f16, 8, _tiny_shapes(), ops.OPT_FACTORED) and not batch_covers(f16, 9, _tiny_shapes(), ops.OPT_FACTORED)
    # the Llama-2-7B shapes are skinny shapes: up to 64 rows, in bf16 and in the 3-bit stream layout too
    for B in (1, 4, 8, 16, 32, 64):
        assert batch_covers(f16, B, _llama7b_shapes())
        assert batch_covers(bf16, B, _llama7b_shapes())
        assert batch_covers(f16, B, _llama7b_shapes(nbits=3, w3s=True))
    assert not batch_covers(f16, 65, _llama7b_shapes())
    assert batch_covers(f16, 32, _llama7b_shapes(nbits=2)) and batch_covers(f16, 32, _llama7b_shapes(nbits=8))
    # bf16 outside the skinny kernel: 4 / 2-bit up to 4 rows
    assert batch_covers(bf16, 4, _tiny_shapes()) and not batch_covers(bf16, 5, _tiny_shapes())
    assert batch_covers(bf16, 2, _tiny_shapes(nbits=2)) and not batch_covers(bf16, 1, _tiny_shapes(nbits=8))
    # 3-bit: the reference container up to 4 rows; the stream layout up to 4 rows outside the skinny kernel
    assert batch_covers(f16, 4, _tiny_shapes(nbits=3)) and not batch_covers(f16, 5, _tiny_shapes(nbits=3))
    assert batch_covers(f16, 4, _tiny_shapes(nbits=3, w3s=True)) and not batch_covers(f16, 5, _tiny_shapes(nbits=3, w3s=True))
    # one uncovered layer is enough to refuse
    assert not batch_covers(f16, 2, _tiny_shapes() + [(256, 256, 64, 5, False)])


def test_supports_batch_needs_the_weights_on_a_device():
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.utils.llama_fused import supports_batch
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, vocab_size=64)
    assert not supports_batch(LlamaForCausalLM(cfg).half(), 2)


def test_generate_batch_host_logic():
    from hqq_amd.utils.generation import batch_kv_bucket, check_batch_lengths, eos_lengths, kv_bucket
    # the length check: T_b + n <= max_cache_len for every row
    check_batch_lengths([3, 9, 5, 12], 52, 64)
    with pytest.raises(ValueError, match="prompt 3"):
        check_batch_lengths([3, 9, 5, 13], 52, 64)
    with pytest.raises(ValueError):
        check_batch_lengths([3, 0], 4, 64)
    with pytest.raises(ValueError):
        check_batch_lengths([3], 0, 64)
    # the cache bucket of a batched step is that of its largest row position
    assert batch_kv_bucket([3, 11, 70], "sdpa", 4096) == kv_bucket(70, "sdpa", 4096) == 128
    assert batch_kv_bucket([3, 11, 63], "sdpa", 4096) == 64
    assert batch_kv_bucket([5, 1500], "sdpa", 4096) == 1536
    assert batch_kv_bucket([5, 1500], "hip", 4096) == 2048 and batch_kv_bucket([5, 10], "hip", 4096) == 1024
    assert batch_kv_bucket([5, 1500], "sdpa", 1024) == 1024
    # per-row EOS: up to and including each row's first EOS, the whole run otherwise
    rows = [[4, 5, 6, 7], [4, 9, 6, 9], [9, 1, 1, 1]]
    assert eos_lengths(rows, 9, 4) == [4, 2, 1]
    assert eos_lengths(rows, None, 4) == [4, 4, 4]
    assert eos_lengths(rows, 9, 3) == [3, 2, 1]
