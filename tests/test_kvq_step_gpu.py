"""The quantised KV cache in the decoders (hqq_amd.utils.kv_cache, llama_fused.FusedLlamaStep(kv_cache=...), GraphedGreedyDecoder(kv_cache=...)) on 2-block toy
models as tests/test_model_gpu.py builds them, max_cache_len 64: the default path is untouched; the composed route (the model's own forward on a
QuantizedStaticCache) is self-consistent and stores what kv_quantize gives; the fused route attends the same dequantised values as the composed one (logits
within the tolerance tests/test_model_gpu.py applies between the kernel attention and SDPA); graphs, batches, capacity and the fallback."""
import gc

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

L = 64


def _quantised(model, dt):
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=dt, device="cuda")
    prepare_for_inference(model, backend="hip")
    group_llama_projections(model)
    return model


def _toy_llama(dt=torch.float16, **kw):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    args = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=512, max_position_embeddings=128)
    args.update(kw)
    return _quantised(LlamaForCausalLM(LlamaConfig(**args)).to(dt).cuda().eval(), dt)


def _toy_qwen3():
    from transformers import Qwen3Config, Qwen3ForCausalLM
    torch.manual_seed(0)
    cfg = Qwen3Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128, vocab_size=512,
                      max_position_embeddings=128)
    return _quantised(Qwen3ForCausalLM(cfg).half().cuda().eval(), torch.float16)


def _ids(T, seed):
    return torch.randint(0, 512, (1, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _prefill(model, cache, ids):
    with torch.no_grad():
        return model(ids, past_key_values=cache, cache_position=torch.arange(ids.shape[1], device="cuda"), use_cache=True).logits[:, -1]


def _qcache(model, kv, gs=None):
    from hqq_amd.utils.kv_cache import QuantizedStaticCache
    return QuantizedStaticCache(model.config, L, {"q8": 8, "q4": 4}[kv], gs)


def _greedy_on(model, cache, ids, n):
    """`model(...)` driven step by step on `cache`, no graphs: prompt + n greedy tokens"""
    tok = _prefill(model, cache, ids).argmax(-1, keepdim=True)
    toks = [tok]
    for t in range(n - 1):
        with torch.no_grad():
            out = model(tok, past_key_values=cache, cache_position=torch.tensor([ids.shape[1] + t], device="cuda"), use_cache=True)
        tok = out.logits[:, -1].argmax(-1, keepdim=True)
        toks.append(tok)
    return torch.cat([ids] + toks, dim=1)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a, b.view(torch.uint8) if b.dtype != torch.uint8 else b)


def test_the_default_is_the_dense_path_untouched():
    from transformers import StaticCache
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = _toy_llama()
    ids = _ids(6, 3)
    for attention in ("sdpa", "hip"):
        plain = GraphedGreedyDecoder(model, max_cache_len=L, attention=attention)
        none = GraphedGreedyDecoder(model, max_cache_len=L, attention=attention, kv_cache=None)
        assert torch.equal(plain.generate(ids, 24), none.generate(ids, 24))
        assert type(none.cache) is StaticCache and none.step is not None and none.step.kv_bits is None and "kc" in none.step.blocks[0]
        assert none.kv_cache_bytes == 2 * 2 * (1 * 2 * L * 64) * 2   # layers x (keys, values) x [1, n_kv, L, hd] x 2 bytes


@pytest.mark.parametrize("kv", ["q8", "q4"])
def test_the_composed_route_is_the_models_own_forward_on_the_quantised_cache(kv):
    from transformers import StaticCache
    from hqq_amd import ops
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.kv_cache import QuantizedStaticCache
    model = _toy_llama()
    ids = _ids(9, 5)
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="sdpa", kv_cache=kv)
    got = dec.generate(ids, 20, use_graph=True)
    assert dec.step is None and dec.graph is not None and isinstance(dec.cache, QuantizedStaticCache)   # no SDPA on packed bytes: the model's own forward, captured
    want = _greedy_on(model, _qcache(model, kv), ids, 20)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert torch.equal(dec.generate(ids, 20, use_graph=True), want)   # the kept cache, reset in place, and the kept graphs
    # after a prefill, layer 0 holds kv_quantize of the dense cache's layer-0 rows of the same prompt (only layer 0's keys and values depend on no attention)
    qc, dc = _qcache(model, kv), StaticCache(config=model.config, max_cache_len=L)
    _prefill(model, qc, ids), _prefill(model, dc, ids)
    T = ids.shape[1]
    lay = qc.layers[0]
    assert lay.keys is None and lay.values is None and lay.nbits == int(kv[1]) and lay.group_size == 32
    want_bufs = ops.kv_alloc(1, 2, L, 64, lay.nbits, 32, torch.float16, "cuda")
    ops.kv_quantize(dc.layers[0].keys[:, :, :T], dc.layers[0].values[:, :, :T], want_bufs, start=0)
    assert all(_same(a, b) for a, b in zip(lay.bufs, want_bufs))   # (positions from T on are zero in both)
    assert int(lay.cumulative_length) == T and qc.get_seq_length() == T


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kv", ["q8", "q4"])
def test_the_fused_route_stays_within_the_logit_tolerance_of_the_composed_one(kv, dt):
    """teacher-forced over 16 positions: both sides attend the same dequantised values, so the kernel's attention arithmetic is the only difference — the
    tolerance tests/test_model_gpu.py applies between the kernel attention and SDPA (5e-3 in fp16, 4e-2 in bf16)"""
    from transformers import StaticCache
    from hqq_amd import ops
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    model = _toy_llama(dt)
    ids = _ids(12, 5)
    T = ids.shape[1]
    forced = GraphedGreedyDecoder(model, max_cache_len=L, attention="sdpa").generate(ids, 20)
    # the composed side: the model's own forward on a QuantizedStaticCache of the format
    qc = _qcache(model, kv)
    _prefill(model, qc, ids)
    want = []
    for t in range(16):
        with torch.no_grad():
            want.append(model(forced[:, T + t:T + t + 1], past_key_values=qc, cache_position=torch.tensor([T + t], device="cuda"), use_cache=True).logits[:, -1].float().clone())
    # the fused side, on its own cache
    fc = _qcache(model, kv)
    _prefill(model, fc, ids)
    step = FusedLlamaStep(model, fc, L, attention="hip", kv_cache=kv)
    assert step.kv_bits == int(kv[1]) and "kvq" in step.blocks[0] and "kc" not in step.blocks[0]
    got = [step(forced[:, T + t:T + t + 1], torch.tensor([T + t], device="cuda")).float().clone() for t in range(16)]
    tol = 5e-3 if dt == torch.float16 else 4e-2
    torch.testing.assert_close(torch.cat(got), torch.cat(want), rtol=tol, atol=tol)
    # layer 0's stored rows of the fused run: kv_quantize of the dense step's layer-0 rows under the same forced tokens
    dc = StaticCache(config=model.config, max_cache_len=L)
    _prefill(model, dc, ids)
    dense = FusedLlamaStep(model, dc, L, attention="hip")
    for t in range(16):
        dense(forced[:, T + t:T + t + 1], torch.tensor([T + t], device="cuda"))
    lay = fc.layers[0]
    want_bufs = ops.kv_alloc(1, 2, L, 64, lay.nbits, 32, dt, "cuda")
    ops.kv_quantize(dc.layers[0].keys[:, :, :T + 16], dc.layers[0].values[:, :, :T + 16], want_bufs, start=0)
    assert all(_same(a, b) for a, b in zip(lay.bufs, want_bufs))
    # what the cache object holds after fused steps: the six packed buffers per layer, and no dense full-length key / value tensor
    gc.collect()
    def dense_kv(t):   # (at 8 bits and head_dim 64 a LEVEL buffer has that shape too: uint8, and one of the six)
        return isinstance(t, torch.Tensor) and tuple(t.shape) == (1, 2, L, 64) and t.is_floating_point()
    for lay in fc.layers:
        assert lay.keys is None and lay.values is None
        held = [t for t in vars(lay).values() if isinstance(t, torch.Tensor)] + list(lay.bufs)
        assert len(lay.bufs) == 6 and not any(dense_kv(t) for t in held)
    assert not any(dense_kv(t) for b in step.blocks for t in b.values())


def test_graph_replay_and_eager_steps_give_the_same_tokens_and_cache_bytes():
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = _toy_llama()
    ids = _ids(7, 9)
    for kv, attention in (("q8", "hip"), ("q4", "hip"), ("q8", "sdpa")):
        a = GraphedGreedyDecoder(model, max_cache_len=L, attention=attention, kv_cache=kv)
        b = GraphedGreedyDecoder(model, max_cache_len=L, attention=attention, kv_cache=kv)
        ta, tb = a.generate(ids, 24, use_graph=True), b.generate(ids, 24, use_graph=False)
        assert (a.step is not None) == (attention == "hip") and a.graph is not None and b.graph is None
        assert torch.equal(ta, tb)
        for la, lb in zip(a.cache.layers, b.cache.layers):
            assert all(_same(x, y) for x, y in zip(la.bufs, lb.bufs))


@pytest.mark.parametrize("kv", ["q8", "q4"])
def test_a_batch_of_ragged_prompts_decodes_each_prompts_batch1_tokens(kv):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = _toy_llama()
    g = torch.Generator().manual_seed(21)
    prompts = [torch.randint(0, 512, (1, T), generator=g).cuda() for T in (3, 9, 5)]
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", kv_cache=kv)
    got = dec.generate_batch(prompts, 20)
    st = dec._batch.get(3)
    assert st is not None and dec.batch_graphs and st["step"].kv_bits == int(kv[1]), "the batched fused step served the batch"
    one = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", kv_cache=kv)
    for b, x in enumerate(prompts):
        assert torch.equal(got[b], one.generate(x, 20)), b


def test_capacity():
    """kv_cache_bytes is the sum of the six buffers' sizes: from the shapes, (hd / 2 + 4 hd / gs) / (2 hd) of the dense cache's bytes at 4 bits and
    (hd + 4 hd / gs) / (2 hd) at 8 — 36 / 128 and 68 / 128 at gs 64; at this model's head_dim 64 with gs 32: 40 / 128 and 72 / 128, and 68 / 128 for q8 with gs 64"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = _toy_llama()
    ids = _ids(5, 1)
    dense = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip")
    dense.generate(ids, 4)
    for kv, gs, num in (("q4", None, 40), ("q8", None, 72), ("q8", 64, 68)):
        dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", kv_cache=kv, kv_group_size=gs)
        assert dec.kv_cache_bytes == 0
        dec.generate(ids, 4)
        assert dec.kv_cache_bytes == sum(t.numel() * t.element_size() for lay in dec.cache.layers for t in lay.bufs)
        assert dec.kv_cache_bytes * 128 == dense.kv_cache_bytes * num
    # a 128-wide head at gs 64: the 36 / 128 and 68 / 128 of the shapes
    wide = _toy_llama(hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=1)
    dense = GraphedGreedyDecoder(wide, max_cache_len=L, attention="hip")
    dense.generate(ids, 4)
    for kv, num in (("q4", 36), ("q8", 68)):
        dec = GraphedGreedyDecoder(wide, max_cache_len=L, attention="hip", kv_cache=kv)
        dec.generate(ids, 4)
        assert dec.step is not None and dec.cache.layers[0].group_size == 64 and dec.kv_cache_bytes * 128 == dense.kv_cache_bytes * num
    with pytest.raises(ValueError):   # 4 bits need 2 * group_size <= head_dim
        GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", kv_cache="q4", kv_group_size=64).generate(ids, 4)


def test_a_variant_the_fused_route_refuses_decodes_through_the_composed_one():
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    model = _toy_qwen3()
    ids = _ids(6, 3)
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", qk_norm="fused", kv_cache="q8")
    assert dec.fused_qk_norm
    got = dec.generate(ids, 20)
    assert dec.step is None and dec.graph is not None   # Qwen3's rotary launch is not rope_cache: refused, the model's own forward on the quantised cache
    assert torch.equal(got, _greedy_on(model, _qcache(model, "q8"), ids, 20))
    qc = _qcache(model, "q8")
    _prefill(model, qc, ids)
    with pytest.raises(ValueError, match="quantised KV cache"):
        FusedLlamaStep(model, qc, L, attention="hip", qk_norm=True, kv_cache="q8")
    llama = _toy_llama()
    lc = _qcache(llama, "q8")
    _prefill(llama, lc, ids)
    with pytest.raises(ValueError, match="quantised KV cache"):   # no SDPA runs on packed bytes
        FusedLlamaStep(llama, lc, L, attention="sdpa", kv_cache="q8")
    with pytest.raises(ValueError, match="QuantizedStaticCache"):   # the cache and the keyword must agree
        FusedLlamaStep(llama, lc, L, attention="hip", kv_cache="q4")
    with pytest.raises(ValueError, match="kv_cache"):
        FusedLlamaStep(llama, lc, L, attention="hip")
