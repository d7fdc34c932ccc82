"""GraphedGreedyDecoder(prefill_attention="hip") on a GPU (utils/prefill_attn.py; ops.attn_prefill / ops.attn_prefill_kvq under the model's own forward): the
prefill's logits and caches against the default prefill, the tokens of generate(), generate_batch() and the speculative generate() against the default decoder's
while the logit gap is kept, the quantised cache (and that nothing is dequantised), the config's restoration, the fall-back and HFGenerator's keyword.

The toys: the tiny Llama of test_batch_decode_gpu (4 query heads on 4 KV heads, hd 64), the GQA Llama (4 on 2, hd 64) and the Qwen3 (q / k-norm, 4 on 2, hd 128) of
test_kvq_step_gpu.  The yardstick of every token comparison is the model's own forward by hand on the cache in question — never the code under test.
The checks are functions; two tests walk them over the toys, so that the suite grows by two entries."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

import test_kvq_step_gpu as kvq  # noqa: E402
from test_batch_decode_gpu import _quantised, _tiny_llama  # noqa: E402

L = 128
TOL = 5e-3      # the bound tests/test_tile_gpu.py holds the tile step to against the model's forward
GAP = 0.05      # ten times that: where the two best logits are further apart, two routes within the bound pick the same token
TOYS = ("llama", "llama_gqa", "qwen3")
OPT_IN = {"llama": {}, "llama_gqa": {}, "qwen3": dict(qk_norm="fused")}


@pytest.fixture(scope="module")
def models():
    """name -> the quantised, patched toy (built once each, left unchanged)"""
    build = {"llama": lambda: _quantised(_tiny_llama()), "llama_gqa": kvq._toy_llama, "qwen3": kvq._toy_qwen3}
    built = {}

    def get(name):
        if name not in built:
            built[name] = build[name]()
        return built[name]
    return get


def _cache(model, kv=None):
    if kv is None:
        return transformers.StaticCache(config=model.config, max_cache_len=L)
    from hqq_amd.utils.kv_cache import QuantizedStaticCache
    return QuantizedStaticCache(model.config, L, int(kv[1]))


def _decoder(model, hip, **kw):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    return GraphedGreedyDecoder(model, max_cache_len=L, **({"prefill_attention": "hip"} if hip else {}), **kw)


def _default_prefill(model, ids, kv=None):
    cache = _cache(model, kv)
    with torch.no_grad():
        out = model(ids, past_key_values=cache, cache_position=torch.arange(ids.shape[1], device="cuda"), use_cache=True)
    return cache, out.logits[0, -1].float()


def _hip_prefill(model, ids, kv=None, **kw):
    dec = _decoder(model, True, **({} if kv is None else {"kv_cache": kv}), **kw)
    assert dec.prefill_hip and dec.prefill_attention == "hip"
    cache = _cache(model, kv)
    with torch.no_grad():
        out = dec._prefill(ids, cache)
    return cache, out.logits[0, -1].float()


def _greedy(model, ids, n, kv=None):
    """n greedy tokens through the model's own forward on its static cache, by hand (the default route): (tokens [1, T + n], the top-1 / top-2 logit gap of
    every one of the n decisions, the prefill's first)"""
    T = ids.shape[1]
    cache, logits = _default_prefill(model, ids, kv)
    toks, gaps = [], []
    for i in range(n):
        top = logits.topk(2).values
        gaps.append(float(top[0] - top[1]))
        toks.append(logits.argmax().view(1, 1))
        if i + 1 < n:
            with torch.no_grad():
                logits = model(toks[-1], past_key_values=cache, cache_position=torch.tensor([T + i], device="cuda"), use_cache=True).logits[0, -1].float()
    return torch.cat([ids] + toks, dim=1), gaps


def _guarded(gaps):
    """how many decisions keep the guard band before the first one that does not: from there on two routes may part legitimately"""
    k = 0
    while k < len(gaps) and gaps[k] > GAP:
        k += 1
    return k


# ---- the prefill itself ---------------------------------------------------------------------------------------------------------------------------------------
def _logits_and_caches_follow_the_default_prefill(models, name):
    """the last row's logits within the bound; layer 0's cached keys and values bit-identical (their inputs are the same: nothing upstream of layer 0's cache
    write attends), the deeper layers' within the bound; nothing written beyond the prompt.  Prompts of 1 row, inside a tile, across one and across two tile edges"""
    model = models(name)
    for T, seed in ((1, 1), (11, 2), (17, 3), (40, 4)):
        ids = kvq._ids(T, seed)
        c0, want = _default_prefill(model, ids)
        c1, got = _hip_prefill(model, ids)
        print(f"{name} T {T}: largest logit difference {float((got - want).abs().max()):.5f}")
        torch.testing.assert_close(got, want, rtol=TOL, atol=TOL)
        assert torch.equal(c1.layers[0].keys, c0.layers[0].keys) and torch.equal(c1.layers[0].values, c0.layers[0].values), (name, T)
        for a, b in zip(c1.layers[1:], c0.layers[1:]):
            torch.testing.assert_close(a.keys.float(), b.keys.float(), rtol=TOL, atol=TOL)
            torch.testing.assert_close(a.values.float(), b.values.float(), rtol=TOL, atol=TOL)
            assert not bool(a.keys[:, :, T:].any()) and not bool(a.values[:, :, T:].any())
            assert int(a.cumulative_length) == int(b.cumulative_length) == T


def _generate_emits_the_default_tokens_while_the_gap_is_kept(models, name):
    """per prompt the gap is measured on the model's own forward by hand; the decisions it guards are emitted by the default decoder and by the "hip" one, through
    the fused step with the kernel attention and through the model's own forward"""
    model = models(name)
    for kw in (dict(attention="hip", **OPT_IN[name]), dict(fused=False)):
        plain, hip = _decoder(model, False, **kw), _decoder(model, True, **kw)
        assert hip.prefill_hip and not plain.prefill_hip and plain.prefill_attention == "model"
        runs = []
        for seed in range(40, 50):
            ids = kvq._ids(5 + 3 * (seed % 7), seed)
            want, gaps = _greedy(model, ids, 10)
            k = _guarded(gaps)
            runs.append(k)
            if k == 0:
                continue
            T = ids.shape[1]
            assert torch.equal(plain.generate(ids, k), want[:, :T + k]), (name, seed, k)
            assert torch.equal(hip.generate(ids, k), want[:, :T + k]), (name, seed, k)
        print(f"{name} {sorted(kw)}: guarded decisions per prompt {runs}")
        assert sum(k >= 1 for k in runs) >= 3 and sum(runs) >= 6, runs
        assert model.config._attn_implementation == "sdpa"


# ---- the quantised cache --------------------------------------------------------------------------------------------------------------------------------------
def _the_quantised_cache_is_attended_packed(models, name, monkeypatch):
    """kv_cache="q8": the logits within the bound; layer 0's six buffers bit-identical; a deeper layer's rows, dequantised, within the bound plus ONE quantisation
    step of the row (an input that moves by less than a step moves its level by at most one).  ops.kv_dequantize is not called during a "hip" prefill — the
    default prefill calls it once per layer"""
    from hqq_amd import ops
    model = models(name)
    hd = model.config.head_dim if name == "qwen3" else 64
    calls = []
    real = ops.kv_dequantize
    monkeypatch.setattr(ops, "kv_dequantize", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for T, seed in ((11, 5), (40, 6)):
        ids = kvq._ids(T, seed)
        calls.clear()
        c0, want = _default_prefill(model, ids, "q8")
        assert len(calls) == len(c0.layers)
        calls.clear()
        c1, got = _hip_prefill(model, ids, "q8")
        assert not calls, f"{len(calls)} full-length dequantisations during a 'hip' prefill"
        assert all(lay.packed_prefill is False for lay in c1.layers)
        print(f"{name} q8 T {T}: largest logit difference {float((got - want).abs().max()):.5f}")
        torch.testing.assert_close(got, want, rtol=TOL, atol=TOL)
        assert all(torch.equal(x, y) for x, y in zip(c1.layers[0].bufs, c0.layers[0].bufs)), (name, T)
        for a, b in zip(c1.layers[1:], c0.layers[1:]):
            for x, y, s in zip(real(a.bufs, hd, T), real(b.bufs, hd, T), (b.bufs[1], b.bufs[4])):
                step = float(s[:, :, :T].float().abs().max())
                assert bool(((x.float() - y.float()).abs() <= TOL * (1 + y.float().abs()) + step).all()), (name, T)
            assert int(a.cumulative_length) == T
    assert model.config._attn_implementation == "sdpa"


def _generate_on_the_quantised_cache_emits_the_default_tokens(models):
    model = models("llama")
    for kv in ("q8", "q4"):
        plain, hip = _decoder(model, False, attention="hip", kv_cache=kv), _decoder(model, True, attention="hip", kv_cache=kv)
        assert hip.prefill_hip
        runs = []
        for seed in range(40, 50):
            ids = kvq._ids(5 + 3 * (seed % 7), seed)
            want, gaps = _greedy(model, ids, 8, kv)
            k = _guarded(gaps)
            runs.append(k)
            if k:
                assert torch.equal(plain.generate(ids, k), want[:, :ids.shape[1] + k]) and torch.equal(hip.generate(ids, k), want[:, :ids.shape[1] + k]), (kv, seed, k)
        print(f"{kv}: guarded decisions per prompt {runs}")
        assert sum(k >= 1 for k in runs) >= 3, runs


# ---- the config ----------------------------------------------------------------------------------------------------------------------------------------------
def _the_config_is_restored_after_the_call_and_after_an_exception(models, monkeypatch):
    from hqq_amd import ops
    from hqq_amd.utils import prefill_attn
    model = models("llama")
    was = model.config._attn_implementation
    assert was != prefill_attn.NAME
    ids = kvq._ids(9, 7)
    for kv in (None, "q8"):
        dec = _decoder(model, True, **({} if kv is None else {"kv_cache": kv}))
        seen = []
        real = ops.attn_prefill_kvq if kv else ops.attn_prefill
        monkeypatch.setattr(ops, "attn_prefill_kvq" if kv else "attn_prefill", lambda *a, **k: (seen.append(model.config._attn_implementation), real(*a, **k))[1])
        cache = _cache(model, kv)
        with torch.no_grad():
            dec._prefill(ids, cache)
        assert seen == [prefill_attn.NAME] * len(cache.layers)                  # every layer attended through the op, under the switched config
        assert model.config._attn_implementation == was and prefill_attn._active is None

        def boom(*a, **k):
            raise RuntimeError("inside the forward")
        monkeypatch.setattr(ops, "attn_prefill_kvq" if kv else "attn_prefill", boom)
        cache = _cache(model, kv)
        with pytest.raises(RuntimeError, match="inside the forward"), torch.no_grad():
            dec._prefill(ids, cache)
        assert model.config._attn_implementation == was and prefill_attn._active is None
        assert all(getattr(lay, "packed_prefill", False) is False for lay in cache.layers)
        monkeypatch.undo()
    with pytest.raises(RuntimeError, match="inside prefill_attn.hip_prefill"):  # the registered function serves nothing outside the context
        prefill_attn.hip_prefill_attention(None, None, None, None, None)


# ---- the fall-back --------------------------------------------------------------------------------------------------------------------------------------------
def _a_model_the_rule_refuses_prefills_as_before(monkeypatch):
    """heads of 32 values: prefill_hip is False, no message, the op is never called and the tokens are the default decoder's (the same code path: bit for bit)"""
    from hqq_amd import ops
    from hqq_amd.utils import llama_fused as lf
    model = _tiny_llama(hidden_size=128)
    assert lf.head_dim(model.config) == 32 and not lf.supports_prefill_attention(model)
    calls = []
    monkeypatch.setattr(ops, "attn_prefill", lambda *a, **k: calls.append(1))
    plain, hip = _decoder(model, False), _decoder(model, True)
    assert hip.prefill_attention == "hip" and hip.prefill_hip is False and plain.prefill_hip is False
    ids = kvq._ids(9, 11)
    assert torch.equal(hip.generate(ids, 6), plain.generate(ids, 6)) and not calls
    # a cache the quantised kernels do not cover refuses as well: q4 rows in groups of 64 need heads of 128 values
    big = _decoder(_tiny_llama(), True, kv_cache="q4", kv_group_size=64)
    assert big.prefill_hip is False


# ---- the other routes -----------------------------------------------------------------------------------------------------------------------------------------
def _guarded_prompts(model, n, want, seeds=range(40, 64)):
    """the first `want` prompts whose first n decisions all keep the gap on the model's own forward: [(ids, tokens [1, T + n])]"""
    out = []
    for seed in seeds:
        ids = kvq._ids(5 + 3 * (seed % 7), seed)
        toks, gaps = _greedy(model, ids, n)
        if _guarded(gaps) == n:
            out.append((ids, toks))
        if len(out) == want:
            break
    assert len(out) == want, f"only {len(out)} of {len(list(seeds))} prompts keep the gap over {n} decisions"
    return out


def _generate_batch_emits_the_default_tokens(models):
    model = models("llama")
    picked = _guarded_prompts(model, 3, 3)
    assert len({ids.shape[1] for ids, _ in picked}) >= 2                        # prompts of different lengths
    for kv in (None, "q8"):
        kw = dict(attention="hip", **({} if kv is None else {"kv_cache": kv}))
        if kv is not None:   # (the gap is a statement about the cache it was measured on)
            picked_kv = [p for p in picked if _guarded(_greedy(model, p[0], 3, kv)[1]) == 3]
            if len(picked_kv) < 2:
                continue
        else:
            picked_kv = picked
        plain, hip = _decoder(model, False, **kw), _decoder(model, True, **kw)
        a = plain.generate_batch([ids for ids, _ in picked_kv], 3)
        b = hip.generate_batch([ids for ids, _ in picked_kv], 3)
        assert hip.prefill_hip and hip._batch and len(b) == len(picked_kv)
        for x, y, (_, toks) in zip(a, b, picked_kv):
            assert torch.equal(x, y), kv
            if kv is None:
                assert torch.equal(y, toks)


def _the_speculative_generate_emits_the_default_tokens(models):
    model = models("llama")
    kw = dict(attention="hip", speculate="ngram", draft_rows=4)
    plain, hip = _decoder(model, False, **kw), _decoder(model, True, **kw)
    assert plain.speculating and hip.speculating and hip.prefill_hip
    for ids, toks in _guarded_prompts(model, 4, 3):
        assert torch.equal(plain.generate(ids, 4), toks) and torch.equal(hip.generate(ids, 4), toks)
        assert hip._spec is not None and hip.spec_stats["tokens"] == 3


def _hfgenerator_passes_the_keyword_on(models):
    from hqq_amd.utils.generation import HFGenerator
    from test_model_gpu import _ToyTokenizer
    model = models("llama")
    gen = HFGenerator(model, _ToyTokenizer(), max_new_tokens=8, cache_size=64, compile="partial", prefill_attention="hip")
    assert gen.decoder.prefill_attention == "hip" and gen.decoder.prefill_hip
    want = HFGenerator(model, _ToyTokenizer(), max_new_tokens=8, cache_size=64, compile="partial")
    assert want.decoder.prefill_attention == "model" and not want.decoder.prefill_hip
    r = gen.generate("7 8 9 10 11 7 8 9", use_chat_template=False, verbose=False)
    assert r["output_tokens"].numel() == 8 and model.config._attn_implementation == "sdpa"
    with pytest.raises(ValueError, match="prefill_attention"):
        HFGenerator(model, _ToyTokenizer(), max_new_tokens=8, prefill_attention="kernel")


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_hip_prefill_follows_the_default_prefill(models):
    """the prefill call itself: logits and caches on the three toys, the quantised cache attended packed, the config's restoration, the fall-back"""
    for name in TOYS:
        _logits_and_caches_follow_the_default_prefill(models, name)
    for name in ("llama", "qwen3"):
        with pytest.MonkeyPatch.context() as mp:
            _the_quantised_cache_is_attended_packed(models, name, mp)
    with pytest.MonkeyPatch.context() as mp:
        _the_config_is_restored_after_the_call_and_after_an_exception(models, mp)
    with pytest.MonkeyPatch.context() as mp:
        _a_model_the_rule_refuses_prefills_as_before(mp)


def test_every_route_emits_the_default_tokens_while_the_gap_is_kept(models):
    """generate() on the three toys and on the quantised caches, generate_batch(), the speculative generate(), and HFGenerator's keyword"""
    for name in TOYS:
        _generate_emits_the_default_tokens_while_the_gap_is_kept(models, name)
    _generate_on_the_quantised_cache_emits_the_default_tokens(models)
    _generate_batch_emits_the_default_tokens(models)
    _the_speculative_generate_emits_the_default_tokens(models)
    _hfgenerator_passes_the_keyword_on(models)
