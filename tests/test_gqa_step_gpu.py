"""gqa_attention="group" in the fused step and the decoders (llama_fused.FusedLlamaStep, GraphedGreedyDecoder, HFGenerator) on the toy models of
tests/test_kvq_step_gpu.py (Llama 4 / 2 heads, Qwen3 4 / 2 with head_dim 128), a Qwen2 toy and one G = 4 Llama (hidden 512, 8 / 2): the step against the model's
own forward with the bound tests/test_tile_gpu.py applies to the tile step ("heads" is held to it first: the yardstick), greedy tokens against "heads" for as
long as a prompt keeps that file's 0.05 logit gap, graphs, batches, the quantised cache, the launch sequence per block, the refusals and the decoders' plumbing."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

import test_kvq_step_gpu as kvq  # noqa: E402
import test_step_launches_gpu as sl  # noqa: E402

L = kvq.L
GAP = 0.05                      # tests/_spec_cases.GAP: the top-1 / top-2 logit gap a prompt must keep on the yardstick route
TOL = 5e-3                      # tests/test_tile_gpu.py's bound on the tile step's fp16 logits against the model's forward
GQA_OPS = ("attn_decode_gqa_batched", "attn_decode_gqa_kvq_batched")
FLAGS = {"llama": {}, "llama_g4": {}, "qwen3": dict(qk_norm=True), "qwen2": dict(qkv_bias=True)}
OPT_IN = {"llama": {}, "llama_g4": {}, "qwen3": dict(qk_norm="fused"), "qwen2": dict(qkv_bias="fused")}
ROTARY = {"llama": "rope_cache", "llama_g4": "rope_cache", "qwen3": "qknorm_rope_cache", "qwen2": "bias_rope_cache"}


@pytest.fixture(scope="module")
def models():
    """name -> the quantised, patched toy (built once each, left unchanged)"""
    import test_qkv_bias_gpu
    build = {"llama": kvq._toy_llama, "qwen3": kvq._toy_qwen3, "qwen2": lambda: kvq._quantised(test_qkv_bias_gpu._tiny_qwen2(), torch.float16),
             "llama_g4": lambda: kvq._toy_llama(hidden_size=512, num_attention_heads=8, num_key_value_heads=2),
             "mha": lambda: kvq._toy_llama(num_key_value_heads=4)}
    built = {}

    def get(name):
        if name not in built:
            built[name] = build[name]()
        return built[name]
    return get


def _prefilled(model, ids, cache_len=L, kv=None):
    from transformers import StaticCache
    from hqq_amd.utils.kv_cache import QuantizedStaticCache
    cache = StaticCache(config=model.config, max_cache_len=cache_len) if kv is None else QuantizedStaticCache(model.config, cache_len, int(kv[1]), None)
    return cache, kvq._prefill(model, cache, ids)


def _route(model, ids, n, flags, gqa, kv=None):
    """greedy decoding through the one-row fused step with the kernel attention, by hand: (tokens [1, T + n], the top-1 / top-2 logit gap of every decode step)"""
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    T = ids.shape[1]
    cache, logits = _prefilled(model, ids, kv=kv)
    step = FusedLlamaStep(model, cache, L, attention="hip", gqa_attention=gqa, **flags, **({} if kv is None else {"kv_cache": kv}))
    assert step.gqa_attention == gqa
    tok = logits.argmax(-1, keepdim=True)
    toks, gaps = [tok], []
    for t in range(n - 1):
        lg = step(tok, torch.tensor([T + t], device="cuda"), L).float()
        top = lg.view(-1).topk(2).values
        gaps.append(float(top[0] - top[1]))
        tok = lg.argmax(-1, keepdim=True)
        toks.append(tok)
    return torch.cat([ids] + toks, dim=1), gaps


# ---- the step ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_group_step_follows_the_models_forward(models):
    """on every toy, teacher-forced over 16 positions: first the "heads" step meets test_tile_gpu's bound on this toy (the yardstick), then the "group" step does"""
    for name in ("llama", "qwen3", "qwen2", "llama_g4"):
        _follows_the_forward(name, models)


def _follows_the_forward(name, models):
    from hqq_amd.utils.llama_fused import FusedLlamaStep, supports_gqa_attention
    model = models(name)
    assert supports_gqa_attention(model)
    T, R = 9, 16
    seq = torch.randint(0, 512, (1, T + R), generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        want = model(seq).logits[0, T - 1 + 1:T + R].float()
    for gqa in ("heads", "group"):
        cache, _ = _prefilled(model, seq[:, :T])
        step = FusedLlamaStep(model, cache, L, attention="hip", gqa_attention=gqa, **FLAGS[name])
        got = torch.cat([step(seq[:, T + t:T + t + 1], torch.tensor([T + t], device="cuda"), L).float().clone() for t in range(R)])
        err = float((got - want).abs().max())
        print(f"{name} {gqa}: largest logit error {err:.5f}")
        torch.testing.assert_close(got, want, rtol=TOL, atol=TOL)


def _guarded(gaps):
    """how many decode steps of a hand-driven "heads" run keep the 0.05 guard band before the first one that does not: the tokens they decide (and the prefill's
    first token) are what another attention arithmetic must reproduce; from the first sub-gap step on the two routes may part legitimately"""
    k = 0
    while k < len(gaps) and gaps[k] > GAP:
        k += 1
    return k


def _compare_guarded(model, flags, opt_in, kv, seeds, what):
    """per prompt: the gap is measured on the "heads" route (the yardstick, not the code under test); the tokens its guarded steps decide are emitted by the
    "group" step driven by hand and by the decoder's captured loop.  The toys' logits are near-flat, so the guarded run of a prompt is short: twelve prompts, and
    the test demands at least eight guarded steps in all and two prompts with at least two"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", gqa_attention="group", **opt_in, **({} if kv is None else {"kv_cache": kv}))
    assert dec.gqa_grouped
    runs = []
    for seed in seeds:
        ids = kvq._ids(5 + seed % 7, seed)
        T = ids.shape[1]
        want, gaps = _route(model, ids, 24, flags, "heads", kv=kv)
        k = _guarded(gaps)
        runs.append(k)
        if k == 0:
            continue
        got, _ = _route(model, ids, 1 + k, flags, "group", kv=kv)
        assert torch.equal(got, want[:, :T + 1 + k]), (what, seed, k)
        assert torch.equal(dec.generate(ids, 1 + k), want[:, :T + 1 + k]), (what, seed, k)
        assert dec.step is not None and dec.step.gqa_attention == "group" and dec.step.kv_bits == (None if kv is None else int(kv[1]))
    print(f"{what}: guarded steps per prompt {runs}")
    assert sum(runs) >= 8 and sum(k >= 2 for k in runs) >= 2, runs


def test_greedy_tokens_equal_the_heads_steps_while_the_gap_is_kept(models):
    for name in ("llama", "qwen3", "qwen2", "llama_g4"):
        _compare_guarded(models(name), FLAGS[name], OPT_IN[name], None, range(40, 52), name)


def test_graph_replay_and_eager_steps_give_the_same_tokens_and_cache_bytes(models):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    for name in ("llama", "qwen3"):
        model = models(name)
        ids = kvq._ids(7, 9)
        a = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", gqa_attention="group", **OPT_IN[name])
        b = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", gqa_attention="group", **OPT_IN[name])
        ta, tb = a.generate(ids, 24, use_graph=True), b.generate(ids, 24, use_graph=False)
        assert a.step.gqa_attention == "group" and a.graph is not None and b.graph is None
        assert torch.equal(ta, tb), name
        for la, lb in zip(a.cache.layers, b.cache.layers):
            assert kvq._same(la.keys, lb.keys) and kvq._same(la.values, lb.values), name


def test_a_batch_of_ragged_prompts_decodes_each_prompts_batch1_tokens(models):
    """on the dense and on the 8-bit cache"""
    for kv in (None, "q8"):
        _ragged_batch(kv, models)


def _ragged_batch(kv, models):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = models("llama")
    g = torch.Generator().manual_seed(21)
    prompts = [torch.randint(0, 512, (1, T), generator=g).cuda() for T in (3, 9, 5)]
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", gqa_attention="group", kv_cache=kv)
    got = dec.generate_batch(prompts, 20)
    st = dec._batch.get(3)
    assert st is not None and dec.batch_graphs and st["step"].gqa_attention == "group", "the batched fused step served the batch, grouped"
    one = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", gqa_attention="group", kv_cache=kv)
    for b, x in enumerate(prompts):
        assert torch.equal(got[b], one.generate(x, 20)), b


def test_on_a_quantised_cache_the_tokens_are_the_heads_steps(models):
    """the same comparison on the same kind of cache, q8 and q4: "heads" there is ops.attn_decode_kvq_batched"""
    for kv in ("q8", "q4"):
        _compare_guarded(models("llama"), {}, {}, kv, range(60, 72), kv)


# ---- the launches -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """test_step_launches_gpu's recorder with the grouped attention's two wrappers added"""
    from hqq_amd import ops
    rec = []

    def recording(name, real):
        def f(*a, **k):
            rec.append(name[:-len("_batched")] if name.endswith("_batched") else name)
            return real(*a, **k)
        return f

    for name in sl.RECORDED + GQA_OPS:
        monkeypatch.setattr(ops, name, recording(name, getattr(ops, name)))
    return rec


def _one_step(model, rows, **kw):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", **kw)
    if rows == 1:
        dec.generate(sl._prompts([5])[0], 2, use_graph=False)
        return dec, dec.step, (dec.tok, dec.pos)
    dec.generate_batch(sl._prompts([5, 6, 3]), 2, use_graph=False)
    st = dec._batch[rows]
    return dec, st["step"], (st["tok"], st["pos"])


LAUNCHES = [
    # the Llama family on the dense cache: ONE MORE launch than "heads" (FOLDED_HIP has 5, KERNELS_HIP 8)
    ("llama", 1, dict(), True, sl._with(sl.FOLDED_SPLIT, attn_decode="attn_decode_gqa")),
    ("llama", 1, dict(glue="kernels"), False, sl._with(sl.KERNELS_SPLIT, attn_decode="attn_decode_gqa")),
    ("llama_g4", 3, dict(), False, sl._with(sl.KERNELS_SPLIT, attn_decode="attn_decode_gqa")),
    # the Qwen families and every quantised-cache step: the same number as "heads"
    ("qwen3", 1, dict(qk_norm="fused"), True, sl._with(sl.FOLDED_SPLIT, rope_cache="qknorm_rope_cache", attn_decode="attn_decode_gqa")),
    ("qwen2", 1, dict(qkv_bias="fused"), True, sl._with(sl.FOLDED_SPLIT, rope_cache="bias_rope_cache", attn_decode="attn_decode_gqa")),
    ("qwen3", 3, dict(qk_norm="fused"), False, sl._with(sl.KERNELS_SPLIT, rope_cache="qknorm_rope_cache", attn_decode="attn_decode_gqa")),
    ("llama", 1, dict(kv_cache="q8"), True, sl._with(sl.FOLDED_SPLIT, rope_cache="rope_kvq_cache", attn_decode="attn_decode_gqa_kvq")),
    ("llama", 3, dict(kv_cache="q4"), False, sl._with(sl.KERNELS_SPLIT, rope_cache="rope_kvq_cache", attn_decode="attn_decode_gqa_kvq")),
]


def test_launch_sequence_per_block(models, calls):
    """exactly the lists of the step's docstring; with the keyword absent the same decoder records no grouped call and, outside the Llama family's dense case, the
    same number of launches"""
    for name, rows, kw, folded, block in LAUNCHES:
        _launches(name, rows, kw, folded, block, models, calls)


def _launches(name, rows, kw, folded, block, models, calls):
    model = models(name)
    dec, step, args = _one_step(model, rows, gqa_attention="group", **kw)
    assert dec.gqa_grouped and step.gqa_attention == "group"
    glue_kernels = kw.get("glue") == "kernels"
    sl._check(step, args, folded, not glue_kernels, block, calls)
    dec, step, args = _one_step(model, rows, **kw)
    assert not dec.gqa_grouped and step.gqa_attention == "heads"
    calls.clear()
    step(*args)
    torch.cuda.synchronize()
    assert not any(c.startswith("attn_decode_gqa") for c in calls), calls
    front = 0 if glue_kernels else 1
    per_block = (len(calls) - front - 1) // len(step.blocks)
    llama_dense = name.startswith("llama") and "kv_cache" not in kw
    assert per_block == len(block) - (1 if llama_dense else 0), (per_block, calls)
    assert ("rope_attn_decode" in calls) == llama_dense


# ---- the refusals and the plumbing ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(models):
    from hqq_amd.utils.llama_fused import FusedLlamaBatchStep, FusedLlamaStep, supports_gqa_attention
    model, mha = models("llama"), models("mha")
    cache, _ = _prefilled(model, kvq._ids(5, 1))
    assert FusedLlamaStep(model, cache, L, attention="hip").gqa_attention == "heads"
    for other in ("Group", "groups", "tile", None, ""):
        with pytest.raises(ValueError, match="gqa_attention"):
            FusedLlamaStep(model, cache, L, attention="hip", gqa_attention=other)
    with pytest.raises(ValueError, match="attention='hip'"):
        FusedLlamaStep(model, cache, L, attention="sdpa", gqa_attention="group")
    with pytest.raises(ValueError, match="verify"):
        FusedLlamaStep(model, cache, L, attention="hip", batch=4, verify=True, gqa_attention="group")
    mcache, _ = _prefilled(mha, kvq._ids(5, 1))
    assert not supports_gqa_attention(mha)
    with pytest.raises(ValueError, match="attn_gqa_covers"):
        FusedLlamaStep(mha, mcache, L, attention="hip", gqa_attention="group")
    with pytest.raises(ValueError, match="attn_gqa_covers"):
        FusedLlamaBatchStep(mha, mcache, L, 1, attention="hip", gqa_attention="group")


def test_an_mha_model_and_sdpa_decode_as_before(models):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    ids = kvq._ids(6, 3)
    mha = models("mha")
    want = GraphedGreedyDecoder(mha, max_cache_len=L, attention="hip").generate(ids, 24)
    dec = GraphedGreedyDecoder(mha, max_cache_len=L, attention="hip", gqa_attention="group")
    assert dec.gqa_grouped is False and dec.gqa_attention == "group"
    assert torch.equal(dec.generate(ids, 24), want) and dec.step is not None and dec.step.gqa_attention == "heads"
    model = models("llama")
    want = GraphedGreedyDecoder(model, max_cache_len=L, attention="sdpa").generate(ids, 24)
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="sdpa", gqa_attention="group")
    assert dec.gqa_grouped is False
    assert torch.equal(dec.generate(ids, 24), want) and dec.step is not None and dec.step.gqa_attention == "heads"


def test_the_setter_rebuilds_and_speculation_never_sees_the_keyword(models):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = models("llama")
    ids = kvq._ids(6, 3)
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip")
    dec.generate(ids, 8)
    assert dec.step.gqa_attention == "heads" and not dec.gqa_grouped
    dec.gqa_attention = "group"
    dec.generate(ids, 8)
    assert dec.gqa_grouped and dec.step.gqa_attention == "group"
    with pytest.raises(ValueError, match="gqa_attention"):
        dec.gqa_attention = "both"
    spec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", gqa_attention="group", speculate="ngram", draft_rows=4)
    spec.generate(ids, 12)
    assert spec.speculating and spec._spec["step"].gqa_attention == "heads" and spec._spec["step"].verify


def test_hfgenerator_passes_the_keyword_on(models):
    from hqq_amd.utils.generation import HFGenerator
    from test_model_gpu import _ToyTokenizer
    gen = HFGenerator(models("llama"), _ToyTokenizer(), max_new_tokens=16, compile="partial", attention="hip", gqa_attention="group")
    assert gen.decoder.gqa_grouped and gen.decoder.gqa_attention == "group"
    r = gen.generate("7 8 9 10 11 7 8 9", use_chat_template=False, verbose=False)
    assert gen.decoder.step.gqa_attention == "group" and r["output_tokens"].numel() == 16
    with pytest.raises(ValueError, match="gqa_attention"):
        HFGenerator(models("llama"), _ToyTokenizer(), max_new_tokens=16, attention="hip", gqa_attention="kv")


def test_a_context_that_splits_the_attention_inside_a_captured_loop():
    """1100 prompt tokens on a cache of 2048: the grouped attention runs with more than one split, its workspace and the merging launch inside the captured step;
    the captured loop emits the tokens of the same step launched eagerly"""
    from hqq_amd import ops
    from hqq_amd.utils.generation import GraphedGreedyDecoder, kv_bucket
    model = kvq._toy_llama(max_position_embeddings=2048)
    Lbig, T = 2048, 1100
    S = ops.attn_gqa_splits(kv_bucket(T + 39, "hip", Lbig), 1, 2)
    assert S > 1
    ids = torch.randint(0, 512, (1, T), generator=torch.Generator().manual_seed(11)).cuda()
    a = GraphedGreedyDecoder(model, max_cache_len=Lbig, attention="hip", gqa_attention="group")
    b = GraphedGreedyDecoder(model, max_cache_len=Lbig, attention="hip", gqa_attention="group")
    want = b.generate(ids, 40, use_graph=False)
    for _ in range(2):
        assert torch.equal(a.generate(ids, 40, use_graph=True), want)
    assert a.gqa_grouped and a.graph is not None and S in a.step.attn_ws and a.step.attn_ws[S] is not None
