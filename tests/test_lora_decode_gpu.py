"""GPU half of the un-merged LoRA decode tests: the two kernels of csrc/lora_decode.hip on the cases of tests/_lora_decode_cases.py (exact bits on the
constructed cases, the derived bound on the randn ones, determinism, row independence, grouped == per layer, the workspace contract, guard regions),
and the fused decode step / GraphedGreedyDecoder with lora="fused" on tiny adapted Llamas (hidden 256, 2 blocks, 4 heads of 64, vocabulary 512, int4,
group_size 64, a cache of 64 positions) against the model's own forward."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

import _lora_decode_cases as C   # noqa: E402

TOL = 5e-3          # rtol = atol on teacher-forced logits: the project's bar for a step that changes arithmetic on this tiny model (tests/test_qknorm_gpu.py)
CACHE = 64


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------
def _guarded(t: torch.Tensor, fill: float = 7.0, pad: int = 64):
    """a dense CUDA copy of t at the front of a larger buffer: (the copy, the buffer's tail, which nothing may write)"""
    buf = torch.full((t.numel() + pad,), fill, dtype=t.dtype, device="cuda")
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf[:t.numel()].view(t.shape), buf[t.numel():]


def _run(cid, rows=None, ws_fill=0x00, layer_ids=None):
    """ops.lora_apply on a case (optionally on the rows `rows` only, or on the layers `layer_ids` only): the outputs, and the guard regions' state"""
    from hqq_amd import ops
    case = C.BY_ID[cid]
    x, layers = C.inputs(cid)
    if layer_ids is not None:
        layers = [layers[i] for i in layer_ids]
    sel = slice(None) if rows is None else rows
    xg = x[sel].contiguous().cuda()
    M = xg.shape[0]
    need = ops.lora_decode_workspace_bytes(M, case.K, [A.shape[1] for A, _, _, _ in layers])
    assert need == C.workspace_bytes(M, case.K, [A.shape[1] for A, _, _, _ in layers])
    ws = torch.full((need + 256,), ws_fill, dtype=torch.uint8, device="cuda")
    ws[need:] = 0xA5
    ys, tails = zip(*[_guarded(y0[sel].contiguous()) for _, _, _, y0 in layers])
    ops.lora_apply(xg, [(A.cuda(), B.cuda(), s) for A, B, s, _ in layers], list(ys), workspace=ws)
    torch.cuda.synchronize()
    intact = all(bool((t == 7.0).all()) for t in tails) and bool((ws[need:] == 0xA5).all())
    return [y.cpu() for y in ys], intact


@pytest.mark.parametrize("cid", [c.id for c in C.CONSTRUCTED])
def test_constructed_cases_bit_for_bit(cid):
    got, intact = _run(cid)
    assert intact, "a guard region after an output or after the used part of the workspace was written"
    for l, (g, want) in enumerate(zip(got, C.expected(cid))):
        assert torch.equal(g, want), (l, int((g != want).sum()), float((g.double() - want.double()).abs().max()))


@pytest.mark.parametrize("cid", [c.id for c in C.RANDN])
def test_randn_cases_within_the_derived_bound(cid):
    got, intact = _run(cid)
    assert intact
    for l, (g, (y64, bound)) in enumerate(zip(got, C.expected(cid))):
        err = (g.double() - y64).abs()
        print(f"{cid} layer {l}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (l, float((err / bound).max()))
    _, layers = C.inputs(cid)
    assert any(not torch.equal(g, y0) for g, (_, _, _, y0) in zip(got, layers)), "the adapter term changed nothing"


def _cid(kind, name):
    """the id of the case of that kind and name (the families rotate over the dtype pairs: the pair is looked up, not restated)"""
    return next(c.id for c in C.CASES if c.kind == kind and c.name == name)


SEVERAL_SLICES = ["randn-group3-base-float16xfloat32", "randn-group3-base-bfloat16xbfloat16", _cid("randn", "K11008-r64"), _cid("randn", "M16"),
                  _cid("randn", "K1032-r256"), _cid("randn", "N584")]


@pytest.mark.parametrize("cid", SEVERAL_SLICES)
def test_two_calls_give_the_same_bits_whatever_the_workspace_held(cid):
    """(the workspace needs no clearing: every partial is written before it is read — a NaN-filled one gives the bits of a zeroed one)"""
    assert cid in C.BY_ID
    a, _ = _run(cid)
    b, _ = _run(cid)
    c, intact = _run(cid, ws_fill=0xFF)   # fp32 0xFFFFFFFF: a NaN in every slot
    assert intact
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z) and bool(torch.isfinite(x.float()).all())


@pytest.mark.parametrize("cid", [_cid("randn", "M5"), _cid("randn", "M16"), "randn-group3-base-bfloat16xfloat32", "randn-group3-base-float16xfloat16"])
def test_a_row_of_a_batch_has_the_bits_of_the_one_row_call(cid):
    case = C.BY_ID[cid]
    full, _ = _run(cid)
    for m in range(case.M):
        one, _ = _run(cid, rows=slice(m, m + 1))
        for l, (f, o) in enumerate(zip(full, one)):
            assert torch.equal(f[m:m + 1], o), (m, l)


@pytest.mark.parametrize("cid", [_cid("randn", "group3"), _cid("randn", "group4"), "constructed-group3-base-bfloat16xfloat32"])
def test_a_grouped_call_equals_the_per_layer_calls(cid):
    assert cid in C.BY_ID
    full, _ = _run(cid)
    for l in range(len(full)):
        one, intact = _run(cid, layer_ids=[l])
        assert intact and torch.equal(full[l], one[0]), l


def _wrapped_layer(ldt):
    """an HQQLinearLoRA around a 264 x 512 int4 layer (two K slices, a ragged second expand tile), rank 17, with a trained-looking lora_B"""
    from hqq_amd.core.peft import HQQLinearLoRA
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    torch.manual_seed(3)
    lin = torch.nn.Linear(512, 264, bias=False).half().cuda()
    w = HQQLinearLoRA(HQQLinear(lin, BaseQuantizeConfig(nbits=4, group_size=64), compute_dtype=torch.float16, device="cuda"), {"r": 17, "lora_alpha": 8})
    w.lora_B.data = torch.randn_like(w.lora_B) * 0.05
    return w.cast(ldt)


@pytest.mark.parametrize("ldt", [torch.float32, torch.float16])
def test_lora_apply_on_a_wrapped_layer_against_float64(ldt):
    """the base layer's output, then ops.lora_apply: within the derived bound of the float64 value of wrapper(x), which is that output + s x A B"""
    from hqq_amd import ops
    w = _wrapped_layer(ldt)
    x = torch.randn(5, 512, generator=torch.Generator().manual_seed(4)).half().cuda()
    with torch.no_grad():
        y0 = w.linear_layer(x)
        ref = w(x)
    y = y0.clone()
    ops.lora_apply(x, [(w.lora_A.data, w.lora_B.data, w._scaling_float())], [y])
    y64, bound = C.reference64(x.cpu(), w.lora_A.data.cpu(), w.lora_B.data.cpu(), w._scaling_float(), y0.cpu())
    err = (y.cpu().double() - y64).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert not torch.equal(y, y0)
    torch.testing.assert_close(y, ref, rtol=2e-2, atol=2e-2)   # (the wrapper's own forward rounds more often: a sanity check, not the bar)


# ---- the step and the decoder ------------------------------------------------------------------------------------------------------------------------
ATTN, MLP = ("q_proj", "k_proj", "v_proj", "o_proj"), ("gate_proj", "up_proj", "down_proj")
FIXTURES = {
    # name: (axis, adapted linears, adapter dtype)
    "axis1-all7-f32": (1, ATTN + MLP, torch.float32),
    "axis1-qv-f16": (1, ("q_proj", "v_proj"), torch.float16),
    "axis0-all7-f32": (0, ATTN + MLP, torch.float32),
}
# the first prompt seed of 0, 1, 2, ... for which the DEFAULT route alone (the model's own forward) has a top-2 logit gap of at least 8 TOL on at least the
# first 24 of its 32 greedy steps (found by running _compared_steps over the seeds on an MI355X; test_greedy_tokens... re-checks the premise)
# compared steps per seed as measured: axis1-all7-f32 1, 2, 0, 2, 0, 5, 2, 8, 2, 0, 0, 32; axis1-qv-f16 1, 0, 2, 3, 32; axis0-all7-f32 0, 1, 0, 1, 0, 0, 5, 6, 2, 7, 0, 32
PROMPT_SEED = {"axis1-all7-f32": 11, "axis1-qv-f16": 4, "axis0-all7-f32": 11}


def _build(name):
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.peft import PeftUtils, is_hqq_lora_layer
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    axis, adapted, ldt = FIXTURES[name]
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=512,
                      max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).half().cuda().eval()
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=axis), compute_dtype=torch.float16, device="cuda")
    peft = {f"self_attn.{n}": ({"r": 8, "lora_alpha": 16, "dropout": 0.0} if n in adapted else None) for n in ATTN}
    peft.update({f"mlp.{n}": ({"r": 4, "lora_alpha": 16, "dropout": 0.0} if n in adapted else None) for n in MLP})
    PeftUtils.add_lora(model, peft)
    g = torch.Generator().manual_seed(5)
    for _, m in model.named_modules():
        if is_hqq_lora_layer(m):   # LoRA's own initialiser zeroes lora_B, which would hide an ignored adapter
            m.lora_B.data = (0.05 * torch.randn(m.lora_B.shape, generator=g)).to(m.lora_B.device)
    if ldt != torch.float32:
        PeftUtils.cast_lora_weights(model, ldt)
    prepare_for_inference(model, backend="hip")
    if axis == 1:
        group_llama_projections(model)
    return model.eval()


@pytest.fixture(scope="module", params=list(FIXTURES))
def adapted(request):
    """(fixture name, the adapted, patched model, the decoder keywords that opt it in) — built once per fixture, left unchanged by the tests"""
    name = request.param
    kw = dict(lora="fused", axis0="fused") if FIXTURES[name][0] == 0 else dict(lora="fused")
    return name, _build(name), kw


def _prompts(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 512, (1, T), generator=g).cuda() for T in lengths]


def _wrappers(model):
    from hqq_amd.core.peft import is_hqq_lora_layer
    return [m for m in model.modules() if is_hqq_lora_layer(m)]


def test_predicates(adapted):
    from hqq_amd.backends.hip import HQQLinearHIP
    from hqq_amd.utils import llama_fused
    name, model, _ = adapted
    axis = FIXTURES[name][0]
    assert all(isinstance(w.linear_layer, HQQLinearHIP) for w in _wrappers(model)) and len(_wrappers(model)) == 2 * len(FIXTURES[name][1])
    assert llama_fused.supports_lora(model) and llama_fused.supports_lora_batch(model, 3) and llama_fused.supports_lora(model, axis0=bool(axis == 0))
    assert not llama_fused.supports_lora(model, axis0=bool(axis == 1))
    assert not llama_fused.supports(model) and not llama_fused.supports_axis0(model) and not llama_fused.supports_batch(model, 3)
    assert not llama_fused.supports_lora_batch(model, 17)


def _block_calls(name):
    axis, adapted_names, _ = FIXTURES[name]
    ad = ["lora_shrink", "lora_expand"]
    qkv = ad if any(n in adapted_names for n in ("q_proj", "k_proj", "v_proj")) else []
    o = ad if "o_proj" in adapted_names else []
    gu = ad if any(n in adapted_names for n in ("gate_proj", "up_proj")) else []
    d = ad if "down_proj" in adapted_names else []
    if axis == 1:
        return ["add_rmsnorm", "gemv_grouped"] + qkv + ["rope_cache", "gemv"] + o + ["add_rmsnorm", "gemv_grouped"] + gu + ["silu_mul", "gemv"] + d
    # axis 0: SiLU * up rides in the grouped launch unless gate | up carry an adapter (the adapter terms come before SiLU)
    return ["add_rmsnorm", "gemv_axis0_grouped"] + qkv + ["rope_cache", "gemv_axis0"] + o + ["add_rmsnorm", "gemv_axis0_grouped"] + gu + \
        (["silu_mul"] if gu else []) + ["gemv_axis0"] + d


RECORDED = ("add_rmsnorm", "gemv", "gemv_grouped", "gemv_block", "gemv_axis0", "gemv_axis0_grouped", "silu_mul", "lora_shrink", "lora_expand", "lora_apply",
            "token_prologue_batched", "rope_cache_batched", "attn_decode_batched", "rope_attn_decode_batched", "argmax_advance_batched")


def test_decoder_takes_the_step_and_its_launch_sequence(adapted, monkeypatch):
    """the recorded ops calls of one step: the kernels-mode list with lora_shrink, lora_expand after each adapted group, nothing after an un-adapted one"""
    from hqq_amd import ops
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    name, model, kw = adapted
    dec = GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw)
    assert dec.fused_lora and not dec.fused and not dec.fused_axis0
    dec.generate(_prompts([5], 7)[0], 4)
    assert dec.step is not None and dec.step.lora and not dec.step.folded and dec.step.one_launch_front and dec.graph is not None, "the step served, a graph was captured"
    assert dec.step.axis0 == (FIXTURES[name][0] == 0)
    rec = []

    def recording(fname, real):
        def f(*a, **k):
            rec.append(fname[:-len("_batched")] if fname.endswith("_batched") else fname)
            return real(*a, **k)
        return f

    for fname in RECORDED:
        monkeypatch.setattr(ops, fname, recording(fname, getattr(ops, fname)))
    dec.step(dec.tok, dec.pos)
    torch.cuda.synchronize()
    assert rec == ["token_prologue"] + _block_calls(name) * len(model.model.layers) + ["add_rmsnorm"], rec
    # the batched step: the same sequence
    dec.generate_batch(_prompts([5, 6, 3], 7), 2, use_graph=False)
    st = dec._batch.get(3)
    assert st is not None and st["step"].lora
    rec.clear()
    st["step"](st["tok"], st["pos"])
    torch.cuda.synchronize()
    assert rec == ["token_prologue"] + _block_calls(name) * len(model.model.layers) + ["add_rmsnorm"], rec


def _teacher_forced(model, prompts, seqs, steps, axis0):
    """the lora step's logits [steps, B, vocab] when row b is fed seqs[b]'s tokens after its prompt (tests/test_qknorm_gpu.py's comparison)"""
    from transformers import StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaBatchStep, FusedLlamaStep
    cfg, B = model.config, len(prompts)
    hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    bc = StaticCache(config=cfg, max_cache_len=CACHE)
    bc.early_initialization(B, cfg.num_key_value_heads, hd, torch.float16, torch.device("cuda"))
    for b, x in enumerate(prompts):
        c = StaticCache(config=cfg, max_cache_len=CACHE)
        with torch.no_grad():
            model(x, past_key_values=c, cache_position=torch.arange(x.shape[1], device="cuda"), use_cache=True)
        for dst, src in zip(bc.layers, c.layers):
            dst.keys[b, :, :x.shape[1]].copy_(src.keys[0, :, :x.shape[1]])
            dst.values[b, :, :x.shape[1]].copy_(src.values[0, :, :x.shape[1]])
    step = FusedLlamaStep(model, bc, CACHE, axis0=axis0, lora=True) if B == 1 else FusedLlamaBatchStep(model, bc, CACHE, B, axis0=axis0, lora=True)
    T = [x.shape[1] for x in prompts]
    out = []
    for t in range(steps):
        tok = torch.stack([seqs[b][0, T[b] + t] for b in range(B)]).view(B, 1)
        pos = torch.tensor([T[b] + t for b in range(B)], device="cuda")
        out.append(step(tok, pos, CACHE).float().clone())
    return torch.stack(out)


def _own_forward_logits(model, seq, T, steps):
    with torch.no_grad():
        return model(seq[:, :T + steps]).logits[0, T:T + steps].float()


def test_teacher_forced_logits_of_one_sequence(adapted):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    name, model, _ = adapted
    x = _prompts([6], 21)[0]
    seq = GraphedGreedyDecoder(model, max_cache_len=CACHE).generate(x, 16)   # the default route's tokens
    got = _teacher_forced(model, [x], [seq], 12, FIXTURES[name][0] == 0)[:, 0]
    want = _own_forward_logits(model, seq, 6, 12)
    print(f"{name}: max |step - model| = {float((got - want).abs().max()):.2e}")
    torch.testing.assert_close(got, want, rtol=TOL, atol=TOL)


def test_adapters_are_not_ignored(adapted):
    """not vacuous: with every lora_B zeroed (in place: the step reads the same tensors), the same step's logits differ from the adapted ones by more
    than ten times the tolerance somewhere"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    name, model, _ = adapted
    x = _prompts([6], 21)[0]
    seq = GraphedGreedyDecoder(model, max_cache_len=CACHE).generate(x, 16)
    with_adapters = _teacher_forced(model, [x], [seq], 12, FIXTURES[name][0] == 0)
    saved = [w.lora_B.data.clone() for w in _wrappers(model)]
    try:
        for w in _wrappers(model):
            w.lora_B.data.zero_()
        without = _teacher_forced(model, [x], [seq], 12, FIXTURES[name][0] == 0)
    finally:
        for w, b in zip(_wrappers(model), saved):
            w.lora_B.data.copy_(b)
    diff = float((with_adapters - without).abs().max())
    print(f"{name}: max |adapted - zeroed| = {diff:.3f}")
    assert diff > 10 * TOL


def test_ragged_batch_of_three(adapted):
    """generate_batch through the batched lora step: each row decodes batch-1 decoding's tokens, and the step's teacher-forced logits are the model's own"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    name, model, kw = adapted
    prompts = _prompts([3, 6, 9], 22)
    dec = GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw)
    got = dec.generate_batch(prompts, 16)
    assert dec._batch.get(3) is not None and dec.batch_graphs and dec._batch[3]["step"].lora, "the batched step served the batch"
    one = GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw)
    for b, x in enumerate(prompts):
        assert got[b].shape == (1, x.shape[1] + 16)
        assert torch.equal(got[b], one.generate(x, 16)), b
    assert one.step is not None and one.step.lora
    logits = _teacher_forced(model, prompts, got, 12, FIXTURES[name][0] == 0)
    for b, x in enumerate(prompts):
        torch.testing.assert_close(logits[:, b], _own_forward_logits(model, got[b], x.shape[1], 12), rtol=TOL, atol=TOL)


def _compared_steps(model, seq, T, n):
    """how many of the n greedy steps of the default route are compared: up to the first whose own top-2 logit gap (the model's own forward on its own
    tokens) is below 8 TOL"""
    with torch.no_grad():
        lg = model(seq[:, :T + n - 1]).logits[0, T - 1:].float()   # the logits each of the n new tokens was picked from
    top = lg.topk(2, dim=-1).values
    close = ((top[:, 0] - top[:, 1]) < 8 * TOL).nonzero()
    return int(close[0]) if close.numel() else n


def test_greedy_tokens_equal_the_default_routes(adapted):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    name, model, kw = adapted
    x = _prompts([6], PROMPT_SEED[name])[0]
    want = GraphedGreedyDecoder(model, max_cache_len=CACHE).generate(x, 32)
    n = _compared_steps(model, want, 6, 32)
    print(f"{name}: prompt seed {PROMPT_SEED[name]}, {n} of 32 steps compared")
    assert n >= 24, "the recorded prompt seed no longer meets its premise on the default route"
    dec = GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw)
    got = dec.generate(x, 32)
    assert dec.step is not None and dec.step.lora and dec.graph is not None
    assert torch.equal(got[:, :6 + n], want[:, :6 + n]), (got.tolist(), want.tolist())


def test_default_route_is_unchanged(adapted):
    """lora="model" and a decoder built without the keyword: the model's own forward, the same tokens"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    name, model, kw = adapted
    x = _prompts([6], 23)[0]
    plain = GraphedGreedyDecoder(model, max_cache_len=CACHE)
    want = plain.generate(x, 12)
    assert plain.step is None and not plain.fused_lora and plain.lora == "model"
    explicit = GraphedGreedyDecoder(model, max_cache_len=CACHE, **dict(kw, lora="model"))
    assert torch.equal(explicit.generate(x, 12), want) and explicit.step is None and not explicit.fused_lora
    with pytest.raises(ValueError, match="lora"):
        GraphedGreedyDecoder(model, max_cache_len=CACHE, lora="yes")


def test_step_refuses_what_it_does_not_serve(adapted):
    from transformers import StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    name, model, _ = adapted
    axis0 = FIXTURES[name][0] == 0
    cache = StaticCache(config=model.config, max_cache_len=CACHE)
    for bad in (dict(glue="folded"), dict(qk_norm=True), dict(qkv_bias=True)):
        with pytest.raises(ValueError, match="lora=True"):
            FusedLlamaStep(model, cache, CACHE, lora=True, axis0=axis0, **bad)
    with pytest.raises(ValueError, match="supports_lora"):   # the other axis
        FusedLlamaStep(model, cache, CACHE, lora=True, axis0=not axis0)


def test_step_refuses_a_model_without_adapters():
    from transformers import LlamaConfig, LlamaForCausalLM, StaticCache
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=512,
                      max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).half().cuda().eval()
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=torch.float16, device="cuda")
    prepare_for_inference(model, backend="hip")
    assert llama_fused.supports(model) and not llama_fused.supports_lora(model)
    with pytest.raises(ValueError, match="supports_lora"):
        llama_fused.FusedLlamaStep(model, StaticCache(config=cfg, max_cache_len=CACHE), CACHE, lora=True)


def test_reloaded_adapters_rebuild_the_kept_state(tmp_path):
    """PeftUtils.load_lora_weights replaces the adapters' tensors: the next generate() sees another fingerprint, rebuilds step and graphs, and matches
    the default route on the new adapters"""
    from hqq_amd.core.peft import PeftUtils
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    name = "axis1-qv-f16"
    model = _build(name)
    x = _prompts([6], PROMPT_SEED[name])[0]
    dec = GraphedGreedyDecoder(model, max_cache_len=CACHE, lora="fused")
    first = dec.generate(x, 16)
    step0, fp0 = dec.step, dec._fp
    assert step0 is not None and step0.lora
    assert torch.equal(dec.generate(x, 16), first) and dec.step is step0, "the kept state serves the next prompt"
    # other adapters, saved by a second model and loaded into the first
    f = str(tmp_path / "lora.pt")
    other = _build(name)
    g = torch.Generator().manual_seed(99)
    for w in _wrappers(other):
        w.lora_B.data = (0.05 * torch.randn(w.lora_B.shape, generator=g)).to(device=w.lora_B.device, dtype=w.lora_B.dtype)
    PeftUtils.save_lora_weights(other, f)
    PeftUtils.load_lora_weights(model, f)
    second = dec.generate(x, 16)
    assert dec._fp != fp0 and dec.step is not step0 and dec.step is not None and dec.step.lora and dec.graph is not None
    assert second.shape == first.shape
    # the comparison prompt for the NEW adapters: the first seed whose default route alone keeps a top-2 gap of 8 TOL over at least 8 of 16 steps
    plain = GraphedGreedyDecoder(model, max_cache_len=CACHE)
    for seed in range(64):
        x2 = _prompts([6], seed)[0]
        want = plain.generate(x2, 16)
        n = _compared_steps(model, want, 6, 16)
        if n >= 8:
            break
    assert n >= 8, "no prompt among 64 seeds meets the premise on the default route"
    got = dec.generate(x2, 16)
    assert dec.step is not None and dec.step.lora
    assert torch.equal(got[:, :6 + n], want[:, :6 + n]), (got.tolist(), want.tolist())
    assert torch.equal(want, GraphedGreedyDecoder(other, max_cache_len=CACHE).generate(x2, 16)), "the loaded adapters are the saved ones"
