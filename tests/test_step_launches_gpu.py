"""What the fused decode step launches, mode by mode (the README's launch counts as explicit lists of hqq_amd.ops calls), when the generate loops take the
one-launch argmax_advance, and the single-sequence C symbols of csrc/block.hip against the ops wrappers bit for bit.  Tiny models: hidden 256, 2 blocks,
4 heads of 64, vocabulary 512, a cache of 64 positions."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

GLUE = ("token_prologue", "rope_cache", "attn_decode", "rope_attn_decode", "argmax_advance")
RECORDED = ("add_rmsnorm", "gemv", "gemv_grouped", "gemv_block", "gemv_axis0", "gemv_axis0_grouped", "silu_mul") + GLUE + tuple(n + "_batched" for n in GLUE) + \
    ("qknorm_rope_cache_batched", "bias_rope_cache_batched", "rope_kvq_cache_batched", "attn_decode_kvq_batched", "rope_cache_shared", "attn_decode_shared",
     "attn_decode_tiled", "moe_router", "moe_gate_up", "moe_down")

KERNELS_SDPA = ["add_rmsnorm", "gemv_grouped", "rope_cache", "gemv", "add_rmsnorm", "gemv_grouped", "silu_mul", "gemv"]
KERNELS_HIP = [("rope_attn_decode" if n == "rope_cache" else n) for n in KERNELS_SDPA]
FOLDED_SDPA = ["gemv_block"] * 4
FOLDED_HIP = ["gemv_block", "rope_attn_decode", "gemv_block", "gemv_block", "gemv_block"]
AXIS0_SDPA = ["add_rmsnorm", "gemv_axis0_grouped", "rope_cache", "gemv_axis0", "add_rmsnorm", "gemv_axis0_grouped", "gemv_axis0"]
# the rotary-and-cache launch and the attention as launches of their own (Qwen3 / Qwen2 / Mixtral with the kernel attention, the quantised cache, the verify step)
KERNELS_SPLIT = ["add_rmsnorm", "gemv_grouped", "rope_cache", "attn_decode", "gemv", "add_rmsnorm", "gemv_grouped", "silu_mul", "gemv"]
FOLDED_SPLIT = ["gemv_block", "rope_cache", "attn_decode", "gemv_block", "gemv_block", "gemv_block"]
MOE_HIP = ["add_rmsnorm", "gemv_grouped", "rope_cache", "attn_decode", "gemv", "add_rmsnorm", "moe_router", "moe_gate_up", "moe_down"]


def _with(block, **other):
    """`block` with other launches in the named ones' places"""
    return [other.get(n, n) for n in block]


def _model(axis):
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=512,
                      max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).half().cuda().eval()
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=axis), compute_dtype=torch.float16, device="cuda")
    prepare_for_inference(model, backend="hip")
    if axis == 1:
        group_llama_projections(model)
    return model


@pytest.fixture(scope="module")
def axis1_model():
    return _model(1)


@pytest.fixture(scope="module")
def axis0_model():
    return _model(0)


@pytest.fixture
def calls(monkeypatch):
    """every hqq_amd.ops function of the decode path wrapped with a recorder; a *_batched name is recorded as its single-sequence name"""
    from hqq_amd import ops
    rec = []

    def recording(name, real):
        def f(*a, **k):
            rec.append(name[:-len("_batched")] if name.endswith("_batched") else name)
            return real(*a, **k)
        return f

    for name in RECORDED:
        monkeypatch.setattr(ops, name, recording(name, getattr(ops, name)))
    return rec


def _prompts(lengths):
    g = torch.Generator().manual_seed(7)
    return [torch.randint(0, 512, (1, T), generator=g).cuda() for T in lengths]


@pytest.mark.parametrize("mode,kw,block,front", [
    ("kernels-sdpa", dict(glue="kernels"), KERNELS_SDPA, False),
    ("kernels-hip", dict(glue="kernels", attention="hip"), KERNELS_HIP, False),
    ("folded-sdpa", dict(), FOLDED_SDPA, True),
    ("folded-hip", dict(attention="hip"), FOLDED_HIP, True),
    ("axis0-sdpa", dict(axis0="fused"), AXIS0_SDPA, True),
    ("batch3-sdpa", dict(), KERNELS_SDPA, True),
])
def test_launch_sequence_of_one_step(mode, kw, block, front, axis1_model, axis0_model, calls):
    _check_llama_mode(mode, kw, block, front, axis0_model if mode.startswith("axis0") else axis1_model, calls)


def _check_llama_mode(mode, kw, block, front, model, calls):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    dec = GraphedGreedyDecoder(model, max_cache_len=64, **kw)
    if mode.startswith("batch3"):
        dec.generate_batch(_prompts([5, 6, 3]), 2, use_graph=False)
        st = dec._batch[3]
        step, args = st["step"], (st["tok"], st["pos"])
    else:
        dec.generate(_prompts([5])[0], 2, use_graph=False)   # prefill (the model's own forward) + one eager step
        step, args = dec.step, (dec.tok, dec.pos)
    assert step is not None and step.folded == mode.startswith("folded") and step.one_launch_front == front
    calls.clear()
    step(*args)
    torch.cuda.synchronize()
    nblocks = len(model.model.layers)
    assert calls == (["token_prologue"] if front else []) + block * nblocks + ["add_rmsnorm"], (mode, calls)


# ---- the modes beyond plain Llama: Qwen3 / Qwen2, Mixtral with the kernel attention, the quantised cache, the verify step, a batch with the kernel attention ----
def _quantised(model, experts=False):
    """as the sibling files prepare their toys: int4, group_size 64, axis 1; the dense families grouped, Mixtral's expert stacks quantised too"""
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    qc = BaseQuantizeConfig(nbits=4, group_size=64, axis=1)
    quantize_model(model, qc, compute_dtype=torch.float16, device="cuda", **(dict(expert_config=qc) if experts else {}))
    prepare_for_inference(model, backend="hip")
    if not experts:
        group_llama_projections(model)
    return model


def _tiny_mixtral():
    """tests/test_moe_step_gpu.py's Mixtral with hidden 256, i.e. heads of 64: the decode-attention kernel covers head_dim 64 / 128 / 256, and that file's toy has 32"""
    from transformers import MixtralConfig, MixtralForCausalLM
    torch.manual_seed(0)
    cfg = MixtralConfig(vocab_size=512, hidden_size=256, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=4, num_experts_per_tok=2, max_position_embeddings=128)
    return _quantised(MixtralForCausalLM(cfg).half().cuda().eval(), experts=True)


@pytest.fixture(scope="module")
def family_models():
    """name -> the quantised, patched toy of that family (built once each, left unchanged) and the decoder keywords that opt it in"""
    import test_qknorm_gpu
    import test_qkv_bias_gpu
    build = {"qwen3": (lambda: _quantised(test_qknorm_gpu._tiny_qwen3()), dict(qk_norm="fused")),
             "qwen2": (lambda: _quantised(test_qkv_bias_gpu._tiny_qwen2()), dict(qkv_bias="fused")),
             "mixtral": (_tiny_mixtral, dict(moe="fused"))}
    built = {}

    def get(name):
        if name not in built:
            built[name] = build[name][0]()
        return built[name], build[name][1]
    return get


def _check(step, args, folded, front, block, calls):
    assert step is not None and step.folded == folded and step.one_launch_front == front
    calls.clear()
    step(*args)
    torch.cuda.synchronize()
    assert calls == (["token_prologue"] if front else []) + block * len(step.blocks) + ["add_rmsnorm"], calls


@pytest.mark.parametrize("mode,kw,block", [
    ("kernels-sdpa", dict(glue="kernels"), KERNELS_SDPA),
    ("kernels-hip", dict(glue="kernels", attention="hip"), KERNELS_SPLIT),
    ("folded-sdpa", dict(), ["gemv_block", "rope_cache"] + ["gemv_block"] * 3),
    ("folded-hip", dict(attention="hip"), FOLDED_SPLIT),
])
@pytest.mark.parametrize("family,rotary", [("qwen3", "qknorm_rope_cache"), ("qwen2", "bias_rope_cache")])
def test_launch_sequence_of_the_qwen_families(family, rotary, mode, kw, block, family_models, calls):
    """the family's rotary-and-cache launch is always one of its own: no rotary-paired q / k copies, no rope_attn_decode"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, opt_in = family_models(family)
    dec = GraphedGreedyDecoder(model, max_cache_len=64, **opt_in, **kw)
    dec.generate(_prompts([5])[0], 2, use_graph=False)
    assert dec.step is not None and all("qkv_rope" not in b for b in dec.step.blocks)
    _check(dec.step, (dec.tok, dec.pos), mode.startswith("folded"), mode.startswith("folded"), _with(block, rope_cache=rotary), calls)


def test_launch_sequence_of_mixtral_with_the_kernel_attention(family_models, calls):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, opt_in = family_models("mixtral")
    dec = GraphedGreedyDecoder(model, max_cache_len=64, attention="hip", **opt_in)
    dec.generate(_prompts([5])[0], 2, use_graph=False)
    _check(dec.step, (dec.tok, dec.pos), False, True, MOE_HIP, calls)


@pytest.mark.parametrize("rows", [1, 3])
def test_launch_sequence_on_the_quantised_cache(rows, axis1_model, calls):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    dec = GraphedGreedyDecoder(axis1_model, max_cache_len=64, attention="hip", kv_cache="q8")
    if rows == 1:
        dec.generate(_prompts([5])[0], 2, use_graph=False)
        step, args = dec.step, (dec.tok, dec.pos)
    else:
        dec.generate_batch(_prompts([5, 6, 3]), 2, use_graph=False)
        st = dec._batch[3]
        step, args = st["step"], (st["tok"], st["pos"])
    block = _with(FOLDED_SPLIT if rows == 1 else KERNELS_SPLIT, rope_cache="rope_kvq_cache", attn_decode="attn_decode_kvq")
    _check(step, args, rows == 1, True, block, calls)


@pytest.mark.parametrize("verify_attention,attn", [("rows", "attn_decode_shared"), ("tile", "attn_decode_tiled")])
def test_launch_sequence_of_the_verify_step(verify_attention, attn, axis1_model, calls):
    """(the step binds its attention kernel when it is built: the recorder — the `calls` fixture — is in place before that)"""
    from transformers import StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    T, R = 5, 4
    cache = StaticCache(config=axis1_model.config, max_cache_len=64)
    with torch.no_grad():
        axis1_model(_prompts([T])[0], past_key_values=cache, cache_position=torch.arange(T, device="cuda"), use_cache=True)
    step = FusedLlamaStep(axis1_model, cache, 64, attention="hip", batch=R, verify=True, verify_attention=verify_attention)
    tok = torch.randint(0, 512, (R, 1), generator=torch.Generator().manual_seed(9)).cuda()
    _check(step, (tok, torch.arange(T, T + R, device="cuda")), False, True, _with(KERNELS_SPLIT, rope_cache="rope_cache_shared", attn_decode=attn), calls)


def test_launch_sequence_of_a_batch_with_the_kernel_attention(axis1_model, calls):
    _check_llama_mode("batch3-hip", dict(attention="hip"), KERNELS_HIP, True, axis1_model, calls)


@pytest.mark.parametrize("glue", ["auto", "kernels"])
def test_when_the_generate_loops_take_argmax_advance(glue, axis1_model, calls):
    """greedy decoding: generate() takes the one-launch argmax_advance unless the decoder was built with glue="kernels" (the comparison leg with
    the separate front and back); generate_batch() takes it either way"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    dec = GraphedGreedyDecoder(axis1_model, max_cache_len=64, glue=glue)
    dec.generate(_prompts([5])[0], 3, use_graph=False)
    assert ("argmax_advance" in calls) == (glue == "auto"), calls
    assert ("token_prologue" in calls) == (glue == "auto")
    calls.clear()
    dec.generate_batch(_prompts([5, 6, 3]), 3, use_graph=False)
    assert dec._batch.get(3) is not None and dec._batch[3]["step"].one_launch_front
    assert "argmax_advance" in calls and "token_prologue" in calls, calls


def test_single_sequence_symbols_equal_the_ops_wrappers():
    """hqq_hip_token_prologue / rope_cache / attn_decode / rope_attn_decode / argmax_advance called through the C ABI, against the hqq_amd.ops
    wrappers of the same names on copies of the same inputs: outputs and both caches bit for bit"""
    from hqq_amd import _C, ops
    lib = _C.lib()
    F16 = ops.F16
    nh, nkv, hd, L, H, V = 4, 2, 64, 32, 256, 512
    g = torch.Generator(device="cuda").manual_seed(11)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=g).half()

    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    scaling = hd ** -0.5
    tok, pos = torch.tensor([[417]], device="cuda"), torch.tensor([19], device="cuda")
    # token_prologue
    emb, ct, st = rnd(V, H), rnd(L, hd), rnd(L, hd)
    a = [torch.full((n,), 7.0, dtype=torch.float16, device="cuda") for n in (H, hd, hd, L)]
    b = [t.clone() for t in a]
    assert lib.hqq_hip_token_prologue(p(tok), p(pos), p(emb), V, H, p(ct), p(st), L, hd, p(a[0]), p(a[1]), p(a[2]), p(a[3]), F16, stream) == 0
    ops.token_prologue(tok, pos, emb, *([b[0], ct, st] + b[1:]))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[0], emb[417]) and torch.equal(a[1], ct[19])
    # rope_cache
    q, k, v = rnd(1, nh * hd), rnd(1, nkv * hd), rnd(1, nkv * hd)
    ang = torch.rand(hd // 2, device="cuda", generator=g) * 6.28
    cos, sin = torch.cat([ang.cos(), ang.cos()]).half(), torch.cat([ang.sin(), ang.sin()]).half()
    kc, vc = rnd(nkv, L, hd), rnd(nkv, L, hd)
    kc1, vc1, kc2, vc2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    qr1, qr2 = torch.empty(1, nh, 1, hd, dtype=torch.float16, device="cuda"), torch.empty(1, nh, 1, hd, dtype=torch.float16, device="cuda")
    assert lib.hqq_hip_rope_cache(p(q), p(k), p(v), p(cos), p(sin), p(pos), p(qr1), p(kc1), p(vc1), nh, nkv, hd, L, F16, stream) == 0
    ops.rope_cache(q, k, v, cos, sin, pos, kc2, vc2, qr2)
    assert torch.equal(qr1, qr2) and torch.equal(kc1, kc2) and torch.equal(vc1, vc2) and not torch.equal(kc1, kc)
    # attn_decode on the caches just written, one workgroup per head and the keys shared out over two
    for splits in (1, 2):
        ws = ops.attn_workspace("cuda", nh, hd, splits)
        o1, o2 = torch.full((nh * hd,), 7.0, dtype=torch.float16, device="cuda"), torch.full((nh * hd,), 7.0, dtype=torch.float16, device="cuda")
        assert lib.hqq_hip_attn_decode(p(qr1), p(kc1), p(vc1), p(pos), p(o1), nh, nkv, hd, L, scaling, F16, splits, p(ws), 0 if ws is None else ws.numel(), stream) == 0
        ops.attn_decode(qr2, kc2, vc2, pos, o2, scaling, splits=splits)
        assert torch.equal(o1, o2) and bool(torch.isfinite(o1).all())
        # rope_attn_decode from the raw projections
        ka, va, kb, vb = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        r1, r2 = torch.full_like(o1, 7.0), torch.full_like(o1, 7.0)
        assert lib.hqq_hip_rope_attn_decode(p(q), p(k), p(v), p(cos), p(sin), p(pos), p(ka), p(va), p(r1), nh, nkv, hd, L, scaling, F16, splits, p(ws),
                                            0 if ws is None else ws.numel(), stream) == 0
        ops.rope_attn_decode(q, k, v, cos, sin, pos, kb, vb, r2, scaling, splits=splits)
        assert torch.equal(r1, r2) and torch.equal(ka, kb) and torch.equal(va, vb) and torch.equal(ka, kc1) and torch.equal(va, vc1)
    # argmax_advance
    logits = rnd(1, V)
    logits[0, [300, 100]] = logits.max() + 1   # a tie: the first index
    s1 = [torch.full((1, 1), -1, device="cuda"), torch.full((1, 1), -1, device="cuda"), torch.tensor([19], device="cuda")]
    s2 = [t.clone() for t in s1]
    assert lib.hqq_hip_argmax_advance(p(logits), V, F16, p(s1[0]), p(s1[1]), p(s1[2]), stream) == 0
    ops.argmax_advance(logits, *s2)
    assert all(torch.equal(x, y) for x, y in zip(s1, s2)) and int(s1[0]) == 100 and int(s1[2]) == 20
    n1, n2 = torch.full((1, 1), -1, device="cuda"), torch.full((1, 1), -1, device="cuda")
    assert lib.hqq_hip_argmax_advance(p(logits), V, F16, p(n1), None, None, stream) == 0
    ops.argmax_advance(logits, n2)
    assert torch.equal(n1, n2) and int(n1) == 100
