"""The opt-in fused decode step for Qwen2 / Qwen2.5 models on the GPU: hqq_hip_bias_rope_cache_batched (the q / k / v projection biases, rotary embedding and
KV-cache write in one launch) bit for bit against the HF ops it restates and against the library's own biased route (gemv_grouped with the biases, then
rope_cache_batched), and GraphedGreedyDecoder(qkv_bias="fused") against the same quantised model decoding under HQQBackend.PYTORCH_FORWARD, token for token."""
import copy

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

# (n_heads, n_kv_heads, head_dim): 192, 640, 256, 384 and 21 threads — an exact multiple of the 256-thread block, ragged last blocks, less than one wave; a head
# count that is no multiple of anything; a head_dim no other block kernel serves
SHAPES = [(4, 2, 64), (8, 2, 128), (3, 1, 128), (2, 1, 256), (5, 2, 6)]
DTYPES = [torch.float16, torch.bfloat16]
L = 16


def _inputs(n_heads, n_kv, hd, dt, B, seed):
    """q / k / v rows and three biases, all different and non-zero"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v = ((1.5 * torch.randn(B, n * hd, device="cuda", generator=g)).to(dt) for n in (n_heads, n_kv, n_kv))
    qb, kb, vb = ((0.5 * torch.randn(n * hd, device="cuda", generator=g)).to(dt) for n in (n_heads, n_kv, n_kv))
    assert all(bool(t.ne(0).any()) for t in (qb, kb, vb)) and not torch.equal(kb, vb)
    return q, k, v, qb, kb, vb


def _rotary_rows(hd, dt, pos):
    """cos / sin [B, hd] of the positions, from HF's Qwen2 rotary module (positions beyond the cache are still positions)"""
    from transformers import Qwen2Config
    from transformers.models.qwen2.modeling_qwen2 import Qwen2RotaryEmbedding
    rot = Qwen2RotaryEmbedding(Qwen2Config(hidden_size=4 * hd, num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=128)).cuda()
    cos, sin = rot(torch.empty(1, 1, hd, dtype=dt, device="cuda"), pos.view(1, -1))
    assert cos.shape[-1] == hd
    return cos[0].contiguous(), sin[0].contiguous()


def _cached(B, n_kv, hd, pos, k_rot, v):
    """zeroed caches [B, n_kv, L, hd] with row b's rotated key / value written at pos[b] by index_copy_ (StaticLayer.update's op); a position outside
    the cache writes nothing"""
    kc = torch.zeros(B, n_kv, L, hd, dtype=k_rot.dtype, device="cuda")
    vc = torch.zeros_like(kc)
    for b in range(B):
        if 0 <= int(pos[b]) < L:
            kc[b].index_copy_(1, pos[b:b + 1], k_rot[b])
            vc[b].index_copy_(1, pos[b:b + 1], v.view(B, n_kv, 1, hd)[b])
    return kc, vc


def _run(q, k, v, qb, kb, vb, cos, sin, pos, n_heads, n_kv, hd):
    from hqq_amd import ops
    B, dt = q.shape[0], q.dtype
    kc = torch.zeros(B, n_kv, L, hd, dtype=dt, device="cuda")
    vc = torch.zeros_like(kc)
    qo = torch.full((B, n_heads, 1, hd), float("nan"), dtype=dt, device="cuda")   # an unwritten element shows
    ops.bias_rope_cache_batched(q, k, v, qb, kb, vb, cos, sin, pos, kc, vc, qo)
    return qo, kc, vc


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_kernel_equals_the_hf_ops_bit_for_bit(n_heads, n_kv, hd, dt):
    """(q + q_bias), (k + k_bias), (v + v_bias) by torch in the dtype -> apply_rotary_pos_emb -> index_copy_ into a zeroed cache, all on the GPU, against
    one launch: torch.equal on q_out and on both whole caches (so every unwritten slot is still zero) — one sequence at position 0, L - 1 and L, and three
    sequences at those positions together.  The row at pos = L leaves both caches untouched and still gets its q_out.  No tolerance: torch's fp16 / bf16 add
    rounds an fp32 sum, which for an addition at these widths (24 >= 2 * 11 + 2) is the correctly rounded sum, the kernel's single rounding."""
    from transformers.models.qwen2.modeling_qwen2 import apply_rotary_pos_emb
    from hqq_amd import ops
    for B, positions in ((1, [0]), (1, [L - 1]), (1, [L]), (3, [0, L - 1, L])):
        q, k, v, qb, kb, vb = _inputs(n_heads, n_kv, hd, dt, B, 100 * hd + n_heads + B + positions[0])
        pos = torch.tensor(positions, device="cuda")
        cos, sin = _rotary_rows(hd, dt, pos)
        qp, kp, vp = q + qb, k + kb, v + vb
        q_want, k_want = apply_rotary_pos_emb(qp.view(B, 1, n_heads, hd).transpose(1, 2), kp.view(B, 1, n_kv, hd).transpose(1, 2), cos.view(B, 1, hd), sin.view(B, 1, hd))
        kc_want, vc_want = _cached(B, n_kv, hd, pos, k_want, vp)
        qo, kc, vc = _run(q, k, v, qb, kb, vb, cos, sin, pos, n_heads, n_kv, hd)
        assert torch.equal(qo, q_want), (B, positions)
        assert torch.equal(kc, kc_want) and torch.equal(vc, vc_want), (B, positions)
        if positions[-1] == L:
            assert torch.count_nonzero(kc[-1]) == 0 and torch.count_nonzero(vc[-1]) == 0
            assert not bool(torch.isnan(qo[-1]).any())
        if B == 1 and positions[0] < L:   # the single-sequence alias: the same call on views
            kc1, vc1 = torch.zeros(n_kv, L, hd, dtype=dt, device="cuda"), torch.zeros(n_kv, L, hd, dtype=dt, device="cuda")
            qo1 = torch.full((1, n_heads, 1, hd), float("nan"), dtype=dt, device="cuda")
            ops.bias_rope_cache(q, k, v, qb, kb, vb, cos.view(-1), sin.view(-1), pos, kc1, vc1, qo1)
            assert torch.equal(qo1, qo) and torch.equal(kc1, kc[0]) and torch.equal(vc1, vc[0])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_two_calls_give_the_same_bits(n_heads, n_kv, hd, dt):
    q, k, v, qb, kb, vb = _inputs(n_heads, n_kv, hd, dt, 3, 7 * hd + n_heads)
    pos = torch.tensor([0, L - 1, 5], device="cuda")
    cos, sin = _rotary_rows(hd, dt, pos)
    a = _run(q, k, v, qb, kb, vb, cos, sin, pos, n_heads, n_kv, hd)
    b = _run(q, k, v, qb, kb, vb, cos, sin, pos, n_heads, n_kv, hd)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not bool(torch.isnan(a[0]).any())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", DTYPES)
def test_kernel_equals_the_library_s_own_biased_route_bit_for_bit(dt, B):
    """tiny axis-1 int4 layers (K = 128, group_size 64, N = 256 / 128 / 128: 4 heads, 2 KV heads, head_dim 64): ops.gemv_grouped WITH the biases ->
    ops.rope_cache_batched, against ops.gemv_grouped WITHOUT them -> ops.bias_rope_cache_batched.  torch.equal on q_out and both caches: the step computes
    what the biased linears compute."""
    from hqq_amd import ops
    K, gs, nbits, n_heads, n_kv, hd = 128, 64, 4, 4, 2, 64
    g = torch.Generator().manual_seed(40 + B)
    layers, biases = [], []
    for N in (n_heads * hd, n_kv * hd, n_kv * hd):
        R = N * K // gs
        U = torch.randint(0, 2 ** nbits, (R, gs), generator=g, dtype=torch.uint8)
        s = (torch.rand(R, 1, generator=g) * 0.04 + 0.01).to(dt).cuda()
        z = (torch.rand(R, 1, generator=g) * (2 ** nbits - 1)).to(dt).cuda()
        layers.append((ops.pack(nbits, U.cuda()), s, z, N))
        biases.append((0.5 * torch.randn(N, generator=g)).to(dt).cuda())
    x = torch.randn(B, K, generator=g).to(dt).cuda()
    pos = torch.tensor([0, L - 1, 7][:B], device="cuda")
    cos, sin = _rotary_rows(hd, dt, pos)

    def caches():
        return (torch.zeros(B, n_kv, L, hd, dtype=dt, device="cuda"), torch.zeros(B, n_kv, L, hd, dtype=dt, device="cuda"),
                torch.full((B, n_heads, 1, hd), float("nan"), dtype=dt, device="cuda"))

    yb = ops.gemv_grouped(x, [(P, s, z, b, N) for (P, s, z, N), b in zip(layers, biases)], K, gs, nbits)
    y0 = ops.gemv_grouped(x, [(P, s, z, None, N) for (P, s, z, N) in layers], K, gs, nbits)
    assert not any(torch.equal(a, b) for a, b in zip(yb, y0))   # the biases reached the biased route
    kc_w, vc_w, qo_w = caches()
    ops.rope_cache_batched(yb[0], yb[1], yb[2], cos, sin, pos, kc_w, vc_w, qo_w)
    kc, vc, qo = caches()
    ops.bias_rope_cache_batched(y0[0], y0[1], y0[2], *biases, cos, sin, pos, kc, vc, qo)
    assert torch.equal(qo, qo_w) and torch.equal(kc, kc_w) and torch.equal(vc, vc_w)
    assert torch.count_nonzero(kc) > 0 and torch.count_nonzero(vc) > 0


# ---- the step and the decoder -------------------------------------------------------------------------------------------------------------
def _attention_linears(model):
    return [getattr(blk.self_attn, n) for blk in model.model.layers for n in ("q_proj", "k_proj", "v_proj")]


def _tiny_qwen2():
    """head_dim 64; q / k / v biases 0.5 randn (Qwen2's initialiser zeroes them, which would hide an ignored or swapped bias)"""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(0)
    cfg = Qwen2Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
                      max_position_embeddings=128)
    model = Qwen2ForCausalLM(cfg).half().cuda().eval().requires_grad_(False)   # (inference only; the quantised layers' bias clones are then plain leaves, deep-copyable)
    g = torch.Generator().manual_seed(11)
    for lin in _attention_linears(model):
        lin.bias.data = (0.5 * torch.randn(lin.out_features, generator=g)).half().cuda()
    return model


def _patched(model):
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.utils.patching import prepare_for_inference
    prepare_for_inference(model, backend="hip")
    group_llama_projections(model)
    return model


@pytest.fixture(scope="module")
def qwen2():
    """(the quantised, patched, grouped model; a deep copy of the quantised model from before the patch; a prompt; the copy's 32 greedy tokens under
    HQQBackend.PYTORCH_FORWARD; a second copy with the q / k / v biases zeroed before its patch) — built once, left unchanged by the tests that share it"""
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    model = _tiny_qwen2()
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=torch.float16, device="cuda")
    ref, zeroed = copy.deepcopy(model), copy.deepcopy(model)
    with torch.no_grad():
        for lin in _attention_linears(zeroed):
            lin.bias.zero_()
    assert all(bool(lin.bias.ne(0).any()) for lin in _attention_linears(model))   # the copies are deep: the model keeps its biases
    _patched(model)
    _patched(zeroed)
    ids = torch.randint(0, 512, (1, 6), generator=torch.Generator().manual_seed(3)).cuda()
    want = _pytorch_forward(lambda: ref.generate(ids, max_new_tokens=32, do_sample=False, pad_token_id=0))
    return model, ref, ids, want, zeroed


def _pytorch_forward(fn):
    from hqq_amd.core.quantize import HQQBackend, HQQLinear
    HQQLinear.set_backend(HQQBackend.PYTORCH_FORWARD)
    try:
        with torch.no_grad():
            return fn()
    finally:
        HQQLinear.set_backend(HQQBackend.HIP)


@pytest.mark.parametrize("glue", ["folded", "kernels"])
def test_fused_qwen2_decoder_emits_the_tokens_of_the_pytorch_backend_and_of_the_default_route(qwen2, glue):
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, _, ids, want, zeroed = qwen2
    assert llama_fused.supports_qkv_bias(model) and llama_fused.supports_qkv_bias_batch(model, 3)
    assert not llama_fused.supports(model) and not llama_fused.arch_supported(model) and not llama_fused.supports_qk_norm(model)
    dec = GraphedGreedyDecoder(model, max_cache_len=64, qkv_bias="fused", glue=glue)
    assert dec.fused_qkv_bias and not dec.fused and not dec.fused_qk_norm and not dec.fused_axis0
    got = dec.generate(ids, 32)
    assert dec.step is not None and dec.graph is not None and dec.step.folded == (glue == "folded") and dec.step.qkv_bias
    assert all("qkv_rope" not in b for b in dec.step.blocks)   # the bias comes before the rotation: no rotary-paired copies
    assert all(rec[3] is None for b in dec.step.blocks for rec in b["qkv"])   # the q|k|v launch stays bias-free
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    default = GraphedGreedyDecoder(model, max_cache_len=64).generate(ids, 32)
    assert torch.equal(got, default), (got.tolist(), default.tolist())
    # not vacuous: the same model with its biases zeroed decodes other tokens through the same step
    assert llama_fused.supports_qkv_bias(zeroed)
    dz = GraphedGreedyDecoder(zeroed, max_cache_len=64, qkv_bias="fused", glue=glue)
    assert dz.fused_qkv_bias
    got_z = dz.generate(ids, 32)
    assert dz.step is not None and dz.step.qkv_bias
    assert not torch.equal(got_z, want), "the biases do not reach the tokens: the comparison above shows nothing"


def test_default_route_is_unchanged(qwen2):
    """without the keyword: the model's own forward, graph-replayed, and the same tokens"""
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, _, ids, want, _ = qwen2
    assert not llama_fused.supports(model)
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    assert dec.fused_qkv_bias is False and dec.fused is False and dec.fused_qk_norm is False
    got = dec.generate(ids, 32)
    assert dec.step is None
    assert torch.equal(got, want), (got.tolist(), want.tolist())


def test_step_refuses_what_it_does_not_serve(qwen2):
    from transformers import LlamaConfig, LlamaForCausalLM, StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    model = qwen2[0]
    cache = StaticCache(config=model.config, max_cache_len=64)
    with pytest.raises(ValueError, match="qkv_bias"):
        FusedLlamaStep(model, cache, 64, qkv_bias=True, axis0=True)
    with pytest.raises(ValueError, match="qkv_bias"):
        FusedLlamaStep(model, cache, 64, qkv_bias=True, qk_norm=True)
    llama = LlamaForCausalLM(LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
                                         max_position_embeddings=128)).half().cuda().eval()
    with pytest.raises(ValueError, match="qkv_bias"):
        FusedLlamaStep(llama, StaticCache(config=llama.config, max_cache_len=64), 64, qkv_bias=True)


def _prompts(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 512, (1, T), generator=g).cuda() for T in lengths]


def test_ragged_batch_decodes_the_tokens_of_batch1_decoding(qwen2):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, ref = qwen2[0], qwen2[1]
    prompts = _prompts([3, 6, 9], 21)
    dec = GraphedGreedyDecoder(model, max_cache_len=64, qkv_bias="fused")
    got = dec.generate_batch(prompts, 16)
    assert dec._batch.get(3) is not None and dec.batch_graphs and dec._batch[3]["step"].qkv_bias, "the batched step served the batch"
    one = GraphedGreedyDecoder(model, max_cache_len=64, qkv_bias="fused")
    for b, x in enumerate(prompts):
        assert got[b].shape == (1, x.shape[1] + 16)
        assert torch.equal(got[b], one.generate(x, 16)), b
        want = _pytorch_forward(lambda: ref.generate(x, max_new_tokens=16, do_sample=False, pad_token_id=0))
        assert torch.equal(got[b], want), (b, got[b].tolist(), want.tolist())


def _teacher_forced(model, prompts, seqs, steps, attention):
    """the batched step's logits [steps, B, vocab] when row b is fed seqs[b]'s tokens after its prompt (tests/test_batch_decode_gpu.py's comparison)"""
    from transformers import StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaBatchStep
    cfg, B, Lc = model.config, len(prompts), 64
    hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    bc = StaticCache(config=cfg, max_cache_len=Lc)
    bc.early_initialization(B, cfg.num_key_value_heads, hd, torch.float16, torch.device("cuda"))
    for b, x in enumerate(prompts):
        c = StaticCache(config=cfg, max_cache_len=Lc)
        with torch.no_grad():
            model(x, past_key_values=c, cache_position=torch.arange(x.shape[1], device="cuda"), use_cache=True)
        for dst, src in zip(bc.layers, c.layers):
            dst.keys[b, :, :x.shape[1]].copy_(src.keys[0, :, :x.shape[1]])
            dst.values[b, :, :x.shape[1]].copy_(src.values[0, :, :x.shape[1]])
    step = FusedLlamaBatchStep(model, bc, Lc, B, attention=attention, qkv_bias=True)
    T = [x.shape[1] for x in prompts]
    out = []
    for t in range(steps):
        tok = torch.stack([seqs[b][0, T[b] + t] for b in range(B)]).view(B, 1)
        pos = torch.tensor([T[b] + t for b in range(B)], device="cuda")
        out.append(step(tok, pos, Lc).float().clone())
    return torch.stack(out)


def test_kernel_attention_on_the_biased_rotated_query(qwen2):
    """attention="hip" with qkv_bias: ops.attn_decode_batched on the new kernel's q_out.  What tests/test_qknorm_gpu.py asks of Qwen3's kernel attention, with
    its tolerance (rtol = atol = 5e-3 on teacher-forced logits): batched decoding emits batch-1 decoding's tokens, and the step's logits on those tokens are
    those of the model's own forward — and of the same step with HF's attention function."""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = qwen2[0]
    prompts = _prompts([3, 6, 9], 22)
    dec = GraphedGreedyDecoder(model, max_cache_len=64, qkv_bias="fused", attention="hip")
    got = dec.generate_batch(prompts, 16)
    assert dec._batch.get(3) is not None and dec.batch_graphs
    one = GraphedGreedyDecoder(model, max_cache_len=64, qkv_bias="fused", attention="hip")
    for b, x in enumerate(prompts):
        assert torch.equal(got[b], one.generate(x, 16)), b
    assert one.step is not None and one.step.attention == "hip" and one.step.qkv_bias
    hip = _teacher_forced(model, prompts, got, 12, "hip")
    sdpa = _teacher_forced(model, prompts, got, 12, "sdpa")
    torch.testing.assert_close(hip, sdpa, rtol=5e-3, atol=5e-3)
    for b, x in enumerate(prompts):
        T = x.shape[1]
        with torch.no_grad():
            want = model(got[b][:, :T + 12]).logits[0, T:T + 12].float()
        torch.testing.assert_close(hip[:, b], want, rtol=5e-3, atol=5e-3)
