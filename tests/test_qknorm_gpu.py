"""The opt-in fused decode step for Qwen3 models on the GPU: hqq_hip_qknorm_rope_cache_batched (per-head q_norm / k_norm, rotary embedding, KV-cache
write in one launch) against the HF modules it restates — bit for bit where the fp32 sum of squares is exact in any order, within a derived bound of
a float64-sum restatement on random inputs — and GraphedGreedyDecoder(qk_norm="fused") against the same quantised model decoding under
HQQBackend.PYTORCH_FORWARD, token for token."""
import copy

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

SHAPES = [(4, 2, 64), (8, 2, 128), (3, 1, 128), (2, 1, 256)]   # (n_heads, n_kv_heads, head_dim): one, one and two rotary pairs per lane; a head count that is no multiple of the workgroup's four waves
DTYPES = [torch.float16, torch.bfloat16]
L = 16
EPS_Q, EPS_K = 1e-6, 1e-5   # two different epsilons: a kernel that used one for both would show


def _inputs(n_heads, n_kv, hd, dt, B, exact, seed):
    """q / k / v rows, norm weights (different for q and k) and the rotary rows of the positions the caller picks"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if exact:   # {+-0.5, +-1, +-2}: squares 0.25 / 1 / 4, every partial sum of up to 256 of them is exact in fp32 whatever the order
        vals = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], device="cuda")
        q = vals[torch.randint(0, 6, (B, n_heads * hd), device="cuda", generator=g)].to(dt)
        k = vals[torch.randint(0, 6, (B, n_kv * hd), device="cuda", generator=g)].to(dt)
    else:
        q = (1.5 * torch.randn(B, n_heads * hd, device="cuda", generator=g)).to(dt)
        k = (1.5 * torch.randn(B, n_kv * hd, device="cuda", generator=g)).to(dt)
    v = torch.randn(B, n_kv * hd, device="cuda", generator=g).to(dt)
    qw = (1 + 0.1 * torch.randn(hd, device="cuda", generator=g)).to(dt)
    kw = (1 + 0.1 * torch.randn(hd, device="cuda", generator=g)).to(dt)
    return q, k, v, qw, kw


def _rotary_rows(hd, dt, pos):
    """cos / sin [B, hd] of the positions, from HF's Qwen3 rotary module (positions beyond the cache are still positions)"""
    from transformers import Qwen3Config
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RotaryEmbedding
    rot = Qwen3RotaryEmbedding(Qwen3Config(hidden_size=4 * hd, num_attention_heads=4, num_key_value_heads=4, head_dim=hd, max_position_embeddings=128)).cuda()
    cos, sin = rot(torch.empty(1, 1, hd, dtype=dt, device="cuda"), pos.view(1, -1))
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


def _run(q, k, v, qw, kw, cos, sin, pos, n_heads, n_kv, hd):
    from hqq_amd import ops
    B, dt = q.shape[0], q.dtype
    kc = torch.zeros(B, n_kv, L, hd, dtype=dt, device="cuda")
    vc = torch.zeros_like(kc)
    qo = torch.full((B, n_heads, 1, hd), float("nan"), dtype=dt, device="cuda")
    ops.qknorm_rope_cache_batched(q, k, v, qw, kw, EPS_Q, EPS_K, cos, sin, pos, kc, vc, qo)
    return qo, kc, vc


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_kernel_equals_the_hf_modules_where_the_sum_of_squares_is_exact(n_heads, n_kv, hd, dt):
    """Qwen3RMSNorm -> apply_rotary_pos_emb -> index_copy_ into a zeroed cache, all on the GPU, against one launch: torch.equal on q_out, both caches
    (so every unwritten slot is still zero) — one sequence at position 0, L - 1 and L, and three sequences at those positions together.  The row at
    pos = L leaves both caches untouched and still gets its q_out.  (Rests, as add_rmsnorm's test does, on rsqrtf and torch.rsqrt agreeing on this device.)"""
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, apply_rotary_pos_emb
    from hqq_amd import ops
    qn, kn = Qwen3RMSNorm(hd, eps=EPS_Q).cuda().to(dt), Qwen3RMSNorm(hd, eps=EPS_K).cuda().to(dt)
    for B, positions in ((1, [0]), (1, [L - 1]), (1, [L]), (3, [0, L - 1, L])):
        q, k, v, qw, kw = _inputs(n_heads, n_kv, hd, dt, B, True, 100 * hd + n_heads + B + positions[0])
        qn.weight.data, kn.weight.data = qw, kw
        pos = torch.tensor(positions, device="cuda")
        cos, sin = _rotary_rows(hd, dt, pos)
        with torch.no_grad():
            q_want, k_want = apply_rotary_pos_emb(qn(q.view(B, 1, n_heads, hd)).transpose(1, 2), kn(k.view(B, 1, n_kv, hd)).transpose(1, 2),
                                                  cos.view(B, 1, hd), sin.view(B, 1, hd))
        kc_want, vc_want = _cached(B, n_kv, hd, pos, k_want, v)
        qo, kc, vc = _run(q, k, v, qw, kw, cos, sin, pos, n_heads, n_kv, hd)
        assert torch.equal(qo, q_want), (B, positions)
        assert torch.equal(kc, kc_want) and torch.equal(vc, vc_want), (B, positions)
        if positions[-1] == L:
            assert torch.count_nonzero(kc[-1]) == 0 and torch.count_nonzero(vc[-1]) == 0
        if B == 1 and positions[0] < L:   # the single-sequence alias: the same call on views
            kc1, vc1 = torch.zeros(n_kv, L, hd, dtype=dt, device="cuda"), torch.zeros(n_kv, L, hd, dtype=dt, device="cuda")
            qo1 = torch.empty(1, n_heads, 1, hd, dtype=dt, device="cuda")
            ops.qknorm_rope_cache(q, k, v, qw, kw, EPS_Q, EPS_K, cos.view(-1), sin.view(-1), pos, kc1, vc1, qo1)
            assert torch.equal(qo1, qo) and torch.equal(kc1, kc[0]) and torch.equal(vc1, vc[0])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_kernel_on_random_inputs_against_a_float64_sum_restatement(n_heads, n_kv, hd, dt):
    """1.5 randn inputs against the same chain with the sum of squares taken in float64 and rounded once to fp32, every other rounding as Qwen3RMSNorm /
    apply_rotary_pos_emb make it.  Equal except on at most 1 % of the elements; a differing element within 3 u (|n1| + |n2|), n1 / n2 the two normalised
    inputs of its rotary pair, u = 2^-10 (fp16) / 2^-7 (bf16).  Derived, not measured: another summation order moves a normalised value by at most one
    ulp of T, each of the two rounded products then by at most 2 u |n|, and the rounded sum adds one more ulp.  Two calls give the same bits."""
    from transformers.models.qwen3.modeling_qwen3 import apply_rotary_pos_emb
    u = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    B = 3
    q, k, v, qw, kw = _inputs(n_heads, n_kv, hd, dt, B, False, 7 * hd + n_heads)
    pos = torch.tensor([0, L - 1, 5], device="cuda")
    cos, sin = _rotary_rows(hd, dt, pos)

    def norm(x, w, eps):   # Qwen3RMSNorm.forward with the variance from a float64 sum
        var = x.double().pow(2).mean(-1, keepdim=True).float()
        return w * (x.float() * torch.rsqrt(var + eps)).to(dt)

    nq, nk = norm(q.view(B, 1, n_heads, hd), qw, EPS_Q).transpose(1, 2), norm(k.view(B, 1, n_kv, hd), kw, EPS_K).transpose(1, 2)
    q_want, k_want = apply_rotary_pos_emb(nq, nk, cos.view(B, 1, hd), sin.view(B, 1, hd))
    kc_want, vc_want = _cached(B, n_kv, hd, pos, k_want, v)
    qo, kc, vc = _run(q, k, v, qw, kw, cos, sin, pos, n_heads, n_kv, hd)
    qo2, kc2, vc2 = _run(q, k, v, qw, kw, cos, sin, pos, n_heads, n_kv, hd)
    assert torch.equal(qo, qo2) and torch.equal(kc, kc2) and torch.equal(vc, vc2)
    assert torch.equal(vc, vc_want)
    k_got = torch.stack([kc[b, :, int(pos[b])] for b in range(B)]).view(B, n_kv, 1, hd)
    written = torch.zeros_like(kc, dtype=torch.bool)
    for b in range(B):
        written[b, :, int(pos[b])] = True
    assert torch.count_nonzero(kc[~written]) == 0
    for name, got, want, n in (("q", qo, q_want, nq), ("k", k_got, k_want, nk)):
        mag = n.float().abs()
        pair = mag[..., :hd // 2] + mag[..., hd // 2:]
        bound = 3 * u * torch.cat([pair, pair], dim=-1)
        err = (got.float() - want.float()).abs()
        differ = got != want
        print(f"{name} {dt} {(n_heads, n_kv, hd)}: {int(differ.sum())} of {differ.numel()} elements differ, max err / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
        assert int(differ.sum()) <= 0.01 * differ.numel(), (name, int(differ.sum()), differ.numel())
        assert bool((err <= bound).all()), (name, float((err - bound).max()))


# ---- the step and the decoder -------------------------------------------------------------------------------------------------------------
def _tiny_qwen3():
    """head_dim 128 != hidden / heads = 64 (an assumed hidden_size // num_attention_heads is caught); q_norm / k_norm weights distinct from one another
    and from the all-ones default, which would hide a swapped or ignored weight"""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    torch.manual_seed(0)
    cfg = Qwen3Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128, vocab_size=512,
                      max_position_embeddings=128)
    model = Qwen3ForCausalLM(cfg).half().cuda().eval()
    g = torch.Generator().manual_seed(11)
    for blk in model.model.layers:
        for nrm in (blk.self_attn.q_norm, blk.self_attn.k_norm):
            nrm.weight.data = (1 + 0.1 * torch.randn(128, generator=g)).half().cuda()
    return model


@pytest.fixture(scope="module")
def qwen3():
    """(the quantised, patched, grouped model; a deep copy of the quantised model from before the patch; a prompt; the copy's 32 greedy tokens under
    HQQBackend.PYTORCH_FORWARD) — built once, left unchanged by the tests that share it"""
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    model = _tiny_qwen3()
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=torch.float16, device="cuda")
    ref = copy.deepcopy(model)
    prepare_for_inference(model, backend="hip")
    group_llama_projections(model)
    ids = torch.randint(0, 512, (1, 6), generator=torch.Generator().manual_seed(3)).cuda()
    want = _pytorch_forward(lambda: ref.generate(ids, max_new_tokens=32, do_sample=False, pad_token_id=0))
    return model, ref, ids, want


def _pytorch_forward(fn):
    from hqq_amd.core.quantize import HQQBackend, HQQLinear
    HQQLinear.set_backend(HQQBackend.PYTORCH_FORWARD)
    try:
        with torch.no_grad():
            return fn()
    finally:
        HQQLinear.set_backend(HQQBackend.HIP)


@pytest.mark.parametrize("glue", ["folded", "kernels"])
def test_fused_qwen3_decoder_emits_the_tokens_of_the_pytorch_backend(qwen3, glue):
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, _, ids, want = qwen3
    assert llama_fused.supports_qk_norm(model) and llama_fused.supports_qk_norm_batch(model, 3)
    assert not llama_fused.supports(model) and not llama_fused.arch_supported(model)
    dec = GraphedGreedyDecoder(model, max_cache_len=64, qk_norm="fused", glue=glue)
    assert dec.fused_qk_norm and not dec.fused and not dec.fused_axis0
    got = dec.generate(ids, 32)
    assert dec.step is not None and dec.graph is not None and dec.step.folded == (glue == "folded") and dec.step.qk_norm
    assert all("qkv_rope" not in b for b in dec.step.blocks)   # the head norm comes before the rotation: no rotary-paired copies
    assert torch.equal(got, want), (got.tolist(), want.tolist())


def test_default_route_is_unchanged(qwen3):
    """without the keyword: the model's own forward, graph-replayed, and the same tokens.  (The replayed forward takes its cache slot from StaticLayer's
    cumulative_length, which the warm-up step in front of a capture advances: the decoder puts it back with the token and the position.)"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, _, ids, want = qwen3
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    assert dec.fused_qk_norm is False and dec.fused is False
    got = dec.generate(ids, 32)
    assert dec.step is None
    assert torch.equal(got, want), (got.tolist(), want.tolist())


def test_step_refuses_what_it_does_not_serve(qwen3):
    from transformers import StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    model = qwen3[0]
    cache = StaticCache(config=model.config, max_cache_len=64)
    with pytest.raises(ValueError, match="qk_norm"):
        FusedLlamaStep(model, cache, 64, qk_norm=True, axis0=True)


def _prompts(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 512, (1, T), generator=g).cuda() for T in lengths]


def test_ragged_batch_decodes_the_tokens_of_batch1_decoding(qwen3):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, ref = qwen3[0], qwen3[1]
    prompts = _prompts([3, 6, 9], 21)
    dec = GraphedGreedyDecoder(model, max_cache_len=64, qk_norm="fused")
    got = dec.generate_batch(prompts, 16)
    assert dec._batch.get(3) is not None and dec.batch_graphs and dec._batch[3]["step"].qk_norm, "the batched step served the batch"
    one = GraphedGreedyDecoder(model, max_cache_len=64, qk_norm="fused")
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
    bc = StaticCache(config=cfg, max_cache_len=Lc)
    bc.early_initialization(B, cfg.num_key_value_heads, cfg.head_dim, torch.float16, torch.device("cuda"))
    for b, x in enumerate(prompts):
        c = StaticCache(config=cfg, max_cache_len=Lc)
        with torch.no_grad():
            model(x, past_key_values=c, cache_position=torch.arange(x.shape[1], device="cuda"), use_cache=True)
        for dst, src in zip(bc.layers, c.layers):
            dst.keys[b, :, :x.shape[1]].copy_(src.keys[0, :, :x.shape[1]])
            dst.values[b, :, :x.shape[1]].copy_(src.values[0, :, :x.shape[1]])
    step = FusedLlamaBatchStep(model, bc, Lc, B, attention=attention, qk_norm=True)
    T = [x.shape[1] for x in prompts]
    out = []
    for t in range(steps):
        tok = torch.stack([seqs[b][0, T[b] + t] for b in range(B)]).view(B, 1)
        pos = torch.tensor([T[b] + t for b in range(B)], device="cuda")
        out.append(step(tok, pos, Lc).float().clone())
    return torch.stack(out)


def test_kernel_attention_on_the_normalised_rotated_query(qwen3):
    """attention="hip" with qk_norm: ops.attn_decode_batched on the new kernel's q_out.  The comparison tests/test_batch_decode_gpu.py makes for
    attention="hip", with its tolerance (rtol = atol = 5e-3 on teacher-forced logits): batched decoding emits batch-1 decoding's tokens, and the
    step's logits on those tokens are those of the model's own forward — and of the same step with HF's attention function."""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = qwen3[0]
    prompts = _prompts([3, 6, 9], 22)
    dec = GraphedGreedyDecoder(model, max_cache_len=64, qk_norm="fused", attention="hip")
    got = dec.generate_batch(prompts, 16)
    assert dec._batch.get(3) is not None and dec.batch_graphs
    one = GraphedGreedyDecoder(model, max_cache_len=64, qk_norm="fused", attention="hip")
    for b, x in enumerate(prompts):
        assert torch.equal(got[b], one.generate(x, 16)), b
    assert one.step is not None and one.step.attention == "hip" and one.step.qk_norm
    hip = _teacher_forced(model, prompts, got, 12, "hip")
    sdpa = _teacher_forced(model, prompts, got, 12, "sdpa")
    torch.testing.assert_close(hip, sdpa, rtol=5e-3, atol=5e-3)
    for b, x in enumerate(prompts):
        T = x.shape[1]
        with torch.no_grad():
            want = model(got[b][:, :T + 12]).logits[0, T:T + 12].float()
        torch.testing.assert_close(hip[:, b], want, rtol=5e-3, atol=5e-3)
