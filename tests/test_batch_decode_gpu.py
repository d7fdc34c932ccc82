"""Batched decoding on a GPU: the *_batched glue kernels of csrc/block.hip against B calls of their batch-1 siblings (bit for bit), the coverage rule
against what the fused linears run, FusedLlamaBatchStep against the model's own forward, and GraphedGreedyDecoder.generate_batch against batch-1
decoding of every prompt (tokens), HF's generate on the reference's arithmetic (tokens) and teacher-forced logits."""
import copy

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---- the glue kernels, row b against the batch-1 kernel on sequence b ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_token_prologue_batched_equals_batch1_calls(dt):
    from hqq_amd import ops
    B, V, H, L, hd = 5, 300, 256, 96, 64
    g = _gen(1)
    embed = torch.randn(V, H, device="cuda", generator=g).to(dt)
    cos_tab = torch.randn(L, hd, device="cuda", generator=g).to(dt)
    sin_tab = torch.randn(L, hd, device="cuda", generator=g).to(dt)
    tok = torch.tensor([[3], [299], [0], [150], [3]], device="cuda")
    pos = torch.tensor([0, 95, 17, 40, 63], device="cuda")
    h, cos, sin, mask = (torch.full((B, n), float("nan"), dtype=dt, device="cuda") for n in (H, hd, hd, L))
    ops.token_prologue_batched(tok, pos, embed, h, cos_tab, sin_tab, cos, sin, mask)
    for b in range(B):
        h1, c1, s1, m1 = (torch.empty(n, dtype=dt, device="cuda") for n in (H, hd, hd, L))
        ops.token_prologue(tok[b:b + 1], pos[b:b + 1], embed, h1, cos_tab, sin_tab, c1, s1, m1)
        assert torch.equal(h[b], h1) and torch.equal(cos[b], c1) and torch.equal(sin[b], s1) and torch.equal(mask[b], m1)
        assert torch.equal(h[b], embed[tok[b, 0]]) and torch.equal(cos[b], cos_tab[pos[b]])
    # without tables and mask: h alone
    h2 = torch.empty_like(h)
    ops.token_prologue_batched(tok, pos, embed, h2)
    assert torch.equal(h2, h)


@pytest.mark.parametrize("dt", DTS)
def test_rope_cache_batched_equals_batch1_calls(dt):
    from hqq_amd import ops
    B, nh, nkv, hd, L = 4, 8, 2, 128, 64
    g = _gen(2)
    q = torch.randn(B, nh * hd, device="cuda", generator=g).to(dt)
    k = torch.randn(B, nkv * hd, device="cuda", generator=g).to(dt)
    v = torch.randn(B, nkv * hd, device="cuda", generator=g).to(dt)
    cos = torch.randn(B, hd, device="cuda", generator=g).to(dt)
    sin = torch.randn(B, hd, device="cuda", generator=g).to(dt)
    pos = torch.tensor([0, 63, 64, 17], device="cuda")   # row 2: outside the cache -> writes nothing
    kc = torch.randn(B, nkv, L, hd, device="cuda", generator=g).to(dt)
    vc = torch.randn(B, nkv, L, hd, device="cuda", generator=g).to(dt)
    kc1, vc1 = kc.clone(), vc.clone()
    qr = torch.empty(B, nh, 1, hd, dtype=dt, device="cuda")
    ops.rope_cache_batched(q, k, v, cos, sin, pos, kc, vc, qr)
    for b in range(B):
        qr1 = torch.empty(1, nh, 1, hd, dtype=dt, device="cuda")
        ops.rope_cache(q[b], k[b], v[b], cos[b], sin[b], pos[b:b + 1], kc1[b], vc1[b], qr1)
        assert torch.equal(qr[b], qr1[0])
    assert torch.equal(kc, kc1) and torch.equal(vc, vc1)   # every position: the written ones and the untouched ones
    assert torch.equal(vc[1, :, 63], v[1].view(nkv, hd)) and torch.equal(vc[3, :, 17], v[3].view(nkv, hd))


def _attn_inputs(B, nh, nkv, hd, L, seed, dt):
    g = _gen(seed)
    q = torch.randn(B, nh * hd, device="cuda", generator=g).to(dt)
    k = torch.randn(B, nkv * hd, device="cuda", generator=g).to(dt)
    v = torch.randn(B, nkv * hd, device="cuda", generator=g).to(dt)
    ang = torch.rand(B, hd // 2, device="cuda", generator=g) * 6.28
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1).to(dt), torch.cat([ang.sin(), ang.sin()], -1).to(dt)
    kc = torch.randn(B, nkv, L, hd, device="cuda", generator=g).to(dt)
    vc = torch.randn(B, nkv, L, hd, device="cuda", generator=g).to(dt)
    return q, k, v, cos, sin, kc, vc


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("hd", [64, 128, 256])
@pytest.mark.parametrize("splits", [1, 8])
def test_attn_decode_batched_equals_batch1_calls(dt, hd, splits):
    from hqq_amd import ops
    B, nh, nkv, L = 4, 8, 2, 512
    pos = torch.tensor([511, 300, 257, 400], device="cuda")   # every share of 8 holds keys
    q, k, v, cos, sin, kc, vc = _attn_inputs(B, nh, nkv, hd, L, hd + splits, dt)
    for b in range(B):   # keys beyond a row's position are never read
        kc[b, :, int(pos[b]) + 1:] = float("nan")
        vc[b, :, int(pos[b]) + 1:] = float("nan")
    scaling = hd ** -0.5
    out = torch.full((B, nh * hd), float("nan"), dtype=dt, device="cuda")
    ops.attn_decode_batched(q, kc, vc, pos, out, scaling, splits=splits)
    kc2, vc2 = kc.clone(), vc.clone()
    out_r = torch.full_like(out, float("nan"))
    ops.rope_attn_decode_batched(q, k, v, cos, sin, pos, kc2, vc2, out_r, scaling, splits=splits)
    for b in range(B):
        o1 = torch.empty(nh * hd, dtype=dt, device="cuda")
        ops.attn_decode(q[b], kc[b], vc[b], pos[b:b + 1], o1, scaling, splits=splits)
        assert torch.equal(out[b], o1), b
        kc1, vc1 = kc[b].clone(), vc[b].clone()
        r1 = torch.empty_like(o1)
        ops.rope_attn_decode(q[b], k[b], v[b], cos[b], sin[b], pos[b:b + 1], kc1, vc1, r1, scaling, splits=splits)
        assert torch.equal(out_r[b], r1), b
        assert torch.equal(kc2[b].nan_to_num(7.0), kc1.nan_to_num(7.0)) and torch.equal(vc2[b].nan_to_num(7.0), vc1.nan_to_num(7.0))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rope", [False, True])
def test_attn_decode_batched_row_with_empty_shares(dt, rope):
    """a row at position 3 inside a launch of 8 splits (chosen for the other rows' long caches): 4 of its shares hold a key, 4 are empty —
    the result stays within the kernel's tolerance of fp64 softmax attention, and the other rows stay bit-identical to their batch-1 calls"""
    from hqq_amd import ops
    B, nh, nkv, hd, L, S = 3, 8, 2, 128, 1024, 8
    pos = torch.tensor([700, 3, 1023], device="cuda")
    q, k, v, cos, sin, kc, vc = _attn_inputs(B, nh, nkv, hd, L, 77, dt)
    for b in range(B):
        kc[b, :, int(pos[b]) + 1:] = float("nan")
        vc[b, :, int(pos[b]) + 1:] = float("nan")
    scaling = hd ** -0.5
    out = torch.full((B, nh * hd), float("nan"), dtype=dt, device="cuda")
    if rope:
        qr = torch.empty(B, nh, 1, hd, dtype=dt, device="cuda")
        kref, vref = kc.clone(), vc.clone()
        ops.rope_cache_batched(q, k, v, cos, sin, pos, kref, vref, qr)   # what the rotary form attends over
        ops.rope_attn_decode_batched(q, k, v, cos, sin, pos, kc, vc, out, scaling, splits=S)
        qq = qr.view(B, nh * hd)
    else:
        ops.attn_decode_batched(q, kc, vc, pos, out, scaling, splits=S)
        kref, vref, qq = kc, vc, q
    assert torch.isfinite(out).all()
    p = 3
    rep = nh // nkv
    kk = kref[1, :, :p + 1].repeat_interleave(rep, 0).double()
    vv = vref[1, :, :p + 1].repeat_interleave(rep, 0).double()
    want = torch.einsum("hj,hjd->hd", torch.softmax(torch.einsum("hd,hjd->hj", qq[1].view(nh, hd).double(), kk) * scaling, -1), vv)
    ulp = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tol = 1e-3 + 1e-3 * want.abs() + want.abs() * ulp
    assert bool(((out[1].view(nh, hd).double() - want).abs() <= tol).all())
    for b in (0, 2):
        o1 = torch.empty(nh * hd, dtype=dt, device="cuda")
        if rope:
            kc1, vc1 = kref[b].clone(), vref[b].clone()
            ops.rope_attn_decode(q[b], k[b], v[b], cos[b], sin[b], pos[b:b + 1], kc1, vc1, o1, scaling, splits=S)
        else:
            ops.attn_decode(q[b], kc[b], vc[b], pos[b:b + 1], o1, scaling, splits=S)
        assert torch.equal(out[b], o1), b


@pytest.mark.parametrize("dt", DTS)
def test_argmax_advance_batched_follows_torch_argmax_per_row(dt):
    from hqq_amd import ops
    B, V = 6, 3001
    g = _gen(9)
    logits = torch.randn(B, V, device="cuda", generator=g).to(dt)
    logits[1, 10] = logits[1, 2000] = 50.0                   # tie: the first index
    logits[2, 7] = float("nan"); logits[2, 5] = 60.0         # a NaN is the maximum
    logits[3, 100] = logits[3, 50] = float("nan")            # the first NaN
    logits[4] = 1.0                                          # all equal: index 0
    logits[5, V - 1] = 80.0                                  # the last index
    nxt = torch.full((B, 1), -1, dtype=torch.int64, device="cuda")
    tok = torch.full((B, 1), -1, dtype=torch.int64, device="cuda")
    pos = torch.arange(B, device="cuda") * 10
    ops.argmax_advance_batched(logits, nxt, tok, pos)
    want = logits.argmax(-1)
    assert torch.equal(nxt.view(-1), want) and torch.equal(tok.view(-1), want)
    assert want[1:].tolist()[:4] == [10, 7, 50, 0] and int(want[5]) == V - 1
    assert torch.equal(pos, torch.arange(B, device="cuda") * 10 + 1)
    ops.argmax_advance_batched(logits, nxt)   # tok / pos skipped
    assert torch.equal(pos, torch.arange(B, device="cuda") * 10 + 1)


# ---- the coverage rule against the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nbits", [4, 2, 3])
def test_batch_coverage_rule_matches_the_kernels(dt, nbits):
    """llama_fused.batch_covers says yes exactly where hqq_hip_gemv_grouped (a pair of layers) and hqq_hip_gemv (each layer) run"""
    from hqq_amd import ops
    from hqq_amd.utils.llama_fused import batch_covers
    for (N, K) in [(256, 256), (512, 512)]:
        layers = []
        for i in range(2):
            W = torch.randn(N, K, device="cuda", generator=_gen(N + i)).to(dt)
            W_q, s, z = ops.quantize(W, nbits=nbits, group_size=64)
            layers.append((W_q, s.to(dt).reshape(-1), z.to(dt).reshape(-1), None, N))
        for B in (1, 2, 4, 5, 8, 16, 17, 32, 64):
            x = torch.randn(B, K, device="cuda", generator=_gen(B)).to(dt)
            covered = batch_covers(dt, B, [(N, K, 64, nbits, False)] * 2)
            ran = []
            for call in (lambda: ops.gemv_grouped(x, layers, K, 64, nbits),
                         lambda: [ops.gemv(x, L_[0], L_[1], L_[2], None, N, K, 64, nbits) for L_ in layers]):
                try:
                    call()
                    ran.append(True)
                except (NotImplementedError, RuntimeError):
                    ran.append(False)
            torch.cuda.synchronize()
            assert ran == [covered, covered], (N, K, B, covered, ran)


# ---- the step and the decoder -------------------------------------------------------------------------------------------------------------
def _tiny_llama(dt=torch.float16, **kw):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    args = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=512,
                max_position_embeddings=128)
    args.update(kw)
    return LlamaForCausalLM(LlamaConfig(**args)).to(dt).cuda().eval()


def _quantised(model, dt=torch.float16, keep_ref=False):
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=dt, device="cuda")
    ref = copy.deepcopy(model) if keep_ref else None
    prepare_for_inference(model, backend="hip")
    group_llama_projections(model)
    return (model, ref) if keep_ref else model


def _prompts(lengths, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (1, T), generator=g).cuda() for T in lengths]


def _pytorch_forward(fn):
    from hqq_amd.core.quantize import HQQBackend, HQQLinear
    HQQLinear.set_backend(HQQBackend.PYTORCH_FORWARD)
    try:
        with torch.no_grad():
            return fn()
    finally:
        HQQLinear.set_backend(HQQBackend.HIP)


def _batch_cache(model, prompts, L):
    """a B-row StaticCache whose row b holds prompt b's prefill (each prompt alone, as generate_batch does it)"""
    from transformers import StaticCache
    cfg = model.config
    B = len(prompts)
    hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    bc = StaticCache(config=cfg, max_cache_len=L)
    bc.early_initialization(B, cfg.num_key_value_heads, hd, model.model.norm.weight.dtype, torch.device("cuda"))
    for b, x in enumerate(prompts):
        c = StaticCache(config=cfg, max_cache_len=L)
        with torch.no_grad():
            model(x, past_key_values=c, cache_position=torch.arange(x.shape[1], device="cuda"), use_cache=True)
        for dst, src in zip(bc.layers, c.layers):
            dst.keys[b, :, :x.shape[1]].copy_(src.keys[0, :, :x.shape[1]])
            dst.values[b, :, :x.shape[1]].copy_(src.values[0, :, :x.shape[1]])
    return bc


def _teacher_forced(model, prompts, seqs, L, steps, attention="sdpa"):
    """the batched step's logits [steps, B, vocab] when row b is fed seqs[b]'s tokens after its prompt"""
    from hqq_amd.utils.llama_fused import FusedLlamaBatchStep
    B = len(prompts)
    bc = _batch_cache(model, prompts, L)
    step = FusedLlamaBatchStep(model, bc, L, B, attention=attention)
    T = [x.shape[1] for x in prompts]
    out = []
    for t in range(steps):
        tok = torch.stack([seqs[b][0, T[b] + t] for b in range(B)]).view(B, 1)
        pos = torch.tensor([T[b] + t for b in range(B)], device="cuda")
        out.append(step(tok, pos, L).float().clone())
    return torch.stack(out)


def test_equal_length_batch_step_against_the_models_own_forward():
    from transformers import StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaBatchStep, supports_batch
    model = _quantised(_tiny_llama())
    B, T, L = 4, 7, 64
    assert supports_batch(model, B)
    ids = torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(4)).cuda()
    cache = StaticCache(config=model.config, max_cache_len=L)
    with torch.no_grad():
        out = model(ids, past_key_values=cache, cache_position=torch.arange(T, device="cuda"), use_cache=True)
    ref_cache = copy.deepcopy(cache)
    tok = out.logits[:, -1].argmax(-1, keepdim=True)
    ref_tok = tok.clone()
    step = FusedLlamaBatchStep(model, cache, L, B)
    bitwise = True
    for t in range(16):
        pos = torch.full((B,), T + t, device="cuda")
        got = step(tok, pos)
        with torch.no_grad():
            want = model(ref_tok, past_key_values=ref_cache, cache_position=torch.tensor([T + t], device="cuda"), use_cache=True).logits[:, -1]
        torch.testing.assert_close(got.float(), want.float(), rtol=5e-3, atol=5e-3)
        bitwise = bitwise and torch.equal(got, want)
        tok, ref_tok = got.argmax(-1, keepdim=True), want.argmax(-1, keepdim=True)
        assert torch.equal(tok, ref_tok), t
    print(f"batched step vs model(...) logits bitwise equal over 16 steps: {bitwise}")


@pytest.mark.parametrize("attention", ["sdpa", "hip"])
def test_ragged_prompts_decode_the_tokens_of_batch1_decoding(attention):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, ref = _quantised(_tiny_llama(), keep_ref=True)
    prompts = _prompts([3, 9, 5, 12], 512, 21)
    n, L = 24, 64
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention=attention)
    got = dec.generate_batch(prompts, n)
    assert dec._batch.get(4) is not None and dec.batch_graphs, "the batched step served the batch"
    one = GraphedGreedyDecoder(model, max_cache_len=L, attention=attention)
    for b, x in enumerate(prompts):
        assert got[b].shape == (1, x.shape[1] + n)
        assert torch.equal(got[b], one.generate(x, n)), b
        if attention == "sdpa":
            want = _pytorch_forward(lambda: ref.generate(x, max_new_tokens=n, do_sample=False, pad_token_id=0))
            assert torch.equal(got[b], want), (b, got[b].tolist(), want.tolist())
    # teacher-forced: the batched step's logits on the generated tokens against the batch-1 forward (reference arithmetic for "sdpa";
    # for "hip", the fused model's own forward, as the batch-1 kernel-attention test compares)
    lg = _teacher_forced(model, prompts, got, L, 12, attention=attention)
    for b, x in enumerate(prompts):
        T = x.shape[1]
        if attention == "sdpa":
            want = _pytorch_forward(lambda: ref(got[b][:, :T + 12]).logits[0, T - 1 + 1:T + 12].float())
        else:
            with torch.no_grad():
                want = model(got[b][:, :T + 12]).logits[0, T:T + 12].float()
        torch.testing.assert_close(lg[:, b], want, rtol=5e-3, atol=5e-3)


def test_a_rows_logits_do_not_depend_on_the_other_rows():
    model = _quantised(_tiny_llama())
    L = 64
    first = _prompts([6], 512, 1)[0]
    a = [first] + _prompts([4, 11, 7], 512, 2)
    b = [first] + _prompts([9, 3, 12], 512, 3)
    seq = [torch.randint(0, 512, (1, 40), generator=torch.Generator().manual_seed(s)).cuda() for s in range(4)]
    seq[0][:, :6] = first
    la = _teacher_forced(model, a, [seq[0]] + [torch.cat([x, seq[i][:, :30]], 1) for i, x in enumerate(a[1:], 1)], L, 16)
    lb = _teacher_forced(model, b, [seq[0]] + [torch.cat([x, seq[i][:, :30]], 1) for i, x in enumerate(b[1:], 1)], L, 16)
    assert torch.equal(la[:, 0], lb[:, 0])


def test_graphs_are_kept_and_follow_the_model():
    from hqq_amd.backends.hip import HQQLinearHIP
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = _quantised(_tiny_llama())
    prompts = _prompts([3, 9, 5], 512, 5)
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    eager = GraphedGreedyDecoder(model, max_cache_len=64).generate_batch(prompts, 20, use_graph=False)
    got = dec.generate_batch(prompts, 20, use_graph=True)
    assert all(torch.equal(x, y) for x, y in zip(got, eager))
    graphs = dict(dec.batch_graphs)
    state = dec._batch[3]
    assert graphs and all(k[0] == 3 for k in graphs)
    again = dec.generate_batch(_prompts([4, 8, 6], 512, 6), 20)   # the same buckets: replayed, nothing captured
    assert dec._batch[3] is state and dec.batch_graphs.keys() == graphs.keys() and all(dec.batch_graphs[k] is g for k, g in graphs.items())
    assert [x.shape[1] for x in again] == [24, 28, 26]
    lay = next(m for m in model.modules() if isinstance(m, HQQLinearHIP))
    with torch.no_grad():
        lay.W_q.add_(0)   # a new version of one layer's packed tensor: the kept state is rebuilt
    dec.generate_batch(prompts, 4)
    assert dec._batch[3] is not state and all(dec.batch_graphs.get(k) is not g for k, g in graphs.items())
    dec.reset()
    assert dec._batch == {} and dec.batch_graphs == {}


def test_each_row_stops_at_its_own_eos():
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = _quantised(_tiny_llama())
    prompts = _prompts([3, 9, 5, 12], 512, 21)
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    full = dec.generate_batch(prompts, 24)
    T1 = prompts[1].shape[1]
    eos = int(full[1][0, T1 + 10])
    cut = [eos in r[0, x.shape[1]:].tolist() for r, x in zip(full, prompts)]
    got = dec.generate_batch(prompts, 24, eos_token_id=eos, check_every=4)
    for b, (x, r) in enumerate(zip(prompts, full)):
        new = r[0, x.shape[1]:].tolist()
        n = new.index(eos) + 1 if cut[b] else 24
        assert torch.equal(got[b], r[:, :x.shape[1] + n]), b
    assert int(got[1][0, -1]) == eos and got[1].shape[1] <= T1 + 11
    assert any(not c for c in cut), "some row runs to full length"


@pytest.mark.parametrize("which", ["bf16", "gqa128"])
def test_batched_decoding_on_other_models(which):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    if which == "bf16":
        model = _quantised(_tiny_llama(torch.bfloat16, num_key_value_heads=2), dt=torch.bfloat16)
        prompts = _prompts([4, 10, 7], 512, 8)
    else:
        model = _quantised(_tiny_llama(hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=1, vocab_size=1024,
                                       max_position_embeddings=256, rope_theta=500000.0))
        prompts = _prompts([9, 3, 12, 6], 1024, 9)
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    got = dec.generate_batch(prompts, 20)
    assert dec._batch.get(len(prompts)) is not None
    one = GraphedGreedyDecoder(model, max_cache_len=64)
    for b, x in enumerate(prompts):
        assert torch.equal(got[b], one.generate(x, 20)), b


def test_uncovered_batches_decode_one_prompt_after_another():
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.llama_fused import supports_batch
    model = _quantised(_tiny_llama())
    assert not supports_batch(model, 17) and supports_batch(model, 16)
    prompts = _prompts([3 + i % 5 for i in range(17)], 512, 10)
    dec = GraphedGreedyDecoder(model, max_cache_len=32)
    got = dec.generate_batch(prompts, 6)
    assert 17 not in dec._batch and not dec.batch_graphs
    one = GraphedGreedyDecoder(model, max_cache_len=32)
    assert all(torch.equal(g, one.generate(x, 6)) for g, x in zip(got, prompts))


def test_sampling_in_the_batched_step():
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model = _quantised(_tiny_llama())
    prompts = _prompts([5, 10, 7], 512, 12)
    torch.manual_seed(123)
    a = GraphedGreedyDecoder(model, max_cache_len=64, do_sample=True, temperature=0.6, top_k=5).generate_batch(prompts, 16)
    torch.manual_seed(123)
    b = GraphedGreedyDecoder(model, max_cache_len=64, do_sample=True, temperature=0.6, top_k=5).generate_batch(prompts, 16)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    inside, total = 0, 0
    for x, r in zip(prompts, a):
        with torch.no_grad():
            top5 = model(r[:, :-1]).logits[0].float().topk(5, dim=-1).indices
        T = x.shape[1]
        for t in range(T - 1, r.shape[1] - 1):
            inside += int(r[0, t + 1]) in top5[t].tolist()
            total += 1
    assert inside >= total - 1, (inside, total)   # (a near-tie at rank 5 / 6 may swap between the step's and the forward's last bits)


def test_hfgenerator_generate_batch():
    from hqq_amd.utils.generation import HFGenerator
    from test_model_gpu import _ToyTokenizer
    model = _quantised(_tiny_llama())
    tok = _ToyTokenizer()
    gen = HFGenerator(model, tok, max_new_tokens=16, compile="partial")
    prompts = ["7 8 9 10 11", "400 3 77", "5 6 7 8 9 10 11 12 13 14"]
    got = gen.generate_batch(prompts, use_chat_template=False, verbose=False)
    assert len(got) == 3 and gen.decoder._batch.get(3) is not None
    for p, r in zip(prompts, got):
        want = gen.generate(p, use_chat_template=False, verbose=False)
        assert set(r) == set(want) == {"output_text", "output_tokens", "input_tokens"}
        assert all(torch.equal(r[k], want[k]) for k in ("output_tokens", "input_tokens")) and r["output_text"] == want["output_text"]
