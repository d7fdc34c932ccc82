"""The grouped axis-0 decode launch (hqq_hip_gemv_axis0_grouped) and the opt-in fused decode step for axis-0 models, on the GPU.  The yardstick of
the launch is ops.gemv_axis0 per layer (pinned to the oracle and to the dequantise kernel in test_axis0_decode_gpu.py): every output must be the
same bits.  The steps are held to the tokens of the model's own forward, which test_axis0_decode_gpu.py holds to the reference's arithmetic."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COMBOS = [(8, torch.float16), (4, torch.float16), (2, torch.float16), (1, torch.float16), (4, torch.bfloat16), (2, torch.bfloat16)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from hqq_amd import ops as o
    assert o.is_available(), "libhqq_hip.so must load on the GPU box (no fallback)"
    return o


def _random_layer(oracle, N, K, gs, nbits, dt, seed, bias):
    """test_axis0_decode_gpu.py's layer: random levels in the axis-0 view [gs, N K / gs], packed by the oracle; scale / zero per column"""
    g = torch.Generator().manual_seed(seed)
    C = N * K // gs
    U = torch.randint(0, 2 ** nbits, (gs, C), generator=g, dtype=torch.uint8).numpy()
    s = (torch.rand(C, generator=g) * 0.004 + 0.001).to(dt)
    z = (torch.rand(C, generator=g) * (2 ** nbits - 1)).to(dt)
    if dt == torch.bfloat16:
        z[::5] = 0.00836
        z[1::11] = 2.0 ** -12
    b = torch.randn(N, generator=g).to(dt).cuda() if bias else None
    P = torch.from_numpy(np.ascontiguousarray(oracle.pack(nbits, U))).cuda()
    return (P, s.reshape(1, -1).cuda(), z.reshape(1, -1).cuda(), b, N)


def _group(oracle, Ns, K, gs, nbits, dt, seed, bias):
    return [_random_layer(oracle, N, K, N if gs is None else gs, nbits, dt, seed + 17 * i, bias) for i, N in enumerate(Ns)]


def _check_bit_equal(ops, oracle, nbits, dt, Ns, K, gs, M, bias, seed):
    layers = _group(oracle, Ns, K, gs, nbits, dt, seed, bias)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed + 1)).to(dt).cuda()
    outs = ops.gemv_axis0_grouped(x, layers, K, gs, nbits)
    assert len(outs) == len(Ns)
    for (P, s, z, b, N), y in zip(layers, outs):
        want = ops.gemv_axis0(x, P, s, z, b, N, K, gs, nbits)
        assert y.dtype == dt and tuple(y.shape) == (M, N)
        assert torch.equal(y, want), (N, int((y != want).sum()))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("Ns", [(256,), (256, 256), (512, 128, 128)])
@pytest.mark.parametrize("M", [1, 2, 5, 16])
@pytest.mark.parametrize("gs", [16, 64, 128, None])
@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_grouped_equals_per_layer_calls(ops, oracle, nbits, dt, gs, M, Ns, bias):
    if gs is None and len(set(Ns)) != 1:
        # group_size None is one group per column, i.e. group_size = N: members of different N have different group sizes, and one call shares one
        # group_size (include/hqq_hip.h).  Such a group is refused on the host, by the predicate and by the wrapper, and nothing is launched
        assert not ops.axis0_grouped_covers(dt, M, Ns, 1024, None, nbits)
        layers = _group(oracle, Ns, 1024, None, nbits, dt, 1, bias)
        with pytest.raises(ValueError, match="equal N"):
            ops.gemv_axis0_grouped(torch.zeros(M, 1024, dtype=dt, device="cuda"), layers, 1024, None, nbits)
        return
    _check_bit_equal(ops, oracle, nbits, dt, Ns, 1024, gs, M, bias, seed=nbits * 100 + (gs or 7) + M)


@pytest.mark.parametrize("Ns,K", [((4096, 4096, 4096), 4096), ((11008, 11008), 4096), ((8192, 1024, 1024), 8192)])
@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_grouped_llama_groups_equal_per_layer_calls(ops, oracle, nbits, dt, Ns, K):
    """the 7B q|k|v and gate|up groups and the 70B GQA group (unequal N, unequal K splits per member), at 1, 2, 5 and 16 rows, with and without
    biases (the layers are packed once per case)"""
    full = _group(oracle, Ns, K, 64, nbits, dt, sum(Ns) + K + nbits, True)
    for bias in (False, True):
        layers = full if bias else [(P, s, z, None, N) for (P, s, z, _, N) in full]
        for M in (1, 2, 5, 16):
            x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(dt).cuda()
            outs = ops.gemv_axis0_grouped(x, layers, K, 64, nbits)
            for (P, s, z, b, N), y in zip(layers, outs):
                want = ops.gemv_axis0(x, P, s, z, b, N, K, 64, nbits)
                assert torch.equal(y, want), (N, M, bias, int((y != want).sum()))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,N,K,gs", [(1, 512, 1024, 64), (5, 256, 1024, None), (16, 2816, 2048, 64), (1, 11008, 4096, 64)])
@pytest.mark.parametrize("nbits,dt", COMBOS)
def test_silu_flag_equals_silu_mul_of_the_two_outputs(ops, oracle, nbits, dt, M, N, K, gs, bias):
    layers = _group(oracle, (N, N), K, gs, nbits, dt, seed=31 + nbits + M, bias=bias)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).to(dt).cuda()
    (a,) = ops.gemv_axis0_grouped(x, layers, K, gs, nbits, flags=ops.BLOCK_SILU)
    gate, up = (ops.gemv_axis0(x, P, s, z, b, N, K, gs, nbits) for (P, s, z, b, N) in layers)
    want = ops.silu_mul(gate, up)
    assert a.dtype == dt and tuple(a.shape) == (M, N)
    assert torch.equal(a, want), int((a != want).sum())
    # and a caller's output buffer is the one written
    out = torch.zeros(M, N, dtype=dt, device="cuda")
    ops.gemv_axis0_grouped(x, layers, K, gs, nbits, outs=[out], flags=ops.BLOCK_SILU)
    assert torch.equal(out, want)


def test_wrapper_refuses_what_the_kernel_does_not_cover(ops, oracle):
    layers = _group(oracle, (256, 256, 256), 1024, 64, 4, torch.float16, 1, False)
    x = torch.randn(1, 1024, device="cuda", dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="HQQ_BLOCK_SILU"):
        ops.gemv_axis0_grouped(x, layers, 1024, 64, 4, outs=[torch.empty(1, 256, device="cuda", dtype=torch.float16)], flags=ops.BLOCK_SILU)
    with pytest.raises(NotImplementedError, match="flags"):
        ops.gemv_axis0_grouped(x, layers, 1024, 64, 4, flags=ops.BLOCK_NORM)
    with pytest.raises(NotImplementedError, match="not covered"):
        ops.gemv_axis0_grouped(torch.randn(17, 1024, device="cuda", dtype=torch.float16), layers, 1024, 64, 4)


def test_deterministic_batch_independent_and_graph_capturable(ops, oracle):
    Ns, K, gs, nbits = (4096, 1024, 1024), 4096, 64, 4
    layers = _group(oracle, Ns, K, gs, nbits, torch.float16, seed=5, bias=True)
    x = torch.randn(16, K, device="cuda", dtype=torch.float16)
    y1 = ops.gemv_axis0_grouped(x, layers, K, gs, nbits)
    y2 = ops.gemv_axis0_grouped(x, layers, K, gs, nbits)
    assert all(torch.equal(a, b) for a, b in zip(y1, y2))
    # rows are independent of the batch they come in (each member's K split is a function of its shape)
    for a, b in zip(ops.gemv_axis0_grouped(x[3:4], layers, K, gs, nbits), y1):
        assert torch.equal(a, b[3:4])
    gu = layers[1:]
    s1 = ops.gemv_axis0_grouped(x, gu, K, gs, nbits, flags=ops.BLOCK_SILU)[0]
    assert torch.equal(ops.gemv_axis0_grouped(x, gu, K, gs, nbits, flags=ops.BLOCK_SILU)[0], s1)
    assert torch.equal(ops.gemv_axis0_grouped(x[7:9], gu, K, gs, nbits, flags=ops.BLOCK_SILU)[0], s1[7:9])
    # inside torch.cuda.graph capture, with the workspace reserved by the eager calls above
    xs = x[:2].clone()
    outs = [torch.empty(2, N, device="cuda", dtype=torch.float16) for N in Ns]
    act = torch.empty(2, Ns[1], device="cuda", dtype=torch.float16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gemv_axis0_grouped(xs, layers, K, gs, nbits, outs=outs)
        ops.gemv_axis0_grouped(xs, gu, K, gs, nbits, outs=[act], flags=ops.BLOCK_SILU)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemv_axis0_grouped(xs, layers, K, gs, nbits, outs=outs)
        ops.gemv_axis0_grouped(xs, gu, K, gs, nbits, outs=[act], flags=ops.BLOCK_SILU)
    xs.copy_(x[5:7])
    for o in outs + [act]:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for o, want in zip(outs, y1):
        assert torch.equal(o, want[5:7])
    assert torch.equal(act, s1[5:7])


# ---- the fused steps on a tiny Llama quantised along axis 0 (test_axis0_decode_gpu.py's model and seeds) -----------------------------------------
def _tiny_llama(dt):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=128)
    return LlamaForCausalLM(cfg).to(dt).cuda().eval()


def _quantised(nbits, dt, with_reference_tokens=False):
    from hqq_amd.backends.hip import HQQLinearHIP
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQBackend, HQQLinear
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    model = _tiny_llama(dt)
    quantize_model(model, BaseQuantizeConfig(nbits=nbits, group_size=64, axis=0), compute_dtype=dt, device="cuda")
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(1)).cuda()
    want = None
    if with_reference_tokens:
        HQQLinear.set_backend(HQQBackend.PYTORCH_FORWARD)
        try:
            with torch.no_grad():
                want = model.generate(ids[:1, :5], max_new_tokens=8, min_new_tokens=8, do_sample=False)
        finally:
            HQQLinear.set_backend(HQQBackend.HIP)
    prepare_for_inference(model, backend="hip")
    lins = [m for m in model.modules() if isinstance(m, HQQLinearHIP)]
    assert len(lins) == 14 and all(m.axis == 0 for m in lins)
    return model, ids, want


CASES = [(4, torch.float16), (2, torch.float16), (4, torch.bfloat16)]


@pytest.mark.parametrize("nbits,dt", CASES)
def test_tiny_llama_axis0_fused_single_sequence(nbits, dt):
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, ids, want = _quantised(nbits, dt, with_reference_tokens=True)
    assert llama_fused.supports_axis0(model) and not llama_fused.supports(model)
    dec = GraphedGreedyDecoder(model, max_cache_len=64, axis0="fused")
    assert dec.fused_axis0 and not dec.fused
    got = dec.generate(ids[:1, :5], 8, use_graph=False)
    print("reference tokens", want[0].tolist(), "fused", got[0].tolist())
    assert torch.equal(got, want)                  # the PYTORCH_FORWARD model.generate tokens: the bar of the unfused route
    assert dec.step is not None and dec.step.axis0 and not dec.step.folded and dec.step.one_launch_front
    base = GraphedGreedyDecoder(model, max_cache_len=64)
    assert not base.fused_axis0 and not base.fused   # without the keyword: today's behaviour
    ref = base.generate(ids[:1, :5], 24, use_graph=False)
    assert base.step is None
    for attention in ("sdpa", "hip"):              # head_dim 64: the decode-attention kernel covers it
        for use_graph in (False, True):
            d = GraphedGreedyDecoder(model, max_cache_len=64, axis0="fused", attention=attention)
            out = d.generate(ids[:1, :5], 24, use_graph=use_graph)
            print(attention, use_graph, out[0, 5:].tolist())
            assert d.step is not None and d.step.axis0
            assert torch.equal(out, ref), (attention, use_graph)
            if use_graph:
                assert d.graphs
                kept = d.step
                assert torch.equal(d.generate(ids[:1, :5], 24, use_graph=True), ref)   # the kept step and graphs serve the next prompt
                assert d.step is kept
                d.reset()
                assert d.step is None and not d.graphs
                assert torch.equal(d.generate(ids[1:, :7], 12), base.generate(ids[1:, :7], 12, use_graph=False))


@pytest.mark.parametrize("nbits,dt", CASES)
def test_tiny_llama_axis0_fused_batch(nbits, dt):
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, ids, _ = _quantised(nbits, dt)
    assert llama_fused.supports_axis0_batch(model, 3) and llama_fused.supports_axis0_batch(model, 16)
    assert not llama_fused.supports_axis0_batch(model, 17) and not llama_fused.supports_batch(model, 3)
    prompts = [ids[0, :5], ids[1, :9], ids[0, 2:5]]
    dec = GraphedGreedyDecoder(model, max_cache_len=64, axis0="fused")
    single = [dec.generate(p.view(1, -1), 12) for p in prompts]
    for attention in ("sdpa", "hip"):
        d = GraphedGreedyDecoder(model, max_cache_len=64, axis0="fused", attention=attention)
        one = single if attention == "sdpa" else [d.generate(p.view(1, -1), 12) for p in prompts]
        outs = d.generate_batch(prompts, 12)
        assert 3 in d._batch and d._batch[3]["step"].axis0 and d.batch_graphs
        for b in range(3):
            print(attention, b, outs[b][0].tolist())
            assert torch.equal(outs[b], one[b]), (attention, b)
    # EOS: a row ends with its first EOS token, the others run on
    row = single[1][0, 9:].tolist()
    eos = row[3]
    outs = dec.generate_batch(prompts, 12, eos_token_id=eos)
    for b in range(3):
        new = single[b][0, prompts[b].numel():].tolist()
        keep = new.index(eos) + 1 if eos in new else len(new)
        assert outs[b][0].tolist() == single[b][0, :prompts[b].numel() + keep].tolist(), b
    assert outs[1].shape[1] == 9 + row.index(eos) + 1
    # 17 prompts: beyond the decode kernel's rows — decoded one after another, the same tokens
    many = [ids[i % 2, :4 + (i % 5)] for i in range(17)]
    outs = dec.generate_batch(many, 6)
    assert 17 not in dec._batch
    for p, o in zip(many, outs):
        assert torch.equal(o, dec.generate(p.view(1, -1), 6))


def test_launch_shape_of_one_step(monkeypatch):
    """per decoder block: 2 grouped axis-0 calls (q|k|v; gate|up with SiLU * up), 2 single-layer calls (o, down), no silu_mul"""
    from hqq_amd import ops as hops
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, ids, _ = _quantised(4, torch.float16)
    calls = {"grouped": 0, "single": 0, "silu_mul": 0, "axis1": 0}
    flags = []
    real = {n: getattr(hops, n) for n in ("gemv_axis0_grouped", "gemv_axis0", "silu_mul", "gemv", "gemv_grouped", "gemv_block")}

    def counting(name, key):
        def f(*a, **k):
            calls[key] += 1
            if name == "gemv_axis0_grouped":
                flags.append((len(a[1]), k.get("flags", 0)))
            return real[name](*a, **k)
        return f

    for name, key in (("gemv_axis0_grouped", "grouped"), ("gemv_axis0", "single"), ("silu_mul", "silu_mul"), ("gemv", "axis1"), ("gemv_grouped", "axis1"),
                      ("gemv_block", "axis1")):
        monkeypatch.setattr(hops, name, counting(name, key))
    nblocks = len(model.model.layers)
    for B in (1, 3):
        dec = GraphedGreedyDecoder(model, max_cache_len=64, axis0="fused")
        if B == 1:
            dec.generate(ids[:1, :5], 2, use_graph=False)       # prefill (the model's own forward) + one eager step
            step, args = dec.step, (dec.tok, dec.pos)
        else:
            dec.generate_batch([ids[0, :5], ids[1, :6], ids[0, :3]], 2, use_graph=False)
            st = dec._batch[3]
            step, args = st["step"], (st["tok"], st["pos"])
        for k in calls:
            calls[k] = 0
        flags.clear()
        step(*args)
        torch.cuda.synchronize()
        assert calls == {"grouped": 2 * nblocks, "single": 2 * nblocks, "silu_mul": 0, "axis1": 0}, (B, calls)
        assert flags == [(3, 0), (2, hops.BLOCK_SILU)] * nblocks


def test_default_decoder_is_unchanged():
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    model, ids, _ = _quantised(4, torch.float16)
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    assert not dec.fused_axis0 and not dec.fused and dec.axis0 == "model"
    assert not llama_fused.supports(model) and group_llama_projections(model) == 0
    dec.generate(ids[:1, :5], 4, use_graph=False)
    assert dec.step is None                                    # the model's own forward decodes
    assert dec._batch_state(3) is None
    off = GraphedGreedyDecoder(model, max_cache_len=64, axis0="fused", fused=False)
    assert not off.fused_axis0                                 # fused=False keeps its meaning
