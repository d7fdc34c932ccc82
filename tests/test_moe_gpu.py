"""GPU half of the mixture-of-experts tests: the routed expert kernels (csrc/moe.hip, hqq_amd.ops.moe_*) and HQQExperts (hqq_amd/core/moe.py) against the
host model and the derived bound of tests/_moe_cases.py, the properties that hold exactly, the two routes, graph capture, and a tiny Mixtral end to end."""
import pytest

torch = pytest.importorskip("torch")

import _moe_cases as C   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    """cid -> (data on the host, HQQExperts on the GPU): built once, never modified (tests that edit a stack clone it)"""
    cache = {}

    def get(cid):
        if cid not in cache:
            data = C.build(C.BY_ID[cid])
            cache[cid] = (data, C.experts(data, device="cuda"))
        return cache[cid]
    return get


def _args(q):
    g = q.layer_meta["gate"]
    return (q.num_experts, q.hidden_dim, q.intermediate_dim, g["group_size"], g["nbits"])


def _stack(q, role):
    return tuple(getattr(q, f"{role}_{k}") for k in ("W_q", "scale", "zero"))


def _dev(data):
    return data["x"].cuda(), data["idx"].cuda(), data["w"].cuda()


def _gate_up(q, x, idx, a=None):
    from hqq_amd import ops
    return ops.moe_gate_up(x, idx, _stack(q, "gate"), _stack(q, "up"), *_args(q), a=a)


def _down(q, a, idx, w):
    from hqq_amd import ops
    return ops.moe_down(a, idx, w, _stack(q, "down"), *_args(q))


# ---- 1. closed-form cases: the model's bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.CLOSED])
def test_closed_form_cases_are_bit_exact(built, cid):
    from hqq_amd.core.moe import HQQExperts
    data, q = built(cid)
    x, idx, w = _dev(data)
    a_want, out_want = C.model(data)
    a = _gate_up(q, x, idx)
    assert a.shape == a_want.shape and torch.equal(a.cpu(), a_want)
    out = _down(q, a_want.cuda(), idx, w)
    assert torch.equal(out.cpu(), out_want)
    assert HQQExperts.fused is None
    assert torch.equal(q(x, idx, w).cpu(), out_want)
    assert torch.equal(q.forward_fused(x, idx, w).cpu(), out_want)
    for e in range(data["case"].E):   # the stacks are what the dequantise kernel reads, too
        assert torch.equal(q.dequantize(e, "down").cpu(), data["down"]["W"][e])


# ---- 2. random cases: within the derived bound of the fp64 model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.RANDOM])
def test_random_cases_stay_inside_the_derived_bound(built, cid):
    data, q = built(cid)
    x, idx, w = _dev(data)
    a = _gate_up(q, x, idx).cpu()
    a_want = C.model_a(data)
    err_a = (a.double() - a_want.double()).abs()
    Da = C.bound_a(data)
    print(cid, "a: max err / bound", float((err_a / Da).max()))
    assert bool((err_a <= Da).all())
    out = _down(q, a.cuda(), idx, w).cpu()                      # from the kernel's own a
    err = (out.double() - C.model_down(data, a).double()).abs()
    D = C.bound_out(data, a)
    print(cid, "out: max err / bound", float((err / D).max()))
    assert bool((err <= D).all())


# ---- 3. properties that hold exactly -----------------------------------------------------------------------------------------------------------------------------
PROP = [c.id for c in C.RANDOM if c.T == 16 and c.k == 2] + [c.id for c in C.RANDOM if c.k == 8]


@pytest.mark.parametrize("cid", PROP)
def test_exact_properties(built, cid):
    from hqq_amd import ops
    from hqq_amd.core.moe import HQQExperts
    data, q = built(cid)
    c = data["case"]
    x, idx, w = _dev(data)
    out = q.forward_fused(x, idx, w)
    assert torch.equal(q.forward_fused(x, idx, w), out)                                     # two calls, the same bits
    for t in (0, c.T // 2, c.T - 1):                                                          # a row of the batch has the bits of the one-row call
        assert torch.equal(q.forward_fused(x[t:t + 1].contiguous(), idx[t:t + 1].contiguous(), w[t:t + 1].contiguous())[0], out[t]), t
    flip = torch.arange(c.k - 1, -1, -1, device="cuda")                                       # the slots' columns permuted together: nothing changes
    assert torch.equal(q.forward_fused(x, idx[:, flip].contiguous(), w[:, flip].contiguous()), out)
    # only the selected experts are read: NaN scales in every expert the first token does not select
    if c.k < c.E:
        hit = torch.zeros(c.E, dtype=torch.bool)
        hit[data["idx"][0]] = True
        st, meta = C.stacks(data)
        for role in C.ROLES:
            st[role, "scale"][~hit] = float("nan")
        poisoned = HQQExperts.from_stacks(st, meta, C.quant_config(c), compute_dtype=c.dt, device="cuda")
        assert bool(torch.isnan(poisoned.gate_scale).any()) and bool(torch.isnan(poisoned.down_scale).any())
        assert torch.equal(poisoned.forward_fused(x[:1].contiguous(), idx[:1].contiguous(), w[:1].contiguous())[0], out[0])
    # all tokens on the same two experts
    k2 = min(c.k, 2)
    same_idx = torch.tensor([[c.E - 1, 1][:k2]] * c.T, device="cuda")
    same_w = w[:, :k2].contiguous()
    got = q.forward_fused(x, same_idx, same_w).cpu()
    d2 = dict(data, idx=same_idx.cpu(), w=same_w.cpu(), case=C.Case(c.kind, c.nbits, c.gs, c.dt, c.T, k2, E=c.E))
    a = _gate_up(q, x, same_idx).cpu()
    assert bool(((a.double() - C.model_a(d2).double()).abs() <= C.bound_a(d2)).all())
    assert bool(((got.double() - C.model_down(d2, a).double()).abs() <= C.bound_out(d2, a)).all())
    # a caller-owned buffer is used as given, and nothing else is needed
    buf = torch.empty((c.T, c.k, c.I), dtype=c.dt, device="cuda")
    assert _gate_up(q, x, idx, a=buf).data_ptr() == buf.data_ptr()
    assert torch.equal(ops.moe_forward(x, idx, w, _stack(q, "gate"), _stack(q, "up"), _stack(q, "down"), *_args(q), a=buf), out)


# ---- 4. the two routes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.RANDOM if c.T == 3 and c.k == 2])
def test_fused_and_composed_routes_agree(built, cid):
    data, q = built(cid)
    x, idx, w = _dev(data)
    a_want, out_want = C.model(data)
    D = C.bound_out(data, a_want, C.bound_a(data))
    fused, composed = q.forward_fused(x, idx, w).cpu().double(), q.forward_composed(x, idx, w).cpu().double()
    print(cid, "fused / composed against the model, max err / bound", float(((fused - out_want.double()).abs() / D).max()),
          float(((composed - out_want.double()).abs() / D).max()))
    assert bool(((fused - out_want.double()).abs() <= D).all()) and bool(((composed - out_want.double()).abs() <= D).all())
    assert bool(((fused - composed).abs() <= 2 * D).all())


def _tiny_experts(dtype=torch.float16, seed=0):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts
    cfg = MixtralConfig(vocab_size=64, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=4, num_experts_per_tok=2, max_position_embeddings=128)
    m = MixtralExperts(cfg)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.gate_up_proj.copy_(torch.randn(m.gate_up_proj.shape, generator=g) * 0.05)
        m.down_proj.copy_(torch.randn(m.down_proj.shape, generator=g) * 0.05)
    return m.to(dtype).cuda()


def test_route_selection(built, monkeypatch):
    from hqq_amd import ops
    from hqq_amd.core.moe import HQQExperts
    from hqq_amd.core.quantize import BaseQuantizeConfig
    calls = []
    real = ops.moe_forward
    monkeypatch.setattr(ops, "moe_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = torch.Generator().manual_seed(9)
    x17 = (torch.randn((17, 128), generator=g) * 0.5).half().cuda()
    idx17 = torch.stack([torch.randperm(4, generator=g)[:2] for _ in range(17)]).cuda()
    w17 = torch.rand((17, 2), generator=g).cuda()
    q8 = HQQExperts(_tiny_experts(), BaseQuantizeConfig(nbits=8, group_size=64, axis=1), compute_dtype=torch.float16, device="cuda")
    q4 = HQQExperts(_tiny_experts(), BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=torch.float16, device="cuda")
    assert torch.equal(q8(x17[:3], idx17[:3], w17[:3]), q8.forward_composed(x17[:3], idx17[:3], w17[:3])) and not calls        # 8-bit composes
    assert torch.equal(q4(x17, idx17, w17), q4.forward_composed(x17, idx17, w17)) and not calls                                # 17 tokens compose
    assert ops.MOE_ROUTE_MAX_T >= 3
    assert torch.equal(q4(x17[:3], idx17[:3], w17[:3]), q4.forward_fused(x17[:3], idx17[:3], w17[:3])) and len(calls) == 2     # 3 tokens go fused
    over = ops.MOE_ROUTE_MAX_T + 1                                                                                              # past the measured cut-off: composed
    if over <= ops.MOE_MAX_T:
        n = len(calls)
        assert torch.equal(q4(x17[:over], idx17[:over], w17[:over]), q4.forward_composed(x17[:over], idx17[:over], w17[:over])) and len(calls) == n
        monkeypatch.setattr(HQQExperts, "fused", True)
        assert torch.equal(q4(x17[:over], idx17[:over], w17[:over]), q4.forward_fused(x17[:over], idx17[:over], w17[:over])) and len(calls) == n + 2
    monkeypatch.setattr(HQQExperts, "fused", True)
    for q, rows in ((q8, 3), (q4, 17)):
        with pytest.raises(NotImplementedError, match="outside"):
            q(x17[:rows], idx17[:rows], w17[:rows])
    monkeypatch.setattr(HQQExperts, "fused", False)
    n = len(calls)
    q4(x17[:3], idx17[:3], w17[:3])
    assert len(calls) == n


@pytest.mark.parametrize("nbits,gs", C.CONFIGS)
def test_every_expert_is_what_hqqlinear_makes_of_its_slice(nbits, gs):
    """the identity of tests/test_moe_cpu.py with the real quantiser"""
    from hqq_amd.core.moe import HQQExperts
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    dense = _tiny_experts(torch.float32)
    cfg = BaseQuantizeConfig(nbits=nbits, group_size=gs, axis=1)
    q = HQQExperts(dense, cfg, compute_dtype=torch.float16, device="cuda", del_orig=False)
    for e in range(4):
        slices = {"gate": dense.gate_up_proj.data[e, :192], "up": dense.gate_up_proj.data[e, 192:], "down": dense.down_proj.data[e]}
        for role in C.ROLES:
            ref = HQQLinear.from_weights(slices[role].clone(), None, cfg, compute_dtype=torch.float16, device="cuda")
            assert torch.equal(getattr(q, role + "_W_q")[e], ref.W_q.data), (e, role)
            assert torch.equal(getattr(q, role + "_scale")[e], ref.meta["scale"]) and torch.equal(getattr(q, role + "_zero")[e], ref.meta["zero"]), (e, role)
            view = q.expert_linear(e, role)
            assert torch.equal(view.dequantize(), ref.dequantize())
            x = torch.randn(2, view.in_features, device="cuda").half()
            assert torch.equal(view(x), ref(x))


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------------------------------------------------
def test_forward_is_captured_and_replayed_on_another_routing(built):
    cid = next(c.id for c in C.RANDOM if c.T == 3 and c.k == 2 and c.nbits == 4 and c.dt == torch.float16)
    data, q = built(cid)
    x, idx, w = (t[:2].contiguous().clone() for t in _dev(data))
    x2, idx2, w2 = (x.flip(0) * 0.5).contiguous(), torch.tensor([[2, 3], [3, 1]], device="cuda"), torch.tensor([[0.25, 0.75], [0.6, 0.4]], device="cuda")
    assert not torch.equal(idx, idx2)
    want2 = q(x2, idx2, w2)
    want1 = q(x, idx, w)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q(x, idx, w)                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = q(x, idx, w)
    graph.replay()
    assert torch.equal(out, want1)
    x.copy_(x2), idx.copy_(idx2), w.copy_(w2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2) and not torch.equal(want1, want2)


# ---- 6. model level --------------------------------------------------------------------------------------------------------------------------------------------------
def test_tiny_mixtral_decodes_the_same_tokens_with_and_without_graphs():
    from transformers import MixtralConfig, MixtralForCausalLM
    from hqq_amd.core.moe import HQQExperts
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    torch.manual_seed(0)
    cfg = MixtralConfig(vocab_size=64, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=4, num_experts_per_tok=2, max_position_embeddings=128)
    model = MixtralForCausalLM(cfg).half().cuda().eval()
    qc = BaseQuantizeConfig(nbits=4, group_size=64, axis=1)
    quantize_model(model, qc, compute_dtype=torch.float16, device="cuda", expert_config=qc)
    prepare_for_inference(model, backend="hip")
    experts = [m for m in model.modules() if isinstance(m, HQQExperts)]
    assert len(experts) == 2
    ids = torch.randint(0, 64, (1, 6), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    dec = GraphedGreedyDecoder(model, max_cache_len=64)
    assert not dec.fused                                           # the model's own forward: MoE blocks have no fused step
    eager = dec.generate(ids, 8, use_graph=False)
    graphed = GraphedGreedyDecoder(model, max_cache_len=64).generate(ids, 8, use_graph=True)
    assert eager.shape[-1] == ids.shape[-1] + 8 and torch.equal(eager, graphed)
