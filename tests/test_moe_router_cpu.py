"""CPU half of the router tests (csrc/moe_router.hip, hqq_amd.ops.moe_router*) and of the two MoE step variants (hqq_amd.utils.llama_fused): the host models of
tests/_router_cases.py against HF's routers and against each other, the condition that no row of a random case is excused, the coverage contract without a
GPU, the StepVariant additions, and the architecture predicate knob by knob on tiny CPU models."""
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")

import _moe_cases as MC      # noqa: E402
import _router_cases as C    # noqa: E402

RANDOM_IDS = [c.id for c in C.RANDOM]


# ---- 1. the case set excuses nothing -----------------------------------------------------------------------------------------------------------------------------
def test_the_grid_covers_what_it_says():
    for cases in (C.RANDOM,):
        assert {c.E for c in cases} == set(C.ES) and {c.k for c in cases} == set(C.KS) and {c.H for c in cases} == set(C.HS) and {c.T for c in cases} == set(C.TS)
        for dt in C.DTYPES:
            sub = [c for c in cases if c.dt == dt]
            assert {c.renorm for c in sub} == {True, False} and {c.round_w for c in sub} == {True, False}
            assert {c.H for c in sub} == set(C.HS) and {c.T for c in sub} == set(C.TS) and {(c.E, c.k) for c in sub} == set(C.PAIRS)


@pytest.mark.parametrize("cid", RANDOM_IDS)
def test_every_row_of_every_random_case_has_a_decided_selection(cid):
    """the share of rows left out of the selection check is 0: recomputed here from x and W alone, not taken from the builder's word"""
    c = C.BY_ID[cid]
    d = C.build(c)
    l64, b = C.logits64(d["x"], d["W"]), C.logit_bound(d["x"], d["W"], c.dt)
    assert tuple(d["x"].shape) == (c.T, c.H) and tuple(d["W"].shape) == (c.E, c.H) and d["x"].dtype == c.dt and d["W"].dtype == c.dt
    ok = C.margin_ok(l64, b, c.k)
    assert ok.shape == (c.T,) and bool(ok.all())
    if c.k < c.E:   # the k-th / (k+1)-th gap itself, spelled out
        v = torch.sort(l64, dim=-1, descending=True)
        gap = v.values[:, c.k - 1] - v.values[:, c.k]
        assert bool((gap > 2.0 * torch.maximum(torch.gather(b, 1, v.indices[:, c.k - 1:c.k]), torch.gather(b, 1, v.indices[:, c.k:c.k + 1]))[:, 0]).all())


# ---- 2. the two host models, and HF's routers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", RANDOM_IDS)
def test_restatement_agrees_with_the_reference(cid):
    c = C.BY_ID[cid]
    d = C.build(c)
    idx, w, l = C.model32(d["x"], d["W"], c.k, c.renorm, c.round_w)
    l64 = C.logits64(d["x"], d["W"])
    assert torch.equal(idx, C.ref_select(l64, c.k))
    assert bool(((l.double() - l64).abs() <= C.logit_bound(d["x"], d["W"], c.dt)).all())
    w64 = C.ref_weights(l, idx, c.renorm)
    assert bool(((w.double() - w64).abs() <= C.weight_bound(l, w64, c.E, c.k, c.renorm, c.dt if c.round_w else None)).all())


@pytest.mark.parametrize("cid", [c.id for c in C.CLOSED])
def test_restatement_gives_the_closed_forms(cid):
    c = C.BY_ID[cid]
    d = C.build(c)
    idx, w, l = C.model32(d["x"], d["W"], c.k, c.renorm, c.round_w)
    assert torch.equal(idx, d["idx"]) and torch.equal(l.float(), d["logits"].float())
    if d["w"] is not None:
        assert torch.equal(w, d["w"])
    if c.kind in ("tie_all", "top_equal"):   # the tie rule: equal logits come out in ascending id
        assert bool((idx[:, 1:] > idx[:, :-1]).all())


def _hf_router(family, E, k, H, renorm):
    if family == "mixtral":
        from transformers.models.mixtral.modeling_mixtral import MixtralTopKRouter
        return MixtralTopKRouter(SimpleNamespace(num_experts_per_tok=k, num_local_experts=E, hidden_size=H))
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeTopKRouter
    return Qwen3MoeTopKRouter(SimpleNamespace(num_experts_per_tok=k, num_experts=E, hidden_size=H, norm_topk_prob=renorm))


@pytest.mark.parametrize("cid", RANDOM_IDS)
def test_reference_agrees_with_hf_routers_in_float32(cid):
    """MixtralTopKRouter (always renormalises) and Qwen3MoeTopKRouter on the CPU in float32: the same experts in the same order on every row (all rows are
    margin-checked), weights within the bound around the reference taken on the router's own logits"""
    pytest.importorskip("transformers")
    c = C.BY_ID[cid]
    d = C.build(c)
    ref_idx = C.ref_select(C.logits64(d["x"], d["W"]), c.k)
    for family in ("mixtral", "qwen3_moe"):
        if family == "mixtral" and not c.renorm:
            continue
        r = _hf_router(family, c.E, c.k, c.H, c.renorm)
        with torch.no_grad():
            r.weight.copy_(d["W"].float())
            logits, scores, idx = r(d["x"].float())
        assert torch.equal(idx, ref_idx), family
        w64 = C.ref_weights(logits, idx, c.renorm)
        assert bool(((scores.double() - w64).abs() <= C.weight_bound(logits, w64, c.E, c.k, c.renorm)).all()), family


@pytest.mark.parametrize("cid", [c.id for c in C.RANDOM if c.round_w])
def test_reference_agrees_with_qwen3_router_in_the_compute_dtype(cid):
    """round_weights is Qwen3-MoE's `.to(router_logits.dtype)`: the router run in T on the CPU, against the reference on its own (T) logits"""
    pytest.importorskip("transformers")
    c = C.BY_ID[cid]
    d = C.build(c)
    r = _hf_router("qwen3_moe", c.E, c.k, c.H, c.renorm).to(c.dt)
    with torch.no_grad():
        r.weight.copy_(d["W"])
        logits, scores, idx = r(d["x"])
    assert scores.dtype == c.dt and logits.dtype == c.dt
    assert bool(((logits.double() - C.logits64(d["x"], d["W"])).abs() <= C.logit_bound(d["x"], d["W"], c.dt)).all())
    assert torch.equal(idx, C.ref_select(C.logits64(d["x"], d["W"]), c.k))
    w64 = C.ref_weights(logits, idx, c.renorm)
    assert bool(((scores.double() - w64).abs() <= C.weight_bound(logits, w64, c.E, c.k, c.renorm, c.dt)).all())


def test_the_stated_order_on_nan_zero_and_ties():
    nan, inf = float("nan"), float("inf")
    l = torch.tensor([[1.0, nan, 3.0, nan, inf, 3.0, -0.0, 0.0],
                      [0.0, -0.0, -1.0, 0.0, -inf, -2.0, -1.0, -0.0]])
    assert C.select32(l, 8).tolist() == [[1, 3, 4, 2, 5, 0, 6, 7], [0, 1, 3, 7, 2, 6, 5, 4]]
    assert C.select32(l, 2).tolist() == [[1, 3], [0, 1]]
    w = C.softmax32(l[:1], C.select32(l[:1], 2), True, None)
    assert bool(torch.isnan(w).all())   # a row with a NaN logit has NaN weights, as torch's softmax gives
    w = C.softmax32(l[1:], C.select32(l[1:], 4), True, None)
    assert w.tolist() == [[0.25] * 4]


# ---- 3. coverage: the contract's edges, without a GPU ------------------------------------------------------------------------------------------------------------
F16, BF16, F32 = 1, 2, 0


def _covers(T, k, E, H, dt=F16):
    from hqq_amd import _C
    return bool(_C.lib().hqq_hip_moe_router_covers(T, k, E, H, dt))


def test_covers_at_every_edge_of_the_contract():
    from hqq_amd import ops
    assert (F32, F16, BF16) == (ops.F32, ops.F16, ops.BF16)
    ok = dict(T=1, k=2, E=8, H=4096)
    assert _covers(**ok) and _covers(**ok, dt=BF16) and not _covers(**ok, dt=F32) and not _covers(**ok, dt=3)
    for T, want in ((0, False), (1, True), (16, True), (17, False)):
        assert _covers(**{**ok, "T": T}) == want
    assert ops.MOE_MAX_T == 16
    for k, want in ((0, False), (1, True), (8, True), (9, False)):
        assert _covers(**{**ok, "k": k, "E": 16}) == want
    for E, want in ((1, False), (2, True), (256, True), (257, False)):   # k <= E <= 256
        assert _covers(**{**ok, "E": E}) == want
    assert _covers(1, 1, 1, 8) and _covers(16, 8, 8, 65536) and _covers(16, 8, 256, 65536)
    for H, want in ((0, False), (8, True), (12, False), (136, True), (65536, True), (65544, False)):
        assert _covers(**{**ok, "H": H}) == want
    assert ops.moe_router_covers(torch.float16, 1, 2, 8, 4096) and ops.moe_router_covers(torch.bfloat16, 16, 8, 128, 2048)
    assert not ops.moe_router_covers(torch.float32, 1, 2, 8, 4096) and not ops.moe_router_covers(torch.float16, 17, 2, 8, 4096)


@pytest.mark.parametrize("args,fragment", [
    (dict(T=17), "17 rows are not covered (1 .. 16)"),
    (dict(T=0), "0 rows are not covered"),
    (dict(k=9, E=16), "9 experts per token are not covered (1 .. 8)"),
    (dict(E=1), "1 experts are not covered (k = 2 .. 256)"),
    (dict(E=257), "257 experts are not covered"),
    (dict(H=12), "H=12 is not covered (a multiple of 8, 8 .. 65536)"),
    (dict(H=65544), "H=65544 is not covered"),
    (dict(dt=F32), "fp32 activations are not covered"),
])
def test_unsupported_calls_say_why_before_any_launch(args, fragment):
    """null pointers on a machine without a GPU: the refusal comes before the arguments are looked at, let alone a launch"""
    from hqq_amd import _C
    a = {**dict(T=1, k=2, E=8, H=4096, dt=F16), **args}
    rc = _C.lib().hqq_hip_moe_router(None, None, None, None, None, a["T"], a["k"], a["E"], a["H"], 1, 0, a["dt"], None)
    assert rc == -4 and fragment in _C.last_error() and "hqq_hip_moe_router" in _C.last_error()
    with pytest.raises(NotImplementedError, match="not covered"):
        _C.check(rc, "hqq_hip_moe_router")


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    from hqq_amd import _C
    assert _C.ABI_VERSION == 9 and _C.lib().hqq_hip_abi_version() == 9
    assert "hqq_hip_moe_router" in _C.SYMBOLS and "hqq_hip_moe_router_covers" in _C.SYMBOLS


def test_ops_moe_router_refuses_host_tensors():
    from hqq_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.moe_router(torch.zeros(1, 8, dtype=torch.float16), torch.zeros(2, 8, dtype=torch.float16), 1)


# ---- 4. StepVariant ------------------------------------------------------------------------------------------------------------------------------------------------
def test_eight_variants_and_the_moe_flag():
    from hqq_amd.utils.llama_fused import FAMILIES, VARIANTS, StepVariant
    assert len(VARIANTS) == 8 and len(set(VARIANTS)) == 8
    assert VARIANTS[-2:] == (StepVariant("mixtral"), StepVariant("qwen3_moe"))   # last in resolve's precedence
    assert FAMILIES["mixtral"].moe and FAMILIES["qwen3_moe"].moe and FAMILIES["qwen3_moe"].qk_norm and not FAMILIES["mixtral"].qk_norm
    assert not any(FAMILIES[f].moe for f in ("llama", "qwen3", "qwen2"))
    for v in VARIANTS[:6]:
        assert set(v.flags()) == {"axis0", "qk_norm", "qkv_bias", "lora"} and StepVariant.from_flags(**v.flags()) == v
    mix, q3m = StepVariant.from_flags(moe=True), StepVariant.from_flags(moe=True, qk_norm=True)
    assert mix == StepVariant("mixtral") and q3m == StepVariant("qwen3_moe")
    assert mix.flags() == {"axis0": False, "qk_norm": False, "qkv_bias": False, "lora": False, "moe": True}
    assert q3m.flags() == {"axis0": False, "qk_norm": True, "qkv_bias": False, "lora": False, "moe": True}
    assert StepVariant.from_flags(**mix.flags()) == mix and StepVariant.from_flags(**q3m.flags()) == q3m
    for kw in (dict(axis0=True), dict(qkv_bias=True), dict(lora=True), dict(qk_norm=True, qkv_bias=True), dict(qk_norm=True, axis0=True)):
        with pytest.raises(ValueError):
            StepVariant.from_flags(moe=True, **kw)
    for family in ("mixtral", "qwen3_moe"):
        for kw in (dict(axis0=True), dict(lora=True)):
            with pytest.raises(ValueError):
                StepVariant(family, **kw)


def test_resolve_takes_an_moe_variant_only_when_every_flag_it_sets_is_opted_into(monkeypatch):
    from hqq_amd.utils import llama_fused
    from hqq_amd.utils.llama_fused import StepVariant
    supported = set()
    monkeypatch.setattr(llama_fused, "variant_supported", lambda m, v, batch=None: v in supported)
    supported.add(StepVariant("qwen3_moe"))
    assert llama_fused.resolve(object(), {"moe"}) is None and llama_fused.resolve(object(), {"qk_norm"}) is None
    assert llama_fused.resolve(object(), {"moe", "qk_norm"}) == StepVariant("qwen3_moe")
    supported.add(StepVariant("mixtral"))
    assert llama_fused.resolve(object(), {"moe"}) == StepVariant("mixtral") and llama_fused.resolve(object(), set()) is None
    supported.add(StepVariant("qwen3"))
    assert llama_fused.resolve(object(), {"moe", "qk_norm"}) == StepVariant("qwen3")   # the MoE variants come last


def test_opt_ins_knows_the_keyword():
    from hqq_amd.utils.generation import opt_ins
    assert opt_ins(axis0="model", moe="fused") == {"moe"}
    with pytest.raises(ValueError, match="moe"):
        opt_ins(moe="yes")


# ---- 5. the architecture predicate, knob by knob -----------------------------------------------------------------------------------------------------------------
def _host_experts(E, H, I, dt=torch.float16):
    return MC.experts(MC.build(MC.Case("random", 4, 64, dt, 1, 1, E=E, H=H, I=I, seed=3)))


def _tiny(family, dt=torch.float16, swap=True, **kw):
    """a tiny CPU model of the family (2 blocks, hidden 128, experts of 192) with every experts module replaced by an HQQExperts on the host"""
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    args = dict(vocab_size=64, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=128,
                num_experts_per_tok=2)
    if family == "mixtral":
        args.update(num_local_experts=4)
        args.update(kw)
        model = tf.MixtralForCausalLM(tf.MixtralConfig(**args))
    else:
        args.update(num_experts=8, moe_intermediate_size=192, head_dim=64, norm_topk_prob=True)
        args.update(kw)
        model = tf.Qwen3MoeForCausalLM(tf.Qwen3MoeConfig(**args))
    model = model.to(dt).eval()
    if swap:
        for blk in model.model.layers:
            if hasattr(blk.mlp, "experts"):
                blk.mlp.experts = _host_experts(blk.mlp.gate.weight.shape[0], 128, 192, dt)
    return model


def _ok(model, family):
    from hqq_amd.utils import llama_fused
    return llama_fused._arch_ok(model, llama_fused.FAMILIES[family])


@pytest.mark.parametrize("family", ["mixtral", "qwen3_moe"])
def test_arch_ok_accepts_the_plain_model_and_nothing_built_on_it_by_default(family):
    from hqq_amd.utils import llama_fused
    m = _tiny(family)
    assert _ok(m, family) and llama_fused.moe_arch_supported(m)
    other = "qwen3_moe" if family == "mixtral" else "mixtral"
    assert not _ok(m, other)
    # the dense predicates, and everything built on them, keep refusing MoE models
    assert not llama_fused.arch_supported(m) and not llama_fused.qk_norm_arch_supported(m) and not llama_fused.qkv_bias_arch_supported(m)
    assert not llama_fused.supports(m) and not llama_fused.supports_moe(m)   # (host tensors: nothing is supported here, and nothing raises)
    assert _ok(_tiny(family, dt=torch.bfloat16), family)


def _set_top_k(n):
    def f(m):
        m.model.layers[1].mlp.gate.top_k = n
    return f


def _router_dtype(m):
    g = m.model.layers[0].mlp.gate
    g.weight = torch.nn.Parameter(g.weight.data.float(), requires_grad=False)


def _router_bias(m):
    g = m.model.layers[0].mlp.gate
    g.bias = torch.nn.Parameter(torch.zeros(g.weight.shape[0], dtype=g.weight.dtype))


def _shared_expert(m):
    m.model.layers[1].mlp.shared_expert = torch.nn.Linear(128, 128)


def _window_on_module(m):
    m.model.layers[0].self_attn.sliding_window = 16


def _norm_topk_not_bool(m):
    m.model.layers[0].mlp.gate.norm_topk_prob = 1


MOE_KNOBS = {
    # knob: (config keywords, edit of the built model, swap the experts, families)
    "sliding_window": (dict(sliding_window=16), None, True, ("mixtral",)),
    "use_sliding_window": (dict(use_sliding_window=True, sliding_window=16), None, True, ("qwen3_moe",)),
    "window_on_module": ({}, _window_on_module, True, ("mixtral", "qwen3_moe")),
    "mlp_only_layers": (dict(mlp_only_layers=[1]), None, True, ("qwen3_moe",)),
    "decoder_sparse_step": (dict(decoder_sparse_step=2), None, True, ("qwen3_moe",)),
    "top_k_9": ({}, _set_top_k(9), True, ("mixtral", "qwen3_moe")),
    "top_k_above_experts": ({}, _set_top_k(5), True, ("mixtral",)),
    "top_k_not_an_integer": ({}, _set_top_k(2.0), True, ("mixtral", "qwen3_moe")),
    "experts_not_hqq": ({}, None, False, ("mixtral", "qwen3_moe")),
    "router_dtype": ({}, _router_dtype, True, ("mixtral", "qwen3_moe")),
    "router_bias": ({}, _router_bias, True, ("mixtral", "qwen3_moe")),
    "shared_expert": ({}, _shared_expert, True, ("mixtral", "qwen3_moe")),
    "norm_topk_prob_not_bool": ({}, _norm_topk_not_bool, True, ("qwen3_moe",)),
    "attention_bias": (dict(attention_bias=True), None, True, ("qwen3_moe",)),
}


@pytest.mark.parametrize("family,knob", [(f, k) for k, v in MOE_KNOBS.items() for f in v[3]])
def test_arch_ok_refuses_knob_by_knob(family, knob):
    kw, edit, swap, _ = MOE_KNOBS[knob]
    m = _tiny(family, swap=swap, **kw)
    if edit is not None:
        edit(m)
    assert not _ok(m, family)


def test_other_moe_model_types_are_refused():
    m = _tiny("mixtral")
    for other in ("qwen2_moe", "phimoe", "olmoe", "deepseek_v3"):
        m.config.model_type = other
        assert not _ok(m, "mixtral") and not _ok(m, "qwen3_moe")


def test_fused_step_refuses_folded_glue_and_unknown_combinations():
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    for kw in (dict(moe=True, glue="folded"), dict(moe=True, qk_norm=True, glue="folded")):
        with pytest.raises(ValueError, match="folded"):
            FusedLlamaStep(_tiny("mixtral"), None, 64, **kw)
    with pytest.raises(ValueError, match="moe=True"):
        FusedLlamaStep(_tiny("mixtral"), None, 64, moe=True, lora=True)
