"""CPU half of the mixture-of-experts tests (hqq_amd/core/moe.py HQQExperts, csrc/moe.hip): the module's construction, storage, composed route and state,
the cases of tests/_moe_cases.py checked against their own premises, and the C ABI's host side.

Quantising needs the GPU in this package (there is no CPU quantiser in the product).  Where a test here has to quantise, hqq_amd.ops.quantize /
hqq_amd.ops.dequantize are replaced, for the duration of that test, by the CPU oracle's restatement (oracle/hqq_oracle.c — a checker, never the product
path): what is under test is that HQQExperts makes the call HQQLinear makes, slice by slice, and stores what comes back; tests/test_moe_gpu.py repeats the
identity with the real quantiser."""
import contextlib
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _moe_cases as C   # noqa: E402

UNSUPPORTED = -4
F32c, F16c, BF16c = 0, 1, 2


@contextlib.contextmanager
def oracle_quantiser(oracle):
    """ops.quantize / ops.dequantize on CPU tensors through the oracle (axis 1, fp16 constants)"""
    from hqq_amd import ops

    def quantize(W, nbits=4, group_size=64, round_zero=False, optimize=True, axis=1, solver_dtype=torch.float32, **kw):
        assert axis == 1 and solver_dtype == torch.float32
        r = oracle.quantize(W.detach().float().numpy(), nbits=nbits, group_size=group_size, round_zero=round_zero, optimize=optimize)
        return torch.from_numpy(oracle.pack(ops.PACK_BITS[nbits], r["Wq"])), torch.from_numpy(r["scale"]), torch.from_numpy(r["zero"])

    def dequantize(W_q, scale, zero, N, K, group_size, nbits, axis=1):
        assert axis == 1 and scale.dtype == torch.float16
        out = oracle.dequantize(nbits, W_q.numpy(), scale.numpy(), zero.numpy(), N, K, group_size, F16c)
        return torch.from_numpy(np.ascontiguousarray(out))

    old = ops.quantize, ops.dequantize
    ops.quantize, ops.dequantize = quantize, dequantize
    try:
        yield
    finally:
        ops.quantize, ops.dequantize = old


def tiny_mixtral_config(**kw):
    from transformers import MixtralConfig
    return MixtralConfig(vocab_size=64, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                         num_local_experts=4, num_experts_per_tok=2, max_position_embeddings=128, **kw)


def tiny_experts(seed=0):
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts
    m = MixtralExperts(tiny_mixtral_config())
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.gate_up_proj.copy_(torch.randn(m.gate_up_proj.shape, generator=g) * 0.05)
        m.down_proj.copy_(torch.randn(m.down_proj.shape, generator=g) * 0.05)
    return m


def cfg_of(nbits, gs):
    from hqq_amd.core.quantize import BaseQuantizeConfig
    return BaseQuantizeConfig(nbits=nbits, group_size=gs, axis=1)


@pytest.fixture(scope="module")
def quantised(oracle):
    """{(nbits, gs): (HQQExperts on the CPU, the dense module it was made from)}"""
    from hqq_amd.core.moe import HQQExperts
    out = {}
    with oracle_quantiser(oracle):
        for nbits, gs in C.CONFIGS:
            dense = tiny_experts()
            out[nbits, gs] = (HQQExperts(dense, cfg_of(nbits, gs), compute_dtype=torch.float16, device="cpu", del_orig=False), dense)
    return out


# ---- 1. per-expert identity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,gs", C.CONFIGS)
def test_every_expert_is_what_hqqlinear_makes_of_its_slice(oracle, quantised, nbits, gs):
    from hqq_amd.core.quantize import HQQLinear, Quantizer
    q, dense = quantised[nbits, gs]
    E, I, H = 4, 192, 128
    assert (q.num_experts, q.intermediate_dim, q.hidden_dim) == (E, I, H)
    per = 8 // nbits
    assert q.gate_W_q.shape == (E, I * H // gs // per, gs) and q.down_W_q.shape == (E, H * I // gs // per, gs) and q.up_scale.shape == (E, I * H // gs, 1)
    for role in C.ROLES:
        for kind in ("W_q", "scale", "zero"):
            t = getattr(q, f"{role}_{kind}")
            assert t.is_contiguous() and t.shape[0] == E and t.dtype == (torch.uint8 if kind == "W_q" else torch.float16)
    with oracle_quantiser(oracle):
        for e in range(E):
            slices = {"gate": dense.gate_up_proj.data[e, :I], "up": dense.gate_up_proj.data[e, I:], "down": dense.down_proj.data[e]}
            for role in C.ROLES:
                lin = torch.nn.Linear(slices[role].shape[1], slices[role].shape[0], bias=False)
                lin.weight.data = slices[role].clone()
                ref = HQQLinear(lin, cfg_of(nbits, gs), compute_dtype=torch.float16, device="cpu")
                assert torch.equal(getattr(q, role + "_W_q")[e], ref.W_q.data) and ref.W_q.dtype == torch.uint8, (e, role)
                assert torch.equal(getattr(q, role + "_scale")[e], ref.meta["scale"]) and torch.equal(getattr(q, role + "_zero")[e], ref.meta["zero"]), (e, role)
                view = q.expert_linear(e, role)
                assert view.W_q.data_ptr() == getattr(q, role + "_W_q")[e].data_ptr() and view.meta["scale"].data_ptr() == getattr(q, role + "_scale")[e].data_ptr()
                assert (view.in_features, view.out_features) == (ref.in_features, ref.out_features) and view.meta["shape"] == ref.meta["shape"]
                want = Quantizer.dequantize(ref.W_q, ref.meta)
                assert torch.equal(view.dequantize(), want)
                assert torch.equal(q.dequantize(e, role), want)       # the host formula of the composed route, against the oracle's restatement


def test_only_silu_experts_are_taken(oracle):
    from hqq_amd.core.moe import HQQExperts, is_experts_module
    m = tiny_experts()
    assert is_experts_module(m) and not is_experts_module(torch.nn.Linear(8, 8))
    m.act_fn = torch.nn.GELU()
    with pytest.raises(NotImplementedError, match="SiLU"):
        HQQExperts(m, cfg_of(4, 64), compute_dtype=torch.float16, device="cpu")


# ---- 2. the composed route is HF's loop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,gs", C.CONFIGS)
@pytest.mark.parametrize("T", [1, 3, 16])
def test_composed_route_is_hf_forward_on_the_dequantised_weights(quantised, nbits, gs, T):
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts
    q, _ = quantised[nbits, gs]
    hf = MixtralExperts(tiny_mixtral_config()).to(torch.float16)
    with torch.no_grad():
        for e in range(4):
            hf.gate_up_proj[e].copy_(torch.cat([q.dequantize(e, "gate"), q.dequantize(e, "up")]))
            hf.down_proj[e].copy_(q.dequantize(e, "down"))
    g = torch.Generator().manual_seed(100 + T)
    x = (torch.randn((T, 128), generator=g) * 0.5).half()
    idx, w = C.routing(C.Case("random", nbits, gs, torch.float16, T, 2), g)
    with torch.no_grad():
        want = MixtralExperts.forward.__wrapped__(hf, x, idx, w) if hasattr(MixtralExperts.forward, "__wrapped__") else hf(x, idx, w)
        got = q.forward_composed(x, idx, w)
        assert torch.equal(q(x, idx, w), got)                          # fused = None composes CPU tensors
    assert got.dtype == torch.float16 and got.shape == (T, 128) and torch.equal(got, want)
    assert float(got.abs().max()) > 0


# ---- 3. closed-form inputs ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def closed():
    return {c.id: C.build(c) for c in C.CLOSED}


@pytest.mark.parametrize("cid", [c.id for c in C.CLOSED])
def test_closed_form_cases_host_model_is_the_composed_route(closed, oracle, cid):
    data = closed[cid]
    c = data["case"]
    st, _ = C.stacks(data)
    for role in C.ROLES:                                               # the packing helper is the BitPack layout
        assert np.array_equal(st[role, "W_q"][0].numpy(), oracle.pack(c.nbits, data[role]["levels"][0].numpy()))
    q = C.experts(data)
    for role in C.ROLES:
        assert torch.equal(q.dequantize(c.E - 1, role), data[role]["W"][c.E - 1])
    a, out = C.model(data)
    with torch.no_grad():
        got = q.forward_composed(data["x"], data["idx"], data["w"])
    assert torch.equal(got, out) and float(out.abs().max()) > 0
    # exact in fp32 in any order: the same bits with fp32 sums in two random orders
    for seed in (1, 2):
        a32, out32 = C.model(data, C.fp32_dot(seed))
        assert torch.equal(a32, a) and torch.equal(out32, out)
    # sensitive to the combine order where a token has more than one slot: reversing it changes a bit somewhere in the k = 8 case
    if c.k == 8:
        rev = torch.zeros_like(out)
        for t in range(c.T):
            for s in reversed(C.slot_order(data["idx"][t])):
                d = (data["down"]["W"][int(data["idx"][t, s])].double() @ a[t, s].double()).to(c.dt)
                rev[t] = rev[t] + (d.float() * data["w"][t, s]).to(c.dt)
        assert not torch.equal(rev, out)


def test_closed_form_cases_cover_the_edges():
    ids = {c.id for c in C.CLOSED}
    assert len(ids) == len(C.CLOSED) == 25
    for c in C.CLOSED:
        idx, _ = C.routing(c, torch.Generator().manual_seed(c.seed))
        if c.k >= 2:
            assert int(idx[0, 0]) > int(idx[0, 1])                     # descending expert order
    assert any(c.k == 1 for c in C.CLOSED) and any(c.E == 8 and c.k == 8 for c in C.CLOSED)
    assert (192 // 64) % 2 == 1 and 192 % 128 != 0                    # an odd number of groups per row; I no multiple of 128


# ---- 4. the bound holds and separates ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_cases():
    return {c.id: C.build(c) for c in C.RANDOM}


@pytest.mark.parametrize("cid", [c.id for c in C.RANDOM])
def test_bound_holds_for_fp32_sums_in_random_orders_and_separates(random_cases, cid):
    data = random_cases[cid]
    c = data["case"]
    a, out = C.model(data)
    Da = C.bound_a(data)
    Dfull = C.bound_out(data, a, Da)
    for seed in (11, 12, 13):
        a32, out32 = C.model(data, C.fp32_dot(seed))
        assert bool(((a32.double() - a.double()).abs() <= Da).all())
        assert bool(((out32.double() - out.double()).abs() <= Dfull).all())
        own = C.model_down(data, a32, C.fp32_dot(seed + 50))            # down from "the kernel's own a"
        assert bool(((own.double() - C.model_down(data, a32).double()).abs() <= C.bound_out(data, a32)).all())
    # one slot's expert replaced by another: outside the bound somewhere
    wrong = data["idx"].clone()
    wrong[c.T - 1, c.k - 1] = (wrong[c.T - 1, c.k - 1] + 1) % c.E
    swapped = dict(data, idx=wrong)
    a_w = C.model_a(swapped)
    assert bool(((a_w.double() - a.double()).abs() > Da).any())
    out_w = C.model_down(data, a, idx=wrong)                            # the right a, the wrong expert's down projection
    assert bool(((out_w.double() - out.double()).abs() > C.bound_out(data, a)).any())
    # one routing weight dropped
    w0 = data["w"].clone()
    w0[0, 0] = 0.0
    out_0 = C.model_down(data, a, w=w0)
    assert bool(((out_0.double() - out.double()).abs() > C.bound_out(data, a)).any())


# ---- 5. state and patching ---------------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip(quantised):
    from hqq_amd.core.moe import HQQExperts
    q, _ = quantised[4, 64]
    sd = q.state_dict()
    assert set(sd) == {f"{r}_{k}" for r in C.ROLES for k in ("W_q", "scale", "zero")} | {"_extra_state"}
    assert all(isinstance(sd[k], torch.Tensor) for k in sd if k != "_extra_state")
    shell = HQQExperts(None, None, compute_dtype=torch.float16, device="cpu")
    assert not shell.ready
    shell.load_state_dict(sd)
    assert shell.ready and (shell.num_experts, shell.hidden_dim, shell.intermediate_dim) == (4, 128, 192) and shell.quant_config == q.quant_config
    for k in sd:
        if k != "_extra_state":
            assert torch.equal(getattr(shell, k), getattr(q, k))
    assert shell.layer_meta["down"]["shape"] == torch.Size([128, 192]) and shell.layer_meta["gate"]["unpack_view_dtype"] == torch.uint8
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((3, 128), generator=g) * 0.5).half()
    idx, w = C.routing(C.Case("random", 4, 64, torch.float16, 3, 2), g)
    assert torch.equal(shell(x, idx, w), q(x, idx, w))


def _moe_modules(model):
    from hqq_amd.core.moe import HQQExperts
    return [(n, m) for n, m in model.named_modules() if n.endswith(".experts")], HQQExperts


def test_quantize_model_replaces_every_experts_module(oracle):
    from transformers import MixtralForCausalLM, Qwen3MoeConfig, Qwen3MoeForCausalLM
    from hqq_amd.core.quantize import HQQLinear
    from hqq_amd.utils.model import LLAMA_LINEAR_TAGS, quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    torch.manual_seed(0)
    qcfg = Qwen3MoeConfig(vocab_size=64, hidden_size=128, intermediate_size=192, moe_intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                          num_key_value_heads=2, num_experts=8, num_experts_per_tok=2, head_dim=32, max_position_embeddings=128)
    for model, E in ((MixtralForCausalLM(tiny_mixtral_config()), 4), (Qwen3MoeForCausalLM(qcfg), 8)):
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        with oracle_quantiser(oracle):
            quantize_model(model, {t: None for t in LLAMA_LINEAR_TAGS}, compute_dtype=torch.float16, device="cpu")      # no expert_config: untouched
        mods, HQQExperts = _moe_modules(model)
        assert len(mods) == 2 and not any(isinstance(m, (HQQExperts, HQQLinear)) for _, m in model.named_modules())
        assert all(torch.equal(p, before[n]) for n, p in model.named_parameters())
        with oracle_quantiser(oracle):
            quantize_model(model, {t: None for t in LLAMA_LINEAR_TAGS}, compute_dtype=torch.float16, device="cpu", expert_config=cfg_of(4, 64))
        mods, _ = _moe_modules(model)
        assert len(mods) == 2 and all(isinstance(m, HQQExperts) and m.ready and m.num_experts == E and m.name == n for n, m in mods)
        for i, layer in enumerate(model.model.layers):                  # the router stays dense
            assert type(layer.mlp.gate).__name__.endswith("TopKRouter") and isinstance(layer.mlp.gate.weight, torch.nn.Parameter)
            assert torch.equal(layer.mlp.gate.weight, before[f"model.layers.{i}.mlp.gate.weight"])
        assert not any(n.endswith("gate_up_proj") or n.endswith("experts.down_proj") for n, _ in model.named_parameters())
        prepare_for_inference(model, backend="hip")                     # no HQQLinear child to patch: the module is left working
        mods, _ = _moe_modules(model)
        assert all(isinstance(m, HQQExperts) for _, m in mods)
        m = mods[0][1]
        g = torch.Generator().manual_seed(1)
        x = (torch.randn((2, 128), generator=g) * 0.5).half()
        out = m(x, torch.tensor([[0, 1], [E - 1, 2]]), torch.tensor([[0.5, 0.5], [0.75, 0.25]]))
        assert out.shape == (2, 128) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0


# ---- the C ABI's host side ---------------------------------------------------------------------------------------------------------------------------------------
def test_covers_refusals_and_constants():
    from hqq_amd import _C, ops
    lib = _C.lib()
    assert ops.MOE_MAX_T == 16 and 1 <= ops.MOE_ROUTE_MAX_T <= ops.MOE_MAX_T
    f16 = torch.float16
    assert ops.moe_covers(f16, 1, 2, 8, 4096, 14336, 64, 4) and ops.moe_covers(torch.bfloat16, 16, 8, 256, 2048, 768, 16, 2)
    assert ops.moe_covers(f16, 3, 2, 4, 128, 192, 64, 4) and ops.moe_covers(f16, 3, 1, 4, 128, 192, 16, 2)
    for bad in ((17, 2, 8, 4096, 14336, 64, 4), (0, 2, 8, 4096, 14336, 64, 4), (1, 9, 16, 4096, 14336, 64, 4), (1, 2, 257, 4096, 14336, 64, 4),
                (1, 2, 8, 4096 + 32, 14336, 32, 4), (1, 2, 8, 4096, 14336 + 32, 32, 4), (1, 2, 8, 4096, 14336, 24, 4), (1, 2, 8, 4096, 14336, 8, 4),
                (1, 2, 8, 128, 192, 128, 4), (1, 2, 8, 4096, 14336, 64, 8), (1, 2, 8, 4096, 14336, 64, 3), (1, 2, 8, 4096, 14336, 64, 1)):
        assert not ops.moe_covers(f16, *bad), bad
        assert b"hqq_hip_moe" in lib.hqq_hip_last_error()
    assert not ops.moe_covers(torch.float32, 1, 2, 8, 4096, 14336, 64, 4) and not ops.moe_covers(f16, 1, 2, 8, 4096, 14336, 64, 4, axis=0)
    assert not ops.moe_covers(f16, 1, 2, 8, 4096, 14336, None, 4)
    # the entry points refuse with the code and a message before anything is launched (no GPU in this process)
    p = ctypes.c_void_p(16)
    assert lib.hqq_hip_moe_gate_up(8, p, p, p, p, p, p, p, p, p, 1, 2, 8, 4096, 14336, 64, F16c, None) == UNSUPPORTED and b"8-bit" in lib.hqq_hip_last_error()
    assert lib.hqq_hip_moe_down(4, p, p, p, p, p, p, p, 17, 2, 8, 4096, 14336, 64, F16c, None) == UNSUPPORTED and b"17 tokens" in lib.hqq_hip_last_error()
    assert lib.hqq_hip_moe_down(4, p, p, p, p, p, p, p, 1, 2, 8, 4096, 14336, 64, F32c, None) == UNSUPPORTED and b"fp32" in lib.hqq_hip_last_error()
    assert lib.hqq_hip_moe_gate_up(5, p, p, p, p, p, p, p, p, p, 1, 2, 8, 4096, 14336, 64, F16c, None) == -1
    with pytest.raises(RuntimeError, match="no CPU path"):
        z = torch.zeros(1)
        ops.moe_gate_up(torch.zeros(1, 128, dtype=f16), torch.zeros(1, 2, dtype=torch.int64), (z, z, z), (z, z, z), 4, 128, 192, 64, 4)


def test_fused_true_raises_outside_coverage(quantised):
    from hqq_amd.core.moe import HQQExperts
    q, _ = quantised[4, 64]
    x = torch.zeros(1, 128, dtype=torch.float16)
    HQQExperts.fused = True
    try:
        with pytest.raises(NotImplementedError, match="outside"):
            q(x, torch.zeros(1, 2, dtype=torch.int64), torch.ones(1, 2))   # CPU tensors are outside what the kernel covers
    finally:
        HQQExperts.fused = None
