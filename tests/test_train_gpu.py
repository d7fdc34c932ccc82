"""The training path's gradients on the GPU against float64, route by route (cases, references and derived bounds: tests/_train_cases.py, proved on
the host by tests/test_train_cpu.py): HQQLinear's input gradient on solver-built meta through the fused dgrad kernel and through every fallback, on
both sides of ops.DGRAD_ROUTE_MAX_M as the module has it, with a counting spy saying which side served; the forward under autograd; non-dense
grad_outputs; activation checkpointing; HQQLinearLoRA's gradients in every option; and a tiny Llama with all seven projections adapted against a
compute-dtype and a float64 torch-only replica (table: profiles/train_grad_errors.md)."""
import functools
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.checkpoint import checkpoint

import _train_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = tc.LORA_ALPHA / tc.LORA_R


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from hqq_amd import ops as o
    assert o.is_available(), "libhqq_hip.so must load on the GPU box (no fallback)"
    return o


class _Spy:
    """ops.gemm_dgrad with its behaviour kept: counts the calls and notes whether the gradient it was handed was dense"""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, g, *a, **kw):
        self.calls.append(g.is_contiguous())
        return self.fn(g, *a, **kw)

    @property
    def n(self):
        return len(self.calls)


@pytest.fixture
def spy(ops, monkeypatch):
    s = _Spy(ops.gemm_dgrad)
    monkeypatch.setattr(ops, "gemm_dgrad", s)
    return s


def _bits(t):
    return t.contiguous().view(torch.int16)


def _build(nbits, dn, axis, N, K, gs, bias, vaf=False):
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    lin = nn.Linear(K, N, bias=bias)
    lin.weight.data = tc.layer_weight(N, K, seed=N + nbits)
    if bias:
        lin.bias.data = tc.randn((N,), seed=N + 1, scale=0.1)
    layer = HQQLinear(lin, BaseQuantizeConfig(nbits=nbits, group_size=gs, axis=axis, view_as_float=vaf), compute_dtype=tc.DTYPES[dn], device="cuda")
    m = layer.meta
    assert bool(torch.isfinite(m["scale"]).all()) and bool(torch.isfinite(m["zero"]).all())
    if axis == 1:   # the premise of the cases, read off the built meta: zero-points below 0 and above the largest level
        assert tc.one_signed_groups(tc.layer_weight(N, K, seed=N + nbits), gs, 1) == (True, True)
        assert tc.zero_point_kinds(m["zero"], nbits) == (True, True), (float(m["zero"].min()), float(m["zero"].max()))
    return layer


@functools.lru_cache(maxsize=None)
def _layer(nbits, dn, axis, N, K, gs, bias, vaf=False):
    """one bare layer per configuration, shared by the tests that leave it as it is; W [N, K] = dequantize() on the host in float64"""
    layer = _build(nbits, dn, axis, N, K, gs, bias, vaf)
    if bias:
        layer.bias = layer.bias.detach().requires_grad_(True)   # (HQQLinear keeps its bias as a plain tensor: a leaf here)
    return layer, layer.dequantize().double().cpu()


def _inputs(shape, N, dn, seed):
    """x in the compute dtype and the fixed fp32 coefficients t of the loss (y.float() * t).sum()"""
    return tc.randn(shape, seed, tc.DTYPES[dn]).cuda(), tc.randn(tuple(shape[:-1]) + (N,), seed + 1).cuda()


def _backward(layer, x0, t):
    x = x0.clone().requires_grad_(True)
    if layer.bias is not None:
        layer.bias.grad = None
    y = layer(x)
    y.retain_grad()
    (y.float() * t).sum().backward()
    return x.grad, y.grad, y.detach()


def _inside(got, want, bound, what):
    ok, worst = tc.within(got, want, bound)
    assert ok, f"{what}: worst |error| / bound = {worst:.3f}"


BARE = [(nb, dn, ax, N, K, gs, b) for nb in tc.NBITS_ALL for dn in tc.DTYPES for ax in (1, 0) for (N, K, gs) in tc.SHAPES for b in (False, True)]
VAF = (4, "f16", 1, 128, 256, 32, True, True)
BARE_IDS = [f"{c[0]}bit-{c[1]}-axis{c[2]}-{c[3]}x{c[4]}g{c[5]}-{'bias' if c[6] else 'nobias'}{'-vaf' if len(c) > 7 else ''}" for c in BARE + [VAF]]


@pytest.mark.parametrize("cfg", BARE + [VAF], ids=BARE_IDS)
def test_bare_layer_input_gradient_on_every_route(ops, spy, cfg):
    from hqq_amd.core.quantize import HQQLinear
    nbits, dn, axis, N, K, gs, bias = cfg[:7]
    dt, R = tc.DTYPES[dn], ops.DGRAD_ROUTE_MAX_M
    assert R >= 2
    layer, W = _layer(*cfg)
    kernel = axis == 1 and nbits in tc.NBITS_KERNEL
    forms = tc.row_forms(R, K)
    xb, tb = _inputs(forms["R+1"], N, dn, seed=K + nbits)   # R rows are the first R of R + 1: one reference serves both sides of the boundary
    first_R = {}
    for name, shape in forms.items():
        x0, t = (xb, tb) if name == "R+1" else (xb[:R], tb[:R]) if name == "R" else _inputs(shape, N, dn, seed=K + nbits + len(name))
        rows, before = x0.numel() // K, spy.n
        xg, go, _ = _backward(layer, x0, t)
        assert spy.n - before == (1 if kernel and 1 <= rows <= R else 0), (name, spy.n - before)
        assert xg.dtype == dt and tuple(xg.shape) == tuple(shape) and go.dtype == dt and layer.W_q.grad is None and not layer.W_q.requires_grad
        if bias:
            assert torch.equal(layer.bias.grad, go.reshape(-1, N).sum(0)), name
        if rows == 0:
            continue
        go2 = go.reshape(-1, N).cpu()
        _inside(xg.reshape(-1, K), tc.ref_dx(go2, W), tc.bound_dx(go2, W, dt), name)
        if name in ("R", "R+1"):
            first_R[name] = (xg[:R], go[:R])
    # both sides of the boundary against the same reference: the same grad_output rows, each result within the bound of the one reference
    assert torch.equal(_bits(first_R["R"][1]), _bits(first_R["R+1"][1]))
    go2 = first_R["R"][1].cpu()
    for name, (xg, _) in first_R.items():
        _inside(xg, tc.ref_dx(go2, W), tc.bound_dx(go2, W, dt), f"first R rows of {name}")
    # the switch: no kernel call, the same bound
    before, flag = spy.n, HQQLinear.fused_backward
    HQQLinear.fused_backward = False
    try:
        xg, go, _ = _backward(layer, xb[:R], tb[:R])
    finally:
        HQQLinear.fused_backward = flag
    assert spy.n == before and HQQLinear.fused_backward is True
    _inside(xg, tc.ref_dx(go.cpu(), W), tc.bound_dx(go.cpu(), W, dt), "fused_backward = False")


@pytest.mark.parametrize("cfg", BARE + [VAF], ids=BARE_IDS)
def test_forward_under_autograd_is_the_inference_forward(ops, cfg):
    N, K, dn = cfg[3], cfg[4], cfg[1]
    layer, _ = _layer(*cfg)
    for name, shape in tc.row_forms(ops.DGRAD_ROUTE_MAX_M, K).items():
        x0, _ = _inputs(shape, N, dn, seed=K + len(name))
        y = layer(x0.clone().requires_grad_(True))
        assert y.requires_grad
        with torch.no_grad():
            assert torch.equal(y.detach(), layer(x0)), name


@pytest.mark.parametrize("N,K,gs", tc.SHAPES)
@pytest.mark.parametrize("nbits,dn", [(4, "f16"), (2, "bf16")])
def test_non_dense_grad_outputs(ops, spy, nbits, dn, N, K, gs):
    dt, R = tc.DTYPES[dn], ops.DGRAD_ROUTE_MAX_M
    layer, W = _layer(nbits, dn, 1, N, K, gs, False)
    m = layer.meta
    x0, t = _inputs((R, K), N, dn, seed=3)
    c, c2 = t.t().contiguous().to(dt), t[:, ::2].contiguous()
    losses = {"expanded": lambda y: y.sum(), "transposed": lambda y: (y.t() * c).sum(), "slice": lambda y: (y[:, ::2].float() * c2).sum()}
    for name, loss in losses.items():
        x = x0.clone().requires_grad_(True)
        y = layer(x)
        y.retain_grad()
        before = spy.n
        l = loss(y)
        l.backward(retain_graph=True)
        assert spy.n == before + 1
        if name != "slice":   # (the slice's backward fills a dense buffer; the other two reach the kernel's wrapper as they are)
            assert spy.calls[-1] is False, name
        go, g1 = y.grad.clone(), x.grad.clone()
        _inside(g1, tc.ref_dx(go.cpu(), W), tc.bound_dx(go.cpu(), W, dt), name)
        dense = spy.fn(go.contiguous(), layer.W_q, m["scale"], m["zero"], N, K, gs, nbits)
        assert torch.equal(_bits(g1), _bits(dense)), name
        l.backward()   # a second pass accumulates: g1 + g1, one more rounding (exact in binary floating point short of overflow)
        _inside(x.grad, 2 * g1.double().cpu(), tc.rounded(2 * g1.double().cpu(), 0.0, dt), name + " twice")


def _lora(layer, dn, train_dtype=torch.float32, train_bias=False, dropout=0.0, seed=11):
    from hqq_amd.core.peft import HQQLinearLoRA
    init = tc.lora_init(layer.in_features, layer.out_features, seed)
    return HQQLinearLoRA(layer, {"r": tc.LORA_R, "lora_alpha": tc.LORA_ALPHA, "dropout": dropout, "train_dtype": train_dtype,
                                 "train_bias": train_bias, "lora_init": init})


@pytest.mark.parametrize("nbits,dn", [(4, "f16"), (2, "bf16"), (3, "f16")])
def test_checkpointing_changes_no_bit(ops, nbits, dn):
    """activation checkpointing re-runs the forward inside backward; the kernels are deterministic, so every gradient keeps its bits"""
    N, K, gs = tc.SHAPES[0]
    R = ops.DGRAD_ROUTE_MAX_M
    x0, t = _inputs((R, K), N, dn, seed=5)
    bare, _ = _layer(nbits, dn, 1, N, K, gs, False)
    lora = _lora(_build(nbits, dn, 1, N, K, gs, True), dn)
    for mod, params in ((bare, []), (lora, [lora.lora_A, lora.lora_B])):
        got = []
        for ck in (False, True):
            for p in params:
                p.grad = None
            x = x0.clone().requires_grad_(True)
            y = checkpoint(mod, x, use_reentrant=False) if ck else mod(x)
            (y.float() * t).sum().backward()
            got.append([x.grad] + [p.grad.clone() for p in params])
        for a, b in zip(*got):
            assert torch.equal(a, b) and bool(a.abs().sum() > 0)


class _FixedDrop(nn.Module):
    """dropout with a fixed mask, already divided by (1 - p)"""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return x * self.m


def _check_lora(layer, lora, dn, Rt, shape, train_bias, mask=None, seed=21):
    dt, N, K = tc.DTYPES[dn], layer.out_features, layer.in_features
    W = layer.dequantize().double().cpu()
    x0, t = _inputs(shape, N, dn, seed)
    x = x0.clone().requires_grad_(True)
    y = lora(x)
    y.retain_grad()
    (y.float() * t).sum().backward()
    go = y.grad
    A, B = lora.lora_A.detach().cpu(), lora.lora_B.detach().cpu()
    m2 = None if mask is None else mask.reshape(-1, K).cpu()
    args = (x0.reshape(-1, K).cpu(), go.reshape(-1, N).cpu(), W, A, B, S)
    ref, bnd = tc.ref_lora(*args, m2), tc.bound_lora(*args, dt, Rt, m2)
    assert x.grad.dtype == dt and tuple(x.grad.shape) == tuple(shape) and lora.lora_A.grad.dtype == Rt and lora.lora_B.grad.dtype == Rt
    assert layer.W_q.grad is None and layer.bias is None
    _inside(lora.lora_A.grad, ref["A"], bnd["A"], "A.grad")
    _inside(lora.lora_B.grad, ref["B"], bnd["B"], "B.grad")
    _inside(x.grad.reshape(-1, K), ref["x"], bnd["x"], "x.grad")
    if train_bias:
        assert lora.bias.requires_grad and lora.bias.grad.dtype == Rt
        _inside(lora.bias.grad, ref["bias"], bnd["bias"], "bias.grad")
    elif lora.bias is not None:   # the frozen bias
        assert lora.bias.grad is None and not lora.bias.requires_grad
    return x0


# base bias / train_bias: a frozen bias, a trained bias taken from the base, a trained bias created on a bias-free base
BIAS_MODES = {"frozen": (True, False), "trained": (True, True), "created": (False, True)}


@pytest.mark.parametrize("mode", list(BIAS_MODES))
@pytest.mark.parametrize("form", ["R", "R+1", "3d"])
@pytest.mark.parametrize("N,K,gs", tc.SHAPES)
@pytest.mark.parametrize("dn", list(tc.DTYPES))
@pytest.mark.parametrize("nbits", [8, 4, 2, 3])
def test_lora_wrapper_gradients(ops, nbits, dn, N, K, gs, form, mode):
    base_bias, train_bias = BIAS_MODES[mode]
    layer = _build(nbits, dn, 1, N, K, gs, base_bias)
    lora = _lora(layer, dn, train_bias=train_bias)
    assert (lora.bias is not None) and lora.bias.dtype == (torch.float32 if train_bias else tc.DTYPES[dn])
    _check_lora(layer, lora, dn, torch.float32, tc.row_forms(ops.DGRAD_ROUTE_MAX_M, K)[form], train_bias)


@pytest.mark.parametrize("form", ["R", "R+1"])
def test_lora_wrapper_gradients_with_bf16_adapters(ops, form):
    N, K, gs = tc.SHAPES[0]
    layer = _build(4, "bf16", 1, N, K, gs, True)
    lora = _lora(layer, "bf16", train_dtype=torch.bfloat16, train_bias=True)
    assert lora.lora_A.dtype == torch.bfloat16 and lora.bias.dtype == torch.bfloat16
    _check_lora(layer, lora, "bf16", torch.bfloat16, tc.row_forms(ops.DGRAD_ROUTE_MAX_M, K)[form], True)


@pytest.mark.parametrize("form", ["R", "R+1", "3d"])
@pytest.mark.parametrize("nbits,dn", [(4, "f16"), (2, "bf16"), (3, "bf16"), (8, "f16")])
def test_lora_wrapper_gradients_under_dropout(ops, nbits, dn, form):
    N, K, gs = tc.SHAPES[1]
    shape = tc.row_forms(ops.DGRAD_ROUTE_MAX_M, K)[form]
    layer = _build(nbits, dn, 1, N, K, gs, True)
    lora = _lora(layer, dn, dropout=tc.P_DROP)
    drop = lora.peft_drop
    assert isinstance(drop, nn.Dropout) and drop.p == tc.P_DROP
    lora.train()
    mask = tc.drop_mask(shape, seed=31, dtype=torch.float32).cuda()
    lora.peft_drop = _FixedDrop(mask)
    x0 = _check_lora(layer, lora, dn, torch.float32, shape, False, mask=mask)
    # eval() turns the module's own dropout off: the p = 0 output, bit for bit
    lora.peft_drop = drop
    plain = _lora(_build(nbits, dn, 1, N, K, gs, True), dn)
    with torch.no_grad():
        assert not torch.equal(lora(x0), plain(x0))
        lora.eval()
        assert torch.equal(lora(x0), plain(x0))


# ---- the whole model ----
TAGS = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
LR = 0.03     # chosen on the float64 replica on the host (round-to-nearest 4- and 2-bit weights): its loss falls by about 0.2 a step; 0.1 still falls, 0.3 does not
STEPS = 3
_TABLES = {}


def _tiny_llama(dt, attn=None):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    kw = {} if attn is None else {"attn_implementation": attn}
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=128, **kw)
    return LlamaForCausalLM(cfg).to(dt).cuda().eval()


def _adapt(model, train_dtype):
    """adapters on all seven projections, seeded and lora_B non-zero: the same values in every replica (modules in name order)"""
    from hqq_amd.core.peft import PeftUtils, is_hqq_lora_layer
    cfg = {"r": tc.LORA_R, "lora_alpha": tc.LORA_ALPHA, "dropout": 0.0, "train_dtype": train_dtype}
    PeftUtils.add_lora(model, {t: dict(cfg) for t in TAGS})
    g = torch.Generator().manual_seed(7)
    wrapped = [(n, m) for n, m in model.named_modules() if is_hqq_lora_layer(m)]
    assert len(wrapped) == 2 * len(TAGS)
    for _, m in wrapped:
        m.lora_A.data = (torch.randn(m.lora_A.shape, generator=g) * 0.05).to(device="cuda", dtype=train_dtype)
        m.lora_B.data = (torch.randn(m.lora_B.shape, generator=g) * 0.05).to(device="cuda", dtype=train_dtype)
    return {n: p for n, p in model.named_parameters() if p.requires_grad}


def _loss(model, ids):
    logits = model(input_ids=ids).logits
    return F.cross_entropy(logits[:, :-1].float().reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))


def _sgd(model, params, ids):
    """the adapter gradients at the start, then STEPS plain SGD steps (no momentum) on the fixed batch: (gradients, losses before each step and after the last)"""
    first, losses = None, []
    for step in range(STEPS + 1):
        for p in params.values():
            p.grad = None
        loss = _loss(model, ids)
        losses.append(float(loss.detach()))
        if step == STEPS:
            break
        loss.backward()
        if first is None:
            first = {n: p.grad.double().clone() for n, p in params.items()}
        with torch.no_grad():
            for p in params.values():
                p -= LR * p.grad
    return first, losses


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _commit():
    try:
        return subprocess.check_output(["git", "describe", "--always", "--dirty"], cwd=ROOT, stderr=subprocess.DEVNULL, text=True).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("HQQ_AMD_COMMIT", "unknown (no git metadata beside the tree)")


def _write_tables():
    out = ["# Adapter gradients of a tiny Llama against a float64 replica", "",
           "Written by tests/test_train_gpu.py::test_whole_model_all_seven_projections_adapted.  hidden 256, 2 layers, batch (2, 12), r = 8 adapters on all",
           "seven projections, cross-entropy on the next token.  err = relative L2 error of a parameter's gradient against replica (b), a float64 torch-only",
           "model with eager attention holding the same dequantised weights; err_a is replica (a), the same torch-only model in the compute dtype, err_ours the",
           "quantised model.  The test requires err_ours <= 2 err_a + 2^-20 per parameter, and after three SGD steps (lr %g) dist_ours <= 2 dist_a over all" % LR,
           "adapters.", "", f"commit: {_commit()}", f"device: {torch.cuda.get_device_name(0)}", ""]
    for key in sorted(_TABLES):
        out += _TABLES[key] + [""]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "train_grad_errors.md"), "w") as f:
        f.write("\n".join(out))


@pytest.mark.parametrize("dn", list(tc.DTYPES))
@pytest.mark.parametrize("nbits", [4, 2])
def test_whole_model_all_seven_projections_adapted(ops, nbits, dn):
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    from hqq_amd.utils.model import quantize_model
    dt = tc.DTYPES[dn]
    ids = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(8)).cuda()
    ours = quantize_model(_tiny_llama(dt), BaseQuantizeConfig(nbits=nbits, group_size=64), compute_dtype=dt, device="cuda")
    rep_a, rep_b = _tiny_llama(dt), _tiny_llama(dt, attn="eager").double()
    quantised = [(n, m) for n, m in ours.named_modules() if isinstance(m, HQQLinear)]
    assert len(quantised) == 2 * len(TAGS)
    for n, m in quantised:   # both replicas hold the quantised model's own dequantised weights
        W = m.dequantize()
        rep_a.get_submodule(n).weight.data = W.clone()
        rep_b.get_submodule(n).weight.data = W.double()
    p_ours, p_a, p_b = _adapt(ours, torch.float32), _adapt(rep_a, torch.float32), _adapt(rep_b, torch.float64)
    assert list(p_ours) == list(p_a) == list(p_b) and len(p_ours) == 4 * len(TAGS)
    frozen = {n: p.detach().clone() for n, p in ours.named_parameters() if not p.requires_grad}
    for n, m in quantised:
        frozen[n + ".scale"], frozen[n + ".zero"] = m.meta["scale"].clone(), m.meta["zero"].clone()
    assert any(n.endswith("W_q") for n in frozen) and any("embed_tokens" in n for n in frozen) and any("norm" in n for n in frozen)

    g_ours, l_ours = _sgd(ours, p_ours, ids)
    g_a, l_a = _sgd(rep_a, p_a, ids)
    g_b, l_b = _sgd(rep_b, p_b, ids)

    rows = [f"## {nbits}-bit, {dn}", "", "| parameter | err_a | err_ours | bound 2 err_a + 2^-20 |", "|---|---|---|---|"]
    bad = []
    for n in p_ours:
        e_a, e_o = _rel(g_a[n], g_b[n]), _rel(g_ours[n], g_b[n])
        rows.append(f"| {n} | {e_a:.3e} | {e_o:.3e} | {2 * e_a + 2.0 ** -20:.3e} |")
        assert float(g_b[n].norm()) > 0
        if not e_o <= 2 * e_a + 2.0 ** -20:
            bad.append((n, e_a, e_o))
    cat = lambda ps: torch.cat([p.detach().double().reshape(-1) for p in ps.values()])
    d_a, d_o = _rel(cat(p_a), cat(p_b)), _rel(cat(p_ours), cat(p_b))
    fmt = lambda ls: " -> ".join(f"{v:.5f}" for v in ls)
    rows += ["", f"loss over {STEPS} SGD steps: ours {fmt(l_ours)}; (a) {fmt(l_a)}; (b) {fmt(l_b)}", "",
             f"final adapters, relative distance to (b): dist_a {d_a:.3e}, dist_ours {d_o:.3e}"]
    print("\n".join(rows))
    _TABLES[(nbits, dn)] = rows
    _write_tables()

    assert not bad, bad
    for name, ls in (("ours", l_ours), ("a", l_a), ("b", l_b)):
        assert all(b < a for a, b in zip(ls, ls[1:])), (name, ls)
    assert d_o <= 2 * d_a, (d_o, d_a)
    now = {n: p for n, p in ours.named_parameters() if not p.requires_grad}
    for n, m in quantised:
        now[n + ".scale"], now[n + ".zero"] = m.meta["scale"], m.meta["zero"]
    assert set(now) == set(frozen)
    for n, v in frozen.items():
        assert now[n].grad is None and now[n].dtype == v.dtype and torch.equal(now[n], v), n
    ours.eval()
    with_grad = ours(input_ids=ids).logits
    assert with_grad.requires_grad
    with torch.no_grad():
        assert torch.equal(ours(input_ids=ids).logits, with_grad.detach())
