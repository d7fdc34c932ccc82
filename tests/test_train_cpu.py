"""tests/_train_cases.py judges itself, no GPU: an emulation of the documented arithmetic (fp32 accumulation in two summation orders, the stated
roundings) stays inside every derived bound on every case, so the GPU file cannot go red because of a bound; three planted defects (a weight row
dropped, `scaling` omitted, the LoRA branch missing from x.grad) leave it; the wrapper itself over a plain nn.Linear, run by autograd on the host,
stays inside the same bounds (the chain of roundings the bounds model is the one autograd performs); and the wrapper's options on nn.Linear bases."""
import numpy as np
import pytest
import torch
from torch import nn

import _train_cases as tc

R = 16   # the row cut-off the cases are built around; the GPU file reads the real one from hqq_amd.ops (tests/test_dgrad_cpu.py pins its value)


def _bf16_round(a32: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), returned as float32 (tests/test_dgrad_gpu.py)"""
    u = np.ascontiguousarray(a32, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def rnd(a32: torch.Tensor, dt) -> torch.Tensor:
    """one rounding of float32 values to dt, returned as float32"""
    if dt == torch.float32:
        return a32
    if dt == torch.float16:
        return a32.to(torch.float16).float()
    return torch.from_numpy(_bf16_round(a32.contiguous().numpy())).reshape(a32.shape)


def contract(a: torch.Tensor, b: torch.Tensor, order: str) -> torch.Tensor:
    """a @ b accumulated in fp32: the library's order, or 32-wide chunks added one after the other from the far end (an MFMA-like k loop, reversed)"""
    a, b = a.float(), b.float()
    if order == "lib":
        return a @ b
    acc = torch.zeros(a.shape[0], b.shape[1])
    for k in reversed(range(0, a.shape[1], 32)):
        acc = acc + a[:, k:k + 32] @ b[k:k + 32]
    return acc


def emu_dx(go, W, dt, order="lib"):
    return rnd(contract(go, W, order), dt)


def emu_lora(x, go, W, A, B, s, dt, Rt, mask, order="lib", defect=None):
    """the wrapper's backward as the module docstring of _train_cases states it, every product rounded to the train dtype Rt"""
    if defect == "row":
        W = W.clone()
        W[W.shape[0] // 2] = 0
    if defect == "scaling":
        s = 1.0
    mm = lambda a, b: rnd(contract(a, b, order), Rt)
    A, B = A.float(), B.float()
    xd = x.float() if mask is None else rnd(x.float() * mask.float(), Rt)
    h = mm(xd, A)
    gl = rnd(go.float() * s, Rt)
    dh = mm(gl, B.t())
    x_lora = mm(dh, A.t())
    if mask is not None:
        x_lora = rnd(x_lora * mask.float(), Rt)
    base = emu_dx(go, W, dt, order)
    xg = base if defect == "lora_x" else rnd(base + rnd(x_lora, dt), dt)
    return {"A": mm(xd.t(), dh), "B": mm(h.t(), gl), "bias": rnd(go.float().sum(0), Rt), "x_base": base, "x": xg}


def _case(N, K, dt, Rt, rows, masked, seed):
    W = tc.layer_weight(N, K, seed).to(dt)                     # synthetic dequantised weights of the layers' value range
    x, go = tc.randn((rows, K), seed + 1, dt), tc.randn((rows, N), seed + 2, dt)
    init = tc.lora_init(K, N, seed + 3)
    A, B = init["lora_A"].to(Rt), init["lora_B"].to(Rt)
    mask = tc.drop_mask((rows, K), seed + 4, Rt) if masked else None
    return x, go, W, A, B, mask


CASES = [(N, K, dn, Rt, rows, masked) for (N, K, _) in tc.SHAPES for dn in tc.DTYPES for Rt in (torch.float32, torch.bfloat16)
         for rows in (1, R, R + 1) for masked in (False, True) if not (Rt == torch.bfloat16 and dn == "f16")]
S = tc.LORA_ALPHA / tc.LORA_R


def test_the_weights_have_one_signed_groups_on_both_sides():
    for N, K, gs in tc.SHAPES:
        assert tc.one_signed_groups(tc.layer_weight(N, K, 1), gs, 1) == (True, True)
        # axis 0 groups are columns of the flat [gs, -1] view: each strides over every third of the rows, none is one-signed (finite meta only there)
        assert tc.one_signed_groups(tc.layer_weight(N, K, 1), gs, 0) == (False, False)
    assert tc.zero_point_kinds(torch.tensor([-0.5, 3.0]), 2) == (True, False) and tc.zero_point_kinds(torch.tensor([0.0, 3.5]), 2) == (False, True)


def test_bf16_round_is_the_cast():
    a = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3
    assert torch.equal(rnd(a, torch.bfloat16), a.to(torch.bfloat16).float())


@pytest.mark.parametrize("order", ["lib", "chunks"])
@pytest.mark.parametrize("N,K,dn,Rt,rows,masked", CASES)
def test_the_documented_arithmetic_stays_inside_every_bound(N, K, dn, Rt, rows, masked, order):
    dt = tc.DTYPES[dn]
    x, go, W, A, B, mask = _case(N, K, dt, Rt, rows, masked, seed=N + rows)
    ok, worst = tc.within(emu_dx(go, W, dt, order), tc.ref_dx(go, W), tc.bound_dx(go, W, dt))
    assert ok, worst
    ref, bnd = tc.ref_lora(x, go, W, A, B, S, mask), tc.bound_lora(x, go, W, A, B, S, dt, Rt, mask)
    got = emu_lora(x, go, W, A, B, S, dt, Rt, mask, order)
    for k in ("A", "B", "bias", "x_base", "x"):
        ok, worst = tc.within(got[k], ref[k], bnd[k])
        assert ok, (k, worst)


@pytest.mark.parametrize("N,K,dn,Rt,rows,masked", CASES)
def test_planted_defects_leave_the_bound(N, K, dn, Rt, rows, masked):
    dt = tc.DTYPES[dn]
    x, go, W, A, B, mask = _case(N, K, dt, Rt, rows, masked, seed=N + rows)
    ref, bnd = tc.ref_lora(x, go, W, A, B, S, mask), tc.bound_lora(x, go, W, A, B, S, dt, Rt, mask)
    row = emu_lora(x, go, W, A, B, S, dt, Rt, mask, defect="row")
    assert not tc.within(row["x_base"], tc.ref_dx(go, W), tc.bound_dx(go, W, dt))[0]        # bare layer
    assert not tc.within(row["x"], ref["x"], bnd["x"])[0]                                    # under a wrapper
    sc = emu_lora(x, go, W, A, B, S, dt, Rt, mask, defect="scaling")
    for k in ("A", "B", "x"):
        assert not tc.within(sc[k], ref[k], bnd[k])[0], k
    assert not tc.within(emu_lora(x, go, W, A, B, S, dt, Rt, mask, defect="lora_x")["x"], ref["x"], bnd["x"])[0]


class _FixedDrop(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return x * self.m


@pytest.mark.parametrize("dn,Rt,masked,train_bias", [("bf16", torch.float32, False, False), ("bf16", torch.float32, True, True),
                                                    ("bf16", torch.bfloat16, True, True), ("f16", torch.float32, True, False)])
def test_autograd_through_the_wrapper_performs_the_documented_chain(dn, Rt, masked, train_bias):
    """HQQLinearLoRA over nn.Linear on the host: the gradients autograd computes stay inside the bounds (what the GPU file asks of the quantised layer)"""
    from hqq_amd.core.peft import HQQLinearLoRA
    dt, (N, K, _) = tc.DTYPES[dn], tc.SHAPES[0]
    x0, go0, W, A, B, mask = _case(N, K, dt, Rt, R + 1, masked, seed=7)
    lin = nn.Linear(K, N, bias=True).to(dt)
    lin.weight.data = W.clone()
    lora = HQQLinearLoRA(lin, {"r": tc.LORA_R, "lora_alpha": tc.LORA_ALPHA, "dropout": tc.P_DROP if masked else 0.0, "train_dtype": Rt,
                               "train_bias": train_bias, "lora_init": {"lora_A": A, "lora_B": B}})
    if masked:
        lora.peft_drop = _FixedDrop(mask)
    x = x0.clone().requires_grad_(True)
    y = lora(x)
    y.retain_grad()
    (y.float() * go0.float()).sum().backward()
    go = y.grad
    ref, bnd = tc.ref_lora(x0, go, W, A, B, S, mask), tc.bound_lora(x0, go, W, A, B, S, dt, Rt, mask)
    got = {"A": lora.lora_A.grad, "B": lora.lora_B.grad, "x": x.grad}
    if train_bias:
        got["bias"] = lora.bias.grad
    else:
        assert lora.bias.grad is None
    for k, g in got.items():
        ok, worst = tc.within(g, ref[k], bnd[k])
        assert ok, (k, worst)
    assert x.grad.dtype == dt and lora.lora_A.grad.dtype == Rt and lora.lora_B.grad.dtype == Rt


def _plain(bias, **cfg):
    from hqq_amd.core.peft import HQQLinearLoRA
    torch.manual_seed(0)
    init = tc.lora_init(64, 32, 5)
    return HQQLinearLoRA(nn.Linear(64, 32, bias=bias), {"r": tc.LORA_R, "lora_alpha": tc.LORA_ALPHA, "lora_init": init, **cfg})


def test_dropout_builds_nn_dropout_and_eval_turns_it_off():
    x = tc.randn((5, 64), 1)
    lora, plain = _plain(True, dropout=tc.P_DROP), _plain(True, dropout=0.0)
    assert isinstance(lora.peft_drop, nn.Dropout) and lora.peft_drop.p == tc.P_DROP and isinstance(plain.peft_drop, nn.Identity)
    with torch.no_grad():
        lora.train()
        torch.manual_seed(1)
        assert not torch.equal(lora(x), plain(x))
        lora.eval()
        assert torch.equal(lora(x), plain(x))


def test_train_bias_on_a_bias_free_layer_creates_a_zero_trainable_bias_in_train_dtype():
    for Rt in (torch.float32, torch.bfloat16):
        lora = _plain(False, train_bias=True, train_dtype=Rt)
        assert isinstance(lora.bias, nn.Parameter) and lora.bias.requires_grad and lora.bias.dtype == Rt
        assert tuple(lora.bias.shape) == (32,) and not bool(lora.bias.any())
    assert _plain(False).bias is None
    frozen = _plain(True).bias
    assert isinstance(frozen, nn.Parameter) and not frozen.requires_grad


def test_train_dtype_bf16_gives_bf16_adapters():
    lora = _plain(True, train_dtype=torch.bfloat16)
    assert lora.lora_A.dtype == torch.bfloat16 and lora.lora_B.dtype == torch.bfloat16 and lora.lora_A.requires_grad and lora.lora_B.requires_grad
    assert _plain(True).lora_A.dtype == torch.float32
