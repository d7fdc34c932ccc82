"""GPU tests of the opt-in fp16 solver (solver_dtype=torch.float16: the reference's GPU precision, optimize.py:231) against fixtures
the reference itself wrote with its fp16 solver on the CPU (tests/golden/make_fp16solve_golden.py): every level, every zero bit, every
scale bit and the iteration count, for axis 1 and axis 0, the standalone optimize and step entry points, the full-size layers by
sha256, and HQQLinear's state_dict byte for byte.  The float32 solver through the new entry points is the old one, bit for bit."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

QF16 = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("qf16_") and f.endswith(".npz")
              and not f.startswith(("qf16_cfg2_", "qf16_refsd_", "qf16_step_", "qf16_overflow_")))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from hqq_amd import ops as o
    assert o.is_available(), "libhqq_hip.so must load on the GPU box (no fallback)"
    return o


def _W(g) -> torch.Tensor:
    """the fixture's input in its own dtype (float32 / float16 / bfloat16 stored as its raw uint16)"""
    a = np.ascontiguousarray(g["W"])
    if str(g["in_dtype"]) == "bfloat16":
        return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(a)


def _nbits(g):
    nb = float(g["nbits"])
    return int(nb) if nb.is_integer() else nb


def _u16(t) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint16)


def _sha(a) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest().encode()


@pytest.mark.parametrize("name", QF16)
def test_fp16_solver_equals_the_reference(ops, name):
    g = load_golden(name)
    nbits, gs, axis = _nbits(g), int(g["gs"]), int(g["axis"])
    Wq, s, z, info = ops.quantize(_W(g).cuda(), nbits=nbits, group_size=gs, round_zero=(nbits == 4), axis=axis, return_info=True,
                                  solver_dtype=torch.float16)
    assert s.dtype == torch.float16 and z.dtype == torch.float16
    pb = ops.PACK_BITS[nbits]
    rows = g["W"].size // gs if axis == 1 else gs
    got = ops.unpack(pb, Wq).cpu().numpy()[:rows]
    want = ops.unpack(pb, torch.from_numpy(g["Wq_packed"]).cuda()).cpu().numpy()[:rows]
    nbad = int((got != want).sum())
    nz = int((_u16(z) != g["zero_f16"].reshape(-1).view(np.uint16)).sum())
    ns = int((_u16(s) != g["scale_f16"].reshape(-1).view(np.uint16)).sum())
    ran = int(info[0].item())
    assert (nbad, nz, ns) == (0, 0, 0), f"{nbad} levels / {nz} zero-points / {ns} scales differ from the reference's fp16 solver"
    assert np.array_equal(Wq.cpu().numpy(), g["Wq_packed"])
    assert ran == int(g["iters_run"]), f"{ran} iterations, the reference ran {int(g['iters_run'])}"


@pytest.mark.parametrize("name", ["qf16_4b_64x256", "qf16_3b_16x2048_normal", "qf16_4b_8x4096_gs1024", "qf16_axis0_4b_64x256",
                                  "qf16_axis0_4b_96x72_gs8"])
def test_standalone_optimize_equals_the_reference(ops, name):
    """optimize_weights_proximal_legacy on its own, from the reference's float32 start (quantize.py:118-134, computed on the CPU as the
    reference does it): the levels and zero-points of the fused quantiser's fixture"""
    from hqq_amd.core.optimize import optimize_weights_proximal_legacy
    g = load_golden(name)
    nbits, gs, axis = _nbits(g), int(g["gs"]), int(g["axis"])
    W = _W(g).float()
    W = W.reshape([-1, gs]) if axis == 1 else W.reshape([gs, -1])
    max_v = round(2 ** nbits - 1)
    _min, _max = W.min(axis=axis, keepdim=True)[0], W.max(axis=axis, keepdim=True)[0]
    denom = _max - _min
    scale = max_v / denom
    scale = torch.where(denom.abs() <= 1e-4, torch.full_like(scale, 1.0), scale).clamp(max=2e4)
    zero = -_min * scale
    if nbits == 4:
        zero = torch.round(zero)
    W_q, scale_out, zero_out = optimize_weights_proximal_legacy(W.cuda(), scale.cuda(), zero.cuda(), [0, max_v], axis=axis,
                                                                solver_dtype=torch.float16)
    assert scale_out.dtype == torch.float16 and zero_out.dtype == torch.float16
    pb = ops.PACK_BITS[nbits]
    want = ops.unpack(pb, torch.from_numpy(g["Wq_packed"]).cuda()).cpu().numpy()[:W.shape[0]]
    assert np.array_equal(W_q.cpu().numpy().astype(np.uint8), want)
    assert np.array_equal(_u16(zero_out), g["zero_f16"].reshape(-1).view(np.uint16))
    # the info the standalone entry point reports: the reference's iteration count
    _, _, info = ops.optimize(W.cuda(), scale.cuda(), zero.cuda(), max_v, axis=axis, return_info=True, solver_dtype=torch.float16)
    assert int(info[0].item()) == int(g["iters_run"])


def test_one_step_equals_the_reference(ops):
    from hqq_amd.core.optimize import optimize_weights_proximal_legacy_step
    g = load_golden("qf16_step_4b_axis1_384x64")
    W, s, z = (torch.from_numpy(g[k]).cuda() for k in ("W", "scale_in", "zero_in"))
    W_r, W_q, zero, scale = optimize_weights_proximal_legacy_step(W, s, z, [0, int(g["max_v"])], float(g["beta"]), float(g["lp_norm"]),
                                                                  int(g["axis"]), solver_dtype=torch.float16)
    assert W_r.dtype == W_q.dtype == zero.dtype == scale.dtype == torch.float16
    assert np.array_equal(_u16(W_r), g["W_r"].reshape(-1).view(np.uint16))
    assert np.array_equal(W_q.cpu().numpy().astype(np.uint8), g["W_q"])
    assert np.array_equal(_u16(zero), g["zero_out"].reshape(-1).view(np.uint16))


def test_overflowing_group_stops_the_layer_after_one_iteration(ops):
    g = load_golden("qf16_overflow_4b")
    gs, R = int(g["gs"]), g["W"].size // int(g["gs"])
    Wq, s, z, info = ops.quantize(_W(g).cuda(), nbits=4, group_size=gs, round_zero=True, return_info=True, solver_dtype=torch.float16)
    assert int(info[0].item()) == 1 == int(g["iters_run"])
    nan = np.isnan(z.float().cpu().numpy().reshape(-1))
    assert list(np.nonzero(nan)[0]) == list(g["nan_groups"])
    ok = ~nan
    # levels, not packed bytes: a packed byte mixes rows (groups) and the NaN group's levels are not defined
    got = ops.unpack(4, Wq).cpu().numpy()[:R]
    want = ops.unpack(4, torch.from_numpy(g["Wq_packed"]).cuda()).cpu().numpy()[:R]
    assert np.array_equal(got[ok], want[ok])
    assert np.array_equal(_u16(z)[ok], g["zero_f16"].reshape(-1).view(np.uint16)[ok])
    assert np.array_equal(_u16(s), g["scale_f16"].reshape(-1).view(np.uint16))


@pytest.mark.parametrize("name,shape,nbits", [("qf16_cfg2_4096_4b", (4096, 4096), 4), ("qf16_cfg2_4096_3b", (4096, 4096), 3),
                                              ("qf16_cfg2_4096_2b", (4096, 4096), 2), ("qf16_cfg2_11008x4096_4b", (11008, 4096), 4)])
def test_full_size_layers_equal_the_reference(ops, name, shape, nbits):
    g = load_golden(name)
    torch.manual_seed(0)
    W = (torch.randn(*shape) * 0.02).half()
    assert _sha(W.numpy()) == g["W_sha256"].tobytes(), "torch's CPU RNG stream differs from the fixture's"
    Wq, s, z, info = ops.quantize(W.cuda(), nbits=nbits, group_size=64, round_zero=(nbits == 4), return_info=True, solver_dtype=torch.float16)
    assert int(info[0].item()) == int(g["iters_run"])
    assert _sha(z.cpu().numpy()) == g["zero_sha256"].tobytes()
    assert _sha(s.cpu().numpy()) == g["scale_sha256"].tobytes()
    assert _sha(Wq.cpu().numpy()) == g["Wq_sha256"].tobytes()


@pytest.mark.parametrize("cdn,cd", [("f16", torch.float16), ("bf16", torch.bfloat16)])
def test_hqqlinear_state_dict_is_the_references(ops, cdn, cd):
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear
    g = load_golden(f"qf16_refsd_cfg1_4b_{cdn}")
    torch.manual_seed(0)
    lin = torch.nn.Linear(1024, 1024, bias=True)
    assert _sha(lin.weight.data.numpy()) == g["W_sha256"].tobytes()
    layer = HQQLinear(lin, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=cd, device="cuda", solver_dtype=torch.float16)
    sd = layer.state_dict()
    keys = sorted(k[len("sha__"):] for k in g if k.startswith("sha__"))
    assert sorted(sd) == keys
    for k in keys:
        v = sd[k]
        assert str(v.dtype).encode() == g["dt__" + k].tobytes(), k
        assert list(v.shape) == g["shape__" + k].tolist(), k
        t = v.detach().cpu().contiguous()
        a = t.view(torch.uint16).numpy() if t.dtype == torch.bfloat16 else t.numpy()
        assert _sha(a) == g["sha__" + k].tobytes(), k
        if "sd__" + k in g:
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(g["sd__" + k]).tobytes(), k


@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("wdt", [torch.float32, torch.float16, torch.bfloat16])
def test_f32_through_the_new_entry_points_is_the_old_solver(ops, axis, wdt):
    from hqq_amd import _C
    W = (torch.randn(512, 1024, generator=torch.Generator().manual_seed(3)) * 0.02).to(wdt).cuda()
    Wq, s, z, info = ops.quantize(W, nbits=4, group_size=64, round_zero=True, axis=axis, return_info=True, solver_dtype=torch.float32)
    # the unchanged ABI 8 entry point, called directly
    Wq0, s0, z0, info0 = torch.empty_like(Wq), torch.empty_like(s), torch.empty_like(z), torch.zeros_like(info)
    L = _C.lib()
    ws = torch.empty((L.hqq_hip_quantize_workspace_bytes(W.numel(), 64, 20),), dtype=torch.uint8, device="cuda")
    fn = L.hqq_hip_quantize if axis == 1 else L.hqq_hip_quantize_axis0
    rc = fn(W.data_ptr(), ops._dt(wdt), W.numel(), 64, 15, 4, 1, 1, 20, 10.0, 0.7, Wq0.data_ptr(), s0.data_ptr(), z0.data_ptr(),
            info0.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _C.check(rc, "hqq_hip_quantize")
    torch.cuda.synchronize()
    assert s.dtype == z.dtype == torch.float32
    assert torch.equal(Wq, Wq0) and torch.equal(info, info0)
    assert torch.equal(s.view(torch.int32), s0.view(torch.int32)) and torch.equal(z.view(torch.int32), z0.view(torch.int32))
    # and the fp16 solver is a different computation on the same input (the gap the keyword exists for)
    Wq16, s16, z16 = ops.quantize(W, nbits=4, group_size=64, round_zero=True, axis=axis, solver_dtype=torch.float16)
    assert s16.dtype == z16.dtype == torch.float16
    assert not torch.equal(z16.float(), z)


def test_optimize_false_and_tensorwise_ignore_the_solver_dtype(ops):
    from hqq_amd.core.quantize import Quantizer
    W = (torch.randn(128, 256, generator=torch.Generator().manual_seed(4)) * 0.02).half().cuda()
    for kw in ({"optimize": False}, {"channel_wise": False}):
        a, ma = Quantizer.quantize(W, nbits=4, group_size=64, axis=1, **kw)
        b, mb = Quantizer.quantize(W, nbits=4, group_size=64, axis=1, solver_dtype=torch.float16, **kw)
        assert torch.equal(a, b) and mb["scale"].dtype == ma["scale"].dtype == torch.float32
        assert torch.equal(ma["scale"], mb["scale"]) and torch.equal(ma["zero"], mb["zero"])


def test_quantize_model_with_the_fp16_solver():
    pytest.importorskip("transformers")
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.core.quantize import BaseQuantizeConfig, HQQLinear, Quantizer
    from hqq_amd.utils.model import quantize_model
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).half().cuda().eval()
    W0 = model.model.layers[1].mlp.down_proj.weight.data.clone()
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64), compute_dtype=torch.float16, device="cuda", solver_dtype=torch.float16)
    layers = [m for m in model.modules() if isinstance(m, HQQLinear)]
    assert len(layers) == 2 * 7 and all(m.solver_dtype == torch.float16 for m in layers)
    down = model.model.layers[1].mlp.down_proj
    ref_q, ref_meta = Quantizer.quantize(W0, nbits=4, group_size=64, axis=1, round_zero=True, solver_dtype=torch.float16)
    assert ref_meta["zero"].dtype == torch.float16
    assert torch.equal(down.W_q.data, ref_q) and torch.equal(down.meta["zero"].reshape(-1), ref_meta["zero"].reshape(-1))
    with torch.no_grad():
        logits = model(torch.randint(0, 512, (1, 8), device="cuda")).logits
    assert torch.isfinite(logits).all()


@pytest.mark.parametrize("op", ["pow", "scalar_mul"])
def test_rocm_fp16_ops_equal_the_cpu_ones_over_every_finite_half(op):
    """The premise under the CPU-written fixtures: torch-ROCm's fp16 `out.pow(lp_norm - 1)` and `(1.0 / beta) * out` (optimize.py:104)
    give the CPU's bits for every finite fp16 input, so the reference's GPU solver differs from these fixtures at most by its own
    reduction order (which is not pinned here)."""
    h = torch.from_numpy(np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).copy())
    h = h[torch.isfinite(h)]
    fn = (lambda t: t.pow(0.7 - 1)) if op == "pow" else (lambda t: (1.0 / 10.0) * t)
    c, g = fn(h), fn(h.cuda()).cpu()
    same = (c.view(torch.int16) == g.view(torch.int16)) | (torch.isnan(c) & torch.isnan(g))
    assert int((~same).sum()) == 0
