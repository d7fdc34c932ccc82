#!/usr/bin/env python3
"""Generate the fp16-solver fixtures (tests/golden/qf16_*.npz, MANIFEST_fp16solve.json) by running the REFERENCE itself
(mobiusml/hqq, imported read-only as make_golden.py does) on the CPU.

    python tests/golden/make_fp16solve_golden.py      # needs the reference checkout (HQQ_REFERENCE); writes tests/golden/qf16_*

The reference solves in fp16 when it quantises on a GPU: optimize_weights_proximal_legacy picks
`dtype = float16 if device.type == "cuda" else float32` (optimize.py:231).  That test chooses nothing else on the path
(torch.cuda.empty_cache() is a no-op without CUDA), so `fp16_solver()` below rebinds the module's `float32` to torch.float16
and the CPU run takes the GPU's precision: W_f / scale / zero in fp16, every eager op rounded once to fp16, torch.mean summed
in float32 by ATen's CPU kernels.  best_error becomes fp16 too, which changes no comparison (the errors are fp16 already).
The reduction order torch-ROCm would use on a GPU is NOT what these files pin: only the CPU's.

Fixture families (every array an output of hqq/core/{quantize,optimize}.py, untouched)
  qf16_<tag>.npz                 Quantizer.quantize(..., device="cpu") under fp16_solver(): input W (+ its dtype), packed W_q, fp16
                                 scale (= 1/scale) and zero, the solver's iteration count; quant_* shapes and edge cases, every width
                                 of SUPPORTED_BITS, gs 8 ... 4096, axis 0, fp16 / bf16 input
  qf16_step_<tag>.npz            one optimize_weights_proximal_legacy_step on fp16 operands (W_r, W_q, new zero)
  qf16_overflow_4b.npz           a group whose W * scale overflows fp16: its zero is NaN, the whole layer stops after one iteration
                                 (nan_groups lists it)
  qf16_cfg2_4096_<nbits>b.npz    sha256 of W_q / zero / scale of the 4096 x 4096 configs[1] layer (as cfg2_*), 4 / 3 / 2 bits
  qf16_cfg2_11008x4096_4b.npz    the same for an 11008 x 4096 MLP-sized layer, 4 bits
  qf16_refsd_cfg1_4b_<cd>.npz    the reference's HQQLinear(..., device="cpu").state_dict() of the configs[0] layer, fp16 / bf16:
                                 sha256 + dtype + shape of every entry, the entries below 64 Ki elements in full
"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference, raw, sha  # noqa: E402

FILES = []


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    FILES.append(name + ".npz")
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.0f} KiB")


def h(a) -> np.ndarray:
    return np.frombuffer(sha(a).encode(), np.uint8)


def main():
    Quantizer, HQQLinear, BaseQuantizeConfig, _ = _import_reference()
    import hqq.core.optimize as ropt
    torch.set_num_threads(os.cpu_count() or 1)
    calls = [0]
    step0 = ropt.optimize_weights_proximal_legacy_step

    def counted_step(*a, **k):
        calls[0] += 1
        return step0(*a, **k)

    @contextlib.contextmanager
    def fp16_solver():
        saved = ropt.float32
        ropt.float32 = torch.float16
        ropt.optimize_weights_proximal_legacy_step = counted_step
        calls[0] = 0
        try:
            yield
        finally:
            ropt.float32 = saved
            ropt.optimize_weights_proximal_legacy_step = step0

    def quantize(W, nbits, gs, axis):
        with fp16_solver():
            Wq, meta = Quantizer.quantize(W.clone(), nbits=nbits, group_size=gs, axis=axis, round_zero=(nbits == 4),
                                          optimize=True, device="cpu", compute_dtype=torch.float16)
        assert meta["scale"].dtype == torch.float16 and meta["zero"].dtype == torch.float16
        return Wq, meta, calls[0]

    def case(tag, W, nbits, gs, axis=1):
        Wq, meta, n = quantize(W, nbits, gs, axis)
        save(tag, W=raw(W), in_dtype=np.array(str(W.dtype).replace("torch.", "")), nbits=np.array(float(nbits)), gs=np.array(gs),
             axis=np.array(axis), Wq_packed=Wq.numpy(), scale_f16=raw(meta["scale"]), zero_f16=raw(meta["zero"]), iters_run=np.array(n))

    widths = {8: "8", 6: "6", 5: "5", 4: "4", 3: "3", 2: "2", 1.58: "1p58", 1: "1"}
    for nbits, nm in widths.items():
        torch.manual_seed(0)
        lin = torch.nn.Linear(256, 64, bias=False)
        case(f"qf16_{nm}b_64x256", lin.weight.data.clone(), nbits, 64)

    torch.manual_seed(0)
    Wn = (torch.randn(16, 2048) * 0.02).half()            # fp16 input
    for nbits in (4, 3, 2):
        case(f"qf16_{nbits}b_16x2048_normal", Wn, nbits, 64)
    torch.manual_seed(9)
    case("qf16_4b_64x512_bf16", (torch.randn(64, 512) * 0.02).bfloat16(), 4, 64)   # bf16 input (-> float32 -> fp16 in the solver)

    torch.manual_seed(3)                                   # the quant_*_edge tensor of make_golden.py
    We = torch.randn(16, 128) * 0.05
    We[0, :64] = 0.125
    We[1, :64] = 0.0
    We[2, :64] = 1.0 + torch.arange(64) * 1e-6
    We[3, :64] = torch.linspace(0, 3e-4, 64)
    We[4, 5] = 40.0
    We[5, :64] = torch.arange(64) * 0.5
    for nbits in (4, 3, 2):
        case(f"qf16_{nbits}b_16x128_edge", We, nbits, 64)

    torch.manual_seed(5)
    Wg = torch.randn(32, 256) * 0.1
    for gs in (8, 16, 32, 128, 256):
        case(f"qf16_4b_32x256_gs{gs}", Wg, 4, gs)
    torch.manual_seed(6)
    Wl = (torch.randn(8, 4096) * 0.05).half()       # (fp16 input: half the bytes)
    for gs in (512, 1024, 4096):
        case(f"qf16_4b_8x4096_gs{gs}", Wl, 4, gs)
    case("qf16_2b_8x4096_gs2048", Wl, 2, 2048)

    torch.manual_seed(11)
    Wa = torch.randn(64, 256) * 0.05
    for nbits in (4, 3, 2, 8):
        case(f"qf16_axis0_{nbits}b_64x256", Wa, nbits, 64, axis=0)
    torch.manual_seed(12)
    case("qf16_axis0_4b_32x80", torch.randn(32, 80) * 0.05, 4, 64, axis=0)
    case("qf16_axis0_4b_96x72_gs8", torch.randn(96, 72) * 0.05, 4, 8, axis=0)
    case("qf16_axis0_4b_128x256_gs128", torch.randn(128, 256) * 0.05, 4, 128, axis=0)
    torch.manual_seed(13)
    case("qf16_axis0_4b_64x256_f16", (torch.randn(64, 256) * 0.02).half(), 4, 64, axis=0)

    # W * scale overflows fp16 in group 3 (values in [100, 100.001]: scale = 15 / 0.001 = 1.5e4, W * scale = 1.5e6 -> inf, zero NaN)
    torch.manual_seed(14)
    Wo = torch.randn(16, 128) * 0.05
    Wo[1, 64:] = 100.0 + torch.linspace(0, 1e-3, 64)
    Wq, meta, n = quantize(Wo, 4, 64, 1)
    nan_groups = np.nonzero(np.isnan(meta["zero"].float().numpy().reshape(-1)))[0]
    assert list(nan_groups) == [3] and n == 1, (nan_groups, n)
    save("qf16_overflow_4b", W=raw(Wo), in_dtype=np.array("float32"), nbits=np.array(4.0), gs=np.array(64), axis=np.array(1),
         Wq_packed=Wq.numpy(), scale_f16=raw(meta["scale"]), zero_f16=raw(meta["zero"]), iters_run=np.array(n), nan_groups=nan_groups)

    # one step on fp16 operands, as the fp16 solver calls it (optimize.py:201-206)
    torch.manual_seed(17)
    Wg = (torch.randn(384, 64) * 0.03)
    max_v = 15
    _min, _max = Wg.min(axis=1, keepdim=True)[0], Wg.max(axis=1, keepdim=True)[0]
    scale = (max_v / (_max - _min)).clamp(max=2e4)
    zero = torch.round(-_min * scale)
    W16, s16, z16 = Wg.half(), scale.half(), zero.half()
    W_r, W_q, zero_out, scale_out = step0(W16.clone(), s16.clone(), z16.clone(), [0, max_v], 1e1, 0.7, 1)
    assert zero_out.dtype == torch.float16 and torch.equal(scale_out, s16)
    save("qf16_step_4b_axis1_384x64", W=raw(W16), scale_in=raw(s16), zero_in=raw(z16), axis=np.array(1), max_v=np.array(max_v),
         beta=np.array(1e1), lp_norm=np.array(0.7), W_r=raw(W_r), W_q=W_q.numpy().astype(np.uint8), zero_out=raw(zero_out))

    # full-size layers: hashes only
    torch.manual_seed(0)
    W2 = (torch.randn(4096, 4096) * 0.02).half()
    for nbits in (4, 3, 2):
        Wq, meta, n = quantize(W2, nbits, 64, 1)
        save(f"qf16_cfg2_4096_{nbits}b", W_sha256=h(raw(W2)), W_head=raw(W2)[:2, :8].copy(), Wq_sha256=h(Wq.numpy()),
             zero_sha256=h(raw(meta["zero"])), scale_sha256=h(raw(meta["scale"])), Wq_head=Wq.numpy()[:4, :16].copy(),
             zero_head=raw(meta["zero"]).reshape(-1)[:16].copy(), scale_head=raw(meta["scale"]).reshape(-1)[:16].copy(), iters_run=np.array(n))
    torch.manual_seed(0)
    W3 = (torch.randn(11008, 4096) * 0.02).half()
    Wq, meta, n = quantize(W3, 4, 64, 1)
    save("qf16_cfg2_11008x4096_4b", W_sha256=h(raw(W3)), W_head=raw(W3)[:2, :8].copy(), Wq_sha256=h(Wq.numpy()),
         zero_sha256=h(raw(meta["zero"])), scale_sha256=h(raw(meta["scale"])), Wq_head=Wq.numpy()[:4, :16].copy(),
         zero_head=raw(meta["zero"]).reshape(-1)[:16].copy(), scale_head=raw(meta["scale"]).reshape(-1)[:16].copy(), iters_run=np.array(n))

    # the reference's state_dict of the configs[0] layer (make_golden.py's refsd_cfg1_4b, with the fp16 solver)
    for cdn, cd in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        torch.manual_seed(0)
        lin = torch.nn.Linear(1024, 1024, bias=True)
        arrs = {"W_sha256": h(lin.weight.data.numpy())}
        with fp16_solver():
            layer = HQQLinear(lin, BaseQuantizeConfig(nbits=4, group_size=64, axis=1), compute_dtype=cd, device="cpu")
        for k, v in layer.state_dict().items():   # every entry by its bytes' sha256 (+ dtype, shape); the small ones in full as well
            assert isinstance(v, torch.Tensor), (k, type(v))
            arrs["sha__" + k] = h(raw(v))
            arrs["dt__" + k] = np.frombuffer(str(v.dtype).encode(), np.uint8)
            arrs["shape__" + k] = np.array(v.shape, dtype=np.int64)
            if v.numel() <= 65536:
                arrs["sd__" + k] = raw(v)
        save(f"qf16_refsd_cfg1_4b_{cdn}", **arrs)

    manifest = {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
                "reference": "mobiusml/hqq v0.2.8.post1, optimize_weights_proximal_legacy with dtype float16 (its GPU precision) on the CPU",
                "files": {f: hashlib.sha256(open(os.path.join(HERE, f), "rb").read()).hexdigest() for f in sorted(FILES)}}
    with open(os.path.join(HERE, "MANIFEST_fp16solve.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print("wrote MANIFEST_fp16solve.json")


if __name__ == "__main__":
    main()
