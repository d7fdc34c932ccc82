"""CPU tests of the opt-in fp16 solver (the reference's GPU precision, optimize.py:231): the ABI 9 entry points reject any other
solver dtype without touching a device, every host layer defaults to the float32 solver, the keyword stays out of the quant config,
and the reference-written fixtures match their manifest."""
import hashlib
import inspect
import json
import os

import pytest

from conftest import GOLDEN

torch = pytest.importorskip("torch")

F32, F16, BF16 = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        _C.build()
    return _C.lib()


def test_abi_version_and_symbols(L):
    from hqq_amd import _C
    assert _C.ABI_VERSION == 9 and L.hqq_hip_abi_version() == 9
    for name in ("hqq_hip_quantize_solver", "hqq_hip_quantize_axis0_solver", "hqq_hip_optimize_solver"):
        assert name in _C.SYMBOLS and hasattr(L, name)


@pytest.mark.parametrize("solver_dtype", [BF16, 3, -1, 7])
def test_solver_dtype_is_an_argument_error_without_a_gpu(L, solver_dtype):
    # null pointers everywhere: the dtype check comes before anything would touch them
    rc = L.hqq_hip_quantize_solver(None, F16, 1024, 64, 15, 4, 1, 1, 20, 10.0, 0.7, solver_dtype, None, None, None, None, None, 0, None)
    assert rc == -3 and b"solver_dtype" in L.hqq_hip_last_error()
    rc = L.hqq_hip_quantize_axis0_solver(None, F16, 1024, 64, 15, 4, 1, 1, 20, 10.0, 0.7, solver_dtype, None, None, None, None, None, 0, None)
    assert rc == -3 and b"solver_dtype" in L.hqq_hip_last_error()
    rc = L.hqq_hip_optimize_solver(None, F16, 1024, 64, 1, 15, None, None, 20, 10.0, 0.7, solver_dtype, None, None, None, None, 0, None)
    assert rc == -3 and b"solver_dtype" in L.hqq_hip_last_error()


@pytest.mark.parametrize("solver_dtype", [F32, F16])
def test_accepted_solver_dtypes_reach_the_other_checks(L, solver_dtype):
    # F32 / F16 pass the dtype check: the next error is the missing workspace, the same for both
    rc = L.hqq_hip_quantize_solver(None, F16, 1024, 64, 15, 4, 1, 1, 20, 10.0, 0.7, solver_dtype, None, None, None, None, None, 0, None)
    assert rc == -5
    rc = L.hqq_hip_quantize_axis0_solver(None, F16, 1024, 64, 15, 4, 1, 1, 20, 10.0, 0.7, solver_dtype, None, None, None, None, None, 0, None)
    assert rc == -5
    # the same workspace serves both precisions
    assert L.hqq_hip_quantize_workspace_bytes(1024, 64, 20) > 0


def _default(fn, name="solver_dtype"):
    return inspect.signature(fn).parameters[name].default


def test_every_layer_defaults_to_the_float32_solver():
    from hqq_amd import ops
    from hqq_amd.core import optimize as opt
    from hqq_amd.core.quantize import HQQLinear, Quantizer
    from hqq_amd.utils.model import quantize_model
    for fn in (ops.quantize, ops.optimize, Quantizer.quantize, opt.optimize_weights_proximal_legacy, opt.optimize_weights_proximal_legacy_step,
               HQQLinear.__init__, HQQLinear.quantize, quantize_model):
        assert _default(fn) is torch.float32, fn.__qualname__


def test_solver_dtype_stays_out_of_the_config():
    from hqq_amd.core.quantize import BaseQuantizeConfig
    cfg = BaseQuantizeConfig(nbits=4, group_size=64)
    assert "solver_dtype" not in json.dumps({k: v for k, v in cfg.items()}, default=str)


@pytest.mark.parametrize("bad", [torch.bfloat16, torch.float64, "float16"])
def test_host_layers_reject_other_solver_dtypes_before_the_device(bad):
    from hqq_amd import ops
    from hqq_amd.core.quantize import Quantizer
    W = torch.zeros(64, 64)
    with pytest.raises(ValueError, match="solver_dtype"):
        ops.quantize(W, solver_dtype=bad)
    with pytest.raises(ValueError, match="solver_dtype"):
        ops.optimize(W, torch.ones(64, 1), torch.zeros(64, 1), 15, solver_dtype=bad)
    with pytest.raises(ValueError, match="solver_dtype"):
        Quantizer.quantize(W, device="cpu", solver_dtype=bad)


def test_fixtures_match_their_manifest():
    with open(os.path.join(GOLDEN, "MANIFEST_fp16solve.json")) as fh:
        man = json.load(fh)
    assert man["torch"] and man["cpu_capability"]
    files = man["files"]
    on_disk = sorted(f for f in os.listdir(GOLDEN) if f.startswith("qf16_") and f.endswith(".npz"))
    assert sorted(files) == on_disk and len(files) >= 40
    for f, digest in files.items():
        with open(os.path.join(GOLDEN, f), "rb") as fh:
            assert hashlib.sha256(fh.read()).hexdigest() == digest, f
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in files) < 3 << 20
