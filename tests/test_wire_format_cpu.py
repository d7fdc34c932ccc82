"""CPU tests of the checkpoint wire format, both directions.

* tests/golden/ours_sd_cfg1_4b.npz is hqq_amd.HQQLinear.state_dict() of the BASELINE configs[0] layer, written ON AN MI355X by
  tests/golden/make_ours_state_dict.py (HIP solver + packer).  tests/golden/refload_ours_cfg1_4b.npz holds what the REFERENCE's
  HQQLinear computes after loading it (tests/golden/make_refload_golden.py): nothing here imports the reference at run time.
* independent of the reference being present: the file carries exactly the keys / dtypes / shapes of the reference's own
  state_dict (tests/golden/refsd_cfg1_4b.npz, written by the reference), and — the solver being bit-exact — the same bytes.
"""
import hashlib

import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")


def _sd(g):
    sd = {}
    for k in g:
        if k.startswith("sd__"):
            name = k[4:]
            dt = getattr(torch, bytes(g["dt__" + name]).decode().split(".")[1])
            t = torch.from_numpy(np.array(g[k]))
            sd[name] = t.view(torch.bfloat16) if dt == torch.bfloat16 else t.to(dt)
    return sd


def test_our_state_dict_is_the_reference_schema_and_the_reference_bytes():
    ours, ref = _sd(load_golden("ours_sd_cfg1_4b")), _sd(load_golden("refsd_cfg1_4b"))
    assert set(ours) == set(ref)
    for k in ref:
        assert ours[k].dtype == ref[k].dtype and ours[k].shape == ref[k].shape, k
        assert torch.equal(ours[k], ref[k]), f"{k}: the HIP-written checkpoint differs from the reference-written one"


def test_the_reference_loads_our_state_dict_and_its_own_forward_agrees(oracle):
    g, r, gr = load_golden("ours_sd_cfg1_4b"), load_golden("refload_ours_cfg1_4b"), load_golden("refsd_cfg1_4b")
    sd = _sd(g)
    N, K = (int(v) for v in sd["shape"])
    nbits, gs = int(sd["nbits"]), int(sd["group_size"])
    # our checkpoint's tensors, dequantised here by the C oracle, are the weights the reference rebuilt from it (and from its own checkpoint)
    Wd = oracle.dequantize(nbits, sd["W_q"].numpy(), sd["scale"].numpy(), sd["zero"].numpy(), N, K, gs, oracle.F16)
    wsha = hashlib.sha256(np.ascontiguousarray(Wd).tobytes()).hexdigest().encode()
    assert wsha == r["Wdeq_sha256_f16"].tobytes(), "the oracle's weights from our checkpoint differ from the reference's"
    assert wsha == gr["Wdeq_sha256_f16"].tobytes(), "our checkpoint does not rebuild the reference checkpoint's weights"
    # the reference's CPU forward on OUR checkpoint vs the oracle's forward, vs our fused GPU forward on it, and vs the reference's forward on ITS checkpoint
    y = r["y_f16"].astype(np.float32)
    yo, _ = oracle.matmul(oracle.to_cd(g["x_f32"], oracle.F16), Wd, sd["bias"].numpy(), oracle.F16)
    np.testing.assert_allclose(yo.astype(np.float32), y, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(y, g["y_f16"].astype(np.float32), rtol=1e-3, atol=1e-3)
    # ... and, in the process that wrote the fixture, the reference's forward on its own checkpoint: same bytes in, same bits out.  (The stored
    # y_f16 of refsd_cfg1_4b.npz is compared with a tolerance only: torch's fp16 CPU matmul sums in a host-dependent order — core count,
    # ISA — and that fixture was written on another host.)
    assert np.array_equal(r["y_f16"].view(np.uint16), r["y_refsd_f16"].view(np.uint16)), "same checkpoint bytes must give the reference the same output bits"
    np.testing.assert_allclose(y, gr["y_f16"].astype(np.float32), rtol=1e-3, atol=1e-3)
