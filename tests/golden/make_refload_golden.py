#!/usr/bin/env python3
"""Write tests/golden/refload_ours_cfg1_4b.npz: what the REFERENCE (mobiusml/hqq) computes from OUR checkpoint.

tests/golden/ours_sd_cfg1_4b.npz is hqq_amd.HQQLinear.state_dict() of the BASELINE configs[0] layer as this build emits it
(tests/golden/make_ours_state_dict.py).  This script loads it into the reference's own HQQLinear (HQQBackend.PYTORCH, CPU) and
records, in one process:
  Wdeq_sha256_f16   sha256 of the reference's dequantize() of our checkpoint (elementwise fp16 ops: host-independent)
  y_f16             the reference's forward on our checkpoint, x = x_f32 of ours_sd_cfg1_4b.npz
  y_refsd_f16       the reference's forward on ITS OWN checkpoint (refsd_cfg1_4b.npz), same x, same process
tests/test_wire_format_cpu.py checks these without the reference: the reference is needed only to regenerate the file.

    HQQ_REFERENCE=<checkout of mobiusml/hqq> python tests/golden/make_refload_golden.py
"""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "refload_ours_cfg1_4b"


def _sd(g):
    sd = {}
    for k in g:
        if k.startswith("sd__"):
            name = k[4:]
            dt = getattr(torch, bytes(g["dt__" + name]).decode().split(".")[1])
            t = torch.from_numpy(np.array(g[k]))
            sd[name] = t.view(torch.bfloat16) if dt == torch.bfloat16 else t.to(dt)
    return sd


def main():
    ref = os.environ.get("HQQ_REFERENCE")
    if not ref or not os.path.isdir(ref):
        sys.exit("set HQQ_REFERENCE to a checkout of mobiusml/hqq")
    stub = types.ModuleType("termcolor")   # hard import at hqq/core/quantize.py:13
    stub.colored = lambda t, *a, **k: t
    sys.modules.setdefault("termcolor", stub)
    sys.path.insert(0, ref)
    from hqq.core.quantize import HQQBackend, HQQLinear
    HQQLinear.set_backend(HQQBackend.PYTORCH)

    g = dict(np.load(os.path.join(HERE, "ours_sd_cfg1_4b.npz")))
    gr = dict(np.load(os.path.join(HERE, "refsd_cfg1_4b.npz")))
    x = torch.from_numpy(g["x_f32"]).half()
    layer = HQQLinear(None, None, compute_dtype=torch.float16, device="cpu")
    layer.load_state_dict(_sd(g))
    layer_r = HQQLinear(None, None, compute_dtype=torch.float16, device="cpu")
    layer_r.load_state_dict(_sd(gr))
    with torch.no_grad():
        y, y_r = layer.forward(x), layer_r.forward(x)
        wsha = hashlib.sha256(layer.dequantize().contiguous().numpy().tobytes()).hexdigest()
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, Wdeq_sha256_f16=np.frombuffer(wsha.encode(), np.uint8), y_f16=y.numpy(), y_refsd_f16=y_r.numpy())
    print(f"  {NAME}.npz  {os.path.getsize(path) / 1024:.0f} KiB")

    mpath = os.path.join(HERE, "MANIFEST.json")
    with open(mpath) as fh:
        manifest = json.load(fh)
    manifest["files"][NAME + ".npz"] = hashlib.sha256(open(path, "rb").read()).hexdigest()
    with open(mpath, "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print("updated MANIFEST.json")


if __name__ == "__main__":
    main()
