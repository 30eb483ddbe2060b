#!/usr/bin/env python3
"""Generate tests/golden/losses3d.npz by running the REFERENCE ``losses.L1Loss3D`` and ``losses.DSSIMLoss3D`` on CPU in float32, both
inputs requiring grad.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_losses3d.py          (build container only)

Per case ``<case>/x`` (prediction) and ``<case>/t`` (target), [nb,ch,frame,row,col], drawn as float16-representable values and stored as
float16 (exact; the losses still run in float32), and per loss class ``<case>/<l1|dssim>/loss``, ``/dx``, ``/dt``.

``mixed_ranges`` stacks frames of three dynamic ranges (0..1, 0..255, -1..1, 0..1): the reference detects the range per call, which in
its loop over frames means per frame.  ``mixed_ranges/dssim/folded`` stores what one range for all frames would give (the reference's
2-D ``DSSIMLoss`` on the frames folded into the batch) and ``mixed_ranges/dssim/per_frame`` the per-frame 2-D losses.  Tensors only, no
reference source text.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, OUT, _stub_modules, npy          # noqa: E402


def f16(z):
    return z.half().float()


def pair(shape, noise=0.1):
    t = torch.rand(shape)
    return t + noise * torch.randn(shape), t


def cases():
    torch.manual_seed(0)
    x, t = pair((2, 3, 4, 24, 19))
    x, t = x.clamp(0.02, 0.98), t.clamp(0.02, 0.98)      # every frame's max stays away from 128 and its min from -0.5 after the maps below
    x[:, :, 1], t[:, :, 1] = x[:, :, 1] * 255, t[:, :, 1] * 255
    x[:, :, 2], t[:, :, 2] = x[:, :, 2] * 2 - 1, t[:, :, 2] * 2 - 1
    yield "mixed_ranges", f16(x), f16(t)
    x, t = pair((1, 2, 3, 47, 75))
    yield "tiles", f16(x.clamp(0, 1)), f16(t)
    x, t = pair((2, 1, 2, 11, 11), 0.2)
    yield "single_window", f16(x.clamp(0, 1)), f16(t)
    x, t = pair((1, 1, 2, 11, 300))
    yield "strip", f16(x.clamp(0, 1)), f16(t)


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import losses as ref_losses                    # src/losses.py: L1Loss3D :107-120, DSSIMLoss3D :183-196

    torch.set_num_threads(4)
    crits = {"l1": ref_losses.L1Loss3D(), "dssim": ref_losses.DSSIMLoss3D()}
    assert repr(crits["l1"]) == "L13D" and repr(crits["dssim"]) == "DSSIM3D"
    out = {}
    for name, x, t in cases():
        out[f"{name}/x"], out[f"{name}/t"] = x.half().numpy(), t.half().numpy()
        for f in range(x.shape[2]):
            hi, lo = float(x[:, :, f].max()), float(x[:, :, f].min())
            assert abs(hi - 128) > 20 and abs(lo + 0.5) > 0.2, (name, f, lo, hi)
        for key, crit in crits.items():
            xr, tr = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
            loss = crit(xr, tr)
            loss.backward()
            out[f"{name}/{key}/loss"], out[f"{name}/{key}/dx"], out[f"{name}/{key}/dt"] = npy(loss), npy(xr.grad), npy(tr.grad)
            print(f"{name:14s} {key:5s} loss {float(loss):.6f}")
    x, t = torch.from_numpy(out["mixed_ranges/x"]).float(), torch.from_numpy(out["mixed_ranges/t"]).float()
    fold = lambda z: z.permute(0, 2, 1, 3, 4).reshape(-1, z.shape[1], z.shape[3], z.shape[4])
    d2 = ref_losses.DSSIMLoss()
    out["mixed_ranges/dssim/folded"] = npy(d2(fold(x), fold(t)))
    out["mixed_ranges/dssim/per_frame"] = np.array([float(d2(x[:, :, f], t[:, :, f])) for f in range(x.shape[2])], dtype=np.float32)
    print("mixed_ranges: folded", float(out["mixed_ranges/dssim/folded"]), "per frame", out["mixed_ranges/dssim/per_frame"])
    np.savez(os.path.join(OUT, "losses3d.npz"), **out)


if __name__ == "__main__":
    main()
