#!/usr/bin/env python3
"""Generate tests/golden/nearest_selector.npz by running the REFERENCE ``losses.NearestSelector`` and ``losses.L1Loss`` on CPU in
float32.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_nearest.py          (build container only)

``unravel_index`` is REPLACED AT RUN TIME by its floor-division form (``index // cols`` for the reference's ``index / cols``).  On
current torch ``/`` is true division, the row index becomes a float tensor, and the reference's ``crop`` stops at its first slice with
``TypeError: only integer tensors of a single element can be converted to an index``.  ``shift_diff`` is the reference's own, unchanged.

Per case ``<case>/cfg`` = (shift, stride), ``<case>/x`` (prediction) and ``<case>/t`` (target) as float16 (the values are drawn
float16-representable, so this is exact; everything is computed in float32), ``<case>/diff`` = the reference's ``shift_diff``; for the
square cases also ``<case>/sel`` (the patched ``unravel_index``), ``<case>/out_`` / ``<case>/tgt_`` (``crop``; copies of input values,
stored as float16), ``<case>/loss`` and ``<case>/dx`` (``L1Loss`` on the crops, ``backward``; the target carries no gradient).
The reference's ``crop`` raises a shape error on non-square images, so ``nonsquare`` holds ``diff`` only.

``golden``: sample b's centre crop of the prediction is the target's window at (0,3), (2,2), (3,1) plus noise -- candidates 3, 10, 13.
The other cases are tests/nearest_ref.py's ``float_case`` under its seeds.  Tensors only, no reference source text.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, OUT, _stub_modules, npy          # noqa: E402
import nearest_ref as R                                      # noqa: E402


def unravel_floor(tensor, cols):
    index = torch.argmin(tensor, dim=1).view(-1, 1)
    return torch.cat([index // cols, index % cols], dim=1)


def golden_case():
    B, C, H, W, shift, stride = R.SHAPES["golden"]
    g = torch.Generator().manual_seed(R.FLOAT_SEEDS["golden"])
    t = torch.rand(B, C, H, W, generator=g).half().float()
    o = torch.rand(B, C, H, W, generator=g)
    for b, (r, c) in enumerate(((0, 3), (2, 2), (3, 1))):
        o[b, :, 2:10, 2:10] = t[b, :, r:r + 8, c:c + 8] + 0.05 * torch.randn(C, 8, 8, generator=g)
    return o.half().float(), t


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import losses as ref_losses                    # src/losses.py: NearestSelector :199-255, L1Loss :95-105

    torch.set_num_threads(4)
    ref_losses.NearestSelector.unravel_index = staticmethod(unravel_floor)
    out = {}
    for name in ("golden", "stride2", "shift3", "nonsquare"):
        B, C, H, W, shift, stride = R.SHAPES[name]
        x, t = golden_case() if name == "golden" else R.float_case(name, R.FLOAT_SEEDS[name])[:2]
        ns = ref_losses.NearestSelector(shift=shift, stride=stride)
        assert repr(ns) == "NS"
        sd, ch, cw, n = R.geometry(H, W, shift, stride)
        diff = ns.shift_diff(x, t, ch, cw)
        out[f"{name}/cfg"] = np.array([shift, stride])
        out[f"{name}/x"], out[f"{name}/t"], out[f"{name}/diff"] = x.half().numpy(), t.half().numpy(), npy(diff)
        print(name, "candidates", torch.argmin(diff, dim=1).tolist(), "margin", R.margin(R.shift_diff(x, t, shift, stride)).min())
        if H != W:
            continue
        xr = x.clone().requires_grad_(True)
        out_, tgt_ = ns.crop(xr, t.clone())
        loss = ref_losses.L1Loss()(out_, tgt_)
        loss.backward()
        assert torch.equal(out_.half().float(), out_.detach()) and torch.equal(tgt_.half().float(), tgt_)
        out[f"{name}/sel"] = npy(unravel_floor(diff, n))
        out[f"{name}/out_"], out[f"{name}/tgt_"] = out_.detach().half().numpy(), tgt_.half().numpy()
        out[f"{name}/loss"], out[f"{name}/dx"] = npy(loss), npy(xr.grad)
    assert out["golden/sel"].tolist() == [[0, 3], [2, 2], [3, 1]]
    np.savez_compressed(os.path.join(OUT, "nearest_selector.npz"), **out)
    print(os.path.getsize(os.path.join(OUT, "nearest_selector.npz")), "bytes")


if __name__ == "__main__":
    main()
