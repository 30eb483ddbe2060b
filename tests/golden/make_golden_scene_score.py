#!/usr/bin/env python3
"""Generate tests/golden/scene_score.npz by running the REFERENCE ``metrics.MSE / PSNR / AE / SSIM`` on CPU for whole-scene pairs.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_scene_score.py          (build container only)

Per case ``<case>/pred`` and ``<case>/target`` (u8 ``[H,W,C]``), ``<case>/ref32/<Q>`` and ``<case>/ref64/<Q>`` for Q in MSE, PSNR,
AE, SSIM, CS.  The target is a smooth random field; the prediction is the target plus noise of sigma = 12 levels, with a block of
exact zeros (a smaller one in the target: black pixels, the 0 / (0 + eps) branch of AE) and with its last 10 rows and last 10
columns inverted -- the band that holds no SSIM window position, so a scorer that skips it is far off in MSE and AE.

``ref32``: the reference classes on the f32 ``v / 255`` tensors ``[1,C,H,W]``.  ``ref64``: the same formulas at float64 on the same
values: MSE, PSNR and AE are the reference classes on double tensors; SSIM is a subclass whose ``create_window`` returns the
reference's f32 window cast to double (the class as shipped builds a float window and so refuses double input).
Tensors only, no reference source text.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, OUT, _stub_modules          # noqa: E402

SHAPES = [(11, 11, 3), (11, 75, 1), (43, 75, 3), (97, 139, 3), (97, 139, 1)]
QS = ("MSE", "PSNR", "AE", "SSIM", "CS")


def make_pair(H, W, C, seed):
    """-> (pred, target) u8 [H,W,C] tensors as described in the module docstring."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(1, C, max(2, H // 8 + 2), max(2, W // 8 + 2), generator=g)
    field = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0]                  # [C,H,W] in [0,1]
    target = (field * 215 + 20).round().clamp(0, 255)
    pred = (target + 12.0 * torch.randn(C, H, W, generator=g)).round().clamp(0, 255)
    y0, x0 = H // 4, W // 4
    pred[:, y0:y0 + max(2, H // 5), x0:x0 + max(2, W // 5)] = 0
    target[:, y0:y0 + max(1, H // 10), x0:x0 + max(1, W // 10)] = 0
    pred[:, H - 10:, :] = 255 - pred[:, H - 10:, :]
    pred[:, :, W - 10:] = 255 - pred[:, :, W - 10:]
    hwc = lambda z: z.permute(1, 2, 0).contiguous().to(torch.uint8)
    return hwc(pred), hwc(target)


def planes(u8):
    """u8 [H,W,C] -> f32 [1,C,H,W], v / 255 with the quotient in double and one rounding to float"""
    return (u8.double() / 255.0).float().permute(2, 0, 1).unsqueeze(0).contiguous()


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import metrics as ref                         # src/metrics.py

    class SSIM64(ref.SSIM):
        def create_window(self, w_size, channel=1):
            return super().create_window(w_size, channel=channel).double()

    torch.set_num_threads(4)
    out = {}
    for k, (H, W, C) in enumerate(SHAPES):
        name = f"s{H}x{W}x{C}"
        pred, target = make_pair(H, W, C, 100 + k)
        out[f"{name}/pred"], out[f"{name}/target"] = pred.numpy(), target.numpy()
        p32, t32 = planes(pred), planes(target)
        for tag, p, t, ssim in (("ref32", p32, t32, ref.SSIM()), ("ref64", p32.double(), t32.double(), SSIM64())):
            s, cs = ssim(p, t, full=True)
            vals = dict(MSE=ref.MSE()(p, t), PSNR=ref.PSNR()(p, t), AE=ref.AE()(p, t)[0], SSIM=s, CS=cs)
            for q in QS:
                assert vals[q].dtype == (torch.float32 if tag == "ref32" else torch.float64)
                out[f"{name}/{tag}/{q}"] = np.array(vals[q].item(), dtype=np.float64)
        print(name, " ".join(f"{q} {float(out[f'{name}/ref64/{q}']):.6g} (f32 off by "
                             f"{abs(float(out[f'{name}/ref32/{q}']) - float(out[f'{name}/ref64/{q}'])) / abs(float(out[f'{name}/ref64/{q}'])):.2g})" for q in QS))
    np.savez(os.path.join(OUT, "scene_score.npz"), **out)


if __name__ == "__main__":
    main()
