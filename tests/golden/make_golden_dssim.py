#!/usr/bin/env python3
"""Generate tests/golden/dssim.npz by running the REFERENCE ``losses.DSSIMLoss`` on CPU in float32, both inputs requiring grad.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_dssim.py          (build container only)

Per case ``<case>/x`` (prediction), ``<case>/t`` (target), ``<case>/loss``, ``<case>/dx``, ``<case>/dt``.  The inputs are drawn as
float16-representable values and stored as float16 (exact; the loss still runs in float32) to keep the file small.

The ``near`` case (prediction = target + 1e-3 noise, SSIM close to 1) is dominated by the ``E[x^2] - mu^2`` cancellation, so it
stores a float64 evaluation written here (the reference's window is float32 and forces float32): ``loss``, ``dx``, ``dt`` are the
float64 results (the gradients rounded to float32), ``loss32`` is the reference's float32 loss, and ``gate_dx`` / ``gate_dt`` =
max(1e-3, 3 x the reference's own float32-vs-float64 error) in the test suite's ``rel_err`` measure.  Tensors only, no reference
source text.
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, OUT, _stub_modules, npy          # noqa: E402


def rel_err(a, b):
    """tests/conftest.py's rel_err: the larger of the max-normalised and the relative L2 error."""
    a, b = a.double(), b.double()
    return max(float((a - b).abs().max() / b.abs().max()), float((a - b).norm() / b.norm()))


def dssim64(x, t):
    """(1 - SSIM) / 2 in float64: the reference's formula with a float64 window."""
    L = (255 if float(x.detach().max()) > 128 else 1) - (-1 if float(x.detach().min()) < -0.5 else 0)
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], dtype=torch.float64)
    g = (g / g.sum()).unsqueeze(1)
    ch = x.shape[1]
    win = g.mm(g.t()).expand(ch, 1, 11, 11).contiguous()
    conv = lambda z: F.conv2d(z, win, groups=ch)
    m1, m2 = conv(x), conv(t)
    s1, s2, s12 = conv(x * x) - m1 * m1, conv(t * t) - m2 * m2, conv(x * t) - m1 * m2
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    ssim = ((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2))
    return (1 - ssim.mean()) / 2


def f16(z):
    return z.half().float()


def cases():
    torch.manual_seed(0)
    t = f16(torch.rand(2, 3, 37, 53))
    yield "rgb01", f16((t + 0.1 * torch.randn_like(t)).clamp(0, 1)), t
    t = f16(torch.rand(2, 1, 48, 40) * 255)
    yield "gray255", f16((t + 12 * torch.randn_like(t)).clamp(0, 255)), t
    t = f16(torch.rand(1, 3, 32, 32) * 2 - 1)
    yield "tanh", f16((t + 0.1 * torch.randn_like(t)).clamp(-1, 1)), t
    t = f16(torch.rand(3, 2, 11, 11))
    yield "single", f16((t + 0.2 * torch.randn_like(t)).clamp(0, 1)), t
    t = f16(torch.rand(1, 1, 11, 300))
    yield "strip_row", f16((t + 0.1 * torch.randn_like(t)).clamp(0, 1)), t
    t = f16(torch.rand(1, 1, 300, 11))
    yield "strip_col", f16((t + 0.1 * torch.randn_like(t)).clamp(0, 1)), t
    t = f16(torch.rand(2, 3, 64, 64) * 0.5)          # [0, 0.5): float16 spacing <= 2.4e-4 keeps the 1e-3 noise resolved
    yield "near", f16(t + 1e-3 * torch.randn_like(t)), t


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import losses as ref_losses                    # src/losses.py: DSSIMLoss :170-180, SSIM :20-93

    torch.set_num_threads(4)
    crit = ref_losses.DSSIMLoss()
    assert repr(crit) == "DSSIM"
    out = {}
    for name, x, t in cases():
        xr, tr = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
        loss = crit(xr, tr)
        loss.backward()
        out[f"{name}/x"], out[f"{name}/t"] = x.half().numpy(), t.half().numpy()
        if name != "near":
            out[f"{name}/loss"], out[f"{name}/dx"], out[f"{name}/dt"] = npy(loss), npy(xr.grad), npy(tr.grad)
            continue
        x64, t64 = x.double().requires_grad_(True), t.double().requires_grad_(True)
        l64 = dssim64(x64, t64)
        l64.backward()
        out["near/loss"], out["near/loss32"] = l64.detach().numpy().copy(), npy(loss)
        out["near/dx"], out["near/dt"] = x64.grad.float().numpy(), t64.grad.float().numpy()
        out["near/gate_dx"] = np.array(max(1e-3, 3 * rel_err(xr.grad, x64.grad)))
        out["near/gate_dt"] = np.array(max(1e-3, 3 * rel_err(tr.grad, t64.grad)))
        print(f"near: loss32 {float(loss.detach()):.9g} loss64 {float(l64.detach()):.12g} gates dx {float(out['near/gate_dx']):.3g} "
              f"dt {float(out['near/gate_dt']):.3g}")
    np.savez(os.path.join(OUT, "dssim.npz"), **out)


if __name__ == "__main__":
    main()
