"""DSSIM loss at the headline size (16x3x1024x1024 f32): native forward, native backward (prediction gradient only, and both
gradients), the whole native loss through autograd, and the torch composition (the oracle's SSIM expression, grouped 11x11
convolutions, through autograd) for comparison.  HIP-event timing after warm-up; one JSON line per measurement.

    python scripts/microbench_dssim.py [--iters N] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from srcgan_amd import DSSIMLoss
from srcgan_amd import _native as N


def timeit(f, iters, warmup=3):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def torch_dssim(x, t):
    """The oracle's metric_ssim expression (oracle/srcgan_oracle.py) with its window built on the inputs' device."""
    L = (255 if torch.max(x) > 128 else 1) - (-1 if torch.min(x) < -0.5 else 0)
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    ch = x.shape[1]
    win = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(ch, 1, 11, 11).contiguous().to(x.device)
    conv = lambda z: F.conv2d(z, win, padding=0, groups=ch)
    mu1, mu2 = conv(x), conv(t)
    s1, s2, s12 = conv(x * x) - mu1.pow(2), conv(t * t) - mu2.pow(2), conv(x * t) - mu1 * mu2
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    m = ((2 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1.pow(2) + mu2.pow(2) + C1) * (s1 + s2 + C2))
    return (1.0 - m.mean()) / 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", type=int, nargs=4, default=[16, 3, 1024, 1024])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, C, H, W = a.shape
    torch.manual_seed(0)
    t = torch.rand(B, C, H, W, device="cuda")
    x = (t + 0.1 * torch.randn_like(t)).clamp_(0, 1)
    lib = N.lib()
    st = N.stream_ptr(x.device)
    out = torch.empty((), device="cuda")
    rng = torch.empty(2, device="cuda")
    scr = torch.empty(lib.srcgan_dssim3d_scratch_floats(B, C, 1, H, W), device="cuda")
    gout = torch.ones((), device="cuda")
    dx, dt = torch.empty_like(x), torch.empty_like(t)

    # a [B,C,H,W] tensor is the F = 1 instance of the loss's [B,C,F,H,W] entry points
    fwd = lambda: N.check(lib.srcgan_dssim3d_loss_fwd(x.data_ptr(), t.data_ptr(), B, C, 1, H, W, out.data_ptr(), rng.data_ptr(),
                                                      scr.data_ptr(), st), "fwd")
    bwd1 = lambda: N.check(lib.srcgan_dssim3d_loss_bwd(x.data_ptr(), t.data_ptr(), B, C, 1, H, W, rng.data_ptr(), gout.data_ptr(),
                                                       dx.data_ptr(), None, st), "bwd")
    bwd2 = lambda: N.check(lib.srcgan_dssim3d_loss_bwd(x.data_ptr(), t.data_ptr(), B, C, 1, H, W, rng.data_ptr(), gout.data_ptr(),
                                                       dx.data_ptr(), dt.data_ptr(), st), "bwd")
    xg = x.clone().requires_grad_(True)

    def native_autograd():
        xg.grad = None
        DSSIMLoss()(xg, t).backward()

    def torch_autograd():
        xg.grad = None
        torch_dssim(xg, t).backward()

    fwd()
    res = {"shape": [B, C, H, W],
           "native_fwd_us": timeit(fwd, a.iters),
           "native_bwd_dx_us": timeit(bwd1, a.iters),
           "native_bwd_dx_dt_us": timeit(bwd2, a.iters),
           "native_autograd_fwd_bwd_us": timeit(native_autograd, a.iters),
           "torch_autograd_fwd_bwd_us": timeit(torch_autograd, max(3, a.iters // 4))}
    nb = x.numel() * 4
    res["hbm_floor_fwd_us"] = 2 * nb / 6.3e12 * 1e6
    res["hbm_floor_bwd_dx_us"] = 3 * nb / 6.3e12 * 1e6
    res["hbm_floor_bwd_dx_dt_us"] = 4 * nb / 6.3e12 * 1e6
    res["loss"] = float(out)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
