#!/usr/bin/env python3
"""Time the multi-frame losses on [nb,ch,frame,row,col] tensors, forward + backward, three ways in one process:

  torch    the reference's algorithm (src/losses.py:107-120, 183-196, 396-453) on torch ops: a Python loop over the frames, each on
           slices output[:, :, f] / target[:, :, f]; SSIM as five grouped 11x11 convolutions with the range read on the host per frame;
           VGG16 as nn.Conv2d / ReLU / MaxPool2d modules in the compute dtype
  loop     the same loop over the native 2-D classes (srcgan_amd.L1Loss / DSSIMLoss / VGG16Loss): what a user could write before
  3-D      srcgan_amd.L1Loss3D / DSSIMLoss3D / VGG16Loss3D (the last with frames_per_pass = 1 and None)

Rounds alternate between the forms (so clock and cache state are shared).  Each round times `reps` back-to-back iterations between two
device events, with `reps` chosen per form from a warm-up iteration so that a window lasts at least --window ms; the median over the
rounds of the per-iteration time is reported.  Peak allocated memory is the high-water mark of one iteration above the inputs.

    python scripts/bench_losses3d.py [--rounds 7] [--warmup 2] [--window 40] [--out profiles/losses3d.txt]
"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PIXEL_SHAPES = ((4, 3, 8, 512, 512), (2, 3, 4, 1024, 1024))       # fp32, L1 and DSSIM
VGG_SHAPE = (2, 3, 4, 512, 512)                                   # bf16


def frame_loop(crit2d):
    def fn(o, t):
        n = o.shape[2]
        return sum(crit2d(o[:, :, f], t[:, :, f]) for f in range(n)) / n
    return fn


def torch_dssim2d(x, t):
    L = (255 if float(x.detach().max()) > 128 else 1) - (-1 if float(x.detach().min()) < -0.5 else 0)
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], device=x.device)
    g = (g / g.sum()).unsqueeze(1)
    ch = x.shape[1]
    win = g.mm(g.t()).expand(ch, 1, 11, 11).contiguous()
    conv = lambda z: F.conv2d(z, win, groups=ch)
    m1, m2 = conv(x), conv(t)
    s1, s2, s12 = conv(x * x) - m1 * m1, conv(t * t) - m2 * m2, conv(x * t) - m1 * m2
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    return (1 - (((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2))).mean()) / 2


class TorchVgg16Loss(nn.Module):
    def __init__(self, sd, dtype):
        super().__init__()
        import vgg_ref as R
        layers, idx = [], 0
        for v in R.VGG16_LAYOUT:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
                idx += 1
            else:
                w = sd[f"features.{idx}.weight"]
                c = nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1)
                c.weight.data.copy_(w)
                c.bias.data.copy_(sd[f"features.{idx}.bias"])
                layers += [c, nn.ReLU()]
                idx += 2
        self.slices = nn.ModuleList(nn.Sequential(*layers[a:b]) for a, b in ((0, 4), (4, 9), (9, 16), (16, 23)))
        self.to(dtype).cuda().requires_grad_(False)
        self.dtype = dtype

    def forward(self, o, t):
        ho, ht, terms = o.to(self.dtype), t.to(self.dtype), []
        for s in self.slices:
            ho, ht = s(ho), s(ht)
            terms.append(F.l1_loss(ho.float(), ht.float()))
        return sum(terms) / 4


def measure(forms, o, t, args):
    """-> {name: (median ms, min, max, reps, peak bytes, loss)}"""
    def once(fn):
        x = o.clone().requires_grad_(True)
        loss = fn(x, t)
        loss.backward()
        return loss

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            once(fn)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    reps, peak, value = {}, {}, {}
    for name, fn in forms:
        once(fn)                                     # code objects, library algorithm choices
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        value[name] = float(once(fn).detach())
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        reps[name] = max(1, min(200, math.ceil(args.window / max(window(fn, 1), 1e-3))))
    times = {name: [] for name, _ in forms}
    for rnd in range(args.warmup + args.rounds):
        for name, fn in forms:
            ms = window(fn, reps[name])
            if rnd >= args.warmup:
                times[name].append(ms)
    return {n: (statistics.median(v), min(v), max(v), reps[n], peak[n], value[n]) for n, v in times.items()}


def report(lines, title, shape, esz, res):
    lines.append(f"\n{title}  {'x'.join(map(str, shape))}  (one tensor = {esz * math.prod(shape) / 1e6:.1f} MB)")
    for name, (ms, lo, hi, reps, peak, val) in res.items():
        lines.append(f"  {name:14s} {ms:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, {reps:3d} per window)   peak +{peak / 1e6:9.1f} MB   loss {val:.7f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=40.0, help="least length of a timed window, ms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses3d.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_losses3d: needs a GPU (a CPU run gives no time)")
    import vgg_ref as R
    from srcgan_amd import DSSIMLoss, DSSIMLoss3D, L1Loss, L1Loss3D, VGG16Loss, VGG16Loss3D

    lines = [f"multi-frame losses, forward + backward; {torch.cuda.get_device_name(0)}; median of {args.rounds} alternating rounds after "
             f"{args.warmup} warm-up rounds, device events around windows of at least {args.window:.0f} ms"]
    for shape in PIXEL_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        t = torch.rand(shape, device="cuda", generator=g)
        o = (t + 0.1 * torch.randn(shape, device="cuda", generator=g)).clamp_(0, 1)
        report(lines, "L1 fp32", shape, 4, measure((("torch", frame_loop(F.l1_loss)), ("loop", frame_loop(L1Loss())), ("3-D", L1Loss3D())), o, t, args))
        report(lines, "DSSIM fp32", shape, 4,
               measure((("torch", frame_loop(torch_dssim2d)), ("loop", frame_loop(DSSIMLoss())), ("3-D", DSSIMLoss3D())), o, t, args))
        del o, t
    sd = R.seeded_state(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.rand(VGG_SHAPE, device="cuda", generator=g)
    o = (t + 0.1 * torch.randn(VGG_SHAPE, device="cuda", generator=g)).clamp_(0, 1)
    forms = (("torch", frame_loop(TorchVgg16Loss(sd, torch.bfloat16))), ("loop", frame_loop(VGG16Loss(weights=sd, dtype="bf16"))),
             ("3-D, 1 / pass", VGG16Loss3D(weights=sd, dtype="bf16", frames_per_pass=1)), ("3-D, all", VGG16Loss3D(weights=sd, dtype="bf16")))
    report(lines, "VGG16 bf16", VGG_SHAPE, 4, measure(forms, o, t, args))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
