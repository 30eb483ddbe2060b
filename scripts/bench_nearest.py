#!/usr/bin/env python3
"""Time the shift-tolerant L1 loss, forward + backward, three ways in one process:

  torch      the reference's algorithm (src/losses.py:199-255 with floor division in unravel_index) on torch ops: (2*shift)^2
             abs-difference-sum passes, a host read of the selection per sample, a zero-filled crop, nn.L1Loss
  crop+L1    srcgan_amd.NearestSelector.crop + srcgan_amd.L1Loss
  fused      srcgan_amd.NearestL1Loss

Rounds alternate between the three (so clock and cache state are shared), each timed with device events after warm-up rounds;
the median is reported.  Peak allocated memory is the high-water mark above the inputs.  The algorithmic bytes are computed from
the shapes (what each form must move if every tensor crossed HBM once per pass that touches it).

    python scripts/bench_nearest.py [--rounds 9] [--warmup 3] [--out profiles/nearest_select.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 3, 1024, 1024), (16, 1, 256, 256))
SHIFT, STRIDE = 2, 1


def torch_composition(output, target, shift=SHIFT, stride=STRIDE):
    nb, ch, row, col = output.shape
    sd, n = shift * stride, 2 * shift
    crop_row, crop_col = row - 2 * sd, col - 2 * sd
    o, t = output.detach(), target.detach()
    diff = []
    for i in range(n):
        for j in range(n):
            oc = o[:, :, sd:sd + crop_row, sd:sd + crop_col]
            tc = t[:, :, i * stride:i * stride + crop_row, j * stride:j * stride + crop_col]
            diff.append(torch.sum(abs(tc - oc), dim=[1, 2, 3]).view(-1, 1))
    index = torch.argmin(torch.cat(diff, dim=1), dim=1).view(-1, 1)
    min_rc = torch.cat([index // n, index % n], dim=1)
    output_ = output[:, :, sd:sd + crop_row, sd:sd + crop_col]
    target_ = torch.zeros(*output_.shape).to(target.device)
    for idx, (r, c) in enumerate(min_rc):
        target_[idx] = target[idx, :, r * stride:r * stride + crop_row, c * stride:c * stride + crop_col]
    return torch.nn.functional.l1_loss(output_, target_)


def algorithmic_bytes(shape, shift=SHIFT, stride=STRIDE):
    B, C, H, W = shape
    full, crop = 4 * B * C * H * W, 4 * B * C * (H - 2 * shift * stride) * (W - 2 * shift * stride)
    n2 = (2 * shift) ** 2
    return {
        # n2 passes of 2 crop reads + temporary write/read twice (difference, abs), zero fill + copy of the crop, l1 forward 2 reads + temporaries,
        # backward: sign pass (2 reads, 1 write) + the zero-padded full-size gradient
        "torch": n2 * (2 * crop + 4 * crop) + 3 * crop + (2 * crop + 2 * crop) + (3 * crop + crop + full),
        # search 2 full reads, gather read + write, contiguous copy of the output crop (read + write), L1 forward 2 reads,
        # L1 backward 2 reads + 1 write, slice backward: zero fill + read + write
        "crop+L1": 2 * full + 2 * crop + 2 * crop + 2 * crop + 3 * crop + (full + 2 * crop),
        # search 2 full reads, backward 2 full reads + 1 full write
        "fused": 2 * full + 3 * full,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_select.txt"))
    args = ap.parse_args()
    from srcgan_amd import L1Loss, NearestL1Loss, NearestSelector

    selector, l1, fused = NearestSelector(SHIFT, STRIDE), L1Loss(), NearestL1Loss(SHIFT, STRIDE)
    forms = (("torch", torch_composition), ("crop+L1", lambda o, t: l1(*selector.crop(o, t))), ("fused", fused))
    lines = [f"shift-tolerant L1 loss, forward + backward, shift={SHIFT} stride={STRIDE}; {torch.cuda.get_device_name(0)}; "
             f"median of {args.rounds} alternating rounds after {args.warmup} warm-up rounds, device events"]
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        t = torch.rand(shape, device="cuda", generator=g)
        o = torch.roll(t, (1, -1), (2, 3)) + 0.05 * torch.randn(shape, device="cuda", generator=g)
        times, peak, value = {k: [] for k, _ in forms}, {}, {}
        for rnd in range(args.warmup + args.rounds):
            for name, fn in forms:
                x = o.clone().requires_grad_(True)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss = fn(x, t)
                loss.backward()
                e1.record()
                torch.cuda.synchronize()
                if rnd >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
                peak[name] = torch.cuda.max_memory_allocated() - base
                value[name] = float(loss.detach())
                del x, loss
        by = algorithmic_bytes(shape)
        lines.append(f"\n{'x'.join(map(str, shape))}  (one tensor = {4 * shape[0] * shape[1] * shape[2] * shape[3] / 1e6:.1f} MB)")
        for name, _ in forms:
            ms = statistics.median(times[name])
            lines.append(f"  {name:8s} {ms:9.3f} ms  (min {min(times[name]):.3f}, max {max(times[name]):.3f})   peak +{peak[name] / 1e6:9.1f} MB   "
                         f"algorithmic {by[name] / 1e6:9.1f} MB -> {by[name] / ms / 1e6:7.1f} GB/s   loss {value[name]:.7f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
