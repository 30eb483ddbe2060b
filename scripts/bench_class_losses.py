#!/usr/bin/env python3
"""Time FLoss, CELoss, ConLoss and CrossLoss, forward + backward, two ways in one process:

  torch    the losses' formulas written on torch ops: clamp / pow / log / mul / mean for the focal loss,
           F.binary_cross_entropy, log + argmax + F.nll_loss, max / min over the batch + F.mse_loss, F.l1_loss on two slices
  native   srcgan_amd.FLoss / CELoss / ConLoss / CrossLoss (csrc/class_losses.hip: one pass forward, one backward)

Rounds alternate between the forms (so clock and cache state are shared).  Each round times `reps` back-to-back iterations between two
device events around a synchronised window, with `reps` chosen per form from a warm-up iteration so that a window lasts at least --window
ms; the median, minimum and maximum over the rounds of the per-iteration time are reported.  Peak allocated memory is the high-water
mark of one iteration above the inputs.  "faster beyond the spread" holds when the slowest native round beats the fastest torch round.

--trace DIR starts `rocprofv3 --kernel-trace --stats` (no counters) on child processes that run only the native losses (one child per
group of cases whose kernels differ, so that a kernel's average belongs to one size) and states each kernel's achieved bytes/s from its
average time and the algorithmic bytes computed here: a forward reads its inputs once, a backward reads them and writes the gradient.
Each child also times a plain device copy of the binary case's tensor with device events, for comparison in the same run.  A second
set of children runs the forwards alone: in the forward + backward loop every forward starts behind the gradient its predecessor has
just written, and the write-back of those dirty lines is charged to the forward's time.

    python scripts/bench_class_losses.py [--rounds 7] [--warmup 2] [--window 40] [--trace DIR] [--out profiles/class_losses.txt]
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINARY, MULTI, CON, CROSS = (16, 1, 1024, 1024), (16, 8, 512, 512), (16, 64, 256, 256), (16, 3, 1024, 1024)
LO, HI = 1e-6, 1.0 - 1e-6


def torch_focal(gamma=2.0):
    def fn(x, t):
        o = torch.clamp(x, min=LO, max=HI)
        if t.shape[1] == 1:
            loss = -0.9 * ((1. - o) ** gamma) * (t * torch.log(o)) - 0.1 * (o ** gamma) * ((1. - t) * torch.log(1. - o))
        else:
            loss = -((1. - o) ** gamma) * (t * torch.log(o))
        return loss.mean()
    return fn


def torch_ce(x, t):
    if t.shape[1] == 1:
        return F.binary_cross_entropy(x, t)
    return F.nll_loss(torch.log(x), torch.argmax(t, dim=1))


def torch_con(f, _):
    r = torch.abs(torch.max(f, dim=0)[0] - torch.min(f, dim=0)[0])
    return F.mse_loss(r, torch.zeros_like(r))


def torch_cross(x, t):
    nb = x.shape[0]
    return F.l1_loss(x[:nb - 1], t[1:nb])


def cases():
    """(title, shape, torch form, native criterion, takes a target, trace group, {kernel name fragment: algorithmic bytes})"""
    from srcgan_amd import CELoss, ConLoss, CrossLoss, FLoss
    n = lambda s: 4 * math.prod(s)
    pix = lambda s: 4 * s[0] * s[2] * s[3]
    con = ConLoss()
    return [
        ("FLoss binary, gamma 2", BINARY, torch_focal(), FLoss(), True, 0, {"cl_flat_fwd_k<ClFocal>": 2 * n(BINARY), "cl_flat_bwd_k<ClFocal>": 3 * n(BINARY)}),
        ("FLoss binary, gamma 1.5", BINARY, torch_focal(1.5), FLoss(gamma=1.5), True, 2, {"cl_flat_fwd_k<ClFocal>": 2 * n(BINARY), "cl_flat_bwd_k<ClFocal>": 3 * n(BINARY)}),
        ("CELoss binary", BINARY, torch_ce, CELoss(), True, 0, {"cl_flat_fwd_k<ClBce>": 2 * n(BINARY), "cl_flat_bwd_k<ClBce>": 3 * n(BINARY)}),
        ("FLoss multi-class, gamma 2", MULTI, torch_focal(), FLoss(), True, 1, {"cl_flat_fwd_k<ClFocal>": 2 * n(MULTI), "cl_flat_bwd_k<ClFocal>": 3 * n(MULTI)}),
        ("CELoss multi-class", MULTI, torch_ce, CELoss(), True, 0, {"cl_nll_fwd_k": n(MULTI) + pix(MULTI), "cl_nll_bwd_k": 2 * n(MULTI) + pix(MULTI)}),
        ("ConLoss", CON, torch_con, lambda f, _: con(f), False, 0, {"cl_range_fwd_k": n(CON), "cl_range_bwd_k": 2 * n(CON)}),
        ("CrossLoss", CROSS, torch_cross, CrossLoss(), True, 0,
         {"cl_flat_fwd_k<ClL1>": 2 * n(CROSS) * 15 // 16, "cl_flat_bwd_k<ClL1>": 2 * n(CROSS) * 15 // 16 + n(CROSS)}),
    ]


def inputs(shape, multi):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(shape, device="cuda", generator=g) * 0.96 + 0.02
    t = torch.rand(shape, device="cuda", generator=g)
    if shape[1] == 1:
        t = (t > 0.5).float()
    return x.requires_grad_(True), t


def once(fn, x, t):
    x.grad = None
    loss = fn(x, t)
    loss.backward()
    return loss


def measure(forms, x, t, args):
    """-> {name: (median ms, min, max, reps, peak bytes, loss)}"""
    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            once(fn, x, t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    reps, peak, value = {}, {}, {}
    for name, fn in forms:
        once(fn, x, t)                                  # code objects
        x.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        value[name] = float(once(fn, x, t).detach())
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


def copy_rate(shape=BINARY, reps=50):
    """bytes/s (read + write) of a plain device copy of one tensor of ``shape``, device events around a synchronised window."""
    src = torch.rand(shape, device="cuda")
    dst = torch.empty_like(src)
    best = 0.0
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        best = max(best, 2 * 4 * src.numel() * reps / (e0.elapsed_time(e1) * 1e-3))
    return best


def traced_child(group, iters):
    """group >= 100: the forwards of group - 100 alone, so that no forward runs behind a backward's freshly written gradient"""
    for title, shape, _, native, _, grp, _ in cases():
        if grp != group % 100:
            continue
        x, t = inputs(shape, shape[1] > 1)
        for _ in range(iters):
            if group >= 100:
                with torch.no_grad():
                    native(x, t)
            else:
                once(native, x, t)
        torch.cuda.synchronize()
        del x, t
    print(json.dumps({"copy_Bps": copy_rate()}), flush=True)


def trace(args, say):
    all_cases = cases()
    groups = sorted({c[5] for c in all_cases})
    for group in groups + [100 + g for g in groups]:
        out = os.path.join(args.trace, f"group{group}")
        os.makedirs(out, exist_ok=True)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "cl", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--traced-child", str(group), "--trace-iters", str(args.trace_iters)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        if res.returncode != 0:
            raise SystemExit(f"rocprofv3 run failed with status {res.returncode}")
        copy = None
        for line in res.stdout.splitlines():
            if line.startswith('{"copy_Bps"'):
                copy = json.loads(line)["copy_Bps"]
        rows = []
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += list(csv.DictReader(f))
        say(f"\nkernel trace, group {group % 100}, {'forwards alone' if group >= 100 else 'forward + backward'}: plain device copy of {'x'.join(map(str, BINARY))} f32 in the same run = "
            + (f"{copy / 1e12:.2f} TB/s (read + write)" if copy else "not measured"))
        for title, shape, _, _, _, grp, kernels in all_cases:
            if grp != group % 100:
                continue
            for frag, nbytes in kernels.items():
                if group >= 100 and "bwd" in frag:
                    continue
                hit = [r for r in rows if frag.replace(" ", "") in r["Name"].replace(" ", "")]
                if not hit:
                    say(f"  {title:28s} {frag:26s} not found in the trace")
                    continue
                for r in hit:
                    avg = float(r["AverageNs"])
                    say(f"  {title:28s} {frag:26s} {int(r['Calls']):5d} calls  avg {avg / 1e3:9.1f} us  {nbytes / 1e6:8.1f} MB  "
                        f"{nbytes / avg / 1e3:6.2f} TB/s" + (f"  ({nbytes / avg * 1e9 / copy * 100:5.1f} % of the copy)" if copy else "")
                        + ("" if len(hit) == 1 else f"  [{r['Name'][:60]}]"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=40.0, help="least length of a timed window, ms")
    ap.add_argument("--trace", default="", help="directory for rocprofv3 kernel traces of the native losses (per-kernel bytes/s)")
    ap.add_argument("--trace-iters", type=int, default=50)
    ap.add_argument("--traced-child", default="", help="(child of --trace) run the native losses of this group and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_losses.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_class_losses: needs a GPU (a CPU run gives no time)")
    if args.traced_child:
        traced_child(int(args.traced_child), args.trace_iters)
        return
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"class losses, forward + backward, fp32; {torch.cuda.get_device_name(0)}; median of {args.rounds} alternating rounds after "
        f"{args.warmup} warm-up rounds, device events around windows of at least {args.window:.0f} ms")
    say(f"plain device copy of {'x'.join(map(str, BINARY))} f32: {copy_rate() / 1e12:.2f} TB/s (read + write)")
    for title, shape, torch_fn, native, _, _, _ in cases():
        x, t = inputs(shape, shape[1] > 1)
        res = measure((("torch", torch_fn), ("native", native)), x, t, args)
        say(f"\n{title}  {'x'.join(map(str, shape))}  (one tensor = {4 * math.prod(shape) / 1e6:.1f} MB)")
        for name, (ms, lo, hi, reps, peak, val) in res.items():
            say(f"  {name:8s} {ms:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, {reps:3d} per window)   peak +{peak / 1e6:9.1f} MB   loss {val:.7f}")
        tq, nt = res["torch"], res["native"]
        say(f"  torch / native = {tq[0] / nt[0]:.2f}; faster beyond the spread of the rounds: {'yes' if nt[2] < tq[1] else 'NO'}")
        del x, t
        torch.cuda.empty_cache()
    if args.trace:
        trace(args, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
