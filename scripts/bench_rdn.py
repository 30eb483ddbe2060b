"""Time the native RDN against the same graph on torch.nn.functional (with torch.cat), in one process.

  python scripts/bench_rdn.py [--samples 3] [--iters 1] [--out profiles/rdn.txt] [--quick] [--trace DIR] [--only A|B]

  network   forward + backward (y.sum()) of RDN 'A' and 'B', x2, bf16 and fp32, at 16 x 3 x 48 x 48 and 16 x 3 x 96 x 96, with the peak
            device memory of each side, and the no_grad forward of both.  The composition runs the same weights through F.conv2d /
            F.relu / torch.cat / F.pixel_shuffle in the same dtype (fp32: as is; bf16: weights and activations cast to bf16).
  classes   the native step's time per kernel class from the library's launch profiler (srcgan_prof_*), for one step of each
            configuration at 16 x 3 x 48 x 48 in bf16: where the time goes.
  gff       the D small launches of GFF.0's K slices: one slice's forward, input-gradient and weight-gradient calls alone
            (1x1, G0 -> G0, on the network's tensors' shapes), HIP events around --op-iters calls; D times their sum over the step time
            is the share of the step spent in them.
  prefixes  the bytes the backward re-reads and re-writes because every dense layer's input gradient is added in place to the range it
            read (layer c: G0 + c G channels read and written where one writer per slice would write G0 + c G once), per step, and
            the time those bytes take at the rate of a device-to-device copy measured in the same run, as a share of the step.

HIP events around --iters calls after a warm-up; the modes of a group alternate round-robin inside every sample and the median of the
samples is reported with the spread (max - min).  No threshold is set: whatever is measured is reported, including the cases the
composition wins.

--trace DIR starts `rocprofv3 --kernel-trace --stats` (no counters) on a child process that runs a few training steps of 'A' x2 bf16 at
16 x 3 x 48 x 48, under `timeout`, and prints the kernels' calls, average and total time from the kernel statistics.  Needs a GPU."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
CONFIGS = {"A": (20, 6, 32), "B": (16, 8, 64)}
G0 = 64


def timed(modes, samples, iters):
    ms = {name: [] for name, _ in modes}
    for _, fn in modes:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(samples):
        for name, fn in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    return {k: (sorted(v)[len(v) // 2], max(v) - min(v)) for k, v in ms.items()}


def copy_rate():
    """read + written bytes per second of a device-to-device copy of 1 GiB (median of 5 windows of 20 copies)"""
    src = torch.empty(1 << 28, device="cuda").normal_()
    dst = torch.empty_like(src)
    r = timed([("copy", lambda: dst.copy_(src))], 5, 20)
    return 2.0 * src.numel() * 4 / (r["copy"][0] * 1e-3)


def composition(w, x, config, scale):
    """RDN from a dict of weights with torch.nn.functional, in x's dtype."""
    D, C, _ = CONFIGS[config]
    conv = lambda t, name, pad: F.conv2d(t, w[name + ".weight"], w[name + ".bias"], padding=pad)
    f1 = conv(x, "SFENet1", 1)
    t = conv(f1, "SFENet2", 1)
    outs = []
    for d in range(D):
        buf = t
        for c in range(C):
            buf = torch.cat((buf, F.relu(conv(buf, f"RDBs.{d}.convs.{c}.conv.0", 1))), 1)
        t = conv(buf, f"RDBs.{d}.LFF", 0) + t
        outs.append(t)
    t = conv(conv(torch.cat(outs, 1), "GFF.0", 0), "GFF.1", 1) + f1
    t = F.pixel_shuffle(conv(t, "UPNet.0", 1), 2 if scale == 4 else scale)
    if scale == 4:
        return conv(F.pixel_shuffle(conv(t, "UPNet.2", 1), 2), "UPNet.4", 1)
    return conv(t, "UPNet.2", 1)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def clear(net, w):
    for p in net.parameters():
        p.grad = None
    for v in w.values():
        v.grad = None


def bench_network(a, say):
    import srcgan_amd as S
    scale = 2
    for config in ([a.only] if a.only else ["A", "B"]):
        for dtype in ("bf16", "fp32"):
            td = torch.bfloat16 if dtype == "bf16" else torch.float32
            torch.manual_seed(0)
            net = S.RDN(scale=scale, G0=G0, RDNconfig=config, dtype=dtype).cuda()
            w = {k: v.detach().to(td).requires_grad_(True) for k, v in net.state_dict().items()}
            for hw in ((8,) if a.quick else (48, 96)):
                x = torch.rand(2 if a.quick else 16, 3, hw, hw, device="cuda")
                xt = x.to(td)

                def native():
                    net(x).sum().backward()

                def torch_f():
                    composition(w, xt, config, scale).float().sum().backward()

                def native_ng():
                    with torch.no_grad():
                        net(x)

                def torch_ng():
                    with torch.no_grad():
                        composition(w, xt, config, scale)

                with torch.no_grad():
                    ref = composition(w, xt, config, scale).float()
                    rel = float((net(x) - ref).norm() / ref.norm())
                    del ref
                peak = {k: peak_of(fn) for k, fn in (("native", native), ("torch", torch_f), ("native_ng", native_ng), ("torch_ng", torch_ng))}
                clear(net, w)
                r = timed([("native", native), ("torch", torch_f)], a.samples, a.iters)
                clear(net, w)
                g = timed([("native", native_ng), ("torch", torch_ng)], a.samples, a.iters)
                cfg = f"'{config}' x{scale} {dtype} {tuple(x.shape)}"
                say(json.dumps({"what": "RDN forward+backward", "cfg": cfg, "native_ms": round(r["native"][0], 3), "native_spread_ms": round(r["native"][1], 3),
                                "torch_ms": round(r["torch"][0], 3), "torch_spread_ms": round(r["torch"][1], 3),
                                "torch_over_native": round(r["torch"][0] / r["native"][0], 3), "native_peak_MiB": round(peak["native"]),
                                "torch_peak_MiB": round(peak["torch"]), "output_rel_l2_native_vs_torch": float(f"{rel:.3g}")}))
                say(json.dumps({"what": "RDN no_grad forward", "cfg": cfg, "native_ms": round(g["native"][0], 3), "native_spread_ms": round(g["native"][1], 3),
                                "torch_ms": round(g["torch"][0], 3), "torch_spread_ms": round(g["torch"][1], 3),
                                "torch_over_native": round(g["torch"][0] / g["native"][0], 3), "native_peak_MiB": round(peak["native_ng"]),
                                "torch_peak_MiB": round(peak["torch_ng"])}))
            del net, w
            torch.cuda.empty_cache()


def step_of(config, dtype, B, hw):
    import srcgan_amd as S
    torch.manual_seed(0)
    net = S.RDN(scale=2, G0=G0, RDNconfig=config, dtype=dtype).cuda()
    x = torch.rand(B, 3, hw, hw, device="cuda")

    def step():
        net(x).sum().backward()
    return net, step


def bench_classes(a, say, copy_bps):
    """per-class times of one step, the GFF slices' launches alone, and the bytes of the in-place gradient prefixes"""
    from srcgan_amd import _native as N, ops
    B, hw = (2, 8) if a.quick else (16, 48)
    for config in ([a.only] if a.only else ["A", "B"]):
        D, C, G = CONFIGS[config]
        net, step = step_of(config, "bf16", B, hw)
        step_ms = timed([("step", step)], a.samples, a.iters)["step"][0]
        N.prof_enable(True)
        N.prof_collect()
        step()
        torch.cuda.synchronize()
        rows = sorted(N.prof_collect(), key=lambda r: -r["ms"])
        N.prof_enable(False)
        total = sum(r["ms"] for r in rows)
        cfg = f"'{config}' x2 bf16 ({B}, 3, {hw}, {hw})"
        for r in rows[:12]:
            say(json.dumps({"what": "kernel class (one step, profiled launches)", "cfg": cfg, "class": r["cls"], "launches": r["count"], "ms": round(r["ms"], 3),
                            "share_of_profiled": round(r["ms"] / total, 3)}))
        say(json.dumps({"what": "step", "cfg": cfg, "step_ms_events": round(step_ms, 3), "profiled_launch_ms_sum": round(total, 3),
                        "launches": sum(r["count"] for r in rows)}))
        # one GFF.0 slice: forward (+ accumulator), input gradient added to a dense buffer's prefix, weight gradient into its columns
        Cb, T = G0 + C * G, torch.bfloat16
        xb = torch.randn(B, hw, hw, Cb, device="cuda").to(T)
        gb = torch.randn(B, hw, hw, Cb, device="cuda").to(T)
        acc0, acc1, dacc = (torch.randn(B, hw, hw, G0, device="cuda").to(T) for _ in range(3))
        wfull = torch.randn(G0, D * G0, 1, 1, device="cuda") * 0.05
        wgrad = torch.zeros_like(wfull)
        wf = ops.pack_weight(wfull, G0, G0, 1, 1, D * G0, 1, 1, 1, G0, T)
        wd = ops.pack_weight(wfull, G0, G0, 1, 1, 1, D * G0, -1, -1, G0, T)
        fwd = lambda: ops.conv_igemm(xb, wf, acc1, kh=1, kw=1, Cin=G0, Cout=G0, r1=acc0, r1_cend=G0, beta1=1.0)
        dgr = lambda: ops.conv_igemm(dacc, wd, gb, kh=1, kw=1, Cin=G0, Cout=G0, r1=gb, r1_cend=G0, beta1=1.0)
        wgr = lambda: ops.conv_wgrad(dacc, xb, wgrad, kh=1, kw=1, Cout=G0, Cin=G0, layout=(D * G0, 1, 1, 1, G0))
        r = timed([("fwd", fwd), ("dgrad", dgr), ("wgrad", wgr)], a.samples, a.op_iters)
        one = r["fwd"][0] + r["dgrad"][0] + r["wgrad"][0]
        say(json.dumps({"what": "GFF.0 slices", "cfg": cfg, "slice_forward_us": round(r["fwd"][0] * 1e3, 1), "slice_dgrad_us": round(r["dgrad"][0] * 1e3, 1),
                        "slice_wgrad_us_incl_slab_alloc": round(r["wgrad"][0] * 1e3, 1), "D": D, "D_slices_ms": round(D * one, 3),
                        "share_of_step": round(D * one / step_ms, 4)}))
        # in-place gradient prefixes: layer c > 0 reads (r1) and writes G0 + c G channels of the block's gradient buffer; with one writer per
        # slice the buffer would be written once.  Extra bytes = the r1 reads + the writes beyond the first.
        npix, esz = B * hw * hw, 2
        touched = sum(G0 + c * G for c in range(C))                      # channels written by the C input gradients of a block
        extra = D * npix * esz * (2 * touched - Cb)                       # reads of the old value + writes, minus one write of the buffer
        ms_extra = extra / copy_bps * 1e3
        say(json.dumps({"what": "in-place gradient prefixes", "cfg": cfg, "extra_bytes_per_step": extra, "buffer_touches_per_block": round(2 * touched / Cb, 2),
                        "ms_at_copy_rate": round(ms_extra, 3), "copy_1GiB_GBps": round(copy_bps / 1e9, 1), "share_of_step": round(ms_extra / step_ms, 4)}))
        del net
        torch.cuda.empty_cache()


def trace(a, say):
    out = a.trace
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "rdn", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--traced-child", "A"] + (["--quick"] if a.quick else [])
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL).returncode
    if rc != 0:
        raise SystemExit(f"rocprofv3 run failed with status {rc}")
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:16]:
        say(json.dumps({"what": "kernel (trace, 'A' x2 bf16, 3 steps)", "name": r["Name"][:110], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                        "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3), "share": round(float(r["TotalDurationNs"]) / total, 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--op-iters", type=int, default=100)
    ap.add_argument("--only", default="", choices=["", "A", "B"], help="one configuration only")
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of a few training steps (per-kernel view)")
    ap.add_argument("--traced-child", default="", help="(child of --trace) run three steps of this configuration and exit")
    ap.add_argument("--out", default="profiles/rdn.txt")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rdn.py needs a GPU")
    if a.traced_child:
        _, step = step_of(a.traced_child, "bf16", 2 if a.quick else 16, 8 if a.quick else 48)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"# scripts/bench_rdn.py --samples {a.samples} --iters {a.iters} --op-iters {a.op_iters}" + (" --quick" if a.quick else "") +
            (f" --only {a.only}" if a.only else "") + f"  ({torch.cuda.get_device_name(0)}; medians of {a.samples} samples, modes alternating)")
        rate = copy_rate()
        bench_classes(a, say, rate)
        if a.trace:
            trace(a, say)
        bench_network(a, say)


if __name__ == "__main__":
    main()
