"""Time the native UnetGenerator against the same graph on torch.nn.functional, in one process.

  python scripts/bench_unet.py [--samples 3] [--iters 1] [--out profiles/unet.txt] [--quick] [--trace DIR]

  network   forward + backward (y.sum()) and the no_grad forward of `init_net(UnetGenerator(., ., num_downs, 64, get_norm_layer('instance')))`,
            what the reference's define_G builds for 'unet_256' / 'unet_128', in bf16 and fp32: num_downs 8, 3 -> 1 channels at
            16 x 3 x 256 x 256 and num_downs 7, 1 -> 3 at 16 x 1 x 128 x 128, with the peak device memory of each side.  The composition runs
            the same weights through F.conv2d / F.leaky_relu / F.instance_norm / F.conv_transpose2d / torch.cat / torch.tanh in the same dtype
            (fp32: as is; bf16: weights and activations cast to bf16).
  classes   the native step's time per kernel class from the library's launch profiler (srcgan_prof_*): where the time of the
            convolutions goes (the norm, ReLU and tanh kernels are not profiled launches).
  trace     --trace DIR starts `rocprofv3 --kernel-trace` (no counters) on a child process, under `timeout`, that runs the fused
            two-output norm and srcgan_relu_nhwc alone on the network's tensor shapes and a 1 GiB device-to-device copy, and prints each
            kernel's median duration and the bytes it reads + writes per second next to the copy's, all from the per-dispatch kernel trace
            of that one run.

HIP events around --iters calls after a warm-up; the modes of a group alternate round-robin inside every sample and the median of the
samples is reported with the spread (max - min).  No threshold is set: whatever is measured is reported, including the cases the
composition wins.  Needs a GPU."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
NGF = 64
REPS = 5
# (B, hw, C) of the trace: the two-output norm at levels 2 and 4 of unet_256 on 256 x 256, the outermost ReLU (level 1)
NORM_SHAPES = ((16, 64 * 64, 128), (16, 16 * 16, 512))
RELU_SHAPE = (16 * 128 * 128, 64)


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


def module_names(n):
    """(down convolutions outermost first, transposed convolutions innermost first): the class's state_dict keys without .weight / .bias"""
    pre = lambda l: "model.model" + "".join((".1" if k == 2 else ".3") + ".model" for k in range(2, l + 1))
    down = [pre(1) + ".0"] + [pre(l) + ".1" for l in range(2, n + 1)]
    up = [pre(n) + ".3"] + [pre(l) + ".5" for l in range(n - 1, 1, -1)] + [pre(1) + ".3"]
    return down, up


def composition(w, x, n):
    """the U-Net translator from a dict of weights (the class's state_dict keys) with torch.nn.functional and torch.cat, in x's dtype"""
    down, up = module_names(n)
    cv = lambda t, m: F.conv2d(t, w[m + ".weight"], w[m + ".bias"], stride=2, padding=1)
    dc = lambda t, m: F.conv_transpose2d(t, w[m + ".weight"], w[m + ".bias"], stride=2, padding=1)
    skips = [cv(x, down[0])]
    for l in range(2, n):
        skips.append(F.instance_norm(cv(F.leaky_relu(skips[-1], 0.2), down[l - 1])))
    h = F.relu(cv(F.leaky_relu(skips[-1], 0.2), down[n - 1]))
    for k, l in enumerate(range(n - 1, 0, -1)):
        h = F.relu(torch.cat([skips[l - 1], F.instance_norm(dc(h, up[k]))], 1))
    return torch.tanh(dc(h, up[n - 1]))


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


def make(cin, cout, n, dtype, quick):
    import srcgan_amd as S
    torch.manual_seed(0)
    net = S.init_net(S.UnetGenerator(cin, cout, n, 16 if quick else NGF, norm_layer=S.get_norm_layer("instance"), dtype=dtype), "normal", 0.02)
    return net.cuda()


def bench_network(a, say):
    from srcgan_amd import _native as N
    for cin, cout, n, B, hw in ((3, 1, 8, 16, 256), (1, 3, 7, 16, 128)):
        if a.quick:
            n, B, hw = 5, 2, 32
        for dtype in ("bf16", "fp32"):
            td = torch.bfloat16 if dtype == "bf16" else torch.float32
            net = make(cin, cout, n, dtype, a.quick)
            w = {k: v.detach().to(td).requires_grad_(True) for k, v in net.state_dict().items()}
            x = torch.rand(B, cin, hw, hw, device="cuda")
            xt = x.to(td)

            def native():
                net(x).sum().backward()

            def torch_f():
                composition(w, xt, n).float().sum().backward()

            def native_ng():
                with torch.no_grad():
                    net(x)

            def torch_ng():
                with torch.no_grad():
                    composition(w, xt, n)

            with torch.no_grad():
                ref = composition(w, xt, n).float()
                rel = float((net(x) - ref).norm() / ref.norm())
                del ref
            peak = {k: peak_of(fn) for k, fn in (("native", native), ("torch", torch_f), ("native_ng", native_ng), ("torch_ng", torch_ng))}
            clear(net, w)
            r = timed([("native", native), ("torch", torch_f)], a.samples, a.iters)
            clear(net, w)
            g = timed([("native", native_ng), ("torch", torch_ng)], a.samples, a.iters)
            cfg = f"unet num_downs {n} ngf {16 if a.quick else NGF} {cin} -> {cout} {dtype} {tuple(x.shape)}"
            say(json.dumps({"what": "forward+backward", "cfg": cfg, "native_ms": round(r["native"][0], 3), "native_spread_ms": round(r["native"][1], 3),
                            "torch_ms": round(r["torch"][0], 3), "torch_spread_ms": round(r["torch"][1], 3),
                            "torch_over_native": round(r["torch"][0] / r["native"][0], 3), "native_peak_MiB": round(peak["native"]),
                            "torch_peak_MiB": round(peak["torch"]), "output_rel_l2_native_vs_torch": float(f"{rel:.3g}")}))
            say(json.dumps({"what": "no_grad forward", "cfg": cfg, "native_ms": round(g["native"][0], 3), "native_spread_ms": round(g["native"][1], 3),
                            "torch_ms": round(g["torch"][0], 3), "torch_spread_ms": round(g["torch"][1], 3),
                            "torch_over_native": round(g["torch"][0] / g["native"][0], 3), "native_peak_MiB": round(peak["native_ng"]),
                            "torch_peak_MiB": round(peak["torch_ng"])}))
            clear(net, w)
            N.prof_enable(True)
            N.prof_collect()
            native()
            torch.cuda.synchronize()
            rows = sorted(N.prof_collect(), key=lambda q: -q["ms"])
            N.prof_enable(False)
            total = sum(q["ms"] for q in rows) or 1.0
            for q in rows[:6]:
                say(json.dumps({"what": "kernel class (one step, profiled launches)", "cfg": cfg, "class": q["cls"], "launches": q["count"], "ms": round(q["ms"], 3),
                                "share_of_profiled": round(q["ms"] / total, 3)}))
            say(json.dumps({"what": "step", "cfg": cfg, "step_ms_events": round(r["native"][0], 3), "profiled_launch_ms_sum": round(total, 3),
                            "launches": sum(q["count"] for q in rows)}))
            del net, w
            torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- the kernels alone, traced
def trace_plan(quick):
    """[(label, kernel name part, bytes moved)] in the order the child launches them, each REPS times; the copy comes last"""
    plan = []
    for dtype, esz in (("bf16", 2), ("fp32", 4)):
        for (B, hw, C) in NORM_SHAPES:
            if quick:
                B, hw = 2, 64
            n = B * hw * C * esz
            plan.append((f"in_skip_forward apply {dtype} ({B}, {hw}, {C}): one read, two writes", "in_skip_apply_k", 3 * n))
        n = (1024 if quick else RELU_SHAPE[0]) * RELU_SHAPE[1] * esz
        plan.append((f"relu_nhwc {dtype} {RELU_SHAPE}", "relu_nhwc_k", 2 * n))
    return plan


def traced_child(quick):
    from srcgan_amd import _native as N
    lib, st = N.lib(), N.stream_ptr(torch.device("cuda"))
    for dtype, td in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        did = N.dtype_id(dtype)
        for (B, hw, C) in NORM_SHAPES:
            if quick:
                B, hw = 2, 64
            x = torch.randn(B * hw, C, device="cuda").to(td)
            a_, r_ = torch.empty_like(x), torch.empty(B * hw, 2 * C, device="cuda", dtype=td)
            stats = torch.empty(B * C * 2, device="cuda")
            scr = torch.empty(lib.srcgan_gn_scratch_floats(B, C), device="cuda")
            for _ in range(REPS):
                N.check(lib.srcgan_in_skip_forward(x.data_ptr(), C, a_.data_ptr(), C, r_.data_ptr(), 2 * C, 0, stats.data_ptr(), B, hw, C, 1e-5, 0.2, did,
                                                   scr.data_ptr(), st), "in_skip")
            del x, a_, r_
        npix, C = (1024 if quick else RELU_SHAPE[0]), RELU_SHAPE[1]
        z, y = torch.randn(npix, C, device="cuda").to(td), torch.empty(npix, 2 * C, device="cuda", dtype=td)
        for _ in range(REPS):
            N.check(lib.srcgan_relu_nhwc(z.data_ptr(), C, y.data_ptr(), 2 * C, 0, npix, C, did, st), "relu")
        del z, y
    torch.cuda.synchronize()
    src = torch.rand(1 << 28, device="cuda")            # 1 GiB of f32
    dst = torch.empty_like(src)
    for _ in range(REPS):
        torch.add(src, 1.0, out=dst)                    # an elementwise kernel (a plain copy may run on a DMA engine, outside the kernel trace)
    torch.cuda.synchronize()


def trace(a, say):
    out = a.trace
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "-d", out, "-o", "unet", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--traced-child"] + (["--quick"] if a.quick else [])
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL).returncode
    if rc != 0:
        raise SystemExit(f"rocprofv3 run failed with status {rc}")
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    ours = [r for r in rows if any(s in r["Kernel_Name"] for s in ("in_skip_apply_k", "relu_nhwc_k"))]
    plan = trace_plan(a.quick)
    if len(ours) != REPS * len(plan):
        raise SystemExit(f"the trace holds {len(ours)} launches of the skip kernels, {REPS * len(plan)} were made")
    big = (1 << 28) * 4
    copies = [dur(r) for r in rows if "elementwise" in r["Kernel_Name"] and dur(r) > 50.0][-REPS:]
    copy_us = statistics.median(copies) if len(copies) == REPS else None
    copy_gbps = round(2 * big / (copy_us * 1e-6) / 1e9, 1) if copy_us else "not measured"
    for i, (label, part, nbytes) in enumerate(plan):
        grp = ours[i * REPS:(i + 1) * REPS]
        assert all(part in r["Kernel_Name"] for r in grp), (label, grp[0]["Kernel_Name"])
        us = statistics.median(dur(r) for r in grp)
        say(json.dumps({"what": "kernel (trace)", "call": label, "kernel": grp[0]["Kernel_Name"][:60], "median_us": round(us, 2), "MB_moved": round(nbytes / 1e6, 1),
                        "GBps": round(nbytes / (us * 1e-6) / 1e9, 1), "copy_1GiB_GBps_same_run": copy_gbps}))
    say(json.dumps({"what": "1 GiB elementwise copy (trace)", "median_us": round(copy_us, 1) if copy_us else "not measured", "GBps_read_plus_written": copy_gbps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of the skip kernels and a 1 GiB copy")
    ap.add_argument("--traced-child", action="store_true", help="(child of --trace) run the kernels alone and exit")
    ap.add_argument("--out", default="profiles/unet.txt")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unet.py needs a GPU")
    if a.traced_child:
        traced_child(a.quick)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"# scripts/bench_unet.py --samples {a.samples} --iters {a.iters}" + (" --quick" if a.quick else "") +
            f"  ({torch.cuda.get_device_name(0)}; medians of {a.samples} samples, modes alternating)")
        if a.trace:
            trace(a, say)
        bench_network(a, say)


if __name__ == "__main__":
    main()
