"""Time the native MDSR and VDSR against the same graphs on torch.nn.functional, in one process.

  python scripts/bench_mdsr.py [--samples 3] [--iters 1] [--out profiles/mdsr.txt] [--quick] [--trace DIR] [--only mdsr|vdsr]

  network   forward + backward (y.sum()) and the no_grad forward of MDSR r16f64 (scale = [2, 3, 4], each scale_idx) and VDSR r20f64, in
            bf16 and fp32, at 16 x 3 x 48 x 48 and 16 x 3 x 96 x 96, with the peak device memory of each side.  The composition runs
            the same weights through F.conv2d / F.relu / F.pixel_shuffle in the same dtype (fp32: as is; bf16: weights and activations
            cast to bf16).
  classes   the native step's time per kernel class from the library's launch profiler (srcgan_prof_*), for one step of MDSR at each
            scale_idx at 16 x 3 x 48 x 48 in bf16 and fp32: where the time goes, and the share of the profiled launches that are 5x5.
  5x5       the launches the four 5x5 convolutions of pre_process add to a step, alone: forward with bias + ReLU, forward with bias +
            residual, the masked input gradient added in place, the weight gradient (its split-K reduce and slab allocation included)
            and the bias gradient (column reduce), on the network's tensor shapes, HIP events around --op-iters calls; their sum times
            the number of such calls per step over the step time is the share of a step spent in the 5x5 launches.

HIP events around --iters calls after a warm-up; the modes of a group alternate round-robin inside every sample and the median of the
samples is reported with the spread (max - min).  No threshold is set: whatever is measured is reported, including the cases the
composition wins.

--trace DIR starts `rocprofv3 --kernel-trace --stats` (no counters) on a child process that runs a few training steps of MDSR x2 bf16 at
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
SCALES = [2, 3, 4]
MDSR_N, VDSR_N, FEATS = 16, 20, 64


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


def _conv(w, t, name):
    k = w[name + ".weight"].shape[-1]
    return F.conv2d(t, w[name + ".weight"], w[name + ".bias"], padding=k // 2)


def _block(w, t, name):
    return _conv(w, F.relu(_conv(w, t, name + ".body.0")), name + ".body.2") + t


def mdsr_composition(w, x, n, idx):
    """MDSR from a dict of weights with torch.nn.functional, in x's dtype."""
    t = _conv(w, F.conv2d(x, w["sub_mean.weight"], w["sub_mean.bias"]), "head.0")
    p = _block(w, _block(w, t, f"pre_process.{idx}.0"), f"pre_process.{idx}.1")
    t = p
    for k in range(n):
        t = _block(w, t, f"body.{k}")
    t = _conv(w, t, f"body.{n}") + p
    s = SCALES[idx]
    for j in range(1 if s == 3 else {2: 1, 4: 2, 8: 3}[s]):
        t = F.pixel_shuffle(_conv(w, t, f"upsample.{idx}.{2 * j}"), 3 if s == 3 else 2)
    return F.conv2d(_conv(w, t, "tail.0"), w["add_mean.weight"], w["add_mean.bias"])


def vdsr_composition(w, x, n, idx=None):
    s = F.conv2d(x, w["sub_mean.weight"], w["sub_mean.bias"])
    t = s
    for k in range(n - 1):
        t = F.relu(_conv(w, t, f"body.{k}.0"))
    return F.conv2d(_conv(w, t, f"body.{n - 1}.0") + s, w["add_mean.weight"], w["add_mean.bias"])


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


def make(kind, dtype, quick):
    import srcgan_amd as S
    torch.manual_seed(0)
    n = 2 if quick else (MDSR_N if kind == "mdsr" else VDSR_N)
    if kind == "mdsr":
        return S.MDSR(n_resblocks=n, n_feats=FEATS, scale=SCALES, rgb_range=1, dtype=dtype).cuda(), n
    return S.VDSR(n_resblocks=n, n_feats=FEATS, rgb_range=1, dtype=dtype).cuda(), n


def bench_network(a, say):
    for kind in ([a.only] if a.only else ["mdsr", "vdsr"]):
        comp = mdsr_composition if kind == "mdsr" else vdsr_composition
        for dtype in ("bf16", "fp32"):
            td = torch.bfloat16 if dtype == "bf16" else torch.float32
            net, n = make(kind, dtype, a.quick)
            w = {k: v.detach().to(td).requires_grad_("mean" not in k) for k, v in net.state_dict().items()}
            for idx in (range(len(SCALES)) if kind == "mdsr" else [None]):
                if idx is not None:
                    net.set_scale(idx)
                for hw in ((8,) if a.quick else (48, 96)):
                    x = torch.rand(2 if a.quick else 16, 3, hw, hw, device="cuda")
                    xt = x.to(td)

                    def native():
                        net(x).sum().backward()

                    def torch_f():
                        comp(w, xt, n, idx).float().sum().backward()

                    def native_ng():
                        with torch.no_grad():
                            net(x)

                    def torch_ng():
                        with torch.no_grad():
                            comp(w, xt, n, idx)

                    with torch.no_grad():
                        ref = comp(w, xt, n, idx).float()
                        rel = float((net(x) - ref).norm() / ref.norm())
                        del ref
                    peak = {k: peak_of(fn) for k, fn in (("native", native), ("torch", torch_f), ("native_ng", native_ng), ("torch_ng", torch_ng))}
                    clear(net, w)
                    r = timed([("native", native), ("torch", torch_f)], a.samples, a.iters)
                    clear(net, w)
                    g = timed([("native", native_ng), ("torch", torch_ng)], a.samples, a.iters)
                    name = f"MDSR r{n}f{FEATS} x{SCALES[idx]}" if kind == "mdsr" else f"VDSR r{n}f{FEATS}"
                    cfg = f"{name} {dtype} {tuple(x.shape)}"
                    say(json.dumps({"what": "forward+backward", "cfg": cfg, "native_ms": round(r["native"][0], 3), "native_spread_ms": round(r["native"][1], 3),
                                    "torch_ms": round(r["torch"][0], 3), "torch_spread_ms": round(r["torch"][1], 3),
                                    "torch_over_native": round(r["torch"][0] / r["native"][0], 3), "native_peak_MiB": round(peak["native"]),
                                    "torch_peak_MiB": round(peak["torch"]), "output_rel_l2_native_vs_torch": float(f"{rel:.3g}")}))
                    say(json.dumps({"what": "no_grad forward", "cfg": cfg, "native_ms": round(g["native"][0], 3), "native_spread_ms": round(g["native"][1], 3),
                                    "torch_ms": round(g["torch"][0], 3), "torch_spread_ms": round(g["torch"][1], 3),
                                    "torch_over_native": round(g["torch"][0] / g["native"][0], 3), "native_peak_MiB": round(peak["native_ng"]),
                                    "torch_peak_MiB": round(peak["torch_ng"])}))
            del net, w
            torch.cuda.empty_cache()


def step_of(idx, dtype, B, hw, quick):
    net, _ = make("mdsr", dtype, quick)
    net.set_scale(idx)
    x = torch.rand(B, 3, hw, hw, device="cuda")

    def step():
        net(x).sum().backward()
    return net, step


def bench_classes(a, say):
    """per-class times of one MDSR step, and the 5x5 launches alone"""
    from srcgan_amd import _native as N, ops
    B, hw = (2, 8) if a.quick else (16, 48)
    for dtype in ("bf16", "fp32"):
        T = torch.bfloat16 if dtype == "bf16" else torch.float32
        step_ms = {}
        for idx in range(len(SCALES)):
            net, step = step_of(idx, dtype, B, hw, a.quick)
            step_ms[idx] = timed([("step", step)], a.samples, a.iters)["step"][0]
            N.prof_enable(True)
            N.prof_collect()
            step()
            torch.cuda.synchronize()
            rows = sorted(N.prof_collect(), key=lambda r: -r["ms"])
            N.prof_enable(False)
            total = sum(r["ms"] for r in rows)
            cfg = f"MDSR x{SCALES[idx]} {dtype} ({B}, 3, {hw}, {hw})"
            for r in rows[:8]:
                say(json.dumps({"what": "kernel class (one step, profiled launches)", "cfg": cfg, "class": r["cls"], "launches": r["count"], "ms": round(r["ms"], 3),
                                "share_of_profiled": round(r["ms"] / total, 3)}))
            k5 = [r for r in rows if ",5x5," in r["cls"]]
            say(json.dumps({"what": "step", "cfg": cfg, "step_ms_events": round(step_ms[idx], 3), "profiled_launch_ms_sum": round(total, 3),
                            "launches": sum(r["count"] for r in rows), "launches_5x5": sum(r["count"] for r in k5), "ms_5x5": round(sum(r["ms"] for r in k5), 3),
                            "share_5x5_of_profiled": round(sum(r["ms"] for r in k5) / total, 4)}))
            del net
            torch.cuda.empty_cache()
        # the calls of one 5x5 ResBlock convolution, alone, on the trunk's shapes
        C_ = FEATS
        xb, yb, rb, gb = (torch.randn(B, hw, hw, C_, device="cuda").to(T) for _ in range(4))
        wfull = torch.randn(C_, C_, 5, 5, device="cuda") * 0.02
        bias = torch.randn(C_, device="cuda")
        wgrad = torch.zeros_like(wfull)
        wf, wd = ops.pack_conv2d_fwd(wfull, T), ops.pack_conv2d_dgrad_s1(wfull, T)
        k5 = dict(kh=5, kw=5, Cin=C_, Cout=C_, pad=(2, 2))
        fwd_relu = lambda: ops.conv_igemm(xb, wf, yb, bias=bias, act=True, slope=0.0, **k5)
        fwd_res = lambda: ops.conv_igemm(xb, wf, yb, bias=bias, r1=rb, r1_cend=C_, beta1=1.0, **k5)
        dgr = lambda: ops.conv_igemm(yb, wd, gb, r1=gb, r1_cend=C_, beta1=1.0, mz=xb, mslope=0.0, **k5)
        wgr = lambda: ops.conv_wgrad(yb, xb, wgrad, kh=5, kw=5, Cout=C_, Cin=C_, pad=(2, 2), layout=(C_ * 25, 25, 5, 1, 0))
        bgr = lambda: ops.col_sum(yb, C_)
        r = timed([("fwd_relu", fwd_relu), ("fwd_res", fwd_res), ("dgrad", dgr), ("wgrad", wgr), ("bias", bgr)], a.samples, a.op_iters)
        # per step: two convolutions with ReLU, two with the residual; four input gradients, four weight gradients, four bias gradients
        per_step = 2 * r["fwd_relu"][0] + 2 * r["fwd_res"][0] + 4 * (r["dgrad"][0] + r["wgrad"][0] + r["bias"][0])
        say(json.dumps({"what": "5x5 launches alone", "cfg": f"64 -> 64 {dtype} ({B}, {hw}, {hw}, 64)", "forward_relu_us": round(r["fwd_relu"][0] * 1e3, 1),
                        "forward_res_us": round(r["fwd_res"][0] * 1e3, 1), "dgrad_us": round(r["dgrad"][0] * 1e3, 1),
                        "wgrad_us_incl_reduce_and_slab_alloc": round(r["wgrad"][0] * 1e3, 1), "bias_grad_us_incl_scratch_alloc": round(r["bias"][0] * 1e3, 1),
                        "per_step_ms": round(per_step, 3), **{f"share_of_step_x{SCALES[i]}": round(per_step / step_ms[i], 4) for i in step_ms}}))


def trace(a, say):
    out = a.trace
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "mdsr", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--traced-child", "0"] + (["--quick"] if a.quick else [])
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL).returncode
    if rc != 0:
        raise SystemExit(f"rocprofv3 run failed with status {rc}")
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:16]:
        say(json.dumps({"what": "kernel (trace, MDSR x2 bf16, 3 steps)", "name": r["Name"][:110], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                        "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3), "share": round(float(r["TotalDurationNs"]) / total, 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--op-iters", type=int, default=100)
    ap.add_argument("--only", default="", choices=["", "mdsr", "vdsr"], help="one network only")
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of a few training steps (per-kernel view)")
    ap.add_argument("--traced-child", default="", help="(child of --trace) run three steps of MDSR at this scale_idx and exit")
    ap.add_argument("--out", default="profiles/mdsr.txt")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mdsr.py needs a GPU")
    if a.traced_child:
        _, step = step_of(int(a.traced_child), "bf16", 2 if a.quick else 16, 8 if a.quick else 48, a.quick)
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
        say(f"# scripts/bench_mdsr.py --samples {a.samples} --iters {a.iters} --op-iters {a.op_iters}" + (" --quick" if a.quick else "") +
            (f" --only {a.only}" if a.only else "") + f"  ({torch.cuda.get_device_name(0)}; medians of {a.samples} samples, modes alternating)")
        bench_classes(a, say)
        if a.trace:
            trace(a, say)
        bench_network(a, say)


if __name__ == "__main__":
    main()
