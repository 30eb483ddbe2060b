"""Time the native DDBPN against the same graph on torch.nn.functional, in one process, and its back-projection kernels alone.

  python scripts/bench_ddbpn.py [--samples 3] [--iters 1] [--op-iters 200] [--out profiles/ddbpn.txt] [--quick] [--trace DIR]

  network   forward + backward (y.sum()) of DDBPN at 16 x 3 x 48 x 48 and 16 x 3 x 96 x 96, scales 2 and 4, bf16 and fp32, with the
            peak device memory of each side.  The composition runs the same weights through F.conv2d / F.conv_transpose2d / F.prelu /
            torch.cat in the same dtype (fp32: as is; bf16: weights and activations cast to bf16), with autograd.
  kernels   srcgan_s2d_shift, srcgan_d2s_shift, srcgan_prelu_forward (crop + bias + residual) and srcgan_prelu_backward (with the
            residual's gradient) alone on a 16 x 384^2 x 32 image / its scale-4 grid, bf16 and fp32: HIP events around --op-iters calls,
            the algorithm's bytes (every operand once) over the time, next to the rate of a device-to-device copy of a 1 GiB tensor
            timed in the same run (read + written bytes over time) and the 8.0 TB/s the part specifies.

HIP events around --iters calls after a warm-up; the modes of a group alternate round-robin inside every sample and the median of the
samples is reported with the spread (max - min).  No threshold is set: whatever is measured is reported, including the cases the
composition wins.

--trace DIR starts `rocprofv3 --kernel-trace --stats` (no counters) on a child process that runs only the four kernels, under
`timeout`, and prints each kernel's average time and achieved bytes/s from the kernel statistics.  Needs a GPU: there is no fallback."""
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
HBM_SPEC = 8.0e12
PROJ = {2: (6, 2, 2), 4: (8, 4, 2), 8: (12, 8, 2)}


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


def composition(w, x, scale):
    """DDBPN from a dict of weights with torch.nn.functional, in x's dtype."""
    k, s, p = PROJ[scale]

    def proj(t, name, up):
        f = F.conv_transpose2d if up else F.conv2d
        return F.prelu(f(t, w[name + ".0.weight"], w[name + ".0.bias"], stride=s, padding=p), w[name + ".1.weight"])

    def module(t, name, up, bottleneck):
        if bottleneck:
            t = F.prelu(F.conv2d(t, w[name + ".bottleneck.0.weight"], w[name + ".bottleneck.0.bias"]), w[name + ".bottleneck.1.weight"])
        a0 = proj(t, name + ".conv_1", up)
        e = proj(a0, name + ".conv_2", not up) - t
        return a0 + proj(e, name + ".conv_3", up)

    t = F.conv2d(x, w["sub_mean.weight"], w["sub_mean.bias"])
    t = F.prelu(F.conv2d(t, w["initial.0.weight"], w["initial.0.bias"], padding=1), w["initial.1.weight"])
    t = F.prelu(F.conv2d(t, w["initial.2.weight"], w["initial.2.bias"]), w["initial.3.weight"])
    hs, ls = [], []
    for i in range(5):
        hs.append(module(t if i == 0 else torch.cat(ls, 1), f"upmodules.{i}", True, i > 1))
        ls.append(module(torch.cat(hs, 1), f"downmodules.{i}", False, i != 0))
    hs.append(module(torch.cat(ls, 1), "upmodules.5", True, True))
    t = F.conv2d(torch.cat(hs, 1), w["reconstruction.0.weight"], w["reconstruction.0.bias"], padding=1)
    return F.conv2d(t, w["add_mean.weight"], w["add_mean.bias"])


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def bench_network(a, say):
    import srcgan_amd as S
    for scale in (2, 4):
        for dtype in ("bf16", "fp32"):
            td = torch.bfloat16 if dtype == "bf16" else torch.float32
            torch.manual_seed(0)
            net = S.DDBPN(scale=scale, rgb_range=1, dtype=dtype).cuda()
            frozen = {k for k, p in net.named_parameters() if not p.requires_grad}
            w = {k: v.detach().to(td).requires_grad_(k not in frozen) for k, v in net.state_dict().items()}
            for hw in ((8,) if a.quick else (48, 96)):
                x = torch.rand(2 if a.quick else 16, 3, hw, hw, device="cuda")
                xt = x.to(td)

                def native():
                    net(x).sum().backward()

                def torch_f():
                    composition(w, xt, scale).float().sum().backward()

                with torch.no_grad():
                    ref = composition(w, xt, scale).float()
                    rel = float((net(x) - ref).norm() / ref.norm())
                    del ref
                peak = {"native": peak_of(native), "torch": peak_of(torch_f)}
                r = timed([("native", native), ("torch", torch_f)], a.samples, a.iters)
                say(json.dumps({"what": "DDBPN forward+backward", "cfg": f"x{scale} {dtype} {tuple(x.shape)}",
                                "native_ms": round(r["native"][0], 3), "native_spread_ms": round(r["native"][1], 3),
                                "torch_ms": round(r["torch"][0], 3), "torch_spread_ms": round(r["torch"][1], 3),
                                "torch_over_native": round(r["torch"][0] / r["native"][0], 3),
                                "native_peak_MiB": round(peak["native"]), "torch_peak_MiB": round(peak["torch"]),
                                "output_rel_l2_native_vs_torch": float(f"{rel:.3g}")}))
                for p in net.parameters():
                    p.grad = None
                for v in w.values():
                    v.grad = None
            del net, w
            torch.cuda.empty_cache()


def kernel_calls(a, dtype):
    """the four calls on one scale-4 case -> [(name, bytes, fn)]"""
    from srcgan_amd import _native as N
    lib = N.lib()
    B, h, C, s, shift = (2, 8, 32, 4, 2) if a.quick else (16, 96, 32, 4, 2)
    Hy, Hg = s * h, h + 1
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    esz = 2 if dtype == "bf16" else 4
    did = N.dtype_id(dtype)
    g = torch.Generator(device="cuda").manual_seed(1)
    img = lambda: torch.randn(B, Hy, Hy, C, device="cuda", generator=g).to(td)
    x, r, dy, y, dres = img(), img(), img(), img(), img()
    grid = torch.randn(B, Hg, Hg, s * s * C, device="cuda", generator=g).to(td)
    dz = torch.empty_like(grid)
    slope = torch.rand(C, device="cuda", generator=g)
    bias = torch.randn(C, device="cuda", generator=g)
    da, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    scr = torch.empty(lib.srcgan_prelu_scratch_floats(B, Hg, Hg, C, s), device="cuda")
    st = N.stream_ptr(torch.device("cuda"))
    p = lambda v: v.data_ptr()
    n, ng = x.numel() * esz, grid.numel() * esz
    keep = (x, r, dy, y, dres, grid, dz, slope, bias, da, db, scr)

    def gather():
        N.check(lib.srcgan_s2d_shift(p(x), C, p(grid), s * s * C, B, Hy, Hy, C, s, shift, Hg, Hg, did, st), "srcgan_s2d_shift")

    def crop():
        N.check(lib.srcgan_d2s_shift(p(grid), s * s * C, p(y), C, B, Hy, Hy, C, s, shift, Hg, Hg, 0, did, st), "srcgan_d2s_shift")

    def fwd():
        N.check(lib.srcgan_prelu_forward(p(grid), s * s * C, p(slope), p(bias), p(r), C, -1.0, p(y), C, B, Hy, Hy, C, s, shift, Hg, Hg, did, st), "srcgan_prelu_forward")

    def bwd():
        N.check(lib.srcgan_prelu_backward(p(dy), C, p(grid), s * s * C, p(slope), p(bias), p(dz), s * s * C, p(dres), C, -1.0, 0, p(da), p(db), B, Hy, Hy, C, s,
                                          shift, Hg, Hg, did, p(scr), st), "srcgan_prelu_backward")

    return [("s2d_shift", n + ng, gather), ("d2s_shift", n + ng, crop), ("prelu_forward", 2 * n + ng, fwd), ("prelu_backward", 2 * n + 2 * ng, bwd)], keep, (B, Hy, C)


def bench_kernels(a, say, copy_bps, only=None):
    for dtype in ((only,) if only else ("bf16", "fp32")):
        calls, keep, (B, Hy, C) = kernel_calls(a, dtype)
        if only:                      # the traced child: the kernels alone
            for _ in range(a.op_iters):
                for _, _, fn in calls:
                    fn()
            torch.cuda.synchronize()
            return
        r = timed([(name, fn) for name, _, fn in calls], a.samples, a.op_iters)
        for name, nbytes, _ in calls:
            say(json.dumps({"what": "kernel call", "name": name, "cfg": f"{B}x{Hy}x{Hy}x{C} scale 4 {dtype}", "us": round(r[name][0] * 1e3, 1),
                            "spread_us": round(r[name][1] * 1e3, 1), "bytes": nbytes, "GBps": round(nbytes / (r[name][0] * 1e-3) / 1e9, 1),
                            "copy_1GiB_GBps": round(copy_bps / 1e9, 1), "hbm_spec_GBps": HBM_SPEC / 1e9}))
        del keep


def trace(a, say, copy_bps):
    """per-kernel times of the four calls from rocprofv3's kernel statistics, one child process per dtype"""
    for dtype in ("bf16", "fp32"):
        out = os.path.join(a.trace, dtype)
        os.makedirs(out, exist_ok=True)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "bp", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--traced-child", dtype, "--op-iters", str(min(a.op_iters, 50))] + (["--quick"] if a.quick else [])
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL).returncode
        if rc != 0:
            raise SystemExit(f"rocprofv3 run failed with status {rc}")
        rows = []
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += list(csv.DictReader(f))
        calls, keep, (B, Hy, C) = kernel_calls(a, dtype)
        nbytes = {"bp_copy_k": calls[0][1], "prelu_fwd_k": calls[2][1], "prelu_bwd_k": calls[3][1], "prelu_finish_k": 0}
        del keep
        for r in rows:
            for key, nb in nbytes.items():
                if key in r["Name"]:
                    avg = float(r["AverageNs"])
                    say(json.dumps({"what": "kernel (trace)", "dtype": dtype, "cfg": f"{B}x{Hy}x{Hy}x{C} scale 4", "name": key, "instance": r["Name"][:96],
                                    "calls": int(r["Calls"]), "avg_us": round(avg / 1e3, 2), "bytes": nb, "GBps": round(nb / avg, 1) if nb else None,
                                    "copy_1GiB_GBps": round(copy_bps / 1e9, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--op-iters", type=int, default=200)
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of the four kernels (per-kernel bytes/s)")
    ap.add_argument("--traced-child", default="", help="(child of --trace) run the kernels in this dtype and exit")
    ap.add_argument("--out", default="profiles/ddbpn.txt")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ddbpn.py needs a GPU")
    if a.traced_child:
        bench_kernels(a, print, 0.0, only=a.traced_child)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"# scripts/bench_ddbpn.py --samples {a.samples} --iters {a.iters} --op-iters {a.op_iters}" + (" --quick" if a.quick else "") +
            f"  ({torch.cuda.get_device_name(0)}; medians of {a.samples} samples, modes alternating)")
        rate = copy_rate()
        bench_kernels(a, say, rate)
        if a.trace:
            trace(a, say, rate)
        bench_network(a, say)


if __name__ == "__main__":
    main()
