"""Time the native RCAN and its channel-attention op against their torch.nn.functional compositions, in one process.

  python scripts/bench_rcan.py [--samples 5] [--iters 3] [--op-iters 1000] [--out profiles/rcan.txt] [--quick] [--trace DIR]

  network   forward + backward (L1-free: y.sum()) of the default RCAN (10 groups x 20 blocks, 64 features, reduction 16, x2) at
            16 x 3 x 48 x 48 and 16 x 3 x 96 x 96, bf16 and fp32.  The composition runs the same weights through F.conv2d /
            F.pixel_shuffle / mean / sigmoid in the same dtype (fp32: as is; bf16: weights and activations cast to bf16), with autograd.
  op        srcgan_ca_forward / srcgan_ca_backward alone at 16 x 96^2 x 64 (reduction 16), bf16 and fp32, against the composition
            mean -> 1x1 conv -> ReLU -> 1x1 conv -> sigmoid -> multiply -> add on a channels-last tensor (forward under no_grad, and
            forward + backward through autograd; the native backward alone is timed too).

HIP events around --iters calls after a warm-up; the modes of a group alternate round-robin inside every sample and the median of the
samples is reported with the spread (max - min); --op-iters 1000 makes an op window 20 - 70 ms.  The op's call-level bytes/s is the
algorithm's traffic (forward: t twice, res once, y once; backward: dy twice, t once, dt once, dres once) over the time of the whole
three-launch call.  It is printed next to the HBM rate: 8.0 TB/s specified, and the rate of a device-to-device copy of a 1 GiB tensor
timed in the same run (read + write bytes over time).

--trace DIR starts `rocprofv3 --kernel-trace --stats` (no counters) on a child process that runs only the native op, under
`timeout`, and prints, from the kernel statistics, the average time and the achieved bytes/s of each of the two bandwidth-bound
kernels per direction (partial sums: E resp. 2 E per element; apply: 3 E) and the gate kernels' time.  Needs a GPU: there is no
fallback."""
import argparse
import csv
import glob
import json
import subprocess
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
HBM_SPEC = 8.0e12


def copy_rate():
    """read + written bytes per second of a device-to-device copy of 1 GiB (median of 5 windows of 20 copies)"""
    src = torch.empty(1 << 28, device="cuda").normal_()
    dst = torch.empty_like(src)
    r = timed([("copy", lambda: dst.copy_(src))], 5, 20)
    return 2.0 * src.numel() * 4 / (r["copy"][0] * 1e-3)


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


def composition(w, x, groups, blocks, scale):
    """RCAN from a dict of weights with torch.nn.functional, in x's dtype."""
    conv = lambda t, k: F.conv2d(t, w[k + ".weight"], w[k + ".bias"], padding=1)
    t = F.conv2d(x, w["sub_mean.weight"], w["sub_mean.bias"])
    head = t = conv(t, "head.0")
    for g in range(groups):
        gin = t
        for b in range(blocks):
            k = f"body.{g}.body.{b}.body."
            xin = t
            t = conv(torch.relu(conv(xin, k + "0")), k + "2")
            s = torch.sigmoid(F.conv2d(torch.relu(F.conv2d(t.mean(dim=(2, 3), keepdim=True), w[k + "3.conv_du.0.weight"], w[k + "3.conv_du.0.bias"])),
                                       w[k + "3.conv_du.2.weight"], w[k + "3.conv_du.2.bias"]))
            t = t * s + xin
        t = conv(t, f"body.{g}.body.{blocks}") + gin
    t = conv(t, f"body.{groups}") + head
    for i in range({2: 1, 4: 2, 8: 3}[scale]):
        t = F.pixel_shuffle(conv(t, f"tail.0.{2 * i}"), 2)
    return F.conv2d(conv(t, "tail.1"), w["add_mean.weight"], w["add_mean.bias"])


def bench_network(a, say):
    import srcgan_amd as S
    groups, blocks = (2, 2) if a.quick else (10, 20)
    for dtype in ("bf16", "fp32"):
        td = torch.bfloat16 if dtype == "bf16" else torch.float32
        torch.manual_seed(0)
        net = S.RCAN(n_resgroups=groups, n_resblocks=blocks, n_feats=64, reduction=16, scale=2, rgb_range=1, dtype=dtype).cuda()
        frozen = {k for k, p in net.named_parameters() if not p.requires_grad}
        w = {k: v.detach().to(td).requires_grad_(k not in frozen) for k, v in net.state_dict().items()}
        for hw in ((16,) if a.quick else (48, 96)):
            x = torch.rand(16, 3, hw, hw, device="cuda")
            xt = x.to(td)

            def native():
                net(x).sum().backward()

            def torch_f():
                composition(w, xt, groups, blocks, 2).float().sum().backward()

            with torch.no_grad():
                ref = composition(w, xt, groups, blocks, 2).float()
                rel = float((net(x) - ref).norm() / ref.norm())
            r = timed([("native", native), ("torch", torch_f)], a.samples, a.iters)
            say(json.dumps({"what": "RCAN forward+backward", "cfg": f"{groups}x{blocks} F=64 x2 {dtype} 16x3x{hw}x{hw}",
                            "native_ms": round(r["native"][0], 3), "native_spread_ms": round(r["native"][1], 3),
                            "torch_ms": round(r["torch"][0], 3), "torch_spread_ms": round(r["torch"][1], 3),
                            "torch_over_native": round(r["torch"][0] / r["native"][0], 3), "output_rel_l2_native_vs_torch": float(f"{rel:.3g}")}))
        del net, w
        torch.cuda.empty_cache()


def bench_op(a, say, copy_bps=0.0, only=None):
    from srcgan_amd import _native as N
    lib = N.lib()
    B, H, Cc, Cr = 16, (16 if a.quick else 96), 64, 4
    hw = H * H
    for dtype in ((only,) if only else ("bf16", "fp32")):
        td = torch.bfloat16 if dtype == "bf16" else torch.float32
        esz = 2 if dtype == "bf16" else 4
        did = N.dtype_id(dtype)
        g = torch.Generator(device="cuda").manual_seed(1)
        t, res, dy = (torch.randn(B, hw, Cc, device="cuda", generator=g).to(td) for _ in range(3))
        w1 = torch.randn(Cr, Cc, device="cuda", generator=g) / 8
        b1 = torch.zeros(Cr, device="cuda") + 0.1
        w2 = torch.randn(Cc, Cr, device="cuda", generator=g) / 2
        b2 = torch.zeros(Cc, device="cuda")
        y, dt, dres = torch.empty_like(t), torch.empty_like(t), torch.empty_like(t)
        saved = torch.empty(B * (2 * Cc + Cr), device="cuda")
        scr = torch.empty(lib.srcgan_ca_scratch_floats(B, hw, Cc), device="cuda")
        dw = [torch.empty(n, device="cuda") for n in (Cr * Cc, Cr, Cc * Cr, Cc)]
        st = N.stream_ptr(torch.device("cuda"))
        p = lambda v: v.data_ptr()

        def nat_fwd():
            N.check(lib.srcgan_ca_forward(p(t), Cc, p(res), Cc, p(y), Cc, p(w1), p(b1), p(w2), p(b2), p(saved), B, hw, Cc, Cr, did, p(scr), st), "srcgan_ca_forward")

        def nat_bwd():
            N.check(lib.srcgan_ca_backward(p(dy), Cc, p(t), Cc, p(w1), p(w2), p(saved), p(dt), Cc, p(dres), Cc, 0, p(dw[0]), p(dw[1]), p(dw[2]), p(dw[3]),
                                           B, hw, Cc, Cr, did, p(scr), st), "srcgan_ca_backward")

        def nat_both():
            nat_fwd()
            nat_bwd()

        if only:                      # the traced child: the native op alone
            for _ in range(a.op_iters):
                nat_both()
            torch.cuda.synchronize()
            return

        # the composition on a channels-last [B, C, H, W] view of the same memory
        t4 = t.view(B, H, H, Cc).permute(0, 3, 1, 2).detach().requires_grad_(True)
        r4 = res.view(B, H, H, Cc).permute(0, 3, 1, 2).detach().requires_grad_(True)
        g4 = dy.view(B, H, H, Cc).permute(0, 3, 1, 2)
        tw = [v.to(td).requires_grad_(True) for v in (w1.view(Cr, Cc, 1, 1), b1, w2.view(Cc, Cr, 1, 1), b2)]

        def comp():
            s = torch.sigmoid(F.conv2d(torch.relu(F.conv2d(t4.mean(dim=(2, 3), keepdim=True), tw[0], tw[1])), tw[2], tw[3]))
            return t4 * s + r4

        def tor_fwd():
            with torch.no_grad():
                comp()

        def tor_both():
            for v in (t4, r4, *tw):
                v.grad = None
            comp().backward(g4)

        nat_fwd()
        with torch.no_grad():
            rel = float((y.view(B, H, H, Cc).permute(0, 3, 1, 2).float() - comp().float()).norm() / comp().float().norm())
        r = timed([("native_fwd", nat_fwd), ("torch_fwd", tor_fwd), ("native_bwd", nat_bwd), ("native_fwd_bwd", nat_both), ("torch_fwd_bwd", tor_both)],
                  a.samples, a.op_iters)
        n = B * hw * Cc * esz
        fb, bb = 4 * n, 5 * n
        say(json.dumps({"what": "channel attention op", "cfg": f"{B}x{H}x{H}x{Cc} Cr={Cr} {dtype}", **{k + "_us": round(v[0] * 1e3, 1) for k, v in r.items()},
                        **{k + "_spread_us": round(v[1] * 1e3, 1) for k, v in r.items()},
                        "fwd_bytes": fb, "bwd_bytes": bb, "native_fwd_TBps": round(fb / (r["native_fwd"][0] * 1e-3) / 1e12, 3),
                        "native_bwd_TBps": round(bb / (r["native_bwd"][0] * 1e-3) / 1e12, 3), "hbm_spec_TBps": HBM_SPEC / 1e12, "copy_1GiB_TBps": round(copy_bps / 1e12, 3),
                        "torch_over_native_fwd": round(r["torch_fwd"][0] / r["native_fwd"][0], 3),
                        "torch_over_native_fwd_bwd": round(r["torch_fwd_bwd"][0] / r["native_fwd_bwd"][0], 3), "output_rel_l2_native_vs_torch": float(f"{rel:.3g}")}))


def trace(a, say):
    """per-kernel times of the native op from rocprofv3's kernel statistics, one child process per dtype"""
    B, H, Cc = 16, (16 if a.quick else 96), 64
    for dtype in ("bf16", "fp32"):
        out = os.path.join(a.trace, dtype)
        os.makedirs(out, exist_ok=True)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "ca", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--traced-child", dtype, "--op-iters", str(min(a.op_iters, 200))] + (["--quick"] if a.quick else [])
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL).returncode
        if rc != 0:
            raise SystemExit(f"rocprofv3 run failed with status {rc}")
        rows = []
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += list(csv.DictReader(f))
        n = B * H * H * Cc * (2 if dtype == "bf16" else 4)
        elems = {"ca_partial_k": None, "ca_apply_fwd_k": 3, "ca_apply_bwd_k": 3, "ca_gate_fwd_k": 0, "ca_gate_bwd_k": 0}
        for r in rows:
            for key, e in elems.items():
                if key in r["Name"]:
                    if e is None:         # MODE 0 reads t, MODE 1 reads dy and t.  (The 16-bit instances come out mangled, "...Li0E...", or
                        #                   demangled without their integer argument: whatever is not marked MODE 0 is MODE 1.)
                        e = 1 if (", 0>" in r["Name"] or "Li0E" in r["Name"]) else 2
                        key = f"ca_partial_k<T, {e - 1}>"
                    avg = float(r["AverageNs"])
                    say(json.dumps({"what": "kernel", "dtype": dtype, "cfg": f"{B}x{H}x{H}x{Cc}", "name": key, "calls": int(r["Calls"]),
                                    "avg_us": round(avg / 1e3, 2), "bytes": e * n, "TBps": round(e * n / avg / 1e3, 3) if e else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--op-iters", type=int, default=1000)
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of the native op (per-kernel bytes/s)")
    ap.add_argument("--traced-child", default="", help="(child of --trace) run the native op in this dtype and exit")
    ap.add_argument("--out", default="profiles/rcan.txt")
    ap.add_argument("--quick", action="store_true", help="tiny shapes and a 2 x 2 network: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rcan.py needs a GPU")
    if a.traced_child:
        bench_op(a, print, only=a.traced_child)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"# scripts/bench_rcan.py --samples {a.samples} --iters {a.iters} --op-iters {a.op_iters}" + (" --quick" if a.quick else "") +
            f"  ({torch.cuda.get_device_name(0)}; medians of {a.samples} samples, modes alternating)")
        bench_op(a, say, copy_rate())
        if a.trace:
            trace(a, say)
        bench_network(a, say)


if __name__ == "__main__":
    main()
