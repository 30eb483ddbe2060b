"""Time SRDenseNetA(1, 3, num_blocks=2, num_layers=2) 'x2' at 16 x 1 x 256 x 256 in bf16: the forward under torch.no_grad() and
forward + backward, and the up-sampler kernel (ConvTranspose2d 256 -> 256, k3 s2 p1 output_padding 1, four parities in one launch)
beside the existing 3x3 stride-1 convolution 256 -> 256 on the same output size, in the same process.

  python scripts/bench_srdense.py [--samples 5] [--iters 10] [--batch 16] [--hw 256] [--dtype bf16] [--rocprof DIR]

HIP events around --iters calls after a warm-up; the modes of a group are interleaved round-robin and the median of the samples is
reported, one JSON line per mode.  The 3x3 convolution does 9 / 2.25 = 4 x the MACs per output pixel of the transposed one; the line
"kernel_ratio" gives the ratio of achieved TFLOP/s (reported, not asserted).

--rocprof DIR starts `rocprofv3 --kernel-trace --stats` (no counters) on a child process that runs the forward only, under
`timeout`, and prints the new kernel's time, TFLOP/s and share of the forward from the kernel statistics."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.getcwd())


def timed(modes, samples, iters):
    ms = {name: [] for name, _ in modes}
    for _, fn in modes:
        for _ in range(3):
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
    return {k: (sorted(v)[len(v) // 2], max(v) - min(v), v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--rocprof", default="")
    ap.add_argument("--forward-only", action="store_true", help="(child of --rocprof) run --iters forwards and exit")
    a = ap.parse_args()

    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "srdense", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--forward-only", "--iters", str(a.iters), "--batch", str(a.batch), "--hw", str(a.hw),
               "--dtype", a.dtype]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit(f"rocprofv3 run failed with status {rc}")
        rows = []
        for path in glob.glob(os.path.join(a.rocprof, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += list(csv.DictReader(f))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        flop = 2.0 * a.batch * a.hw * a.hw * 9 * 256 * 256
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]:
            print(f"{float(r['TotalDurationNs']) / total * 100:6.2f} %  {int(r['Calls']):5d} calls  {float(r['AverageNs']) / 1e3:10.1f} us  {r['Name'][:110]}")
        for r in rows:
            if "deconv_k3s2" in r["Name"]:
                avg = float(r["AverageNs"])
                print(json.dumps({"kernel": "deconv_k3s2", "calls": int(r["Calls"]), "avg_us": round(avg / 1e3, 1), "tflops": round(flop / avg / 1e3, 1),
                                  "share_of_forward_kernels": round(float(r["TotalDurationNs"]) / total, 4)}))
        return

    import srcgan_amd as S
    from srcgan_amd import ops
    torch.manual_seed(0)
    net = S.SRDenseNetA(1, 3, num_blocks=2, num_layers=2, mode="x2", dtype=a.dtype).cuda()
    x = torch.rand(a.batch, 1, a.hw, a.hw, device="cuda")

    def fwd():
        with torch.no_grad():
            return net(x)

    if a.forward_only:
        for _ in range(a.iters + 2):
            fwd()
        torch.cuda.synchronize()
        return

    xg = x.clone().requires_grad_(True)

    def fwd_bwd():
        net(xg).sum().backward()

    cfg = f"SRDenseNetA(1,3,nB=2,L=2,x2) {a.dtype} B={a.batch} {a.hw}x{a.hw}"
    for name, (med, spread, v) in timed([("forward", fwd), ("forward_backward", fwd_bwd)], a.samples, a.iters).items():
        print(json.dumps({"cfg": cfg, "mode": name, "iters": a.iters, "ms": [round(t, 3) for t in v], "median_ms": round(med, 3), "spread_ms": round(spread, 3)}), flush=True)
    del xg
    for p in net.parameters():
        p.grad = None
    torch.cuda.empty_cache()

    # the kernel beside the 3x3 stride-1 convolution 256 -> 256 on the same output size
    B, H = a.batch, a.hw
    xi = ops.to_nhwc(torch.randn(B, 256, H, H, device="cuda"), dtype=a.dtype)
    wt = torch.randn(256, 256, 3, 3, device="cuda") * 0.02
    bias = torch.zeros(256, device="cuda")
    big = torch.empty(B, 2 * H, 2 * H, 256, dtype=xi.dtype, device="cuda").normal_()
    out = torch.empty_like(big)
    wp = ops.pack_conv2d_fwd(wt, a.dtype)
    packed = ops.pack_deconv3x3s2(wt, a.dtype)
    modes = [("deconv_k3s2", lambda: ops.deconv3x3s2(xi, wt, bias, relu=True, packed=packed, y=out)),
             ("conv3x3_s1", lambda: ops.conv_igemm(big, wp, out, kh=3, kw=3, Cout=256, pad=(1, 1), bias=bias, act=True, slope=0.0))]
    res = timed(modes, a.samples, a.iters)
    flop = {"deconv_k3s2": 2.0 * B * H * H * 9 * 256 * 256, "conv3x3_s1": 2.0 * B * 4 * H * H * 9 * 256 * 256}
    tf = {}
    for name, (med, spread, v) in res.items():
        tf[name] = flop[name] / (med * 1e-3) / 1e12
        print(json.dumps({"kernel": name, "out": f"{B}x{2 * H}x{2 * H}x256 {a.dtype}", "median_ms": round(med, 3), "spread_ms": round(spread, 3),
                          "tflops": round(tf[name], 1)}), flush=True)
    print(json.dumps({"kernel_ratio": "deconv_k3s2 TFLOP/s over conv3x3_s1 TFLOP/s", "value": round(tf["deconv_k3s2"] / tf["conv3x3_s1"], 3)}))


if __name__ == "__main__":
    main()
