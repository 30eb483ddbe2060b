"""Time the generator's forward under torch.no_grad(): RDDBNet(3,3,4,nb=23), bf16, B=16, 256x256 -> 1024x1024, seeded input.

Runs on any tree of this project: where the native library has srcgan_rddbnet_infer, no_grad takes the rolling inference
workspace (on a tree whose model has an INFER_FUSED_TAIL switch -- the experiment of DESIGN section 8 row 5c -- both tail forms
are timed, interleaved round-robin); on an older tree it takes the only path there is (the training forward and its whole-network workspace).  To compare
two trees, run the script from each tree's root back to back in one GPU job.

  python scripts/bench_infer.py [--samples 5] [--iters 20] [--batch 16] [--hw 256] [--nb 23] [--dtype bf16] [--grad]

--grad adds the tree's own grad-mode forward (interleaved round-robin with the no_grad mode) for orientation; the yardstick of
the inference path is the parent tree's no_grad time, not this.  Prints one JSON line per mode: per-forward milliseconds of
every sample (device events around --iters forwards), median, spread (max - min) and the peak allocation of one forward."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--nb", type=int, default=23)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    import srcgan_amd
    from srcgan_amd import RDDBNet, _native as N
    has_infer = "srcgan_rddbnet_infer" in N.SIGNATURES
    torch.manual_seed(0)
    net = RDDBNet(3, 3, 4, nf=64, nb=a.nb, gc=32, dtype=a.dtype).cuda()
    x = torch.rand(a.batch, 3, a.hw, a.hw, device="cuda")

    def no_grad():
        with torch.no_grad():
            return net(x)

    def grad():
        return net(x)

    import srcgan_amd.model as M
    if hasattr(M, "INFER_FUSED_TAIL"):           # (b) unfused and (c) fused tail, interleaved in this process
        def switched(flag):
            def run():
                M.INFER_FUSED_TAIL = flag
                return no_grad()
            return run
        modes = [("no_grad_unfused", switched(False)), ("no_grad_fused", switched(True))]
    else:
        modes = [("no_grad", no_grad)]
    if a.grad:
        modes.append(("grad", grad))
    peak, ms = {}, {name: [] for name, _ in modes}
    for name, fn in modes:                       # warm every mode up before any is timed
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        y = fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        del y
    for _ in range(a.samples):                   # round-robin over the modes
        for name, fn in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)
    for name, _ in modes:
        v = sorted(ms[name])
        print(json.dumps({"tree": a.label or os.path.basename(os.getcwd()), "mode": name,
                          "path": "infer" if (has_infer and name != "grad") else "training-forward",
                          "cfg": f"RDDBNet(3,3,4,nb={a.nb}) {a.dtype} B={a.batch} {a.hw}x{a.hw}", "iters": a.iters,
                          "ms": [round(t, 3) for t in ms[name]], "median_ms": round(v[len(v) // 2], 3),
                          "spread_ms": round(v[-1] - v[0], 3), "peak_gb": round(peak[name] / 1e9, 3)}), flush=True)


if __name__ == "__main__":
    main()
