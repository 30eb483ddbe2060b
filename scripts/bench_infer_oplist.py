"""Time one ResDeconv(1, 3) pass three ways, interleaved round-robin in one process: the grad-mode forward (training workspace),
srcgan_resdeconv_infer with fold_tail = 0 (slot-planned workspace, the training forward's launches) and with fold_tail = 1
(deconv13 -> pred folded into four parity 2x2 convolutions, what the module runs under torch.no_grad()).

  python scripts/bench_infer_oplist.py [--samples 5] [--iters 10] [--dtype bf16] [--shapes 16x256,1x2048] [--out profiles/infer_oplist.txt]

Prints one JSON line per shape and mode: per-pass milliseconds of every sample (device events around --iters passes), median,
spread (max - min), peak allocation of one pass and the planner's workspace figure; --out also writes the lines to a file."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--shapes", default="16x256,1x2048", help="comma-separated BxHW (square inputs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from srcgan_amd import ResDeconv, _native as N
    import srcgan_amd.model as M
    lib = N.lib()
    torch.manual_seed(0)
    net = ResDeconv(1, 3, dtype=a.dtype).cuda()
    params = list(net.parameters())
    args = (net.tar_ch, N.dtype_id(net.compute_dtype), net.layers_cfg, 0)
    lines = []
    for shape in a.shapes.split(","):
        B, hw = (int(v) for v in shape.split("x"))
        x = torch.rand(B, 1, hw, hw, device="cuda")
        x3 = torch.cat([x, x, x], dim=1)
        cfg = N.ResDeconvCfg(3, 3, B, hw, hw, args[1], (C.c_int * 4)(*net.layers_cfg), 0)
        plan = {"grad": lib.srcgan_resdeconv_ws_bytes(C.byref(cfg)),
                "fold_tail=0": lib.srcgan_resdeconv_infer_ws_bytes(C.byref(cfg), 0),
                "fold_tail=1": lib.srcgan_resdeconv_infer_ws_bytes(C.byref(cfg), 1)}

        def infer(fold):
            def run():
                with torch.no_grad():
                    return M._oplist_forward(x3, M._RESDECONV, args, params, extra=(fold,))
            return run

        modes = [("grad", lambda: net(x)), ("fold_tail=0", infer(0)), ("fold_tail=1", infer(1))]
        peak, ms = {}, {name: [] for name, _ in modes}
        for name, fn in modes:                       # warm every mode up before any is timed
            for _ in range(2):
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
            lines.append(json.dumps({"cfg": f"ResDeconv(1,3) {a.dtype} B={B} {hw}x{hw}", "mode": name, "iters": a.iters,
                                     "ms": [round(t, 3) for t in ms[name]], "median_ms": round(v[len(v) // 2], 3),
                                     "spread_ms": round(v[-1] - v[0], 3), "peak_mb": round(peak[name] / 1e6, 1),
                                     "planner_ws_mb": round(plan[name] / 1e6, 1)}))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
