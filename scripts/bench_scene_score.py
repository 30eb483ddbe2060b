"""Time ``score_scene`` on whole u8 RGB scenes against the composition it replaces, in one process, and record time, peak allocation
and effective bandwidth of both in profiles/scene_score.txt.

  python scripts/bench_scene_score.py [--sizes 2048 8192] [--samples 7] [--out profiles/scene_score.txt]

  fused     score_scene(pred_u8, target_u8, full=True): one tile kernel over both u8 scenes + a two-stage fold
  composed  data.arr2rgb of both scenes (two f32 [1,3,H,W] tensors) -> metrics.MSE, PSNR, AE, SSIM: four more passes over them

Both are warmed up, then timed interleaved round-robin with device events around work that ends in a synchronise; the median, the
minimum and the maximum of --samples runs are written down.  The peak is torch.cuda.max_memory_allocated above the allocation at
the start of the call (the two u8 scenes excluded).  Effective GB/s = the 2 * H * W * C bytes of the two u8 scenes over the median
time, beside the 6.3 TB/s an MI355X streams from HBM; for the composition it is the same useful bytes, not its own traffic.  There
is no pass mark; the numbers are written down, and the values of both paths are printed so that they can be compared."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())

HBM_GBS = 6300.0          # achievable HBM streaming rate of an MI355X (8 TB/s peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "scene_score.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scene_score: needs a GPU (a CPU run measures nothing)")

    from srcgan_amd import data, metrics as M, score_scene
    lines = []
    for hw in a.sizes:
        g = torch.Generator().manual_seed(hw)
        target = torch.randint(0, 256, (hw, hw, 3), dtype=torch.uint8, generator=g).cuda()
        pred = (target.to(torch.int16) + torch.randint(-12, 13, (hw, hw, 3), dtype=torch.int16, generator=g).cuda()).clamp_(0, 255).to(torch.uint8)

        def fused():
            d = score_scene(pred, target, full=True)
            return [d[k] for k in ("MSE", "PSNR", "AE", "SSIM", "CS")]

        def composed():
            p, t = data.arr2rgb(pred)[None], data.arr2rgb(target)[None]
            s, cs = M.SSIM()(p, t, full=True)
            return [M.MSE()(p, t), M.PSNR()(p, t), M.AE()(p, t)[0], s, cs]

        modes = [("fused", fused), ("composed", composed)]
        peak, ms, value = {}, {m: [] for m, _ in modes}, {}
        for m, fn in modes:                             # warm up, then one run for the peak and the values
            fn()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            y = fn()
            torch.cuda.synchronize()
            peak[m] = torch.cuda.max_memory_allocated() - base
            value[m] = [float(v) for v in y]
            del y
        for _ in range(a.samples):
            for m, fn in modes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms[m].append(e0.elapsed_time(e1))
        nbytes = 2 * hw * hw * 3
        for m, _ in modes:
            v = sorted(ms[m])
            med = v[len(v) // 2]
            lines.append(json.dumps({"scene": f"{hw}x{hw}x3 u8 pair", "mode": m, "median_ms": round(med, 3), "min_ms": round(v[0], 3),
                                     "max_ms": round(v[-1], 3), "samples": len(v), "peak_mib": round(peak[m] / 2 ** 20, 2),
                                     "effective_gbs": round(nbytes / (med * 1e-3) / 1e9, 1), "hbm_gbs": HBM_GBS,
                                     "mse_psnr_ae_ssim_cs": [float(f"{x:.7g}") for x in value[m]]}))
            print(lines[-1], flush=True)
        del pred, target
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# scripts/bench_scene_score.py: score_scene (fused) against arr2rgb x 2 + metrics.MSE / PSNR / AE / SSIM (composed), same process,\n"
                "# interleaved; peak = max_memory_allocated above the start of the call (the two u8 scenes excluded); effective_gbs = the u8 bytes\n"
                "# of both scenes over the median time\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
