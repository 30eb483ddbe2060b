"""Time ``cascade_scene`` on one 1024x1024 LR scene at up = 4 against the composition a user had to write before it existed, in one
process, and record time and peak allocation of both in profiles/cascade_scene.txt.

  python scripts/bench_cascade_scene.py [--hw 1024] [--up 4] [--tile 512] [--batch 1] [--samples 3] [--out profiles/cascade_scene.txt]
  python scripts/bench_cascade_scene.py --ensemble 8 [...] [--ensemble-out profiles/scene_ensemble.txt]

Two configurations, each timed both ways (interleaved round-robin, device events, the median of --samples runs):

  feather/lab  SRDN(1,1,4) -> ResDeconv(1,2), const, LAB, halo 32, feathered blend, 8-bit output
  crop/lab     SRCNN(1,1,4) -> SRCNN(1,2,4), const, LAB, exact halo, crop, 8-bit output

  fused     one cascade_scene(...) call on the u8 colour scene
  composed  data.arr2gray(scene) -> ops.bilinear_up(gray, up) -> upscale_scene(sr, up-sampled) = L -> upscale_scene(col, L) = ab
            -> torch.cat -> data.lab2img: five scene-sized f32 tensors on the way

The peak is torch.cuda.max_memory_allocated above the allocation at the start of the call (the input scene excluded, the result
included).  There is no pass mark; the numbers are written down.

With --ensemble N the fused call of each configuration is timed with ensemble=N against N x its ensemble=1 time instead
(bench_scene.py's ``ensemble_ab``: alternating rounds, medians, the peak of both) and the lines are APPENDED to --ensemble-out."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--up", type=int, default=4)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "cascade_scene.txt"))
    ap.add_argument("--ensemble", type=int, default=1, choices=[1, 2, 4, 8])
    ap.add_argument("--ensemble-out", default=os.path.join("profiles", "scene_ensemble.txt"))
    a = ap.parse_args()

    from srcgan_amd import SRCNN, SRDN, ResDeconv, cascade_scene, data, ops, upscale_scene
    torch.manual_seed(0)
    scene = torch.randint(0, 256, (a.hw, a.hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    up = a.up

    def composed(sr, col, **kw):
        gray = data.arr2gray(scene)[None]
        big = ops.bilinear_up(gray, up)
        del gray
        l = upscale_scene(sr, big, up=1, **kw)
        del big
        ab = upscale_scene(col, l, up=1, **kw)
        return data.lab2img(torch.cat([l, ab], 1)[0])

    configs = []
    sr, col = SRDN(1, 1, up).cuda().eval(), ResDeconv(1, 2).cuda().eval()
    kw = dict(tile=a.tile, halo=32, multiple=16, batch=a.batch, blend="feather")
    configs.append(("feather/lab SRDN(1,1,%d) -> ResDeconv(1,2)" % up,
                    lambda sr=sr, col=col, kw=kw, e=1: cascade_scene(sr, col, scene, up=up, const=True, space="lab", out="u8", ensemble=e, **kw),
                    lambda sr=sr, col=col, kw=kw: composed(sr, col, **kw)))
    sr, col = SRCNN(1, 1, up).cuda().eval(), SRCNN(1, 2, up).cuda().eval()
    kw = dict(tile=a.tile, batch=a.batch, blend="crop")
    # the composition runs the networks in two passes, each with its own exact halo (6); the fused chain needs their sum (12)
    configs.append(("crop/lab SRCNN(1,1,%d) -> SRCNN(1,2,%d)" % (up, up),
                    lambda sr=sr, col=col, kw=kw, e=1: cascade_scene(sr, col, scene, up=up, const=True, space="lab", out="u8", halo=None, ensemble=e,
                                                                     **kw),
                    lambda sr=sr, col=col, kw=kw: composed(sr, col, halo=None, **kw)))

    if a.ensemble > 1:
        from bench_scene import append_lines, ensemble_ab
        lines = []
        for name, fused, _ in configs:
            r = ensemble_ab(lambda e: fused(e=e), a.ensemble, a.samples)
            lines.append(json.dumps({"cfg": name, "run": "cascade_scene", "scene": f"{a.hw}x{a.hw} u8 RGB, up {up}, tile {a.tile}, batch {a.batch}", **r}))
            print(lines[-1], flush=True)
        append_lines(a.ensemble_out, lines)
        return

    lines = []
    for name, fused, comp in configs:
        modes = [("fused", fused), ("composed", comp)]
        peak, ms = {}, {m: [] for m, _ in modes}
        for m, fn in modes:                             # warm up, then one run for the peak
            fn()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            y = fn()
            torch.cuda.synchronize()
            peak[m] = torch.cuda.max_memory_allocated() - base
            assert y.dtype == torch.uint8 and tuple(y.shape) == (a.hw * up, a.hw * up, 3)
            del y
        for _ in range(a.samples):
            for m, fn in modes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms[m].append(e0.elapsed_time(e1))
        for m, _ in modes:
            v = sorted(ms[m])
            lines.append(json.dumps({"config": name, "mode": m, "scene": f"{a.hw}x{a.hw} u8 RGB, up {up}, tile {a.tile}, batch {a.batch}",
                                     "ms": [round(t, 2) for t in ms[m]], "median_ms": round(v[len(v) // 2], 2),
                                     "peak_mib": round(peak[m] / 2 ** 20, 1)}))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# scripts/bench_cascade_scene.py: cascade_scene (fused) against arr2gray + bilinear_up + two upscale_scene passes + cat + lab2img\n"
                "# (composed), same process; peak = max_memory_allocated above the start of the call (the input scene excluded)\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
