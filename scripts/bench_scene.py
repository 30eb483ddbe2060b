"""Measure whole-scene inference (srcgan_amd.infer): RDDBNet(3,3,4,nb=23), bf16, on a 2048x2048 scene -> 8192x8192.

  python scripts/bench_scene.py [--scene 2048] [--big 4096] [--nb 23] [--dtype bf16] [--reps 3] [--out profiles/scene_infer.txt]
  python scripts/bench_scene.py --ensemble 8 [--scene 2048] [--nb 23] [--dtype bf16] [--reps 3] [--ensemble-out profiles/scene_ensemble.txt]

Three runs on the same scene, each timed with device events (median of --reps) with its peak allocation above what was resident
before the call (torch.cuda.max_memory_allocated):
  whole    the whole-image no_grad forward (one tensor, one workspace)
  exact    upscale_scene(tile=1024, halo=None): halo = the receptive radius 15 nb + 3, crop; the relative difference to `whole`
  feather  upscale_scene(tile=512, halo=32, blend="feather")
then a --big x --big scene (which the whole-image path cannot hold) in feather mode, and the yardstick of the gather / scatter
kernels: the same copies done with torch slicing in this process, side by side (and the cascade's fused gather, which has no torch
twin).  A measurement tool only: no test runs it and no
gate is set on its numbers.  One JSON line per measurement, echoed to --out.

With --ensemble N only the geometric self-ensemble is measured: upscale_scene(tile=512, halo=32, blend="feather", ensemble=N) against
N x the ensemble=1 time of the same call (`ensemble_ab`: alternating rounds, device events, medians, the peak of both); its line is
APPENDED to --ensemble-out, the file scripts/bench_cascade_scene.py --ensemble appends to as well."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())


def timed(fn, reps):
    """-> (median ms, peak bytes above the resident set, last result)"""
    fn()                                              # warm-up: allocator, weight pack
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms, y = [], None
    for _ in range(reps):
        del y
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2], torch.cuda.max_memory_allocated() - base, y


def ensemble_ab(call, n, reps):
    """``call(ensemble)`` runs one scene.  Times ensemble=n and ensemble=1 in alternating rounds (device events, median of ``reps``)
    and takes each one's peak allocation above what was resident before the call -> the fields of one result line; ``ratio`` is the
    ensemble=n time over n x the ensemble=1 time: what views, folds and the accumulators cost beyond running the network n times."""
    peak, ms = {}, {1: [], n: []}
    for e in (1, n):                                  # warm up (allocator, weight pack, workspaces of every tile shape), then the peak
        call(e)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        y = call(e)
        torch.cuda.synchronize()
        peak[e] = torch.cuda.max_memory_allocated() - base
        del y
    for _ in range(reps):
        for e in (1, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(e)
            e1.record()
            torch.cuda.synchronize()
            ms[e].append(e0.elapsed_time(e1))
    med = {e: sorted(v)[len(v) // 2] for e, v in ms.items()}
    return {"ensemble": n, "ms_1": round(med[1], 2), f"ms_{n}": round(med[n], 2), "ratio_to_n_times_1": round(med[n] / (n * med[1]), 4),
            "peak_mib_1": round(peak[1] / 2 ** 20, 1), f"peak_mib_{n}": round(peak[n] / 2 ** 20, 1), "rounds": reps}


def append_lines(path, lines):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensemble", type=int, default=1, choices=[1, 2, 4, 8])
    ap.add_argument("--ensemble-out", default=os.path.join("profiles", "scene_ensemble.txt"))
    ap.add_argument("--scene", type=int, default=2048)
    ap.add_argument("--big", type=int, default=4096)
    ap.add_argument("--nb", type=int, default=23)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "scene_infer.txt"))
    a = ap.parse_args()

    from srcgan_amd import RDDBNet, infer
    torch.manual_seed(0)
    net = RDDBNet(3, 3, 4, nf=64, nb=a.nb, gc=32, dtype=a.dtype).cuda().eval()
    up = 4
    lines = []

    def emit(**kw):
        kw = {"cfg": f"RDDBNet(3,3,4,nb={a.nb}) {a.dtype}", **kw}
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    S = a.scene
    x = torch.rand(1, 3, S, S, device="cuda")
    if a.ensemble > 1:
        r = ensemble_ab(lambda e: infer.upscale_scene(net, x, up=up, tile=512, halo=32, blend="feather", ensemble=e), a.ensemble, a.reps)
        emit(run="upscale_scene feather", scene=S, tile=512, halo=32, **r)
        append_lines(a.ensemble_out, lines)
        return

    def whole():
        with torch.no_grad():
            return net(x)

    ms, peak, ref = timed(whole, a.reps)
    ref = ref.cpu()
    emit(run="whole", scene=S, ms=round(ms, 1), peak_gb=round(peak / 1e9, 3))
    halo = infer.receptive_halo(net)
    ms, peak, y = timed(lambda: infer.upscale_scene(net, x, up=up, tile=1024), a.reps)
    rel = float((y.cpu() - ref).norm() / ref.norm())
    emit(run="exact", scene=S, tile=1024, halo=halo, overhead=round(((1024 + 2 * halo) / 1024) ** 2, 2), ms=round(ms, 1),
         peak_gb=round(peak / 1e9, 3), rel_l2_vs_whole=rel)
    ms, peak, y = timed(lambda: infer.upscale_scene(net, x, up=up, tile=512, halo=32, blend="feather"), a.reps)
    rel = float((y.cpu() - ref).norm() / ref.norm())
    emit(run="feather", scene=S, tile=512, halo=32, overhead=round(((512 + 64) / 512) ** 2, 2), ms=round(ms, 1),
         peak_gb=round(peak / 1e9, 3), rel_l2_vs_whole=rel)
    del y, ref

    # the copies alone, against torch slicing (the 512 / 32 plan of the scene above; crop and feather write-back)
    plan = infer.plan_tiles(S, S, 512, 32)
    (th, tw), idx = max(plan.classes.items(), key=lambda kv: len(kv[1]))
    tiles = [plan.tiles[i] for i in idx]
    org = [(t.y0, t.x0) for t in tiles]
    ms_native, _, g = timed(lambda: infer.tile_gather(x, org, th, tw), 5)
    ms_torch, _, g2 = timed(lambda: torch.stack([x[0, :, t.y0:t.y0 + th, t.x0:t.x0 + tw] for t in tiles]), 5)
    emit(run="gather", tiles=len(idx), shape=[th, tw], native_ms=round(ms_native, 3), torch_slicing_ms=round(ms_torch, 3), equal=bool(torch.equal(g, g2)))
    del g, g2
    # the fused gather of the cascade: a u8 RGB scene -> gray, up-sampled x2 inside the gather, on the same plan
    rgb = torch.randint(0, 256, (S // 2, S // 2, 3), dtype=torch.uint8, device="cuda")
    ms_native, _, g = timed(lambda: infer.tile_gather_ex(rgb, "u8rgb2gray", 2, org, th, tw), 5)
    emit(run="gather_fused", kind="u8rgb2gray", s=2, tiles=len(idx), shape=[th, tw], native_ms=round(ms_native, 3))
    del g, rgb
    hr = torch.rand(len(idx), 3, th * up, tw * up, device="cuda")
    dst = torch.zeros(1, 3, S * up, S * up, device="cuda")

    def torch_crop():
        for n, t in enumerate(tiles):
            cy0, cy1, cx0, cx1 = t.core
            dst[0, :, cy0 * up:cy1 * up, cx0 * up:cx1 * up] = hr[n, :, (cy0 - t.y0) * up:(cy1 - t.y0) * up, (cx0 - t.x0) * up:(cx1 - t.x0) * up]

    ms_native, _, _ = timed(lambda: infer.tile_scatter(hr, dst, up, plan.rects(idx, False), False), 5)
    ms_torch, _, _ = timed(torch_crop, 5)
    emit(run="scatter_crop", tiles=len(idx), native_ms=round(ms_native, 3), torch_slicing_ms=round(ms_torch, 3))
    weights = [plan.weights(t, up).cuda() for t in tiles]

    def torch_feather():
        for n, t in enumerate(tiles):
            sy0, sy1, sx0, sx1 = t.support
            dst[0, :, sy0 * up:sy1 * up, sx0 * up:sx1 * up] += weights[n] * hr[n, :, (sy0 - t.y0) * up:(sy1 - t.y0) * up, (sx0 - t.x0) * up:(sx1 - t.x0) * up]

    ms_native, _, _ = timed(lambda: infer.tile_scatter(hr, dst, up, plan.rects(idx, True), True), 5)
    ms_torch, _, _ = timed(torch_feather, 5)
    emit(run="scatter_feather", tiles=len(idx), native_ms=round(ms_native, 3), torch_slicing_ms=round(ms_torch, 3))
    del hr, dst, weights, x

    # a scene the whole-image path cannot hold
    B = a.big
    torch.cuda.empty_cache()
    u8 = torch.randint(0, 256, (B, B, 3), dtype=torch.uint8, device="cuda")
    ms, peak, y = timed(lambda: infer.upscale_scene(net, u8, up=up, tile=512, halo=32, batch=4, blend="feather", out="u8"), 1)
    emit(run="feather_big", scene=B, tile=512, halo=32, batch=4, out=list(y.shape), ms=round(ms, 1), peak_gb=round(peak / 1e9, 3))

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
