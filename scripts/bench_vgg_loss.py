"""Time VGG16Loss / PerceptionLoss forward + backward against the same loss composed from torch.nn.functional, in one process, and
record time and peak allocation of both in profiles/vgg_loss.txt.

  python scripts/bench_vgg_loss.py [--sizes 1024 256] [--batch 16] [--dtypes bf16 fp32] [--kinds 0 1] [--samples 7] [--out profiles/vgg_loss.txt]

  native    the module's forward (one srcgan_vggloss_forward_frames) and loss.backward() (one srcgan_vggloss_backward_frames)
  composed  F.conv2d / F.relu / F.max_pool2d on NCHW tensors of the same dtype (torch.autocast for bf16), the target branch under
            no_grad, F.l1_loss / F.mse_loss on the taps, loss.backward() through autograd -- the same weights

Both are warmed up, then timed interleaved round-robin with device events around work that ends in a synchronise; the median, the
minimum and the maximum of --samples runs are written down.  The peak is torch.cuda.max_memory_allocated above the allocation at
the start of the call (inputs and weights excluded).  There is no pass mark; the numbers are written down, with both loss values."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 256])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "vgg_loss.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vgg_loss: needs a GPU (a CPU run measures nothing)")

    import vgg_ref as R                       # layouts and seeded weights only
    from srcgan_amd import VGG16Loss, PerceptionLoss
    lines = []
    for kind in a.kinds:
        sd = R.seeded_state(kind, 0)
        dev_sd = {k: v.cuda() for k, v in sd.items()}
        layout = (R.VGG16_LAYOUT, R.VGG19_LAYOUT)[kind]
        nconv = sum(1 for v in layout if v != "M")

        def taps(x):
            h, idx, seen, out = x, 0, 0, []
            for v in layout:
                if v == "M":
                    h, idx = F.max_pool2d(h, 2, 2), idx + 1
                    continue
                h = F.conv2d(h, dev_sd[f"features.{idx}.weight"], dev_sd[f"features.{idx}.bias"], padding=1)
                seen += 1
                if kind == 1 and seen == nconv:
                    out.append(h)
                    break
                h, idx = F.relu(h), idx + 2
                if kind == 0 and idx - 1 in R.VGG16_TAPS:
                    out.append(h)
            return out

        for hw in a.sizes:
            for dname in a.dtypes:
                g = torch.Generator().manual_seed(hw)
                out = torch.rand(a.batch, 3, hw, hw, generator=g).cuda()
                tgt = torch.rand(a.batch, 3, hw, hw, generator=g).cuda()
                mod = (VGG16Loss(weights=sd, dtype=dname) if kind == 0 else PerceptionLoss(weights=sd, dtype=dname)).cuda()

                def native():
                    o = out.clone().requires_grad_(True)
                    loss = mod(o, tgt)
                    loss.backward()
                    return loss.detach(), o.grad

                def composed():
                    o = out.clone().requires_grad_(True)
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dname == "bf16"):
                        ho = taps(o)
                        with torch.no_grad():
                            ht = taps(tgt)
                        loss = F.mse_loss(ho[0].float(), ht[0].float()) if kind == 1 else sum(F.l1_loss(x.float(), y.float()) for x, y in zip(ho, ht)) / 4
                    loss.backward()
                    return loss.detach(), o.grad

                modes = [("native", native), ("composed", composed)]
                peak, ms, value = {}, {m: [] for m, _ in modes}, {}
                for m, fn in modes:                         # warm up, then one run for the peak and the value
                    fn()
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    y = fn()
                    torch.cuda.synchronize()
                    peak[m] = torch.cuda.max_memory_allocated() - base
                    value[m] = float(y[0])
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
                    lines.append(json.dumps({"loss": "VGG16Loss" if kind == 0 else "PerceptionLoss", "input": f"{a.batch}x3x{hw}x{hw}", "dtype": dname, "mode": m,
                                             "fwd_bwd_median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3), "samples": len(v),
                                             "peak_mib": round(peak[m] / 2 ** 20, 1), "loss_value": float(f"{value[m]:.7g}")}))
                    print(lines[-1], flush=True)
                del out, tgt, mod
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# scripts/bench_vgg_loss.py: forward + backward of the native perceptual losses against the torch.nn.functional composition, same\n"
                "# process, interleaved; peak = max_memory_allocated above the start of the call (inputs and weights excluded)\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
