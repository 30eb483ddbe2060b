"""Dump the raw results of the DSSIM and perceptual losses, the SSIM metric and score_scene at the shapes the tests use, so that two
builds of the library can be compared byte for byte.

  python scripts/dump_loss_bits.py dump FILE.npz          run from the root of the tree under test, on the GPU
  python scripts/dump_loss_bits.py compare A.npz B.npz    exit status 1 on any difference

  DSSIMLoss                  the six cases of tests/golden/dssim.npz: loss, dx, dt with the target requiring grad, dx with it not
  metrics.SSIM(full=True)    the same cases
  VGG16Loss, PerceptionLoss  (2,3,20,28), (1,1,32,32), (1,3,16,16) x fp32, bf16, fp16: loss and dx with grad, loss under no_grad
  score_scene(full=True)     one f32 3-channel scene of 43x50 and one u8 scene of the same size
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))

DSSIM_CASES = ["rgb01", "gray255", "tanh", "single", "strip_row", "strip_col"]
VGG_SHAPES = [(2, 3, 20, 28), (1, 1, 32, 32), (1, 3, 16, 16)]


def dump(path):
    import vgg_ref as R                       # seeded weights and inputs only
    from srcgan_amd import DSSIMLoss, VGG16Loss, PerceptionLoss
    from srcgan_amd.metrics import SSIM, score_scene
    out = {}

    def put(key, t):
        out[key] = t.detach().float().cpu().numpy() if t.dtype != torch.float64 else t.detach().cpu().numpy()

    g = np.load(os.path.join("tests", "golden", "dssim.npz"), allow_pickle=False)
    for case in DSSIM_CASES:
        x0, t0 = torch.from_numpy(g[f"{case}/x"]).float().cuda(), torch.from_numpy(g[f"{case}/t"]).float().cuda()
        for tgrad in (True, False):
            x, t = x0.clone().requires_grad_(True), t0.clone().requires_grad_(tgrad)
            loss = DSSIMLoss()(x, t)
            loss.backward()
            if tgrad:
                put(f"dssim/{case}/loss", loss)
                put(f"dssim/{case}/dx", x.grad)
                put(f"dssim/{case}/dt", t.grad)
            else:
                put(f"dssim/{case}/dx_only", x.grad)
        ssim, cs = SSIM()(x0, t0, full=True)
        put(f"ssim/{case}/ssim", ssim)
        put(f"ssim/{case}/cs", cs)

    for kind, cls in ((0, VGG16Loss), (1, PerceptionLoss)):
        for shape in VGG_SHAPES:
            sd, o0, t0 = R.make_case(kind, shape, 0)
            o0, t0 = o0.cuda(), t0.cuda()
            for dname in ("fp32", "bf16", "fp16"):
                crit = cls(weights=sd, dtype=dname).cuda()
                key = f"{cls.__name__}/{'x'.join(map(str, shape))}/{dname}"
                o = o0.clone().requires_grad_(True)
                loss = crit(o, t0)
                loss.backward()
                put(f"{key}/loss", loss)
                put(f"{key}/dx", o.grad)
                with torch.no_grad():
                    put(f"{key}/loss_no_grad", crit(o0, t0))

    gen = torch.Generator().manual_seed(0)
    tgt = torch.rand(1, 3, 43, 50, generator=gen)
    pred = (tgt + 0.05 * torch.randn(1, 3, 43, 50, generator=gen)).clamp_(0, 1)
    to_u8 = lambda v: (v[0].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous()
    for name, p, t in (("f32", pred.cuda(), tgt.cuda()), ("u8", to_u8(pred).cuda(), to_u8(tgt).cuda())):
        for k, v in score_scene(p, t, full=True).items():
            put(f"score_scene/{name}/{k}", v)

    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.savez(path, **out)
    print(f"dump_loss_bits: wrote {len(out)} arrays to {path}")


def compare(pa, pb):
    a, b = np.load(pa, allow_pickle=False), np.load(pb, allow_pickle=False)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad.append(k)
    print(f"dump_loss_bits: {len(a.files)} arrays in {pa}, {len(b.files)} in {pb}, {len(bad)} mismatches")
    for k in bad:
        print(f"  MISMATCH {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
