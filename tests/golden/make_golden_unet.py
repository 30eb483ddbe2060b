#!/usr/bin/env python3
"""Golden vectors of UnetGenerator (reference src/model/basicModel.py:257-354), produced by running the REFERENCE's
``init_net(UnetGenerator(in, out, num_downs, ngf, norm_layer=get_norm_layer('instance')), 'normal', 0.02)`` -- what its ``define_G`` does
for 'unet_128' / 'unet_256' with num_downs 7 / 8 -- on the CPU.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_unet.py

Writes tests/golden/unet_d5_1to3.npz (5 levels, ngf 16, x (2, 1, 32, 32) -> 3 channels: the bottleneck is 1 x 1) and
tests/golden/unet_d6_3to1.npz (6 levels, ngf 16, x (1, 3, 64, 64) -> 1 channel: the loop over ``num_downs - 5`` runs once).  Each file holds
the construction seed and cfg = [input_nc, output_nc, ngf, num_downs], x, a target t, y, the L1 loss, dx, shape and sketch (fingerprint) of
every seeded weight in state_dict order (``names``), every parameter gradient of the float32 run, and of a float64 run of the same instance
y, loss, dx and the parameter gradients.  Only tensors and name lists are stored, no reference source text.

Dead biases, the storage of large gradients and the seed choice: as in make_golden_resnetgen.py.  A bias is dead when an InstanceNorm2d
follows its convolution directly: every down convolution's but the first and the last (the innermost block has no down norm), every
transposed convolution's but the outermost."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _stub_modules, npy          # noqa: E402
from make_golden_srdense import rel_l2, sketch                # noqa: E402

BIG = 2048
NGF = 16
CASES = (("unet_d5_1to3", 1, 3, 5, (2, 1, 32, 32)), ("unet_d6_3to1", 3, 1, 6, (1, 3, 64, 64)))


def run(make, shape, seed, dtype):
    torch.manual_seed(seed)
    m = make()
    weights = {k: npy(v) for k, v in m.state_dict().items()}
    m = m.to(dtype)
    torch.manual_seed(1000 + seed)
    x = torch.rand(*shape).to(dtype).requires_grad_(True)
    y = m(x)
    t = (torch.rand(*y.shape) * 2 - 1).to(dtype)           # the range of tanh
    loss = nn.L1Loss()(y, t)
    loss.backward()
    return m, weights, x, t, y, loss


def dead_names(m):
    """biases of convolutions that an InstanceNorm2d follows directly inside their nn.Sequential"""
    dead = []
    for name, seq in m.named_modules():
        if isinstance(seq, nn.Sequential):
            mods = list(seq.named_children())
            for (ka, a), (_, b) in zip(mods, mods[1:]):
                if isinstance(a, (nn.Conv2d, nn.ConvTranspose2d)) and isinstance(b, nn.InstanceNorm2d):
                    dead.append(f"{name}.{ka}.bias")
    return dead


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import model.basicModel as bm

    torch.set_num_threads(4)
    for tag, cin, cout, nd, shape in CASES:
        make = lambda: bm.init_net(bm.UnetGenerator(cin, cout, nd, NGF, norm_layer=bm.get_norm_layer("instance")), "normal", 0.02)
        for seed in range(64):
            m, weights, x, t, y, loss = run(make, shape, seed, torch.float32)
            m64, _, x64, _, y64, loss64 = run(make, shape, seed, torch.float64)
            names = list(weights)
            dset = set(dead_names(m))
            dead = [k for k in names if k in dset]
            g = {k: npy(p.grad) for k, p in m.named_parameters()}
            g64 = {k: npy(p.grad) for k, p in m64.named_parameters()}
            live = [rel_l2(g[k], g64[k]) for k in names if k not in dead] + [rel_l2(npy(x.grad), npy(x64.grad))]
            ratio = {k: float(np.abs(g[k]).max() / np.abs(g[k[:-4] + "weight"]).max()) for k in dead}
            ok = max(live) < 1e-4
            print(f"{tag}: seed {seed}: worst live f32-vs-f64 gradient error {max(live):.3e}, worst dead-bias ratio {max(ratio.values()):.3e}, "
                  f"worst dead-bias |g| in float64 {max(float(np.abs(g64[k]).max()) for k in dead):.1e}", "-> taken" if ok else "-> skipped")
            if ok:
                break
        else:
            raise SystemExit(f"{tag}: no seed below 1e-4")
        out = dict(seed=np.array(seed), cfg=np.array([cin, cout, NGF, nd]), x=npy(x), t=npy(t), y=npy(y), loss=npy(loss), dx=npy(x.grad),
                   y64=npy(y64), loss64=npy(loss64), dx64=npy(x64.grad), names=np.array(names), dead=np.array(dead))
        for k, w in weights.items():
            out["wshape/" + k] = np.array(w.shape)
            out["wsketch/" + k] = sketch(w)
        for k in names:
            if g[k].size > BIG:
                out["gsketch/" + k], out["gslice/" + k] = sketch(g[k]), g[k][0].copy()
                out["gsketch64/" + k], out["gslice64/" + k] = sketch(g64[k]), g64[k][0].copy()
            else:
                out["grad/" + k], out["grad64/" + k] = g[k], g64[k]
        for k in dead:
            out["dead_ratio/" + k] = np.array(ratio[k])
        path = os.path.join(OUT, f"{tag}.npz")
        np.savez(path, **out)
        print(tag, "y", tuple(y.shape), "loss", float(loss.detach()), "params", len(names), "dead", len(dead), "bytes", os.path.getsize(path))
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
