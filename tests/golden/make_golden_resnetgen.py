#!/usr/bin/env python3
"""Golden vectors of ResnetGenerator (reference src/model/basicModel.py:105-254), produced by running the REFERENCE's
``define_G(in, out, ngf, 'resnet_{6,9}blocks', 'instance', False, 'normal', 0.02)`` on the CPU.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_resnetgen.py

Writes tests/golden/resnetgen_1to3.npz (6 blocks, ngf 16, x (2, 1, 8, 12) -> 3 channels) and tests/golden/resnetgen_3to1.npz (9 blocks,
ngf 16, x (2, 3, 16, 12) -> 1 channel).  Each file holds the construction seed and cfg = [input_nc, output_nc, ngf, n_blocks], x, a
target t, y, the L1 loss, dx, shape and sketch (fingerprint) of every seeded weight in state_dict order (``names``), every parameter
gradient of the float32 run, and of a float64 run of the same instance y, loss, dx and the parameter gradients.  Only tensors and name
lists are stored, no reference source text.

Dead biases.  Every bias but the last layer's sits in front of an InstanceNorm2d, which subtracts the mean it adds: its gradient is zero
in exact arithmetic, and what a run leaves there is rounding noise (about 1e-8 in float32, 1e-17 in float64).  ``dead`` lists them, and
``dead_ratio/<name>`` is the reference's own float32 figure  max|g_bias| / max|g_weight of the same layer|,  the absolute measure the
tests hold them to.  They take no part in the seed choice.

A gradient of more than BIG elements is stored as its sketch plus its first slice (``gsketch/``, ``gslice/`` for the float32 run,
``gsketch64/``, ``gslice64/`` for the float64 one), which keeps every file below 1 MiB; the others are stored whole (``grad/``,
``grad64/``).

sketch(t): see make_golden_srdense.py.  Seed choice: as there -- the first construction seed at which the reference's own f32 LIVE
gradients (weights, the last bias, dx) are within 1e-4 (relative L2) of its float64 ones; the seeds tried are printed.
"""
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
CASES = (("resnetgen_1to3", 1, 3, 6, (2, 1, 8, 12)), ("resnetgen_3to1", 3, 1, 9, (2, 3, 16, 12)))


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


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import model.basicModel as bm

    torch.set_num_threads(4)
    for tag, cin, cout, nblk, shape in CASES:
        make = lambda: bm.define_G(cin, cout, NGF, f"resnet_{nblk}blocks", "instance", False, "normal", 0.02)
        for seed in range(64):
            m, weights, x, t, y, loss = run(make, shape, seed, torch.float32)
            m64, _, x64, _, y64, loss64 = run(make, shape, seed, torch.float64)
            names = list(weights)
            last_bias = names[-1]
            dead = [k for k in names if k.endswith(".bias") and k != last_bias]
            g = {k: npy(p.grad) for k, p in m.named_parameters()}
            g64 = {k: npy(p.grad) for k, p in m64.named_parameters()}
            live = [rel_l2(g[k], g64[k]) for k in names if k not in dead] + [rel_l2(npy(x.grad), npy(x64.grad))]
            ratio = {k: float(np.abs(g[k]).max() / np.abs(g[k[:-4] + "weight"]).max()) for k in dead}
            ok = max(live) < 1e-4
            print(f"{tag}: seed {seed}: worst live f32-vs-f64 gradient error {max(live):.3e}, worst dead-bias ratio {max(ratio.values()):.3e}",
                  "-> taken" if ok else "-> skipped")
            if ok:
                break
        else:
            raise SystemExit(f"{tag}: no seed below 1e-4")
        out = dict(seed=np.array(seed), cfg=np.array([cin, cout, NGF, nblk]), x=npy(x), t=npy(t), y=npy(y), loss=npy(loss), dx=npy(x.grad),
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
