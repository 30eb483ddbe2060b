#!/usr/bin/env python3
"""Golden vectors of RCAN (reference src/model/rcan.py with src/model/common.py), produced by running the REFERENCE class on the CPU.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_rcan.py

Writes tests/golden/rcan_x{2,3,4}.npz: the construction seed and cfg, x, a target t, y, the L1 loss, dx, a sketch (fingerprint) of every
seeded weight, every parameter gradient of the float32 run, and of a float64 run of the same instance y, loss, dx and the parameter
gradients.  All three use n_resgroups = n_resblocks = 2, n_feats = 32, reduction = 8, rgb_range = 1.  Only tensors are stored, no
reference source text.

The float64 gradients of the large tensors (more than BIG elements) are stored as their sketch plus their first output-channel slice
(``gsketch64/`` and ``gslice64/``), which keeps every file below 1 MiB; the float32 ones are stored whole.

sketch(t): see make_golden_srdense.py.  Seed choice: as there -- the first construction seed at which the reference's own f32
gradients are within 1e-4 (relative L2) of its float64 ones; the seeds tried are printed, with the range of the attention gates.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _stub_modules, npy          # noqa: E402
from make_golden_srdense import rel_l2, sketch                # noqa: E402

BIG = 2048
NG, NB, F, RED = 2, 2, 32, 8
CASES = (("rcan_x2", 2, (2, 3, 9, 7)),
         ("rcan_x3", 3, (1, 3, 6, 5)),
         ("rcan_x4", 4, (2, 3, 5, 6)))


def run(cls, scale, shape, seed, dtype):
    args = types.SimpleNamespace(n_resgroups=NG, n_resblocks=NB, n_feats=F, reduction=RED, scale=[scale], rgb_range=1, n_colors=3, res_scale=1)
    torch.manual_seed(seed)
    m = cls(args)
    weights = {k: npy(v) for k, v in m.state_dict().items()}
    m = m.to(dtype)
    gates = []
    for mod in m.modules():
        if type(mod).__name__ == "CALayer":
            mod.conv_du.register_forward_hook(lambda _m, _i, o: gates.append(npy(o)))
    torch.manual_seed(1000 + seed)
    x = torch.rand(*shape).to(dtype).requires_grad_(True)
    y = m(x)
    t = torch.rand(*y.shape).to(dtype)
    loss = nn.L1Loss()(y, t)
    loss.backward()
    return m, weights, x, t, y, loss, gates


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import model.rcan as rcan

    torch.set_num_threads(4)
    for tag, scale, shape in CASES:
        for seed in range(64):
            m, weights, x, t, y, loss, gates = run(rcan.RCAN, scale, shape, seed, torch.float32)
            m64, _, x64, _, y64, loss64, _ = run(rcan.RCAN, scale, shape, seed, torch.float64)
            pairs = [(k, p, q) for (k, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()) if p.requires_grad]
            worst = max(rel_l2(npy(p.grad), npy(q.grad)) for _, p, q in pairs)
            worst = max(worst, rel_l2(npy(x.grad), npy(x64.grad)))
            lo, hi = min(g.min() for g in gates), max(g.max() for g in gates)
            print(f"{tag}: seed {seed}: worst f32-vs-f64 gradient error {worst:.3e}, gates in [{lo:.3f}, {hi:.3f}]", "-> taken" if worst < 1e-4 else "-> skipped")
            if worst < 1e-4:
                break
        else:
            raise SystemExit(f"{tag}: no seed below 1e-4")
        out = dict(seed=np.array(seed), cfg=np.array([NG, NB, F, RED, scale]), x=npy(x), t=npy(t), y=npy(y), loss=npy(loss), dx=npy(x.grad),
                   y64=npy(y64), loss64=npy(loss64), dx64=npy(x64.grad), names=np.array(list(weights)),
                   frozen=np.array([k for k, p in m.named_parameters() if not p.requires_grad]))
        for k, w in weights.items():
            out["wshape/" + k] = np.array(w.shape)
            out["wsketch/" + k] = sketch(w)
        for k, p, q in pairs:
            g, g64 = npy(p.grad), npy(q.grad)
            out["grad/" + k] = g
            if g.size > BIG:
                out["gsketch64/" + k] = sketch(g64)
                out["gslice64/" + k] = g64[0].copy()
            else:
                out["grad64/" + k] = g64
        path = os.path.join(OUT, f"{tag}.npz")
        np.savez(path, **out)
        print(tag, "y", tuple(y.shape), "loss", float(loss), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
