#!/usr/bin/env python3
"""Golden vectors of DDBPN (reference src/model/ddbpn.py with src/model/common.py), produced by running the REFERENCE class on the CPU.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_ddbpn.py

Writes tests/golden/ddbpn_x{2,4,8}.npz: the construction seed and scale, x, a target t, y, the L1 loss, dx, the state_dict's key names,
the frozen names, a shape and a sketch (fingerprint) of every seeded weight, the parameter gradients of the float32 run, and of a
float64 run of the same instance y, loss, dx and the parameter gradients.  rgb_range = 1.  Only tensors are stored, no reference
source text.

The network has 1.3 M, 2.2 M and 4.9 M parameters at the three scales, so neither the weights nor the large gradients are stored
whole: a gradient of more than BIG elements is stored as its sketch plus its first slice (``first_slice``), in float32 (``gsketch/``,
``gslice/``) and float64 (``gsketch64/``, ``gslice64/``); smaller ones whole (``grad/``, ``grad64/``).  Every file stays below 1 MiB.

Before the run the PReLU slopes are moved away from their initial 0.25 by tests/ddbpn_ref.py::set_slopes (seeded values in
[-0.3, 1.3], some exactly 0), so the fixture exercises them; the tests apply the same rule to the native instance.

sketch(t): see make_golden_srdense.py.  Seed choice: as there -- the first construction seed at which the reference's own f32
gradients are within 1e-4 (relative L2) of its float64 ones; the seeds tried are printed.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, REF, _stub_modules, npy          # noqa: E402
from make_golden_srdense import rel_l2, sketch                # noqa: E402
from ddbpn_ref import set_slopes                              # noqa: E402

BIG = 2048
CASES = (("ddbpn_x2", 2, (2, 3, 7, 5)),
         ("ddbpn_x4", 4, (1, 3, 5, 6)),
         ("ddbpn_x8", 8, (1, 3, 3, 4)))


def first_slice(g):
    """g[0], or g[0, 0] where g[0] itself has more than 256 elements (a projection weight: one k x k kernel)"""
    return (g[0] if g[0].size <= 256 else g[0, 0]).copy()


def run(cls, scale, shape, seed, dtype):
    args = types.SimpleNamespace(scale=[scale], rgb_range=1, n_colors=3)
    torch.manual_seed(seed)
    m = cls(args)
    weights = {k: npy(v) for k, v in m.state_dict().items()}          # as seeded, before the slopes are moved
    set_slopes(m, seed)
    m = m.to(dtype)
    torch.manual_seed(1000 + seed)
    x = torch.rand(*shape).to(dtype).requires_grad_(True)
    y = m(x)
    t = torch.rand(*y.shape).to(dtype)
    loss = nn.L1Loss()(y, t)
    loss.backward()
    return m, weights, x, t, y, loss


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import model.ddbpn as ddbpn

    torch.set_num_threads(4)
    for tag, scale, shape in CASES:
        for seed in range(64):
            m, weights, x, t, y, loss = run(ddbpn.DDBPN, scale, shape, seed, torch.float32)
            m64, _, x64, _, y64, loss64 = run(ddbpn.DDBPN, scale, shape, seed, torch.float64)
            pairs = [(k, p, q) for (k, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()) if p.requires_grad]
            worst = max(rel_l2(npy(p.grad), npy(q.grad)) for _, p, q in pairs)
            worst = max(worst, rel_l2(npy(x.grad), npy(x64.grad)))
            print(f"{tag}: seed {seed}: worst f32-vs-f64 gradient error {worst:.3e}", "-> taken" if worst < 1e-4 else "-> skipped")
            if worst < 1e-4:
                break
        else:
            raise SystemExit(f"{tag}: no seed below 1e-4")
        out = dict(seed=np.array(seed), scale=np.array(scale), x=npy(x), t=npy(t), y=npy(y), loss=npy(loss), dx=npy(x.grad),
                   y64=npy(y64), loss64=npy(loss64), dx64=npy(x64.grad), names=np.array(list(weights)),
                   params=np.array([k for k, _ in m.named_parameters()]),
                   frozen=np.array([k for k, p in m.named_parameters() if not p.requires_grad]))
        for k, w in weights.items():
            out["wshape/" + k] = np.array(w.shape)
            out["wsketch/" + k] = sketch(w)
        for k, p, q in pairs:
            g, g64 = npy(p.grad), npy(q.grad)
            if g.size > BIG:
                out["gsketch/" + k] = sketch(g)
                out["gslice/" + k] = first_slice(g)
                out["gsketch64/" + k] = sketch(g64)
                out["gslice64/" + k] = first_slice(g64)
            else:
                out["grad/" + k] = g
                out["grad64/" + k] = g64
        path = os.path.join(OUT, f"{tag}.npz")
        np.savez_compressed(path, **out)
        print(tag, "y", tuple(y.shape), "loss", float(loss), "keys", len(weights), "parameters", len(list(m.parameters())), "bytes", os.path.getsize(path))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
