#!/usr/bin/env python3
"""Golden vectors of RDN (reference src/model/rdn.py), produced by running the REFERENCE class on the CPU.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_rdn.py

Writes tests/golden/rdn_a_x2.npz ('A' x2, 2x3x7x5), rdn_b_x3.npz ('B' x3, 1x3x5x6) and rdn_a_x4_gray.npz ('A' x4, n_colors = 1, 1x1x6x4):
the construction seed, scale, RDNconfig, (D, C, G), G0 and n_colors, x, a target t, y, the L1 loss, dx, the state_dict's key names
(= parameters() order), shape and sketch (fingerprint) of every seeded weight, the parameter gradients of the float32 run, and of a
float64 run of the same instance y, loss, dx and the parameter gradients.  Only tensors are stored, no reference source text.

'B' has 22.3 M parameters in 300 tensors, so the weights are not stored, and a gradient of more than 2048 elements is stored as its
sketch plus its first 64 elements; the entries are stacked (tests/rdn_ref.py::pack_gradients holds the layout).  Every file stays
below 1 MiB.

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
from rdn_ref import CONFIGS, pack_gradients                   # noqa: E402

CASES = (("rdn_a_x2", "A", 2, 3, (2, 3, 7, 5)),
         ("rdn_b_x3", "B", 3, 3, (1, 3, 5, 6)),
         ("rdn_a_x4_gray", "A", 4, 1, (1, 1, 6, 4)))
G0 = 64


def run(cls, config, scale, n_colors, shape, seed, dtype):
    args = types.SimpleNamespace(scale=[scale], G0=G0, RDNkSize=3, RDNconfig=config, n_colors=n_colors)
    torch.manual_seed(seed)
    m = cls(args)
    weights = {k: npy(v) for k, v in m.state_dict().items()}
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
    import model.rdn as rdn

    torch.set_num_threads(4)
    for tag, config, scale, n_colors, shape in CASES:
        for seed in range(64):
            m, weights, x, t, y, loss = run(rdn.RDN, config, scale, n_colors, shape, seed, torch.float32)
            m64, _, x64, _, y64, loss64 = run(rdn.RDN, config, scale, n_colors, shape, seed, torch.float64)
            pairs = [(k, p, q) for (k, p), (_, q) in zip(m.named_parameters(), m64.named_parameters())]
            worst = max(rel_l2(npy(p.grad), npy(q.grad)) for _, p, q in pairs)
            worst = max(worst, rel_l2(npy(x.grad), npy(x64.grad)))
            print(f"{tag}: seed {seed}: worst f32-vs-f64 gradient error {worst:.3e}", "-> taken" if worst < 1e-4 else "-> skipped")
            if worst < 1e-4:
                break
        else:
            raise SystemExit(f"{tag}: no seed below 1e-4")
        names = list(weights)
        assert names == [k for k, _ in m.named_parameters()]
        out = dict(seed=np.array(seed), scale=np.array(scale), config=np.array(config), dcg=np.array(CONFIGS[config]), G0=np.array(G0),
                   n_colors=np.array(n_colors), x=npy(x), t=npy(t), y=npy(y), loss=npy(loss), dx=npy(x.grad), y64=npy(y64), loss64=npy(loss64),
                   dx64=npy(x64.grad), names=np.array(names),
                   wshape=np.array([list(weights[k].shape) + [0] * (4 - weights[k].ndim) for k in names]),
                   wsketch=np.stack([sketch(weights[k]) for k in names]))
        out.update(pack_gradients([(k, npy(p.grad)) for k, p, _ in pairs]))
        out.update(pack_gradients([(k, npy(q.grad)) for k, _, q in pairs], "64"))
        path = os.path.join(OUT, f"{tag}.npz")
        np.savez_compressed(path, **out)
        print(tag, "y", tuple(y.shape), "loss", float(loss.detach()), "keys", len(names), "bytes", os.path.getsize(path))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
