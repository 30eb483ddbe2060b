#!/usr/bin/env python3
"""Golden vectors of SRDenseNetA / SRDenseNetB (reference src/model/model.py:643-786), produced by running the REFERENCE classes
on the CPU.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_srdense.py

Writes tests/golden/srdense_{a_x2,a_x4,b_x2,b_x4}.npz: the construction seed and cfg, x, a target t, y, the L1 loss, dx, a sketch
(fingerprint) of every seeded weight, every parameter gradient, and the gradients of a float64 run of the same instance.  All four
use growth_rate 16, num_blocks 2, num_layers 2.  Only tensors are stored, no reference source text.

The 256 x 256 x 3 x 3 gradient of ``deconv.0.weight`` alone is 2.4 MB, beyond the size limit of a committed file, so that one tensor is
stored as its sketch plus its first output-channel slice (``gslice/`` and ``gsketch/``; float64 run: ``gslice64/``).

sketch(t): a 64-bucket count sketch of the flattened tensor in float64 -- element i goes to bucket i mod 64 with the sign of a fixed
integer hash of i.  E ||sketch(a) - sketch(b)||^2 = ||a - b||^2, so the relative error of two sketches estimates the relative L2
error of the tensors; of two equal tensors the sketches are equal bit for bit.

Seed choice: a ReLU pre-activation within rounding of zero makes two correct evaluations of the backward disagree (see
tests/test_gpu_modules.py::test_resdeconv_golden_f32), so the generator takes the first construction seed at which the reference's
own f32 parameter gradients are within 1e-4 (relative L2) of its float64 ones, and prints the seeds it tried.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _stub_modules, npy          # noqa: E402

BIG = "deconv.0.weight"
G, NB, L = 16, 2, 2
CASES = (("srdense_a_x2", "SRDenseNetA", 1, 3, "x2", (2, 1, 5, 7)),
         ("srdense_a_x4", "SRDenseNetA", 1, 3, "x4", (2, 1, 5, 7)),
         ("srdense_b_x2", "SRDenseNetB", 3, 1, "x2", (2, 3, 13, 18)),      # odd height: the parity input gradient meets a ragged edge
         ("srdense_b_x4", "SRDenseNetB", 3, 1, "x4", (1, 3, 10, 14)))      # 5 x 7 after the first stage: odd at the second


def sketch(t):
    v = np.asarray(t, dtype=np.float64).reshape(-1)
    i = np.arange(v.size, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    sign = 1.0 - 2.0 * ((h >> np.uint64(15)) & np.uint64(1)).astype(np.float64)
    out = np.zeros(64, dtype=np.float64)
    np.add.at(out, (i % np.uint64(64)).astype(np.int64), sign * v)
    return out


def first_slice(g, transposed):
    """First output-channel slice of a weight gradient: ConvTranspose2d weights are [in, out, kh, kw], Conv2d ones [out, in, kh, kw]."""
    return g[:, 0] if transposed else g[0]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def run(cls, ic, oc, mode, shape, seed, dtype):
    torch.manual_seed(seed)
    m = cls(ic, oc, num_blocks=NB, num_layers=L, growth_rate=G, mode=mode)
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
    import model.model as legacy

    torch.set_num_threads(4)
    for tag, cname, ic, oc, mode, shape in CASES:
        cls = getattr(legacy, cname)
        tr = cname == "SRDenseNetA"
        for seed in range(64):
            m, weights, x, t, y, loss = run(cls, ic, oc, mode, shape, seed, torch.float32)
            m64, _, x64, _, y64, loss64 = run(cls, ic, oc, mode, shape, seed, torch.float64)
            worst = max(rel_l2(npy(p.grad), npy(q.grad)) for (_, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()))
            worst = max(worst, rel_l2(npy(x.grad), npy(x64.grad)))
            print(f"{tag}: seed {seed}: worst f32-vs-f64 gradient error {worst:.3e}", "-> taken" if worst < 1e-4 else "-> skipped")
            if worst < 1e-4:
                break
        else:
            raise SystemExit(f"{tag}: no seed below 1e-4")
        out = dict(seed=np.array(seed), cfg=np.array([ic, oc, G, NB, L, int(mode[1])]), x=npy(x), t=npy(t), y=npy(y), loss=npy(loss), dx=npy(x.grad),
                   y64=npy(y64), loss64=npy(loss64), dx64=npy(x64.grad), names=np.array(list(weights)))
        for k, w in weights.items():
            out["wshape/" + k] = np.array(w.shape)
            out["wsketch/" + k] = sketch(w)
        for (k, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()):
            g, g64 = npy(p.grad), npy(q.grad)
            if k == BIG:
                out["gsketch/" + k] = sketch(g)
                out["gslice/" + k] = first_slice(g, tr).copy()
                out["gslice64/" + k] = first_slice(g64, tr).copy()
            else:
                out["grad/" + k] = g
                out["grad64/" + k] = g64
        path = os.path.join(OUT, f"{tag}.npz")
        np.savez(path, **out)
        print(tag, "y", tuple(y.shape), "loss", float(loss), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
