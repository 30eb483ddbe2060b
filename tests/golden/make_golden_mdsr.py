#!/usr/bin/env python3
"""Golden vectors of MDSR and VDSR (reference src/model/mdsr.py, src/model/vdsr.py with src/model/common.py), produced by running the
REFERENCE classes on the CPU.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_mdsr.py

Writes tests/golden/mdsr_s234_idx{0,1,2}.npz -- ONE instance (one construction seed) of scale = [2, 3, 4], n_resblocks = 2, n_feats = 32,
rgb_range = 1, run at each scale_idx on a shape of its own -- and tests/golden/vdsr.npz (n_resblocks = 4, n_feats = 32, rgb_range = 1,
shape (2, 3, 11, 37)).  Each file holds the construction seed and cfg, x, a target t, y, the L1 loss, dx, shape and sketch (fingerprint)
of every seeded weight in state_dict order (``names``), the frozen parameters (``frozen``), the trainable parameters whose ``.grad`` is
None after the backward (``nograd``: MDSR's branches off the graph), every parameter gradient of the float32 run, and of a float64 run of
the same instance y, loss, dx and the parameter gradients.  Only tensors and name lists are stored, no reference source text.

The reference constructors look ``url['r{}f{}'.format(n_resblocks, n_feats)]`` up and so refuse every size but the published ones with
KeyError.  This script therefore adds the key of the small size to the IMPORTED module's ``url`` dict at run time (``url['r2f32'] = ''``
for MDSR, ``url['r4f32'] = ''`` for VDSR); nothing else of the reference is touched.

A gradient of more than BIG elements is stored as its sketch plus its first output-channel slice (``gsketch/``, ``gslice/`` for the
float32 run, ``gsketch64/``, ``gslice64/`` for the float64 one), which keeps every file below 1 MiB; the others are stored whole
(``grad/``, ``grad64/``).

sketch(t): see make_golden_srdense.py.  Seed choice: as there -- the first construction seed at which the reference's own f32
gradients are within 1e-4 (relative L2) of its float64 ones, here in all three branches at once; the seeds tried are printed.
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
NB, F, SCALES = 2, 32, [2, 3, 4]
MDSR_SHAPES = ((2, 3, 9, 7), (1, 3, 6, 5), (2, 3, 5, 6))
VDSR_NB, VDSR_SHAPE = 4, (2, 3, 11, 37)


def run(make, idx, shape, seed, dtype):
    torch.manual_seed(seed)
    m = make()
    weights = {k: npy(v) for k, v in m.state_dict().items()}
    m = m.to(dtype)
    if idx is not None:
        m.set_scale(idx)
    torch.manual_seed(1000 + seed + (idx or 0))
    x = torch.rand(*shape).to(dtype).requires_grad_(True)
    y = m(x)
    t = torch.rand(*y.shape).to(dtype)
    loss = nn.L1Loss()(y, t)
    loss.backward()
    return m, weights, x, t, y, loss


def worst_error(m, m64, x, x64):
    pairs = [(k, p, q) for (k, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()) if p.grad is not None]
    assert all(q.grad is not None for _, _, q in pairs)
    return max([rel_l2(npy(p.grad), npy(q.grad)) for _, p, q in pairs] + [rel_l2(npy(x.grad), npy(x64.grad))]), pairs


def save(tag, seed, cfg, extra, m, weights, x, t, y, loss, x64, y64, loss64, pairs):
    out = dict(seed=np.array(seed), cfg=np.array(cfg), x=npy(x), t=npy(t), y=npy(y), loss=npy(loss), dx=npy(x.grad),
               y64=npy(y64), loss64=npy(loss64), dx64=npy(x64.grad), names=np.array(list(weights)),
               frozen=np.array([k for k, p in m.named_parameters() if not p.requires_grad]),
               nograd=np.array([k for k, p in m.named_parameters() if p.requires_grad and p.grad is None], dtype="U64"), **extra)
    for k, w in weights.items():
        out["wshape/" + k] = np.array(w.shape)
        out["wsketch/" + k] = sketch(w)
    for k, p, q in pairs:
        g, g64 = npy(p.grad), npy(q.grad)
        if g.size > BIG:
            out["gsketch/" + k], out["gslice/" + k] = sketch(g), g[0].copy()
            out["gsketch64/" + k], out["gslice64/" + k] = sketch(g64), g64[0].copy()
        else:
            out["grad/" + k], out["grad64/" + k] = g, g64
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez(path, **out)
    print(tag, "y", tuple(y.shape), "loss", float(loss.detach()), "grads", len(pairs), "without", len(out["nograd"]), "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import model.mdsr as mdsr
    import model.vdsr as vdsr
    mdsr.url[f"r{NB}f{F}"] = ""               # the small sizes of the fixtures (see the docstring)
    vdsr.url[f"r{VDSR_NB}f{F}"] = ""

    torch.set_num_threads(4)
    make = lambda: mdsr.MDSR(types.SimpleNamespace(n_resblocks=NB, n_feats=F, scale=SCALES, rgb_range=1, n_colors=3))
    for seed in range(64):
        runs = []
        for idx, shape in enumerate(MDSR_SHAPES):
            a = run(make, idx, shape, seed, torch.float32)
            b = run(make, idx, shape, seed, torch.float64)
            worst, pairs = worst_error(a[0], b[0], a[2], b[2])
            runs.append((a, b, worst, pairs))
        ws = [r[2] for r in runs]
        print(f"mdsr: seed {seed}: worst f32-vs-f64 gradient errors {['%.3e' % w for w in ws]}", "-> taken" if max(ws) < 1e-4 else "-> skipped")
        if max(ws) < 1e-4:
            break
    else:
        raise SystemExit("mdsr: no seed below 1e-4")
    for idx, ((m, weights, x, t, y, loss), (_, _, x64, _, y64, loss64), _, pairs) in enumerate(runs):
        save(f"mdsr_s234_idx{idx}", seed, [NB, F, 1, idx], dict(scales=np.array(SCALES)), m, weights, x, t, y, loss, x64, y64, loss64, pairs)

    make = lambda: vdsr.VDSR(types.SimpleNamespace(n_resblocks=VDSR_NB, n_feats=F, rgb_range=1, n_colors=3))
    for seed in range(64):
        a = run(make, None, VDSR_SHAPE, seed, torch.float32)
        b = run(make, None, VDSR_SHAPE, seed, torch.float64)
        worst, pairs = worst_error(a[0], b[0], a[2], b[2])
        print(f"vdsr: seed {seed}: worst f32-vs-f64 gradient error {worst:.3e}", "-> taken" if worst < 1e-4 else "-> skipped")
        if worst < 1e-4:
            break
    else:
        raise SystemExit("vdsr: no seed below 1e-4")
    (m, weights, x, t, y, loss), (_, _, x64, _, y64, loss64) = a, b
    save("vdsr", seed, [VDSR_NB, F, 1], {}, m, weights, x, t, y, loss, x64, y64, loss64, pairs)


if __name__ == "__main__":
    main()
