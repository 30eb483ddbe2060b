#!/usr/bin/env python3
"""Generate tests/golden/class_losses.npz by running the REFERENCE ``losses.FLoss``, ``losses.CELoss``, ``losses.ConLoss`` and
``losses.CrossLoss`` on CPU in float32, the output (feats) requiring grad.

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_class_losses.py          (build container only)

Per case ``<case>/x`` (and ``<case>/t``), ``<case>/loss`` and ``<case>/dx`` (the reference's ``output.grad``).  Inputs of the ordinary
cases are drawn by tests/class_losses_ref.py as float16-representable values in [0.02, 0.98] and stored as float16 (exact; the losses
run in float32); every CELoss target position and every ConLoss column has a unique maximum (and minimum), which is asserted here.

Three special cases are float32 only -- a float64 evaluation is wrong for them, because 1e-6 as float32 lies below the float64 bound:
``edges_focal`` / ``edges_ce``: [0, 1e-7, f32(1e-6), 0.5, f32(1 - 1e-6), 1] with target 1 (the clamp bounds from both sides; the -100
clamp of BCELoss); ``ties``: ConLoss columns with a repeated maximum and a repeated minimum.  Tensors only, no reference source text.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, OUT, _stub_modules, npy          # noqa: E402
import class_losses_ref as R                                   # noqa: E402


def unique_extremes(a, axis):
    s = np.sort(a, axis=axis)
    hi, lo = np.take(s, [-1, -2], axis=axis), np.take(s, [0, 1], axis=axis)
    return bool(np.all(np.take(hi, 0, axis=axis) > np.take(hi, 1, axis=axis)) and np.all(np.take(lo, 0, axis=axis) < np.take(lo, 1, axis=axis)))


def main():
    sys.dont_write_bytecode = True
    _stub_modules()
    sys.path.insert(0, REF)
    import losses as ref_losses                    # src/losses.py: CELoss :150-167, ConLoss :258-274, CrossLoss :277-293, FLoss :296-341

    torch.set_num_threads(4)
    bx, bt = R.flat_inputs((2, 1, 9, 11), seed=1)
    mx, mt = R.flat_inputs((2, 4, 9, 11), seed=1)
    feats = R.range_inputs((5, 3 * 7 * 9), seed=1).reshape(5, 3, 7, 9)
    cx, ct = R.cross_inputs((3, 2, 5, 7), seed=1)
    ones = np.ones_like(R.EDGES_X)
    cases = [
        ("focal_binary", ref_losses.FLoss(), bx, bt),
        ("focal_multi", ref_losses.FLoss(), mx, mt),
        ("focal_g15_sum", ref_losses.FLoss(gamma=1.5, size_average=False), bx, bt),
        ("focal_g3", ref_losses.FLoss(gamma=3.), mx, mt),
        ("ce_binary", ref_losses.CELoss(), bx, bt),
        ("ce_multi", ref_losses.CELoss(), mx, mt),
        ("con", ref_losses.ConLoss(), feats, None),
        ("cross", ref_losses.CrossLoss(), cx, ct),
        ("edges_focal", ref_losses.FLoss(), R.EDGES_X, ones),
        ("edges_ce", ref_losses.CELoss(), R.EDGES_X, ones),
        ("ties", ref_losses.ConLoss(), R.ties_inputs(), None),
    ]
    assert [repr(c[1]) for c in cases[:8:2]] == ["Focal", "Focal", "CE", "ConLoss"] and repr(cases[7][1]) == "CrossLoss"
    assert unique_extremes(mt, 1) and unique_extremes(feats, 0)
    out = {}
    for name, crit, x, t in cases:
        special = name.startswith("edges") or name == "ties"
        store = np.float32 if special else np.float16
        for a in (x, t):
            if a is not None and not special:
                assert np.array_equal(a.astype(np.float16).astype(np.float32), a), name
        if not special and name != "cross":
            assert x.min() >= 0.01 and x.max() <= 0.99 or name == "con", name
        xr = torch.from_numpy(np.asarray(x, np.float32)).clone().requires_grad_(True)
        args = (xr,) if t is None else (xr, torch.from_numpy(np.asarray(t, np.float32)))
        loss = crit(*args)
        loss.backward()
        out[f"{name}/x"] = np.asarray(x, store)
        if t is not None:
            out[f"{name}/t"] = np.asarray(t, store)
        out[f"{name}/loss"], out[f"{name}/dx"] = npy(loss).astype(np.float32), npy(xr.grad)
        print(f"{name:14s} loss {float(loss):.6f}" + (f"  dx {npy(xr.grad).ravel()}" if special else ""))
    np.savez(os.path.join(OUT, "class_losses.npz"), **out)


if __name__ == "__main__":
    main()
