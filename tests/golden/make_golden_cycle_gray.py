#!/usr/bin/env python3
"""Golden vectors of ONE cycle step in the gray configuration ``opt.net == 'SRdens'`` (reference src/train.py:166-170, 228-340),
produced by the REFERENCE's own ``train.SRCycleGAN.optimize_parameters`` on the CPU.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_cycle_gray.py

``src/train.py`` imports ``RDDBNetA`` from the ``model`` package, which has no source for it, and a few modules the step never
touches.  The script therefore puts ``SRDenseNetA``, ``SRDenseNetB``, ``NLayerDiscriminator`` and ``RDDBNetB`` of ``model.model`` into
the package namespace, adds a placeholder ``RDDBNetA`` (never constructed in this branch) and stubs ``utils`` / ``dataset`` /
``visdom`` like ``make_golden._stub_modules``.  Every class the 'SRdens' branch runs is the reference's.

Writes tests/golden/cycle_srdens.npz.  Only tensors and names are stored, no reference source text.

Weights are NOT stored (the two 64-wide discriminators alone are ~5 MB).  They are filled by a recipe that the tests replay into
the native modules: ``torch.manual_seed(s)``; nets in the order G_A, G_B, D_A, D_B; within a net in ``state_dict()`` order; every
tensor ``0.05 * randn(shape)``, a BatchNorm ``weight`` ``1 + 0.05 * randn(shape)``; ``running_mean`` / ``running_var`` /
``num_batches_tracked`` are left as constructed.  The file stores ``s``, the key lists and a fingerprint (sum, sum of squares, first 4
values, as make_golden_resdeconv.py) of every tensor, so a drift of either side's key order fails loudly.

Stored: realA [2,1,24,20], realB [2,3,48,40]; real_B_Gray, real_A_RGB, fake_B, fake_A, recl_A, recl_B, iden_A, iden_B; the ten
scalar losses; after the step, per parameter the gradient's fingerprint (f32 run ``gfp/``, f64 run ``gfp64/``) and the full gradient
of a few small tensors per network (``grad/``) -- the generators' ``.grad`` is loss_G's gradient, the discriminators' is loss_D_*'s;
the post-step fingerprint of every state_dict entry (``wfp1/``) and the discriminators' BatchNorm running statistics in full
(``bn1/``): each discriminator runs three times per step (once frozen inside backward_G, twice in backward_D_*).

Seed choice is a condition, not a measurement: the same step is evaluated in float64 on a deep copy, and a seed is refused when any
parameter gradient of the f32 run differs from the f64 run by more than 1e-4 (max |g32 - g64| / max |g64|) -- a ReLU / LeakyReLU
pre-activation within rounding of zero makes two correct evaluations disagree (tests/test_gpu_modules.py::test_resdeconv_golden_f32).
The observed value of the chosen seed is printed and stored as ``ref_f32_vs_f64``.
"""
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _stub_modules, npy          # noqa: E402
from make_golden_resdeconv import fingerprint                 # noqa: E402

NETS = ("G_A", "G_B", "D_A", "D_B")
LOSSES = ("loss_D_A", "loss_G_A", "loss_cycle_A", "loss_iden_A", "loss_D_B", "loss_G_B", "loss_cycle_B", "loss_iden_B", "loss_G")
IMAGES = ("real_B_Gray", "real_A_RGB", "fake_B", "fake_A", "recl_A", "recl_B", "iden_A", "iden_B")
# full gradients: first and last convolution of every network, one dense-block convolution per generator, one BN pair per discriminator
FULL = {"G_A": ("conv_first.weight", "conv_first.bias", "conv_last.weight", "conv_last.bias", "dense_blocks.1.block.1.conv.weight", "reconstruction.weight"),
        "G_B": ("conv_first.weight", "conv_first.bias", "conv_last.weight", "conv_last.bias", "dense_blocks.1.block.1.conv.weight", "reconstruction.weight"),
        "D_A": ("model.0.weight", "model.0.bias", "model.3.weight", "model.3.bias", "model.8.weight", "model.8.bias"),
        "D_B": ("model.0.weight", "model.0.bias", "model.3.weight", "model.3.bias", "model.8.weight", "model.8.bias")}
SHAPE_A, SHAPE_B = (2, 1, 24, 20), (2, 3, 48, 40)        # LR 24 x 20 -> HR 48 x 40: non-square, not a multiple of 16


def fill_by_recipe(nets, seed):
    """The weight recipe of the module docstring, on CPU tensors (the generator is the CPU's, whatever device the nets are on)."""
    torch.manual_seed(seed)
    for net in nets:
        for key, t in net.state_dict().items():
            leaf = key.rsplit(".", 1)[-1]
            if leaf in ("running_mean", "running_var", "num_batches_tracked"):
                continue
            owner = net.get_submodule(key.rsplit(".", 1)[0]) if "." in key else net
            v = 0.05 * torch.randn(tuple(t.shape))
            if isinstance(owner, nn.BatchNorm2d) and leaf == "weight":
                v = 1.0 + v
            with torch.no_grad():
                t.copy_(v)


def nets_of(m):
    return (m.netG_A, m.netG_B, m.netD_A, m.netD_B)


def import_reference_train():
    _stub_modules()
    for name, attrs in (("utils", {"Logger": object}), ("dataset", {"load_dataset": None})):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    sys.path.insert(0, REF)
    import model
    import model.model as legacy
    for name in ("SRDenseNetA", "SRDenseNetB", "NLayerDiscriminator", "RDDBNetB"):
        setattr(model, name, getattr(legacy, name))

    class RDDBNetA(nn.Module):                    # placeholder: the reference ships no source for it; 'SRdens' never builds it
        def __init__(self, *a, **k):
            raise NotImplementedError("RDDBNetA has no reference source")
    model.RDDBNetA = RDDBNetA
    import train
    return train


class Opt:
    device = torch.device("cpu"); lr = 1e-4; beta1 = 0.5; batch_size = 1; num_works = 0; num_epochs = 25; pool_size = 4
    lambda_identity = 1.0; lambda_A = 10; lambda_B = 10; n_epochs_decay = 100; matrix = 0; lr_policy = "cosine"
    mode = "x2"; net = "SRdens"; scaling_factor = 2


def one_step(train, seed, double):
    torch.manual_seed(seed)                       # (the constructors draw their own initial weights; the recipe overwrites them)
    m = train.SRCycleGAN(Opt)
    for net in nets_of(m):
        net.train()
    fill_by_recipe(nets_of(m), seed)
    torch.manual_seed(1000 + seed)
    realA, realB = torch.rand(*SHAPE_A), torch.rand(*SHAPE_B)
    before = {n: {k: fingerprint(v) for k, v in net.state_dict().items()} for n, net in zip(NETS, nets_of(m))}
    if double:
        m = copy.deepcopy(m)                      # the optimisers of the copy hold the copy's parameters
        for net in nets_of(m):
            net.double()
        m.criterionGAN.double()
        realA, realB = realA.double(), realB.double()
    m.optimize_parameters(realA, realB)
    return m, realA, realB, before


def worst_grad_gap(m32, m64):
    worst, where = 0.0, None
    for n, a, b in zip(NETS, nets_of(m32), nets_of(m64)):
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            g32, g64 = p.grad.double(), q.grad
            gap = float((g32 - g64).abs().max() / g64.abs().max().clamp_min(1e-300))
            if gap > worst:
                worst, where = gap, f"{n}/{k}"
    return worst, where


def main():
    sys.dont_write_bytecode = True
    train = import_reference_train()
    torch.set_num_threads(4)
    for seed in range(64):
        m, realA, realB, before = one_step(train, seed, False)
        m64, _, _, _ = one_step(train, seed, True)
        worst, where = worst_grad_gap(m, m64)
        print(f"cycle_srdens: seed {seed}: worst f32-vs-f64 parameter gradient gap {worst:.3e} at {where}", "-> taken" if worst <= 1e-4 else "-> refused")
        if worst <= 1e-4:
            break
    else:
        raise SystemExit("cycle_srdens: no seed within 1e-4")

    out = dict(s=np.array(seed), ref_f32_vs_f64=np.array(worst), realA=npy(realA), realB=npy(realB))
    for k in IMAGES:
        out[k] = npy(getattr(m, k))
    for k in LOSSES:
        out[k] = np.array(float(getattr(m, k).detach()))
        out[k + "_64"] = np.array(float(getattr(m64, k).detach()))
    out["loss_D"] = np.array(float(m.loss_D_A.detach()) + float(m.loss_D_B.detach()))          # the 'loss_D' of the log line, train.py:396
    out["loss_D_64"] = np.array(float(m64.loss_D_A.detach()) + float(m64.loss_D_B.detach()))
    for n, net, net64 in zip(NETS, nets_of(m), nets_of(m64)):
        out[f"keys/{n}"] = np.array(list(net.state_dict()))
        out[f"pnames/{n}"] = np.array([k for k, _ in net.named_parameters()])
        for k, fp in before[n].items():
            out[f"wfp/{n}/{k}"] = fp
        for k, v in net.state_dict().items():
            out[f"wfp1/{n}/{k}"] = fingerprint(v)
            if n.startswith("D_") and k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked"):
                out[f"bn1/{n}/{k}"] = npy(v)
        for (k, p), (_, q) in zip(net.named_parameters(), net64.named_parameters()):
            out[f"gfp/{n}/{k}"] = fingerprint(p.grad)
            out[f"gfp64/{n}/{k}"] = fingerprint(q.grad)
            if k in FULL[n]:
                out[f"grad/{n}/{k}"] = npy(p.grad)
        missing = [k for k in FULL[n] if f"grad/{n}/{k}" not in out]
        assert not missing, (n, missing)
    path = os.path.join(OUT, "cycle_srdens.npz")
    np.savez(path, **out)
    print("cycle_srdens: seed", seed, "ref_f32_vs_f64", worst, {k: float(out[k]) for k in LOSSES}, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
