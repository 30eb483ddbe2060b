"""Float64 restatement of RDN for the tests (our own words; the formulas are those of Residual Dense Network for Image
Super-Resolution, arXiv:1802.08797): a function of a state_dict, so it runs with any weights, on the CPU, and autograd gives its gradients.

    f1 = SFENet1(x);  x_0 = SFENet2(f1)
    block d:  t_0 = x_d;  t_{c+1} = cat[t_c, ReLU(conv3x3_c(t_c))], c < C;  x_{d+1} = LFF(t_C) + x_d          (LFF: 1x1)
    y = UPNet(GFF.1(GFF.0(cat[x_1 .. x_D])) + f1)        GFF.0: 1x1, GFF.1: 3x3;  UPNet: (3x3, PixelShuffle) once (x2, x3) or twice (x4), 3x3

``cfg`` = (D, C, G); G0 and the colours are read off the weights.  The restatement concatenates, as the paper does; the native plan does
not (csrc/oplist.hip, rdn_plan), and GFF.0 runs there as D 1x1 convolutions over column slices of its weight, summed one after the other.

``store``: None, or a 16-bit torch dtype -- the storage emulation: the input, every tensor an op of the native executor writes and
every convolution weight is rounded to that type (forward only: the backward is the exact one of the rounded forward); biases stay as
they are.  That includes every partial sum of GFF.0: the running sum is rounded D times where a concatenating implementation rounds once.
``gff_once=True`` rounds GFF.0's output once instead, to measure what the D roundings cost.

``mut`` names one deliberate mistake (tests/test_rdn_teeth.py): MUTATIONS."""
import numpy as np
import torch
import torch.nn.functional as F

import net_ref
from net_ref import BIG, first_slice, rel_l2, sketch, worst          # noqa: F401  (the tests and the fixture generator take them from here)

CONFIGS = {"A": (20, 6, 32), "B": (16, 8, 64)}
MUTATIONS = ("drop_block", "short_read", "slot_off", "lff_no_residual", "gff_swap", "no_global_residual", "shuffle_order", "skip_stage2")
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def config(cfg):
    return CONFIGS[cfg] if isinstance(cfg, str) else tuple(int(v) for v in cfg)


def names(cfg, scale):
    """state_dict keys = parameters() order of the reference class"""
    D, C, _ = config(cfg)
    mods = ["SFENet1", "SFENet2"]
    for d in range(D):
        mods += [f"RDBs.{d}.convs.{c}.conv.0" for c in range(C)] + [f"RDBs.{d}.LFF"]
    mods += ["GFF.0", "GFF.1", "UPNet.0", "UPNet.2"] + (["UPNet.4"] if scale == 4 else [])
    return [f"{m}.{p}" for m in mods for p in ("weight", "bias")]


def shapes(cfg, scale, G0=64, n_colors=3):
    D, C, G = config(cfg)
    r2 = 4 if scale == 4 else scale * scale
    w = {"SFENet1": (G0, n_colors, 3, 3), "SFENet2": (G0, G0, 3, 3), "GFF.0": (G0, D * G0, 1, 1), "GFF.1": (G0, G0, 3, 3), "UPNet.0": (G * r2, G0, 3, 3)}
    for d in range(D):
        for c in range(C):
            w[f"RDBs.{d}.convs.{c}.conv.0"] = (G, G0 + c * G, 3, 3)
        w[f"RDBs.{d}.LFF"] = (G0, G0 + C * G, 1, 1)
    if scale == 4:
        w["UPNet.2"], w["UPNet.4"] = (G * 4, G, 3, 3), (n_colors, G, 3, 3)
    else:
        w["UPNet.2"] = (n_colors, G, 3, 3)
    return w


def random_state_dict(cfg, scale, G0=64, n_colors=3, seed=0, gain=1.0):
    """float64 weights of a fan-in scaled normal distribution (the tests of the restatement alone need no seeded torch modules)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for m, s in shapes(cfg, scale, G0, n_colors).items():
        fan = s[1] * s[2] * s[3]
        sd[m + ".weight"] = torch.randn(*s, generator=g, dtype=torch.float64) * gain / fan ** 0.5
        sd[m + ".bias"] = torch.randn(s[0], generator=g, dtype=torch.float64) * 0.1
    return {k: sd[k] for k in names(cfg, scale)}


def pixel_shuffle(x, r, mut=None):
    """net_ref.pixel_shuffle, or with the sub-pixel index in front of the channel ("shuffle_order")"""
    if mut != "shuffle_order":
        return net_ref.pixel_shuffle(x, r)
    B, Cr, H, W = x.shape
    C = Cr // (r * r)
    return x.reshape(B, r, r, C, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, C, r * H, r * W)


def forward(sd, x, cfg, scale, store=None, mut=None, gff_once=False):
    """sd: name -> tensor (the model's state_dict, any float dtype; the computation runs in x's dtype, pass float64)."""
    D, C, G = config(cfg)
    w = {k: v.to(x.dtype) for k, v in sd.items()}
    q = lambda t: net_ref.q(t, store)
    G0 = w["SFENet1.weight"].shape[0]
    conv = lambda t, name, pad: F.conv2d(t, q(w[name + ".weight"]), w[name + ".bias"], padding=pad)
    f1 = q(conv(q(x), "SFENet1", 1))
    t = q(conv(f1, "SFENet2", 1))
    outs = []
    for d in range(D):
        xin, buf = t, t
        for c in range(C):
            src = buf
            if mut == "short_read" and c >= 1:           # the newest slice is not read
                src = torch.cat([buf[:, :-G], torch.zeros_like(buf[:, -G:])], dim=1)
            new = q(F.relu(conv(src, f"RDBs.{d}.convs.{c}.conv.0", 1)))
            if mut == "slot_off" and c == 0:             # layer 0 writes the slot of layer 1, which overwrites it: its own slot stays empty
                new = torch.zeros_like(new)
            buf = torch.cat([buf, new], dim=1)
        z = conv(buf, f"RDBs.{d}.LFF", 0)
        t = q(z if mut == "lff_no_residual" else z + xin)
        if mut == "drop_block" and d == D - 1:
            t = xin
        outs.append(t)
    if mut == "gff_swap":
        outs[0], outs[1] = outs[1], outs[0]
    if store is None or gff_once:          # gff_once: the concatenating order under storage rounding (GFF.0's output rounded once)
        acc = q(conv(torch.cat(outs, dim=1), "GFF.0", 0))
    else:            # the native order: one K slice per block, the running sum stored after each
        wg, acc = q(w["GFF.0.weight"]), None
        for d in range(D):
            part = F.conv2d(outs[d], wg[:, d * G0:(d + 1) * G0], w["GFF.0.bias"] if d == 0 else None)
            acc = q(part if acc is None else part + acc)
    z = conv(acc, "GFF.1", 1)
    t = q(z if mut == "no_global_residual" else z + f1)
    r = 2 if scale == 4 else scale
    t = pixel_shuffle(q(conv(t, "UPNet.0", 1)), r, mut)
    if scale == 4:
        if mut == "skip_stage2":
            t = F.interpolate(t, scale_factor=2, mode="nearest")
        else:
            t = pixel_shuffle(q(conv(t, "UPNet.2", 1)), 2, mut)
        return q(conv(t, "UPNet.4", 1))
    return q(conv(t, "UPNet.2", 1))


def run(sd, x, target, cfg, scale, store=None, mut=None, loss_scale=1.0, gff_once=False):
    """Forward, L1 loss against ``target`` (times ``loss_scale``) and backward in float64 -> (y, loss, dx, {name: gradient}) as float64
    CPU tensors (a parameter a mutation leaves unused has a zero gradient)."""
    return net_ref.run_l1(lambda w, v: forward(w, v, cfg, scale, store, mut, gff_once), sd, x, target, loss_scale=loss_scale)


def pack_gradients(named, suffix=""):
    """The fixture's layout of a run's parameter gradients, {name: numpy array} in parameters() order -> npz entries.  A 'B' network has
    300 parameters, so the entries are few and stacked (an .npz entry costs some 300 bytes of headers): the gradients of at most BIG
    elements whole, flattened one behind the other (``gsmall``, with ``gsmall_off``), of the others the sketches stacked (``gsketch``)
    and the first slices flattened (``gslice``, ``gslice_off``); ``small`` / ``big`` hold the names."""
    small = [(k, g) for k, g in named if g.size <= BIG]
    big = [(k, g) for k, g in named if g.size > BIG]
    off = lambda parts: np.cumsum([0] + [p.size for p in parts]).astype(np.int64)
    slices = [first_slice(torch.from_numpy(g)).numpy().reshape(-1) for _, g in big]
    return {"small": np.array([k for k, _ in small]), "big": np.array([k for k, _ in big]),
            "gsmall" + suffix: np.concatenate([g.reshape(-1) for _, g in small]), "gsmall_off": off([g for _, g in small]),
            "gsketch" + suffix: np.stack([sketch(g) for _, g in big]), "gslice" + suffix: np.concatenate(slices), "gslice_off": off(slices)}


def fixture_errors(z, y, loss, dx, grads, suffix="", measure=None):
    """{what: relative error} of a run against a fixture's float32 (suffix "") or float64 ("64") values: y, loss, dx and every parameter
    gradient -- whole where the fixture holds it whole, through sketch and first slice where it does not.  measure(a, b): rel_l2, or the
    project's fp32 gate measure, conftest.rel_err."""
    m = measure or rel_l2
    e = net_ref.fixture_head(z, y, loss, dx, suffix, measure)
    assert sorted(grads) == sorted([str(k) for k in z["small"]] + [str(k) for k in z["big"]])
    so, lo = z["gsmall_off"], z["gslice_off"]
    for i, k in enumerate(map(str, z["small"])):
        e["grad " + k] = m(grads[k].detach().double().cpu().reshape(-1), z["gsmall" + suffix][so[i]:so[i + 1]])
    for i, k in enumerate(map(str, z["big"])):
        g = grads[k].detach().double().cpu()
        e["grad " + k] = max(m(sketch(g.numpy()), z["gsketch" + suffix][i]), m(first_slice(g).reshape(-1), z["gslice" + suffix][lo[i]:lo[i + 1]]))
    return e
