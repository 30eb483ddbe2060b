"""Float64 restatement of MDSR and VDSR for the tests (our own words; the formulas are those of Enhanced Deep Residual Networks for
Single Image Super-Resolution, arXiv:1707.02921, section 3.3 / figure 5, and of Accurate Image Super-Resolution Using Very Deep
Convolutional Networks, arXiv:1511.04587): functions of a state_dict, so they run with any weights, on the CPU, and autograd gives
their gradients.

    shift(x; W, b) = W x + b per pixel (a frozen 1x1 convolution on the colours)
    block_k(x) = conv_k(ReLU(conv_k(x))) + x                                  k x k convolutions, padding k // 2, with bias
    MDSR, branch i:  h = conv3(shift_sub(x));  p = block_5(block_5(h))        the two 5x5 blocks of branch i
                     r = conv3(block_3(... block_3(p))) + p                   n_resblocks blocks; the skip starts BEHIND the 5x5 blocks
                     y = shift_add(conv3(up_i(r)))                            up_i: (3x3 to r^2 F, PixelShuffle(r)): r = 3 once, r = 2 once per x2
    VDSR:            s = shift_sub(x);  y = shift_add(conv3(ReLU(conv3(... ReLU(conv3(s))))) + s)       n_resblocks convolutions

Parameters of the branches j != i take no part: their gradient is None (``run`` reports no entry for them).

``store``: None, or a 16-bit torch dtype -- the storage emulation: the input, every tensor an op of the native executor writes (the
shifts' outputs, every convolution's output behind its fused ReLU / residual) and every convolution weight is rounded to that type
(forward only: the backward is the exact one of the rounded forward); biases and the shifts' parameters stay as they are.

``mut`` names one deliberate mistake (tests/test_mdsr_teeth.py): MUTATIONS."""
import torch.nn.functional as F

import net_ref
from net_ref import pixel_shuffle, rel_l2, sketch, worst          # noqa: F401  (the tests take them from here)

MUTATIONS = ("wrong_branch", "skip_from_head", "k3_crop", "no_relu", "vdsr_skip_after_add_mean", "inactive_grad")


def up_convs(scale):
    """indices inside upsample.<i> of the convolutions of scale ``scale`` (each followed by its PixelShuffle)"""
    return [0] if scale == 3 else [2 * j for j in range({2: 1, 4: 2, 8: 3}[scale])]


def mdsr_names(n_resblocks, scales):
    """state_dict keys = parameters() order of the reference class"""
    mods = ["sub_mean", "add_mean"]
    mods += [f"pre_process.{i}.{b}.body.{c}" for i in range(len(scales)) for b in (0, 1) for c in (0, 2)]
    mods += [f"upsample.{i}.{c}" for i, s in enumerate(scales) for c in up_convs(s)]
    mods += ["head.0"] + [f"body.{k}.body.{c}" for k in range(n_resblocks) for c in (0, 2)] + [f"body.{n_resblocks}", "tail.0"]
    return [f"{m}.{p}" for m in mods for p in ("weight", "bias")]


def vdsr_names(n_resblocks):
    return [f"{m}.{p}" for m in ["sub_mean", "add_mean"] + [f"body.{k}.0" for k in range(n_resblocks)] for p in ("weight", "bias")]


def mdsr_branch(n_resblocks, scales, idx):
    """the names on the graph of branch idx, frozen shifts excluded"""
    off = [n for n in mdsr_names(n_resblocks, scales)
           if any(n.startswith(f"{part}.{j}.") for part in ("pre_process", "upsample") for j in range(len(scales)) if j != idx)]
    return [n for n in mdsr_names(n_resblocks, scales) if n not in off and not n.startswith(("sub_mean", "add_mean"))]


class _Net:
    def __init__(self, sd, x, store, mut):
        self.w = {k: v.to(x.dtype) for k, v in sd.items()}
        self.store, self.mut = store, mut

    def q(self, t):
        return net_ref.q(t, self.store)

    def shift(self, t, name):
        return self.q(F.conv2d(t, self.w[name + ".weight"], self.w[name + ".bias"]))

    def conv(self, t, name, relu=False, res=None, crop=False):
        """one op of the native executor: convolution + bias (+ ReLU) (+ res), stored once"""
        w = self.q(self.w[name + ".weight"])
        if crop:
            w = w[:, :, 1:-1, 1:-1]
        z = F.conv2d(t, w, self.w[name + ".bias"], padding=w.shape[-1] // 2)
        if relu and self.mut != "no_relu":
            z = F.relu(z)
        return self.q(z if res is None else z + res)

    def block(self, t, name, crop=False):
        return self.conv(self.conv(t, name + ".body.0", relu=True, crop=crop), name + ".body.2", res=t, crop=crop)


def mdsr_forward(sd, x, n_resblocks, scales, idx, store=None, mut=None):
    """sd: name -> tensor (the model's state_dict, any float dtype; the computation runs in x's dtype, pass float64)."""
    n = _Net(sd, x, store, mut)
    if mut == "wrong_branch":
        idx = (idx + 1) % len(scales)
    h = n.conv(n.shift(n.q(x), "sub_mean"), "head.0")
    p = h
    for b in (0, 1):
        p = n.block(p, f"pre_process.{idx}.{b}", crop=mut == "k3_crop")
    t = p
    for k in range(n_resblocks):
        t = n.block(t, f"body.{k}")
    t = n.conv(t, f"body.{n_resblocks}", res=h if mut == "skip_from_head" else p)
    for c in up_convs(scales[idx]):
        t = pixel_shuffle(n.conv(t, f"upsample.{idx}.{c}"), 3 if scales[idx] == 3 else 2)
    return n.shift(n.conv(t, "tail.0"), "add_mean")


def vdsr_forward(sd, x, n_resblocks, store=None, mut=None):
    n = _Net(sd, x, store, mut)
    x = n.q(x)
    s = n.shift(x, "sub_mean")
    t = s
    for k in range(n_resblocks - 1):
        t = n.conv(t, f"body.{k}.0", relu=True)
    if mut == "vdsr_skip_after_add_mean":       # the image itself added behind add_mean: off by the colour means (adding s there is the same function)
        return n.q(n.shift(n.conv(t, f"body.{n_resblocks - 1}.0"), "add_mean") + x)
    return n.shift(n.conv(t, f"body.{n_resblocks - 1}.0", res=s), "add_mean")


def run(sd, x, target, forward, store=None, mut=None, loss_scale=1.0):
    """Forward (``forward(sd, x, store, mut)``), L1 loss against ``target`` (times ``loss_scale``) and backward in float64 ->
    (y, loss, dx, {name: gradient}) as float64 CPU tensors.  A parameter that is not on the graph has no entry (the reference leaves
    its ``.grad`` at None); neither have the frozen shifts.  ``mut`` "inactive_grad": a zero gradient where the reference has none (what
    a zero fill of the whole arena would report)."""
    return net_ref.run_l1(lambda w, v: forward(w, v, store, mut), sd, x, target, frozen=lambda k: k.startswith(("sub_mean", "add_mean")),
                          loss_scale=loss_scale, missing="zero" if mut == "inactive_grad" else "absent")


def mdsr_run(sd, x, target, n_resblocks, scales, idx, **kw):
    return run(sd, x, target, lambda s, v, store, mut: mdsr_forward(s, v, n_resblocks, scales, idx, store, mut), **kw)


def vdsr_run(sd, x, target, n_resblocks, **kw):
    return run(sd, x, target, lambda s, v, store, mut: vdsr_forward(s, v, n_resblocks, store, mut), **kw)


def fixture_grad_names(z):
    """the parameters a fixture holds a gradient of, in ``names`` order"""
    return [str(k) for k in z["names"] if "grad/" + str(k) in z or "gsketch/" + str(k) in z]


def fixture_errors(z, y, loss, dx, grads, suffix="", measure=None):
    """{what: relative error} of a run against a fixture's float32 (suffix "") or float64 ("64") values: y, loss, dx and every parameter
    gradient -- whole where the fixture holds it whole, through sketch and first output-channel slice where it does not.  The set of
    parameters with a gradient must be the fixture's.  measure(a, b): rel_l2, or the project's fp32 gate measure, conftest.rel_err."""
    e = net_ref.fixture_head(z, y, loss, dx, suffix, measure)
    assert sorted(grads) == sorted(fixture_grad_names(z)), sorted(set(grads) ^ set(fixture_grad_names(z)))
    assert not set(grads) & {str(k) for k in z["nograd"]} and not set(grads) & {str(k) for k in z["frozen"]}
    for k, g in grads.items():
        e["grad " + k] = net_ref.keyed_grad_error(z, k, g, suffix, measure)
    return e
