"""Float64 restatement of RCAN for the tests (our own words; the formulas are those of the Residual Channel Attention Network,
arXiv:1807.02758): a function of a state_dict, so it runs with any weights, on the CPU, and autograd gives its gradients.

    sub_mean (1x1) -> head (3x3) -> groups x [ blocks x [3x3, ReLU, 3x3, channel attention, + block input], 3x3, + group input ]
    -> 3x3, + head output -> per stage [3x3 to r^2 F, PixelShuffle(r)] -> 3x3 to 3 -> add_mean (1x1)

``store``: None, or a 16-bit torch dtype -- the storage emulation: the input, every tensor an op of the native executor writes and
every 3x3 convolution weight is rounded to that type (forward only: the backward is the exact one of the rounded forward); biases,
the attention MLP and the MeanShift parameters stay as they are, as in the native code."""
import torch
import torch.nn.functional as F

import net_ref
from net_ref import sketch          # noqa: F401  (tests/test_rcan_host.py takes it from here)


def channel_attention(t, w1, b1, w2, b2):
    p = t.mean(dim=(2, 3), keepdim=True)
    h = torch.relu(F.conv2d(p, w1, b1))
    return t * torch.sigmoid(F.conv2d(h, w2, b2))


def forward(sd, x, n_resgroups, n_resblocks, scale, store=None):
    """sd: name -> tensor (the model's state_dict, any float dtype; the computation runs in x's dtype, pass float64)."""
    w = {k: v.to(x.dtype) for k, v in sd.items()}
    q = lambda t: net_ref.q(t, store)
    conv = lambda t, name: F.conv2d(t, q(w[name + ".weight"]), w[name + ".bias"], padding=1)
    t = q(F.conv2d(q(x), w["sub_mean.weight"], w["sub_mean.bias"]))
    head = t = q(conv(t, "head.0"))
    for g in range(n_resgroups):
        gin = t
        for b in range(n_resblocks):
            k = f"body.{g}.body.{b}.body."
            xin = t
            t = q(torch.relu(conv(xin, k + "0")))
            t = q(conv(t, k + "2"))
            t = q(channel_attention(t, w[k + "3.conv_du.0.weight"], w[k + "3.conv_du.0.bias"], w[k + "3.conv_du.2.weight"], w[k + "3.conv_du.2.bias"]) + xin)
        t = q(conv(t, f"body.{g}.body.{n_resblocks}") + gin)
    t = q(conv(t, f"body.{n_resgroups}") + head)
    stages = [(0, 3)] if scale == 3 else [(2 * i, 2) for i in range({2: 1, 4: 2, 8: 3}[scale])]
    for idx, r in stages:
        t = q(F.pixel_shuffle(q(conv(t, f"tail.0.{idx}")), r))
    t = q(conv(t, "tail.1"))
    return q(F.conv2d(t, w["add_mean.weight"], w["add_mean.bias"]))


def run(sd, x, target, n_resgroups, n_resblocks, scale, store=None, frozen=("sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias")):
    """Forward, L1 loss against ``target`` and backward in float64 -> (y, loss, dx, {name: gradient}) as float64 CPU tensors."""
    return net_ref.run_l1(lambda w, v: forward(w, v, n_resgroups, n_resblocks, scale, store), sd, x, target, frozen=frozen)
