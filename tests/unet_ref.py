"""Float64 restatement of the U-Net translator for the tests (our own words; the network is the generator of Image-to-Image Translation with
Conditional Adversarial Networks, arXiv:1611.07004, appendix 6.1.1, as pix2pix's ``UnetGenerator`` builds it), with InstanceNorm and biases:
a function of a state_dict, without in-place operations and without a recursion, so it runs with any weights, on the CPU, and autograd
gives its gradients.

Levels l = 1 (outermost) .. n, widths C_l = ngf min(2^(l-1), 8); conv = 4x4 stride 2 pad 1, deconv = ConvTranspose2d 4x4 stride 2 pad 1.

    down:  d_1 = conv(x);  d_l = IN(conv(leaky(d_{l-1}, 0.2))), 1 < l < n;  d_n = conv(leaky(d_{n-1}))        (the innermost has no IN)
    up:    u_{n-1} = IN(deconv(relu(d_n)));  u_{l-1} = IN(deconv([relu(d_l) | relu(u_l)]));  y = tanh(deconv([relu(d_1) | relu(u_1)]))

The original applies its LeakyReLU in place on the tensor it also concatenates, so its concatenation carries leaky(d_l); the only reader
of a concatenation is a ReLU, and relu(leaky(z)) = relu(z): the same function and the same gradients (tests/test_unet_ref.py holds this
restatement to the original's float64 run within 1e-10).

Every bias in front of an IN -- all but the first and the last down convolution's and the last transposed convolution's -- has a gradient
that is zero in exact arithmetic (``dead_biases``), held in the absolute measure ``dead_ratio`` of resnetgen_ref.

``store``: None, or a 16-bit torch dtype -- the storage emulation: the input, every tensor an op of the native executor writes (a
convolution's output behind its fused activation, both activated outputs of an IN, the tanh) and every convolution weight is rounded to that
type (forward only); biases stay as they are.  ``round_grads`` (with ``store``): the gradient of every convolution output that an IN follows
is rounded to that type as well, on its way back -- the tensor the native backward stores in 16 bits and sums into that convolution's bias
gradient.  In exact arithmetic the sum is zero; what the rounding leaves there is the yardstick for the dead biases in the 16-bit modes, which
the forward-only emulation (1e-15) cannot give.  ``mut`` names one deliberate mistake: MUTATIONS (tests/test_unet_teeth.py)."""
import torch
import torch.nn.functional as F

import net_ref
from net_ref import rel_l2, sketch, worst                      # noqa: F401  (the tests take them from here)
from resnetgen_ref import dead_ratio, fixture_errors           # noqa: F401  (the same fixture layout, the same absolute measure)

MUTATIONS = ("halves_swapped", "skip_without_relu", "down_relu", "parity_taps", "inner_norm", "inner_2c", "no_first_bias")


class _RoundGrad(torch.autograd.Function):
    """identity whose gradient is rounded to ``store`` on the way back"""

    @staticmethod
    def forward(ctx, t, store):
        ctx.store = store
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.store).to(g.dtype), None


def _prefix(l):
    """state_dict prefix of block l's nn.Sequential: the submodule sits at index 1 of the outermost block, at 3 of every other"""
    return "model.model" + "".join((".1" if k == 2 else ".3") + ".model" for k in range(2, l + 1))


def down_modules(n):
    return [_prefix(1) + ".0"] + [_prefix(l) + ".1" for l in range(2, n + 1)]


def up_modules(n):
    """innermost first, the order they run in and the order of the state_dict"""
    return [_prefix(n) + ".3"] + [_prefix(l) + ".5" for l in range(n - 1, 1, -1)] + [_prefix(1) + ".3"]


def names(n):
    return [f"{m}.{p}" for m in down_modules(n) + up_modules(n) for p in ("weight", "bias")]


def dead_biases(n):
    return [m + ".bias" for m in down_modules(n)[1:-1] + up_modules(n)[:-1]]


def forward(sd, x, n, store=None, mut=None, round_grads=False):
    """sd: name -> tensor (any float dtype; the computation runs in x's dtype, pass float64)."""
    assert mut is None or mut in MUTATIONS
    w = {k: v.to(x.dtype) for k, v in sd.items()}
    q = lambda t: net_ref.q(t, store)
    qn = (lambda t: _RoundGrad.apply(q(t), store)) if round_grads and store is not None else q         # a convolution output in front of an IN
    dn, up = down_modules(n), up_modules(n)
    inorm = lambda t: F.instance_norm(t, eps=1e-5)
    leaky = (lambda t: F.relu(t)) if mut == "down_relu" else (lambda t: F.leaky_relu(t, 0.2))
    skip_act = (lambda t: t) if mut == "skip_without_relu" else F.relu

    def conv(t, m, bias=True):
        return F.conv2d(t, q(w[m + ".weight"]), w[m + ".bias"] if bias else None, stride=2, padding=1)

    def deconv(t, m):
        wt = q(w[m + ".weight"])
        if mut == "parity_taps":            # even output rows take the kernel rows of the odd ones and the reverse
            wt = wt[:, :, [1, 0, 3, 2]]
        return F.conv_transpose2d(t, wt, w[m + ".bias"], stride=2, padding=1)

    z = conv(q(x), dn[0], bias=mut != "no_first_bias")
    a = q(leaky(z))                         # the epilogue stores leaky(z); relu of the stored value is relu(z), rounded once
    skips = [q(skip_act(z)) if mut == "skip_without_relu" else F.relu(a)]
    for l in range(2, n):
        z = inorm(qn(conv(a, dn[l - 1])))
        a = q(leaky(z))
        skips.append(q(skip_act(z)))
    z = conv(a, dn[n - 1])
    if mut == "inner_norm":
        z = inorm(z)
    h = q(F.relu(z))
    for k, l in enumerate(range(n - 1, 0, -1)):
        if k == 0 and mut == "inner_2c":    # a second half, the ReLU of the negated tensor, through a copy of the weight's rows
            t = F.conv_transpose2d(torch.cat([h, q(F.relu(-z))], 1), torch.cat([q(w[up[0] + ".weight"])] * 2, 0), w[up[0] + ".bias"], stride=2, padding=1)
        else:
            t = deconv(h, up[k])
        u = q(F.relu(inorm(qn(t))))
        h = torch.cat([u, skips[l - 1]] if mut == "halves_swapped" else [skips[l - 1], u], 1)
    return q(torch.tanh(q(deconv(h, up[n - 1]))))


def run(sd, x, target, n, store=None, loss_scale=1.0, mut=None, round_grads=False):
    """Forward, L1 loss against ``target`` (times ``loss_scale``) and backward in float64 -> (y, loss, dx, {name: gradient})."""
    return net_ref.run_l1(lambda w, v: forward(w, v, n, store, mut, round_grads), sd, x, target, loss_scale=loss_scale, missing="absent")
