"""Float64 restatement of the ResNet translator for the tests (our own words; the network is the generator of Unpaired Image-to-Image
Translation using Cycle-Consistent Adversarial Networks, arXiv:1703.10593, appendix 7.2: c7s1-k, d2k, d4k, R4k x n, u2k, uk, c7s1-out),
with InstanceNorm and biases: functions of a state_dict, so they run with any weights, on the CPU, and autograd gives their gradients.

    pad_p(x)[i][j] = x[r(i, H)][r(j, W)],  r(i, H) = p - i (i < p),  2 (H - 1) - (i - p) (i >= H + p),  i - p otherwise
    stem:    IN+ReLU(conv7(pad_3(x)));  twice IN+ReLU(conv3 stride 2 pad 1)
    block:   x + IN(conv3(pad_1(ReLU(IN(conv3(pad_1(x)))))))            ('zero': conv3 with zero padding 1, no pad_1)
    tail:    twice IN+ReLU(deconv3 stride 2 pad 1 output_padding 1);  tanh(conv7(pad_3(.)))

Every bias but the last sits in front of an IN, which removes it: its gradient is zero in exact arithmetic (``dead_biases``).  The tests
hold those to an ABSOLUTE measure, ``dead_ratio`` = max|g_bias| / max|g_weight of the layer|; a relative one explodes on them
(tests/test_resnetgen_teeth.py).

``store``: None, or a 16-bit torch dtype -- the storage emulation: the input, every tensor an op of the native executor writes (each
convolution's output, each IN's output behind its ReLU / residual, the tanh) and every convolution weight is rounded to that type
(forward only); the pads copy, biases stay as they are.

Also here, in numpy float64 on NHWC arrays: references of the pad (``reflect_pad``), of its backward written as the SCATTER it is the
adjoint of (``reflect_pad_bwd``; the kernel is a gather) and of tanh' (``tanh_bwd``).  ``mut`` names one deliberate mistake: MUTATIONS."""
import numpy as np
import torch
import torch.nn.functional as F

import net_ref
from net_ref import rel_l2, sketch, worst          # noqa: F401  (the tests take them from here)

MUTATIONS = ("dropped_mirror", "symmetric", "replicate", "swapped_axes", "acc_overwrites", "term_twice", "tanh_from_z")


# ------------------------------------------------------------------------------------------------------------ kernels
def r(i, n, p, mut=None):
    """source index of padded index i on an axis of n pixels"""
    if mut == "replicate":
        return min(max(i - p, 0), n - 1)
    if mut == "symmetric":              # the edge pixel repeated: off by one on both mirrors
        return p - 1 - i if i < p else 2 * n - 1 - (i - p) if i >= n + p else i - p
    return p - i if i < p else 2 * (n - 1) - (i - p) if i >= n + p else i - p


def _maps(H, W, p, mut):
    if mut == "swapped_axes":           # the rows mirrored by the columns' rule and the reverse (clipped into the image)
        ri = [min(max(r(i, W, p), 0), H - 1) for i in range(H + 2 * p)]
        rj = [min(max(r(j, H, p), 0), W - 1) for j in range(W + 2 * p)]
        return np.array(ri), np.array(rj)
    return np.array([r(i, H, p, mut) for i in range(H + 2 * p)]), np.array([r(j, W, p, mut) for j in range(W + 2 * p)])


def reflect_pad(x, p, mut=None):
    """x [B, H, W, C] -> [B, H + 2p, W + 2p, C] by indexing with r()"""
    ri, rj = _maps(x.shape[1], x.shape[2], p, mut)
    return x[:, ri][:, :, rj]


def reflect_pad_bwd(dy, H, W, p, old=None, mut=None):
    """dy [B, H + 2p, W + 2p, C] float64 -> (dx [B, H, W, C], sum of |terms|): every padded pixel adds its gradient to its source, then
    the old dx (``old``: accumulate)."""
    dy = np.asarray(dy, dtype=np.float64)
    ri, rj = _maps(H, W, p, mut)
    dx = np.zeros((dy.shape[0], H, W, dy.shape[3]))
    mag = np.zeros_like(dx)
    for i in range(H + 2 * p):
        if mut == "dropped_mirror" and i < p:
            continue
        rep = 2 if (mut == "term_twice" and i < p) else 1
        for _ in range(rep):
            np.add.at(dx, (slice(None), ri[i], rj), dy[:, i])
            np.add.at(mag, (slice(None), ri[i], rj), np.abs(dy[:, i]))
    if old is not None and mut != "acc_overwrites":
        dx += np.asarray(old, dtype=np.float64)
        mag += np.abs(np.asarray(old, dtype=np.float64))
    return dx, mag


def tanh_bwd(dy, y, z=None, old=None, mut=None):
    """dz = dy (1 - y^2) from the saved OUTPUT (+ old)"""
    dy, y = np.asarray(dy, dtype=np.float64), np.asarray(y, dtype=np.float64)
    s = np.asarray(z, dtype=np.float64) if mut == "tanh_from_z" else y
    g = dy * (1.0 - s * s)
    return g if old is None or mut == "acc_overwrites" else g + np.asarray(old, dtype=np.float64)


def reflect_pad_bwd_rows(dy, H, W, p, r0, r1):
    """Rows [r0, r1) of the pad's backward by slices and flipped slices, in torch float32 on dy's device (exact while the values are small
    integers): what the test past 2 GiB compares against band by band, without a second padded copy.  dy [B, H + 2p, W + 2p, C]."""
    S = dy[:, r0 + p:r1 + p].float()
    for i in range(max(r0, 1), min(r1, p + 1)):
        S[:, i - r0] += dy[:, p - i].float()
    for i in range(max(r0, H - 1 - p), min(r1, H - 1)):
        S[:, i - r0] += dy[:, p + 2 * (H - 1) - i].float()
    out = S[:, :, p:p + W].clone()
    out[:, :, 1:p + 1] += S[:, :, :p].flip(2)
    out[:, :, W - 1 - p:W - 1] += S[:, :, W + p:W + 2 * p].flip(2)
    return out


# ------------------------------------------------------------------------------------------------------------ the network
def conv_modules(n_blocks, padding="reflect"):
    """the modules with parameters, in state_dict order"""
    a, b = (1, 5) if padding == "reflect" else (0, 3)
    mods = ["model.1", "model.4", "model.7"]
    mods += [f"model.{10 + k}.conv_block.{c}" for k in range(n_blocks) for c in (a, b)]
    return mods + [f"model.{10 + n_blocks}", f"model.{13 + n_blocks}", f"model.{17 + n_blocks}"]


def names(n_blocks, padding="reflect"):
    return [f"{m}.{p}" for m in conv_modules(n_blocks, padding) for p in ("weight", "bias")]


def dead_biases(n_blocks, padding="reflect"):
    return [m + ".bias" for m in conv_modules(n_blocks, padding)[:-1]]


def forward(sd, x, n_blocks, padding="reflect", store=None):
    """sd: name -> tensor (any float dtype; the computation runs in x's dtype, pass float64)."""
    w = {k: v.to(x.dtype) for k, v in sd.items()}
    q = lambda t: net_ref.q(t, store)
    mods = conv_modules(n_blocks, padding)
    pad = lambda t, p: F.pad(t, (p, p, p, p), mode="reflect")
    conv = lambda t, m, **kw: q(F.conv2d(t, q(w[m + ".weight"]), w[m + ".bias"], **kw))
    norm = lambda t, relu=True, res=None: q(F.relu(F.instance_norm(t, eps=1e-5)) if relu else F.instance_norm(t, eps=1e-5) + res)
    t = norm(conv(pad(q(x), 3), mods[0]))
    t = norm(conv(t, mods[1], stride=2, padding=1))
    t = norm(conv(t, mods[2], stride=2, padding=1))
    for k in range(n_blocks):
        m1, m2 = mods[3 + 2 * k], mods[4 + 2 * k]
        if padding == "reflect":
            h = norm(conv(pad(t, 1), m1))
            t = norm(conv(pad(h, 1), m2), relu=False, res=t)
        else:
            h = norm(conv(t, m1, padding=1))
            t = norm(conv(h, m2, padding=1), relu=False, res=t)
    for m in mods[-3:-1]:
        t = norm(q(F.conv_transpose2d(t, q(w[m + ".weight"]), w[m + ".bias"], stride=2, padding=1, output_padding=1)))
    return q(torch.tanh(conv(pad(t, 3), mods[-1])))


def run(sd, x, target, n_blocks, padding="reflect", store=None, loss_scale=1.0):
    """Forward, L1 loss against ``target`` (times ``loss_scale``) and backward in float64 -> (y, loss, dx, {name: gradient})."""
    return net_ref.run_l1(lambda w, v: forward(w, v, n_blocks, padding, store), sd, x, target, loss_scale=loss_scale, missing="absent")


def dead_ratio(grads, name):
    """max|g_bias| / max|g_weight| of the layer of bias ``name``: the bias gradient in units of its layer's weight gradient"""
    return float(grads[name].detach().abs().max()) / float(grads[name[:-4] + "weight"].detach().abs().max())


def fixture_errors(z, y, loss, dx, grads, suffix="", measure=None):
    """({what: relative error}, {dead bias: dead_ratio}) of a run against a fixture's float32 (suffix "") or float64 ("64") values: y,
    loss, dx and every LIVE parameter gradient -- whole where the fixture holds it whole, through sketch and first slice where it does
    not.  The dead biases are reported in their absolute measure and compared with nothing."""
    e = net_ref.fixture_head(z, y, loss, dx, suffix, measure)
    dead = [str(k) for k in z["dead"]]
    assert list(grads) == [str(k) for k in z["names"]]
    for k, g in grads.items():
        if k not in dead:
            e["grad " + k] = net_ref.keyed_grad_error(z, k, g, suffix, measure)
    return e, {k: dead_ratio(grads, k) for k in dead}
