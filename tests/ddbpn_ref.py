"""Float64 restatement of DDBPN for the tests (our own words; the formulas are those of Deep Back-Projection Networks,
arXiv:1803.02735): a function of a state_dict, so it runs with any weights, on the CPU, and autograd gives its gradients.

    sub_mean (1x1) -> 3x3 (3 -> 128) + PReLU -> 1x1 (128 -> 32) + PReLU -> six up- and five down-modules, alternating, each fed the
    concatenation of all earlier outputs at its resolution -> 3x3 over the six HR outputs -> add_mean (1x1)
    module(x): [x = PReLU(1x1(x))]  a0 = P(x);  e = P'(a0) - x;  out = a0 + P(e)      P, P' = projection + PReLU, up / down or down / up

A projection is Conv2d / ConvTranspose2d with (k, s, p) = (6, 2, 2), (8, 4, 2), (12, 8, 2).  ``s1=True`` runs each as the native code
does: a stride-1 convolution with T = ceil(k / s) taps per axis over a shifted space-to-depth view (``down_s1`` / ``up_s1`` with
``pack_down`` / ``pack_up``, ``s2d_shift`` / ``d2s_shift``); ``mut`` names one deliberate mistake in that route (tests/test_back_proj_teeth.py).

``store``: None, or a 16-bit torch dtype -- the storage emulation: the input, every tensor an op of the native executor writes and
every convolution weight is rounded to that type (forward only: the backward is the exact one of the rounded forward); biases and PReLU
slopes stay as they are, and a transposed projection's bias is added after its output was stored, as in the native code.

Also here: the PReLU backward formula, a numpy-float32 restatement of the PReLU backward kernel's summation order
(``prelu_param_sums_f32``) from which the tolerance of the slope / bias gradients is measured, and the rule both the fixture generator
and the tests use to move the PReLU slopes away from their initial 0.25 (``set_slopes``)."""
import numpy as np
import torch
import torch.nn.functional as F

import net_ref
from net_ref import sketch          # noqa: F401  (the fixture test and tests/test_ddbpn_host.py take it from here)

PROJ = {2: (6, 2, 2), 4: (8, 4, 2), 8: (12, 8, 2)}
N0, NR, DEPTH = 128, 32, 6
FROZEN = ("sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias")
PR_CHUNK = 2048         # grid positions per partial-sum block of the PReLU backward kernel

# da[c] / db[c] of the PReLU backward may differ from float64 by K * 2^-24 * sum |terms|.  K is 4 x the largest figure of the numpy-float32
# restatement of the kernel's summation order over the cases of tests/test_gpu_back_proj.py, rounded up to the next integer and nothing else
# (measured on the CPU: da 1.55 -> 6.2 -> 7, db 0.92 -> 3.7 -> 4; the terms' own float32 roundings are part of the figure;
# tests/test_back_proj_teeth.py re-measures it).
K_RECORDED = {"da": 7.0, "db": 4.0}


def set_slopes(model, seed):
    """Move every PReLU slope away from 0.25, in place: slope k (in parameters() order) of n channels gets uniform values in
    [-0.3, 1.3] from RandomState(7919 * seed + k), rounded to float32, with every fifth one (i % 5 == 2) exactly 0."""
    k = 0
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.PReLU):
                n = mod.weight.numel()
                v = np.random.RandomState(7919 * int(seed) + k).uniform(-0.3, 1.3, n).astype(np.float32)
                v[np.arange(n) % 5 == 2] = 0.0
                mod.weight.copy_(torch.from_numpy(v).to(mod.weight.dtype))
                k += 1
    return k


# ------------------------------------------------------------------------------------------------ the stride-1 route
def geometry(scale, h, w):
    """(T, shift, Hg, Wg, pad_down, pad_up) of the native plan for an LR size h x w: the grid is (h + 1) x (w + 1) with shift 2; at scale 2
    its border rows are all padding, so it is h x w with shift 0 and both convolutions are 3x3 pad 1."""
    k, s, _ = PROJ[scale]
    T = -(-k // s)
    if scale == 2:
        return T, 0, h, w, 1, 1
    return T, 2, h + 1, w + 1, 0, T - 1


def s2d_shift(x, s, shift, Hg, Wg, mut=None):
    """x [B,C,Hy,Wy] -> g [B, s*s*C, Hg, Wg]: g[(a*s+b)*C + c, m, n] = x[c, s*m + a - shift, s*n + b - shift], zero outside the image."""
    B, C, Hy, Wy = x.shape
    if mut == "offset1":
        shift = shift - 1 if shift else 1
    xp = F.pad(x, (shift, s * Wg - Wy - shift, shift, s * Hg - Hy - shift))
    v = xp.reshape(B, C, Hg, s, Wg, s)
    v = v.permute(0, 5, 3, 1, 2, 4) if mut == "swap_ab" else v.permute(0, 3, 5, 1, 2, 4)
    return v.reshape(B, s * s * C, Hg, Wg)


def d2s_shift(g, C, s, shift, Hy, Wy, mut=None):
    """The adjoint: y[c, oy, ox] = g[(a*s+b)*C + c, m, n] at (s*m + a, s*n + b) = (oy + shift, ox + shift)."""
    B, _, Hg, Wg = g.shape
    if mut == "offset1":
        shift = shift - 1 if shift else 1
    if mut == "drop_border":          # the grid's last row and column lost
        g = torch.cat([g[:, :, :-1], torch.zeros_like(g[:, :, -1:])], dim=2)
    v = g.reshape(B, s, s, C, Hg, Wg)
    v = v.permute(0, 3, 4, 2, 5, 1) if mut == "swap_ab" else v.permute(0, 3, 4, 1, 5, 2)
    v = v.reshape(B, C, s * Hg, s * Wg)
    v = F.pad(v, (0, max(0, shift + Wy - s * Wg), 0, max(0, shift + Hy - s * Hg)))
    return v[:, :, shift:shift + Hy, shift:shift + Wy]


def pack_down(w, s, mut=None):
    """Conv2d weight [co,ci,k,k] -> W2 [co, s*s*ci, T, T]: W2[co, (a*s+b)*ci_n + ci, j, i] = w'[co, ci, s*j + a, s*i + b], w' = w zero-padded
    behind to T*s taps."""
    co, ci, k, _ = w.shape
    T = -(-k // s)
    e = T * s - k
    wp = F.pad(w, (e, 0, e, 0)) if mut == "pad_front" else F.pad(w, (0, e, 0, e))
    v = wp.reshape(co, ci, T, s, T, s).permute(0, 3, 5, 1, 2, 4)
    return v.reshape(co, s * s * ci, T, T)


def pack_up(w, s, mut=None):
    """ConvTranspose2d weight [ci,co,k,k] -> W3 [s*s*co, ci, T, T]: W3[(a*s+b)*co_n + co, ci, j, i] = w'[ci, co, s*(T-1-j) + a, s*(T-1-i) + b]."""
    ci, co, k, _ = w.shape
    T = -(-k // s)
    e = T * s - k
    wp = F.pad(w, (e, 0, e, 0)) if mut == "pad_front" else F.pad(w, (0, e, 0, e))
    v = wp.reshape(ci, co, T, s, T, s)
    if mut != "noflip":
        v = v.flip(2, 4)
    v = v.permute(3, 5, 1, 0, 2, 4)
    return v.reshape(s * s * co, ci, T, T)


def down_s1(x, w, b, scale, mut=None):
    """Conv2d(k, s, 2) of an HR tensor [B,C,s*h,s*w] through the gather and a T x T stride-1 convolution -> [B,co,h,w]."""
    _, s, _ = PROJ[scale]
    h, wd = x.shape[2] // s, x.shape[3] // s
    _, shift, Hg, Wg, pad, _ = geometry(scale, h, wd)
    return F.conv2d(s2d_shift(x, s, shift, Hg, Wg, mut), pack_down(w, s, mut), b, padding=pad)


def up_s1(x, w, b, scale, mut=None):
    """ConvTranspose2d(k, s, 2) of an LR tensor through a T x T stride-1 convolution to s*s*co channels and the crop; the bias, one per
    ``co``, is added behind the crop (the native PReLU kernel adds it)."""
    _, s, _ = PROJ[scale]
    h, wd = x.shape[2], x.shape[3]
    _, shift, _, _, _, pad = geometry(scale, h, wd)
    g = F.conv2d(x, pack_up(w, s, mut), None, padding=pad)
    y = d2s_shift(g, w.shape[1], s, shift, s * h, s * wd, mut)
    if b is None:
        return y
    if mut == "bias_once":            # the bias of sub-position (0, 0) only: not replicated over the s*s phases
        mask = torch.zeros_like(y)
        mask[:, :, (s - shift) % s::s, (s - shift) % s::s] = 1
        return y + b.view(1, -1, 1, 1) * mask
    return y + b.view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------ PReLU
def prelu_forward(z, a, r=None, beta=1.0, bias=None, mut=None):
    """y = PReLU_c(z + bias) + beta * r on NCHW tensors; a, bias: [C]."""
    v = z if bias is None else z + bias.view(1, -1, 1, 1)
    pos = v >= 0 if mut == "ge" else v > 0
    y = torch.where(pos, v, a.view(1, -1, 1, 1) * v)
    if r is not None:
        y = y + (-beta if mut == "beta_sign" else beta) * r
    return y


def prelu_backward(dy, z, a, bias=None, mut=None):
    """(dz, da, db): dz = dy * (v > 0 ? 1 : a[c]); da[c] = sum of dy * v over v <= 0; db[c] = sum of dz; v = z + bias."""
    v = z if bias is None else z + bias.view(1, -1, 1, 1)
    pos = v >= 0 if mut == "ge" else v > 0
    dz = torch.where(pos, dy, a.view(1, -1, 1, 1) * dy)
    terms = dy * v if mut == "da_all" else torch.where(pos, torch.zeros_like(v), dy * v)
    return dz, terms.sum(dim=(0, 2, 3)), dz.sum(dim=(0, 2, 3))


def prelu_param_sums_f32(terms_a, terms_b, vec, drop_chunk=None):
    """The PReLU backward kernel's two parameter sums in numpy float32, in the kernel's order.  terms_*: [npos, C], one row per grid
    position in the order the kernel walks them (record-major, then the s*s sub-positions; a position outside the image contributes 0).
    A block takes PR_CHUNK positions with PL = 256 // (C // vec) position lanes; lane l adds positions l, l + PL, ... in ascending order,
    the lanes are folded in lane order; the finishing kernel's lane j adds chunks j, j + 64, ... and lane 0 adds the 64 lane sums."""
    outs = []
    for terms in (terms_a, terms_b):
        t = np.asarray(terms, dtype=np.float32)
        npos, C = t.shape
        PL = 256 // (C // vec)
        nchunk = -(-npos // PR_CHUNK)
        part = np.zeros((nchunk, C), dtype=np.float32)
        for k in range(nchunk):
            blk = t[k * PR_CHUNK:(k + 1) * PR_CHUNK]
            acc = np.zeros((PL, C), dtype=np.float32)
            for i in range(0, blk.shape[0], PL):
                row = blk[i:i + PL]
                acc[:row.shape[0]] = acc[:row.shape[0]] + row
            s = np.zeros(C, dtype=np.float32)
            for l in range(PL):
                s = s + acc[l]
            part[k] = s
        if drop_chunk is not None:
            part[drop_chunk] = 0
        lanes = np.zeros((64, C), dtype=np.float32)
        for k in range(nchunk):
            lanes[k % 64] = lanes[k % 64] + part[k]
        s = np.zeros(C, dtype=np.float32)
        for j in range(64):
            s = s + lanes[j]
        outs.append(s)
    return outs


def sum_error_in_units(got, terms64):
    """max over channels of |got - sum terms| / (2^-24 * sum |terms|), the unit K_RECORDED is written in.  terms64: [npos, C] float64."""
    exact = terms64.sum(axis=0)
    N = np.abs(terms64).sum(axis=0)
    err = np.abs(np.asarray(got, dtype=np.float64) - exact)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(2.0 ** -24 * N, 1e-300))))


# ------------------------------------------------------------------------------------------------ the network
def forward(sd, x, scale, store=None, s1=False, mut=None):
    """sd: name -> tensor (the model's state_dict, any float dtype; the computation runs in x's dtype, pass float64)."""
    w = {k: v.to(x.dtype) for k, v in sd.items()}
    k, s, p = PROJ[scale]
    q = lambda t: net_ref.q(t, store)

    def act(z, slope, res=None, beta=1.0, bias=None):
        return q(prelu_forward(z, w[slope], res, beta, bias, mut))

    def proj(t, name, up, res=None, beta=1.0):
        wt, b = q(w[name + ".0.weight"]), w[name + ".0.bias"]
        if up:      # the transposed projection is stored without its bias; PReLU adds it
            if s1 and mut == "bias_once":
                return act(q(up_s1(t, wt, b, scale, mut)), name + ".1.weight", res, beta)
            z = up_s1(t, wt, None, scale, mut) if s1 else F.conv_transpose2d(t, wt, None, stride=s, padding=p)
            return act(q(z), name + ".1.weight", res, beta, bias=b)
        z = down_s1(t, wt, b, scale, mut) if s1 else F.conv2d(t, wt, b, stride=s, padding=p)
        return act(q(z), name + ".1.weight", res, beta)

    def module(t, name, up, bottleneck):
        if bottleneck:
            t = act(q(F.conv2d(t, q(w[name + ".bottleneck.0.weight"]), w[name + ".bottleneck.0.bias"])), name + ".bottleneck.1.weight")
        a0 = proj(t, name + ".conv_1", up)
        e = proj(a0, name + ".conv_2", not up, res=t, beta=-1.0)
        return proj(e, name + ".conv_3", up, res=a0, beta=1.0)

    t = q(F.conv2d(q(x), w["sub_mean.weight"], w["sub_mean.bias"]))
    t = act(q(F.conv2d(t, q(w["initial.0.weight"]), w["initial.0.bias"], padding=1)), "initial.1.weight")
    t = act(q(F.conv2d(t, q(w["initial.2.weight"]), w["initial.2.bias"])), "initial.3.weight")
    h_list, l_list = [], []
    for i in range(DEPTH - 1):
        lr = t if i == 0 else torch.cat(l_list, dim=1)
        h_list.append(module(lr, f"upmodules.{i}", True, i > 1))
        l_list.append(module(torch.cat(h_list, dim=1), f"downmodules.{i}", False, i != 0))
    h_list.append(module(torch.cat(l_list, dim=1), f"upmodules.{DEPTH - 1}", True, True))
    t = q(F.conv2d(torch.cat(h_list, dim=1), q(w["reconstruction.0.weight"]), w["reconstruction.0.bias"], padding=1))
    return q(F.conv2d(t, w["add_mean.weight"], w["add_mean.bias"]))


def run(sd, x, target, scale, store=None, s1=False, mut=None, frozen=FROZEN, loss_scale=1.0):
    """Forward, L1 loss against ``target`` (times ``loss_scale``) and backward in float64 -> (y, loss, dx, {name: gradient}) as float64
    CPU tensors."""
    return net_ref.run_l1(lambda w, v: forward(w, v, scale, store, s1, mut), sd, x, target, frozen=frozen, loss_scale=loss_scale)


# ------------------------------------------------------------------------------------------------ the kernels' test cases
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
STORE_EPS = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}      # half an ulp of the storage type, relative
KERNEL_SCALES = (2, 4, 8)
KERNEL_SHAPE = dict(B=2, h=3, w=5, C=32)                                 # LR 3 x 5; at scale 8 the grid has 3072 positions: two chunks
SLOPES = (0.0, -0.2, 1.25, 0.25, 1.0, 0.7, -0.05, 0.1)                   # cycled over the channels: 0, negative, > 1, 1 among them


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(a):
    return torch.as_tensor(a).permute(0, 3, 1, 2)


def kernel_inputs(scale, dtype, seed=0):
    """Inputs of one kernel case as float64 NHWC numpy arrays holding values the storage type represents exactly: an HR image x, a grid
    tensor (the pre-shuffle output of a transposed projection) and a plain pre-activation z with exact zeros, a residual r, a gradient
    dy and an earlier residual gradient `old`, all at HR; slopes (SLOPES) and a bias whose every fourth entry is 0, in float32."""
    B, h, w, C = (KERNEL_SHAPE[k] for k in ("B", "h", "w", "C"))
    _, s, _ = PROJ[scale]
    _, shift, Hg, Wg, _, _ = geometry(scale, h, w)
    g = torch.Generator().manual_seed(1000 * scale + seed)
    rt = lambda *shape: torch.randn(*shape, generator=g).to(TDT[dtype]).double()
    inp = dict(scale=scale, s=s, shift=shift, Hg=Hg, Wg=Wg, B=B, Hy=s * h, Wy=s * w, C=C, dtype=dtype)
    for name in ("x", "z", "r", "dy", "old"):
        inp[name] = rt(B, s * h, s * w, C)
    inp["grid"] = rt(B, Hg, Wg, s * s * C)
    inp["z"].view(-1)[::7] = 0.0
    inp["grid"].view(-1)[::5] = 0.0
    inp["slope"] = torch.tensor([SLOPES[c % len(SLOPES)] for c in range(C)], dtype=torch.float32)
    bias = torch.randn(C, generator=g)
    bias[::4] = 0.0
    inp["bias"] = bias
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


def kernel_reference(inp, form, beta, accumulate, mut=None):
    """Float64 results of one PReLU case on the stored inputs.  form "plain": z is inp["z"], no bias; form "grid": z is inp["grid"] read
    through the crop, with the bias.  -> dict: y, dz (in z's layout), dres, da, db, the float64 terms of da / db in the kernel's walk
    order ([npos, C]) and the magnitudes the per-element bounds are written in."""
    s, shift, Hg, Wg, C = inp["s"], inp["shift"], inp["Hg"], inp["Wg"], inp["C"]
    a, r, dy, old = (torch.from_numpy(np.asarray(inp[k], dtype=np.float64)) for k in ("slope", "r", "dy", "old"))
    if form == "plain":
        zi, bias = _nchw(inp["z"]), None
    else:
        zi, bias = d2s_shift(_nchw(inp["grid"]), C, s, shift, inp["Hy"], inp["Wy"], mut), torch.from_numpy(inp["bias"].astype(np.float64))
    v = zi if bias is None else zi + bias.view(1, -1, 1, 1)
    y = prelu_forward(zi, a, _nchw(r), beta, bias, mut)
    dz, da, db = prelu_backward(_nchw(dy), zi, a, bias, mut)
    gd = _nchw(dy)
    pos = v >= 0 if mut == "ge" else v > 0
    ta = gd * v if mut == "da_all" else torch.where(pos, torch.zeros_like(v), gd * v)
    to_grid = (lambda t: _nhwc(t)) if form == "plain" else (lambda t: _nhwc(s2d_shift(t, s, shift, Hg, Wg)))
    dres = beta * gd + (_nchw(old) if accumulate else 0.0)
    out = dict(y=_nhwc(y), dz=to_grid(dz), dres=_nhwc(dres), da=da, db=db,
               terms_a=to_grid(ta).reshape(-1, C), terms_b=to_grid(dz).reshape(-1, C),
               mag_y=_nhwc(v.abs() + (a.view(1, -1, 1, 1) * v).abs() + _nchw(r).abs()), mag_dz=to_grid((a.view(1, -1, 1, 1) * gd).abs() + gd.abs()),
               mag_dres=_nhwc(gd.abs() + (_nchw(old).abs() if accumulate else 0.0)))
    return {k: t.numpy() for k, t in out.items()}


def kernel_terms_f32(inp, form):
    """The da / db terms as the kernel forms them, every operation in float32: v = z + bias, g * v where v <= 0, and dz = v > 0 ? g : a * g."""
    s, shift, Hg, Wg, C = inp["s"], inp["shift"], inp["Hg"], inp["Wg"], inp["C"]
    f = lambda t: t.to(torch.float32)
    if form == "plain":
        v = f(_nchw(inp["z"]))
    else:
        v = f(d2s_shift(_nchw(inp["grid"]), C, s, shift, inp["Hy"], inp["Wy"])) + torch.from_numpy(inp["bias"]).view(1, -1, 1, 1)
    gd, a = f(_nchw(inp["dy"])), torch.from_numpy(inp["slope"]).view(1, -1, 1, 1)
    ta = torch.where(v > 0, torch.zeros_like(v), gd * v)
    tb = torch.where(v > 0, gd, a * gd)
    to_grid = (lambda t: _nhwc(t)) if form == "plain" else (lambda t: _nhwc(s2d_shift(t, s, shift, Hg, Wg)))
    return to_grid(ta).reshape(-1, C).numpy(), to_grid(tb).reshape(-1, C).numpy()


def elem_excess(got, want, mag, dtype, nops):
    """Largest |got - want| / bound over the elements, bound = nops * 2^-24 * mag (nops float32 operations, each within 2^-24 of the
    magnitudes it combines; doubled where a fused multiply-add may replace two roundings by one) + half an ulp of the storage type
    (+ 2^-25, float16's subnormal spacing).  <= 1 passes."""
    f32 = nops * 2.0 ** -24 * np.asarray(mag, dtype=np.float64)
    bound = f32 + STORE_EPS[dtype] * (np.abs(want) + f32) + (2.0 ** -25 if dtype == "fp16" else 0.0)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


def vec_of(dtype):
    return 4 if dtype == "fp32" else 8
