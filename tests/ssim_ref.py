"""Float64 CPU references of the kernels of csrc/metrics.hip, their float32 restatements, one deliberate mistake each, and the case
tables of tests/test_gpu_metrics_kernels.py and tests/test_metrics_kernels_teeth.py.  No GPU import.

The DSSIM gradient is bounded per pixel (the comment above dssim_bwd_k gives the formula):

  |dx(q) - dx64(q)| <= K * 2^-24 * N_x(q)
  N_x(q) = |g| / (2n) * [ (w (*) A^_x)(q) + 2 |x(q)| (w (*) |b|)(q) + |y(q)| (w (*) |c|)(q) ]
  A^_x   = 2 (|mu_y B1 D| + |mu_x S/A2| + |mu_y A1 D| + |mu_x S/B2|)

(*) the transposed 11x11 correlation over the valid positions, n = B C (H-10)(W-10) times F: the gradient's own expression with every
term replaced by its absolute value.  A corner pixel is covered by one position with weight w[0]^2, and N(q) is as small there as the
gradient is, so the bound is as tight at the corner as in the middle; no measure here is normalised by a tensor's maximum or norm.

All inputs are float16-representable values stored as float32, from fixed seeds.

`fault`: one deliberate mistake each, on the float64 loss and gradient (FAULTS; tests/test_metrics_kernels_teeth.py shows that
`within` at K notices every one):
  drop_corner_position    window position (0, 0) left out of the sum
  drop_last_position_row  the last row of window positions left out
  halo_9                  positions 10 pixels away from q not accumulated into the gradient of q (gradient only)
  n_full                  normalised by H W instead of (H-10)(W-10)
  range_from_truth        the dynamic range taken from the target
  x_for_y                 the per-pixel combination reads y(q) where x(q) is meant (gradient only)
  plane_swap              planes (b, c) and (b, c+1) exchanged in the output (gradient only; needs B C even)
  shift_window            the window read one pixel to the right (zeros behind the last column)
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import losses3d_ref as L3

U32 = 2.0 ** -24                # unit round-off of f32
FAULTS = ("drop_corner_position", "drop_last_position_row", "halo_9", "n_full", "range_from_truth", "x_for_y", "plane_swap", "shift_window")
GOUT = 3.0                      # the upstream scalar of every backward case

# ------------------------------------------------------------------------------------------------ recorded CPU measurements
# `python tests/ssim_ref.py` prints every figure below from the tables of this file; tests/test_metrics_kernels_teeth.py asserts that
# each constant is the stated multiple of what the restatement gives today.
#
# K = 4 x the largest err / (2^-24 N) of restated32 against grad64 over BWD_CASES (dx and dt).  The margin of 4 is over the reference:
# the kernel forms each window sum in two separable passes and multiplies by reciprocals where the restatement runs one 121-tap
# correlation and divides -- a few more roundings per term on the same conditioning.  Per case (dx, dt):
RESTATED_RATIO = {
    "single": (1.93, 3.00), "tile2": (10.42, 10.98), "ragged2c": (5.76, 5.15), "strip_row": (10.74, 12.29), "strip_col": (6.20, 7.96),
    "frames": (8.30, 9.13), "signed": (11.71, 5.32), "smooth": (48.08, 48.74), "near": (7.29, 7.19),
}
K = 4 * max(max(v) for v in RESTATED_RATIO.values())        # 194.96
# ("truth_range", the case beyond that table, measures 3.67, 6.08.)
# tol_f = 8 x the worst |restated32 loss - float64 loss| over FWD_SHAPES x probes (floor 2^-24); tol_m likewise for the two outputs of
# the metric over METRIC_SHAPES (floor 2^-22).  The margin is wider than K's because ssim_tile_k sums 256 map values near 1 in f32 per
# tile before the fold, which the restatement does not; the metric's fold is f32, the loss's f64.  Both worst cases are the 11x11 image:
# one window position, so nothing averages the position's own f32 error (the variances are differences of window sums near 0.3).
RESTATED_LOSS_ERR = 5.62e-7
RESTATED_METRIC_ERR = 2.56e-6
TOL_F = max(8 * RESTATED_LOSS_ERR, 2.0 ** -24)              # 4.5e-6
TOL_M = max(8 * RESTATED_METRIC_ERR, 2.0 ** -22)            # 2.05e-5
# AE: 4 x the worst |numpy-f32 restatement - float64| (degrees) per case family.  "same" (pred = truth) is the ill-conditioned one:
# the quotient is 1 - 1e-6 / |p|^2, a few f32 steps below 1, and acos turns a step of 6e-8 there into 1e-3 degrees.
RESTATED_AE_ERR = {"exact": 4.98e-4, "random": 2.62e-4, "same": 7.35e-3}
TOL_AE = {k: 4 * v for k, v in RESTATED_AE_ERR.items()}


def q16(v):
    """float16-representable values stored as float32"""
    return v.half().float()


def window64():
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], dtype=torch.float64)
    return g / g.sum()


# ------------------------------------------------------------------------------------------------ float64 terms, loss, gradient
def _corr(z, win2d):
    ch = z.shape[1]
    return F.conv2d(z, win2d.expand(ch, 1, 11, 11).contiguous(), groups=ch)


def _corr_t(m, win2d):
    """the transposed ("full") correlation: position map [B,C,OH,OW] -> pixels [B,C,OH+10,OW+10]"""
    ch = m.shape[1]
    return F.conv_transpose2d(m, win2d.expand(ch, 1, 11, 11).contiguous(), groups=ch)


def dssim_terms(x, t, L=None, fault=None):
    """The quantities of the comment above dssim_bwd_k for float64 [B,C,H,W] tensors: window means, A1, A2, B1, B2, D, S, the position
    maps b = -S/B2, c = 2 A1 D, a_x, a_y, and the loss (losses3d_ref.dssim2d and its range rule; with a fault, the mean of the faulty map)."""
    rng_of = t if fault == "range_from_truth" else x
    L = L3._range(rng_of.detach()) if L is None else L
    g = window64()
    win = torch.outer(g, g)
    xs, ts = x, t
    if fault == "shift_window":
        xs, ts = F.pad(x[..., 1:], (0, 1)), F.pad(t[..., 1:], (0, 1))
    mx, my = _corr(xs, win), _corr(ts, win)
    exx, eyy, exy = _corr(xs * xs, win), _corr(ts * ts, win), _corr(xs * ts, win)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    A1, A2 = 2 * mx * my + C1, mx * mx + my * my + C1
    B1, B2 = 2 * (exy - mx * my) + C2, (exx - mx * mx) + (eyy - my * my) + C2
    D = 1 / (A2 * B2)
    S = A1 * B1 * D
    keep = torch.ones_like(S)
    if fault == "drop_corner_position":
        keep[..., 0, 0] = 0
    if fault == "drop_last_position_row":
        keep[..., -1, :] = 0
    B, C, H, W = x.shape
    n = B * C * (H * W if fault == "n_full" else (H - 10) * (W - 10))
    if fault in (None, "halo_9", "x_for_y", "plane_swap"):
        loss = L3.dssim2d(x, t, L)
    else:
        loss = (1 - (S * keep).sum() / n) / 2
    a_x = 2 * (my * B1 * D - mx * S / A2 - my * A1 * D + mx * S / B2)
    a_y = 2 * (mx * B1 * D - my * S / A2 - mx * A1 * D + my * S / B2)
    return dict(mx=mx, my=my, A1=A1, A2=A2, B1=B1, B2=B2, D=D, S=S, b=-S / B2 * keep, c=2 * A1 * D * keep, a_x=a_x * keep, a_y=a_y * keep,
                loss=loss, n=n, L=L, win=win)


def _frames(z):
    return [z[:, :, f] for f in range(z.shape[2])]


def loss64(x, t, fault=None):
    """the mean over frames of the per-frame DSSIM of [B,C,F,H,W] tensors in float64 (a torch scalar; differentiable)"""
    x, t = torch.as_tensor(x).double(), torch.as_tensor(t).double()
    if fault is None:
        return L3.dssim_3d(x, t)
    return sum(dssim_terms(a, b, fault=fault)["loss"] for a, b in zip(_frames(x), _frames(t))) / x.shape[2]


def _grad_formula(x, t, gout, fault=None, absolute=False):
    """dx, dt of [B,C,F,H,W] float64 tensors by the formula of dssim_bwd_k; absolute = True: every term replaced by its absolute value
    (grad_scale).  The faults of the backward pass alone live here."""
    Fr = x.shape[2]
    dx, dt = torch.zeros_like(x), torch.zeros_like(t)
    for f in range(Fr):
        a, b = x[:, :, f], t[:, :, f]
        T = dssim_terms(a, b, fault=fault)
        win = T["win"].clone()
        if fault == "halo_9":
            win[10, :] = 0      # conv_transpose2d adds position p into pixel p + k with weight win[k]: k = 10 is 10 pixels away
            win[:, 10] = 0
        if absolute:
            mx, my, A1, A2, B1, B2, D, S = (T[k].abs() for k in ("mx", "my", "A1", "A2", "B1", "B2", "D", "S"))
            ax = 2 * (my * B1 * D + mx * S / A2 + my * A1 * D + mx * S / B2)
            ay = 2 * (mx * B1 * D + my * S / A2 + mx * A1 * D + my * S / B2)
            mb, mc, xa, ya, sc = T["b"].abs(), T["c"].abs(), a.abs(), b.abs(), abs(gout) / (2 * T["n"] * Fr)
        else:
            ax, ay, mb, mc, xa, ya, sc = T["a_x"], T["a_y"], T["b"], T["c"], a, b, -gout / (2 * T["n"] * Fr)
        wb, wc = _corr_t(mb, win), _corr_t(mc, win)
        xq = ya if fault == "x_for_y" else xa
        dx[:, :, f] = sc * (_corr_t(ax, win) + 2 * xq * wb + ya * wc)
        dt[:, :, f] = sc * (_corr_t(ay, win) + 2 * ya * wb + xa * wc)
    return dx, dt


def _swap_planes(d):
    B, C = d.shape[:2]
    v = d.reshape(B * C // 2, 2, *d.shape[2:])
    return v.flip(1).reshape(d.shape).clone()


def grad64(x, t, gout, fault=None):
    """dx, dt of gout * loss64 by float64 autograd: a loop over frames, each with its own range, and a mean over frames (as
    losses3d_ref.dssim_3d).  halo_9 and x_for_y are mistakes of the backward pass alone and go through the formula."""
    x, t = torch.as_tensor(x).detach().double(), torch.as_tensor(t).detach().double()
    if fault in ("halo_9", "x_for_y"):
        return _grad_formula(x, t, gout, fault)
    x, t = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
    (gout * loss64(x, t, None if fault == "plane_swap" else fault)).backward()
    dx, dt = x.grad.detach(), t.grad.detach()
    if fault == "plane_swap":
        dx, dt = _swap_planes(dx), _swap_planes(dt)
    return dx, dt


def grad_formula64(x, t, gout):
    """the fault-free formula (the teeth file checks it against autograd: it is what grad_scale takes absolute values of)"""
    return _grad_formula(torch.as_tensor(x).double(), torch.as_tensor(t).double(), gout)


def grad_scale(x, t, gout):
    """N_x, N_t: the per-pixel scale of the bound (module docstring)"""
    return _grad_formula(torch.as_tensor(x).double(), torch.as_tensor(t).double(), gout, absolute=True)


def within(got, ref, N, K, what):
    """|got - ref| <= K 2^-24 N for every element, decided with .all() so that a NaN fails; prints the largest err / (2^-24 N)"""
    err = (torch.as_tensor(got).double().cpu() - ref).abs()
    ok = bool((err <= K * U32 * N).all())
    ratio = torch.where(N > 0, err / (U32 * N).clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    at = np.unravel_index(int(ratio.argmax()), tuple(ratio.shape))
    print(f"[ssim] {what}: max err / (2^-24 N) {float(ratio.max()):.2f} at {tuple(int(i) for i in at)} of {tuple(ratio.shape)} (K {K})")
    return ok


def max_ratio(got, ref, N):
    err = (torch.as_tensor(got).double() - ref).abs()
    return float((err / (U32 * N)).max())


# ------------------------------------------------------------------------------------------------ float32 restatements
def _ssim_maps32(x, t, L):
    """SSIM and contrast maps of float32 [B,C,H,W] tensors in float32 torch: one 121-tap correlation, a division"""
    g = window64()
    ch = x.shape[1]
    win = torch.outer(g, g).float().expand(ch, 1, 11, 11).contiguous()
    conv = lambda z: F.conv2d(z, win, groups=ch)
    m1, m2 = conv(x), conv(t)
    s1, s2, s12 = conv(x * x) - m1 * m1, conv(t * t) - m2 * m2, conv(x * t) - m1 * m2
    C1, C2 = np.float32(0.01 * L) ** 2, np.float32(0.03 * L) ** 2
    v1, v2 = 2 * s12 + float(C2), s1 + s2 + float(C2)
    return ((2 * m1 * m2 + float(C1)) * v1) / ((m1 * m1 + m2 * m2 + float(C1)) * v2), v1 / v2


def restated32(x, t, gout):
    """-> (loss, dx, dt) of the same loss in float32 torch on the CPU.  It exists only to measure what float32 arithmetic alone costs
    against float64."""
    x, t = torch.as_tensor(x).detach().float().clone().requires_grad_(True), torch.as_tensor(t).detach().float().clone().requires_grad_(True)
    Fr = x.shape[2]
    loss = sum((1 - _ssim_maps32(x[:, :, f], t[:, :, f], L3._range(x[:, :, f].detach()))[0].mean()) / 2 for f in range(Fr)) / Fr
    (np.float32(gout) * loss).backward()
    return float(loss.detach()), x.grad.detach(), t.grad.detach()


def metric64(x, t):
    """[B, 2] float64: per image the mean of the SSIM map and of the contrast map, range from the whole prediction"""
    x, t = torch.as_tensor(x).double(), torch.as_tensor(t).double()
    T = dssim_terms(x, t)
    return torch.stack([T["S"].mean((1, 2, 3)), (T["B1"] / T["B2"]).mean((1, 2, 3))], 1)


def metric32(x, t):
    s, cs = _ssim_maps32(torch.as_tensor(x).float(), torch.as_tensor(t).float(), L3._range(torch.as_tensor(x)))
    return torch.stack([s.mean((1, 2, 3)), cs.mean((1, 2, 3))], 1)


# ------------------------------------------------------------------------------------------------ backward cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit_pair(shape, g, scale=1.0):
    """target uniform in [0, scale), prediction = target + 0.1 scale noise, clamped"""
    t = torch.rand(shape, generator=g) * scale
    x = (t + 0.1 * scale * torch.randn(shape, generator=g)).clamp(0, scale)
    return x, t


def _make_bwd(name):
    shape, kind = BWD_CASES[name]
    g = _gen(1000 + sorted(BWD_CASES).index(name))
    if kind == "unit":
        x, t = _unit_pair(shape, g)
    elif kind == "frames":                          # frame 0 in [0,1], frame 1 in [0,255]
        x, t = _unit_pair(shape, g)
        x[:, :, 1] *= 255
        t[:, :, 1] *= 255
    elif kind == "signed":                          # [-1, 1]: L = 2
        x, t = _unit_pair(shape, g)
        x, t = 2 * x - 1, 2 * t - 1
    elif kind == "smooth":                          # a low-variance smooth image plus 0.02 noise: C2 dominates B2
        H, W = shape[-2:]
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        base = (0.5 + 0.2 * torch.sin(yy / 17) * torch.cos(xx / 23)).expand(shape)
        t = base + 0.02 * torch.randn(shape, generator=g)
        x = base + 0.02 * torch.randn(shape, generator=g)
    elif kind == "near":                            # x = t + 1e-3 noise on [0, 0.5): SSIM close to 1
        t = torch.rand(shape, generator=g) * 0.5
        x = t + 1e-3 * torch.randn(shape, generator=g)
    elif kind == "truth_signed":                    # prediction in [0,1] (L = 1), target in [-1,1] (L = 2 if taken from it)
        x, t = _unit_pair(shape, g)
        t = 2 * t - 1
    return q16(x).contiguous(), q16(t).contiguous()


# name -> ((B,C,F,H,W), data): the smallest shapes that reach each branch of the 32x32 output tile with its 10-pixel halo
BWD_CASES = {
    "single": ((1, 1, 1, 11, 11), "unit"),          # one position; every pixel is a border pixel
    "tile2": ((2, 1, 1, 32, 32), "unit"),           # exactly one tile, two planes
    "ragged2c": ((1, 2, 1, 33, 43), "unit"),        # a one-pixel second tile row, a ragged second column, two channels
    "strip_row": ((1, 1, 1, 11, 75), "unit"),       # one position row across three tiles
    "strip_col": ((1, 1, 1, 75, 11), "unit"),
    "frames": ((1, 1, 2, 43, 75), "frames"),        # 2x3 tiles, per-frame range and invF
    "signed": ((2, 1, 1, 21, 21), "signed"),        # L = 2
    "smooth": ((1, 1, 1, 43, 75), "smooth"),
    "near": ((1, 1, 1, 43, 43), "near"),
    # beyond the table K is measured on: the one case whose two tensors differ in range (range_from_truth needs it)
    "truth_range": ((2, 1, 1, 21, 21), "truth_signed"),
}
K_CASES = tuple(k for k in BWD_CASES if k != "truth_range")


@functools.lru_cache(maxsize=None)
def bwd_case(name):
    """One shared, read-only case: dict(x, t, dx, dt, Nx, Nt, loss) -- x, t float32 [B,C,F,H,W]; the rest float64"""
    x, t = _make_bwd(name)
    dx, dt = grad64(x, t, GOUT)
    Nx, Nt = grad_scale(x, t, GOUT)
    return dict(x=x, t=t, dx=dx, dt=dt, Nx=Nx, Nt=Nt, loss=float(loss64(x, t)))


def applicable(fault, name):
    shape, kind = BWD_CASES[name]
    if fault == "plane_swap":
        return shape[0] * shape[1] % 2 == 0
    if fault == "range_from_truth":
        return kind == "truth_signed"
    return True


# ------------------------------------------------------------------------------------------------ forward probes
FWD_SHAPES = [(1, 1, 1, 11, 11), (1, 1, 1, 27, 27), (1, 1, 1, 37, 53), (1, 1, 2, 27, 27)]      # the last: the probe in frame 1 only
METRIC_SHAPES = [(11, 11), (27, 27), (37, 53)]                                                # B = 2, C = 1, another probe per image


def probe_blocks(H, W):
    """[(name, y0, x0, size)]: blocks of 11x11 pixels (6x6 on an 11x11 image, which has one window position: an 11x11 block would be the
    whole image) at the four corners, the middle of each edge, across the 16-position tile seam (pixels 16 to 26 on each axis), inside
    the last, ragged tile of positions, and in the interior.  Blocks that coincide are listed once."""
    s = 11 if min(H, W) > 11 else 6
    my, mx = (H - s) // 2, (W - s) // 2
    out = [("corner00", 0, 0), ("corner01", 0, W - s), ("corner10", H - s, 0), ("corner11", H - s, W - s),
           ("edge_top", 0, mx), ("edge_bottom", H - s, mx), ("edge_left", my, 0), ("edge_right", my, W - s), ("interior", my, mx)]
    if min(H, W) >= 27:
        out.append(("seam", 16, 16))
        ly, lx = 16 * ((H - 11) // 16), 16 * ((W - 11) // 16)          # first position of the last tile = its first pixel
        out.append(("last_tile", min(ly + 2, H - s), min(lx + 2, W - s)))
    seen, res = set(), []
    for name, y0, x0 in out:
        if (y0, x0) not in seen:
            seen.add((y0, x0))
            res.append((name, y0, x0, s))
    return res


@functools.lru_cache(maxsize=None)
def _texture(H, W, k):
    """a random texture in [0,1] and unrelated values for the blocks, per image / frame index k"""
    g = _gen(2000 + 97 * H + W + 7919 * k)
    return q16(torch.rand(H, W, generator=g)), q16(torch.rand(H, W, generator=g))


def probe_plane(H, W, k, block):
    """-> (pred, truth) [H,W]: pred = truth except the block (None: no block)"""
    t, other = _texture(H, W, k)
    x = t.clone()
    if block is not None:
        _, y0, x0, s = block
        x[y0:y0 + s, x0:x0 + s] = other[y0:y0 + s, x0:x0 + s]
    return x, t


def fwd_probe(shape, block):
    """-> (pred, truth) [B,C,F,H,W] of one loss probe: the block in the last frame only"""
    B, C, Fr, H, W = shape
    planes = [probe_plane(H, W, f, block if f == Fr - 1 else None) for f in range(Fr)]
    x, t = torch.stack([p[0] for p in planes]), torch.stack([p[1] for p in planes])
    return x.view(1, 1, Fr, H, W).contiguous(), t.view(1, 1, Fr, H, W).contiguous()


def fwd_probes():
    return [(shape, blk) for shape in FWD_SHAPES for blk in probe_blocks(*shape[-2:])]


def metric_probe(H, W, i):
    """-> (pred, truth) [2,1,H,W]: image 0 carries block i, image 1 block i + 1 (cyclically)"""
    blocks = probe_blocks(H, W)
    planes = [probe_plane(H, W, b, blocks[(i + b) % len(blocks)]) for b in range(2)]
    return torch.stack([p[0] for p in planes]).unsqueeze(1).contiguous(), torch.stack([p[1] for p in planes]).unsqueeze(1).contiguous()


def metric_probes():
    return [(H, W, i) for H, W in METRIC_SHAPES for i in range(len(probe_blocks(H, W)))]


# ------------------------------------------------------------------------------------------------ range cases
def range_case(hw_shape, seed=3000):
    """[2,1,3,H,W] float32 in (-0.4, 100) with per-frame extremes planted at the first element, the last element, index 255, index 256
    and the last index of the last plane (where the image has them), a different place for min and max in every frame"""
    H, W = hw_shape
    hw = H * W
    x = q16(torch.rand(2, 1, 3, H, W, generator=_gen(seed + hw)) * 100 - 0.4 * torch.rand(2, 1, 3, H, W, generator=_gen(seed + hw + 1)))
    spots = [(0, 0), (0, hw - 1), (1, hw - 1), (0, min(255, hw - 1)), (0, min(256, hw - 1)), (1, 0)]      # (plane, flat index)
    for f in range(3):
        (plo, ilo), (phi, ihi) = spots[(2 * f) % len(spots)], spots[(2 * f + 1) % len(spots)]
        x[plo, 0, f].view(-1)[ilo] = -0.4375 - f / 64
        x[phi, 0, f].view(-1)[ihi] = 101.0 + f
    return x.contiguous()


def threshold_cases():
    """(name, pred, truth [1,1,1,13,13], L the float64 rule gives): the extremes exactly at and just past the rule's thresholds"""
    g = _gen(3100)
    base = q16(torch.rand(1, 1, 1, 13, 13, generator=g) * 0.8 + 0.1)
    truth = q16(torch.rand(1, 1, 1, 13, 13, generator=g) * 0.8 + 0.1)
    out = []
    for name, idx, val, L in (("max_128", 5, 128.0, 1.0), ("max_128.5", 5, 128.5, 255.0), ("min_-0.5", 160, -0.5, 1.0),
                              ("min_below_-0.5", 160, float(np.nextafter(np.float32(-0.5), np.float32(-1))), 2.0)):
        x = base.clone()
        x.view(-1)[idx] = val
        out.append((name, x, truth, L))
    return out


# ------------------------------------------------------------------------------------------------ angular error
def ae64(p, t):
    """[B] float64: mean over pixels of acos(<p,t> / (|p||t| + 1e-6)) in degrees; 1e-6 is the kernel's f32 constant"""
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    dot, n1, n2 = (p * t).sum(1), np.sqrt((p * p).sum(1)), np.sqrt((t * t).sum(1))
    return np.degrees(np.arccos(dot / (n1 * n2 + float(np.float32(1e-6))))).reshape(p.shape[0], -1).mean(1)


def ae32(p, t):
    """the same formula in numpy float32, channel sums in the kernel's order"""
    p, t = np.asarray(p, dtype=np.float32), np.asarray(t, dtype=np.float32)
    dot = np.zeros(p[:, 0].shape, np.float32); n1 = dot.copy(); n2 = dot.copy()
    for c in range(p.shape[1]):
        dot += p[:, c] * t[:, c]; n1 += p[:, c] * p[:, c]; n2 += t[:, c] * t[:, c]
    a = np.float32(57.29577951308232) * np.arccos(dot / (np.sqrt(n1) * np.sqrt(n2) + np.float32(1e-6)))
    return a.reshape(p.shape[0], -1).mean(1, dtype=np.float32)


AE_HW = [1, 255, 256 * 64 - 1, 256 * 64 + 1]
# (pred pixel, truth pixel, angle without eps): orthogonal vectors, and a zero pixel, give 0 / (. + 1e-6) = 0 -> 90 degrees exactly
AE_PAIRS = [((1, 1, 0), (1, 0, 1), 60.0), ((1, 0, 0), (0, 1, 0), 90.0), ((1, 0, 0), (-1, 0, 0), 180.0), ((0, 0, 0), (0, 1, 0), 90.0),
            ((0, 0, 0), (0, 0, 0), 90.0)]


def ae_case(family, hw, C=3):
    """-> (pred, truth) float32 numpy [2, C, 1, hw]"""
    g = np.random.default_rng(4000 + hw + 10 * C)
    if family == "exact":       # pixels drawn from AE_PAIRS, image 1 without the first pair: another mix per image
        p, t = np.zeros((2, 3, 1, hw), np.float32), np.zeros((2, 3, 1, hw), np.float32)
        for b in range(2):
            pick = g.integers(b, len(AE_PAIRS), hw)
            for i, (pp, tt, _) in enumerate(AE_PAIRS):
                p[b, :, 0, pick == i] = np.float32(pp)
                t[b, :, 0, pick == i] = np.float32(tt)
        return p, t
    p = g.random((2, C, 1, hw), dtype=np.float32).astype(np.float16).astype(np.float32)
    if family == "same":
        return p, p.copy()
    return p, g.random((2, C, 1, hw), dtype=np.float32).astype(np.float16).astype(np.float32)


def ae_cases():
    return [("exact", hw, 3) for hw in AE_HW] + [(fam, hw, C) for fam in ("random", "same") for hw in AE_HW for C in (1, 3)]


# ------------------------------------------------------------------------------------------------ the measurements behind the constants
def measure():
    """every CPU figure the constants above are multiples of"""
    ratios = {}
    for name in BWD_CASES:
        c = bwd_case(name)
        _, dx32, dt32 = restated32(c["x"], c["t"], GOUT)
        ratios[name] = (max_ratio(dx32, c["dx"], c["Nx"]), max_ratio(dt32, c["dt"], c["Nt"]))
    loss_err = max(abs(restated32(x, t, 1.0)[0] - float(loss64(x, t))) for x, t in (fwd_probe(s, b) for s, b in fwd_probes()))
    metric_err = max(float((metric32(x, t).double() - metric64(x, t)).abs().max()) for x, t in (metric_probe(*m) for m in metric_probes()))
    ae = {}
    for fam, hw, C in ae_cases():
        p, t = ae_case(fam, hw, C)
        ae[fam] = max(ae.get(fam, 0.0), float(np.abs(ae32(p, t).astype(np.float64) - ae64(p, t)).max()))
    return dict(ratios=ratios, loss_err=loss_err, metric_err=metric_err, ae=ae)


if __name__ == "__main__":
    m = measure()
    for k, v in m["ratios"].items():
        print(f"restated32 {k}: dx {v[0]:.2f} dt {v[1]:.2f}")
    print("K = 4 x", max(max(m["ratios"][k]) for k in K_CASES))
    print("loss_err", m["loss_err"], "metric_err", m["metric_err"])
    print("ae", m["ae"])
    print("smallest probe loss", min(float(loss64(*fwd_probe(s, b))) for s, b in fwd_probes()))
