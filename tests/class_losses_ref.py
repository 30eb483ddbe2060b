"""The five computations of csrc/class_losses.hip in numpy, for the tests of FLoss, CELoss, ConLoss and CrossLoss (our own restatement):

    focal   o = clamp(x, lo, hi), lo = f32(1e-6), hi = f32(1 - 1e-6)
            binary (shape[1] == 1):  l = -0.9 (1-o)^g t log o - 0.1 o^g (1-t) log(1-o)        otherwise:  l = -(1-o)^g t log o
            loss = mean l (or sum);  dx = gout dl/do (/ n) where lo <= x <= hi, 0 outside
    bce     l = -(t max(log o, -100) + (1-t) max(log(1-o), -100));  loss = mean l;  dx = gout (o - t) / max(o (1-o), 1e-12) / n
    nll     [N, C, S]: k = first maximum of t[n, :, s];  loss = mean over N S of -log x[n, k, s];  dx = -gout / (x[n,k,s] N S) at k, else 0
    range   [nb, M]: r = max_b - min_b;  loss = mean_m r^2;  dx = +2 r gout / M at the first maximum, -2 r gout / M at the first minimum
    cross   [nb, S]: loss = mean |x[b] - t[b+1]| over (nb-1) S;  dx[b] = sign(.) gout / ((nb-1) S), zeros for the last sample

Every function runs in ``dt`` = float64 (the reference: true powers, numpy's sums) or float32 written in the kernels' order of operations:
powers by repeated multiplication (integer gamma) or exp(gamma log b), b^(gamma-1) = b^gamma / b, the upstream factor
gout * (1 / (float)n), and the kernels' two-stage summation emulated lane by lane (``_reduce32``).  ``mutate`` names one deliberate
mistake (MUTATIONS) for the teeth test.  In float64 the functions also return N per quantity.

Tolerances.  A quantity with float64 value v is held to  K * 2^-24 * N,  N = the sum of the absolute values of the quantity's own terms
(DESIGN 3.7): for a loss the sum of |term| times the mean's factor, for a gradient element the absolute values of the summands of
dl/do times |gout| / n.  An element whose N is 0 (outside the clamp, a channel that is not the arg-max, a sample that is no extreme,
CrossLoss's last sample, equal operands of the L1) must be exactly 0.  K is not chosen: ``measure_k`` gives, per quantity, the largest
error of the float32 restatement in those units over the cases of the GPU grid, and the kernel gets 4 x that (the project's margin, which
here also covers the device's logf / expf against numpy's).  K_RECORDED is 4 x the measured figure rounded up to the next integer."""
import math

import numpy as np

LO, HI = np.float32(1e-6), np.float32(1.0 - 1e-6)        # torch.clamp's float32 bounds
FWD_BLOCKS, FWD_THREADS, BWD_BLOCKS, BWD_THREADS = 1024, 512, 2048, 256       # csrc/class_losses.hip: CL_FWD_*, CL_BWD_*
GRID = BWD_BLOCKS * BWD_THREADS * 4                       # elements one pass of the backward grid covers, and of the forward grid
assert GRID == FWD_BLOCKS * FWD_THREADS * 4
MUTATIONS = ("alpha_swapped", "no_one_minus_t", "grad_exponent", "no_clamp_mask", "clamp_exclusive", "nll_div_ncs", "argmax_last",
             "nll_grad_all_channels", "range_last_tie", "range_div_nbm", "range_no_min", "cross_same_sample", "cross_last_nonzero",
             "drop_tail")
QUANTITIES = ("focal_loss", "focal_grad", "bce_loss", "bce_grad", "nll_loss", "nll_grad", "range_loss", "range_grad", "cross_loss",
              "cross_grad")
# 4 x the float32 restatement's largest error over the grid below, in units of 2^-24 N, rounded up to the next integer.
# Measured (measure_k, numpy on the CPU): focal_loss 1.16, focal_grad 8.16, bce_loss 0.51, bce_grad 2.92, nll_loss 1.40, nll_grad 2.14,
# range_loss 1.19, range_grad 1.92, cross_loss 0.82, cross_grad 1.19.  The largest figure, focal_grad, is the general-gamma path:
# exp(gamma log b) carries the rounding of a product of magnitude up to 7 into the exponent.
K_RECORDED = {"focal_loss": 5.0, "focal_grad": 33.0, "bce_loss": 3.0, "bce_grad": 12.0, "nll_loss": 6.0, "nll_grad": 9.0,
              "range_loss": 5.0, "range_grad": 8.0, "cross_loss": 4.0, "cross_grad": 5.0}

EDGES_X = np.array([0.0, 1e-7, LO, 0.5, HI, 1.0], np.float32).reshape(6, 1)       # with target 1: the clamp bounds, both sides


# ------------------------------------------------------------------------------------------------ float32 summation of the kernels
def _tree(v):
    """Lane 0 of the wave shuffle reduction (v += shfl_down(v, o), o = 32 .. 1) over the last axis of 64."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _block(acc):
    """[blocks, threads] per-thread sums -> [blocks] partials: the wave sums added as (r0 + r1) + (r2 + r3) (four waves) or
    ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) (eight)."""
    r = _tree(acc.reshape(acc.shape[0], -1, 64))
    while r.shape[1] > 1:
        r = r[:, 0::2] + r[:, 1::2]
    return r[:, 0]


def _strided(acc, items, T):
    """acc[tau] += items[tau], items[tau + T], ... one after the other."""
    it = -(-len(items) // T)
    pad = np.zeros(it * T, np.float32)
    pad[:len(items)] = items
    for row in pad.reshape(it, T):
        acc = acc + row
    return acc


def _reduce32(terms, vec, scale):
    """The kernels' sum of ``terms`` (float32, element order) times ``scale``: threads take groups of four (``vec``) or single elements
    grid-stride, then the elements a group of four does not cover; wave shuffles, block partials, one block over the partials."""
    terms = np.asarray(terms, np.float32).ravel()
    n = len(terms)
    nv = n // 4 if vec else 0
    ns = n - 4 * nv
    blocks = min(max(-(-(nv + ns) // FWD_THREADS), 1), FWD_BLOCKS)
    T = blocks * FWD_THREADS
    acc = np.zeros(T, np.float32)
    if nv:
        it = -(-nv // T)
        pad = np.zeros((it * T, 4), np.float32)
        pad[:nv] = terms[:4 * nv].reshape(nv, 4)
        for grp in pad.reshape(it, T, 4):
            for j in range(4):
                acc = acc + grp[:, j]
    acc = _strided(acc, terms[4 * nv:], T)
    part = _block(acc.reshape(blocks, FWD_THREADS))
    fin = _block(_strided(np.zeros(256, np.float32), part, 256).reshape(1, 256))[0]
    return np.float32(fin * np.float32(scale))


def _sum(terms, vec, scale, dt):
    return float(terms.sum() * scale) if dt == np.float64 else _reduce32(terms, vec, scale)


def _upstream(gout, n, dt):
    """gout * 1 / n as the kernels form it: the host's 1.f / (float)n, one product on the device."""
    if dt == np.float64:
        return gout / n
    return np.float32(gout) * (np.float32(1) / np.float32(n))


def _powers(b, logb, gamma, dt):
    """b^gamma and b^(gamma-1)."""
    if dt == np.float64:
        return b ** gamma, b ** (gamma - 1.0)
    if 0 <= gamma <= 8 and gamma == int(gamma):
        pm1 = np.ones_like(b)
        for _ in range(1, int(gamma)):
            pm1 = pm1 * b
        return (pm1 * b if gamma > 0 else np.ones_like(b)), pm1
    p = np.exp(np.float32(gamma) * logb)
    return p, p / b


# ------------------------------------------------------------------------------------------------ the five computations
def focal(x, t, gamma=2.0, mean=True, gout=1.0, dt=np.float64, mutate=None):
    x, t = np.asarray(x, dt), np.asarray(t, dt)
    binary, n = x.shape[1] == 1, x.size
    lo, hi, one = dt(LO), dt(HI), dt(1)
    o = np.minimum(np.maximum(x, lo), hi)
    om = one - o
    lg, l1 = np.log(o), np.log(om)
    p1, p1m = _powers(om, l1, gamma, dt)
    p0, p0m = _powers(o, lg, gamma, dt)
    if mutate == "grad_exponent":
        p1m, p0m = p1, p0
    a1, a0 = (dt(0.1), dt(0.9)) if mutate == "alpha_swapped" else (dt(0.9), dt(0.1))
    w0 = np.ones_like(t) if mutate == "no_one_minus_t" else one - t
    gm = dt(gamma)
    if binary:
        A, B = (-a1 * p1) * (t * lg), (a0 * p0) * (w0 * l1)
        d1, d0 = (a1 * t), (a0 * w0)
        e = [d1 * (gm * p1m * lg), d1 * (p1 / o), d0 * (p0 / om), d0 * (gm * p0m * l1)]
        d = d1 * (gm * p1m * lg - p1 / o) + d0 * (p0 / om - gm * p0m * l1)
    else:
        A, B = -p1 * (t * lg), np.zeros_like(t)
        e = [t * (gm * p1m * lg), t * (p1 / o)]
        d = t * (gm * p1m * lg - p1 / o)
    ell = A - B
    mask = (x >= lo) & (x <= hi)
    if mutate == "clamp_exclusive":
        mask = (x > lo) & (x < hi)
    if mutate == "no_clamp_mask":
        mask = np.ones_like(mask)
    scale = 1.0 / n if mean else 1.0
    g = _upstream(gout, n, dt) if mean else dt(gout)
    grad = np.where(mask, d * g, dt(0)).astype(dt)
    if mutate == "drop_tail":
        ell.flat[-1] = 0
        grad.flat[-1] = 0
    out = {"loss": _sum(ell, True, scale, dt), "grad": grad}
    if dt == np.float64:
        out["Nloss"] = float((np.abs(A) + np.abs(B)).sum() * scale)
        out["Ngrad"] = np.where(mask, sum(np.abs(v) for v in e) * abs(g), 0.0)
    return out


def bce(x, t, gout=1.0, dt=np.float64, mutate=None):
    o, t = np.asarray(x, dt), np.asarray(t, dt)
    n, one = o.size, dt(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = np.maximum(np.log(o), dt(-100)), np.maximum(np.log(one - o), dt(-100))
    A, B = t * a, (one - t) * b
    ell = -(A + B)
    den = np.maximum((one - o) * o, dt(1e-12))
    g = _upstream(gout, n, dt)
    grad = ((o - t) / den * g).astype(dt)
    if mutate == "drop_tail":
        ell.flat[-1] = 0
        grad.flat[-1] = 0
    out = {"loss": _sum(ell, True, 1.0 / n, dt), "grad": grad}
    if dt == np.float64:
        out["Nloss"] = float((np.abs(A) + np.abs(B)).sum() / n)
        out["Ngrad"] = np.where(o == t, 0.0, (np.abs(o) + np.abs(t)) / den * abs(g))
    return out


def nll(x, t, gout=1.0, dt=np.float64, mutate=None):
    x, t = np.asarray(x, dt), np.asarray(t, dt)
    Nn, C = x.shape[0], x.shape[1]
    x, t = x.reshape(Nn, C, -1), t.reshape(Nn, C, -1)
    S = x.shape[2]
    k = (C - 1 - np.argmax(t[:, ::-1], axis=1)) if mutate == "argmax_last" else np.argmax(t, axis=1)
    ok = np.take_along_axis(x, k[:, None, :], 1)[:, 0, :]
    ell = -np.log(ok)
    count = Nn * S * (C if mutate == "nll_div_ncs" else 1)
    gk = (-_upstream(gout, count, dt) / ok).astype(dt)
    grad = np.zeros_like(x)
    if mutate == "nll_grad_all_channels":
        grad[:] = gk[:, None, :]
    else:
        np.put_along_axis(grad, k[:, None, :], gk[:, None, :], 1)
    out = {"loss": _sum(ell, S % 4 == 0, 1.0 / count, dt), "grad": grad}
    if dt == np.float64:
        out["Nloss"] = float(np.abs(ell).sum() / count)
        out["Ngrad"] = np.abs(grad)
    return out


def batch_range(f, gout=1.0, dt=np.float64, mutate=None):
    f = np.asarray(f, dt)
    nb = f.shape[0]
    f = f.reshape(nb, -1)
    M = f.shape[1]
    r = f.max(axis=0) - f.min(axis=0)
    if mutate == "range_last_tie":
        imx, imn = nb - 1 - np.argmax(f[::-1], axis=0), nb - 1 - np.argmin(f[::-1], axis=0)
    else:
        imx, imn = np.argmax(f, axis=0), np.argmin(f, axis=0)
    count = M * (nb if mutate == "range_div_nbm" else 1)
    c = ((dt(2) * r) * _upstream(gout, count, dt)).astype(dt)
    cols = np.arange(M)
    grad, Ng = np.zeros_like(f), np.zeros(f.shape)
    grad[imx, cols] += c
    Ng[imx, cols] += np.abs(c)
    if mutate != "range_no_min":
        grad[imn, cols] += -c
        Ng[imn, cols] += np.abs(c)
    out = {"loss": _sum(r * r, M % 4 == 0, 1.0 / count, dt), "grad": grad}
    if dt == np.float64:
        out["Nloss"] = float((r * r).sum() / count)
        out["Ngrad"] = Ng
    return out


def cross(x, t, gout=1.0, dt=np.float64, mutate=None):
    x, t = np.asarray(x, dt), np.asarray(t, dt)
    nb = x.shape[0]
    x, t = x.reshape(nb, -1), t.reshape(nb, -1)
    S = x.shape[1]
    n = (nb - 1) * S
    d = x[:-1] - (t[:-1] if mutate == "cross_same_sample" else t[1:])
    ell = np.abs(d)
    g = _upstream(gout, n, dt)
    grad = np.zeros_like(x)
    grad[:-1] = np.sign(d) * g
    if mutate == "cross_last_nonzero":
        grad[-1] = np.sign(x[-1] - t[-1]) * g
    if mutate == "drop_tail":
        ell[-1, -1] = 0
        grad[-2, -1] = 0
    out = {"loss": _sum(ell, S % 4 == 0, 1.0 / n, dt), "grad": grad}
    if dt == np.float64:
        out["Nloss"] = float(ell.sum() / n)
        out["Ngrad"] = np.abs(grad)
    return out


# ------------------------------------------------------------------------------------------------ comparison
def tolerance(q, N, K=None):
    return (K or K_RECORDED)[q] * 2.0 ** -24 * np.asarray(N, np.float64)


def units(got, ref, N):
    """Largest error in units of 2^-24 N (an element with N = 0 must be exact: any error there is infinite)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(err == 0, 0.0, err / (2.0 ** -24 * np.asarray(N, np.float64)))
    return float(np.max(np.nan_to_num(u, nan=np.inf)))


def worst(q, got, ref, N, K=None):
    """Largest |got - ref| / tolerance over the elements (<= 1: within the bound)."""
    return units(got, ref, N) / (K or K_RECORDED)[q]


# ------------------------------------------------------------------------------------------------ the GPU grid
FLAT_SHAPES = ((1, 1), (3, 1, 5, 7), (2, 1, 33, 65), (1, 1, GRID + 5))      # n = 1; one block, n % 4 != 0; blocks and a tail; past one grid pass
FOCAL_CASES = tuple((s, 2.0, True) for s in FLAT_SHAPES) + (
    ((3, 1, 5, 7), 1.5, False), ((2, 1, 33, 65), 3.0, True), ((2, 1, 33, 65), 1.5, True),
    ((3, 4, 5, 7), 2.0, True), ((2, 5, 33, 65), 2.0, True), ((3, 4, 5, 7), 1.5, False), ((2, 5, 33, 65), 3.0, True))
BCE_CASES = FLAT_SHAPES
# (N, C, S, where the maximum lies): S = 4291 is odd (rows misaligned: 4-byte path), S = 1028 takes the 16-byte path
NLL_CASES = ((1, 2, 1, "any"), (3, 4, 35, "any"), (2, 5, 4291, "any"), (2, 3, 1028, "any"), (3, 4, 35, "first"), (3, 4, 35, "last"))
RANGE_CASES = ((1, 7), (2, 105), (5, 4291), (16, 33), (3, 1028))
CROSS_CASES = ((2, 3, 5, 7), (3, 1, 1, 1), (4, 2, 33, 65), (3, 4, 1, 257))     # S = 105 (target + S misaligned), 1, 4290, 1028 (16-byte path)


def _f16(a):
    return np.asarray(a, np.float16).astype(np.float32)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _levels(rng, shape, axis):
    """Distinct levels 0 .. shape[axis]-1 in an independent random order along ``axis`` at every other position."""
    idx = np.broadcast_to(np.arange(shape[axis]).reshape([-1 if a == axis else 1 for a in range(len(shape))]), shape)
    return rng.permuted(idx, axis=axis).astype(np.float32)


def flat_inputs(shape, seed=0):
    """x in [0.02, 0.98]; t: 0 / 1 for one channel, a per-position permutation of the levels c / 8 otherwise.  float16-representable."""
    rng = _rng(1, seed, *shape)
    x = _f16(rng.uniform(0.02, 0.98, shape))
    t = rng.integers(0, 2, shape).astype(np.float32) if shape[1] == 1 else _levels(rng, shape, 1) / 8
    return x, t


def nll_inputs(case, seed=0):
    Nn, C, S, where = case
    rng = _rng(2, seed, Nn, C, S, len(where))
    x = _f16(rng.uniform(0.02, 0.98, (Nn, C, S)))
    t = _levels(rng, (Nn, C, S), 1)
    if where != "any":
        k, top = (0 if where == "first" else C - 1), np.argmax(t, axis=1)[:, None, :]
        cur = t[:, k:k + 1, :].copy()
        np.put_along_axis(t, top, cur, 1)
        t[:, k, :] = C - 1
    return x, t / 8


def range_inputs(case, seed=0):
    """Every column: nb distinct levels out of 0 .. 31 in random order, plus a column base, over 32: maximum and minimum are unique."""
    nb, M = case
    rng = _rng(3, seed, nb, M)
    return (_levels(rng, (32, M), 0)[:nb] + rng.integers(0, 32, (1, M))) / 32


def cross_inputs(shape, seed=0):
    rng = _rng(4, seed, *shape)
    x, t = _f16(rng.uniform(0, 1, shape)), _f16(rng.uniform(0, 1, shape))
    t.reshape(shape[0], -1)[1:].flat[::7] = x.reshape(shape[0], -1)[:-1].flat[::7]        # equal operands: sign(0) = 0
    return x, t


def ties_inputs():
    """ConLoss columns with a repeated maximum and a repeated minimum (and one constant column)."""
    return np.array([[1, 0, 2, 5, 3], [3, 0, 2, 5, 1], [3, 4, 0, 5, 1], [1, 4, 0, 5, 3]], np.float32) / 8


def grid():
    """(quantity prefix, function, inputs, keyword arguments) of every case of the GPU grid."""
    for shape, gamma, mean in FOCAL_CASES:
        yield "focal", focal, flat_inputs(shape), {"gamma": gamma, "mean": mean}
    for shape in BCE_CASES:
        yield "bce", bce, flat_inputs(shape), {}
    for case in NLL_CASES:
        yield "nll", nll, nll_inputs(case), {}
    for case in RANGE_CASES:
        yield "range", batch_range, (range_inputs(case),), {}
    for shape in CROSS_CASES:
        yield "cross", cross, cross_inputs(shape), {}


def measure_k(cases=None):
    """Per quantity: the float32 restatement's largest error over the grid, in units of 2^-24 N."""
    k = {q: 0.0 for q in QUANTITIES}
    for name, fn, inp, kw in (cases or grid()):
        for gout in (1.0, 3.0):
            ref = fn(*inp, gout=gout, **kw)
            got = fn(*inp, gout=gout, dt=np.float32, **kw)
            k[name + "_loss"] = max(k[name + "_loss"], units(got["loss"], ref["loss"], ref["Nloss"]))
            k[name + "_grad"] = max(k[name + "_grad"], units(got["grad"], ref["grad"], ref["Ngrad"]))
    return k


def k_from(measured):
    return {q: float(max(math.ceil(4 * v), 1)) for q, v in measured.items()}
