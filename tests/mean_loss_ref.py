"""The flat mean losses of csrc/elementwise.hip (srcgan_loss_fwd / srcgan_loss_bwd / srcgan_psnr_from_mse; loss_fwd_k<0..4>, loss_final_k,
loss_bwd_k<0..4>, psnr_k) in numpy: case tables as plain data, our own restatement, and the comparisons the GPU tests and the teeth share.

    kind 0  e = |a - b|                                   de/da = sign(a - b), sign(0) = 0
    kind 1  e = (a - b)^2                                 de/da = 2 (a - b)
    kind 2  e = (a - label)^2                             de/da = 2 (a - label)
    kind 3  e = max(x, 0) - x t + log1p(exp(-|x|))        de/dx = 1 / (1 + exp(-x)) - t          (t = label; torch's stable BCE-with-logits)
    kind 4  e = label * a                                 de/da = label
    out = (sum e) * (float)(1.0 / n);   da[i] = de/da[i] * g,  g = gout[0] * (gscale / (float)n)   (f32 roundings: one quotient on the host,
    one product on the device; gscale = -1 gives the target's gradient of kinds 0 and 1)
    psnr = 10 log10(1 / mse)

Launch geometry (srcgan_loss_fwd).  The range splits into a scalar head up to the first 16-byte boundary (0..3 elements, only when a and b
share one 16-byte phase), nv groups of four and a scalar rest; with differing phases every element is scalar (nv = 0).  ns = n - 4 nv single
elements.  blocks = min(1024, ceil(max(nv + 1, ns) / 256)) of 256 threads; thread tau adds its groups tau, tau + T, ... (T = blocks * 256),
four terms each, then its single elements tau, tau + T, ...; 64 lanes fold by shuffles (6 additions), the four waves as (r0 + r1) +
(r2 + r3) (2), loss_final_k adds ceil(blocks / 256) partials per thread and folds 256 threads the same way (6 + 2), and the sum is multiplied
by 1 / n (1).  With both operands 16-byte aligned: nv = n4 = n / 4, blocks = min(1024, ceil((n4 + 1) / 256)), tail in block 0.

LENGTHS holds the smallest n at which each path exists: one thread alone (1..3), the first group (4), group + tail (5, 7), two groups (8),
one block short of / at / past 256 groups (1023, 1024, 1027), and around 1024 * 256 groups = 1 048 576 elements: the largest uncapped grid
(1 048 572: n4 + 1 = 262 144 = 1024 * 256), the same with a tail of three (1 048 575), the capped grid filled exactly once (1 048 576), one and
three tail elements behind it (1 048 577, 1 048 579), and two trips plus a tail of one (2 097 157 = 2 * 1 048 576 + 5: n4 = 524 289).

Exact part.  Small-integer operands: every term and every partial sum is an integer below 2^24, so every summation order gives the same
f32 bits and the expected value is f32(S) * f32(1.0 / n), one rounding.  Backward of kinds 0 and 4 is sign * g and label * g with
label = +-1: exact products of the one f32 number g.

Float64 part.  Random reals, label 0.9, logits of scale 6 plus planted logits of +-100 and +-90 (exp(100) overflows f32: only the stable
form survives them).  Bounds:
    value             |out - ref64| <= (D + 4) * 2^-24 * mean64|e|,  D = the longest chain of additions (``geometry``)
    kinds 1, 2 grad   5 * 2^-24 * |ref64| per element: the rounded difference, the product, the two roundings of g
    kind 3            K * 2^-24 * N, N = (sigma64(x) + |t|) |g| per gradient element, N = mean(|max(x,0)| + |x t| + log1p(exp(-|x|))) for the
                      value.  K comes from class_losses_ref.K_RECORDED ('bce_grad' = 12, 'bce_loss' = 3): ClBce is the same family (logf of a
                      sum, one quotient), measured there at 4 x a float32 restatement.  Not set from this kernel's own output.
    psnr              K_PSNR * 2^-24 * N, N = |ref64| + 10 / ln 10 (the rounding of the quotient 1 / mse reaches the result through the
                      logarithm's derivative, 10 / (ln 10 * y) * y 2^-24); K_PSNR = 'bce_loss' = 3.  mse = 1 gives exactly 0, mse = 0 +inf.
    Decided with (err <= bound).all(): a NaN fails.
Observed on an MI355X (units of 2^-24 N; see OBSERVED_ON_DEVICE).

``mutate`` names one deliberate mistake (MUTATIONS) for tests/test_mean_loss_teeth.py."""
import math

import numpy as np
import torch

import class_losses_ref as CR

KINDS = (0, 1, 2, 3, 4)
KIND_NAMES = {0: "l1", 1: "mse", 2: "label_mse", 3: "bce_logits", 4: "signed"}
CAP_BLOCKS, THREADS = 1024, 256                      # csrc/elementwise.hip: LOSS_BLOCKS, the block size of loss_fwd_k
CAP_ELEMS = CAP_BLOCKS * THREADS * 4                  # 1 048 576: what the capped grid covers in one trip of groups of four
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1027, 1048572, 1048575, 1048576, 1048577, 1048579, 2097157)
A_PHASES = (0, 4, 8, 12)                              # byte phase of a within 16
DA_PHASES = (0, 4)
GOUTS = (1.0, 3.0, -0.5)
GSCALES = (1.0, -1.0)
EXACT_KINDS = (0, 1, 2, 4)
# exact part: (low, high) of a (and b), the labels, and max |e|
EXACT_RANGE = {0: ((0, 3), (0.0,), 3), 1: ((0, 2), (0.0,), 4), 2: ((0, 2), (0.0, 1.0), 4), 4: ((-3, 3), (-1.0, 1.0), 3)}
REAL_LABEL = 0.9                                      # the reference's smoothed real label
LOGIT_SCALE = 6.0
PLANTED_LOGITS = (100.0, -100.0, 90.0, -90.0, 0.0)
PSNR_MSE = (1.0, 0.25, 1e-3, 1e-10)
K_BCE_GRAD, K_BCE_VALUE = CR.K_RECORDED["bce_grad"], CR.K_RECORDED["bce_loss"]
K_PSNR = CR.K_RECORDED["bce_loss"]
K_SQUARE_GRAD = 5.0
MUTATIONS = ("drop_tail", "head_twice", "skip_at_cap", "div_n_minus_1", "signed_label_flipped", "target_grad_not_negated", "sign0_is_1",
             "bce_not_stable")
# Largest figures seen on an MI355X by tests/test_gpu_mean_loss.py (profiles/mean_loss_and_forms.txt): the value as a fraction of its
# (D + 4) bound (2.52 units at worst), the others in units of 2^-24 N against the K named in the key.  A record, not a bound.
OBSERVED_ON_DEVICE = {"value_over_D_plus_4": 0.091, "square_grad_of_5": 1.82, "bce_value_of_3": 0.53, "bce_grad_of_12": 1.60, "psnr_of_3": 0.66}


# ------------------------------------------------------------------------------------------------ launch geometry
def span(n, pa, pb=None):
    """(head, nv, ns): scalar head, groups of four, single elements in all, for byte phases pa (and pb) of the operands."""
    if pb is not None and pb != pa:
        return 0, 0, n
    head = min((16 - pa) % 16 // 4, n)
    nv = (n - head) // 4
    return head, nv, n - 4 * nv


def geometry(n, pa=0, pb=None):
    """blocks, T, the terms one thread adds at most, and D = the longest chain of additions a term passes through."""
    head, nv, ns = span(n, pa, pb)
    blocks = min(CAP_BLOCKS, -(-max(nv + 1, ns) // THREADS))
    T = blocks * THREADS
    per_thread = 4 * -(-nv // T) + max(1, -(-ns // T))
    D = per_thread + 6 + 2 + -(-blocks // 256) + 6 + 2 + 1
    return {"head": head, "nv": nv, "ns": ns, "blocks": blocks, "T": T, "per_thread": per_thread, "D": D}


# ------------------------------------------------------------------------------------------------ inputs
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def critical_indices(n):
    """Where a counting mistake shows: both ends, the last group / first tail element, the first element of the second trip and its
    neighbours."""
    c = {0, 1, 2, 3, n - 1, n - 2, n - 3, 4 * (n // 4) - 1, 4 * (n // 4), CAP_ELEMS - 1, CAP_ELEMS, CAP_ELEMS + 3, CAP_ELEMS + 4}
    return np.array(sorted(i for i in c if 0 <= i < n), np.int64)


def exact_inputs(kind, n):
    """Small integers as f32 (a, b or None).  At the critical indices the term is the largest the range allows (never 0), so one element
    more or less always moves the sum."""
    (lo, hi), _, _ = EXACT_RANGE[kind]
    rng = _rng(11, kind, n)
    a = rng.integers(lo, hi + 1, n).astype(np.float32)
    b = rng.integers(lo, hi + 1, n).astype(np.float32) if kind < 2 else None
    c = critical_indices(n)
    a[c] = hi
    if b is not None:
        b[c] = lo
        z = np.arange(5, n, 11)
        z = z[~np.isin(z, c)]
        b[z] = a[z]                                   # equal operands: sign(0) = 0
    return a, b


def real_inputs(kind, n):
    """f32 reals: images in [0, 1) for kinds 0..2, logits of scale 6 for kinds 3 and 4 with the planted logits at the front (as far as n
    allows).  Every seventh target of kinds 0 and 1 equals its operand."""
    rng = _rng(12, kind, n)
    if kind >= 3:
        a = (rng.standard_normal(n) * LOGIT_SCALE).astype(np.float32)
        k = min(len(PLANTED_LOGITS), n)
        a[:k] = PLANTED_LOGITS[:k]
        return a, None
    a = rng.random(n, np.float32)
    if kind == 2:
        return a, None
    b = rng.random(n, np.float32)
    b[3::7] = a[3::7]
    return a, b


def real_label(kind, real=True):
    if kind == 4:
        return -1.0 if real else 1.0
    return (REAL_LABEL if real else 0.0) if kind >= 2 else 0.0


# ------------------------------------------------------------------------------------------------ the restatement
def _terms(kind, a, b, label, dt, mutate=None):
    """Per-element e and the sum of the absolute values of its summands, in ``dt``."""
    x = np.asarray(a, dt)
    t = np.asarray(b, dt) if kind < 2 else dt(np.float32(label))        # the ABI takes the label as a float
    if kind == 0:
        e = np.abs(x - t)
        return e, e
    if kind in (1, 2):
        d = x - t
        return d * d, d * d
    if kind == 4:
        e = x * (dt(-label) if mutate == "signed_label_flipped" else t)
        return e, np.abs(e)
    with np.errstate(over="ignore"):
        if mutate == "bce_not_stable":
            parts = (x, x * t, np.log(dt(1) + np.exp(-x)))                  # x - x t + log(1 + exp(-x)): overflows for x << 0
        else:
            parts = (np.maximum(x, dt(0)), x * t, np.log1p(np.exp(-np.abs(x))))
    return parts[0] - parts[1] + parts[2], np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2])


def _weights(n, mutate):
    """How often each element is counted (the counting mistakes of MUTATIONS)."""
    w = np.ones(n)
    if mutate == "drop_tail":
        w[4 * (n // 4):] = 0
    if mutate == "head_twice":
        w[0] = 2
    if mutate == "skip_at_cap" and n > CAP_ELEMS:
        w[CAP_ELEMS] = 0
    return w


def forward(kind, a, b, label, dt=np.float64, mutate=None):
    """{'loss', 'sum', 'mean_abs', 'N'}: terms in ``dt``, summed in float64 (exact for the small-integer operands)."""
    n = len(a)
    e, absparts = _terms(kind, a, b, label, dt, mutate)
    w = _weights(n, mutate)
    S = float((e.astype(np.float64) * w).sum())
    count = n - 1 if mutate == "div_n_minus_1" and n > 1 else n
    return {"loss": S / count, "sum": S, "count": count, "mean_abs": float(np.abs(e).astype(np.float64).sum() / n),
            "N": float(absparts.astype(np.float64).sum() / n)}


def exact_value(S, count):
    """f32(S) * f32(1.0 / n), rounded once: what any summation order gives when every partial sum is an integer below 2^24."""
    assert S == int(S) and abs(S) < 2 ** 24
    return np.float32(np.float32(S) * np.float32(1.0 / count))


def upstream32(gout, gscale, n):
    """g as the library forms it: gscale / (float)n on the host, gout[0] * that on the device."""
    return np.float32(np.float32(gout) * np.float32(np.float32(gscale) / np.float32(n)))


def backward(kind, a, b, label, gout, gscale, dt=np.float64, mutate=None):
    """{'grad', 'N'}: de/da * g per element; g in f32 roundings for dt = float32, exact for float64."""
    n = len(a)
    if mutate == "target_grad_not_negated":
        gscale = abs(gscale)
    if mutate == "div_n_minus_1" and n > 1:
        n = n - 1                                     # the divisor only
    x = np.asarray(a, dt)
    t = np.asarray(b, dt) if kind < 2 else dt(np.float32(label))        # the ABI takes the label as a float
    g = upstream32(gout, gscale, n) if dt == np.float32 else np.float64(gout) * np.float64(gscale) / n
    if kind == 0:
        d = np.sign(x - t)
        if mutate == "sign0_is_1":
            d = np.where(x - t == 0, dt(1), d)
        Nn = np.abs(d)
    elif kind in (1, 2):
        d = dt(2) * (x - t)
        Nn = np.abs(d)
    elif kind == 4:
        d = np.full(len(a), dt(-label) if mutate == "signed_label_flipped" else t, dt)
        Nn = np.abs(d)
    else:
        with np.errstate(over="ignore"):
            sg = dt(1) / (dt(1) + np.exp(-x))
        d = sg - t
        Nn = sg + abs(t)
    return {"grad": (d * g).astype(dt), "N": (Nn * abs(g)).astype(np.float64)}


def psnr(mse, dt=np.float64):
    m = dt(np.float32(mse))
    with np.errstate(divide="ignore"):
        return dt(10) * np.log10(dt(1) / m)


# ------------------------------------------------------------------------------------------------ comparisons
def _t(v):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32)).reshape(-1))


def exact_forward_ok(kind, n, got, ref):
    """got (f32) has the bits of f32(S) * f32(1.0 / n) for the restatement's S of small-integer operands."""
    assert n * EXACT_RANGE[kind][2] < 2 ** 24, (kind, n)                    # every partial sum is an exact integer
    return torch.equal(_t(got), _t(exact_value(ref["sum"], n)))


def exact_backward_ok(got, want32):
    """Kinds 0 and 4: every element equals the f32 restatement (torch.equal: -0 == 0, a NaN never)."""
    return torch.equal(_t(got), _t(want32))


def value_bound(kind, n, ref, pa=0, pb=None):
    D = geometry(n, pa, pb)["D"]
    bound = (D + 4) * 2.0 ** -24 * ref["mean_abs"]
    if kind == 3:
        bound = min(bound, K_BCE_VALUE * 2.0 ** -24 * ref["N"])
    return bound


def value_ok(kind, n, got, ref, pa=0, pb=None):
    err = np.abs(np.asarray(got, np.float64) - ref["loss"])
    return bool((err <= value_bound(kind, n, ref, pa, pb)).all())


def value_units(kind, n, got, ref, pa=0, pb=None):
    """(err / (2^-24 mean|e|), D + 4) and, for kind 3, err / (2^-24 N)."""
    err = float(np.abs(np.float64(got) - ref["loss"]))
    u = err / (2.0 ** -24 * ref["mean_abs"]) if ref["mean_abs"] else (0.0 if err == 0 else math.inf)
    un = err / (2.0 ** -24 * ref["N"]) if ref["N"] else (0.0 if err == 0 else math.inf)
    return u, geometry(n, pa, pb)["D"] + 4, un


def grad_bound(kind, ref):
    if kind in (1, 2):
        return K_SQUARE_GRAD * 2.0 ** -24 * np.abs(ref["grad"].astype(np.float64))
    if kind == 3:
        return K_BCE_GRAD * 2.0 ** -24 * ref["N"]
    raise ValueError("kinds 0 and 4 are exact")


def grad_ok(kind, got, ref):
    err = np.abs(np.asarray(got, np.float64) - ref["grad"].astype(np.float64))
    return bool((err <= grad_bound(kind, ref)).all())


def grad_units(kind, got, ref):
    """Largest err / (2^-24 N'), N' = |ref64| (kinds 1, 2) or N (kind 3); an element with N' = 0 must be exact."""
    err = np.abs(np.asarray(got, np.float64) - ref["grad"].astype(np.float64))
    den = 2.0 ** -24 * (np.abs(ref["grad"].astype(np.float64)) if kind in (1, 2) else ref["N"])
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(err == 0, 0.0, err / den)
    return float(np.max(np.nan_to_num(u, nan=np.inf)))


def psnr_bound(mse):
    return K_PSNR * 2.0 ** -24 * (abs(float(psnr(mse))) + 10.0 / math.log(10.0))


def psnr_ok(mse, got):
    if np.float32(mse) == 1:
        return float(got) == 0.0
    return bool(abs(np.float64(got) - psnr(mse)) <= psnr_bound(mse))
