"""Channel attention + block residual in numpy, for the tests of srcgan_ca_forward / srcgan_ca_backward (our own restatement):

    p[b,c] = mean_hw t[b,.,c];  h = relu(W1 p + b1);  s = sigmoid(W2 h + b2);  y = t s[b,c] (+ res)
    dres (=, +=) g;  ds = sum_hw g t;  dz2 = ds s (1 - s);  dW2 = sum_b dz2 (x) h;  db2 = sum_b dz2;  dh = (W2^T dz2) [h > 0]
    dW1 = sum_b dh (x) p;  db1 = sum_b dh;  dt = g s[b,c] + (W1^T dh)[b,c] / hw

``forward`` / ``backward`` run in ``dt`` = float64 (the reference) or float32 (every product, sum and the gate rounded to f32, sums taken
one term after the other: what a plain f32 evaluation commits).  Tensors are [B, hw, C].  ``mutate`` names one deliberate mistake
(MUTATIONS) for the teeth test.

Tolerances.  An element with float64 value v is held to  K * 2^-24 * N  (+ one rounding of the storage type for a 16-bit output), N = the
sum of the absolute values of the terms the element is made of, PLUS what the errors of the stages before it contribute (``scales``).
That second part makes N larger than the element's own terms alone (for dt: |g s| + |dp| / hw): dp, dh and dz2 are sums of terms of
both signs, so their own magnitude can be far below the rounding errors they inherit from s, ds and the pooled mean, and a bound in
units of the literal N would be ill-conditioned; every K below is in units of this N and of no other.  K is not chosen: ``measure_k``
gives, per quantity, the largest error of the float32 restatement in those units on the very inputs of the GPU grid (``grid_cases``),
and the kernel gets 4 x that, because its summation order differs.  K_RECORDED is 4 x the measured figure, rounded up to the next
integer and nothing else, as measured on the CPU; tests/test_chan_attn_teeth.py re-measures it."""
import itertools

import numpy as np

CHUNK = 256                     # the kernel's pixels per partial-sum block (csrc/chan_attn.hip: CA_CHUNK)
MUTATIONS = ("pool_drops_pixel", "pool_padded_count", "gate_of_next_sample", "no_sigmoid_derivative", "no_relu_mask", "no_dp_term",
             "dres_stored", "dw2_one_sample")
QUANTITIES = ("p", "h", "s", "y", "dt", "dres", "dw1", "db1", "dw2", "db2")
# 4 x the float32 restatement's largest error over grid_cases() and the three storage types, in units of 2^-24 N, rounded up to the
# next integer.  Measured (measure_k, largest of fp32 / bf16 / fp16): p 7.66, h 2.18, s 2.19, y 1.49, dt 1.51, dres 1.00, dw1 0.44, db1 0.31,
# dw2 1.19, db2 1.83.
K_RECORDED = {"p": 31.0, "h": 9.0, "s": 9.0, "y": 6.0, "dt": 7.0, "dres": 4.0, "dw1": 2.0, "db1": 2.0, "dw2": 5.0, "db2": 8.0}
STORE_EPS = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}       # half an ulp, relative


def _sum(a, axis, dt):
    """Sum along ``axis``: one term after the other in float32, numpy's own in float64."""
    if dt == np.float64:
        return a.sum(axis=axis)
    return np.take(np.cumsum(a, axis=axis, dtype=np.float32), -1, axis=axis)


def forward(t, res, w1, b1, w2, b2, dt=np.float64, mutate=None):
    t, w1, b1, w2, b2 = (np.asarray(v, dt) for v in (t, w1, b1, w2, b2))
    B, hw, C = t.shape
    pool = t[:, :-1] if (mutate == "pool_drops_pixel" and hw > 1) else t
    count = (hw // 8 + 1) * 8 if mutate == "pool_padded_count" else hw
    p = (_sum(pool, 1, dt) / dt(count)).astype(dt)
    h = np.maximum(_sum(w1[None] * p[:, None, :], 2, dt) + b1[None], dt(0)).astype(dt)
    z = (_sum(w2[None] * h[:, None, :], 2, dt) + b2[None]).astype(dt)
    s = (dt(1) / (dt(1) + np.exp(-z).astype(dt))).astype(dt)
    gate = np.roll(s, -1, axis=0) if mutate == "gate_of_next_sample" else s
    y = (t * gate[:, None, :]).astype(dt)
    if res is not None:
        y = (y + np.asarray(res, dt)).astype(dt)
    return {"p": p, "h": h, "s": s, "y": y}


def backward(g, t, w1, w2, saved, dres_old=None, dt=np.float64, mutate=None):
    """saved: forward()'s dict.  dres_old: None (dres = g) or the tensor dres adds to."""
    g, t, w1, w2 = (np.asarray(v, dt) for v in (g, t, w1, w2))
    p, h, s = (np.asarray(saved[k], dt) for k in ("p", "h", "s"))
    B, hw, C = t.shape
    ds = _sum((g * t).astype(dt), 1, dt)
    dz2 = ds if mutate == "no_sigmoid_derivative" else (ds * (s * (dt(1) - s)).astype(dt)).astype(dt)
    dh = _sum(w2.T[None] * dz2[:, None, :], 2, dt).astype(dt)               # [B, Cr]
    if mutate != "no_relu_mask":
        dh = np.where(h > 0, dh, dt(0)).astype(dt)
    dp = _sum(w1.T[None] * dh[:, None, :], 2, dt).astype(dt)               # [B, C]
    nb = 1 if mutate == "dw2_one_sample" else B
    out = {
        "dw2": _sum((dz2[:nb, :, None] * h[:nb, None, :]).astype(dt), 0, dt),
        "db2": _sum(dz2, 0, dt),
        "dw1": _sum((dh[:, :, None] * p[:, None, :]).astype(dt), 0, dt),
        "db1": _sum(dh, 0, dt),
    }
    dtv = (g * s[:, None, :]).astype(dt)
    if mutate != "no_dp_term":
        dtv = (dtv + (dp / dt(hw)).astype(dt)[:, None, :]).astype(dt)
    out["dt"] = dtv
    out["dres"] = g.copy() if (dres_old is None or mutate == "dres_stored") else (g + np.asarray(dres_old, dt)).astype(dt)
    return out


def scales(t, res, g, w1, b1, w2, b2, dres_old=None):
    """N per quantity, in float64 from the float64 reference: the element's own terms in absolute value, plus what the errors of the
    stages it is computed from contribute (each stage's N times the magnitude it is multiplied by)."""
    t, g, w1, b1, w2, b2 = (np.asarray(v, np.float64) for v in (t, g, w1, b1, w2, b2))
    f = forward(t, res, w1, b1, w2, b2)
    p, h, s = f["p"], f["h"], f["s"]
    B, hw, C = t.shape
    a1, a2 = np.abs(w1), np.abs(w2)
    Np = np.abs(t).mean(axis=1)
    Nh = Np @ a1.T + np.abs(b1)[None]
    Ns = 0.25 * (Nh @ a2.T + np.abs(b2)[None]) + s
    Ny = np.abs(t) * (s + Ns)[:, None, :] + (np.abs(np.asarray(res, np.float64)) if res is not None else 0.0)
    Nds = np.abs(g * t).sum(axis=1)
    ds = (g * t).sum(axis=1)
    Ndz = Nds * s * (1 - s) + np.abs(ds) * Ns
    Ndh = Ndz @ a2
    Ndp = Ndh @ a1
    dz2 = ds * s * (1 - s)
    dh = np.where(h > 0, dz2 @ w2, 0.0)
    N = {"p": Np, "h": Nh, "s": Ns, "y": Ny,
         "dt": np.abs(g) * (s + Ns)[:, None, :] + (Ndp / hw)[:, None, :],
         "dres": np.abs(g) + (np.abs(np.asarray(dres_old, np.float64)) if dres_old is not None else 0.0),
         "dw2": (Ndz[:, :, None] * np.abs(h)[:, None, :] + np.abs(dz2)[:, :, None] * Nh[:, None, :]).sum(axis=0),
         "db2": Ndz.sum(axis=0),
         "dw1": (Ndh[:, :, None] * np.abs(p)[:, None, :] + np.abs(dh)[:, :, None] * Np[:, None, :]).sum(axis=0),
         "db1": Ndh.sum(axis=0)}
    return N


def tolerance(name, ref, N, dtype="fp32", K=None):
    """Per-element bound for quantity ``name``; the storage rounding is added for the tensors kept in the storage type."""
    k = (K or K_RECORDED)[name]
    tol = k * 2.0 ** -24 * N
    if name in ("y", "dt", "dres"):
        tol = tol + STORE_EPS[dtype] * np.abs(ref) + (2.0 ** -25 if dtype == "fp16" else 0.0)
    return tol


def worst(name, got, ref, N, dtype="fp32", K=None):
    """Largest |got - ref| / tolerance over the elements (<= 1: within the bound)."""
    tol = tolerance(name, ref, N, dtype, K)
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))))


def units(got, ref, N):
    """Largest error in units of 2^-24 N."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(2.0 ** -24 * N, 1e-300))))


def grid_cases():
    """(B, hw, C, Cr, with_res, dres_accumulate, null_grad) of the GPU grid: hw = 1, 63, one below / at / above the chunk, two chunks and
    a ragged tail; res, dres_accumulate and the parameter-gradient pointer set to null (0..3; 4: none) cycle through the cases."""
    out = []
    for i, (hw, C, B) in enumerate(itertools.product((1, 63, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1), (16, 64, 96), (1, 3))):
        for j, Cr in enumerate((1, 4, C)):
            n = 3 * i + j
            out.append((B, hw, C, Cr, (n + hw) & 1, ((n >> 1) + hw) & 1, n % 5))
    return out


def make_inputs(case, dtype="fp32", seed=0):
    """Inputs of one grid case, already rounded to the storage type (returned as float32 arrays holding representable values)."""
    import torch
    B, hw, C, Cr, with_res, acc, _ = case
    rng = np.random.default_rng(seed + 7919 * (hw * 131 + C * 7 + Cr * 3 + B))
    td = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    rnd = lambda a: torch.from_numpy(a.astype(np.float32)).to(td).float().numpy()
    t = rnd(rng.standard_normal((B, hw, C)) + 0.3)
    res = rnd(rng.standard_normal((B, hw, C))) if with_res else None
    g = rnd(rng.standard_normal((B, hw, C)))
    old = rnd(rng.standard_normal((B, hw, C))) if acc else None
    w1 = (rng.standard_normal((Cr, C)) / np.sqrt(C)).astype(np.float32)
    b1 = (0.2 * rng.standard_normal(Cr) + 0.1).astype(np.float32)
    w2 = (rng.standard_normal((C, Cr)) / np.sqrt(Cr)).astype(np.float32)
    b2 = (0.2 * rng.standard_normal(C)).astype(np.float32)
    return dict(t=t, res=res, g=g, old=old, w1=w1, b1=b1, w2=w2, b2=b2)


def reference(inp, mutate=None):
    """float64 forward + backward of one case -> dict of all QUANTITIES."""
    f = forward(inp["t"], inp["res"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], mutate=mutate)
    b = backward(inp["g"], inp["t"], inp["w1"], inp["w2"], f, inp["old"], mutate=mutate)
    return {**f, **b}


def measure_k(dtype="fp32", cases=None):
    """Per quantity: the float32 restatement's largest error over the grid, in units of 2^-24 N."""
    k = {q: 0.0 for q in QUANTITIES}
    for case in (cases or grid_cases()):
        inp = make_inputs(case, dtype)
        ref = reference(inp)
        N = scales(inp["t"], inp["res"], inp["g"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], inp["old"])
        f = forward(inp["t"], inp["res"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], dt=np.float32)
        b = backward(inp["g"], inp["t"], inp["w1"], inp["w2"], f, inp["old"], dt=np.float32)
        for q, v in {**f, **b}.items():
            k[q] = max(k[q], units(v, ref[q], N[q]))
    return k
