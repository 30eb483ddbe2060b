"""References, case tables and exactness conditions of tests/test_gpu_groupnorm.py (no GPU needed; tests/test_groupnorm_teeth.py
runs everything here on the CPU).

  * float64 references of srcgan_gn_forward / srcgan_gn_backward exactly as include/srcgan_amd.h states them, each with the float64
    sum of the absolute terms of its expression (the N of the bounds).  `defect=` makes one named mistake: the teeth test shows
    that the GPU file's comparisons tell each from the right answer.
  * stats_f32_model: the statistics algorithm of csrc/groupnorm.hip restated in numpy float32 -- per-thread sums around the
    thread's first sample, then (count, mean, M2) combined over the pixel lanes of a block, the blocks, the channels of a group.
  * the case tables, and the conditions under which a backward case is exact in f32 whatever the order of summation.
An operand is a triple (buffer [npix, cs], cs, coff): its C channels are [coff, coff + C) of every cs-channel record, everything
else holds the sentinel 1000; the kernel gets the address of element coff."""
import numpy as np
import torch

DTS = ["fp32", "bf16", "fp16"]
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
EPS_T = {"fp32": 2.0 ** -20, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
EPP = {"fp32": 4, "bf16": 8, "fp16": 8}
U32 = 2.0 ** -24
SENT = 1000.0
EPS = 1e-5
SLOPE = 0.2
GN_MAXBLK = 32
STAT_UNITS = 8          # c of the statistics bounds (see test_gpu_groupnorm.py: counted roundings, not a measurement)


def f32(v):
    """the float64 value of v rounded to f32: what a float argument of the C ABI carries"""
    return float(torch.tensor(v, dtype=torch.float32))


# --------------------------------------------------------------------------- geometry of the two-stage statistics
def geometry(dt, hw, C):
    """VG channel vectors per pixel, PL pixel lanes per block, nblk = clamp(hw * VG / 2048, 1, 32) blocks of per = cdiv(hw, nblk)
    pixels; ranges[k] = (p0, p1) of block k, p1 <= p0 for an empty one"""
    epp = EPP[dt]
    assert C % epp == 0 and 256 % (C // epp) == 0, (dt, C)
    VG = C // epp
    nblk = max(1, min(GN_MAXBLK, hw * VG // 2048))
    per = -(-hw // nblk)
    ranges = [(k * per, min(k * per + per, hw)) for k in range(nblk)]
    return dict(epp=epp, VG=VG, PL=256 // VG, nblk=nblk, per=per, ranges=ranges)


def empty_blocks(dt, hw, C):
    return [k for k, (p0, p1) in enumerate(geometry(dt, hw, C)["ranges"]) if p1 <= p0]


def chain_length(dt, hw, C, G):
    """the longest serial f32 chain of a sum: a thread's samples, the lanes, the blocks, the channels of a group"""
    g = geometry(dt, hw, C)
    return -(-g["per"] // g["PL"]) + g["PL"] + g["nblk"] + C // G


# --------------------------------------------------------------------------- operands
def make_op(vals, cs=None, coff=0):
    npix, C = vals.shape
    cs = cs or C + coff
    assert coff + C <= cs
    buf = torch.full((npix, cs), SENT, dtype=vals.dtype, device=vals.device)
    buf[:, coff:coff + C] = vals
    return (buf, cs, coff)


def blank_op(npix, C, tdt, device, cs=None, coff=0):
    cs = cs or C + coff
    return (torch.full((npix, cs), SENT, dtype=tdt, device=device), cs, coff)


def vals_of(op, C, shift=0):
    """the operand's [npix, C] values; shift moves the channel offset (the teeth test's perturbation)"""
    buf, _, coff = op
    return buf[:, coff + shift:coff + shift + C]


def ptr_of(op):
    buf, _, coff = op
    return buf.data_ptr() + coff * buf.element_size()


def outside_untouched(op, C):
    buf, cs, coff = op
    keep = torch.ones(cs, dtype=torch.bool, device=buf.device)
    keep[coff:coff + C] = False
    return bool((buf[:, keep] == SENT).all())


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# --------------------------------------------------------------------------- float64 references
def group_index(C, G, device, defect=None):
    cpg = C // G
    c = torch.arange(C, device=device)
    if defect == "group_off_by_one":            # the last channel of every group but the last one is given to the next group
        return ((c + 1) // cpg).clamp_max(G - 1)
    return c // cpg


def stats64(x, B, hw, C, G, defect=None, dt=None):
    """float64 mean and biased variance [B, G] of the stored x ([B*hw, C])"""
    v = x.double().reshape(B, hw, G, C // G)
    if defect == "drop_pixel":
        v = v[:, :hw - 1]
    elif defect == "drop_last_block":
        g = geometry(dt, hw, C)
        last = [r for r in g["ranges"] if r[1] > r[0]][-1]
        v = v[:, :last[0]]
    mean = v.mean((1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean((1, 3))
    if defect == "n_is_hw":                     # M2 divided by hw, not by hw * cpg
        var = var * (C // G)
    return mean, var


def rstd64(var):
    return (var + f32(EPS)) ** -0.5


def stats_tensor(mean, var):
    """[B, G, 2] f32 = {mean, rstd}: the layout of the kernels' stats"""
    return torch.stack([mean, rstd64(var)], -1).float()


def _per_channel(stats, B, C, G, defect=None):
    gi = group_index(C, G, stats.device, defect)
    s = stats.double().reshape(B, G, 2)
    return s[:, gi, 0].reshape(B, 1, C), s[:, gi, 1].reshape(B, 1, C)


def _vec(p, C, device, fill):
    return torch.full((C,), fill, dtype=torch.float64, device=device) if p is None else p.double()


def ref_forward(x, res, gamma, beta, stats, B, hw, C, G, relu, slope, defect=None):
    """float64 act((x - mu) r gamma + beta + res) with mu, r the GIVEN statistics (f32 numbers read as float64), and
    N = |x - mu| r |gamma| + |beta| + |res|; both [B*hw, C]"""
    mu, r = _per_channel(stats, B, C, G, defect)
    xv = x.double().reshape(B, hw, C)
    gam, bet = _vec(gamma, C, x.device, 1.0), _vec(beta, C, x.device, 0.0)
    core = (xv - mu) * r * gam
    v = core + bet
    n = core.abs() + bet.abs()
    if res is not None:
        rv = res.double().reshape(B, hw, C)
        v, n = v + rv, n + rv.abs()
    if relu:
        v = torch.where(v > 0, v, v * f32(slope))
    return v.reshape(B * hw, C), n.reshape(B * hw, C)


def ref_backward(dy, yact, x, gamma, stats, slope, B, hw, C, G, defect=None):
    """float64 srcgan_gn_backward: g = dy [* (yact > 0 ? 1 : slope)], xhat = (x - mu) r, per (image, channel) sums sg, sgx,
    S1 = sum_group gamma sg / n, S2 = sum_group gamma sgx / n (n = hw cpg), dx = r (g gamma - S1 - xhat S2), dres = g,
    dbeta = sum_b sg, dgamma = sum_b sgx, and the N of each bound."""
    cpg = C // G
    n = hw * cpg
    mu, r = _per_channel(stats, B, C, G)
    g = dy.double().reshape(B, hw, C)
    if yact is not None:
        a = yact.double().reshape(B, hw, C)
        g = g * torch.where((a >= 0) if defect == "ge_mask" else (a > 0), 1.0, f32(slope))
    xh = (x.double().reshape(B, hw, C) - mu) * r
    gam = _vec(gamma, C, dy.device, 1.0)
    sg, sgx = g.sum(1), (g * xh).sum(1)
    grp = lambda t: t.reshape(B, G, cpg).sum(2).repeat_interleave(cpg, 1).reshape(B, 1, C) / n
    S1, S2 = grp(sg * gam), grp(sgx * gam)
    A1, A2 = grp((g * gam).abs().sum(1)), grp((g * gam * xh).abs().sum(1))
    xterm = 0.0 if defect == "no_xhat_term" else xh * S2
    dx = r * (g * gam - S1 - xterm)
    ndx = r * ((g * gam).abs() + A1 + xh.abs() * A2)
    dres = g * gam if defect == "gamma_on_dres" else g
    return dict(dx=dx.reshape(B * hw, C), n_dx=ndx.reshape(B * hw, C), dres=dres.reshape(B * hw, C), g=g.reshape(B * hw, C),
                dbeta=sg.sum(0), dgamma=sgx.sum(0), n_dbeta=g.abs().sum((0, 1)), n_dgamma=(g * xh).abs().sum((0, 1)),
                sg=sg, sgx=sgx, S1=S1, S2=S2, xh=xh)


# --------------------------------------------------------------------------- the statistics in numpy float32
def _combine(n, mean, m2, nb, mb, m2b):
    """chan_combine of csrc/common.h on f32 arrays: (n, mean, M2) += (nb, mb, m2b); n and nb are f32 scalars"""
    if nb <= 0:
        return n, mean, m2
    nn = np.float32(n + nb)
    d = mb - mean
    mean = mean + d * np.float32(nb / nn)
    m2 = m2 + (m2b + d * d * np.float32(np.float32(n * nb) / nn))
    return nn, mean, m2


def stats_f32_model(x, dt, B, hw, C, G):
    """The device algorithm in IEEE float32 (no fused multiply-add), x = the stored values [B*hw, C].  -> f32 [B, G, 2]"""
    geo = geometry(dt, hw, C)
    PL = geo["PL"]
    xv = x.float().cpu().numpy().reshape(B, hw, C).astype(np.float32)
    one, zero = np.float32(1), np.float32(0)
    bn, bmean, bm2 = zero, np.zeros((B, C), np.float32), np.zeros((B, C), np.float32)
    for p0, p1 in geo["ranges"]:
        cnt = max(p1 - p0, 0)
        if cnt == 0:
            continue
        steps = -(-cnt // PL)
        blk = np.zeros((B, steps * PL, C), np.float32)
        blk[:, :cnt] = xv[:, p0:p1]
        blk = blk.reshape(B, steps, PL, C)
        valid = (np.arange(steps * PL) < cnt).reshape(steps, PL)
        sh = np.where(valid[0][None, :, None], blk[:, 0], zero)
        s0, s1 = np.zeros((B, PL, C), np.float32), np.zeros((B, PL, C), np.float32)
        for k in range(steps):
            v = blk[:, k] - sh
            m = valid[k][None, :, None]
            s0 = np.where(m, s0 + v, s0)
            s1 = np.where(m, s1 + v * v, s1)
        nsmp = valid.sum(0).astype(np.float32)
        inv = np.where(nsmp > 0, one / np.maximum(nsmp, one), zero).astype(np.float32)[None, :, None]
        tmean = sh + s0 * inv
        tm2 = s1 - s0 * s0 * inv
        ln, lmean, lm2 = zero, np.zeros((B, C), np.float32), np.zeros((B, C), np.float32)
        for q in range(PL):
            ln, lmean, lm2 = _combine(ln, lmean, lm2, nsmp[q], tmean[:, q], tm2[:, q])
        bn, bmean, bm2 = _combine(bn, bmean, bm2, np.float32(cnt), lmean, lm2)
    cpg = C // G
    cm, c2 = bmean.reshape(B, G, cpg), bm2.reshape(B, G, cpg)
    gn, gmean, gm2 = zero, np.zeros((B, G), np.float32), np.zeros((B, G), np.float32)
    for i in range(cpg):
        gn, gmean, gm2 = _combine(gn, gmean, gm2, np.float32(hw), cm[:, :, i], c2[:, :, i])
    invn = one / (np.float32(hw) * np.float32(cpg))
    rstd = one / np.sqrt(gm2 * invn + np.float32(EPS), dtype=np.float32)
    assert gmean.dtype == np.float32 and rstd.dtype == np.float32
    return torch.from_numpy(np.stack([gmean, rstd], -1))


def stat_units(stats, mean64, var64):
    """The two errors of stats ([B, G, 2]) in the units of their bounds: |mean - mean64| / (2^-24 (|mean64| + sd64)) and
    |rstd - rstd64| / rstd64 / (2^-24 (1 + |mean64| / sd64)), sd64 = sqrt(var64 + eps).  -> two [B, G] float64 tensors"""
    s = stats.double().reshape(mean64.shape + (2,))
    sd = (var64 + f32(EPS)).sqrt()
    um = (s[..., 0] - mean64).abs() / (U32 * (mean64.abs() + sd))
    ur = (s[..., 1] * sd - 1.0).abs() / (U32 * (1.0 + mean64.abs() / sd))
    return um, ur


# --------------------------------------------------------------------------- case tables
def stat_shapes(dt):
    """(B, hw, C, G, what the shape reaches)"""
    s = []
    if dt == "fp32":
        s += [(2, 105, 1024, 32, "empty block 12 of 13, one pixel lane"), (2, 105, 1024, 1024, "the same with G == C"),
              (2, 289, 512, 32, "17x17 of ResDeconv layer 4: block 17 of 18 is empty")]
    else:
        s += [(2, 289, 1024, 32, "block 17 of 18 is empty")]
    s += [(2, 5, 64, 32, "pixel lanes without a sample"), (2, 1, 64, 32, "hw = 1"), (2, 1, 64, 64, "hw = 1, G == C: variance 0"),
          (2, 5, 64, 64, "InstanceNorm form on 5 pixels")]
    if dt != "fp32":
        s += [(2, hw, 8, G, "one channel vector per pixel, 256 pixel lanes") for hw in (2, 3) for G in (8, 1)]
    s += [(16, 66 * 65, 64, 32, "fp32: 32-block cap, short last block, second grid-stride trip")]
    if dt != "fp32":
        s += [(16, 66 * 65, 128, 32, "16 bits: 32-block cap, short last block, second grid-stride trip")]
    s += [(2, 256, 256, 32, "whole blocks (8 in fp32, 4 in 16 bits)")]
    return s


STAT_VARIANTS = ["mean0", "mean30", "mean1000", "chan"]


def stat_data(B, hw, C, variant, tdt, seed):
    """unit-variance normal data; image b is moved by k + b / 8 with k = 0, 30, 1000 standard deviations -- a different offset per
    image, and every image of the B = 16 cases within two standard deviations of the nominal mean ('chan': every channel by its
    own offset of about 3 standard deviations, so that the channels of a group have different means)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, hw, C, generator=gen)
    x += 0.125 * torch.arange(B).float().view(B, 1, 1)
    if variant == "chan":
        x += 3.0 * torch.randn(1, 1, C, generator=gen)
    else:
        x += {"mean0": 0.0, "mean30": 30.0, "mean1000": 1000.0}[variant]
    return x.reshape(B * hw, C).to(tdt)


def spike_positions(dt, B, hw, C):
    """(image, pixel, channel) of the single non-zero sample: the first and last pixel of every block's range, the last pixel of
    the image, a pixel of the last image, every lane of one channel vector"""
    geo = geometry(dt, hw, C)
    pos = []
    for p0, p1 in geo["ranges"]:
        if p1 > p0:
            pos += [(0, p0, 0), (0, p1 - 1, C - 1)]
    pos += [(0, hw - 1, C // 2), (B - 1, hw // 2, 1)]
    v0 = geo["epp"] if C >= 2 * geo["epp"] else 0
    pos += [(0, hw // 3, v0 + i) for i in range(geo["epp"])]
    return sorted(set(pos))


def spike_shapes(dt):
    s = [(2, 5, 64, 32), (2, 66 * 65, 64 if dt == "fp32" else 128, 32)]
    s += [(2, 289, 512, 32), (2, 105, 1024, 32)] if dt == "fp32" else [(2, 289, 1024, 32), (2, 3, 8, 1)]
    return s


def apply_data(B, hw, C, G, tdt, seed):
    """x for the forward apply cases, exact in every storage type: x = o_b + k_c + z with o_b = 2 - 3 b, k_c = c mod 2 and z a
    non-zero multiple of 1/8, |z| <= 3/8, that sums to zero over the pixels of every (image, channel) (pairs +z, -z and one
    triple z, z, -2z).  The group's mean is then o_b + mean(k_c) exactly, a multiple of 1/2, and |x - mean| >= 1/8 everywhere:
    no result of (x - mean) r gamma comes near fp16's subnormal range, where eps_T N would not hold for a correct kernel."""
    assert hw >= 5 and hw % 2 == 1 and B <= 2 and ((C // G) % 2 == 0 or C == G)
    gen = torch.Generator().manual_seed(seed)
    npair = (hw - 3) // 2
    mag = torch.randint(1, 4, (B, npair, C), generator=gen).float() / 8
    sgn = torch.where(torch.rand(B, npair, C, generator=gen) < 0.5, -1.0, 1.0)
    t = torch.where(torch.rand(B, 1, C, generator=gen) < 0.5, -1.0, 1.0) / 8
    z = torch.cat([mag * sgn, -mag * sgn, t, t, -2 * t], 1)
    z = z[:, torch.randperm(hw, generator=gen)]
    x = z + (2.0 - 3.0 * torch.arange(B).float()).view(B, 1, 1) + (torch.arange(C) % 2).float().view(1, 1, C)
    assert bool((z.sum(1) == 0).all()) and bool((x.to(tdt).float() == x).all())
    return x.reshape(B * hw, C).to(tdt)


def affine(C, seed, device="cpu"):
    """gamma = +-[0.5, 1.5], |beta| in [0.25, 1.25]"""
    gen = torch.Generator().manual_seed(seed)
    sg = lambda: torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
    return (sg() * (0.5 + torch.rand(C, generator=gen))).to(device), (sg() * (0.25 + torch.rand(C, generator=gen))).to(device)


# exact backward cases: (B, hw, C, G); n = hw * C / G is a power of two
def exact_bwd_shapes(dt):
    s = [(2, 16, 64, 32), (3, 64, 64, 64), (2, 256, 256, 32), (2, 1, 64, 32)]
    if dt != "fp32":
        s += [(2, 4, 8, 8), (2, 4, 8, 1)]
    return s


def sum_only_bwd_shapes(dt):
    """hw * cpg is no power of two: dbeta, dgamma and dres are still exact"""
    return [(2, 105, 1024, 32), (2, 289, 512, 32)] if dt == "fp32" else [(2, 289, 1024, 32), (2, 3, 8, 1), (2, 5, 64, 32)]


def exact_bwd_case(B, hw, C, G, tdt, seed, with_gamma=True, with_yact=True, slope=0.5):
    """Integer-valued operands of srcgan_gn_backward with crafted statistics (stats is an input of the call)."""
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
    mean = ri(-3, 3, B, G)
    rstd = 2.0 ** ri(-1, 1, B, G)
    cpg = C // G
    x = mean.repeat_interleave(cpg, 1).view(B, 1, C) + ri(-8, 8, B, hw, C)
    dy = ri(-4, 4, B, hw, C)
    gamma = torch.tensor([-1.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (C,), generator=gen)] if with_gamma else None
    yact = ri(-1, 1, B, hw, C) if with_yact else None
    q = lambda t: None if t is None else t.reshape(B * hw, C).to(tdt)
    return dict(B=B, hw=hw, C=C, G=G, x=q(x), dy=q(dy), yact=q(yact), gamma=gamma, stats=torch.stack([mean, rstd], -1), slope=slope)


def _is_f32(t):
    return bool((t.float().double() == t).all())


def exact_bwd_conditions(k, ref, sums_only=False):
    """On the reference alone: why the case is exact.  The operands are what the table says; every per-(image, channel) sum, its
    gamma-weighted group sum, S1, S2, xhat S2 and the bracket of dx are f32 numbers, and so is dx: the kernel's f32 arithmetic
    makes no rounding error in any order, with or without fused multiply-add, and the cast to the storage type is the only
    rounding (the same round-to-nearest-even on both sides)."""
    B, hw, C, G = k["B"], k["hw"], k["C"], k["G"]
    n = hw * C // G
    mean, rstd = k["stats"][..., 0], k["stats"][..., 1]
    assert bool((mean == mean.round()).all()) and bool(((rstd == 0.5) | (rstd == 1) | (rstd == 2)).all())
    x, dy = k["x"].double(), k["dy"].double()
    assert bool((x == x.round()).all()) and bool((dy == dy.round()).all()) and float(dy.abs().max()) <= 4
    assert float((x.view(B, hw, C) - mean.double().repeat_interleave(C // G, 1).view(B, 1, C)).abs().max()) <= 8
    assert k["slope"] in (0.0, 0.5)
    if k["yact"] is not None:
        assert set(k["yact"].double().unique().tolist()) <= {-1.0, 0.0, 1.0} and bool((k["yact"] == 0).any())
    # every partial sum is a multiple of 1/8 (g in halves, xhat in halves, gamma in halves) below 2^21: exact in any order
    assert float(ref["n_dgamma"].max()) * 8 < 2 ** 24 and float(ref["n_dbeta"].max()) * 8 < 2 ** 24
    gmax = 2.0 if k["gamma"] is not None else 1.0
    assert float(ref["n_dgamma"].max()) * gmax * (C // G) * 16 < 2 ** 24
    for name in ("sg", "sgx", "dbeta", "dgamma", "dres"):
        assert _is_f32(ref[name]), name
    if sums_only:
        return
    assert n & (n - 1) == 0, "hw * cpg must be a power of two"
    for name in ("S1", "S2", "dx"):
        assert _is_f32(ref[name]), name
    mu, r = _per_channel(k["stats"], B, C, G)
    gam = _vec(k["gamma"], C, x.device, 1.0)
    xs2 = ref["xh"] * ref["S2"]
    inner = ref["S1"] + xs2
    bracket = ref["g"].view(B, hw, C) * gam - inner
    assert _is_f32(xs2) and _is_f32(inner) and _is_f32(bracket) and _is_f32(r * bracket)


# float64 backward cases: the statistics shapes that matter for the backward's own sums and its apply kernel
def f64_bwd_shapes(dt):
    s = [(2, 105, 1024, 32), (2, 289, 512, 32)] if dt == "fp32" else [(2, 289, 1024, 32), (2, 3, 8, 8), (2, 3, 8, 1)]
    s += [(2, 5, 64, 32), (2, 256, 256, 32), (16, 66 * 65, 64 if dt == "fp32" else 128, 32)]
    return s
