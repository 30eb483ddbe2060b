"""Direct tests, through the C ABI, of srcgan_gn_forward / srcgan_gn_backward (csrc/groupnorm.hip): GroupNorm(32) with residual
and ReLU of the ResDeconv colouriser and, with G == C and no affine part, the InstanceNorm2d of the discriminator.  fp32, bf16
and fp16 throughout; references, case tables and exactness conditions are in tests/groupnorm_ref.py.

Every output buffer is filled with the sentinel 1000 and compared whole; every input is compared with its copy afterwards.
Two kinds of assertion only:
  * EXACT -- the bits (or, for dx, the values) of the float64 reference cast once: crafted integer statistics and operands, for
    which every f32 intermediate is exact in any order (groupnorm_ref.exact_bwd_conditions says why, on the reference alone);
  * PER ELEMENT against float64 of the stored inputs:
      statistics  |mean - mean64| <= 8 * 2^-24 (|mean64| + sd64),  |rstd - rstd64| / rstd64 <= 8 * 2^-24 (1 + |mean64| / sd64),
                  sd64 = sqrt(var64 + eps).  The 8: three stored f32 partial means (thread, block, channel), each rounded to
                  half an ulp of |mean| and entering a difference twice, the final t1 * invn + eps and a 1-ulp rsqrtf.  Counted,
                  not measured; the numpy-f32 restatement of the algorithm stays under 4 (tests/test_groupnorm_teeth.py).
      forward     |y - ref| <= eps_T N, N = |x - mu| r |gamma| + |beta| + |res|, mu and r the f32 statistics the call returned
      backward    |dx - ref| <= (eps_T + 512 * 2^-24) N, N = r (|g gamma| + sum|g gamma| / n + |xhat| sum|g gamma xhat| / n);
                  dgamma, dbeta: 512 * 2^-24 * sum |terms| (512 bounds the longest serial f32 chain; asserted per case)
      chain       forward -> backward against float64 autograd of F.group_norm + residual + leaky_relu: (eps_T + 1e-5) N
    eps_T = 2^-20 / 2^-8 / 2^-11.  Each tolerance test prints its maxima ("[gn] ..." lines, pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

import groupnorm_ref as R
from groupnorm_ref import DTS, TDT, EPS_T, EPP, U32, SENT, EPS, SLOPE, same_bits

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- comparisons (shared with the CPU teeth test)
def check_stats(stats, mean64, var64):
    """-> (both bounds hold everywhere, largest mean error, largest rstd error), the errors in units of 2^-24 (bound: 8)"""
    um, ur = R.stat_units(stats, mean64, var64)
    return bool((um <= R.STAT_UNITS).all()) and bool((ur <= R.STAT_UNITS).all()), float(um.max()), float(ur.max())


def within(out, ref, bound):
    """-> (|out - ref| <= bound for every element, largest |out - ref| / bound)"""
    err = (out.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return bool((err <= bound).all()), float(ratio.max())            # a NaN anywhere fails


def equal_cast(out, ref64):
    """torch.equal with the float64 reference cast once to out's type (through f32, which the exact cases' values are)"""
    return torch.equal(out, ref64.float().to(out.dtype).reshape(out.shape))


def bits_cast(out, ref64):
    return same_bits(out.contiguous(), ref64.float().to(out.dtype).reshape(out.shape).contiguous())


def report(what, dt, **kv):
    print(f"[gn] {what} {dt}: " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in kv.items()))


# --------------------------------------------------------------------------- the library
class Lib:
    def __init__(self):
        from srcgan_amd import _native as N
        self.N, self.lib = N, N.lib()

    def st(self):
        return self.N.stream_ptr(torch.device("cuda"))

    def scratch(self, B, C):
        """NaN-filled: a slot read before it is written cannot pass for a number"""
        return torch.full((self.lib.srcgan_gn_scratch_floats(B, C) + 8,), float("nan"), device="cuda")

    def forward_raw(self, x, x_cs, res, res_cs, y, y_cs, gamma, beta, stats, B, hw, C, G, relu, slope, dtype, scratch, eps=EPS):
        self.N.check(self.lib.srcgan_gn_forward(x, x_cs, res, res_cs, y, y_cs, gamma, beta, stats, B, hw, C, G, eps, relu, slope, dtype,
                                                scratch, self.st()), "srcgan_gn_forward")

    def forward(self, x, res, y, gamma, beta, B, hw, C, G, relu=0, slope=0.0):
        """x, res, y: operands (groupnorm_ref.make_op); -> stats [B, G, 2]; the 8 floats behind it must keep the sentinel"""
        p = lambda t: None if t is None else t.data_ptr()
        stats = torch.full((B * G * 2 + 8,), SENT, device="cuda")
        scr = self.scratch(B, C)
        self.forward_raw(R.ptr_of(x), x[1], None if res is None else R.ptr_of(res), 0 if res is None else res[1], R.ptr_of(y), y[1],
                         p(gamma), p(beta), stats.data_ptr(), B, hw, C, G, relu, slope, self.N.dtype_id(x[0].dtype), scr.data_ptr())
        assert bool((stats[B * G * 2:] == SENT).all()), "wrote past the statistics"
        return stats[:B * G * 2].view(B, G, 2)

    def backward_raw(self, dy, dy_cs, yact, ya_cs, x, x_cs, gamma, stats, dx, dx_cs, dres, dr_cs, dres_acc, dgamma, dbeta, acc, slope,
                     B, hw, C, G, dtype, scratch):
        self.N.check(self.lib.srcgan_gn_backward(dy, dy_cs, yact, ya_cs, x, x_cs, gamma, stats, dx, dx_cs, dres, dr_cs, dres_acc, dgamma, dbeta,
                                                 acc, slope, B, hw, C, G, dtype, scratch, self.st()), "srcgan_gn_backward")

    def backward(self, dy, yact, x, gamma, stats, dx, dres, B, hw, C, G, slope=0.0, dres_acc=0, dgamma=None, dbeta=None, acc=0):
        p = lambda t: None if t is None else t.data_ptr()
        o = lambda op: (None, 0) if op is None else (R.ptr_of(op), op[1])
        scr = self.scratch(B, C)
        st = stats.contiguous()
        self.backward_raw(R.ptr_of(dy), dy[1], *o(yact), R.ptr_of(x), x[1], p(gamma), st.data_ptr(), R.ptr_of(dx), dx[1], *o(dres), dres_acc,
                          p(dgamma), p(dbeta), acc, slope, B, hw, C, G, self.N.dtype_id(x[0].dtype), scr.data_ptr())


@pytest.fixture(scope="module")
def L():
    return Lib()


def dev_op(vals, cs=None, coff=0):
    return R.make_op(vals.cuda(), cs, coff)


def unchanged(op, copy):
    return same_bits(op[0], copy)


# --------------------------------------------------------------------------- 1. statistics
@pytest.mark.parametrize("dt", DTS)
def test_statistics_against_float64(L, dt):
    """stats[b][g] = {mean, rstd} against float64 of the stored x, on the shapes of groupnorm_ref.stat_shapes (what each reaches
    is in the table) with the images' means at 0, 30 and 1000 standard deviations and with channel offsets that differ inside a
    group.  y of the same call (gamma, beta given, no activation) is held to the forward bound, so the apply kernel runs at
    every shape too -- its second grid-stride trip at B = 16."""
    tdt = TDT[dt]
    worst = dict(mean=(0.0, None), rstd=(0.0, None), y=(0.0, None))
    for si, (B, hw, C, G, why) in enumerate(R.stat_shapes(dt)):
        gamma, beta = R.affine(C, 40 + si, "cuda")
        for vi, variant in enumerate(R.STAT_VARIANTS):
            x = dev_op(R.stat_data(B, hw, C, variant, tdt, 1000 + 10 * si + vi))
            x0 = x[0].clone()
            y = R.blank_op(B * hw, C, tdt, "cuda")
            stats = L.forward(x, None, y, gamma, beta, B, hw, C, G)
            assert unchanged(x, x0)
            mean64, var64 = R.stats64(R.vals_of(x, C), B, hw, C, G)
            ok, um, ur = check_stats(stats, mean64, var64)
            name = f"B{B} hw{hw} C{C} G{G} {variant}"
            assert ok, f"{dt} {name} ({why}): mean {um:.2f}, rstd {ur:.2f} units of 2^-24, bound {R.STAT_UNITS}"
            ref, n = R.ref_forward(R.vals_of(x, C), None, gamma, beta, stats, B, hw, C, G, 0, 0.0)
            oky, uy = within(R.vals_of(y, C), ref, EPS_T[dt] * n)
            assert oky, f"{dt} {name}: y is {uy:.3f} of its bound"
            for k, v in (("mean", um), ("rstd", ur), ("y", uy)):
                if v > worst[k][0]:
                    worst[k] = (v, name)
    report("statistics", dt, mean_units=worst["mean"][0], mean_case=worst["mean"][1], rstd_units=worst["rstd"][0], rstd_case=worst["rstd"][1],
           y_of_bound=worst["y"][0], y_case=worst["y"][1])


@pytest.mark.parametrize("dt", DTS)
def test_constant_group(L, dt):
    """Every value is 1000.1 (as stored: 1000 in bf16 and fp16): the mean must be that f32 number exactly -- every shifted sum and
    every M2 is exactly 0 -- rstd = 1 / sqrt(eps) within the bound, and y == beta (0 without beta) exactly."""
    tdt = TDT[dt]
    for B, hw, C, G in ((2, 289, 512 if dt == "fp32" else 1024, 32), (2, 5, 64, 32), (2, 1, 64, 64), (2, 4290, 64, 32)):
        gamma, beta = R.affine(C, 7, "cuda")
        x = dev_op(torch.full((B * hw, C), 1000.1).to(tdt))
        x0 = x[0].clone()
        c = float(x[0][0, 0])
        for bt in (beta, None):
            y = R.blank_op(B * hw, C, tdt, "cuda", C + EPP[dt], EPP[dt])
            stats = L.forward(x, None, y, gamma, bt, B, hw, C, G)
            assert bool((stats[..., 0] == c).all()), (dt, hw, C, stats[..., 0].double().sub(c).abs().max())
            ok, _, ur = check_stats(stats, torch.full((B, G), c, dtype=torch.float64, device="cuda"), torch.zeros(B, G, dtype=torch.float64, device="cuda"))
            assert ok, ur
            want = (beta if bt is not None else torch.zeros(C, device="cuda")).to(tdt).expand(B * hw, C)
            assert torch.equal(R.vals_of(y, C), want) and R.outside_untouched(y, C)
        assert unchanged(x, x0)


@pytest.mark.parametrize("dt", DTS)
def test_every_pixel_counted_once(L, dt):
    """x = 0 except one sample of 2^10: mean = 2^10 / n, var = 2^20 (n - 1) / n^2 in its group and 0 elsewhere, to the statistics'
    bound -- a pixel dropped or counted twice is a 100 % error.  The sample visits the first and last pixel of every block's
    range, the last pixel of the image, a pixel of the last image and every lane of one 16-byte channel vector."""
    tdt = TDT[dt]
    for B, hw, C, G in R.spike_shapes(dt):
        n = hw * (C // G)
        x = dev_op(torch.zeros(B * hw, C, dtype=tdt))
        y = R.blank_op(B * hw, C, tdt, "cuda")
        got, changed = [], []
        for b, p, c in R.spike_positions(dt, B, hw, C):
            x[0][b * hw + p, c] = 1024.0
            x0 = x[0].clone()
            got.append(((b, p, c), L.forward(x, None, y, None, None, B, hw, C, G).clone()))
            changed.append(not unchanged(x, x0))
            x[0][b * hw + p, c] = 0.0
        assert not any(changed), "srcgan_gn_forward changed x"
        for (b, p, c), stats in got:
            mean64 = torch.zeros(B, G, dtype=torch.float64, device="cuda")
            var64 = torch.zeros_like(mean64)
            mean64[b, c // (C // G)] = 1024.0 / n
            var64[b, c // (C // G)] = 2.0 ** 20 * (n - 1) / n ** 2
            ok, um, ur = check_stats(stats, mean64, var64)
            assert ok, f"{dt} hw{hw} C{C}: sample at image {b}, pixel {p}, channel {c}: mean {um:.3g}, rstd {ur:.3g} units"


@pytest.mark.parametrize("dt", DTS)
def test_batch_independence_and_repeatability(L, dt):
    """Image b of a B = 3 call has the bits of a B = 1 call on it (statistics and y), and a second call gives the same bits."""
    tdt = TDT[dt]
    for hw, C, G in ((289, 512 if dt == "fp32" else 1024, 32), (5, 64, 64), (300, 64, 32)):
        B = 3
        gamma, beta = R.affine(C, 9, "cuda")
        x = dev_op(R.stat_data(B, hw, C, "chan", tdt, 77), C + EPP[dt], 0)
        y, y2 = R.blank_op(B * hw, C, tdt, "cuda"), R.blank_op(B * hw, C, tdt, "cuda")
        s = L.forward(x, None, y, gamma, beta, B, hw, C, G, 1, SLOPE)
        s2 = L.forward(x, None, y2, gamma, beta, B, hw, C, G, 1, SLOPE)
        assert same_bits(s, s2) and same_bits(y[0], y2[0])
        for b in range(B):
            xb = (x[0][b * hw:(b + 1) * hw], x[1], x[2])
            yb = R.blank_op(hw, C, tdt, "cuda")
            sb = L.forward(xb, None, yb, gamma, beta, 1, hw, C, G, 1, SLOPE)
            assert same_bits(sb[0], s[b]) and same_bits(yb[0], y[0][b * hw:(b + 1) * hw]), (dt, hw, C, b)


# --------------------------------------------------------------------------- 2. forward apply
@pytest.mark.parametrize("dt", DTS)
def test_forward_apply_elementwise(L, dt):
    """y against float64 act((x - mu) r gamma + beta + res) with the call's own f32 statistics, element by element, for relu 0 / 1,
    slope 0 / 0.2, res null / given and gamma / beta null, one null, both given; x, res and y each in a channel stride of its own
    (C + 2, 3, 4 vectors) and one or two vectors into its buffer.  Where relu meets slope 0 the zeros carry the sign of the
    header's expression (v * 0 = -0 for v < 0).  Everything outside y's slice keeps the sentinel; x and res are unchanged."""
    tdt, epp = TDT[dt], EPP[dt]
    worst = 0.0
    for B, hw, C, G in ((2, 37, 64, 32), (2, 5, 64, 64)):
        gamma, beta = R.affine(C, 11, "cuda")
        gen = torch.Generator().manual_seed(12)
        x = dev_op(R.apply_data(B, hw, C, G, tdt, 13), C + 2 * epp, epp)
        resop = dev_op(torch.randn(B * hw, C, generator=gen).to(tdt), C + 3 * epp, 2 * epp)
        x0, r0 = x[0].clone(), resop[0].clone()
        mean64, var64 = R.stats64(R.vals_of(x, C), B, hw, C, G)
        assert float((R.vals_of(x, C).double().view(B, hw, G, -1) - mean64[:, None, :, None]).abs().min()) >= 0.125
        for relu in (0, 1):
            for slope in (0.0, SLOPE):
                for res in (None, resop):
                    for gm, bt in ((None, None), (gamma, None), (None, beta), (gamma, beta)):
                        y = R.blank_op(B * hw, C, tdt, "cuda", C + 4 * epp, epp)
                        stats = L.forward(x, res, y, gm, bt, B, hw, C, G, relu, slope)
                        what = (dt, hw, G, relu, slope, res is not None, gm is not None, bt is not None)
                        assert check_stats(stats, mean64, var64)[0], what
                        ref, n = R.ref_forward(R.vals_of(x, C), None if res is None else R.vals_of(res, C), gm, bt, stats, B, hw, C, G, relu, slope)
                        ok, u = within(R.vals_of(y, C), ref, EPS_T[dt] * n)
                        assert ok, (what, u)
                        assert R.outside_untouched(y, C), what
                        if relu and slope == 0.0:
                            yv = R.vals_of(y, C)
                            z = yv == 0
                            assert bool(z.any()) and torch.equal(torch.signbit(yv[z]), torch.signbit(ref[z])), what
                        worst = max(worst, u)
        assert unchanged(x, x0) and unchanged(resop, r0)
    report("forward apply", dt, worst_of_bound=worst, eps=EPS_T[dt])


# --------------------------------------------------------------------------- 3. backward, exact
def _bwd_ops(k, dt, inplace_cs=None):
    """dy, yact, x as operands in strides of their own; blank dx and dres"""
    C, epp, npix, tdt = k["C"], EPP[dt], k["B"] * k["hw"], TDT[dt]
    dy = dev_op(k["dy"], C + 2 * epp, epp)
    ya = None if k["yact"] is None else dev_op(k["yact"], C + 3 * epp, 2 * epp)
    x = dev_op(k["x"], C + epp, 0)
    dx = R.blank_op(npix, C, tdt, "cuda", C + 4 * epp, 2 * epp)
    dres = R.blank_op(npix, C, tdt, "cuda", C + 5 * epp, epp)
    return dy, ya, x, dx, dres


def _run_exact(L, dt, k, ref, what):
    """one exact case through every output form"""
    B, hw, C, G, tdt, slope = k["B"], k["hw"], k["C"], k["G"], TDT[dt], k["slope"]
    gamma = None if k["gamma"] is None else k["gamma"].cuda()
    stats = k["stats"].cuda()
    dy, ya, x, dx, dres = _bwd_ops(k, dt)
    copies = [t[0].clone() for t in (dy, x)] + ([ya[0].clone()] if ya is not None else [])
    dgamma, dbeta = torch.full((C + 8,), SENT, device="cuda"), torch.full((C + 8,), SENT, device="cuda")
    L.backward(dy, ya, x, gamma, stats, dx, dres, B, hw, C, G, slope, 0, dgamma, dbeta, 0)
    exp_dg, exp_db = ref["dgamma"].cuda(), ref["dbeta"].cuda()
    assert equal_cast(R.vals_of(dx, C), ref["dx"].cuda()) and R.outside_untouched(dx, C), (what, "dx")
    assert bits_cast(R.vals_of(dres, C), ref["dres"].cuda()) and R.outside_untouched(dres, C), (what, "dres")
    assert equal_cast(dgamma[:C], exp_dg) and equal_cast(dbeta[:C], exp_db), (what, "dgamma / dbeta")
    assert bool((dgamma[C:] == SENT).all()) and bool((dbeta[C:] == SENT).all()), what
    # accumulate onto integers: dres += g, dgamma += , dbeta +=
    gen = torch.Generator().manual_seed(5)
    old_r = torch.randint(-8, 9, (B * hw, C), generator=gen).float()
    old_g, old_b = torch.randint(-8, 9, (C,), generator=gen).float().cuda(), torch.randint(-8, 9, (C,), generator=gen).float().cuda()
    dres2 = dev_op(old_r.to(tdt), dres[1], dres[2])
    dx2 = R.blank_op(B * hw, C, tdt, "cuda", dx[1], dx[2])
    dg2, db2 = old_g.clone(), old_b.clone()
    L.backward(dy, ya, x, gamma, stats, dx2, dres2, B, hw, C, G, slope, 1, dg2, db2, 1)
    assert same_bits(dx2[0], dx[0]), (what, "dx of the accumulating call")
    assert equal_cast(R.vals_of(dres2, C), ref["dres"].cuda() + old_r.double().cuda()) and R.outside_untouched(dres2, C), (what, "dres +=")
    assert equal_cast(dg2, exp_dg + old_g.double()) and equal_cast(db2, exp_db + old_b.double()), (what, "dgamma / dbeta +=")
    # any one of dres, dgamma, dbeta null: the others as before
    for drop in ("dres", "dgamma", "dbeta"):
        dx3, dres3 = R.blank_op(B * hw, C, tdt, "cuda", dx[1], dx[2]), R.blank_op(B * hw, C, tdt, "cuda", dres[1], dres[2])
        dg3, db3 = torch.full((C,), SENT, device="cuda"), torch.full((C,), SENT, device="cuda")
        L.backward(dy, ya, x, gamma, stats, dx3, None if drop == "dres" else dres3, B, hw, C, G, slope, 0,
                   None if drop == "dgamma" else dg3, None if drop == "dbeta" else db3, 0)
        assert same_bits(dx3[0], dx[0]), (what, drop)
        assert same_bits(dres3[0], torch.full_like(dres3[0], SENT) if drop == "dres" else dres[0]), (what, drop)
        assert same_bits(dg3, torch.full_like(dg3, SENT) if drop == "dgamma" else dgamma[:C]), (what, drop)
        assert same_bits(db3, torch.full_like(db3, SENT) if drop == "dbeta" else dbeta[:C]), (what, drop)
    for t, c in zip((dy, x) + ((ya,) if ya is not None else ()), copies):
        assert unchanged(t, c), (what, "an input changed")
    return dx


@pytest.mark.parametrize("dt", DTS)
def test_backward_exact(L, dt):
    """Crafted statistics (mean an integer, rstd in {1/2, 1, 2}), x integers within 8 of the mean, dy integers in [-4, 4], gamma in
    {-1, 1/2, 1, 2} or null, yact in {-1, 0, 1} or null (the zeros tell > from >=), slope 0 and 1/2, hw * cpg a power of two:
    dx equals the float64 reference cast once, dres its bits (slope 0 makes -0 of a negative dy), dgamma and dbeta equal it,
    plain and accumulated onto integers, and with any one of dres, dgamma, dbeta null."""
    for si, (B, hw, C, G) in enumerate(R.exact_bwd_shapes(dt)):
        for vi, (wg, wy, slope) in enumerate(((True, True, 0.5), (True, True, 0.0), (False, True, 0.5), (True, False, 0.0), (False, False, 0.0))):
            k = R.exact_bwd_case(B, hw, C, G, TDT[dt], 2000 + 10 * si + vi, wg, wy, slope)
            ref = R.ref_backward(k["dy"], k["yact"], k["x"], k["gamma"], k["stats"], slope, B, hw, C, G)
            R.exact_bwd_conditions(k, ref)
            _run_exact(L, dt, k, ref, (dt, B, hw, C, G, wg, wy, slope))


@pytest.mark.parametrize("dt", DTS)
def test_backward_in_place_over_dy(L, dt):
    """The discriminator's call (nets.hip, InstanceNorm2d): dx written over dy, yact null, G == C, gamma null, no parameter
    gradients, dy in a stride larger than C.  Both pointers are __restrict__ in gn_bwd_apply_k; the result must have the bits of
    the out-of-place call, on the exact case and on random data."""
    tdt, epp = TDT[dt], EPP[dt]
    for B, hw, C in ((3, 64, 64), (2, 4290, 64), (2, 5, 64)):
        k = R.exact_bwd_case(B, hw, C, C, tdt, 31, False, False, 0.0)       # yact null: the slope passed (0.2, as the caller does) is not used
        stats = k["stats"].cuda()
        for data in ("int", "normal"):
            dyv = k["dy"] if data == "int" else torch.randn(B * hw, C, generator=torch.Generator().manual_seed(3)).to(tdt)
            dy = dev_op(dyv, C + 2 * epp, epp)
            x = dev_op(k["x"], C + epp, 0)
            x0, dy0 = x[0].clone(), dy[0].clone()
            dx = R.blank_op(B * hw, C, tdt, "cuda", C + 2 * epp, epp)
            L.backward(dy, None, x, None, stats, dx, None, B, hw, C, C, 0.2)
            assert unchanged(dy, dy0) and unchanged(x, x0)
            if data == "int" and hw == 64:
                ref = R.ref_backward(k["dy"], None, k["x"], None, k["stats"], 0.2, B, hw, C, C)
                R.exact_bwd_conditions(k, ref)
                assert equal_cast(R.vals_of(dx, C), ref["dx"].cuda())
            L.backward(dy, None, x, None, stats, dy, None, B, hw, C, C, 0.2)
            assert same_bits(dy[0], dx[0]), (dt, B, hw, C, data)
            assert unchanged(x, x0)


@pytest.mark.parametrize("dt", DTS)
def test_backward_sums_exact_where_n_is_no_power_of_two(L, dt):
    """The empty-block shapes (and 3 and 5 pixels): 1 / (hw cpg) is not exact, but dbeta, dgamma and dres are still sums of
    integers and halves -- compared as bits, through the blocks that have no pixel."""
    for si, (B, hw, C, G) in enumerate(R.sum_only_bwd_shapes(dt)):
        k = R.exact_bwd_case(B, hw, C, G, TDT[dt], 2500 + si, True, True, 0.5)
        ref = R.ref_backward(k["dy"], k["yact"], k["x"], k["gamma"], k["stats"], 0.5, B, hw, C, G)
        R.exact_bwd_conditions(k, ref, sums_only=True)
        dy, ya, x, dx, dres = _bwd_ops(k, dt)
        dgamma, dbeta = torch.full((C + 8,), SENT, device="cuda"), torch.full((C + 8,), SENT, device="cuda")
        L.backward(dy, ya, x, k["gamma"].cuda(), k["stats"].cuda(), dx, dres, B, hw, C, G, 0.5, 0, dgamma, dbeta, 0)
        assert bits_cast(dgamma[:C], ref["dgamma"].cuda()) and bits_cast(dbeta[:C], ref["dbeta"].cuda()), (dt, hw, C)
        assert bits_cast(R.vals_of(dres, C), ref["dres"].cuda()) and R.outside_untouched(dres, C) and R.outside_untouched(dx, C)
        assert bool((dgamma[C:] == SENT).all()) and bool((dbeta[C:] == SENT).all())
        refc = R.ref_backward(R.vals_of(dy, C), R.vals_of(ya, C), R.vals_of(x, C), k["gamma"].cuda(), k["stats"].cuda(), 0.5, B, hw, C, G)
        ok, u = within(R.vals_of(dx, C), refc["dx"], (EPS_T[dt] + 512 * U32) * refc["n_dx"])
        assert ok, (dt, hw, C, u)


# --------------------------------------------------------------------------- 4. backward against float64
@pytest.mark.parametrize("dt", DTS)
def test_backward_against_float64(L, dt):
    """Random reals rounded to the storage type, the statistics and the activated output of the forward call (affine, residual,
    LeakyReLU 0.2): dx per element within (eps_T + 512 * 2^-24) N, dgamma / dbeta within 512 * 2^-24 * sum |terms|, dres the bits
    of dy * (y > 0 ? 1 : slope) in f32 cast once, and with dres_accumulate the bits of round(round(g) + old).  512 bounds the longest serial chain (asserted from the geometry)."""
    tdt = TDT[dt]
    worst = dict(dx=0.0, dgamma=0.0, dbeta=0.0)
    for si, (B, hw, C, G) in enumerate(R.f64_bwd_shapes(dt)):
        assert R.chain_length(dt, hw, C, G) < 512
        gen = torch.Generator().manual_seed(3000 + si)
        gamma, beta = R.affine(C, 50 + si, "cuda")
        x = dev_op(R.stat_data(B, hw, C, "chan", tdt, 3100 + si))
        res = dev_op(torch.randn(B * hw, C, generator=gen).to(tdt))
        dy = dev_op(torch.randn(B * hw, C, generator=gen).to(tdt))
        y = R.blank_op(B * hw, C, tdt, "cuda")
        stats = L.forward(x, res, y, gamma, beta, B, hw, C, G, 1, SLOPE)
        dx, dres = R.blank_op(B * hw, C, tdt, "cuda"), R.blank_op(B * hw, C, tdt, "cuda")
        dgamma, dbeta = torch.full((C,), SENT, device="cuda"), torch.full((C,), SENT, device="cuda")
        copies = [t[0].clone() for t in (dy, y, x)]
        L.backward(dy, y, x, gamma, stats, dx, dres, B, hw, C, G, SLOPE, 0, dgamma, dbeta, 0)
        for t, c in zip((dy, y, x), copies):
            assert unchanged(t, c)
        ref = R.ref_backward(dy[0], y[0], x[0], gamma, stats, SLOPE, B, hw, C, G)
        ok, u = within(dx[0], ref["dx"], (EPS_T[dt] + 512 * U32) * ref["n_dx"])
        assert ok, (dt, B, hw, C, G, "dx", u)
        okg, ug = within(dgamma, ref["dgamma"], 512 * U32 * ref["n_dgamma"])
        okb, ub = within(dbeta, ref["dbeta"], 512 * U32 * ref["n_dbeta"])
        assert okg and okb, (dt, B, hw, C, G, ug, ub)
        gf = dy[0].float() * torch.where(y[0].float() > 0, torch.ones((), device="cuda"), torch.full((), SLOPE, device="cuda"))
        assert same_bits(dres[0], gf.to(tdt)), (dt, B, hw, C, G, "dres")
        # dres_accumulate on values that are not representable sums: g is rounded to the storage type, then added to the old value
        # in f32 and rounded again (the header's contract; one rounding of g + old would differ in 16 bits)
        old_r = torch.randn(B * hw, C, generator=gen).to(tdt).cuda()
        dres2, dx2 = (old_r.clone(), C, 0), R.blank_op(B * hw, C, tdt, "cuda")
        L.backward(dy, y, x, gamma, stats, dx2, dres2, B, hw, C, G, SLOPE, 1)
        assert same_bits(dres2[0], (gf.to(tdt).float() + old_r.float()).to(tdt)), (dt, B, hw, C, G, "dres +=")
        assert same_bits(dx2[0], dx[0])
        worst = dict(dx=max(worst["dx"], u), dgamma=max(worst["dgamma"], ug), dbeta=max(worst["dbeta"], ub))
    report("backward vs float64 (fraction of the bound)", dt, **worst)


def _autograd(x, res, gamma, beta, g_of_y, B, hw, C, G, instance):
    """float64 y = leaky_relu(norm(x) + res) and dx for the upstream gradient g_of_y(mask) arriving at the pre-activation"""
    x64 = x.double().view(B, hw, C).permute(0, 2, 1).contiguous().requires_grad_(True)
    r64 = res.double().view(B, hw, C).permute(0, 2, 1)
    if instance:
        pre = F.instance_norm(x64, eps=R.f32(EPS)) + r64
    else:
        pre = F.group_norm(x64, G, gamma.double(), beta.double(), eps=R.f32(EPS)) + r64
    y = F.leaky_relu(pre, R.f32(SLOPE)).detach()
    pre.backward(g_of_y.double().view(B, hw, C).permute(0, 2, 1))
    back = lambda t: t.permute(0, 2, 1).reshape(B * hw, C)
    return back(y), back(x64.grad)


@pytest.mark.parametrize("instance", [False, True])
@pytest.mark.parametrize("dt", DTS)
def test_chain_against_float64_autograd(L, dt, instance):
    """srcgan_gn_forward -> srcgan_gn_backward (with the forward's statistics and its stored y as the mask) against float64
    autograd of F.group_norm + residual + F.leaky_relu -- and, with G == C and no affine part, of F.instance_norm: y and dx per
    element within (eps_T + 1e-5) N, N of the two element-wise bounds with float64 statistics (1e-5 is for the statistics)."""
    tdt = TDT[dt]
    B, hw, C = 2, 35, 64
    G = C if instance else 32
    gen = torch.Generator().manual_seed(4000 + instance)
    gamma, beta = (None, None) if instance else R.affine(C, 60, "cuda")
    x = dev_op((torch.randn(B * hw, C, generator=gen) * 1.5 + 0.5).to(tdt))
    res = dev_op(torch.randn(B * hw, C, generator=gen).to(tdt))
    dy = dev_op(torch.randn(B * hw, C, generator=gen).to(tdt))
    y, dx = R.blank_op(B * hw, C, tdt, "cuda"), R.blank_op(B * hw, C, tdt, "cuda")
    stats = L.forward(x, res, y, gamma, beta, B, hw, C, G, 1, SLOPE)
    L.backward(dy, y, x, gamma, stats, dx, None, B, hw, C, G, SLOPE)
    g = dy[0].double() * torch.where(y[0].double() > 0, 1.0, R.f32(SLOPE))
    y_ref, dx_ref = _autograd(x[0], res[0], gamma, beta, g, B, hw, C, G, instance)
    m64, v64 = R.stats64(x[0], B, hw, C, G)
    s64 = torch.stack([m64, R.rstd64(v64)], -1)
    _, n_fwd = R.ref_forward(x[0], res[0], gamma, beta, s64, B, hw, C, G, 1, SLOPE)
    rb = R.ref_backward(dy[0], y[0], x[0], gamma, s64, SLOPE, B, hw, C, G)
    assert float((rb["dx"] - dx_ref).abs().max()) < 1e-9, "groupnorm_ref.ref_backward disagrees with autograd"
    ok, u = within(y[0], y_ref, (EPS_T[dt] + 1e-5) * n_fwd)
    assert ok, (dt, instance, "y", u)
    okb, ub = within(dx[0], dx_ref, (EPS_T[dt] + 1e-5) * rb["n_dx"])
    assert okb, (dt, instance, "dx", ub)
    report(f"chain instance={instance} (fraction of the bound)", dt, y=u, dx=ub)


# --------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("dt", DTS)
def test_refusals(L, dt):
    """Each of these is an error whose message names the entry point, and nothing is written: C / epp not dividing 256 (C = 96 in
    fp32: 24 vectors; 6 vectors in 16 bits), C = 1032, G not dividing C, a channel stride that is no multiple of epp, a bad dtype,
    and each required pointer null."""
    tdt, epp, did = TDT[dt], EPP[dt], L.N.dtype_id(TDT[dt])
    B, hw = 2, 3
    Cmax = 1040
    xb = torch.zeros(B * hw, Cmax + 8, dtype=tdt, device="cuda")
    out = [torch.full((B * hw, Cmax + 8), SENT, dtype=tdt, device="cuda") for _ in range(2)]
    f32s = [torch.full((2 * Cmax,), SENT, device="cuda") for _ in range(3)]      # stats / dgamma / dbeta
    ones = torch.ones(Cmax, device="cuda")
    scr = L.scratch(B, Cmax)
    X, Y, D, S, SC = xb.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), f32s[0].data_ptr(), scr.data_ptr()

    def fwd(C=64, G=32, cs=None, dtype=did, x=X, y=Y, stats=S, scratch=SC, res=None, res_cs=0, x_cs=None, y_cs=None):
        cs = cs or C
        L.forward_raw(x, x_cs or cs, res, res_cs, y, y_cs or cs, ones.data_ptr(), ones.data_ptr(), stats, B, hw, C, G, 0, 0.0, dtype, scratch)

    def bwd(C=64, G=32, cs=None, dtype=did, dy=X, x=X, stats=S, dx=Y, scratch=SC, dres=D, **kw):
        cs = cs or C
        g = lambda n: kw.get(n, cs)
        L.backward_raw(dy, g("dy_cs"), X, g("ya_cs"), x, g("x_cs"), ones.data_ptr(), stats, dx, g("dx_cs"), dres, g("dr_cs"), 0,
                       f32s[1].data_ptr(), f32s[2].data_ptr(), 0, 0.0, B, hw, C, G, dtype, scratch)

    bad_c = 96 if dt == "fp32" else 48
    cases = [dict(C=bad_c, G=bad_c // epp), dict(C=1032, G=1), dict(C=64, G=24), dict(dtype=7)]
    fcases = cases + [dict(x_cs=64 + epp // 2), dict(y_cs=64 + epp // 2), dict(res=X, res_cs=64 + epp // 2),
                      dict(x=None), dict(y=None), dict(stats=None), dict(scratch=None)]
    bcases = cases + [dict(dy_cs=64 + epp // 2), dict(ya_cs=64 + epp // 2), dict(x_cs=64 + epp // 2), dict(dx_cs=64 + epp // 2), dict(dr_cs=64 + epp // 2),
                      dict(dy=None), dict(x=None), dict(stats=None), dict(dx=None), dict(scratch=None)]
    for fn, name, cs_ in ((fwd, "srcgan_gn_forward", fcases), (bwd, "srcgan_gn_backward", bcases)):
        for kw in cs_:
            with pytest.raises(RuntimeError, match=name):
                fn(**kw)
    torch.cuda.synchronize()
    for t in out + f32s:
        assert bool((t == SENT).all())
    fwd()                   # the plain arguments are accepted
    bwd()
    torch.cuda.synchronize()
