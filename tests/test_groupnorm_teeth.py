"""The comparisons of tests/test_gpu_groupnorm.py and tests/test_gpu_resample.py have teeth: on the CPU, each reference is compared,
through the GPU files' own comparison functions, with a copy of itself that makes one of the mistakes those tests are there to
catch.  Every such comparison must fail (and the unperturbed one must pass).  The file also runs groupnorm_ref's exactness
conditions for every exact case, holds the numpy-f32 restatement of the statistics to half of the device's bound on every
statistics case, and checks that the shapes listed as having an empty block have one.  No kernel runs here."""
import pytest
import torch
import torch.nn.functional as F

import groupnorm_ref as R
import test_gpu_groupnorm as T
import test_gpu_resample as S

DTS = R.DTS


# --------------------------------------------------------------------------- the case tables say what they claim
def test_listed_shapes_have_an_empty_trailing_block():
    assert R.empty_blocks("fp32", 105, 1024) == [12] and R.geometry("fp32", 105, 1024)["PL"] == 1
    assert R.empty_blocks("fp32", 289, 512) == [17]
    for dt in ("bf16", "fp16"):
        assert R.empty_blocks(dt, 289, 1024) == [17]
    for hw in (81, 89, 90, 97, 98, 99):
        assert R.empty_blocks("fp32", hw, 1024)
    for hw in (305, 306, 321):
        assert R.empty_blocks("fp32", hw, 512) and R.empty_blocks("bf16", hw, 1024)
    # the other branches the table names
    assert R.geometry("bf16", 5, 64)["PL"] == 32 and R.geometry("bf16", 3, 8)["VG"] == 1
    for dt, C in (("fp32", 64), ("bf16", 128), ("fp16", 128)):
        g = R.geometry(dt, 66 * 65, C)
        assert 66 * 65 * g["VG"] // 2048 > R.GN_MAXBLK == g["nblk"] and g["ranges"][-1][1] - g["ranges"][-1][0] < g["per"]
        assert 16 * 66 * 65 * g["VG"] > 4096 * 256
    assert R.geometry("fp32", 256, 256)["nblk"] == 8 and not R.empty_blocks("fp32", 256, 256)
    for dt in DTS:
        for B, hw, C, G in R.f64_bwd_shapes(dt):
            assert R.chain_length(dt, hw, C, G) < 512


@pytest.mark.parametrize("dt", DTS)
def test_f32_restatement_uses_half_the_bound(dt):
    """the statistics algorithm in numpy float32 stays within 4 of the bound's 8 units on every statistics case"""
    worst = 0.0
    for si, (B, hw, C, G, _) in enumerate(R.stat_shapes(dt)):
        for vi, variant in enumerate(R.STAT_VARIANTS):
            x = R.stat_data(B, hw, C, variant, R.TDT[dt], 1000 + 10 * si + vi)
            mean64, var64 = R.stats64(x, B, hw, C, G)
            um, ur = R.stat_units(R.stats_f32_model(x, dt, B, hw, C, G), mean64, var64)
            assert float(um.max()) <= 4 and float(ur.max()) <= 4, (dt, B, hw, C, G, variant, float(um.max()), float(ur.max()))
            worst = max(worst, float(um.max()), float(ur.max()))
    print(f"[gn] numpy-f32 restatement {dt}: worst {worst:.2f} units")


@pytest.mark.parametrize("dt", DTS)
def test_exact_cases_are_exact(dt):
    for si, (B, hw, C, G) in enumerate(R.exact_bwd_shapes(dt)):
        for vi, (wg, wy, slope) in enumerate(((True, True, 0.5), (True, True, 0.0), (False, True, 0.5), (True, False, 0.0), (False, False, 0.0))):
            k = R.exact_bwd_case(B, hw, C, G, R.TDT[dt], 2000 + 10 * si + vi, wg, wy, slope)
            R.exact_bwd_conditions(k, R.ref_backward(k["dy"], k["yact"], k["x"], k["gamma"], k["stats"], slope, B, hw, C, G))
    for si, (B, hw, C, G) in enumerate(R.sum_only_bwd_shapes(dt)):
        k = R.exact_bwd_case(B, hw, C, G, R.TDT[dt], 2500 + si, True, True, 0.5)
        R.exact_bwd_conditions(k, R.ref_backward(k["dy"], k["yact"], k["x"], k["gamma"], k["stats"], 0.5, B, hw, C, G), sums_only=True)
    k = R.exact_bwd_case(3, 64, 64, 64, R.TDT[dt], 31, False, False, 0.0)
    R.exact_bwd_conditions(k, R.ref_backward(k["dy"], None, k["x"], None, k["stats"], 0.2, 3, 64, 64, 64))
    for B, hw, C, G in ((2, 37, 64, 32), (2, 5, 64, 64)):
        x = R.apply_data(B, hw, C, G, R.TDT[dt], 13)
        mean64, _ = R.stats64(x, B, hw, C, G)
        assert float((x.double().view(B, hw, G, -1) - mean64[:, None, :, None]).abs().min()) >= 0.125


def test_reference_backward_is_autograd():
    """groupnorm_ref.ref_backward against float64 autograd of group_norm + residual + leaky_relu"""
    B, hw, C, G = 2, 35, 64, 32
    gen = torch.Generator().manual_seed(1)
    x, res, dy = (torch.randn(B * hw, C, generator=gen) for _ in range(3))
    gamma, beta = R.affine(C, 60)
    m, v = R.stats64(x, B, hw, C, G)
    s64 = torch.stack([m, R.rstd64(v)], -1)
    y, _ = R.ref_forward(x, res, gamma, beta, s64, B, hw, C, G, 1, R.SLOPE)
    g = dy.double() * torch.where(y > 0, 1.0, R.f32(R.SLOPE))
    y_ref, dx_ref = T._autograd(x, res, gamma, beta, g, B, hw, C, G, False)
    rb = R.ref_backward(dy, y, x, gamma, s64, R.SLOPE, B, hw, C, G)
    assert float((y - y_ref).abs().max()) < 1e-12 and float((rb["dx"] - dx_ref).abs().max()) < 1e-12


# --------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("dt", DTS)
def test_statistics_comparison_notices(dt):
    """one pixel dropped, the last block's range dropped, hw for hw * cpg in the variance -- on the data whose mean is within a
    few standard deviations of 0: the bounds grow with |mean| / sd, and at 1000 standard deviations one pixel in 17 160 samples
    (a change of 6e-5 / sd) is inside them, which is why the counting test (test_every_pixel_counted_once) exists"""
    for si, (B, hw, C, G, _) in enumerate(R.stat_shapes(dt)):
        for variant in ("mean0", "chan"):
            x = R.stat_data(B, hw, C, variant, R.TDT[dt], 1000 + 10 * si)
            mean64, var64 = R.stats64(x, B, hw, C, G)
            assert T.check_stats(R.stats_tensor(mean64, var64), mean64, var64)[0]
            defects = (["drop_pixel"] if hw > 1 else []) + (["drop_last_block"] if R.geometry(dt, hw, C)["nblk"] > 1 else []) + (["n_is_hw"] if G < C else [])
            for d in defects:
                if d == "n_is_hw" and float(var64.max()) == 0:
                    continue
                assert not T.check_stats(R.stats_tensor(*R.stats64(x, B, hw, C, G, d, dt)), mean64, var64)[0], (dt, B, hw, C, G, variant, d)


# --------------------------------------------------------------------------- forward
@pytest.mark.parametrize("dt", DTS)
def test_forward_comparison_notices(dt):
    """a group index off by one at a group boundary; x's channel offset shifted by one vector"""
    tdt, epp = R.TDT[dt], R.EPP[dt]
    B, hw, C, G = 2, 37, 64, 32
    gamma, beta = R.affine(C, 11)
    x = R.make_op(R.apply_data(B, hw, C, G, tdt, 13), C + 2 * epp, 0)
    x[0][:, C:] = x[0][:, :2 * epp] + 0.25                      # the shifted view reads data, not the sentinel
    stats = R.stats_tensor(*R.stats64(R.vals_of(x, C), B, hw, C, G))
    for relu, slope in ((0, 0.0), (1, R.SLOPE)):
        ref, n = R.ref_forward(R.vals_of(x, C), None, gamma, beta, stats, B, hw, C, G, relu, slope)
        assert T.within(ref.float().to(tdt), ref, R.EPS_T[dt] * n)[0]
        bad, _ = R.ref_forward(R.vals_of(x, C), None, gamma, beta, stats, B, hw, C, G, relu, slope, "group_off_by_one")
        assert not T.within(bad.float().to(tdt), ref, R.EPS_T[dt] * n)[0]
        bad, _ = R.ref_forward(R.vals_of(x, C, epp), None, gamma, beta, stats, B, hw, C, G, relu, slope)
        assert not T.within(bad.float().to(tdt), ref, R.EPS_T[dt] * n)[0]
        nan = ref.float().to(tdt).clone()
        nan[3, 5] = float("nan")                                    # one NaN element (a scratch slot read before it was written)
        assert not T.within(nan, ref, R.EPS_T[dt] * n)[0]


# --------------------------------------------------------------------------- backward
@pytest.mark.parametrize("dt", DTS)
def test_backward_exact_comparison_notices(dt):
    """>= for > in the mask, gamma applied to dres, the xhat term of dx dropped, += for = in dgamma, a channel offset shifted"""
    tdt, epp = R.TDT[dt], R.EPP[dt]
    for B, hw, C, G in ((2, 16, 64, 32), (2, 256, 256, 32)):
        k = R.exact_bwd_case(B, hw, C, G, tdt, 2000, True, True, 0.5)
        args = lambda **kw: (kw.get("dy", k["dy"]), k["yact"], kw.get("x", k["x"]), k["gamma"], k["stats"], 0.5, B, hw, C, G)
        ref = R.ref_backward(*args())
        cast = lambda t: t.float().to(tdt)
        assert T.equal_cast(cast(ref["dx"]), ref["dx"]) and T.bits_cast(cast(ref["dres"]), ref["dres"]) and T.equal_cast(ref["dgamma"].float(), ref["dgamma"])
        ge = R.ref_backward(*args(), defect="ge_mask")
        assert not T.equal_cast(cast(ge["dx"]), ref["dx"]) and not T.bits_cast(cast(ge["dres"]), ref["dres"])
        assert not T.equal_cast(ge["dgamma"].float(), ref["dgamma"]) and not T.equal_cast(ge["dbeta"].float(), ref["dbeta"])
        assert not T.bits_cast(cast(R.ref_backward(*args(), defect="gamma_on_dres")["dres"]), ref["dres"])
        assert not T.equal_cast(cast(R.ref_backward(*args(), defect="no_xhat_term")["dx"]), ref["dx"])
        old = torch.randint(-8, 9, (C,), generator=torch.Generator().manual_seed(5)).double()
        assert not T.equal_cast((old + ref["dgamma"]).float(), ref["dgamma"])            # accumulate = 0 must overwrite
        assert T.equal_cast((old + ref["dgamma"]).float(), ref["dgamma"] + old)
        for name in ("dy", "x"):                                                        # one operand read one vector further on
            op = R.make_op(k[name], C + epp, 0)
            op[0][:, C:] = op[0][:, :epp] + 1
            sh = R.ref_backward(*args(**{name: R.vals_of(op, C, epp)}))
            assert not T.equal_cast(cast(sh["dx"]), ref["dx"]) and not T.equal_cast(sh["dgamma"].float(), ref["dgamma"]), name
        # slope 0: a negative dy under the mask is -0, and the bit comparison of dres sees a +0 in its place
        k0 = R.exact_bwd_case(B, hw, C, G, tdt, 2001, True, True, 0.0)
        r0 = R.ref_backward(k0["dy"], k0["yact"], k0["x"], k0["gamma"], k0["stats"], 0.0, B, hw, C, G)
        plus = cast(r0["dres"]).clone()
        plus[plus == 0] = 0.0
        assert T.equal_cast(plus, r0["dres"]) and not T.bits_cast(plus, r0["dres"])


@pytest.mark.parametrize("dt", DTS)
def test_backward_float64_comparison_notices(dt):
    """the same defects on random reals, through the per-element bound"""
    tdt, epp = R.TDT[dt], R.EPP[dt]
    B, hw, C, G = 2, 5, 64, 32
    gen = torch.Generator().manual_seed(9)
    gamma, beta = R.affine(C, 50)
    x = R.stat_data(B, hw, C, "chan", tdt, 3100)
    dy, yact = torch.randn(B * hw, C, generator=gen).to(tdt), torch.randn(B * hw, C, generator=gen).to(tdt)
    yact.view(-1)[::5] = 0.0
    stats = R.stats_tensor(*R.stats64(x, B, hw, C, G))
    ref = R.ref_backward(dy, yact, x, gamma, stats, R.SLOPE, B, hw, C, G)
    bound = (R.EPS_T[dt] + 512 * R.U32) * ref["n_dx"]
    cast = lambda t: t.float().to(tdt)
    assert T.within(cast(ref["dx"]), ref["dx"], bound)[0]
    for d in ("ge_mask", "no_xhat_term"):
        bad = R.ref_backward(dy, yact, x, gamma, stats, R.SLOPE, B, hw, C, G, d)
        assert not T.within(cast(bad["dx"]), ref["dx"], bound)[0], d
    ge = R.ref_backward(dy, yact, x, gamma, stats, R.SLOPE, B, hw, C, G, "ge_mask")
    assert not T.within(ge["dgamma"].float(), ref["dgamma"], 512 * R.U32 * ref["n_dgamma"])[0]
    assert not T.within(ge["dbeta"].float(), ref["dbeta"], 512 * R.U32 * ref["n_dbeta"])[0]
    assert T.within(ref["dgamma"].float(), ref["dgamma"], 512 * R.U32 * ref["n_dgamma"])[0]
    # statistics with one pixel dropped, fed to the backward: dx leaves its bound as well
    bad_stats = R.stats_tensor(*R.stats64(x, B, hw, C, G, "drop_pixel"))
    assert not T.within(cast(R.ref_backward(dy, yact, x, gamma, bad_stats, R.SLOPE, B, hw, C, G)["dx"]), ref["dx"], bound)[0]


# --------------------------------------------------------------------------- the resamplers
@pytest.mark.parametrize("up", S.UPS)
def test_bilinear_reference_and_its_teeth(up):
    """bilinear_explicit is F.interpolate in float64; without the clamp at 0, without the clamp of the upper neighbour, or with
    the two weights swapped it is not, by the exact comparison and by the per-element bound"""
    for i, (H, W) in enumerate(S.UP_SIZES):
        src, real = S.int_data(3, H, W, 10 * up + i), S.real_data(3, H, W, 100 * up + i)
        ref, _ = S.ref_bilinear_up(src, up)
        rref, n = S.ref_bilinear_up(real, up)
        assert float((S.bilinear_explicit(src, up) - ref).abs().max()) < 1e-12
        assert S.within(S.bilinear_explicit(real, up).float(), rref, 4 * S.U32 * n)[0]
        assert S.within(S.bilinear_explicit(real, up).float(), rref, S.bilinear_bound(n, real))[0]
        nan = rref.float().clone()
        nan[0, 0, 0] = float("nan")
        assert not S.within(nan, rref, S.bilinear_bound(n, real))[0] and not S.exact(nan, rref)
        if up in (1, 2, 4, 8):
            assert S.exact(S.bilinear_explicit(src, up).float(), ref)
        if up == 1 or (H, W) == (1, 1):
            continue                         # every sample sits on a pixel: the defects change nothing
        for d in ("no_clamp_at_0", "no_border_clamp", "weights_swapped"):
            assert not S.exact(S.bilinear_explicit(src, up, d).float(), ref), (up, H, W, d)
            assert not S.within(S.bilinear_explicit(real, up, d).float(), rref, 4 * S.U32 * n)[0], (up, H, W, d)


def test_nearest_forms_of_torch_agree_for_the_callers_factors():
    """size= and scale_factor= of F.interpolate give the same picture for 2, 4, 1/2, 1/4 (what the callers pass)"""
    for i, ((H, W), (OH, OW)) in enumerate(S.NEAREST):
        src = S.real_data(6, H, W, 500 + i).unsqueeze(0)
        want = F.interpolate(src, size=(OH, OW))
        for f in (2, 4):
            if (OH, OW) == (H * f, W * f):
                assert torch.equal(want, F.interpolate(src, scale_factor=f))
            if (OH * f, OW * f) == (H, W):
                assert torch.equal(want, F.interpolate(src, scale_factor=1.0 / f))
