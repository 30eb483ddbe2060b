"""CPU: what the per-pixel bound of tests/test_gpu_metrics_kernels.py notices, and that its constants are what tests/ssim_ref.py says
they are.

  * the float32 restatement (ssim_ref.restated32) stays within K / 4 of the float64 gradient on every backward case: the reference
    alone meets the bound with room;
  * every applicable mistake of ssim_ref.FAULTS is reported by `within` at K, on dx of every backward case;
  * one planted NaN fails;
  * the formula that grad_scale takes absolute values of is the float64 autograd gradient;
  * every forward probe's float64 loss is at least 100 x tol_f, and the two forward mistakes move the loss by more than tol_f on the
    probes they touch;
  * K, tol_f, tol_m and the AE tolerances are the recorded multiples of what the restatements give today.
"""
import math

import numpy as np
import pytest
import torch

import ssim_ref as S

NAMES = list(S.BWD_CASES)


@pytest.fixture(scope="module")
def measured():
    return S.measure()


# ------------------------------------------------------------------------------------------------ the backward bound
@pytest.mark.parametrize("name", NAMES)
def test_restatement_stays_within_a_quarter_of_K(name):
    c = S.bwd_case(name)
    _, dx32, dt32 = S.restated32(c["x"], c["t"], S.GOUT)
    assert S.within(dx32, c["dx"], c["Nx"], S.K / 4, f"restated32 {name} dx")
    assert S.within(dt32, c["dt"], c["Nt"], S.K / 4, f"restated32 {name} dt")


@pytest.mark.parametrize("name", NAMES)
def test_formula_is_the_autograd_gradient(name):
    """2^-20 of a float32 unit of N: the float64 formula and float64 autograd differ by rounding alone"""
    c = S.bwd_case(name)
    fx, ft = S.grad_formula64(c["x"], c["t"], S.GOUT)
    assert S.within(fx, c["dx"], c["Nx"], 2.0 ** -20, f"formula {name} dx") and S.within(ft, c["dt"], c["Nt"], 2.0 ** -20, f"formula {name} dt")
    assert float(c["Nx"].min()) > 0 and float(c["Nt"].min()) > 0
    assert bool((c["dx"].abs() <= c["Nx"] * (1 + 1e-12)).all()) and bool((c["dt"].abs() <= c["Nt"] * (1 + 1e-12)).all())


@pytest.mark.parametrize("fault", S.FAULTS)
@pytest.mark.parametrize("name", NAMES)
def test_every_fault_is_reported(name, fault):
    if not S.applicable(fault, name):
        assert fault in ("plane_swap", "range_from_truth")
        return
    c = S.bwd_case(name)
    bx, bt = S.grad64(c["x"], c["t"], S.GOUT, fault)
    assert not S.within(bx, c["dx"], c["Nx"], S.K, f"{fault} {name} dx")
    if fault != "x_for_y":          # that one is a mistake in dx alone
        assert not S.within(bt, c["dt"], c["Nt"], S.K, f"{fault} {name} dt")


def test_every_fault_has_a_case():
    for fault in S.FAULTS:
        assert any(S.applicable(fault, n) for n in NAMES), fault
    c = S.bwd_case("truth_range")
    assert S.L3._range(c["x"]) == 1.0 and S.L3._range(c["t"]) == 2.0


def test_dropped_corner_position_is_far_outside():
    """the one position that covers the corner pixel alone: dropping it moves that pixel by its whole value, thousands of bounds"""
    c = S.bwd_case("ragged2c")
    bx, _ = S.grad64(c["x"], c["t"], S.GOUT, "drop_corner_position")
    assert float(bx[0, 0, 0, 0, 0]) == 0.0
    assert S.max_ratio(bx, c["dx"], c["Nx"]) > 1000 * S.K


@pytest.mark.parametrize("name", ["single", "frames"])
def test_a_planted_nan_fails(name):
    c = S.bwd_case(name)
    assert S.within(c["dx"].clone(), c["dx"], c["Nx"], S.K, f"clean {name}")
    bad = c["dx"].clone()
    bad.view(-1)[bad.numel() // 2] = math.nan
    assert not S.within(bad, c["dx"], c["Nx"], S.K, f"nan {name}")


def test_case_data_is_float16_representable_and_in_its_range():
    for name in NAMES:
        c = S.bwd_case(name)
        for z in (c["x"], c["t"]):
            assert z.dtype == torch.float32 and torch.equal(z, z.half().float())
    f = S.bwd_case("frames")["x"]
    assert S.L3._range(f[:, :, 0]) == 1.0 and S.L3._range(f[:, :, 1]) == 255.0
    assert S.L3._range(S.bwd_case("signed")["x"]) == 2.0


# ------------------------------------------------------------------------------------------------ the recorded constants
def _recorded(measured_value, recorded):
    """the recorded figure is today's measurement, rounded up in its last digit"""
    return measured_value <= recorded <= 1.02 * measured_value


def test_K_is_four_times_the_restatement(measured):
    for name in S.K_CASES:
        for got, rec in zip(measured["ratios"][name], S.RESTATED_RATIO[name]):
            assert abs(got - rec) <= 0.011, (name, got, rec)          # recorded to two decimals, the worst rounded up
    assert set(S.RESTATED_RATIO) == set(S.K_CASES)
    assert S.K == 4 * max(max(v) for v in S.RESTATED_RATIO.values())
    assert max(measured["ratios"]["truth_range"]) <= S.K / 4


def test_forward_tolerances_are_eight_times_the_restatement(measured):
    assert _recorded(measured["loss_err"], S.RESTATED_LOSS_ERR) and S.TOL_F == max(8 * S.RESTATED_LOSS_ERR, 2.0 ** -24)
    assert _recorded(measured["metric_err"], S.RESTATED_METRIC_ERR) and S.TOL_M == max(8 * S.RESTATED_METRIC_ERR, 2.0 ** -22)


def test_ae_tolerances_are_four_times_the_restatement(measured):
    for fam, rec in S.RESTATED_AE_ERR.items():
        assert _recorded(measured["ae"][fam], rec), (fam, measured["ae"][fam])
        assert S.TOL_AE[fam] == 4 * rec


# ------------------------------------------------------------------------------------------------ the forward probes
def _touches(fault, H, W, blk):
    """the block reaches the centre tap of a window position that the mistake drops (the last position row) or changes (the first
    position column, which a shifted window never reads from, and the last, which then reads zeros)"""
    _, y0, x0, s = blk
    if fault == "drop_last_position_row":
        return y0 + s > H - 6
    return x0 < 6 or x0 + s > W - 6


@pytest.mark.parametrize("shape,blk", S.fwd_probes(), ids=lambda v: "x".join(map(str, v[-2:])) if len(v) == 5 else v[0])
def test_probe_losses_are_large_and_the_forward_faults_move_them(shape, blk):
    x, t = S.fwd_probe(shape, blk)
    loss = float(S.loss64(x, t))
    assert loss >= 100 * S.TOL_F, (shape, blk, loss)
    for fault in ("drop_last_position_row", "shift_window"):
        if _touches(fault, shape[-2], shape[-1], blk):
            assert abs(float(S.loss64(x, t, fault)) - loss) > S.TOL_F, (fault, shape, blk)


def test_probe_table_covers_the_named_places():
    assert [b[0] for b in S.probe_blocks(37, 53)] == ["corner00", "corner01", "corner10", "corner11", "edge_top", "edge_bottom", "edge_left",
                                                     "edge_right", "interior", "seam", "last_tile"]
    assert any(b[1:] == (16, 16, 11) for b in S.probe_blocks(27, 27))        # on 27x27 the seam block is the last corner
    for shape in S.FWD_SHAPES:
        H, W = shape[-2:]
        for fault in ("drop_last_position_row", "shift_window"):
            assert any(_touches(fault, H, W, b) for b in S.probe_blocks(H, W)), (shape, fault)
    x, t = S.fwd_probe(S.FWD_SHAPES[-1], S.probe_blocks(27, 27)[0])
    assert torch.equal(x[:, :, 0], t[:, :, 0]) and not torch.equal(x[:, :, 1], t[:, :, 1])
    px, pt = S.metric_probe(37, 53, 0)
    m = S.metric64(px, pt)
    assert abs(float(m[0, 0]) - float(m[1, 0])) > 100 * S.TOL_M        # the two images of a metric probe differ


def test_metric_reference_is_the_loss_reference():
    px, pt = S.metric_probe(27, 27, 3)
    m = S.metric64(px, pt)
    assert abs((1 - float(m[:, 0].mean())) / 2 - float(S.loss64(px.unsqueeze(2), pt.unsqueeze(2)))) < 1e-14


# ------------------------------------------------------------------------------------------------ range and AE designs
@pytest.mark.parametrize("hw", [(11, 11), (257, 257)])
def test_range_case_extremes_sit_where_they_were_planted(hw):
    x = S.range_case(hw)
    n = hw[0] * hw[1]
    assert x.shape[:3] == (2, 1, 3)
    for f in range(3):
        fr = x[:, 0, f].reshape(2, n)
        assert float(fr.min()) == -0.4375 - f / 64 and float(fr.max()) == 101.0 + f
    where = {(int(p), int(i)) for f in range(3) for v in (x[:, 0, f].reshape(2, n),) for p, i in (divmod(int(v.argmin()), n), divmod(int(v.argmax()), n))}
    want = {(0, 0), (0, n - 1), (1, n - 1), (1, 0)} | ({(0, 255), (0, 256)} if n > 256 else set())
    assert where == want


def test_threshold_cases_follow_the_float64_rule():
    for name, x, t, L in S.threshold_cases():
        assert S.L3._range(x) == L, name
        l32 = S.restated32(x, t, 1.0)[0]
        assert abs(l32 - float(S.loss64(x, t))) <= S.TOL_F / 8, (name, l32)
    # and the rule matters: the loss under the neighbouring L is far away
    name, x, t, L = S.threshold_cases()[0]
    assert abs(float(S.L3.dssim2d(x[:, :, 0].double(), t[:, :, 0].double(), 255.0)) - float(S.loss64(x, t))) > 1000 * S.TOL_F


def test_ae_designs():
    for hw in S.AE_HW:
        p, t = S.ae_case("exact", hw)
        ref = S.ae64(p, t)
        for b in range(2):
            ang = np.zeros(hw)
            for pp, tt, a in S.AE_PAIRS:
                hit = (p[b, :, 0].T == np.float32(pp)).all(1) & (t[b, :, 0].T == np.float32(tt)).all(1)
                ang[hit] = a
            assert (ang > 0).all()
            assert abs(ref[b] - ang.mean()) < 0.09        # eps moves only the 180 degree pixels, by 0.081 degrees
    p, t = S.ae_case("same", 255, 3)
    assert np.array_equal(p, t) and (0.02 < S.ae64(p, t)).all() and (S.ae64(p, t) < 0.3).all()      # about 0.1 degrees, not 0: the formula's eps
