"""CPU: the NearestSelector / NearestL1Loss interface (names, reprs, the refusals raised before any launch), and
tests/nearest_ref.py -- the float64 restatement the GPU tests use -- against every array of the reference's fixture
(tests/golden/nearest_selector.npz)."""
import numpy as np
import pytest
import torch

import nearest_ref as R
from conftest import load_golden

CASES = ["golden", "stride2", "shift3", "nonsquare"]


def test_names_are_exported():
    import srcgan_amd
    from srcgan_amd import losses
    for name in ("NearestSelector", "NearestL1Loss"):
        assert getattr(srcgan_amd, name) is getattr(losses, name)
        assert name in srcgan_amd.__all__ and name in losses.__all__
    ns = srcgan_amd.NearestSelector()
    assert repr(ns) == "NS" and (ns.shift, ns.stride, ns.criter) == (2, 1, "l1")
    m = srcgan_amd.NearestL1Loss()
    assert repr(m) == "NSL1" and (m.shift, m.stride) == (2, 1) and isinstance(m, torch.nn.Module)
    assert list(m.parameters()) == [] and list(m.buffers()) == []


def test_unravel_index_is_floor_division_of_the_first_minimum():
    from srcgan_amd import NearestSelector
    diff = torch.tensor([[5., 1., 3., 1.], [2., 2., 2., 2.], [9., 8., 7., 6.]])
    rc = NearestSelector.unravel_index(diff, 2)
    assert rc.dtype == torch.int64 and rc.tolist() == [[0, 1], [0, 0], [1, 1]]
    assert np.array_equal(R.select(diff.numpy(), 2), rc.numpy())


def test_cpu_inputs_have_no_fallback():
    from srcgan_amd import NearestL1Loss, NearestSelector
    x, t = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NearestL1Loss()(x, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NearestSelector().crop(x, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NearestSelector().shift_diff(x, t, 12, 12)


@pytest.mark.parametrize("xs, ts, kw", [
    ((1, 3, 16, 16), (1, 3, 16, 17), {}),                      # shape mismatch
    ((2, 3, 16, 16), (1, 3, 16, 16), {}),
    ((3, 16, 16), (3, 16, 16), {}),                            # not 4-D
    ((1, 1, 3, 16, 16), (1, 1, 3, 16, 16), {}),
    ((1, 3, 4, 16), (1, 3, 4, 16), {}),                        # empty crop: H = 2 * shift * stride
    ((1, 3, 16, 3), (1, 3, 16, 3), {}),
    ((1, 3, 16, 16), (1, 3, 16, 16), {"shift": 2, "stride": 4}),
    ((1, 3, 16, 16), (1, 3, 16, 16), {"shift": 0}),
    ((1, 3, 16, 16), (1, 3, 16, 16), {"stride": 0}),
])
def test_shape_errors(xs, ts, kw):
    from srcgan_amd import NearestL1Loss, NearestSelector
    for dev in ("cpu", "meta"):
        x, t = torch.empty(xs, device=dev), torch.empty(ts, device=dev)
        with pytest.raises(ValueError):
            NearestL1Loss(**kw)(x, t)
        with pytest.raises(ValueError):
            NearestSelector(**kw).crop(x, t)


def test_shift_diff_refuses_crops_that_leave_the_image():
    from srcgan_amd import NearestSelector
    x = torch.empty(1, 1, 12, 12, device="meta")
    for ch, cw in ((0, 8), (8, 0), (10, 8), (8, 10)):          # (n - 1) * stride + crop > H or W
        with pytest.raises(ValueError):
            NearestSelector().shift_diff(x, x, ch, cw)


def test_library_refuses_on_the_host():
    """the planner is host code: its refusals carry an error string and need no device"""
    from srcgan_amd import _native as N
    lib = N.lib()
    assert lib.srcgan_shift_search_scratch_floats(16, 3, 1024, 1024, 2, 1, 1020, 1020) == 16 * 3 * 32 * 16 * 16 + 16
    for args, msg in (((1, 1, 24, 24, 5, 1, 4, 4), b"kept in registers"), ((1, 1, 164, 164, 2, 40, 4, 4), b"does not fit in LDS"),
                      ((1, 1, 12, 12, 2, 1, 0, 8), b"empty crop"), ((1, 1, 12, 12, 2, 1, 8, 10), b"leave the 12 x 12 image"),
                      ((1, 1, 12, 12, 2, 1, 10, 8), b"leave the 12 x 12 image")):
        assert lib.srcgan_shift_search_scratch_floats(*args) == 0
        assert msg in lib.srcgan_last_error(), (args, lib.srcgan_last_error())


# --------------------------------------------------------------------------- the restatement against the reference's arrays
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_fixture(case):
    g = load_golden("nearest_selector")
    shift, stride = (int(v) for v in g[f"{case}/cfg"])
    x, t = g[f"{case}/x"].astype(np.float32), g[f"{case}/t"].astype(np.float32)
    sd, ch, cw, n = R.geometry(x.shape[2], x.shape[3], shift, stride)
    diff = R.shift_diff(x, t, shift, stride)
    # the reference sums C*ch*cw float32 terms below 1 per entry: its own rounding is within count * 2^-24 of the largest sum
    count = x.shape[1] * ch * cw
    assert np.abs(diff - g[f"{case}/diff"]).max() <= count * 2.0 ** -24 * diff.max()
    if case == "golden":
        assert np.argmin(diff, axis=1).tolist() == [3, 10, 13]
    if case == "nonsquare":
        assert f"{case}/sel" not in g
        return
    ref = R.l1(x, t, shift, stride)
    out_, tgt_, sel = R.crops(x, t, shift, stride)
    assert np.array_equal(sel, g[f"{case}/sel"]) and np.array_equal(ref["sel"], sel)
    assert np.array_equal(out_, g[f"{case}/out_"].astype(np.float32)) and np.array_equal(tgt_, g[f"{case}/tgt_"].astype(np.float32))
    assert abs(ref["loss"] - float(g[f"{case}/loss"])) <= 1e-6 * ref["loss"]
    dx = g[f"{case}/dx"].astype(np.float64)
    assert np.array_equal(np.sign(dx), np.sign(ref["dout"])) and np.abs(dx - ref["dout"]).max() <= 1e-6 * np.abs(dx).max()
    assert not ref["dout"][:, :, :sd].any() and not ref["dout"][:, :, :, :sd].any()
