"""CPU: what the fixture comparison of tests/test_gpu_losses3d.py notices.  The float64 restatements of tests/losses3d_ref.py meet the
reference's fixture (tests/golden/losses3d.npz) at the GPU test's gates -- |loss - fixture| < 1e-5, rel_err of dx and dt < 1e-3 -- on
every case, and each of five deliberate mistakes of a 5-D implementation misses them:

  one_range, plane_index   on ``mixed_ranges`` (DSSIM): with frames of one dynamic range the first changes nothing and the second only
                           permutes the planes inside a sum, which is why the fixture has a case whose frames differ in range
  next_frame, missing_inv_f, f_minus_1   on every case, for both losses
"""
import pytest
import torch

import losses3d_ref as L
import vgg_ref as R
from conftest import load_golden, rel_err

CASES = ["mixed_ranges", "tiles", "single_window", "strip"]
FNS = {"l1": L.l1_3d, "dssim": L.dssim_3d}


def _meets(g, case, key, fault):
    x, t = torch.from_numpy(g[f"{case}/x"]).double(), torch.from_numpy(g[f"{case}/t"]).double()
    loss, dx, dt = L.loss_and_grads(FNS[key], x, t, fault)
    return (abs(loss - float(g[f"{case}/{key}/loss"])) < 1e-5 and rel_err(dx, g[f"{case}/{key}/dx"]) < 1e-3
            and rel_err(dt, g[f"{case}/{key}/dt"]) < 1e-3)


@pytest.mark.parametrize("key", ["l1", "dssim"])
@pytest.mark.parametrize("case", CASES)
def test_restatement_meets_the_fixture(case, key):
    assert _meets(load_golden("losses3d"), case, key, None)


@pytest.mark.parametrize("fault", ["one_range", "plane_index"])
def test_range_and_plane_faults_miss_on_mixed_ranges(fault):
    assert not _meets(load_golden("losses3d"), "mixed_ranges", "dssim", fault)


@pytest.mark.parametrize("key", ["l1", "dssim"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("fault", ["next_frame", "missing_inv_f", "f_minus_1"])
def test_frame_faults_miss_everywhere(fault, case, key):
    assert not _meets(load_golden("losses3d"), case, key, fault)


def test_mixed_ranges_is_not_the_folded_batch():
    """the point of the per-frame range: the 3-D loss is the mean of the per-frame 2-D losses, far from the 2-D loss of the frames folded
    into the batch under one range (both stored by the generator from the reference's classes)"""
    g = load_golden("losses3d")
    loss, per_frame, folded = float(g["mixed_ranges/dssim/loss"]), g["mixed_ranges/dssim/per_frame"], float(g["mixed_ranges/dssim/folded"])
    assert abs(loss - float(per_frame.astype("float64").mean())) < 1e-6
    assert abs(loss - folded) > 0.5 * loss


def test_fixture_frames_stay_clear_of_the_range_thresholds():
    g = load_golden("losses3d")
    for case in CASES:
        x = torch.from_numpy(g[f"{case}/x"]).float()
        for f in range(x.shape[2]):
            assert abs(float(x[:, :, f].max()) - 128) > 20 and abs(float(x[:, :, f].min()) + 0.5) > 0.2, (case, f)


@pytest.mark.parametrize("shape", sorted(L.CASE_SEEDS))
def test_vgg_case_seeds_keep_the_float64_margin(shape):
    assert L.margin(*L.make_case(shape, L.CASE_SEEDS[shape])) >= R.MIN_MARGIN


def test_vgg_restatement_is_the_mean_of_the_frames():
    sd, out, tgt, loss, grad = L.case((1, 1, 3, 32, 32))
    per = [R.loss_and_grad(out[:, :, f], tgt[:, :, f], sd, 0) for f in range(3)]
    assert abs(loss - sum(p[0] for p in per) / 3) < 1e-12
    assert torch.equal(grad[:, :, 1], per[1][1] / 3)
    # and the frames taken as a batch give the same value: every per-frame mean has the same count
    fold = lambda z: z.permute(0, 2, 1, 3, 4).reshape(-1, 1, 32, 32)
    lb, _ = R.loss_and_grad(fold(out), fold(tgt), sd, 0)
    assert abs(lb - loss) < 1e-12
