"""CPU: the public surface of FLoss, CELoss, ConLoss and CrossLoss (exports, reprs, constructor attributes, every refusal), the float64
restatement of tests/class_losses_ref.py against the reference's float32 results in tests/golden/class_losses.npz, and the recorded K."""
import math

import numpy as np
import pytest
import torch

import class_losses_ref as R
from conftest import load_golden

NAMES = ("FLoss", "CELoss", "ConLoss", "CrossLoss")
# fixture case -> (quantity prefix, restatement, keyword arguments)
FIXTURE = {"focal_binary": ("focal", R.focal, {}), "focal_multi": ("focal", R.focal, {}),
           "focal_g15_sum": ("focal", R.focal, {"gamma": 1.5, "mean": False}), "focal_g3": ("focal", R.focal, {"gamma": 3.0}),
           "ce_binary": ("bce", R.bce, {}), "ce_multi": ("nll", R.nll, {}), "con": ("range", R.batch_range, {}), "cross": ("cross", R.cross, {}),
           "edges_focal": ("focal", R.focal, {}), "edges_ce": ("bce", R.bce, {}), "ties": ("range", R.batch_range, {})}


def fixture_inputs(z, name):
    x = z[name + "/x"].astype(np.float32)
    return (x, z[name + "/t"].astype(np.float32)) if name + "/t" in z else (x,)


def test_exports_and_reprs():
    import srcgan_amd
    from srcgan_amd import losses
    for name in NAMES:
        assert name in srcgan_amd.__all__ and name in losses.__all__
        assert getattr(srcgan_amd, name) is getattr(losses, name)
    assert [repr(getattr(losses, n)()) for n in NAMES] == ["Focal", "CE", "ConLoss", "CrossLoss"]


def test_constructor_attributes():
    from srcgan_amd import losses
    f = losses.FLoss()
    assert (f.gamma, f.weight, f.size_average) == (2., None, True)
    w = [0.25, 0.75]
    f = losses.FLoss(1.5, w, False)
    assert (f.gamma, f.weight, f.size_average) == (1.5, w, False)
    f = losses.FLoss(gamma=3., size_average=False)
    assert (f.gamma, f.weight, f.size_average) == (3., None, False)
    for name in NAMES:
        assert isinstance(getattr(losses, name)(), torch.nn.Module)


@pytest.mark.parametrize("name", ["FLoss", "CELoss", "CrossLoss"])
def test_two_tensor_refusals(name):
    from srcgan_amd import losses
    crit = getattr(losses, name)()
    x, t = torch.rand(2, 1, 4, 5), torch.rand(2, 1, 4, 5)
    with pytest.raises(ValueError, match=name):
        crit(x, torch.rand(2, 1, 4, 6))
    with pytest.raises(ValueError, match=name):
        crit(x, t[0])
    with pytest.raises(ValueError, match=name + ".*empty"):
        crit(torch.rand(2, 1, 0, 5), torch.rand(2, 1, 0, 5))
    with pytest.raises(ValueError, match=name + ".*detach the target"):
        crit(x, t.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(x, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(x.clone().requires_grad_(True), t)


def test_dimension_refusals():
    from srcgan_amd import losses
    for crit in (losses.FLoss(), losses.CELoss()):
        with pytest.raises(ValueError, match="at least 2-D"):
            crit(torch.rand(5), torch.rand(5))
    cross = losses.CrossLoss()
    with pytest.raises(ValueError, match="CrossLoss.*4-D"):
        cross(torch.rand(2, 3, 4), torch.rand(2, 3, 4))
    with pytest.raises(ValueError, match="CrossLoss.*at least two samples"):       # the reference returns NaN here
        cross(torch.rand(1, 3, 4, 5), torch.rand(1, 3, 4, 5))


def test_conloss_refusals():
    from srcgan_amd import losses
    con = losses.ConLoss()
    with pytest.raises(ValueError, match="ConLoss"):
        con(torch.tensor(1.0))
    with pytest.raises(ValueError, match="ConLoss.*empty"):
        con(torch.rand(3, 0))
    for feats in (torch.rand(4), torch.rand(2, 3), torch.rand(2, 3, 4, 5, 6)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            con(feats)


def test_fixture_holds_tensors_only_and_stays_small():
    z = load_golden("class_losses")
    assert sorted({k.split("/")[0] for k in z}) == sorted(FIXTURE)
    for k, v in z.items():
        assert v.dtype in (np.float16, np.float32), k
    assert sum(v.nbytes for v in z.values()) < 200_000
    for name in FIXTURE:
        special = name.startswith("edges") or name == "ties"
        if not special and name not in ("con", "cross"):
            x = z[name + "/x"].astype(np.float32)
            assert 0.01 <= x.min() and x.max() <= 0.99, name


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_float64_restatement_against_the_reference(name):
    """The reference's float32 loss and gradient lie within the GPU tests' bound of the float64 restatement; so does the float32 one."""
    z = load_golden("class_losses")
    q, fn, kw = FIXTURE[name]
    inp = fixture_inputs(z, name)
    ref = fn(*inp, **kw)
    want = z[name + "/dx"].reshape(ref["grad"].shape)
    assert R.worst(q + "_loss", z[name + "/loss"], ref["loss"], ref["Nloss"]) <= 1
    assert R.worst(q + "_grad", want, ref["grad"], ref["Ngrad"]) <= 1
    assert np.array_equal(want == 0, ref["Ngrad"] == 0)                             # the exact zeros are the reference's zeros
    got = fn(*inp, dt=np.float32, **kw)
    assert R.worst(q + "_loss", got["loss"], ref["loss"], ref["Nloss"]) <= 1
    assert R.worst(q + "_grad", got["grad"], ref["grad"], ref["Ngrad"]) <= 1


def test_edges_are_the_float32_clamp():
    z = load_golden("class_losses")
    dx = z["edges_focal/dx"].ravel()
    assert dx[0] == 0 and dx[1] == 0 and dx[5] == 0                  # outside [lo, hi]: exactly zero
    assert dx[2] < -1.5e5 and dx[4] < 0                              # the bounds themselves pass the gradient
    assert float(np.float32(1e-6)) < 1e-6                              # why a float64 evaluation would clamp it
    assert abs(float(z["edges_ce/loss"]) - (100 + 16.118 + 13.8155 + 0.6931) / 6) < 1e-3      # log 0 is clamped at -100


def test_measure_k_reproduces_the_recorded_k():
    measured = R.measure_k()
    print("[class_losses] float32 restatement, largest error in units of 2^-24 N:", {q: round(v, 2) for q, v in measured.items()})
    for q in R.QUANTITIES:
        want = 4.0 * measured[q]
        assert want <= R.K_RECORDED[q] <= max(math.ceil(want), 1) + 1e-9, (q, measured[q], R.K_RECORDED[q])
