"""CPU: the float64 comparisons of tests/test_gpu_vgg_loss.py have teeth.  Each deliberate mistake of vgg_ref.FAULTS, made in the float64
composition itself, moves the loss or the gradient of the shared test case by more than the 1e-3 gate (F32_TOL) those tests apply --
so a native implementation with that mistake cannot pass them."""
import pytest
import torch

import vgg_ref as R

F32_TOL = 1e-3                      # the gate of tests/test_gpu_vgg_loss.py (= tests/test_gpu_modules.py F32_TOL)
SHAPE = (2, 3, 20, 28)              # pools floor 5x7 -> 2x3: ceil pooling changes the shapes' content


def test_pick_pool_with_the_first_maximum_is_torchs_max_pool():
    sd, out, tgt, loss, grad = R.case(0, SHAPE)
    l2, g2 = R.loss_and_grad(out, tgt, sd, 0, pick_pool=True)
    assert l2 == loss and torch.equal(g2, grad)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_comparison_notices(fault):
    sd, out, tgt, loss, grad = R.case(0, SHAPE)
    l2, g2 = R.loss_and_grad(out, tgt, sd, 0, fault=fault)
    e_loss, e_grad = R.errors(l2, g2, loss, grad)
    print(fault, "loss error", e_loss, "gradient error", e_grad)
    assert max(e_loss, e_grad) > 10 * F32_TOL


@pytest.mark.parametrize("fault", ["ceil_pool", "last_max", "relu_ge", "swapped_branches"])
def test_comparison_notices_on_vgg19(fault):
    sd, out, tgt, loss, grad = R.case(1, SHAPE)
    l2, g2 = R.loss_and_grad(out, tgt, sd, 1, fault=fault)
    e_loss, e_grad = R.errors(l2, g2, loss, grad)
    print(fault, "loss error", e_loss, "gradient error", e_grad)
    assert max(e_loss, e_grad) > 10 * F32_TOL


def test_shared_cases_keep_their_margin():
    """every fp32-gated case stays MIN_MARGIN away from each ReLU / argmax / sign decision in float64 (vgg_ref.CASE_SEEDS)"""
    for (kind, shape), seed in R.CASE_SEEDS.items():
        m = R.margin(kind, *R.make_case(kind, shape, seed))
        print(kind, shape, "seed", seed, "margin", m)
        assert m >= R.MIN_MARGIN
    assert R.first_seed(0, (1, 3, 16, 16)) == R.CASE_SEEDS[(0, (1, 3, 16, 16))]


def test_reference_key_lists():
    """the lists the host test compares state_dict() with: ten / sixteen convolutions under the reference's module names"""
    assert len(R.VGG16LOSS_KEYS) == 20 and R.VGG16LOSS_KEYS[0] == "slice1.0.weight" and R.VGG16LOSS_KEYS[-1] == "slice4.21.bias"
    assert len(R.PERCEPTION_KEYS) == 32 and R.PERCEPTION_KEYS[0] == "features.0.weight" and R.PERCEPTION_KEYS[-1] == "features.34.bias"
    assert sorted(R.to_slice_keys(R.seeded_state(0))) == sorted(R.VGG16LOSS_KEYS)
    assert sorted(R.seeded_state(1)) == sorted(R.PERCEPTION_KEYS)
