"""CPU: what the fixture comparison of tests/test_gpu_mdsr.py and tests/test_gpu_vdsr.py notices.  Each deliberate mistake of
tests/mdsr_ref.py (``mut``), run in float64 on the fixture's own weights, misses the fixture at the 1e-3 gate of the fp32 GPU tests -- in
y, the loss, dx, a parameter gradient, or in the SET of parameters that have a gradient -- while the unmutated run sits orders below it
(tests/test_mdsr_ref.py)."""
import pytest
import torch

import mdsr_ref
from conftest import load_golden, rel_err
from test_mdsr_ref import FIXTURES, fixture_run, native, ref_run

GATE = 1e-3


def mutated(tag, mut):
    z = load_golden(tag)
    return z, ref_run(z, tag, native(z, tag).state_dict(), mut=mut)


def test_the_unmutated_run_passes_the_gate():
    for tag in FIXTURES:
        z, (y, loss, dx, g) = fixture_run(tag)
        assert mdsr_ref.worst(mdsr_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err))[1] < GATE / 10


@pytest.mark.parametrize("tag", ["mdsr_s234_idx0", "mdsr_s234_idx1", "mdsr_s234_idx2"])
def test_the_wrong_branch_has_another_size_and_other_parameters_on_the_graph(tag):
    """scale_idx off by one: another output size (the three scales differ), and against a target of that size other parameters with a
    gradient than the fixture's -- ``fixture_errors`` holds the set before any value"""
    z = load_golden(tag)
    n, scales, idx = int(z["cfg"][0]), [int(s) for s in z["scales"]], int(z["cfg"][3])
    sd, x = native(z, tag).state_dict(), torch.from_numpy(z["x"])
    y = mdsr_ref.mdsr_forward({k: v.double() for k, v in sd.items()}, x.double(), n, scales, idx, mut="wrong_branch")
    assert tuple(y.shape) != tuple(z["y"].shape)
    y, loss, dx, g = mdsr_ref.mdsr_run(sd, x, torch.zeros_like(y), n, scales, idx, mut="wrong_branch")
    assert set(g) == set(mdsr_ref.mdsr_branch(n, scales, (idx + 1) % 3)) != set(mdsr_ref.fixture_grad_names(z))
    with pytest.raises(AssertionError):
        mdsr_ref.fixture_errors(z, torch.from_numpy(z["y"]), z["loss"], dx, g, "", measure=rel_err)


@pytest.mark.parametrize("mut", ["skip_from_head", "k3_crop", "no_relu"])
@pytest.mark.parametrize("tag", ["mdsr_s234_idx0", "mdsr_s234_idx1", "mdsr_s234_idx2"])
def test_each_mistake_misses_the_mdsr_fixtures(tag, mut):
    z, (y, loss, dx, g) = mutated(tag, mut)
    e = mdsr_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err)
    k, v = mdsr_ref.worst(e)
    print(f"[mdsr teeth] {tag} {mut}: y {e['y']:.2e} dx {e['dx']:.2e} worst {v:.2e} ({k})")
    assert e["y"] > GATE or e["dx"] > GATE, (mut, e["y"], e["dx"])          # seen without a single parameter gradient
    assert v > GATE


@pytest.mark.parametrize("mut", ["no_relu", "vdsr_skip_after_add_mean"])
def test_each_mistake_misses_the_vdsr_fixture(mut):
    z, (y, loss, dx, g) = mutated("vdsr", mut)
    e = mdsr_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err)
    k, v = mdsr_ref.worst(e)
    print(f"[mdsr teeth] vdsr {mut}: y {e['y']:.2e} dx {e['dx']:.2e} worst {v:.2e} ({k})")
    assert e["y"] > GATE and v > GATE


def test_a_gradient_reported_for_an_inactive_branch_is_noticed():
    """values alone would pass -- the extra gradients are zeros beside a correct run -- so the comparison holds the SET against the fixture"""
    z, (y, loss, dx, g) = mutated("mdsr_s234_idx1", "inactive_grad")
    extra = set(g) - set(mdsr_ref.fixture_grad_names(z))
    assert extra == {str(k) for k in z["nograd"]} and len(extra) == 22
    with pytest.raises(AssertionError):
        mdsr_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err)
    kept = {k: v for k, v in g.items() if k not in extra}
    assert mdsr_ref.worst(mdsr_ref.fixture_errors(z, y, loss, dx, kept, "", measure=rel_err))[1] < GATE / 10


def test_the_mutation_list_is_the_one_the_tests_run():
    assert set(mdsr_ref.MUTATIONS) == {"wrong_branch", "skip_from_head", "k3_crop", "no_relu", "vdsr_skip_after_add_mean", "inactive_grad"}
