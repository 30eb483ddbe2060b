"""CPU: what the fixture comparison of tests/test_gpu_rdn.py notices.  Each deliberate mistake of tests/rdn_ref.py (``mut``), run in
float64 on the fixture's own weights, misses the fixture at the 1e-3 gate of the fp32 GPU test -- in y, the loss, dx or a parameter
gradient -- while the unmutated run sits orders below it (tests/test_rdn_ref.py)."""
import pytest
import torch

import rdn_ref
from conftest import load_golden, rel_err
from test_rdn_ref import fixture_run

GATE = 1e-3


def mutated(tag, mut):
    import srcgan_amd
    z = load_golden(tag)
    torch.manual_seed(int(z["seed"]))
    m = srcgan_amd.RDN(scale=int(z["scale"]), G0=int(z["G0"]), RDNconfig=str(z["config"]), n_colors=int(z["n_colors"]))
    y, loss, dx, g = rdn_ref.run(m.state_dict(), torch.from_numpy(z["x"]), torch.from_numpy(z["t"]), str(z["config"]), int(z["scale"]), mut=mut)
    return rdn_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err)


def test_the_unmutated_run_passes_the_gate():
    for tag in ("rdn_a_x2", "rdn_a_x4_gray"):
        z, (y, loss, dx, g) = fixture_run(tag)
        assert rdn_ref.worst(rdn_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err))[1] < GATE / 10


@pytest.mark.parametrize("mut", [m for m in rdn_ref.MUTATIONS if m != "skip_stage2"])
def test_each_mistake_misses_the_fixture(mut):
    e = mutated("rdn_a_x2", mut)
    k, v = rdn_ref.worst(e)
    print(f"[rdn teeth] {mut}: y {e['y']:.2e} dx {e['dx']:.2e} worst {v:.2e} ({k})")
    assert e["y"] > GATE or e["dx"] > GATE, (mut, e["y"], e["dx"])          # seen without a single parameter gradient
    assert v > GATE


@pytest.mark.parametrize("mut", ["skip_stage2", "shuffle_order"])
def test_each_mistake_of_the_second_stage_misses_the_x4_fixture(mut):
    e = mutated("rdn_a_x4_gray", mut)
    k, v = rdn_ref.worst(e)
    print(f"[rdn teeth] x4 {mut}: y {e['y']:.2e} dx {e['dx']:.2e} worst {v:.2e} ({k})")
    assert e["y"] > GATE and v > GATE


def test_the_mutation_list_is_the_one_the_tests_run():
    assert set(rdn_ref.MUTATIONS) == {"drop_block", "short_read", "slot_off", "lff_no_residual", "gff_swap", "no_global_residual", "shuffle_order", "skip_stage2"}
