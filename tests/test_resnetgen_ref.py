"""CPU: pins tests/resnetgen_ref.py (our float64 restatement of the ResNet translator) to the two reference fixtures, so the GPU tests
never need the reference; the dead biases (in front of an InstanceNorm) are held in their absolute measure."""
import pytest
import torch

import resnetgen_ref as R
from conftest import load_golden

FIXTURES = ("resnetgen_1to3", "resnetgen_3to1")
_RUNS = {}


def native(z, dtype=None):
    """the native class with the fixture's seeded weights, built as the fixture was: through define_G"""
    import srcgan_amd
    cin, cout, ngf, nblk = (int(v) for v in z["cfg"])
    torch.manual_seed(int(z["seed"]))
    m = srcgan_amd.define_G(cin, cout, ngf, f"resnet_{nblk}blocks", "instance", False, "normal", 0.02)
    if dtype is not None:
        m.compute_dtype = dtype                 # define_G has the reference's signature: no dtype argument
    return m


def fixture_run(tag):
    """(fixture, the restatement's float64 run on the seeded weights of the native class), computed once per fixture"""
    if tag not in _RUNS:
        z = load_golden(tag)
        _RUNS[tag] = (z, R.run(native(z).state_dict(), torch.from_numpy(z["x"]), torch.from_numpy(z["t"]), int(z["cfg"][3])))
    return _RUNS[tag]


@pytest.mark.parametrize("tag", FIXTURES)
def test_resnetgen_ref_reproduces_the_fixture(tag):
    z, (y, loss, dx, g) = fixture_run(tag)
    nblk = int(z["cfg"][3])
    assert [str(n) for n in z["names"]] == R.names(nblk) and [str(n) for n in z["dead"]] == R.dead_biases(nblk)
    assert tuple(y.shape) == (z["x"].shape[0], int(z["cfg"][1])) + z["x"].shape[2:]
    e64, d64 = R.fixture_errors(z, y, loss, dx, g, "64")
    e32, _ = R.fixture_errors(z, y, loss, dx, g, "")
    (k64, w64), (k32, w32) = R.worst(e64), R.worst(e32)
    print(f"[resnetgen_ref] {tag}: worst against the float64 values {w64:.2e} ({k64}), against the float32 values {w32:.2e} ({k32}); "
          f"worst dead-bias ratio in float64 {max(d64.values()):.2e}, the reference's float32 one {max(float(z['dead_ratio/' + k]) for k in d64):.2e}")
    assert w64 < 1e-10, k64
    assert w32 < 1e-4, k32
    assert max(d64.values()) < 1e-12                                          # zero in exact arithmetic
    assert max(float(z["dead_ratio/" + k]) for k in d64) < 1.1e-6            # the reference's own float32 run


def test_storage_emulation_in_float64_rounds_nothing():
    z, (y, _, dx, g) = fixture_run("resnetgen_1to3")
    sd, x, t = native(z).state_dict(), torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    live = [k for k in g if k not in R.dead_biases(6)]
    b = R.run(sd, x, t, 6, store=torch.float64)
    assert R.rel_l2(b[0], y) < 1e-13 and R.rel_l2(b[2], dx) < 1e-12 and max(R.rel_l2(b[3][k], g[k]) for k in live) < 1e-12
    c = R.run(sd, x, t, 6, store=torch.bfloat16)
    assert 1e-4 < R.rel_l2(c[0], y) < 1e-1


def test_zero_padding_is_another_function_with_other_keys():
    z, (y, _, _, _) = fixture_run("resnetgen_1to3")
    sd = native(z).state_dict()
    sdz = dict(zip(R.names(6, "zero"), sd.values()))
    yz = R.forward({k: v.double() for k, v in sdz.items()}, torch.from_numpy(z["x"]).double(), 6, "zero")
    assert yz.shape == y.shape and R.rel_l2(yz, y) > 1e-3
