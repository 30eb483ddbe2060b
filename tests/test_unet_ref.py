"""CPU: pins tests/unet_ref.py (our float64 restatement of the U-Net translator, without in-place operations) to the two reference
fixtures, so the GPU tests never need the reference; the dead biases (in front of an InstanceNorm) are held in their absolute measure."""
import pytest
import torch

import unet_ref as R
from conftest import load_golden

FIXTURES = ("unet_d5_1to3", "unet_d6_3to1")
_RUNS = {}


def native(z, dtype=None):
    """the native class with the fixture's seeded weights, built as the fixture was: init_net on the class, as the reference's define_G does"""
    import srcgan_amd
    cin, cout, ngf, nd = (int(v) for v in z["cfg"])
    torch.manual_seed(int(z["seed"]))
    return srcgan_amd.init_net(srcgan_amd.UnetGenerator(cin, cout, nd, ngf, norm_layer=srcgan_amd.get_norm_layer("instance"), dtype=dtype), "normal", 0.02)


def fixture_run(tag):
    """(fixture, the restatement's float64 run on the seeded weights of the native class), computed once per fixture"""
    if tag not in _RUNS:
        z = load_golden(tag)
        _RUNS[tag] = (z, R.run(native(z).state_dict(), torch.from_numpy(z["x"]), torch.from_numpy(z["t"]), int(z["cfg"][3])))
    return _RUNS[tag]


@pytest.mark.parametrize("tag", FIXTURES)
def test_unet_ref_reproduces_the_fixture(tag):
    z, (y, loss, dx, g) = fixture_run(tag)
    n = int(z["cfg"][3])
    assert [str(k) for k in z["names"]] == R.names(n) and [str(k) for k in z["dead"]] == R.dead_biases(n)
    assert len(R.names(n)) == 4 * n and len(R.dead_biases(n)) == 2 * n - 3
    assert tuple(y.shape) == (z["x"].shape[0], int(z["cfg"][1])) + z["x"].shape[2:]
    e64, d64 = R.fixture_errors(z, y, loss, dx, g, "64")
    e32, _ = R.fixture_errors(z, y, loss, dx, g, "")
    (k64, w64), (k32, w32) = R.worst(e64), R.worst(e32)
    print(f"[unet_ref] {tag}: worst against the float64 values {w64:.2e} ({k64}), against the float32 values {w32:.2e} ({k32}); "
          f"worst dead-bias ratio in float64 {max(d64.values()):.2e}, the reference's float32 one {max(float(z['dead_ratio/' + k]) for k in d64):.2e}")
    assert w64 < 1e-10, k64
    assert w32 < 1e-4, k32
    assert max(d64.values()) < 1e-12                                          # zero in exact arithmetic
    assert max(float(z["dead_ratio/" + k]) for k in d64) < 1e-5               # the reference's own float32 run: 2.2e-6 / 3.2e-6


def test_the_live_biases_are_the_three_the_norms_do_not_follow():
    z, (_, _, _, g) = fixture_run("unet_d5_1to3")
    live = [k for k in R.names(5) if k.endswith(".bias") and k not in R.dead_biases(5)]
    assert live == ["model.model.0.bias", "model.model.1.model.3.model.3.model.3.model.1.bias", "model.model.3.bias"]
    assert all(R.dead_ratio(g, k) > 1e-3 for k in live)


def test_storage_emulation_in_float64_rounds_nothing():
    z, (y, _, dx, g) = fixture_run("unet_d5_1to3")
    sd, x, t = native(z).state_dict(), torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    live = [k for k in g if k not in R.dead_biases(5)]
    b = R.run(sd, x, t, 5, store=torch.float64)
    assert R.rel_l2(b[0], y) < 1e-13 and R.rel_l2(b[2], dx) < 1e-12 and max(R.rel_l2(b[3][k], g[k]) for k in live) < 1e-12
    c = R.run(sd, x, t, 5, store=torch.bfloat16)
    assert 1e-4 < R.rel_l2(c[0], y) < 1e-1
    # rounding the gradient tensors in front of the norms too: nothing in float64; in bfloat16 the dead biases leave exact zero by about
    # 2^-9 of their layer's gradients (the 16-bit yardstick of tests/test_gpu_unet.py), where the forward-only emulation leaves 1e-15
    d = R.run(sd, x, t, 5, store=torch.float64, round_grads=True)
    assert all(torch.equal(d[3][k], b[3][k]) for k in g)
    dead = R.dead_biases(5)
    e = R.run(sd, x, t, 5, store=torch.bfloat16, loss_scale=1024.0, round_grads=True)
    c = R.run(sd, x, t, 5, store=torch.bfloat16, loss_scale=1024.0)
    assert max(R.dead_ratio(c[3], k) for k in dead) < 1e-12
    assert 2.0 ** -12 < max(R.dead_ratio(e[3], k) for k in dead) < 1.0          # far from zero, and still below the layer's weight gradient
    assert torch.equal(e[0], c[0]) and max(R.rel_l2(e[3][k], c[3][k]) for k in live) < 2.0 ** -6
