"""CPU: the shared checks of tests/net_checks.py and the runner and sketch of tests/net_ref.py have teeth.  One function stands guard
for every network family, so each thing it gates is pushed just past its bound here, alone, on synthetic tuples: y, dx, one parameter
gradient, the loss, a non-finite gradient, the gradients' names."""
import numpy as np
import pytest
import torch

import net_checks as NC
import net_ref
from test_mdsr_ref import fixture_run

NAMES = ("a.weight", "a.bias", "b.weight")
EMU = 0.01          # the storage emulation's error in every tensor: the 16-bit bound is 1.5 * 0.01 + 5e-3 = 0.02


def _ref():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(2, 3, 8, 8), torch.tensor(0.25, dtype=torch.float64), r(2, 3, 4, 4), {k: r(4, 5) for k in NAMES}


def _off(ref, d=0.0, **only):
    """the run ``ref`` in step()'s form with relative error ``d`` everywhere, or ``only[what]`` in one of y, loss, dx, a gradient's name"""
    y, loss, dx, g = ref
    e = lambda what: 1.0 + only.get(what, d)
    return y * e("y"), float(loss) * e("loss"), dx * e("dx"), {k: v * e(k) for k, v in g.items()}


@pytest.mark.parametrize("names", ["set", "list"])
def test_check_fp32_passes_within_the_gate_and_fails_just_past_it(names):
    ref = _ref()
    NC.check_fp32("teeth", "within", _off(ref, 0.9 * NC.F32_TOL), ref, names=names)
    for what in ("y", "loss", "dx", "a.bias"):
        with pytest.raises(AssertionError):
            NC.check_fp32("teeth", what, _off(ref, **{what: 1.1 * NC.F32_TOL}), ref, names=names)


@pytest.mark.parametrize("names", ["set", "list"])
def test_check_16bit_passes_within_the_bound_and_fails_just_past_it(names):
    ref = _ref()
    emu, bound = _off(ref, EMU), NC.bound16(EMU)
    assert bound == pytest.approx(0.02)
    NC.check_16bit("teeth", "within", "bf16", _off(ref, 0.95 * bound), ref, emu, names=names)
    for what in ("y", "dx", "b.weight"):
        with pytest.raises(AssertionError):
            NC.check_16bit("teeth", what, "bf16", _off(ref, **{what: 1.05 * bound}), ref, emu, names=names)
    for bad in (float("nan"), float("inf")):
        got = _off(ref)
        got[3]["a.weight"][1, 2] = bad
        with pytest.raises(AssertionError):
            NC.check_16bit("teeth", "non-finite", "bf16", got, ref, emu, names=names)


def test_the_loss_is_no_part_of_the_16_bit_gate_and_skipped_gradients_are_the_callers():
    ref = _ref()
    NC.check_16bit("teeth", "", "fp16", _off(ref, loss=0.5), ref, _off(ref, EMU), names="list")
    NC.check_16bit("teeth", "", "fp16", _off(ref, **{"a.bias": 0.5}), ref, _off(ref, EMU), names="list", skip=("a.bias",))
    NC.check_fp32("teeth", "skip", _off(ref, **{"a.bias": 0.5}), ref, names="list", skip=("a.bias",))


def _renamed(got, keys):
    return got[:3] + ({k: got[3].get(k, torch.zeros(4, 5, dtype=torch.float64)) for k in keys},)


@pytest.mark.parametrize("keys, as_set", [(NAMES[:2], False), (NAMES + ("c.weight",), False), (NAMES[::-1], True)], ids=["missing", "extra", "reordered"])
def test_the_names_must_be_the_restatements(keys, as_set):
    ref = _ref()
    got, emu = _renamed(_off(ref), keys), _off(ref, EMU)
    with pytest.raises(AssertionError):
        NC.check_fp32("teeth", "names", got, ref, names="list")
    with pytest.raises(AssertionError):
        NC.check_16bit("teeth", "names", "bf16", got, ref, emu, names="list")
    if as_set:          # the same gradients in another order are the same set
        NC.check_fp32("teeth", "names", got, ref, names="set")
        NC.check_16bit("teeth", "names", "bf16", got, ref, emu, names="set")
    else:
        with pytest.raises(AssertionError):
            NC.check_fp32("teeth", "names", got, ref, names="set")
        with pytest.raises(AssertionError):
            NC.check_16bit("teeth", "names", "bf16", got, ref, emu, names="set")


def test_run_l1_reports_an_unused_parameter_as_asked_and_a_frozen_one_never():
    sd = {"used": torch.tensor([2.0, -3.0]), "unused": torch.ones(3), "frozen": torch.tensor([0.5])}
    forward = lambda p, x: x * p["used"].sum() + p["frozen"]
    x, t = torch.tensor([[1.0, 2.0]]), torch.zeros(1, 2)
    for frozen in (("frozen",), lambda k: k.startswith("fro")):
        y, loss, dx, g = net_ref.run_l1(forward, sd, x, t, frozen=frozen, loss_scale=4.0, missing="absent")
        assert list(g) == ["used"] and y.dtype == torch.float64 and not y.requires_grad
        # y = -x + 0.5 = (-0.5, -1.5); loss = 4 mean |y| = 4; dy = 4 sign(y) / 2 = -2: dx = -2 * -1 = 2, d used = -2 (1 + 2) = -6
        assert float(loss) == 4.0 and torch.equal(dx, torch.full((1, 2), 2.0, dtype=torch.float64))
        assert torch.equal(g["used"], torch.full((2,), -6.0, dtype=torch.float64))
        _, _, _, g0 = net_ref.run_l1(forward, sd, x, t, frozen=frozen, loss_scale=4.0, missing="zero")
        assert list(g0) == ["used", "unused"] and torch.equal(g0["unused"], torch.zeros(3, dtype=torch.float64)) and torch.equal(g0["used"], g["used"])
    with pytest.raises(AssertionError):
        net_ref.run_l1(forward, sd, x, t, missing="none")


def test_sketch_is_the_written_rule_and_reproduces_stored_values():
    v = np.random.RandomState(0).standard_normal(333)
    want = [0.0] * 64
    for i, e in enumerate(v):
        h = (i * 2654435761 + 40503) & 0xFFFFFFFF
        want[i % 64] += -e if (h >> 15) & 1 else e
    assert np.allclose(net_ref.sketch(v), want, rtol=0, atol=1e-12)
    assert np.array_equal(net_ref.sketch(torch.from_numpy(v).reshape(3, 111)), net_ref.sketch(v))
    z, (_, _, _, g) = fixture_run("mdsr_s234_idx0")
    big = [k for k in g if "gsketch64/" + k in z]
    assert len(big) >= 3
    for k in big[:3]:
        assert net_ref.rel_l2(net_ref.sketch(g[k]), z["gsketch64/" + k]) < 1e-10, k
