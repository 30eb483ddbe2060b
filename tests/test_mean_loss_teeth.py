"""CPU: the comparisons the GPU tests of the flat mean losses use (tests/mean_loss_ref.py) have teeth.  Every single-mistake variant of
the restatement fails them at a case of the GPU table, and the true float32 restatement passes every case of the table."""
import numpy as np
import pytest

import mean_loss_ref as R

_CACHE = {}


def _exact(kind, n):
    if ("e", kind, n) not in _CACHE:
        _CACHE["e", kind, n] = R.exact_inputs(kind, n)
    return _CACHE["e", kind, n]


def _real(kind, n):
    if ("r", kind, n) not in _CACHE:
        _CACHE["r", kind, n] = R.real_inputs(kind, n)
    return _CACHE["r", kind, n]


def _f32_value(kind, a, b, label, mutate=None):
    """The float32 restatement of the forward: f32 terms, f32 sums (numpy's own order), one product by f32(1 / n)."""
    e, _ = R._terms(kind, a, b, label, np.float32, mutate)
    w = R._weights(len(a), mutate).astype(np.float32)
    count = len(a) - 1 if mutate == "div_n_minus_1" and len(a) > 1 else len(a)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.sum(e * w, dtype=np.float32) * np.float32(1.0 / count))


# ------------------------------------------------------------------------------------------------ the true restatement passes the table
@pytest.mark.parametrize("n", R.LENGTHS)
@pytest.mark.parametrize("kind", R.EXACT_KINDS)
def test_true_restatement_passes_the_exact_table(kind, n):
    a, b = _exact(kind, n)
    for label in R.EXACT_RANGE[kind][1]:
        ref = R.forward(kind, a, b, label)
        assert R.exact_forward_ok(kind, n, _f32_value(kind, a, b, label), ref)
        if kind in (0, 4):
            for gout in R.GOUTS:
                for gscale in R.GSCALES:
                    want = R.backward(kind, a, b, label, gout, gscale, dt=np.float32)["grad"]
                    g = R.upstream32(gout, gscale, n)                       # written out once more: sign * g and label * g are exact
                    direct = np.where(a > b, g, np.where(a < b, -g, np.float32(0))) if kind == 0 else np.full(n, np.float32(label) * g)
                    assert R.exact_backward_ok(direct, want)
    if kind == 0:
        g = R.backward(0, a, b, 0.0, 1.0, 1.0, dt=np.float32)["grad"]
        assert ((a == b).any() or n < 1023) and np.all(g[a == b] == 0)


@pytest.mark.parametrize("n", R.LENGTHS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_true_restatement_passes_the_float64_table(kind, n):
    a, b = _real(kind, n)
    label = R.real_label(kind)
    ref = R.forward(kind, a, b, label)
    for pa, pb in ((0, None), (4, 4), (4, 8)):
        assert R.value_ok(kind, n, _f32_value(kind, a, b, label), ref, pa, pb if kind < 2 else None)
    if kind in (1, 2, 3):
        for gscale in R.GSCALES:
            r64 = R.backward(kind, a, b, label, 3.0, gscale)
            assert R.grad_ok(kind, R.backward(kind, a, b, label, 3.0, gscale, dt=np.float32)["grad"], r64)


def test_true_psnr_passes():
    for mse in R.PSNR_MSE:
        assert R.psnr_ok(mse, R.psnr(mse, np.float32)), mse
    assert R.psnr(0.0, np.float32) == np.inf


def test_geometry_of_the_aligned_launch():
    """The figures the issue's lengths were chosen for."""
    g = R.geometry(1048572)
    assert (g["blocks"], g["nv"], g["ns"], g["per_thread"]) == (1024, 262143, 0, 5)
    assert R.geometry(1048568)["blocks"] == 1024 and R.geometry(1048564)["blocks"] == 1024 and R.geometry(1048560)["blocks"] == 1024
    assert R.geometry(1047548)["blocks"] == 1023                              # the grid below the cap
    g = R.geometry(1048576)
    assert (g["blocks"], g["nv"], g["per_thread"]) == (1024, 262144, 5)        # the capped grid filled exactly once
    g = R.geometry(2097157)
    assert (g["nv"], g["ns"], g["per_thread"]) == (524289, 1, 4 * 3 + 1)       # two full trips, one group in a third, a tail of one
    assert R.geometry(5, 4)["head"] == 3 and R.geometry(5, 4)["nv"] == 0 and R.geometry(7, 12)["nv"] == 1
    assert R.geometry(1027, 4, 8)["ns"] == 1027 and R.geometry(1027, 4, 8)["blocks"] == 5
    for n in R.LENGTHS:
        for kind in R.EXACT_KINDS:
            assert n * R.EXACT_RANGE[kind][2] < 2 ** 24


# ------------------------------------------------------------------------------------------------ every mutant is caught
# mutation -> (kind, n, which comparison must fail)
CASES = {
    "drop_tail": [(0, 5, "exact_value"), (1, 1048579, "exact_value"), (4, 2097157, "exact_value"), (0, 1027, "value")],
    "head_twice": [(0, 1, "exact_value"), (2, 1048577, "exact_value"), (1, 1027, "value")],
    "skip_at_cap": [(0, 1048577, "exact_value"), (1, 2097157, "exact_value"), (4, 1048579, "exact_value")],
    "div_n_minus_1": [(0, 1048576, "exact_value"), (1, 2097157, "exact_value"), (0, 2097157, "exact_grad"), (2, 1027, "grad"),
                      (3, 1027, "grad")],
    "signed_label_flipped": [(4, 7, "exact_value"), (4, 7, "exact_grad")],
    "target_grad_not_negated": [(0, 7, "exact_grad"), (1, 1027, "grad")],
    "sign0_is_1": [(0, 1027, "exact_grad")],
    "bce_not_stable": [(3, 1027, "value32")],
}


def test_every_mutation_has_a_case():
    assert sorted(CASES) == sorted(R.MUTATIONS)


@pytest.mark.parametrize("mutation", sorted(CASES))
def test_mutation_fails_the_comparison(mutation):
    for kind, n, what in CASES[mutation]:
        gscale = -1.0 if mutation == "target_grad_not_negated" else 1.0
        if what.startswith("exact"):
            a, b = _exact(kind, n)
            label = R.EXACT_RANGE[kind][1][-1]
            ref = R.forward(kind, a, b, label)
            if what == "exact_value":
                bad = R.forward(kind, a, b, label, mutate=mutation)
                assert R.exact_forward_ok(kind, n, R.exact_value(ref["sum"], n), ref)
                assert not R.exact_forward_ok(kind, n, R.exact_value(bad["sum"], bad["count"]), ref), (mutation, kind, n)
                assert not R.exact_forward_ok(kind, n, _f32_value(kind, a, b, label, mutation), ref), (mutation, kind, n)
            else:
                want = R.backward(kind, a, b, label, 3.0, gscale, dt=np.float32)["grad"]
                bad = R.backward(kind, a, b, label, 3.0, gscale, dt=np.float32, mutate=mutation)["grad"]
                assert R.exact_backward_ok(want.copy(), want)
                assert not R.exact_backward_ok(bad, want), (mutation, kind, n)
        else:
            a, b = _real(kind, n)
            label = R.real_label(kind)
            if what in ("value", "value32"):
                ref = R.forward(kind, a, b, label)
                assert R.value_ok(kind, n, _f32_value(kind, a, b, label), ref)
                assert not R.value_ok(kind, n, _f32_value(kind, a, b, label, mutation), ref), (mutation, kind, n)
                if what == "value":                       # a mistake in float64 as well ('bce_not_stable' is none: float64 does not overflow)
                    assert not R.value_ok(kind, n, R.forward(kind, a, b, label, mutate=mutation)["loss"], ref), (mutation, kind, n)
            else:
                ref = R.backward(kind, a, b, label, 3.0, gscale)
                assert R.grad_ok(kind, R.backward(kind, a, b, label, 3.0, gscale, dt=np.float32)["grad"], ref)
                for dt in (np.float64, np.float32):
                    assert not R.grad_ok(kind, R.backward(kind, a, b, label, 3.0, gscale, dt=dt, mutate=mutation)["grad"], ref), (mutation, kind, n)


def test_a_nan_fails_every_comparison():
    a, b = _real(1, 1027)
    ref = R.forward(1, a, b, 0.0)
    assert not R.value_ok(1, 1027, np.float32("nan"), ref)
    r = R.backward(1, a, b, 0.0, 1.0, 1.0)
    g = r["grad"].astype(np.float32)
    g[17] = np.nan
    assert not R.grad_ok(1, g, r)
    ae, be = _exact(0, 7)
    want = R.backward(0, ae, be, 0.0, 1.0, 1.0, dt=np.float32)["grad"]
    bad = want.copy()
    bad[3] = np.nan
    assert not R.exact_backward_ok(bad, want)
    assert not R.psnr_ok(0.25, np.float32("nan"))


def test_one_ulp_fails_the_exact_comparison():
    a, b = _exact(1, 1048579)
    ref = R.forward(1, a, b, 0.0)
    v = R.exact_value(ref["sum"], len(a))
    assert not R.exact_forward_ok(1, len(a), np.nextafter(v, np.float32(np.inf)), ref)
