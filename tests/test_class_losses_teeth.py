"""CPU: the comparison the GPU tests of the class losses use (tests/class_losses_ref.py: ``worst`` <= 1 at K_RECORDED, N = 0 exact) has
teeth.  Every mutation of the restatement -- the mistakes a kernel of this kind can make -- fails it on inputs the GPU tests run, while
the unmutated float32 restatement passes it on the same inputs."""
import numpy as np
import pytest

import class_losses_ref as R


def _tie_target():
    x, t = R.nll_inputs((3, 4, 35, "any"))
    t[:, 0], t[:, 2] = 1.0, 1.0                    # the maximum twice: first = channel 0, last = channel 2
    return x, t


EDGES = (R.EDGES_X, np.ones_like(R.EDGES_X))
# mutation -> (quantity prefix, function, inputs, keyword arguments, the quantity that must fail)
CASES = {
    "alpha_swapped": ("focal", R.focal, R.flat_inputs((3, 1, 5, 7)), {}, ("loss", "grad")),
    "no_one_minus_t": ("focal", R.focal, R.flat_inputs((3, 1, 5, 7)), {}, ("loss", "grad")),
    "grad_exponent": ("focal", R.focal, R.flat_inputs((3, 1, 5, 7)), {}, ("grad",)),
    "no_clamp_mask": ("focal", R.focal, EDGES, {}, ("grad",)),
    "clamp_exclusive": ("focal", R.focal, EDGES, {}, ("grad",)),
    "nll_div_ncs": ("nll", R.nll, R.nll_inputs((3, 4, 35, "any")), {}, ("loss", "grad")),
    "argmax_last": ("nll", R.nll, _tie_target(), {}, ("loss", "grad")),
    "nll_grad_all_channels": ("nll", R.nll, R.nll_inputs((3, 4, 35, "any")), {}, ("grad",)),
    "range_last_tie": ("range", R.batch_range, (R.ties_inputs(),), {}, ("grad",)),
    "range_div_nbm": ("range", R.batch_range, (R.range_inputs((2, 105)),), {}, ("loss", "grad")),
    "range_no_min": ("range", R.batch_range, (R.range_inputs((2, 105)),), {}, ("grad",)),
    "cross_same_sample": ("cross", R.cross, R.cross_inputs((2, 3, 5, 7)), {}, ("loss", "grad")),
    "cross_last_nonzero": ("cross", R.cross, R.cross_inputs((2, 3, 5, 7)), {}, ("grad",)),
}
TAILS = (("focal", R.focal, R.flat_inputs((3, 1, 5, 7)), {}), ("focal", R.focal, R.flat_inputs((3, 4, 5, 7)), {"gamma": 1.5, "mean": False}),
         ("bce", R.bce, R.flat_inputs((3, 1, 5, 7)), {}), ("cross", R.cross, R.cross_inputs((2, 3, 5, 7)), {}))


def _worst(q, got, ref):
    return {"loss": R.worst(q + "_loss", got["loss"], ref["loss"], ref["Nloss"]),
            "grad": R.worst(q + "_grad", got["grad"], ref["grad"], ref["Ngrad"])}


def test_every_mutation_has_a_case():
    assert sorted(list(CASES) + ["drop_tail"]) == sorted(R.MUTATIONS)


@pytest.mark.parametrize("mutation", sorted(CASES))
def test_mutation_fails_the_comparison(mutation):
    q, fn, inp, kw, must_fail = CASES[mutation]
    ref = fn(*inp, **kw)
    clean = _worst(q, fn(*inp, dt=np.float32, **kw), ref)
    assert clean["loss"] <= 1 and clean["grad"] <= 1, clean
    for dt in (np.float64, np.float32):
        bad = _worst(q, fn(*inp, dt=dt, mutate=mutation, **kw), ref)
        for what in must_fail:
            assert bad[what] > 1, (mutation, what, bad)


@pytest.mark.parametrize("idx", range(len(TAILS)))
def test_a_dropped_tail_element_fails(idx):
    q, fn, inp, kw = TAILS[idx]
    ref = fn(*inp, **kw)
    clean = _worst(q, fn(*inp, dt=np.float32, **kw), ref)
    assert clean["loss"] <= 1 and clean["grad"] <= 1, clean
    bad = _worst(q, fn(*inp, dt=np.float32, mutate="drop_tail", **kw), ref)
    assert bad["loss"] > 1 and bad["grad"] > 1, bad


def test_an_inexact_zero_fails():
    """An element that must be exactly zero fails at any magnitude."""
    x, t = R.cross_inputs((2, 3, 5, 7))
    ref = R.cross(x, t)
    got = ref["grad"].copy()
    got[-1, 0] = 1e-30
    assert R.worst("cross_grad", got, ref["grad"], ref["Ngrad"]) > 1
