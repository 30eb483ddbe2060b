"""CPU: the comparisons of tests/test_gpu_chan_attn.py have teeth, and their tolerances are what tests/chan_attn_ref.py says they are.

  * every mutation of the numpy restatement (chan_attn_ref.MUTATIONS), evaluated in float64 -- so nothing but the mistake separates it
    from the reference -- is caught by the per-element comparison of the quantity it spoils, at every storage type's tolerance, on cases
    of the GPU grid;
  * K_RECORDED is 4 x the float32 restatement's own largest error over the whole grid and the three storage types, rounded up to the
    next integer, and the restatement itself passes every comparison with room to spare."""
import math

import numpy as np
import pytest

import chan_attn_ref as R

# the quantity each mutation must spoil, and what a case needs for the mutation to change anything
SPOILS = {"pool_drops_pixel": ("p", lambda c: c[1] > 1), "pool_padded_count": ("p", lambda c: True),
          "gate_of_next_sample": ("y", lambda c: c[0] > 1), "no_sigmoid_derivative": ("db2", lambda c: True),
          "no_relu_mask": ("dt", lambda c: c[3] >= 4), "no_dp_term": ("dt", lambda c: True),
          "dres_stored": ("dres", lambda c: c[5] == 1), "dw2_one_sample": ("dw2", lambda c: c[0] > 1)}


def test_every_mutation_is_listed():
    assert set(SPOILS) == set(R.MUTATIONS)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutation_is_noticed(mutation, dtype):
    q, applies = SPOILS[mutation]
    cases = [c for c in R.grid_cases() if applies(c)]
    assert len(cases) >= 12
    caught = 0
    for case in cases[::4]:                            # (a stride coprime to the three Cr values that follow one another in the grid)
        inp = R.make_inputs(case, dtype)
        ref, bad = R.reference(inp), R.reference(inp, mutate=mutation)
        N = R.scales(inp["t"], inp["res"], inp["g"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], inp["old"])
        if all(np.array_equal(bad[k], ref[k]) for k in R.QUANTITIES):
            continue                                   # the mistake changes nothing here (every hidden unit on, or every one off: Cr = 1)
        assert R.worst(q, bad[q], ref[q], N[q], dtype) > 1.0, (mutation, case)
        caught += 1
    assert caught >= 4


def test_recorded_k_is_four_times_the_restatements_error():
    measured = {q: 0.0 for q in R.QUANTITIES}
    for dtype in ("fp32", "bf16", "fp16"):
        for q, v in R.measure_k(dtype).items():
            measured[q] = max(measured[q], v)
    print("[ca] float32 restatement, largest error in units of 2^-24 N:", {q: round(v, 2) for q, v in measured.items()})
    for q in R.QUANTITIES:
        want = 4.0 * measured[q]
        assert want <= R.K_RECORDED[q] <= math.ceil(want) + 1e-9, (q, measured[q], R.K_RECORDED[q])


def test_restatement_passes_with_room():
    for dtype in ("fp32", "bf16", "fp16"):
        for case in R.grid_cases()[::7]:
            inp = R.make_inputs(case, dtype)
            ref = R.reference(inp)
            N = R.scales(inp["t"], inp["res"], inp["g"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], inp["old"])
            f = R.forward(inp["t"], inp["res"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], dt=np.float32)
            b = R.backward(inp["g"], inp["t"], inp["w1"], inp["w2"], f, inp["old"], dt=np.float32)
            for q, v in {**f, **b}.items():
                assert R.worst(q, v, ref[q], N[q], dtype) <= 0.25 + 1e-9, (q, case, dtype)
