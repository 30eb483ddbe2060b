"""The comparisons of tests/test_gpu_nearest.py have teeth: on the CPU, nearest_ref's restatement is compared, through the GPU
file's own comparison functions and on the GPU file's own data, with copies of itself that each make one mistake a shift-search kernel
can make.  Every such comparison must fail and the unperturbed one must pass.  The file also holds every float-valued case (the
fixture's and the generated ones) to the margin condition that makes the selection immune to float32 rounding.  No kernel runs here."""
import numpy as np
import pytest

import nearest_ref as R
import test_gpu_nearest as T
from conftest import load_golden


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


@pytest.mark.parametrize("name", T.NAMES)
def test_unperturbed_restatement_passes_every_comparison(name):
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, ref = T.int_ref(name)
    assert ref["diff"].max() < 2 ** 24 and np.array_equal(ref["diff"], np.round(ref["diff"]))
    again = R.l1(o.numpy(), t.numpy(), shift, stride)
    assert T.same_values(_f32(again["diff"]), ref["diff"]) and T.same_values(again["sel"].astype(np.int32), ref["sel"])
    assert T.same_values(R.crops(o.numpy(), t.numpy(), shift, stride)[1], ref["tgt_"])
    assert T.within_one_ulp(np.float32(again["loss"]), ref["loss"])
    assert T.within_gate(_f32(again["dout"]), ref["dout"]) and T.within_gate(_f32(again["dtgt"]), ref["dtgt"])
    fo, ft, planted, fref = T.float_ref(name)
    assert T.within_gate(_f32(fref["diff"]), fref["diff"]) and T.same_values(fref["sel"], planted.numpy())


def _mutant_is_caught(name, defect):
    """the integer comparisons (exact sums, selection, crops, gradients) and the float ones (gate on the sums, exact selection)"""
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, ref = T.int_ref(name)
    bad = R.l1(o.numpy(), t.numpy(), shift, stride, defect=defect)
    _, bad_tgt, _ = R.crops(o.numpy(), t.numpy(), shift, stride, defect=defect)
    fo, ft, _, fref = T.float_ref(name)
    fbad = R.l1(fo.numpy(), ft.numpy(), shift, stride, defect=defect)
    return {
        "int_diff": not T.same_values(_f32(bad["diff"]), ref["diff"]),
        "int_sel": not T.same_values(bad["sel"], ref["sel"]),
        "int_crop": not T.same_values(bad_tgt, ref["tgt_"]),
        "int_grad": not (T.same_values(_f32(bad["dout"]), _f32(ref["dout"])) and T.same_values(_f32(bad["dtgt"]), _f32(ref["dtgt"]))),
        "float_diff": not T.within_gate(_f32(fbad["diff"]), fref["diff"]),
        "float_sel": not T.same_values(fbad["sel"], fref["sel"]),
        "float_loss": not abs(fbad["loss"] - fref["loss"]) <= T.GATE * fref["loss"],
    }


def test_r_and_c_swapped():
    for name in ("golden", "nonsquare", "tiles"):
        c = _mutant_is_caught(name, "rc_swapped")
        assert c["int_sel"] and c["int_crop"] and c["int_grad"] and c["float_sel"] and c["float_loss"], (name, c)


def test_candidate_index_off_by_one():
    for name in T.NAMES:
        c = _mutant_is_caught(name, "candidate_off_by_one")
        assert c["int_diff"] and c["float_diff"], (name, c)


def test_last_minimum_instead_of_first():
    """only a tie tells the two rules apart: the constant-target case of the GPU file"""
    B, C, H, W, shift, stride = R.SHAPES["nonsquare"]
    o = R.int_case("nonsquare", 7)[0].numpy()
    t = np.full_like(o, 3.0)
    diff = R.shift_diff(o, t, shift, stride)
    assert (diff == diff[:, :1]).all()
    assert T.same_values(R.select(diff, 2 * shift), np.zeros((B, 2)))
    assert not T.same_values(R.select(diff, 2 * shift, "last_minimum"), np.zeros((B, 2)))


def test_stride_ignored():
    c = _mutant_is_caught("stride2", "stride_ignored")
    assert c["int_diff"] and c["int_crop"] and c["int_grad"] and c["float_diff"], c


def test_dropped_edge_row():
    for name in T.NAMES:
        c = _mutant_is_caught(name, "edge_row_dropped")
        assert c["int_diff"], (name, c)
    for name in ("tiny", "golden", "shift3"):           # one row of 3 .. 24: above the gate; of 96 (tiles) it is the exact case's to catch
        assert _mutant_is_caught(name, "edge_row_dropped")["float_diff"], name


def test_apron_one_short():
    for name in T.NAMES:
        c = _mutant_is_caught(name, "apron_short")
        assert c["int_diff"], (name, c)


def test_crop_row_as_the_column_extent():
    for name in ("nonsquare", "one_tile"):
        B, C, H, W, shift, stride = R.SHAPES[name]
        assert H != W
        assert _mutant_is_caught(name, "crop_row_for_columns")["int_crop"], name


def test_every_defect_is_exercised():
    import inspect
    src = inspect.getsource(inspect.getmodule(test_every_defect_is_exercised))
    for d in R.DEFECTS:
        assert src.count(f'"{d}"') >= 1, d


# --------------------------------------------------------------------------- the margin condition of every float-valued case
@pytest.mark.parametrize("name", T.NAMES)
def test_generated_float_cases_have_a_clear_winner(name):
    fo, ft, planted, fref = T.float_ref(name)
    m = R.margin(fref["diff"])
    assert m.min() > R.MARGIN, (name, m)
    assert np.array_equal(fref["sel"], planted.numpy())
    assert np.array_equal(fo.numpy(), fo.half().float().numpy()) and np.array_equal(ft.numpy(), ft.half().float().numpy())


@pytest.mark.parametrize("case", ["golden", "stride2", "shift3", "nonsquare"])
def test_fixture_cases_have_a_clear_winner(case):
    g = load_golden("nearest_selector")
    shift, stride = (int(v) for v in g[f"{case}/cfg"])
    assert g[f"{case}/x"].dtype == np.float16 and g[f"{case}/t"].dtype == np.float16
    m = R.margin(R.shift_diff(g[f"{case}/x"].astype(np.float64), g[f"{case}/t"].astype(np.float64), shift, stride))
    assert m.min() > R.MARGIN, (case, m)
