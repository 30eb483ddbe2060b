"""CPU: the comparisons of tests/test_gpu_back_proj.py and tests/test_gpu_ddbpn.py have teeth -- each deliberate mistake in the
restatement's stride-1 route (tests/ddbpn_ref.py, ``mut``) fails the comparison the GPU tests would apply to a kernel that made it: the
bit comparison of gather and crop, the per-element bound of PReLU (ddbpn_ref.elem_excess <= 1), the bound of the slope / bias gradients
(K_RECORDED) and the networks' 1e-3 ``rel_err`` gate.  The unmutated route passes each of them.  Also re-measures K_RECORDED."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddbpn_ref as R
from conftest import load_golden, rel_err

GATE = 1e-3


def bits_equal(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("scale", R.KERNEL_SCALES)
@pytest.mark.parametrize("mut", ["offset1", "swap_ab"])
def test_gather_and_crop_mistakes_fail_the_bit_comparison(scale, mut):
    inp = R.kernel_inputs(scale, "bf16")
    s, shift, Hg, Wg, C = inp["s"], inp["shift"], inp["Hg"], inp["Wg"], inp["C"]
    x, grid = R._nchw(inp["x"]), R._nchw(inp["grid"])
    assert bits_equal(R.s2d_shift(x, s, shift, Hg, Wg), R.s2d_shift(x, s, shift, Hg, Wg, None))
    assert not bits_equal(R.s2d_shift(x, s, shift, Hg, Wg, mut), R.s2d_shift(x, s, shift, Hg, Wg))
    assert not bits_equal(R.d2s_shift(grid, C, s, shift, inp["Hy"], inp["Wy"], mut), R.d2s_shift(grid, C, s, shift, inp["Hy"], inp["Wy"]))


@pytest.mark.parametrize("scale", [4, 8])
def test_a_dropped_border_row_of_the_grid_fails_the_bit_comparison(scale):
    inp = R.kernel_inputs(scale, "fp16")
    args = (R._nchw(inp["grid"]), inp["C"], inp["s"], inp["shift"], inp["Hy"], inp["Wy"])
    assert not bits_equal(R.d2s_shift(*args, "drop_border"), R.d2s_shift(*args))
    ref, bad = R.kernel_reference(inp, "grid", 1.0, False), R.kernel_reference(inp, "grid", 1.0, False, "drop_border")
    assert R.elem_excess(bad["y"], ref["y"], ref["mag_y"], "fp16", 4) > 1.0


def test_a_channel_offset_shifted_by_4_fails_the_bit_comparison():
    inp = R.kernel_inputs(2, "fp32")
    C = inp["C"]
    buf = np.full((*inp["x"].shape[:-1], 3 * C), 1000.0)
    buf[..., C:2 * C] = inp["x"]
    gather = lambda lo: R._nhwc(R.s2d_shift(R._nchw(buf[..., lo:lo + C]), inp["s"], inp["shift"], inp["Hg"], inp["Wg"])).numpy()
    want = R._nhwc(R.s2d_shift(R._nchw(inp["x"]), inp["s"], inp["shift"], inp["Hg"], inp["Wg"])).numpy()
    assert bits_equal(gather(C), want) and not bits_equal(gather(C + 4), want)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("mut, what", [("ge", "dz"), ("beta_sign", "y")])
def test_prelu_mistakes_fail_the_per_element_bound(dtype, mut, what):
    """z >= 0 for z > 0 shows in dz at the exact zeros of z where the slope is not 1 (y is 0 there either way); the sign of beta in y."""
    inp = R.kernel_inputs(4, dtype)
    assert (inp["z"] == 0).sum() > 100 and 1.25 in R.SLOPES and 0.0 in R.SLOPES and min(R.SLOPES) < 0
    ref, bad = R.kernel_reference(inp, "plain", -1.0, False), R.kernel_reference(inp, "plain", -1.0, False, mut)
    nops = {"y": 4, "dz": 2}[what]
    assert R.elem_excess(ref[what], ref[what], ref["mag_" + what], dtype, nops) == 0.0
    assert R.elem_excess(bad[what], ref[what], ref["mag_" + what], dtype, nops) > 1.0


@pytest.mark.parametrize("form", ["plain", "grid"])
def test_slope_gradient_mistakes_fail_the_sum_bound(form):
    inp = R.kernel_inputs(8, "fp32")
    ref = R.kernel_reference(inp, form, 1.0, False)
    ta, tb = R.kernel_terms_f32(inp, form)
    da, db = R.prelu_param_sums_f32(ta, tb, R.vec_of("fp32"))
    assert R.sum_error_in_units(da, ref["terms_a"]) <= R.K_RECORDED["da"] and R.sum_error_in_units(db, ref["terms_b"]) <= R.K_RECORDED["db"]
    all_z = R.kernel_reference(inp, form, 1.0, False, "da_all")["da"]                 # summed over every z, not only z <= 0
    assert R.sum_error_in_units(all_z, ref["terms_a"]) > R.K_RECORDED["da"]
    nchunk = -(-ta.shape[0] // R.PR_CHUNK)                                            # the grid form has two chunks: either of them lost
    assert nchunk == (2 if form == "grid" else 1)
    for chunk in range(nchunk):
        da1, db1 = R.prelu_param_sums_f32(ta, tb, R.vec_of("fp32"), drop_chunk=chunk)
        assert R.sum_error_in_units(da1, ref["terms_a"]) > R.K_RECORDED["da"] and R.sum_error_in_units(db1, ref["terms_b"]) > R.K_RECORDED["db"]


@pytest.mark.parametrize("scale, mut", [(2, "noflip"), (4, "noflip"), (8, "pad_front"), (4, "bias_once"), (2, "swap_ab"), (4, "offset1")])
def test_projection_mistakes_fail_the_1e_3_gate(scale, mut):
    k, s, p = R.PROJ[scale]
    g = torch.Generator().manual_seed(7)
    x_lr = torch.randn(2, 32, 3, 5, generator=g, dtype=torch.float64)
    x_hr = torch.randn(2, 32, 3 * s, 5 * s, generator=g, dtype=torch.float64)
    wu = torch.randn(32, 32, k, k, generator=g, dtype=torch.float64) * 0.02
    wd = torch.randn(32, 32, k, k, generator=g, dtype=torch.float64) * 0.02
    b = torch.randn(32, generator=g, dtype=torch.float64) * 0.1
    up, down = F.conv_transpose2d(x_lr, wu, b, stride=s, padding=p), F.conv2d(x_hr, wd, b, stride=s, padding=p)
    assert rel_err(R.up_s1(x_lr, wu, b, scale), up) < 1e-12 and rel_err(R.down_s1(x_hr, wd, b, scale), down) < 1e-12
    bad_up, bad_down = rel_err(R.up_s1(x_lr, wu, b, scale, mut), up), rel_err(R.down_s1(x_hr, wd, b, scale, mut), down)
    assert bad_up > GATE
    if mut not in ("noflip", "bias_once"):         # (these two are mistakes of the transposed form alone)
        assert bad_down > GATE


@pytest.mark.parametrize("tag, mut", [("ddbpn_x2", "noflip"), ("ddbpn_x8", "pad_front"), ("ddbpn_x4", "bias_once"), ("ddbpn_x4", "ge")])
def test_network_mistakes_fail_the_fixture_comparison(tag, mut):
    """The mistake anywhere in the network against the reference fixture, as tests/test_gpu_ddbpn.py compares: y (and the loss with it)."""
    import srcgan_amd
    z = load_golden(tag)
    torch.manual_seed(int(z["seed"]))
    m = srcgan_amd.DDBPN(scale=int(z["scale"]), rgb_range=1)
    R.set_slopes(m, int(z["seed"]))
    sd = {k: v.double() for k, v in m.state_dict().items()}
    x = torch.from_numpy(z["x"]).double()
    with torch.no_grad():
        good, bad = R.forward(sd, x, int(z["scale"]), s1=True), R.forward(sd, x, int(z["scale"]), s1=True, mut=mut)
    assert rel_err(good, z["y"]) < GATE
    if mut == "ge":         # z >= 0 changes no forward value: it is the gradients that catch it, through the zero slopes' neighbours
        assert rel_err(bad, z["y"]) < GATE
        return
    assert rel_err(bad, z["y"]) > GATE


def test_k_recorded_is_4x_the_measured_figure_rounded_up():
    mx = {"da": 0.0, "db": 0.0}
    for dtype in ("fp32", "bf16", "fp16"):
        for scale in R.KERNEL_SCALES:
            inp = R.kernel_inputs(scale, dtype)
            for form in ("plain", "grid"):
                ref = R.kernel_reference(inp, form, 1.0, False)
                ta, tb = R.kernel_terms_f32(inp, form)
                da, db = R.prelu_param_sums_f32(ta, tb, R.vec_of(dtype))
                mx["da"] = max(mx["da"], R.sum_error_in_units(da, ref["terms_a"]))
                mx["db"] = max(mx["db"], R.sum_error_in_units(db, ref["terms_b"]))
    print(f"[bp] float32 restatement, error in units of 2^-24 * sum |terms|: da {mx['da']:.3f} db {mx['db']:.3f}")
    assert R.K_RECORDED == {k: float(math.ceil(4 * v)) for k, v in mx.items()}
