"""CPU: the comparison the GPU tests make against tests/unet_ref.py has teeth -- each deliberate mistake of unet_ref.MUTATIONS, a
mistake a native U-Net could make, moves y or a live gradient far above the fp32 gate of 1e-3.

The case is five levels at ngf 16 on (1, 1, 64, 64), so the bottleneck is 2 x 2 and an InstanceNorm on the innermost level -- one of the
mistakes -- can be computed at all; the weights are the constructor's (torch's default initialisation: the biases are not zero, so a
dropped one shows)."""
import functools

import pytest
import torch
import torch.nn as nn

import unet_ref as R

N_LEVELS = 5
_BASE = {}


def base():
    if not _BASE:
        import srcgan_amd
        torch.manual_seed(21)
        m = srcgan_amd.UnetGenerator(1, 3, N_LEVELS, 16, norm_layer=functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False))
        g = torch.Generator().manual_seed(22)
        x, t = torch.rand(1, 1, 64, 64, generator=g), torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        _BASE.update(sd=sd, x=x, t=t, run=R.run(sd, x, t, N_LEVELS))
    return _BASE


def worst_error(mut):
    b = base()
    y, _, dx, g = R.run(b["sd"], b["x"], b["t"], N_LEVELS, mut=mut)
    yr, _, dxr, gr = b["run"]
    live = [k for k in gr if k not in R.dead_biases(N_LEVELS) and k in g]
    e = {"y": R.rel_l2(y, yr), "dx": R.rel_l2(dx, dxr)}
    e.update({"grad " + k: R.rel_l2(g[k], gr[k]) for k in live})
    return R.worst(e)


def test_the_unmutated_run_is_itself():
    assert worst_error(None)[1] == 0.0
    assert len(base()["run"][3]) == 4 * N_LEVELS


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_a_mistake_fails_the_gate_by_far(mut):
    k, e = worst_error(mut)
    print(f"[unet teeth] {mut}: worst error {e:.2e} ({k})")
    assert e > 3e-2 > 1e-3, (mut, k, e)


def test_the_relative_measure_fails_on_a_dead_bias_and_the_absolute_one_holds():
    from test_unet_ref import fixture_run
    z, (_, _, _, g64) = fixture_run("unet_d5_1to3")
    dead = [str(k) for k in z["dead"]]
    assert len(dead) == 7 and "model.model.3.bias" not in dead and "model.model.0.bias" not in dead
    rel = max(R.rel_l2(z["grad/" + k], g64[k]) for k in dead)                 # the reference's own float32 run against float64
    ab = max(float(z["dead_ratio/" + k]) for k in dead)
    print(f"[unet teeth] dead biases, reference f32 vs float64: relative L2 {rel:.2e}, max|g_b| / max|g_w| {ab:.2e}")
    assert rel > 1e3                                                          # any relative gate explodes
    assert ab < 1e-5 < 1e-3                                                   # the absolute one holds, with the fp32 gate's room
    assert R.dead_ratio(g64, "model.model.3.bias") > 1e-3                     # and still has teeth on a bias that is not dead
