"""CPU: the references the GPU tests of the reflection-pad and tanh kernels compare against have teeth -- each deliberate mistake of
resnetgen_ref.MUTATIONS fails the comparison the GPU test makes (exact equality on small integers) -- and the relative measure fails on
a dead bias where the absolute one holds."""
import numpy as np
import pytest
import torch

import resnetgen_ref as R
from test_resnetgen_ref import fixture_run

# (B, H, W, C), p: the shapes of tests/test_gpu_reflect_pad.py (H = p + 1 and H = 2: one pixel collects three / two terms per axis)
SHAPES = [((2, 4, 9, 8), 3), ((1, 2, 2, 16), 1), ((2, 5, 4, 64), 3), ((1, 7, 6, 256), 1)]


def ints(shape, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float64)


def test_the_gather_formulation_is_the_adjoint():
    """R(i, H) of the kernel's description, evaluated here in plain Python, against the scatter of resnetgen_ref.reflect_pad_bwd"""
    def readers(i, n, p):
        return ([p - i] if 1 <= i <= p else []) + [i + p] + ([p + 2 * (n - 1) - i] if n - 1 - p <= i <= n - 2 else [])
    for (B, H, W, C), p in SHAPES:
        dy = ints((B, H + 2 * p, W + 2 * p, C), 1)
        ref, _ = R.reflect_pad_bwd(dy, H, W, p)
        got = np.zeros_like(ref)
        for i in range(H):
            for j in range(W):
                for a in readers(i, H, p):
                    for b in readers(j, W, p):
                        got[:, i, j] += dy[:, a, b]
        assert np.array_equal(got, ref)
        assert max(len(readers(i, H, p)) for i in range(H)) == (3 if H <= 2 * p + 1 and H > 2 else 2)
    # <x, pad^T dy> == <pad x, dy>
    x, dy = ints((2, 4, 9, 8), 2), ints((2, 10, 15, 8), 3)
    assert float((R.reflect_pad(x, 3) * dy).sum()) == float((x * R.reflect_pad_bwd(dy, 4, 9, 3)[0]).sum())


def test_the_band_wise_formulation_is_the_adjoint_too():
    for (B, H, W, C), p in SHAPES + [((1, 11, 9, 8), 3)]:
        dy = ints((B, H + 2 * p, W + 2 * p, C), 9)
        ref, _ = R.reflect_pad_bwd(dy, H, W, p)
        cuts = [0, H] if H < 4 else [0, 1, H // 2, H]
        got = torch.cat([R.reflect_pad_bwd_rows(torch.from_numpy(dy), H, W, p, a, b) for a, b in zip(cuts, cuts[1:])], 1)
        assert np.array_equal(got.double().numpy(), ref)


def test_the_forward_reference_is_torch_reflection_padding():
    for (B, H, W, C), p in SHAPES:
        x = ints((B, H, W, C), 4)
        t = torch.nn.functional.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (p, p, p, p), mode="reflect").permute(0, 2, 3, 1).numpy()
        assert np.array_equal(R.reflect_pad(x, p), t)


@pytest.mark.parametrize("mut", ["dropped_mirror", "symmetric", "replicate", "swapped_axes", "acc_overwrites", "term_twice"])
def test_pad_backward_mutations_fail_the_exact_comparison(mut):
    failed = 0
    for (B, H, W, C), p in SHAPES:
        dy, old = ints((B, H + 2 * p, W + 2 * p, C), 5), ints((B, H, W, C), 6)
        ref, _ = R.reflect_pad_bwd(dy, H, W, p, old=old)
        bad, _ = R.reflect_pad_bwd(dy, H, W, p, old=old, mut=mut)
        assert np.abs(ref).max() <= 10 * 8
        failed += not np.array_equal(ref, bad)
    assert failed >= (3 if mut == "swapped_axes" else 4)      # H == W hides a swap of the axes


@pytest.mark.parametrize("mut", ["symmetric", "replicate", "swapped_axes"])
def test_pad_forward_mutations_fail_the_exact_comparison(mut):
    for (B, H, W, C), p in SHAPES:
        x = ints((B, H, W, C), 7)
        if mut == "swapped_axes" and H == W:
            continue
        assert not np.array_equal(R.reflect_pad(x, p), R.reflect_pad(x, p, mut=mut))


def test_tanh_backward_from_the_input_fails_the_bound():
    """the GPU test's bound: 4 x max(2^-24, numpy float32 tanh's own error) x |dy|"""
    z = np.linspace(-12, 12, 4097)
    y, dy = np.tanh(z), np.random.default_rng(8).uniform(-1, 1, z.shape)
    eps = 4 * max(2.0 ** -24, float(np.abs(np.tanh(z.astype(np.float32)).astype(np.float64) - y).max()))
    ref = R.tanh_bwd(dy, y)
    assert np.abs(R.tanh_bwd(dy, y, z=z, mut="tanh_from_z") - ref).max() > 1.0 > eps
    old = np.ones_like(z)
    assert np.abs(R.tanh_bwd(dy, y, old=old, mut="acc_overwrites") - R.tanh_bwd(dy, y, old=old)).max() == 1.0
    # and near saturation 1 - y^2 cancels: a relative bound would ask for digits that y does not hold
    y32 = np.tanh(z.astype(np.float32)).astype(np.float64)
    sat = np.abs(z) > 8
    assert np.abs(R.tanh_bwd(dy, y32) - ref)[sat].max() <= eps * np.abs(dy[sat]).max()
    assert (np.abs(R.tanh_bwd(dy, y32) - ref)[sat] / np.abs(ref[sat])).max() > 1e-2


def test_the_relative_measure_fails_on_a_dead_bias_and_the_absolute_one_holds():
    z, (_, _, _, g64) = fixture_run("resnetgen_1to3")
    dead = [str(k) for k in z["dead"]]
    assert len(dead) == 17 and "model.23.bias" not in dead
    rel = max(R.rel_l2(z["grad/" + k], g64[k]) for k in dead)                 # the reference's own float32 run against float64
    ab = max(float(z["dead_ratio/" + k]) for k in dead)
    print(f"[resnetgen teeth] dead biases, reference f32 vs float64: relative L2 {rel:.2e}, max|g_b| / max|g_w| {ab:.2e}")
    assert rel > 1e3                                                          # any relative gate explodes
    assert ab < 1.1e-6 < 1e-3                                                 # the absolute one holds, with the fp32 gate's room
    # and the absolute measure still has teeth: a bias gradient that is NOT dead (the last layer's) is far above the gate
    assert R.dead_ratio(g64, "model.23.bias") > 1e-3
