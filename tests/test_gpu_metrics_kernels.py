"""Direct tests, through the C ABI, of the eight kernels of csrc/metrics.hip: ae_partial_k / fold_k (srcgan_metric_ae),
minmax_frames_partial_k / minmax_fold_k, ssim_tile_k, dssim_fold_partial_k / dssim_fold_k (srcgan_dssim3d_loss_fwd, srcgan_metric_ssim)
and dssim_bwd_k (srcgan_dssim3d_loss_bwd), each against a float64 restatement of the same operation (tests/ssim_ref.py).

  * DSSIM gradient, EVERY element: |d - d64| <= K 2^-24 N(q), N(q) the gradient's own expression with every term replaced by its
    absolute value (ssim_ref.grad_scale): it shrinks at borders and corners exactly as the gradient does, so a corner pixel, covered by
    one window position with weight w[0]^2 and 1e-7 of the tensor's largest gradient, is held as tightly as an interior one.
  * SSIM forward (a scalar): pred = truth except one block of unrelated values, the block at every place where a window position can
    be dropped, doubled or read from the neighbouring tile; |loss - loss64| <= tol_f, the metric's two outputs per image within tol_m.
  * range kernels: torch.equal with amin / amax per frame; the thresholds of the range rule through the loss they select.
  * angular error: designs of exact angles and random data against the float64 formula.
K, tol_f, tol_m and the AE tolerances are multiples of what a float32 restatement on the CPU loses against float64 (ssim_ref, recorded
there and checked by tests/test_metrics_kernels_teeth.py); none comes from what the kernels give.  No tolerance is normalised by a
tensor's maximum or norm.  Each test prints what the kernel uses of its bound ("[ssim] ..." lines, pytest -s)."""
import math

import numpy as np
import pytest
import torch

import ssim_ref as S

pytestmark = pytest.mark.gpu

GUARD = 64        # floats in front of and behind every output: 256 bytes, so the output keeps its alignment


def bits(a):
    return a.contiguous().view(torch.int32)


class Guarded:
    """n floats inside a NaN-filled buffer with GUARD floats on each side"""
    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), math.nan, device="cuda")

    def ptr(self):
        return self.buf[GUARD:].data_ptr()

    def inner(self):
        return self.buf[GUARD:GUARD + self.n]

    def check(self, what):
        assert bool(self.buf[:GUARD].isnan().all()) and bool(self.buf[GUARD + self.n:].isnan().all()), f"{what}: wrote outside its buffer"
        assert not bool(self.inner().isnan().any()), f"{what}: an element was left unwritten (or is NaN)"
        return self.inner()


class Lib:
    def __init__(self):
        from srcgan_amd import _native as N
        self.N, self.lib = N, N.lib()

    def st(self):
        return self.N.stream_ptr(torch.device("cuda"))

    def dssim_fwd(self, x, t):
        """-> (loss, range [F, 2]) of [B,C,F,H,W] device tensors; the scratch is NaN-filled: no slot may be read before it is written"""
        B, C, Fr, H, W = x.shape
        out, rng = Guarded(1), Guarded(2 * Fr)
        scr = torch.full((self.lib.srcgan_dssim3d_scratch_floats(B, C, Fr, H, W),), math.nan, device="cuda")
        self.N.check(self.lib.srcgan_dssim3d_loss_fwd(x.data_ptr(), t.data_ptr(), B, C, Fr, H, W, out.ptr(), rng.ptr(), scr.data_ptr(), self.st()),
                     "srcgan_dssim3d_loss_fwd")
        return float(out.check("loss")[0]), rng.check("range").view(Fr, 2).clone()

    def dssim_bwd(self, x, t, rng, gout, want_dt):
        B, C, Fr, H, W = x.shape
        dp, dt = Guarded(x.numel()), Guarded(x.numel()) if want_dt else None
        self.N.check(self.lib.srcgan_dssim3d_loss_bwd(x.data_ptr(), t.data_ptr(), B, C, Fr, H, W, rng.data_ptr(), gout.data_ptr(), dp.ptr(),
                                                      dt.ptr() if want_dt else None, self.st()), "srcgan_dssim3d_loss_bwd")
        return dp.check("dpred").view(x.shape), dt.check("dtruth").view(x.shape) if want_dt else None

    def metric(self, fn, x, t, nout):
        B, C, H, W = x.shape
        out = Guarded(B * nout)
        scr = torch.full((self.lib.srcgan_metric_scratch_floats(B, C, H, W),), math.nan, device="cuda")
        self.N.check(fn(x.data_ptr(), t.data_ptr(), B, C, H, W, out.ptr(), scr.data_ptr(), self.st()), "srcgan_metric")
        return out.check("metric").view(B, nout).double().cpu()

    def ssim(self, x, t):
        return self.metric(self.lib.srcgan_metric_ssim, x, t, 2)

    def ae(self, p, t):
        return self.metric(self.lib.srcgan_metric_ae, p, t, 1)[:, 0]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return Lib()


def frame_range(x):
    """[F, 2]: amin and amax of every frame of a [B,C,F,H,W] tensor"""
    return torch.stack([x.amin((0, 1, 3, 4)), x.amax((0, 1, 3, 4))], 1)


# --------------------------------------------------------------------------- 1. the DSSIM gradient, element by element
@pytest.mark.parametrize("want_dt", [True, False], ids=["dx_dt", "dx_only"])
@pytest.mark.parametrize("name", list(S.BWD_CASES))
def test_dssim_gradient_per_pixel(L, name, want_dt):
    """srcgan_dssim3d_loss_fwd then srcgan_dssim3d_loss_bwd with a device scalar gout = 3 on the case table of ssim_ref.BWD_CASES (the
    smallest shapes that reach each branch of the 32x32 output tile with its 10-pixel halo), with dtruth given and with dtruth = NULL
    (the two instances of the kernel).  Every element of dpred and dtruth within K 2^-24 N(q) of float64 autograd; the outputs sit in
    NaN-filled buffers whose guard floats stay NaN and whose every inner element is written; pred and truth keep their bits; the range
    buffer holds amin and amax of each frame of pred exactly."""
    c = S.bwd_case(name)
    x, t = c["x"].cuda(), c["t"].cuda()
    x0, t0 = x.clone(), t.clone()
    loss, rng = L.dssim_fwd(x, t)
    assert torch.equal(rng, frame_range(x0)), (rng, frame_range(x0))
    gout = torch.tensor([S.GOUT], device="cuda")
    dp, dt = L.dssim_bwd(x, t, rng, gout, want_dt)
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(x0)) and torch.equal(bits(t), bits(t0)) and float(gout) == S.GOUT
    print(f"[ssim] {name}: loss {loss:.9f}, float64 {c['loss']:.9f}, difference {abs(loss - c['loss']):.2e}")
    assert S.within(dp, c["dx"], c["Nx"], S.K, f"{name} dpred ({'with' if want_dt else 'without'} dtruth)")
    if want_dt:
        assert S.within(dt, c["dt"], c["Nt"], S.K, f"{name} dtruth")


# --------------------------------------------------------------------------- 2. SSIM forward: position probes
@pytest.mark.parametrize("shape", S.FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dssim_loss_position_probes(L, shape):
    """pred = truth, a random texture, except one block of unrelated values (ssim_ref.probe_blocks: the corners, the middle of each
    edge, across the 16-position tile seam, inside the last ragged tile, the interior; in the two-frame shape in frame 1 only):
    |loss - loss64| <= tol_f, every probe's loss being at least 100 tol_f (teeth file).  A window position dropped, counted twice or
    read from the neighbouring tile moves the probe whose block it covers."""
    worst = 0.0
    for blk in S.probe_blocks(*shape[-2:]):
        x, t = S.fwd_probe(shape, blk)
        want = float(S.loss64(x, t))
        got, rng = L.dssim_fwd(x.cuda(), t.cuda())
        assert torch.equal(rng.cpu(), frame_range(x))
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= S.TOL_F, (shape, blk, got, want)
    print(f"[ssim] loss probes {shape}: max |loss - loss64| {worst:.3e} (tol_f {S.TOL_F:.3e})")


@pytest.mark.parametrize("hw", S.METRIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metric_ssim_position_probes(L, hw):
    """srcgan_metric_ssim on B = 2, C = 1 with a different probe block in each image: out[b][0] against the float64 mean of image b's SSIM
    map and out[b][1] against its contrast mean, both within tol_m -- the per-image fold is addressed too."""
    worst = 0.0
    for i in range(len(S.probe_blocks(*hw))):
        x, t = S.metric_probe(*hw, i)
        want = S.metric64(x, t)
        got = L.ssim(x.cuda(), t.cuda())
        err = (got - want).abs()
        worst = max(worst, float(err.max()))
        assert bool((err <= S.TOL_M).all()), (hw, i, got, want)
    print(f"[ssim] metric probes {hw}: max |out - float64| {worst:.3e} (tol_m {S.TOL_M:.3e})")


# --------------------------------------------------------------------------- 3. the range kernels
@pytest.mark.parametrize("hw", [(11, 11), (257, 257)], ids=["121", "257x257"])
def test_frame_range_is_exact(L, hw):
    """F = 3, B C = 2; the per-frame extremes sit at the first element, the last element, index 255, index 256 and the last index of the
    last plane (ssim_ref.range_case).  hw = 121 is one block per frame; 257 x 257 > 256 * 256 reaches the grid-stride loop."""
    x = S.range_case(hw)
    t = x.flip(0).contiguous()
    _, rng = L.dssim_fwd(x.cuda(), t.cuda())
    assert torch.equal(rng.cpu(), frame_range(x)), (rng, frame_range(x))


def test_range_thresholds_select_the_reference_dynamic_range(L):
    """max exactly 128.0: L stays 1; 128.5: 255; min exactly -0.5: the floor stays 0; nextafter(-0.5, -1): -1.  The loss must be the
    float64 reference's with the L its rule gives (the neighbouring L is more than 1000 tol_f away: teeth file)."""
    for name, x, t, Lr in S.threshold_cases():
        want = float(S.L3.dssim2d(x[:, :, 0].double(), t[:, :, 0].double(), Lr))
        got, rng = L.dssim_fwd(x.cuda(), t.cuda())
        assert torch.equal(rng.cpu(), frame_range(x))
        print(f"[ssim] threshold {name}: |loss - loss64| {abs(got - want):.3e} (tol_f {S.TOL_F:.3e})")
        assert abs(got - want) <= S.TOL_F, (name, got, want)
        m = L.ssim(x[:, :, 0].cuda(), t[:, :, 0].cuda())
        assert abs((1 - float(m[0, 0])) / 2 - want) <= S.TOL_M, (name, m)


# --------------------------------------------------------------------------- 4. angular error
@pytest.mark.parametrize("family", ["exact", "random", "same"])
def test_metric_ae_against_float64(L, family):
    """srcgan_metric_ae, B = 2, hw in {1, 255, 256 * 64 - 1, 256 * 64 + 1} (one pixel; less than a block; one short of and one past
    64 blocks of 256), against the float64 value of the same formula, 1e-6 included.  exact: C = 3, pixels drawn from pairs at 60, 90 and
    180 degrees, a zero prediction and two zeros (both 90), another mix per image.  random: [0,1] data at C = 1 and 3.  same:
    pred = truth, which is about 0.1 degrees, not 0 -- the formula's eps makes it so, and it is pinned as such."""
    worst = 0.0
    for fam, hw, C in S.ae_cases():
        if fam != family:
            continue
        p, t = S.ae_case(fam, hw, C)
        want = S.ae64(p, t)
        got = L.ae(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()).numpy()
        assert np.isfinite(got).all()
        err = np.abs(got - want)
        worst = max(worst, float(err.max()))
        assert (err <= S.TOL_AE[fam]).all(), (fam, hw, C, got, want)
    print(f"[ssim] ae {family}: max |out - float64| {worst:.3e} degrees (tolerance {S.TOL_AE[family]:.3e})")
