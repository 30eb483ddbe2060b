"""Direct tests, through the C ABI, of the f32 resamplers of csrc/elementwise.hip against torch in float64: srcgan_bilinear_up (the
F.interpolate(scale_factor=up, mode="bilinear") of the Const cascade), srcgan_bilinear_down and srcgan_nearest_resize.

Every output buffer is filled with the sentinel 1000, with 8 floats behind it that must keep it; every input is compared with its
copy.  Two kinds of assertion: EXACT -- torch.equal with the float64 reference cast to f32, where every weight is a
multiple of 1/16 and the data are integers, or where the kernel only moves data; and PER ELEMENT against float64,
|out - ref| <= 4 * 2^-24 * sum |w tap| (bilinear_bound; where sum |w tap| is itself below 2^-30 max |src| the float64 reference's own
coordinate rounding, 2^-40 max |src|, is added: see REF64).
bilinear_explicit restates the sample in float64 with the clamps spelled out, so that tests/test_groupnorm_teeth.py can show on
the CPU that it equals F.interpolate and that the comparisons notice a missing clamp or swapped weights."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
# The float64 reference's own error.  F.interpolate forms the coordinate as (o + 0.5) * (1 / up) - 0.5 in float64, off by up to 2^-52
# times the coordinate (< 2^11 at these sizes), which the lerp turns into that much of a tap difference (<= 2 max |src|): 2^-40 max |src|.
# It matters only where the exact sample sits on one pixel whose value is 0 (coordinate 3 k + 1 at up = 3): the reference is then 1e-16
# of a neighbour, not 0, and sum |w tap| is as small, so the kernel's exact 0 is 100 % of nothing away.  bilinear_bound therefore keeps
# 4 * 2^-24 * sum |w tap| for every element and adds the reference's error ONLY where sum |w tap| < 2^-30 max |src|.
REF64 = 2.0 ** -40
REF64_BELOW = 2.0 ** -30
SENT = 1000.0
UP_SIZES = [(1, 1), (1, 7), (5, 1), (2, 3), (13, 37)]
UPS = [1, 2, 3, 4, 8]


# --------------------------------------------------------------------------- references and comparisons (shared with the CPU teeth test)
def bilinear_explicit(src, up, defect=None):
    """float64 x`up` bilinear up-sampling, align_corners=False, of [N, H, W] written out: source coordinate (o + 0.5) / up - 0.5
    clamped at 0, lower neighbour its integer part, upper neighbour clamped at the border, weights 1 - l and l.
    defect: 'no_clamp_at_0', 'no_border_clamp' (the neighbour past the border reads as 0), 'weights_swapped'."""
    s64 = src.double()
    N, H, W = s64.shape

    def axis(n):
        o = torch.arange(n * up, dtype=torch.float64, device=src.device)
        s = (o + 0.5) / up - 0.5
        if defect != "no_clamp_at_0":
            s = s.clamp_min(0.0)
        i0 = s.to(torch.int64).clamp_max(n - 1)             # truncation, as the kernel's (int)s
        l = s - i0.double()
        i1 = i0 + 1
        inside = i1 <= n - 1
        if defect != "no_border_clamp":
            i1, inside = torch.where(inside, i1, i0), torch.ones_like(inside)
        w0, w1 = (l, 1.0 - l) if defect == "weights_swapped" else (1.0 - l, l)
        return i0, i1.clamp_max(n - 1), w0, w1 * inside.double()

    y0, y1, wy0, wy1 = axis(H)
    x0, x1, wx0, wx1 = axis(W)
    rows = lambda t, yi: t[:, yi]
    lerp_x = lambda t: t[:, :, x0] * wx0 + t[:, :, x1] * wx1
    return lerp_x(rows(s64, y0)) * wy0[:, None] + lerp_x(rows(s64, y1)) * wy1[:, None]


def ref_bilinear_up(src, up):
    """float64 F.interpolate and the float64 sum of the absolute weighted taps (the weights are non-negative)"""
    f = lambda t: F.interpolate(t.double().unsqueeze(0), scale_factor=up, mode="bilinear", align_corners=False)[0]
    return f(src), f(src.abs())


def bilinear_bound(n, src):
    """4 * 2^-24 * sum |w tap| per element; + REF64 max |src| only where sum |w tap| < REF64_BELOW max |src| (see REF64)"""
    m = src.abs().max().double()
    return 4 * U32 * n + torch.where(n < REF64_BELOW * m, REF64 * m, torch.zeros_like(m))


def exact(out, ref64):
    return torch.equal(out, ref64.float().reshape(out.shape))


def within(out, ref, bound):
    err = (out.double() - ref).abs()
    ok = bool((err <= bound).all())                      # a NaN anywhere fails
    return ok, float((err / bound.clamp_min(1e-300)).max())


def int_data(N, H, W, seed, device="cpu"):
    return torch.randint(-64, 65, (N, H, W), generator=torch.Generator().manual_seed(seed)).float().to(device)


def real_data(N, H, W, seed, device="cpu"):
    return torch.randn(N, H, W, generator=torch.Generator().manual_seed(seed)).to(device)


# --------------------------------------------------------------------------- the library
class Lib:
    def __init__(self):
        from srcgan_amd import _native as N
        self.N, self.lib = N, N.lib()

    def st(self):
        return self.N.stream_ptr(torch.device("cuda"))

    def _run(self, name, fn, src, out_shape, *args):
        n = 1
        for d in out_shape:
            n *= d
        dst = torch.full((n + 8,), SENT, device="cuda")
        copy = src.clone()
        self.N.check(fn(src.data_ptr(), dst.data_ptr(), *args, self.st()), name)
        assert torch.equal(src, copy), f"{name} changed its input"
        assert bool((dst[n:] == SENT).all()), f"{name} wrote past its output"
        return dst[:n].view(out_shape)

    def bilinear_up(self, src, up):
        N, H, W = src.shape
        return self._run("srcgan_bilinear_up", self.lib.srcgan_bilinear_up, src, (N, H * up, W * up), 1, N, H, W, up)

    def bilinear_down(self, src, up):
        N, H, W = src.shape
        return self._run("srcgan_bilinear_down", self.lib.srcgan_bilinear_down, src, (N, H // up, W // up), 1, N, H, W, up)

    def nearest(self, src, OH, OW, split=1):
        N, H, W = src.shape
        return self._run("srcgan_nearest_resize", self.lib.srcgan_nearest_resize, src, (N, OH, OW), split, N // split, H, W, OH, OW)


@pytest.fixture(scope="module")
def L():
    return Lib()


# --------------------------------------------------------------------------- bilinear up
@pytest.mark.parametrize("up", [1, 2, 4, 8])
def test_bilinear_up_exact_on_integers(L, up):
    """Integers in [-64, 64] and up a power of two: 1 / up, every coordinate, every weight (a multiple of 1 / 16) and every
    product and sum are exact in f32, so the output equals float64 F.interpolate cast to f32, at every size -- one-pixel axes
    (both neighbours are the same pixel), two and three pixels, 13 x 37."""
    for i, (H, W) in enumerate(UP_SIZES):
        src = int_data(3, H, W, 10 * up + i, "cuda")
        ref, _ = ref_bilinear_up(src, up)
        assert exact(L.bilinear_up(src, up), ref), (up, H, W)


@pytest.mark.parametrize("up", UPS)
def test_bilinear_up_against_float64(L, up):
    """Random reals at every factor, and integers at up = 3 (1 / 3 is rounded): per element within 4 * 2^-24 * sum |w tap|
    (bilinear_bound: the reference's own error is added only where sum |w tap| is about 0)."""
    worst = 0.0
    for i, (H, W) in enumerate(UP_SIZES):
        for src in [real_data(3, H, W, 100 * up + i, "cuda")] + ([int_data(3, H, W, 7 + i, "cuda")] if up == 3 else []):
            ref, n = ref_bilinear_up(src, up)
            ok, u = within(L.bilinear_up(src, up), ref, bilinear_bound(n, src))
            assert ok, (up, H, W, u)
            worst = max(worst, u)
    print(f"[resample] bilinear_up x{up}: worst error {worst:.3f} of the bound 4 * 2^-24 * sum |w tap|")


# --------------------------------------------------------------------------- bilinear down
@pytest.mark.parametrize("up", [2, 4, 6])
def test_bilinear_down_exact_on_integers(L, up):
    """The mean of the centre 2 x 2 of every up x up block: integers give quarters, exact.  Equal to float64
    F.interpolate(scale_factor=1 / up, mode="bilinear") cast to f32 on sizes up * {1, 3} x up * {1, 5}."""
    for h in (1, 3):
        for w in (1, 5):
            src = int_data(3, up * h, up * w, up + 10 * h + w, "cuda")
            ref = F.interpolate(src.double().unsqueeze(0), scale_factor=1.0 / up, mode="bilinear", align_corners=False)[0]
            assert ref.shape == (3, h, w)
            assert exact(L.bilinear_down(src, up), ref), (up, h, w)


def test_bilinear_down_refusals(L):
    """An odd factor and a factor that does not divide H or W are errors that name the entry point; nothing is written."""
    src = torch.zeros(3, 12, 12, device="cuda")
    dst = torch.full((3 * 12 * 12,), SENT, device="cuda")
    for H, W, up in ((12, 12, 3), (12, 12, 1), (12, 12, 8), (10, 12, 4), (12, 10, 4), (12, 12, 0)):
        with pytest.raises(RuntimeError, match="srcgan_bilinear_down"):
            L.N.check(L.lib.srcgan_bilinear_down(src.data_ptr(), dst.data_ptr(), 1, 3, H, W, up, L.st()), "srcgan_bilinear_down")
    torch.cuda.synchronize()
    assert bool((dst == SENT).all())


# --------------------------------------------------------------------------- nearest
NEAREST = ([((H, W), (H * f, W * f)) for f in (2, 3, 4) for H, W in ((1, 1), (5, 8), (7, 3))]
           + [((H * f, W * f), (H, W)) for f in (2, 3, 4) for H, W in ((1, 1), (5, 8), (7, 3))]
           + [((7, 7), (3, 3)), ((5, 5), (13, 13)), ((1, 1), (4, 4)), ((7, 5), (3, 13)), ((1, 13), (4, 5))])


def test_nearest_resize_is_torch_nearest(L):
    """Pure data movement: equal to F.interpolate(size=(OH, OW)) (mode 'nearest': source index floor(dst * in / out), the scale
    in f32), for the factors 2, 3, 4 and their inverses on odd and even sizes and the uneven pairs 7 -> 3, 5 -> 13, 1 -> 4.  For
    the factors the callers pass (2, 4, 1/2, 1/4) the scale_factor= form, which the reference uses, gives the same picture."""
    for i, ((H, W), (OH, OW)) in enumerate(NEAREST):
        src = real_data(6, H, W, 500 + i, "cuda")
        want = F.interpolate(src.unsqueeze(0), size=(OH, OW))[0]
        assert torch.equal(L.nearest(src, OH, OW, split=2), want), (H, W, OH, OW)
        for f in (2, 4):
            if (OH, OW) == (H * f, W * f):
                assert torch.equal(want, F.interpolate(src.unsqueeze(0), scale_factor=f)[0])
            if (OH * f, OW * f) == (H, W):
                assert torch.equal(want, F.interpolate(src.unsqueeze(0), scale_factor=1.0 / f)[0])


# --------------------------------------------------------------------------- more than 4096 * 256 elements
def test_second_grid_stride_trip(L):
    """Every kernel caps its grid at 4096 blocks of 256: outputs above 1 048 576 elements take a second trip of the loop.
    x2 on 3 x 600 x 300 (2.16 M outputs) for bilinear_up and nearest; bilinear_down by 2 from 3 x 1400 x 1100 (1.155 M outputs)
    and from 3 x 600 x 300."""
    src = int_data(3, 600, 300, 900, "cuda")
    ref, _ = ref_bilinear_up(src, 2)
    assert ref.numel() > 4096 * 256 and exact(L.bilinear_up(src, 2), ref)
    real = real_data(3, 600, 300, 901, "cuda")
    ref, n = ref_bilinear_up(real, 2)
    assert within(L.bilinear_up(real, 2), ref, bilinear_bound(n, real))[0]
    assert torch.equal(L.nearest(real, 1200, 600, split=3), F.interpolate(real.unsqueeze(0), size=(1200, 600))[0])
    for s in (src, int_data(3, 1400, 1100, 902, "cuda")):
        ref = F.interpolate(s.double().unsqueeze(0), scale_factor=0.5, mode="bilinear", align_corners=False)[0]
        assert exact(L.bilinear_down(s, 2), ref)
    assert ref.numel() > 4096 * 256
