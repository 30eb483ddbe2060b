"""Direct tests, through the C ABI, of the back-projection kernels (csrc/back_proj.hip): srcgan_s2d_shift, srcgan_d2s_shift,
srcgan_prelu_forward and srcgan_prelu_backward on the cases of tests/ddbpn_ref.py (kernel_inputs): scales 2, 4, 8, B = 2, LR 3 x 5,
C = 32; every operand once dense and once as channels [32, 64) of a 96-channel buffer; fp32, bf16, fp16.

Gather and crop are bit-exact.  PReLU forward, dz and dres are held per element to float64 of the stored inputs (ddbpn_ref.elem_excess:
a few float32 roundings + one of the storage type); da / db to K * 2^-24 * sum |terms| with K = ddbpn_ref.K_RECORDED (4 x the float32
restatement's own error, tests/test_back_proj_teeth.py).  Slopes include 0, a negative value and 1.25, z holds exact zeros.  Each
backward runs twice and the two runs' bits are compared.  The maxima are printed ("[bp] ..." lines, pytest -s)."""
import numpy as np
import pytest
import torch

import ddbpn_ref as R

pytestmark = pytest.mark.gpu
SENT = 1000.0
LAYOUTS = {"dense": (1, 0), "slice": (3, 1)}        # (buffer channels / C, slice index)


class Lib:
    def __init__(self):
        from srcgan_amd import _native as N
        self.N, self.lib = N, N.lib()

    def st(self):
        return self.N.stream_ptr(torch.device("cuda"))


@pytest.fixture(scope="module")
def L():
    return Lib()


class Buf:
    """An NHWC tensor of ``ch`` channels living as slice ``idx`` of a buffer ``mult`` times as wide; everything else holds a sentinel."""

    def __init__(self, a, dtype, layout, shape=None):
        mult, idx = LAYOUTS[layout]
        shape = tuple(a.shape) if a is not None else shape
        self.ch, self.cs, self.lo = shape[-1], shape[-1] * mult, shape[-1] * idx
        self.t = torch.full((*shape[:-1], self.cs), SENT, device="cuda", dtype=R.TDT[dtype])
        if a is not None:
            self.view().copy_(torch.from_numpy(np.ascontiguousarray(a)).to(R.TDT[dtype]))

    def view(self):
        return self.t[..., self.lo:self.lo + self.ch]

    def ptr(self):
        return self.t.data_ptr() + self.lo * self.t.element_size()

    def get(self):
        """the slice as float64 numpy; asserts that nothing outside it was written"""
        outside = torch.ones(self.cs, dtype=torch.bool, device="cuda")
        outside[self.lo:self.lo + self.ch] = False
        assert bool((self.t[..., outside] == SENT).all()), "wrote outside the channel slice"
        return self.view().double().cpu().numpy()


def geom(inp):
    return inp["B"], inp["Hy"], inp["Wy"], inp["C"], inp["s"], inp["shift"], inp["Hg"], inp["Wg"]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("scale", R.KERNEL_SCALES)
def test_gather_and_crop_are_bit_exact(L, scale, layout, dtype):
    inp = R.kernel_inputs(scale, dtype)
    B, Hy, Wy, C, s, shift, Hg, Wg = geom(inp)
    did = L.N.dtype_id(dtype)
    x, g = Buf(inp["x"], dtype, layout), Buf(None, dtype, layout, (B, Hg, Wg, s * s * C))
    L.N.check(L.lib.srcgan_s2d_shift(x.ptr(), x.cs, g.ptr(), g.cs, B, Hy, Wy, C, s, shift, Hg, Wg, did, L.st()), "srcgan_s2d_shift")
    want = R._nhwc(R.s2d_shift(R._nchw(inp["x"]), s, shift, Hg, Wg)).numpy()
    assert np.array_equal(g.get(), want)
    # the crop of the gathered grid gives the image back; of a random grid, the restatement's crop; accumulate adds once
    src, y = Buf(inp["grid"], dtype, layout), Buf(inp["old"], dtype, layout)
    L.N.check(L.lib.srcgan_d2s_shift(src.ptr(), src.cs, y.ptr(), y.cs, B, Hy, Wy, C, s, shift, Hg, Wg, 0, did, L.st()), "srcgan_d2s_shift")
    crop = R._nhwc(R.d2s_shift(R._nchw(inp["grid"]), C, s, shift, Hy, Wy)).numpy()
    assert np.array_equal(y.get(), crop)
    back = Buf(None, dtype, layout, (B, Hy, Wy, C))
    L.N.check(L.lib.srcgan_d2s_shift(g.ptr(), g.cs, back.ptr(), back.cs, B, Hy, Wy, C, s, shift, Hg, Wg, 0, did, L.st()), "srcgan_d2s_shift")
    assert np.array_equal(back.get(), inp["x"])
    acc = Buf(inp["old"], dtype, layout)
    L.N.check(L.lib.srcgan_d2s_shift(src.ptr(), src.cs, acc.ptr(), acc.cs, B, Hy, Wy, C, s, shift, Hg, Wg, 1, did, L.st()), "srcgan_d2s_shift")
    # the float32 sum of the two stored values (the float64 sum of two such values is exact, so its rounding is the float32 sum), stored once
    assert np.array_equal(acc.get(), torch.from_numpy((inp["old"] + crop).astype(np.float32)).to(R.TDT[dtype]).double().numpy())


def run_prelu(L, inp, form, beta, accumulate, layout, dtype):
    B, Hy, Wy, C, s, shift, Hg, Wg = geom(inp)
    if form == "plain":
        s, shift, Hg, Wg = 1, 0, Hy, Wy
    did = L.N.dtype_id(dtype)
    p = lambda t: None if t is None else t.data_ptr()
    z = Buf(inp["z"] if form == "plain" else inp["grid"], dtype, layout)
    r, dy = Buf(inp["r"], dtype, layout), Buf(inp["dy"], dtype, layout)
    y = Buf(None, dtype, layout, (B, Hy, Wy, C))
    slope = torch.from_numpy(inp["slope"]).cuda()
    bias = None if form == "plain" else torch.from_numpy(inp["bias"]).cuda()
    L.N.check(L.lib.srcgan_prelu_forward(z.ptr(), z.cs, p(slope), p(bias), r.ptr(), r.cs, beta, y.ptr(), y.cs, B, Hy, Wy, C, s, shift, Hg, Wg, did, L.st()),
              "srcgan_prelu_forward")
    out = {"y": y.get()}
    runs = []
    for _ in range(2):
        dz = Buf(None, dtype, layout, tuple(z.view().shape))
        dres = Buf(inp["old"] if accumulate else None, dtype, layout, (B, Hy, Wy, C))
        n = L.lib.srcgan_prelu_scratch_floats(B, Hg, Wg, C, s)
        scr = torch.full((n + 8,), float("nan"), device="cuda")
        scr[n:] = SENT
        da, db = torch.full((C + 8,), SENT, device="cuda"), torch.full((C + 8,), SENT, device="cuda")
        L.N.check(L.lib.srcgan_prelu_backward(dy.ptr(), dy.cs, z.ptr(), z.cs, p(slope), p(bias), dz.ptr(), dz.cs, dres.ptr(), dres.cs, beta, int(accumulate),
                                              p(da), p(db) if bias is not None else None, B, Hy, Wy, C, s, shift, Hg, Wg, did, p(scr), L.st()),
                  "srcgan_prelu_backward")
        assert bool((scr[n:] == SENT).all()) and bool((da[C:] == SENT).all()) and bool((db[C:] == SENT).all()), "wrote past a buffer"
        if bias is None:
            assert bool((db == SENT).all())
        runs.append((dz.t.clone(), dres.t.clone(), da.clone(), db.clone()))
        out.update(dz=dz.get(), dres=dres.get(), da=da[:C].double().cpu().numpy(), db=db[:C].double().cpu().numpy() if bias is not None else None)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two runs differ in their bits"
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("scale", R.KERNEL_SCALES)
def test_prelu_per_element_against_float64(L, scale, layout, dtype):
    inp = R.kernel_inputs(scale, dtype)
    mx = {}
    for form, beta, accumulate in (("plain", -1.0, False), ("plain", 1.0, True), ("grid", 1.0, False), ("grid", -1.0, True)):
        got = run_prelu(L, inp, form, beta, accumulate, layout, dtype)
        ref = R.kernel_reference(inp, form, beta, accumulate)
        fig = {"y": R.elem_excess(got["y"], ref["y"], ref["mag_y"], dtype, 4),
               "dz": R.elem_excess(got["dz"], ref["dz"], ref["mag_dz"], dtype, 2),
               "dres": R.elem_excess(got["dres"], ref["dres"], ref["mag_dres"], dtype, 2),
               "da": R.sum_error_in_units(got["da"], ref["terms_a"]) / R.K_RECORDED["da"]}
        if got["db"] is not None:
            fig["db"] = R.sum_error_in_units(got["db"], ref["terms_b"]) / R.K_RECORDED["db"]
        for k, v in fig.items():
            mx[k] = max(mx.get(k, 0.0), v)
        if form == "plain":     # exact zeros of z: y there is beta * r alone, and dz is slope * dy (z > 0 is false at 0), to the bit
            zero = inp["z"] == 0
            assert zero.sum() > 100 and np.array_equal(got["y"][zero], (beta * inp["r"])[zero])
            sd = torch.from_numpy(inp["slope"][None, None, None, :] * inp["dy"].astype(np.float32)).to(R.TDT[dtype]).double().numpy()
            assert np.array_equal(got["dz"][zero], sd[zero])
    print(f"[bp] x{scale} {layout} {dtype}: largest error / bound " + " ".join(f"{k} {v:.3f}" for k, v in mx.items()))
    assert all(v <= 1.0 for v in mx.values()), mx


def test_errors_name_the_entry_point(L):
    t = torch.zeros(2 * 4 * 4 * 32, device="cuda")
    p = t.data_ptr()
    lib = L.lib
    assert lib.srcgan_s2d_shift(p, 32, p, 128, 1, 4, 4, 32, 2, 0, 1, 1, L.N.dtype_id("fp32"), L.st()) != 0
    assert b"srcgan_s2d_shift" in lib.srcgan_last_error()
    assert lib.srcgan_prelu_forward(p, 32, p, None, None, 0, 0.5, p, 32, 1, 4, 4, 32, 1, 0, 4, 4, L.N.dtype_id("fp32"), L.st()) != 0
    assert b"srcgan_prelu_forward" in lib.srcgan_last_error() and b"beta" in lib.srcgan_last_error()
    assert lib.srcgan_prelu_backward(p, 32, p, 32, p, None, p, 32, None, 0, 1.0, 0, None, None, 1, 4, 4, 32, 1, 0, 4, 4, 7, p, L.st()) != 0
    assert b"srcgan_prelu_backward" in lib.srcgan_last_error()


def test_counts_past_2_31(L):
    """One channel of bf16 on a 46342^2 image: 2^31 + 4.7e5 work items per launch, where an index kept in 32 bits would wrap, on the
    kernels' element-wise path.  Gather and crop against torch views, PReLU against torch on the device."""
    n, s = 46342, 2
    assert n * n > 2 ** 31 and n % s == 0
    Hg = n // s
    did = L.N.dtype_id("bf16")
    x = torch.empty(1, n, n, 1, device="cuda", dtype=torch.bfloat16).uniform_(-1, 1)
    x.view(-1)[::3] = 0
    grid = torch.empty(1, Hg, Hg, s * s, device="cuda", dtype=torch.bfloat16)
    L.N.check(L.lib.srcgan_s2d_shift(x.data_ptr(), 1, grid.data_ptr(), s * s, 1, n, n, 1, s, 0, Hg, Hg, did, L.st()), "srcgan_s2d_shift")
    assert torch.equal(grid, x.view(Hg, s, Hg, s).permute(0, 2, 1, 3).reshape(1, Hg, Hg, s * s))
    back = torch.empty_like(x)
    L.N.check(L.lib.srcgan_d2s_shift(grid.data_ptr(), s * s, back.data_ptr(), 1, 1, n, n, 1, s, 0, Hg, Hg, 0, did, L.st()), "srcgan_d2s_shift")
    assert torch.equal(back, x)
    del back
    # PReLU through the crop: z = the grid, so PReLU(crop(grid)) = PReLU(x); the last rows are what a 32-bit index would get wrong
    slope = torch.tensor([-0.75], device="cuda")
    y = torch.empty_like(x)
    L.N.check(L.lib.srcgan_prelu_forward(grid.data_ptr(), s * s, slope.data_ptr(), None, None, 0, 1.0, y.data_ptr(), 1, 1, n, n, 1, s, 0, Hg, Hg, did, L.st()),
              "srcgan_prelu_forward")
    assert torch.equal(y, torch.where(x > 0, x, (x.float() * -0.75).to(torch.bfloat16)))
    dy, dz = y, torch.empty_like(grid)                 # any gradient will do: y itself
    scr = torch.empty(L.lib.srcgan_prelu_scratch_floats(1, Hg, Hg, 1, s), device="cuda")
    da = torch.zeros(1, device="cuda")
    L.N.check(L.lib.srcgan_prelu_backward(dy.data_ptr(), 1, grid.data_ptr(), s * s, slope.data_ptr(), None, dz.data_ptr(), s * s, None, 0, 1.0, 0, da.data_ptr(),
                                          None, 1, n, n, 1, s, 0, Hg, Hg, did, scr.data_ptr(), L.st()), "srcgan_prelu_backward")
    want_dz = torch.where(x > 0, dy, (dy.float() * -0.75).to(torch.bfloat16))
    assert torch.equal(dz, want_dz.view(Hg, s, Hg, s).permute(0, 2, 1, 3).reshape(1, Hg, Hg, s * s))
    del want_dz, dz
    exact, mag = 0.0, 0.0
    for rows in torch.arange(n, device="cuda").chunk(16):       # float64 in slices: dy * z over z <= 0
        t = torch.where(x[0, rows] > 0, 0.0, dy[0, rows].double() * x[0, rows].double())
        exact, mag = exact + float(t.sum()), mag + float(t.abs().sum())
    # K_RECORDED was measured on sums of a few thousand terms.  Here a term passes through up to `depth` float32 additions -- 8 in its
    # lane, 256 lanes folded, then the finishing kernel's lane (chunks / 64) and its 64 lane sums -- each within 2^-24 of a partial sum
    # that is at most sum |terms| (the terms have one sign); + 2 for the term's own product.  The worst case of that order, not a fit.
    nchunk = -(-(Hg * Hg * s * s) // R.PR_CHUNK)
    depth = R.PR_CHUNK // 256 + 256 + -(-nchunk // 64) + 64 + 2
    err = abs(float(da) - exact) / (2.0 ** -24 * mag)
    print(f"[bp] 46342^2 x 1 bf16: da error {err:.1f} in units of 2^-24 * sum |terms| (worst case of the order: {depth})")
    assert err <= depth
