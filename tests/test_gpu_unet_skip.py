"""GPU, through the C ABI: the two kernels of csrc/unet_skip.hip.

srcgan_in_skip_forward must have the BITS of two srcgan_gn_forward calls with G == C and no affine part -- (relu = 1, slope 0.2) for its dense
output ``a``, (relu = 1, slope 0) for the half ``r`` of the skip buffer -- and their statistics: the executor's backward hands the saved
statistics to srcgan_gn_backward, and the fused op replaces exactly those two calls.  srcgan_relu_nhwc must equal torch.relu.  Every case runs
with an input whose channel stride exceeds C, writes ``r`` into channels [0, C) of a 2 C-wide buffer whose other half holds a sentinel, and
has guard elements around every output; inputs are compared with their copies afterwards."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENT, GUARD, EPS, SLOPE = 1000.0, 64, 1e-5, 0.2
# (C, H, W): both tiny planes at every width (2 x 2 is the smallest plane the network normalises; 2 x 3: an odd pixel count);
# 48 x 48 at C = 16: 4 (f32) / 2 (16-bit) partial blocks per image in the statistics pass
SHAPES = [(C, h, w) for C in (16, 128, 512) for (h, w) in ((2, 2), (2, 3))] + [(16, 48, 48)]


class Lib:
    def __init__(self):
        from srcgan_amd import _native as N
        self.N, self.lib = N, N.lib()
        self.st = N.stream_ptr(torch.device("cuda"))

    def scratch(self, B, C):
        return torch.full((self.lib.srcgan_gn_scratch_floats(B, C) + 8,), float("nan"), device="cuda")


@pytest.fixture(scope="module")
def L():
    return Lib()


def guarded(npix, cs, dtype, fill=SENT):
    """-> (whole buffer, view [npix, cs] in its middle): GUARD elements of the fill on either side"""
    buf = torch.full((npix * cs + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + npix * cs].view(npix, cs)


def guards_intact(buf, fill=SENT):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


@pytest.mark.parametrize("C, H, W", SHAPES)
@pytest.mark.parametrize("dt", list(DT))
def test_in_skip_forward_has_the_bits_of_two_norm_calls(L, dt, C, H, W):
    B, hw, tdt, did = 2, H * W, DT[dt], L.N.dtype_id(dt)
    npix, x_cs = B * hw, C + 16
    g = torch.Generator().manual_seed(C + 7 * H + W)
    _, x = guarded(npix, x_cs, tdt)
    x[:, :C] = (torch.randn(npix, C, generator=g) * 1.5 + torch.randn(1, C, generator=g)).to(tdt).cuda()
    x0 = x.clone()
    # the reference: two srcgan_gn_forward calls
    ya, yr = torch.full((npix, C), SENT, dtype=tdt, device="cuda"), torch.full((npix, C), SENT, dtype=tdt, device="cuda")
    sa, sr = torch.full((B * C * 2,), SENT, device="cuda"), torch.full((B * C * 2,), SENT, device="cuda")
    for y, s, slope in ((ya, sa, SLOPE), (yr, sr, 0.0)):
        L.N.check(L.lib.srcgan_gn_forward(x.data_ptr(), x_cs, None, 0, y.data_ptr(), C, None, None, s.data_ptr(), B, hw, C, C, EPS, 1, slope, did,
                                          L.scratch(B, C).data_ptr(), L.st), "srcgan_gn_forward")
    assert torch.equal(sa, sr) and bool((ya >= 0).any()) and bool((ya < 0).any()) and bool((yr == 0).any())
    # the fused call
    abuf, a = guarded(npix, C, tdt)
    rbuf, r = guarded(npix, 2 * C, tdt)
    sbuf = torch.full((B * C * 2 + 2 * GUARD,), SENT, device="cuda")
    stats = sbuf[GUARD:GUARD + B * C * 2]
    L.N.check(L.lib.srcgan_in_skip_forward(x.data_ptr(), x_cs, a.data_ptr(), C, r.data_ptr(), 2 * C, 0, stats.data_ptr(), B, hw, C, EPS, SLOPE, did,
                                           L.scratch(B, C).data_ptr(), L.st), "srcgan_in_skip_forward")
    torch.cuda.synchronize()
    assert torch.equal(stats, sa)
    assert torch.equal(a, ya)
    assert torch.equal(r[:, :C], yr)
    assert bool((r[:, C:] == SENT).all()), "the other half of the skip buffer was touched"
    assert guards_intact(abuf) and guards_intact(rbuf) and guards_intact(sbuf)
    assert torch.equal(x, x0)
    # the second half of the buffer, through the offset: the same values, the first half untouched
    rbuf2, r2 = guarded(npix, 2 * C, tdt)
    L.N.check(L.lib.srcgan_in_skip_forward(x.data_ptr(), x_cs, a.data_ptr(), C, r2.data_ptr(), 2 * C, C, stats.data_ptr(), B, hw, C, EPS, SLOPE, did,
                                           L.scratch(B, C).data_ptr(), L.st), "srcgan_in_skip_forward")
    assert torch.equal(r2[:, C:], yr) and bool((r2[:, :C] == SENT).all()) and guards_intact(rbuf2)


def test_in_skip_forward_refuses_what_it_cannot_address(L):
    x = torch.zeros(8, 16, device="cuda")
    a, r, s = torch.zeros(8, 16, device="cuda"), torch.zeros(8, 32, device="cuda"), torch.zeros(64, device="cuda")
    scr = L.scratch(2, 16)
    call = lambda x_cs, a_cs, r_cs, r_coff, C: L.lib.srcgan_in_skip_forward(x.data_ptr(), x_cs, a.data_ptr(), a_cs, r.data_ptr(), r_cs, r_coff, s.data_ptr(),
                                                                            2, 4, C, EPS, SLOPE, 0, scr.data_ptr(), L.st)
    assert call(16, 16, 32, 0, 16) == 0
    for args, what in (((16, 16, 32, 20, 16), "smaller than the channels"), ((16, 16, 32, 2, 16), "multiples of 4"), ((16, 12, 32, 0, 16), "smaller than the channels"),
                       ((16, 16, 32, 0, 6), "multiple of 4")):
        assert call(*args) != 0 and what in L.lib.srcgan_last_error().decode(), args


@pytest.mark.parametrize("C, x_cs, y_cs, y_coff", [(16, 32, 32, 0), (16, 16, 32, 16), (128, 144, 256, 0), (512, 528, 1024, 0), (3, 8, 8, 0), (5, 8, 16, 8), (6, 7, 13, 3)])
@pytest.mark.parametrize("dt", list(DT))
def test_relu_nhwc_equals_torch_relu(L, dt, C, x_cs, y_cs, y_coff):
    """strided input, output into a channel range of a wider buffer whose other channels keep the sentinel; (3, 8, 8), (5, 8, 16) and
    (6, 7, 13) take the element-wise path; a negative-only input gives all zeros"""
    tdt, did, npix = DT[dt], L.N.dtype_id(dt), 2 * 5 * 7
    g = torch.Generator().manual_seed(C + y_coff)
    for negative in (False, True):
        _, x = guarded(npix, x_cs, tdt)
        v = torch.randn(npix, C, generator=g)
        x[:, :C] = (-v.abs() - 0.5 if negative else v).to(tdt).cuda()
        x0 = x.clone()
        ybuf, y = guarded(npix, y_cs, tdt)
        L.N.check(L.lib.srcgan_relu_nhwc(x.data_ptr(), x_cs, y.data_ptr(), y_cs, y_coff, npix, C, did, L.st), "srcgan_relu_nhwc")
        torch.cuda.synchronize()
        assert torch.equal(y[:, y_coff:y_coff + C], torch.relu(x[:, :C]))
        assert not negative or bool((y[:, y_coff:y_coff + C] == 0).all())
        keep = torch.ones(y_cs, dtype=torch.bool, device="cuda")
        keep[y_coff:y_coff + C] = False
        assert bool((y[:, keep] == SENT).all()) and guards_intact(ybuf) and torch.equal(x, x0)


def test_relu_nhwc_refuses_a_range_outside_the_stride(L):
    x, y = torch.zeros(4, 16, device="cuda"), torch.zeros(4, 32, device="cuda")
    assert L.lib.srcgan_relu_nhwc(x.data_ptr(), 16, y.data_ptr(), 32, 24, 4, 16, 0, L.st) != 0
    assert "channel stride / offset" in L.lib.srcgan_last_error().decode()
    assert L.lib.srcgan_relu_nhwc(x.data_ptr(), 8, y.data_ptr(), 32, 0, 4, 16, 0, L.st) != 0
