"""Direct tests, through the C ABI, of csrc/reflect_pad.hip: srcgan_reflect_pad_nhwc, srcgan_reflect_pad_bwd_nhwc, srcgan_tanh_forward and
srcgan_tanh_backward in fp32, bf16 and fp16.

The pad is bit-equal to indexing with r() (resnetgen_ref.reflect_pad).  Its backward is bit-equal to float64 on integer operands
|v| <= 8 (ten terms stay below 256, exact in bf16), with accumulate 0 and 1; on random reals it is held to
    fp32:     |got - ref| <= 10 * 2^-24 * sum|terms|                     nine additions and the old value, each rounded once
    16 bits:  one rounding of the storage type of the float64 sum (u |ref|, u = 2^-8 / 2^-11; fp16: + half its smallest subnormal) plus that
tanh is held per element to float64 on z in [-12, 12] (0, denormals and saturation included):
    forward:  EPS = 4 x the larger of 2^-24 and numpy-float32 tanh's own largest error on the same inputs (16 bits: + one rounding)
    backward: EPS * |dy| -- absolute, because 1 - y^2 cancels near saturation; 16 bits: + one rounding.  With accumulate the bound is WIDER than
              that by 2^-24 |ref|: the f32 addition of the old value is one more rounding, of the sum, and does not scale with |dy|
The kernels take one thread per 16-byte piece and have no grid loop, so "a second trip" has no case; GRID_SHAPE spans several blocks
with a channel count whose pieces per pixel are no power of two.  One bf16 tensor past 2 GiB is checked band by band against flipped
slices.  The maxima are printed ("[rp] ..." lines, pytest -s); DESIGN 3.13 has the figures measured on an MI355X."""
import numpy as np
import pytest
import torch

import large_extent as LE
import resnetgen_ref as R

pytestmark = pytest.mark.gpu
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
U = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
FLOOR = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25}
SENT = 1000.0
GRID_SHAPE = ((2, 33, 31, 24), 2)
# ((B, H, W, C), p, channel stride or None = C, channel offset)
CASES = [((2, 4, 9, 8), 3, None, 0), ((1, 2, 2, 16), 1, None, 0), ((2, 5, 4, 64), 3, 72, 8), ((1, 7, 6, 256), 1, None, 0), (*GRID_SHAPE, None, 0),
         ((1, 3, 5, 3), 2, 8, 0),          # three image channels in an 8-channel record, element by element
         ((2, 5, 4, 64), 3, 72, 2)]        # C and the strides allow 16-byte pieces, the bases (8 bytes in fp32, 4 in 16 bits) do not: element by element
IDS = [f"{'x'.join(map(str, s))}p{p}" + (f"cs{cs}off{off}" if cs else "") for s, p, cs, off in CASES]


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
    """An NHWC tensor of C channels at channel ``off`` of records of ``cs`` channels; everything else holds a sentinel."""

    def __init__(self, a, dtype, cs, off, shape=None):
        shape = tuple(a.shape) if a is not None else shape
        self.C, self.cs, self.off = shape[-1], cs or shape[-1], off
        self.t = torch.full((*shape[:-1], self.cs), SENT, device="cuda", dtype=TDT[dtype])
        if a is not None:
            self.view().copy_(torch.from_numpy(np.ascontiguousarray(a)).to(TDT[dtype]))

    def view(self):
        return self.t[..., self.off:self.off + self.C]

    def ptr(self):
        return self.t.data_ptr() + self.off * self.t.element_size()

    def get(self):
        outside = torch.ones(self.cs, dtype=torch.bool, device="cuda")
        outside[self.off:self.off + self.C] = False
        assert bool((self.t[..., outside] == SENT).all()), "wrote outside the channel slice"
        return self.view().double().cpu().numpy()


def stored(a, dtype):
    """a float64 array rounded to the storage type, as float64"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(TDT[dtype]).double().numpy()


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape, p, cs, off", CASES, ids=IDS)
def test_forward_is_bit_equal_to_indexing(L, shape, p, cs, off, dtype):
    B, H, W, C = shape
    x = stored(np.random.default_rng(1).uniform(-4, 4, shape), dtype)
    xb, yb = Buf(x, dtype, cs, off), Buf(None, dtype, cs, off, (B, H + 2 * p, W + 2 * p, C))
    L.N.check(L.lib.srcgan_reflect_pad_nhwc(xb.ptr(), xb.cs, yb.ptr(), yb.cs, B, H, W, C, p, L.N.dtype_id(dtype), L.st()), "srcgan_reflect_pad_nhwc")
    assert np.array_equal(yb.get(), R.reflect_pad(x, p))
    assert np.array_equal(xb.get(), x)


def run_bwd(L, dy, old, shape, p, cs, off, acc, dtype):
    B, H, W, C = shape
    dyb, dxb = Buf(dy, dtype, cs, off), Buf(old, dtype, cs, off)
    L.N.check(L.lib.srcgan_reflect_pad_bwd_nhwc(dyb.ptr(), dyb.cs, dxb.ptr(), dxb.cs, B, H, W, C, p, acc, L.N.dtype_id(dtype), L.st()),
              "srcgan_reflect_pad_bwd_nhwc")
    assert np.array_equal(dyb.get(), dy)
    return dxb.get()


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape, p, cs, off", CASES, ids=IDS)
def test_backward_is_bit_equal_to_float64_on_small_integers(L, shape, p, cs, off, acc, dtype):
    B, H, W, C = shape
    g = np.random.default_rng(2)
    dy = g.integers(-8, 9, size=(B, H + 2 * p, W + 2 * p, C)).astype(np.float64)
    old = g.integers(-8, 9, size=shape).astype(np.float64)
    want, mag = R.reflect_pad_bwd(dy, H, W, p, old=old if acc else None)
    assert mag.max() <= 80
    assert np.array_equal(run_bwd(L, dy, old, shape, p, cs, off, acc, dtype), want)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape, p, cs, off", CASES, ids=IDS)
def test_backward_on_random_reals(L, shape, p, cs, off, acc, dtype):
    B, H, W, C = shape
    g = np.random.default_rng(3)
    dy, old = stored(g.uniform(-1, 1, (B, H + 2 * p, W + 2 * p, C)), dtype), stored(g.uniform(-1, 1, shape), dtype)
    want, mag = R.reflect_pad_bwd(dy, H, W, p, old=old if acc else None)
    got = run_bwd(L, dy, old, shape, p, cs, off, acc, dtype)
    b32 = 10 * 2.0 ** -24 * mag
    tol = b32 + U[dtype] * (np.abs(want) + b32) + FLOOR[dtype]
    excess = np.abs(got - want) / tol
    print(f"[rp] pad backward {shape} p {p} acc {acc} {dtype}: max |got - ref| / bound {excess.max():.3f}")
    assert excess.max() <= 1.0


def test_refusals_before_the_launch(L):
    t = torch.zeros(2, 4, 4, 8, device="cuda")
    y = torch.zeros(2, 12, 12, 8, device="cuda")
    for p, what in ((0, "at least 1"), (4, "smaller than H"), (-1, "at least 1")):
        assert L.lib.srcgan_reflect_pad_nhwc(t.data_ptr(), 8, y.data_ptr(), 8, 2, 4, 4, 8, p, 0, L.st()) != 0
        assert what in L.lib.srcgan_last_error().decode()
        assert L.lib.srcgan_reflect_pad_bwd_nhwc(y.data_ptr(), 8, t.data_ptr(), 8, 2, 4, 4, 8, p, 0, 0, L.st()) != 0
    assert L.lib.srcgan_reflect_pad_nhwc(t.data_ptr(), 8, y.data_ptr(), 8, 2, 4, 3, 8, 3, 0, L.st()) != 0          # p >= W
    assert L.lib.srcgan_reflect_pad_nhwc(t.data_ptr(), 4, y.data_ptr(), 8, 2, 4, 4, 8, 1, 0, L.st()) != 0          # stride below the channels
    assert L.lib.srcgan_reflect_pad_nhwc(None, 8, y.data_ptr(), 8, 2, 4, 4, 8, 1, 0, L.st()) != 0
    assert L.lib.srcgan_tanh_forward(t.data_ptr(), 8, None, 8, 32, 8, 0, L.st()) != 0
    assert L.lib.srcgan_tanh_backward(t.data_ptr(), 8, t.data_ptr(), 8, y.data_ptr(), 4, 32, 8, 0, 0, L.st()) != 0
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- tanh
def tanh_inputs():
    z = np.concatenate([np.linspace(-12, 12, 4001), [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-38, -1e-38, 9.01, -9.01, 9.5, -9.5, 12.0, -12.0, 1e-4, -1e-4, 0.5493061443]])
    z = np.concatenate([z, np.zeros(-len(z) % 24)])
    return z


def eps_tanh(z):
    """4 x the larger of 2^-24 and numpy-float32 tanh's own largest error on the inputs"""
    own = np.abs(np.tanh(z.astype(np.float32)).astype(np.float64) - np.tanh(z.astype(np.float32).astype(np.float64))).max()
    return 4 * max(2.0 ** -24, float(own))


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C, cs, off", [(8, None, 0), (24, 40, 8), (3, 8, 0), (8, 16, 2)])      # the last: a base that is not 16-byte aligned
def test_tanh_forward_and_backward_per_element(L, C, cs, off, dtype):
    z = stored(tanh_inputs(), dtype).reshape(-1, C)
    npix, did = z.shape[0], L.N.dtype_id(dtype)
    eps = eps_tanh(z)
    ref = np.tanh(z)
    zb, yb = Buf(z, dtype, cs, off), Buf(None, dtype, cs, off, z.shape)
    L.N.check(L.lib.srcgan_tanh_forward(zb.ptr(), zb.cs, yb.ptr(), yb.cs, npix, C, did, L.st()), "srcgan_tanh_forward")
    y = yb.get()
    tol = eps + U[dtype] * (np.abs(ref) + eps) + FLOOR[dtype]
    fe = np.abs(y - ref)
    assert (fe <= tol).all() and np.abs(y).max() <= 1.0
    assert np.array_equal(y[z == 0], z[z == 0])
    g = np.random.default_rng(4)
    dy, old = stored(g.uniform(-2, 2, z.shape), dtype), stored(g.uniform(-1, 1, z.shape), dtype)
    worst = []
    for acc in (0, 1):
        dyb, ysb, dzb = Buf(dy, dtype, cs, off), Buf(y, dtype, cs, off), Buf(old, dtype, cs, off)
        L.N.check(L.lib.srcgan_tanh_backward(dyb.ptr(), dyb.cs, ysb.ptr(), ysb.cs, dzb.ptr(), dzb.cs, npix, C, acc, did, L.st()), "srcgan_tanh_backward")
        want = R.tanh_bwd(dy, y, old=old if acc else None)          # from the SAVED output, as stored
        b32 = eps * np.abs(dy) + (2.0 ** -24 * np.abs(want) if acc else 0.0)
        tolb = b32 + U[dtype] * (np.abs(want) + b32) + FLOOR[dtype]
        be = np.abs(dzb.get() - want)
        worst.append(float((be / np.maximum(tolb, 1e-300)).max()))
        assert (be <= tolb).all()
    print(f"[rp] tanh C {C} {dtype}: EPS {eps:.3e}; forward max |err| {fe.max():.3e} ({(fe / tol).max():.3f} of the bound); "
          f"backward max |err| / bound {worst[0]:.3f}, accumulate {worst[1]:.3f}")


# ---------------------------------------------------------------------------------------------------------------- past 2 GiB
def test_pad_and_its_backward_past_2_gib(L):
    """bf16 (1, 4100, 4100, 64), p 3: x is 2,151,680,000 B and the padded tensor 2,157,982,208 B -- both cross 2^31 (at 16 x 3 x 1024^2 the
    padded 64-channel tensor of the network is 2.17 GB).  Forward: the centre equals x, every border row and column equals the row /
    column it mirrors.  Backward on hashed integers in [-4, 4] (at most four terms: exact): band by band against slices and flipped
    slices of dy (resnetgen_ref.reflect_pad_bwd_rows, held to the scatter on the CPU by tests/test_resnetgen_teeth.py)."""
    B, H, W, C, p = 1, 4100, 4100, 64, 3
    PH, PW = H + 2 * p, W + 2 * p
    xb, yb = LE.Buf("rp/x", LE.INT4, B, H, W, C, torch.bfloat16), LE.Buf("rp/dy", LE.INT4, B, PH, PW, C, torch.bfloat16)
    assert len(xb.boundaries()) == 1 and len(yb.boundaries()) == 1
    free = torch.cuda.mem_get_info()[0]
    if free < 3 * yb.nbytes:
        pytest.fail(f"needs {3 * yb.nbytes >> 20} MiB of device memory, {free >> 20} MiB are free")
    x = LE.fill(torch.empty(xb.shape, device="cuda", dtype=torch.bfloat16), xb)
    y = torch.full(yb.shape, SENT, device="cuda", dtype=torch.bfloat16)
    did = L.N.dtype_id("bf16")
    L.N.check(L.lib.srcgan_reflect_pad_nhwc(x.data_ptr(), C, y.data_ptr(), C, B, H, W, C, p, did, L.st()), "srcgan_reflect_pad_nhwc")
    BAND = 256
    for r0 in range(0, H, BAND):
        r1 = min(H, r0 + BAND)
        assert torch.equal(y[:, p + r0:p + r1, p:p + W], x[:, r0:r1]), f"centre rows {r0}..{r1}"
    for k in range(1, p + 1):               # padded row p - k mirrors padded row p + k; row PH - 1 - p + k mirrors PH - 1 - p - k; columns alike
        assert torch.equal(y[:, p - k], y[:, p + k]) and torch.equal(y[:, PH - 1 - p + k], y[:, PH - 1 - p - k])
        assert torch.equal(y[:, :, p - k], y[:, :, p + k]) and torch.equal(y[:, :, PW - 1 - p + k], y[:, :, PW - 1 - p - k])
    # the last pixel of the last row sits past 2^31 bytes and came from x's last-but-p pixel, past 2^31 too
    assert (PH * PW - 1) * C * 2 > LE.G31 and ((H - 1 - p) * W + W - 1 - p) * C * 2 > LE.G31
    assert torch.equal(y[0, PH - 1, PW - 1], x[0, H - 1 - p, W - 1 - p])
    # backward: y becomes dy, x receives dx
    LE.fill(y, yb)
    x.fill_(SENT)
    L.N.check(L.lib.srcgan_reflect_pad_bwd_nhwc(y.data_ptr(), C, x.data_ptr(), C, B, H, W, C, p, 0, did, L.st()), "srcgan_reflect_pad_bwd_nhwc")
    for r0 in range(0, H, BAND):
        r1 = min(H, r0 + BAND)
        want = R.reflect_pad_bwd_rows(y, H, W, p, r0, r1)
        assert float(want.abs().max()) <= 16
        assert torch.equal(x[:, r0:r1].float(), want), f"dx rows {r0}..{r1}"
    # accumulate adds dx once more: twice the gradient (exact)
    L.N.check(L.lib.srcgan_reflect_pad_bwd_nhwc(y.data_ptr(), C, x.data_ptr(), C, B, H, W, C, p, 1, did, L.st()), "srcgan_reflect_pad_bwd_nhwc")
    for r0 in (0, H // 2 // BAND * BAND, (H - 1) // BAND * BAND):
        r1 = min(H, r0 + BAND)
        assert torch.equal(x[:, r0:r1].float(), 2 * R.reflect_pad_bwd_rows(y, H, W, p, r0, r1))
