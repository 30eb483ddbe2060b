"""Direct tests of the four layout kernels of csrc/elementwise.hip -- nchw_to_nhwc_k, nhwc_to_nchw_k and the 16-bit
image-channel fast paths nchw_to_nhwc8_k, nhwc8_to_nchw_k -- in bits against permute + one cast (tests/param_kernels_ref.py), in
one direction at a time: a round trip cannot see a consistent permutation.  Every shape runs through ops.to_nhwc / ops.to_nchw
and, through the ABI, into a destination pre-filled with a sentinel with a guard behind it.  The fast paths are taken for a
16-bit type, 8-channel records, channel offset 0, H W a multiple of 4 and 16-byte aligned pointers; each such shape runs again
with the source one element into a larger buffer, which sends it down the general kernel, and both results must have the same
bits.  tests/test_param_kernels_teeth.py shows on the CPU that the comparison tells H and W exchanged, channels rotated by one,
a pixel left out and a non-zero pad channel from the right answer."""
import pytest
import torch

import param_kernels_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import _native as N, ops

    class Lib:
        pass
    o = Lib()
    o.N, o.ops, o.lib = N, ops, N.lib()
    return o


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _to_nhwc_abi(L, xd, cs, dt, src_shift=0):
    """srcgan_nchw_f32_to_nhwc into a sentinel-filled destination with a guard -> (result [B,H,W,cs], guard) on the CPU;
    src_shift: the source starts that many elements into a larger buffer"""
    B, C, H, W = xd.shape
    if src_shift:
        big = torch.full((xd.numel() + 8,), R.SENT, device="cuda")
        big[src_shift:src_shift + xd.numel()] = xd.reshape(-1)
        xd = big[src_shift:src_shift + xd.numel()]
    n = B * H * W * cs
    dst = torch.full((n + GUARD,), R.SENT, dtype=R.TDT[dt], device="cuda")
    L.N.check(L.lib.srcgan_nchw_f32_to_nhwc(xd.data_ptr(), dst.data_ptr(), B, C, H, W, cs, L.N.dtype_id(dt), _stream()), "to_nhwc")
    out = dst.cpu()
    return out[:n].view(B, H, W, cs), out[n:]


def _to_nchw_abi(L, bd, C, coff, src_shift=0):
    B, H, W, cs = bd.shape
    if src_shift:
        big = torch.full((bd.numel() + 16,), float("nan"), dtype=bd.dtype, device="cuda")
        big[src_shift:src_shift + bd.numel()] = bd.reshape(-1)
        bd = big[src_shift:src_shift + bd.numel()]
    n = B * C * H * W
    dst = torch.full((n + GUARD,), R.SENT, device="cuda")
    L.N.check(L.lib.srcgan_nhwc_to_nchw_f32(bd.data_ptr(), dst.data_ptr(), B, C, H, W, cs, coff, L.N.dtype_id(bd.dtype), _stream()), "to_nchw")
    out = dst.cpu()
    return out[:n].view(B, C, H, W), out[n:]


def _guard_ok(g, dt):
    return R.same_bits(g, torch.full((GUARD,), R.SENT, dtype=R.TDT[dt]))


def _fast(dt, cs, coff, H, W):
    return dt != "fp32" and cs == 8 and coff == 0 and (H * W) % 4 == 0


@pytest.mark.parametrize("dt", R.DTS)
def test_to_nhwc_bits(L, dt):
    """NCHW f32 -> NHWC of the type, channels [C, cs) exactly +0, over C x cs x H W x B of the sweep"""
    nfast = 0
    for n, (B, C, H, W, cs) in enumerate(R.layout_cases()):
        x = R.layout_values((B, C, H, W), 11 * n + 3)
        want = R.nhwc_ref(x, cs, dt)
        xd = x.cuda()
        what = f"{dt} B {B} C {C} H {H} W {W} cs {cs}"
        assert R.same_bits(L.ops.to_nhwc(xd, cs, dt).cpu(), want), what
        got, guard = _to_nhwc_abi(L, xd, cs, dt)
        assert R.same_bits(got, want) and _guard_ok(guard, dt), what
        if _fast(dt, cs, 0, H, W):
            nfast += 1
            assert xd.data_ptr() % 16 == 0
            slow, guard = _to_nhwc_abi(L, xd, cs, dt, src_shift=1)          # misaligned source: the general kernel
            assert R.same_bits(slow, got) and _guard_ok(guard, dt), what + " (general kernel on the fast path's shape)"
    assert nfast == (0 if dt == "fp32" else 2 * 2 * 3)                       # C 1, 3, 8 with cs 8; H W 64, 512; B 1, 3


@pytest.mark.parametrize("dt", R.DTS)
def test_to_nchw_bits(L, dt):
    """NHWC of the type -> NCHW f32 of channels [coff, coff + C); the record's other channels hold NaN and none may come out"""
    nfast = 0
    for n, (B, C, H, W, cs) in enumerate(R.layout_cases()):
        coff = R.layout_coff(C, cs)
        buf = torch.full((B, H, W, cs), float("nan"), dtype=R.TDT[dt])
        buf[..., coff:coff + C] = R.layout_values((B, H, W, C), 13 * n + 5).to(R.TDT[dt])
        want = R.nchw_ref(buf, C, coff)
        assert not bool(torch.isnan(want).any())
        bd = buf.cuda()
        what = f"{dt} B {B} C {C} H {H} W {W} cs {cs} coff {coff}"
        assert R.same_bits(L.ops.to_nchw(bd, C, coff).cpu(), want), what
        got, guard = _to_nchw_abi(L, bd, C, coff)
        assert R.same_bits(got, want) and _guard_ok(guard, "fp32"), what
        if _fast(dt, cs, coff, H, W):
            nfast += 1
            slow, guard = _to_nchw_abi(L, bd, C, coff, src_shift=1)
            assert R.same_bits(slow, got) and _guard_ok(guard, "fp32"), what + " (general kernel on the fast path's shape)"
    assert nfast == (0 if dt == "fp32" else 2 * 2 * 3)
    assert any(R.layout_coff(C, cs) > 0 and cs > C + R.layout_coff(C, cs) for (_, C, _, _, cs) in R.layout_cases())


def test_general_kernels_past_the_grid_cap(L):
    """4097 panels of 64 pixels (C = 1, 4097 x 64): a block of the 4096-block grid takes a second panel, both directions"""
    x = R.layout_values((1, 1, 4097, 64), 91)
    for dt in ("fp32", "bf16"):
        want = R.nhwc_ref(x, 1, dt)
        got, guard = _to_nhwc_abi(L, x.cuda(), 1, dt)
        assert R.same_bits(got, want) and _guard_ok(guard, dt)
        back, guard = _to_nchw_abi(L, want.cuda(), 1, 0)
        assert R.same_bits(back, R.nchw_ref(want, 1, 0)) and _guard_ok(guard, "fp32")


def test_fast_kernels_past_the_grid_cap(L):
    """2052 x 2048 pixels of 3 channels in bf16: 1 050 624 quads, above the 4096 x 256 threads of a grid, both directions"""
    B, C, H, W = 1, 3, 2052, 2048
    assert B * H * W // 4 > 4096 * 256
    x = R.layout_values((B, C, H, W), 92)
    want = R.nhwc_ref(x, 8, "bf16")
    got = L.ops.to_nhwc(x.cuda(), 8, "bf16")
    assert got.data_ptr() % 16 == 0 and R.same_bits(got.cpu(), want)
    del got
    src = want.clone()
    src[..., 3:] = float("nan")
    back = L.ops.to_nchw(src.cuda(), 3)
    assert R.same_bits(back.cpu(), R.nchw_ref(src, 3, 0))
