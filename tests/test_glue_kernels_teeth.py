"""The exact comparisons of tests/test_gpu_glue_kernels.py have teeth: on the CPU, each family's own reference is compared, by
the same bit comparison, with a copy of itself that makes one of the mistakes the GPU tests are there to catch -- one pixel
dropped, a channel offset shifted by 4, a plane index off by one.  Every such comparison must fail.  No kernel runs here."""
import pytest
import torch

import test_gpu_glue_kernels as G

DTS = G.DTS


def _differs(a, b):
    return not G.same_bits(a, b)


def _without_last_pixel(want, initial, npix, cs, coff, C, plane=0):
    """`want` as a kernel that skipped the last pixel would have left it"""
    idx = G.chan_index(npix, cs, coff, C, plane, want.element_size(), want.device)[-1]
    out = want.clone()
    out.reshape(-1)[idx] = initial.reshape(-1)[idx]
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_reduction_reference_notices(dt, mode):
    torch.manual_seed(1)
    k = G.reduce_case("int", 1023, 64, G.TDT[dt], "cpu", 128, 32, 160, 64)
    ref = [r.float() for r in G.ref_col_reduce(mode, k, 0.125)[0]]
    same = lambda other: all(G.same_bits(a, b.float()) for a, b in zip(ref, other))
    assert same(G.ref_col_reduce(mode, k, 0.125)[0])
    assert not same(G.ref_col_reduce(mode, k, 0.125, npix=1022)[0])              # one pixel dropped
    assert not same(G.ref_col_reduce(mode, k, 0.125, a_coff=36)[0])              # channel offset + 4
    if mode == 2:
        assert not same(G.ref_col_reduce(mode, k, 0.125, z_coff=68)[0])


@pytest.mark.parametrize("dt", DTS)
def test_residual_join_reference_notices(dt):
    torch.manual_seed(2)
    B, H, W, C = 2, 5, 7, 48
    npix, kce = B * H * W, 64 // (4 if dt == "fp32" else 2)
    yv, xv, mv = G._join_values(B, H, W, C, G.TDT[dt], "cpu")
    (y, ys), (x, xs), (mz, ms) = G.operand(yv, 96, 12, True), G.operand(xv, 96, 4, True), G.operand(mv, 96, 8, True)
    want = G.ref_add_inplace(y, ys, x, xs, mz, ms, G.SLOPE, npix, C)
    assert G.same_bits(want, G.ref_add_inplace(y, ys, x, xs, mz, ms, G.SLOPE, npix, C))
    assert _differs(want, G.ref_add_inplace(y, ys, x, xs, mz, ms, G.SLOPE, npix - 1, C))                  # one pixel dropped
    for d in (4, kce):                                                                                        # channel offset + 4; plane index + 1
        sh = lambda s: (s[0], s[1] + d, s[2])
        assert _differs(want, G.ref_add_inplace(y, sh(ys), x, xs, mz, ms, G.SLOPE, npix, C))
        assert _differs(want, G.ref_add_inplace(y, ys, x, sh(xs), mz, ms, G.SLOPE, npix, C))
        assert _differs(want, G.ref_add_inplace(y, ys, x, xs, mz, sh(ms), G.SLOPE, npix, C))
    # the interleaved form and the factor at +-0.0: 1 only where mz > 0
    (y, ys), (x, xs), (mz, ms) = G.operand(yv, 96, 32, False), G.operand(xv, 64, 0, False), G.operand(mv, 128, 64, False)
    want = G.ref_add_inplace(y, ys, x, xs, mz, ms, G.SLOPE, npix, C)
    assert _differs(want, G.ref_add_inplace(y, ys, x, (xs[0], 4, 0), mz, ms, G.SLOPE, npix, C))
    ge = G.put(y, (G.take(y, npix, *ys[:2], C).float() + G.take(x, npix, *xs[:2], C).float())
               * torch.where(G.take(mz, npix, *ms[:2], C).float() >= 0, 1.0, G.SLOPE), npix, *ys[:2], C)
    assert _differs(want, ge)                                                                                 # '>=' instead of '>'


@pytest.mark.parametrize("dt", DTS)
def test_data_movement_references_notice(dt):
    torch.manual_seed(3)
    tdt = G.TDT[dt]
    kce = 64 // (4 if dt == "fp32" else 2)
    B, H, W, C = 2, 5, 9, 64
    # upsample2 from a blocked source
    v = G.plant_zeros(torch.randn(B, H, W, C)).to(tdt)
    src, (s_cs, s_coff, s_plane) = G.operand(v, 128, 16, True)
    dst = torch.full((B, 2 * H, 2 * W, 96), G.SENT, dtype=tdt)
    want = G.ref_upsample2(src, s_cs, s_coff, s_plane, dst, 96, B, H, W, C)
    assert _differs(want, _without_last_pixel(want, dst, B * 4 * H * W, 96, 0, C))
    assert _differs(want, G.ref_upsample2(src, s_cs, s_coff + 4, s_plane, dst, 96, B, H, W, C))
    assert _differs(want, G.ref_upsample2(src, s_cs, s_coff - kce // 2, s_plane, dst, 96, B, H, W, C))
    assert _differs(want, G.ref_upsample2(src, s_cs, s_coff + kce, s_plane, dst, 96, B, H, W, C))             # plane index + 1
    # sum2x2 on integer data: one of the four pixels of a block dropped, the channel offset shifted
    srcv, mz = G._sum2x2_operands("int", B, H, W, C, tdt, "cpu")
    bits = lambda s: (s[0]).to(tdt)
    want = bits(G.ref_sum2x2(srcv, 96, mz, 72, G.SLOPE, B, H, W, C))
    one_out = srcv.clone()
    one_out[:C] = 0
    assert srcv[:C].abs().sum() > 0
    assert _differs(want, bits(G.ref_sum2x2(one_out, 96, mz, 72, G.SLOPE, B, H, W, C)))
    shifted = torch.cat([srcv[4:], srcv[:4]])
    assert _differs(want, bits(G.ref_sum2x2(shifted, 96, mz, 72, G.SLOPE, B, H, W, C)))
    assert _differs(want, bits(G.ref_sum2x2(srcv, 96, torch.cat([mz[4:], mz[:4]]), 72, G.SLOPE, B, H, W, C)))
    # pixel shuffle, both directions
    r, Cs, cs_lo, cs_hi = 3, 3, 3 * 9 + 8, 3 + 6
    lo = G.slice_buffer(torch.randn(B * H * W, Cs * r * r).to(tdt), cs_lo, 0)
    hi0 = torch.full((B * H * r * W * r * cs_hi,), G.SENT, dtype=tdt)
    want = G.ref_pixel_shuffle(lo, cs_lo, hi0, cs_hi, B, H, W, Cs, r, 0)
    assert _differs(want, _without_last_pixel(want, hi0, B * H * r * W * r, cs_hi, 0, Cs))
    assert _differs(want, G.ref_pixel_shuffle(lo[4:], cs_lo, hi0, cs_hi, B, H, W, Cs, r, 0))
    lo0 = torch.full_like(lo, G.SENT)
    back = G.ref_pixel_shuffle(want, cs_hi, lo0, cs_lo, B, H, W, Cs, r, 1)
    assert G.same_bits(back, lo)
    assert _differs(back, _without_last_pixel(back, lo0, B * H * W, cs_lo, 0, Cs * r * r))
    assert _differs(back, G.ref_pixel_shuffle(want[4:], cs_hi, lo0, cs_lo, B, H, W, Cs, r, 1))
    # activation mask
    n = 257
    g, act = torch.randn(n + 5).to(tdt), G.plant_zeros(torch.randn(n + 5)).to(tdt)
    g[n - 1], act[n - 1] = 1.5, -1.0
    want = G.ref_mask(g, act, G.SLOPE, n)
    assert _differs(want, G.ref_mask(g, act, G.SLOPE, n - 1))
    assert _differs(want, G.ref_mask(g, torch.cat([act[4:], act[:4]]), G.SLOPE, n))
    assert _differs(want[:n], torch.where(act.float() >= 0, g.float(), g.float() * G.SLOPE).to(tdt)[:n])              # '>=' instead of '>'
