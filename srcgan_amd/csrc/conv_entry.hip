// srcgan_conv_igemm: the front door of every forward and input-gradient convolution.  Host code only -- it checks the descriptor,
// turns it into the kernels' parameter block (ConvP) and hands that to one kernel family:
//   sg_deconv_k3s2 (deconv_k3s2.hip)   npar == 4, 3x3: ConvTranspose2d(k3, s2, p1, output_padding 1), four parities in one launch
//   sg_dgrad_s2k4  (conv_par4.hip)     npar == 4, 2x2: input gradient of a 4x4 stride-2 convolution, four parities in one launch
//   sg_conv3x3_dma (conv3x3_dma.hip)   3x3 stride 1
//   sg_conv_generic (conv_igemm.hip)   everything else, the 1x1 four-parity form of ConvTranspose2d(k2, s2) included
// Every refusal happens before the first HIP call.
#include "conv_params.h"

static const bool g_force_generic = sg_env("SRCGAN_GENERIC_3X3") != nullptr;   // A/B switch for benchmarking

// ---- step 1: what any kernel family needs to hold of a descriptor
static int check_desc(const srcgan_conv_desc* d) {
    SG_REQUIRE(d && d->x && d->wp && d->y, "srcgan_conv_igemm: null pointer");
    SG_REQUIRE(sg_dtype_ok(d->dtype), "srcgan_conv_igemm: bad dtype %d", d->dtype);
    const int epp = d->dtype == SRCGAN_F32 ? 4 : 8;
    SG_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->OH > 0 && d->OW > 0 && d->Cin > 0 && d->Cout > 0,
               "srcgan_conv_igemm: non-positive dimension");
    SG_REQUIRE(d->Cin % epp == 0 && d->x_cs % epp == 0 && d->x_coff % epp == 0,
               "srcgan_conv_igemm: input channels/stride/offset (%d,%d,%d) must be multiples of %d", d->Cin, d->x_cs, d->x_coff, epp);
    SG_REQUIRE((d->x_plane || d->x_coff + d->Cin <= d->x_cs) && (d->y_plane || d->y_coff + d->Cout <= d->y_cs),
               "srcgan_conv_igemm: channel slice exceeds stride");
    SG_REQUIRE(!d->x_plane || (d->kh == 3 && d->kw == 3 && d->stride == 1), "srcgan_conv_igemm: a blocked-layout input is supported by the 3x3 stride-1 kernel only");
    SG_REQUIRE(((uintptr_t)d->x % 16) == 0 && ((uintptr_t)d->wp % 16) == 0, "srcgan_conv_igemm: x/wp must be 16-byte aligned");
    SG_REQUIRE(d->os >= 1 && d->oa >= 0 && d->ob >= 0 && d->oa < d->os && d->ob < d->os, "srcgan_conv_igemm: bad output scale/offset");
    SG_REQUIRE((d->OH - 1) * d->os + d->oa < d->YH && (d->OW - 1) * d->os + d->ob < d->YW, "srcgan_conv_igemm: output extent exceeds tensor");
    if (d->sign_out || d->sign_in) {
        const bool dense32 = d->kh == 3 && d->kw == 3 && d->stride == 1 && sg_is16(d->dtype) && d->Cout == 32 && d->os == 1 && d->oa == 0 && d->ob == 0 &&
                             d->YH == d->OH && d->YW == d->OW && d->x_plane && !(d->sign_in && d->mz) && (!d->sign_out || d->act);
        // 64 channels (8 mask bytes per pixel): written by the up-sampler's 1x1 parity form, read by a 3x3 s1 convolution without other operands
        const bool up_out = d->sign_out && !d->sign_in && d->kh == 1 && d->kw == 1 && d->npar == 4 && sg_is16(d->dtype) && d->Cout == 64 && d->act;
        const bool in64 = d->sign_in && !d->sign_out && d->kh == 3 && d->kw == 3 && d->stride == 1 && sg_is16(d->dtype) && d->Cout == 64 && d->os == 1 &&
                          d->YH == d->OH && d->YW == d->OW && !d->mz && !d->r1 && !d->r2;
        SG_REQUIRE(dense32 || up_out || in64,
                   "srcgan_conv_igemm: sign masks need a 3x3 s1 16-bit conv with Cout == 32 on a blocked input, unscaled output (act for sign_out, no mz beside sign_in); "
                   "or Cout == 64: sign_out of the 1x1 four-parity form with act, sign_in of a 3x3 s1 conv without other operands");
    }
    return 0;
}

// ---- step 2: descriptor -> ConvP.  Channel strides become bytes, a plane stride of 0 (interleaved NHWC) becomes the 64-byte chunk;
// vec / vec16 / buf16 say which epilogue forms the operands' alignment allows.  npar, wpar and the tile counts are the routes' business.
static ConvP build_params(const srcgan_conv_desc* d) {
    const int esz = d->dtype == SRCGAN_F32 ? 4 : 2, epp = 16 / esz;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.x = d->x; p.wp = d->wp; p.bias = d->bias; p.y = d->y; p.r1 = d->r1; p.r2 = d->r2; p.mz = d->mz;
    p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.xcoff = d->x_coff;
    p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout; p.YH = d->YH; p.YW = d->YW; p.ycoff = d->y_coff;
    p.pad_y = d->pad_y; p.pad_x = d->pad_x; p.os = d->os; p.oa = d->oa; p.ob = d->ob;
    p.r1coff = d->r1_coff; p.r1cend = d->r1_cend;
    p.r2coff = d->r2_coff; p.r2cend = d->r2_cend;
    p.mzcoff = d->mz_coff; p.mzc0 = d->mz_c0;
    auto pl = [](long v) { return v ? v : 64L; };      // plane stride 0 = interleaved NHWC
    p.xpix = (long)d->x_cs * esz; p.xplane = pl(d->x_plane); p.ypix = (long)d->y_cs * esz; p.yplane = pl(d->y_plane);
    p.r1pix = (long)d->r1_cs * esz; p.r1plane = pl(d->r1_plane); p.r2pix = (long)d->r2_cs * esz; p.r2plane = pl(d->r2_plane);
    p.mzpix = (long)d->mz_cs * esz; p.mzplane = pl(d->mz_plane);
    p.rev = d->rev_batch;
    p.sgn_out = (unsigned char*)d->sign_out; p.sgn_in = (const unsigned char*)d->sign_in;
    p.alpha = d->alpha; p.beta1 = d->beta1; p.beta2 = d->beta2; p.slope = d->slope; p.mslope = d->mslope;
    p.act = d->act;
    p.nchunk = cdiv(d->Cin, 64 / esz);
    auto m4 = [](int v) { return (v & 3) == 0; };
    p.vec = m4(d->Cout) && m4(d->y_cs) && m4(d->y_coff) && ((uintptr_t)d->y % 16 == 0) &&
            (!d->bias || ((uintptr_t)d->bias % 16 == 0)) &&
            (!d->r1 || (m4(d->r1_cs) && m4(d->r1_coff) && m4(d->r1_cend) && (uintptr_t)d->r1 % 16 == 0)) &&
            (!d->r2 || (m4(d->r2_cs) && m4(d->r2_coff) && m4(d->r2_cend) && (uintptr_t)d->r2 % 16 == 0)) &&
            (!d->mz || (m4(d->mz_cs) && m4(d->mz_coff) && m4(d->mz_c0) && (uintptr_t)d->mz % 16 == 0));
    auto me = [&](int v) { return v % epp == 0; };
    p.vec16 = p.vec && me(d->Cout) && me(d->y_cs) && me(d->y_coff) &&
              (!d->r1 || (me(d->r1_cs) && me(d->r1_coff) && me(d->r1_cend))) &&
              (!d->r2 || (me(d->r2_cs) && me(d->r2_coff) && me(d->r2_cend))) &&
              (!d->mz || (me(d->mz_cs) && me(d->mz_coff) && me(d->mz_c0)));
    const long lim = (1L << 31) - (1L << 20);
    p.buf16 = p.vec16 && p.yplane < lim && p.ypix < (1 << 20) && (!d->r1 || (p.r1plane < lim && p.r1pix < (1 << 20))) &&
              (!d->r2 || (p.r2plane < lim && p.r2pix < (1 << 20))) && (!d->mz || (p.mzplane < lim && p.mzpix < (1 << 20)));
    return p;
}

// The generic, four-parity and self-loading kernels carry a halo piece's byte offset inside its image in 32 bits (h_goff): one image of the
// input, H * W pixel records, must stay below 2 GiB.  Only the loader-specialised 3x3 stride-1 kernel rebases per tile (conv3x3_dma.hip,
// which applies this check itself where it falls back to the self-loading kernel).  Any number of such images is fine: the image base is 64-bit.
int sg_require_image_31(const ConvP& p) {
    SG_REQUIRE((long)p.H * p.W * p.xpix < (1L << 31),
               "srcgan_conv_igemm: one image of the input must be below 2 GiB for this kernel (%d x %d pixels of %ld bytes); only the loader-specialised "
               "3x3 stride-1 form (pad 1, whole 64-byte input chunks, 18 rows below 2 GiB) takes larger images", p.H, p.W, p.xpix);
    return 0;
}

// ---- step 3: the kernel family.  The parity forms (npar != 0) come first, each with the rule its kernel sets
static int route(const srcgan_conv_desc* d, ConvP& p, hipStream_t st) {
    if (d->npar && d->kh == 3) {
        // ConvTranspose2d(k3, s2, p1, output_padding 1): the four output parities (1, 2, 2 and 4 taps) in one launch (deconv_k3s2.hip)
        SG_REQUIRE(d->npar == 4 && d->kw == 3 && d->stride == 2 && d->pad_y == 1 && d->pad_x == 1 && d->os == 2 && d->oa == 0 && d->ob == 0 &&
                   d->OH == d->H && d->OW == d->W && d->YH == 2 * d->H && d->YW == 2 * d->W && d->wpar_stride > 0 && d->wpar_stride % 16 == 0 &&
                   !d->x_plane && !d->y_plane && !d->sign_in && !d->sign_out,
                   "srcgan_conv_igemm: npar == 4 with a 3x3 kernel is the transposed stride-2 form: stride 2, pad 1, os 2, oa == ob == 0, OH x OW = H x W, "
                   "YH x YW = 2H x 2W, the four parity packs wpar_stride bytes apart, interleaved tensors, no sign masks");
        SG_TRY(sg_require_image_31(p));
        p.npar = 4; p.wpar = d->wpar_stride;
        return sg_deconv_k3s2(p, d->dtype, st);
    }
    if (d->npar && d->kh == 1 && d->kw == 1) {
        // four output parities of a stride-2 scatter in one launch: parity q = (oa, ob) = (q >> 1, q & 1) uses the pack at wp + q * wpar_stride
        SG_REQUIRE(d->npar == 4 && d->stride == 1 && d->os == 2 && d->oa == 0 && d->ob == 0 && d->wpar_stride > 0 && d->wpar_stride % 16 == 0 &&
                   !d->sign_in, "srcgan_conv_igemm: npar == 4 with a 1x1 kernel needs os == 2, oa == ob == 0 and the four packs wpar_stride bytes apart");
        SG_REQUIRE(!d->sign_out || p.buf16, "srcgan_conv_igemm: sign_out of the 1x1 four-parity form needs 16-byte accessible output channels");
        p.npar = 4; p.wpar = d->wpar_stride;
    } else if (d->npar) {
        SG_REQUIRE(d->npar == 4 && d->kh == 2 && d->kw == 2 && d->stride == 1 && d->wpar_stride > 0 && d->wpar_stride % 16 == 0 && !d->x_plane && !d->y_plane &&
                   !d->sign_in && !d->sign_out,
                   "srcgan_conv_igemm: npar must be 0 or 4 (2x2 stride-1 parity packs wpar_stride bytes apart, interleaved tensors, no bias / sign masks)");
        // (the message's wording is pinned by tests/test_conv_entry_host.py and dates from before the U-Net: a bias IS taken now -- the epilogue
        //  this kernel shares with every other one always added it; ConvTranspose2d(k4, s2, p1) + bias is this launch, RD_DECONV4 in oplist.hip)
        SG_TRY(sg_require_image_31(p));
        p.wpar = d->wpar_stride;
        return sg_dgrad_s2k4(p, d->dtype, st);
    }
    if (d->kh == 3 && d->kw == 3 && d->stride == 1 && (!g_force_generic || d->x_plane)) return sg_conv3x3_dma(p, d->dtype, st);
    SG_TRY(sg_require_image_31(p));
    return sg_conv_generic(p, d->dtype, d->kh, d->kw, d->stride, st);
}

extern "C" int srcgan_conv_igemm(const srcgan_conv_desc* d, void* stream) {
    SG_TRY(check_desc(d));
    ConvP p = build_params(d);
    return route(d, p, (hipStream_t)stream);
}
