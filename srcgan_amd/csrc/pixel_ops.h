// Per-pixel device functions that more than one kernel evaluates and whose callers rely on getting the SAME BITS from each of them:
//   sg_gray_u8          8-bit RGB -> gray          srcgan_u8rgb_to_planes mode 0 (colour.hip)  and  srcgan_tile_gather_ex kind 2 (tiles.hip)
//   sg_bilinear_sample  one x`up` bilinear sample  srcgan_bilinear_up (elementwise.hip)        and  srcgan_tile_gather_ex s > 1   (tiles.hip)
//   sg_lab_to_u8rgb     normalised LAB -> 8-bit    srcgan_lab_planes_to_u8rgb (colour.hip)     and  srcgan_tile_scatter_u8 mode 1 (tiles.hip)
// hipcc contracts a * b + c into a fused multiply-add wherever it sees the pattern after inlining, and which products it picks depends
// on the surrounding code (loop unrolling, packed-math pairing), so two call sites of the same C++ expression need not round alike.
// The first two are therefore written as a fixed sequence of rounding steps: contraction is switched off inside them
// (`#pragma clang fp contract(off)`: every * and - below is one rounding; the headers' __fmul_rn / __fsub_rn are plain operators that
// inherit the translation unit's contraction, so the pragma is what pins them) and the fused steps are spelled __fmaf_rn / __fma_rn.
// The sequences are the ones hipcc chose for the former in-kernel expressions (for the bilinear sample: in the unrolled main loop).
#pragma once
#include <hip/hip_runtime.h>

// u8 -> f32 exactly as data.arr2rgb / srcgan_u8rgb_to_planes mode 1: the quotient in double, one rounding to float
__device__ __forceinline__ float sg_u8_unit(unsigned char v) { return (float)((double)v / 255.0); }

// skimage rgb2gray of an 8-bit pixel (dataset.py:114-123): /255 and the luma weights in double, one rounding to float
__device__ __forceinline__ float sg_gray_u8(unsigned char r8, unsigned char g8, unsigned char b8) {
#pragma clang fp contract(off)
    const double r = (double)r8 / 255.0, g = (double)g8 / 255.0, b = (double)b8 / 255.0;
    return (float)__fma_rn(0.0721, b, __fma_rn(0.2125, r, 0.7154 * g));
}

// One axis of F.interpolate(scale_factor=up, mode="bilinear", align_corners=False): output index o -> source coordinate
// (o + 0.5) / up - 0.5 clamped at 0, its two neighbours (the upper one clamped at the border) and their weights.
// The coordinate is (2 o + 1 - up) / (2 up): its integer part and remainder are taken in integers, so each weight is one correctly
// rounded quotient, whatever the size of the coordinate.
struct SgLerp { int i0, i1; float w0, w1; };
__device__ __forceinline__ SgLerp sg_bilinear_axis(int o, int n, int up) {
    const int num = 2 * o + 1 - up, den = 2 * up;
    int i0 = 0, r = 0;
    if (num > 0) { i0 = num / den; r = num - i0 * den; }
    i0 = min(i0, n - 1);                                   // num / den <= n - 1 for every o < n * up; the clamp only documents it
    return SgLerp{i0, i0 + (i0 < n - 1 ? 1 : 0), (float)(den - r) / (float)den, (float)r / (float)den};
}
// The sample at the two axes' positions (a caller with several samples in one row or column computes that axis once).
// tap(y, x) returns the source sample; it is called with 0 <= y < H, 0 <= x < W only
template <typename Tap>
__device__ __forceinline__ float sg_bilinear_sample(Tap tap, const SgLerp& y, const SgLerp& x) {
#pragma clang fp contract(off)
    const float top = __fmaf_rn(x.w1, tap(y.i0, x.i1), x.w0 * tap(y.i0, x.i0));
    const float bot = __fmaf_rn(x.w1, tap(y.i1, x.i1), x.w0 * tap(y.i1, x.i0));
    return __fmaf_rn(y.w0, top, y.w1 * bot);
}

// normalised (L, a, b) -> 8-bit RGB (dataset.py:92-104: L*100, ab*255-128, skimage lab2rgb, *255, truncation to uint8).  Double
// arithmetic; moved here unchanged from lab_planes_to_u8rgb_k, so both callers inline the same expression tree.
__device__ __forceinline__ double sg_lin_to_srgb(double c) { return c > 0.0031308 ? 1.055 * pow(c, 1.0 / 2.4) - 0.055 : c * 12.92; }
__device__ __forceinline__ double sg_lab_finv(double t) { return t > 0.2068966 ? t * t * t : (t - 16.0 / 116.0) / 7.787; }
__device__ __forceinline__ void sg_lab_to_u8rgb(float Ln, float an, float bn, unsigned char (&rgb)[3]) {
    // inverse of the sRGB->XYZ matrix rounded to 6 places (numpy.linalg.inv in the reference)
    const double m00 = 3.240481343200527, m01 = -1.5371515162713185, m02 = -0.49853632616888777;
    const double m10 = -0.9692549499965682, m11 = 1.8759900014898907, m12 = 0.04155592655829284;
    const double m20 = 0.05564663913517715, m21 = -0.20404133836651123, m22 = 1.0573110696453443;
    const double L = (double)Ln * 100.0, A = (double)an * 255.0 - 128.0, Bb = (double)bn * 255.0 - 128.0;
    const double fy = (L + 16.0) / 116.0, fx = A / 500.0 + fy;
    double fz = fy - Bb / 200.0;
    if (fz < 0.0) fz = 0.0;
    const double x = sg_lab_finv(fx) * 0.95047, y = sg_lab_finv(fy), z = sg_lab_finv(fz) * 1.08883;
    double c[3] = {m00 * x + m01 * y + m02 * z, m10 * x + m11 * y + m12 * z, m20 * x + m21 * y + m22 * z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double v = sg_lin_to_srgb(c[k]);
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        rgb[k] = (unsigned char)(v * 255.0);
    }
}
