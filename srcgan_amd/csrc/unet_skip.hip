// The skip connection of the U-Net generator (reference src/model/basicModel.py:257-354) without torch.cat, on NHWC activations.
//
// A level's down-sampled tensor z = IN(conv(.)) has two consumers, each behind its own activation: the next down convolution reads
// LeakyReLU(z, 0.2), the level's transposed convolution reads [ReLU(z) | ReLU(up path)] -- the reference's in-place LeakyReLU puts
// leaky(z) into the concatenation, and ReLU(leaky(z)) = ReLU(z).  The concatenation is ONE buffer of 2 C channels whose halves are
// written in place by their producers:
//
//   srcgan_in_skip_forward   InstanceNorm2d (no affine part) with both activations from one read of the normalised value:
//                            a = LeakyReLU(z, slope) dense, r = ReLU(z) into channels [r_coff, r_coff + C) of the skip buffer.
//                            One statistics pass (the partial / fold kernels of srcgan_gn_forward, G == C: the same bits, the same
//                            saved layout, so srcgan_gn_backward serves) + one read / two-write pass.
//   srcgan_relu_nhwc         y[.., y_coff : y_coff + C] = max(x, 0): the outermost level, which has no norm -- its convolution
//                            stores LeakyReLU(z) from its epilogue, and ReLU(LeakyReLU(z)) = ReLU(z).
// HBM-bound; 16-byte accesses along the channels (srcgan_relu_nhwc: element by element where C, strides or bases do not allow them),
// every output element written exactly once, no atomics, every address in 64 bits.
#include "common.h"

namespace {
template <typename T, int V> struct alignas(sizeof(T) * V) Pk { T e[V]; };

// stats [B][C]{mean, rstd}; e walks the 16-byte pieces of [B * hw][C]
template <typename T>
__global__ __launch_bounds__(256) void in_skip_apply_k(const T* __restrict__ x, int x_cs, T* __restrict__ a, int a_cs, T* __restrict__ r, int r_cs,
                                                       const float* __restrict__ stats, long hw, int C, float slope, long nvec) {
    constexpr int EPP = DT<T>::EPP;
    typedef Pk<T, EPP> pk;
    const int VG = C / EPP;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nvec; e += (long)gridDim.x * 256) {
        const int c0 = (int)(e % VG) * EPP; const long q = e / VG; const long b = q / hw;
        const pk xv = *(const pk*)(x + q * x_cs + c0);
        const float* sp = stats + (b * C + c0) * 2;
        pk av, rv;
#pragma unroll
        for (int i = 0; i < EPP; ++i) {
            // srcgan_gn_forward without gamma / beta computes xhat * 1 + 0: the + 0 turns a negative zero into a positive one, as there
            const float v = (to_f(xv.e[i]) - sp[2 * i]) * sp[2 * i + 1] + 0.f;
            av.e[i] = from_f<T>(v > 0.f ? v : v * slope);
            rv.e[i] = from_f<T>(v > 0.f ? v : v * 0.f);
        }
        *(pk*)(a + q * a_cs + c0) = av;
        *(pk*)(r + q * r_cs + c0) = rv;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void relu_nhwc_k(const T* __restrict__ x, int x_cs, T* __restrict__ y, int y_cs, int C, long nvec) {
    typedef Pk<T, V> pk;
    const int VG = C / V;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nvec) return;
    const int c0 = (int)(e % VG) * V; const long q = e / VG;
    const pk xv = *(const pk*)(x + q * x_cs + c0);
    pk o;
#pragma unroll
    for (int i = 0; i < V; ++i) { const float v = to_f(xv.e[i]); o.e[i] = from_f<T>(v > 0.f ? v : 0.f); }
    *(pk*)(y + q * y_cs + c0) = o;
}

static inline int ew_blocks(long n) {
    const long b = cdivl(n, 256);
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
}  // namespace

extern "C" int srcgan_in_skip_forward(const void* x, int x_cs, void* a, int a_cs, void* r, int r_cs, int r_coff, float* stats, int B, long hw, int C,
                                      float eps, float slope, int dtype, float* scratch, void* stream) {
    const char* who = "srcgan_in_skip_forward";
    SG_REQUIRE(x && a && r && stats && scratch, "%s: null pointer", who);
    SG_REQUIRE(sg_dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    const int epp = dtype == SRCGAN_F32 ? 4 : 8, esz = dtype == SRCGAN_F32 ? 4 : 2;
    SG_REQUIRE(B > 0 && hw > 0 && C > 0 && C % epp == 0, "%s: bad B / hw / C (C a multiple of %d)", who, epp);
    SG_REQUIRE(x_cs % epp == 0 && a_cs % epp == 0 && r_cs % epp == 0 && r_coff % epp == 0, "%s: channel strides and the offset must be multiples of %d", who, epp);
    SG_REQUIRE(x_cs >= C && a_cs >= C && r_coff >= 0 && r_coff + C <= r_cs, "%s: a channel stride is smaller than the channels it holds", who);
    SG_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)r % 16 == 0, "%s: tensors must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    SG_TRY(sg_gn_stats(x, x_cs, stats, B, hw, C, C, eps, dtype, scratch, st));        // refuses what srcgan_gn_forward refuses (C <= 1024, C / epp | 256)
    const long nvec = (long)B * hw * (C / epp);
    char* rp = (char*)r + (size_t)r_coff * esz;
    if (dtype == SRCGAN_F32)
        hipLaunchKernelGGL(in_skip_apply_k<float>, dim3(ew_blocks(nvec)), dim3(256), 0, st, (const float*)x, x_cs, (float*)a, a_cs, (float*)rp, r_cs, (const float*)stats, hw, C, slope, nvec);
    else if (dtype == SRCGAN_BF16)
        hipLaunchKernelGGL(in_skip_apply_k<__bf16>, dim3(ew_blocks(nvec)), dim3(256), 0, st, (const __bf16*)x, x_cs, (__bf16*)a, a_cs, (__bf16*)rp, r_cs, (const float*)stats, hw, C, slope, nvec);
    else
        hipLaunchKernelGGL(in_skip_apply_k<_Float16>, dim3(ew_blocks(nvec)), dim3(256), 0, st, (const _Float16*)x, x_cs, (_Float16*)a, a_cs, (_Float16*)rp, r_cs, (const float*)stats, hw, C, slope, nvec);
    SG_LAUNCH_CHECK();
    return 0;
}

#define RELU_LAUNCH(T_, V_) hipLaunchKernelGGL((relu_nhwc_k<T_, V_>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const T_*)x, x_cs, (T_*)yp, y_cs, C, nvec)
extern "C" int srcgan_relu_nhwc(const void* x, int x_cs, void* y, int y_cs, int y_coff, long npix, int C, int dtype, void* stream) {
    const char* who = "srcgan_relu_nhwc";
    SG_REQUIRE(x && y, "%s: null pointer", who);
    SG_REQUIRE(sg_dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    SG_REQUIRE(npix > 0 && C > 0 && x_cs >= C && y_coff >= 0 && y_coff + C <= y_cs, "%s: bad npix / C / channel stride / offset", who);
    const int epp = dtype == SRCGAN_F32 ? 4 : 8, esz = dtype == SRCGAN_F32 ? 4 : 2;
    char* yp = (char*)y + (size_t)y_coff * esz;
    const bool vec = C % epp == 0 && x_cs % epp == 0 && y_cs % epp == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)yp % 16 == 0;
    const int v = vec ? epp : 1;
    const long nvec = npix * (C / v), nb = cdivl(nvec, 256);
    SG_REQUIRE(nb < (1L << 31), "%s: too many elements for one launch", who);
    if (dtype == SRCGAN_F32) { if (vec) RELU_LAUNCH(float, 4); else RELU_LAUNCH(float, 1); }
    else if (dtype == SRCGAN_BF16) { if (vec) RELU_LAUNCH(__bf16, 8); else RELU_LAUNCH(__bf16, 1); }
    else { if (vec) RELU_LAUNCH(_Float16, 8); else RELU_LAUNCH(_Float16, 1); }
    SG_LAUNCH_CHECK();
    return 0;
}
#undef RELU_LAUNCH
