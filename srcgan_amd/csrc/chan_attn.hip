// Channel attention (squeeze-and-excitation) fused with the block residual, forward and backward, on NHWC activations
// (reference src/model/rcan.py:11-27 CALayer, :45-49 RCAB.forward):
//     p[b,c] = mean_hw t[b,.,c];  h = relu(W1 p + b1);  s = sigmoid(W2 h + b2);  y = t * s[b,c] (+ res)
// Replaces AdaptiveAvgPool2d(1), the two 1x1 convolutions on a [B,C,1,1] tensor, ReLU, Sigmoid, the broadcast multiply and the add.
//
// HBM-bound.  Forward: one read pass over t for the pooled sums, one read (t, res) / write (y) pass.  Backward: one read pass over
// (dy, t) for ds = sum_hw dy * t, one read (dy [, dres]) / write (dt, dres) pass.  Three launches each way:
//   ca_partial_k   per (sample, chunk of CA_CHUNK pixels, channel) sums; the chunking depends on hw alone
//   ca_gate_*_k    one block per sample folds the chunks in a fixed order and runs the tiny MLP (or its transpose)
//   ca_apply_*_k   the element-wise pass; the backward one carries, in trailing blocks of the same grid, the batch sums of the four
//                  parameter gradients (one thread per element, samples added in index order)
// No atomics anywhere: two runs on the same inputs give the same bits.  All sums and the gate are f32; y / dt / dres are rounded once.
//
// Also here: MeanShift (reference src/model/common.py:11-21), a frozen 1x1 convolution on the 3 image channels, as an element-wise
// kernel on the 8-channel image records (sg_meanshift).
#include "common.h"
#include "../../include/srcgan_amd.h"

#define DISPATCH_DTYPE(dtype, ...) \
    if ((dtype) == SRCGAN_F32) { using T = float; __VA_ARGS__; } \
    else if ((dtype) == SRCGAN_BF16) { using T = __bf16; __VA_ARGS__; } \
    else if ((dtype) == SRCGAN_F16) { using T = _Float16; __VA_ARGS__; } \
    else SG_FAIL("bad dtype %d", (int)(dtype));

namespace {
constexpr int CA_CHUNK = 256;           // pixels per partial-sum block
constexpr int CA_MAXC = 1024;

static inline int ew_blocks(long n, int per_block = 256) {
    long b = cdivl(n, per_block);
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
static inline long ca_nchunk(long hw) { return cdivl(hw, CA_CHUNK); }

// MODE 0: sum t.  MODE 1: sum dy * t.   partial[(b * nchunk + chunk) * C + c]
// A block's 256 threads are PL = 256 / (C / EPP) pixel lanes x C / EPP channel groups (threads beyond PL * VG idle); each thread adds its
// pixels in ascending order, then one thread per channel adds the PL lane sums in lane order.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void ca_partial_k(const T* __restrict__ t, int t_cs, const T* __restrict__ dy, int dy_cs, long hw, int C,
                                                    float* __restrict__ partial) {
    constexpr int EPP = DT<T>::EPP;
    typedef __attribute__((ext_vector_type(EPP))) T vecT;
    __shared__ float red[256 * EPP];
    const int b = blockIdx.y, VG = C / EPP, PL = 256 / VG;
    const int cg = threadIdx.x % VG, pl = threadIdx.x / VG, c0 = cg * EPP;
    const long p0 = (long)blockIdx.x * CA_CHUNK, p1 = (p0 + CA_CHUNK < hw) ? p0 + CA_CHUNK : hw;
    float s[EPP];
#pragma unroll
    for (int i = 0; i < EPP; ++i) s[i] = 0.f;
    if (pl < PL) {
        for (long px = p0 + pl; px < p1; px += PL) {
            const size_t q = (size_t)b * hw + px;
            const vecT tv = *(const vecT*)(t + q * t_cs + c0);
            if (MODE == 0) {
#pragma unroll
                for (int i = 0; i < EPP; ++i) s[i] += to_f(tv[i]);
            } else {
                const vecT gv = *(const vecT*)(dy + q * dy_cs + c0);
#pragma unroll
                for (int i = 0; i < EPP; ++i) s[i] += to_f(gv[i]) * to_f(tv[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < EPP; ++i) red[(pl * VG + cg) * EPP + i] = s[i];      // = red[pl * C + c]
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f;
        for (int q = 0; q < PL; ++q) a += red[q * C + c];
        partial[((size_t)b * gridDim.x + blockIdx.x) * C + c] = a;
    }
}

// sum of the nchunk partials of every channel of sample b, in a fixed order: J = max(1, 256 / C) strided sub-sums per channel
// (sub-sum j takes chunks j, j + J, ...), added in ascending j.  Result in out[c] (shared memory, C floats); tmp holds J * C floats.
__device__ __forceinline__ void ca_fold(const float* __restrict__ partial, int b, long nchunk, int C, float* tmp, float* out) {
    const int J = C >= 256 ? 1 : 256 / C;
    for (int w = threadIdx.x; w < J * C; w += 256) {
        const int c = w % C, j = w / C;
        float a = 0.f;
        for (long k = j; k < nchunk; k += J) a += partial[((size_t)b * nchunk + k) * C + c];
        tmp[w] = a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f;
        for (int j = 0; j < J; ++j) a += tmp[j * C + c];
        out[c] = a;
    }
    __syncthreads();
}

// saved[b] = { p[C], h[Cr], s[C] }
__global__ __launch_bounds__(256) void ca_gate_fwd_k(const float* __restrict__ partial, long nchunk, long hw, int C, int Cr, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                     float* __restrict__ saved) {
    __shared__ float tmp[CA_MAXC], p[CA_MAXC], h[CA_MAXC];
    const int b = blockIdx.x;
    float* sv = saved + (size_t)b * (2 * C + Cr);
    ca_fold(partial, b, nchunk, C, tmp, p);
    for (int c = threadIdx.x; c < C; c += 256) { const float m = p[c] / (float)hw; p[c] = m; sv[c] = m; }
    __syncthreads();
    for (int j = threadIdx.x; j < Cr; j += 256) {
        float a = b1[j];
        for (int c = 0; c < C; ++c) a += w1[(size_t)j * C + c] * p[c];
        a = a > 0.f ? a : 0.f;
        h[j] = a; sv[C + j] = a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = b2[c];
        for (int j = 0; j < Cr; ++j) a += w2[(size_t)c * Cr + j] * h[j];
        sv[C + Cr + c] = 1.f / (1.f + expf(-a));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ca_apply_fwd_k(const T* __restrict__ t, int t_cs, const T* __restrict__ res, int r_cs, T* __restrict__ y, int y_cs,
                                                      const float* __restrict__ saved, long hw, int C, int Cr, long nvec) {
    constexpr int EPP = DT<T>::EPP;
    typedef __attribute__((ext_vector_type(EPP))) T vecT;
    const int VG = C / EPP;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nvec; e += (long)gridDim.x * 256) {
        const int c0 = (int)(e % VG) * EPP; const long q = e / VG; const long b = q / hw;
        const float* s = saved + (size_t)b * (2 * C + Cr) + C + Cr + c0;
        const vecT tv = *(const vecT*)(t + q * t_cs + c0);
        vecT rv; if (res) rv = *(const vecT*)(res + q * r_cs + c0);
        vecT o;
#pragma unroll
        for (int i = 0; i < EPP; ++i) {
            float v = to_f(tv[i]) * s[i];
            if (res) v += to_f(rv[i]);
            o[i] = from_f<T>(v);
        }
        *(vecT*)(y + q * y_cs + c0) = o;
    }
}

// one block per sample: ds -> dz2 = ds s (1 - s) -> dh = (W2^T dz2) [h > 0] -> dp / hw.   work[b] = { dz2[C], dh[Cr], dp/hw[C] }
__global__ __launch_bounds__(256) void ca_gate_bwd_k(const float* __restrict__ partial, long nchunk, long hw, int C, int Cr, const float* __restrict__ w1,
                                                     const float* __restrict__ w2, const float* __restrict__ saved, float* __restrict__ work) {
    __shared__ float tmp[CA_MAXC], dz[CA_MAXC], dh[CA_MAXC];
    const int b = blockIdx.x;
    const float* sv = saved + (size_t)b * (2 * C + Cr);
    float* wk = work + (size_t)b * (2 * C + Cr);
    ca_fold(partial, b, nchunk, C, tmp, dz);
    for (int c = threadIdx.x; c < C; c += 256) { const float s = sv[C + Cr + c], v = dz[c] * (s * (1.f - s)); dz[c] = v; wk[c] = v; }
    __syncthreads();
    for (int j = threadIdx.x; j < Cr; j += 256) {
        float a = 0.f;
        for (int c = 0; c < C; ++c) a += w2[(size_t)c * Cr + j] * dz[c];
        a = sv[C + j] > 0.f ? a : 0.f;
        dh[j] = a; wk[C + j] = a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f;
        for (int j = 0; j < Cr; ++j) a += w1[(size_t)j * C + c] * dh[j];
        wk[C + Cr + c] = a / (float)hw;
    }
}

// blocks [0, napply): dt = dy s + dp / hw, dres (= or +=) dy.   blocks [napply, gridDim.x): the parameter gradients, one thread per element
// of { dW2 [C, Cr], db2 [C], dW1 [Cr, C], db1 [Cr] }, samples added in index order.
template <typename T>
__global__ __launch_bounds__(256) void ca_apply_bwd_k(const T* __restrict__ dy, int dy_cs, T* __restrict__ dt, int dt_cs, T* __restrict__ dres, int dr_cs, int dres_acc,
                                                      const float* __restrict__ saved, const float* __restrict__ work, float* __restrict__ dw1,
                                                      float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2, int B, long hw, int C,
                                                      int Cr, long nvec, int napply) {
    constexpr int EPP = DT<T>::EPP;
    typedef __attribute__((ext_vector_type(EPP))) T vecT;
    const int rec = 2 * C + Cr;
    if ((int)blockIdx.x >= napply) {
        const long CCr = (long)C * Cr, total = 2 * CCr + C + Cr;
        const long nb = gridDim.x - napply;
        for (long e = (long)(blockIdx.x - napply) * 256 + threadIdx.x; e < total; e += nb * 256) {
            float a = 0.f;
            if (e < CCr) {                      // dW2[c][j] = sum_b dz2[b][c] h[b][j]
                if (!dw2) continue;
                const int c = (int)(e / Cr), j = (int)(e % Cr);
                for (int b = 0; b < B; ++b) a += work[(size_t)b * rec + c] * saved[(size_t)b * rec + C + j];
                dw2[e] = a;
            } else if (e < CCr + C) {           // db2[c]
                if (!db2) continue;
                const int c = (int)(e - CCr);
                for (int b = 0; b < B; ++b) a += work[(size_t)b * rec + c];
                db2[c] = a;
            } else if (e < 2 * CCr + C) {       // dW1[j][c] = sum_b dh[b][j] p[b][c]
                if (!dw1) continue;
                const long r = e - CCr - C;
                const int j = (int)(r / C), c = (int)(r % C);
                for (int b = 0; b < B; ++b) a += work[(size_t)b * rec + C + j] * saved[(size_t)b * rec + c];
                dw1[r] = a;
            } else {                            // db1[j]
                if (!db1) continue;
                const int j = (int)(e - 2 * CCr - C);
                for (int b = 0; b < B; ++b) a += work[(size_t)b * rec + C + j];
                db1[j] = a;
            }
        }
        return;
    }
    const int VG = C / EPP;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nvec; e += (long)napply * 256) {
        const int c0 = (int)(e % VG) * EPP; const long q = e / VG; const long b = q / hw;
        const float* s = saved + (size_t)b * rec + C + Cr + c0;
        const float* dp = work + (size_t)b * rec + C + Cr + c0;
        const vecT gv = *(const vecT*)(dy + q * dy_cs + c0);
        vecT o;
#pragma unroll
        for (int i = 0; i < EPP; ++i) o[i] = from_f<T>(to_f(gv[i]) * s[i] + dp[i]);
        *(vecT*)(dt + q * dt_cs + c0) = o;
        if (dres) {
            vecT r = gv;
            if (dres_acc) {
                const vecT old = *(const vecT*)(dres + q * dr_cs + c0);
#pragma unroll
                for (int i = 0; i < EPP; ++i) r[i] = from_f<T>(to_f(gv[i]) + to_f(old[i]));
            }
            *(vecT*)(dres + q * dr_cs + c0) = r;
        }
    }
}

// y[q][0..2] = M x[q][0..2] (+ bias), M = W (transpose == 0) or W^T; channels 3..7 of the 8-channel record are written as zero
template <typename T>
__global__ __launch_bounds__(256) void meanshift_k(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ w, const float* __restrict__ bias,
                                                   int transpose, long npix) {
    float m[9], bb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[r * 3 + c] = transpose ? w[c * 3 + r] : w[r * 3 + c];
        bb[r] = bias ? bias[r] : 0.f;
    }
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < npix; q += (long)gridDim.x * 256) {
        float v[4], o[4], z[4] = {0.f, 0.f, 0.f, 0.f};
        load4<T>(x + q * 8, v);
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = bb[r] + m[r * 3] * v[0] + m[r * 3 + 1] * v[1] + m[r * 3 + 2] * v[2];
        o[3] = 0.f;
        store4<T>(y + q * 8, o);
        store4<T>(y + q * 8 + 4, z);
    }
}

static int ca_check(const char* who, int B, long hw, int C, int Cr, int dtype) {
    SG_REQUIRE(sg_dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    SG_REQUIRE(B > 0 && hw > 0, "%s: bad B / hw", who);
    SG_REQUIRE(C > 0 && C % 8 == 0 && C <= CA_MAXC, "%s: C = %d must be a multiple of 8, at most %d", who, C, CA_MAXC);
    SG_REQUIRE(Cr >= 1 && Cr <= C, "%s: Cr = %d must be in 1..C", who, Cr);
    SG_REQUIRE(B <= 65535 && ca_nchunk(hw) <= 0x7fffffffL, "%s: B / hw too large", who);
    return 0;
}
}  // namespace

extern "C" size_t srcgan_ca_scratch_floats(int B, long hw, int C) {
    if (B <= 0 || hw <= 0 || C <= 0) return 0;
    return (size_t)B * (size_t)ca_nchunk(hw) * C + (size_t)B * 3 * C;
}

extern "C" int srcgan_ca_forward(const void* t, int t_cs, const void* res, int res_cs, void* y, int y_cs, const float* w1, const float* b1,
                                 const float* w2, const float* b2, float* saved, int B, long hw, int C, int Cr, int dtype, float* scratch, void* stream) {
    SG_REQUIRE(t && y && w1 && b1 && w2 && b2 && saved && scratch, "srcgan_ca_forward: null pointer");
    SG_TRY(ca_check("srcgan_ca_forward", B, hw, C, Cr, dtype));
    const int epp = dtype == SRCGAN_F32 ? 4 : 8;
    SG_REQUIRE(t_cs >= C && y_cs >= C && t_cs % epp == 0 && y_cs % epp == 0 && (!res || (res_cs >= C && res_cs % epp == 0)),
               "srcgan_ca_forward: channel strides must be multiples of %d and at least C", epp);
    hipStream_t st = (hipStream_t)stream;
    const long nchunk = ca_nchunk(hw), nvec = (long)B * hw * (C / epp);
    DISPATCH_DTYPE(dtype, {
        hipLaunchKernelGGL((ca_partial_k<T, 0>), dim3((unsigned)nchunk, B), dim3(256), 0, st, (const T*)t, t_cs, (const T*)nullptr, 0, hw, C, scratch);
        hipLaunchKernelGGL(ca_gate_fwd_k, dim3(B), dim3(256), 0, st, (const float*)scratch, nchunk, hw, C, Cr, w1, b1, w2, b2, saved);
        hipLaunchKernelGGL(ca_apply_fwd_k<T>, dim3(ew_blocks(nvec)), dim3(256), 0, st, (const T*)t, t_cs, (const T*)res, res_cs, (T*)y, y_cs,
                           (const float*)saved, hw, C, Cr, nvec);
    });
    SG_LAUNCH_CHECK();
    return 0;
}

extern "C" int srcgan_ca_backward(const void* dy, int dy_cs, const void* t, int t_cs, const float* w1, const float* w2, const float* saved, void* dt,
                                  int dt_cs, void* dres, int dres_cs, int dres_accumulate, float* dw1, float* db1, float* dw2, float* db2, int B,
                                  long hw, int C, int Cr, int dtype, float* scratch, void* stream) {
    SG_REQUIRE(dy && t && w1 && w2 && saved && dt && scratch, "srcgan_ca_backward: null pointer");
    SG_TRY(ca_check("srcgan_ca_backward", B, hw, C, Cr, dtype));
    const int epp = dtype == SRCGAN_F32 ? 4 : 8;
    SG_REQUIRE(dy_cs >= C && t_cs >= C && dt_cs >= C && dy_cs % epp == 0 && t_cs % epp == 0 && dt_cs % epp == 0 && (!dres || (dres_cs >= C && dres_cs % epp == 0)),
               "srcgan_ca_backward: channel strides must be multiples of %d and at least C", epp);
    hipStream_t st = (hipStream_t)stream;
    const long nchunk = ca_nchunk(hw), nvec = (long)B * hw * (C / epp);
    float* work = scratch + (size_t)B * nchunk * C;
    const int napply = ew_blocks(nvec);
    const long nparam = 2L * C * Cr + C + Cr;
    const int ngrad = (dw1 || db1 || dw2 || db2) ? (int)(cdivl(nparam, 256) > 256 ? 256 : cdivl(nparam, 256)) : 0;
    DISPATCH_DTYPE(dtype, {
        hipLaunchKernelGGL((ca_partial_k<T, 1>), dim3((unsigned)nchunk, B), dim3(256), 0, st, (const T*)t, t_cs, (const T*)dy, dy_cs, hw, C, scratch);
        hipLaunchKernelGGL(ca_gate_bwd_k, dim3(B), dim3(256), 0, st, (const float*)scratch, nchunk, hw, C, Cr, w1, w2, saved, work);
        hipLaunchKernelGGL(ca_apply_bwd_k<T>, dim3(napply + ngrad), dim3(256), 0, st, (const T*)dy, dy_cs, (T*)dt, dt_cs, (T*)dres, dres_cs, dres_accumulate,
                           saved, (const float*)work, dw1, db1, dw2, db2, B, hw, C, Cr, nvec, napply);
    });
    SG_LAUNCH_CHECK();
    return 0;
}

int sg_meanshift(const void* x, void* y, const float* w, const float* bias, int transpose, long npix, int dtype, hipStream_t st) {
    SG_REQUIRE(x && y && w && npix > 0, "meanshift: bad arguments");
    DISPATCH_DTYPE(dtype, {
        hipLaunchKernelGGL(meanshift_k<T>, dim3(ew_blocks(npix)), dim3(256), 0, st, (const T*)x, (T*)y, w, bias, transpose, npix);
    });
    SG_LAUNCH_CHECK();
    return 0;
}
