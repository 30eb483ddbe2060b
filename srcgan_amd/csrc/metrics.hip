// Evaluation metrics on device (reference src/metrics.py:10-144, driven by the test loop src/testCas.py:65-90): angular error,
// SSIM, value range.  MSE / PSNR reuse the loss reductions (elementwise.hip).  NCHW f32 in (network outputs), f32 out.
// All reductions are two-stage with a fixed order (deterministic).
#include "common.h"
#include "../../include/srcgan_amd.h"

namespace {
constexpr int MT_BLK = 64;      // partial blocks per image

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    __syncthreads();
    return t;       // valid in thread 0
}

// AE (metrics.py:12-33): per pixel acos(<p,t> / (|p||t| + eps)) in degrees; partial[b][blk] = sum over the block's pixels
__global__ __launch_bounds__(256) void ae_partial_k(const float* __restrict__ p, const float* __restrict__ t, int C, long hw, float* __restrict__ partial) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const float* pb = p + (size_t)b * C * hw; const float* tb = t + (size_t)b * C * hw;
    float s = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
        float dot = 0.f, np = 0.f, nt = 0.f;
        for (int c = 0; c < C; ++c) { const float a = pb[(size_t)c * hw + i], q = tb[(size_t)c * hw + i]; dot += a * q; np += a * a; nt += q * q; }
        s += 57.29577951308232f * acosf(dot / (sqrtf(np) * sqrtf(nt) + 1e-6f));
    }
    const float tot = block_sum(s, red);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = tot;
}
// out[b*nout + j] = scale * sum_k partial[(b*nblk + k)*nout + j]
__global__ void fold_k(const float* __restrict__ partial, int nblk, int nout, float scale, float* __restrict__ out) {
    const int b = blockIdx.x, j = threadIdx.x;
    if (j >= nout) return;
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += partial[((size_t)b * nblk + k) * nout + j];
    out[b * nout + j] = s * scale;
}

// per-frame min / max of a [BC, F, HW] tensor over all BC planes of frame f = blockIdx.y (SSIM picks its dynamic range from them,
// metrics.py:100-107; DSSIMLoss3D picks one range per frame, like the reference's loop over frames):
// partial[(f*gridDim.x + blk)*2 + {min, max}], folded by minmax_fold_k on a (1, F) grid
__global__ __launch_bounds__(256) void minmax_frames_partial_k(const float* __restrict__ x, int BC, int F, long hw, float* __restrict__ partial) {
    __shared__ float rmin[4], rmax[4];
    float lo = 3.4e38f, hi = -3.4e38f;
    for (int bc = 0; bc < BC; ++bc) {
        const float* xp = x + ((size_t)bc * F + blockIdx.y) * hw;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) { const float v = xp[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_down(lo, o, 64)); hi = fmaxf(hi, __shfl_down(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { rmin[threadIdx.x >> 6] = lo; rmax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = rmin[0]; hi = rmax[0];
        for (int w = 1; w < 4; ++w) { lo = fminf(lo, rmin[w]); hi = fmaxf(hi, rmax[w]); }
        float* o = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = lo; o[1] = hi;
    }
}
__global__ __launch_bounds__(256) void minmax_fold_k(const float* __restrict__ partial, int nblk, float* __restrict__ out) {
    __shared__ float rmin[4], rmax[4];
    partial += (size_t)blockIdx.y * nblk * 2; out += 2 * blockIdx.y;       // one (min, max) pair per frame
    float lo = 3.4e38f, hi = -3.4e38f;
    for (int k = threadIdx.x; k < nblk; k += 256) { lo = fminf(lo, partial[2 * k]); hi = fmaxf(hi, partial[2 * k + 1]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_down(lo, o, 64)); hi = fmaxf(hi, __shfl_down(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { rmin[threadIdx.x >> 6] = lo; rmax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { lo = fminf(lo, rmin[w]); hi = fmaxf(hi, rmax[w]); }
        out[0] = lo; out[1] = hi;
    }
}

// SSIM (metrics.py:72-144): 11x11 gaussian (sigma 1.5) depth-wise "valid" windows of x, y, x^2, y^2, xy; one workgroup per
// 16x16 tile of the (H-10)x(W-10) map of one (image, channel): 26x26 patches in LDS, separable passes, map value + contrast term
// summed per tile: partial[((b*C + c)*ntiles + tile)*2 + {ssim, cs}].  The dynamic range L is read from device memory
// (written by the range kernel) so the whole metric is stream-ordered without a host round trip.
// Frames: blockIdx.z = f of a [B,C,F,H,W] tensor; plane (bc, f) starts at element (bc*F + f)*H*W (64-bit), its partials sit at
// ((bc*F + f)*ntiles + tile)*2 and its dynamic range is range[2f .. 2f+1].  A 4-D tensor is the F = 1 instance (same addresses).
__global__ __launch_bounds__(256) void ssim_tile_k(const float* __restrict__ p, const float* __restrict__ t, int F, int H, int W, int tiles_x, int ntiles,
                                                  const float* __restrict__ range, float* __restrict__ partial) {
    __shared__ float sp[26][27], st[26][27];
    __shared__ float hz[5][26][16];
    __shared__ float red[4];
    __shared__ float gw[11];
    const int bc = blockIdx.y, tile = blockIdx.x, ty = tile / tiles_x, tx = tile % tiles_x;
    const size_t plane = (size_t)bc * F + blockIdx.z;
    range += 2 * blockIdx.z;
    const int oy0 = ty * 16, ox0 = tx * 16, OH = H - 10, OW = W - 10;
    const int tid = threadIdx.x;
    if (tid < 11) {
        float s = 0.f;
        for (int i = 0; i < 11; ++i) s += expf(-(float)((i - 5) * (i - 5)) / 4.5f);
        gw[tid] = expf(-(float)((tid - 5) * (tid - 5)) / 4.5f) / s;
    }
    const float* pb = p + plane * H * W; const float* tb = t + plane * H * W;
    for (int i = threadIdx.x; i < 26 * 26; i += 256) {
        const int y = i / 26, x = i % 26, gy = oy0 + y, gx = ox0 + x;
        const bool ok = gy < H && gx < W;
        sp[y][x] = ok ? pb[(size_t)gy * W + gx] : 0.f;
        st[y][x] = ok ? tb[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 26 * 16; i += 256) {
        const int y = i / 16, x = i % 16;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) { const float w = gw[k], u = sp[y][x + k], v = st[y][x + k]; a += w * u; b += w * v; aa += w * u * u; bb += w * v * v; ab += w * u * v; }
        hz[0][y][x] = a; hz[1][y][x] = b; hz[2][y][x] = aa; hz[3][y][x] = bb; hz[4][y][x] = ab;
    }
    __syncthreads();
    const int y = threadIdx.x / 16, x = threadIdx.x % 16;
    float ssim = 0.f, cs = 0.f;
    if (oy0 + y < OH && ox0 + x < OW) {
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 11; ++k)
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] += gw[k] * hz[q][y + k][x];
        const float max_val = range[1] > 128.f ? 255.f : 1.f, min_val = range[0] < -0.5f ? -1.f : 0.f, L = max_val - min_val;
        const float C1 = (0.01f * L) * (0.01f * L), C2 = (0.03f * L) * (0.03f * L);
        const float mu1sq = m[0] * m[0], mu2sq = m[1] * m[1], mu12 = m[0] * m[1];
        const float v1 = 2.f * (m[4] - mu12) + C2, v2 = (m[2] - mu1sq) + (m[3] - mu2sq) + C2;
        cs = v1 / v2;
        ssim = ((2.f * mu12 + C1) * v1) / ((mu1sq + mu2sq + C1) * v2);
    }
    const float s0 = block_sum(ssim, red);
    const float s1 = block_sum(cs, red);
    if (threadIdx.x == 0) { float* o = partial + (plane * ntiles + tile) * 2; o[0] = s0; o[1] = s1; }
}

// DSSIM loss forward fold: out = (1 - mean of the ssim_tile_k map sums) / 2 over all npart tiles of all (image, channel) slices.
// Two stages of fixed order (deterministic): DS_FOLD workgroups each sum one contiguous chunk, then one workgroup sums their
// results.  Accumulates in f64: the loss is a small difference from 1, and a batch's loss then equals the mean of its images'
// losses to f32 rounding.
constexpr int DS_FOLD = 256;
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];     // valid in every thread; blockDim.x == 256
}
__global__ __launch_bounds__(256) void dssim_fold_partial_k(const float* __restrict__ partial, long npart, double* __restrict__ dpart) {
    __shared__ double red[4];
    const long chunk = (npart + DS_FOLD - 1) / DS_FOLD, i0 = blockIdx.x * chunk, i1 = i0 + chunk < npart ? i0 + chunk : npart;
    double s = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) s += (double)partial[2 * i];
    const double tot = block_sum_f64(s, red);
    if (threadIdx.x == 0) dpart[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void dssim_fold_k(const double* __restrict__ dpart, double npos, float* __restrict__ out) {
    __shared__ double red[4];
    const double tot = block_sum_f64(dpart[threadIdx.x], red);
    if (threadIdx.x == 0) out[0] = (float)(0.5 * (1.0 - tot / npos));
}

// DSSIM loss backward (gradient of (1 - mean SSIM) / 2).  For one window position p with window means mu_x, mu_y, e_xx, e_yy, e_xy:
//   A1 = 2 mu_x mu_y + C1, A2 = mu_x^2 + mu_y^2 + C1, B1 = 2 s_xy + C2, B2 = s_xx + s_yy + C2, D = 1/(A2 B2), S = A1 B1 D
//   a_x = dS/dmu_x = 2 [mu_y B1 D - mu_x S/A2 - mu_y A1 D + mu_x S/B2]   (a_y: x and y swapped)
//   b = dS/de_xx = dS/de_yy = -S/B2,   c = dS/de_xy = 2 A1 D
// (S/A1 = B1 D and S/B1 = A1 D: nothing divides by A1 or B1, which can be 0).  Then for every pixel q of the H x W slice
//   dx(q) = -g/(2N) [(w * a_x)(q) + 2 x(q) (w * b)(q) + y(q) (w * c)(q)],  dy(q) likewise with a_y, 2 y(q), x(q)
// where * is the transposed ("full") 11x11 correlation over the valid positions covering q and N = B C (H-10)(W-10).
// One workgroup per 32x32 output tile of one (image, channel): the 52x52 input patch (10-pixel halo each side) -> window
// statistics of the 42x42 positions that cover the tile (separable, in LDS) -> the 3 or 4 position maps (zero outside the valid
// range) -> separable transposed blur back onto the tile.  No intermediate map leaves LDS; each output is written by one thread.
// Every pass is register-blocked along its stencil axis (a thread slides the 11 taps over a run of 7, 7, 8 or 4 outputs), so each
// LDS value is read once per run instead of once per tap.
// Frames: blockIdx.z = f of a [B,C,F,H,W] tensor, addressed like ssim_tile_k; the upstream scalar enters as gout[0] * invF (the mean
// over frames).  The 4-D loss is the F = 1, invF = 1 instance: the same addresses and, the product by 1 being exact, the same bits.
constexpr int DS_T = 32, DS_P = DS_T + 20, DS_Q = DS_T + 10, DS_QS = DS_Q + 1;
template <bool DY>
__global__ __launch_bounds__(256) void dssim_bwd_k(const float* __restrict__ p, const float* __restrict__ t, int F, int H, int W, int tiles_x,
                                                  const float* __restrict__ range, const float* __restrict__ gout, float invF, float inv2n,
                                                  float* __restrict__ dp, float* __restrict__ dt) {
    constexpr int NM = DY ? 4 : 3;                            // maps: b, c, a_x [, a_y]
    constexpr int RH = 7, RV = 7, RT = 8, RO = 4;             // run lengths of the four passes
    static_assert(DS_Q % RH == 0 && DS_Q % RV == 0 && DS_T % RT == 0 && DS_T % RO == 0, "runs tile the passes");
    static_assert((DS_Q / RV) * DS_Q <= 256 && DS_T * (DS_T / RO) == 256, "one vertical run per thread");
    // region 0: the x / y patches [2][52][52], later the horizontally blurred maps [NM][42][32]
    // region 1: the horizontal window sums [5][52][42], later the position maps [NM][42][43]
    __shared__ float r0[2 * DS_P * DS_P];
    __shared__ float r1[5 * DS_P * DS_Q];
    __shared__ float gws[11];
    static_assert(NM * DS_Q * DS_T <= 2 * DS_P * DS_P && NM * DS_Q * DS_QS <= 5 * DS_P * DS_Q, "LDS aliasing");
    float* sx = r0; float* sy = r0 + DS_P * DS_P;
    const int tid = threadIdx.x, bc = blockIdx.y, tile = blockIdx.x, ty = tile / tiles_x, tx = tile % tiles_x;
    const int oy0 = ty * DS_T, ox0 = tx * DS_T, OH = H - 10, OW = W - 10;
    if (tid < 11) {
        float s = 0.f;
        for (int i = 0; i < 11; ++i) s += expf(-(float)((i - 5) * (i - 5)) / 4.5f);
        gws[tid] = expf(-(float)((tid - 5) * (tid - 5)) / 4.5f) / s;
    }
    const size_t base = ((size_t)bc * F + blockIdx.z) * H * W;
    range += 2 * blockIdx.z;
    const float* pb = p + base; const float* tb = t + base;
    for (int i = tid; i < DS_P * DS_P; i += 256) {
        const int y = i / DS_P, x = i % DS_P, gy = oy0 - 10 + y, gx = ox0 - 10 + x;
        const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
        sx[i] = ok ? pb[(size_t)gy * W + gx] : 0.f;
        sy[i] = ok ? tb[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    float w[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) w[k] = gws[k];
    // this thread's outputs: column lx, rows ly0 .. ly0+3
    const int lx = tid % DS_T, ly0 = RO * (tid / DS_T);
    float xv[RO], yv[RO];
#pragma unroll
    for (int k = 0; k < RO; ++k) { const int i = (ly0 + k + 10) * DS_P + lx + 10; xv[k] = sx[i]; yv[k] = sy[i]; }
    // horizontal window sums of x, y, x^2, y^2, xy: 52 rows x 6 runs of 7 position columns
    float* hz = r1;
    for (int i = tid; i < DS_P * (DS_Q / RH); i += 256) {
        const int y = i / (DS_Q / RH), x0 = RH * (i % (DS_Q / RH));
        float u[RH + 10], v[RH + 10];
#pragma unroll
        for (int j = 0; j < RH + 10; ++j) { u[j] = sx[y * DS_P + x0 + j]; v[j] = sy[y * DS_P + x0 + j]; }
#pragma unroll
        for (int o = 0; o < RH; ++o) {
            float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) { const float uu = u[o + k], vv = v[o + k]; a += w[k] * uu; b += w[k] * vv; aa += w[k] * uu * uu; bb += w[k] * vv * vv; ab += w[k] * uu * vv; }
            const int h = y * DS_Q + x0 + o;
            hz[h] = a; hz[DS_P * DS_Q + h] = b; hz[2 * DS_P * DS_Q + h] = aa; hz[3 * DS_P * DS_Q + h] = bb; hz[4 * DS_P * DS_Q + h] = ab;
        }
    }
    __syncthreads();
    // vertical sums -> position maps: one run of 7 position rows of one position column per thread (6 x 42 = 252 threads),
    // held in registers until every thread has finished reading hz
    const float max_val = range[1] > 128.f ? 255.f : 1.f, min_val = range[0] < -0.5f ? -1.f : 0.f, L = max_val - min_val;
    const float C1 = (0.01f * L) * (0.01f * L), C2 = (0.03f * L) * (0.03f * L);
    const bool vact = tid < (DS_Q / RV) * DS_Q;
    const int vx = tid % DS_Q, vy0 = RV * (tid / DS_Q);
    float mv[RV][NM];
#pragma unroll
    for (int o = 0; o < RV; ++o)
#pragma unroll
        for (int q = 0; q < NM; ++q) mv[o][q] = 0.f;
    if (vact) {
        float m[RV][5];
#pragma unroll
        for (int o = 0; o < RV; ++o)
#pragma unroll
            for (int q = 0; q < 5; ++q) m[o][q] = 0.f;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float h[RV + 10];
#pragma unroll
            for (int j = 0; j < RV + 10; ++j) h[j] = hz[q * DS_P * DS_Q + (vy0 + j) * DS_Q + vx];
#pragma unroll
            for (int o = 0; o < RV; ++o)
#pragma unroll
                for (int k = 0; k < 11; ++k) m[o][q] += w[k] * h[o + k];
        }
        const int px = ox0 - 10 + vx;
#pragma unroll
        for (int o = 0; o < RV; ++o) {
            const int py = oy0 - 10 + vy0 + o;
            if (py < 0 || py >= OH || px < 0 || px >= OW) continue;
            const float* mo = m[o];
            const float mu1sq = mo[0] * mo[0], mu2sq = mo[1] * mo[1], mu12 = mo[0] * mo[1];
            const float B1 = 2.f * (mo[4] - mu12) + C2, B2 = (mo[2] - mu1sq) + (mo[3] - mu2sq) + C2;
            const float A1 = 2.f * mu12 + C1, A2 = mu1sq + mu2sq + C1;
            const float rA2 = 1.f / A2, rB2 = 1.f / B2, D = rA2 * rB2, S = A1 * B1 * D;
            const float B1D = B1 * D, A1D = A1 * D, SA2 = S * rA2, SB2 = S * rB2;
            mv[o][0] = -SB2;
            mv[o][1] = 2.f * A1D;
            mv[o][2] = 2.f * (mo[1] * B1D - mo[0] * SA2 - mo[1] * A1D + mo[0] * SB2);
            if (DY) mv[o][NM - 1] = 2.f * (mo[0] * B1D - mo[1] * SA2 - mo[0] * A1D + mo[1] * SB2);
        }
    }
    __syncthreads();
    float* mp = r1;                                          // [NM][42][43]
    if (vact) {
#pragma unroll
        for (int o = 0; o < RV; ++o)
#pragma unroll
            for (int q = 0; q < NM; ++q) mp[(q * DS_Q + vy0 + o) * DS_QS + vx] = mv[o][q];
    }
    __syncthreads();
    // transposed horizontal blur: output column lx is covered by position columns lx .. lx+10 with weight w[10-k] = w[k]
    // (the window is symmetric), so it reads like a forward correlation.  42 rows x 4 runs of 8 output columns.
    float* th = r0;                                          // [NM][42][32]; the patch is dead (x, y of the outputs are in xv / yv)
    for (int i = tid; i < DS_Q * (DS_T / RT); i += 256) {
        const int y = i / (DS_T / RT), x0 = RT * (i % (DS_T / RT));
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            float h[RT + 10];
#pragma unroll
            for (int j = 0; j < RT + 10; ++j) h[j] = mp[(q * DS_Q + y) * DS_QS + x0 + j];
#pragma unroll
            for (int o = 0; o < RT; ++o) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) acc += w[k] * h[o + k];
                th[(q * DS_Q + y) * DS_T + x0 + o] = acc;
            }
        }
    }
    __syncthreads();
    // transposed vertical blur of this thread's 4 outputs, then the per-pixel combination
    float acc[RO][NM];
#pragma unroll
    for (int q = 0; q < NM; ++q) {
        float h[RO + 10];
#pragma unroll
        for (int j = 0; j < RO + 10; ++j) h[j] = th[(q * DS_Q + ly0 + j) * DS_T + lx];
#pragma unroll
        for (int o = 0; o < RO; ++o) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) a += w[k] * h[o + k];
            acc[o][q] = a;
        }
    }
    const float g = gout[0] * invF;
    const float sc = -g * inv2n;
    const int gx = ox0 + lx;
#pragma unroll
    for (int o = 0; o < RO; ++o) {
        const int gy = oy0 + ly0 + o;
        if (gy < H && gx < W) {
            const size_t off = base + (size_t)gy * W + gx;
            dp[off] = sc * (acc[o][2] + 2.f * xv[o] * acc[o][0] + yv[o] * acc[o][1]);
            if (DY) dt[off] = sc * (acc[o][NM - 1] + 2.f * yv[o] * acc[o][0] + xv[o] * acc[o][1]);
        }
    }
}
static inline int ds3_blocks(long n) { const long b = cdivl(n, 256); return (int)(b > 256 ? 256 : b); }       // range blocks per frame
}  // namespace

void sg_minmax_frames(const float* x, int planes, int frames, long n, int nblk, float* partial, float* range, hipStream_t st) {
    hipLaunchKernelGGL(minmax_frames_partial_k, dim3(nblk, frames), dim3(256), 0, st, x, planes, frames, n, partial);
    hipLaunchKernelGGL(minmax_fold_k, dim3(1, frames), dim3(256), 0, st, (const float*)partial, nblk, range);
}

extern "C" int srcgan_metric_scratch_floats(int B, int C, int H, int W) {
    const long tiles = (long)cdiv(H > 10 ? H - 10 : 1, 16) * cdiv(W > 10 ? W - 10 : 1, 16);
    const long a = (long)B * MT_BLK, s = (long)B * C * tiles * 2, m = 2 * 256;
    return (int)((a > s ? a : s) + m + 16);
}

// out[b] = mean angular error (degrees) of image b
extern "C" int srcgan_metric_ae(const float* pred, const float* truth, int B, int C, int H, int W, float* out, float* scratch, void* stream) {
    SG_REQUIRE(pred && truth && out && scratch && B > 0 && C > 0 && H > 0 && W > 0, "srcgan_metric_ae: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const long hw = (long)H * W;
    hipLaunchKernelGGL(ae_partial_k, dim3(MT_BLK, B), dim3(256), 0, st, pred, truth, C, hw, scratch);
    hipLaunchKernelGGL(fold_k, dim3(B), dim3(64), 0, st, (const float*)scratch, MT_BLK, 1, 1.f / (float)hw, out);
    SG_LAUNCH_CHECK();
    return 0;
}

// out[b][0] = mean of the SSIM map of image b (all channels), out[b][1] = mean contrast term; range_from = the tensor whose min / max
// select the dynamic range (the prediction, metrics.py:100-107)
extern "C" int srcgan_metric_ssim(const float* pred, const float* truth, int B, int C, int H, int W, float* out, float* scratch, void* stream) {
    SG_REQUIRE(pred && truth && out && scratch && B > 0 && C > 0, "srcgan_metric_ssim: bad arguments");
    SG_REQUIRE(H >= 11 && W >= 11, "srcgan_metric_ssim: images must be at least 11x11 (valid 11x11 windows)");
    hipStream_t st = (hipStream_t)stream;
    const int OH = H - 10, OW = W - 10, tiles_x = cdiv(OW, 16), ntiles = tiles_x * cdiv(OH, 16);
    float* range = scratch + (size_t)B * C * ntiles * 2;
    float* mm = range + 8;
    const long n = (long)B * C * H * W;
    sg_minmax_frames(pred, 1, 1, n, ds3_blocks(n), mm, range, st);        // one frame: the tensor is one contiguous run
    hipLaunchKernelGGL(ssim_tile_k, dim3(ntiles, B * C), dim3(256), 0, st, pred, truth, 1, H, W, tiles_x, ntiles, (const float*)range, scratch);
    hipLaunchKernelGGL(fold_k, dim3(B), dim3(64), 0, st, (const float*)scratch, C * ntiles, 2, 1.f / ((float)C * OH * OW), out);
    SG_LAUNCH_CHECK();
    return 0;
}

// ---- DSSIM loss (losses.DSSIMLoss and DSSIMLoss3D, reference src/losses.py:170-196): contiguous f32 [B,C,F,H,W], a [B,C,H,W] tensor
// being F = 1; the loss is the mean over frames of the per-frame DSSIM, each frame with the dynamic range of its own prediction.  One
// range launch, one tile launch and one fold cover all frames; nothing is copied per frame.

extern "C" long srcgan_dssim3d_scratch_floats(int B, int C, int F, int H, int W) {
    if (B <= 0 || C <= 0 || F <= 0 || H < 11 || W < 11) return 0;
    const long tiles = (long)cdiv(H - 10, 16) * cdiv(W - 10, 16);
    const long mm = (long)F * 256 * 2;          // per-frame range partials; the DS_FOLD f64 partials of the fold alias them
    return (long)B * C * F * tiles * 2 + (mm > 2 * DS_FOLD ? mm : 2 * DS_FOLD) + 16;
}

static int ds3_check(const char* who, int B, int C, int F, int H, int W) {
    SG_REQUIRE(B > 0 && C > 0 && F > 0, "%s: bad arguments", who);
    SG_REQUIRE(H >= 11 && W >= 11, "%s: images must be at least 11x11 (valid 11x11 windows)", who);
    SG_REQUIRE((long)B * C <= 65535 && F <= 65535, "%s: B*C and F must be at most 65535", who);
    return 0;
}

// out[0] = mean over f of (1 - SSIM_f) / 2; range[f][0..1] = min / max of frame f of the prediction (kept for the backward).  Every
// frame has the same number of window positions, so the mean over frames is one fold over all B*C*F plane sums.
extern "C" int srcgan_dssim3d_loss_fwd(const float* pred, const float* truth, int B, int C, int F, int H, int W, float* out, float* range,
                                       float* scratch, void* stream) {
    SG_REQUIRE(pred && truth && out && range && scratch, "srcgan_dssim3d_loss_fwd: null pointer");
    SG_TRY(ds3_check("srcgan_dssim3d_loss_fwd", B, C, F, H, W));
    hipStream_t st = (hipStream_t)stream;
    const int OH = H - 10, OW = W - 10, tiles_x = cdiv(OW, 16), ntiles = tiles_x * cdiv(OH, 16);
    const long npart = (long)B * C * F * ntiles, hw = (long)H * W;
    float* mm = scratch + (size_t)npart * 2;
    const int planes = F == 1 ? 1 : B * C;          // one frame: the tensor is one contiguous run, so no block idles on a small image
    const long n = F == 1 ? (long)B * C * hw : hw;
    sg_minmax_frames(pred, planes, F, n, ds3_blocks(n), mm, range, st);
    hipLaunchKernelGGL(ssim_tile_k, dim3(ntiles, B * C, F), dim3(256), 0, st, pred, truth, F, H, W, tiles_x, ntiles, (const float*)range, scratch);
    double* dpart = (double*)mm;            // the range partials are consumed by sg_minmax_frames before this point
    hipLaunchKernelGGL(dssim_fold_partial_k, dim3(DS_FOLD), dim3(256), 0, st, (const float*)scratch, npart, dpart);
    hipLaunchKernelGGL(dssim_fold_k, dim3(1), dim3(DS_FOLD), 0, st, (const double*)dpart, (double)B * C * F * OH * OW, out);
    SG_LAUNCH_CHECK();
    return 0;
}

// dpred = gout[0] * d loss / d pred on the [B,C,F,H,W] layout; dtruth (may be null) likewise; range = what the forward wrote
extern "C" int srcgan_dssim3d_loss_bwd(const float* pred, const float* truth, int B, int C, int F, int H, int W, const float* range,
                                       const float* gout, float* dpred, float* dtruth, void* stream) {
    SG_REQUIRE(pred && truth && range && gout && dpred, "srcgan_dssim3d_loss_bwd: null pointer");
    SG_TRY(ds3_check("srcgan_dssim3d_loss_bwd", B, C, F, H, W));
    hipStream_t st = (hipStream_t)stream;
    const int tiles_x = cdiv(W, DS_T), ntiles = tiles_x * cdiv(H, DS_T);
    const float invF = 1.0f / (float)F, inv2n = (float)(0.5 / ((double)B * C * (H - 10) * (W - 10)));
    if (dtruth)
        hipLaunchKernelGGL(dssim_bwd_k<true>, dim3(ntiles, B * C, F), dim3(256), 0, st, pred, truth, F, H, W, tiles_x, range, gout, invF, inv2n, dpred, dtruth);
    else
        hipLaunchKernelGGL(dssim_bwd_k<false>, dim3(ntiles, B * C, F), dim3(256), 0, st, pred, truth, F, H, W, tiles_x, range, gout, invF, inv2n, dpred, dtruth);
    SG_LAUNCH_CHECK();
    return 0;
}
