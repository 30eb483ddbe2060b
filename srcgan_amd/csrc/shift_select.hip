// Registration-tolerant pixel loss (reference src/losses.py:199-255, NearestSelector): per sample, compare the centre crop of the
// prediction with the target shifted by each of n x n offsets (n = 2 * shift, offsets in units of `stride`), keep the offset of the
// smallest L1 sum, and hand the two crops to an L1 criterion.
//
//   srcgan_shift_search:  one pass over both tensors.  A workgroup owns one 32 x 64 tile of one (b, c) crop plane, stages the target
//                         window (tile + (n-1)*stride apron) in LDS once, keeps 8 prediction pixels per lane in registers and
//                         accumulates all n*n candidates in n*n registers (at stride 1 every window value read from LDS feeds up to n
//                         candidates); wave shuffles + a fixed-order sum over the four waves give one
//                         n*n vector of partials per workgroup.  A second launch sums each sample's partials in a fixed order, takes
//                         the first minimum and writes (r, c); a third (one thread) folds the minima into the L1 loss.  No atomics.
//   srcgan_shift_gather:  bit-exact copy of each sample's selected window (the selection is read on the device).
//   srcgan_shift_l1_bwd:  full-size gradients of mean |output_crop - target_window| -- the expression of loss_bwd_k<0> (elementwise.hip).
#include "common.h"

#define SS_TW 64                   // tile columns = lanes of a wave: a wave's LDS read is 64 consecutive dwords of one window row
#define SS_TH 32                   // tile rows: 4 waves x SS_ROWS
#define SS_ROWS 8
#define SS_MAX_SHIFT 4             // n*n <= 64 accumulators stay in registers
#define SS_LDS_FLOATS 12288        // 48 KiB window budget per workgroup

__device__ __forceinline__ float ss_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// window pitch in floats: rows start 16-byte aligned (16-byte staging stores), and one spare 16-byte slot keeps the pitch off the
// multiples of 64 dwords.  The shifted reads cannot collide whatever the pitch: one wave reads 64 consecutive dwords of ONE window row.
static inline int ss_pitch(int apron) { return (SS_TW + apron + 3) / 4 * 4 + 4; }

// stride 1: the n candidate rows of neighbouring pixels overlap, so a lane walks its column of the window once per j -- SS_ROWS + n - 1
// LDS reads feed SS_ROWS * n terms (2.9x fewer reads than one per term at n = 4, 4.3x at n = 8).  MASKED: the wave's tile part is cut by
// the crop's edge; the window rows and columns past the image hold whatever LDS held, and the select drops them.
template <int NS, bool MASKED>
__device__ __forceinline__ void ss_accum_stride1(const float* wp, int pitch, const float (&o)[SS_ROWS], float (&acc)[NS * NS], bool xok,
                                                 int rows_here) {
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int rr = 0; rr < SS_ROWS + NS - 1; ++rr) {
            const float v = wp[rr * pitch + j];
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int r = rr - i;
                if (r >= 0 && r < SS_ROWS) {
                    const float a = fabsf(v - o[r]);
                    acc[i * NS + j] += MASKED ? ((xok && r < rows_here) ? a : 0.f) : a;
                }
            }
        }
}

template <int NS, bool D1>
__global__ __launch_bounds__(256) void ss_search_k(const float* __restrict__ output, const float* __restrict__ target, int H, int W,
                                                   int sd, int d, int ch, int cw, int tiles_x, int tiles_per_plane, int pitch, int vec,
                                                   float* __restrict__ partial) {
    constexpr int N2 = NS * NS;
    extern __shared__ __attribute__((aligned(16))) float ss_win[];
    __shared__ float red[4 * N2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane = blockIdx.x / tiles_per_plane, t = blockIdx.x % tiles_per_plane;
    const int ty0 = (t / tiles_x) * SS_TH, tx0 = (t % tiles_x) * SS_TW;
    const int apron = (NS - 1) * d;
    const int wh = min(SS_TH, ch - ty0) + apron;          // window rows ty0 .. ty0 + wh - 1 <= ch - 1 + apron <= H - 1
    const int ww = min(SS_TW, cw - tx0) + apron;          // window columns tx0 .. tx0 + ww - 1 <= cw - 1 + apron <= W - 1
    const size_t pbase = (size_t)plane * H * W;
    const float* __restrict__ tp = target + pbase + (size_t)ty0 * W + tx0;

    // this lane's prediction pixels: column tx0 + lane, rows ty0 + wave * 8 + r
    const float* __restrict__ op = output + pbase + (size_t)(sd + ty0 + wave * SS_ROWS) * W + sd + tx0 + lane;
    const bool xok = tx0 + lane < cw;
    const int rows_here = ch - (ty0 + wave * SS_ROWS);     // rows r < rows_here are inside the crop
    float o[SS_ROWS];
#pragma unroll
    for (int r = 0; r < SS_ROWS; ++r) o[r] = (xok && r < rows_here) ? op[(size_t)r * W] : 0.f;

    if (vec) {            // W % 4 == 0 and a 16-byte aligned base: tx0 + 4k + 3 < W whenever tx0 + 4k < tx0 + ww <= W
        const int q = (ww + 3) >> 2;
        for (int e = tid; e < wh * q; e += 256) {
            const int r = e / q, k = e - r * q;
            *(f32x4*)(ss_win + r * pitch + 4 * k) = *(const f32x4*)(tp + (size_t)r * W + 4 * k);
        }
    } else {
        for (int e = tid; e < wh * ww; e += 256) {
            const int r = e / ww, k = e - r * ww;
            ss_win[r * pitch + k] = tp[(size_t)r * W + k];
        }
    }
    __syncthreads();

    float acc[N2];
#pragma unroll
    for (int k = 0; k < N2; ++k) acc[k] = 0.f;
    if constexpr (D1) {
        const float* wp = ss_win + wave * SS_ROWS * pitch + lane;
        if (tx0 + SS_TW <= cw && rows_here >= SS_ROWS) ss_accum_stride1<NS, false>(wp, pitch, o, acc, xok, rows_here);      // wave-uniform
        else ss_accum_stride1<NS, true>(wp, pitch, o, acc, xok, rows_here);
    } else {
#pragma unroll
        for (int r = 0; r < SS_ROWS; ++r) {
            if (xok && r < rows_here) {
                const float* wp = ss_win + (wave * SS_ROWS + r) * pitch + lane;
#pragma unroll
                for (int i = 0; i < NS; ++i)
#pragma unroll
                    for (int j = 0; j < NS; ++j) acc[i * NS + j] += fabsf(wp[i * d * pitch + j * d] - o[r]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < N2; ++k) {
        const float s = ss_wave_sum(acc[k]);
        if (lane == 0) red[wave * N2 + k] = s;
    }
    __syncthreads();
    if (tid < N2) partial[(size_t)blockIdx.x * N2 + tid] = (red[tid] + red[N2 + tid]) + (red[2 * N2 + tid] + red[3 * N2 + tid]);
}

// one workgroup per sample: fixed-order sum of its P = C * tiles partial vectors, first minimum, (r, c)
template <int NS>
__global__ __launch_bounds__(256) void ss_select_k(const float* __restrict__ partial, int P, float* __restrict__ diff,
                                                   int* __restrict__ sel, float* __restrict__ minval) {
    constexpr int N2 = NS * NS;
    __shared__ float red[4 * N2];
    __shared__ float tot[N2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    float acc[N2];
#pragma unroll
    for (int k = 0; k < N2; ++k) acc[k] = 0.f;
    for (int p = tid; p < P; p += 256) {
        const float* __restrict__ q = partial + ((size_t)b * P + p) * N2;
#pragma unroll
        for (int k = 0; k < N2; ++k) acc[k] += q[k];
    }
#pragma unroll
    for (int k = 0; k < N2; ++k) {
        const float s = ss_wave_sum(acc[k]);
        if (lane == 0) red[wave * N2 + k] = s;
    }
    __syncthreads();
    if (tid < N2) {
        const float s = (red[tid] + red[N2 + tid]) + (red[2 * N2 + tid] + red[3 * N2 + tid]);
        tot[tid] = s;
        diff[(size_t)b * N2 + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        float bv = tot[0];
        for (int k = 1; k < N2; ++k)
            if (tot[k] < bv) { bv = tot[k]; best = k; }          // strict: the first minimum wins (torch.argmin)
        sel[2 * b] = best / NS;
        sel[2 * b + 1] = best % NS;
        minval[b] = bv;
    }
}

__global__ void ss_loss_k(const float* __restrict__ minval, int B, double n, float* __restrict__ loss) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += minval[b];
    *loss = (float)((double)s / n);
}

struct SsPlan { int n, apron, tiles_x, tiles_y, pitch; long blocks; };

static int ss_plan(const char* who, int B, int C, int H, int W, int shift, int stride, int crop_h, int crop_w, SsPlan& p) {
    SG_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape B=%d C=%d H=%d W=%d", who, B, C, H, W);
    SG_REQUIRE(shift >= 1 && stride >= 1, "%s: shift and stride must be at least 1, got shift=%d stride=%d", who, shift, stride);
    SG_REQUIRE(shift <= SS_MAX_SHIFT, "%s: shift=%d is not supported: the (2*shift)^2 candidate sums are kept in registers, shift <= %d",
               who, shift, SS_MAX_SHIFT);
    SG_REQUIRE(crop_h >= 1 && crop_w >= 1, "%s: empty crop %d x %d", who, crop_h, crop_w);
    p.n = 2 * shift;
    const long apron = (long)(p.n - 1) * stride;
    SG_REQUIRE(apron + crop_h <= H && apron + crop_w <= W && (long)shift * stride + crop_h <= H && (long)shift * stride + crop_w <= W,
               "%s: the shifted %d x %d crops leave the %d x %d image (shift=%d stride=%d)", who, crop_h, crop_w, H, W, shift, stride);
    p.apron = (int)apron;
    p.pitch = ss_pitch(p.apron);
    SG_REQUIRE((long)(SS_TH + apron) * p.pitch <= SS_LDS_FLOATS,
               "%s: the target window of a %d x %d tile with a %ld-pixel apron (shift=%d stride=%d) does not fit in LDS (%ld > %d floats)",
               who, SS_TH, SS_TW, apron, shift, stride, (long)(SS_TH + apron) * p.pitch, SS_LDS_FLOATS);
    p.tiles_x = cdiv(crop_w, SS_TW);
    p.tiles_y = cdiv(crop_h, SS_TH);
    p.blocks = (long)B * C * p.tiles_x * p.tiles_y;
    SG_REQUIRE(p.blocks <= 0x7fffffffL, "%s: too many tiles (%ld)", who, p.blocks);
    return 0;
}

extern "C" size_t srcgan_shift_search_scratch_floats(int B, int C, int H, int W, int shift, int stride, int crop_h, int crop_w) {
    SsPlan p;
    if (ss_plan("srcgan_shift_search", B, C, H, W, shift, stride, crop_h, crop_w, p)) return 0;
    return (size_t)p.blocks * p.n * p.n + (size_t)B;
}

template <int NS>
static int ss_search_launch(const float* output, const float* target, int B, int C, int H, int W, int shift, int stride, int crop_h,
                            int crop_w, const SsPlan& p, float* diff, int* sel, float* loss, float* scratch, hipStream_t st) {
    const int vec = (W % 4 == 0) && ((uintptr_t)target % 16 == 0);
    float* minval = scratch + (size_t)p.blocks * NS * NS;
    const size_t lds = (size_t)(SS_TH + p.apron) * p.pitch * sizeof(float);
    if (stride == 1)
        hipLaunchKernelGGL((ss_search_k<NS, true>), dim3((unsigned)p.blocks), dim3(256), lds, st, output, target, H, W, shift * stride, stride,
                           crop_h, crop_w, p.tiles_x, p.tiles_x * p.tiles_y, p.pitch, vec, scratch);
    else
        hipLaunchKernelGGL((ss_search_k<NS, false>), dim3((unsigned)p.blocks), dim3(256), lds, st, output, target, H, W, shift * stride, stride,
                           crop_h, crop_w, p.tiles_x, p.tiles_x * p.tiles_y, p.pitch, vec, scratch);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(ss_select_k<NS>, dim3(B), dim3(256), 0, st, scratch, C * p.tiles_x * p.tiles_y, diff, sel, minval);
    SG_LAUNCH_CHECK();
    if (loss) {
        hipLaunchKernelGGL(ss_loss_k, dim3(1), dim3(1), 0, st, minval, B, (double)B * C * crop_h * crop_w, loss);
        SG_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int srcgan_shift_search(const float* output, const float* target, int B, int C, int H, int W, int shift, int stride,
                                   int crop_h, int crop_w, float* diff, int* sel, float* loss, float* scratch, void* stream) {
    SG_REQUIRE(output && target && diff && sel && scratch, "srcgan_shift_search: null pointer");
    SsPlan p;
    SG_TRY(ss_plan("srcgan_shift_search", B, C, H, W, shift, stride, crop_h, crop_w, p));
    hipStream_t st = (hipStream_t)stream;
    switch (shift) {
        case 1: return ss_search_launch<2>(output, target, B, C, H, W, shift, stride, crop_h, crop_w, p, diff, sel, loss, scratch, st);
        case 2: return ss_search_launch<4>(output, target, B, C, H, W, shift, stride, crop_h, crop_w, p, diff, sel, loss, scratch, st);
        case 3: return ss_search_launch<6>(output, target, B, C, H, W, shift, stride, crop_h, crop_w, p, diff, sel, loss, scratch, st);
        default: return ss_search_launch<8>(output, target, B, C, H, W, shift, stride, crop_h, crop_w, p, diff, sel, loss, scratch, st);
    }
}

// ----------------------------------------------------------------------------------------------------- gather / backward
// a selection outside [0, n) (a caller's stale buffer) is clamped, so no address leaves the image
__device__ __forceinline__ int ss_sel(const int* __restrict__ sel, int idx, int n) { return min(max(sel[idx], 0), n - 1); }

// one workgroup per 256-column chunk of one crop row
__global__ __launch_bounds__(256) void ss_gather_k(const float* __restrict__ target, const int* __restrict__ sel, int C, int H, int W,
                                                   int n, int d, int ch, int cw, int chunks, float* __restrict__ dst) {
    const int chunk = blockIdx.x % chunks, row = blockIdx.x / chunks;
    const int y = row % ch, plane = row / ch, b = plane / C;
    const int x = chunk * 256 + threadIdx.x;
    if (x >= cw) return;
    const int ry = ss_sel(sel, 2 * b, n) * d, rx = ss_sel(sel, 2 * b + 1, n) * d;
    dst[((size_t)plane * ch + y) * cw + x] = target[((size_t)plane * H + ry + y) * W + rx + x];
}

extern "C" int srcgan_shift_gather(const float* target, const int* sel, int B, int C, int H, int W, int shift, int stride, int crop_h,
                                   int crop_w, float* dst, void* stream) {
    SG_REQUIRE(target && sel && dst, "srcgan_shift_gather: null pointer");
    SsPlan p;
    SG_TRY(ss_plan("srcgan_shift_gather", B, C, H, W, shift, stride, crop_h, crop_w, p));
    const int chunks = cdiv(crop_w, 256);
    const long blocks = (long)B * C * crop_h * chunks;
    SG_REQUIRE(blocks <= 0x7fffffffL, "srcgan_shift_gather: too many rows (%ld blocks)", blocks);
    hipLaunchKernelGGL(ss_gather_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, target, sel, C, H, W, p.n, stride, crop_h,
                       crop_w, chunks, dst);
    SG_LAUNCH_CHECK();
    return 0;
}

__device__ __forceinline__ float ss_sign(float a, float b) { const float v = a - b; return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// one workgroup per 256-column chunk of one full-size row; every element of doutput (and dtarget) is written exactly once
__global__ __launch_bounds__(256) void ss_l1_bwd_k(const float* __restrict__ output, const float* __restrict__ target,
                                                   const int* __restrict__ sel, int C, int H, int W, int n, int sd, int d, int ch, int cw,
                                                   int chunks, const float* __restrict__ gout, float gs, float* __restrict__ doutput,
                                                   float* __restrict__ dtarget) {
    const int chunk = blockIdx.x % chunks, row = blockIdx.x / chunks;
    const int y = row % H, plane = row / H, b = plane / C;
    const int x = chunk * 256 + threadIdx.x;
    if (x >= W) return;
    const float g = gout[0] * gs;                // upstream gradient * 1/N
    const int ry = ss_sel(sel, 2 * b, n) * d, rx = ss_sel(sel, 2 * b + 1, n) * d;
    const size_t base = (size_t)plane * H * W, e = base + (size_t)y * W + x;
    const int cy = y - sd, cx = x - sd;          // crop coordinates of this prediction pixel
    float v = 0.f;
    if (cy >= 0 && cy < ch && cx >= 0 && cx < cw) v = ss_sign(output[e], target[base + (size_t)(cy + ry) * W + cx + rx]) * g;
    doutput[e] = v;
    if (dtarget) {
        const int wy = y - ry, wx = x - rx;      // crop coordinates of this target pixel inside the selected window
        float u = 0.f;
        if (wy >= 0 && wy < ch && wx >= 0 && wx < cw) u = ss_sign(output[base + (size_t)(wy + sd) * W + wx + sd], target[e]) * -g;
        dtarget[e] = u;
    }
}

extern "C" int srcgan_shift_l1_bwd(const float* output, const float* target, const int* sel, int B, int C, int H, int W, int shift,
                                   int stride, int crop_h, int crop_w, const float* gout, float* doutput, float* dtarget, void* stream) {
    SG_REQUIRE(output && target && sel && gout && doutput, "srcgan_shift_l1_bwd: null pointer");
    SsPlan p;
    SG_TRY(ss_plan("srcgan_shift_l1_bwd", B, C, H, W, shift, stride, crop_h, crop_w, p));
    const int chunks = cdiv(W, 256);
    const long blocks = (long)B * C * H * chunks;
    SG_REQUIRE(blocks <= 0x7fffffffL, "srcgan_shift_l1_bwd: too many rows (%ld blocks)", blocks);
    const long N = (long)B * C * crop_h * crop_w;
    hipLaunchKernelGGL(ss_l1_bwd_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, output, target, sel, C, H, W, p.n,
                       shift * stride, stride, crop_h, crop_w, chunks, gout, 1.0f / (float)N, doutput, dtarget);
    SG_LAUNCH_CHECK();
    return 0;
}
