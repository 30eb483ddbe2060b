// Whole-scene inference plumbing (srcgan_amd/infer.py): a scene too large for one forward stays on the device, tiles of one common
// shape are gathered with a halo into an NCHW f32 batch, and the network's HR tiles are written back by crop or by a feathered blend.
// Three memory-bound copies; no arithmetic intensity to speak of, so the only levers are coalescing and access width:
//   * consecutive threads take consecutive 4-pixel units of one row, a unit is one 16-byte load / store where the row start, the row
//     pitch and the base pointer are 16-byte aligned, and four scalar accesses otherwise (same values either way: these are copies);
//   * tile origins / write-back rectangles travel in the kernel arguments (no device allocation, no host-to-device copy per launch);
//     a launch carries SG_GATHER_CHUNK / SG_SCATTER_CHUNK tiles and the entry points chunk above that;
//   * no atomics: crop rectangles are disjoint, and the feathered blend adds one tile per launch, so the additions to a pixel happen
//     in tile order on the stream and the result is the same bits run after run.
// There is ONE gather, tile_gather_k<VEC, KIND, UP>, behind both srcgan_tile_gather (kind from the dtype, s = 1) and
// srcgan_tile_gather_ex: it converts (KIND: f32 as is, u8 -> v / 255, u8 RGB -> gray) and, with UP, up-samples (bilinear x s) the
// scene while it gathers, with pixel_ops.h's per-sample functions, and is thereby bit-identical to gathering from the materialised
// scene -- so the cascade driver (infer.py cascade_scene) never makes an f32 scene.  Its other fused form, srcgan_tile_scatter_u8,
// converts the network's tiles (RGB planes, or L + ab planes) to 8-bit RGB while it writes their cores back; it shares the
// rectangle checks and the argument chunking with srcgan_tile_scatter, not the kernel.
// The geometric self-ensemble (infer.py, ensemble=) adds the eight D4 views of a window: srcgan_tile_gather_d4 gathers a view directly
// (mirrors inside tile_gather_k, transpositions in tile_gather_t_k) and srcgan_d4_accumulate folds a network output back to the
// identity orientation into an f32 accumulator.  Transpositions stage 32 x 32 blocks through LDS (transpose_block), so that both
// sides of global memory are still walked along W.
#include "common.h"
#include "pixel_ops.h"

namespace {
constexpr int SG_GATHER_CHUNK = 128;        // 128 x 8 B  = 1 KiB of kernel arguments
constexpr int SG_SCATTER_CHUNK = 64;        // 64 x 40 B = 2.5 KiB (the limit is 4 KiB)
constexpr int SG_TILE_MAX_SIDE = 16384;     // per-tile extent (LR for gather, HR for scatter): grid.x stays far below 2^31

struct GatherArgs { int yx[SG_GATHER_CHUNK][2]; };
// One HR write-back rectangle ("support") per tile, in LR pixels: the core widened by half a ramp on every blended side.
// ny_lo / ny_hi / nx_lo / nx_hi: ramp lengths in LR pixels at the low / high end of the support (0 = no ramp on that side).
struct ScatterTile { int y0, x0, sy0, sy1, sx0, sx1, ny_lo, ny_hi, nx_lo, nx_hi; };
struct ScatterArgs { ScatterTile t[SG_SCATTER_CHUNK]; };

// One sample of the CONVERTED scene at (c, y, x), 0 <= y < H, 0 <= x < W.  KIND 0: f32 planes; 1: u8 HWC, v / 255; 2: u8 RGB -> gray.
template <int KIND>
__device__ __forceinline__ float scene_at(const void* __restrict__ src, int C, int H, int W, int c, int y, int x) {
    if constexpr (KIND == 0) {
        return ((const float*)src)[((size_t)c * H + y) * W + x];
    } else {
        const unsigned char* p = (const unsigned char*)src + ((size_t)y * W + x) * C;
        if constexpr (KIND == 1) return sg_u8_unit(p[c]);
        else return sg_gray_u8(p[0], p[1], p[2]);
    }
}

// dst[t][c][ty][tx] = U(c, min(y0 + wy, OH - 1), min(x0 + wx, OW - 1)), U = the converted scene (UP: up-sampled x s, s > 1, OH x OW =
// H s x W s; else s is unused and OH x OW = H x W), evaluated per sample: every tap is an in-scene read.  (wy, wx) = (ty, tx), or with
// `flip` bit 0 / bit 1 the mirrored row th - 1 - ty / column tw - 1 - tx of the window (the D4 views without a transposition): a
// mirrored unit is read forwards, as the segment it mirrors, and stored reversed.  VEC = 4: tw % 4 == 0 and dst 16-byte aligned
// (host-checked); a unit of f32 planes taken as they are is one 16-byte load where `src_vec_ok` (row pitch and base aligned) and the
// unit is aligned and inside the row -- the same values either way.
// grid: x = units of one (tile, channel) plane, y = channel (f32) or 1 (u8: a thread writes all planes of its pixels), z = tile.
template <int VEC, int KIND, bool UP>
__global__ __launch_bounds__(256) void tile_gather_k(const void* __restrict__ src, float* __restrict__ dst, int C, int H, int W, int s,
                                                     int th, int tw, int src_vec_ok, int flip, GatherArgs a) {
    const int upr = tw / VEC;                                   // units per row
    const long unit = (long)blockIdx.x * 256 + threadIdx.x;
    if (unit >= (long)th * upr) return;
    const int ty = (int)(unit / upr), tx = (int)(unit - (long)ty * upr) * VEC;
    const bool fx = flip & 2;
    const int wy = (flip & 1) ? th - 1 - ty : ty, wx = fx ? tw - VEC - tx : tx;    // window row; first window column of the unit
    const int y0 = a.yx[blockIdx.z][0], x0 = a.yx[blockIdx.z][1];
    const int OH = UP ? H * s : H, OW = UP ? W * s : W;
    const int oy = min(y0 + wy, OH - 1);
    SgLerp ly{}, lx[VEC]{};                                     // UP: the row's and the VEC columns' positions, once for all planes
    if constexpr (UP) {
        ly = sg_bilinear_axis(oy, H, s);
#pragma unroll
        for (int i = 0; i < VEC; ++i) lx[i] = sg_bilinear_axis(min(x0 + wx + i, OW - 1), W, s);
    }
    const int Cd = KIND == 2 ? 1 : C;                           // planes written
    const int c_lo = KIND == 0 ? (int)blockIdx.y : 0, c_hi = KIND == 0 ? c_lo + 1 : Cd;
    const size_t plane = (size_t)th * tw;
    float* d = dst + (size_t)blockIdx.z * Cd * plane + (size_t)ty * tw + tx;
    for (int c = c_lo; c < c_hi; ++c) {
        float v[VEC];
        bool wide = false;
        if constexpr (KIND == 0 && !UP && VEC == 4) {
            wide = src_vec_ok && !((x0 + wx) & 3) && x0 + wx + 3 < W;
            if (wide) load4<float>((const float*)src + ((size_t)c * H + oy) * W + x0 + wx, v);
        }
        if (!wide) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const int ox = min(x0 + wx + i, OW - 1);
                if constexpr (UP) v[i] = sg_bilinear_sample([&](int y, int x) { return scene_at<KIND>(src, C, H, W, c, y, x); }, ly, lx[i]);
                else v[i] = scene_at<KIND>(src, C, H, W, c, oy, ox);
            }
        }
        if constexpr (VEC == 4) {
            if (fx) { const float w[4] = {v[3], v[2], v[1], v[0]}; store4<float>(d + c * plane, w); }
            else store4<float>(d + c * plane, v);
        } else {
            d[c * plane] = v[0];
        }
    }
}

// ---- the transposing kernels (the D4 views with bit 0 of `op` set) ----
// A transposed copy read and written naively has one side striding through memory; instead a workgroup stages one SG_TR x SG_TR
// block through LDS: `load(r, c, v)` fetches elements (r, c .. c + VEC - 1) of the source block, rows along the source's fast axis,
// and `store(r, c, v)` receives elements (r, c .. c + VEC - 1) of the DESTINATION block, element (r, c) of it being element (c, r)
// of the source block -- both sides of global memory are walked along W.  Bounds are the callbacks' business.
// The LDS pitch is SG_TR + 1 dwords.  All accesses are 4-byte ones (banks = dword address mod 32, conflicts within a 32-lane half).
// VEC 1: a half writes one row (33 r + c, c = 0..31) and reads one column (33 c + r == c + r): 32 distinct banks each.  VEC 4: a half
// covers 4 rows x 8 units; element i of every unit goes to 33 r + 4 q + i == (r + 4 q) + i with r in a run of 4 and 4 q a multiple of
// 4 -- distinct -- and comes back from 33 (4 q + i) + r == (4 q + r) + i: distinct again.  A pitch of 32 would make the column side
// a 32-way conflict.
constexpr int SG_TR = 32;

template <int VEC, typename Load, typename Store>
__device__ __forceinline__ void transpose_block(Load load, Store store) {
    __shared__ float lds[SG_TR][SG_TR + 1];
    constexpr int UPR = SG_TR / VEC, PASS = 256 / UPR;          // units per block row; block rows per pass of the 256 threads
    const int r = threadIdx.x / UPR, c = (threadIdx.x % UPR) * VEC;
#pragma unroll
    for (int k = 0; k < SG_TR; k += PASS) {
        float v[VEC];
        load(r + k, c, v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) lds[r + k][c + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SG_TR; k += PASS) {
        float v[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = lds[c + i][r + k];
        store(r + k, c, v);
    }
}

// Elements x .. x + VEC - 1 of a row `p` of `n`, or with `mirror` elements n - 1 - x .. n - 1 - x - (VEC - 1) in that order: the
// mirrored segment is one forward access, reversed in registers.  VEC 4: n % 4 == 0, x % 4 == 0 and p 16-byte aligned.
template <int VEC>
__device__ __forceinline__ void load_row(const float* p, int n, int x, bool mirror, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        float w[4];
        load4<float>(p + (mirror ? n - 4 - x : x), w);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = mirror ? w[3 - i] : w[i];
    } else {
        v[0] = p[mirror ? n - 1 - x : x];
    }
}
template <int VEC>
__device__ __forceinline__ void store_row(float* p, int n, int x, bool mirror, const float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float w[4] = {mirror ? v[3] : v[0], mirror ? v[2] : v[1], mirror ? v[1] : v[2], mirror ? v[0] : v[3]};
        store4<float>(p + (mirror ? n - 4 - x : x), w);
    } else {
        p[mirror ? n - 1 - x : x] = v[0];
    }
}

// The transposed views of the gather: dst[t][c] is [tw][th], dst[t][c][y][x] = window[x'][y'], y' = (flip & 1) ? tw - 1 - y : y,
// x' = (flip & 2) ? th - 1 - x : x, the window being what tile_gather_k<.., flip = 0> writes, sample for sample (the same per-sample
// functions; the bilinear positions are recomputed per sample, which changes no bit).  The source block is a block of the WINDOW
// (rows = scene rows), so scene reads run along W; the destination block is a block of the view.  VEC = 4 (th % 4 == 0, tw % 4 == 0,
// dst 16-byte aligned; host-checked): a unit lies inside or outside the window as a whole and is stored as 16 bytes.
// grid: x = blocks of the window (row-major), y = plane written, z = tile.
template <int VEC, int KIND, bool UP>
__global__ __launch_bounds__(256) void tile_gather_t_k(const void* __restrict__ src, float* __restrict__ dst, int C, int H, int W, int s,
                                                       int th, int tw, int flip, GatherArgs a) {
    const int nbb = cdiv(tw, SG_TR);
    const int a0 = (int)(blockIdx.x / nbb) * SG_TR, b0 = (int)(blockIdx.x % nbb) * SG_TR;       // the block's origin in the window
    const int y0 = a.yx[blockIdx.z][0], x0 = a.yx[blockIdx.z][1];
    const int OH = UP ? H * s : H, OW = UP ? W * s : W;
    const int c = blockIdx.y;
    float* d = dst + ((size_t)blockIdx.z * gridDim.y + c) * th * tw;
    transpose_block<VEC>(
        [&](int r, int cc, float (&v)[VEC]) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const int wa = a0 + r, wb = b0 + cc + i;
                v[i] = 0.0f;
                if (wa >= th || wb >= tw) continue;
                const int oy = min(y0 + wa, OH - 1), ox = min(x0 + wb, OW - 1);
                if constexpr (UP)
                    v[i] = sg_bilinear_sample([&](int y, int x) { return scene_at<KIND>(src, C, H, W, c, y, x); }, sg_bilinear_axis(oy, H, s),
                                              sg_bilinear_axis(ox, W, s));
                else v[i] = scene_at<KIND>(src, C, H, W, c, oy, ox);
            }
        },
        [&](int r, int cc, const float (&v)[VEC]) {
            const int wb = b0 + r, wa = a0 + cc;                // view row <-> window column; view columns <-> window rows wa ..
            if (wb >= tw || wa >= th) return;
            store_row<VEC>(d + (size_t)((flip & 1) ? tw - 1 - wb : wb) * th, th, wa, flip & 2, v);
        });
}

// acc[a][b] = ((first ? 0 : acc[a][b]) + view[y][x]) * scale: one addition and one multiplication, each rounded (contraction is
// off here, so no surrounding code can turn the pair into something else); `first` does not read acc at all.
__device__ __forceinline__ float d4_fold(float acc, float v, float scale) {
#pragma clang fp contract(off)
    const float sum = acc + v;
    return sum * scale;
}
template <int VEC>
__device__ __forceinline__ void d4_fold_row(float* p, const float (&v)[VEC], int first, float scale) {
    float o[VEC] = {};
    if (!first) load_row<VEC>(p, 0, 0, false, o);
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = d4_fold(o[i], v[i], scale);
    store_row<VEC>(p, 0, 0, false, o);
}

// The fold of an untransposed view ([ah][aw], like acc): y = (flip & 1) ? ah - 1 - a : a, x = (flip & 2) ? aw - 1 - b : b.
// VEC = 4: aw % 4 == 0 and both pointers 16-byte aligned.  grid: x = units of a plane, y = plane.
template <int VEC>
__global__ __launch_bounds__(256) void d4_accumulate_k(const float* __restrict__ view, float* __restrict__ acc, int ah, int aw, int flip,
                                                       int first, float scale) {
    const int upr = aw / VEC;
    const long unit = (long)blockIdx.x * 256 + threadIdx.x;
    if (unit >= (long)ah * upr) return;
    const int ya = (int)(unit / upr), xb = (int)(unit - (long)ya * upr) * VEC;
    const size_t plane = (size_t)ah * aw;
    float v[VEC];
    load_row<VEC>(view + blockIdx.y * plane + (size_t)((flip & 1) ? ah - 1 - ya : ya) * aw, aw, xb, flip & 2, v);
    d4_fold_row<VEC>(acc + blockIdx.y * plane + (size_t)ya * aw + xb, v, first, scale);
}

// The fold of a transposed view ([aw][ah]): acc[a][b] takes view[y][x], y = (flip & 1) ? aw - 1 - b : b, x = (flip & 2) ? ah - 1 - a : a.
// The source block is a block of the view (its rows <-> b, its columns <-> a), the destination block the block (a0, b0) of acc.
// VEC = 4: ah % 4 == 0, aw % 4 == 0 and both pointers 16-byte aligned.  grid: x = blocks of acc (row-major), y = plane.
template <int VEC>
__global__ __launch_bounds__(256) void d4_accumulate_t_k(const float* __restrict__ view, float* __restrict__ acc, int ah, int aw, int flip,
                                                         int first, float scale) {
    const int nbb = cdiv(aw, SG_TR);
    const int a0 = (int)(blockIdx.x / nbb) * SG_TR, b0 = (int)(blockIdx.x % nbb) * SG_TR;
    const size_t plane = (size_t)ah * aw;
    const float* v0 = view + blockIdx.y * plane;
    float* d0 = acc + blockIdx.y * plane;
    transpose_block<VEC>(
        [&](int r, int cc, float (&v)[VEC]) {
            const int b = b0 + r, ya = a0 + cc;
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] = 0.0f;
            if (b < aw && ya < ah) load_row<VEC>(v0 + (size_t)((flip & 1) ? aw - 1 - b : b) * ah, ah, ya, flip & 2, v);
        },
        [&](int r, int cc, const float (&v)[VEC]) {
            const int ya = a0 + r, b = b0 + cc;
            if (ya < ah && b < aw) d4_fold_row<VEC>(d0 + (size_t)ya * aw + b, v, first, scale);
        });
}

// ramp weight of HR position j inside a support of n HR pixels: (j + 0.5) / n_lo rising over the first n_lo, 1 - (jj + 0.5) / n_hi
// falling over the last n_hi, 1 between (infer.py TilePlan.axis_weights is the same arithmetic in torch f32)
__device__ __forceinline__ float ramp_w(int j, int n, int n_lo, int n_hi) {
    if (j < n_lo) return ((float)j + 0.5f) / (float)n_lo;
    const int jj = j - (n - n_hi);
    if (jj >= 0) return 1.0f - ((float)jj + 0.5f) / (float)n_hi;
    return 1.0f;
}

// feather == 0: dst = tile on the support.  feather == 1: dst = fma(wy * wx, tile, dst) (ONE tile per launch, see the entry point).
// VEC = 4 is chosen per tile: `vec_ok` (dst pitch / pointers / tile pitch aligned) and the support's HR x-range 4-aligned in both.
__global__ __launch_bounds__(256) void tile_scatter_k(const float* __restrict__ tiles, float* __restrict__ dst, int C, int SH, int SW,
                                                      int TH, int TW, int up, int feather, int vec_ok, ScatterArgs a) {
    const ScatterTile t = a.t[blockIdx.z];
    const int hx0 = t.sx0 * up, hy0 = t.sy0 * up, hw = (t.sx1 - t.sx0) * up, hh = (t.sy1 - t.sy0) * up;
    const int ox = hx0 - t.x0 * up, oy = hy0 - t.y0 * up;                      // support origin inside the HR tile
    const bool vec = vec_ok && !(hx0 & 3) && !(hw & 3) && !(ox & 3);
    const int V = vec ? 4 : 1, upr = hw / V;
    const long unit = (long)blockIdx.x * 256 + threadIdx.x;
    if (unit >= (long)hh * upr) return;
    const int j = (int)(unit / upr), i = (int)(unit - (long)j * upr) * V;
    const int c = blockIdx.y;
    const float* s = tiles + (((size_t)blockIdx.z * C + c) * TH + oy + j) * TW + ox + i;
    float* d = dst + ((size_t)c * SH + hy0 + j) * SW + hx0 + i;
    const float wy = feather ? ramp_w(j, hh, t.ny_lo * up, t.ny_hi * up) : 1.0f;
    if (vec) {
        float v[4];
        load4<float>(s, v);
        if (feather) {
            float o[4];
            load4<float>(d, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = __fmaf_rn(wy * ramp_w(i + k, hw, t.nx_lo * up, t.nx_hi * up), v[k], o[k]);
        }
        store4<float>(d, v);
    } else {
        *d = feather ? __fmaf_rn(wy * ramp_w(i, hw, t.nx_lo * up, t.nx_hi * up), *s, *d) : *s;
    }
}

// dst[px][c] = floor(clamp(src[c][px], 0, 1) * 255).  WORD: hw * C % 4 == 0 and dst 4-byte aligned -- a thread makes one aligned word
// (4 consecutive bytes of the HWC stream; the lanes of a wave read runs of consecutive pixels from each plane); else one byte.
__device__ __forceinline__ unsigned int unit_to_u8(float v) { return (unsigned int)floorf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }

template <bool WORD>
__global__ __launch_bounds__(256) void planes_to_u8hwc_k(const float* __restrict__ src, unsigned char* __restrict__ dst, int C, long hw) {
    const long nunit = WORD ? hw * C / 4 : hw * C;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < nunit; u += (long)gridDim.x * 256) {
        if constexpr (WORD) {
            unsigned int word = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long b = 4 * u + q, px = b / C;
                word |= unit_to_u8(src[(size_t)(b - px * C) * hw + px]) << (8 * q);
            }
            ((unsigned int*)dst)[u] = word;
        } else {
            const long px = u / C;
            dst[u] = (unsigned char)unit_to_u8(src[(size_t)(u - px * C) * hw + px]);
        }
    }
}

// Crop-mode write-back fused with the 8-bit conversion: dst u8 [SH][SW][3].  MODE 0: ta = 3 RGB planes, floor(clamp(v, 0, 1) * 255) as
// planes_to_u8hwc_k.  MODE 1: ta = the L plane, tb = the two chroma planes, sg_lab_to_u8rgb as lab_planes_to_u8rgb_k.
// A thread owns one GROUP: the pixels of one rectangle row whose linear index p = y * SW + x lies in [4 g, 4 g + 4) -- 12 bytes that
// start at byte 12 g, 4-byte aligned whatever SW is.  A group that lies wholly inside the row is stored as three words; a group cut
// by the rectangle's left / right end (its other pixels belong to a neighbouring tile, or to the previous / next scene row) stores
// only its own pixels, byte by byte: nothing outside the rectangle is read or written, so disjoint rectangles never race.
// A row of hw pixels touches at most hw / 4 + 2 groups; that bound sizes the grid and threads past a row's last group exit.
template <int MODE>
__global__ __launch_bounds__(256) void tile_scatter_u8_k(const float* __restrict__ ta, const float* __restrict__ tb, unsigned char* __restrict__ dst,
                                                         int SW, int TH, int TW, int up, int word_ok, ScatterArgs a) {
    const ScatterTile t = a.t[blockIdx.z];
    const int hx0 = t.sx0 * up, hy0 = t.sy0 * up, hw = (t.sx1 - t.sx0) * up, hh = (t.sy1 - t.sy0) * up;
    const int ox = hx0 - t.x0 * up, oy = hy0 - t.y0 * up;                      // rectangle origin inside the HR tile
    const int gpr = hw / 4 + 2;
    const long unit = (long)blockIdx.x * 256 + threadIdx.x;
    if (unit >= (long)hh * gpr) return;
    const int j = (int)(unit / gpr), k = (int)(unit - (long)j * gpr);
    const long p0 = (long)(hy0 + j) * SW + hx0, p1 = p0 + hw;                  // this row of the rectangle, in linear pixel indices
    const long q = ((p0 >> 2) + k) * 4;                                        // first pixel of the group
    if (q >= p1) return;
    const size_t plane = (size_t)TH * TW, row = (size_t)(oy + j) * TW + ox;
    const float* sa = ta + (size_t)blockIdx.z * (MODE == 0 ? 3 : 1) * plane + row;
    const float* sb = MODE == 0 ? nullptr : tb + (size_t)blockIdx.z * 2 * plane + row;
    unsigned int b[4][3];
    bool in[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        in[n] = q + n >= p0 && q + n < p1;
        b[n][0] = b[n][1] = b[n][2] = 0;
        if (!in[n]) continue;
        const long i = q + n - p0;                                             // 0 <= i < hw
        if constexpr (MODE == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) b[n][c] = unit_to_u8(sa[c * plane + i]);
        } else {
            unsigned char rgb[3];
            sg_lab_to_u8rgb(sa[i], sb[i], sb[plane + i], rgb);
#pragma unroll
            for (int c = 0; c < 3; ++c) b[n][c] = rgb[c];
        }
    }
    unsigned char* d = dst + (size_t)q * 3;
    if (word_ok && in[0] && in[3]) {
        unsigned int* w = (unsigned int*)d;
        w[0] = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
        w[1] = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
        w[2] = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
    } else {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (!in[n]) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[3 * n + c] = (unsigned char)b[n][c];
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The gather behind all three entry points: `who` names the caller in the messages.  op: the D4 view of every window (0 = the window
// itself; bit 0 transposes, bit 1 mirrors the view's rows, bit 2 its columns).
int tile_gather(const char* who, const void* src, int src_kind, int C, int H, int W, int s, float* dst, int T, int th, int tw,
                const int* origins_yx, int op, void* stream) {
    SG_REQUIRE(src && dst && origins_yx, "%s: null pointer", who);
    SG_REQUIRE(op >= 0 && op <= 7, "%s: op = %d (0..7: bit 0 transposes, bit 1 mirrors rows, bit 2 mirrors columns)", who, op);
    SG_REQUIRE(src_kind >= 0 && src_kind <= 2, "%s: src_kind = %d (0 f32 planes, 1 u8 HWC, 2 u8 RGB -> gray)", who, src_kind);
    SG_REQUIRE(src_kind == 0 ? (C >= 1 && C <= 8) : src_kind == 1 ? (C == 1 || C == 3) : C == 3,
               "%s: C = %d (f32 planes: 1..8; u8 HWC: 1 or 3; u8 RGB -> gray: 3)", who, C);
    SG_REQUIRE(H > 0 && W > 0 && T > 0 && th > 0 && tw > 0, "%s: bad extents (scene %dx%d, %d tiles of %dx%d)", who, H, W, T, th, tw);
    SG_REQUIRE(s >= 1 && (long)H * s < (1L << 30) && (long)W * s < (1L << 30), "%s: s = %d (must be >= 1, and the up-sampled scene below 2^30 per side)", who, s);
    SG_REQUIRE(th <= SG_TILE_MAX_SIDE && tw <= SG_TILE_MAX_SIDE, "%s: tile %dx%d is larger than the launch limit of %d per side", who, th, tw, SG_TILE_MAX_SIDE);
    const int OH = H * s, OW = W * s;
    for (int t = 0; t < T; ++t)
        SG_REQUIRE(origins_yx[2 * t] >= 0 && origins_yx[2 * t] < OH && origins_yx[2 * t + 1] >= 0 && origins_yx[2 * t + 1] < OW,
                   "%s: origin (%d, %d) of tile %d is outside the %dx%d scene", who, origins_yx[2 * t], origins_yx[2 * t + 1], t, OH, OW);
    const bool transposed = op & 1;
    const int flip = op >> 1;
    const bool vec = (tw % 4 == 0) && (!transposed || th % 4 == 0) && aligned16(dst);
    const int src_vec_ok = src_kind == 0 && (W % 4 == 0) && aligned16(src);
    const int Cd = src_kind == 2 ? 1 : C;
    const size_t per_tile = (size_t)Cd * th * tw;
    using Kernel = decltype(&tile_gather_k<1, 0, false>);
    using KernelT = decltype(&tile_gather_t_k<1, 0, false>);
    static constexpr Kernel kernels[2][3][2] = {                                                // [vec][src_kind][s > 1]
        {{tile_gather_k<1, 0, false>, tile_gather_k<1, 0, true>}, {tile_gather_k<1, 1, false>, tile_gather_k<1, 1, true>},
         {tile_gather_k<1, 2, false>, tile_gather_k<1, 2, true>}},
        {{tile_gather_k<4, 0, false>, tile_gather_k<4, 0, true>}, {tile_gather_k<4, 1, false>, tile_gather_k<4, 1, true>},
         {tile_gather_k<4, 2, false>, tile_gather_k<4, 2, true>}}};
    static constexpr KernelT kernels_t[2][3][2] = {
        {{tile_gather_t_k<1, 0, false>, tile_gather_t_k<1, 0, true>}, {tile_gather_t_k<1, 1, false>, tile_gather_t_k<1, 1, true>},
         {tile_gather_t_k<1, 2, false>, tile_gather_t_k<1, 2, true>}},
        {{tile_gather_t_k<4, 0, false>, tile_gather_t_k<4, 0, true>}, {tile_gather_t_k<4, 1, false>, tile_gather_t_k<4, 1, true>},
         {tile_gather_t_k<4, 2, false>, tile_gather_t_k<4, 2, true>}}};
    for (int t0 = 0; t0 < T; t0 += SG_GATHER_CHUNK) {
        const int n = T - t0 < SG_GATHER_CHUNK ? T - t0 : SG_GATHER_CHUNK;
        GatherArgs a;
        memset(&a, 0, sizeof(a));
        memcpy(a.yx, origins_yx + 2 * t0, sizeof(int) * 2 * n);
        float* d = dst + (size_t)t0 * per_tile;             // per_tile * 4 bytes is a multiple of 16 whenever tw % 4 == 0
        if (transposed) {
            const dim3 grid((unsigned)(cdiv(th, SG_TR) * cdiv(tw, SG_TR)), Cd, n);
            hipLaunchKernelGGL(kernels_t[vec][src_kind][s > 1], grid, dim3(256), 0, (hipStream_t)stream, src, d, C, H, W, s, th, tw, flip, a);
        } else {
            const dim3 grid((unsigned)cdivl((long)th * (vec ? tw / 4 : tw), 256), src_kind == 0 ? C : 1, n);
            hipLaunchKernelGGL(kernels[vec][src_kind][s > 1], grid, dim3(256), 0, (hipStream_t)stream, src, d, C, H, W, s, th, tw, src_vec_ok,
                               flip, a);
        }
        SG_LAUNCH_CHECK();
    }
    return 0;
}

// What both write-backs check alike: the extents, and every 10-int rectangle (`allow_ramps`: the feathered f32 write-back only).
int scatter_check(const char* who, const int* rects, int T, int th, int tw, int H, int W, int up, bool allow_ramps) {
    SG_REQUIRE(up >= 1, "%s: up = %d (must be >= 1)", who, up);
    SG_REQUIRE(H > 0 && W > 0 && T > 0 && th > 0 && tw > 0, "%s: bad extents (scene %dx%d, %d tiles of %dx%d)", who, H, W, T, th, tw);
    SG_REQUIRE((long)th * up <= SG_TILE_MAX_SIDE && (long)tw * up <= SG_TILE_MAX_SIDE && (long)H * up < (1L << 30) && (long)W * up < (1L << 30),
               "%s: HR tile %ldx%ld is larger than the launch limit of %d per side", who, (long)th * up, (long)tw * up, SG_TILE_MAX_SIDE);
    for (int t = 0; t < T; ++t) {
        const int* r = rects + 10 * t;
        const int y0 = r[0], x0 = r[1], sy0 = r[2], sy1 = r[3], sx0 = r[4], sx1 = r[5];
        // the rectangle lies inside the scene AND inside the tile: nothing outside either is ever touched
        SG_REQUIRE(sy0 >= 0 && sy0 < sy1 && sy1 <= H && sx0 >= 0 && sx0 < sx1 && sx1 <= W && sy0 >= y0 && sy1 <= y0 + th && sx0 >= x0 && sx1 <= x0 + tw,
                   "%s: write-back rectangle [%d,%d)x[%d,%d) of tile %d (origin %d,%d, %dx%d) leaves the tile or the %dx%d scene",
                   who, sy0, sy1, sx0, sx1, t, y0, x0, th, tw, H, W);
        SG_REQUIRE(r[6] >= 0 && r[7] >= 0 && r[8] >= 0 && r[9] >= 0 && r[6] + r[7] <= sy1 - sy0 && r[8] + r[9] <= sx1 - sx0,
                   "%s: ramps of tile %d overlap inside its write-back rectangle", who, t);
        SG_REQUIRE(allow_ramps || (r[6] | r[7] | r[8] | r[9]) == 0, "%s: crop mode takes no ramps (tile %d)", who, t);
    }
    return 0;
}

// Rectangles [t0, t0 + n) into the kernel arguments; returns the largest units(hh, hw) over them, hh x hw = a rectangle in HR pixels.
template <typename Units>
long scatter_chunk(ScatterArgs& a, const int* rects, int t0, int n, int up, Units units) {
    memset(&a, 0, sizeof(a));
    long most = 0;
    for (int k = 0; k < n; ++k) {
        const int* r = rects + 10 * (t0 + k);
        a.t[k] = ScatterTile{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]};
        const long u = units((long)(r[3] - r[2]) * up, (long)(r[5] - r[4]) * up);
        if (u > most) most = u;
    }
    return most;
}
}   // namespace

extern "C" int srcgan_tile_gather(const void* src, int src_u8, int C, int H, int W, float* dst, int T, int th, int tw,
                                  const int* origins_yx, void* stream) {
    return tile_gather("srcgan_tile_gather", src, src_u8 ? 1 : 0, C, H, W, 1, dst, T, th, tw, origins_yx, 0, stream);
}

extern "C" int srcgan_tile_gather_ex(const void* src, int src_kind, int C, int H, int W, int s, float* dst, int T, int th, int tw,
                                     const int* origins_yx, void* stream) {
    return tile_gather("srcgan_tile_gather_ex", src, src_kind, C, H, W, s, dst, T, th, tw, origins_yx, 0, stream);
}

extern "C" int srcgan_tile_gather_d4(const void* src, int src_kind, int C, int H, int W, int s, float* dst, int T, int th, int tw,
                                     const int* origins_yx, int op, void* stream) {
    return tile_gather("srcgan_tile_gather_d4", src, src_kind, C, H, W, s, dst, T, th, tw, origins_yx, op, stream);
}

extern "C" int srcgan_d4_accumulate(const float* view, float* acc, long planes, int ah, int aw, int op, int first, float scale,
                                    void* stream) {
    const char* who = "srcgan_d4_accumulate";
    SG_REQUIRE(view && acc, "%s: null pointer", who);
    SG_REQUIRE(op >= 0 && op <= 7, "%s: op = %d (0..7: bit 0 transposes, bit 1 mirrors rows, bit 2 mirrors columns)", who, op);
    SG_REQUIRE(planes > 0 && planes < (1L << 31) && ah > 0 && aw > 0, "%s: bad extents (%ld planes of %dx%d)", who, planes, ah, aw);
    SG_REQUIRE(ah <= SG_TILE_MAX_SIDE && aw <= SG_TILE_MAX_SIDE, "%s: plane %dx%d is larger than the launch limit of %d per side", who, ah, aw, SG_TILE_MAX_SIDE);
    SG_REQUIRE(scale - scale == 0.0f, "%s: scale = %g (must be finite)", who, (double)scale);
    const size_t plane = (size_t)ah * aw;
    const uintptr_t vb = (uintptr_t)view, ab = (uintptr_t)acc, bytes = (uintptr_t)planes * plane * sizeof(float);
    SG_REQUIRE(vb + bytes <= ab || ab + bytes <= vb, "%s: view must not alias acc", who);
    const bool transposed = op & 1;
    const int flip = op >> 1;
    first = first ? 1 : 0;
    const bool vec = (aw % 4 == 0) && (!transposed || ah % 4 == 0) && aligned16(view) && aligned16(acc);
    const unsigned gx = transposed ? (unsigned)(cdiv(ah, SG_TR) * cdiv(aw, SG_TR)) : (unsigned)cdivl((long)ah * (vec ? aw / 4 : aw), 256);
    const auto kernel = transposed ? (vec ? d4_accumulate_t_k<4> : d4_accumulate_t_k<1>) : (vec ? d4_accumulate_k<4> : d4_accumulate_k<1>);
    constexpr long SG_PLANE_CHUNK = 65535;                  // grid.y
    for (long p0 = 0; p0 < planes; p0 += SG_PLANE_CHUNK) {  // plane * 4 bytes is a multiple of 16 whenever aw % 4 == 0
        const long n = planes - p0 < SG_PLANE_CHUNK ? planes - p0 : SG_PLANE_CHUNK;
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, view + p0 * plane, acc + p0 * plane, ah, aw, flip,
                           first, scale);
        SG_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int srcgan_tile_scatter(const float* tiles, float* dst, int C, int H, int W, int up, int T, int th, int tw,
                                   const int* rects, int feather, void* stream) {
    const char* who = "srcgan_tile_scatter";
    SG_REQUIRE(tiles && dst && rects, "%s: null pointer", who);
    SG_REQUIRE(C >= 1 && C <= 8, "%s: C = %d (1..8 planes)", who, C);
    feather = feather ? 1 : 0;
    SG_TRY(scatter_check(who, rects, T, th, tw, H, W, up, feather));
    const int SH = H * up, SW = W * up, TH = th * up, TW = tw * up;
    const int vec_ok = (SW % 4 == 0) && (TW % 4 == 0) && aligned16(dst) && aligned16(tiles) && (((size_t)C * TH * TW) % 4 == 0);
    // crop: disjoint rectangles, one launch per chunk.  feather: one tile per launch -- stream order is the order of the additions.
    const int step = feather ? 1 : SG_SCATTER_CHUNK;
    for (int t0 = 0; t0 < T; t0 += step) {
        const int n = T - t0 < step ? T - t0 : step;
        ScatterArgs a;
        const long units = scatter_chunk(a, rects, t0, n, up, [](long hh, long hw) { return hh * hw; });
        const dim3 grid((unsigned)cdivl(units, 256), C, n);              // sized for the scalar path; vector tiles leave threads idle
        hipLaunchKernelGGL(tile_scatter_k, grid, dim3(256), 0, (hipStream_t)stream, tiles + (size_t)t0 * C * TH * TW, dst, C, SH, SW, TH, TW, up,
                           feather, vec_ok, a);
        SG_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int srcgan_planes_to_u8hwc(const float* src, unsigned char* dst, int C, long hw, void* stream) {
    SG_REQUIRE(src && dst, "srcgan_planes_to_u8hwc: null pointer");
    SG_REQUIRE(C >= 1 && C <= 8, "srcgan_planes_to_u8hwc: C = %d (1..8 planes)", C);
    SG_REQUIRE(hw > 0, "srcgan_planes_to_u8hwc: hw = %ld", hw);
    const bool word = ((hw * C) % 4 == 0) && (((uintptr_t)dst & 3) == 0);
    long nb = cdivl(word ? hw * C / 4 : hw * C, 256); if (nb > 16384) nb = 16384;
    if (word) hipLaunchKernelGGL(planes_to_u8hwc_k<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, src, dst, C, hw);
    else hipLaunchKernelGGL(planes_to_u8hwc_k<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, src, dst, C, hw);
    SG_LAUNCH_CHECK();
    return 0;
}

extern "C" int srcgan_tile_scatter_u8(const float* tiles_a, int Ca, const float* tiles_b, int Cb, unsigned char* dst, int H, int W, int up,
                                      int T, int th, int tw, const int* rects, int mode, void* stream) {
    SG_REQUIRE(tiles_a && dst && rects, "srcgan_tile_scatter_u8: null pointer");
    SG_REQUIRE(mode == 0 || mode == 1, "srcgan_tile_scatter_u8: mode = %d (0 RGB planes, 1 L + ab planes)", mode);
    SG_REQUIRE(mode == 0 ? (Ca == 3 && !tiles_b && Cb == 0) : (Ca == 1 && tiles_b && Cb == 2),
               "srcgan_tile_scatter_u8: mode %d takes %s, got Ca = %d, Cb = %d", mode,
               mode == 0 ? "Ca = 3 and no second tensor (tiles_b null, Cb = 0)" : "Ca = 1 (L) and Cb = 2 (ab)", Ca, Cb);
    SG_TRY(scatter_check("srcgan_tile_scatter_u8", rects, T, th, tw, H, W, up, false));
    const int SW = W * up, TH = th * up, TW = tw * up;
    const int word_ok = ((uintptr_t)dst & 3) == 0;
    for (int t0 = 0; t0 < T; t0 += SG_SCATTER_CHUNK) {
        const int n = T - t0 < SG_SCATTER_CHUNK ? T - t0 : SG_SCATTER_CHUNK;
        ScatterArgs a;
        const long units = scatter_chunk(a, rects, t0, n, up, [](long hh, long hw) { return hh * (hw / 4 + 2); });   // rows x groups per row
        const dim3 grid((unsigned)cdivl(units, 256), 1, n);
        const size_t plane = (size_t)TH * TW;
        if (mode == 0)
            hipLaunchKernelGGL(tile_scatter_u8_k<0>, grid, dim3(256), 0, (hipStream_t)stream, tiles_a + (size_t)t0 * 3 * plane, (const float*)nullptr,
                               dst, SW, TH, TW, up, word_ok, a);
        else
            hipLaunchKernelGGL(tile_scatter_u8_k<1>, grid, dim3(256), 0, (hipStream_t)stream, tiles_a + (size_t)t0 * plane, tiles_b + (size_t)t0 * 2 * plane,
                               dst, SW, TH, TW, up, word_ok, a);
        SG_LAUNCH_CHECK();
    }
    return 0;
}
