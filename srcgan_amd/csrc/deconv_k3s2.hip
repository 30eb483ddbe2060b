// ConvTranspose2d(k3, s2, p1, output_padding 1) -- the up-sampler of SRDenseNetA (reference src/model/model.py:698-701) -- with ALL
// FOUR output parities in one launch.
//
//   y[2i + a][2j + b][co] = sum over wy in [0, a], wx in [0, b], ci:  x[i + wy][j + wx][ci] * W[ci][co][ky][kx],
//                           ky = a ? 2 - 2 wy : 1,  kx = b ? 2 - 2 wx : 1          (x reads zero past the lower / right edge)
//
// so the parities (0,0), (0,1), (1,0), (1,1) are 1-, 2-, 2- and 4-tap stride-1 convolutions over the same (TH+1) x 33 input window:
// 9 (parity, tap) products per staged tile, 2.25 taps per output pixel.  The k2 s2 form's four 1x1 parities share nothing but the
// centre pixel; here the window position (wy, wx) serves every parity with a >= wy and b >= wx, and its pixel fragment is read from
// LDS once for all of them (4 fragment reads per k-step for 9 MFMA groups).
//   GEMM orientation as conv_igemm.hip: D[M = 32 output channels][N = 32 positions j] per parity; a wave owns PT rows i.
//   LDS: window (80 B per pixel: conflict-free ds_read_b128 of 32 consecutive pixels) + 9 x 32 weight rows of the K chunk.
//   Weights: pack q = a * 2 + b at wp + q * wpar bytes, Wp[row tile][chunk][tap wy * (b + 1) + wx][row][k] (srcgan_pack_weight with
//   tys = a + 1, txs = b + 1); LDS slot of (q, tap) = {0, 1, 3, 5}[q] + tap.
#include "conv_epilogue.h"
#include "launch.h"
#include <type_traits>

template <typename T, int PT>
__global__ __launch_bounds__(256, 2) void deconv_k3s2_k(const ConvP p) {
    using D = DT<T>;
    constexpr int TH = 4 * PT, TW = 32, IHT = TH + 1, IWT = TW + 1;
    constexpr int COT = 32, PIXB = 80, NPAR = 4, NSLOT = 9, WROWS = NSLOT * COT;
    constexpr int NPH = IHT * IWT * 4, NPW = WROWS * 4;              // 16-byte pieces of the window / of a chunk's weights
    constexpr int HIT = (NPH + 255) / 256, WIT = (NPW + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds_h = smem;
    char* lds_w = smem + IHT * IWT * PIXB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    int L;
    {   // XCD-aware block -> tile map (conv_igemm.hip): the channel tiles of a spatial tile and neighbouring tiles share an L2
        const int nblk = gridDim.x, bid = blockIdx.x, xcd = bid & 7, q8 = nblk >> 3, r8 = nblk & 7;
        L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    }
    const int ct = L % p.ctiles;
    int t = L / p.ctiles;
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y;
    const int b = t / p.tiles_y;
    const int t0 = ty * TH, u0 = tx * TW;            // first (i, j) of the tile = the window's origin in x

    f32x16 acc[NPAR][1][PT];
#pragma unroll
    for (int q = 0; q < NPAR; ++q)
#pragma unroll
        for (int k = 0; k < PT; ++k)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[q][0][k][i] = 0.f;

    const char* xb = (const char*)p.x + (size_t)b * p.H * p.W * p.xpix + (size_t)p.xcoff * sizeof(T);
    // row tiles of the packs: 64 rows (32 if the layer has <= 32 output channels)
    const int cotp = p.Cout <= 32 ? 32 : 64, rt = (ct * COT) / cotp, roff = (ct * COT) % cotp;
    const int part = tid & 3;
    int h_goff[HIT];
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int pc = it * 256 + tid, pix = pc >> 2;
        const int iy = pix / IWT, ix = pix - iy * IWT;
        const int gy = t0 + iy, gx = u0 + ix;
        const bool ok = pc < NPH && gy < p.H && gx < p.W;
        h_goff[it] = ok ? ((gy * p.W + gx) * (int)p.xpix + part * 16) : -1;
    }
    // weight piece `it` of this thread: LDS row (it * 256 + tid) >> 2 = slot * 32 + rr.  Its source: pack q of the slot, chunk c, tap
    long w_off[WIT]; int w_step[WIT];                 // byte offset for chunk 0 / bytes per chunk
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
        int slot = (it * 256 + tid) >> 7;
        if (slot > NSLOT - 1) slot = NSLOT - 1;          // the last pass has 128 pieces: the other threads load a valid piece and drop it
        const int q = slot == 0 ? 0 : slot < 3 ? 1 : slot < 5 ? 2 : 3;
        const int ntap = ((q >> 1) + 1) * ((q & 1) + 1), tap = slot - (q == 0 ? 0 : q == 1 ? 1 : q == 2 ? 3 : 5);
        w_step[it] = ntap * cotp * 64;
        w_off[it] = (long)q * p.wpar + ((long)rt * p.nchunk * ntap + tap) * cotp * 64 + (long)(roff + ((tid >> 2) & 31)) * 64 + part * 16;
    }
    u32x4 hreg[HIT], wreg[WIT];
    auto issue = [&](int c) {
        const bool cok = c * D::KCE + part * D::EPP < p.Cin;
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int off = (h_goff[it] >= 0 && cok) ? h_goff[it] + c * 64 : 0;
            hreg[it] = *(const u32x4*)(xb + off);
        }
#pragma unroll
        for (int it = 0; it < WIT; ++it) wreg[it] = *(const u32x4*)((const char*)p.wp + w_off[it] + (long)c * w_step[it]);
    };
    auto stage = [&](int c) {
        const bool cok = c * D::KCE + part * D::EPP < p.Cin;
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int pc = it * 256 + tid;
            u32x4 v = hreg[it];
            if (!(h_goff[it] >= 0 && cok)) v = u32x4{0u, 0u, 0u, 0u};
            if (HIT * 256 == NPH || pc < NPH) *(u32x4*)(lds_h + (pc >> 2) * PIXB + part * 16) = v;
        }
#pragma unroll
        for (int it = 0; it < WIT; ++it) {
            const int pc = it * 256 + tid;
            if (WIT * 256 == NPW || pc < NPW) *(u32x4*)(lds_w + (pc >> 2) * PIXB + part * 16) = wreg[it];
        }
    };

    using frag_t = typename std::conditional<std::is_same<T, float>::value, f32x4, bf16x8>::type;
    issue(0);
    for (int c = 0; c < p.nchunk; ++c) {
        stage(c);                               // the previous chunk's readers passed the barrier at the end of the last iteration
        __syncthreads();
        if (c + 1 < p.nchunk) issue(c + 1);     // in flight while this chunk's MFMAs run
#pragma unroll
        for (int wy = 0; wy < 2; ++wy)
#pragma unroll
            for (int wx = 0; wx < 2; ++wx)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int koff = ks * 32 + h * 16;
                    frag_t bb[PT];
#pragma unroll
                    for (int q = 0; q < PT; ++q)
                        bb[q] = *(const frag_t*)(lds_h + ((wave * PT + q + wy) * IWT + r + wx) * PIXB + koff);
#pragma unroll
                    for (int par = 0; par < NPAR; ++par) {
                        const int pa = par >> 1, pb = par & 1;
                        if (wy > pa || wx > pb) continue;          // this window position is no tap of parity (pa, pb)
                        const int slot = (par == 0 ? 0 : par == 1 ? 1 : par == 2 ? 3 : 5) + wy * (pb + 1) + wx;
                        const frag_t a = *(const frag_t*)(lds_w + (slot * COT + r) * PIXB + koff);
#pragma unroll
                        for (int q = 0; q < PT; ++q) {
                            if constexpr (std::is_same<T, float>::value) {
#pragma unroll
                                for (int j = 0; j < 4; ++j)
                                    acc[par][0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bb[q][j], acc[par][0][q], 0, 0, 0);
                            } else
                                acc[par][0][q] = sg_mfma16<T>(a, bb[q], acc[par][0][q]);
                        }
                    }
                }
        __syncthreads();                        // all waves are done reading this chunk's LDS image
    }

    // ---- epilogue: parity (a, b) -> y[2i + a][2j + b], bias + activation fused (every parity covers all H x W positions)
    constexpr int RS = COT * 4 + 16;
    char* lw = smem + wave * 32 * RS;
#pragma unroll
    for (int par = 0; par < NPAR; ++par) {
        ConvP pq = p;
        pq.os = 2; pq.oa = par >> 1; pq.ob = par & 1;
#pragma unroll
        for (int q = 0; q < PT; ++q) conv_epilogue_lds_row<T, 1, PT>(pq, acc[par], q, lw, b, ct, t0 + wave * PT + q, u0, lane);
    }
}

template <typename T, int PT>
static int launch_deconv_k3s2(const ConvP& p, hipStream_t st) {
    constexpr int TH = 4 * PT, IHT = TH + 1, IWT = 33;
    constexpr size_t STAGE = (size_t)IHT * IWT * 80 + (size_t)9 * 32 * 80, EPI = (size_t)4 * 32 * (32 * 4 + 16);
    constexpr size_t SMEM = STAGE > EPI ? STAGE : EPI;
    // only the LDS-transposed epilogue is instantiated (the per-element form spills beside the 128 accumulator registers)
    SG_REQUIRE(p.buf16, "srcgan_conv_igemm: the transposed 3x3 stride-2 form needs output channels, strides and offsets that are multiples of 16 bytes");
    constexpr auto kern = deconv_k3s2_k<T, PT>;
    int dev = 0;
    SG_TRY(sg_current_device(dev));
    SG_TRY(sg_allow_lds<kern>(SMEM, dev));
    ConvP q = p;
    q.tiles_x = cdiv(p.W, 32);
    q.tiles_y = cdiv(p.H, TH);
    q.ctiles = cdiv(p.Cout, 32);
    dim3 grid((unsigned)((size_t)q.tiles_x * q.tiles_y * p.B * q.ctiles), 1, 1);
    char cls[96];
    snprintf(cls, sizeof(cls), "deconv_k3s2<%s,4 parities>", sg_dtype_tag<T>());
    const double px = (double)p.B * p.H * p.W;
    const int tok = sg_prof_start(cls, 2.0 * px * 9 * p.Cin * p.Cout, (px * p.Cin + 4 * px * p.Cout) * sizeof(T), st);
    hipLaunchKernelGGL(kern, grid, dim3(256), SMEM, st, q);
    sg_prof_stop(tok, st);
    SG_LAUNCH_CHECK();
    return 0;
}

// entry used by srcgan_conv_igemm for descriptors with npar == 4, kh == kw == 3, stride == 2
int sg_deconv_k3s2(const ConvP& p, int dtype, hipStream_t st) {
    return sg_dtype_dispatch(dtype, [&](auto t) { return launch_deconv_k3s2<decltype(t), 2>(p, st); });
}
