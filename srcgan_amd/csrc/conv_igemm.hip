// Implicit-GEMM convolution for gfx950 (MI355X): NHWC, halo tile staged once in LDS and
// reused by every filter tap, MFMA contraction over (tap, channel-chunk), fused epilogue
// (bias, scale, two residuals, LeakyReLU, LeakyReLU' mask, pixel-shuffle store).
//
// Replaces aten::convolution / the dgrad half of aten::convolution_backward behind
//   reference src/model/rddb.py:52-58,63-68 (RDB 3x3 convs + "cat" + 0.2*x5+x),
//   rddb.py:28-38,93-97 (ConvTranspose2d k2 s2 == 4 x [1x1 conv -> strided store]),
//   src/model/model.py:612-634 (PatchGAN 4x4 s2 / s1 convs).
//
// GEMM orientation: D[M = Cout][N = pixels] so that each lane of the 32x32 MFMA result holds
// 4 *consecutive output channels* of one pixel -> 8/16-byte epilogue loads and stores in NHWC.
//   A operand (M x K): packed weights, row = cout, k = cin within the chunk
//   B operand (K x N): LDS halo tile, col = 32 consecutive output pixels of one row
// LDS image: one pixel (or one weight row) = 64 B of channels padded to 80 B -> ds_read_b128
// of 32 consecutive pixels is bank-conflict free (stride 5 slots of 16 B, coprime with 16).
// Both dtypes use the same byte layout: 64 B = 32 bf16 (2 x mfma_32x32x16_bf16 k-steps)
//                                            = 16 f32  (8 x mfma_32x32x2_f32).
//
// Reached through sg_conv_generic (bottom of the file); srcgan_conv_igemm itself is in conv_entry.hip.
#include "conv_epilogue.h"
#include "launch.h"
#include <type_traits>

// Cost-removal switches of this kernel's hot loop (scripts/microbench_generic.py): only in a -DSG_DIAG -DSG_IG_DIAG variant --
// as run-time branches they stop the compiler from hoisting fragment reads over MFMAs, so even other SG_DIAG variants leave them out.
#if defined(SG_DIAG) && defined(SG_IG_DIAG)
#define IG_DBG(p, bit) ((p).dbg & (bit))
#else
#define IG_DBG(p, bit) 0
#endif


// Occupancy: hipcc takes 188 registers for the 64-accumulator forms (2 workgroups per CU).  Capping them at 168 (3 per CU,
// __launch_bounds__(256, 3)) changed neither the kernels' times nor the training step (same-box A/B, round 2).
template <typename T, int KH, int KW, int S, int MT, int PT, bool WPK>
__global__ __launch_bounds__(256) void conv_igemm_k(const ConvP p) {
    using D = DT<T>;
    constexpr int TH = 4 * PT, TW = 32;
    constexpr int IHT = (TH - 1) * S + KH, IWT = (TW - 1) * S + KW;
    constexpr int COT = 32 * MT, NTAP = KH * KW, PIXB = 80;
    constexpr int WROWS = (WPK ? KW : NTAP) * COT;
    constexpr int NPH = IHT * IWT * 4;     // 16-byte pieces of the halo tile
    constexpr int NPW = WROWS * 4;         // 16-byte pieces of one weight stage
    constexpr int HIT = (NPH + 255) / 256, WIT = (NPW + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds_h = smem;
    char* lds_w = smem + IHT * IWT * PIXB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    // XCD-aware block -> tile map: blocks b, b+8, b+16.. share an XCD (and its L2); give each XCD a contiguous
    // run of tiles so neighbouring tiles' halos and the Cout tiles of one spatial tile hit the same L2.
    int L;
    {
        const int nblk = gridDim.x, bid = blockIdx.x, xcd = bid & 7, q8 = nblk >> 3, r8 = nblk & 7;
        L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    }
    // npar == 4 (ConvTranspose2d k2 s2 as four 1x1 convolutions, rddb.py:28-38, in ONE launch): the ctiles channel tiles are
    // (parity, tile within the parity); the four parities of a spatial tile are consecutive blocks of one XCD, so the input
    // tile comes from HBM once and from that L2 three times (four launches read the input four times)
    // npar == 2 (16-bit, 64 channels): a 128-row tile = both COLUMN parities of an output pixel pair, the channel-tile index is
    // the ROW parity; a lane group then writes 256 contiguous bytes and a workgroup whole 8-KiB row segments -- the four-parity
    // form's 128-byte records 256 bytes apart ran at 2.5 TB/s where the same kernel writing contiguously reaches 4.3
    int ct = L % p.ctiles, par = 0;
    if (p.npar) { const int cpp = p.ctiles / p.npar; par = ct / cpp; ct -= par * cpp; }
    int t = L / p.ctiles;
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y;
    const int b = t / p.tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int gy0 = oy0 * S - p.pad_y, gx0 = ox0 * S - p.pad_x;

    f32x16 acc[MT][PT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < PT; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][q][i] = 0.f;

    const char* xb = (const char*)p.x + (size_t)b * p.H * p.W * p.xpix + (size_t)p.xcoff * sizeof(T);
    const char* wb = (const char*)p.wp + (size_t)par * p.wpar + (size_t)ct * p.nchunk * NTAP * COT * 64;

    // ---- per-thread staging descriptors (independent of the channel chunk).  Loads are issued
    // unconditionally from a clamped address and zeroed by a select afterwards: no branches, so the
    // compiler keeps all of a stage's loads in flight together.
    // (Round 3, measured: for stride 2 the 32 lanes of a pixel-fragment read are 160 bytes apart -- 8 distinct 16-byte slots, a 2-way
    //  bank conflict, SQ_LDS_BANK_CONFLICT 104 k cycles/us on the 4x4 stride-2 layers.  Keeping the even halo columns of a row in
    //  front of the odd ones makes those reads consecutive and conflict-free; the layers' time did not move (0.841 -> 0.843 ms per
    //  discriminator pass, same-box A/B): with 2 chunks x 16 MFMAs between barrier pairs they are bound by the per-tile prologue
    //  and the barrier chain, not by LDS reads.  Not kept.)
    int h_goff[HIT];                  // byte offset of this thread's halo piece in image b (chunk 0), -1 = outside
    const int part = tid & 3;
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int pc = it * 256 + tid, pix = pc >> 2;
        const int iy = pix / IWT, ix = pix - iy * IWT;
        const int gy = gy0 + iy, gx = gx0 + ix;
        const bool ok = pc < NPH && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
        h_goff[it] = ok ? ((gy * p.W + gx) * (int)p.xpix + part * 16) : -1;
    }
    // Two register stages (NRS == 2, kernels with few taps): the loads of chunk c + 2 are issued while chunk c computes.  With one
    // stage a chunk's loads have only that chunk's MFMA phase to land in -- 32 MFMAs per wave for a 2x2 kernel, ~1000 cycles
    // against 1500-2500 of load latency -- and the stride-2 parity gradients ran at 0.4 PFLOP/s (4x4 s1, 128 MFMAs: 1.05).
    // (measured on the stride-2 parity gradients, 2x2 taps: 1.445 -> 1.408 ms per discriminator pass with NRS = 2 -- the loads'
    //  latency is not what bounds them.  Each parity launch moves ~445 MB for 69 GFLOP (154 FLOP/B): they are close to memory-
    //  bound as four separate launches; one kernel producing all four parities from one staged dy tile would need a third of the
    //  traffic -- DESIGN.md section 8.)  Kept switchable; the default is one stage (36 fewer VGPRs).
    constexpr int NRS = 1;
    u32x4 hreg[NRS][HIT];
    u32x4 wreg[NRS][WPK ? 1 : WIT];
    auto issue_halo = [&](int c, auto rs) {
        constexpr int R = decltype(rs)::value;
        const bool cok = c * D::KCE + part * D::EPP < p.Cin;
        if (IG_DBG(p, 2) && c > 0) return;            // diagnostic builds: operand traffic of the first chunk only
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int off = (h_goff[it] >= 0 && cok) ? h_goff[it] + c * 64 : 0;
            hreg[R][it] = *(const u32x4*)(xb + off);
        }
    };
    auto write_halo = [&](int c, auto rs) {
        constexpr int R = decltype(rs)::value;
        const bool cok = c * D::KCE + part * D::EPP < p.Cin;
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int pc = it * 256 + tid;
            u32x4 v = hreg[R][it];
            if (!(h_goff[it] >= 0 && cok)) v = u32x4{0u, 0u, 0u, 0u};
            if (HIT * 256 == NPH || pc < NPH) *(u32x4*)(lds_h + (pc >> 2) * PIXB + part * 16) = v;
        }
    };
    auto issue_w = [&](int c, auto rs) {
        constexpr int R = decltype(rs)::value;
        if (IG_DBG(p, 8) && c > 0) return;            // diagnostic builds: weight traffic of the first chunk only
        if constexpr (!WPK) {
            if (MT == 4 && NTAP == 1 && p.wsplit) {      // rows 0..63 / 64..127 of the tile: two 64-row packs [chunk][row][64 B], wsplit bytes apart
#pragma unroll
                for (int it = 0; it < WIT; ++it) {
                    const int pc = it * 256 + tid, row = pc >> 2;
                    wreg[R][it] = *(const u32x4*)(wb + (row >= 64 ? p.wsplit : 0) + ((size_t)c * 64 + (row & 63)) * 64 + (pc & 3) * 16);
                }
                return;
            }
            const char* ws = wb + (size_t)c * NTAP * COT * 64;
#pragma unroll
            for (int it = 0; it < WIT; ++it) {
                const int pc = it * 256 + tid;
                wreg[R][it] = *(const u32x4*)(ws + (size_t)((WIT * 256 == NPW || pc < NPW) ? pc : 0) * 16);
            }
        }
    };
    auto write_w = [&](auto rs) {
        constexpr int R = decltype(rs)::value;
        if constexpr (!WPK) {
#pragma unroll
            for (int it = 0; it < WIT; ++it) {
                const int pc = it * 256 + tid;
                if (WIT * 256 == NPW || pc < NPW) *(u32x4*)(lds_w + (pc >> 2) * PIXB + part * 16) = wreg[R][it];
            }
        }
    };

    // WPK (4x4 and larger kernels): one kernel row of weights in LDS at a time (LDS budget).  The row is prefetched into
    // registers one row ahead -- while the previous row's MFMAs run -- so its L2 latency is not exposed between two
    // barriers (it was: 16 MFMAs per wave against a 1-2 us load, matrix pipe 22 % busy on the 4x4 stride-2 layers).
    // Two rows ahead (even KH): one row's MFMA phase is 16-32 MFMAs per wave, 0.25-0.5 us -- less than the L2 round trip of the
    // row's loads, which was exposed once per kernel row (4x4 stride-2 layers: 16 rows per workgroup).
    constexpr int WPD = (WPK && KH % 2 == 0) ? 2 : 1;
    u32x4 wv[WPD][WPK ? WIT : 1];
    auto issue_wrow = [&](int c, int ky, int slot) {
        if (IG_DBG(p, 8) && (c > 0 || ky > 0)) return;
        if constexpr (WPK) {
            const char* ws = wb + ((size_t)c * NTAP + (size_t)ky * KW) * COT * 64;
#pragma unroll
            for (int it = 0; it < WIT; ++it) {
                const int pc = it * 256 + tid;
                wv[slot][it] = *(const u32x4*)(ws + (size_t)((WIT * 256 == NPW || pc < NPW) ? pc : 0) * 16);
            }
        }
    };
    auto write_wrow = [&](int slot) {
        if constexpr (WPK) {
#pragma unroll
            for (int it = 0; it < WIT; ++it) {
                const int pc = it * 256 + tid;
                if (WIT * 256 == NPW || pc < NPW) *(u32x4*)(lds_w + (pc >> 2) * PIXB + part * 16) = wv[slot][it];
            }
        }
    };

    using RS0 = std::integral_constant<int, 0>;
    using RS1 = std::integral_constant<int, NRS - 1>;
    auto chunk = [&](int c, auto rs) {
        // registers (chunk c) -> LDS; the previous chunk's readers passed the barrier at the end of the previous call
        if (!(IG_DBG(p, 16) && c > 0)) {
            write_halo(c, rs);
            write_w(rs);
            write_wrow(0);            // kernel row 0 of this chunk
        }
        __syncthreads();
        if (c + NRS < p.nchunk) {     // prefetch into the registers just drained: in flight while NRS chunks' MFMAs run
            issue_halo(c + NRS, rs);
            issue_w(c + NRS, rs);
        }
        // Fragment reads run ONE step (tap column, k-half) ahead of the MFMAs, in a register double buffer.  As plain
        // "read, then multiply" code hipcc emitted `ds_read x3, s_waitcnt lgkmcnt(0), v_mfma` per step (ISA of the 4x4 stride-2
        // layers): every MFMA behind an exposed LDS latency, matrix pipe 28 % busy with 2 waves per SIMD.
        // Two steps ahead where a step has only one or two MFMAs per wave (64 cycles: less than an LDS round trip).
        using frag_t = typename std::conditional<std::is_same<T, float>::value, f32x4, bf16x8>::type;
        constexpr int NSTEP = KW * 2, NFLAT = WPK ? NSTEP : KH * NSTEP;      // WPK: the ring restarts with every kernel row (its weights are rewritten)
        constexpr int PD = (MT * PT <= 2 && NSTEP >= 4) ? 2 : 1, NB = PD + 1;
        frag_t fa[NB][MT], fb[NB][PT];
        auto rd = [&](int kyw, int g) {          // flat step g of the ring; kyw = the kernel row in LDS (WPK)
            const int ky = WPK ? kyw : g / NSTEP, s2 = g % NSTEP;
            const int kx = s2 >> 1, ks = s2 & 1;
            const int tapw = WPK ? kx : ky * KW + kx;
            const int koff = ks * 32 + h * 16;
#pragma unroll
            for (int m = 0; m < MT; ++m)
                fa[g % NB][m] = *(const frag_t*)(lds_w + (tapw * COT + m * 32 + r) * PIXB + koff);
#pragma unroll
            for (int q = 0; q < PT; ++q)
                fb[g % NB][q] = *(const frag_t*)(lds_h + (((wave * PT + q) * S + ky) * IWT + r * S + kx) * PIXB + koff);
        };
#pragma unroll
        for (int ky = 0; ky < KH; ++ky) {
            if constexpr (WPK) {
                if (ky > 0) {
                    __syncthreads();  // the previous row's readers are done
                    if (!IG_DBG(p, 16)) write_wrow(ky % WPD);
                    __syncthreads();
                }
                // the row WPD ahead, into the registers just written out
                if (ky + WPD < KH) issue_wrow(c, ky + WPD, ky % WPD);
                else if (c + 1 < p.nchunk) issue_wrow(c + 1, ky + WPD - KH, ky % WPD);
            }
            if (WPK || ky == 0) {
#pragma unroll
                for (int g = 0; g < PD; ++g) rd(ky, g);
            }
#pragma unroll
            for (int s2 = 0; s2 < NSTEP; ++s2) {
                const int g = (WPK ? 0 : ky * NSTEP) + s2;
                if (g + PD < NFLAT) rd(ky, g + PD);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int q = 0; q < PT; ++q) {
                        if constexpr (std::is_same<T, float>::value) {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g % NB][m][j], fb[g % NB][q][j], acc[m][q], 0, 0, 0);
                        } else if (IG_DBG(p, 1)) {      // keep the fragment reads alive without the matrix pipe
                            const u32x4 t = __builtin_bit_cast(u32x4, fa[g % NB][m]) ^ __builtin_bit_cast(u32x4, fb[g % NB][q]);
                            acc[0][0][0] += __builtin_bit_cast(float, t[0] ^ t[1] ^ t[2] ^ t[3]);
                        } else
                            acc[m][q] = sg_mfma16<T>(fa[g % NB][m], fb[g % NB][q], acc[m][q]);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();   // all waves are done reading this chunk's LDS image
    };
    issue_halo(0, RS0{});
    issue_w(0, RS0{});
    issue_wrow(0, 0, 0);
    if constexpr (WPD == 2) issue_wrow(0, 1, 1);
    if constexpr (NRS == 2) {
        if (p.nchunk > 1) { issue_halo(1, RS1{}); issue_w(1, RS1{}); }
        for (int c = 0; c < p.nchunk; c += 2) {
            chunk(c, RS0{});
            if (c + 1 < p.nchunk) chunk(c + 1, RS1{});
        }
    } else {
        for (int c = 0; c < p.nchunk; ++c) chunk(c, RS0{});
    }

    // Epilogue.  The MFMA result holds one pixel per lane and 4 channels per register group: stored as it stands every
    // instruction scatters 8-byte pieces over 32 pixels (a strided parity store of a stride-2 gradient wrote 16 contiguous bytes
    // per pixel: those convolutions ran at 380 TFLOP/s, store-bound).  With 16-byte-aligned operands each wave transposes a
    // row of its tile through LDS (the stage buffers are free: every wave passed the loop's last barrier) and reads it back
    // with the lanes of a pixel contiguous: 128-byte segments per pixel for residual / mask loads and the store.
    if (IG_DBG(p, 4)) {                               // diagnostic builds: no epilogue (keep the accumulators alive)
        float keep = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < PT; ++q)
#pragma unroll
                for (int i = 0; i < 16; ++i) keep += acc[m][q][i];
        if (keep == 1.2345e-30f) *(float*)p.y = keep;
        return;
    }
    ConvP pe = p;
    if (p.npar == 2) { pe.oa = par; pe.ob = 0; }
    else if (p.npar) { pe.oa = par >> 1; pe.ob = par & 1; }
    if (p.buf16) {
        constexpr int RS = COT * 4 + 16;
        constexpr bool OPS = !(MT == 4 && NTAP == 1);          // the pixel-pair form of the up-sampler has no residual / mask operands
        char* lw = smem + wave * 32 * RS;
#pragma unroll
        for (int q = 0; q < PT; ++q) conv_epilogue_lds_row<T, MT, PT, OPS>(pe, acc, q, lw, b, ct, oy0 + wave * PT + q, ox0, lane);
    } else
        conv_epilogue<T, MT, PT>(pe, acc, b, ct, oy0 + wave * PT, ox0, r, h);
}

// ------------------------------------------------------------------ host launcher
template <typename T, int KH, int KW, int S, int MT, int PT, bool WPK>
static int launch_igemm(const ConvP& p, int ctiles, hipStream_t st) {
    constexpr int TH = 4 * PT, TW = 32;
    constexpr int IHT = (TH - 1) * S + KH, IWT = (TW - 1) * S + KW;
    constexpr int COT = 32 * MT, NTAP = KH * KW;
    constexpr size_t STAGE = (size_t)IHT * IWT * 80 + (size_t)(WPK ? KW : NTAP) * COT * 80, EPI = (size_t)4 * 32 * (COT * 4 + 16);
    constexpr size_t SMEM = STAGE > EPI ? STAGE : EPI;       // the LDS-transposed epilogue reuses the stage buffers
    constexpr auto kern = conv_igemm_k<T, KH, KW, S, MT, PT, WPK>;
    int dev = 0;
    SG_TRY(sg_current_device(dev));
    SG_TRY(sg_allow_lds<kern>(SMEM, dev));
    ConvP q = p;
    q.tiles_x = cdiv(p.OW, TW);
    q.tiles_y = cdiv(p.OH, TH);
    q.ctiles = ctiles;
    q.dbg = sg_dbg_flags();
    dim3 grid((unsigned)((size_t)q.tiles_x * q.tiles_y * p.B * ctiles), 1, 1);
    char cls[96];
    snprintf(cls, sizeof(cls), "conv_igemm<%s,%dx%d,s%d,MT%d>", sg_dtype_tag<T>(), KH, KW, S, MT);
    // algorithmic work: 2*pixels*taps*Cin*Cout flop; bytes: input read once + output written once
    const double px = (double)p.B * p.OH * p.OW * (p.npar ? p.npar : 1);
    const int tok = sg_prof_start(cls, 2.0 * px * NTAP * p.Cin * p.Cout,
                                  ((double)p.B * p.H * p.W * p.Cin + px * p.Cout) * sizeof(T), st);
    hipLaunchKernelGGL(kern, grid, dim3(256), SMEM, st, q);
    sg_prof_stop(tok, st);
    SG_LAUNCH_CHECK();
    return 0;
}

#ifndef SG_UP_PT
#define SG_UP_PT 1      // rows per wave of the up-sampler's pixel-pair form (2: 128 accumulator registers beside the 128-row epilogue -- spills, 16 % slower)
#endif
template <typename T, int MT>
static int dispatch_shape(const ConvP& p, int kh, int kw, int s, int ctiles, hipStream_t st) {
#define SG_CASE(KH_, KW_, S_, PT_, WPK_) \
    if (kh == KH_ && kw == KW_ && s == S_) return launch_igemm<T, KH_, KW_, S_, MT, PT_, WPK_>(p, ctiles, st);
    SG_CASE(3, 3, 1, 2, false)
    SG_CASE(1, 1, 1, 2, false)
    SG_CASE(2, 2, 2, 1, false)
#ifndef SG_PT22
#define SG_PT22 2
#endif
    SG_CASE(2, 2, 1, SG_PT22, false)
    SG_CASE(1, 2, 1, 2, false)
    SG_CASE(2, 1, 1, 2, false)
    SG_CASE(4, 4, 2, 1, true)
    SG_CASE(4, 4, 1, 2, true)
    SG_CASE(3, 4, 1, 2, true)        // parity classes of the 7x7 stride-2 stem's input gradient (resdeconv.py:113): 3 or 4 taps per axis
    SG_CASE(4, 3, 1, 2, true)
    SG_CASE(3, 3, 2, 1, false)
    SG_CASE(7, 7, 2, 1, true)        // ResDeconv stem (resdeconv.py:113)
    SG_CASE(1, 1, 2, 2, false)       // ResDeconv down-sample shortcut (resdeconv.py:12-15,157-161)
    SG_CASE(5, 5, 1, 2, true)        // ESPCN conv1 (espcn.py:33), SRCNN conv3 (srcnn.py:36)
    SG_CASE(9, 9, 1, 2, true)        // SRCNN conv1 (srcnn.py:32)
    SG_CASE(7, 7, 1, 2, true)        // ResnetGenerator's first and last layer behind ReflectionPad2d(3) (basicModel.py:164-165, 189-190)
#undef SG_CASE
    SG_FAIL("srcgan_conv_igemm: unsupported kernel %dx%d stride %d", kh, kw, s);
}

// entry used by srcgan_conv_igemm for every shape that has no kernel of its own; p.npar == 4: the 1x1 four-parity form
int sg_conv_generic(const ConvP& p, int dtype, int kh, int kw, int stride, hipStream_t st) {
    // pixel-pair form: 64 channels of 2 bytes, dense interleaved output -> one 128-row tile per ROW parity writes both column parities
    // (yplane == 64 stands for interleaved NHWC: the entry turns a plane stride of 0 into the 64-byte chunk, and a descriptor that
    //  passes 64 itself addresses the same bytes)
    if (p.npar == 4 && kh == 1 && kw == 1 && sg_is16(dtype) && p.Cout == 64 && p.ypix == 128 && p.ycoff == 0 && p.yplane == 64 && p.YW == 2 * p.OW &&
        p.buf16 && !p.bias && !p.r1 && !p.r2 && !p.mz && p.Cin % 32 == 0) {
        ConvP q = p;
        q.npar = 2; q.wpar = 2 * p.wpar; q.wsplit = p.wpar;
        q.Cout = 128; q.ypix *= 2; q.YW = p.YW / 2; q.osx = 1;
        return sg_dtype_dispatch16(dtype, [&](auto t) { return launch_igemm<decltype(t), 1, 1, 1, 4, SG_UP_PT, false>(q, 2, st); });
    }
    // Cout <= 32 -> one 32-row M tile per workgroup, otherwise 64-row tiles.
    const int npm = p.npar ? p.npar : 1;        // channel tiles = parities x tiles of one parity
    if (p.Cout <= 32) return sg_dtype_dispatch(dtype, [&](auto t) { return dispatch_shape<decltype(t), 1>(p, kh, kw, stride, npm, st); });
#ifdef SG_MT4_22
    // (variant) stride-2 parity gradients with >= 128 output rows: one 128-row tile per workgroup halves the dy staging per FLOP
    if (dtype == SRCGAN_BF16 && kh == 2 && kw == 2 && stride == 1 && p.Cout % 128 == 0)       // (the variant instantiates bf16 only)
        return launch_igemm<__bf16, 2, 2, 1, 4, SG_PT22, false>(p, p.Cout / 128, st);
#endif
    const int ctiles = cdiv(p.Cout, 64) * npm;
    return sg_dtype_dispatch(dtype, [&](auto t) { return dispatch_shape<decltype(t), 2>(p, kh, kw, stride, ctiles, st); });
}
