/*
 * srcgan_amd.h -- C ABI of the MI355X (gfx950) native SRCGAN training hot path.
 *
 * Drop-in boundary.  The reference (huster-wgm/SRCGAN) has no native code: its
 * hot path is torch.nn modules executed by ATen.  Each
 * entry point below replaces the ATen work behind one reference call site; the
 * Python host (srcgan_amd/) mirrors the reference's nn.Module / loss classes and
 * reaches these symbols through ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless said
 *     otherwise; `stream` is a hipStream_t passed as void*.
 *   - activations are NHWC ("channels-last") with an explicit channel stride
 *     (`cs`, elements per pixel) and channel offset (`coff`) so a convolution
 *     can read a channel prefix of a dense-block buffer and write its own
 *     channel slice -- this is what removes torch.cat (rddb.py:64-67).
 *   - dtype: SRCGAN_F32 (exact f32 MFMA, parity mode), SRCGAN_BF16 (bf16
 *     storage + bf16 MFMA, f32 accumulate; perf mode) or SRCGAN_F16 (the same
 *     kernels on IEEE half).
 *   - return value: 0 on success, non-zero on error; srcgan_last_error() gives
 *     the message (thread-local).  Shape/alignment violations are rejected on
 *     the host before any launch.
 */
#ifndef SRCGAN_AMD_H
#define SRCGAN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRCGAN_F32 0
#define SRCGAN_BF16 1
#define SRCGAN_F16 2        /* IEEE half storage + f16 MFMA (same rate as bf16), f32 accumulate: 3 more mantissa bits than bf16, 5-bit exponent
                               (BASELINE.json configs[4]); gradients below 2^-24 vanish, so training harnesses scale the loss */

int srcgan_version(void);
const char* srcgan_last_error(void);
/* bytes of one element of dtype */
int srcgan_dtype_size(int dtype);

/* ---------------------------------------------------------------------------
 * Layout: NCHW f32 (the reference's tensor format, dataset.py:131) <-> NHWC.
 * to_nhwc writes channels [0,C) and zero-fills [C,cs).
 * ------------------------------------------------------------------------- */
int srcgan_nchw_f32_to_nhwc(const float* src, void* dst, int B, int C, int H, int W,
                            int cs, int dtype, void* stream);
int srcgan_nhwc_to_nchw_f32(const void* src, float* dst, int B, int C, int H, int W,
                            int cs, int coff, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Weight packing.  Canonical torch weights stay f32 [Cout,Cin,kh,kw] (Conv2d) or
 * [Cin,Cout,kh,kw] (ConvTranspose2d) so state_dict / Adam are untouched; kernels
 * read a packed copy  Wp[row_tile][k_chunk][tap][row][k]  (dtype, zero padded).
 * packed(row r, k, tap (ty,tx)) = w[off + r*sr + k*sk + ty*sty + tx*stx].
 * The same routine produces forward, flipped/transposed dgrad and stride-2
 * parity-class packs by choice of strides.
 * ------------------------------------------------------------------------- */
size_t srcgan_packed_weight_bytes(int rows, int kdim, int ntaps, int dtype);
int srcgan_pack_weight(const float* w, void* wp, int rows, int kdim, int tys, int txs,
                       long sr, long sk, long sty, long stx, long off, int dtype, void* stream);
/* Fill only the k-range [k_off, k_off+kdim) of a packed matrix whose full K is k_total, values scaled by
 * `scale` (the caller zeroes the buffer first).  Used to assemble the composite transposed weights of the
 * dense-block backward: K = [conv5 co | conv4 co | ...] for one input-channel slice. */
int srcgan_pack_weight_part(const float* w, void* wp, int rows, int kdim, int tys, int txs,
                            long sr, long sk, long sty, long stx, long off, int k_off, int k_total, float scale,
                            int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Implicit-GEMM convolution (forward form).  Replaces aten::convolution for
 *   rddb.py:52-58 (3x3 s1), rddb.py:28-38 (k2 s2 deconv = 4 x 1x1 + pixel
 *   shuffle store), model/model.py:612-634 (4x4 s2 / s1), and -- with packed
 *   transposed weights -- every dgrad of aten::convolution_backward.
 *
 *   v   = alpha * (conv(x)[co] + bias[co])
 *       + (co < r1_cend ? beta1 * r1 : 0) + (co < r2_cend ? beta2 * r2 : 0)
 *   v   = act ? leaky_relu(v, slope) : v
 *   v  *= (co >= mz_c0 && mz) ? (mz > 0 ? 1 : mslope) : 1      (LeakyReLU' mask)
 *   y[b, oy*os+oa, ox*os+ob, ycoff+co] = v
 * r1/r2/mz are indexed like y.  r1 may alias y (in-place accumulate).
 * ------------------------------------------------------------------------- */
typedef struct srcgan_conv_desc {
    const void* x; const void* wp; const float* bias; void* y;
    const void* r1; const void* r2; const void* mz;
    int dtype;
    int kh, kw, stride;
    int B, H, W, Cin, x_cs, x_coff;         /* input tensor; Cin = channels read (multiple of 16B piece) */
    int OH, OW, Cout;                       /* conv output extent and true Cout */
    int YH, YW, y_cs, y_coff;               /* output tensor extent (after os scaling) */
    int pad_y, pad_x, os, oa, ob;
    int r1_cs, r1_coff, r1_cend;
    int r2_cs, r2_coff, r2_cend;
    int mz_cs, mz_coff, mz_c0;
    float alpha, beta1, beta2, slope, mslope;
    int act;
    /* plane strides in BYTES for the blocked layout (0 = interleaved NHWC): channel c of pixel q lives at
     * q*cs*esz + (c/KCE)*plane + (c%KCE)*esz with KCE = 64/esz channels; blocked tensors use cs = KCE. */
    long x_plane, y_plane, r1_plane, r2_plane, mz_plane;
    int rev_batch;     /* walk the images in reverse order (3x3 s1 kernel): consecutive layers alternate so that a layer starts on
                          the data its predecessor touched last (Infinity Cache reuse when a layer's footprint exceeds 256 MB) */
    /* LeakyReLU sign masks, one bit per channel instead of re-reading the 2-byte activation in the backward pass (3x3 s1 bf16,
     * Cout == 32, os == 1, blocked input: the dense-block convs).  u32 per output pixel (b, oy, ox), bit c = output channel c.
     *   sign_out: written by a forward conv with act != 0 (bit = activation output > 0)
     *   sign_in : read instead of mz:  v *= bit ? 1 : mslope
     * 64 channels (round 3; Cout / 8 = 8 bytes per output pixel, byte c / 8, bit c % 8): sign_out of the 1x1 four-parity form with act
     * (the up-sampler's last stage, rddb.py:93-97), sign_in of a 3x3 s1 convolution with Cout == 64 and no other epilogue operand
     * (conv_last's input gradient, rddb.py:98,113).
     * A descriptor that sets either and does not meet the conditions is refused (no silent fallback). */
    void* sign_out; const void* sign_in;
    /* npar == 4: the input gradient of a 4x4 stride-2 pad-1 convolution (model/model.py:612-634) with all four output parities in
     * ONE launch.  x = dy [B,H,W,Cin = the layer's Cout], y = dx [B,YH,YW,..] (Cout = the layer's Cin), kh = kw = 2, stride = 1:
     *   dx[2t+a][2u+b] = sum_{ty,tx in {0,1}} dy[t+a-1+ty][u+b-1+tx] * pack_q[tap (ty,tx)],   q = 2a + b,
     * pack_q = wp + q * wpar_stride bytes (rows = the layer's Cin, k = its Cout, taps ky = (a?2:3) - 2ty, kx = (b?2:3) - 2tx).
     * OH / OW / pad / os / oa / ob are derived from YH, YW; epilogue operands (mz, r1, ...) are indexed like y.  npar == 0: plain.
     * npar == 4 with kh = kw = 1 (ConvTranspose2d k2 s2 as four 1x1 convolutions, rddb.py:28-38, in one launch): os = 2, oa = ob = 0;
     *   y[2oy+a][2ox+b] = epilogue(x[oy][ox] * pack_q),  q = 2a + b,  pack_q = wp + q * wpar_stride bytes (Cout rows each).
     * npar == 4 with kh = kw = 3, stride = 2, pad 1 (ConvTranspose2d k3 s2 p1 output_padding 1, model/model.py:698-701, in one launch):
     *   x [B,H,W,Cin], y [B,2H,2W,..], OH x OW = H x W, os = 2, oa = ob = 0;
     *   y[2i+a][2j+b] = epilogue(sum_{wy <= a, wx <= b} x[i+wy][j+wx] * pack_q[tap wy * (b + 1) + wx]),  q = 2a + b (x = 0 past the edge),
     * pack_q = wp + q * wpar_stride bytes: rows = Cout, k = Cin, (a + 1) x (b + 1) taps with ky = a ? 2 - 2 wy : 1, kx = b ? 2 - 2 wx : 1 of
     * the canonical weight [Cin][Cout][3][3].  bias and act are fused; 16-byte accessible output channels are required. */
    int npar; long wpar_stride;
} srcgan_conv_desc;
/* Extents.  Tensors may be of any size (image bases and plane offsets are 64-bit; tested past 4 GiB).  Refused before launch:
 *   - one image of the input (H * W pixel records) of 2 GiB or more, except for the loader-specialised 3x3 stride-1 kernel (pad 1,
 *     Cin in whole 64-byte chunks or a single chunk, 18 input rows below 2 GiB), which takes images of any size;
 *   - a residual operand (r1 / r2) in channel planes of 2 GiB - 1 MiB or more beside a 3x3 stride-1 convolution with more than 32
 *     output channels. */
int srcgan_conv_igemm(const srcgan_conv_desc* d, void* stream);

/* ---------------------------------------------------------------------------
 * Weight gradient (the wgrad third of aten::convolution_backward):
 *   dW[co, tap, ci] = alpha * sum_{b,oy,ox} dy[b,oy,ox,co] * x[b, oy*s+ky-pad, ox*s+kx-pad, ci]
 * computed split-K over pixel ranges into an f32 slab, then reduced in a fixed
 * order (deterministic) and scattered to the canonical f32 gradient:
 *   grad[off + co*sr + ci*sk + ky*sty + kx*stx] (=|+=) value
 * ------------------------------------------------------------------------- */
typedef struct srcgan_wgrad_desc {
    const void* dy; const void* x; float* slab; float* grad;
    float* bias_grad;                       /* optional: bias_grad[co] (=|+=, as `accumulate` says) alpha * sum_p dy[p,co], fused (3x3 kernels only) */
    int dtype;
    int kh, kw, stride;
    int B, H, W, Cin, x_cs, x_coff;         /* x tensor; Cin = true input channels */
    int OH, OW, Cout, dy_cs, dy_coff;       /* dy tensor; Cout = true output channels */
    int pad_y, pad_x;
    int nsplit;
    long sr, sk, sty, stx, off;
    float alpha;
    int accumulate;
} srcgan_wgrad_desc;
/* slab bytes needed for (Cout,Cin,kh,kw,nsplit) */
size_t srcgan_conv_wgrad_slab_bytes(int Cout, int Cin, int kh, int kw, int nsplit);
/* a good nsplit for this problem (fills the chip, bounded slab) */
int srcgan_conv_wgrad_nsplit(int B, int OH, int OW, int Cout, int Cin, int stride);
int srcgan_conv_wgrad(const srcgan_wgrad_desc* d, void* stream);

/* ---------------------------------------------------------------------------
 * Dense-block weight gradient (3x3, stride 1, pad 1): ONE pass over a ResidualDenseBlock_5's activation buffer x
 * (C channels) and its dense gradient buffer dy (G channels = [dy5|dy4|dy3|dy2|dy1]) yields the weight and bias
 * gradients of all five convolutions (rddb.py:52-58).  Rows [g0,g1) of dy belong to a Conv2d weight
 * grad[g1-g0][Cin][3][3] (canonical f32) with bias gradient bias[g1-g0]; values are scaled by alpha.
 * Big (128 x 64 channel) tiles: 346 FLOP per staged byte vs 124-190 for srcgan_conv_wgrad.
 * ------------------------------------------------------------------------- */
typedef struct srcgan_wgrad_seg { int g0, g1; float* grad; float* bias; int Cin; float alpha; } srcgan_wgrad_seg;
typedef struct srcgan_wgrad_dense_desc {
    const void* dy; const void* x; float* slab;
    int dtype;
    int B, H, W;
    int G, dy_cs, dy_coff;
    int C, x_cs, x_coff;
    int nseg;
    srcgan_wgrad_seg seg[8];
    int accumulate;
    long dy_plane, x_plane;                 /* blocked-layout plane strides in bytes (0 = interleaved NHWC) */
} srcgan_wgrad_dense_desc;
size_t srcgan_wgrad_dense_slab_bytes(int G, int C, int dtype, int B, int H, int W);
int srcgan_wgrad_dense(const srcgan_wgrad_dense_desc* d, void* stream);

/* ---------------------------------------------------------------------------
 * Column reductions over pixels (deterministic two-stage):
 *   mode 0: out0[c] = scale * sum a[p,c]                         (bias grad; BN mean)
 *   mode 1: out0[c] = scale * sum (a[p,c]-m[c])^2                (BN variance)
 *   mode 2: out0[c] = scale * sum g[p,c] ; out1[c] = scale * sum g[p,c]*(z[p,c]-m[c])*rstd[c]   (BN backward; a = g)
 *   mode 3: out0[c] = mean of a[p,c] ; out1[c] = its biased variance -- ONE pass over a (per-thread shifted sums, partials
 *           combined exactly in a fixed order); `scale` and `m` are not used                       (BN statistics, training)
 * scratch: 2*nblk*C floats, nblk = srcgan_col_reduce_blocks(npix).
 * ------------------------------------------------------------------------- */
int srcgan_col_reduce_blocks(long npix);
int srcgan_col_reduce(int mode, const void* a, int a_cs, int a_coff, const void* z, int z_cs, int z_coff,
                      const float* m, const float* rstd, long npix, int C, float scale,
                      float* out0, float* out1, float* scratch, int dtype, void* stream);

/* BatchNorm2d(train)+LeakyReLU (model/model.py:622-623,630-631), NHWC.
 * bn_finalize: mean/var -> rstd, running-stat update (momentum .1, unbiased var), nbt++.
 * bn_apply:    y = lrelu(gamma*(z-mean)*rstd+beta)
 * bn_bwd_apply:dz = gamma*rstd*(g - sum_g/N - xhat*sum_gx/N)   (g already holds dy*lrelu'(y))
 * Shape constraints of bn_apply_lrelu and bn_bwd_apply (anything else is refused with an error, nothing is launched): the tensors
 * are dense NHWC, cs == C; C is a multiple of epp = 4 (f32) or 8 (bf16 / fp16), i.e. of one 16-byte vector; C/epp divides 256
 * (a thread owns one vector of channels and 256/(C/epp) threads share a pixel column), so C <= 1024 (f32) / 2048 (16-bit).
 * bn_bwd_apply may run in place, dz == g: a thread reads the elements it writes, and no others, before it writes them; the result
 * has the same bits as the out-of-place call.  z must not alias dz. */
int srcgan_bn_finalize(const float* mean, const float* var, float* rstd, float* running_mean,
                       float* running_var, int64_t* num_batches_tracked, int C, long count,
                       float momentum, float eps, void* stream);
int srcgan_bn_eval_rstd(const float* running_var, float* rstd, int C, float eps, void* stream);
int srcgan_bn_apply_lrelu(const void* z, void* y, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, long npix, int C, int cs, float slope, int dtype, void* stream);
int srcgan_bn_bwd_apply(const void* g, const void* z, void* dz, const float* mean, const float* rstd,
                        const float* gamma, const float* sum_g, const float* sum_gx, long npix, int C, int cs,
                        int dtype, void* stream);

/* y[p, ycoff+c] = (y + x[p, xcoff+c]) * (mz ? (mz[p, mzcoff+c] > 0 ? 1 : mslope) : 1) for c < C
 * (residual gradient joins; optional LeakyReLU' of the tensor the gradient belongs to) */
int srcgan_add_inplace(void* y, int y_cs, int y_coff, const void* x, int x_cs, int x_coff,
                       const void* mz, int mz_cs, int mz_coff, float mslope, long npix, int C, int dtype, void* stream);
/* same with blocked-layout plane strides (bytes, 0 = interleaved NHWC) for each tensor */
int srcgan_add_inplace_planes(void* y, int y_cs, int y_coff, long y_plane, const void* x, int x_cs, int x_coff, long x_plane,
                              const void* mz, int mz_cs, int mz_coff, long mz_plane, float mslope, long npix, int C,
                              int dtype, void* stream);

/* GroupNorm (+ residual add + ReLU) on NHWC activations (resdeconv.py:61-97,118-121; nn.GroupNorm(G, C), affine, biased
 * variance): y = act?((x - mean[b][g]) * rstd[b][g] * gamma[c] + beta[c] [+ res]), act = (Leaky)ReLU with `slope` (0 = ReLU;
 * edsr.py:43-49 uses 0.2) when relu != 0.  stats: device f32 [B][G][2] = {mean, rstd}
 * (written by forward, read by backward).  backward: g = dy [* (yact > 0)] (yact = the forward output when ReLU was applied);
 * dx = GroupNorm backward of g; dres (optional) = g (gradient of the residual branch; += when dres_accumulate); dgamma / dbeta
 * (optional) f32 [C], += when accumulate (a GroupNorm module applied twice, edsr.py:41,47,49).
 * scratch: srcgan_gn_scratch_floats(B, C) floats.  C/epp must divide 256 (epp = 16 bytes of channels).
 * gamma and / or beta may be null: no affine part -- with G == C that is nn.InstanceNorm2d(C) (model/model.py:598-631 with
 * norm_layer = InstanceNorm2d, basicModel.py:24-25).
 * Pinned by tests/test_gpu_groupnorm.py:
 *   - every operand has its own channel stride (a multiple of epp, >= C); nothing outside [0, C) of a record is read or written.
 *   - the statistics are those of the STORED x: |mean - mean64| <= 8 * 2^-24 (|mean64| + sd), |rstd - rstd64| <= 8 * 2^-24
 *     (1 + |mean64| / sd) rstd64, sd = sqrt(var64 + eps), also with the mean 1000 standard deviations from 0; image b of a batch
 *     has the bits of a call on that image alone, and a call repeated has the same bits.
 *   - a constant group: mean is that number exactly, the variance exactly 0, rstd = rsqrtf(eps) (316.2278 for 1e-5), y = beta.
 *   - y is ONE f32 expression cast once; with relu != 0 and slope == 0 a negative value gives -0 (v * 0), not +0.
 *   - the mask of the backward is yact > 0 (a stored 0, of either sign, takes the slope); g = dy * slope is an f32 product (-0 for a
 *     negative dy at slope 0).  dres = g cast once; with dres_accumulate, in a 16-bit type, g is FIRST rounded to the storage type
 *     and then added to the old value and rounded again (two roundings; exact whenever g is representable).
 *   - dx may be written over dy (dx == dy, same stride): a thread reads the elements it writes, and no others, before it writes
 *     them; the result has the bits of the out-of-place call.  (Read from the code, not tested: dx must not alias x or yact,
 *     dres must not alias dy or dx.)
 *   - dgamma / dbeta are overwritten unless accumulate; each of dres, dgamma, dbeta may be null on its own.
 *   - an error (C/epp not dividing 256, C > 1024, G not dividing C, a stride that is no multiple of epp, a bad dtype, a null
 *     required pointer) names the entry point in srcgan_last_error() and writes nothing. */
size_t srcgan_gn_scratch_floats(int B, int C);
int srcgan_gn_forward(const void* x, int x_cs, const void* res, int res_cs, void* y, int y_cs, const float* gamma, const float* beta,
                      float* stats, int B, long hw, int C, int G, float eps, int relu, float slope, int dtype, float* scratch, void* stream);
int srcgan_gn_backward(const void* dy, int dy_cs, const void* yact, int ya_cs, const void* x, int x_cs, const float* gamma, const float* stats,
                       void* dx, int dx_cs, void* dres, int dres_cs, int dres_accumulate, float* dgamma, float* dbeta, int accumulate,
                       float slope, int B, long hw, int C, int G, int dtype, float* scratch, void* stream);

/* Channel attention fused with the block residual, on NHWC activations (rcan.py:11-27 CALayer, :45-49 RCAB.forward):
 *   p[b][c] = mean_hw t[b][.][c];  h[b] = relu(W1 p[b] + b1);  s[b] = sigmoid(W2 h[b] + b2);  y = t * s[b][c] (+ res)
 * W1 [Cr][C], b1 [Cr], W2 [C][Cr], b2 [C]: device f32 (the two 1x1 convolutions of conv_du, as stored).  saved: device f32
 * [B][2C + Cr], per sample { p[C], h[Cr], s[C] } (written by forward, read by backward).  res may be null (y = t * s).
 * backward, g = dy:  dres (optional) = g (+= when dres_accumulate);  ds = sum_hw g t;  dz2 = ds s (1 - s);  dW2 = sum_b dz2 (x) h;
 * db2 = sum_b dz2;  dh = (W2^T dz2) [h > 0];  dW1 = sum_b dh (x) p;  db1 = sum_b dh;  dt = g s[b][c] + (W1^T dh)[b][c] / hw.
 * dw1 / db1 / dw2 / db2: device f32, overwritten; each may be null on its own.
 * scratch: srcgan_ca_scratch_floats(B, hw, C) floats (no state between calls).
 *   - C a multiple of 8, at most 1024; 1 <= Cr <= C; every operand has its own channel stride (a multiple of 16 bytes of
 *     channels, >= C); nothing outside [0, C) of a record is read or written.
 *   - three launches each way, no host synchronisation, no atomics: the pixel sums are taken per chunk of 256 pixels (a chunking that
 *     depends on hw alone) and folded in a fixed order, the batch sums of the parameter gradients run in sample order.  A call
 *     repeated gives the same bits.  Sums and the gate are f32; y, dt and dres are each rounded to the storage type once.
 *   - no output may alias an input or another output (the kernels take __restrict__ pointers).
 *   - an error (C no multiple of 8 or > 1024, Cr outside 1..C, a bad stride or dtype, a null required pointer) names the entry
 *     point in srcgan_last_error() and writes nothing. */
size_t srcgan_ca_scratch_floats(int B, long hw, int C);
int srcgan_ca_forward(const void* t, int t_cs, const void* res, int res_cs, void* y, int y_cs, const float* w1, const float* b1,
                      const float* w2, const float* b2, float* saved, int B, long hw, int C, int Cr, int dtype, float* scratch, void* stream);
int srcgan_ca_backward(const void* dy, int dy_cs, const void* t, int t_cs, const float* w1, const float* w2, const float* saved, void* dt,
                       int dt_cs, void* dres, int dres_cs, int dres_accumulate, float* dw1, float* db1, float* dw2, float* db2, int B,
                       long hw, int C, int Cr, int dtype, float* scratch, void* stream);

/* Back-projection glue of DDBPN (ddbpn.py:13-66) on NHWC activations; csrc/back_proj.hip, DESIGN.md section 3.9.  An image tensor
 * y [B][Hy][Wy][C] and a grid tensor g [B][Hg][Wg][s*s*C], channel (a*s + b)*C + c, are tied by the index map
 *   (m, n, a, b) <-> (oy, ox) = (s*m + a - shift, s*n + b - shift).
 *   srcgan_s2d_shift:  g[m][n][(a,b,c)] = x[oy][ox][c], zero where (oy, ox) lies outside the image (the whole grid is written).
 *   srcgan_d2s_shift:  y[oy][ox][c] = g[m][n][(a,b,c)] (+= when accumulate); grid positions that map outside the image are dropped.
 *     Each is the other's adjoint.  Pure copies: bit-exact.
 *   srcgan_prelu_forward:  y = PReLU_c(z + bias[c]) + beta * r,  PReLU_c(v) = v > 0 ? v : slope[c] * v.  z is a grid tensor read through
 *     the map (s == 1, shift == 0, Hg x Wg == Hy x Wy: a plain tensor); bias and r may be null; beta is +1 or -1; slope / bias: device f32 [C].
 *   srcgan_prelu_backward: dz = dy * (z + bias > 0 ? 1 : slope[c]) in z's layout, zero at grid positions outside the image (the whole
 *     grid is written);  dres (optional) = beta * dy (+= when dres_accumulate);  dslope[c] = sum of dy * (z + bias) over z + bias <= 0;
 *     dbias[c] = sum of dz (dslope / dbias: device f32, overwritten, each may be null).  scratch: srcgan_prelu_scratch_floats(B, Hg, Wg, C, s).
 *   - every operand is a channel slice: its pointer addresses the slice's first channel, *_cs is the channel stride of the buffer it
 *     lives in.  Nothing outside the slice is read or written.  16-byte accesses when C, the strides and the pointers are multiples of
 *     16 bytes, element-wise otherwise.  All counts are 64-bit.  The backward needs C / (16-byte vector or 1) <= 256.
 *   - the parameter sums are taken per chunk of 2048 grid positions and folded in a fixed order: no atomics, a call repeated gives the
 *     same bits.  Arithmetic is f32; y, dz and dres are rounded to the storage type once.
 *   - no output may alias an input (dres excepted, which is read when it accumulates).  The grid must cover the image:
 *     (Hy - 1 + shift) / s < Hg, likewise for the width.  An error names the entry point in srcgan_last_error() and writes nothing. */
int srcgan_s2d_shift(const void* x, int x_cs, void* g, int g_cs, int B, int Hx, int Wx, int C, int s, int shift, int Hg, int Wg, int dtype, void* stream);
int srcgan_d2s_shift(const void* g, int g_cs, void* y, int y_cs, int B, int Hy, int Wy, int C, int s, int shift, int Hg, int Wg, int accumulate, int dtype,
                     void* stream);
int srcgan_prelu_forward(const void* z, int z_cs, const float* slope, const float* bias, const void* r, int r_cs, float beta, void* y, int y_cs, int B,
                         int Hy, int Wy, int C, int s, int shift, int Hg, int Wg, int dtype, void* stream);
size_t srcgan_prelu_scratch_floats(int B, int Hg, int Wg, int C, int s);
int srcgan_prelu_backward(const void* dy, int dy_cs, const void* z, int z_cs, const float* slope, const float* bias, void* dz, int dz_cs, void* dres,
                          int dres_cs, float beta, int dres_accumulate, float* dslope, float* dbias, int B, int Hy, int Wy, int C, int s, int shift,
                          int Hg, int Wg, int dtype, float* scratch, void* stream);

/* x2 nearest up-sampling of an NHWC feature map (src may be a channel slice of a blocked buffer: s_plane != 0) and its
 * adjoint: dst[y][x] = sum of the 2x2 block of src, times LeakyReLU'(mz[y][x]) when mz is given.  Replaces
 * F.interpolate(scale_factor=2, mode='nearest') and its backward in the legacy generators (model/model.py:384-386,428-433). */
int srcgan_upsample2_nhwc(const void* src, int s_cs, int s_coff, long s_plane, void* dst, int d_cs,
                          int B, int H, int W, int C, int dtype, void* stream);
int srcgan_sum2x2_nhwc(const void* src, int s_cs, void* dst, int d_cs, const void* mz, int m_cs, float mslope,
                       int B, int H, int W, int C, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Loss reductions on flat f32 arrays (replace aten::l1_loss / mse_loss and their
 * backward; losses.py:95-147, train.py:67-128).  out: device f32 scalar.
 *   kind 0: mean |a-b|          kind 1: mean (a-b)^2      kind 2: mean (a-label)^2
 *   kind 3: mean of max(a,0) - a label + log1p(exp(-|a|))  (BCE with logits against the scalar label, the stable form)
 *   kind 4: mean of label * a   (label = -1 / +1: -mean for real, +mean for fake)
 * Kinds 0 and 1 need b; kinds 2..4 ignore it (it may be NULL).  a and b: contiguous f32 at ANY 4-byte alignment.  Where they share a
 * 16-byte phase the forward reads a scalar head, 16-byte groups and a scalar tail, where they differ it reads element by element; the
 * summation order therefore depends on the phases (and on nothing else: two calls give the same bits, and 16-byte aligned operands
 * sum as n / 4 groups plus the tail in block 0).  No front end copies to re-align.
 * fwd: out[0] = (sum of the terms, two stages of fixed order, f32) * (float)(1.0 / n).
 * bwd: da[i] = d term / d a[i] * g,  g = gout[0] * (gscale / (float)n): gout is a DEVICE scalar (the upstream gradient, never read on
 *      the host), gscale a host factor divided by (float)n on the host; gscale = -1 gives the gradient w.r.t. b of kinds 0 and 1.
 *      d/da: sign(a-b) with sign(0) = 0 | 2 (a-b) | 2 (a-label) | 1 / (1 + exp(-a)) - label | label.  Every element of da is written once;
 *      da needs 4-byte alignment only.
 * Refused (non-zero return, nothing launched): a NULL a / out / scratch / gout / da, n <= 0, a kind outside 0..4, kind 0 or 1 without b.
 * scratch: srcgan_loss_scratch_floats() floats.
 * Pinned by tests/test_gpu_mean_loss.py:
 *   - small-integer operands (every partial sum an integer < 2^24): out has the bits of f32(S) * f32(1.0 / n) at n = 1..8, 1023, 1024,
 *     1027, around the capped grid (1 048 572 .. 1 048 579) and over two grid-stride trips (2 097 157), with a at byte phase 0, 4, 8, 12
 *     and b at the same and at another phase; da of kinds 0 and 4 has the bits of sign * g / label * g for gout 1, 3, -0.5, gscale +-1.
 *   - reals: |out - float64| <= (D + 4) 2^-24 mean|term|, D the longest chain of additions of the launch; da of kinds 1 and 2 within
 *     5 * 2^-24 |float64| per element; kind 3 within 3 * 2^-24 N (value) and 12 * 2^-24 N (gradient), N the sum of the absolute terms,
 *     with logits of +-100 planted.
 *   - scratch may hold NaN on entry; nothing is written behind scratch, out or da, and a and b are unchanged.
 *   - srcgan_psnr_from_mse: within 3 * 2^-24 (|psnr| + 10 / ln 10) of float64; mse = 1 gives exactly 0, mse = 0 gives +inf.
 * ------------------------------------------------------------------------- */
int srcgan_loss_scratch_floats(void);
int srcgan_loss_fwd(int kind, const float* a, const float* b, float label, long n, float* out,
                    float* scratch, void* stream);
int srcgan_loss_bwd(int kind, const float* a, const float* b, float label, long n, const float* gout,
                    float gscale, float* da, void* stream);
/* psnr = 10*log10(1/mse) from a device mse scalar (losses.py:144-147) */
int srcgan_psnr_from_mse(const float* mse, float* out, void* stream);

/* ---------------------------------------------------------------------------
 * Classification-style losses (losses.py:150-167 CELoss, :258-274 ConLoss, :277-293 CrossLoss, :296-341 FLoss; class_losses.hip).
 * All tensors f32, contiguous, any 4-byte alignment (16-byte accesses where the pointers allow them); counts are 64-bit.  out: device
 * f32 scalar.  scratch: srcgan_loss_scratch_floats() floats.  Every forward sums in two stages of fixed order (no atomics: two calls
 * give the same bits); every backward reads the upstream gradient gout[0] from the device and writes EVERY element of its gradient
 * exactly once (no memset).  Only the gradient w.r.t. output / feats is produced.
 *
 *   srcgan_focal_*: flat over n elements.  o = clamp(output, lo, hi), lo = (float)1e-6, hi = (float)(1.0 - 1e-6);
 *       binary != 0:  l = -0.9 (1-o)^gamma t log o - 0.1 o^gamma (1-t) log(1-o)      binary == 0:  l = -(1-o)^gamma t log o
 *     out = sum l / n (mean != 0) or sum l.  doutput = gout * dl/do (/ n) where lo <= output <= hi, bounds included, and exactly 0
 *     outside (clamp's gradient).  An integer gamma in [0, 8] is taken by repeated multiplication; any other gamma from exp(gamma log b)
 *     on the logarithms of the formula (no powf).
 *   srcgan_bce_*: nn.BCELoss, mean: l = -(t max(log o, -100) + (1-t) max(log(1-o), -100)); doutput = gout (o - t) / max(o (1-o), 1e-12) / n.
 *     No range check: an output outside [0, 1] gives NaN.
 *   srcgan_nll_argmax_*: output / target [N, C, S].  Per (n, s): k = the FIRST maximum of target[n, :, s] (strict >, lowest channel wins);
 *     out = mean over the N*S positions of -log output[n, k, s]; doutput = -gout / (output[n, k, s] N S) at channel k, 0 at the others.
 *   srcgan_batch_range_*: feats [nb, M].  r[m] = max_b - min_b; out = mean_m r^2.  dfeats = +2 r gout / M at the first maximum's sample,
 *     -2 r gout / M at the first minimum's (lowest sample on ties; the two add where both are one sample), 0 elsewhere; the indices are
 *     recomputed from feats.  A NaN in a column makes the loss NaN (the gradient is then unspecified).
 *   srcgan_cross_l1_*: output / target [nb, S], nb >= 2.  out = mean over (nb-1) S elements of |output[b] - target[b+1]|;
 *     doutput[b] = sign(.) gout * (1 / (float)((nb-1) S)) for b < nb-1 (sign(0) = 0, the expression of srcgan_loss_bwd), zeros for b = nb-1.
 * ------------------------------------------------------------------------- */
int srcgan_focal_fwd(const float* output, const float* target, long n, int binary, float gamma, int mean, float* out,
                     float* scratch, void* stream);
int srcgan_focal_bwd(const float* output, const float* target, long n, int binary, float gamma, int mean, const float* gout,
                     float* doutput, void* stream);
int srcgan_bce_fwd(const float* output, const float* target, long n, float* out, float* scratch, void* stream);
int srcgan_bce_bwd(const float* output, const float* target, long n, const float* gout, float* doutput, void* stream);
int srcgan_nll_argmax_fwd(const float* output, const float* target, int N, int C, long S, float* out, float* scratch, void* stream);
int srcgan_nll_argmax_bwd(const float* output, const float* target, int N, int C, long S, const float* gout, float* doutput, void* stream);
int srcgan_batch_range_fwd(const float* feats, int nb, long M, float* out, float* scratch, void* stream);
int srcgan_batch_range_bwd(const float* feats, int nb, long M, const float* gout, float* dfeats, void* stream);
int srcgan_cross_l1_fwd(const float* output, const float* target, int nb, long S, float* out, float* scratch, void* stream);
int srcgan_cross_l1_bwd(const float* output, const float* target, int nb, long S, const float* gout, float* doutput, void* stream);

/* In-step preprocessing (trainCas.py:85-90): gray = .2125R+.7154G+.0721B (NCHW f32 in/out),
 * bilinear x(1/up) with align_corners=False == mean of the centre 2x2 of each up x up block. */
int srcgan_rgb_to_gray(const float* rgb, float* gray, int B, int H, int W, void* stream);
int srcgan_bilinear_down(const float* src, float* dst, int B, int C, int H, int W, int up, void* stream);
/* nearest: the rule of F.interpolate(size=(OH, OW)), source index min(floor(dst * (float)in / out), in - 1) with the scale in f32.
 * Equal to it bit for bit for any ratio (tests/test_gpu_resample.py: 2, 3, 4, their inverses, 7 -> 3, 5 -> 13, 1 -> 4); for the
 * factors the callers pass (2, 4, 1/2, 1/4) F.interpolate(scale_factor=) gives the same picture. */
int srcgan_nearest_resize(const float* src, float* dst, int B, int C, int H, int W, int OH, int OW, void* stream);
/* bilinear x up (integer up >= 1, align_corners=False): the second half of the blur of trainCasConst.py:89-92.  The source
 * coordinate (2 o + 1 - up) / (2 up) is split in integers, each weight is one rounded quotient: equal to float64 F.interpolate cast
 * to f32 on integer data for up = 1, 2, 4, 8, within 4 * 2^-24 * sum |w tap| of it for the tested factors 1, 2, 3, 4, 8
 * (tests/test_gpu_resample.py; the constant is measured to hold there, not derived for every up).
 * srcgan_bilinear_down is exact on integer data (weights 1/4). */
int srcgan_bilinear_up(const float* src, float* dst, int B, int C, int H, int W, int up, void* stream);
/* Gray-path preprocessing of the cycle step (train.py:251-260), NCHW f32, s = 2 or 4:
 *   gray_nearest_down: y[B,1,H/s,W/s], y[b,0,oy,ox] = gray(rgb[b,:,oy*s,ox*s])  == nearest x(1/s) of srcgan_rgb_to_gray (s | H, W)
 *   rep3_nearest_up:   y[B,3,s*h,s*w], y[b,c,Y,X]   = x[b,0,Y/s,X/s]            == nearest x s of cat([x, x, x], 1)
 * Each is one pass over the low-resolution side; no full-resolution gray image and no 3-channel low-resolution tensor is made. */
int srcgan_gray_nearest_down(const float* rgb, float* y, int B, int H, int W, int s, void* stream);
int srcgan_rep3_nearest_up(const float* x, float* y, int B, int h, int w, int s, void* stream);

/* ---------------------------------------------------------------------------
 * Whole-network passes (C++ sequencing of the kernels above; one call per
 * nn.Module.forward / autograd backward).
 *
 * RDDBNet (rddb.py:85-114).  params/grads: arrays of device f32 pointers in
 * state_dict order (conv_first.weight, conv_first.bias, RRDB_trunk.0.RDB1.conv1.weight, ...).
 * ------------------------------------------------------------------------- */
typedef struct srcgan_rddbnet_cfg {
    int in_ch, out_ch, up, nf, nb, gc;
    int B, H, W;
    int dtype;
    int down;          /* 0: RDDBNet (LR->HR, deconv up-sampler).  >0: HR->LR mirror
                          ("RDDBNetA", build-defined): `down` = /2^k factor, strided 3x3 convs */
    int legacy;        /* 0: rddb.py RDDBNet.  1: model/model.py:394-440 RDDBNetB (G_A of train.py:172): nearest x2 +
                          upconv1/upconv2, HRconv applied 8 times, conv_last with bias; `up` = 2 ('x2': upconv1 twice) or
                          4 ('x4').  2: model/model.py:347-391 legacy RDDBNet (its trunk result is discarded by the
                          reference's forward: not computed, no gradients); `up` = 1, 2 or 4.
                          3: srdn.py:56-74 SRDN (conv_first, RRDB_encoder, + skip, RRDB_decoder, + skip, conv_last; its trunk_conv
                          is never applied: pass it, it gets no gradient); `up` = 1, `nb` = RRDBs per stack.
                          params/grads follow the respective state_dict order. */
} srcgan_rddbnet_cfg;
/* Per-call options of the whole-network entry points (the plain forms pass NULL):
 *   wpack / pack    persistent packed-weight buffer (srcgan_*_wpack_bytes(cfg), 256-byte aligned).  NULL: the weights are packed
 *                   into the call's workspace every call.  Given: packed into it only when pack != 0, so a caller that tracks
 *                   weight updates packs ONCE per optimiser step although a cycle step runs each generator three times
 *                   (train.py:228-260).  Forward and backward packs are separate regions: pack the forward set in a forward
 *                   call, the backward set in a backward call.  The layout depends on the cfg's channel counts, dtype, up /
 *                   down / legacy (and for the discriminator on H, W parity), not on B, H, W.
 *                   pack == 2 ("verify"): `guard` points at two 64-bit device words {fingerprint the pack was made from,
 *                   fingerprint of the parameters now} (srcgan_params_fingerprint); the pack kernels run but do nothing when the
 *                   words are equal -- the decision is taken on the device, with no host synchronisation, so weight updates the
 *                   host cannot see (p.data.mul_(), raw-pointer writes) are still honoured.  The caller copies word 1 to word 0
 *                   after the call.
 *   rrdb_lo/rrdb_hi rddbnet backward only.  hi <= 0: the whole backward.  Otherwise this call handles the RRDBs [lo, hi), last
 *                   to first; the call with hi == number of RRDBs also runs everything behind the trunk (conv_last, up-sampler,
 *                   trunk_conv), the call with lo == 0 everything in front of it (conv_first, dx).  Calls come in descending,
 *                   gap-free order on one stream with the same ws / scratch / grads; when a call returns, the gradients of the
 *                   parameters it covers are final (data parallel: their all-reduce starts while earlier blocks still compute).
 * The `ws` / `scratch` parameters of every whole-network entry point below (and `wpack`, `grads`, a weight-gradient `slab`): the
 * contents on entry are unspecified.  A call reads no byte of them that it (or, for a backward, its forward on the same `ws`) has not
 * written, and writes nothing outside the first *_bytes bytes: results do not depend on what the buffers held. */
typedef struct srcgan_net_opts {
    void* wpack;
    int pack;
    int rrdb_lo, rrdb_hi;
    const void* guard;
} srcgan_net_opts;
/* 64-bit order-independent fingerprint of a list of f32 tensors (every bit of every element).  table_dev: device int64
 * [ntensors][3] = {pointer, element count, first block}; tensor t is served by the blocks [first block(t), first block(t+1)) of 16384
 * elements each; nblocks = their total.  out_u64: one device word (zeroed and accumulated on `stream`). */
int srcgan_params_fingerprint(const void* table_dev, int ntensors, long nblocks, void* out_u64, void* stream);
int srcgan_rddbnet_num_params(const srcgan_rddbnet_cfg* c);
size_t srcgan_rddbnet_ws_bytes(const srcgan_rddbnet_cfg* c);        /* training-forward workspace (kept for backward; grows with nb) */
size_t srcgan_rddbnet_bwd_scratch_bytes(const srcgan_rddbnet_cfg* c);
int srcgan_rddbnet_forward(const srcgan_rddbnet_cfg* c, const float* x_nchw, const float* const* params,
                           void* ws, float* y_nchw, void* stream);
/* grads[i] may be NULL (parameter frozen); dx_nchw may be NULL */
int srcgan_rddbnet_backward(const srcgan_rddbnet_cfg* c, const float* dy_nchw, const float* const* params,
                            void* ws, void* scratch, float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_rddbnet_wpack_bytes(const srcgan_rddbnet_cfg* c);
int srcgan_rddbnet_forward_ex(const srcgan_rddbnet_cfg* c, const float* x_nchw, const float* const* params,
                              void* ws, float* y_nchw, const srcgan_net_opts* opt, void* stream);
int srcgan_rddbnet_backward_ex(const srcgan_rddbnet_cfg* c, const float* dy_nchw, const float* const* params,
                               void* ws, void* scratch, float* const* grads, float* dx_nchw, const srcgan_net_opts* opt, void* stream);
/* Inference forward (no backward can follow).  Same cfg, parameter order and packed-weight handling (opt->wpack / pack / guard;
 * the pack buffer of srcgan_rddbnet_wpack_bytes serves both) as srcgan_rddbnet_forward_ex, and the same launches, so the output is
 * bit-identical to it; only the workspace differs.  Its activation part (srcgan_rddbnet_infer_ws_bytes minus
 * srcgan_rddbnet_wpack_bytes) does not depend on nb: the trunk runs on THREE dense buffers in rotation (RDB r+1 takes the buffer
 * that is neither RDB r's nor its RRDB's input buffer) plus an nf-channel copy of the first trunk input for the global skip;
 * tensors at any other resolution (up-sampler stages, legacy tails, RDDBNetA's down stages) ping-pong between two buffers; no
 * LeakyReLU sign mask is written.  Serves every cfg srcgan_rddbnet_ws_bytes accepts (0 + srcgan_last_error otherwise).
 * The HR tail is always unfused: a fused tail kernel was built, measured slower than the launches it replaces and not kept
 * (DESIGN section 8, row 5c). */
size_t srcgan_rddbnet_infer_ws_bytes(const srcgan_rddbnet_cfg* c);
int srcgan_rddbnet_infer(const srcgan_rddbnet_cfg* c, const float* x_nchw, const float* const* params, void* ws,
                         float* y_nchw, const srcgan_net_opts* opt, void* stream);
/* Parameter layout questions, answered by the planner that defines the layout.  num_rrdb: RRDBs in the trunk (SRDN: both stacks;
 * legacy RDDBNet: 0), -1 on a bad cfg.  phase_params: the parameters [*first, *end) (state_dict order) whose gradients a backward
 * call over the RRDBs [lo, hi) finalises (srcgan_net_opts.rrdb_lo/hi): hi == num_rrdb extends the range to the last parameter,
 * lo == 0 to parameter 0, so gap-free descending phases tile [0, num_params) and a network without a trunk is one range.
 * Non-zero + srcgan_last_error on a bad cfg or a range outside [0, num_rrdb]. */
int srcgan_rddbnet_num_rrdb(const srcgan_rddbnet_cfg* c);
int srcgan_rddbnet_phase_params(const srcgan_rddbnet_cfg* c, int lo, int hi, int* first, int* end);

/* NLayerDiscriminator (model/model.py:595-639).  params in state_dict order of the
 * learnable tensors: conv0.w, conv0.b, [conv_l.w, bn_l.gamma, bn_l.beta]*, conv_last.w, conv_last.b.
 * bn_state: per BN layer running_mean, running_var (f32) ; nbt: int64 counters.
 * norm = 1: norm_layer = nn.InstanceNorm2d (model/model.py:607-610: the normalised convolutions then HAVE a bias; InstanceNorm2d
 * as basicModel.py:24-25 builds it -- no affine parameters, no running statistics, instance statistics in train and eval mode):
 * learnable tensors conv0.w, conv0.b, [conv_l.w, conv_l.b]*, conv_last.w, conv_last.b; bn_running / bn_nbt are not read. */
typedef struct srcgan_nlayerd_cfg {
    int in_ch, ndf, n_layers;
    int B, H, W;
    int dtype;
    int training;
    int norm;              /* 0 = BatchNorm2d (the reference's default), 1 = InstanceNorm2d */
} srcgan_nlayerd_cfg;
int srcgan_nlayerd_num_params(const srcgan_nlayerd_cfg* c);
int srcgan_nlayerd_out_hw(const srcgan_nlayerd_cfg* c, int* oh, int* ow);
size_t srcgan_nlayerd_ws_bytes(const srcgan_nlayerd_cfg* c);
size_t srcgan_nlayerd_bwd_scratch_bytes(const srcgan_nlayerd_cfg* c);
int srcgan_nlayerd_forward(const srcgan_nlayerd_cfg* c, const float* x_nchw, const float* const* params,
                           float* const* bn_running, int64_t* const* bn_nbt, void* ws, float* y_nchw, void* stream);
int srcgan_nlayerd_backward(const srcgan_nlayerd_cfg* c, const float* dy_nchw, const float* const* params,
                            void* ws, void* scratch, float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_nlayerd_wpack_bytes(const srcgan_nlayerd_cfg* c);
int srcgan_nlayerd_forward_ex(const srcgan_nlayerd_cfg* c, const float* x_nchw, const float* const* params,
                              float* const* bn_running, int64_t* const* bn_nbt, void* ws, float* y_nchw,
                              const srcgan_net_opts* opt, void* stream);
int srcgan_nlayerd_backward_ex(const srcgan_nlayerd_cfg* c, const float* dy_nchw, const float* const* params,
                               void* ws, void* scratch, float* const* grads, float* dx_nchw, const srcgan_net_opts* opt, void* stream);

/* ResDeconv colouriser (resdeconv.py:99-195; C network of trainCas.py:31,99-100): [B,3,H,W] f32 NCHW -> [B,tar_ch,H,W];
 * H, W multiples of 16.  params/grads in state_dict order (conv1.weight, bn1.{weight,bias}, layer1.0.conv1.weight, ...,
 * pred.weight); a null grads[i] skips that gradient.  The input gradient is optional (the reference harnesses feed data). */
typedef struct srcgan_resdeconv_cfg {
    int in_ch, out_ch;     /* in_ch must be 3 (a 1-channel source is replicated by the caller, resdeconv.py:166-167) */
    int B, H, W;
    int dtype;
    int layers[4];         /* BasicBlocks per stage, resdeconv.py:107,123-137 ([2,2,2,2] = ResNet-18 layout, [3,4,6,3] = ResNet-34);
                            * all zero = [2,2,2,2].  The up path uses layers[2], layers[1], layers[0]. */
    int norm;              /* 0 = BN='GN': nn.GroupNorm(32, C) (the reference's default); 1 = BN='IN': nn.InstanceNorm2d(C), which has
                            * no parameters -- the state_dict then holds the convolution weights only */
} srcgan_resdeconv_cfg;
int srcgan_resdeconv_num_params(const srcgan_resdeconv_cfg* c);
size_t srcgan_resdeconv_ws_bytes(const srcgan_resdeconv_cfg* c);
size_t srcgan_resdeconv_bwd_scratch_bytes(const srcgan_resdeconv_cfg* c);
int srcgan_resdeconv_forward(const srcgan_resdeconv_cfg* c, const float* x_nchw, const float* const* params, void* ws,
                             float* y_nchw, void* stream);
/* dx_nchw: gradient w.r.t. the input [B,3,H,W] f32, or NULL */
int srcgan_resdeconv_backward(const srcgan_resdeconv_cfg* c, const float* dy_nchw, const float* const* params, void* ws,
                              void* scratch, float* const* grads, float* dx_nchw, void* stream);
/* Inference forward (no backward can follow): the launches of srcgan_resdeconv_forward in the same order with the same arguments,
 * on a workspace whose tensors share slots -- a slot is handed back after its tensor's last reader, an op's output never aliases its
 * inputs.  The activation part (infer_act_bytes = infer_ws_bytes minus the packed weights) does not depend on `layers`.
 * fold_tail = 0: bit-identical to srcgan_resdeconv_forward.  fold_tail = 1: deconv13 -> pred (resdeconv.py:194-195, linear: no bias,
 * nothing between them) run as four parity 2x2 convolutions 64 -> tar_ch on the half-resolution tensor with composed weights
 * (srcgan_fold_tail_pack); the 64-channel full-resolution tensor is never made.  Equal in real arithmetic, not bit for bit.
 * infer_plan (for tests of the planner): per op k, ranges[6k..6k+5] = byte {offset, size} of its input, its residual operand
 * (0, 0: none) and its output inside the workspace; writes at most `cap` ops, returns the op count or -1. */
size_t srcgan_resdeconv_infer_ws_bytes(const srcgan_resdeconv_cfg* c, int fold_tail);
size_t srcgan_resdeconv_infer_act_bytes(const srcgan_resdeconv_cfg* c, int fold_tail);
int srcgan_resdeconv_infer_plan(const srcgan_resdeconv_cfg* c, int fold_tail, size_t* ranges, int cap);
int srcgan_resdeconv_infer(const srcgan_resdeconv_cfg* c, const float* x_nchw, const float* const* params, void* ws,
                           float* y_nchw, int fold_tail, void* stream);
/* Composed weights of ConvTranspose2d(64, 64, k2 s2, no bias) [64,64,2,2] followed by Conv2d(64, tar, 3x3 p1, no bias) [tar,64,3,3]
 * (tar <= 8), both f32: four packs Wp[parity a * 2 + b][chunk][tap dy * 2 + dx][row (32)][k] of the 2x2 stride-1 convolutions that
 * give output pixel (2i + a, 2j + b) from the input pixels (i + a - 1 + dy, j + b - 1 + dx); rows >= tar are zero. */
size_t srcgan_fold_tail_pack_bytes(int dtype);
int srcgan_fold_tail_pack(const float* w_deconv, const float* w_conv, void* wp, int tar, int dtype, void* stream);

/* SR networks selectable as --SRModel (trainCas.py:169): kind 0 = ESPCN (espcn.py:18-51; the CLI default), kind 1 = SRCNN
 * (srcnn.py:17-42), kind 2 = EDSR (edsr.py:37-110: GroupNorm residual blocks, [B,out_ch,H*up,W*up]).  [B,in_ch,H,W] f32 NCHW -> ESPCN [B,out_ch,H*up,W*up] / SRCNN [B,out_ch,H,W].  params/grads in state_dict
 * order (conv1.weight, conv1.bias, ...).  dx_nchw: gradient w.r.t. the input [B,in_ch,H,W] f32, or NULL. */
typedef struct srcgan_srnet_cfg {
    int kind, in_ch, out_ch, up, base;     /* base = base_kernel / base_channel (64) */
    int B, H, W;
    int dtype;
    int nres;                              /* EDSR: num_residuals (50) */
} srcgan_srnet_cfg;
int srcgan_srnet_num_params(const srcgan_srnet_cfg* c);
size_t srcgan_srnet_ws_bytes(const srcgan_srnet_cfg* c);
size_t srcgan_srnet_bwd_scratch_bytes(const srcgan_srnet_cfg* c);
int srcgan_srnet_forward(const srcgan_srnet_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_srnet_backward(const srcgan_srnet_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                          float* const* grads, float* dx_nchw, void* stream);
/* Inference forward of ESPCN / SRCNN / EDSR: as srcgan_resdeconv_infer with fold_tail = 0 (bit-identical to srcgan_srnet_forward;
 * the activation part does not depend on nres). */
size_t srcgan_srnet_infer_ws_bytes(const srcgan_srnet_cfg* c);
size_t srcgan_srnet_infer_act_bytes(const srcgan_srnet_cfg* c);
int srcgan_srnet_infer_plan(const srcgan_srnet_cfg* c, size_t* ranges, int cap);
int srcgan_srnet_infer(const srcgan_srnet_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);

/* SRDenseNetA (kind 0, LR -> HR) / SRDenseNetB (kind 1, HR -> LR), reference src/model/model.py:643-786: conv_first (in_ch -> 1),
 * conv (1 -> growth * num_layers) + ReLU, num_blocks DenseBlocks of num_layers 3x3 layers with `growth` channels each, a 1x1 bottleneck
 * to 256 + ReLU, the up-sampler ConvTranspose2d(256, 256, k3 s2 p1 output_padding 1) + ReLU (A) or the down-sampler Conv2d(256, 256,
 * k3 s2 p1) + ReLU (B) applied once (up = 2: mode 'x2') or twice with the SAME weights (up = 4: 'x4'; their gradients add over the two
 * uses), reconstruction (256 -> 1), conv_last (1 -> out_ch).  [B,in_ch,H,W] f32 NCHW -> A: [B,out_ch,H*up,W*up]; B: each stage maps n to
 * (n + 1) / 2 (any H, W >= 2, odd sizes included).  params / grads in state_dict order: conv_first.{weight,bias}, conv.conv.*,
 * dense_blocks.<i>.block.<j>.conv.*, bottleneck.0.*, deconv.0.*, reconstruction.*, conv_last.*.
 * The dense blocks run concat-free in ONE buffer of growth * num_layers * (num_blocks + 1) channels (every block's output is the next
 * block's input prefix), so a cfg is refused unless growth % 8 == 0 (a layer's slice is addressed in 16-byte pieces) and growth *
 * num_layers is a multiple of the 64-byte K chunk (16 channels in f32, 32 in bf16 / f16: the slice offset of block i is growth *
 * num_layers * (i + 1)).  The infer entry runs the forward's launches on a slot-planned workspace (same bits). */
typedef struct srcgan_srdense_cfg {
    int kind, in_ch, out_ch;
    int B, H, W;
    int dtype;
    int growth, num_blocks, num_layers;
    int up;                                /* 2 or 4 */
} srcgan_srdense_cfg;
int srcgan_srdense_num_params(const srcgan_srdense_cfg* c);
int srcgan_srdense_out_hw(const srcgan_srdense_cfg* c, int* oh, int* ow);
size_t srcgan_srdense_ws_bytes(const srcgan_srdense_cfg* c);
size_t srcgan_srdense_bwd_scratch_bytes(const srcgan_srdense_cfg* c);
int srcgan_srdense_forward(const srcgan_srdense_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
/* grads[i] may be NULL; dx_nchw: gradient w.r.t. the input [B,in_ch,H,W] f32, or NULL */
int srcgan_srdense_backward(const srcgan_srdense_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                            float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_srdense_infer_ws_bytes(const srcgan_srdense_cfg* c);
int srcgan_srdense_infer(const srcgan_srdense_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);

/* RCAN, the Residual Channel Attention Network (reference src/model/rcan.py:69-116 with common.py:11-21,59-86): sub_mean (MeanShift, a
 * frozen 1x1 convolution 3 -> 3 + bias) -> head (3x3, 3 -> n_feats) -> n_resgroups x [ n_resblocks x [3x3 + ReLU, 3x3, channel
 * attention (srcgan_ca_forward) + block input], 3x3 + group input ] -> 3x3 + head output -> Upsampler (per x2 stage 3x3 to 4 n_feats
 * + PixelShuffle(2); scale 3: 3x3 to 9 n_feats + PixelShuffle(3)) -> 3x3 to 3 -> add_mean (MeanShift).  [B,3,H,W] f32 NCHW ->
 * [B,3,H*scale,W*scale].  params / grads in parameters() order, which is registration order: sub_mean.{weight,bias}, add_mean.{weight,
 * bias}, head.0.*, body.<g>.body.<b>.body.{0,2}.*, body.<g>.body.<b>.body.3.conv_du.{0,2}.*, body.<g>.body.<n_resblocks>.*,
 * body.<n_resgroups>.*, tail.0.<2 stage>.*, tail.1.*.  MeanShift runs from its parameters (params[0..3]) and takes no gradient:
 * grads[0..3] must be NULL.  Refused: in_ch or out_ch != 3, scale not in {2, 3, 4, 8}, n_feats no multiple of 16 or > 1024,
 * n_feats / reduction < 1.  The infer entries are those of srcgan_srnet_infer (same launches on the slot-planned workspace, same bits;
 * one `saved` region serves every attention op; the activation part does not depend on n_resgroups / n_resblocks from 2 x 2 on). */
typedef struct srcgan_rcan_cfg {
    int in_ch, out_ch;
    int B, H, W;
    int dtype;
    int n_resgroups, n_resblocks, n_feats, reduction, scale;
} srcgan_rcan_cfg;
int srcgan_rcan_num_params(const srcgan_rcan_cfg* c);
size_t srcgan_rcan_ws_bytes(const srcgan_rcan_cfg* c);
size_t srcgan_rcan_bwd_scratch_bytes(const srcgan_rcan_cfg* c);
int srcgan_rcan_forward(const srcgan_rcan_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_rcan_backward(const srcgan_rcan_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                         float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_rcan_infer_ws_bytes(const srcgan_rcan_cfg* c);
size_t srcgan_rcan_infer_act_bytes(const srcgan_rcan_cfg* c);
int srcgan_rcan_infer_plan(const srcgan_rcan_cfg* c, size_t* ranges, int cap);
int srcgan_rcan_infer(const srcgan_rcan_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);

/* DDBPN, the Dense Deep Back-Projection Network (reference src/model/ddbpn.py:68-130): sub_mean (MeanShift) -> 3x3 (3 -> 128) + PReLU ->
 * 1x1 (128 -> 32) + PReLU -> six up- and five down-modules (DenseProjection, :29-66), alternating, each reading the concatenation of
 * all earlier outputs at its resolution -> 3x3 (192 -> 3) at HR -> add_mean.  [B,3,H,W] f32 NCHW -> [B,3,H*scale,W*scale].
 * n0 = 128, nr = 32 and depth = 6 are the reference's constants.  A projection Conv2d / ConvTranspose2d (k, s, 2) with (k, s) = (6, 2),
 * (8, 4), (12, 8) runs as a stride-1 convolution of ceil(k / s) taps per axis on a space-to-depth view (srcgan_s2d_shift; the
 * transposed one is cropped inside srcgan_prelu_forward); the two concatenations are one LR buffer of 5 nr and one HR buffer of 6 nr
 * channels that every module writes its slice of.  params / grads in parameters() order, which is registration order: sub_mean.{weight,
 * bias}, initial.{0.weight, 0.bias, 1.weight, 2.weight, 2.bias, 3.weight}, upmodules.<i>.[bottleneck.{0.weight, 0.bias, 1.weight},]
 * conv_<1..3>.{0.weight, 0.bias, 1.weight}, downmodules.<i>. likewise, reconstruction.0.{weight, bias}, add_mean.{weight, bias}.
 * MeanShift runs from its parameters and takes no gradient: grads[0], grads[1] and the last two must be NULL.
 * Refused: in_ch or out_ch != 3, scale not in {2, 4, 8}.  The infer entries are those of srcgan_rcan_infer. */
typedef struct srcgan_ddbpn_cfg {
    int in_ch, out_ch;
    int B, H, W;
    int dtype;
    int scale;
} srcgan_ddbpn_cfg;
int srcgan_ddbpn_num_params(const srcgan_ddbpn_cfg* c);
size_t srcgan_ddbpn_ws_bytes(const srcgan_ddbpn_cfg* c);
size_t srcgan_ddbpn_bwd_scratch_bytes(const srcgan_ddbpn_cfg* c);
int srcgan_ddbpn_forward(const srcgan_ddbpn_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_ddbpn_backward(const srcgan_ddbpn_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                          float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_ddbpn_infer_ws_bytes(const srcgan_ddbpn_cfg* c);
size_t srcgan_ddbpn_infer_act_bytes(const srcgan_ddbpn_cfg* c);
int srcgan_ddbpn_infer_plan(const srcgan_ddbpn_cfg* c, size_t* ranges, int cap);
int srcgan_ddbpn_infer(const srcgan_ddbpn_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);

/* RDN, the Residual Dense Network (reference src/model/rdn.py:45-105, arXiv 1802.08797): SFENet1 (3x3, n_colors -> G0) -> SFENet2 (3x3) ->
 * D residual dense blocks [ C x (3x3 + ReLU, G0 + c G -> G, on the concatenation of the block's input and all earlier layers), 1x1 LFF
 * (G0 + C G -> G0) + the block's input ] -> GFF.0 (1x1 over the concatenation of the D block outputs) -> GFF.1 (3x3) + SFENet1's output
 * -> UPNet (3x3 to r^2 G + PixelShuffle(r) for r = 2, 3; twice with r = 2 at scale 4) -> 3x3 to n_colors.
 * [B,n_colors,H,W] f32 NCHW -> [B,n_colors,H*scale,W*scale].  The reference's RDNconfig 'A' is (D, C, G) = (20, 6, 32), 'B' (16, 8, 64).
 * No concatenation is made: block d owns one buffer of G0 + C G channels whose layers read a prefix and write their slice, the LFF
 * writes the prefix of the next block's buffer, and GFF.0 runs as D 1x1 convolutions over K slices of its weight, one behind each
 * block, summing into two alternating G0-channel accumulators (in a 16-bit dtype the running sum is rounded D times where the
 * reference rounds once).  params / grads in parameters() order: SFENet1.{weight,bias}, SFENet2.*, RDBs.<d>.convs.<c>.conv.0.* for
 * c < C then RDBs.<d>.LFF.*, GFF.0.*, GFF.1.*, UPNet.0.*, UPNet.2.* and at scale 4 UPNet.4.*: 4 + D (2 C + 2) + 8 tensors, two more at
 * scale 4.  Refused: in_ch outside 1..8, scale not in {2, 3, 4}, D, C, G or G0 < 1, G0 or G no multiple of 32 (a slice starts at
 * G0 + c G and has to start a K chunk of the 16-bit types), G0 + C G > 8192.  The infer entries are those of srcgan_rcan_infer; the
 * activation part holds two dense buffers and a handful of G0-channel tensors and does not depend on D from 2 on. */
typedef struct srcgan_rdn_cfg {
    int in_ch;                  /* n_colors, also the output's channels */
    int B, H, W;
    int dtype;
    int scale;
    int G0, D, C, G;
} srcgan_rdn_cfg;
int srcgan_rdn_num_params(const srcgan_rdn_cfg* c);
size_t srcgan_rdn_ws_bytes(const srcgan_rdn_cfg* c);
size_t srcgan_rdn_bwd_scratch_bytes(const srcgan_rdn_cfg* c);
int srcgan_rdn_forward(const srcgan_rdn_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_rdn_backward(const srcgan_rdn_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                        float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_rdn_infer_ws_bytes(const srcgan_rdn_cfg* c);
size_t srcgan_rdn_infer_act_bytes(const srcgan_rdn_cfg* c);
int srcgan_rdn_infer_plan(const srcgan_rdn_cfg* c, size_t* ranges, int cap);
int srcgan_rdn_infer(const srcgan_rdn_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);

/* MDSR, the multi-scale EDSR (reference src/model/mdsr.py:13-66 with common.py, arXiv 1707.02921): sub_mean -> head (3x3, 3 -> F) ->
 * pre_process[idx] (two ResBlocks of 5x5 convolutions: conv + ReLU, conv, + the block's input) -> body (n_resblocks 3x3 ResBlocks and a
 * 3x3 convolution) + the pre_process output -> upsample[idx] (3x3 to r^2 F + PixelShuffle(r): r = 3 once, r = 2 once / twice / three
 * times for scale 2 / 4 / 8) -> tail (3x3, F -> 3) -> add_mean.  [B,3,H,W] f32 NCHW -> [B,3,H*s,W*s], s = scales[scale_idx].
 * One module, several graphs: pre_process and upsample exist once per entry of scales, and scale_idx says which pair the call runs.
 * params / grads hold ALL parameters in parameters() order (registration order, mdsr.py:22-23, 27, 41, 47-49): sub_mean.{weight,bias},
 * add_mean.*, pre_process.<i>.{0,1}.body.{0,2}.* for every i, upsample.<i>.{0[,2[,4]]}.* for every i, head.0.*, body.<k>.body.{0,2}.*,
 * body.<n_resblocks>.*, tail.0.*: 4 + 8 nscale + (2, 2, 4 or 6 per scale 2, 3, 4, 8) + 2 + 4 n_resblocks + 2 + 2 tensors.  The branches
 * off the graph cost nothing: their weights are not packed, they take no gradient pass and no zero fill, their entries of grads (and of
 * params) are never read and may be null, and every size query of {scales = {.., s, ..}, scale_idx -> s} equals that of {scales = {s},
 * scale_idx = 0}.  The MeanShift layers are frozen (their grads entries must be null).  Refused: in_ch or out_ch != 3, nscale outside
 * 1..4, a scale not in {2, 3, 4, 8}, scale_idx outside [0, nscale), n_feats no multiple of 16 or above 1024, n_resblocks < 1.  All ranks
 * of a data-parallel step must use the same scale_idx.  The 5x5 convolutions run on the generic implicit-GEMM kernel.
 *
 * VDSR (reference src/model/vdsr.py:13-45): sub_mean -> 3x3 (3 -> F) + ReLU -> n_resblocks - 2 times 3x3 (F -> F) + ReLU -> 3x3 (F -> 3)
 * + the sub_mean output -> add_mean.  [B,3,H,W] -> [B,3,H,W].  params / grads: sub_mean.*, add_mean.*, body.<k>.0.{weight,bias} for
 * k < n_resblocks: 4 + 2 n_resblocks tensors.  Refused: in_ch != 3, n_resblocks < 2, n_feats no multiple of 16 or above 1024.
 * The entry points of both families are those of srcgan_rcan_*. */
typedef struct srcgan_mdsr_cfg {
    int in_ch, out_ch;          /* both 3: MeanShift is a 3-channel convolution (common.py:16) */
    int B, H, W;
    int dtype;
    int n_resblocks, n_feats;
    int nscale;                 /* 1..4 */
    int scales[4];              /* each 2, 3, 4 or 8 (common.py:63-84) */
    int scale_idx;              /* the branch on the graph */
} srcgan_mdsr_cfg;
typedef struct srcgan_vdsr_cfg {
    int in_ch;                  /* 3, also the output's channels */
    int B, H, W;
    int dtype;
    int n_resblocks, n_feats;   /* n_resblocks >= 2 */
} srcgan_vdsr_cfg;
int srcgan_mdsr_num_params(const srcgan_mdsr_cfg* c);
size_t srcgan_mdsr_ws_bytes(const srcgan_mdsr_cfg* c);
size_t srcgan_mdsr_bwd_scratch_bytes(const srcgan_mdsr_cfg* c);
int srcgan_mdsr_forward(const srcgan_mdsr_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_mdsr_backward(const srcgan_mdsr_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                         float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_mdsr_infer_ws_bytes(const srcgan_mdsr_cfg* c);
size_t srcgan_mdsr_infer_act_bytes(const srcgan_mdsr_cfg* c);
int srcgan_mdsr_infer_plan(const srcgan_mdsr_cfg* c, size_t* ranges, int cap);
int srcgan_mdsr_infer(const srcgan_mdsr_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_vdsr_num_params(const srcgan_vdsr_cfg* c);
size_t srcgan_vdsr_ws_bytes(const srcgan_vdsr_cfg* c);
size_t srcgan_vdsr_bwd_scratch_bytes(const srcgan_vdsr_cfg* c);
int srcgan_vdsr_forward(const srcgan_vdsr_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_vdsr_backward(const srcgan_vdsr_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                         float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_vdsr_infer_ws_bytes(const srcgan_vdsr_cfg* c);
size_t srcgan_vdsr_infer_act_bytes(const srcgan_vdsr_cfg* c);
int srcgan_vdsr_infer_plan(const srcgan_vdsr_cfg* c, size_t* ranges, int cap);
int srcgan_vdsr_infer(const srcgan_vdsr_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);

/* nn.ReflectionPad2d and nn.Tanh (csrc/reflect_pad.hip), NHWC, channel stride *_cs elements, all three dtypes: 16-byte accesses along the
 * channels when C, strides and bases allow them, element by element otherwise; 64-bit addresses, no atomics, every output element
 * written exactly once.
 *   srcgan_reflect_pad_nhwc:     y [B, H+2p, W+2p, C], y[i][j] = x[r(i, H)][r(j, W)], r(i, H) = p - i for i < p, 2 (H-1) - (i - p) for
 *                                i >= H + p, i - p otherwise.  Refused before the launch: p < 1, p >= H, p >= W.
 *   srcgan_reflect_pad_bwd_nhwc: the adjoint as a gather: dx[i][j] = sum of dy over R(i, H) x R(j, W); R(i, H) holds i + p, p - i when
 *                                1 <= i <= p, and p + 2 (H-1) - i when H-1-p <= i <= H-2 (up to 9 terms on a small image).  Summed in f32,
 *                                rows outer, ascending index; accumulate != 0: the old dx is added last; rounded once.
 *   srcgan_tanh_forward:         y = tanh(z), computed in f32, on npix records of C channels.
 *   srcgan_tanh_backward:        dz = dy (1 - y^2) from the saved y; accumulate != 0: added to the old dz (last), rounded once. */
int srcgan_reflect_pad_nhwc(const void* x, int x_cs, void* y, int y_cs, int B, int H, int W, int C, int p, int dtype, void* stream);
int srcgan_reflect_pad_bwd_nhwc(const void* dy, int dy_cs, void* dx, int dx_cs, int B, int H, int W, int C, int p, int accumulate, int dtype, void* stream);
int srcgan_tanh_forward(const void* z, int z_cs, void* y, int y_cs, long npix, int C, int dtype, void* stream);
int srcgan_tanh_backward(const void* dy, int dy_cs, const void* y, int y_cs, void* dz, int dz_cs, long npix, int C, int accumulate, int dtype, void* stream);

/* ResnetGenerator (reference src/model/basicModel.py:141-254, the translator of multi-task.py's define_G(.., 'resnet_9blocks', 'instance'))
 * with InstanceNorm2d (no parameters) and use_bias = True: ReflectionPad2d(3) -> 7x7 (in -> ngf) -> IN -> ReLU -> two 3x3 s2 p1
 * (ngf -> 2 ngf -> 4 ngf), each IN + ReLU -> n_blocks x [pad 1, 3x3 p0, IN, ReLU, pad 1, 3x3 p0, IN, + the block's input] -> two
 * ConvTranspose2d(k3, s2, p1, output_padding 1) (4 ngf -> 2 ngf -> ngf), each IN + ReLU -> ReflectionPad2d(3) -> 7x7 (ngf -> out) -> tanh.
 * [B,in_ch,H,W] f32 NCHW -> [B,out_ch,H,W].  The padded tensors are materialised (srcgan_reflect_pad_nhwc) and the convolutions behind
 * them run with pad 0.  padding = 0: 'reflect'; 1: 'zero' (the block convolutions take pad 1, their pad ops drop out; the pads around
 * the 7x7 layers stay).  params / grads in parameters() order: every convolution's {weight, bias}: 2 (6 + 2 n_blocks) tensors.
 * Refused: H or W no multiple of 4 or below 8 (the quarter-resolution pad 1 needs two pixels; an odd size gives the reference another
 * output size), ngf no multiple of 16, in_ch or out_ch outside 1..8, n_blocks < 0, padding not 0 / 1.  Entry points as srcgan_rcan_*. */
typedef struct srcgan_resnetgen_cfg {
    int in_ch, out_ch;
    int B, H, W;
    int dtype;
    int ngf, n_blocks;
    int padding;                /* 0 = 'reflect', 1 = 'zero' */
} srcgan_resnetgen_cfg;
int srcgan_resnetgen_num_params(const srcgan_resnetgen_cfg* c);
size_t srcgan_resnetgen_ws_bytes(const srcgan_resnetgen_cfg* c);
size_t srcgan_resnetgen_bwd_scratch_bytes(const srcgan_resnetgen_cfg* c);
int srcgan_resnetgen_forward(const srcgan_resnetgen_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_resnetgen_backward(const srcgan_resnetgen_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                              float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_resnetgen_infer_ws_bytes(const srcgan_resnetgen_cfg* c);
size_t srcgan_resnetgen_infer_act_bytes(const srcgan_resnetgen_cfg* c);
int srcgan_resnetgen_infer_plan(const srcgan_resnetgen_cfg* c, size_t* ranges, int cap);
int srcgan_resnetgen_infer(const srcgan_resnetgen_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);

/* The U-Net's skip connection without a concatenation (csrc/unet_skip.hip), NHWC, channel strides *_cs elements, all three dtypes, 64-bit
 * addresses, no atomics, every output element written exactly once.
 *   srcgan_in_skip_forward: InstanceNorm2d without an affine part, two activated outputs from one read of the normalised value z:
 *                           a = LeakyReLU(z, slope), dense; r = ReLU(z) into channels [r_coff, r_coff + C) of a buffer of r_cs channels.
 *                           The statistics are srcgan_gn_forward's with G == C (the same kernels): a and r have the bits of that entry with
 *                           (relu = 1, slope) and (relu = 1, 0), stats [B][C]{mean, rstd} is its saved layout (srcgan_gn_backward serves),
 *                           scratch is srcgan_gn_scratch_floats(B, C).  16-byte accesses: C, strides and r_coff multiples of 4 (f32) / 8.
 *   srcgan_relu_nhwc:       y[.., y_coff : y_coff + C] = max(x, 0) on npix records; 16-byte accesses where C, strides and bases allow them,
 *                           element by element otherwise. */
int srcgan_in_skip_forward(const void* x, int x_cs, void* a, int a_cs, void* r, int r_cs, int r_coff, float* stats, int B, long hw, int C,
                           float eps, float slope, int dtype, float* scratch, void* stream);
int srcgan_relu_nhwc(const void* x, int x_cs, void* y, int y_cs, int y_coff, long npix, int C, int dtype, void* stream);

/* UnetGenerator (reference src/model/basicModel.py:257-354) with InstanceNorm2d (no parameters) and use_bias = True.  Levels l = 1 (outermost)
 * .. n = num_downs, widths C_l = ngf min(2^(l-1), 8).  Down: d_1 = conv4x4 s2 p1 (in -> C_1), d_l = IN(conv4x4 s2 p1(LeakyReLU(d_{l-1}, 0.2))),
 * the innermost d_n without the IN.  Up: u_{n-1} = IN(deconv(ReLU(d_n))), u_{l-1} = IN(deconv([ReLU(d_l) | ReLU(u_l)])), deconv =
 * ConvTranspose2d(k4, s2, p1); y = tanh(deconv([ReLU(d_1) | ReLU(u_1)]) (2 C_1 -> out)).  [B,in_ch,H,W] f32 NCHW -> [B,out_ch,H,W].
 * The skip [ReLU(d_l) | ReLU(u_l)] is one 2 C_l-channel buffer written in place by its two producers; nothing is concatenated.
 * params / grads in parameters() order: the down convolutions' {weight, bias} outermost first, then the transposed convolutions'
 * innermost first: 4 num_downs tensors.  Refused: num_downs < 5, H or W no positive multiple of 2^num_downs, ngf not 16, 32, 64 or 128
 * (a multiple of 16 whose widths InstanceNorm's kernels take), in_ch or out_ch outside 1..8.  Entry points as srcgan_resnetgen_*. */
typedef struct srcgan_unet_cfg {
    int in_ch, out_ch;
    int B, H, W;
    int dtype;
    int ngf, num_downs;
} srcgan_unet_cfg;
int srcgan_unet_num_params(const srcgan_unet_cfg* c);
size_t srcgan_unet_ws_bytes(const srcgan_unet_cfg* c);
size_t srcgan_unet_bwd_scratch_bytes(const srcgan_unet_cfg* c);
int srcgan_unet_forward(const srcgan_unet_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);
int srcgan_unet_backward(const srcgan_unet_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                         float* const* grads, float* dx_nchw, void* stream);
size_t srcgan_unet_infer_ws_bytes(const srcgan_unet_cfg* c);
size_t srcgan_unet_infer_act_bytes(const srcgan_unet_cfg* c);
int srcgan_unet_infer_plan(const srcgan_unet_cfg* c, size_t* ranges, int cap);
int srcgan_unet_infer(const srcgan_unet_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* stream);

/* Kernels of the frozen VGG feature path, NHWC, channel stride *_cs elements, all three dtypes (16-byte accesses along the channels
 * when strides and bases allow them, element by element otherwise).
 *   srcgan_maxpool2_nhwc:     nn.MaxPool2d(2, 2), ceil_mode = False: [B,H,W,C] -> [B,H/2,W/2,C]; an odd last row / column is dropped.
 *   srcgan_maxpool2_bwd_nhwc: dx = its gradient.  The argmax is recomputed from x (no index tensor): the first maximum of a window in
 *                             the order (0,0), (0,1), (1,0), (1,1) takes dy (torch's strict >).  Channels [0,C) of EVERY pixel of dx are
 *                             written exactly once (a dropped row / column gets zeros): no memset, no atomics.  relu_mask = 1: x is a
 *                             post-ReLU activation and dx is the gradient w.r.t. its pre-activation (zero where the maximum is not > 0).
 *   srcgan_feat_loss_fwd:     out_sum[0] = sum over npix pixels and channels [0,C) of |a - b| (kind 0) or (a - b)^2 (kind 1), accumulated
 *                             in f32 in two stages of fixed order (deterministic).  scratch: srcgan_loss_scratch_floats() floats.
 *   srcgan_feat_loss_bwd:     g = (accumulate ? g : 0) + scale * sign(a - b) (kind 0, sign(0) = 0) or scale * 2 (a - b) (kind 1). */
int srcgan_maxpool2_nhwc(const void* src, int s_cs, void* dst, int d_cs, int B, int H, int W, int C, int dtype, void* stream);
int srcgan_maxpool2_bwd_nhwc(const void* dy, int dy_cs, const void* x, int x_cs, void* dx, int dx_cs, int B, int H, int W, int C,
                             int relu_mask, int dtype, void* stream);
int srcgan_feat_loss_fwd(int kind, const void* a, int a_cs, const void* b, int b_cs, long npix, int C, int dtype,
                         float* out_sum, float* scratch, void* stream);
int srcgan_feat_loss_bwd(int kind, const void* a, int a_cs, const void* b, int b_cs, void* g, int g_cs, int accumulate, float scale,
                         long npix, int C, int dtype, void* stream);

/* Perceptual losses on a frozen VGG feature extractor (reference src/losses.py:344-393, 455-470), on the op-list executor.
 *   kind 0: VGG16Loss -- torchvision vgg16.features[0:23] (ten 3x3 convolutions + ReLU, three max-pools); the loss is the mean over
 *           the taps relu1_2, relu2_2, relu3_3, relu4_3 of the L1 mean between the two branches' features.
 *   kind 1: PerceptionLoss -- vgg19.features[0:35]: sixteen convolutions, four max-pools, ending at conv5_4 WITHOUT its ReLU; one tap,
 *           MSE.  H, W >= 16 (kind 0: >= 8).
 * The images of a call are frames of 5-D tensors (losses.VGG16Loss3D, reference src/losses.py:396-453; a [B, C_in, H, W] tensor is
 * F = 1, f0 = 0, k = 1 with c->B = B).  out5d / tgt5d / dout5d: contiguous f32 [Bt, C_in, F, H, W] with C_in = 1 or 3.  A call covers
 * the k frames [f0, f0 + k) as c->B = Bt * k images (image j * Bt + b = frame f0 + j of sample b): the input pack reads the frames in
 * place, and the input-gradient store writes them in place -- every element of those k frames of dout5d exactly once, other frames
 * untouched.  C_in = 1: the plane is replicated to the three VGG channels inside the pack and the three channel gradients are summed
 * into the one plane (what autograd does for the reference's torch.cat).
 * params: weight, bias of every convolution in order (f32, canonical layout); frozen: there are no parameter gradients.  forward keeps
 * the output branch's activations in ws (the target branch runs on a slot-planned region that retains only its taps) and writes the
 * loss, the mean over the k frames of the per-frame loss, to loss_out (device f32); backward writes d loss / d out * gout_dev[0] *
 * gscale to dout5d.  Inside the backward gradients travel at unit scale (tap k contributes sign(a - b) * N_1 / N_k, resp. 2 (a - b));
 * the factor 1 / (ntaps * N_1) is applied in the final f32 store, so 16-bit gradients do not underflow at training sizes.
 * infer: the same loss value (same launches, same bits) with both branches on slot-planned regions, for no_grad. */
typedef struct srcgan_vggloss_cfg {
    int kind;
    int B, H, W;
    int dtype;
} srcgan_vggloss_cfg;
int srcgan_vggloss_num_params(const srcgan_vggloss_cfg* c);
size_t srcgan_vggloss_ws_bytes(const srcgan_vggloss_cfg* c);
size_t srcgan_vggloss_bwd_scratch_bytes(const srcgan_vggloss_cfg* c);
size_t srcgan_vggloss_infer_ws_bytes(const srcgan_vggloss_cfg* c);
int srcgan_vggloss_forward_frames(const srcgan_vggloss_cfg* c, const float* out5d, const float* tgt5d, int C_in, int F, int f0, int k,
                                  const float* const* params, void* ws, float* loss_out, void* stream);
int srcgan_vggloss_backward_frames(const srcgan_vggloss_cfg* c, const float* gout_dev, float gscale, int C_in, int F, int f0, int k,
                                   const float* const* params, void* ws, void* scratch, float* dout5d, void* stream);
int srcgan_vggloss_infer_frames(const srcgan_vggloss_cfg* c, const float* out5d, const float* tgt5d, int C_in, int F, int f0, int k,
                                const float* const* params, void* ws, float* loss_out, void* stream);

/* nn.PixelShuffle(r) on NHWC (espcn.py:44,50): src [B,H,W,C*r*r] -> dst [B,H*r,W*r,C]; inverse = 1: the adjoint, src [B,H*r,W*r,C]
 * -> dst [B,H,W,C*r*r].  srcgan_mask_inplace: g *= (act > 0 ? 1 : slope) over n elements (ReLU' / LeakyReLU' on an incoming gradient). */
int srcgan_pixel_shuffle_nhwc(const void* src, int s_cs, void* dst, int d_cs, int B, int H, int W, int C, int r, int inverse,
                              int dtype, void* stream);
int srcgan_mask_inplace(void* g, const void* act, float slope, long n, int dtype, void* stream);

/* Evaluation metrics on device (metrics.py:10-144; test loop testCas.py:65-90).  pred / truth: [B,C,H,W] f32 NCHW.
 *   srcgan_metric_ae:   out[b] = mean over pixels of acos(<p,t>/(|p||t| + 1e-6)) in degrees
 *   srcgan_metric_ssim: out[b][0] = mean SSIM (11x11 gaussian sigma 1.5 "valid" windows, dynamic range from the prediction's
 *                       min / max as metrics.py:100-107), out[b][1] = mean contrast term
 * MSE / PSNR: srcgan_loss_fwd(kind 1) + srcgan_psnr_from_mse.  scratch: srcgan_metric_scratch_floats(B, C, H, W) floats.
 * Pinned by tests/test_gpu_metrics_kernels.py:
 *   - srcgan_metric_ae: the value of the formula as written, 1e-6 included, per image: 60, 90 and 180 degree pixels, a zero prediction
 *     and two zero pixels (both 90 degrees) in any mix; pred == truth gives about 0.1 degrees, not 0 (the quotient is 1 - 1e-6 / |p|^2);
 *     hw = 1, less than a block, one short of and one past 64 blocks of 256.  Within 4 x the error of a float32 restatement.
 *   - srcgan_metric_ssim: out[b][0] and out[b][1] are image b's own means (a block of unrelated values in one image does not reach the
 *     other), every window position counted once wherever the block sits: corners, edges, the 16-position tile seam, the last ragged
 *     tile.  The dynamic range comes from the whole prediction: max > 128 (128.0 itself does not count) -> 255, min < -0.5 (-0.5 itself
 *     does not) -> floor -1.  Nothing outside out[0 .. 2B) is written; no scratch slot is read before it is written. */
int srcgan_metric_scratch_floats(int B, int C, int H, int W);
int srcgan_metric_ae(const float* pred, const float* truth, int B, int C, int H, int W, float* out, float* scratch, void* stream);
int srcgan_metric_ssim(const float* pred, const float* truth, int B, int C, int H, int W, float* out, float* scratch, void* stream);

/* DSSIM training loss (losses.py:170-196, DSSIMLoss and DSSIMLoss3D): the mean over frames f of (1 - SSIM(pred_f, truth_f)) / 2 with the
 * metric's SSIM (11x11 gaussian sigma 1.5 "valid" depth-wise windows), each frame with the dynamic range of its own prediction (min /
 * max over all B*C planes of that frame), as the reference's loop over frames has it.  pred / truth / dpred / dtruth: contiguous f32
 * [B,C,F,H,W], a [B,C,H,W] tensor being F = 1; plane (b, c) of frame f starts at element ((b*C + c)*F + f)*H*W (64-bit offsets);
 * H, W >= 11; B*C and F at most 65535.
 *   srcgan_dssim3d_loss_fwd: out[0] = the loss (a device scalar); range[f][0..1] = min / max of frame f of pred (device, 2 F floats),
 *                            which backward reads; scratch: srcgan_dssim3d_scratch_floats(B, C, F, H, W) floats (0 for a refused
 *                            shape).  One range launch, one tile launch and one f64 fold cover all frames; no per-frame copy, no host
 *                            synchronisation.
 *   srcgan_dssim3d_loss_bwd: dpred = gout[0] * dloss/dpred, dtruth = gout[0] * dloss/dtruth (overwritten); gout is a device scalar,
 *                            which enters as gout[0] * (1.0f / F), range the buffer the forward wrote for the same inputs.  dtruth may
 *                            be NULL (no target gradient).  One fused pass per 32x32 output tile; deterministic (every element
 *                            written once, no atomics).
 * The gradient of frame f has the bits of a one-frame backward of that frame at upstream gout[0] * (1.0f / F).
 * Pinned by tests/test_gpu_metrics_kernels.py:
 *   - srcgan_dssim3d_loss_bwd: EVERY element of dpred and dtruth is within K * 2^-24 * N(q) of float64 autograd, N(q) the gradient's own
 *     expression with every term replaced by its absolute value (it shrinks at the border as the gradient does: the corner pixel, covered
 *     by one window position with weight w[0]^2, is held as tightly as an interior one); K = 195 is 4 x what a float32 restatement
 *     loses.  Shapes from one window position (11x11) to 2x3 output tiles with ragged edges, strips, two planes, two channels, two
 *     frames of different range, L = 2, near-constant windows and SSIM near 1; with dtruth and with dtruth == NULL.  Every element of
 *     the outputs is written and nothing around them; pred, truth and gout are not written.
 *   - srcgan_dssim3d_loss_fwd: range[f] = (amin, amax) of frame f of pred, exactly, wherever the extremes sit (first and last element,
 *     index 255 and 256, the last plane; more than 256 * 256 elements per frame); the loss counts every window position once (the
 *     probes of srcgan_metric_ssim, also in one frame of two) and follows the range rule at its thresholds (see srcgan_metric_ssim). */
long srcgan_dssim3d_scratch_floats(int B, int C, int F, int H, int W);
int srcgan_dssim3d_loss_fwd(const float* pred, const float* truth, int B, int C, int F, int H, int W, float* out, float* range,
                            float* scratch, void* stream);
int srcgan_dssim3d_loss_bwd(const float* pred, const float* truth, int B, int C, int F, int H, int W, const float* range,
                            const float* gout, float* dpred, float* dtruth, void* stream);

/* Registration-tolerant pixel loss (losses.py:199-255, NearestSelector; with L1Loss at :522).  output / target: [B,C,H,W] f32 NCHW,
 * contiguous.  n = 2 * shift; candidate k = i * n + j compares output[:, :, sd : sd + crop_h, sd : sd + crop_w] (sd = shift * stride)
 * with target[:, :, i * stride : i * stride + crop_h, j * stride : j * stride + crop_w] (crop_h = H - 2 sd, crop_w = W - 2 sd in the
 * loss; any crop that keeps every window inside the image is accepted).
 *   srcgan_shift_search: diff[b][k] = sum over c, y, x of |target window - output crop| (f32 [B, n*n]); sel[b] = (k* / n, k* % n) of the
 *                        FIRST minimum k* (int32 [B, 2]); loss (may be NULL) = sum_b diff[b][k*] / (B C crop_h crop_w), a device scalar.
 *                        One pass over both tensors, no atomics, fixed summation order: two calls give the same bits.
 *                        scratch: srcgan_shift_search_scratch_floats(...) floats (0 and an error string when the configuration is refused).
 *                        Refused with an error string: shift > 4 (the n*n sums are kept in registers), a target window (tile + (n-1) *
 *                        stride apron) that does not fit in LDS, an empty crop, a window that leaves the image.
 *   srcgan_shift_gather: dst[b] = target[b, :, r*stride : r*stride + crop_h, c*stride : c*stride + crop_w] with (r, c) = sel[b] read on
 *                        the device ([B,C,crop_h,crop_w] f32, a bit-exact copy).
 *   srcgan_shift_l1_bwd: gradients of mean |output crop - selected target window|, full size [B,C,H,W] f32, overwritten: doutput =
 *                        sign(o - t') * gout[0] * (1 / (float)N) inside the crop (N = B C crop_h crop_w, sign(0) = 0; the expression of
 *                        srcgan_loss_bwd) and 0 on the border; dtarget (may be NULL) = -sign * g at each sample's window, 0 elsewhere. */
size_t srcgan_shift_search_scratch_floats(int B, int C, int H, int W, int shift, int stride, int crop_h, int crop_w);
int srcgan_shift_search(const float* output, const float* target, int B, int C, int H, int W, int shift, int stride, int crop_h,
                        int crop_w, float* diff, int* sel, float* loss, float* scratch, void* stream);
int srcgan_shift_gather(const float* target, const int* sel, int B, int C, int H, int W, int shift, int stride, int crop_h, int crop_w,
                        float* dst, void* stream);
int srcgan_shift_l1_bwd(const float* output, const float* target, const int* sel, int B, int C, int H, int W, int shift, int stride,
                        int crop_h, int crop_w, const float* gout, float* doutput, float* dtarget, void* stream);

/* Space-to-depth forms of an image-channel tensor for a 4x4 stride-2 pad-1 first layer (NLayerDiscriminator, model/model.py:612):
 * block (j,i) of the (H/2+1) x (W/2+1) grid = the 2x2 pixels (2j-1+dy, 2i-1+dx) as a 32-channel record [dy][dx][8], zero
 * outside the image / past C; the layer becomes a 2x2 stride-1 convolution with K = 4 x 32 and no padded K.
 * srcgan_s2d_wgrad_unfold maps the gradient of the folded weight [Cout][32][2][2] to the canonical [Cout][Cin][4][4]. */
int srcgan_nchw_f32_to_s2d(const float* src, void* dst, int B, int C, int H, int W, int dtype, void* stream);
int srcgan_s2d_to_nchw_f32(const void* src, float* dst, int B, int C, int H, int W, int dtype, void* stream);
int srcgan_s2d_wgrad_unfold(const float* gfold, float* grad, int Cout, int Cin, int accumulate, void* stream);

/* Input pipeline colour conversions on device (dataset.py:114-159 behind G2RGB / G2LAB.__getitem__ :179-199,:234-254; the
 * reference calls skimage.color per sample on the host).  rgb: [B,H*W,3] interleaved 8-bit; dst: f32 planes [B,C,H*W].
 *   mode 0: gray = rgb2gray(rgb)                               C = 1   (_arr2gray)
 *   mode 1: rgb / 255                                          C = 3   (_arr2rgb)
 *   mode 2: (L/100, (a+128)/255, (b+128)/255) of rgb2lab(rgb)  C = 3   (_arr2lab)
 *   mode 3: ((a+128)/255, (b+128)/255)                         C = 2   (_arr2ab)
 * srcgan_lab_planes_to_u8rgb is the inverse used for visualisation (_lab2img, dataset.py:92-104; truncating store). */
int srcgan_u8rgb_to_planes(const unsigned char* rgb, float* dst, int B, long hw, int mode, void* stream);
int srcgan_lab_planes_to_u8rgb(const float* lab, unsigned char* rgb, int B, long hw, void* stream);

/* ---- whole-scene inference: tile gather / write-back (csrc/tiles.hip, srcgan_amd/infer.py) ----
 * A scene stays on the device; tiles of ONE common shape are gathered into an NCHW f32 batch, the network runs on the batch, and its
 * HR tiles are written back.  Tile origins and rectangles are HOST arrays: they travel in the kernel arguments (no device allocation,
 * no host-to-device copy), chunked internally when T exceeds what one launch carries.
 *
 * srcgan_tile_gather: dst[t][c][ty][tx] = scene(c, min(y0_t + ty, H - 1), min(x0_t + tx, W - 1)) -- a tile that passes the right /
 *   bottom edge is filled by edge replication and nothing outside the scene is read.  src_u8 = 1: the scene is u8 HWC (C = 1 or 3),
 *   mapped v / 255 exactly as srcgan_u8rgb_to_planes mode 1; src_u8 = 0: f32 planes [C][H][W], C <= 8.  origins_yx: T pairs (y0, x0)
 *   inside the scene.  16-byte accesses along W where tw, the origin, W and the pointers allow, scalar otherwise (same bits).
 * srcgan_tile_scatter: tiles [T][C][th*up][tw*up] -> scene [C][H*up][W*up].  rects: 10 ints per tile, in LR pixels:
 *   y0, x0 (tile origin), sy0, sy1, sx0, sx1 (the write-back rectangle: inside the tile and inside the scene, so the replicated
 *   excess of a tile is dropped), ny_lo, ny_hi, nx_lo, nx_hi (ramp lengths at the low / high end of the rectangle).
 *   feather = 0: scene = tile on the rectangle (rectangles must be disjoint; ramps must be 0).
 *   feather = 1: scene = fma(wy * wx, tile, scene); w = (j + 0.5) / n rising over a low ramp of n HR pixels, 1 - (j + 0.5) / n over a
 *   high ramp, 1 between (f32).  The caller zeroes the scene first.  No atomics: one launch per tile, so a pixel receives its
 *   contributions in tile order on `stream` and the result is bitwise reproducible.
 * srcgan_planes_to_u8hwc: dst[px][c] = floor(clamp(src[c][px], 0, 1) * 255) -- the reference's tensor2image for in-range values;
 *   out-of-range values saturate instead of wrapping.  C <= 8. */
int srcgan_tile_gather(const void* src, int src_u8, int C, int H, int W, float* dst, int T, int th, int tw,
                       const int* origins_yx, void* stream);
int srcgan_tile_scatter(const float* tiles, float* dst, int C, int H, int W, int up, int T, int th, int tw,
                        const int* rects, int feather, void* stream);
int srcgan_planes_to_u8hwc(const float* src, unsigned char* dst, int C, long hw, void* stream);

/* ---- cascade inference without scene-sized f32 intermediates (infer.py cascade_scene) ----
 * srcgan_tile_gather_ex: srcgan_tile_gather of a scene that is converted and up-sampled while it is read.
 *   src_kind 0: f32 planes [C][H][W], C <= 8; 1: u8 HWC (C = 1 or 3), v / 255; 2: u8 [H][W][3] -> ONE gray plane, the arithmetic of
 *   srcgan_u8rgb_to_planes mode 0 (C = 3 is the source's channel count; dst holds one plane per tile).
 *   s >= 1: dst[t][c][ty][tx] = U(c, min(y0_t + ty, H s - 1), min(x0_t + tx, W s - 1)), U = the converted scene up-sampled s times
 *   bilinearly (align_corners = False) exactly as srcgan_bilinear_up computes it; s = 1: no interpolation.  Origins are on the
 *   up-sampled grid, inside [0, H s) x [0, W s).  Every sample is evaluated from in-scene reads by the device functions the
 *   materialising kernels use, so the result is bit-identical to srcgan_tile_gather of the materialised scene; with s = 1 and
 *   src_kind 0 / 1 the call IS srcgan_tile_gather.
 * srcgan_tile_scatter_u8: crop-mode write-back into an 8-bit RGB scene dst [H*up][W*up][3], the conversion fused into the store.
 *   rects as srcgan_tile_scatter (disjoint rectangles, ramps 0).  mode 0: tiles_a [T][3][th*up][tw*up] RGB planes, tiles_b NULL,
 *   Cb = 0; bytes as srcgan_planes_to_u8hwc.  mode 1: tiles_a [T][1][..] the L plane, tiles_b [T][2][..] the chroma planes (normalised
 *   LAB); bytes as srcgan_lab_planes_to_u8rgb.  Aligned 12-byte stores of 4 pixels in the interior of a rectangle row, byte stores at
 *   its ends; no read-modify-write, no atomics, any W. */
int srcgan_tile_gather_ex(const void* src, int src_kind, int C, int H, int W, int s, float* dst, int T, int th, int tw,
                          const int* origins_yx, void* stream);
int srcgan_tile_scatter_u8(const float* tiles_a, int Ca, const float* tiles_b, int Cb, unsigned char* dst_u8hwc, int H, int W, int up,
                           int T, int th, int tw, const int* rects, int mode, void* stream);

/* ---- geometric self-ensemble: the D4 views of a tile and their fold (infer.py upscale_scene / cascade_scene, ensemble=) ----
 * op = 0..7 numbers the dihedral group of the square: t = op & 1 (transpose), fy = (op >> 1) & 1 (mirror the view's rows), fx =
 * (op >> 2) & 1 (mirror its columns).  The view of a window win[th][tw] is [Hv][Wv] = [tw][th] if t, else [th][tw], and
 *   view[y][x] = win[a][b],  y' = fy ? Hv - 1 - y : y,  x' = fx ? Wv - 1 - x : x,  (a, b) = t ? (x', y') : (y', x').
 * op 0 identity, 2 np.flipud, 4 np.fliplr, 6 rot180, 1 transpose, 3 np.rot90(k=1), 5 np.rot90(k=3), 7 anti-transpose.
 * srcgan_tile_gather_d4: dst[t][c] = the `op` view of exactly the window srcgan_tile_gather_ex returns -- the same kinds, the same
 *   conversion, up-sampling and clamping, every sample evaluated by the same device functions, so the bits are those of transforming
 *   srcgan_tile_gather_ex's output and op = 0 IS srcgan_tile_gather_ex.  th, tw are the window's extents whatever op is.  A mirrored
 *   row is read forwards as the segment it mirrors and reversed in registers; a transposition stages 32 x 32 blocks through LDS
 *   (pitch 33 dwords, conflict-free on both sides), so scene reads and tile writes both run along W.  16-byte stores where th, tw
 *   and dst allow, scalar otherwise (same bits).
 * srcgan_d4_accumulate: the same mapping read in the other direction.  acc is [planes][ah][aw] in identity orientation, view is
 *   [planes][Hv][Wv], (Hv, Wv) = op & 1 ? (aw, ah) : (ah, aw):
 *     acc[a][b] = ((first ? 0 : acc[a][b]) + view[y][x]) * scale      in f32: one addition, one multiplication, never contracted;
 *   `first` != 0 does not read acc.  An ensemble of V views calls it V times in op order, first = 1 on the first and scale = 1 / V
 *   on the last (1 elsewhere; V is a power of two, so the scale is exact).  view must not overlap acc.  16-byte accesses where ah,
 *   aw and both pointers allow, scalar otherwise (same bits); the same LDS transposition for op & 1.
 * Both validate before launching (null pointers, op outside 0..7, C / kind combinations, extents over 16384 per side, origins
 * outside the grid, a non-finite scale, aliasing) and write nothing on error. */
int srcgan_tile_gather_d4(const void* src, int src_kind, int C, int H, int W, int s, float* dst, int T, int th, int tw,
                          const int* origins_yx, int op, void* stream);
int srcgan_d4_accumulate(const float* view, float* acc, long planes, int ah, int aw, int op, int first, float scale, void* stream);

/* ---- whole-scene scoring (csrc/scene_score.hip, metrics.py score_scene) ----
 * MSE, PSNR, AE, SSIM and CS of metrics.py:10-144 for ONE image pair of any size, in one pass and without scene-sized intermediates.
 *   pred / truth: kind 0 = f32 planes [C][H][W] (taken as is), kind 1 = u8 [H][W][C] (v / 255 as srcgan_tile_gather kind 1; any byte
 *   alignment of the base and of W * C).  C = 1 or 3; H, W >= 11.  The SSIM dynamic range follows the prediction: 1 for a u8
 *   prediction, from a stream-ordered min / max pass for an f32 one.
 *   srcgan_scene_score_tile:     T, the edge of a workgroup's tile of SSIM positions (host only).
 *   srcgan_scene_score_ws_bytes: workspace size (host only); 0 and srcgan_last_error() for bad arguments.  16 bytes per tile plus
 *                                a fixed part of at most 8 KiB: at most H * W * C / 16 for scenes of 256 x 256 and more.
 *   srcgan_scene_score:          out5 (device, 5 doubles) = MSE, PSNR (+inf for MSE 0), AE in degrees, SSIM, CS.  One tile kernel
 *                                + a two-stage f64 fold of fixed order: bitwise reproducible, no atomics, no host synchronisation.
 *                                workspace: 16-byte aligned device memory of ws_bytes. */
int srcgan_scene_score_tile(void);
size_t srcgan_scene_score_ws_bytes(long H, long W, int C);
int srcgan_scene_score(const void* pred, int pred_kind, const void* truth, int truth_kind, long H, long W, int C,
                       double* out5, void* workspace, void* stream);

/* Fused multi-tensor Adam (torch.optim.Adam.step() of trainCas.py:38-41,143-150 / train.py:191-192,331-340; torch's
 * single-tensor arithmetic, default flags: no weight decay, no amsgrad).  tensors_dev: device array of records
 * {float* p; const float* g; float* m; float* v;} (32 bytes; p, m and v 16-byte aligned, g 4-byte aligned is enough --
 * srcgan_amd.optim.Adam sends anything else through torch's own step); chunks_dev: device array of nchunks records
 * {int tensor; int off; int n; int pad;} (16 bytes; off a multiple of 4, n <= 4096).  `step` = the 1-based step count of
 * every tensor in the launch. */
int srcgan_adam_step(const void* tensors_dev, const void* chunks_dev, int nchunks, double lr, double beta1, double beta2, double eps,
                     long step, void* stream);

/* ---------------------------------------------------------------------------
 * Launch profiling for bench.py: when enabled, every conv_igemm / conv_wgrad launch is bracketed by
 * HIP events on its launch stream.  collect() synchronises, aggregates per kernel class
 * (template instance) and returns the number of classes; get(i) reads one aggregate:
 * launches, total ms, total algorithmic flop and bytes.
 * ------------------------------------------------------------------------- */
int srcgan_prof_enable(int on);
int srcgan_prof_collect(void);
int srcgan_prof_get(int i, const char** cls, long* count, double* ms, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* SRCGAN_AMD_H */
