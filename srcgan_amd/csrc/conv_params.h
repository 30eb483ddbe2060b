// Shared by the convolution kernels and their entry (conv_entry.hip): the launch parameters, tensor addressing and the kernel
// families' entry points.  The fused epilogues are in conv_epilogue.h.
#pragma once
#include "common.h"

// Tensor addressing: byte offset of channel c of pixel index q = q*pix + (c / KCE)*plane + (c % KCE)*sizeof(T), KCE = the
// 64-byte channel chunk.  Interleaved NHWC is pix = Cs*sizeof(T), plane = 64; the "blocked" layout used for the
// dense-block buffers is pix = 64, plane = npixels*64 (each 64-byte chunk of every pixel contiguous across pixels:
// operand fetches become >=128-byte contiguous; measured 3.4 TB/s -> 6.7 TB/s LDS-DMA ingest, scripts/hip/dma_stream_test.hip).
struct ConvP {
    const void* x; const void* wp; const float* bias; void* y;
    const void* r1; const void* r2; const void* mz;
    int B, H, W, Cin, xcoff;
    int OH, OW, Cout, YH, YW, ycoff;
    int pad_y, pad_x, os, oa, ob;
    int r1coff, r1cend, r2coff, r2cend, mzcoff, mzc0;
    long xpix, xplane, ypix, yplane, r1pix, r1plane, r2pix, r2plane, mzpix, mzplane;     // bytes
    float alpha, beta1, beta2, slope, mslope;
    int act, vec, nchunk, tiles_x, tiles_y, ctiles;
    int vec16;    // every epilogue tensor allows 16-byte accesses per lane (LDS-transposed epilogue)
    int buf16;    // vec16, and every epilogue tensor's channel plane is below 2 GiB: the row epilogue's 32-bit buffer offsets (conv_epilogue_lds_row)
    int rev;      // images are walked last to first
    long wpar;    // dgrad_s2k4 (conv_par4.hip) and the four-parity 1x1 form: bytes between the packs of consecutive output parities
    int npar;     // conv_igemm_k: 4 = the channel-tile index also selects an output parity (oa, ob) = (par >> 1, par & 1) and its weight pack;
                  // 2 = it selects the ROW parity oa only: a 128-row tile holds both column parities of a pixel pair (osx, wsplit)
    int osx;      // row epilogue: output pixel step along x (0 = os).  The pair form writes [.., 2H, W, 2 x C] with osx = 1, os = 2
    long wsplit;  // != 0: rows 64..127 of a 128-row weight tile come from a second 64-row pack wsplit bytes behind the first (1x1 kernels)
    unsigned char* sgn_out; const unsigned char* sgn_in;   // LeakyReLU sign masks, Cout / 8 bytes per output pixel: byte c / 8, bit c % 8 (loader-specialised
                                                           // 3x3 kernel: Cout == 32 either way, Cout == 64 read only; row epilogue of the generic kernel: written)
    int dbg;      // diagnostic builds only: 1 = skip MFMAs, 2 = skip operand DMA after the first chunk, 4 = skip epilogue
    unsigned long long* trace;   // diagnostic: per-barrier timestamps of workgroup 0 (SRCGAN_TRACE=1), else null
};

template <typename T>
__device__ __forceinline__ size_t chan_off(int c, long plane) {        // byte offset of channel c inside a pixel record
    constexpr int KCE = DT<T>::KCE;
    return (size_t)(c / KCE) * plane + (size_t)(c % KCE) * sizeof(T);
}

// The kernel families behind srcgan_conv_igemm (conv_entry.hip checks the descriptor, builds p and picks one).  Each returns 0 or
// leaves a message in srcgan_last_error().
int sg_conv3x3_dma(const ConvP& p, int dtype, hipStream_t st);      // conv3x3_dma.hip: 3x3 stride 1
int sg_dgrad_s2k4(const ConvP& p, int dtype, hipStream_t st);       // conv_par4.hip: npar == 4, 2x2 parity packs of a 4x4 stride-2 input gradient
int sg_deconv_k3s2(const ConvP& p, int dtype, hipStream_t st);      // deconv_k3s2.hip: npar == 4, transposed 3x3 stride 2
int sg_conv_generic(const ConvP& p, int dtype, int kh, int kw, int stride, hipStream_t st);      // conv_igemm.hip: every other shape
int sg_require_image_31(const ConvP& p);                            // conv_entry.hip: one image of the input below 2 GiB (all but the loader-specialised 3x3 kernel)
