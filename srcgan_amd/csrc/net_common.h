// What the whole-network sequencers (nets.hip: the RRDB generators and the discriminator; oplist.hip: the op-list executor) share:
// tensor references, the convolution descriptor builder, canonical weight layouts, the stride-2 input gradient, the bump allocator,
// the weight-gradient calls and the batched weight packing.  Host code only.
#pragma once
#include "common.h"
#include <algorithm>
#include <vector>

// ---- state with ONE instance per process (defined in nets.hip), whichever translation unit calls
// rev_batch of the next 3x3 stride-1 launch: consecutive launches walk the batch in alternating directions, whichever network issues them
// (SRCGAN_NO_ZIGZAG=1 disables: always 0); see srcgan_conv_desc.rev_batch
int sg_zigzag_next();
// PackList::run: the cached device-side job tables, keyed by tag / device / parameter pointer / dtype / job count, behind one mutex
int sg_pack_list_run(const std::vector<SgPackJob>& jobs, long nblk, void* wp_base, int dtype, const char* tag, const void* key_ptr, void* st,
                     const unsigned long long* guard);

namespace {

struct TRef { void* p; int cs; int coff; long plane; };     // plane: blocked-layout plane stride in bytes (0 = NHWC)
static inline TRef tref(void* p, int cs, int coff = 0, long plane = 0) { return TRef{p, cs, coff, plane}; }
static inline TRef sl(TRef t, int coff) { return TRef{t.p, t.cs, t.coff + coff, t.plane}; }
static const TRef TNULL = {nullptr, 0, 0, 0};

static inline int round_up(int v, int a) { return (v + a - 1) / a * a; }
static inline int img_cs(int c) { return round_up(c, 8); }     // image-like tensors: channels padded to 8

struct Conv {
    srcgan_conv_desc d;
    Conv(int dtype, int kh, int kw, int stride) {
        memset(&d, 0, sizeof(d));
        d.dtype = dtype; d.kh = kh; d.kw = kw; d.stride = stride;
        d.os = 1; d.alpha = 1.f; d.slope = 0.2f; d.mslope = 0.2f;
    }
    Conv& in(TRef x, int B, int H, int W, int Cin) { d.x = x.p; d.x_cs = x.cs; d.x_coff = x.coff; d.x_plane = x.plane; d.B = B; d.H = H; d.W = W; d.Cin = Cin; return *this; }
    Conv& w(const void* wp, const float* bias = nullptr) { d.wp = wp; d.bias = bias; return *this; }
    Conv& out(TRef y, int OH, int OW, int Cout) { d.y = y.p; d.y_cs = y.cs; d.y_coff = y.coff; d.y_plane = y.plane; d.OH = OH; d.OW = OW; d.Cout = Cout; d.YH = OH; d.YW = OW; return *this; }
    Conv& pad(int py, int px) { d.pad_y = py; d.pad_x = px; return *this; }
    Conv& scatter(int os, int oa, int ob, int YH, int YW) { d.os = os; d.oa = oa; d.ob = ob; d.YH = YH; d.YW = YW; return *this; }
    Conv& alpha(float a) { d.alpha = a; return *this; }
    Conv& res1(TRef r, int cend, float beta) { d.r1 = r.p; d.r1_cs = r.cs; d.r1_coff = r.coff; d.r1_plane = r.plane; d.r1_cend = cend; d.beta1 = beta; return *this; }
    Conv& res2(TRef r, int cend, float beta) { d.r2 = r.p; d.r2_cs = r.cs; d.r2_coff = r.coff; d.r2_plane = r.plane; d.r2_cend = cend; d.beta2 = beta; return *this; }
    Conv& lrelu() { d.act = 1; return *this; }
    Conv& sign_out(void* m) { d.sign_out = m; return *this; }                  // write / read the LeakyReLU sign mask (u32 per pixel)
    Conv& sign_in(const void* m) { d.sign_in = m; return *this; }
    Conv& mask(TRef z, int c0) { d.mz = z.p; d.mz_cs = z.cs; d.mz_coff = z.coff; d.mz_plane = z.plane; d.mz_c0 = c0; return *this; }
    int run(void* st) {
        if (d.kh == 3 && d.kw == 3 && d.stride == 1) d.rev_batch = sg_zigzag_next();
        return srcgan_conv_igemm(&d, st);
    }
};

// canonical weight layouts
struct WLayout { long sr, sk, sty, stx, off; };
// Conv2d weight [co][ci][kh][kw]: forward pack rows = co
static inline WLayout lay_fwd(int cin, int kh, int kw) { return {(long)cin * kh * kw, (long)kh * kw, kw, 1, 0}; }
// Conv2d dgrad for stride 1: rows = ci, k = co, taps flipped
static inline WLayout lay_dgrad_s1(int cin, int kh, int kw) { return {(long)kh * kw, (long)cin * kh * kw, -kw, -1, (long)kh * kw - 1}; }
// Input gradient of a k x k stride-2 convolution with padding `pad`, by output parity a (0 / 1) along one axis:
//   dx[2 j + a] = sum over the kernel rows ky == (a + pad) mod 2 of dy[j + (a + pad - ky) / 2] * w[ky]
// -> a stride-1 sub-convolution with n taps; tap t (ascending dy row) uses ky = ky_max - 2 t and needs `lead` rows above row j.
// (4x4 p1: 2 taps, ky_max 3 / 2, lead 1 / 0;  3x3 p1: 1 / 2 taps, lead 0;  7x7 p3: 3 / 4 taps)
struct Par2 { int n, ky_max, lead; };
static inline Par2 par2(int k, int pad, int a) {
    int ky_max = k - 1;
    if (((ky_max ^ (a + pad)) & 1) != 0) --ky_max;
    Par2 r; r.ky_max = ky_max; r.n = ky_max >= 0 ? ky_max / 2 + 1 : 0; r.lead = (ky_max - a - pad) / 2;
    return r;
}

struct Bump {   // workspace bump allocator (256-byte aligned)
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; }
};

static int wgrad_call(int dtype, TRef dy, int OH, int OW, int Cout, TRef x, int B, int H, int W, int Cin, int kh, int kw,
                      int stride, int pad_y, int pad_x, WLayout lay, float alpha, float* slab, float* grad, void* st,
                      float* bias_grad = nullptr, int accumulate = 0) {
    srcgan_wgrad_desc d;
    memset(&d, 0, sizeof(d));
    d.dy = dy.p; d.dy_cs = dy.cs; d.dy_coff = dy.coff; d.x = x.p; d.x_cs = x.cs; d.x_coff = x.coff;
    d.slab = slab; d.grad = grad; d.bias_grad = bias_grad; d.dtype = dtype; d.kh = kh; d.kw = kw; d.stride = stride;
    d.B = B; d.H = H; d.W = W; d.Cin = Cin; d.OH = OH; d.OW = OW; d.Cout = Cout; d.pad_y = pad_y; d.pad_x = pad_x;
    d.nsplit = srcgan_conv_wgrad_nsplit(B, OH, OW, Cout, Cin, stride);
    d.sr = lay.sr; d.sk = lay.sk; d.sty = lay.sty; d.stx = lay.stx; d.off = lay.off;
    d.alpha = alpha; d.accumulate = accumulate;
    return srcgan_conv_wgrad(&d, st);
}
static size_t wgrad_slab(int B, int OH, int OW, int Cout, int Cin, int kh, int kw, int stride) {
    return srcgan_conv_wgrad_slab_bytes(Cout, Cin, kh, kw, srcgan_conv_wgrad_nsplit(B, OH, OW, Cout, Cin, stride));
}
static int bias_grad(int dtype, TRef dy, long npix, int C, float scale, float* out, float* scratch, void* st) {
    return srcgan_col_reduce(0, dy.p, dy.cs, dy.coff, nullptr, 0, 0, nullptr, nullptr, npix, C, scale, out, nullptr, scratch, dtype, st);
}

// ---- batched weight packing with a cached device-side job table (the cache: sg_pack_list_run)
struct PackList {
    std::vector<SgPackJob> jobs; long nblk = 0; int dtype; char* base;
    PackList(int dt, void* wp_base) : dtype(dt), base((char*)wp_base) {}
    void add(const float* w, void* wp, int rows, int kdim, int tys, int txs, long sr, long sk, long sty, long stx, long off,
             int k_off = 0, int k_total = -1, float scale = 1.f) {
        SgPackJob j;
        memset(&j, 0, sizeof(j));
        j.w = w; j.wp_off = (size_t)((char*)wp - base); j.rows = rows; j.kdim = kdim; j.tys = tys; j.txs = txs;
        j.sr = sr; j.sk = sk; j.sty = sty; j.stx = stx; j.off = off; j.k_off = k_off; j.k_total = k_total < 0 ? kdim : k_total; j.scale = scale;
        sg_pack_job_finish(j, dtype, nblk);
        jobs.push_back(j);
    }
    void add(const float* w, void* wp, int rows, int kdim, int tys, int txs, WLayout L) { add(w, wp, rows, kdim, tys, txs, L.sr, L.sk, L.sty, L.stx, L.off); }
    int run(const char* tag, const void* key_ptr, void* st, const unsigned long long* guard = nullptr) {
        return sg_pack_list_run(jobs, nblk, base, dtype, tag, key_ptr, st, guard);
    }
};

// opts.pack == 2: the persistent pack is re-made only if the device-side guard words differ (srcgan_net_opts)
static inline const unsigned long long* pack_guard(const srcgan_net_opts* o) {
    return (o && o->wpack && o->pack == 2) ? (const unsigned long long*)o->guard : nullptr;
}

// ---- the input gradient of a k x k, stride 2, padding `pad` convolution cin -> cout: four stride-1 sub-convolutions over dy, one
// per output parity q = (a, b) = (q >> 1, q & 1), each with its own pack of par2() taps per axis (rows = cin, k = cout), made
// from the canonical weight w [cout][cin][k][k]
struct S2Dgrad {
    int k, pad, cin, cout;
    void plan(Bump& wb, int dtype, size_t wd[4]) const {
        for (int q = 0; q < 4; ++q) wd[q] = wb.take(srcgan_packed_weight_bytes(cin, cout, par2(k, pad, q >> 1).n * par2(k, pad, q & 1).n, dtype));
    }
    void pack(PackList& packs, const float* w, char* wp, const size_t wd[4]) const {
        const long kk = (long)k * k;
        for (int q = 0; q < 4; ++q) {
            const Par2 py = par2(k, pad, q >> 1), px = par2(k, pad, q & 1);
            packs.add(w, wp + wd[q], cin, cout, py.n, px.n, kk, (long)cin * kk, -2 * k, -2, (long)py.ky_max * k + px.ky_max);
        }
    }
    // dy [B, OH, OW, cout] -> dx [B, H, W, cin].  acc: dx already holds a contribution, add to it; mz: multiply by LeakyReLU' of
    // this tensor (either may be TNULL).  fuse: all four parities from one staged dy tile in ONE launch (conv_par4.hip: 4x4 p1,
    // equally spaced packs, 16-byte accessible operands) where that applies; SRCGAN_NO_PAR4 (diagnostic builds) keeps the four.
    // bias: per dx channel, added in either form -- the same four sub-convolutions ARE ConvTranspose2d(k4, s2, p1) of dy with the
    // stored weight [in][out][4][4] read as w [cout][cin][4][4] (the op-list executor's RD_DECONV4).
    int run(int dt, TRef dy, int B, int OH, int OW, TRef dx, int H, int W, const char* wp, const size_t wd[4], TRef acc, TRef mz,
            bool fuse, void* st, float mslope = 0.2f, const float* bias = nullptr) const {
        static const bool no_par4 = sg_env("SRCGAN_NO_PAR4") != nullptr;
        auto launch = [&](Conv& cv) {
            if (acc.p) cv.res1(acc, cin, 1.f);
            if (mz.p) { cv.mask(mz, 0); cv.d.mslope = mslope; }
            return cv.run(st);
        };
        const int vec = 16 / (dt == SRCGAN_F32 ? 4 : 2);
        const size_t wstep = wd[1] - wd[0];
        const bool even = wd[2] - wd[1] == wstep && wd[3] - wd[2] == wstep;
        if (fuse && !no_par4 && k == 4 && pad == 1 && even && H >= 2 && W >= 2 && cin % vec == 0 && dx.cs % vec == 0 && (uintptr_t)bias % 16 == 0) {
            Conv cv(dt, 2, 2, 1);
            cv.in(dy, B, OH, OW, cout).w(wp + wd[0], bias).out(dx, (H + 1) / 2, (W + 1) / 2, cin).scatter(2, 0, 0, H, W);
            cv.d.npar = 4; cv.d.wpar_stride = (long)wstep;
            return launch(cv);
        }
        for (int q = 0; q < 4; ++q) {
            const int a = q >> 1, b = q & 1;
            const int mh = (H - a + 1) / 2, mw = (W - b + 1) / 2;
            if (mh <= 0 || mw <= 0) continue;
            const Par2 py = par2(k, pad, a), px = par2(k, pad, b);
            Conv cv(dt, py.n, px.n, 1);
            cv.in(dy, B, OH, OW, cout).w(wp + wd[q], bias).out(dx, mh, mw, cin).pad(py.lead, px.lead).scatter(2, a, b, H, W);
            SG_TRY(launch(cv));
        }
        return 0;
    }
};

}  // namespace
