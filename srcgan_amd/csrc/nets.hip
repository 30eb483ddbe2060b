// Whole-network sequencing for the SRCGAN hot path: one C call per nn.Module.forward and one per
// autograd backward.  Pure host code that chains the gfx950 kernels of conv_igemm.hip,
// conv_wgrad.hip and elementwise.hip on the caller's stream (no allocation, no synchronisation:
// graph-capturable).
//
//   RRDB generators (RDDBNet, RDDBNetA, RDDBNetB, legacy RDDBNet, SRDN)   reference src/model/rddb.py:48-114, model.py:347-440, srdn.py
//   NLayerDiscriminator (PatchGAN, BatchNorm2d / InstanceNorm2d)          reference src/model/model.py:595-639
//   op-list networks: ResDeconv, ESPCN, SRCNN, EDSR                        reference src/model/{resdeconv,espcn,srcnn,edsr}.py
//
// Memory design (HBM): activations live in NHWC.  Each ResidualDenseBlock_5 owns ONE dense buffer of
// nf+4*gc channels; conv k reads the channel prefix [0, nf+(k-1)gc) and writes its own slice, so the
// four torch.cat copies of rddb.py:64-67 (and CatBackward) never exist.  conv5's epilogue fuses
// "x5*0.2 + x" (rddb.py:68), and for RDB3 also the RRDB residual (rddb.py:82), writing straight into
// channels [0,nf) of the next block's dense buffer.  Backward mirrors this with a dense *gradient*
// buffer per block that the dgrads of conv5..conv1 accumulate into in place.
#include "common.h"
#include <algorithm>
#include <vector>
#include <map>
#include <string>
#include <mutex>

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
    // consecutive 3x3 s1 launches walk the batch in alternating directions (SRCGAN_NO_ZIGZAG=1 disables): see srcgan_conv_desc.rev_batch
    int run(void* st) {
        static const bool zig = sg_env("SRCGAN_NO_ZIGZAG") == nullptr;
        static int flip = 0;
        if (zig && d.kh == 3 && d.kw == 3 && d.stride == 1) { d.rev_batch = flip; flip ^= 1; }
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

// ---- batched weight packing with a cached device-side job table
struct PackCache { std::vector<SgPackJob> host; SgPackJob* dev = nullptr; SgPackJob* pinned = nullptr; size_t cap = 0; hipEvent_t staged = nullptr; };
static std::map<std::string, PackCache> g_pack_cache;
static std::mutex g_pack_mutex;

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
        if (jobs.empty()) return 0;
        int dev = 0;
        SG_HIP(hipGetDevice(&dev));
        char key[112];
        snprintf(key, sizeof(key), "%s:%d:%p:%d:%zu", tag, dev, key_ptr, dtype, jobs.size());
        std::lock_guard<std::mutex> lock(g_pack_mutex);
        PackCache& c = g_pack_cache[key];
        const size_t bytes = jobs.size() * sizeof(SgPackJob);
        if (c.host.size() != jobs.size() || memcmp(c.host.data(), jobs.data(), bytes) != 0) {
            // cold path (first call / parameters or buffers moved).  The table is staged in pinned memory and copied on the
            // call's stream: stream order puts the copy behind every earlier pack kernel that still reads the old table and in
            // front of this call's -- no host synchronisation.  Only a table that outgrows its buffers allocates (first call,
            // behind a stream drain: the old device table may still be in use), and a second re-staging waits for the first
            // one's copy to have left the pinned buffer.
            if (c.cap < bytes) {
                SG_HIP(hipStreamSynchronize((hipStream_t)st));
                if (c.dev) SG_HIP(hipFree(c.dev));
                if (c.pinned) SG_HIP(hipHostFree(c.pinned));
                SG_HIP(hipMalloc((void**)&c.dev, bytes));
                SG_HIP(hipHostMalloc((void**)&c.pinned, bytes, hipHostMallocDefault));
                c.cap = bytes;
            }
            if (!c.staged) SG_HIP(hipEventCreateWithFlags(&c.staged, hipEventDisableTiming));
            else SG_HIP(hipEventSynchronize(c.staged));
            memcpy(c.pinned, jobs.data(), bytes);
            SG_HIP(hipMemcpyAsync(c.dev, c.pinned, bytes, hipMemcpyHostToDevice, (hipStream_t)st));
            SG_HIP(hipEventRecord(c.staged, (hipStream_t)st));
            c.host = jobs;
        }
        return sg_pack_multi_launch(c.dev, (int)jobs.size(), nblk, base, dtype, (hipStream_t)st, guard);
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
    int run(int dt, TRef dy, int B, int OH, int OW, TRef dx, int H, int W, const char* wp, const size_t wd[4], TRef acc, TRef mz,
            bool fuse, void* st, float mslope = 0.2f) const {
        static const bool no_par4 = sg_env("SRCGAN_NO_PAR4") != nullptr;
        auto launch = [&](Conv& cv) {
            if (acc.p) cv.res1(acc, cin, 1.f);
            if (mz.p) { cv.mask(mz, 0); cv.d.mslope = mslope; }
            return cv.run(st);
        };
        const int vec = 16 / (dt == SRCGAN_F32 ? 4 : 2);
        const size_t wstep = wd[1] - wd[0];
        const bool even = wd[2] - wd[1] == wstep && wd[3] - wd[2] == wstep;
        if (fuse && !no_par4 && k == 4 && pad == 1 && even && H >= 2 && W >= 2 && cin % vec == 0 && dx.cs % vec == 0) {
            Conv cv(dt, 2, 2, 1);
            cv.in(dy, B, OH, OW, cout).w(wp + wd[0]).out(dx, (H + 1) / 2, (W + 1) / 2, cin).scatter(2, 0, 0, H, W);
            cv.d.npar = 4; cv.d.wpar_stride = (long)wstep;
            return launch(cv);
        }
        for (int q = 0; q < 4; ++q) {
            const int a = q >> 1, b = q & 1;
            const int mh = (H - a + 1) / 2, mw = (W - b + 1) / 2;
            if (mh <= 0 || mw <= 0) continue;
            const Par2 py = par2(k, pad, a), px = par2(k, pad, b);
            Conv cv(dt, py.n, px.n, 1);
            cv.in(dy, B, OH, OW, cout).w(wp + wd[q]).out(dx, mh, mw, cin).pad(py.lead, px.lead).scatter(2, a, b, H, W);
            SG_TRY(launch(cv));
        }
        return 0;
    }
};

// ======================================================================================== RDDBNet
// The generator families: the values of srcgan_rddbnet_cfg.legacy (include/srcgan_amd.h describes each)
enum RddbFamily { RDDB_PLAIN = 0, RDDB_NETB = 1, RDDB_LEGACY = 2, RDDB_SRDN = 3 };

// What does not depend on where the activations live: validated geometry, the tail's op list, packed-weight offsets, parameter
// indices.  Activation and mask offsets belong to the buffer-naming policy (RddbNames).
struct RddbPlan {
    int dtype, esz, nf, gc, nb, C, nst, ndn, kce, nplane; long plane_bytes;
    int B, H, W;           // input
    int Ht, Wt;            // trunk resolution
    int HO, WO;            // output resolution
    int in_cs, out_cs;
    int nparams;
    // the family, and the facts about it the walkers branch on
    RddbFamily family;
    bool x2_tail;             // tail = nearest x2 / shared 3x3 convs + LeakyReLU, conv_last with bias (model/model.py:347-440)
    bool has_trunk_conv;      // trunk_conv + global skip behind the RRDBs
    int nup;                  // ConvTranspose up-sampler stages that run (the tail families up-sample in their tail: 0)
    int nrr;                  // RRDBs in the trunk (SRDN: encoder + decoder = 2 nb, srdn.py:56-74; legacy RDDBNet: 0)
    int ndense;               // dense buffers (legacy RDDBNet discards its trunk: one buffer holds conv_first's output)
    const char* tag;          // pack-cache tag stem ("_fwd" / "_bwd" / "_bwd_dx" is appended at the call)
    size_t wpack_bytes;                            // packed weights: total size; the offsets below are relative to its start
    size_t w_rdb_d0, w_rdb_dsz;                    // contiguous region of the composite dense-block dgrad packs
    size_t w_first_f, w_first_d, w_trunk_f, w_trunk_d, w_last_f, w_last_d;
    std::vector<size_t> w_rdb_f, w_rdb_d;          // [nb*15]
    size_t w_up_f[5][4], w_up_d[5];
    size_t w_dn_f[5], w_dn_d[5][4];
    // parameter indices
    int p_first_w, p_first_b, p_rdb0, p_trunk_w, p_trunk_b, p_up0, p_dn0, p_last_w;
    int ntail, nlw, p_lg[3], p_last_b;       // nearest-x2 tail: ops, shared weights and their parameters, conv_last's bias
    S2Dgrad dn_dgrad() const { return S2Dgrad{3, 1, nf, nf}; }      // input gradient of a down stage of RDDBNetA (3x3 s2 p1, nf -> nf)
    int prdb(int r) const { return p_rdb0 + r * 10 + ((family == RDDB_SRDN && r >= 3 * nb) ? 2 : 0); }     // SRDN: trunk_conv's two parameters sit between the stacks
    struct TailOp { int conv, w, hin, win, hout, wout; } tail[16];     // conv: 1 = 3x3 conv w + LReLU, 0 = nearest x2
    size_t lw_f[3], lw_d[3];
};

static int log2i(int v) { int n = 0; while ((1 << n) < v) ++n; return n; }

static int rddb_plan(const srcgan_rddbnet_cfg* c, RddbPlan& P) {
    SG_REQUIRE(c, "rddbnet: null cfg");
    SG_REQUIRE(sg_dtype_ok(c->dtype), "rddbnet: bad dtype %d", c->dtype);
    SG_REQUIRE(c->in_ch > 0 && c->in_ch <= 8 && c->out_ch > 0 && c->out_ch <= 8, "rddbnet: in/out channels must be in 1..8");
    SG_REQUIRE(c->nf > 0 && c->gc > 0 && c->nf % 8 == 0 && c->gc % 8 == 0, "rddbnet: nf and gc must be multiples of 8 (nf=%d gc=%d)", c->nf, c->gc);
    SG_REQUIRE(c->nb >= 1 && c->B > 0 && c->H > 0 && c->W > 0, "rddbnet: bad nb/B/H/W");
    SG_REQUIRE(c->up >= 1 && (c->up & (c->up - 1)) == 0 && c->up <= 16, "rddbnet: upscale_factor must be a power of two <= 16");
    SG_REQUIRE(c->down >= 0 && (c->down == 0 || ((c->down & (c->down - 1)) == 0 && c->down <= 16)), "rddbnet: bad down factor");
    SG_REQUIRE(!(c->down > 1 && c->up > 1), "rddbnet: up and down are exclusive");
    SG_REQUIRE(c->legacy >= 0 && c->legacy <= 3, "rddbnet: legacy must be 0..3");
    P.family = (RddbFamily)c->legacy;
    P.x2_tail = P.family == RDDB_NETB || P.family == RDDB_LEGACY;
    SG_REQUIRE(!P.x2_tail || (c->down == 0 && (c->up == 2 || c->up == 4 || (P.family == RDDB_LEGACY && c->up == 1))),
               "rddbnet: legacy generators take mode x2 / x4 (legacy RDDBNet also x1) and no down factor");
    SG_REQUIRE(P.family != RDDB_SRDN || (c->up == 1 && c->down == 0), "rddbnet: SRDN keeps the resolution (its upscale_factor is unused, srdn.py:67-74): pass up = 1");
    P.has_trunk_conv = P.family == RDDB_PLAIN || P.family == RDDB_NETB;
    P.nrr = P.family == RDDB_SRDN ? 2 * c->nb : (P.family == RDDB_LEGACY ? 0 : c->nb);
    P.ndense = P.family == RDDB_LEGACY ? 1 : 3 * P.nrr;
    P.tag = P.family == RDDB_NETB ? "rddbB" : P.family == RDDB_LEGACY ? "rddbL" : P.family == RDDB_SRDN ? "srdn" : "rddb";
    P.ntail = 0; P.nlw = 0;
    P.dtype = c->dtype; P.esz = c->dtype == SRCGAN_F32 ? 4 : 2;
    P.nf = c->nf; P.gc = c->gc; P.nb = c->nb; P.C = c->nf + 4 * c->gc;
    P.B = c->B; P.H = c->H; P.W = c->W;
    P.nst = c->down > 0 ? 0 : log2i(c->up);
    P.nup = P.x2_tail ? 0 : P.nst;
    P.ndn = c->down > 1 ? log2i(c->down) : 0;
    if (P.ndn) SG_REQUIRE(c->H % c->down == 0 && c->W % c->down == 0, "rddbnet: H, W must be divisible by the down factor");
    P.Ht = c->H >> P.ndn; P.Wt = c->W >> P.ndn;
    P.HO = P.Ht << P.nst; P.WO = P.Wt << P.nst;
    P.in_cs = img_cs(c->in_ch); P.out_cs = img_cs(c->out_ch);
    // dense buffers use the blocked layout [plane = 64-byte channel chunk][pixel][64 B]: every operand fetch of the 3x3 kernel
    // and of the dense wgrad is then >= 1 KiB contiguous (64-byte pieces at a 384-byte pixel stride ran at half rate)
    P.kce = 64 / P.esz; P.nplane = (P.C + P.kce - 1) / P.kce; P.plane_bytes = (long)c->B * P.Ht * P.Wt * 64;
    if (P.x2_tail) {
        int h = P.Ht, w = P.Wt;
        auto op = [&](int conv, int wi) {
            RddbPlan::TailOp& o = P.tail[P.ntail++];
            o.conv = conv; o.w = wi; o.hin = h; o.win = w;
            if (!conv) { h *= 2; w *= 2; }
            o.hout = h; o.wout = w;
        };
        if (P.family == RDDB_NETB) {    // RDDBNetB (model.py:427-439): weights 0 = upconv1, 1 = upconv2, 2 = HRconv
            if (c->up == 4) { op(0, 0); op(1, 0); op(0, 0); op(1, 1); }
            else { op(0, 0); op(1, 0); op(1, 0); }
            for (int k = 0; k < 8; ++k) op(1, 2);
            P.nlw = 3;
        } else {                        // legacy RDDBNet (model.py:381-391): weights 0 = upconv, 1 = HRconv
            for (int t = 1; t < c->up; t *= 2) { op(0, 0); op(1, 0); }
            if (c->up == 1) op(1, 0);
            op(1, 1); op(1, 1);
            P.nlw = 2;
        }
    }
    Bump wb;
    auto pk = [&](int rows, int k, int taps) { return wb.take(srcgan_packed_weight_bytes(rows, k, taps, c->dtype)); };
    P.w_first_f = pk(c->nf, P.in_cs, 9); P.w_first_d = pk(c->in_ch, c->nf, 9);
    for (int s = 0; s < P.ndn; ++s) { P.w_dn_f[s] = pk(c->nf, c->nf, 9); P.dn_dgrad().plan(wb, c->dtype, P.w_dn_d[s]); }
    const int nrdb = (P.nrr ? P.nrr : c->nb) * 3;
    P.w_rdb_f.resize(nrdb * 5); P.w_rdb_d.resize(nrdb * 5);
    for (int i = 0; i < nrdb; ++i)
        for (int k = 0; k < 5; ++k) {
            const int cin = c->nf + k * c->gc, cout = k < 4 ? c->gc : c->nf;
            P.w_rdb_f[i * 5 + k] = pk(cout, cin, 9);
        }
    P.w_trunk_f = pk(c->nf, c->nf, 9); P.w_trunk_d = pk(c->nf, c->nf, 9);
    for (int s = 0; s < P.nst; ++s) { for (int q = 0; q < 4; ++q) P.w_up_f[s][q] = pk(c->nf, c->nf, 1); P.w_up_d[s] = pk(c->nf, c->nf, 4); }
    P.w_last_f = pk(c->out_ch, c->nf, 9); P.w_last_d = pk(c->nf, P.out_cs, 9);
    for (int k = 0; k < P.nlw; ++k) { P.lw_f[k] = pk(c->nf, c->nf, 9); P.lw_d[k] = pk(c->nf, c->nf, 9); }
    // dense-block backward: slice j of the block input gets its gradient from ONE conv over the concatenated
    // output-gradients [dy5 | dy4 | ... | dy_{j+1}] (rows = slice channels, K = nf + (4-j)*gc)
    P.w_rdb_d0 = wb.off;
    for (int i = 0; i < nrdb; ++i)
        for (int j = 0; j < 5; ++j) P.w_rdb_d[i * 5 + j] = pk(j == 0 ? c->nf : c->gc, c->nf + (4 - j) * c->gc, 9);
    P.w_rdb_dsz = wb.off - P.w_rdb_d0;
    P.wpack_bytes = wb.off + 256;
    // parameter indices (state_dict order)
    int n = 0;
    P.p_first_w = n++; P.p_first_b = n++;
    P.p_dn0 = n; n += 2 * P.ndn;
    P.p_rdb0 = n; n += c->nb * 30;
    P.p_trunk_w = n++; P.p_trunk_b = n++;
    if (P.family == RDDB_SRDN) n += c->nb * 30;          // RRDB_decoder
    P.p_up0 = n;
    if (P.x2_tail) for (int k = 0; k < P.nlw; ++k) { P.p_lg[k] = n; n += 2; }
    else n += P.nst;
    P.p_last_w = n++;
    P.p_last_b = P.x2_tail ? n++ : -1;
    P.nparams = n;
    return 0;
}

// ---- where the forward's activations live.  The launch sequence of a generator is ONE walker (RddbCall::forward) over a
// buffer-naming policy: the training policy keeps every tensor a backward reads (one dense buffer per ResidualDenseBlock_5, the
// LeakyReLU sign masks, every up-sampler stage), the inference policy keeps only what a later launch of the same pass reads.
struct RddbNames {
    size_t xin = 0, fea0 = 0, dn[5] = {}, T = 0, U[6] = {}, out = 0, tail[16] = {}, wpk = 0, total = 0;      // 0 = the policy has no such buffer
    std::vector<size_t> A;      // dense buffer of RDB r
    size_t home = 0;            // inference: nf-channel copy (whole leading planes) of the trunk input, which the rotation overwrites
    bool rolling = false;       // inference policy
    size_t bm = 0; long bm_bytes = 0;   // sign masks of a dense buffer's four LeakyReLU slices: offset inside the buffer, bytes per slice (0 = not written)
    size_t um = 0; long um_bytes = 0;   // sign mask of the last up-sampler stage's output (8 bytes per HR pixel; 0 = not written): conv_last's input gradient
                                // reads it instead of the 64-channel activation (2.1 GB at the bench size)
};

// Training: every tensor has a buffer of its own, in the forward's order; the backward (RddbBwd) reads the same names.
static void rddb_train_names(const srcgan_rddbnet_cfg* c, const RddbPlan& P, RddbNames& N) {
    const size_t e = P.esz, B = c->B, nf = c->nf;
    Bump b;
    N.xin = b.take(B * c->H * c->W * P.in_cs * e);
    if (P.ndn) N.fea0 = b.take(B * c->H * c->W * nf * e);     // conv_first output at HR (HR->LR variant only)
    for (int s = 0; s < P.ndn; ++s) N.dn[s] = b.take(B * (c->H >> (s + 1)) * (c->W >> (s + 1)) * nf * e);
    // one bit per element for LeakyReLU' (instead of re-reading the activation in the backward pass): bf16, 32-channel slices
    static const bool no_sign = sg_env("SRCGAN_NO_SIGNMASK") != nullptr || sg_env("SRCGAN_DMA_CFG") != nullptr;
    N.bm_bytes = (!no_sign && sg_is16(c->dtype) && c->gc == 32 && nf % 32 == 0 && P.family != RDDB_LEGACY) ? (long)B * P.Ht * P.Wt * 4 : 0;
    N.bm = align_up((size_t)P.nplane * P.plane_bytes, 256);
    const size_t szA = align_up(N.bm + 4 * (size_t)N.bm_bytes, 256);
    const size_t A0 = b.take(szA * P.ndense);
    N.A.resize(P.ndense);
    for (int r = 0; r < P.ndense; ++r) N.A[r] = A0 + (size_t)r * szA;
    N.T = b.take(B * P.Ht * P.Wt * nf * e);
    for (int s = 0; s <= P.nup; ++s) N.U[s] = b.take(B * (P.Ht << s) * (P.Wt << s) * nf * e);
    if (P.family == RDDB_SRDN) N.U[0] = N.T;           // SRDN: conv_last reads trunk output + skip, accumulated in place in T
    for (int k = 0; k < P.ntail; ++k) N.tail[k] = b.take(B * P.tail[k].hout * P.tail[k].wout * nf * e);
    N.out = b.take(B * P.HO * P.WO * P.out_cs * e);
    N.um_bytes = (!no_sign && sg_is16(c->dtype) && nf == 64 && P.nst > 0 && P.family == RDDB_PLAIN) ? (long)B * P.HO * P.WO * 8 : 0;
    if (N.um_bytes) N.um = b.take((size_t)N.um_bytes);
    N.wpk = b.off;
    N.total = N.wpk + P.wpack_bytes;
}

// Inference: the workspace does not grow with nb.  THREE dense buffers rotate: RDB r reads its own buffer and writes channels
// [0,nf) of the next one, and RDB 3i+2 also reads the RRDB input (buffer of RDB 3i), so the buffer of RDB r+1 is the one that
// is neither RDB r's nor RDB 3i's -- for r = 3i+2 that is the buffer of RDB 3i+1, dead by then.  The network's first trunk
// input (trunk_conv's skip; SRDN: the two stack skips, one after the other) is copied to `home`.  Everything at a resolution
// other than the trunk's ping-pongs between two buffers; no sign mask is written.
static void rddb_infer_names(const srcgan_rddbnet_cfg* c, const RddbPlan& P, RddbNames& N) {
    const size_t e = P.esz, B = c->B, nf = c->nf;
    Bump b;
    N.rolling = true;
    N.xin = b.take(B * c->H * c->W * P.in_cs * e);
    if (P.ndn) {     // HR->LR stages: conv_first's output and the stage outputs alternate; the last stage writes the trunk input
        const size_t pp0 = b.take(B * c->H * c->W * nf * e);
        const size_t pp1 = P.ndn > 1 ? b.take(B * (c->H >> 1) * (c->W >> 1) * nf * e) : 0;
        N.fea0 = pp0;
        for (int s = 0; s < P.ndn; ++s) N.dn[s] = (s & 1) ? pp0 : pp1;
    }
    const size_t szA = align_up((size_t)P.nplane * P.plane_bytes, 256);
    size_t slot[3] = {0, 0, 0};
    for (int k = 0; k < 3 && k < P.ndense; ++k) slot[k] = b.take(szA);
    N.A.resize(P.ndense);
    int cur = 0, rrdb_in = 0;
    for (int r = 0; r < P.ndense; ++r) {
        if (r % 3 == 0) rrdb_in = cur;
        N.A[r] = slot[cur];
        int nxt = 0;
        while (nxt == cur || nxt == rrdb_in) ++nxt;
        cur = nxt;
    }
    if (P.nrr) N.home = b.take((size_t)((nf + P.kce - 1) / P.kce) * P.plane_bytes);
    if (P.family != RDDB_LEGACY) N.T = b.take(B * P.Ht * P.Wt * nf * e);       // legacy RDDBNet has no trunk output
    if (P.x2_tail) {
        N.U[0] = b.take(B * P.Ht * P.Wt * nf * e);
        size_t pp[2];
        for (int k = 0; k < 2; ++k) pp[k] = b.take(B * P.HO * P.WO * nf * e);
        for (int k = 0; k < P.ntail; ++k) N.tail[k] = pp[k & 1];
    } else if (P.family == RDDB_SRDN) {
        N.U[0] = N.T;
    } else {        // stage s has 4^s times the trunk's pixels: even stages share one buffer, odd stages the other
        size_t pp[2] = {0, 0};
        for (int k = 0; k < 2 && k <= P.nst; ++k) {
            const int top = ((P.nst - k) & ~1) + k;        // largest stage <= nst with the parity of k
            pp[k] = b.take(B * (P.Ht << top) * (P.Wt << top) * nf * e);
        }
        for (int s = 0; s <= P.nst; ++s) N.U[s] = pp[s & 1];
    }
    N.out = b.take(B * P.HO * P.WO * P.out_cs * e);
    N.wpk = b.off;
    N.total = N.wpk + P.wpack_bytes;       // the packed-weight region is the training policy's, as is
}

struct RddbBwdPlan {
    size_t dout, dU[6], Pg[3], szP, dfea_dn[5], dxin, slab, colscr, total;
};
static void rddb_bwd_plan(const srcgan_rddbnet_cfg* c, const RddbPlan& P, RddbBwdPlan& Q) {
    const size_t e = P.esz, B = c->B;
    Bump b;
    Q.dout = b.take(B * P.HO * P.WO * P.out_cs * e);
    for (int s = 0; s <= P.nup; ++s) Q.dU[s] = b.take(B * (P.Ht << s) * (P.Wt << s) * c->nf * e);
    if (P.x2_tail) { Q.dU[1] = b.take(B * P.HO * P.WO * c->nf * e); Q.dU[2] = b.take(B * P.HO * P.WO * c->nf * e); }   // ping-pong
    Q.szP = align_up((size_t)P.nplane * P.plane_bytes, 256);
    for (int i = 0; i < 3; ++i) Q.Pg[i] = b.take(Q.szP);
    for (int s = 0; s <= P.ndn; ++s) Q.dfea_dn[s] = b.take(B * (c->H >> s) * (c->W >> s) * c->nf * e);
    Q.dxin = b.take(B * c->H * c->W * P.in_cs * e);
    size_t slab = 0;
    auto mx = [&](size_t v) { if (v > slab) slab = v; };
    mx(wgrad_slab(c->B, c->H, c->W, c->nf, P.in_cs, 3, 3, 1));
    for (int k = 0; k < 5; ++k) mx(wgrad_slab(c->B, P.Ht, P.Wt, k < 4 ? c->gc : c->nf, c->nf + k * c->gc, 3, 3, 1));
    mx(wgrad_slab(c->B, P.Ht, P.Wt, c->nf, c->nf, 3, 3, 1));
    for (int s = 0; s < P.nup; ++s) mx(wgrad_slab(c->B, P.Ht << s, P.Wt << s, c->nf, c->nf, 2, 2, 2));
    for (int k = 0; k < P.ntail; ++k) if (P.tail[k].conv) mx(wgrad_slab(c->B, P.tail[k].hout, P.tail[k].wout, c->nf, c->nf, 3, 3, 1));
    for (int s = 0; s < P.ndn; ++s) mx(wgrad_slab(c->B, c->H >> (s + 1), c->W >> (s + 1), c->nf, c->nf, 3, 3, 2));
    mx(wgrad_slab(c->B, P.HO, P.WO, c->out_ch, c->nf, 3, 3, 1));
    mx(srcgan_wgrad_dense_slab_bytes(P.C, P.C, c->dtype, c->B, P.Ht, P.Wt));
    Q.slab = b.take(slab);
    const long maxpix = (long)B * (P.HO > c->H ? P.HO : c->H) * (P.WO > c->W ? P.WO : c->W);
    Q.colscr = b.take((size_t)2 * srcgan_col_reduce_blocks(maxpix) * P.C * sizeof(float));
    Q.total = b.off + 256;
}

}  // namespace

extern "C" int srcgan_rddbnet_num_params(const srcgan_rddbnet_cfg* c) { RddbPlan P; if (rddb_plan(c, P)) return -1; return P.nparams; }
extern "C" int srcgan_rddbnet_num_rrdb(const srcgan_rddbnet_cfg* c) { RddbPlan P; if (rddb_plan(c, P)) return -1; return P.nrr; }
extern "C" size_t srcgan_rddbnet_wpack_bytes(const srcgan_rddbnet_cfg* c) { RddbPlan P; if (rddb_plan(c, P)) return 0; return P.wpack_bytes; }
extern "C" size_t srcgan_rddbnet_ws_bytes(const srcgan_rddbnet_cfg* c) {
    RddbPlan P; if (rddb_plan(c, P)) return 0;
    RddbNames N; rddb_train_names(c, P, N); return N.total;
}
extern "C" size_t srcgan_rddbnet_infer_ws_bytes(const srcgan_rddbnet_cfg* c) {
    RddbPlan P; if (rddb_plan(c, P)) return 0;
    RddbNames N; rddb_infer_names(c, P, N); return N.total;
}
extern "C" size_t srcgan_rddbnet_bwd_scratch_bytes(const srcgan_rddbnet_cfg* c) {
    RddbPlan P; if (rddb_plan(c, P)) return 0;
    RddbBwdPlan Q; rddb_bwd_plan(c, P, Q); return Q.total;
}

// The parameters [first, end) a backward call over the RRDBs [lo, hi) finalises (state_dict order): hi == nrr extends the range to
// the last parameter, lo == 0 to parameter 0; a network without a trunk is one range.
extern "C" int srcgan_rddbnet_phase_params(const srcgan_rddbnet_cfg* c, int lo, int hi, int* first, int* end) {
    RddbPlan P;
    SG_TRY(rddb_plan(c, P));
    SG_REQUIRE(first && end, "srcgan_rddbnet_phase_params: null pointer");
    SG_REQUIRE(lo >= 0 && lo <= hi && hi <= P.nrr, "srcgan_rddbnet_phase_params: RRDB range [%d,%d) outside [0,%d)", lo, hi, P.nrr);
    *first = lo == 0 ? 0 : P.prdb(3 * lo);
    *end = hi == P.nrr ? P.nparams : P.prdb(3 * hi);
    return 0;
}

namespace {

// ---- one native call on a generator: what the forward and the backward both need to address their operands
struct RddbCall {
    const srcgan_rddbnet_cfg* c; const RddbPlan& P; const RddbNames& N;
    const float* const* params; const srcgan_net_opts* opt; void* st;
    const int dt, nf, gc, B, H, W;      // H, W: trunk resolution
    char* w8;
    char* wp;            // packed weights: a persistent buffer of the caller's (packed once per optimiser step) or a region of this call's workspace
    bool do_pack;
    RddbCall(const srcgan_rddbnet_cfg* c_, const RddbPlan& P_, const RddbNames& N_, const float* const* params_, void* ws,
             const srcgan_net_opts* opt_, void* st_)
        : c(c_), P(P_), N(N_), params(params_), opt(opt_), st(st_), dt(c_->dtype), nf(c_->nf), gc(c_->gc), B(c_->B), H(P_.Ht), W(P_.Wt),
          w8((char*)ws), wp((opt_ && opt_->wpack) ? (char*)opt_->wpack : (char*)ws + N_.wpk), do_pack(!(opt_ && opt_->wpack) || opt_->pack) {}
    TRef T_(size_t off, int cs) const { return tref(w8 + off, cs); }
    TRef Abuf(int r) const { return tref(w8 + N.A[r], P.kce, 0, P.plane_bytes); }
    int forward(const float* x_nchw, float* y_nchw) const;
};

int RddbCall::forward(const float* x_nchw, float* y_nchw) const {
    SG_REQUIRE(x_nchw && params && w8 && y_nchw, "srcgan_rddbnet_forward: null pointer");
    SG_REQUIRE(((uintptr_t)w8 % 256) == 0, "srcgan_rddbnet_forward: workspace must be 256-byte aligned");
    SG_REQUIRE(((uintptr_t)wp % 256) == 0, "srcgan_rddbnet_forward: wpack must be 256-byte aligned");
    // inference: copy the nf leading channels of a dense buffer (whole planes of the blocked layout: one contiguous copy) to `home`
    auto to_home = [&](TRef a) {
        return hipMemcpyAsync(w8 + N.home, a.p, (size_t)((nf + P.kce - 1) / P.kce) * P.plane_bytes, hipMemcpyDeviceToDevice, (hipStream_t)st);
    };

    // ---- pack weights for this call (f32 canonical -> dtype, MFMA-friendly): ONE batched launch
    PackList packs(dt, wp);
    packs.add(params[P.p_first_w], wp + P.w_first_f, nf, c->in_ch, 3, 3, (long)c->in_ch * 9, 9, 3, 1, 0);
    for (int s = 0; s < P.ndn; ++s)
        packs.add(params[P.p_dn0 + 2 * s], wp + P.w_dn_f[s], nf, nf, 3, 3, (long)nf * 9, 9, 3, 1, 0);
    for (int i = 0; i < P.nrr * 3; ++i)
        for (int k = 0; k < 5; ++k) {
            const int cin = nf + k * gc, cout = k < 4 ? gc : nf;
            packs.add(params[P.prdb(i) + k * 2], wp + P.w_rdb_f[i * 5 + k], cout, cin, 3, 3, (long)cin * 9, 9, 3, 1, 0);
        }
    if (P.family != RDDB_SRDN) packs.add(params[P.p_trunk_w], wp + P.w_trunk_f, nf, nf, 3, 3, (long)nf * 9, 9, 3, 1, 0);
    for (int s = 0; s < P.nup; ++s)
        for (int q = 0; q < 4; ++q)   // ConvTranspose2d weight [ci][co][2][2]; parity (a,b) = q: rows = co, k = ci
            packs.add(params[P.p_up0 + s], wp + P.w_up_f[s][q], nf, nf, 1, 1, 4, (long)nf * 4, 0, 0, q);
    for (int k = 0; k < P.nlw; ++k)
        packs.add(params[P.p_lg[k]], wp + P.lw_f[k], nf, nf, 3, 3, (long)nf * 9, 9, 3, 1, 0);
    packs.add(params[P.p_last_w], wp + P.w_last_f, c->out_ch, nf, 3, 3, (long)nf * 9, 9, 3, 1, 0);

    SG_REQUIRE(!(opt && opt->pack == 2) || (opt->wpack && opt->guard), "srcgan_rddbnet_forward: pack == 2 needs wpack and guard");
    if (do_pack) SG_TRY(packs.run((std::string(P.tag) + "_fwd").c_str(), params[0], st, pack_guard(opt)));

    // ---- input: NCHW f32 -> NHWC (channels zero-padded to 8)
    SG_TRY(srcgan_nchw_f32_to_nhwc(x_nchw, w8 + N.xin, B, c->in_ch, c->H, c->W, P.in_cs, dt, st));
    // conv_first (rddb.py:89,108).  The trunk input lives in channels [0,nf) of the first dense buffer so the
    // first RDB reads it in place and the global skip (rddb.py:110) reads it back later.
    TRef trunk_in = Abuf(0);
    TRef fea = P.ndn ? T_(N.fea0, nf) : trunk_in;
    SG_TRY(Conv(dt, 3, 3, 1).in(T_(N.xin, P.in_cs), B, c->H, c->W, P.in_cs).w(wp + P.w_first_f, params[P.p_first_b])
               .out(fea, c->H, c->W, nf).pad(1, 1).run(st));
    // optional HR->LR stages (build-defined RDDBNetA): 3x3 s2 p1 + bias + LeakyReLU
    for (int s = 0; s < P.ndn; ++s) {
        TRef o = (s == P.ndn - 1) ? trunk_in : T_(N.dn[s], nf);
        SG_TRY(Conv(dt, 3, 3, 2).in(fea, B, c->H >> s, c->W >> s, nf).w(wp + P.w_dn_f[s], params[P.p_dn0 + 2 * s + 1])
                   .out(o, c->H >> (s + 1), c->W >> (s + 1), nf).pad(1, 1).lrelu().run(st));
        fea = o;
    }
    if (N.rolling && P.nrr) { SG_HIP(to_home(trunk_in)); trunk_in = tref(w8 + N.home, P.kce, 0, P.plane_bytes); }
    // RRDB trunk (rddb.py:62-68,78-82).  The legacy RDDBNet computes it and throws it away (model.py:382-383): skipped.
    for (int i = 0; i < P.nrr; ++i) {
        for (int j = 0; j < 3; ++j) {
            const int r = i * 3 + j;
            TRef A = Abuf(r);
            for (int k = 0; k < 4; ++k) {
                const int cin = nf + k * gc;
                Conv cv(dt, 3, 3, 1);
                cv.in(A, B, H, W, cin).w(wp + P.w_rdb_f[r * 5 + k], params[P.prdb(r) + k * 2 + 1]).out(sl(A, cin), H, W, gc).pad(1, 1).lrelu();
                if (N.bm_bytes) cv.sign_out((char*)A.p + N.bm + (size_t)k * N.bm_bytes);
                SG_TRY(cv.run(st));
            }
            // conv5 + residual(s) -> channels [0,nf) of the next dense buffer (or the trunk output)
            const bool last = (r == P.nrr * 3 - 1);
            TRef dst = last ? T_(N.T, nf) : Abuf(r + 1);
            Conv cv(dt, 3, 3, 1);
            cv.in(A, B, H, W, P.C).w(wp + P.w_rdb_f[r * 5 + 4], params[P.prdb(r) + 4 * 2 + 1]).out(dst, H, W, nf).pad(1, 1);
            if (j < 2) cv.alpha(0.2f).res1(A, nf, 1.f);
            else cv.alpha(0.04f).res1(A, nf, 0.2f).res2(Abuf(i * 3), nf, 1.f);   // RRDB: 0.2*(0.2*x5 + x_rdb3) + x_rrdb
            SG_TRY(cv.run(st));
        }
        if (P.family == RDDB_SRDN && i == c->nb - 1) {       // SRDN: fea = fea + RRDB_encoder(fea) (srdn.py:70-71), in the decoder's first buffer
            TRef d0 = Abuf((i + 1) * 3);
            SG_TRY(srcgan_add_inplace_planes(d0.p, d0.cs, 0, d0.plane, trunk_in.p, trunk_in.cs, 0, trunk_in.plane, nullptr, 0, 0, 0, 0.f,
                                             (long)B * H * W, nf, dt, st));
            if (N.rolling) SG_HIP(to_home(d0));       // the decoder's input takes the encoder input's place
        }
    }
    if (P.family == RDDB_SRDN) {       // fea = fea + RRDB_decoder(fea) (srdn.py:72-73): T += fea1, then conv_last reads T (= U[0])
        TRef f1 = N.rolling ? trunk_in : Abuf(c->nb * 3), Tt = T_(N.T, nf);
        SG_TRY(srcgan_add_inplace_planes(Tt.p, Tt.cs, 0, 0, f1.p, f1.cs, 0, f1.plane, nullptr, 0, 0, 0, 0.f, (long)B * H * W, nf, dt, st));
    }
    // trunk_conv + global skip (rddb.py:109-110)
    if (P.has_trunk_conv)
        SG_TRY(Conv(dt, 3, 3, 1).in(T_(N.T, nf), B, H, W, nf).w(wp + P.w_trunk_f, params[P.p_trunk_b]).out(T_(N.U[0], nf), H, W, nf)
                   .pad(1, 1).res1(trunk_in, nf, 1.f).run(st));
    if (P.x2_tail) {
        // legacy tail (model.py:384-390, 427-439): [nearest x2 -> 3x3 conv -> LeakyReLU] stages, HRconv applied repeatedly
        TRef cur = P.family == RDDB_LEGACY ? trunk_in : T_(N.U[0], nf);
        for (int k = 0; k < P.ntail; ++k) {
            const RddbPlan::TailOp& o = P.tail[k];
            TRef dst = T_(N.tail[k], nf);
            if (o.conv)
                SG_TRY(Conv(dt, 3, 3, 1).in(cur, B, o.hin, o.win, nf).w(wp + P.lw_f[o.w], params[P.p_lg[o.w] + 1]).out(dst, o.hout, o.wout, nf)
                           .pad(1, 1).lrelu().run(st));
            else
                SG_TRY(srcgan_upsample2_nhwc(cur.p, cur.cs, cur.coff, cur.plane, dst.p, dst.cs, B, o.hin, o.win, nf, dt, st));
            cur = dst;
        }
        SG_HIP(hipMemsetAsync(w8 + N.out, 0, (size_t)B * P.HO * P.WO * P.out_cs * P.esz, (hipStream_t)st));
        SG_TRY(Conv(dt, 3, 3, 1).in(cur, B, P.HO, P.WO, nf).w(wp + P.w_last_f, params[P.p_last_b]).out(T_(N.out, P.out_cs), P.HO, P.WO, c->out_ch)
                   .pad(1, 1).run(st));
        SG_TRY(srcgan_nhwc_to_nchw_f32(w8 + N.out, y_nchw, B, c->out_ch, P.HO, P.WO, P.out_cs, 0, dt, st));
        return 0;
    }
    // up-sampler: ConvTranspose2d(k2,s2) + LeakyReLU == 4 x (1x1 conv -> stride-2 scatter) (rddb.py:93-97,111-112)
    for (int s = 0; s < P.nup; ++s) {
        const int h = H << s, w = W << s;
        // all four output parities in one launch (the input is read from HBM once: conv_igemm.hip, npar): the stage's four packs
        // are equal-sized and consecutive (rddb_plan), hence equally spaced
        Conv cv(dt, 1, 1, 1);
        cv.in(T_(N.U[s], nf), B, h, w, nf).w(wp + P.w_up_f[s][0]).out(T_(N.U[s + 1], nf), h, w, nf).scatter(2, 0, 0, 2 * h, 2 * w).lrelu();
        cv.d.npar = 4; cv.d.wpar_stride = (long)(P.w_up_f[s][1] - P.w_up_f[s][0]);
        if (N.um_bytes && s == P.nup - 1) cv.sign_out(w8 + N.um);       // LeakyReLU sign of the tensor conv_last reads
        SG_TRY(cv.run(st));
    }
    // conv_last (no bias, rddb.py:98,113) as a convolution to all out_cs = 8 padded channels: the packed weight rows beyond out_ch
    // are zero, so channels out_ch.. come out as the zeros the padding wants -- and the output is 16 bytes per pixel through the
    // vectorised epilogue (with Cout = 3 it took the per-element form: three 2-byte stores per pixel of a 1024x1024 image, and a
    // 268 MB memset in front; 0.67 ms + 0.06 ms per step at the bench size)
    SG_TRY(Conv(dt, 3, 3, 1).in(T_(N.U[P.nup], nf), B, P.HO, P.WO, nf).w(wp + P.w_last_f).out(T_(N.out, P.out_cs), P.HO, P.WO, P.out_cs)
               .pad(1, 1).run(st));
    SG_TRY(srcgan_nhwc_to_nchw_f32(w8 + N.out, y_nchw, B, c->out_ch, P.HO, P.WO, P.out_cs, 0, dt, st));
    return 0;
}

}  // namespace

static int rddb_forward(const srcgan_rddbnet_cfg* c, bool infer, const float* x_nchw, const float* const* params, void* ws,
                        float* y_nchw, const srcgan_net_opts* opt, void* st) {
    RddbPlan P;
    SG_TRY(rddb_plan(c, P));
    RddbNames N;
    if (infer) rddb_infer_names(c, P, N); else rddb_train_names(c, P, N);
    return RddbCall(c, P, N, params, ws, opt, st).forward(x_nchw, y_nchw);
}

extern "C" int srcgan_rddbnet_forward_ex(const srcgan_rddbnet_cfg* c, const float* x_nchw, const float* const* params,
                                         void* ws, float* y_nchw, const srcgan_net_opts* opt, void* st) {
    return rddb_forward(c, false, x_nchw, params, ws, y_nchw, opt, st);
}

// Inference forward: same launches, same kernels, same descriptors as srcgan_rddbnet_forward_ex apart from buffer addresses and
// the sign masks, which are not written.
extern "C" int srcgan_rddbnet_infer(const srcgan_rddbnet_cfg* c, const float* x_nchw, const float* const* params, void* ws,
                                    float* y_nchw, const srcgan_net_opts* opt, void* st) {
    return rddb_forward(c, true, x_nchw, params, ws, y_nchw, opt, st);
}

extern "C" int srcgan_rddbnet_forward(const srcgan_rddbnet_cfg* c, const float* x_nchw, const float* const* params,
                                      void* ws, float* y_nchw, void* st) {
    return srcgan_rddbnet_forward_ex(c, x_nchw, params, ws, y_nchw, nullptr, st);
}

namespace {

// ---- the backward, in stages that mirror the forward's order in reverse.  The running gradient of the trunk-resolution feature
// (dU0) and the three rotating dense gradient buffers (Pg) sit in the scratch, also between the calls of a phased backward.
struct RddbBwd : RddbCall {
    const RddbBwdPlan& Q;
    char* s8; float* const* grads;
    float* slab; float* colscr;
    const long npix_t;
    RddbBwd(const RddbCall& call, const RddbBwdPlan& Q_, void* scratch, float* const* grads_)
        : RddbCall(call), Q(Q_), s8((char*)scratch), grads(grads_), slab((float*)(s8 + Q_.slab)), colscr((float*)(s8 + Q_.colscr)),
          npix_t((long)B * H * W) {}
    TRef S_(size_t off, int cs) const { return tref(s8 + off, cs); }
    float* G(int idx) const { return grads[idx]; }
    TRef dout() const { return S_(Q.dout, P.out_cs); }
    TRef dU0() const { return S_(Q.dU[0], nf); }
    // Dense gradient buffers (3, rotating): Gd = [dy5 (nf) | dy4 | dy3 | dy2 | dy1] -- the mirror image of the forward
    // dense buffer.  Slice j of the block input gets its gradient from ONE conv over the channel prefix holding
    // dy5..dy_{j+1} (composite transposed weights), so every gradient element is written exactly once: no
    // read-modify-write accumulation, and the same prefix-read / slice-write pattern as forward.
    TRef Pg(int g) const { return tref(s8 + Q.Pg[g], P.kce, 0, P.plane_bytes); }
    int pack_dgrad(bool pack_dx) const;
    int output_plain() const;
    int output_tail() const;
    int trunk_entry() const;
    int rrdb_range(int r_lo, int r_hi) const;
    int input_side(float* dx_nchw) const;
};

// ---- packed dgrad weights (flipped / transposed views of the canonical tensors): ONE batched launch
int RddbBwd::pack_dgrad(bool pack_dx) const {
    PackList packs(dt, wp);
    const WLayout L = lay_dgrad_s1(nf, 3, 3);
    packs.add(params[P.p_last_w], wp + P.w_last_d, nf, c->out_ch, 3, 3, L);
    for (int s = 0; s < P.nup; ++s)   // deconv dgrad = 2x2 s2 conv over dy: rows = ci, k = co, tap = (a,b)
        packs.add(params[P.p_up0 + s], wp + P.w_up_d[s], nf, nf, 2, 2, (long)nf * 4, 4, 2, 1, 0);
    for (int k = 0; k < P.nlw; ++k)
        packs.add(params[P.p_lg[k]], wp + P.lw_d[k], nf, nf, 3, 3, L);
    if (P.family != RDDB_SRDN) packs.add(params[P.p_trunk_w], wp + P.w_trunk_d, nf, nf, 3, 3, L);
    SG_TRY(sg_fill_zero_guarded(wp + P.w_rdb_d0, P.w_rdb_dsz, pack_guard(opt), (hipStream_t)st));
    for (int r = 0; r < P.nrr * 3; ++r) {
        const float a5 = (r % 3 == 2) ? 0.04f : 0.2f;       // d(x5)/d(block out), RDB3 carries the RRDB 0.2 too
        for (int j = 0; j < 5; ++j) {
            const int rows = j == 0 ? nf : gc, ss = j == 0 ? 0 : nf + (j - 1) * gc, ktot = nf + (4 - j) * gc;
            for (int m = 5; m > j; --m) {                   // block of K coming from forward conv m
                const int cin_m = nf + (m - 1) * gc, cout_m = m == 5 ? nf : gc;
                const int k_off = m == 5 ? 0 : nf + (4 - m) * gc;
                packs.add(params[P.prdb(r) + (m - 1) * 2], wp + P.w_rdb_d[r * 5 + j], rows, cout_m, 3, 3,
                                               9, (long)cin_m * 9, -3, -1, (long)ss * 9 + 8, k_off, ktot, m == 5 ? a5 : 1.f);
            }
        }
    }
    for (int s = 0; s < P.ndn; ++s) P.dn_dgrad().pack(packs, params[P.p_dn0 + 2 * s], wp, P.w_dn_d[s]);
    if (pack_dx) packs.add(params[P.p_first_w], wp + P.w_first_d, c->in_ch, nf, 3, 3, lay_dgrad_s1(c->in_ch, 3, 3));
    return packs.run((std::string(P.tag) + (pack_dx ? "_bwd_dx" : "_bwd")).c_str(), params[0], st, pack_guard(opt));
}

// ---- output side of the ConvTranspose families: conv_last, then the up-sampler stages; leaves d(U[0]) in dU0
int RddbBwd::output_plain() const {
    // conv_last
    TRef Ul = T_(N.U[P.nup], nf);
    if (G(P.p_last_w))
        SG_TRY(wgrad_call(dt, dout(), P.HO, P.WO, c->out_ch, Ul, B, P.HO, P.WO, nf, 3, 3, 1, 1, 1, lay_fwd(nf, 3, 3), 1.f, slab, G(P.p_last_w), st));
    {
        Conv cv(dt, 3, 3, 1);
        cv.in(dout(), B, P.HO, P.WO, P.out_cs).w(wp + P.w_last_d).out(S_(Q.dU[P.nup], nf), P.HO, P.WO, nf).pad(1, 1);
        if (P.nup > 0) {                      // LeakyReLU after the last deconv
            if (N.um_bytes) { cv.sign_in(w8 + N.um); cv.d.mslope = 0.2f; }
            else cv.mask(Ul, 0);
        }
        SG_TRY(cv.run(st));
    }
    // up-sampler stages, last to first
    for (int s = P.nup - 1; s >= 0; --s) {
        const int h = H << s, w = W << s;
        TRef dHR = S_(Q.dU[s + 1], nf), Us = T_(N.U[s], nf);
        if (G(P.p_up0 + s))   // dW[ci][co][a][b] = sum x[y,x,ci] * dy[2y+a,2x+b,co]: wgrad with roles (dy := x, x := dy), k2 s2
            SG_TRY(wgrad_call(dt, Us, h, w, nf, dHR, B, 2 * h, 2 * w, nf, 2, 2, 2, 0, 0, WLayout{(long)nf * 4, 4, 2, 1, 0}, 1.f, slab, G(P.p_up0 + s), st));
        Conv cv(dt, 2, 2, 2);
        cv.in(dHR, B, 2 * h, 2 * w, nf).w(wp + P.w_up_d[s]).out(S_(Q.dU[s], nf), h, w, nf).pad(0, 0);
        if (s > 0) cv.mask(Us, 0);
        SG_TRY(cv.run(st));
    }
    return 0;
}

// ---- output side of the nearest-x2 tail families: conv_last (with bias), then the tail's op list; leaves d(tail input) in dU0.
// dcur = gradient w.r.t. an op's output, already times LeakyReLU' of that output.
int RddbBwd::output_tail() const {
    TRef tin = P.family == RDDB_LEGACY ? Abuf(0) : T_(N.U[0], nf);          // tail input (not an activation output)
    auto obuf = [&](int k) { return k < 0 ? tin : T_(N.tail[k], nf); };
    TRef Fl = obuf(P.ntail - 1);
    if (G(P.p_last_w))
        SG_TRY(wgrad_call(dt, dout(), P.HO, P.WO, c->out_ch, Fl, B, P.HO, P.WO, nf, 3, 3, 1, 1, 1, lay_fwd(nf, 3, 3), 1.f, slab, G(P.p_last_w), st, G(P.p_last_b)));
    else if (G(P.p_last_b)) SG_TRY(bias_grad(dt, dout(), (long)B * P.HO * P.WO, c->out_ch, 1.f, G(P.p_last_b), colscr, st));
    int pp = 0;
    auto nextbuf = [&](int k_in) { if (k_in < 0) return dU0(); pp ^= 1; return S_(Q.dU[1 + pp], nf); };   // k_in: index of the op whose output gets this gradient
    TRef dcur = nextbuf(P.ntail - 1);
    {
        Conv cv(dt, 3, 3, 1);
        cv.in(dout(), B, P.HO, P.WO, P.out_cs).w(wp + P.w_last_d).out(dcur, P.HO, P.WO, nf).pad(1, 1);
        if (P.ntail > 0 && P.tail[P.ntail - 1].conv) cv.mask(Fl, 0);
        SG_TRY(cv.run(st));
    }
    bool seen[3] = {false, false, false};
    for (int k = P.ntail - 1; k >= 0; --k) {
        const RddbPlan::TailOp& o = P.tail[k];
        TRef xin_k = obuf(k - 1);
        const bool in_act = k > 0 && P.tail[k - 1].conv;          // the op's input is a LeakyReLU output
        TRef dst = nextbuf(k - 1);
        if (o.conv) {
            const int pw = P.p_lg[o.w];
            if (G(pw)) SG_TRY(wgrad_call(dt, dcur, o.hout, o.wout, nf, xin_k, B, o.hin, o.win, nf, 3, 3, 1, 1, 1, lay_fwd(nf, 3, 3), 1.f, slab, G(pw), st, G(pw + 1), seen[o.w] ? 1 : 0));
            else if (G(pw + 1)) SG_REQUIRE(false, "rddbnet (legacy): a shared convolution's bias gradient needs its weight gradient too");
            seen[o.w] = true;
            Conv cv(dt, 3, 3, 1);
            cv.in(dcur, B, o.hout, o.wout, nf).w(wp + P.lw_d[o.w]).out(dst, o.hin, o.win, nf).pad(1, 1);
            if (in_act) cv.mask(xin_k, 0);
            SG_TRY(cv.run(st));
        } else {
            // nearest x2 backward = 2x2 block sums; the up-sampled tensor's own LeakyReLU' (if any) is applied at its resolution
            SG_REQUIRE(xin_k.plane == 0 || !in_act, "rddbnet (legacy): unexpected blocked activation");
            SG_TRY(srcgan_sum2x2_nhwc(dcur.p, dcur.cs, dst.p, dst.cs, in_act ? xin_k.p : nullptr, xin_k.cs, 0.2f, B, o.hin, o.win, nf, dt, st));
        }
        dcur = dst;
    }
    // unused parameters of the forward (upconv2 in mode x2): their gradient is zero here, None in the reference
    for (int k = 0; k < P.nlw; ++k)
        if (!seen[k]) {
            if (G(P.p_lg[k])) SG_HIP(hipMemsetAsync(G(P.p_lg[k]), 0, (size_t)nf * nf * 9 * sizeof(float), (hipStream_t)st));
            if (G(P.p_lg[k] + 1)) SG_HIP(hipMemsetAsync(G(P.p_lg[k] + 1), 0, (size_t)nf * sizeof(float), (hipStream_t)st));
        }
    return 0;
}

// ---- from dU0 into channels [0,nf) of the first dense gradient buffer
int RddbBwd::trunk_entry() const {
    if (!P.has_trunk_conv) {
        // SRDN: d(decoder output) = d(fea2) = dU0 itself (no trunk_conv)
        TRef g0 = Pg(0), d0 = dU0();
        SG_HIP(hipMemsetAsync(g0.p, 0, (size_t)cdiv(nf, P.kce) * P.plane_bytes, (hipStream_t)st));
        return srcgan_add_inplace_planes(g0.p, g0.cs, 0, g0.plane, d0.p, d0.cs, 0, 0, nullptr, 0, 0, 0, 0.f, npix_t, nf, dt, st);
    }
    // U0 = fea + trunk_conv(T): d(trunk_conv out) = dU0, d(fea) += dU0 (joined on the input side)
    if (G(P.p_trunk_w))
        SG_TRY(wgrad_call(dt, dU0(), H, W, nf, T_(N.T, nf), B, H, W, nf, 3, 3, 1, 1, 1, lay_fwd(nf, 3, 3), 1.f, slab, G(P.p_trunk_w), st, G(P.p_trunk_b)));
    else if (G(P.p_trunk_b)) SG_TRY(bias_grad(dt, dU0(), npix_t, nf, 1.f, G(P.p_trunk_b), colscr, st));
    return Conv(dt, 3, 3, 1).in(dU0(), B, H, W, nf).w(wp + P.w_trunk_d).out(Pg(0), H, W, nf).pad(1, 1).run(st);
}

// ---- the RRDBs [r_lo, r_hi), last to first
int RddbBwd::rrdb_range(int r_lo, int r_hi) const {
    for (int i = r_hi - 1; i >= r_lo; --i) {
        if (P.family == RDDB_SRDN && i == c->nb - 1) {
            // between the stacks: d(fea1) = d(fea2) + d(decoder input); it feeds the encoder's output AND the skip around it
            TRef g0 = Pg(0), d0 = dU0();
            SG_TRY(srcgan_add_inplace_planes(g0.p, g0.cs, 0, g0.plane, d0.p, d0.cs, 0, 0, nullptr, 0, 0, 0, 0.f, npix_t, nf, dt, st));
            SG_HIP(hipMemsetAsync(d0.p, 0, (size_t)npix_t * nf * P.esz, (hipStream_t)st));
            SG_TRY(srcgan_add_inplace_planes(d0.p, d0.cs, 0, 0, g0.p, g0.cs, 0, g0.plane, nullptr, 0, 0, 0, 0.f, npix_t, nf, dt, st));
        }
        for (int j3 = 2; j3 >= 0; --j3) {                  // RDB3, RDB2, RDB1 use Pg(0), Pg(1), Pg(2)
            const int r = i * 3 + j3, g = 2 - j3;
            TRef A = Abuf(r), Gd = Pg(g), nxt = Pg((g + 1) % 3);
            const float a5 = (j3 == 2) ? 0.04f : 0.2f;     // folded into the packed conv5 block; wgrad/bias use it as alpha
            const float bres = (j3 == 2) ? 0.2f : 1.f;     // block-input residual: d(in) += bres * d(out)
            const int pbase = P.prdb(r);
            auto slice_grad = [&](int m) -> int {
                // gradient of input slice j = m-1 from [dy5 .. dy_m]
                const int j = m - 1, ktot = nf + (4 - j) * gc;
                Conv cv(dt, 3, 3, 1);
                cv.in(Gd, B, H, W, ktot).w(wp + P.w_rdb_d[r * 5 + j]).pad(1, 1);
                if (j > 0) {
                    // slice x_j is a LeakyReLU output: multiply by its derivative -> this IS dy_j
                    cv.out(sl(Gd, nf + (4 - j) * gc), H, W, gc);
                    if (N.bm_bytes) { cv.sign_in((const char*)A.p + N.bm + (size_t)(j - 1) * N.bm_bytes); cv.d.mslope = 0.2f; }
                    else cv.mask(sl(A, nf + (j - 1) * gc), 0);
                } else {
                    cv.out(nxt, H, W, nf).res1(Gd, nf, bres);
                    if (j3 == 0) cv.res2(nxt, nf, 1.f);     // RRDB skip; nxt == Pg(0) still holds d(out_rrdb): in-place, same element
                }
                return cv.run(st);
            };
            for (int m = 5; m >= 2; --m) SG_TRY(slice_grad(m));
            // weight + bias gradients of the block's five convs in ONE pass over (Gd, A) -- wgrad_dense.hip.  They need dy5..dy1, not the
            // block-input gradient: that convolution (m = 1) runs AFTER them, so that the next block's first gradient-slice convolution
            // (64 -> 32, memory-bound) follows a convolution instead of the weight-gradient kernels: 65 -> 57 us per launch, -0.4 ms per
            // step (same-box A/B of the two orders)
            {
                srcgan_wgrad_dense_desc wd;
                memset(&wd, 0, sizeof(wd));
                wd.dy = Gd.p; wd.dy_cs = Gd.cs; wd.dy_coff = Gd.coff; wd.dy_plane = Gd.plane; wd.G = P.C;
                wd.x = A.p; wd.x_cs = A.cs; wd.x_coff = A.coff; wd.x_plane = A.plane; wd.C = P.C;
                wd.slab = slab; wd.dtype = dt; wd.B = B; wd.H = H; wd.W = W;
                bool any = false;
                for (int m = 5; m >= 1; --m) {
                    srcgan_wgrad_seg& sg = wd.seg[wd.nseg++];
                    sg.g0 = m == 5 ? 0 : nf + (4 - m) * gc; sg.g1 = sg.g0 + (m == 5 ? nf : gc);
                    sg.grad = G(pbase + 2 * (m - 1)); sg.bias = G(pbase + 2 * (m - 1) + 1);
                    sg.Cin = nf + (m - 1) * gc; sg.alpha = m == 5 ? a5 : 1.f;
                    any = any || sg.grad || sg.bias;
                }
                if (any) SG_TRY(srcgan_wgrad_dense(&wd, st));
            }
            SG_TRY(slice_grad(1));
        }
    }
    return 0;
}

// ---- input side: the global-skip join, the down stages, conv_first, dx
int RddbBwd::input_side(float* dx_nchw) const {
    TRef dfea = dU0();
    if (P.nrr) {
        // gradient w.r.t. the trunk input feature = dcur + dU0 (global skip); for the HR->LR variant the trunk input
        // is a LeakyReLU output, so its derivative is applied in the same pass.
        // (dU0 is not needed any more: the join is accumulated into it, NHWC)
        TRef dcur = Pg(0), trunk_in = Abuf(0);
        SG_TRY(srcgan_add_inplace_planes(dfea.p, dfea.cs, dfea.coff, dfea.plane, dcur.p, dcur.cs, dcur.coff, dcur.plane,
                                         P.ndn ? trunk_in.p : nullptr, trunk_in.cs, 0, trunk_in.plane, 0.2f, npix_t, nf, dt, st));
    }
    for (int s = P.ndn - 1; s >= 0; --s) {     // 3x3 s2 p1 stages of RDDBNetA, last to first
        const int hi = c->H >> s, wi = c->W >> s, ho = hi / 2, wo = wi / 2;
        TRef xin_s = s == 0 ? T_(N.fea0, nf) : T_(N.dn[s - 1], nf);
        const int pw = P.p_dn0 + 2 * s;
        if (G(pw)) SG_TRY(wgrad_call(dt, dfea, ho, wo, nf, xin_s, B, hi, wi, nf, 3, 3, 2, 1, 1, lay_fwd(nf, 3, 3), 1.f, slab, G(pw), st, G(pw + 1)));
        else if (G(pw + 1)) SG_TRY(bias_grad(dt, dfea, (long)B * ho * wo, nf, 1.f, G(pw + 1), colscr, st));
        TRef dst = S_(Q.dfea_dn[s], nf);
        SG_TRY(P.dn_dgrad().run(dt, dfea, B, ho, wo, dst, hi, wi, wp, P.w_dn_d[s], TNULL, s > 0 ? xin_s : TNULL, false, st));
        dfea = dst;
    }
    // conv_first
    TRef xin = T_(N.xin, P.in_cs);
    if (G(P.p_first_w))
        SG_TRY(wgrad_call(dt, dfea, c->H, c->W, nf, xin, B, c->H, c->W, c->in_ch, 3, 3, 1, 1, 1, lay_fwd(c->in_ch, 3, 3), 1.f, slab, G(P.p_first_w), st, G(P.p_first_b)));
    else if (G(P.p_first_b)) SG_TRY(bias_grad(dt, dfea, (long)B * c->H * c->W, nf, 1.f, G(P.p_first_b), colscr, st));
    if (dx_nchw) {
        TRef dxin = S_(Q.dxin, P.in_cs);
        SG_HIP(hipMemsetAsync(dxin.p, 0, (size_t)B * c->H * c->W * P.in_cs * P.esz, (hipStream_t)st));
        SG_TRY(Conv(dt, 3, 3, 1).in(dfea, B, c->H, c->W, nf).w(wp + P.w_first_d).out(dxin, c->H, c->W, c->in_ch).pad(1, 1).run(st));
        SG_TRY(srcgan_nhwc_to_nchw_f32(dxin.p, dx_nchw, B, c->in_ch, c->H, c->W, P.in_cs, 0, dt, st));
    }
    return 0;
}

}  // namespace

extern "C" int srcgan_rddbnet_backward_ex(const srcgan_rddbnet_cfg* c, const float* dy_nchw, const float* const* params,
                                          void* ws, void* scratch, float* const* grads, float* dx_nchw, const srcgan_net_opts* opt, void* st) {
    RddbPlan P;
    SG_TRY(rddb_plan(c, P));
    RddbNames N;
    rddb_train_names(c, P, N);
    RddbBwdPlan Q;
    rddb_bwd_plan(c, P, Q);
    SG_REQUIRE(dy_nchw && params && ws && scratch && grads, "srcgan_rddbnet_backward: null pointer");
    SG_REQUIRE(((uintptr_t)ws % 256) == 0 && ((uintptr_t)scratch % 256) == 0, "srcgan_rddbnet_backward: buffers must be 256-byte aligned");
    // Phased backward (data parallel: the gradients of the RRDBs a phase covers are final when it returns, so their all-reduce
    // starts while earlier blocks still compute).  A call handles the RRDBs [lo, hi), last to first; the call with hi == nrr also
    // runs everything behind the trunk (conv_last, up-sampler, trunk_conv), the call with lo == 0 everything in front of it
    // (conv_first / down-sampling stages, dx).  Calls must come in descending, gap-free order on one stream with the same
    // scratch: the running gradient sits in the scratch between them.  srcgan_rddbnet_phase_params names a phase's parameters.
    int r_lo = 0, r_hi = P.nrr;
    if (opt && opt->rrdb_hi > 0) { r_lo = opt->rrdb_lo; r_hi = opt->rrdb_hi; }
    SG_REQUIRE(r_lo >= 0 && r_lo <= r_hi && r_hi <= P.nrr, "srcgan_rddbnet_backward: RRDB range [%d,%d) outside [0,%d)", r_lo, r_hi, P.nrr);
    SG_REQUIRE(P.nrr > 0 || (r_lo == 0), "srcgan_rddbnet_backward: a network without a trunk has one phase");
    const bool first_phase = r_hi == P.nrr, last_phase = r_lo == 0;
    const RddbBwd K(RddbCall(c, P, N, params, ws, opt, st), Q, scratch, grads);
    if (first_phase) {
        const bool pack_dx = dx_nchw || (opt && opt->wpack);       // a persistent pack serves later calls that may want dx
        if (K.do_pack) SG_TRY(K.pack_dgrad(pack_dx));
        // dy: NCHW f32 -> NHWC
        SG_TRY(srcgan_nchw_f32_to_nhwc(dy_nchw, K.dout().p, c->B, c->out_ch, P.HO, P.WO, P.out_cs, c->dtype, st));
        SG_TRY(P.x2_tail ? K.output_tail() : K.output_plain());
        if (P.nrr) SG_TRY(K.trunk_entry());
    }
    SG_TRY(K.rrdb_range(r_lo, r_hi));
    if (last_phase) SG_TRY(K.input_side(dx_nchw));
    return 0;
}

extern "C" int srcgan_rddbnet_backward(const srcgan_rddbnet_cfg* c, const float* dy_nchw, const float* const* params,
                                       void* ws, void* scratch, float* const* grads, float* dx_nchw, void* st) {
    return srcgan_rddbnet_backward_ex(c, dy_nchw, params, ws, scratch, grads, dx_nchw, nullptr, st);
}

// ======================================================================================== NLayerDiscriminator
namespace {
// One convolution layer as the kernels run it.  The first layer of an even-sized input runs in space-to-depth form (blocks of 2x2
// pixels x 8 channels, srcgan_nchw_f32_to_s2d) and is described as what it then is: a 2x2 s1 p0 convolution over (H/2+1) x (W/2+1)
// blocks of 32 channels with a folded weight.  Only the layout conversions, the folded pack jobs and the unfolding of the weight
// gradient know the difference.
enum DPost { D_LRELU, D_BNORM, D_INORM, D_FINAL };       // what follows the convolution (D_FINAL: nothing, the 1-channel prediction map)
struct DLayer {
    int k, stride, pad;
    int H, W, Cin, in_cs;            // input; Cin: input channels of the weight as run; in_cs: channel stride = the forward's (zero-padded) reduction length
    int OH, OW, Cout, out_cs;        // output; out_cs: channel stride = the input gradient's reduction length
    DPost post;
    bool folded;                     // the weight as run is the space-to-depth fold of the canonical [Cout][in_ch][4][4]
    int pw, pb, pg, pbeta, bn_idx;   // parameter indices (-1 if absent); index among the BatchNorm layers
    size_t X, Y, Z, stat;            // workspace: input, output, convolution output in front of a normalisation, its statistics
    size_t wf, wf_bytes, wd[4], wd_bytes;       // packed weights: forward; input gradient (stride 1: wd[0], wd_bytes; stride 2: one per parity)
    bool normed() const { return post == D_BNORM || post == D_INORM; }
    S2Dgrad s2() const { return S2Dgrad{k, pad, Cin, Cout}; }
};
struct DPlan {
    int esz, L, nparams, cmax;         // L convs; cmax: widest channel count (>= 8)
    bool inorm;                        // norm_layer = InstanceNorm2d: the normalised layers are GroupNorm(G = C) without affine part
    DLayer y[8];
    size_t colscr, gnscr, wpk, total;  // gnscr: GroupNorm scratch (instance norm)
    bool s2d() const { return y[0].folded; }
};

static int d_plan(const srcgan_nlayerd_cfg* c, DPlan& P) {
    SG_REQUIRE(c, "nlayerd: null cfg");
    SG_REQUIRE(sg_dtype_ok(c->dtype), "nlayerd: bad dtype");
    SG_REQUIRE(c->in_ch > 0 && c->in_ch <= 8, "nlayerd: input_nc must be in 1..8");
    SG_REQUIRE(c->ndf > 0 && c->ndf % 8 == 0, "nlayerd: ndf must be a multiple of 8");
    SG_REQUIRE(c->n_layers >= 1 && c->n_layers <= 5, "nlayerd: n_layers must be in 1..5");
    SG_REQUIRE(c->B > 0 && c->H > 0 && c->W > 0, "nlayerd: bad B/H/W");
    SG_REQUIRE(c->norm == 0 || c->norm == 1, "nlayerd: norm must be 0 (BatchNorm2d) or 1 (InstanceNorm2d)");
    P.inorm = c->norm == 1;
    P.esz = c->dtype == SRCGAN_F32 ? 4 : 2; P.L = c->n_layers + 2;
    // the module's layers (model/model.py:612-634): 4x4 p1, stride 2 for the first n_layers, ndf * min(2^l, 8) channels, 1 at the end
    int n = 0, nbn = 0, h = c->H, w = c->W, cin = c->in_ch;
    P.cmax = 8;
    for (int l = 0; l < P.L; ++l) {
        DLayer& y = P.y[l];
        const bool last = l == P.L - 1, nrm = l >= 1 && !last, bn = nrm && !P.inorm;
        y.k = 4; y.stride = l < c->n_layers ? 2 : 1; y.pad = 1; y.folded = false;
        y.H = h; y.W = w; y.Cin = cin; y.in_cs = l == 0 ? img_cs(cin) : cin;
        y.OH = (h + 2 - 4) / y.stride + 1; y.OW = (w + 2 - 4) / y.stride + 1;
        SG_REQUIRE(y.OH > 0 && y.OW > 0, "nlayerd: input %dx%d too small for %d layers", c->H, c->W, c->n_layers);
        y.Cout = last ? 1 : c->ndf * (l < 3 ? 1 << l : 8); y.out_cs = last ? 8 : y.Cout;
        y.post = last ? D_FINAL : !nrm ? D_LRELU : P.inorm ? D_INORM : D_BNORM;
        y.pw = n++;
        y.pb = (!nrm || P.inorm) ? n++ : -1;
        y.pg = bn ? n++ : -1;
        y.pbeta = bn ? n++ : -1;
        y.bn_idx = bn ? nbn++ : -1;
        if (y.Cout > P.cmax) P.cmax = y.Cout;
        h = y.OH; w = y.OW; cin = y.Cout;
    }
    P.nparams = n;
    static const bool no_s2d = sg_env("SRCGAN_NO_S2D") != nullptr;
    if (!no_s2d && c->H % 2 == 0 && c->W % 2 == 0) {
        DLayer& y = P.y[0];
        y.folded = true; y.k = 2; y.stride = 1; y.pad = 0; y.H = c->H / 2 + 1; y.W = c->W / 2 + 1; y.Cin = y.in_cs = 32;
    }
    const size_t e = P.esz, B = c->B;
    Bump b, wb;      // activations; packed weights (forward: rows = Cout, k = in_cs; input gradient: rows = Cin, k = out_cs)
    P.y[0].X = b.take(B * P.y[0].H * P.y[0].W * P.y[0].in_cs * e);
    for (int l = 0; l < P.L; ++l) {
        DLayer& y = P.y[l];
        y.wf = wb.take(y.wf_bytes = srcgan_packed_weight_bytes(y.Cout, y.in_cs, y.k * y.k, c->dtype));
        y.wd_bytes = y.stride == 1 ? srcgan_packed_weight_bytes(y.Cin, y.out_cs, y.k * y.k, c->dtype) : 0;     // stride 2: four packs, S2Dgrad
        if (y.stride == 1) y.wd[0] = wb.take(y.wd_bytes); else y.s2().plan(wb, c->dtype, y.wd);
        const size_t sz = B * y.OH * y.OW * y.out_cs * e;
        y.Y = b.take(sz);
        if (y.normed()) {      // BatchNorm: mean[C], var[C], rstd[C]; instance norm: {mean, rstd}[B][C]
            y.Z = b.take(sz);
            y.stat = b.take((P.inorm ? (size_t)2 * B * y.Cout : (size_t)3 * y.Cout) * sizeof(float));
        }
        if (l + 1 < P.L) P.y[l + 1].X = y.Y;
    }
    P.gnscr = 0;
    if (P.inorm) {
        SG_REQUIRE(P.cmax <= 1024 && P.cmax % (16 / (int)e) == 0 && 256 % (P.cmax / (16 / (int)e)) == 0, "nlayerd: InstanceNorm2d needs channel counts that are powers of two up to 1024");
        P.gnscr = b.take(srcgan_gn_scratch_floats(c->B, P.cmax) * sizeof(float));
    }
    P.colscr = b.take((size_t)2 * srcgan_col_reduce_blocks((long)B * P.y[0].OH * P.y[0].OW) * P.cmax * sizeof(float));
    P.wpk = b.off;
    P.total = align_up(P.wpk + wb.off + 256, 256);
    return 0;
}

struct DBwdPlan { size_t dO, g[2], dxin, slab, colscr, sums, gfold, gnscr, total; };
static void d_bwd_plan(const srcgan_nlayerd_cfg* c, const DPlan& P, DBwdPlan& Q) {
    const size_t e = P.esz, B = c->B;
    const DLayer& y0 = P.y[0]; const DLayer& yl = P.y[P.L - 1];
    Bump b;
    Q.dO = b.take(B * yl.OH * yl.OW * yl.out_cs * e);
    size_t mx = 0, slab = 0;       // largest gradient of a hidden activation (two buffers alternate); largest weight-gradient slab
    for (int l = 0; l < P.L; ++l) {
        const DLayer& y = P.y[l];
        if (l < P.L - 1) mx = std::max(mx, B * y.OH * y.OW * y.Cout * e);
        slab = std::max(slab, wgrad_slab(c->B, y.OH, y.OW, y.Cout, y.Cin, y.k, y.k, y.stride));
    }
    Q.g[0] = b.take(mx); Q.g[1] = b.take(mx);
    Q.dxin = b.take(B * y0.H * y0.W * y0.in_cs * e);
    Q.gfold = b.take((size_t)y0.Cout * 32 * 4 * sizeof(float));
    Q.slab = b.take(slab);
    Q.colscr = b.take((size_t)2 * srcgan_col_reduce_blocks((long)B * y0.OH * y0.OW) * P.cmax * sizeof(float));
    Q.sums = b.take((size_t)2 * P.cmax * sizeof(float));
    Q.gnscr = P.inorm ? b.take(srcgan_gn_scratch_floats(c->B, P.cmax) * sizeof(float)) : 0;
    Q.total = b.off + 256;
}

// ---- one native call on the discriminator, in named steps (a forward call has no scratch, gradients or backward plan)
struct DCall {
    const srcgan_nlayerd_cfg* c; const DPlan& P; const float* const* params; const srcgan_net_opts* opt; void* st;
    const int dt, B;
    char* w8;
    char* wp;            // packed weights: a persistent buffer of the caller's or a region of this call's workspace
    bool do_pack;
    const DBwdPlan* Q; char* s8; float* const* grads;
    DCall(const srcgan_nlayerd_cfg* c_, const DPlan& P_, const float* const* params_, void* ws, const srcgan_net_opts* opt_, void* st_,
          const DBwdPlan* Q_ = nullptr, void* scratch = nullptr, float* const* grads_ = nullptr)
        : c(c_), P(P_), params(params_), opt(opt_), st(st_), dt(c_->dtype), B(c_->B), w8((char*)ws),
          wp((opt_ && opt_->wpack) ? (char*)opt_->wpack : (char*)ws + P_.wpk), do_pack(!(opt_ && opt_->wpack) || opt_->pack),
          Q(Q_), s8((char*)scratch), grads(grads_) {}
    TRef X(const DLayer& y) const { return tref(w8 + y.X, y.in_cs); }
    TRef Y(const DLayer& y) const { return tref(w8 + y.Y, y.out_cs); }
    float* W(size_t off) const { return (float*)(w8 + off); }
    float* S(size_t off) const { return (float*)(s8 + off); }
    int pack_forward() const {
        PackList packs(dt, wp);
        for (int l = 0; l < P.L; ++l) {
            const DLayer& y = P.y[l];
            if (y.folded) {
                // W[co][c][2ty+dy][2tx+dx] -> k = (dy,dx,c8), taps (ty,tx): one part per (dy,dx); channels c >= Cin stay zero
                SG_TRY(sg_fill_zero_guarded(wp + y.wf, y.wf_bytes, pack_guard(opt), (hipStream_t)st));
                for (int q = 0; q < 4; ++q)
                    packs.add(params[y.pw], wp + y.wf, y.Cout, c->in_ch, 2, 2, (long)c->in_ch * 16, 16, 8, 2, (q >> 1) * 4 + (q & 1), q * 8, 32);
            } else
                packs.add(params[y.pw], wp + y.wf, y.Cout, y.Cin, y.k, y.k, lay_fwd(y.Cin, y.k, y.k));
        }
        return packs.run(P.s2d() ? "d_fwd_s2d" : "d_fwd", params[0], st, pack_guard(opt));
    }
    // Z -> Y: BatchNorm2d (batch statistics in training mode, running statistics otherwise) or InstanceNorm2d, then LeakyReLU
    int norm_forward(const DLayer& y, float* const* bn_running, int64_t* const* bn_nbt) const {
        const int C = y.Cout, bi = y.bn_idx;
        const long npix = (long)B * y.OH * y.OW;
        if (y.post == D_INORM)          // no affine part, instance statistics in either mode
            return srcgan_gn_forward(w8 + y.Z, C, nullptr, 0, w8 + y.Y, C, nullptr, nullptr, W(y.stat), B, (long)y.OH * y.OW, C, C, 1e-5f, 1, 0.2f, dt, W(P.gnscr), st);
        float* mean = W(y.stat); float* var = mean + C; float* rstd = var + C;
        if (c->training) {
            SG_TRY(srcgan_col_reduce(3, w8 + y.Z, C, 0, nullptr, 0, 0, nullptr, nullptr, npix, C, 1.f, mean, var, W(P.colscr), dt, st));      // one pass: mean and variance
            SG_TRY(srcgan_bn_finalize(mean, var, rstd, bn_running ? bn_running[2 * bi] : nullptr, bn_running ? bn_running[2 * bi + 1] : nullptr,
                                      bn_nbt ? bn_nbt[bi] : nullptr, C, npix, 0.1f, 1e-5f, st));
        } else {
            SG_REQUIRE(bn_running, "srcgan_nlayerd_forward: eval mode needs running statistics");
            SG_TRY(srcgan_bn_eval_rstd(bn_running[2 * bi + 1], rstd, C, 1e-5f, st));
            mean = bn_running[2 * bi];
        }
        return srcgan_bn_apply_lrelu(w8 + y.Z, w8 + y.Y, mean, rstd, params[y.pg], params[y.pbeta], npix, C, C, 0.2f, dt, st);
    }
    int forward(const float* x_nchw, float* const* bn_running, int64_t* const* bn_nbt, float* y_nchw) const {
        if (do_pack) SG_TRY(pack_forward());
        const DLayer& y0 = P.y[0]; const DLayer& yl = P.y[P.L - 1];
        if (P.s2d()) SG_TRY(srcgan_nchw_f32_to_s2d(x_nchw, w8 + y0.X, B, c->in_ch, c->H, c->W, dt, st));
        else SG_TRY(srcgan_nchw_f32_to_nhwc(x_nchw, w8 + y0.X, B, c->in_ch, c->H, c->W, y0.in_cs, dt, st));
        for (int l = 0; l < P.L; ++l) {     // conv + bias + LeakyReLU, conv -> norm -> LeakyReLU ..., conv + bias (model/model.py:612-634)
            const DLayer& y = P.y[l];
            Conv cv(dt, y.k, y.k, y.stride);
            cv.in(X(y), B, y.H, y.W, y.in_cs).w(wp + y.wf, y.pb >= 0 ? params[y.pb] : nullptr).pad(y.pad, y.pad);
            cv.out(y.normed() ? tref(w8 + y.Z, y.Cout) : Y(y), y.OH, y.OW, y.Cout);
            if (y.post == D_LRELU) cv.lrelu();
            if (y.post == D_FINAL) SG_HIP(hipMemsetAsync(w8 + y.Y, 0, (size_t)B * y.OH * y.OW * y.out_cs * P.esz, (hipStream_t)st));     // padded with zeros to out_cs
            SG_TRY(cv.run(st));
            if (y.normed()) SG_TRY(norm_forward(y, bn_running, bn_nbt));
        }
        return srcgan_nhwc_to_nchw_f32(w8 + yl.Y, y_nchw, B, 1, yl.OH, yl.OW, yl.out_cs, 0, dt, st);
    }
    // ---- backward steps.  dcur = gradient w.r.t. a layer's output, already times LeakyReLU' of that output (the mask is fused in
    // the input-gradient convolution that produced it).  Packed input-gradient weights: the first layer's only if someone may ask for dx
    int pack_dgrad(bool pack_dx) const {
        PackList packs(dt, wp);
        for (int l = pack_dx ? 0 : 1; l < P.L; ++l) {
            const DLayer& y = P.y[l];
            if (y.folded) {
                // dX'[j,i,(dy,dx,c)] = sum_{u,v,co} dY[j-1+u, i-1+v, co] * W[co][c][2(1-u)+dy][2(1-v)+dx]: rows (dy,dx,c8), k = co, 2x2 taps.
                // The rows of one (dy,dx) are a strided slice of the weight: one part per (dy,dx) and per half of k (so that no part
                // is a whole matrix, which would zero-fill all 32 rows of its view), written at row offset (dy*2+dx)*8.
                const int cin = c->in_ch, cout = y.Cout, kce = 64 / P.esz;
                SG_TRY(sg_fill_zero_guarded(wp + y.wd[0], y.wd_bytes, pack_guard(opt), (hipStream_t)st));
                for (int q = 0; q < 4; ++q)
                    for (int hk = 0; hk < 2; ++hk)
                        packs.add(params[y.pw], wp + y.wd[0] + (size_t)q * 8 * kce * P.esz, cin, cout / 2, 2, 2, 16, (long)cin * 16, -8, -2,
                                  10 + (q >> 1) * 4 + (q & 1) + (long)hk * (cout / 2) * cin * 16, hk * (cout / 2), cout);
            } else if (y.stride == 1)
                packs.add(params[y.pw], wp + y.wd[0], y.Cin, y.Cout, y.k, y.k, lay_dgrad_s1(y.Cin, y.k, y.k));
            else
                y.s2().pack(packs, params[y.pw], wp, y.wd);
        }
        return packs.run(P.s2d() ? (pack_dx ? "d_bwd_dx_s2d" : "d_bwd_s2d") : (pack_dx ? "d_bwd_dx" : "d_bwd"), params[0], st, pack_guard(opt));
    }
    // dcur: d/d(normalised output) -> d/d(convolution output), in place; BatchNorm's gamma and beta gradients
    int norm_backward(const DLayer& y, TRef dcur) const {
        const int C = y.Cout;
        const long npix = (long)B * y.OH * y.OW;
        if (y.post == D_INORM)          // per (image, channel)
            return srcgan_gn_backward(dcur.p, dcur.cs, nullptr, 0, w8 + y.Z, C, nullptr, W(y.stat), dcur.p, dcur.cs, nullptr, 0, 0,
                                      nullptr, nullptr, 0, 0.2f, B, (long)y.OH * y.OW, C, C, dt, S(Q->gnscr), st);
        if (y.post != D_BNORM) return 0;
        // BatchNorm (training mode): needs sum g, sum g*xhat
        float* mean = W(y.stat); float* rstd = mean + 2 * C; float* sums = S(Q->sums);
        SG_TRY(srcgan_col_reduce(2, dcur.p, dcur.cs, 0, w8 + y.Z, C, 0, mean, rstd, npix, C, 1.f, sums, sums + C, S(Q->colscr), dt, st));
        if (grads[y.pbeta]) SG_HIP(hipMemcpyAsync(grads[y.pbeta], sums, C * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)st));
        if (grads[y.pg]) SG_HIP(hipMemcpyAsync(grads[y.pg], sums + C, C * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)st));
        return srcgan_bn_bwd_apply(dcur.p, w8 + y.Z, dcur.p, mean, rstd, params[y.pg], sums, sums + C, npix, C, C, dt, st);
    }
    // weight and bias gradient (a folded weight's gradient is taken in the folded form, then unfolded to [Cout][in_ch][4][4])
    int param_grads(const DLayer& y, TRef dcur) const {
        if (grads[y.pw]) {
            float* g = y.folded ? S(Q->gfold) : grads[y.pw];
            SG_TRY(wgrad_call(dt, dcur, y.OH, y.OW, y.Cout, X(y), B, y.H, y.W, y.Cin, y.k, y.k, y.stride, y.pad, y.pad, lay_fwd(y.Cin, y.k, y.k), 1.f, S(Q->slab), g, st));
            if (y.folded) SG_TRY(srcgan_s2d_wgrad_unfold(g, grads[y.pw], y.Cout, c->in_ch, 0, st));
        }
        if (y.pb >= 0 && grads[y.pb]) SG_TRY(bias_grad(dt, dcur, (long)B * y.OH * y.OW, y.Cout, 1.f, grads[y.pb], S(Q->colscr), st));
        return 0;
    }
    // gradient of a layer's input into dst, times LeakyReLU' of mz (the input itself where it is a layer's post-activation, or TNULL)
    int input_grad(const DLayer& y, TRef dcur, TRef dst, TRef mz) const {
        if (y.stride == 2) return y.s2().run(dt, dcur, B, y.OH, y.OW, dst, y.H, y.W, wp, y.wd, TNULL, mz, true, st);
        Conv cv(dt, y.k, y.k, 1);       // stride 1: the "full" convolution with the flipped kernel
        cv.in(dcur, B, y.OH, y.OW, y.out_cs).w(wp + y.wd[0]).out(dst, y.H, y.W, y.Cin).pad(y.k - 1 - y.pad, y.k - 1 - y.pad);
        if (mz.p) cv.mask(mz, 0);
        return cv.run(st);
    }
    // the first layer's input gradient, in the input's layout, and from there to NCHW f32
    int write_dx(TRef dcur, float* dx_nchw) const {
        const DLayer& y = P.y[0];
        TRef dxin = tref(s8 + Q->dxin, y.in_cs);
        if (!P.s2d())       // NHWC: the padded image channels, which the convolution does not write (the space-to-depth form is written whole)
            SG_HIP(hipMemsetAsync(dxin.p, 0, (size_t)B * y.H * y.W * y.in_cs * P.esz, (hipStream_t)st));
        SG_TRY(input_grad(y, dcur, dxin, TNULL));
        if (P.s2d()) return srcgan_s2d_to_nchw_f32(dxin.p, dx_nchw, B, c->in_ch, c->H, c->W, dt, st);
        return srcgan_nhwc_to_nchw_f32(dxin.p, dx_nchw, B, c->in_ch, c->H, c->W, y.in_cs, 0, dt, st);
    }
    int backward(const float* dy_nchw, float* dx_nchw) const {
        if (do_pack) SG_TRY(pack_dgrad(dx_nchw || (opt && opt->wpack)));       // a persistent pack serves later calls that may want dx
        const DLayer& yl = P.y[P.L - 1];
        TRef dcur = tref(s8 + Q->dO, yl.out_cs);        // dy -> NHWC (1 channel, padded with zeros to 8)
        SG_TRY(srcgan_nchw_f32_to_nhwc(dy_nchw, dcur.p, B, 1, yl.OH, yl.OW, yl.out_cs, dt, st));
        for (int l = P.L - 1; l > 0; --l) {
            const DLayer& y = P.y[l];
            TRef dst = tref(s8 + Q->g[l & 1], y.Cin);
            SG_TRY(norm_backward(y, dcur));
            SG_TRY(param_grads(y, dcur));
            SG_TRY(input_grad(y, dcur, dst, X(y)));
            dcur = dst;
        }
        SG_TRY(param_grads(P.y[0], dcur));      // the first layer has no normalisation, and its input gradient is dx
        if (dx_nchw) SG_TRY(write_dx(dcur, dx_nchw));
        return 0;
    }
};
}  // namespace

extern "C" int srcgan_nlayerd_num_params(const srcgan_nlayerd_cfg* c) { DPlan P; if (d_plan(c, P)) return -1; return P.nparams; }
extern "C" int srcgan_nlayerd_out_hw(const srcgan_nlayerd_cfg* c, int* oh, int* ow) {
    DPlan P; SG_TRY(d_plan(c, P)); if (oh) *oh = P.y[P.L - 1].OH; if (ow) *ow = P.y[P.L - 1].OW; return 0;
}
extern "C" size_t srcgan_nlayerd_ws_bytes(const srcgan_nlayerd_cfg* c) { DPlan P; if (d_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_nlayerd_bwd_scratch_bytes(const srcgan_nlayerd_cfg* c) {
    DPlan P; if (d_plan(c, P)) return 0; DBwdPlan Q; d_bwd_plan(c, P, Q); return Q.total;
}
extern "C" size_t srcgan_nlayerd_wpack_bytes(const srcgan_nlayerd_cfg* c) { DPlan P; if (d_plan(c, P)) return 0; return P.total - P.wpk; }

extern "C" int srcgan_nlayerd_forward(const srcgan_nlayerd_cfg* c, const float* x_nchw, const float* const* params,
                                      float* const* bn_running, int64_t* const* bn_nbt, void* ws, float* y_nchw, void* st) {
    return srcgan_nlayerd_forward_ex(c, x_nchw, params, bn_running, bn_nbt, ws, y_nchw, nullptr, st);
}
extern "C" int srcgan_nlayerd_backward(const srcgan_nlayerd_cfg* c, const float* dy_nchw, const float* const* params,
                                       void* ws, void* scratch, float* const* grads, float* dx_nchw, void* st) {
    return srcgan_nlayerd_backward_ex(c, dy_nchw, params, ws, scratch, grads, dx_nchw, nullptr, st);
}

extern "C" int srcgan_nlayerd_forward_ex(const srcgan_nlayerd_cfg* c, const float* x_nchw, const float* const* params,
                                         float* const* bn_running, int64_t* const* bn_nbt, void* ws, float* y_nchw,
                                         const srcgan_net_opts* opt, void* st) {
    DPlan P;
    SG_TRY(d_plan(c, P));
    SG_REQUIRE(x_nchw && params && ws && y_nchw, "srcgan_nlayerd_forward: null pointer");
    SG_REQUIRE(((uintptr_t)ws % 256) == 0, "srcgan_nlayerd_forward: workspace must be 256-byte aligned");
    const DCall K(c, P, params, ws, opt, st);
    SG_REQUIRE(((uintptr_t)K.wp % 256) == 0, "srcgan_nlayerd_forward: wpack must be 256-byte aligned");
    return K.forward(x_nchw, bn_running, bn_nbt, y_nchw);
}

extern "C" int srcgan_nlayerd_backward_ex(const srcgan_nlayerd_cfg* c, const float* dy_nchw, const float* const* params,
                                          void* ws, void* scratch, float* const* grads, float* dx_nchw, const srcgan_net_opts* opt, void* st) {
    DPlan P;
    SG_TRY(d_plan(c, P));
    SG_REQUIRE(c->training || P.inorm, "srcgan_nlayerd_backward: backward through eval-mode BatchNorm is not supported");
    SG_REQUIRE(dy_nchw && params && ws && scratch && grads, "srcgan_nlayerd_backward: null pointer");
    DBwdPlan Q;
    d_bwd_plan(c, P, Q);
    return DCall(c, P, params, ws, opt, st, &Q, scratch, grads).backward(dy_nchw, dx_nchw);
}

// ======================================================================================== op-list networks
// ResDeconv colouriser -- reference src/model/resdeconv.py:99-195 (the second network of every trainCas step,
// trainCas.py:31,99-100): ResNet-18-style encoder (7x7 s2 stem, BasicBlocks 64-128-256-512 with 3x3 s2 + 1x1 s2 shortcut at
// each widening) and a mirrored decoder (ConvTranspose2d k2 s2 + two BasicBlocks per scale), GroupNorm(32) + ReLU, no biases.
// ESPCN -- src/model/espcn.py:18-51 (the CLI default --SRModel, trainCas.py:169): 5x5, 3x3, 3x3 convs + ReLU, 3x3 conv to
// 64 r^2 channels, PixelShuffle(r), 3x3 conv.   SRCNN -- src/model/srcnn.py:17-42: 9x9, 1x1, 5x5 convs, each + ReLU.
//
// Each network is a short op list built once per call; forward walks it, backward walks it in reverse.  A tensor with two
// consumers (a block's input: first convolution + shortcut) gets its first gradient contribution by a plain store and the
// second through the convolution epilogue's in-place residual operand.  The gradient stored for the output of a
// convolution with a fused ReLU is the gradient w.r.t. its pre-activation: whoever writes it applies the mask (the consumer's
// dgrad epilogue, or srcgan_mask_inplace for the gradient arriving from the loss).
namespace {
struct RdT { int C, cs, H, W, act; size_t off; };       // act: produced by a convolution with a fused ReLU
struct RdOp {
    int type;                 // 0 conv (+bias)(+ReLU), 1 GroupNorm(+res)(+ReLU), 2 ConvTranspose2d k2 s2, 3 PixelShuffle(r),
                              // 4 (inference plans only) ConvTranspose2d k2 s2 followed by a bias-free 3x3 conv, folded into four parity 2x2 convs
                              // 5 ConvTranspose2d k3 s2 p1 output_padding 1 + bias + ReLU (deconv_k3s2.hip)
                              // 6 MaxPool2d(2, 2) (vgg_loss.hip)
                              // 7 channel attention + block residual (chan_attn.hip): in = t, res = the block's input, w = conv_du.0.weight (its bias and
                              //   conv_du.2.{weight,bias} follow), ngrp = C / reduction, stats = the op's `saved` region
                              // 8 MeanShift, a frozen 1x1 convolution on the 3 image channels (chan_attn.hip)
                              // 9 shifted space-to-depth gather (back_proj.hip): image `in` -> grid `out`, k = the scale, pad = the shift
                              // 10 per-channel PReLU (+ bias)(+ beta * res) (back_proj.hip): in = the pre-activation z, kept for the backward -- a plain
                              //    tensor (k = 1) or the grid tensor of a transposed projection, cropped while it is read (k = the scale, pad = the shift);
                              //    w = the slope, bias = the transposed projection's bias or -1, slope = beta, res at channel rcoff of its tensor
    int in, out, res, relu;
    int icoff, iC, ocoff, oC; // type 0 on a dense buffer: reads channels [icoff, icoff + iC) of `in`, writes [ocoff, ocoff + oC) of `out` (iC / oC == 0: the whole tensor)
    int rcoff;                // type 10: first channel of the residual in `res`
    int proj, ps, pk;         // type 0, proj != 0: a DDBPN projection in its stride-1 form over the space-to-depth view (k = ceil(pk / ps) taps): 1 = Conv2d
                              // pk x pk stride ps (in = the gathered grid), 2 = ConvTranspose2d (out = the grid); w is the stored weight, re-ordered
                              // into the f32 staging area wst (an offset into the pack region) before it is packed
    size_t wst;
    int share;                // != 0: a module applied a second time -- op share - 1 owns the packs, this op's weight and bias gradients add to its
    int k, s, pad, w, bias;   // w: parameter index of the weight (GroupNorm: gamma, beta = w + 1; -1 = no affine part); bias: parameter index or -1
    int w2;                   // type 4: parameter index of the 3x3 convolution's weight (w = the transposed convolution's)
    int ngrp;                 // GroupNorm: groups (InstanceNorm2d: = channels)
    float slope;              // GroupNorm activation: 0 = ReLU, 0.2 = LeakyReLU (edsr.py:42)
    size_t wf[4], wd[4], stats;
    S2Dgrad s2(int cin, int cout) const { return S2Dgrad{k, pad, cin, cout}; }      // input gradient of a stride-2 convolution with k > 1
};
static inline int rd_cin(const RdOp& o, const RdT& ti) { return o.iC ? o.iC : ti.C; }
static inline int rd_cout(const RdOp& o, const RdT& to) { return o.oC ? o.oC : to.C; }
// ConvTranspose2d weight [ci][co][3][3], output parity q = (a, b): rows = co, k = ci, taps (wy, wx) in [0, a] x [0, b] with ky = a ? 2 - 2 wy : 1
static inline void deconv3_pack(PackList& packs, const float* w, char* wp, const size_t wf[4], int cin, int cout) {
    for (int q = 0; q < 4; ++q) {
        const int a = q >> 1, b = q & 1;
        packs.add(w, wp + wf[q], cout, cin, a + 1, b + 1, 9, (long)cout * 9, -6, -2, (a ? 2 : 1) * 3 + (b ? 2 : 1));
    }
}
struct RdPlan {
    int dtype, esz, B, H, W, in_ch, out_ch, in_cs, out_cs, nparams, maxC;
    std::vector<RdT> T; std::vector<RdOp> ops;
    size_t xin, gnfwd, wpk, total, act_bytes;
    size_t wpack;             // inference plans: bytes of the packed-weight part
    std::vector<size_t> g;    // backward: gradient buffer offsets (scratch), same shapes as T
    size_t projscr, prscr;    // backward: a projection's weight gradient in its stride-1 form; the PReLU partial sums
    size_t slab, gnscr, colscr, btmp, bwd_total;      // btmp: a bias gradient on its way to being added (second use of a shared module)
    std::vector<int> taps;    // tensors whose last reader is a loss behind the walk (frozen feature extractors): the slot planner keeps them
};

struct RdBuilder {
    RdPlan& P; Bump b; int np = 0; int B;
    int inorm = 0;            // normalisation layers are InstanceNorm2d (no parameters) instead of GroupNorm(32, C)
    int frozen = 0;           // no parameter takes a gradient and the ops form a chain: the backward scratch is two alternating gradient buffers
    RdBuilder(RdPlan& p, int B_) : P(p), B(B_) {}
    int tensor(int C, int cs, int H, int W, int act = 0) { P.T.push_back(RdT{C, cs, H, W, act, b.take((size_t)B * H * W * cs * P.esz)}); return (int)P.T.size() - 1; }
    int conv(int in, int cout, int k, int s, int pad, bool bias = false, bool relu = false) {
        const RdT ti = P.T[in];
        const int oh = (ti.H + 2 * pad - k) / s + 1, ow = (ti.W + 2 * pad - k) / s + 1;
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 0; o.in = in; o.res = -1; o.k = k; o.s = s; o.pad = pad; o.relu = relu; o.w = np++; o.bias = bias ? np++ : -1;
        o.out = tensor(cout, cout < 8 ? 8 : cout, oh, ow, relu);
        P.ops.push_back(o); return o.out;
    }
    // convolution between channel slices of dense buffers (the concat-free dense blocks of SRDenseNet)
    void conv_slice(int in, int icoff, int iC, int out, int ocoff, int oC, int k, int pad) {
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 0; o.in = in; o.out = out; o.res = -1; o.k = k; o.s = 1; o.pad = pad; o.relu = 1; o.w = np++; o.bias = np++;
        o.icoff = icoff; o.iC = iC; o.ocoff = ocoff; o.oC = oC;
        P.ops.push_back(o);
    }
    int deconv3(int in, int cout) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 5; o.in = in; o.out = tensor(cout, cout, 2 * ti.H, 2 * ti.W, 1); o.res = -1; o.k = 3; o.s = 2; o.pad = 1; o.relu = 1; o.w = np++; o.bias = np++;
        P.ops.push_back(o); return o.out;
    }
    // the last op applies the module of op `first` again (same parameters, same packs)
    void share_last(int first) {
        RdOp& o = P.ops.back();
        o.w = P.ops[first].w; o.bias = P.ops[first].bias; o.share = first + 1;
        np -= 2;
    }
    int gn(int in, int res, int relu) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 1; o.in = in; o.out = tensor(ti.C, ti.cs, ti.H, ti.W); o.res = res; o.relu = relu; o.bias = -1;
        if (inorm) { o.w = -1; o.ngrp = ti.C; } else { o.w = np; np += 2; o.ngrp = 32; }
        o.stats = b.take((size_t)B * o.ngrp * 2 * sizeof(float));
        P.ops.push_back(o); return o.out;
    }
    int deconv(int in, int cout) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 2; o.in = in; o.out = tensor(cout, cout, 2 * ti.H, 2 * ti.W); o.res = -1; o.k = 2; o.s = 2; o.w = np++; o.bias = -1;
        P.ops.push_back(o); return o.out;
    }
    int shuffle(int in, int r) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 3; o.in = in; o.res = -1; o.k = r; o.w = -1; o.bias = -1;
        o.out = tensor(ti.C / (r * r), ti.C / (r * r), ti.H * r, ti.W * r);
        P.ops.push_back(o); return o.out;
    }
    int pool(int in) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 6; o.in = in; o.res = -1; o.k = 2; o.s = 2; o.w = -1; o.bias = -1;
        o.out = tensor(ti.C, ti.cs, ti.H / 2, ti.W / 2);
        P.ops.push_back(o); return o.out;
    }
    int ca(int in, int res, int cr) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 7; o.in = in; o.res = res; o.out = tensor(ti.C, ti.cs, ti.H, ti.W); o.bias = -1; o.ngrp = cr;
        o.w = np; np += 4;
        o.stats = b.take((size_t)B * (2 * ti.C + cr) * sizeof(float));
        P.ops.push_back(o); return o.out;
    }
    int meanshift(int in) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 8; o.in = in; o.res = -1; o.k = 1; o.s = 1; o.w = np++; o.bias = np++;
        o.out = tensor(3, 8, ti.H, ti.W);
        P.ops.push_back(o); return o.out;
    }
    // convolution with explicit parameter indices reading the channel prefix [0, iC) of `in` (iC == 0: all of it) into a new tensor
    int conv_at(int in, int iC, int cout, int k, int pad, int widx, int bidx, int proj = 0, int ps = 0, int pk = 0) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 0; o.in = in; o.res = -1; o.k = k; o.s = 1; o.pad = pad; o.w = widx; o.bias = bidx; o.iC = iC; o.proj = proj; o.ps = ps; o.pk = pk;
        o.out = tensor(cout, cout < 8 ? 8 : cout, ti.H + 2 * pad - k + 1, ti.W + 2 * pad - k + 1);
        P.ops.push_back(o); return o.out;
    }
    int gather(int in, int iC, int s, int shift, int Hg, int Wg) {
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 9; o.in = in; o.res = -1; o.k = s; o.pad = shift; o.w = -1; o.bias = -1; o.iC = iC;
        o.out = tensor(s * s * iC, s * s * iC, Hg, Wg);
        P.ops.push_back(o); return o.out;
    }
    // out < 0: a new C-channel tensor of H x W; otherwise channels [ocoff, ocoff + C) of `out`
    int prelu(int in, int C, int H, int W, int s, int shift, int aidx, int bidx, int res, int rcoff, float beta, int out = -1, int ocoff = 0) {
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = 10; o.in = in; o.res = res; o.rcoff = rcoff; o.slope = beta; o.k = s; o.pad = shift; o.w = aidx; o.bias = bidx;
        o.out = out >= 0 ? out : tensor(C, C, H, W); o.ocoff = ocoff; o.oC = C;
        P.ops.push_back(o); return o.out;
    }
    size_t prelu_scratch() const {
        size_t v = 0;
        for (const RdOp& o : P.ops) if (o.type == 10) v = std::max(v, srcgan_prelu_scratch_floats(B, P.T[o.in].H, P.T[o.in].W, o.oC, o.k));
        return v;
    }
    void tap(int t) { P.taps.push_back(t); }
    // BasicBlock (resdeconv.py:56-97).  state_dict order inside a block: conv1, bn1, conv2, bn2, downsample.{0,1}
    int block(int x, int planes, int stride) {
        const bool ds = stride != 1 || P.T[x].C != planes;
        int t = conv(x, planes, 3, stride, 1);
        t = gn(t, -1, 1);
        t = conv(t, planes, 3, 1, 1);
        const int gn2_param = np; if (!inorm) np += 2;      // bn2's parameters precede the shortcut's in the state_dict
        int idn = x;
        if (ds) { idn = conv(x, planes, 1, stride, 0); idn = gn(idn, -1, 0); }
        const int out = gn(t, idn, 1);
        if (!inorm) { P.ops.back().w = gn2_param; np -= 2; }
        return out;
    }
    void input(int in_ch, int H, int W) {
        P.in_ch = in_ch; P.in_cs = img_cs(in_ch); P.H = H; P.W = W;
        P.xin = b.take((size_t)B * H * W * P.in_cs * P.esz);
        P.T.push_back(RdT{in_ch, P.in_cs, H, W, 0, P.xin});
    }
    size_t ca_scratch() const {       // the largest attention op's scratch (0: the plan has none)
        size_t v = 0;
        for (const RdOp& o : P.ops) if (o.type == 7) v = std::max(v, srcgan_ca_scratch_floats(B, (long)P.T[o.in].H * P.T[o.in].W, P.T[o.in].C));
        return v;
    }
    void finish(int dtype) {
        P.nparams = np;
        P.maxC = 8;
        for (const RdT& t : P.T) if (t.C > P.maxC) P.maxC = t.C;
        P.out_ch = P.T.back().C; P.out_cs = P.T.back().cs;
        P.gnfwd = b.take(std::max(srcgan_gn_scratch_floats(B, P.maxC > 1024 ? 1024 : P.maxC), ca_scratch()) * sizeof(float));
        P.act_bytes = b.off;
        P.wpk = b.off;
        Bump wb;
        auto pk = [&](int rows, int k, int taps) { return wb.take(srcgan_packed_weight_bytes(rows, k, taps, dtype)); };
        for (RdOp& o : P.ops) {
            const RdT ti = P.T[o.in], to = P.T[o.out];
            const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
            if (o.share) {
                memcpy(o.wf, P.ops[o.share - 1].wf, sizeof(o.wf)); memcpy(o.wd, P.ops[o.share - 1].wd, sizeof(o.wd));
            } else if (o.type == 0) {
                o.wf[0] = pk(cout, cin, o.k * o.k);
                if (o.s == 1) o.wd[0] = pk(cin, cout, o.k * o.k);
                else if (o.k == 1) o.wd[0] = pk(cin, cout, 1);
                else o.s2(cin, cout).plan(wb, dtype, o.wd);
            } else if (o.type == 2) {
                for (int q = 0; q < 4; ++q) o.wf[q] = pk(to.C, ti.C, 1);
                o.wd[0] = pk(ti.C, to.C, 4);
            } else if (o.type == 5) {       // four parity packs, equally spaced (the 4-tap pack's size)
                const size_t step = srcgan_packed_weight_bytes(to.C, ti.C, 4, dtype), w0 = wb.take(4 * step);
                for (int q = 0; q < 4; ++q) o.wf[q] = w0 + q * step;
                o.wd[0] = pk(ti.C, to.C, 9);
            }
            if (o.type == 0 && o.proj) o.wst = wb.take((size_t)cout * cin * o.k * o.k * sizeof(float));
        }
        P.total = align_up(P.wpk + wb.off + 256, 256);
        // backward scratch
        Bump s;
        P.g.resize(P.T.size());
        if (frozen) {       // op k maps tensor k to tensor k + 1, and a gradient is dead once its op has run: even and odd tensors share a buffer each
            size_t mx = 0;
            for (const RdT& t : P.T) mx = std::max(mx, (size_t)B * t.H * t.W * t.cs * P.esz);
            const size_t g0 = s.take(mx), g1 = s.take(mx);
            for (size_t i = 0; i < P.T.size(); ++i) P.g[i] = (i & 1) ? g1 : g0;
            P.slab = P.gnscr = P.colscr = P.btmp = P.projscr = P.prscr = 0;
            P.bwd_total = s.off + 256;
            return;
        }
        long maxpix = 1;
        for (size_t i = 0; i < P.T.size(); ++i) {
            P.g[i] = s.take((size_t)B * P.T[i].H * P.T[i].W * P.T[i].cs * P.esz);
            if ((long)B * P.T[i].H * P.T[i].W > maxpix) maxpix = (long)B * P.T[i].H * P.T[i].W;
        }
        size_t slab = 0;
        for (const RdOp& o : P.ops) {
            const RdT ti = P.T[o.in], to = P.T[o.out];
            size_t v = 0;
            if (o.type == 0) v = wgrad_slab(B, to.H, to.W, rd_cout(o, to), rd_cin(o, ti), o.k, o.k, o.s);
            else if (o.type == 2) v = wgrad_slab(B, ti.H, ti.W, ti.C, to.C, 2, 2, 2);
            else if (o.type == 5) v = wgrad_slab(B, ti.H, ti.W, ti.C, to.C, 3, 3, 2);
            if (v > slab) slab = v;
        }
        P.slab = s.take(slab);
        size_t projscr = 0;
        for (const RdOp& o : P.ops) if (o.type == 0 && o.proj) projscr = std::max(projscr, (size_t)rd_cout(o, P.T[o.out]) * rd_cin(o, P.T[o.in]) * o.k * o.k * sizeof(float));
        P.projscr = projscr ? s.take(projscr) : 0;
        P.prscr = prelu_scratch() ? s.take(prelu_scratch() * sizeof(float)) : 0;
        P.gnscr = s.take(std::max(srcgan_gn_scratch_floats(B, P.maxC > 1024 ? 1024 : P.maxC), ca_scratch()) * sizeof(float));
        P.colscr = s.take((size_t)2 * srcgan_col_reduce_blocks(maxpix) * P.maxC * sizeof(float));
        P.btmp = 0;           // only plans that apply a module twice carry it (the others keep their size)
        for (const RdOp& o : P.ops) if (o.share && !P.btmp) P.btmp = s.take((size_t)P.maxC * sizeof(float));
        P.bwd_total = s.off + 256;
    }
};

static int rd_common(int dtype, int B, int H, int W, RdPlan& P, const char* who) {
    SG_REQUIRE(sg_dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    SG_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad B/H/W", who);
    P.dtype = dtype; P.esz = dtype == SRCGAN_F32 ? 4 : 2; P.B = B;
    return 0;
}

static int rd_plan(const srcgan_resdeconv_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "resdeconv: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "resdeconv"));
    SG_REQUIRE(c->in_ch == 3 && c->out_ch > 0 && c->out_ch <= 8, "resdeconv: the stem takes 3 channels (resdeconv.py:113), tar_ch must be in 1..8");
    SG_REQUIRE(c->H % 16 == 0 && c->W % 16 == 0, "resdeconv: H and W must be multiples of 16 (four stride-2 stages mirrored by four x2 deconvolutions)");
    int layers[4];
    const bool dflt = c->layers[0] == 0 && c->layers[1] == 0 && c->layers[2] == 0 && c->layers[3] == 0;
    for (int l = 0; l < 4; ++l) {
        layers[l] = dflt ? 2 : c->layers[l];
        SG_REQUIRE(layers[l] >= 1 && layers[l] <= 64, "resdeconv: layers[%d] = %d (1..64 BasicBlocks per stage)", l, layers[l]);
    }
    SG_REQUIRE(c->norm == 0 || c->norm == 1, "resdeconv: norm must be 0 (GroupNorm(32, C)) or 1 (InstanceNorm2d)");
    RdBuilder nb(P, c->B);
    nb.inorm = c->norm == 1;
    nb.input(c->in_ch, c->H, c->W);
    int t = nb.conv(0, 64, 7, 2, 3);
    t = nb.gn(t, -1, 1);
    const int widths[4] = {64, 128, 256, 512};
    for (int l = 0; l < 4; ++l)                 // _make_layer (resdeconv.py:148-163): the first block carries the stride / shortcut
        for (int k = 0; k < layers[l]; ++k) t = nb.block(t, widths[l], (k == 0 && l > 0) ? 2 : 1);
    const int up_w[3] = {256, 128, 64};
    for (int l = 0; l < 3; ++l) {               // upRes1..3 use layers[2], layers[1], layers[0] (resdeconv.py:131-137)
        t = nb.deconv(t, up_w[l]);
        for (int k = 0; k < layers[2 - l]; ++k) t = nb.block(t, up_w[l], 1);
    }
    t = nb.deconv(t, 64);
    nb.conv(t, c->out_ch, 3, 1, 1);
    nb.finish(c->dtype);
    return 0;
}

// kind 0: ESPCN(in_ch, ou_ch, upscale_factor, base_kernel) espcn.py:18-51;  kind 1: SRCNN(in_ch, ou_ch, ., base_kernel) srcnn.py:17-42
static int sr_plan(const srcgan_srnet_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srnet: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srnet"));
    SG_REQUIRE(c->kind >= 0 && c->kind <= 2, "srnet: kind must be 0 (ESPCN), 1 (SRCNN) or 2 (EDSR)");
    SG_REQUIRE(c->kind != 2 || (c->nres >= 1 && c->base % 32 == 0 && (c->up & (c->up - 1)) == 0), "srnet: EDSR needs num_residuals >= 1, base_channel % 32 == 0 and a power-of-two upscale factor");
    SG_REQUIRE(c->in_ch > 0 && c->in_ch <= 8 && c->out_ch > 0 && c->out_ch <= 8, "srnet: in/out channels must be in 1..8");
    SG_REQUIRE(c->base > 0 && c->base % 16 == 0, "srnet: base_kernel must be a multiple of 16");
    SG_REQUIRE(c->up >= 1 && c->up <= 8, "srnet: upscale_factor must be in 1..8");
    RdBuilder nb(P, c->B);
    nb.input(c->in_ch, c->H, c->W);
    if (c->kind == 0) {
        int t = nb.conv(0, c->base, 5, 1, 2, true, true);
        t = nb.conv(t, c->base, 3, 1, 1, true, true);
        t = nb.conv(t, c->base / 2, 3, 1, 1, true, true);
        t = nb.conv(t, c->base * c->up * c->up, 3, 1, 1, true, false);
        t = nb.shuffle(t, c->up);
        nb.conv(t, c->out_ch, 3, 1, 1, true, false);
    } else if (c->kind == 1) {
        int t = nb.conv(0, c->base, 9, 1, 4, true, true);
        t = nb.conv(t, c->base / 2, 1, 1, 0, true, true);
        nb.conv(t, c->out_ch, 5, 1, 2, true, true);
    } else {
        // EDSR (edsr.py:37-110): input_conv; num_residuals x [conv1 -> gn -> LeakyReLU(0.2) -> conv2 -> gn (the SAME GroupNorm
        // module) -> + x]; mid_conv + input_conv's output; ConvTranspose2d k2 s2 per x2 stage; output_conv.  state_dict order
        // inside a block: conv1.{w,b}, conv2.{w,b}, gn.{w,b}.
        const int feat = nb.conv(0, c->base, 3, 1, 1, true, false);
        int t = feat;
        for (int i = 0; i < c->nres; ++i) {
            const int base = nb.np, x = t;
            t = nb.conv(x, c->base, 3, 1, 1, true, false);
            P.ops.back().w = base; P.ops.back().bias = base + 1;
            t = nb.gn(t, -1, 1);
            P.ops.back().w = base + 4; P.ops.back().slope = 0.2f;
            t = nb.conv(t, c->base, 3, 1, 1, true, false);
            P.ops.back().w = base + 2; P.ops.back().bias = base + 3;
            t = nb.gn(t, x, 0);
            P.ops.back().w = base + 4;
            nb.np = base + 6;
        }
        t = nb.conv(t, c->base, 3, 1, 1, true, false);
        P.ops.back().res = feat;
        for (int f = 1; f < c->up; f *= 2) t = nb.deconv(t, c->base);
        nb.conv(t, c->out_ch, 3, 1, 1, true, false);
    }
    nb.finish(c->dtype);
    return 0;
}
// SRDenseNetA (kind 0, LR -> HR) / SRDenseNetB (kind 1, HR -> LR) -- reference src/model/model.py:643-786.  conv_first (in -> 1
// channel) -> conv (1 -> g L) + ReLU -> num_blocks DenseBlocks -> 1x1 bottleneck to 256 + ReLU -> the shared up- / down-sampler once
// ('x2') or twice ('x4') -> reconstruction (256 -> 1) -> conv_last.  state_dict order = the order the ops are built in.
//
// Concat-free dense blocks, in-place prefixing: DenseBlock i maps its input x (C_i = g L (i + 1) channels) to cat[x, c_1 .. c_L], and
// that is exactly the next block's input, so ALL blocks share ONE buffer of g L (num_blocks + 1) channels: the block's first layer reads
// the prefix [0, C_i), layer j > 1 reads [C_i, C_i + g (j - 1)) (the block-local concatenation: model.py:666-669 does not feed x to its
// DenseLayers), each writes its own g-channel slice, and the bottleneck reads the whole buffer.  No copy, no torch.cat, no CatBackward.
// Backward: the bottleneck's input gradient is the first writer of the whole gradient buffer; every layer's dgrad adds to the
// slice range it read through the epilogue's in-place residual, masked by ReLU' of the stored activation.
static int sd_plan(const srcgan_srdense_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srdense: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srdense"));
    SG_REQUIRE(c->kind == 0 || c->kind == 1, "srdense: kind must be 0 (SRDenseNetA) or 1 (SRDenseNetB)");
    SG_REQUIRE(c->in_ch > 0 && c->in_ch <= 8 && c->out_ch > 0 && c->out_ch <= 8, "srdense: in/out channels must be in 1..8");
    SG_REQUIRE(c->num_blocks >= 1 && c->num_layers >= 1 && c->growth >= 1, "srdense: growth_rate, num_blocks and num_layers must be positive");
    SG_REQUIRE(c->up == 2 || c->up == 4, "srdense: mode must be 'x2' or 'x4' (up = 2 or 4)");
    SG_REQUIRE(c->growth % 8 == 0, "srdense: growth_rate must be a multiple of 8 (growth_rate = %d): every layer writes a growth_rate-channel slice, and slices are "
               "addressed in 16-byte pieces", c->growth);
    const int g = c->growth, L = c->num_layers, nB = c->num_blocks, gL = g * L, kce = 64 / P.esz;
    SG_REQUIRE(gL % kce == 0, "srdense: growth_rate * num_layers = %d must be a multiple of the 64-byte K chunk (%d channels in this dtype): a dense block's "
               "slice offset growth_rate * num_layers * (i + 1) has to start a chunk", gL, kce);
    SG_REQUIRE(c->kind == 0 || (c->H >= 2 && c->W >= 2), "srdense: SRDenseNetB needs H, W >= 2");
    SG_REQUIRE((long)gL * (nB + 1) <= 8192, "srdense: more than 8192 concatenated channels");
    RdBuilder nb(P, c->B);
    nb.input(c->in_ch, c->H, c->W);
    const int t1 = nb.conv(0, 1, 3, 1, 1, true, false);                      // conv_first
    const int Ctot = gL * (nB + 1);
    const int D = nb.tensor(Ctot, Ctot, c->H, c->W, 1);
    nb.conv_slice(t1, 0, 0, D, 0, gL, 3, 1);                                 // conv
    for (int i = 0; i < nB; ++i) {
        const int Ci = gL * (i + 1);
        nb.conv_slice(D, 0, Ci, D, Ci, g, 3, 1);                             // ConvLayer: the whole block input
        for (int j = 1; j < L; ++j) nb.conv_slice(D, Ci, g * j, D, Ci + g * j, g, 3, 1);     // DenseLayer j: c_1 .. c_j
    }
    int t = nb.conv(D, 256, 1, 1, 0, true, true);                            // bottleneck
    int first = -1;
    for (int f = 1; f < c->up; f *= 2) {                                     // deconv: ONE module, applied once or twice
        t = c->kind == 0 ? nb.deconv3(t, 256) : nb.conv(t, 256, 3, 2, 1, true, true);
        if (first < 0) first = (int)P.ops.size() - 1; else nb.share_last(first);
    }
    t = nb.conv(t, 1, 3, 1, 1, true, false);                                 // reconstruction
    nb.conv(t, c->out_ch, 3, 1, 1, true, false);                             // conv_last
    nb.finish(c->dtype);
    return 0;
}
// RCAN (rcan.py:69-116).  Parameter indices follow parameters() order = registration order: sub_mean (:82), add_mean (:100, assigned
// before head / body / tail at :102-104), head, body, tail -- the two MeanShift ops get their indices by hand.
static int rcan_plan(const srcgan_rcan_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srcgan_rcan: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srcgan_rcan"));
    SG_REQUIRE(c->in_ch == 3 && c->out_ch == 3, "srcgan_rcan: n_colors must be 3 (MeanShift is a 3-channel convolution, common.py:16)");
    SG_REQUIRE(c->scale == 2 || c->scale == 3 || c->scale == 4 || c->scale == 8, "srcgan_rcan: scale = %d must be 2, 3, 4 or 8 (common.py:63-84)", c->scale);
    SG_REQUIRE(c->n_feats > 0 && c->n_feats % 16 == 0 && c->n_feats <= 1024, "srcgan_rcan: n_feats = %d must be a multiple of 16, at most 1024", c->n_feats);
    SG_REQUIRE(c->reduction >= 1 && c->n_feats / c->reduction >= 1, "srcgan_rcan: n_feats / reduction must be at least 1 (n_feats = %d, reduction = %d)",
               c->n_feats, c->reduction);
    SG_REQUIRE(c->n_resgroups >= 1 && c->n_resblocks >= 1 && (long)c->n_resgroups * c->n_resblocks <= 100000, "srcgan_rcan: n_resgroups and n_resblocks must be positive");
    const int F = c->n_feats, cr = F / c->reduction;
    RdBuilder nb(P, c->B);
    nb.input(3, c->H, c->W);
    int t = nb.meanshift(0);                                    // sub_mean: parameters 0, 1
    nb.np = 4;                                                  // add_mean: parameters 2, 3
    const int head = nb.conv(t, F, 3, 1, 1, true, false);
    t = head;
    for (int g = 0; g < c->n_resgroups; ++g) {
        const int gin = t;
        for (int k = 0; k < c->n_resblocks; ++k) {              // RCAB (:30-49)
            const int x = t;
            t = nb.conv(x, F, 3, 1, 1, true, true);
            t = nb.conv(t, F, 3, 1, 1, true, false);
            t = nb.ca(t, x, cr);
        }
        t = nb.conv(t, F, 3, 1, 1, true, false);                // ResidualGroup (:60-66)
        P.ops.back().res = gin;
    }
    t = nb.conv(t, F, 3, 1, 1, true, false);                    // :93, 110-111
    P.ops.back().res = head;
    if (c->scale == 3) { t = nb.conv(t, 9 * F, 3, 1, 1, true, false); t = nb.shuffle(t, 3); }
    else for (int f = 1; f < c->scale; f *= 2) { t = nb.conv(t, 4 * F, 3, 1, 1, true, false); t = nb.shuffle(t, 2); }
    t = nb.conv(t, 3, 3, 1, 1, true, false);
    nb.meanshift(t);
    P.ops.back().w = 2; P.ops.back().bias = 3; nb.np -= 2;
    nb.finish(c->dtype);
    return 0;
}
// DDBPN (ddbpn.py:68-130).  n0, nr and depth are the reference's constants (:73-75).  Parameter indices follow parameters() order =
// registration order (sub_mean, initial, upmodules, downmodules, reconstruction, add_mean), not the order the modules run in (up 0,
// down 0, up 1, ...), so every op gets its indices by hand.  Inside a DenseProjection: [bottleneck.0.{w,b}, bottleneck.1.weight,]
// conv_1.0.{w,b}, conv_1.1.weight, conv_2..., conv_3... (:32-53).
//
// A projection (k, s, p = 2) in its stride-1 form, T = ceil(k / s) taps, LR h x w, HR s h x s w:
//   up   (ConvTranspose2d): T x T convolution, pad 1, to s^2 nr channels on the grid; PReLU reads it through the crop and adds the bias
//   down (Conv2d):          gather to the grid (s^2 nr channels); T x T convolution, pad 0 (scale 2: 1), + bias; plain PReLU
// The grid is (h + 1) x (w + 1) with shift 2; at scale 2 its border rows are all padding, so it is h x w with shift 0 (plain
// space-to-depth / PixelShuffle) and 3x3 pad-1 convolutions.  PReLU's fused residual carries e = b_0 - x and out = a_0 + a_1 (:61-64);
// `out` goes straight into its slice of the concatenation buffer (l_list: LR, 5 nr channels; h_list: HR, 6 nr), whose consumers read
// the prefix.  Backward: the reconstruction's input gradient is the first writer of the whole HR gradient buffer, the last up-module's
// bottleneck that of the LR one; every other consumer adds to the range it read.
static int ddbpn_plan(const srcgan_ddbpn_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srcgan_ddbpn: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srcgan_ddbpn"));
    SG_REQUIRE(c->in_ch == 3 && c->out_ch == 3, "srcgan_ddbpn: n_colors must be 3 (MeanShift is a 3-channel convolution, common.py:16)");
    SG_REQUIRE(c->scale == 2 || c->scale == 4 || c->scale == 8, "srcgan_ddbpn: scale = %d must be 2, 4 or 8 (ddbpn.py:14-18)", c->scale);
    SG_REQUIRE((long)c->H * c->scale < (1 << 24) && (long)c->W * c->scale < (1 << 24), "srcgan_ddbpn: image too large");
    const int n0 = 128, nr = 32, depth = 6;
    const int s = c->scale, k = s == 2 ? 6 : s == 4 ? 8 : 12, T = (k + s - 1) / s;
    const int shift = s == 2 ? 0 : 2, h = c->H, w = c->W, Hg = h + (s == 2 ? 0 : 1), Wg = w + (s == 2 ? 0 : 1);
    RdBuilder nb(P, c->B);
    nb.input(3, h, w);
    int t = nb.meanshift(0);                                    // sub_mean: parameters 0, 1
    t = nb.conv_at(t, 0, n0, 3, 1, 2, 3);
    t = nb.prelu(t, n0, h, w, 1, 0, 4, -1, -1, 0, 1.f);
    t = nb.conv_at(t, 0, nr, 1, 0, 5, 6);
    const int x0 = nb.prelu(t, nr, h, w, 1, 0, 7, -1, -1, 0, 1.f);
    const int L = nb.tensor((depth - 1) * nr, (depth - 1) * nr, h, w), Hh = nb.tensor(depth * nr, depth * nr, s * h, s * w);
    // x: channels [0, nr) of its tensor; returns PReLU(projection(x)) + beta * res, a new tensor or the slice ocoff of `out`
    auto proj = [&](bool up, int x, int pb, int res, float beta, int out, int ocoff) {
        if (up) {
            const int g = nb.conv_at(x, nr, s * s * nr, T, 1, pb, -1, 2, s, k);
            return nb.prelu(g, nr, s * h, s * w, s, shift, pb + 2, pb + 1, res, 0, beta, out, ocoff);
        }
        const int g = nb.gather(x, nr, s, shift, Hg, Wg);
        const int z = nb.conv_at(g, 0, nr, T, s == 2 ? 1 : 0, pb, pb + 1, 1, s, k);
        return nb.prelu(z, nr, h, w, 1, 0, pb + 2, -1, res, 0, beta, out, ocoff);
    };
    auto module = [&](bool up, int in, int iC, bool bneck, int pb, int out, int ocoff) {       // DenseProjection.forward (:55-66)
        int x = in;
        if (bneck) {
            const int z = nb.conv_at(in, iC, nr, 1, 0, pb, pb + 1);
            x = nb.prelu(z, nr, P.T[z].H, P.T[z].W, 1, 0, pb + 2, -1, -1, 0, 1.f);
            pb += 3;
        }
        const int a0 = proj(up, x, pb, -1, 1.f, -1, 0);
        const int e = proj(!up, a0, pb + 3, x, -1.f, -1, 0);
        proj(up, e, pb + 6, a0, 1.f, out, ocoff);
    };
    int up_pb[6], down_pb[5], pb = 8;
    for (int i = 0; i < depth; ++i) { up_pb[i] = pb; pb += i > 1 ? 12 : 9; }                   // bottleneck: i > 1 (:93)
    for (int i = 0; i < depth - 1; ++i) { down_pb[i] = pb; pb += i != 0 ? 12 : 9; }            // bottleneck: i != 0 (:101)
    for (int i = 0; i < depth - 1; ++i) {                                                       // :118-124
        module(true, i == 0 ? x0 : L, i * nr, i > 1, up_pb[i], Hh, i * nr);
        module(false, Hh, (i + 1) * nr, i != 0, down_pb[i], L, i * nr);
    }
    module(true, L, (depth - 1) * nr, true, up_pb[depth - 1], Hh, (depth - 1) * nr);           // :126
    t = nb.conv_at(Hh, 0, 3, 3, 1, pb, pb + 1);                                                 // reconstruction
    nb.np = pb + 2;
    nb.meanshift(t);                                                                            // add_mean: the last two parameters
    nb.finish(c->dtype);
    return 0;
}
static inline TRef rd_t(char* base, const RdT& t) { return tref(base + t.off, t.cs); }
static inline const char* sr_tag(int kind) { return kind == 0 ? "espcn" : kind == 1 ? "srcnn" : "edsr"; }      // pack-cache tag stem / name in messages

// the forward in three parts (a frozen feature extractor packs once and walks twice, on two inputs)
static int rd_pack_fwd(const RdPlan& P, const float* const* params, void* ws, const char* tag, void* st) {
    const int dt = P.dtype;
    char* w8 = (char*)ws; char* wp = w8 + P.wpk;
    PackList packs(dt, wp);
    for (const RdOp& o : P.ops) {
        const RdT ti = P.T[o.in], to = P.T[o.out];
        const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
        if (o.share) continue;          // packed by the module's first use
        if (o.type == 0 && o.proj) {    // the stored weight in its stride-1 form: an f32 Conv2d weight [cout][cin][k][k] in the staging area
            SG_TRY(sg_proj_repack(params[o.w], (float*)(wp + o.wst), o.proj - 1, o.proj == 1 ? cout : cout / (o.ps * o.ps), o.proj == 1 ? cin / (o.ps * o.ps) : cin,
                                  o.pk, o.ps, 0, (hipStream_t)st));
            packs.add((const float*)(wp + o.wst), wp + o.wf[0], cout, cin, o.k, o.k, lay_fwd(cin, o.k, o.k));
        } else
        if (o.type == 0) packs.add(params[o.w], wp + o.wf[0], cout, cin, o.k, o.k, (long)cin * o.k * o.k, (long)o.k * o.k, o.k, 1, 0);
        else if (o.type == 2)
            for (int q = 0; q < 4; ++q) packs.add(params[o.w], wp + o.wf[q], to.C, ti.C, 1, 1, 4, (long)to.C * 4, 0, 0, q);
        else if (o.type == 5) deconv3_pack(packs, params[o.w], wp, o.wf, ti.C, to.C);
    }
    char key[64]; snprintf(key, sizeof(key), "%s_fwd", tag);
    SG_TRY(packs.run(key, params[0], st));
    for (const RdOp& o : P.ops)      // composed weights of a folded tail: made from both sources on every call, like the packs above
        if (o.type == 4) SG_TRY(sg_fold_tail_pack(params[o.w], params[o.w2], wp + o.wf[0], P.T[o.out].C, dt, (hipStream_t)st));
    return 0;
}
// fr != nullptr: x_nchw is a 5-D tensor whose frames [f0, f0 + k) are the B images (common.h, SgFrames)
static int rd_walk(const RdPlan& P, const float* x_nchw, const float* const* params, void* ws, void* st, const SgFrames* fr = nullptr) {
    const int dt = P.dtype, B = P.B;
    char* w8 = (char*)ws; char* wp = w8 + P.wpk;
    if (fr) SG_TRY(sg_frames_pack(x_nchw, w8 + P.xin, P.in_cs, B / fr->k, *fr, P.H, P.W, dt, (hipStream_t)st));
    else SG_TRY(srcgan_nchw_f32_to_nhwc(x_nchw, w8 + P.xin, B, P.in_ch, P.H, P.W, P.in_cs, dt, st));
    float* gnscr = (float*)(w8 + P.gnfwd);
    for (const RdOp& o : P.ops) {
        const RdT ti = P.T[o.in], to = P.T[o.out];
        TRef xin = rd_t(w8, ti), out = rd_t(w8, to);
        if (o.type == 0) {
            if (to.C < to.cs) SG_HIP(hipMemsetAsync(out.p, 0, (size_t)B * to.H * to.W * to.cs * P.esz, (hipStream_t)st));
            Conv cv(dt, o.k, o.k, o.s);
            cv.in(sl(xin, o.icoff), B, ti.H, ti.W, ti.C < 8 ? ti.cs : rd_cin(o, ti)).w(wp + o.wf[0], o.bias >= 0 ? params[o.bias] : nullptr)
                .out(sl(out, o.ocoff), to.H, to.W, rd_cout(o, to)).pad(o.pad, o.pad);
            if (o.relu) { cv.lrelu(); cv.d.slope = 0.f; }
            if (o.res >= 0) cv.res1(rd_t(w8, P.T[o.res]), to.C, 1.f);          // y = conv(x) + res (edsr.py:97-98)
            SG_TRY(cv.run(st));
        } else if (o.type == 1) {
            const void* res = o.res >= 0 ? (w8 + P.T[o.res].off) : nullptr;
            SG_TRY(srcgan_gn_forward(xin.p, ti.cs, res, o.res >= 0 ? P.T[o.res].cs : 0, out.p, to.cs, o.w >= 0 ? params[o.w] : nullptr,
                                     o.w >= 0 ? params[o.w + 1] : nullptr, (float*)(w8 + o.stats), B, (long)ti.H * ti.W, ti.C, o.ngrp, 1e-5f, o.relu,
                                     o.slope, dt, gnscr, st));
        } else if (o.type == 2) {
            for (int q = 0; q < 4; ++q)
                SG_TRY(Conv(dt, 1, 1, 1).in(xin, B, ti.H, ti.W, ti.C).w(wp + o.wf[q]).out(out, ti.H, ti.W, to.C)
                           .scatter(2, q >> 1, q & 1, to.H, to.W).run(st));
        } else if (o.type == 3) {
            SG_TRY(srcgan_pixel_shuffle_nhwc(xin.p, ti.cs, out.p, to.cs, B, ti.H, ti.W, to.C, o.k, 0, dt, st));
        } else if (o.type == 5) {
            // output pixel (2i + a, 2j + b) = the 1, 2, 2 or 4 taps of parity (a, b) over x[i..i+1][j..j+1]: all four in one launch
            Conv cv(dt, 3, 3, 2);
            cv.in(xin, B, ti.H, ti.W, ti.C).w(wp + o.wf[0], params[o.bias]).out(out, ti.H, ti.W, to.C).pad(1, 1).scatter(2, 0, 0, to.H, to.W).lrelu();
            cv.d.slope = 0.f; cv.d.npar = 4; cv.d.wpar_stride = (long)(o.wf[1] - o.wf[0]);
            SG_TRY(cv.run(st));
        } else if (o.type == 6) {
            SG_TRY(srcgan_maxpool2_nhwc(xin.p, ti.cs, out.p, to.cs, B, ti.H, ti.W, ti.C, dt, st));
        } else if (o.type == 7) {
            const void* res = o.res >= 0 ? (w8 + P.T[o.res].off) : nullptr;
            SG_TRY(srcgan_ca_forward(xin.p, ti.cs, res, o.res >= 0 ? P.T[o.res].cs : 0, out.p, to.cs, params[o.w], params[o.w + 1], params[o.w + 2],
                                     params[o.w + 3], (float*)(w8 + o.stats), B, (long)ti.H * ti.W, ti.C, o.ngrp, dt, gnscr, st));
        } else if (o.type == 8) {
            SG_TRY(sg_meanshift(xin.p, out.p, params[o.w], params[o.bias], 0, (long)B * ti.H * ti.W, dt, (hipStream_t)st));
        } else if (o.type == 9) {
            SG_TRY(srcgan_s2d_shift(xin.p, ti.cs, out.p, to.cs, B, ti.H, ti.W, o.iC, o.k, o.pad, to.H, to.W, dt, st));
        } else if (o.type == 10) {
            const void* res = o.res >= 0 ? (w8 + P.T[o.res].off + (size_t)o.rcoff * P.esz) : nullptr;
            SG_TRY(srcgan_prelu_forward(xin.p, ti.cs, params[o.w], o.bias >= 0 ? params[o.bias] : nullptr, res, o.res >= 0 ? P.T[o.res].cs : 0, o.slope,
                                        (char*)out.p + (size_t)o.ocoff * P.esz, to.cs, B, to.H, to.W, o.oC, o.k, o.pad, ti.H, ti.W, dt, st));
        } else {
            // folded tail: output pixel (2i + a, 2j + b) = 2x2 window of the half-resolution input at (i + a - 1, j + b - 1) times the
            // composed weights of parity (a, b) -- the geometry of the 4x4 stride-2 input gradient, so its four-parity kernel serves.
            // All to.cs channels are written (the pack's rows >= to.C are zero): no memset of the padded channels.
            Conv cv(dt, 2, 2, 1);
            cv.in(xin, B, ti.H, ti.W, ti.C).w(wp + o.wf[0]).out(out, ti.H, ti.W, to.cs).scatter(2, 0, 0, to.H, to.W);
            cv.d.npar = 4; cv.d.wpar_stride = (long)(o.wf[1] - o.wf[0]);
            SG_TRY(cv.run(st));
        }
    }
    return 0;
}
static int rd_forward(const RdPlan& P, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, const char* tag, void* st) {
    SG_REQUIRE(x_nchw && params && ws && y_nchw, "%s forward: null pointer", tag);
    SG_REQUIRE(((uintptr_t)ws % 256) == 0, "%s forward: workspace must be 256-byte aligned", tag);
    SG_TRY(rd_pack_fwd(P, params, ws, tag, st));
    SG_TRY(rd_walk(P, x_nchw, params, ws, st));
    const RdT& last = P.T.back();
    SG_TRY(srcgan_nhwc_to_nchw_f32((char*)ws + last.off, y_nchw, P.B, P.out_ch, last.H, last.W, last.cs, 0, P.dtype, st));
    return 0;
}

// ---- inference: the same op list on a liveness-planned workspace.  rd_forward walks whatever offsets the plan holds, so an
// inference plan is the training plan with its addresses rewritten: a tensor's slot is handed back after its last reader (as `in`
// or as `res`) and reused by later tensors of the same byte size -- one pool per size: a network's stages each cycle through a
// handful of equal tensors, so the pool sizes do not depend on the depth.  An op's output slot is taken BEFORE its inputs are
// handed back: it never aliases them (the kernels take __restrict__ pointers).  GroupNorm statistics share one region (nothing reads
// them after the op), and only the forward packs are laid out.  fold: the trailing ConvTranspose2d k2 s2 -> bias-free 3x3 conv pair
// becomes one op of type 4, and the full-resolution tensor between them gets no slot.
static inline size_t rd_bytes(const RdPlan& P, const RdT& t) { return (size_t)P.B * t.H * t.W * t.cs * P.esz; }

static int rd_infer_replan(RdPlan& P, bool fold, const char* who, size_t spare = 0) {
    if (fold) {
        const int n = (int)P.ops.size();
        SG_REQUIRE(n >= 2, "%s: no tail to fold", who);
        const RdOp d = P.ops[n - 2], c = P.ops[n - 1];
        SG_REQUIRE(d.type == 2 && c.type == 0 && c.in == d.out && c.k == 3 && c.s == 1 && c.pad == 1 && c.bias < 0 && !c.relu && c.res < 0 &&
                   P.T[d.in].C == 64 && P.T[d.out].C == 64 && P.T[c.out].cs == 8,
                   "%s: the tail is not ConvTranspose2d(64, 64, k2 s2) -> bias-free 3x3 convolution to <= 8 channels", who);
        RdOp f; memset(&f, 0, sizeof(f));
        f.type = 4; f.in = d.in; f.out = c.out; f.res = -1; f.k = 2; f.s = 1; f.w = d.w; f.w2 = c.w; f.bias = -1;
        P.ops.resize(n - 2);
        P.ops.push_back(f);
    }
    const int nops = (int)P.ops.size(), nt = (int)P.T.size();
    std::vector<int> last(nt, -1);
    for (int k = 0; k < nops; ++k) { last[P.ops[k].in] = k; if (P.ops[k].res >= 0) last[P.ops[k].res] = k; }
    last[nt - 1] = nops;                                       // the output conversion reads the last tensor
    for (int t : P.taps) last[t] = nops;                       // a tap's last reader is the loss, behind the walk
    Bump b;
    std::map<size_t, std::vector<size_t>> pool;                // byte size -> free slots
    auto get = [&](int t) {
        const size_t sz = align_up(rd_bytes(P, P.T[t]), 256);
        std::vector<size_t>& f = pool[sz];
        if (f.empty()) P.T[t].off = b.take(sz);
        else { P.T[t].off = f.back(); f.pop_back(); }
    };
    auto put = [&](int t) { pool[align_up(rd_bytes(P, P.T[t]), 256)].push_back(P.T[t].off); };
    for (RdT& t : P.T) t.off = 0;
    std::vector<char> have(nt, 0);          // a dense buffer is the output of many ops: it takes its slot at the first
    get(0); have[0] = 1;
    P.xin = P.T[0].off;
    for (int k = 0; k < nops; ++k) {
        const RdOp& o = P.ops[k];
        if (!have[o.out]) { get(o.out); have[o.out] = 1; }
        if (last[o.in] == k) put(o.in);
        if (o.res >= 0 && o.res != o.in && last[o.res] == k) put(o.res);
    }
    if (spare) b.take(spare);
    size_t stats = 0;
    size_t cascr = 0;
    for (const RdOp& o : P.ops) {
        if (o.type == 1) stats = std::max(stats, (size_t)P.B * o.ngrp * 2 * sizeof(float));
        if (o.type == 7) {          // the attention ops' saved {p, h, s}: nothing reads them after the op either
            stats = std::max(stats, (size_t)P.B * (2 * P.T[o.in].C + o.ngrp) * sizeof(float));
            cascr = std::max(cascr, srcgan_ca_scratch_floats(P.B, (long)P.T[o.in].H * P.T[o.in].W, P.T[o.in].C));
        }
    }
    const size_t stats_off = b.take(stats);
    for (RdOp& o : P.ops) if (o.type == 1 || o.type == 7) o.stats = stats_off;
    P.gnfwd = b.take(std::max(srcgan_gn_scratch_floats(P.B, P.maxC > 1024 ? 1024 : P.maxC), cascr) * sizeof(float));
    P.act_bytes = b.off;
    P.wpk = b.off;
    Bump wb;
    auto pk = [&](int rows, int k, int taps) { return wb.take(srcgan_packed_weight_bytes(rows, k, taps, P.dtype)); };
    for (RdOp& o : P.ops) {
        const RdT ti = P.T[o.in], to = P.T[o.out];
        if (o.share) memcpy(o.wf, P.ops[o.share - 1].wf, sizeof(o.wf));
        else if (o.type == 0) o.wf[0] = pk(rd_cout(o, to), rd_cin(o, ti), o.k * o.k);
        else if (o.type == 2) { for (int q = 0; q < 4; ++q) o.wf[q] = pk(to.C, ti.C, 1); }
        else if (o.type == 4) { for (int q = 0; q < 4; ++q) o.wf[q] = pk(to.cs, ti.C, 4); }
        else if (o.type == 5) {
            const size_t step = srcgan_packed_weight_bytes(to.C, ti.C, 4, P.dtype), w0 = wb.take(4 * step);
            for (int q = 0; q < 4; ++q) o.wf[q] = w0 + q * step;
        }
        if (o.type == 0 && o.proj && !o.share) o.wst = wb.take((size_t)rd_cout(o, to) * rd_cin(o, ti) * o.k * o.k * sizeof(float));
    }
    P.wpack = wb.off;
    P.total = align_up(P.wpk + wb.off + 256, 256);
    return 0;
}
static int rd_infer_plan(const srcgan_resdeconv_cfg* c, int fold, RdPlan& P) {
    SG_TRY(rd_plan(c, P));
    SG_REQUIRE(fold == 0 || fold == 1, "resdeconv: fold_tail must be 0 or 1");
    return rd_infer_replan(P, fold != 0, "resdeconv");
}
static int sr_infer_plan(const srcgan_srnet_cfg* c, RdPlan& P) {
    SG_TRY(sr_plan(c, P));
    // EDSR with ONE residual block: its input is input_conv's output, which the global skip keeps alive anyway, so it needs one
    // feature slot fewer than every deeper stack (4).  It gets the fourth as a spare: the activation part is then a function of
    // the shapes alone, and a caller can size one workspace for a family of depths.
    const size_t spare = (c->kind == 2 && c->nres == 1) ? (size_t)c->B * c->H * c->W * c->base * P.esz : 0;
    return rd_infer_replan(P, false, "srnet", spare);
}
static int sd_infer_plan(const srcgan_srdense_cfg* c, RdPlan& P) {
    SG_TRY(sd_plan(c, P));
    return rd_infer_replan(P, false, "srdense");
}
static int rcan_infer_plan(const srcgan_rcan_cfg* c, RdPlan& P) {
    SG_TRY(rcan_plan(c, P));
    return rd_infer_replan(P, false, "srcgan_rcan");
}
static int ddbpn_infer_plan(const srcgan_ddbpn_cfg* c, RdPlan& P) {
    SG_TRY(ddbpn_plan(c, P));
    return rd_infer_replan(P, false, "srcgan_ddbpn");
}
// per-op byte ranges {in, res, out} x {offset, bytes} of a plan (res: 0, 0 where the op has none) -- what the planner's tests inspect
static int rd_plan_ranges(const RdPlan& P, size_t* ranges, int cap) {
    const int n = (int)P.ops.size();
    for (int k = 0; k < n && k < cap && ranges; ++k) {
        const RdOp& o = P.ops[k];
        size_t* r = ranges + 6 * k;
        r[0] = P.T[o.in].off; r[1] = rd_bytes(P, P.T[o.in]);
        r[2] = o.res >= 0 ? P.T[o.res].off : 0; r[3] = o.res >= 0 ? rd_bytes(P, P.T[o.res]) : 0;
        r[4] = P.T[o.out].off; r[5] = rd_bytes(P, P.T[o.out]);
    }
    return n;
}

// A loss that sits behind the walk and reads the plan's taps (P.taps[k]) against a second branch's: the backward starts from it instead of
// from dy_nchw.  Tap k adds scale[k] * d|a - b| (kind 0) or scale[k] * d(a - b)^2 (kind 1) to its tensor's gradient; the input gradient
// leaves times gout[0] * gscale on the frames fr of the 5-D tensor dx_nchw (rd_walk).
struct RdTapLoss { int kind; const RdPlan* Pb; float scale[4]; const float* gout; float gscale; SgFrames fr; };

static int rd_backward(const RdPlan& P, const float* dy_nchw, float* dx_nchw, const float* const* params, void* ws, void* scratch, float* const* grads,
                       const char* tag, void* st, const RdTapLoss* tl = nullptr) {
    SG_REQUIRE((dy_nchw || tl) && params && ws && scratch && grads, "%s backward: null pointer", tag);
    SG_REQUIRE(((uintptr_t)ws % 256) == 0 && ((uintptr_t)scratch % 256) == 0, "%s backward: buffers must be 256-byte aligned", tag);
    const int dt = P.dtype, B = P.B;
    char* w8 = (char*)ws; char* s8 = (char*)scratch; char* wp = w8 + P.wpk;
    float* slab = (float*)(s8 + P.slab); float* gnscr = (float*)(s8 + P.gnscr); float* colscr = (float*)(s8 + P.colscr);
    auto G = [&](int idx) { return idx >= 0 ? grads[idx] : nullptr; };
    {   // dgrad weight packs
        PackList packs(dt, wp);
        for (const RdOp& o : P.ops) {
            const RdT ti = P.T[o.in], to = P.T[o.out];
            const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
            if (o.share) continue;
            if (o.type == 0 && (o.in != 0 || dx_nchw)) {
                if (o.proj) packs.add((const float*)(wp + o.wst), wp + o.wd[0], cin, cout, o.k, o.k, lay_dgrad_s1(cin, o.k, o.k));     // staged by the forward
                else if (o.s == 1) packs.add(params[o.w], wp + o.wd[0], cin, cout, o.k, o.k, lay_dgrad_s1(cin, o.k, o.k));
                else if (o.k == 1) packs.add(params[o.w], wp + o.wd[0], cin, cout, 1, 1, 1, (long)cin, 0, 0, 0);
                else o.s2(cin, cout).pack(packs, params[o.w], wp, o.wd);
            } else if (o.type == 2) {
                packs.add(params[o.w], wp + o.wd[0], ti.C, to.C, 2, 2, (long)to.C * 4, 4, 2, 1, 0);
            } else if (o.type == 5) {       // the input gradient is a 3x3 s2 p1 convolution of dy: rows = ci, k = co, taps as stored
                packs.add(params[o.w], wp + o.wd[0], ti.C, to.C, 3, 3, lay_fwd(to.C, 3, 3));
            }
        }
        char key[64]; snprintf(key, sizeof(key), "%s_bwd", tag);
        SG_TRY(packs.run(key, params[0], st));
    }
    std::vector<char> written(P.T.size(), 0), seen_param(P.nparams + 2, 0);
    auto gt = [&](int id) { return tref(s8 + P.g[id], P.T[id].cs); };
    if (!tl) {
        const RdT& last = P.T.back();
        const int id = (int)P.T.size() - 1;
        SG_TRY(srcgan_nchw_f32_to_nhwc(dy_nchw, s8 + P.g[id], B, P.out_ch, last.H, last.W, last.cs, dt, st));
        if (last.act) SG_TRY(srcgan_mask_inplace(s8 + P.g[id], w8 + last.off, 0.f, (long)B * last.H * last.W * last.cs, dt, st));
        written[id] = 1;
    }
    for (int k = (int)P.ops.size() - 1; k >= 0; --k) {
        const RdOp& o = P.ops[k];
        const RdT ti = P.T[o.in], to = P.T[o.out];
        auto tap_of = [&](int t) { if (tl) for (size_t i = 0; i < P.taps.size(); ++i) if (P.taps[i] == t) return (int)i; return -1; };
        if (const int tk = tap_of(o.out); tk >= 0) {       // (a frozen chain: one op per tensor, so this runs once per tap)
            const RdT tb = tl->Pb->T[o.out];
            SG_TRY(srcgan_feat_loss_bwd(tl->kind, w8 + to.off, to.cs, w8 + tb.off, tb.cs, s8 + P.g[o.out], to.cs, written[o.out], tl->scale[tk],
                                        (long)B * to.H * to.W, to.C, dt, st));
            // the stored gradient of an activated tensor is the one w.r.t. its pre-activation (a pool behind a tap leaves the mask to this pass)
            if (to.act) SG_TRY(srcgan_mask_inplace(s8 + P.g[o.out], w8 + to.off, 0.f, (long)B * to.H * to.W * to.cs, dt, st));
            written[o.out] = 1;
        }
        SG_REQUIRE(written[o.out], "%s backward: internal error (gradient of tensor %d missing)", tag, o.out);
        const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
        TRef xin = sl(rd_t(w8, ti), o.icoff), dy = sl(gt(o.out), o.ocoff);
        const bool need_dx = o.in != 0 || dx_nchw;
        TRef dx = need_dx ? sl(gt(o.in), o.icoff) : TNULL;
        bool acc = need_dx && written[o.in];
        // a module applied twice (SRDenseNet's shared up- / down-sampler): the later use's parameter gradients add to the earlier one's
        const int pacc0 = (o.type == 0 || o.type == 5) ? seen_param[o.w] : 0;
        auto bias_sum = [&](TRef g, long npix, int C, float* out) -> int {
            if (!pacc0) return bias_grad(dt, g, npix, C, 1.f, out, colscr, st);
            float* tmp = (float*)(s8 + P.btmp);
            SG_TRY(bias_grad(dt, g, npix, C, 1.f, tmp, colscr, st));
            return srcgan_add_inplace(out, C, 0, tmp, C, 0, nullptr, 0, 0, 0.f, 1, C, SRCGAN_F32, st);
        };
        if (o.type == 0) {
            if (o.res >= 0) {       // y = conv(x) + res: the residual's gradient is dy itself
                const RdT tr = P.T[o.res];
                TRef dr = gt(o.res);
                if (!written[o.res]) SG_HIP(hipMemcpyAsync(dr.p, dy.p, (size_t)B * tr.H * tr.W * tr.cs * P.esz, hipMemcpyDeviceToDevice, (hipStream_t)st));
                else SG_TRY(srcgan_add_inplace(dr.p, tr.cs, 0, dy.p, to.cs, 0, nullptr, 0, 0, 0.f, (long)B * tr.H * tr.W, tr.C, dt, st));
                written[o.res] = 1;
                acc = need_dx && written[o.in];
            }
            const bool fused_bias = o.bias >= 0 && o.k == 3 && G(o.w);
            if (G(o.w)) {       // a projection: the gradient of the stride-1 form, then back into the stored layout
                float* gw = o.proj ? (float*)(s8 + P.projscr) : G(o.w);
                SG_TRY(wgrad_call(dt, dy, to.H, to.W, cout, xin, B, ti.H, ti.W, cin, o.k, o.k, o.s, o.pad, o.pad, lay_fwd(cin, o.k, o.k), 1.f, slab, gw, st,
                                  fused_bias ? G(o.bias) : nullptr, pacc0));
                if (o.proj)
                    SG_TRY(sg_proj_repack(gw, G(o.w), o.proj - 1, o.proj == 1 ? cout : cout / (o.ps * o.ps), o.proj == 1 ? cin / (o.ps * o.ps) : cin, o.pk, o.ps, 1,
                                          (hipStream_t)st));
            }
            if (o.bias >= 0 && G(o.bias) && !fused_bias) SG_TRY(bias_sum(dy, (long)B * to.H * to.W, cout, G(o.bias)));
            seen_param[o.w] = 1;
            if (need_dx) {
                // (a slice of a dense buffer has several consumers: every contribution is masked by the same ReLU', and the mask of a sum
                //  that already holds masked terms leaves them as they are)
                SG_REQUIRE(!(acc && ti.act) || o.iC, "%s backward: internal error (activated tensor with two consumers)", tag);
                if ((o.in == 0 || ti.C < ti.cs) && !acc) SG_HIP(hipMemsetAsync(dx.p, 0, (size_t)B * ti.H * ti.W * ti.cs * P.esz, (hipStream_t)st));    // padded image channels
                if (o.s == 1) {
                    Conv cv(dt, o.k, o.k, 1);
                    cv.in(dy, B, to.H, to.W, to.C < 8 ? to.cs : cout).w(wp + o.wd[0]).out(dx, ti.H, ti.W, cin).pad(o.k - 1 - o.pad, o.k - 1 - o.pad);
                    if (acc) cv.res1(dx, cin, 1.f);
                    if (ti.act) { cv.mask(xin, 0); cv.d.mslope = 0.f; }
                    SG_TRY(cv.run(st));
                } else if (o.k == 1) {
                    if (!acc) SG_HIP(hipMemsetAsync(dx.p, 0, (size_t)B * ti.H * ti.W * ti.cs * P.esz, (hipStream_t)st));
                    Conv cv(dt, 1, 1, 1);
                    cv.in(dy, B, to.H, to.W, to.C).w(wp + o.wd[0]).out(dx, to.H, to.W, ti.C).pad(0, 0).scatter(2, 0, 0, ti.H, ti.W);
                    if (acc) cv.res1(dx, ti.C, 1.f);
                    SG_TRY(cv.run(st));
                } else
                    SG_TRY(o.s2(ti.C, to.C).run(dt, dy, B, to.H, to.W, dx, ti.H, ti.W, wp, o.wd, acc ? dx : TNULL, ti.act ? xin : TNULL, false, st, 0.f));
                written[o.in] = 1;
            }
        } else if (o.type == 1) {
            void* dres = nullptr; int dres_cs = 0, dres_acc = 0;
            if (o.res >= 0) {       // first contribution to the shortcut's source: plain store, later ones add
                dres = s8 + P.g[o.res]; dres_cs = P.T[o.res].cs; dres_acc = written[o.res]; written[o.res] = 1;
            }
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (GroupNorm input has two consumers or a fused activation)", tag);
            const int pacc = o.w >= 0 ? seen_param[o.w] : 0;       // a GroupNorm module applied more than once (edsr.py:41,47,49): gradients add
            if (o.w >= 0) seen_param[o.w] = 1;
            SG_TRY(srcgan_gn_backward(dy.p, to.cs, o.relu ? (w8 + to.off) : nullptr, to.cs, xin.p, ti.cs, o.w >= 0 ? params[o.w] : nullptr,
                                      (const float*)(w8 + o.stats), dx.p, ti.cs, dres, dres_cs, dres_acc, o.w >= 0 ? G(o.w) : nullptr,
                                      o.w >= 0 ? G(o.w + 1) : nullptr, pacc, o.slope, B, (long)ti.H * ti.W, ti.C, o.ngrp, dt, gnscr, st));
            written[o.in] = 1;
        } else if (o.type == 2) {
            if (G(o.w))     // dW[ci][co][a][b] = sum x[y,x,ci] * dy[2y+a,2x+b,co]: wgrad with roles (dy := x, x := dy), k2 s2
                SG_TRY(wgrad_call(dt, xin, ti.H, ti.W, ti.C, dy, B, to.H, to.W, to.C, 2, 2, 2, 0, 0, WLayout{(long)to.C * 4, 4, 2, 1, 0}, 1.f, slab, G(o.w), st));
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (deconvolution input)", tag);
            SG_TRY(Conv(dt, 2, 2, 2).in(dy, B, to.H, to.W, to.C).w(wp + o.wd[0]).out(dx, ti.H, ti.W, ti.C).pad(0, 0).run(st));
            written[o.in] = 1;
        } else if (o.type == 5) {
            // dW[ci][co][ky][kx] = sum x[i][j][ci] * dy[2i + ky - 1][2j + kx - 1][co]: the stride-2 wgrad with the roles of x and dy exchanged
            if (G(o.w))
                SG_TRY(wgrad_call(dt, xin, ti.H, ti.W, ti.C, dy, B, to.H, to.W, to.C, 3, 3, 2, 1, 1, lay_fwd(to.C, 3, 3), 1.f, slab, G(o.w), st, nullptr, pacc0));
            if (G(o.bias)) SG_TRY(bias_sum(dy, (long)B * to.H * to.W, to.C, G(o.bias)));
            seen_param[o.w] = 1;
            SG_REQUIRE(!acc, "%s backward: internal error (transposed convolution input with two consumers)", tag);
            // dx[i][j][ci] = sum dy[2i + ky - 1][2j + kx - 1][co] * W[ci][co][ky][kx]: the forward 3x3 stride-2 pad-1 convolution
            Conv cv(dt, 3, 3, 2);
            cv.in(dy, B, to.H, to.W, to.C).w(wp + o.wd[0]).out(dx, ti.H, ti.W, ti.C).pad(1, 1);
            if (ti.act) { cv.mask(xin, 0); cv.d.mslope = 0.f; }
            SG_TRY(cv.run(st));
            written[o.in] = 1;
        } else if (o.type == 7) {
            void* dres = nullptr; int dres_cs = 0, dres_acc = 0;
            if (o.res >= 0) {       // the block's input: this op stores (or adds to the group convolution's copy), the block's first convolution adds
                dres = s8 + P.g[o.res]; dres_cs = P.T[o.res].cs; dres_acc = written[o.res]; written[o.res] = 1;
            }
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (attention input has two consumers or a fused activation)", tag);
            SG_TRY(srcgan_ca_backward(dy.p, to.cs, xin.p, ti.cs, params[o.w], params[o.w + 2], (const float*)(w8 + o.stats), dx.p, ti.cs, dres, dres_cs,
                                      dres_acc, G(o.w), G(o.w + 1), G(o.w + 2), G(o.w + 3), B, (long)ti.H * ti.W, ti.C, o.ngrp, dt, gnscr, st));
            written[o.in] = 1;
        } else if (o.type == 8) {
            SG_REQUIRE(!G(o.w) && !G(o.bias), "%s backward: MeanShift is frozen (its gradient pointers must be null)", tag);
            SG_REQUIRE(!acc, "%s backward: internal error (MeanShift input with two consumers)", tag);
            if (need_dx) {
                SG_TRY(sg_meanshift(dy.p, dx.p, params[o.w], nullptr, 1, (long)B * ti.H * ti.W, dt, (hipStream_t)st));
                written[o.in] = 1;
            }
        } else if (o.type == 9) {       // the gather's adjoint is the crop; a second consumer's contribution is added
            SG_TRY(srcgan_d2s_shift(dy.p, to.cs, dx.p, ti.cs, B, ti.H, ti.W, o.iC, o.k, o.pad, to.H, to.W, acc, dt, st));
            written[o.in] = 1;
        } else if (o.type == 10) {
            void* dres = nullptr; int dres_cs = 0, dres_acc = 0;
            if (o.res >= 0) { dres = s8 + P.g[o.res] + (size_t)o.rcoff * P.esz; dres_cs = P.T[o.res].cs; dres_acc = written[o.res]; written[o.res] = 1; }
            SG_REQUIRE(!acc && !ti.act && o.in != o.res, "%s backward: internal error (PReLU input with two consumers or a fused activation)", tag);
            SG_TRY(srcgan_prelu_backward((char*)dy.p + (size_t)dy.coff * P.esz, to.cs, xin.p, ti.cs, params[o.w], o.bias >= 0 ? params[o.bias] : nullptr, dx.p, ti.cs,
                                         dres, dres_cs, o.slope, dres_acc, G(o.w), G(o.bias), B, to.H, to.W, o.oC, o.k, o.pad, ti.H, ti.W, dt,
                                         (float*)(s8 + P.prscr), st));
            written[o.in] = 1;
        } else if (o.type == 6) {
            SG_REQUIRE(!acc, "%s backward: internal error (pooled tensor with two consumers)", tag);
            SG_TRY(srcgan_maxpool2_bwd_nhwc(dy.p, to.cs, xin.p, ti.cs, dx.p, ti.cs, B, ti.H, ti.W, ti.C, ti.act && tap_of(o.in) < 0, dt, st));
            written[o.in] = 1;
        } else {
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (PixelShuffle input)", tag);
            SG_TRY(srcgan_pixel_shuffle_nhwc(dy.p, to.cs, dx.p, ti.cs, B, ti.H, ti.W, to.C, o.k, 1, dt, st));
            written[o.in] = 1;
        }
    }
    if (dx_nchw) {       // gradient w.r.t. the network input (an end-to-end cascade: trainCas.py:108 feeds one network's output to the next)
        SG_REQUIRE(written[0], "%s backward: internal error (no input gradient was produced)", tag);
        if (tl) return sg_frames_grad_store(s8 + P.g[0], P.in_cs, dx_nchw, B / tl->fr.k, tl->fr, P.H, P.W, tl->gout, tl->gscale, dt, (hipStream_t)st);
        SG_TRY(srcgan_nhwc_to_nchw_f32(s8 + P.g[0], dx_nchw, B, P.in_ch, P.H, P.W, P.in_cs, 0, dt, st));
    }
    return 0;
}
}  // namespace

extern "C" int srcgan_resdeconv_num_params(const srcgan_resdeconv_cfg* c) { RdPlan P; if (rd_plan(c, P)) return -1; return P.nparams; }
extern "C" size_t srcgan_resdeconv_ws_bytes(const srcgan_resdeconv_cfg* c) { RdPlan P; if (rd_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_resdeconv_bwd_scratch_bytes(const srcgan_resdeconv_cfg* c) { RdPlan P; if (rd_plan(c, P)) return 0; return P.bwd_total; }
extern "C" int srcgan_resdeconv_forward(const srcgan_resdeconv_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(rd_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, "resdeconv", st);
}
extern "C" int srcgan_resdeconv_backward(const srcgan_resdeconv_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                                         float* const* grads, float* dx_nchw, void* st) {
    RdPlan P;
    SG_TRY(rd_plan(c, P));
    return rd_backward(P, dy_nchw, dx_nchw, params, ws, scratch, grads, "resdeconv", st);
}

extern "C" int srcgan_srnet_num_params(const srcgan_srnet_cfg* c) { RdPlan P; if (sr_plan(c, P)) return -1; return P.nparams; }
extern "C" size_t srcgan_srnet_ws_bytes(const srcgan_srnet_cfg* c) { RdPlan P; if (sr_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_srnet_bwd_scratch_bytes(const srcgan_srnet_cfg* c) { RdPlan P; if (sr_plan(c, P)) return 0; return P.bwd_total; }
extern "C" int srcgan_srnet_forward(const srcgan_srnet_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(sr_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, sr_tag(c->kind), st);
}
extern "C" int srcgan_srnet_backward(const srcgan_srnet_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                                     float* const* grads, float* dx_nchw, void* st) {
    RdPlan P;
    SG_TRY(sr_plan(c, P));
    return rd_backward(P, dy_nchw, dx_nchw, params, ws, scratch, grads, sr_tag(c->kind), st);
}

// Inference forwards of the op-list networks: rd_forward on the liveness-planned workspace (same launches, same arguments apart from
// buffer addresses -> the same bits), and for ResDeconv optionally the folded tail.  The job tables are cached under tags of their
// own: the packs sit at other offsets than the training forward's (no dgrad packs between them).
extern "C" size_t srcgan_resdeconv_infer_ws_bytes(const srcgan_resdeconv_cfg* c, int fold_tail) { RdPlan P; if (rd_infer_plan(c, fold_tail, P)) return 0; return P.total; }
extern "C" size_t srcgan_resdeconv_infer_act_bytes(const srcgan_resdeconv_cfg* c, int fold_tail) { RdPlan P; if (rd_infer_plan(c, fold_tail, P)) return 0; return P.total - P.wpack; }
extern "C" int srcgan_resdeconv_infer_plan(const srcgan_resdeconv_cfg* c, int fold_tail, size_t* ranges, int cap) {
    RdPlan P;
    if (rd_infer_plan(c, fold_tail, P)) return -1;
    return rd_plan_ranges(P, ranges, cap);
}
extern "C" int srcgan_resdeconv_infer(const srcgan_resdeconv_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw,
                                      int fold_tail, void* st) {
    RdPlan P;
    SG_TRY(rd_infer_plan(c, fold_tail, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, fold_tail ? "resdeconv_fold" : "resdeconv_infer", st);
}
extern "C" size_t srcgan_srnet_infer_ws_bytes(const srcgan_srnet_cfg* c) { RdPlan P; if (sr_infer_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_srnet_infer_act_bytes(const srcgan_srnet_cfg* c) { RdPlan P; if (sr_infer_plan(c, P)) return 0; return P.total - P.wpack; }
extern "C" int srcgan_srnet_infer_plan(const srcgan_srnet_cfg* c, size_t* ranges, int cap) {
    RdPlan P;
    if (sr_infer_plan(c, P)) return -1;
    return rd_plan_ranges(P, ranges, cap);
}
extern "C" int srcgan_srnet_infer(const srcgan_srnet_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(sr_infer_plan(c, P));
    char tag[32]; snprintf(tag, sizeof(tag), "%s_infer", sr_tag(c->kind));
    return rd_forward(P, x_nchw, params, ws, y_nchw, tag, st);
}

// SRDenseNetA / SRDenseNetB on the op-list executor (sd_plan); the inference entry runs the same launches on the slot-planned workspace.
extern "C" int srcgan_srdense_num_params(const srcgan_srdense_cfg* c) { RdPlan P; if (sd_plan(c, P)) return -1; return P.nparams; }
extern "C" size_t srcgan_srdense_ws_bytes(const srcgan_srdense_cfg* c) { RdPlan P; if (sd_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_srdense_bwd_scratch_bytes(const srcgan_srdense_cfg* c) { RdPlan P; if (sd_plan(c, P)) return 0; return P.bwd_total; }
extern "C" int srcgan_srdense_out_hw(const srcgan_srdense_cfg* c, int* oh, int* ow) {
    RdPlan P;
    SG_TRY(sd_plan(c, P));
    SG_REQUIRE(oh && ow, "srcgan_srdense_out_hw: null pointer");
    *oh = P.T.back().H; *ow = P.T.back().W;
    return 0;
}
extern "C" int srcgan_srdense_forward(const srcgan_srdense_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(sd_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, c->kind ? "srdenseB" : "srdenseA", st);
}
extern "C" int srcgan_srdense_backward(const srcgan_srdense_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                                       float* const* grads, float* dx_nchw, void* st) {
    RdPlan P;
    SG_TRY(sd_plan(c, P));
    return rd_backward(P, dy_nchw, dx_nchw, params, ws, scratch, grads, c->kind ? "srdenseB" : "srdenseA", st);
}
extern "C" size_t srcgan_srdense_infer_ws_bytes(const srcgan_srdense_cfg* c) { RdPlan P; if (sd_infer_plan(c, P)) return 0; return P.total; }
extern "C" int srcgan_srdense_infer(const srcgan_srdense_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(sd_infer_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, c->kind ? "srdenseB_infer" : "srdenseA_infer", st);
}

// RCAN on the op-list executor (rcan_plan); the inference entries run the same launches on the slot-planned workspace.
extern "C" int srcgan_rcan_num_params(const srcgan_rcan_cfg* c) { RdPlan P; if (rcan_plan(c, P)) return -1; return P.nparams; }
extern "C" size_t srcgan_rcan_ws_bytes(const srcgan_rcan_cfg* c) { RdPlan P; if (rcan_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_rcan_bwd_scratch_bytes(const srcgan_rcan_cfg* c) { RdPlan P; if (rcan_plan(c, P)) return 0; return P.bwd_total; }
extern "C" int srcgan_rcan_forward(const srcgan_rcan_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(rcan_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, "rcan", st);
}
extern "C" int srcgan_rcan_backward(const srcgan_rcan_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                                    float* const* grads, float* dx_nchw, void* st) {
    RdPlan P;
    SG_TRY(rcan_plan(c, P));
    return rd_backward(P, dy_nchw, dx_nchw, params, ws, scratch, grads, "rcan", st);
}
extern "C" size_t srcgan_rcan_infer_ws_bytes(const srcgan_rcan_cfg* c) { RdPlan P; if (rcan_infer_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_rcan_infer_act_bytes(const srcgan_rcan_cfg* c) { RdPlan P; if (rcan_infer_plan(c, P)) return 0; return P.total - P.wpack; }
extern "C" int srcgan_rcan_infer_plan(const srcgan_rcan_cfg* c, size_t* ranges, int cap) {
    RdPlan P;
    if (rcan_infer_plan(c, P)) return -1;
    return rd_plan_ranges(P, ranges, cap);
}
extern "C" int srcgan_rcan_infer(const srcgan_rcan_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(rcan_infer_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, "rcan_infer", st);
}

// DDBPN on the op-list executor (ddbpn_plan); the inference entries run the same launches on the slot-planned workspace.
extern "C" int srcgan_ddbpn_num_params(const srcgan_ddbpn_cfg* c) { RdPlan P; if (ddbpn_plan(c, P)) return -1; return P.nparams; }
extern "C" size_t srcgan_ddbpn_ws_bytes(const srcgan_ddbpn_cfg* c) { RdPlan P; if (ddbpn_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_ddbpn_bwd_scratch_bytes(const srcgan_ddbpn_cfg* c) { RdPlan P; if (ddbpn_plan(c, P)) return 0; return P.bwd_total; }
extern "C" int srcgan_ddbpn_forward(const srcgan_ddbpn_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(ddbpn_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, "ddbpn", st);
}
extern "C" int srcgan_ddbpn_backward(const srcgan_ddbpn_cfg* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch,
                                     float* const* grads, float* dx_nchw, void* st) {
    RdPlan P;
    SG_TRY(ddbpn_plan(c, P));
    return rd_backward(P, dy_nchw, dx_nchw, params, ws, scratch, grads, "ddbpn", st);
}
extern "C" size_t srcgan_ddbpn_infer_ws_bytes(const srcgan_ddbpn_cfg* c) { RdPlan P; if (ddbpn_infer_plan(c, P)) return 0; return P.total; }
extern "C" size_t srcgan_ddbpn_infer_act_bytes(const srcgan_ddbpn_cfg* c) { RdPlan P; if (ddbpn_infer_plan(c, P)) return 0; return P.total - P.wpack; }
extern "C" int srcgan_ddbpn_infer_plan(const srcgan_ddbpn_cfg* c, size_t* ranges, int cap) {
    RdPlan P;
    if (ddbpn_infer_plan(c, P)) return -1;
    return rd_plan_ranges(P, ranges, cap);
}
extern "C" int srcgan_ddbpn_infer(const srcgan_ddbpn_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(ddbpn_infer_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, "ddbpn_infer", st);
}

// ======================================================================================== frozen VGG feature losses
// losses.VGG16Loss (reference src/losses.py:344-393) and losses.PerceptionLoss (:455-470): torchvision's VGG16 / VGG19 `features` prefix as an
// op list of 3x3 convolutions (+ bias + ReLU) and max-pools, walked twice with one set of packs -- on the network's output, whose
// activations stay for the backward, and on the target, on a slot-planned region that keeps only the taps -- and one feature-distance
// reduction per tap.  Frozen: the backward launches input gradients only, on two alternating gradient buffers, at unit scale (see
// include/srcgan_amd.h).
namespace {
struct VggPlan {
    RdPlan P, Pt;             // output branch (every activation kept) / target branch (slot-planned, offsets inside the same workspace)
    int kind, ntap;
    size_t sums, lscr, total;
    float wsum[4];            // loss = sum_k wsum[k] * sum|a_k - b_k|  (1 / (ntaps N_k))
    float gscale[4], gfinal;  // tap k's gradient factor inside the backward (N_1 / N_k), and the one of the final store (1 / (ntaps N_1))
};

// move a slot-planned plan's activation part to `base` of a workspace whose packs are another plan's
static void vgg_rebase(RdPlan& Q, size_t base, const RdPlan& packs) {
    for (RdT& t : Q.T) t.off += base;
    Q.xin += base; Q.gnfwd += base;
    for (size_t k = 0; k < Q.ops.size(); ++k) memcpy(Q.ops[k].wf, packs.ops[k].wf, sizeof(Q.ops[k].wf));
    Q.wpk = packs.wpk;
}

static int vgg_plan(const srcgan_vggloss_cfg* c, bool infer, VggPlan& V) {
    SG_REQUIRE(c, "vggloss: null cfg");
    RdPlan& P = V.P;
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "vggloss"));
    SG_REQUIRE(c->kind == 0 || c->kind == 1, "vggloss: kind must be 0 (VGG16Loss) or 1 (PerceptionLoss)");
    const int minhw = c->kind == 0 ? 8 : 16;
    SG_REQUIRE(c->H >= minhw && c->W >= minhw, "vggloss: H and W must be at least %d (%d max-pools)", minhw, c->kind == 0 ? 3 : 4);
    V.kind = c->kind;
    RdBuilder nb(P, c->B);
    nb.frozen = 1;
    nb.input(3, c->H, c->W);
    int t = 0;
    if (c->kind == 0) {       // vgg16.features[0:23]; taps behind indices 3, 8, 15, 22 (losses.py:354-361, 381-393)
        const int width[4] = {64, 128, 256, 512}, nconv[4] = {2, 2, 3, 3};
        for (int s = 0; s < 4; ++s) {
            if (s) t = nb.pool(t);
            for (int k = 0; k < nconv[s]; ++k) t = nb.conv(t, width[s], 3, 1, 1, true, true);
            nb.tap(t);
        }
    } else {                  // vgg19.features[0:35]: conv5_4 without its ReLU (losses.py:459-468)
        const int width[5] = {64, 128, 256, 512, 512}, nconv[5] = {2, 2, 4, 4, 4};
        for (int s = 0; s < 5; ++s) {
            if (s) t = nb.pool(t);
            for (int k = 0; k < nconv[s]; ++k) t = nb.conv(t, width[s], 3, 1, 1, true, !(s == 4 && k == 3));
        }
        nb.tap(t);
    }
    nb.finish(c->dtype);
    V.ntap = (int)P.taps.size();
    const RdT t1 = P.T[P.taps[0]];
    const double n1 = (double)c->B * t1.C * t1.H * t1.W;
    for (int k = 0; k < V.ntap; ++k) {
        const RdT tk = P.T[P.taps[k]];
        const double nk = (double)c->B * tk.C * tk.H * tk.W;
        V.wsum[k] = (float)(1.0 / (V.ntap * nk));
        V.gscale[k] = (float)(n1 / nk);
    }
    V.gfinal = (float)(1.0 / (V.ntap * n1));
    const size_t packs = P.total - P.wpk;
    V.Pt = P;
    SG_TRY(rd_infer_replan(V.Pt, false, "vggloss"));
    const size_t slot_bytes = V.Pt.act_bytes;
    if (infer) {              // both branches on slot-planned regions, the packs laid out by the replan (forward packs only)
        const size_t ipacks = V.Pt.total - V.Pt.wpk;
        P = V.Pt;
        Bump b;
        b.take(slot_bytes);
        const size_t tgt = b.take(slot_bytes);
        V.sums = b.take(4 * sizeof(float));
        V.lscr = b.take((size_t)srcgan_loss_scratch_floats() * sizeof(float));
        P.wpk = b.off;
        vgg_rebase(V.Pt, tgt, P);
        V.total = align_up(b.off + ipacks, 256);
        return 0;
    }
    Bump b;
    b.take(P.act_bytes);
    const size_t tgt = b.take(slot_bytes);
    V.sums = b.take(4 * sizeof(float));
    V.lscr = b.take((size_t)srcgan_loss_scratch_floats() * sizeof(float));
    P.wpk = b.off;
    vgg_rebase(V.Pt, tgt, P);
    V.total = align_up(b.off + packs, 256);
    return 0;
}

static int vgg_forward(const VggPlan& V, const float* out5d, const float* tgt5d, const float* const* params, void* ws, float* loss_out,
                       const char* tag, void* st, const SgFrames& fr) {
    SG_REQUIRE(out5d && tgt5d && params && ws && loss_out, "%s: null pointer", tag);
    SG_REQUIRE(((uintptr_t)ws % 256) == 0, "%s: workspace must be 256-byte aligned", tag);
    const RdPlan& P = V.P;
    char* w8 = (char*)ws;
    SG_TRY(rd_pack_fwd(P, params, ws, tag, st));
    SG_TRY(rd_walk(P, out5d, params, ws, st, &fr));
    SG_TRY(rd_walk(V.Pt, tgt5d, params, ws, st, &fr));
    float* sums = (float*)(w8 + V.sums);
    for (int k = 0; k < V.ntap; ++k) {
        const RdT a = P.T[P.taps[k]], b = V.Pt.T[P.taps[k]];
        SG_TRY(srcgan_feat_loss_fwd(V.kind, w8 + a.off, a.cs, w8 + b.off, b.cs, (long)P.B * a.H * a.W, a.C, P.dtype, sums + k, (float*)(w8 + V.lscr), st));
    }
    return sg_vgg_combine(sums, V.wsum, V.ntap, loss_out, (hipStream_t)st);
}

static int vgg_backward(const srcgan_vggloss_cfg* c, const float* gout_dev, float gscale, const float* const* params, void* ws, void* scratch,
                        float* dout, void* st, const SgFrames& fr) {
    VggPlan V;
    SG_TRY(vgg_plan(c, false, V));
    SG_REQUIRE(gout_dev && dout, "vggloss backward: null pointer");
    RdTapLoss tl;
    tl.kind = V.kind; tl.Pb = &V.Pt; tl.gout = gout_dev; tl.gscale = gscale * V.gfinal; tl.fr = fr;
    for (int k = 0; k < 4; ++k) tl.scale[k] = k < V.ntap ? V.gscale[k] : 0.f;
    std::vector<float*> nograds(V.P.nparams, nullptr);       // frozen: every parameter gradient is skipped
    return rd_backward(V.P, nullptr, dout, params, ws, scratch, nograds.data(), c->kind ? "vgg19loss" : "vgg16loss", st, &tl);
}

// the frames [f0, f0 + k) of a [Bt, C_in, F, H, W] tensor as the c->B = Bt * k images of a call
static int vgg_frames(const srcgan_vggloss_cfg* c, int C_in, int F, int f0, int k, SgFrames& fr) {
    SG_REQUIRE(c, "vggloss frames: null cfg");
    SG_REQUIRE(C_in == 1 || C_in == 3, "vggloss frames: C_in must be 1 or 3, got %d", C_in);
    SG_REQUIRE(F > 0 && k > 0 && f0 >= 0 && f0 <= F - k, "vggloss frames: frames [%d, %d + %d) leave the %d frames of the tensor", f0, f0, k, F);
    SG_REQUIRE(c->B > 0 && c->B % k == 0, "vggloss frames: cfg.B = %d is not a multiple of the %d frames of the call", c->B, k);
    fr.Cin = C_in; fr.F = F; fr.f0 = f0; fr.k = k;
    return 0;
}
}  // namespace

extern "C" int srcgan_vggloss_num_params(const srcgan_vggloss_cfg* c) { VggPlan V; if (vgg_plan(c, false, V)) return -1; return V.P.nparams; }
extern "C" size_t srcgan_vggloss_ws_bytes(const srcgan_vggloss_cfg* c) { VggPlan V; if (vgg_plan(c, false, V)) return 0; return V.total; }
extern "C" size_t srcgan_vggloss_infer_ws_bytes(const srcgan_vggloss_cfg* c) { VggPlan V; if (vgg_plan(c, true, V)) return 0; return V.total; }
extern "C" size_t srcgan_vggloss_bwd_scratch_bytes(const srcgan_vggloss_cfg* c) { VggPlan V; if (vgg_plan(c, false, V)) return 0; return V.P.bwd_total; }
extern "C" int srcgan_vggloss_forward_frames(const srcgan_vggloss_cfg* c, const float* out5d, const float* tgt5d, int C_in, int F, int f0, int k,
                                             const float* const* params, void* ws, float* loss_out, void* st) {
    SgFrames fr; VggPlan V;
    SG_TRY(vgg_frames(c, C_in, F, f0, k, fr));
    SG_TRY(vgg_plan(c, false, V));
    return vgg_forward(V, out5d, tgt5d, params, ws, loss_out, c->kind ? "vgg19loss" : "vgg16loss", st, fr);
}
extern "C" int srcgan_vggloss_infer_frames(const srcgan_vggloss_cfg* c, const float* out5d, const float* tgt5d, int C_in, int F, int f0, int k,
                                           const float* const* params, void* ws, float* loss_out, void* st) {
    SgFrames fr; VggPlan V;
    SG_TRY(vgg_frames(c, C_in, F, f0, k, fr));
    SG_TRY(vgg_plan(c, true, V));
    return vgg_forward(V, out5d, tgt5d, params, ws, loss_out, c->kind ? "vgg19loss_infer" : "vgg16loss_infer", st, fr);
}
extern "C" int srcgan_vggloss_backward_frames(const srcgan_vggloss_cfg* c, const float* gout_dev, float gscale, int C_in, int F, int f0, int k,
                                              const float* const* params, void* ws, void* scratch, float* dout5d, void* st) {
    SgFrames fr;
    SG_TRY(vgg_frames(c, C_in, F, f0, k, fr));
    return vgg_backward(c, gout_dev, gscale, params, ws, scratch, dout5d, st, fr);
}
