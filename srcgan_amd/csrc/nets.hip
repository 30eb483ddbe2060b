// Whole-network sequencing for the SRCGAN hot path: one C call per nn.Module.forward and one per
// autograd backward.  Pure host code that chains the gfx950 kernels of conv_igemm.hip,
// conv_wgrad.hip and elementwise.hip on the caller's stream (no allocation, no synchronisation:
// graph-capturable).
//
//   RRDB generators (RDDBNet, RDDBNetA, RDDBNetB, legacy RDDBNet, SRDN)   reference src/model/rddb.py:48-114, model.py:347-440, srdn.py
//   NLayerDiscriminator (PatchGAN, BatchNorm2d / InstanceNorm2d)          reference src/model/model.py:595-639
// The op-list networks (ResDeconv, ESPCN, SRCNN, EDSR, SRDenseNetA/B, RCAN, DDBPN, the frozen VGG features) are sequenced by oplist.hip;
// net_common.h holds what the two files share, and this file defines its two pieces of per-process state.
//
// Memory design (HBM): activations live in NHWC.  Each ResidualDenseBlock_5 owns ONE dense buffer of
// nf+4*gc channels; conv k reads the channel prefix [0, nf+(k-1)gc) and writes its own slice, so the
// four torch.cat copies of rddb.py:64-67 (and CatBackward) never exist.  conv5's epilogue fuses
// "x5*0.2 + x" (rddb.py:68), and for RDB3 also the RRDB residual (rddb.py:82), writing straight into
// channels [0,nf) of the next block's dense buffer.  Backward mirrors this with a dense *gradient*
// buffer per block that the dgrads of conv5..conv1 accumulate into in place.
#include "net_common.h"
#include <map>
#include <mutex>
#include <string>

// ---- the per-process state behind net_common.h
int sg_zigzag_next() {
    static const bool zig = sg_env("SRCGAN_NO_ZIGZAG") == nullptr;
    static int flip = 0;
    const int rev = flip;
    flip ^= 1;
    return zig ? rev : 0;
}

namespace {
struct PackCache { std::vector<SgPackJob> host; SgPackJob* dev = nullptr; SgPackJob* pinned = nullptr; size_t cap = 0; hipEvent_t staged = nullptr; };
std::map<std::string, PackCache> g_pack_cache;
std::mutex g_pack_mutex;
}  // namespace

int sg_pack_list_run(const std::vector<SgPackJob>& jobs, long nblk, void* wp_base, int dtype, const char* tag, const void* key_ptr, void* st,
                     const unsigned long long* guard) {
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
    return sg_pack_multi_launch(c.dev, (int)jobs.size(), nblk, wp_base, dtype, (hipStream_t)st, guard);
}

namespace {

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
