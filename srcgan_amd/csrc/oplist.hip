// The op-list executor: networks that are a short list of ops built once per call (RdPlan); the forward walks the list, the backward
// walks it in reverse.  Pure host code that chains the gfx950 kernels on the caller's stream (no allocation, no synchronisation:
// graph-capturable), like nets.hip.
//
//   ResDeconv, ESPCN, SRCNN, EDSR     reference src/model/{resdeconv,espcn,srcnn,edsr}.py
//   SRDenseNetA / SRDenseNetB         reference src/model/model.py:643-786
//   RCAN, DDBPN, RDN, MDSR, VDSR      reference src/model/{rcan,ddbpn,rdn,mdsr,vdsr}.py
//   ResnetGenerator, UnetGenerator    reference src/model/basicModel.py:141-354
//   frozen VGG16 / VGG19 features     reference src/losses.py:344-393, 455-470 (VGG16Loss, PerceptionLoss)
#include "net_common.h"
#include <map>

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
struct RdT { int C, cs, H, W, act; size_t off; int act0; float aslope; int skip; };
// act: produced with a fused activation, so its stored gradient is the one w.r.t. the pre-activation -- its channels from act0 on (RDN's
// dense buffers: the prefix [0, G0) is a block's input, a plain sum); aslope: that activation's negative slope (0 = ReLU), which the
// backward masks take.  skip != 0 (the U-Net): the tensor is LeakyReLU(z), and ReLU(z) of the same z sits in channels [0, C) of the skip
// buffer `skip`, whose gradient slice the tensor's one consumer folds into its input gradient (tensor 0 is the network input: never a skip)
// What an op does.  Every place that branches on the kind is a switch over this enum WITHOUT a default, so -Wswitch names the switch a
// new kind is missing from: a kind a walker has nothing to do for gets an explicit empty case, one it must never meet an "internal error".
enum RdKind {
    RD_CONV = 0,      // convolution (+ bias)(+ ReLU)(+ res); on a dense buffer between channel slices; proj_form != 0: a DDBPN projection
    RD_NORM,          // GroupNorm / InstanceNorm2d (+ res)(+ ReLU / LeakyReLU)
    RD_DECONV2,       // ConvTranspose2d k2 s2
    RD_SHUFFLE,       // PixelShuffle(k)
    RD_FOLD_TAIL,     // (inference plans only) ConvTranspose2d k2 s2 followed by a bias-free 3x3 conv, folded into four parity 2x2 convs
    RD_DECONV3,       // ConvTranspose2d k3 s2 p1 output_padding 1 + bias (+ ReLU) (deconv_k3s2.hip)
    RD_POOL,          // MaxPool2d(2, 2) (vgg_loss.hip)
    RD_ATTN,          // channel attention + block residual (chan_attn.hip): in = t, res = the block's input, w = conv_du.0.weight (its bias and
                      // conv_du.2.{weight,bias} follow), stats = the op's `saved` region
    RD_MEANSHIFT,     // MeanShift, a frozen 1x1 convolution on the 3 image channels (chan_attn.hip)
    RD_GATHER,        // shifted space-to-depth gather (back_proj.hip): image `in` -> grid `out`
    RD_PRELU,         // per-channel PReLU (+ bias)(+ beta * res) (back_proj.hip): in = the pre-activation z, kept for the backward -- a plain
                      // tensor (scale 1) or the grid tensor of a transposed projection, cropped while it is read (scale, shift of the grid);
                      // w = the slope's parameter, bias = the transposed projection's bias or -1, res at channel rcoff of its tensor
    RD_REFLECT,       // ReflectionPad2d(pad) (reflect_pad.hip): the padded tensor is materialised, the convolution behind it runs with pad 0
    RD_TANH,          // Tanh (reflect_pad.hip); the backward reads the saved output
    RD_DECONV4,       // ConvTranspose2d k4 s2 p1 + bias: the four parity 2x2 convolutions of a 4x4 stride-2 input gradient (S2Dgrad), in one
                      // launch where conv_par4.hip's conditions hold
    RD_NORM_SKIP,     // InstanceNorm2d with two activated outputs (unet_skip.hip): out = LeakyReLU(z, slope), and ReLU(z) into channels
                      // [0, C) of the skip buffer `skip`
    RD_RELU,          // ReLU of `in` into channels [ocoff, ocoff + C) of `out` (unet_skip.hip): the outermost U-Net level's half of its skip buffer
};
struct RdOp {
    RdKind type;
    int in, out, res, relu;
    int icoff, iC, ocoff, oC; // RD_CONV on a dense buffer: reads channels [icoff, icoff + iC) of `in`, writes [ocoff, ocoff + oC) of `out` (iC / oC == 0: the whole tensor)
    int rcoff;                // RD_PRELU: first channel of the residual in `res`
    int wkoff, wktot;         // RD_CONV, wktot != 0: the weight is the K slice [wkoff, wkoff + cin) of a parameter [cout][wktot][k][k] (RDN's GFF.0, one slice
                              // per block); the slices of one parameter cover its columns once, so each stores its part of the gradient
    // RD_CONV, proj_form != 0: a DDBPN projection in its stride-1 form over the space-to-depth view (k = ceil(proj_kernel / proj_stride) taps):
    // 1 = Conv2d proj_kernel x proj_kernel stride proj_stride (in = the gathered grid), 2 = ConvTranspose2d (out = the grid); w is the stored
    // weight, re-ordered into the f32 staging area wst (an offset into the pack region) before it is packed
    int proj_form, proj_stride, proj_kernel;
    size_t wst;
    int skip;                 // RD_NORM_SKIP: the skip buffer that takes ReLU(z)
    int share;                // != 0: a module applied a second time -- op share - 1 owns the packs, this op's weight and bias gradients add to its
    union { int k; int scale; };        // kernel size; RD_GATHER / RD_PRELU: the space-to-depth scale of the grid
    int s;
    union { int pad; int shift; };      // padding; RD_GATHER / RD_PRELU: the grid's shift
    int w, bias;              // w: parameter index of the weight (RD_NORM: gamma, beta = w + 1; -1 = no affine part); bias: parameter index or -1
    int w2;                   // RD_FOLD_TAIL: parameter index of the 3x3 convolution's weight (w = the transposed convolution's)
    union { int ngrp; int attn_width; };        // RD_NORM: groups (InstanceNorm2d: = channels); RD_ATTN: the reduced width C / reduction
    union { float slope; float beta; };         // RD_NORM / RD_CONV activation: 0 = ReLU, 0.2 = LeakyReLU (edsr.py:42); RD_PRELU: the residual's factor
    size_t wf[4], wd[4], stats;
    S2Dgrad s2(int cin, int cout) const { return S2Dgrad{k, pad, cin, cout}; }      // input gradient of a stride-2 convolution with k > 1
};
static inline int rd_cin(const RdOp& o, const RdT& ti) { return o.iC ? o.iC : ti.C; }
static inline int rd_cout(const RdOp& o, const RdT& to) { return o.oC ? o.oC : to.C; }
// the canonical Conv2d layouts of an op's weight (forward pack / weight gradient; stride-1 input-gradient pack), K-sliced where the op says so
static inline WLayout rd_lay_fwd(const RdOp& o, int cin) { WLayout L = lay_fwd(o.wktot ? o.wktot : cin, o.k, o.k); L.off += (long)o.wkoff * o.k * o.k; return L; }
static inline WLayout rd_lay_dgrad(const RdOp& o, int cin) { WLayout L = lay_dgrad_s1(o.wktot ? o.wktot : cin, o.k, o.k); L.off += (long)o.wkoff * o.k * o.k; return L; }
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

// ---- what an op needs of the regions a plan shares between its ops, by kind
struct RdFwdNeed { size_t stats, scratch_floats; };       // saved statistics (bytes); forward scratch beyond the floor of rd_fwd_scratch_bytes
static RdFwdNeed rd_fwd_need(const RdPlan& P, const RdOp& o) {
    const RdT ti = P.T[o.in];
    switch (o.type) {
    case RD_NORM: case RD_NORM_SKIP: return {(size_t)P.B * o.ngrp * 2 * sizeof(float), 0};
    case RD_ATTN: return {(size_t)P.B * (2 * ti.C + o.attn_width) * sizeof(float), srcgan_ca_scratch_floats(P.B, (long)ti.H * ti.W, ti.C)};      // saved {p, h, s}
    case RD_CONV: case RD_DECONV2: case RD_SHUFFLE: case RD_FOLD_TAIL: case RD_DECONV3: case RD_POOL: case RD_MEANSHIFT: case RD_GATHER: case RD_PRELU:
    case RD_REFLECT: case RD_TANH: case RD_DECONV4: case RD_RELU:
        break;
    }
    return {0, 0};
}
struct RdBwdNeed { size_t slab, proj, prelu_floats; };     // split-K slab; a projection's weight gradient in its stride-1 form; PReLU partial sums
static RdBwdNeed rd_bwd_need(const RdPlan& P, const RdOp& o) {
    const RdT ti = P.T[o.in], to = P.T[o.out];
    switch (o.type) {
    case RD_CONV: {
        const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
        return {wgrad_slab(P.B, to.H, to.W, cout, cin, o.k, o.k, o.s), o.proj_form ? (size_t)cout * cin * o.k * o.k * sizeof(float) : 0, 0};
    }
    case RD_DECONV2: return {wgrad_slab(P.B, ti.H, ti.W, ti.C, to.C, 2, 2, 2), 0, 0};
    case RD_DECONV3: return {wgrad_slab(P.B, ti.H, ti.W, ti.C, to.C, 3, 3, 2), 0, 0};
    case RD_DECONV4: return {wgrad_slab(P.B, ti.H, ti.W, ti.C, to.C, 4, 4, 2), 0, 0};
    case RD_PRELU: return {0, 0, srcgan_prelu_scratch_floats(P.B, ti.H, ti.W, o.oC, o.scale)};
    case RD_NORM: case RD_SHUFFLE: case RD_FOLD_TAIL: case RD_POOL: case RD_ATTN: case RD_MEANSHIFT: case RD_GATHER: case RD_REFLECT: case RD_TANH:
    case RD_NORM_SKIP: case RD_RELU:
        break;
    }
    return {0, 0, 0};
}
// the forward scratch in bytes: GroupNorm's partial sums for the widest tensor of the plan (every plan's floor), or the largest op's need
static size_t rd_fwd_scratch_bytes(const RdPlan& P) {
    size_t v = srcgan_gn_scratch_floats(P.B, P.maxC > 1024 ? 1024 : P.maxC);
    for (const RdOp& o : P.ops) v = std::max(v, rd_fwd_need(P, o).scratch_floats);
    return v * sizeof(float);
}
// The ONE place that lays out an op list's packs: offsets into the pack region, whose size it returns.  The forward packs and a projection's
// f32 staging area always; the input-gradient packs only for a training plan.  A module's second use shares the first one's packs.
static size_t rd_layout_packs(RdPlan& P, bool train) {
    Bump wb;
    auto pk = [&](int rows, int k, int taps) { return wb.take(srcgan_packed_weight_bytes(rows, k, taps, P.dtype)); };
    for (RdOp& o : P.ops) {
        const RdT ti = P.T[o.in], to = P.T[o.out];
        const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
        if (o.share) {
            memcpy(o.wf, P.ops[o.share - 1].wf, sizeof(o.wf));
            if (train) memcpy(o.wd, P.ops[o.share - 1].wd, sizeof(o.wd));
            continue;
        }
        switch (o.type) {
        case RD_CONV:
            o.wf[0] = pk(cout, cin, o.k * o.k);
            if (train) {
                if (o.s == 1) o.wd[0] = pk(cin, cout, o.k * o.k);
                else if (o.k == 1) o.wd[0] = pk(cin, cout, 1);
                else o.s2(cin, cout).plan(wb, P.dtype, o.wd);
            }
            if (o.proj_form) o.wst = wb.take((size_t)cout * cin * o.k * o.k * sizeof(float));
            break;
        case RD_DECONV2:
            for (int q = 0; q < 4; ++q) o.wf[q] = pk(to.C, ti.C, 1);
            if (train) o.wd[0] = pk(ti.C, to.C, 4);
            break;
        case RD_FOLD_TAIL:      // four composed 2x2 packs of to.cs rows (inference plans only: rd_infer_replan makes the op)
            for (int q = 0; q < 4; ++q) o.wf[q] = pk(to.cs, ti.C, 4);
            break;
        case RD_DECONV3: {      // four parity packs, equally spaced (the 4-tap pack's size)
            const size_t step = srcgan_packed_weight_bytes(to.C, ti.C, 4, P.dtype), w0 = wb.take(4 * step);
            for (int q = 0; q < 4; ++q) o.wf[q] = w0 + q * step;
            if (train) o.wd[0] = pk(ti.C, to.C, 9);
            break;
        }
        case RD_DECONV4:        // the parity packs of the 4x4 s2 p1 input gradient whose "cin" is this op's output width
            S2Dgrad{4, 1, to.C, ti.C}.plan(wb, P.dtype, o.wf);
            if (train) o.wd[0] = pk(ti.C, to.C, 16);
            break;
        case RD_NORM: case RD_SHUFFLE: case RD_POOL: case RD_ATTN: case RD_MEANSHIFT: case RD_GATHER: case RD_PRELU: case RD_REFLECT: case RD_TANH:
        case RD_NORM_SKIP: case RD_RELU:
            break;              // no packed weights
        }
    }
    return wb.off;
}

struct RdBuilder {
    RdPlan& P; Bump b; int np = 0; int B;
    int inorm = 0;            // normalisation layers are InstanceNorm2d (no parameters) instead of GroupNorm(32, C)
    int frozen = 0;           // no parameter takes a gradient and the ops form a chain: the backward scratch is two alternating gradient buffers
    std::vector<std::pair<int, int>> gshare;      // (t, owner < t): tensor t's gradient lives in owner's buffer (equal shapes; never alive together)
    RdBuilder(RdPlan& p, int B_) : P(p), B(B_) {}
    int tensor(int C, int cs, int H, int W, int act = 0) { P.T.push_back(RdT{C, cs, H, W, act, b.take((size_t)B * H * W * cs * P.esz)}); return (int)P.T.size() - 1; }
    int conv(int in, int cout, int k, int s, int pad, bool bias = false, bool relu = false) {
        const RdT ti = P.T[in];
        const int oh = (ti.H + 2 * pad - k) / s + 1, ow = (ti.W + 2 * pad - k) / s + 1;
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_CONV; o.in = in; o.res = -1; o.k = k; o.s = s; o.pad = pad; o.relu = relu; o.w = np++; o.bias = bias ? np++ : -1;
        o.out = tensor(cout, cout < 8 ? 8 : cout, oh, ow, relu);
        P.ops.push_back(o); return o.out;
    }
    // convolution between channel slices of dense buffers (the concat-free dense blocks of SRDenseNet)
    void conv_slice(int in, int icoff, int iC, int out, int ocoff, int oC, int k, int pad) {
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_CONV; o.in = in; o.out = out; o.res = -1; o.k = k; o.s = 1; o.pad = pad; o.relu = 1; o.w = np++; o.bias = np++;
        o.icoff = icoff; o.iC = iC; o.ocoff = ocoff; o.oC = oC;
        P.ops.push_back(o);
    }
    // convolution with explicit parameter indices between channel ranges of existing tensors (iC / oC == 0: the whole tensor)
    RdOp& conv_to(int in, int icoff, int iC, int out, int ocoff, int oC, int k, int pad, int widx, int bidx, bool relu) {
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_CONV; o.in = in; o.out = out; o.res = -1; o.k = k; o.s = 1; o.pad = pad; o.relu = relu; o.w = widx; o.bias = bidx;
        o.icoff = icoff; o.iC = iC; o.ocoff = ocoff; o.oC = oC;
        P.ops.push_back(o); return P.ops.back();
    }
    int deconv3(int in, int cout, bool relu = true) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_DECONV3; o.in = in; o.out = tensor(cout, cout, 2 * ti.H, 2 * ti.W, relu); o.res = -1; o.k = 3; o.s = 2; o.pad = 1; o.relu = relu; o.w = np++; o.bias = np++;
        P.ops.push_back(o); return o.out;
    }
    int reflect(int in, int p) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_REFLECT; o.in = in; o.res = -1; o.pad = p; o.w = -1; o.bias = -1;
        o.out = tensor(ti.C, ti.cs, ti.H + 2 * p, ti.W + 2 * p);
        P.ops.push_back(o); return o.out;
    }
    int tanh(int in) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_TANH; o.in = in; o.res = -1; o.w = -1; o.bias = -1;
        o.out = tensor(ti.C, ti.cs, ti.H, ti.W);
        P.ops.push_back(o); return o.out;
    }
    int deconv4(int in, int cout) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_DECONV4; o.in = in; o.out = tensor(cout, cout < 8 ? 8 : cout, 2 * ti.H, 2 * ti.W); o.res = -1; o.k = 4; o.s = 2; o.pad = 1; o.w = np++; o.bias = np++;
        P.ops.push_back(o); return o.out;
    }
    // InstanceNorm2d of `in` -> a new tensor LeakyReLU(z, slope), and ReLU(z) into channels [0, C) of the skip buffer
    int norm_skip(int in, int skip, float slope) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_NORM_SKIP; o.in = in; o.out = tensor(ti.C, ti.cs, ti.H, ti.W, 1); o.res = -1; o.relu = 1; o.slope = slope; o.skip = skip; o.w = -1; o.bias = -1; o.ngrp = ti.C;
        P.T[o.out].aslope = slope; P.T[o.out].skip = skip;
        o.stats = b.take(rd_fwd_need(P, o).stats);
        P.ops.push_back(o); return o.out;
    }
    // ReLU of `in` into channels [ocoff, ocoff + C) of `out`
    void relu_to(int in, int out, int ocoff) {
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_RELU; o.in = in; o.out = out; o.res = -1; o.ocoff = ocoff; o.oC = P.T[in].C; o.w = -1; o.bias = -1;
        P.ops.push_back(o);
    }
    // InstanceNorm2d (+ ReLU) of `in` into channels [ocoff, ocoff + C) of `out`
    void inorm_to(int in, int out, int ocoff, int relu) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_NORM; o.in = in; o.out = out; o.res = -1; o.relu = relu; o.bias = -1; o.w = -1; o.ngrp = ti.C; o.ocoff = ocoff; o.oC = ti.C;
        o.stats = b.take(rd_fwd_need(P, o).stats);
        P.ops.push_back(o);
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
        o.type = RD_NORM; o.in = in; o.out = tensor(ti.C, ti.cs, ti.H, ti.W); o.res = res; o.relu = relu; o.bias = -1;
        if (inorm) { o.w = -1; o.ngrp = ti.C; } else { o.w = np; np += 2; o.ngrp = 32; }
        o.stats = b.take(rd_fwd_need(P, o).stats);
        P.ops.push_back(o); return o.out;
    }
    int deconv(int in, int cout) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_DECONV2; o.in = in; o.out = tensor(cout, cout, 2 * ti.H, 2 * ti.W); o.res = -1; o.k = 2; o.s = 2; o.w = np++; o.bias = -1;
        P.ops.push_back(o); return o.out;
    }
    int shuffle(int in, int r) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_SHUFFLE; o.in = in; o.res = -1; o.k = r; o.w = -1; o.bias = -1;
        o.out = tensor(ti.C / (r * r), ti.C / (r * r), ti.H * r, ti.W * r);
        P.ops.push_back(o); return o.out;
    }
    int pool(int in) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_POOL; o.in = in; o.res = -1; o.k = 2; o.s = 2; o.w = -1; o.bias = -1;
        o.out = tensor(ti.C, ti.cs, ti.H / 2, ti.W / 2);
        P.ops.push_back(o); return o.out;
    }
    int ca(int in, int res, int cr) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_ATTN; o.in = in; o.res = res; o.out = tensor(ti.C, ti.cs, ti.H, ti.W); o.bias = -1; o.attn_width = cr;
        o.w = np; np += 4;
        o.stats = b.take(rd_fwd_need(P, o).stats);
        P.ops.push_back(o); return o.out;
    }
    int meanshift(int in) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_MEANSHIFT; o.in = in; o.res = -1; o.k = 1; o.s = 1; o.w = np++; o.bias = np++;
        o.out = tensor(3, 8, ti.H, ti.W);
        P.ops.push_back(o); return o.out;
    }
    // convolution with explicit parameter indices reading the channel prefix [0, iC) of `in` (iC == 0: all of it) into a new tensor
    int conv_at(int in, int iC, int cout, int k, int pad, int widx, int bidx, int proj_form = 0, int proj_stride = 0, int proj_kernel = 0) {
        const RdT ti = P.T[in];
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_CONV; o.in = in; o.res = -1; o.k = k; o.s = 1; o.pad = pad; o.w = widx; o.bias = bidx; o.iC = iC;
        o.proj_form = proj_form; o.proj_stride = proj_stride; o.proj_kernel = proj_kernel;
        o.out = tensor(cout, cout < 8 ? 8 : cout, ti.H + 2 * pad - k + 1, ti.W + 2 * pad - k + 1);
        P.ops.push_back(o); return o.out;
    }
    int gather(int in, int iC, int s, int shift, int Hg, int Wg) {
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_GATHER; o.in = in; o.res = -1; o.scale = s; o.shift = shift; o.w = -1; o.bias = -1; o.iC = iC;
        o.out = tensor(s * s * iC, s * s * iC, Hg, Wg);
        P.ops.push_back(o); return o.out;
    }
    // out < 0: a new C-channel tensor of H x W; otherwise channels [ocoff, ocoff + C) of `out`
    int prelu(int in, int C, int H, int W, int s, int shift, int aidx, int bidx, int res, int rcoff, float beta, int out = -1, int ocoff = 0) {
        RdOp o; memset(&o, 0, sizeof(o));
        o.type = RD_PRELU; o.in = in; o.res = res; o.rcoff = rcoff; o.beta = beta; o.scale = s; o.shift = shift; o.w = aidx; o.bias = bidx;
        o.out = out >= 0 ? out : tensor(C, C, H, W); o.ocoff = ocoff; o.oC = C;
        P.ops.push_back(o); return o.out;
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
    void finish() {
        P.nparams = np;
        P.maxC = 8;
        for (const RdT& t : P.T) if (t.C > P.maxC) P.maxC = t.C;
        P.out_ch = P.T.back().C; P.out_cs = P.T.back().cs;
        P.gnfwd = b.take(rd_fwd_scratch_bytes(P));
        P.act_bytes = b.off;
        P.wpk = b.off;
        P.total = align_up(P.wpk + rd_layout_packs(P, true) + 256, 256);
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
        std::vector<int> owner(P.T.size(), -1);
        for (const auto& gs : gshare) owner[gs.first] = gs.second;
        for (size_t i = 0; i < P.T.size(); ++i) {
            P.g[i] = owner[i] >= 0 ? P.g[owner[i]] : s.take((size_t)B * P.T[i].H * P.T[i].W * P.T[i].cs * P.esz);
            if ((long)B * P.T[i].H * P.T[i].W > maxpix) maxpix = (long)B * P.T[i].H * P.T[i].W;
        }
        RdBwdNeed need = {0, 0, 0};
        for (const RdOp& o : P.ops) {
            const RdBwdNeed n = rd_bwd_need(P, o);
            need.slab = std::max(need.slab, n.slab); need.proj = std::max(need.proj, n.proj); need.prelu_floats = std::max(need.prelu_floats, n.prelu_floats);
        }
        P.slab = s.take(need.slab);
        P.projscr = need.proj ? s.take(need.proj) : 0;
        P.prscr = need.prelu_floats ? s.take(need.prelu_floats * sizeof(float)) : 0;
        P.gnscr = s.take(rd_fwd_scratch_bytes(P));
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
    nb.finish();
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
    nb.finish();
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
    nb.finish();
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
    nb.finish();
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
    nb.finish();
    return 0;
}
// RDN (rdn.py:45-105): SFENet1, SFENet2, D residual dense blocks of C 3x3 + ReLU layers and a 1x1 local fusion (LFF) + the block's input,
// GFF = 1x1 over the concatenation of all D block outputs and a 3x3, + SFENet1's output, UPNet (PixelShuffle).  Parameter indices follow
// parameters() order: SFENet1, SFENet2, per block convs.<c>.conv.0 and LFF, GFF.0, GFF.1, UPNet -- the GFF.0 slices run inside the block
// loop, so every op of the trunk gets its indices by hand.
//
// No concatenation anywhere.  Block d owns a dense buffer of G0 + C G channels: layer c reads the prefix [0, G0 + c G) and writes the
// slice [G0 + c G, + G); the LFF reads the whole buffer, takes the prefix [0, G0) -- the block's input -- as its residual and writes the
// prefix of block d + 1's buffer (the last one a plain G0-channel tensor).  GFF.0 is linear, so it runs as D 1x1 convolutions over K
// slices of its weight, acc_d = W[:, d G0 : (d + 1) G0] x_{d+1} (+ bias at d = 0) + acc_{d-1}, each right behind its block's LFF, on two
// alternating accumulators (an op's output must not alias its operands).  Under the slot planner a dense buffer is dead once the next
// block's LFF has read it: two dense buffers and a handful of G0-channel tensors, whatever D is.
// Backward: the LFF's input gradient is the first writer of the whole gradient buffer of its block (the residual's share, dy on the
// prefix, rides in the epilogue); the layers and the GFF slice add to the range they read, under ReLU' from channel G0 on.  The
// accumulators share ONE gradient buffer (the residual's factor is 1: the gradient passes through), the dense buffers two.
static int rdn_plan(const srcgan_rdn_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srcgan_rdn: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srcgan_rdn"));
    SG_REQUIRE(c->in_ch >= 1 && c->in_ch <= 8, "srcgan_rdn: n_colors = %d must be in 1..8", c->in_ch);
    SG_REQUIRE(c->scale == 2 || c->scale == 3 || c->scale == 4, "srcgan_rdn: scale = %d must be 2 or 3 or 4 (rdn.py:76-91)", c->scale);
    SG_REQUIRE(c->D >= 1 && c->C >= 1 && c->G >= 1 && c->G0 >= 1, "srcgan_rdn: D, C, G and G0 must be positive (D = %d, C = %d, G = %d, G0 = %d)", c->D, c->C, c->G, c->G0);
    SG_REQUIRE(c->G0 % 32 == 0 && c->G % 32 == 0, "srcgan_rdn: G0 = %d and G = %d must be multiples of 32 channels (the K chunk of the 16-bit types): layer c's "
               "slice starts at channel G0 + c G", c->G0, c->G);
    SG_REQUIRE((long)c->G0 + (long)c->C * c->G <= 8192, "srcgan_rdn: more than 8192 channels in a dense buffer (G0 + C G = %ld)", (long)c->G0 + (long)c->C * c->G);
    SG_REQUIRE(c->D <= 4096, "srcgan_rdn: D = %d blocks (at most 4096)", c->D);
    const int G0 = c->G0, D = c->D, C = c->C, G = c->G, Cb = G0 + C * G, r = c->scale, H = c->H, W = c->W;
    const int per_block = 2 * C + 2, gff = 4 + D * per_block;
    RdBuilder nb(P, c->B);
    nb.input(c->in_ch, H, W);
    const int f1 = nb.conv(0, G0, 3, 1, 1, true, false);                                   // SFENet1: parameters 0, 1
    std::vector<int> buf(D);
    for (int d = 0; d < D; ++d) {
        buf[d] = nb.tensor(Cb, Cb, H, W, 1);
        P.T[buf[d]].act0 = G0;
        if (d >= 2) nb.gshare.push_back({buf[d], buf[d - 2]});
    }
    const int xD = nb.tensor(G0, G0, H, W), acc[2] = {nb.tensor(G0, G0, H, W), nb.tensor(G0, G0, H, W)};
    nb.gshare.push_back({acc[1], acc[0]});
    nb.conv_to(f1, 0, 0, buf[0], 0, G0, 3, 1, 2, 3, false);                                 // SFENet2
    for (int d = 0; d < D; ++d) {
        const int pb = 4 + d * per_block, out = d + 1 < D ? buf[d + 1] : xD;
        for (int l = 0; l < C; ++l) nb.conv_to(buf[d], 0, G0 + l * G, buf[d], G0 + l * G, G, 3, 1, pb + 2 * l, pb + 2 * l + 1, true);
        nb.conv_to(buf[d], 0, 0, out, 0, G0, 1, 0, pb + 2 * C, pb + 2 * C + 1, false).res = buf[d];           // LFF + x (rdn.py:43)
        RdOp& g = nb.conv_to(out, 0, G0, acc[d & 1], 0, 0, 1, 0, gff, d == 0 ? gff + 1 : -1, false);           // GFF.0, slice d
        g.res = d ? acc[(d - 1) & 1] : -1; g.wkoff = d * G0; g.wktot = D * G0;
    }
    nb.np = gff + 2;
    int t = nb.conv(acc[(D - 1) & 1], G0, 3, 1, 1, true, false);                             // GFF.1, + f__1 (rdn.py:102-103)
    P.ops.back().res = f1;
    for (int f = 1; f < (r == 3 ? 2 : r); f *= 2) {                                          // UPNet (rdn.py:76-89)
        t = nb.conv(t, G * (r == 3 ? 9 : 4), 3, 1, 1, true, false);
        t = nb.shuffle(t, r == 3 ? 3 : 2);
    }
    nb.conv(t, c->in_ch, 3, 1, 1, true, false);
    nb.finish();
    return 0;
}
// MDSR (mdsr.py:13-66).  One module, several graphs: pre_process[i] and upsample[i] exist once per entry of scales, and the plan holds the
// ops of the pair scale_idx alone -- the other branches are parameter indices nobody refers to: not packed, no gradient pass, no zero
// fill, their params / grads entries never read.  So every size of {scales, scale_idx = k} is that of {scales = {scales[k]}, 0}.
// Parameter indices follow parameters() order = registration order: sub_mean, add_mean (:22-23), pre_process, upsample (the ModuleLists
// of :27, 41 are assigned before head / body / tail at :47-49), head, body, tail -- every op gets its indices by hand.
// A ResBlock (common.py:36-57) is conv + bias + ReLU, then conv + bias with `res` = the block's input; its input therefore has two
// consumers (three for the pre_process output, which the body's last convolution adds: mdsr.py:56-57), and the backward gives it the
// residual's share by a plain store and the convolutions' through the in-place residual operand, as for EDSR and RCAN.
static int mdsr_up_params(int s) { return s == 8 ? 6 : s == 4 ? 4 : 2; }     // Upsampler (common.py:59-86): one conv per x2 stage, one for x3
static int mdsr_plan(const srcgan_mdsr_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srcgan_mdsr: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srcgan_mdsr"));
    SG_REQUIRE(c->in_ch == 3 && c->out_ch == 3, "srcgan_mdsr: n_colors must be 3 (MeanShift is a 3-channel convolution, common.py:16)");
    SG_REQUIRE(c->nscale >= 1 && c->nscale <= 4, "srcgan_mdsr: nscale = %d must be in 1..4 (the scale list has at most 4 entries)", c->nscale);
    for (int i = 0; i < c->nscale; ++i)
        SG_REQUIRE(c->scales[i] == 2 || c->scales[i] == 3 || c->scales[i] == 4 || c->scales[i] == 8,
                   "srcgan_mdsr: scales[%d] = %d must be 2, 3, 4 or 8 (common.py:63-84)", i, c->scales[i]);
    SG_REQUIRE(c->scale_idx >= 0 && c->scale_idx < c->nscale, "srcgan_mdsr: scale_idx = %d must be in [0, nscale = %d)", c->scale_idx, c->nscale);
    SG_REQUIRE(c->n_feats > 0 && c->n_feats % 16 == 0 && c->n_feats <= 1024, "srcgan_mdsr: n_feats = %d must be a multiple of 16, at most 1024", c->n_feats);
    SG_REQUIRE(c->n_resblocks >= 1 && c->n_resblocks <= 100000, "srcgan_mdsr: n_resblocks = %d must be in 1..100000", c->n_resblocks);
    const int F = c->n_feats, idx = c->scale_idx, s = c->scales[idx];
    const int pre = 4 + 8 * idx;
    int up = 4 + 8 * c->nscale, head = up;
    for (int i = 0; i < c->nscale; ++i) { if (i < idx) up += mdsr_up_params(c->scales[i]); head += mdsr_up_params(c->scales[i]); }
    const int body = head + 2, tail = body + 4 * c->n_resblocks + 2;
    RdBuilder nb(P, c->B);
    nb.input(3, c->H, c->W);
    // a convolution with bias at parameters (w, w + 1)
    auto cv = [&](int in, int cout, int k, int w, bool relu, int res) {
        const int t = nb.conv(in, cout, k, 1, k / 2, true, relu);
        RdOp& o = P.ops.back();
        o.w = w; o.bias = w + 1; o.res = res;
        return t;
    };
    auto resblock = [&](int x, int k, int w) { return cv(cv(x, F, k, w, true, -1), F, k, w + 2, false, x); };
    int t = nb.meanshift(0);                                    // sub_mean: parameters 0, 1; add_mean: 2, 3
    t = cv(t, F, 3, head, false, -1);
    t = resblock(t, 5, pre);                                    // pre_process[idx] (:27-32, 54)
    const int x = resblock(t, 5, pre + 4);
    t = x;
    for (int k = 0; k < c->n_resblocks; ++k) t = resblock(t, 3, body + 4 * k);
    t = cv(t, F, 3, body + 4 * c->n_resblocks, false, x);       // res += x (:56-57): the pre_process output, not the head's
    if (s == 3) { t = cv(t, 9 * F, 3, up, false, -1); t = nb.shuffle(t, 3); }
    else for (int f = 1, w = up; f < s; f *= 2, w += 2) { t = cv(t, 4 * F, 3, w, false, -1); t = nb.shuffle(t, 2); }
    t = cv(t, 3, 3, tail, false, -1);
    nb.meanshift(t);
    P.ops.back().w = 2; P.ops.back().bias = 3;
    nb.np = tail + 2;
    nb.finish();
    return 0;
}
// the pack-cache tag stem of a branch: one job table per scale_idx, so set_scale between two steps re-stages none
static inline const char* mdsr_tag(int idx) { return idx == 0 ? "mdsr0" : idx == 1 ? "mdsr1" : idx == 2 ? "mdsr2" : "mdsr3"; }
// VDSR (vdsr.py:13-45): sub_mean, n_resblocks - 1 times 3x3 + ReLU (the first from the 3 colours), 3x3 to the 3 colours + the sub_mean
// output (:41-42), add_mean.  parameters() order: sub_mean, add_mean (:21-22), body.<k>.0.  The sub_mean output has two consumers: the
// last convolution's residual stores its gradient, the first convolution's input gradient adds to it in place.
static int vdsr_plan(const srcgan_vdsr_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srcgan_vdsr: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srcgan_vdsr"));
    SG_REQUIRE(c->in_ch == 3, "srcgan_vdsr: n_colors must be 3 (MeanShift is a 3-channel convolution, common.py:16)");
    SG_REQUIRE(c->n_feats > 0 && c->n_feats % 16 == 0 && c->n_feats <= 1024, "srcgan_vdsr: n_feats = %d must be a multiple of 16, at most 1024", c->n_feats);
    SG_REQUIRE(c->n_resblocks >= 2 && c->n_resblocks <= 100000, "srcgan_vdsr: n_resblocks = %d must be in 2..100000 (the first and the last convolution, vdsr.py:32-35)",
               c->n_resblocks);
    RdBuilder nb(P, c->B);
    nb.input(3, c->H, c->W);
    const int x = nb.meanshift(0);                              // sub_mean: parameters 0, 1
    nb.np = 4;                                                  // add_mean: parameters 2, 3
    int t = x;
    for (int k = 0; k < c->n_resblocks - 1; ++k) t = nb.conv(t, c->n_feats, 3, 1, 1, true, true);
    t = nb.conv(t, 3, 3, 1, 1, true, false);
    P.ops.back().res = x;                                       // res += x (:41-42)
    nb.meanshift(t);
    P.ops.back().w = 2; P.ops.back().bias = 3; nb.np -= 2;
    nb.finish();
    return 0;
}
// ResnetGenerator (basicModel.py:141-254) with InstanceNorm2d (no parameters) and use_bias = True: pad 3, 7x7, IN, ReLU; two 3x3 s2 p1,
// each IN + ReLU; n_blocks x [pad 1, 3x3 p0, IN, ReLU, pad 1, 3x3 p0, IN, + x]; two ConvTranspose2d k3 s2 p1 op1 WITHOUT the fused ReLU,
// each IN + ReLU; pad 3, 7x7 + bias, tanh.  parameters() order = the order the ops are built in.  The padded tensors are materialised and
// the convolutions behind them run with pad 0.  A block's input has two consumers: the closing norm's residual stores its gradient
// first (the backward walks in reverse), the pad's backward -- or, with padding 'zero', the convolution's input gradient -- adds.
// Every bias but the last sits in front of an InstanceNorm: its gradient is zero in exact arithmetic and is computed like any other.
static int resnetgen_plan(const srcgan_resnetgen_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srcgan_resnetgen: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srcgan_resnetgen"));
    SG_REQUIRE(c->in_ch >= 1 && c->in_ch <= 8 && c->out_ch >= 1 && c->out_ch <= 8, "srcgan_resnetgen: input_nc = %d and output_nc = %d must be in 1..8", c->in_ch, c->out_ch);
    SG_REQUIRE(c->H >= 8 && c->W >= 8 && c->H % 4 == 0 && c->W % 4 == 0, "srcgan_resnetgen: H = %d and W = %d must be multiples of 4, at least 8 (two stride-2 stages "
               "mirrored by two x2 transposed convolutions; the reflection pad at a quarter of the resolution needs two pixels)", c->H, c->W);
    SG_REQUIRE(c->ngf > 0 && c->ngf % 16 == 0 && c->ngf <= 1024, "srcgan_resnetgen: ngf = %d must be a multiple of 16, at most 1024", c->ngf);
    SG_REQUIRE(c->n_blocks >= 0 && c->n_blocks <= 4096, "srcgan_resnetgen: n_blocks = %d must be in 0..4096", c->n_blocks);
    SG_REQUIRE(c->padding == 0 || c->padding == 1, "srcgan_resnetgen: padding must be 0 ('reflect') or 1 ('zero')");
    const int F = c->ngf, bp = c->padding == 1 ? 1 : 0;
    RdBuilder nb(P, c->B);
    nb.inorm = 1;
    nb.input(c->in_ch, c->H, c->W);
    int t = nb.reflect(0, 3);
    t = nb.conv(t, F, 7, 1, 0, true, false);
    t = nb.gn(t, -1, 1);
    for (int i = 0; i < 2; ++i) {
        t = nb.conv(t, (2 << i) * F, 3, 2, 1, true, false);
        t = nb.gn(t, -1, 1);
    }
    for (int k = 0; k < c->n_blocks; ++k) {         // ResnetBlock (:200-254)
        const int x = t;
        t = bp ? x : nb.reflect(x, 1);
        t = nb.conv(t, 4 * F, 3, 1, bp, true, false);
        t = nb.gn(t, -1, 1);
        if (!bp) t = nb.reflect(t, 1);
        t = nb.conv(t, 4 * F, 3, 1, bp, true, false);
        t = nb.gn(t, x, 0);
    }
    for (int i = 0; i < 2; ++i) {
        t = nb.deconv3(t, (2 >> i) * F, false);
        t = nb.gn(t, -1, 1);
    }
    t = nb.reflect(t, 3);
    t = nb.conv(t, c->out_ch, 7, 1, 0, true, false);
    nb.tanh(t);
    nb.finish();
    return 0;
}
// UnetGenerator (basicModel.py:257-354) with InstanceNorm2d (no parameters) and use_bias = True.  Levels 1 (outermost) .. n, widths
// C_l = ngf min(2^(l-1), 8); d_l: level l's down-sampled pre-activation, u_l: the up path's norm output at level l.
//   down:  a_1 = LeakyReLU(conv(x)) from the epilogue; a_l = LeakyReLU(IN(conv(a_{l-1}))), l = 2 .. n-1; a_n = ReLU(conv(a_{n-1})), no IN
//   skip:  R_l = [ReLU(d_l) | ReLU(u_l)], ONE 2 C_l-channel buffer: RD_RELU (l = 1: ReLU(a_1) = ReLU(d_1)) / RD_NORM_SKIP write the first
//          half, the up path's RD_NORM + ReLU the second.  (The reference's in-place LeakyReLU puts leaky(d_l) into its torch.cat, whose
//          only consumer is a ReLU: ReLU(leaky(z)) = ReLU(z).)
//   up:    deconv(a_n) -> IN + ReLU -> R_{n-1}[C:];  deconv(R_l) -> IN + ReLU -> R_{l-1}[C:];  tanh(deconv(R_1))
// parameters() order = the order the ops are built in.  Backward: an up op runs before its level's down op, so the transposed
// convolution's input gradient, masked by R_l itself, is the first writer of g(R_l); the next level's down convolution adds its own input
// gradient to the first half and masks by LeakyReLU'(a_l): g_z = leaky'(z) (g_a + relu'(z) g_r), stored as g(a_l), the gradient at the
// norm's output.  Every bias in front of an IN (all but the first and last down convolution's and the last transposed one's) has a
// gradient that is zero in exact arithmetic and is computed like any other.
static int unet_plan(const srcgan_unet_cfg* c, RdPlan& P) {
    SG_REQUIRE(c, "srcgan_unet: null cfg");
    SG_TRY(rd_common(c->dtype, c->B, c->H, c->W, P, "srcgan_unet"));
    SG_REQUIRE(c->in_ch >= 1 && c->in_ch <= 8 && c->out_ch >= 1 && c->out_ch <= 8, "srcgan_unet: input_nc = %d and output_nc = %d must be in 1..8", c->in_ch, c->out_ch);
    SG_REQUIRE(c->num_downs >= 5 && c->num_downs <= 24, "srcgan_unet: num_downs = %d must be at least 5 (the reference builds five blocks whatever it is given) "
               "and at most 24", c->num_downs);
    const long m = 1L << c->num_downs;
    SG_REQUIRE(c->H % m == 0 && c->W % m == 0, "srcgan_unet: H = %d and W = %d must be positive multiples of 2^num_downs = %ld (every level halves the image, and "
               "the skip connections need the up path to return to the same sizes)", c->H, c->W, m);
    SG_REQUIRE(c->ngf == 16 || c->ngf == 32 || c->ngf == 64 || c->ngf == 128, "srcgan_unet: ngf = %d must be a multiple of 16 -- 16, 32, 64 or 128: InstanceNorm's "
               "kernels take up to 1024 channels, in numbers whose 16-byte pieces divide 256", c->ngf);
    const int n = c->num_downs, F = c->ngf;
    auto width = [&](int l) { return F * std::min(1 << std::min(l - 1, 3), 8); };
    RdBuilder nb(P, c->B);
    nb.inorm = 1;
    nb.input(c->in_ch, c->H, c->W);
    std::vector<int> R(n, -1);
    int a = nb.conv(0, width(1), 4, 2, 1, true, true);
    P.ops.back().slope = 0.2f; P.T[a].aslope = 0.2f;
    R[1] = nb.tensor(2 * width(1), 2 * width(1), P.T[a].H, P.T[a].W, 1);
    nb.relu_to(a, R[1], 0);
    P.T[a].skip = R[1];
    for (int l = 2; l < n; ++l) {
        const int d = nb.conv(a, width(l), 4, 2, 1, true, false);
        R[l] = nb.tensor(2 * width(l), 2 * width(l), P.T[d].H, P.T[d].W, 1);
        a = nb.norm_skip(d, R[l], 0.2f);
    }
    int src = nb.conv(a, width(n), 4, 2, 1, true, true);        // the innermost level: ReLU from the epilogue, no norm, C_n channels to its deconv
    for (int l = n - 1; l >= 1; --l) {
        const int t = nb.deconv4(src, width(l));
        nb.inorm_to(t, R[l], width(l), 1);
        src = R[l];
    }
    nb.tanh(nb.deconv4(src, c->out_ch));
    nb.finish();
    return 0;
}
static inline TRef rd_t(char* base, const RdT& t) { return tref(base + t.off, t.cs); }
static inline const char* sr_tag(int kind) { return kind == 0 ? "espcn" : kind == 1 ? "srcnn" : "edsr"; }      // pack-cache tag stem / name in messages

// the forward in three parts (a frozen feature extractor packs once and walks twice, on two inputs)
static int rd_pack_fwd(const RdPlan& P, const float* const* params, void* ws, const char* tag, void* st) {
    const int dt = P.dtype;
    char* w8 = (char*)ws; char* wp = w8 + P.wpk;
    PackList packs(dt, wp);
    const RdOp* fold = nullptr;         // a plan has at most one folded tail (its last op)
    for (const RdOp& o : P.ops) {
        const RdT ti = P.T[o.in], to = P.T[o.out];
        const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
        if (o.share) continue;          // packed by the module's first use
        switch (o.type) {
        case RD_CONV:
            if (o.proj_form) {          // the stored weight in its stride-1 form: an f32 Conv2d weight [cout][cin][k][k] in the staging area
                const int s2 = o.proj_stride * o.proj_stride;
                SG_TRY(sg_proj_repack(params[o.w], (float*)(wp + o.wst), o.proj_form - 1, o.proj_form == 1 ? cout : cout / s2, o.proj_form == 1 ? cin / s2 : cin,
                                      o.proj_kernel, o.proj_stride, 0, (hipStream_t)st));
                packs.add((const float*)(wp + o.wst), wp + o.wf[0], cout, cin, o.k, o.k, lay_fwd(cin, o.k, o.k));
            } else
                packs.add(params[o.w], wp + o.wf[0], cout, cin, o.k, o.k, rd_lay_fwd(o, cin));
            break;
        case RD_DECONV2:
            for (int q = 0; q < 4; ++q) packs.add(params[o.w], wp + o.wf[q], to.C, ti.C, 1, 1, 4, (long)to.C * 4, 0, 0, q);
            break;
        case RD_DECONV3: deconv3_pack(packs, params[o.w], wp, o.wf, ti.C, to.C); break;
        case RD_FOLD_TAIL: fold = &o; break;        // composed from two sources, behind the batched launch
        case RD_DECONV4: S2Dgrad{4, 1, to.C, ti.C}.pack(packs, params[o.w], wp, o.wf); break;      // the stored [in][out][4][4] is that convolution's [cout][cin][4][4]
        case RD_NORM: case RD_SHUFFLE: case RD_POOL: case RD_ATTN: case RD_MEANSHIFT: case RD_GATHER: case RD_PRELU: case RD_REFLECT: case RD_TANH:
        case RD_NORM_SKIP: case RD_RELU:
            break;                      // no packed weights
        }
    }
    char key[64]; snprintf(key, sizeof(key), "%s_fwd", tag);
    SG_TRY(packs.run(key, params[0], st));
    if (fold)       // made on every call, like the packs above
        SG_TRY(sg_fold_tail_pack(params[fold->w], params[fold->w2], wp + fold->wf[0], P.T[fold->out].C, dt, (hipStream_t)st));
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
        switch (o.type) {
        case RD_CONV: {
            if (to.C < to.cs) SG_HIP(hipMemsetAsync(out.p, 0, (size_t)B * to.H * to.W * to.cs * P.esz, (hipStream_t)st));
            Conv cv(dt, o.k, o.k, o.s);
            cv.in(sl(xin, o.icoff), B, ti.H, ti.W, ti.C < 8 ? ti.cs : rd_cin(o, ti)).w(wp + o.wf[0], o.bias >= 0 ? params[o.bias] : nullptr)
                .out(sl(out, o.ocoff), to.H, to.W, rd_cout(o, to)).pad(o.pad, o.pad);
            if (o.relu) { cv.lrelu(); cv.d.slope = o.slope; }
            if (o.res >= 0) cv.res1(rd_t(w8, P.T[o.res]), rd_cout(o, to), 1.f);        // y = conv(x) + res (edsr.py:97-98); a wider `res`: its prefix
            SG_TRY(cv.run(st));
            break;
        }
        case RD_NORM: {
            const void* res = o.res >= 0 ? (w8 + P.T[o.res].off) : nullptr;
            SG_TRY(srcgan_gn_forward(xin.p, ti.cs, res, o.res >= 0 ? P.T[o.res].cs : 0, (char*)out.p + (size_t)o.ocoff * P.esz, to.cs, o.w >= 0 ? params[o.w] : nullptr,
                                     o.w >= 0 ? params[o.w + 1] : nullptr, (float*)(w8 + o.stats), B, (long)ti.H * ti.W, ti.C, o.ngrp, 1e-5f, o.relu,
                                     o.slope, dt, gnscr, st));
            break;
        }
        case RD_DECONV2:
            for (int q = 0; q < 4; ++q)
                SG_TRY(Conv(dt, 1, 1, 1).in(xin, B, ti.H, ti.W, ti.C).w(wp + o.wf[q]).out(out, ti.H, ti.W, to.C)
                           .scatter(2, q >> 1, q & 1, to.H, to.W).run(st));
            break;
        case RD_SHUFFLE:
            SG_TRY(srcgan_pixel_shuffle_nhwc(xin.p, ti.cs, out.p, to.cs, B, ti.H, ti.W, to.C, o.k, 0, dt, st));
            break;
        case RD_FOLD_TAIL: {
            // output pixel (2i + a, 2j + b) = 2x2 window of the half-resolution input at (i + a - 1, j + b - 1) times the
            // composed weights of parity (a, b) -- the geometry of the 4x4 stride-2 input gradient, so its four-parity kernel serves.
            // All to.cs channels are written (the pack's rows >= to.C are zero): no memset of the padded channels.
            Conv cv(dt, 2, 2, 1);
            cv.in(xin, B, ti.H, ti.W, ti.C).w(wp + o.wf[0]).out(out, ti.H, ti.W, to.cs).scatter(2, 0, 0, to.H, to.W);
            cv.d.npar = 4; cv.d.wpar_stride = (long)(o.wf[1] - o.wf[0]);
            SG_TRY(cv.run(st));
            break;
        }
        case RD_DECONV3: {
            // output pixel (2i + a, 2j + b) = the 1, 2, 2 or 4 taps of parity (a, b) over x[i..i+1][j..j+1]: all four in one launch
            Conv cv(dt, 3, 3, 2);
            cv.in(xin, B, ti.H, ti.W, ti.C).w(wp + o.wf[0], params[o.bias]).out(out, ti.H, ti.W, to.C).pad(1, 1).scatter(2, 0, 0, to.H, to.W);
            if (o.relu) cv.lrelu();
            cv.d.slope = 0.f; cv.d.npar = 4; cv.d.wpar_stride = (long)(o.wf[1] - o.wf[0]);
            SG_TRY(cv.run(st));
            break;
        }
        case RD_POOL:
            SG_TRY(srcgan_maxpool2_nhwc(xin.p, ti.cs, out.p, to.cs, B, ti.H, ti.W, ti.C, dt, st));
            break;
        case RD_ATTN: {
            const void* res = o.res >= 0 ? (w8 + P.T[o.res].off) : nullptr;
            SG_TRY(srcgan_ca_forward(xin.p, ti.cs, res, o.res >= 0 ? P.T[o.res].cs : 0, out.p, to.cs, params[o.w], params[o.w + 1], params[o.w + 2],
                                     params[o.w + 3], (float*)(w8 + o.stats), B, (long)ti.H * ti.W, ti.C, o.attn_width, dt, gnscr, st));
            break;
        }
        case RD_MEANSHIFT:
            SG_TRY(sg_meanshift(xin.p, out.p, params[o.w], params[o.bias], 0, (long)B * ti.H * ti.W, dt, (hipStream_t)st));
            break;
        case RD_GATHER:
            SG_TRY(srcgan_s2d_shift(xin.p, ti.cs, out.p, to.cs, B, ti.H, ti.W, o.iC, o.scale, o.shift, to.H, to.W, dt, st));
            break;
        case RD_PRELU: {
            const void* res = o.res >= 0 ? (w8 + P.T[o.res].off + (size_t)o.rcoff * P.esz) : nullptr;
            SG_TRY(srcgan_prelu_forward(xin.p, ti.cs, params[o.w], o.bias >= 0 ? params[o.bias] : nullptr, res, o.res >= 0 ? P.T[o.res].cs : 0, o.beta,
                                        (char*)out.p + (size_t)o.ocoff * P.esz, to.cs, B, to.H, to.W, o.oC, o.scale, o.shift, ti.H, ti.W, dt, st));
            break;
        }
        case RD_REFLECT:        // all cs channels: an image record's zero channels stay zero
            SG_TRY(srcgan_reflect_pad_nhwc(xin.p, ti.cs, out.p, to.cs, B, ti.H, ti.W, ti.cs, o.pad, dt, st));
            break;
        case RD_TANH:
            SG_TRY(srcgan_tanh_forward(xin.p, ti.cs, out.p, to.cs, (long)B * ti.H * ti.W, ti.cs, dt, st));
            break;
        case RD_DECONV4:
            // y[2t + a][2u + b][co] = bias[co] + sum over the 2x2 taps of parity (a, b) and ci of x[t + a - 1 + ty][u + b - 1 + tx][ci] W[ci][co][ky][kx]:
            // conv_par4.hip's formula; one launch where its conditions hold, four 2x2 launches otherwise (1..8 output channels)
            if (to.C < to.cs) SG_HIP(hipMemsetAsync(out.p, 0, (size_t)B * to.H * to.W * to.cs * P.esz, (hipStream_t)st));
            SG_TRY((S2Dgrad{4, 1, to.C, ti.C}.run(dt, xin, B, ti.H, ti.W, out, to.H, to.W, wp, o.wf, TNULL, TNULL, true, st, 0.f, params[o.bias])));
            break;
        case RD_NORM_SKIP: {
            const RdT ts = P.T[o.skip];
            SG_TRY(srcgan_in_skip_forward(xin.p, ti.cs, out.p, to.cs, w8 + ts.off, ts.cs, 0, (float*)(w8 + o.stats), B, (long)ti.H * ti.W, ti.C, 1e-5f, o.slope,
                                          dt, gnscr, st));
            break;
        }
        case RD_RELU:
            SG_TRY(srcgan_relu_nhwc(xin.p, ti.cs, out.p, to.cs, o.ocoff, (long)B * ti.H * ti.W, ti.C, dt, st));
            break;
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
// becomes one RD_FOLD_TAIL op, and the full-resolution tensor between them gets no slot.
static inline size_t rd_bytes(const RdPlan& P, const RdT& t) { return (size_t)P.B * t.H * t.W * t.cs * P.esz; }

static int rd_infer_replan(RdPlan& P, bool fold, const char* who, size_t spare = 0) {
    if (fold) {
        const int n = (int)P.ops.size();
        SG_REQUIRE(n >= 2, "%s: no tail to fold", who);
        const RdOp d = P.ops[n - 2], c = P.ops[n - 1];
        SG_REQUIRE(d.type == RD_DECONV2 && c.type == RD_CONV && c.in == d.out && c.k == 3 && c.s == 1 && c.pad == 1 && c.bias < 0 && !c.relu && c.res < 0 &&
                   P.T[d.in].C == 64 && P.T[d.out].C == 64 && P.T[c.out].cs == 8,
                   "%s: the tail is not ConvTranspose2d(64, 64, k2 s2) -> bias-free 3x3 convolution to <= 8 channels", who);
        RdOp f; memset(&f, 0, sizeof(f));
        f.type = RD_FOLD_TAIL; f.in = d.in; f.out = c.out; f.res = -1; f.k = 2; f.s = 1; f.w = d.w; f.w2 = c.w; f.bias = -1;
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
        if (o.skip && !have[o.skip]) { get(o.skip); have[o.skip] = 1; }      // a second output: alive until its reader, the level's transposed convolution
        if (last[o.in] == k) put(o.in);
        if (o.res >= 0 && o.res != o.in && last[o.res] == k) put(o.res);
    }
    if (spare) b.take(spare);
    size_t stats = 0;           // GroupNorm statistics and the attention ops' saved {p, h, s} share one region: nothing reads them after the op
    for (const RdOp& o : P.ops) stats = std::max(stats, rd_fwd_need(P, o).stats);
    const size_t stats_off = b.take(stats);
    for (RdOp& o : P.ops) if (rd_fwd_need(P, o).stats) o.stats = stats_off;
    P.gnfwd = b.take(rd_fwd_scratch_bytes(P));
    P.act_bytes = b.off;
    P.wpk = b.off;
    P.wpack = rd_layout_packs(P, false);
    P.total = align_up(P.wpk + P.wpack + 256, 256);
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
// the families without a deviation: the training plan, slot-planned
#define RD_INFER_PLAN(NAME, CFG, PLAN, WHO) \
    static int NAME(const CFG* c, RdPlan& P) { SG_TRY(PLAN(c, P)); return rd_infer_replan(P, false, WHO); }
RD_INFER_PLAN(sd_infer_plan, srcgan_srdense_cfg, sd_plan, "srdense")
RD_INFER_PLAN(rcan_infer_plan, srcgan_rcan_cfg, rcan_plan, "srcgan_rcan")
RD_INFER_PLAN(ddbpn_infer_plan, srcgan_ddbpn_cfg, ddbpn_plan, "srcgan_ddbpn")
RD_INFER_PLAN(rdn_infer_plan, srcgan_rdn_cfg, rdn_plan, "srcgan_rdn")
RD_INFER_PLAN(mdsr_infer_plan, srcgan_mdsr_cfg, mdsr_plan, "srcgan_mdsr")
RD_INFER_PLAN(vdsr_infer_plan, srcgan_vdsr_cfg, vdsr_plan, "srcgan_vdsr")
RD_INFER_PLAN(resnetgen_infer_plan, srcgan_resnetgen_cfg, resnetgen_plan, "srcgan_resnetgen")
RD_INFER_PLAN(unet_infer_plan, srcgan_unet_cfg, unet_plan, "srcgan_unet")
#undef RD_INFER_PLAN
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
    // tensors whose gradient nobody wants: the network input when dx_nchw is null, and its reflection-padded copy
    std::vector<char> nograd(P.T.size(), 0);
    nograd[0] = !dx_nchw;
    for (const RdOp& o : P.ops) if (o.type == RD_REFLECT && nograd[o.in]) nograd[o.out] = 1;
    {   // dgrad weight packs
        PackList packs(dt, wp);
        for (const RdOp& o : P.ops) {
            const RdT ti = P.T[o.in], to = P.T[o.out];
            const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
            if (o.share) continue;
            switch (o.type) {
            case RD_CONV:
                if (nograd[o.in]) break;                // the network input's gradient is not wanted
                if (o.proj_form) packs.add((const float*)(wp + o.wst), wp + o.wd[0], cin, cout, o.k, o.k, lay_dgrad_s1(cin, o.k, o.k));     // staged by the forward
                else if (o.s == 1) packs.add(params[o.w], wp + o.wd[0], cin, cout, o.k, o.k, rd_lay_dgrad(o, cin));
                else if (o.k == 1) packs.add(params[o.w], wp + o.wd[0], cin, cout, 1, 1, 1, (long)cin, 0, 0, 0);
                else o.s2(cin, cout).pack(packs, params[o.w], wp, o.wd);
                break;
            case RD_DECONV2:
                packs.add(params[o.w], wp + o.wd[0], ti.C, to.C, 2, 2, (long)to.C * 4, 4, 2, 1, 0);
                break;
            case RD_DECONV3:        // the input gradient is a 3x3 s2 p1 convolution of dy: rows = ci, k = co, taps as stored
                packs.add(params[o.w], wp + o.wd[0], ti.C, to.C, 3, 3, lay_fwd(to.C, 3, 3));
                break;
            case RD_DECONV4:        // the input gradient is a 4x4 s2 p1 convolution of dy: rows = ci, k = co, taps as stored
                packs.add(params[o.w], wp + o.wd[0], ti.C, to.C, 4, 4, lay_fwd(to.C, 4, 4));
                break;
            case RD_FOLD_TAIL:
                SG_FAIL("%s backward: internal error (a folded tail in a training plan)", tag);
            case RD_NORM: case RD_SHUFFLE: case RD_POOL: case RD_ATTN: case RD_MEANSHIFT: case RD_GATHER: case RD_PRELU: case RD_REFLECT: case RD_TANH:
            case RD_NORM_SKIP: case RD_RELU:
                break;              // no packed weights
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
        if (nograd[o.out]) continue;
        SG_REQUIRE(written[o.out], "%s backward: internal error (gradient of tensor %d missing)", tag, o.out);
        const int cin = rd_cin(o, ti), cout = rd_cout(o, to);
        TRef xin = sl(rd_t(w8, ti), o.icoff), dy = sl(gt(o.out), o.ocoff);
        const bool need_dx = !nograd[o.in];
        TRef dx = need_dx ? sl(gt(o.in), o.icoff) : TNULL;
        bool acc = need_dx && written[o.in];
        // a module applied twice (SRDenseNet's shared up- / down-sampler): the later use's parameter gradients add to the earlier one's
        auto bias_sum = [&](TRef g, long npix, int C, float* out, int pacc0) -> int {
            if (!pacc0) return bias_grad(dt, g, npix, C, 1.f, out, colscr, st);
            float* tmp = (float*)(s8 + P.btmp);
            SG_TRY(bias_grad(dt, g, npix, C, 1.f, tmp, colscr, st));
            return srcgan_add_inplace(out, C, 0, tmp, C, 0, nullptr, 0, 0, 0.f, 1, C, SRCGAN_F32, st);
        };
        switch (o.type) {
        case RD_CONV: {
            const int pacc0 = o.wktot ? 0 : seen_param[o.w];       // (K slices of one parameter: disjoint columns, each stored once)
            const bool res_in = o.res >= 0 && o.res == o.in;       // the residual is the input's own prefix (RDN's LFF): its gradient joins dx below
            if (o.res >= 0 && !res_in && P.g[o.res] == P.g[o.out]) written[o.res] = 1;        // an accumulator chain on one gradient buffer: dy is it
            else if (o.res >= 0 && !res_in) {       // y = conv(x) + res: the residual's gradient is dy itself
                const RdT tr = P.T[o.res];
                TRef dr = gt(o.res);
                if (!written[o.res]) SG_HIP(hipMemcpyAsync(dr.p, dy.p, (size_t)B * tr.H * tr.W * tr.cs * P.esz, hipMemcpyDeviceToDevice, (hipStream_t)st));
                else SG_TRY(srcgan_add_inplace(dr.p, tr.cs, 0, dy.p, to.cs, 0, nullptr, 0, 0, 0.f, (long)B * tr.H * tr.W, tr.C, dt, st));
                written[o.res] = 1;
                acc = need_dx && written[o.in];
            }
            const bool fused_bias = o.bias >= 0 && o.k == 3 && G(o.w);
            if (G(o.w)) {       // a projection: the gradient of the stride-1 form, then back into the stored layout
                float* gw = o.proj_form ? (float*)(s8 + P.projscr) : G(o.w);
                SG_TRY(wgrad_call(dt, dy, to.H, to.W, cout, xin, B, ti.H, ti.W, cin, o.k, o.k, o.s, o.pad, o.pad, rd_lay_fwd(o, cin), 1.f, slab, gw, st,
                                  fused_bias ? G(o.bias) : nullptr, pacc0));
                if (o.proj_form) {
                    const int s2 = o.proj_stride * o.proj_stride;
                    SG_TRY(sg_proj_repack(gw, G(o.w), o.proj_form - 1, o.proj_form == 1 ? cout : cout / s2, o.proj_form == 1 ? cin / s2 : cin, o.proj_kernel,
                                          o.proj_stride, 1, (hipStream_t)st));
                }
            }
            if (o.bias >= 0 && G(o.bias) && !fused_bias) SG_TRY(bias_sum(dy, (long)B * to.H * to.W, cout, G(o.bias), pacc0));
            seen_param[o.w] = 1;
            if (need_dx) {
                // (a slice of a dense buffer has several consumers: every contribution is masked by the same ReLU', and the mask of a sum
                //  that already holds masked terms leaves them as they are)
                SG_REQUIRE(!(acc && ti.act) || o.iC, "%s backward: internal error (activated tensor with two consumers)", tag);
                if ((o.in == 0 || ti.C < ti.cs) && !acc) SG_HIP(hipMemsetAsync(dx.p, 0, (size_t)B * ti.H * ti.W * ti.cs * P.esz, (hipStream_t)st));    // padded image channels
                if (o.s == 1) {
                    Conv cv(dt, o.k, o.k, 1);
                    cv.in(dy, B, to.H, to.W, to.C < 8 ? to.cs : cout).w(wp + o.wd[0]).out(dx, ti.H, ti.W, cin).pad(o.k - 1 - o.pad, o.k - 1 - o.pad);
                    SG_REQUIRE(!(acc && res_in), "%s backward: internal error (a residual that is its op's input needs the first write)", tag);
                    if (acc) cv.res1(dx, cin, 1.f);
                    else if (res_in) cv.res1(dy, cout, 1.f);        // dx[:, :cout] += dy
                    const int c0 = std::max(0, ti.act0 - o.icoff);
                    if (ti.act && c0 < cin) { cv.mask(xin, c0); cv.d.mslope = ti.aslope; }
                    SG_TRY(cv.run(st));
                } else if (o.k == 1) {
                    if (!acc) SG_HIP(hipMemsetAsync(dx.p, 0, (size_t)B * ti.H * ti.W * ti.cs * P.esz, (hipStream_t)st));
                    Conv cv(dt, 1, 1, 1);
                    cv.in(dy, B, to.H, to.W, to.C).w(wp + o.wd[0]).out(dx, to.H, to.W, ti.C).pad(0, 0).scatter(2, 0, 0, ti.H, ti.W);
                    if (acc) cv.res1(dx, ti.C, 1.f);
                    SG_TRY(cv.run(st));
                } else {
                    // xin = LeakyReLU(z) with ReLU(z) in a skip buffer (the U-Net): the transposed convolution behind the buffer stored
                    // relu'(z) g_r there; this one adds g_a and masks the sum by leaky'(z) -- the gradient at z, in one epilogue
                    TRef add = acc ? dx : TNULL;
                    if (ti.skip) {
                        SG_REQUIRE(!acc && written[ti.skip] && ti.act, "%s backward: internal error (the skip buffer's gradient must precede its level's down convolution)", tag);
                        add = gt(ti.skip);
                    }
                    SG_TRY(o.s2(ti.C, to.C).run(dt, dy, B, to.H, to.W, dx, ti.H, ti.W, wp, o.wd, add, ti.act ? xin : TNULL, o.k == 4 && o.pad == 1, st, ti.aslope));
                }
                written[o.in] = 1;
            }
            break;
        }
        case RD_NORM: {
            void* dres = nullptr; int dres_cs = 0, dres_acc = 0;
            if (o.res >= 0) {       // first contribution to the shortcut's source: plain store, later ones add
                dres = s8 + P.g[o.res]; dres_cs = P.T[o.res].cs; dres_acc = written[o.res]; written[o.res] = 1;
            }
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (GroupNorm input has two consumers or a fused activation)", tag);
            const int pacc = o.w >= 0 ? seen_param[o.w] : 0;       // a GroupNorm module applied more than once (edsr.py:41,47,49): gradients add
            if (o.w >= 0) seen_param[o.w] = 1;
            // (a slice of an activated buffer -- the U-Net's skip: its reader's input gradient arrived masked by the buffer itself)
            SG_TRY(srcgan_gn_backward((char*)dy.p + (size_t)dy.coff * P.esz, to.cs, o.relu && !to.act ? (w8 + to.off + (size_t)o.ocoff * P.esz) : nullptr, to.cs, xin.p, ti.cs,
                                      o.w >= 0 ? params[o.w] : nullptr,
                                      (const float*)(w8 + o.stats), dx.p, ti.cs, dres, dres_cs, dres_acc, o.w >= 0 ? G(o.w) : nullptr,
                                      o.w >= 0 ? G(o.w + 1) : nullptr, pacc, o.slope, B, (long)ti.H * ti.W, ti.C, o.ngrp, dt, gnscr, st));
            written[o.in] = 1;
            break;
        }
        case RD_DECONV2:
            if (G(o.w))     // dW[ci][co][a][b] = sum x[y,x,ci] * dy[2y+a,2x+b,co]: wgrad with roles (dy := x, x := dy), k2 s2
                SG_TRY(wgrad_call(dt, xin, ti.H, ti.W, ti.C, dy, B, to.H, to.W, to.C, 2, 2, 2, 0, 0, WLayout{(long)to.C * 4, 4, 2, 1, 0}, 1.f, slab, G(o.w), st));
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (deconvolution input)", tag);
            SG_TRY(Conv(dt, 2, 2, 2).in(dy, B, to.H, to.W, to.C).w(wp + o.wd[0]).out(dx, ti.H, ti.W, ti.C).pad(0, 0).run(st));
            written[o.in] = 1;
            break;
        case RD_DECONV3: {
            const int pacc0 = seen_param[o.w];
            // dW[ci][co][ky][kx] = sum x[i][j][ci] * dy[2i + ky - 1][2j + kx - 1][co]: the stride-2 wgrad with the roles of x and dy exchanged
            if (G(o.w))
                SG_TRY(wgrad_call(dt, xin, ti.H, ti.W, ti.C, dy, B, to.H, to.W, to.C, 3, 3, 2, 1, 1, lay_fwd(to.C, 3, 3), 1.f, slab, G(o.w), st, nullptr, pacc0));
            if (G(o.bias)) SG_TRY(bias_sum(dy, (long)B * to.H * to.W, to.C, G(o.bias), pacc0));
            seen_param[o.w] = 1;
            SG_REQUIRE(!acc, "%s backward: internal error (transposed convolution input with two consumers)", tag);
            // dx[i][j][ci] = sum dy[2i + ky - 1][2j + kx - 1][co] * W[ci][co][ky][kx]: the forward 3x3 stride-2 pad-1 convolution
            Conv cv(dt, 3, 3, 2);
            cv.in(dy, B, to.H, to.W, to.C).w(wp + o.wd[0]).out(dx, ti.H, ti.W, ti.C).pad(1, 1);
            if (ti.act) { cv.mask(xin, 0); cv.d.mslope = ti.aslope; }
            SG_TRY(cv.run(st));
            written[o.in] = 1;
            break;
        }
        case RD_DECONV4: {
            // dW[ci][co][ky][kx] = sum x[i][j][ci] * dy[2i + ky - 1][2j + kx - 1][co]: the stride-2 wgrad with the roles of x and dy exchanged
            if (G(o.w))
                SG_TRY(wgrad_call(dt, xin, ti.H, ti.W, ti.C, dy, B, to.H, to.W, to.C, 4, 4, 2, 1, 1, lay_fwd(to.C, 4, 4), 1.f, slab, G(o.w), st));
            if (G(o.bias)) SG_TRY(bias_sum(dy, (long)B * to.H * to.W, to.C, G(o.bias), 0));
            SG_REQUIRE(!acc, "%s backward: internal error (transposed convolution input with two consumers)", tag);
            // dx[i][j][ci] = sum dy[2i + ky - 1][2j + kx - 1][co] * W[ci][co][ky][kx]: the forward 4x4 stride-2 pad-1 convolution, masked by
            // the input itself where that is an activation's output (the skip buffer [ReLU | ReLU], the innermost level's ReLU)
            Conv cv(dt, 4, 4, 2);
            cv.in(dy, B, to.H, to.W, to.C < 8 ? to.cs : to.C).w(wp + o.wd[0]).out(dx, ti.H, ti.W, ti.C).pad(1, 1);
            if (ti.act) { cv.mask(xin, 0); cv.d.mslope = ti.aslope; }
            SG_TRY(cv.run(st));
            written[o.in] = 1;
            break;
        }
        case RD_NORM_SKIP:
            // dy = g(out) is the gradient at the norm's output already: the consumer of `out` folded the skip buffer's share in
            SG_REQUIRE(!acc && !ti.act && written[o.skip], "%s backward: internal error (two-output norm)", tag);
            SG_TRY(srcgan_gn_backward(dy.p, to.cs, nullptr, 0, xin.p, ti.cs, nullptr, (const float*)(w8 + o.stats), dx.p, ti.cs, nullptr, 0, 0, nullptr, nullptr, 0,
                                      0.f, B, (long)ti.H * ti.W, ti.C, o.ngrp, dt, gnscr, st));
            written[o.in] = 1;
            break;
        case RD_RELU:           // nothing to launch: the consumer of `in` has folded this buffer's gradient into g(in) (RdT::skip)
            SG_REQUIRE(written[o.in] && P.T[o.in].skip == o.out, "%s backward: internal error (ReLU into a skip buffer without a consumer that folds its gradient)", tag);
            break;
        case RD_ATTN: {
            void* dres = nullptr; int dres_cs = 0, dres_acc = 0;
            if (o.res >= 0) {       // the block's input: this op stores (or adds to the group convolution's copy), the block's first convolution adds
                dres = s8 + P.g[o.res]; dres_cs = P.T[o.res].cs; dres_acc = written[o.res]; written[o.res] = 1;
            }
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (attention input has two consumers or a fused activation)", tag);
            SG_TRY(srcgan_ca_backward(dy.p, to.cs, xin.p, ti.cs, params[o.w], params[o.w + 2], (const float*)(w8 + o.stats), dx.p, ti.cs, dres, dres_cs,
                                      dres_acc, G(o.w), G(o.w + 1), G(o.w + 2), G(o.w + 3), B, (long)ti.H * ti.W, ti.C, o.attn_width, dt, gnscr, st));
            written[o.in] = 1;
            break;
        }
        case RD_MEANSHIFT:
            SG_REQUIRE(!G(o.w) && !G(o.bias), "%s backward: MeanShift is frozen (its gradient pointers must be null)", tag);
            SG_REQUIRE(!acc, "%s backward: internal error (MeanShift input with two consumers)", tag);
            if (need_dx) {
                SG_TRY(sg_meanshift(dy.p, dx.p, params[o.w], nullptr, 1, (long)B * ti.H * ti.W, dt, (hipStream_t)st));
                written[o.in] = 1;
            }
            break;
        case RD_GATHER:         // the gather's adjoint is the crop; a second consumer's contribution is added
            SG_TRY(srcgan_d2s_shift(dy.p, to.cs, dx.p, ti.cs, B, ti.H, ti.W, o.iC, o.scale, o.shift, to.H, to.W, acc, dt, st));
            written[o.in] = 1;
            break;
        case RD_PRELU: {
            void* dres = nullptr; int dres_cs = 0, dres_acc = 0;
            if (o.res >= 0) { dres = s8 + P.g[o.res] + (size_t)o.rcoff * P.esz; dres_cs = P.T[o.res].cs; dres_acc = written[o.res]; written[o.res] = 1; }
            SG_REQUIRE(!acc && !ti.act && o.in != o.res, "%s backward: internal error (PReLU input with two consumers or a fused activation)", tag);
            SG_TRY(srcgan_prelu_backward((char*)dy.p + (size_t)dy.coff * P.esz, to.cs, xin.p, ti.cs, params[o.w], o.bias >= 0 ? params[o.bias] : nullptr, dx.p, ti.cs,
                                         dres, dres_cs, o.beta, dres_acc, G(o.w), G(o.bias), B, to.H, to.W, o.oC, o.scale, o.shift, ti.H, ti.W, dt,
                                         (float*)(s8 + P.prscr), st));
            written[o.in] = 1;
            break;
        }
        case RD_POOL:
            SG_REQUIRE(!acc, "%s backward: internal error (pooled tensor with two consumers)", tag);
            SG_TRY(srcgan_maxpool2_bwd_nhwc(dy.p, to.cs, xin.p, ti.cs, dx.p, ti.cs, B, ti.H, ti.W, ti.C, ti.act && tap_of(o.in) < 0, dt, st));
            written[o.in] = 1;
            break;
        case RD_SHUFFLE:
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (PixelShuffle input)", tag);
            SG_TRY(srcgan_pixel_shuffle_nhwc(dy.p, to.cs, dx.p, ti.cs, B, ti.H, ti.W, to.C, o.k, 1, dt, st));
            written[o.in] = 1;
            break;
        case RD_REFLECT:        // a block's input feeds the pad and the block's closing residual: the second contribution adds
            SG_REQUIRE(!ti.act, "%s backward: internal error (reflection pad of a tensor with a fused activation)", tag);
            if (need_dx) {
                SG_TRY(srcgan_reflect_pad_bwd_nhwc(dy.p, to.cs, dx.p, ti.cs, B, ti.H, ti.W, ti.cs, o.pad, acc, dt, st));
                written[o.in] = 1;
            }
            break;
        case RD_TANH:
            SG_REQUIRE(!acc && !ti.act, "%s backward: internal error (tanh input has two consumers or a fused activation)", tag);
            SG_TRY(srcgan_tanh_backward(dy.p, to.cs, w8 + to.off, to.cs, dx.p, ti.cs, (long)B * ti.H * ti.W, ti.cs, 0, dt, st));
            written[o.in] = 1;
            break;
        case RD_FOLD_TAIL:
            SG_FAIL("%s backward: internal error (a folded tail in a training plan)", tag);
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

// ---- the C entry points of a family, written once.  CFG: the configuration struct; PLAN / IPLAN: its training and inference plan
// functions; TAG: the pack-cache tag stem, also the name in messages (an expression of c, evaluated once the plan stands).  The training
// forward's job table is cached under "<TAG>_fwd", the backward's under "<TAG>_bwd", the inference forward's under "<TAG>_infer_fwd": its packs
// sit at other offsets (no input-gradient packs between them).  An inference forward is rd_forward on the slot-planned workspace: the same
// launches with the same arguments apart from buffer addresses -> the same bits.  Failure: -1 from the int queries, 0 from the sizes.
#define RD_TRAIN_ENTRIES(STEM, CFG, PLAN, TAG) \
    extern "C" int srcgan_##STEM##_num_params(const CFG* c) { RdPlan P; if (PLAN(c, P)) return -1; return P.nparams; } \
    extern "C" size_t srcgan_##STEM##_ws_bytes(const CFG* c) { RdPlan P; if (PLAN(c, P)) return 0; return P.total; } \
    extern "C" size_t srcgan_##STEM##_bwd_scratch_bytes(const CFG* c) { RdPlan P; if (PLAN(c, P)) return 0; return P.bwd_total; } \
    extern "C" int srcgan_##STEM##_forward(const CFG* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) { \
        RdPlan P; \
        SG_TRY(PLAN(c, P)); \
        return rd_forward(P, x_nchw, params, ws, y_nchw, TAG, st); \
    } \
    extern "C" int srcgan_##STEM##_backward(const CFG* c, const float* dy_nchw, const float* const* params, void* ws, void* scratch, \
                                            float* const* grads, float* dx_nchw, void* st) { \
        RdPlan P; \
        SG_TRY(PLAN(c, P)); \
        return rd_backward(P, dy_nchw, dx_nchw, params, ws, scratch, grads, TAG, st); \
    }
#define RD_INFER_ENTRIES(STEM, CFG, IPLAN, TAG) \
    extern "C" size_t srcgan_##STEM##_infer_ws_bytes(const CFG* c) { RdPlan P; if (IPLAN(c, P)) return 0; return P.total; } \
    extern "C" size_t srcgan_##STEM##_infer_act_bytes(const CFG* c) { RdPlan P; if (IPLAN(c, P)) return 0; return P.total - P.wpack; } \
    extern "C" int srcgan_##STEM##_infer_plan(const CFG* c, size_t* ranges, int cap) { \
        RdPlan P; \
        if (IPLAN(c, P)) return -1; \
        return rd_plan_ranges(P, ranges, cap); \
    } \
    extern "C" int srcgan_##STEM##_infer(const CFG* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) { \
        RdPlan P; \
        SG_TRY(IPLAN(c, P)); \
        char tag[32]; snprintf(tag, sizeof(tag), "%s_infer", TAG); \
        return rd_forward(P, x_nchw, params, ws, y_nchw, tag, st); \
    }
#define RD_FAMILY(STEM, CFG, PLAN, IPLAN, TAG) RD_TRAIN_ENTRIES(STEM, CFG, PLAN, TAG) RD_INFER_ENTRIES(STEM, CFG, IPLAN, TAG)

RD_FAMILY(srnet, srcgan_srnet_cfg, sr_plan, sr_infer_plan, sr_tag(c->kind))
RD_FAMILY(rcan, srcgan_rcan_cfg, rcan_plan, rcan_infer_plan, "rcan")
RD_FAMILY(ddbpn, srcgan_ddbpn_cfg, ddbpn_plan, ddbpn_infer_plan, "ddbpn")
RD_FAMILY(rdn, srcgan_rdn_cfg, rdn_plan, rdn_infer_plan, "rdn")
RD_FAMILY(mdsr, srcgan_mdsr_cfg, mdsr_plan, mdsr_infer_plan, mdsr_tag(c->scale_idx))
RD_FAMILY(vdsr, srcgan_vdsr_cfg, vdsr_plan, vdsr_infer_plan, "vdsr")
RD_FAMILY(resnetgen, srcgan_resnetgen_cfg, resnetgen_plan, resnetgen_infer_plan, "resnetgen")
RD_FAMILY(unet, srcgan_unet_cfg, unet_plan, unet_infer_plan, "unet")

// ResDeconv: the inference entry points take fold_tail, and the folded plan's job table has a tag of its own
RD_TRAIN_ENTRIES(resdeconv, srcgan_resdeconv_cfg, rd_plan, "resdeconv")
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

// SRDenseNetA / SRDenseNetB: out_hw beside the regular training entries; of the inference entries only the size and the forward
RD_TRAIN_ENTRIES(srdense, srcgan_srdense_cfg, sd_plan, c->kind ? "srdenseB" : "srdenseA")
extern "C" int srcgan_srdense_out_hw(const srcgan_srdense_cfg* c, int* oh, int* ow) {
    RdPlan P;
    SG_TRY(sd_plan(c, P));
    SG_REQUIRE(oh && ow, "srcgan_srdense_out_hw: null pointer");
    *oh = P.T.back().H; *ow = P.T.back().W;
    return 0;
}
extern "C" size_t srcgan_srdense_infer_ws_bytes(const srcgan_srdense_cfg* c) { RdPlan P; if (sd_infer_plan(c, P)) return 0; return P.total; }
extern "C" int srcgan_srdense_infer(const srcgan_srdense_cfg* c, const float* x_nchw, const float* const* params, void* ws, float* y_nchw, void* st) {
    RdPlan P;
    SG_TRY(sd_infer_plan(c, P));
    return rd_forward(P, x_nchw, params, ws, y_nchw, c->kind ? "srdenseB_infer" : "srdenseA_infer", st);
}
#undef RD_FAMILY
#undef RD_INFER_ENTRIES
#undef RD_TRAIN_ENTRIES

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
    nb.finish();
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
