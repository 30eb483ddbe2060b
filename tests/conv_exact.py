"""Operands and float64 references for the direct tests of the convolution and weight-gradient kernels
(tests/test_gpu_conv_exact.py on the GPU, tests/test_conv_exact_teeth.py on the CPU).  No kernel runs here.

Exact part.  x and w are ternary {-1, 0, 1} (x: density 1/2; w: density min(1/2, 864 / K), K = Cin kh kw), bias, residuals and
incoming gradients are integers in [-4, 4], every scale is 1, 1/2 or 1/4.  Every product and every partial sum of the contraction
is then an integer far below 2^24, so ANY order of f32 summation -- any MFMA shape, K split, slab order or tile walk -- gives the same
bits, and one missing, doubled or misplaced term moves the accumulator by at least 1.  The reference is a float64 convolution, the
epilogue as include/srcgan_amd.h states it for srcgan_conv_desc, cast ONCE to the storage type (round to nearest even, as the
kernels' stores do).  The builders assert, on the reference alone, the conditions that make the comparison an exact one
(check_exact); a case that breaks one is a mistake in the case table.

Float64 part.  Random reals rounded to the storage type, the reference's production constants, and a per-element bound
    |out - ref64| <= eps_T |ref64| + (K + 8) 2^-23 N,      N = the float64 sum of the absolute terms of the expression.

All tensors a builder returns are float64 and hold values the three storage types represent exactly (exact part) or values already
rounded to the case's type (float64 part); buffers are logical NHWC [B, H, W, cs]."""
import math
import zlib

import torch
import torch.nn.functional as F

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTS = ("fp32", "bf16", "fp16")
DT_TAG = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}
PREC = {"fp32": 24, "bf16": 8, "fp16": 11}              # significant bits
EPS = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SENTINEL = 1000.0                                        # exact in all three types
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))


def gen(name):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(name.encode()))
    return g


def ternary(shape, p, g):
    nz = torch.rand(shape, generator=g) < p
    sg = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (nz * sg).double()


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def w_density(K):
    return min(0.5, 864.0 / K)


def rounded(t, dt):
    return t.to(TDT[dt]).double()


def reals(shape, g, dt, scale=1.0, centred=True):
    t = torch.rand(shape, generator=g, dtype=torch.float64)
    return rounded((t - 0.5 if centred else t) * scale, dt)


def nchw(buf, c0, c):
    return buf[..., c0:c0 + c].permute(0, 3, 1, 2)


def conv_ref(x, w, stride, pad, OH, OW):
    """out[b, co, oy, ox] = sum x[b, ci, oy s + ky - pad_y, ox s + kx - pad_x] w[co, ci, ky, kx], zero outside x: the forward form of
    srcgan_conv_igemm with an explicit output extent (the parity forms pass extents F.conv2d's symmetric padding does not give)."""
    kh, kw = w.shape[2:]
    H, W = x.shape[2:]
    need_h, need_w = (OH - 1) * stride + kh, (OW - 1) * stride + kw
    xp = F.pad(x, (pad[1], max(0, need_w - W - pad[1]), pad[0], max(0, need_h - H - pad[0])))
    return F.conv2d(xp, w, None, stride)[:, :, :OH, :OW]


def epilogue(conv, bias=None, alpha=1.0, r1=None, beta1=0.0, r1_cend=0, r2=None, beta2=0.0, r2_cend=0, act=False, slope=0.0,
             mz=None, mz_c0=0, mslope=0.0, gt_act=torch.gt, gt_mz=torch.gt, absconv=None):
    """srcgan_conv_desc's expression in float64 on [B, Cout, OH, OW] operands (r1 / r2: their first *_cend channels).
    -> (v before the activation, v, N): N = the sum of the absolute terms carried through the same factors (absconv given).
    gt_act / gt_mz: the comparisons, replaceable by the teeth tests."""
    v = conv if bias is None else conv + bias.view(1, -1, 1, 1)
    v = alpha * v
    n = None
    if absconv is not None:
        n = abs(alpha) * (absconv if bias is None else absconv + bias.abs().view(1, -1, 1, 1))
    for r, beta, cend in ((r1, beta1, r1_cend), (r2, beta2, r2_cend)):
        if r is not None and cend > 0:
            v = v.clone()
            v[:, :cend] += beta * r[:, :cend]
            if n is not None:
                n = n.clone()
                n[:, :cend] += (beta * r[:, :cend]).abs()
    pre = v
    fac = torch.ones_like(v)
    if act:
        fac = torch.where(gt_act(v, 0), fac, fac * slope)
        v = torch.where(gt_act(v, 0), v, v * slope)
    if mz is not None:
        f = torch.where(gt_mz(mz, 0), torch.ones_like(mz), torch.full_like(mz, mslope))
        f[:, :mz_c0] = 1.0
        v = v * f
        fac = fac * f
    return pre, v, (n * fac.abs() if n is not None else None)


def ulp(m, dt):
    return 2.0 ** (math.floor(math.log2(m)) - (PREC[dt] - 1)) if m > 0 else 0.0


def check_exact(name, dt, bound, pre, v, alpha, f32_out=False):
    """The conditions under which bit equality is the right assertion; evaluated on the reference alone."""
    assert float(bound.max()) < 2.0 ** 24, (name, "a partial sum may leave the exact integers", float(bound.max()))
    for t in (pre, v):
        assert torch.equal(t.float().double(), t), (name, "v is not an f32 number")
    m = float(pre.abs().max())
    u = ulp(m, "fp32" if f32_out else dt)
    assert abs(alpha) >= u, (name, dt, f"one unit of the accumulator ({alpha}) is below one ulp ({u}) at max |v| = {m}")


# ---------------------------------------------------------------------------------------------------------------- srcgan_conv_igemm
CONV_DEFAULTS = dict(k=(3, 3), s=1, pad=(1, 1), cin=64, cout=32, hw=(5, 7), B=2, dts=DTS, blocked=False, x_coff=0, x_cs=None, y_in_x=False,
                     y_coff=0, y_cs=None, y_extra=(0, 0), os=1, oa=0, ob=0, OHW=None, bias=True, alpha=1.0, act=False, slope=0.25,
                     r1=None, beta1=0.5, r1_cend=None, r1_coff=None, r1_cs=None, r2=False, beta2=0.25, r2_cend=None, mz=False, mz_c0=0,
                     mz_coff=0, mz_cs=None, mslope=0.5, sign_out=False, sign_in=False, rev=0, real=False, y_blocked=False, ep_blocked=False)


def conv_case(name, **kw):
    bad = set(kw) - set(CONV_DEFAULTS)
    assert not bad, bad
    c = dict(CONV_DEFAULTS, name=name, form="conv")
    c.update(kw)
    return c


PERSISTENT = "units > 2 CUs + 3"


def persistent_batch(ncu, tiles_per_image=9):
    """images so that the 3x3 kernel's work units exceed 2 * CUs + 3: more than two units per workgroup, so every workgroup loops
    and, with the units split evenly over the 8 XCDs, some workgroups of each XCD take a third trip"""
    return (2 * ncu + 3) // tiles_per_image + 1


def build_conv(c, dt="fp32", ncu=256):
    """-> dict of float64 tensors: the operand buffers, the initial y buffer, and `want`, the whole y buffer after the call."""
    g = gen(c["name"])
    real = c["real"]
    (kh, kw), s, pad = c["k"], c["s"], c["pad"]
    B = persistent_batch(ncu) if c["B"] == PERSISTENT else c["B"]
    (H, W), cin, cout = c["hw"], c["cin"], c["cout"]
    OH, OW = c["OHW"] or ((H + 2 * pad[0] - kh) // s + 1, (W + 2 * pad[1] - kw) // s + 1)
    os_, oa, ob = c["os"], c["oa"], c["ob"]
    YH, YW = OH * os_ + c["y_extra"][0], OW * os_ + c["y_extra"][1]
    x_coff = c["x_coff"]
    x_cs = c["x_cs"] or x_coff + cin
    y_coff = c["y_coff"]
    y_cs = x_cs if c["y_in_x"] else (c["y_cs"] or y_coff + cout)
    rnd = (lambda shape, sc=1.0: reals(shape, g, dt, sc)) if real else None
    xbuf = rnd((B, H, W, x_cs)) if real else ternary((B, H, W, x_cs), 0.5, g)
    K = cin * kh * kw
    w = rounded(torch.randn((cout, cin, kh, kw), generator=g, dtype=torch.float64) * 0.1, dt) if real else ternary((cout, cin, kh, kw), w_density(K), g)
    bias = None
    if c["bias"]:
        bias = torch.randn(cout, generator=g, dtype=torch.float64).float().double() * 0.1 if real else ints((cout,), -4, 4, g)
    res = (lambda shape: rnd(shape)) if real else (lambda shape: ints(shape, -4, 4, g))
    if c["y_in_x"]:
        assert (YH, YW) == (H, W)
        y0 = xbuf
    else:
        y0 = torch.full((B, YH, YW, y_cs), SENTINEL, dtype=torch.float64)
    lat = lambda buf: buf[:, oa::os_, ob::os_][:, :OH, :OW]
    out = dict(case=c, B=B, H=H, W=W, OH=OH, OW=OW, YH=YH, YW=YW, x_cs=x_cs, y_cs=y_cs, x=xbuf, w=w, bias=bias, y0=y0)
    ep = dict(bias=bias, alpha=F32(c["alpha"]), act=c["act"], slope=F32(c["slope"]), mslope=F32(c["mslope"]))
    if c["r1"]:
        cend = c["r1_cend"] or cout
        if c["r1"] == "y":
            r1_coff = y_coff if c["r1_coff"] is None else c["r1_coff"]
            if not c["y_in_x"]:
                lat(y0)[..., r1_coff:r1_coff + cend] = res((B, OH, OW, cend))
            r1buf, r1_cs = y0, y_cs
        elif c["r1"] == "x":                  # the residual is a channel slice of the input buffer (conv5 of a dense block)
            assert (YH, YW) == (H, W)
            r1buf, r1_cs, r1_coff = xbuf, x_cs, c["r1_coff"] or 0
        else:
            r1_coff = c["r1_coff"] or 0
            r1_cs = c["r1_cs"] or r1_coff + cend
            r1buf = res((B, YH, YW, r1_cs))
        out.update(r1=r1buf, r1_cs=r1_cs, r1_coff=r1_coff, r1_cend=cend)
        ep.update(r1=nchw(lat(r1buf), r1_coff, cend), beta1=F32(c["beta1"]), r1_cend=cend)
    if c["r2"]:
        cend = c["r2_cend"] or cout
        r2buf = res((B, YH, YW, cend))
        out.update(r2=r2buf, r2_cend=cend)
        ep.update(r2=nchw(lat(r2buf), 0, cend), beta2=F32(c["beta2"]), r2_cend=cend)
    if c["mz"] or c["sign_in"]:
        mz_coff = c["mz_coff"]
        mz_cs = c["mz_cs"] or mz_coff + cout
        mzbuf = rnd((B, YH, YW, mz_cs)) if real else ints((B, YH, YW, mz_cs), -2, 2, g)
        out.update(mz=mzbuf, mz_cs=mz_cs)
        ep.update(mz=nchw(lat(mzbuf), mz_coff, cout), mz_c0=c["mz_c0"])
    xin = nchw(xbuf, x_coff, cin)
    conv = conv_ref(xin, w, s, pad, OH, OW)
    absconv = conv_ref(xin.abs(), w.abs(), s, pad, OH, OW)
    pre, v, n = epilogue(conv, absconv=absconv, **ep)
    want = y0.clone()
    lat(want)[..., y_coff:y_coff + cout] = v.permute(0, 2, 3, 1)
    out.update(conv=conv, ep=ep, pre=pre, v=v, N=n, want=want, K=K, bound=absconv + (bias.abs().view(1, -1, 1, 1) if bias is not None else 0.0))
    return out


def pack_sign32(bits):
    """bool [B, 32, OH, OW] -> int32 [B, OH, OW], bit c = channel c"""
    wgt = (2 ** torch.arange(32, dtype=torch.int64)).view(1, 32, 1, 1)
    word = (bits.to(torch.int64) * wgt).sum(1)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)


def unpack_sign32(word, C=32):
    return ((word.to(torch.int64).unsqueeze(1) >> torch.arange(C, dtype=torch.int64, device=word.device).view(1, C, 1, 1)) & 1).bool()


def pack_sign8(bits):
    """bool [B, C, OH, OW] -> uint8 [B, OH, OW, C / 8]: byte c / 8, bit c % 8"""
    B, C, H, W = bits.shape
    b = bits.permute(0, 2, 3, 1).reshape(B, H, W, C // 8, 8).to(torch.int64)
    return (b * (2 ** torch.arange(8, dtype=torch.int64))).sum(-1).to(torch.uint8)


def unpack_sign8(mask):
    """uint8 [B, H, W, C / 8] -> bool [B, C, H, W]"""
    B, H, W, n = mask.shape
    bits = ((mask.to(torch.int64).unsqueeze(-1) >> torch.arange(8, dtype=torch.int64, device=mask.device)) & 1).bool()
    return bits.reshape(B, H, W, n * 8).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------- four parities in one launch
def par_case(name, form, **kw):
    d = dict(name=name, form=form, cin=64, cout=64, hw=(5, 7), B=2, dts=DTS, bias=False, alpha=1.0, act=False, slope=0.25, mz=False,
             mslope=0.5, r1=False, beta1=0.5, sign_out=False, y_cs=None, real=False)
    bad = set(kw) - set(d)
    assert not bad, bad
    d.update(kw)
    return d


def build_par(c, dt="fp32"):
    """up1x1: ConvTranspose2d(k2, s2) (+ LeakyReLU) of x [B, cin, H, W], w [cin, cout, 2, 2]       (rddb.py:28-38)
    par4:   input gradient of Conv2d(cin -> cout, 4x4, s2, p1) at input extent H x W, by float64 autograd (model/model.py:612-634)
    deconv3: ConvTranspose2d(cin -> cout, k3, s2, p1, output_padding 1) + bias + ReLU               (model/model.py:698-701)"""
    g = gen(c["name"])
    real, form = c["real"], c["form"]
    B, (H, W), cin, cout = c["B"], c["hw"], c["cin"], c["cout"]
    rnd = lambda shape, sc=1.0: reals(shape, g, dt, sc)
    tern = lambda shape, p: rnd(shape) if real else ternary(shape, p, g)
    wmk = lambda shape, K: rounded(torch.randn(shape, generator=g, dtype=torch.float64) * 0.1, dt) if real else ternary(shape, w_density(K), g)
    out = dict(case=c, B=B)
    ep = dict(alpha=F32(c["alpha"]), act=c["act"], slope=F32(c["slope"]), mslope=F32(c["mslope"]))
    if form == "up1x1":
        x, w = tern((B, cin, H, W), 0.5), wmk((cin, cout, 2, 2), cin)
        conv, absconv = F.conv_transpose2d(x, w, None, 2, 0), F.conv_transpose2d(x.abs(), w.abs(), None, 2, 0)
        K = cin
    elif form == "par4":
        oh, ow = (H - 2) // 2 + 1, (W - 2) // 2 + 1
        x, w = (rnd((B, cout, oh, ow)) if real else ints((B, cout, oh, ow), -4, 4, g)), wmk((cout, cin, 4, 4), 4 * cout)      # x = dy
        def dgrad(dy, wt):
            z = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
            F.conv2d(z, wt, None, 2, 1).backward(dy)
            return z.grad
        conv, absconv = dgrad(x, w), dgrad(x.abs(), w.abs())
        K = 4 * cout
    else:
        x, w = tern((B, cin, H, W), 0.5), wmk((cin, cout, 3, 3), 4 * cin)
        conv = F.conv_transpose2d(x, w, None, 2, 1, output_padding=1)
        absconv = F.conv_transpose2d(x.abs(), w.abs(), None, 2, 1, output_padding=1)
        K = 4 * cin
    YH, YW = conv.shape[2:]
    Cy = conv.shape[1]
    if c["bias"]:
        ep["bias"] = torch.randn(Cy, generator=g, dtype=torch.float64).float().double() * 0.1 if real else ints((Cy,), -4, 4, g)
    y_cs = c["y_cs"] or Cy
    y0 = torch.full((B, YH, YW, y_cs), SENTINEL, dtype=torch.float64)
    if c["r1"]:
        r1 = rnd((B, YH, YW, Cy)) if real else ints((B, YH, YW, Cy), -4, 4, g)
        out["r1"] = r1
        ep.update(r1=r1.permute(0, 3, 1, 2), beta1=F32(c["beta1"]), r1_cend=Cy)
    if c["mz"]:
        mz = rnd((B, YH, YW, Cy)) if real else ints((B, YH, YW, Cy), -2, 2, g)
        out["mz"] = mz
        ep.update(mz=mz.permute(0, 3, 1, 2), mz_c0=0)
    pre, v, n = epilogue(conv, absconv=absconv, **ep)
    want = y0.clone()
    want[..., :Cy] = v.permute(0, 2, 3, 1)
    bound = absconv + (ep["bias"].abs().view(1, -1, 1, 1) if c["bias"] else 0.0)
    out.update(x=x.permute(0, 2, 3, 1).contiguous(), w=w, bias=ep.get("bias"), y0=y0, want=want, conv=conv, ep=ep, pre=pre, v=v, N=n, K=K, bound=bound,
               YH=YH, YW=YW, y_cs=y_cs, Cy=Cy)
    return out


def swap_parities(buf, p, q):
    """NHWC buffer with the output parities p = (a, b) and q swapped (the extents of the two sub-lattices must agree)"""
    out = buf.clone()
    out[:, p[0]::2, p[1]::2] = buf[:, q[0]::2, q[1]::2]
    out[:, q[0]::2, q[1]::2] = buf[:, p[0]::2, p[1]::2]
    return out


# ---------------------------------------------------------------------------------------------------------------- srcgan_conv_wgrad
def wgrad_case(name, **kw):
    d = dict(name=name, form="wgrad", k=(3, 3), s=1, pad=(1, 1), cin=32, cout=32, hw=(9, 33), B=2, dts=DTS, x_cs=None, x_coff=0, dy_cs=None,
             dy_coff=0, nsplit=None, accumulate=False, alpha=1.0, bias_grad=False, layout="canonical", real=False)
    bad = set(kw) - set(d)
    assert not bad, bad
    d.update(kw)
    return d


def wgrad_ref(x, dy, cout, cin, k, s, pad):
    """dW[co, ci, ky, kx] = sum_{b, oy, ox} dy[b, co, oy, ox] x[b, ci, oy s + ky - pad, ox s + kx - pad], by float64 autograd"""
    w = torch.zeros(cout, cin, k[0], k[1], dtype=torch.float64, requires_grad=True)
    OH, OW = dy.shape[2:]
    conv_ref(x, w, s, pad, OH, OW).backward(dy)
    return w.grad


def build_wgrad(c, dt="fp32"):
    g = gen(c["name"])
    real = c["real"]
    k, s, pad, B, (H, W), cin, cout = c["k"], c["s"], c["pad"], c["B"], c["hw"], c["cin"], c["cout"]
    OH, OW = (H + 2 * pad[0] - k[0]) // s + 1, (W + 2 * pad[1] - k[1]) // s + 1
    epp = 8
    x_cs = c["x_cs"] or c["x_coff"] + -(-cin // epp) * epp
    dy_cs = c["dy_cs"] or c["dy_coff"] + -(-cout // epp) * epp
    xbuf = reals((B, H, W, x_cs), g, dt) if real else ternary((B, H, W, x_cs), 0.5, g)
    dybuf = reals((B, OH, OW, dy_cs), g, dt) if real else ints((B, OH, OW, dy_cs), -4, 4, g)
    # the kernels fetch channels in 16-byte pieces: the tensors own ZERO padding behind the true channel counts
    xbuf[..., c["x_coff"] + cin:c["x_coff"] + -(-cin // epp) * epp] = 0
    dybuf[..., c["dy_coff"] + cout:c["dy_coff"] + -(-cout // epp) * epp] = 0
    x, dy = nchw(xbuf, c["x_coff"], cin), nchw(dybuf, c["dy_coff"], cout)
    alpha = F32(c["alpha"])
    gw = wgrad_ref(x, dy, cout, cin, k, s, pad)
    gabs = wgrad_ref(x.abs(), dy.abs(), cout, cin, k, s, pad)
    n = k[0] * k[1]
    if c["layout"] == "canonical":            # [Cout, Cin, kh, kw]
        lay, shape, perm = (cin * n, n, k[1], 1, 0), (cout, cin, k[0], k[1]), None
    else:                                     # "transposed": [Cin, Cout, kh, kw] (a ConvTranspose2d weight), 5 elements into a larger buffer
        lay, shape, perm = (n, cout * n, k[1], 1, 5), (cin, cout, k[0], k[1]), (1, 0, 2, 3)
    numel = cout * cin * n + lay[4] + (3 if lay[4] else 0)
    g0 = (ints((numel,), -4, 4, g) if c["accumulate"] else torch.full((numel,), SENTINEL, dtype=torch.float64))
    val = alpha * (gw.permute(*perm) if perm else gw)
    want = g0.clone()
    body = want[lay[4]:lay[4] + cout * cin * n].view(shape)
    body.copy_(body + val if c["accumulate"] else val)
    out = dict(case=c, x=xbuf, dy=dybuf, grad0=g0, want=want, layout=lay, OH=OH, OW=OW, N=abs(alpha) * gabs, val=val, K=B * OH * OW, perm=perm,
               shape=shape, off=lay[4], bound=gabs)
    if c["bias_grad"]:                        # follows `accumulate` like the weight gradient
        b0 = ints((cout,), -4, 4, g) if c["accumulate"] else torch.full((cout,), SENTINEL, dtype=torch.float64)
        out["bias0"] = b0
        out["bias_want"] = alpha * dy.sum((0, 2, 3)) + (b0 if c["accumulate"] else 0.0)
        out["bias_N"] = abs(alpha) * dy.abs().sum((0, 2, 3))
    return out


# --------------------------------------------------------------------------------------------------------------- srcgan_wgrad_dense
def dense_case(name, **kw):
    d = dict(name=name, form="dense", nf=64, gc=32, hw=(8, 32), B=2, dts=DTS, blocked=False, accumulate=False, no_grad=None, no_bias=None,
             segs=None, real=False)
    bad = set(kw) - set(d)
    assert not bad, bad
    d.update(kw)
    return d


def dense_segments(nf, gc):
    """(g0, co, cin, alpha) of conv5 .. conv1 of a ResidualDenseBlock_5 in its gradient buffer [dy5 (nf) | dy4 | dy3 | dy2 | dy1]"""
    return [(0 if m == 5 else nf + (4 - m) * gc, nf if m == 5 else gc, nf + (m - 1) * gc, 0.5 if m == 5 else 1.0) for m in (5, 4, 3, 2, 1)]


def build_dense(c, dt="fp32"):
    g = gen(c["name"])
    real = c["real"]
    B, (H, W) = c["B"], c["hw"]
    segs = c["segs"] or dense_segments(c["nf"], c["gc"])
    Cc = max(cin for _, _, cin, _ in segs)
    G = max(g0 + co for g0, co, _, _ in segs)
    A = reals((B, H, W, Cc), g, dt) if real else ternary((B, H, W, Cc), 0.5, g)
    Gd = reals((B, H, W, G), g, dt) if real else ints((B, H, W, G), -4, 4, g)
    out = dict(case=c, A=A, Gd=Gd, G=G, C=Cc, segs=[], K=B * H * W)
    for i, (g0, co, cin, alpha) in enumerate(segs):
        if real:
            alpha = F32(0.2) if alpha != 1.0 else 1.0
        x, dy = nchw(A, 0, cin), nchw(Gd, g0, co)
        gw = alpha * wgrad_ref(x, dy, co, cin, (3, 3), 1, (1, 1))
        gn = alpha * wgrad_ref(x.abs(), dy.abs(), co, cin, (3, 3), 1, (1, 1))
        gb, gbn = alpha * dy.sum((0, 2, 3)), alpha * dy.abs().sum((0, 2, 3))
        w0 = ints(gw.shape, -4, 4, g) if c["accumulate"] else torch.full(gw.shape, SENTINEL, dtype=torch.float64)
        b0 = ints(gb.shape, -4, 4, g) if c["accumulate"] else torch.full(gb.shape, SENTINEL, dtype=torch.float64)
        has_w, has_b = i != c["no_grad"], i != c["no_bias"]
        out["segs"].append(dict(g0=g0, g1=g0 + co, cin=cin, alpha=alpha, w0=w0 if has_w else None, b0=b0 if has_b else None,
                                w_want=(w0 + gw if c["accumulate"] else gw) if has_w else None,
                                b_want=(b0 + gb if c["accumulate"] else gb) if has_b else None, w_N=gn, b_N=gbn))
    return out


def bound64(ref, N, K, dt, f32_out=False):
    """the per-element bound of the float64 part"""
    return (0.0 if f32_out else EPS[dt]) * ref.abs() + (K + 8) * 2.0 ** -23 * N
