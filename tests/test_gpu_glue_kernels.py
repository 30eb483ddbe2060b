"""Direct parity tests, through the C ABI, of the element-wise and reduction kernels of csrc/elementwise.hip that hold the
networks together: the column reductions (modes 0, 1, 2), the BatchNorm pieces, the residual join, the x2 nearest
up-sampling and its adjoint, PixelShuffle and the activation mask.

Every assertion is one of two kinds:
  * EXACT -- the output has the bits of a reference: integer-valued inputs whose sums are exact in f32 in any order (the
    reductions), one f32 expression rounded once (the residual join, the mask), or plain data movement;
  * ELEMENT-WISE -- |out - ref| <= eps_T * N for EVERY element, ref in float64 from the quantised inputs, N the float64 sum of
    the absolute values of the expression's terms, eps_T = 2^-8 (bf16), 2^-11 (fp16), 2^-20 (f32): one output rounding (at most
    2^-8, 2^-11, 2^-24 of |out| <= N, and less than that by the factor 1 + 2^-p) plus a handful of f32 operations (2^-24 N each).  No measure is normalised by a tensor's maximum.
The references are written over (buffer, channel stride, channel offset, plane stride), so that the CPU test
tests/test_glue_kernels_teeth.py can show that they tell a dropped pixel, a channel offset shifted by 4 and a plane index
off by one from the right answer.  Each tolerance test prints its measured maximum ("[glue] ..." lines, pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTS = ["fp32", "bf16", "fp16"]
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
EPS_T = {"fp32": 2.0 ** -20, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
EPP = {"fp32": 4, "bf16": 8, "fp16": 8}
U32 = 2.0 ** -24          # unit round-off of f32
SENT = 1000.0             # sentinel outside every slice: exact in all three types, far from any datum
SLOPE = 0.2


# --------------------------------------------------------------------------- helpers shared with the CPU teeth test
def chan_index(npix, cs, coff, C, plane_bytes, esz, device):
    """Flat element offsets [npix, C] of channels [coff, coff + C): interleaved records of cs elements (plane_bytes == 0) or the
    blocked layout [plane][pixel][64 bytes] with the plane stride in bytes."""
    p = torch.arange(npix, device=device).unsqueeze(1)
    c = coff + torch.arange(C, device=device).unsqueeze(0)
    if plane_bytes == 0:
        return p * cs + c
    kce = 64 // esz
    return p * kce + (c // kce) * (plane_bytes // esz) + c % kce


def take(buf, npix, cs, coff, C, plane_bytes=0):
    return buf.reshape(-1)[chan_index(npix, cs, coff, C, plane_bytes, buf.element_size(), buf.device)]


def put(buf, val, npix, cs, coff, C, plane_bytes=0):
    """A copy of buf with the slice replaced: what an in-place kernel must leave behind, everything else untouched."""
    out = buf.clone()
    out.reshape(-1)[chan_index(npix, cs, coff, C, plane_bytes, buf.element_size(), buf.device)] = val.to(buf.dtype)
    return out


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def slice_buffer(vals, cs, coff, misalign=0):
    """[npix, C] values as channels [coff, coff + C) of an interleaved buffer of stride cs filled with the sentinel; misalign
    moves the base pointer by that many elements."""
    npix, C = vals.shape
    flat = torch.full((npix * cs + misalign,), SENT, dtype=vals.dtype, device=vals.device)
    b = flat[misalign:]
    b.view(npix, cs)[:, coff:coff + C] = vals
    return b


def reduce_case(kind, npix, C, tdt, device, a_cs=None, a_coff=0, z_cs=None, z_coff=0, misalign=0):
    """Operands of a column reduction.  kind 'int': a, z integers in [-4, 4], mean an integer in [-2, 2], rstd in {0.5, 1, 2}:
    every term |a|, (a - mean)^2 <= 36, |a (z - mean) rstd| <= 48 is a multiple of 0.5 and every partial sum stays below
    64 * 131073 < 2^23, so any f32 summation order is exact.  kind 'normal': random normal data around 0.3."""
    a_cs, z_cs = a_cs or C, z_cs or C
    if kind == "int":
        av = torch.randint(-4, 5, (npix, C), device=device).to(tdt)
        zv = torch.randint(-4, 5, (npix, C), device=device).to(tdt)
        mean = torch.randint(-2, 3, (C,), device=device).float()
        rstd = 2.0 ** torch.randint(-1, 2, (C,), device=device).float()
    else:
        av = (torch.randn(npix, C, device=device) * 1.5 + 0.3).to(tdt)
        zv = (torch.randn(npix, C, device=device) * 1.5 + 0.3).to(tdt)
        mean = 0.3 + 0.1 * torch.randn(C, device=device)
        rstd = (1.0 + 0.1 * torch.rand(C, device=device)) / 1.5
    return dict(a=slice_buffer(av, a_cs, a_coff, misalign), a_cs=a_cs, a_coff=a_coff,
                z=slice_buffer(zv, z_cs, z_coff, misalign), z_cs=z_cs, z_coff=z_coff, mean=mean, rstd=rstd, npix=npix, C=C)


def ref_col_reduce(mode, k, scale, npix=None, a_coff=None, z_coff=None):
    """float64 results and the float64 sums of the absolute terms of srcgan_col_reduce modes 0, 1, 2 (npix / a_coff / z_coff
    override the case's own: the teeth test's perturbations)."""
    npix = k["npix"] if npix is None else npix
    a_coff = k["a_coff"] if a_coff is None else a_coff
    z_coff = k["z_coff"] if z_coff is None else z_coff
    av = take(k["a"], npix, k["a_cs"], a_coff, k["C"]).double()
    if mode == 0:
        terms = [av]
    elif mode == 1:
        terms = [(av - k["mean"].double()) ** 2]
    else:
        zv = take(k["z"], npix, k["z_cs"], z_coff, k["C"]).double()
        terms = [av, av * (zv - k["mean"].double()) * k["rstd"].double()]
    return [t.sum(0) * scale for t in terms], [t.abs().sum(0) * scale for t in terms]


def lrelu_factor(mz, slope):
    """LeakyReLU'(mz) as the kernels take it: 1 where mz > 0, slope elsewhere (so at +0.0 and -0.0 too), in f32"""
    return torch.where(mz.float() > 0, torch.ones((), device=mz.device), torch.full((), slope, device=mz.device))


def ref_add_inplace(y, ys, x, xs, mz, ms, slope, npix, C):
    """What srcgan_add_inplace(_planes) leaves in y's buffer: (y + x) [* LeakyReLU'(mz)] as one f32 expression, cast once.
    ys / xs / ms = (cs, coff, plane stride in bytes)."""
    r = take(y, npix, ys[0], ys[1], C, ys[2]).float() + take(x, npix, xs[0], xs[1], C, xs[2]).float()
    if mz is not None:
        r = r * lrelu_factor(take(mz, npix, ms[0], ms[1], C, ms[2]), slope)
    return put(y, r, npix, ys[0], ys[1], C, ys[2])


def ref_upsample2(src, s_cs, s_coff, s_plane, dst, d_cs, B, H, W, C):
    v = take(src, B * H * W, s_cs, s_coff, C, s_plane).float().view(B, H, W, C).permute(0, 3, 1, 2)
    up = F.interpolate(v, scale_factor=2, mode="nearest").permute(0, 2, 3, 1).reshape(B * 4 * H * W, C)
    return put(dst, up, B * 4 * H * W, d_cs, 0, C)


def ref_sum2x2(src, s_cs, mz, m_cs, slope, B, H, W, C):
    """float64 result [B*H*W, C] and the float64 sum of the four absolute terms (both times LeakyReLU'(mz)); src and mz are the
    buffers at the slice's first channel"""
    v = take(src, B * 4 * H * W, s_cs, 0, C).double().view(B, 2 * H, 2 * W, C).permute(0, 3, 1, 2)
    s = (F.avg_pool2d(v, 2) * 4).permute(0, 2, 3, 1).reshape(B * H * W, C)
    n = (F.avg_pool2d(v.abs(), 2) * 4).permute(0, 2, 3, 1).reshape(B * H * W, C)
    if mz is not None:
        f = lrelu_factor(take(mz, B * H * W, m_cs, 0, C), slope).double()
        s, n = s * f, n * f
    return s, n


def ref_pixel_shuffle(src, s_cs, dst, d_cs, B, H, W, C, r, inverse):
    if inverse:
        v = take(src, B * H * r * W * r, s_cs, 0, C).float().view(B, H * r, W * r, C).permute(0, 3, 1, 2)
        o = F.pixel_unshuffle(v, r).permute(0, 2, 3, 1).reshape(B * H * W, C * r * r)
        return put(dst, o, B * H * W, d_cs, 0, C * r * r)
    v = take(src, B * H * W, s_cs, 0, C * r * r).float().view(B, H, W, C * r * r).permute(0, 3, 1, 2)
    o = F.pixel_shuffle(v, r).permute(0, 2, 3, 1).reshape(B * H * r * W * r, C)
    return put(dst, o, B * H * r * W * r, d_cs, 0, C)


def ref_mask(g, act, slope, n=None):
    n = g.numel() if n is None else n
    out = g.clone()
    gf = g[:n].float()
    out[:n] = torch.where(act[:n].float() > 0, gf, gf * torch.full((), slope, device=g.device)).to(g.dtype)
    return out


def plant_zeros(v):
    """+0.0, -0.0, a small negative and a small positive value at every 7th element of a value tensor, in turn"""
    f = v.view(-1)
    for i, x in enumerate((0.0, -0.0, -2.0 ** -14, 2.0 ** -14)):
        f[i::7] = x
    return v


def operand(vals, Ctot, coff, blocked):
    """[B,H,W,C] values as channels [coff, coff + C) of a Ctot-channel tensor (sentinel elsewhere), interleaved NHWC or blocked
    (ops.make_blocked).  Returns (buffer, (cs, coff, plane stride in bytes))."""
    from srcgan_amd import ops
    B, H, W, C = vals.shape
    full = torch.full((B, H, W, Ctot), SENT, dtype=vals.dtype, device=vals.device)
    full[..., coff:coff + C] = vals
    if not blocked:
        return full, (Ctot, coff, 0)
    buf, plane = ops.make_blocked(full)
    return buf.contiguous(), (64 // vals.element_size(), coff, plane)


# --------------------------------------------------------------------------- the library
class Lib:
    def __init__(self):
        from srcgan_amd import _native as N
        self.N, self.lib = N, N.lib()

    def st(self):
        return self.N.stream_ptr(torch.device("cuda"))

    def col_reduce(self, mode, k, scale):
        """out0 [, out1] of length C; the 8 floats behind each output, and out1 in modes 0 and 1, must stay untouched"""
        C, npix, dev = k["C"], k["npix"], k["a"].device
        out0, out1 = torch.full((C + 8,), SENT, device=dev), torch.full((C + 8,), SENT, device=dev)
        scr = torch.empty(2 * self.lib.srcgan_col_reduce_blocks(npix) * C, dtype=torch.float32, device=dev)
        self.N.check(self.lib.srcgan_col_reduce(mode, k["a"].data_ptr(), k["a_cs"], k["a_coff"], k["z"].data_ptr() if mode == 2 else None,
                                                k["z_cs"], k["z_coff"], k["mean"].data_ptr() if mode >= 1 else None,
                                                k["rstd"].data_ptr() if mode == 2 else None, npix, C, scale, out0.data_ptr(),
                                                out1.data_ptr() if mode == 2 else None, scr.data_ptr(), self.N.dtype_id(k["a"].dtype), self.st()),
                     "srcgan_col_reduce")
        assert bool((out0[C:] == SENT).all()) and bool((out1[C if mode == 2 else 0:] == SENT).all()), "wrote past its C channels"
        return [out0[:C], out1[:C]][:2 if mode == 2 else 1]

    def mean_var(self, a, npix, C):
        """mode 3 on a dense tensor: mean and biased variance of every channel in one pass"""
        mean, var = torch.empty(C, device=a.device), torch.empty(C, device=a.device)
        scr = torch.empty(2 * self.lib.srcgan_col_reduce_blocks(npix) * C, dtype=torch.float32, device=a.device)
        self.N.check(self.lib.srcgan_col_reduce(3, a.data_ptr(), C, 0, None, 0, 0, None, None, npix, C, 1.0, mean.data_ptr(), var.data_ptr(),
                                                scr.data_ptr(), self.N.dtype_id(a.dtype), self.st()), "srcgan_col_reduce")
        return mean, var

    def bn_finalize(self, mean, var, count, momentum, eps, rmean=None, rvar=None, nbt=None):
        C = mean.numel()
        rstd = torch.full((C + 8,), SENT, device=mean.device)
        p = lambda t: None if t is None else t.data_ptr()
        self.N.check(self.lib.srcgan_bn_finalize(mean.data_ptr(), var.data_ptr(), rstd.data_ptr(), p(rmean), p(rvar), p(nbt), C, count,
                                                 momentum, eps, self.st()), "srcgan_bn_finalize")
        return rstd

    def bn_eval_rstd(self, rvar, eps):
        C = rvar.numel()
        rstd = torch.full((C + 8,), SENT, device=rvar.device)
        self.N.check(self.lib.srcgan_bn_eval_rstd(rvar.data_ptr(), rstd.data_ptr(), C, eps, self.st()), "srcgan_bn_eval_rstd")
        return rstd

    def bn_apply(self, z, y, mean, rstd, gamma, beta, npix, C, cs, slope=SLOPE):
        self.N.check(self.lib.srcgan_bn_apply_lrelu(z.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                    npix, C, cs, slope, self.N.dtype_id(z.dtype), self.st()), "srcgan_bn_apply_lrelu")

    def bn_bwd(self, g, z, dz, mean, rstd, gamma, sum_g, sum_gx, npix, C, cs):
        self.N.check(self.lib.srcgan_bn_bwd_apply(g.data_ptr(), z.data_ptr(), dz.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                  sum_g.data_ptr(), sum_gx.data_ptr(), npix, C, cs, self.N.dtype_id(z.dtype), self.st()),
                     "srcgan_bn_bwd_apply")

    def add_inplace(self, y, ys, x, xs, mz, ms, slope, npix, C):
        ms = ms or (0, 0, 0)
        mp = None if mz is None else mz.data_ptr()
        if ys[2] == 0 and xs[2] == 0 and ms[2] == 0:
            rc = self.lib.srcgan_add_inplace(y.data_ptr(), ys[0], ys[1], x.data_ptr(), xs[0], xs[1], mp, ms[0], ms[1], slope, npix, C,
                                             self.N.dtype_id(y.dtype), self.st())
        else:
            rc = self.lib.srcgan_add_inplace_planes(y.data_ptr(), ys[0], ys[1], ys[2], x.data_ptr(), xs[0], xs[1], xs[2], mp, ms[0], ms[1], ms[2],
                                                    slope, npix, C, self.N.dtype_id(y.dtype), self.st())
        self.N.check(rc, "srcgan_add_inplace")

    def upsample2(self, src, s_cs, s_coff, s_plane, dst, d_cs, B, H, W, C):
        self.N.check(self.lib.srcgan_upsample2_nhwc(src.data_ptr(), s_cs, s_coff, s_plane, dst.data_ptr(), d_cs, B, H, W, C,
                                                    self.N.dtype_id(src.dtype), self.st()), "srcgan_upsample2_nhwc")

    def sum2x2(self, src, s_cs, dst, d_cs, mz, m_cs, slope, B, H, W, C):
        self.N.check(self.lib.srcgan_sum2x2_nhwc(src.data_ptr(), s_cs, dst.data_ptr(), d_cs, None if mz is None else mz.data_ptr(), m_cs, slope,
                                                 B, H, W, C, self.N.dtype_id(src.dtype), self.st()), "srcgan_sum2x2_nhwc")

    def pixel_shuffle(self, src, s_cs, dst, d_cs, B, H, W, C, r, inverse):
        self.N.check(self.lib.srcgan_pixel_shuffle_nhwc(src.data_ptr(), s_cs, dst.data_ptr(), d_cs, B, H, W, C, r, inverse,
                                                        self.N.dtype_id(src.dtype), self.st()), "srcgan_pixel_shuffle_nhwc")

    def mask(self, g, act, slope, n):
        self.N.check(self.lib.srcgan_mask_inplace(g.data_ptr(), act.data_ptr(), slope, n, self.N.dtype_id(g.dtype), self.st()), "srcgan_mask_inplace")


@pytest.fixture(scope="module")
def L():
    return Lib()


def report(what, dt, value, bound):
    print(f"[glue] {what} {dt}: max normalised error {value:.3e} (bound {bound:.3e})")


def assert_elementwise(out, ref, norm, eps, what, dt):
    """|out - ref| <= eps * norm for every element; prints the largest |out - ref| / norm"""
    err = (out.double() - ref).abs()
    ratio = torch.where(norm > 0, err / norm.clamp_min(1e-300), torch.zeros_like(err))
    report(what, dt, float(ratio.max()), eps)
    bad = err > eps * norm
    assert not bool(bad.any()), f"{what} {dt}: {int(bad.sum())} elements over the bound, worst ratio {float(ratio.max()):.3e} > {eps:.3e}"


# --------------------------------------------------------------------------- 1. column reductions
EXACT_SHAPES = [(n, c) for n in (1, 3, 255, 257, 1023, 4099, 131073) for c in (1, 3, 8, 24, 64, 65, 128, 512) if not (n == 131073 and c > 64)]
# layouts of a 64-channel slice: (a_cs, a_coff, z_cs, z_coff, base pointer offset in elements)
EXACT_LAYOUTS = [(96, 32, 96, 32, 0),       # slice of a wider tensor: stays on the vector kernel
                 (96, 4, 96, 4, 0),         # offset 4: no 16-byte vector in a 16-bit type -> the scalar kernel (f32: still vector)
                 (64, 0, 64, 0, 1),         # base pointer one element off 16 bytes -> scalar
                 (96, 32, 128, 64, 0),      # mode 2: z in a stride and at an offset of its own
                 (96, 32, 80, 4, 0)]        # mode 2: a vectorisable, z not (16-bit) -> scalar


def _exact(L, mode, k, scale):
    ref, _ = ref_col_reduce(mode, k, scale)
    out = L.col_reduce(mode, k, scale)
    again = L.col_reduce(mode, k, scale)
    for o, o2, r in zip(out, again, ref):
        assert same_bits(o, r.float()), (mode, k["npix"], k["C"], k["a_cs"], k["a_coff"], float((o.double() - r).abs().max()))
        assert same_bits(o, o2), "a second call gave other bits"


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_col_reduce_counts_every_pixel_once(L, dt, mode):
    """Integer-valued operands (reduce_case 'int') and a power-of-two scale: every partial sum is exact in f32 whatever the order,
    so the result must have the bits of the float64 sum -- a pixel or channel dropped or counted twice cannot hide.  The shapes
    take the scalar kernel (C = 1, 3, 65; 24 in f32, where 256 % 6 != 0; its second 64-channel trip at C = 65 ... 512 when
    taken), the vector kernel with 256 / (C / epp) = 1 ... 256 pixel lanes, the four-pixels-in-flight body with every tail
    length, and the grid capped at 512 blocks with empty trailing blocks (npix = 131073: per = 257, 511 * 257 > npix)."""
    torch.manual_seed(100 + mode)
    for npix, C in EXACT_SHAPES:
        _exact(L, mode, reduce_case("int", npix, C, TDT[dt], "cuda"), 0.125)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_col_reduce_slices_and_alignment(L, dt, mode):
    """The same exact check on a 64-channel slice in the layouts of EXACT_LAYOUTS; everything outside the slice holds 1000, so a
    wrong stride or offset is unmistakable."""
    torch.manual_seed(200 + mode)
    for a_cs, a_coff, z_cs, z_coff, mis in EXACT_LAYOUTS:
        for npix in (3, 1023, 4099):
            _exact(L, mode, reduce_case("int", npix, 64, TDT[dt], "cuda", a_cs, a_coff, z_cs, z_coff, mis), 2.0)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_col_reduce_accuracy(L, dt, mode):
    """Random normal data against float64 of the quantised inputs: per channel |out - ref| <= 512 * 2^-24 * sum |terms| (both in
    float64, both times `scale`).  A chain of n f32 additions is off by at most (n - 1) * 2^-24 * sum |terms| to first order,
    and 512 bounds the longest serial chain at these sizes: with per = 257 pixels per block and one pixel lane (C / epp = 256)
    a thread adds 257 terms, otherwise a thread adds per / PL terms and one thread then adds the PL <= 256 lane sums; the
    finalise step adds 16 block partials per lane (4 chains of 4) and then 32 lane sums: about 257 + 50.  The terms' own
    rounding (a - mean, the products) adds 3 * 2^-24 * sum |terms|, inside the same bound."""
    torch.manual_seed(300 + mode)
    worst = 0.0
    for npix, C in ((100003, 128), (4097, 64), (131073, 8)):
        k = reduce_case("normal", npix, C, TDT[dt], "cuda")
        scale = 1.0 if mode == 2 else 1.0 / npix
        ref, norm = ref_col_reduce(mode, k, float(torch.tensor(scale, dtype=torch.float32)))
        for o, r, n in zip(L.col_reduce(mode, k, scale), ref, norm):
            err = (o.double() - r).abs()
            worst = max(worst, float((err / n).max()))
            assert bool((err <= 512 * U32 * n).all()), (mode, npix, C, float((err / n).max()))
    report(f"col_reduce mode {mode}", dt, worst, 512 * U32)


# --------------------------------------------------------------------------- 2. BatchNorm pieces
@pytest.mark.parametrize("count", [1, 2, 98304])
@pytest.mark.parametrize("C", [1, 64, 257, 512])
def test_bn_finalize_and_eval_rstd(L, C, count):
    """rstd = (var + eps)^-1/2, the running statistics with the unbiased factor count / (count - 1) (1 at count = 1) and
    num_batches_tracked + 1 -- once, also when C > 256 launches two blocks -- against float64 of the f32 inputs.  Bound:
    4 * 2^-24 * N, N = the float64 sum of the absolute terms (rstd and the running variance have positive terms only: that is
    4 * 2^-24 relative; the running mean has N = |(1 - m) rm| + |m mean|).  The f32 chain: rstd rounds var + eps (a quarter ulp of
    the result) and takes the hardware reciprocal square root (1 ulp = 2 * 2^-24); a running statistic rounds 1 - m, two or
    three products, the f32 form of count / (count - 1) and one sum: at most 4 roundings on any term's way to the result.  The 8
    floats behind each output keep their sentinel (C = 257: the second block's idle threads), and with null pointers for the
    running statistics only rstd is written."""
    torch.manual_seed(400 + C)
    mom, eps = 0.1, 1e-5
    m64, e64 = float(torch.tensor(mom, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    mean = torch.randn(C, device="cuda")
    var = torch.rand(C, device="cuda") * 4 + 1e-3
    var[0] = 0.0
    rmean0 = torch.full((C + 8,), SENT, device="cuda"); rmean0[:C] = torch.randn(C, device="cuda")
    rvar0 = torch.full((C + 8,), SENT, device="cuda"); rvar0[:C] = torch.rand(C, device="cuda") + 0.5
    nbt = torch.tensor([41, 7], dtype=torch.int64, device="cuda")
    rmean, rvar = rmean0.clone(), rvar0.clone()
    rstd = L.bn_finalize(mean, var, count, mom, eps, rmean, rvar, nbt)
    assert nbt.tolist() == [42, 7]
    for t in (rstd, rmean, rvar):
        assert bool((t[C:] == SENT).all())
    ref_rstd = (var.double() + e64) ** -0.5
    unb = count / (count - 1) if count > 1 else 1.0
    t_mean = [(1 - m64) * rmean0[:C].double(), m64 * mean.double()]
    t_var = [(1 - m64) * rvar0[:C].double(), m64 * var.double() * unb]
    assert_elementwise(rstd[:C], ref_rstd, ref_rstd, 4 * U32, "bn_finalize rstd", "fp32")
    assert_elementwise(rmean[:C], t_mean[0] + t_mean[1], t_mean[0].abs() + t_mean[1].abs(), 4 * U32, "bn_finalize running_mean", "fp32")
    assert_elementwise(rvar[:C], t_var[0] + t_var[1], t_var[0].abs() + t_var[1].abs(), 4 * U32, "bn_finalize running_var", "fp32")
    # null running statistics: rstd has the same bits, nothing else moves
    rstd2 = L.bn_finalize(mean, var, count, mom, eps)
    assert same_bits(rstd, rstd2) and nbt.tolist() == [42, 7]
    # the evaluation-mode form: the same expression on the running variance
    rstd3 = L.bn_eval_rstd(var, eps)
    assert same_bits(rstd, rstd3)


def bn_apply_case(npix, C, tdt, device):
    """Per-channel constants on coarse binary grids (gamma, beta, mean multiples of 1/16; rstd in {0.5, 1, 2}), so that the
    kernel's sc = rstd * gamma and sh = beta - mean * sc are exact and the reference alone stays far inside the bound; |z| >= 2^-6
    so that no result lands in fp16's subnormal range without a cancellation (where N >= |sh| >= 2^-9 carries the bound: fp16's
    subnormal step is 2^-24).  Channel
    0 has sh = 0.  Planted rows: z = 0 (u = sh: exactly 0 in channel 0), z = -+2^-6 against the sign of sc (u slightly negative
    in channel 0), z = the type's nearest value to -sh / sc (u = 0 or a rounding away from it) and that value times 1 + 2^-7."""
    q = lambda t: torch.round(t * 16) / 16
    gamma = q(torch.randn(C, device=device))
    gamma = torch.where(gamma == 0, torch.full_like(gamma, 0.0625), gamma)
    rstd = 2.0 ** torch.randint(-1, 2, (C,), device=device).float()
    mean, beta = q(torch.randn(C, device=device) * 0.5), q(torch.randn(C, device=device))
    mean[0], beta[0] = 0.0, 0.0
    z = torch.randn(npix, C, device=device)
    z = torch.where(z < 0, -torch.ones_like(z), torch.ones_like(z)) * z.abs().clamp_min(2.0 ** -6)
    sc = rstd * gamma
    sh = beta - mean * sc
    z[0] = 0.0
    z[1] = -(2.0 ** -6) * torch.sign(sc)
    z[2] = -sh / sc
    z[3] = (-sh / sc).to(tdt).float() * (1 + 2.0 ** -7)
    return z.to(tdt), mean, rstd, gamma, beta


def ref_bn_apply(z, mean, rstd, gamma, beta, slope):
    sc = rstd.double() * gamma.double()
    sh = beta.double() - mean.double() * sc
    u = z.double() * sc + sh
    s64 = float(torch.tensor(slope, dtype=torch.float32))
    return torch.where(u > 0, u, u * s64), (z.double() * sc).abs() + sh.abs(), u


def _bn_shapes(dt):
    return [(7, 256), (1025, 64), (130, 512), (4097, 4 if dt == "fp32" else 8)]


@pytest.mark.parametrize("dt", DTS)
def test_bn_apply_lrelu_elementwise(L, dt):
    """y = lrelu(z * sc + sh), sc = rstd * gamma, sh = beta - mean * sc, against float64, element by element:
    |y - ref| <= eps_T * (|z sc| + |sh|).  The last shape has one channel vector per pixel (G = 1, 256 pixel lanes)."""
    torch.manual_seed(500)
    for npix, C in _bn_shapes(dt):
        z, mean, rstd, gamma, beta = bn_apply_case(npix, C, TDT[dt], "cuda")
        ref, norm, u = ref_bn_apply(z, mean, rstd, gamma, beta, SLOPE)
        assert bool((u == 0).any()) and bool(((u < 0) & (u > -0.1)).any()) and bool((u > 0).any())        # the slope branch's edge is in the data
        y = torch.full((npix + 1, C), SENT, dtype=TDT[dt], device="cuda")
        L.bn_apply(z, y, mean, rstd, gamma, beta, npix, C, C)
        assert bool((y[npix] == SENT).all())
        assert_elementwise(y[:npix], ref, norm, EPS_T[dt], f"bn_apply_lrelu {npix}x{C}", dt)


def bn_bwd_case(npix, C, tdt, device):
    sgn = lambda n: torch.where(torch.rand(n, device=device) < 0.5, -1.0, 1.0)
    g, z = torch.randn(npix, C, device=device).to(tdt), (torch.randn(npix, C, device=device) * 1.5 + 0.3).to(tdt)
    mean, rstd = 0.3 + 0.5 * torch.randn(C, device=device), 0.5 + 1.5 * torch.rand(C, device=device)
    gamma = sgn(C) * (0.25 + torch.rand(C, device=device))
    sum_g, sum_gx = npix * sgn(C) * (0.1 + torch.rand(C, device=device)), npix * torch.randn(C, device=device)
    return g, z, mean, rstd, gamma, sum_g, sum_gx


def ref_bn_bwd(g, z, mean, rstd, gamma, sum_g, sum_gx, npix):
    ka, kb = gamma.double() * rstd.double(), sum_g.double() / npix
    kc, d = rstd.double() * sum_gx.double() / npix, z.double() - mean.double()
    return ka * (g.double() - kb - d * kc), ka.abs() * (g.double().abs() + kb.abs() + d.abs() * kc.abs())


@pytest.mark.parametrize("dt", DTS)
def test_bn_bwd_apply_elementwise_and_in_place(L, dt):
    """dz = ka (g - kb - (z - mu) kc), ka = gamma rstd, kb = sum_g / n, kc = rstd sum_gx / n, against float64, element by element:
    |dz - ref| <= eps_T * |ka| (|g| + |kb| + |z - mu| |kc|) (f32: 1 / n, three constants' products and five operations per element,
    about 9 * 2^-24 N, under 2^-20 N; N >= |ka| |kb| >= 0.0125 keeps fp16's subnormal step, 2^-24, under the bound).  The in-place call
    (dz == g, as the discriminator's backward makes it) must give the bits of the out-of-place call."""
    torch.manual_seed(600)
    for npix, C in _bn_shapes(dt):
        g, z, mean, rstd, gamma, sum_g, sum_gx = bn_bwd_case(npix, C, TDT[dt], "cuda")
        ref, norm = ref_bn_bwd(g, z, mean, rstd, gamma, sum_g, sum_gx, npix)
        dz = torch.full((npix + 1, C), SENT, dtype=TDT[dt], device="cuda")
        L.bn_bwd(g, z, dz, mean, rstd, gamma, sum_g, sum_gx, npix, C, C)
        assert bool((dz[npix] == SENT).all())
        assert_elementwise(dz[:npix], ref, norm, EPS_T[dt], f"bn_bwd_apply {npix}x{C}", dt)
        gi = g.clone()
        L.bn_bwd(gi, z, gi, mean, rstd, gamma, sum_g, sum_gx, npix, C, C)
        assert same_bits(gi, dz[:npix])


COMPOSITION_SEED = {"fp32": 13, "bf16": 0, "fp16": 4}       # per type: the quantised z differs, and so does what is near the kink


def composition_case(tdt, seed):
    """z [2,128,33,17] around a per-channel mean near 0.5, gamma = +-[0.5, 1.5], beta = -sign(gamma) [0.25, 1.25] (so that
    sh = beta - mean gamma rstd has no cancellation and N >= 0.5 everywhere), dy normal.  Generated on the CPU from a fixed seed
    chosen so that no pre-activation lies within 1e-5 of LeakyReLU's kink (asserted by the test): the native chain's statistics
    differ from float64 by about 1e-7, and an element that changed sides would compare a gradient times 1 with one times 0.2."""
    gen = torch.Generator().manual_seed(seed)
    C = 128
    z = (torch.randn(2, C, 33, 17, generator=gen) + 0.5 + 0.2 * torch.randn(1, C, 1, 1, generator=gen)).to(tdt)
    sg = torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
    gamma = sg * (0.5 + torch.rand(C, generator=gen))
    beta = -sg * (0.25 + torch.rand(C, generator=gen))
    dy = torch.randn(2, C, 33, 17, generator=gen).to(tdt)
    return z, gamma, beta, dy


def composition_reference(z, gamma, beta, g_of_pre):
    """float64: y = leaky_relu(batch_norm(z, training)) and dz by autograd for the upstream gradient g = g_of_pre(pre) arriving
    at the normalisation's output; the terms' norms of both bounds"""
    z64 = z.double().requires_grad_(True)
    g64, b64 = gamma.double(), beta.double()
    pre = F.batch_norm(z64, None, None, g64, b64, training=True, eps=1e-5)
    y = F.leaky_relu(pre, SLOPE).detach()
    g = g_of_pre(pre.detach())
    pre.backward(g)
    zd = z64.detach()
    mu, var = zd.mean((0, 2, 3), keepdim=True), zd.var((0, 2, 3), unbiased=False, keepdim=True)
    rstd = (var + 1e-5) ** -0.5
    sc = g64.view(1, -1, 1, 1) * rstd
    n_fwd = (zd * sc).abs() + (b64.view(1, -1, 1, 1) - mu * sc).abs()
    npix = zd.numel() // zd.shape[1]
    kb = g.sum((0, 2, 3), keepdim=True) / npix
    kc = rstd * (g * (zd - mu) * rstd).sum((0, 2, 3), keepdim=True) / npix
    n_bwd = sc.abs() * (g.abs() + kb.abs() + (zd - mu).abs() * kc.abs())
    return y, z64.grad, n_fwd, n_bwd, pre.detach()


@pytest.mark.parametrize("dt", DTS)
def test_batchnorm_chain_against_float64(L, dt):
    """The discriminator's sequence (nets.hip, norm_forward / norm_backward): col_reduce(3) -> bn_finalize -> bn_apply_lrelu, then
    g = dy * lrelu'(y) (srcgan_mask_inplace) -> col_reduce(2) -> bn_bwd_apply in place, on npix = 2 * 33 * 17, C = 128, against
    float64 leaky_relu(batch_norm(training)) and float64 autograd.  Bound per element: (eps_T + 1e-5) * N with the N of the two
    element-wise tests -- eps_T for the element's own arithmetic, 1e-5 for the statistics (what test_single_pass_mean_and_variance
    grants the variance).
    The chain stores g in the activation type between the two kernels, and eps_T is one rounding to that type (2^-8, 2^-11), so
    a second 16-bit rounding has no room in it: an exact-arithmetic chain, run on the CPU, is up to 2 eps_T N from a reference
    that never rounds g (2533 elements over the bound in fp16).  The store is therefore checked on its own, to the bit --
    g has the bits of where(y > 0, dy, dy * 0.2) in f32 cast once, and y lies on float64's side of the kink everywhere -- and
    autograd starts from that stored g: float64 of the quantised inputs, as everywhere in this file."""
    tdt = TDT[dt]
    z, gamma, beta, dy = composition_case(tdt, COMPOSITION_SEED[dt])
    B, C, H, W = z.shape
    npix = B * H * W
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(npix, C).contiguous().cuda()
    nchw = lambda t: t.view(B, H, W, C).permute(0, 3, 1, 2).cpu()
    zd, dyd, gam, bet = nhwc(z), nhwc(dy), gamma.cuda(), beta.cuda()
    mean, var = L.mean_var(zd, npix, C)
    rstd = L.bn_finalize(mean, var, npix, 0.1, 1e-5)[:C].clone()
    y = torch.empty_like(zd)
    L.bn_apply(zd, y, mean, rstd, gam, bet, npix, C, C)
    g = dyd.clone()
    L.mask(g, y, SLOPE, g.numel())
    assert same_bits(g.view(-1), ref_mask(dyd.view(-1), y.view(-1), SLOPE))
    g_stored = nchw(g).double()
    y_ref, dz_ref, n_fwd, n_bwd, pre = composition_reference(z, gamma, beta, lambda pre: g_stored)
    assert float(pre.abs().min()) > 1e-5, "composition_case: a pre-activation sits on LeakyReLU's kink; choose another seed"
    assert torch.equal(nchw(y).float() > 0, pre > 0)
    assert_elementwise(y, nhwc(y_ref), nhwc(n_fwd), EPS_T[dt] + 1e-5, "batchnorm chain forward", dt)
    k = dict(a=g, a_cs=C, a_coff=0, z=zd, z_cs=C, z_coff=0, mean=mean, rstd=rstd, npix=npix, C=C)
    sum_g, sum_gx = L.col_reduce(2, k, 1.0)
    L.bn_bwd(g, zd, g, mean, rstd, gam, sum_g, sum_gx, npix, C, C)
    assert_elementwise(g, nhwc(dz_ref), nhwc(n_bwd), EPS_T[dt] + 1e-5, "batchnorm chain backward", dt)


@pytest.mark.parametrize("dt", DTS)
def test_bn_apply_refuses_shapes_it_cannot_vectorise(L, dt):
    """cs != C, C / epp not dividing 256 (24 in f32, 48 in 16 bits: six vectors) and C % epp != 0 are errors, for the forward and
    the backward kernel, and nothing is written."""
    epp = EPP[dt]
    for C, cs in ((64, 72), (6 * epp, 6 * epp), (epp + epp // 2, epp + epp // 2)):
        npix = 5
        z = torch.zeros(npix, cs, dtype=TDT[dt], device="cuda")
        y = torch.full((npix, cs), SENT, dtype=TDT[dt], device="cuda")
        c = [torch.ones(C, device="cuda") for _ in range(6)]
        with pytest.raises(RuntimeError, match="dense NHWC"):
            L.bn_apply(z, y, c[0], c[1], c[2], c[3], npix, C, cs)
        with pytest.raises(RuntimeError, match="dense NHWC"):
            L.bn_bwd(z, z, y, c[0], c[1], c[2], c[4], c[5], npix, C, cs)
        torch.cuda.synchronize()
        assert bool((y == SENT).all())


# --------------------------------------------------------------------------- 3. residual join
def _join_values(B, H, W, C, tdt, device):
    y, x = torch.randn(B, H, W, C, device=device).to(tdt), torch.randn(B, H, W, C, device=device).to(tdt)
    x.view(-1)[5::11] = -y.view(-1)[5::11]                         # exact cancellations
    return y, x, plant_zeros(torch.randn(B, H, W, C, device=device)).to(tdt)


@pytest.mark.parametrize("dt", DTS)
def test_add_inplace_interleaved_slices(L, dt):
    """y[:, 32:64] of 96 channels += x[:, 0:32] of 64, times LeakyReLU'(mz[:, 64:96] of 128) or not: the bits of the same f32
    expression in torch, cast once (the kernel's and torch's casts both round to nearest even; no case needed an allowance),
    and every channel outside y's slice keeps its sentinel.  mz holds +0.0, -0.0 and small values of both signs."""
    torch.manual_seed(700)
    C = 32
    for npix in (1, 257, 5000):
        for with_mz, slope in ((False, 0.0), (True, SLOPE), (True, 0.0)):
            yv, xv, mv = _join_values(1, 1, npix, C, TDT[dt], "cuda")
            (y, ys), (x, xs), (mz, ms) = operand(yv, 96, 32, False), operand(xv, 64, 0, False), operand(mv, 128, 64, False)
            if not with_mz:
                mz, ms = None, None
            want = ref_add_inplace(y, ys, x, xs, mz, ms, slope, npix, C)
            L.add_inplace(y, ys, x, xs, mz, ms, slope, npix, C)
            assert same_bits(y, want), (npix, with_mz, slope)


@pytest.mark.parametrize("which", ["y", "x", "mz", "all"])
@pytest.mark.parametrize("dt", DTS)
def test_add_inplace_blocked_planes(L, dt, which):
    """The blocked layout [plane][B*H*W][64 bytes] (ops.make_blocked; plane stride B*H*W*64 bytes, pixel record KCE channels) for
    each operand in turn and for all three, the others interleaved.  C = 48 and 80 from offsets 12, 4 and 8 of 96 channels: every
    slice starts inside a plane and crosses one or more plane boundaries in every type (KCE = 16 in f32, 32 in 16 bits)."""
    torch.manual_seed(710)
    B, H, W = 2, 5, 7
    npix = B * H * W
    for C in (48, 80):
        yv, xv, mv = _join_values(B, H, W, C, TDT[dt], "cuda")
        (y, ys), (x, xs), (mz, ms) = (operand(v, 96, off, which in (nm, "all")) for v, off, nm in ((yv, 12, "y"), (xv, 4, "x"), (mv, 8, "mz")))
        want = ref_add_inplace(y, ys, x, xs, mz, ms, SLOPE, npix, C)
        L.add_inplace(y, ys, x, xs, mz, ms, SLOPE, npix, C)
        assert same_bits(y, want), (C, which)


# --------------------------------------------------------------------------- 4. data movement
@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("dt", DTS)
def test_upsample2_nhwc_bits(L, dt, blocked):
    """F.interpolate(scale_factor=2, mode='nearest') of a 64-channel slice into channels [0, 64) of a 96-channel destination:
    equal bits, the destination's other channels untouched.  Source: interleaved (s_cs = 96, s_coff = 32), or channels [16, 80)
    of a blocked 96-channel buffer -- from inside the first plane into the later ones (planes 0-2 in 16 bits, 1-4 in f32)."""
    torch.manual_seed(800)
    B, C = 2, 64
    for H, W in ((1, 1), (5, 9), (16, 33)):
        v = plant_zeros(torch.randn(B, H, W, C, device="cuda")).to(TDT[dt])
        src, (s_cs, s_coff, s_plane) = operand(v, 96, 16 if blocked else 32, blocked)
        dst = torch.full((B, 2 * H, 2 * W, 96), SENT, dtype=TDT[dt], device="cuda")
        want = ref_upsample2(src, s_cs, s_coff, s_plane, dst, 96, B, H, W, C)
        L.upsample2(src, s_cs, s_coff, s_plane, dst, 96, B, H, W, C)
        assert same_bits(dst, want), (H, W)


def _sum2x2_operands(kind, B, H, W, C, tdt, device):
    """src: channels [32, 96) of 96; dst: channels [16, 80) of 80 + 16; mz: channels [8, 72) of 72 (views at the slice's start)"""
    if kind == "int":
        sv = torch.randint(-4, 5, (B, 2 * H, 2 * W, C), device=device).to(tdt)
    else:
        sv = torch.randn(B, 2 * H, 2 * W, C, device=device).to(tdt)
    mv = plant_zeros(torch.randn(B, H, W, C, device=device)).to(tdt)
    src = torch.full((B * 4 * H * W * 96,), SENT, dtype=tdt, device=device)
    src.view(-1, 96)[:, 32:] = sv.view(-1, C)
    mz = torch.full((B * H * W * 72 + 8,), SENT, dtype=tdt, device=device)
    mz[8:].view(-1, 72)[:, :C] = mv.view(-1, C)
    return src[32:], mz[8:]


@pytest.mark.parametrize("dt", DTS)
def test_sum2x2_nhwc_is_the_adjoint_of_upsample2(L, dt):
    """dst = the sum of each 2x2 block [times LeakyReLU'(mz)], C = 64, B = 2, with every operand a slice of a wider tensor.
    Integer data in [-4, 4]: sums of four are exact, so the result has the bits of avg_pool2d * 4 times the f32 factor, cast
    once, and <up(x), g> = <x, sum2x2(g)> holds exactly in float64.  Random data: |out - ref| <= eps_T * sum of the four
    absolute terms (times the factor), element by element.  The destination's other channels keep their sentinel."""
    torch.manual_seed(810)
    B, C, tdt = 2, 64, TDT[dt]
    for H, W in ((1, 1), (5, 9), (16, 33)):
        for kind in ("int", "normal"):
            for with_mz in (False, True):
                src, mz = _sum2x2_operands(kind, B, H, W, C, tdt, "cuda")
                if not with_mz:
                    mz = None
                ref, norm = ref_sum2x2(src, 96, mz, 72, SLOPE, B, H, W, C)
                dstb = torch.full((B * H * W, 96), SENT, dtype=tdt, device="cuda")
                L.sum2x2(src, 96, dstb.view(-1)[16:], 96, mz, 72, SLOPE, B, H, W, C)
                assert bool((dstb[:, :16] == SENT).all()) and bool((dstb[:, 80:] == SENT).all())
                out = dstb[:, 16:80]
                if kind == "int":
                    want = take(src, B * 4 * H * W, 96, 0, C).float().view(B, 2 * H, 2 * W, C).permute(0, 3, 1, 2)
                    want = (F.avg_pool2d(want, 2) * 4).permute(0, 2, 3, 1).reshape(B * H * W, C)
                    if with_mz:
                        want = want * lrelu_factor(take(mz, B * H * W, 72, 0, C), SLOPE)
                    assert same_bits(out.contiguous(), want.to(tdt)), (H, W, with_mz)
                else:
                    assert_elementwise(out, ref, norm, EPS_T[dt], f"sum2x2 {H}x{W} mz={with_mz}", dt)
        # adjoint identity on integer data, both kernels' outputs, float64 inner products
        x = torch.randint(-4, 5, (B, H, W, C), device="cuda").to(tdt)
        gsrc, _ = _sum2x2_operands("int", B, H, W, C, tdt, "cuda")
        up = torch.empty(B * 4 * H * W, C, dtype=tdt, device="cuda")
        L.upsample2(x, C, 0, 0, up, C, B, H, W, C)
        sg = torch.empty(B * H * W, C, dtype=tdt, device="cuda")
        L.sum2x2(gsrc, 96, sg, C, None, 0, 0.0, B, H, W, C)
        gv = take(gsrc, B * 4 * H * W, 96, 0, C).double()
        assert float((up.double() * gv).sum()) == float((x.double().view(-1, C) * sg.double()).sum())


@pytest.mark.parametrize("dt", DTS)
def test_pixel_shuffle_nhwc_both_directions(L, dt):
    """F.pixel_shuffle / F.pixel_unshuffle on NHWC records with strides larger than the channel counts (padding = sentinel, kept),
    r in {2, 3, 4}, C in {1, 3, 8}, 1x1 and 7x5, B = 2: equal bits, and forward then inverse returns the input."""
    torch.manual_seed(820)
    B, tdt = 2, TDT[dt]
    for r in (2, 3, 4):
        for C in (1, 3, 8):
            for H, W in ((1, 1), (7, 5)):
                lo_cs, hi_cs = C * r * r + 3, C + 2
                lo = slice_buffer(plant_zeros(torch.randn(B * H * W, C * r * r, device="cuda")).to(tdt), lo_cs, 0)
                hi = torch.full((B * H * r * W * r * hi_cs,), SENT, dtype=tdt, device="cuda")
                want = ref_pixel_shuffle(lo, lo_cs, hi, hi_cs, B, H, W, C, r, 0)
                L.pixel_shuffle(lo, lo_cs, hi, hi_cs, B, H, W, C, r, 0)
                assert same_bits(hi, want), (r, C, H, W)
                back = torch.full_like(lo, SENT)
                L.pixel_shuffle(hi, hi_cs, back, lo_cs, B, H, W, C, r, 1)
                assert same_bits(back, lo), (r, C, H, W)
                src = slice_buffer(torch.randn(B * H * r * W * r, C, device="cuda").to(tdt), hi_cs, 0)
                dst = torch.full_like(lo, SENT)
                want = ref_pixel_shuffle(src, hi_cs, dst, lo_cs, B, H, W, C, r, 1)
                L.pixel_shuffle(src, hi_cs, dst, lo_cs, B, H, W, C, r, 1)
                assert same_bits(dst, want), (r, C, H, W)


@pytest.mark.parametrize("dt", DTS)
def test_mask_inplace_bits(L, dt):
    """g *= act > 0 ? 1 : slope over the first n elements: the bits of where(act > 0, g, g * slope) in f32 cast once (slope 0 turns
    a negative g into -0.0 on both sides -- the fp16 kernel once returned +0.0 there, its product compiled to a fused
    g * slope + 0.0); act holds +0.0 and -0.0; the elements behind n are untouched."""
    torch.manual_seed(830)
    for n in (1, 255, 257, 70001):
        for slope in (0.0, SLOPE):
            g = torch.randn(n + 5, device="cuda").to(TDT[dt])
            act = plant_zeros(torch.randn(n + 5, device="cuda")).to(TDT[dt])
            want = ref_mask(g, act, slope, n)
            L.mask(g, act, slope, n)
            assert same_bits(g, want), (n, slope)
