"""Direct tests of the convolution forms the U-Net is the first op-list network to reach (srcgan_amd.UnetGenerator, csrc/oplist.hip
unet_plan), through the C ABI alone (srcgan_conv_igemm, srcgan_conv_wgrad), issued the way the executor issues them:

  * the down convolution: 4x4, stride 2, pad 1, with bias, with and without the fused LeakyReLU(0.2), at 2x2 -> 1x1 (the bottleneck),
    4x6 -> 2x3 and 32x32 -> 16x16, from 1 and 3 image channels (an 8-channel record, zero padded) and from 16 and 128;
  * RD_DECONV4, ConvTranspose2d(k4, s2, p1) + bias as the parity packs of the 4x4 stride-2 input gradient: ONE four-parity launch
    (128 -> 128, 256 -> 64) or FOUR 2x2 launches (32 -> 3, 32 -> 1: the outermost layer), at 1x1 -> 2x2, 1x2 -> 2x4 and 8x8 -> 16x16,
    the output written into a wider buffer;
  * its weight gradient, the stride-2 wgrad with the roles of x and dy exchanged, on NaN-filled guarded slabs;
  * its input gradient, the forward 4x4 stride-2 convolution of dy masked by a ReLU'd operand (the skip buffer);
  * the accumulate-then-mask step of the backward: the down convolution's four-parity input gradient + the skip buffer's gradient slice
    (r1, a prefix of a buffer twice as wide), times LeakyReLU'(0.2) of the stored activation:  g_z = leaky'(z) (g_a + relu'(z) g_r).

Operands are the small integers of tests/conv_exact.py, for which every order of f32 summation gives the same bits; references are float64
(torch's conv_transpose2d and autograd); outputs are compared whole with ``torch.equal`` in fp32, bf16 and fp16.  0.2 is no dyadic number:
where a slope of 0.2 applies, the reference multiplies the exact integer by float32(0.2) in float32 and rounds once to the storage type, as
the epilogue does.  Each case prints the kernel classes it ran and holds them against the intended form."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact as CE
from conv_exact import DTS, DT_TAG, TDT, SENTINEL
from test_gpu_mdsr_convs import Prof, same
from ws_guard import NAN, guarded_slabs

pytestmark = pytest.mark.gpu
_BUILT = {}


@pytest.fixture(scope="module")
def ops():
    from srcgan_amd import ops as o
    return o


def once(key, make):
    if key not in _BUILT:
        _BUILT[key] = make()
    return _BUILT[key]


def leaky32(pre64, mask64, slope):
    """where(mask > 0, pre, pre * float32(slope)) in float32: one rounding, the epilogue's"""
    p = pre64.float()
    return torch.where(mask64 > 0, p, p * torch.tensor(slope, dtype=torch.float32))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def par_packs(ops, w, rows, kdim, T):
    """the four parity packs of S2Dgrad{4, 1, cin = rows, cout = kdim} from w [kdim][rows][4][4], in one buffer -> (buffer, step)"""
    packs = [ops.pack_weight(w, rows, kdim, 2, 2, 16, rows * 16, -8, -2, (2 if a else 3) * 4 + (2 if b else 3), T) for a in (0, 1) for b in (0, 1)]
    step = packs[0].numel()
    return torch.cat(packs), step


# ------------------------------------------------------------------------------------------------ the down convolution
DOWN = [(cin, hw, act) for cin in (1, 3, 16, 128) for hw in ((2, 2), (4, 6), (32, 32)) for act in (False, True)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin, hw, act", DOWN)
def test_down_convolution_exact(ops, cin, hw, act, dt):
    cout = 32 if cin < 128 else 128
    c = CE.conv_case(f"unet_down_{cin}_{hw[0]}x{hw[1]}", k=(4, 4), s=2, pad=(1, 1), cin=cin, cout=cout, hw=hw, x_cs=max(cin, 8), y_cs=cout + 16)
    b, T = once(c["name"], lambda: CE.build_conv(c)), TDT[dt]
    CE.check_exact(c["name"], dt, b["bound"], b["pre"], b["pre"], 1.0)
    xb = b["x"].clone()
    xb[..., cin:] = 0                                   # an image record's padding channels are zero
    x, y = xb.to(T).cuda(), b["y0"].to(T).cuda()
    wp = ops.pack_weight(b["w"].float().cuda(), cout, cin, 4, 4, cin * 16, 16, 4, 1, 0, T)
    with Prof() as pr:
        ops.conv_igemm(x, wp, y, kh=4, kw=4, stride=2, Cin=max(cin, 8), Cout=cout, pad=(1, 1), bias=b["bias"].float().cuda(), act=act, slope=0.2)
        torch.cuda.synchronize()
    print(f"[class] {c['name']}-{'lrelu' if act else 'plain'}-{dt}: {', '.join(pr.classes)}")
    assert len(pr.classes) == 1 and pr.classes[0].startswith(f"conv_igemm<{DT_TAG[dt]},4x4,s2")
    want = torch.full(b["y0"].shape, SENTINEL, dtype=torch.float32)
    want[..., :cout] = nhwc(leaky32(b["pre"], b["pre"], 0.2) if act else b["pre"].float())
    assert b["OH"] == hw[0] // 2 and b["OW"] == hw[1] // 2
    same(y.cpu(), want.double() if dt == "fp32" else want.to(T).double(), "y")
    same(x.cpu(), xb, "x after the call")


# ------------------------------------------------------------------------------------------------ RD_DECONV4
def build_deconv(cin, cout, hw):
    g = CE.gen(f"unet_deconv4_{cin}_{cout}_{hw[0]}x{hw[1]}")
    x = CE.ternary((2, cin, hw[0], hw[1]), 0.5, g)
    w = CE.ternary((cin, cout, 4, 4), CE.w_density(4 * cin), g)
    bias = CE.ints((cout,), -4, 4, g)
    y = F.conv_transpose2d(x, w, bias, 2, 1)
    bound = F.conv_transpose2d(x.abs(), w.abs(), bias.abs(), 2, 1)
    dy = CE.ternary(tuple(y.shape), 0.5, g)             # the gradient arriving at the output
    mz = CE.ints((2, cin, hw[0], hw[1]), -2, 2, g).clamp_min(0)      # the ReLU'd operand the input gradient is masked by
    wv = w.clone().requires_grad_(True)
    xv = x.clone().requires_grad_(True)
    F.conv_transpose2d(xv, wv, None, 2, 1).backward(dy)
    wa, xa = w.abs().clone().requires_grad_(True), x.abs().clone().requires_grad_(True)
    F.conv_transpose2d(xa, wa, None, 2, 1).backward(dy.abs())
    return dict(x=x, w=w, bias=bias, y=y, bound=bound, dy=dy, mz=mz, gw=wv.grad, gx=xv.grad, gw_bound=wa.grad, gx_bound=xa.grad)


DECONV = [(cin, cout, hw) for (cin, cout) in ((128, 128), (256, 64), (32, 3), (32, 1)) for hw in ((1, 1), (1, 2), (8, 8))]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin, cout, hw", DECONV)
def test_transposed_convolution_exact(ops, cin, cout, hw, dt):
    b, T = once(("deconv", cin, cout, hw), lambda: build_deconv(cin, cout, hw)), TDT[dt]
    name = f"unet_deconv4_{cin}_{cout}_{hw[0]}x{hw[1]}"
    CE.check_exact(name, dt, b["bound"], b["y"], b["y"], 1.0)
    H, W = 2 * hw[0], 2 * hw[1]
    y_cs = cout + 32 if cout >= 8 else 8                # a wider buffer: the channels behind cout keep the sentinel
    x = nhwc(b["x"]).to(T).cuda()
    y = torch.full((2, H, W, y_cs), SENTINEL, dtype=T, device="cuda")
    bias = b["bias"].float().cuda()
    wall, step = par_packs(ops, b["w"].float().cuda(), cout, cin, T)
    vec = 4 if dt == "fp32" else 8
    with Prof() as pr:
        if cout % vec == 0:                             # S2Dgrad::run: all four parities from one staged tile
            ops.conv_igemm(x, wall, y, kh=2, kw=2, Cout=cout, OH=(H + 1) // 2, OW=(W + 1) // 2, os=2, npar=4, wpar_stride=step, bias=bias)
        else:
            for q in range(4):
                a, bb = q >> 1, q & 1
                ops.conv_igemm(x, wall[q * step:(q + 1) * step], y, kh=2, kw=2, Cout=cout, OH=(H - a + 1) // 2, OW=(W - bb + 1) // 2, pad=(1 - a, 1 - bb),
                               os=2, oa=a, ob=bb, bias=bias)
        torch.cuda.synchronize()
    print(f"[class] {name}-{dt}: {', '.join(pr.classes)}")
    if cout % vec == 0:
        assert pr.classes == [f"dgrad_s2k4<{DT_TAG[dt]},4 parities>"]
    else:
        assert pr.classes and all(k.startswith(f"conv_igemm<{DT_TAG[dt]},2x2,s1") for k in pr.classes)      # (the profiler reports a class once)
    want = torch.full((2, H, W, y_cs), SENTINEL, dtype=torch.float64)
    want[..., :cout] = nhwc(b["y"])
    same(y.cpu(), want, "y")
    same(x.cpu(), nhwc(b["x"]), "x after the call")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin, cout", [(128, 128), (256, 64), (32, 3), (32, 1)])
def test_transposed_convolution_weight_gradient_exact(ops, cin, cout, dt):
    """dW[ci][co][ky][kx] = sum x[i][j][ci] dy[2i + ky - 1][2j + kx - 1][co]: srcgan_conv_wgrad with dy := x, x := dy, k4 s2 p1, written in
    the stored layout [ci][co][4][4]; the slab's contents on entry are unspecified"""
    hw = (8, 8)
    b, T = once(("deconv", cin, cout, hw), lambda: build_deconv(cin, cout, hw)), TDT[dt]
    CE.check_exact(f"unet_deconv4_wgrad_{cin}_{cout}", dt, b["gw_bound"] + 8, b["gw"], b["gw"], 1.0, f32_out=True)
    ccs = max(cout, 8)
    xd = nhwc(b["x"]).to(T).cuda()
    dyb = torch.zeros(2, 16, 16, ccs, dtype=torch.float64)
    dyb[..., :cout] = nhwc(b["dy"])
    dyd = dyb.to(T).cuda()
    grad = torch.full((cin * cout * 16,), SENTINEL, device="cuda")
    with guarded_slabs(NAN, "cuda") as g, Prof() as pr:
        ops.conv_wgrad(xd, dyd, grad, kh=4, kw=4, stride=2, Cout=cin, Cin=cout, pad=(1, 1), layout=(cout * 16, 16, 4, 1, 0))
        torch.cuda.synchronize()
        assert g.calls == 1
    print(f"[class] unet_deconv4_wgrad_{cin}_{cout}-{dt}: {', '.join(pr.classes)}")
    assert len(pr.classes) == 1 and pr.classes[0].startswith(f"conv_wgrad<{DT_TAG[dt]},4x4,s2")
    same(grad.cpu().view(cin, cout, 4, 4), b["gw"], "grad")
    same(xd.cpu(), nhwc(b["x"]), "x after the call")
    same(dyd.cpu(), dyb, "dy after the call")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin, cout", [(128, 128), (256, 64), (32, 3), (32, 1)])
def test_transposed_convolution_input_gradient_exact(ops, cin, cout, dt):
    """dx[i][j][ci] = relu'(mz) sum dy[2i + ky - 1][2j + kx - 1][co] W[ci][co][ky][kx]: the forward 4x4 stride-2 pad-1 convolution of dy
    through the pack rows = ci, k = co, taps as stored, masked (slope 0) by the ReLU'd tensor the op read"""
    hw = (8, 8)
    b, T = once(("deconv", cin, cout, hw), lambda: build_deconv(cin, cout, hw)), TDT[dt]
    CE.check_exact(f"unet_deconv4_dgrad_{cin}_{cout}", dt, b["gx_bound"], b["gx"], b["gx"], 1.0)
    ccs = max(cout, 8)
    dyb = torch.zeros(2, 16, 16, ccs, dtype=torch.float64)
    dyb[..., :cout] = nhwc(b["dy"])
    dyd, mz = dyb.to(T).cuda(), nhwc(b["mz"]).to(T).cuda()
    dx = torch.full((2, 8, 8, cin), SENTINEL, dtype=T, device="cuda")
    wp = ops.pack_weight(b["w"].float().cuda(), cin, cout, 4, 4, cout * 16, 16, 4, 1, 0, T)
    with Prof() as pr:
        ops.conv_igemm(dyd, wp, dx, kh=4, kw=4, stride=2, Cin=ccs, Cout=cin, pad=(1, 1), mz=mz, mz_c0=0, mslope=0.0)
        torch.cuda.synchronize()
    print(f"[class] unet_deconv4_dgrad_{cin}_{cout}-{dt}: {', '.join(pr.classes)}")
    assert len(pr.classes) == 1 and pr.classes[0].startswith(f"conv_igemm<{DT_TAG[dt]},4x4,s2")
    assert bool((b["mz"] > 0).any()) and bool((b["mz"] == 0).any())
    same(dx.cpu(), nhwc(b["gx"] * (b["mz"] > 0)), "dx")
    same(mz.cpu(), nhwc(b["mz"]), "mz after the call")


# ------------------------------------------------------------------------------------------------ accumulate, then mask
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin, cout, hw", [(16, 32, (16, 16)), (128, 128, (8, 12)), (512, 512, (2, 2))])
def test_accumulate_then_mask_exact(ops, cin, cout, hw, dt):
    """g_z = leaky'(z) (g_a + relu'(z) g_r): the four-parity input gradient of the down convolution cin -> cout (g_a), plus channels
    [0, cin) of the skip buffer's 2 cin-channel gradient (r1: relu'(z) g_r, stored there by the transposed convolution), times
    LeakyReLU'(0.2) of the stored activation a = leaky(z) -- the mask applies AFTER the sum.  In the network r1 is zero wherever the mask
    is 0.2, so either order would do there; here r1 is NOT masked beforehand, so the order the epilogue promises shows"""
    name = f"unet_accmask_{cin}_{cout}_{hw[0]}x{hw[1]}"

    def build():
        g = CE.gen(name)
        dy = CE.ternary((2, cout, hw[0] // 2, hw[1] // 2), 0.5, g)
        w = CE.ternary((cout, cin, 4, 4), CE.w_density(4 * cout), g)
        a = CE.ints((2, cin, *hw), -2, 2, g)
        gr = CE.ints((2, 2 * cin, *hw), -4, 4, g)
        z = torch.zeros(2, cin, *hw, dtype=torch.float64, requires_grad=True)
        F.conv2d(z, w, None, 2, 1).backward(dy)
        za = torch.zeros(2, cin, *hw, dtype=torch.float64, requires_grad=True)
        F.conv2d(za, w.abs(), None, 2, 1).backward(dy.abs())
        return dict(dy=dy, w=w, a=a, gr=gr, pre=z.grad + gr[:, :cin], bound=za.grad + gr[:, :cin].abs())

    b, T = once(name, build), TDT[dt]
    CE.check_exact(name, dt, b["bound"], b["pre"], b["pre"], 1.0)
    dy, a, gr = nhwc(b["dy"]).to(T).cuda(), nhwc(b["a"]).to(T).cuda(), nhwc(b["gr"]).to(T).cuda()
    dx = torch.full((2, *hw, cin), SENTINEL, dtype=T, device="cuda")
    wall, step = par_packs(ops, b["w"].float().cuda(), cin, cout, T)
    with Prof() as pr:
        ops.conv_igemm(dy, wall, dx, kh=2, kw=2, Cout=cin, OH=(hw[0] + 1) // 2, OW=(hw[1] + 1) // 2, os=2, npar=4, wpar_stride=step,
                       r1=gr, r1_cend=cin, beta1=1.0, mz=a, mz_c0=0, mslope=0.2)
        torch.cuda.synchronize()
    print(f"[class] {name}-{dt}: {', '.join(pr.classes)}")
    assert pr.classes == [f"dgrad_s2k4<{DT_TAG[dt]},4 parities>"]
    want = nhwc(leaky32(b["pre"], b["a"], 0.2))
    same(dx.cpu(), want.double() if dt == "fp32" else want.to(T).double(), "dx")
    # mask-then-add would differ: the formula's order matters wherever a <= 0 and the skip's share is not zero
    other = nhwc(leaky32(b["pre"] - b["gr"][:, :cin], b["a"], 0.2) + b["gr"][:, :cin].float())
    assert not torch.equal(other, want)
    same(gr.cpu(), nhwc(b["gr"]), "the skip buffer's gradient after the call")
    same(a.cpu(), nhwc(b["a"]), "a after the call")
