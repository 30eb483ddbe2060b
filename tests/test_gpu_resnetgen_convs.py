"""Direct tests of the convolution shapes ResnetGenerator is the first network to reach (srcgan_amd.ResnetGenerator, csrc/oplist.hip
resnetgen_plan), through the C ABI alone (srcgan_conv_igemm, srcgan_conv_wgrad): the network sits on top of these calls, so a shape the
kernels mishandle shows here first.  7x7 stride 1 is a new instance of the generic implicit-GEMM kernel and of the weight-gradient
kernel (the 7x7 of ResDeconv has stride 2); 3x3 stride 1 with padding 0, and with padding 2 for its input gradient, are the
convolutions behind a materialised ReflectionPad2d(1).

Operands and float64 references are those of tests/conv_exact.py: small integers, for which every order of f32 summation gives the
same bits, compared with `torch.equal` on the WHOLE output buffer, in fp32, bf16 and fp16; the extents leave a ragged second tile in
both directions (32 columns, 8 rows):

  * 7x7, padding 0, from an image record (C = 1 and C = 3 in 8 channels, the other five / seven holding junk that the zero rows of the
    pack must cancel) to 16 and to 64 channels, with bias;
  * 7x7, padding 0, from 64 to 3 and to 1 channels inside 8-channel records (the other channels keep their sentinel), with bias;
  * their input gradients as the backward issues them: dy through the TRANSPOSED pack (rows = ci, k = co, taps flipped) at padding 6;
  * their weight gradients: one split, an uneven number and the planner's own; stored and accumulated; on NaN-filled guarded slabs;
  * 3x3, padding 0, 64 -> 64 with bias, its padding-2 input gradient, and its weight gradient with the fused bias gradient;
  * ConvTranspose2d(k3, s2, p1, output_padding 1) + bias WITHOUT the ReLU (here InstanceNorm and ReLU follow the layer).

Each 7x7 case holds the kernel class it ran (the launch profiler) against the one intended; the others print theirs."""
import pytest
import torch

import conv_exact as CE
from conv_exact import conv_case, par_case, wgrad_case, DTS, DT_TAG, TDT
from test_gpu_mdsr_convs import Prof, same
from ws_guard import NAN, guarded_slabs

pytestmark = pytest.mark.gpu

K7 = dict(k=(7, 7), pad=(0, 0), hw=(17, 45))                      # -> 11 x 39
D7 = dict(k=(7, 7), pad=(6, 6), hw=(11, 39), bias=False)          # -> 17 x 45

# (case, row tiles of 32, transposed pack, 7x7 class expected)
CONV_CASES = [
    (conv_case("rg_7x7_c1_16", cin=1, x_cs=8, cout=16, **K7), 1, False, True),
    (conv_case("rg_7x7_c3_64", cin=3, x_cs=8, cout=64, **K7), 2, False, True),
    (conv_case("rg_7x7_64_c3", cin=64, cout=3, y_cs=8, **K7), 1, False, True),
    (conv_case("rg_7x7_64_c1", cin=64, cout=1, y_cs=8, **K7), 1, False, True),
    (conv_case("rg_7x7_dgrad_16_c1", cin=16, cout=1, y_cs=8, **D7), 1, True, True),
    (conv_case("rg_7x7_dgrad_64_c3", cin=64, cout=3, y_cs=8, **D7), 1, True, True),
    (conv_case("rg_7x7_dgrad_c3_64", cin=3, x_cs=8, cout=64, **D7), 2, True, True),
    (conv_case("rg_7x7_dgrad_c1_64", cin=1, x_cs=8, cout=64, **D7), 2, True, True),
    (conv_case("rg_3x3_p0_64", cin=64, cout=64, k=(3, 3), pad=(0, 0), hw=(13, 39)), 2, False, False),
    (conv_case("rg_3x3_p0_256", cin=256, cout=256, k=(3, 3), pad=(0, 0), hw=(6, 7)), 2, False, False),
    (conv_case("rg_3x3_p2_dgrad_64", cin=64, cout=64, k=(3, 3), pad=(2, 2), hw=(11, 37), bias=False), 2, True, False),
]
WGRAD_CASES = [(wgrad_case(f"rg_7x7_wgrad_{ci}_{co}_ns{ns}_{'acc' if acc else 'store'}", cin=ci, cout=co, nsplit=ns, accumulate=acc, **K7), True)
               for ci, co in ((1, 16), (3, 64), (64, 3), (64, 1)) for ns, acc in ((1, False), (3, True), (None, False))]
WGRAD_CASES += [(wgrad_case(f"rg_3x3_p0_wgrad_64_{'acc' if acc else 'store'}", cin=64, cout=64, k=(3, 3), pad=(0, 0), hw=(13, 39), bias_grad=True,
                            accumulate=acc), False) for acc in (False, True)]
DECONV_CASES = [par_case(f"rg_deconv3_plain_{hw[0]}x{hw[1]}_{ci}_{co}", "deconv3", cin=ci, cout=co, hw=hw, bias=True, act=False)
                for hw, ci, co in (((5, 33), 64, 32), ((3, 5), 256, 128), ((9, 7), 32, 16))]
_BUILT = {}


def built(c):
    """exact operands are the same numbers in every storage type: one reference per case"""
    if c["name"] not in _BUILT:
        _BUILT[c["name"]] = {"conv": CE.build_conv, "wgrad": CE.build_wgrad, "deconv3": CE.build_par}[c["form"]](c)
    return _BUILT[c["name"]]


def _params(cases):
    return [pytest.param(*c, dt, id=f"{c[0]['name']}-{dt}") for c in cases for dt in DTS]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import ops as o
    return o


@pytest.mark.parametrize("c,mt,transposed,k7,dt", _params(CONV_CASES))
def test_resnetgen_conv_exact(ops, c, mt, transposed, k7, dt):
    b, T = built(c), TDT[dt]
    CE.check_exact(c["name"], dt, b["bound"], b["pre"], b["v"], b["ep"]["alpha"])
    x = b["x"].to(T).cuda()
    y = b["y0"].to(T).cuda()
    k = c["k"][0]
    # an image record enters with all its 8 channels, as the executor passes it (rd_walk: ti.C < 8 ? ti.cs : cin)
    kw = dict(kh=k, kw=k, stride=1, Cin=8 if c["cin"] < 8 else c["cin"], Cout=c["cout"], OH=b["OH"], OW=b["OW"], pad=c["pad"],
              bias=b["bias"].float().cuda() if b["bias"] is not None else None)
    if transposed:
        W = b["w"].permute(1, 0, 2, 3).flip(2, 3).contiguous().float().cuda()
        wp = ops.pack_conv2d_dgrad_s1(W, T)
        assert torch.equal(wp, ops.pack_conv2d_fwd(b["w"].float().cuda(), T)), "transposed pack"
    else:
        wp = ops.pack_conv2d_fwd(b["w"].float().cuda(), T)
    with Prof() as pr:
        ops.conv_igemm(x, wp, y, **kw)
        torch.cuda.synchronize()
    print(f"[class] {c['name']}-{dt}: {', '.join(pr.classes)}")
    assert len(pr.classes) == 1
    if k7:
        assert pr.classes == [f"conv_igemm<{DT_TAG[dt]},7x7,s1,MT{mt}>"]
    same(y.cpu(), b["want"], "y")
    same(x.cpu(), b["x"], "x after the call")


@pytest.mark.parametrize("c,k7,dt", _params(WGRAD_CASES))
def test_resnetgen_wgrad_exact(ops, c, k7, dt):
    b, T = built(c), TDT[dt]
    CE.check_exact(c["name"], dt, b["bound"] + 8, b["val"], b["want"], CE.F32(c["alpha"]), f32_out=True)
    x, dy = b["x"].to(T).cuda(), b["dy"].to(T).cuda()
    grad = b["grad0"].float().cuda()
    bias = b["bias0"].float().cuda() if c["bias_grad"] else None
    with guarded_slabs(NAN, "cuda") as g, Prof() as pr:           # the slab's contents on entry are unspecified
        ops.conv_wgrad(dy, x, grad, kh=c["k"][0], kw=c["k"][1], stride=1, Cout=c["cout"], Cin=c["cin"], pad=c["pad"], layout=b["layout"],
                       nsplit=c["nsplit"], accumulate=c["accumulate"], bias_grad=bias)
        torch.cuda.synchronize()
        assert g.calls == 1
    print(f"[class] {c['name']}-{dt}: {', '.join(pr.classes)}")
    if k7:
        assert pr.classes == [f"conv_wgrad<{DT_TAG[dt]},7x7,s1,MT1>"]
    same(x.cpu(), b["x"], "x after the call")
    same(dy.cpu(), b["dy"], "dy after the call")
    same(grad.cpu(), b["want"], "grad")
    if c["bias_grad"]:
        same(bias.cpu(), b["bias_want"], "bias gradient")


@pytest.mark.parametrize("c", DECONV_CASES, ids=[c["name"] for c in DECONV_CASES])
@pytest.mark.parametrize("dt", DTS)
def test_deconv3_without_the_relu_exact(ops, c, dt):
    b, T = built(c), TDT[dt]
    CE.check_exact(c["name"], dt, b["bound"], b["pre"], b["v"], b["ep"]["alpha"])
    assert bool((b["v"] < 0).any()), "no negative output: the case could not tell a fused ReLU"
    x, y = b["x"].to(T).cuda(), b["y0"].to(T).cuda()
    with Prof() as pr:
        ops.deconv3x3s2(x, b["w"].float().cuda(), b["bias"].float().cuda(), relu=False, y=y)
        torch.cuda.synchronize()
    assert pr.classes == [f"deconv_k3s2<{DT_TAG[dt]},4 parities>"]
    same(y.cpu(), b["want"], "y")
    same(x.cpu(), b["x"], "x after the call")
