"""Direct tests of the convolution shapes RDN brings (srcgan_amd.RDN, csrc/oplist.hip rdn_plan), through the C ABI alone
(srcgan_conv_igemm, srcgan_conv_wgrad): the network sits on top of these calls, so a shape the kernels mishandle shows here first.

Operands and float64 references are those of tests/conv_exact.py: small integers, for which every order of f32 summation gives the
same bits, compared with `torch.equal` on the WHOLE output buffer (the channels beside the written slice and the operand buffers must
survive), in fp32, bf16 and fp16, on 2 x 9 x 7 images.  With (G0, G, C) = (64, 32, 6) ('A') and (64, 64, 8) ('B'):

  * a dense layer c, 3x3, G0 + c G -> G: reads the prefix of the block's buffer, writes the slice at G0 + c G with bias and ReLU;
  * its input gradient, G -> G0 + c G: added in place to the prefix, under ReLU' from channel G0 on (the prefix below G0 is the block's
    input, a plain sum); layer 0's has nothing to mask;
  * its weight gradient with the fused bias gradient, both operands slices of the wide buffers;
  * the LFF, 1x1, G0 + C G -> G0: r1 is the prefix of ANOTHER wide tensor, y the prefix of a third; its input gradient G0 -> G0 + C G
    is the first writer of the gradient buffer, with dy itself as r1 on the first G0 channels and the mask from G0 on;
  * a GFF slice, 1x1, G0 -> G0 with the accumulator as r1; its input gradient added in place to the prefix of a wide buffer."""
import pytest
import torch

import conv_exact as CE
from conv_exact import conv_case, wgrad_case, DTS, TDT
from ws_guard import NAN, guarded_slabs

pytestmark = pytest.mark.gpu

HW = (9, 7)
CONFIGS = [(64, 32, 6, (0, 5)), (64, 64, 8, (0, 7))]           # (G0, G, C, the layers tested)


def _cases():
    conv, wgrad = [], []
    for G0, G, C, layers in CONFIGS:
        Cb, t = G0 + C * G, f"g{G}"
        for c in layers:
            cin = G0 + c * G
            conv.append(conv_case(f"rdn_{t}_layer{c}", cin=cin, cout=G, hw=HW, y_in_x=True, x_cs=Cb, y_coff=cin, act=True, slope=0.0))
            kw = dict(mz=True, mz_c0=G0, mz_cs=Cb, mslope=0.0) if c else {}
            conv.append(conv_case(f"rdn_{t}_layer{c}_dgrad", cin=G, x_coff=cin, x_cs=Cb, cout=cin, hw=HW, y_in_x=True, bias=False, r1="y", r1_cend=cin,
                                  beta1=1.0, **kw))
            wgrad.append(wgrad_case(f"rdn_{t}_layer{c}_wgrad", cin=cin, cout=G, hw=HW, x_cs=Cb, dy_coff=cin, dy_cs=Cb, bias_grad=True))
        conv.append(conv_case(f"rdn_{t}_lff", k=(1, 1), pad=(0, 0), cin=Cb, cout=G0, hw=HW, y_cs=Cb, r1="own", r1_cs=Cb, r1_cend=G0, beta1=1.0))
        conv.append(conv_case(f"rdn_{t}_lff_dgrad", k=(1, 1), pad=(0, 0), cin=G0, cout=Cb, hw=HW, bias=False, r1="own", r1_cs=G0, r1_cend=G0, beta1=1.0,
                              mz=True, mz_c0=G0, mslope=0.0))
        wgrad.append(wgrad_case(f"rdn_{t}_lff_wgrad", k=(1, 1), pad=(0, 0), cin=Cb, cout=G0, hw=HW))
    conv.append(conv_case("rdn_gff_slice", k=(1, 1), pad=(0, 0), cin=64, x_cs=256, cout=64, hw=HW, r1="own", beta1=1.0))
    conv.append(conv_case("rdn_gff_slice_nobias", k=(1, 1), pad=(0, 0), cin=64, cout=64, hw=HW, bias=False, r1="own", beta1=1.0))
    conv.append(conv_case("rdn_gff_slice_dgrad", k=(1, 1), pad=(0, 0), cin=64, cout=64, hw=HW, y_cs=256, bias=False, r1="y", beta1=1.0))
    return conv, wgrad


CONV_CASES, WGRAD_CASES = _cases()
_BUILT = {}


def built(c):
    """exact operands are the same numbers in every storage type: one reference per case"""
    if c["name"] not in _BUILT:
        _BUILT[c["name"]] = CE.build_conv(c) if c["form"] == "conv" else CE.build_wgrad(c)
    return _BUILT[c["name"]]


def _params(cases):
    return [pytest.param(c, dt, id=f"{c['name']}-{dt}") for c in cases for dt in DTS]


def same(got, want64, what):
    want = want64.to(got.dtype)
    if not torch.equal(got, want):
        d = got.double() != want.double()
        idx = d.nonzero()
        raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} elements differ; first at {idx[0].tolist()}: got {float(got[tuple(idx[0])])}, "
                             f"want {float(want[tuple(idx[0])])}; max |diff| {float((got.double() - want.double())[d].abs().max())}")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import ops as o
    return o


@pytest.mark.parametrize("c,dt", _params(CONV_CASES))
def test_rdn_conv_exact(ops, c, dt):
    b, T = built(c), TDT[dt]
    CE.check_exact(c["name"], dt, b["bound"], b["pre"], b["v"], b["ep"]["alpha"])
    x = b["x"].to(T).cuda()
    y = x if c["y_in_x"] else b["y0"].to(T).cuda()
    kw = dict(kh=c["k"][0], kw=c["k"][1], stride=1, Cin=c["cin"], x_coff=c["x_coff"], Cout=c["cout"], y_coff=c["y_coff"], OH=b["OH"], OW=b["OW"], pad=c["pad"],
              bias=b["bias"].float().cuda() if b["bias"] is not None else None, act=c["act"], slope=c["slope"], mslope=c["mslope"])
    keep = {}
    if c["r1"] == "y":
        kw.update(r1=y, r1_coff=b["r1_coff"], r1_cend=b["r1_cend"], beta1=c["beta1"])
    elif c["r1"]:
        keep["r1"] = (b["r1"].to(T).cuda(), b["r1"])
        kw.update(r1=keep["r1"][0], r1_coff=b["r1_coff"], r1_cend=b["r1_cend"], beta1=c["beta1"])
    if c["mz"]:
        keep["mz"] = (b["mz"].to(T).cuda(), b["mz"])
        kw.update(mz=keep["mz"][0], mz_coff=c["mz_coff"], mz_c0=c["mz_c0"])
    ops.conv_igemm(x, ops.pack_conv2d_fwd(b["w"].float().cuda(), T), y, **kw)
    torch.cuda.synchronize()
    same(y.cpu(), b["want"], "y")
    if not c["y_in_x"]:
        same(x.cpu(), b["x"], "x after the call")
    for name, (t, ref) in keep.items():
        same(t.cpu(), ref, name + " after the call")


@pytest.mark.parametrize("c,dt", _params(WGRAD_CASES))
def test_rdn_wgrad_exact(ops, c, dt):
    b, T = built(c), TDT[dt]
    CE.check_exact(c["name"], dt, b["bound"] + 8, b["val"], b["want"], CE.F32(c["alpha"]), f32_out=True)
    x, dy = b["x"].to(T).cuda(), b["dy"].to(T).cuda()
    grad = b["grad0"].float().cuda()
    gb = b["bias0"].float().cuda() if c["bias_grad"] else None
    with guarded_slabs(NAN, "cuda") as g:           # the slab's contents on entry are unspecified
        ops.conv_wgrad(dy, x, grad, kh=c["k"][0], kw=c["k"][1], stride=1, Cout=c["cout"], Cin=c["cin"], dy_coff=c["dy_coff"], x_coff=c["x_coff"], pad=c["pad"],
                       layout=b["layout"], accumulate=False, bias_grad=gb)
        torch.cuda.synchronize()
        assert g.calls == 1
    same(x.cpu(), b["x"], "x after the call")
    same(dy.cpu(), b["dy"], "dy after the call")
    same(grad.cpu(), b["want"], "grad")
    if gb is not None:
        same(gb.cpu(), b["bias_want"], "bias_grad")
