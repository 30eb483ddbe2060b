"""Direct tests of the convolution regime MDSR is the first network to reach (srcgan_amd.MDSR, csrc/oplist.hip mdsr_plan): 5x5, stride 1,
64 -> 64 -- several K chunks on the 64-row tile of the generic implicit-GEMM kernel -- through the C ABI alone (srcgan_conv_igemm,
srcgan_conv_wgrad, srcgan_col_reduce): the network sits on top of these calls, so a shape the kernels mishandle shows here first.
ESPCN.conv1 and SRCNN.conv3 reach 5x5 only with one K chunk or with Cout <= 32.

Operands and float64 references are those of tests/conv_exact.py: small integers, for which every order of f32 summation gives the
same bits, compared with `torch.equal` on the WHOLE output buffer, in fp32, bf16 and fp16, on 2 x 11 x 37 images (two 32-pixel tile
columns, the second ragged; two 8-row tiles, the second ragged):

  * the first convolution of a 5x5 ResBlock: 64 -> 64 with bias and ReLU;
  * the second: bias, alpha and a residual r1 (the block's input); a 96-channel r1 buffer, so the residual is a prefix of a wider tensor;
  * 32 -> 32, the 32-row tile (n_feats = 32, the fixtures' width);
  * the input gradient as the backward issues it: dy through the TRANSPOSED pack (rows = ci, k = co, taps flipped) at padding
    k - 1 - pad, the ReLU' mask mz of the stored activation, r1 aliasing y (the gradient already there is added in place) -- and its
    first-writer form without r1;
  * the weight gradient 64 x 64 and 32 x 32: one split, an uneven number of splits and the planner's own; stored into a sentinel-filled
    tensor and accumulated onto integers; on NaN-filled guarded slabs;
  * the bias gradient through the path the executor takes for kernels other than 3x3 (srcgan_col_reduce; the fused one is 3x3 only).

Each case records the kernel class it ran (the launch profiler, as tests/test_gpu_conv_exact.py does) and holds it against the one
intended."""
import ctypes as C

import pytest
import torch

import conv_exact as CE
from conv_exact import conv_case, wgrad_case, DTS, DT_TAG, TDT
from ws_guard import NAN, guarded_slabs

pytestmark = pytest.mark.gpu

HW = (11, 37)
K5 = dict(k=(5, 5), pad=(2, 2), hw=HW)

CONV_CASES = [
    (conv_case("mdsr_5x5_64_relu", cin=64, cout=64, act=True, slope=0.0, **K5), 2, False),
    (conv_case("mdsr_5x5_64_res", cin=64, cout=64, alpha=0.5, r1="own", r1_cs=96, beta1=1.0, **K5), 2, False),
    (conv_case("mdsr_5x5_32_relu", cin=32, cout=32, act=True, slope=0.0, **K5), 1, False),
    (conv_case("mdsr_5x5_32_res", cin=32, cout=32, r1="own", beta1=1.0, **K5), 1, False),
    (conv_case("mdsr_5x5_64_dgrad", cin=64, cout=64, bias=False, r1="y", beta1=1.0, mz=True, mslope=0.0, **K5), 2, True),
    (conv_case("mdsr_5x5_64_dgrad_first", cin=64, cout=64, bias=False, mz=True, mslope=0.0, **K5), 2, True),
    (conv_case("mdsr_5x5_32_dgrad", cin=32, cout=32, bias=False, r1="y", beta1=1.0, mz=True, mslope=0.0, **K5), 1, True),
]
WGRAD_CASES = [(wgrad_case(f"mdsr_5x5_wgrad_{c}_ns{ns}_{'acc' if acc else 'store'}", cin=c, cout=c, nsplit=ns, accumulate=acc, **K5), mt)
               for c, mt in ((64, 2), (32, 1)) for ns in (1, 3, None) for acc in (False, True)]
_BUILT = {}


def built(c):
    """exact operands are the same numbers in every storage type: one reference per case"""
    if c["name"] not in _BUILT:
        _BUILT[c["name"]] = CE.build_conv(c) if c["form"] == "conv" else CE.build_wgrad(c)
    return _BUILT[c["name"]]


def _params(cases):
    return [pytest.param(*c, dt, id=f"{c[0]['name']}-{dt}") for c in cases for dt in DTS]


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


class Prof:
    """records the kernel classes launched inside the block"""

    def __enter__(self):
        from srcgan_amd import _native as N
        N.prof_enable(True)
        N.prof_collect()
        return self

    def __exit__(self, et, ev, tb):
        from srcgan_amd import _native as N
        self.classes = [r["cls"] for r in N.prof_collect()]
        N.prof_enable(False)
        return False


@pytest.mark.parametrize("c,mt,transposed,dt", _params(CONV_CASES))
def test_mdsr_conv_exact(ops, c, mt, transposed, dt):
    b, T = built(c), TDT[dt]
    CE.check_exact(c["name"], dt, b["bound"], b["pre"], b["v"], b["ep"]["alpha"])
    x = b["x"].to(T).cuda()
    y = b["y0"].to(T).cuda()
    kw = dict(kh=5, kw=5, stride=1, Cin=c["cin"], Cout=c["cout"], OH=b["OH"], OW=b["OW"], pad=c["pad"], alpha=c["alpha"],
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
    if transposed:
        # the case's weight [rows][k][ty][tx] is the input-gradient view of the Conv2d weight W[co = k][ci = rows][4 - ty][4 - tx]: the
        # backward packs W through the transposed layout, and that pack must be the forward pack of the view
        W = b["w"].permute(1, 0, 2, 3).flip(2, 3).contiguous().float().cuda()
        wp = ops.pack_conv2d_dgrad_s1(W, T)
        assert torch.equal(wp, ops.pack_conv2d_fwd(b["w"].float().cuda(), T)), "transposed pack"
    else:
        wp = ops.pack_conv2d_fwd(b["w"].float().cuda(), T)
    with Prof() as pr:
        ops.conv_igemm(x, wp, y, **kw)
        torch.cuda.synchronize()
    print(f"[class] {c['name']}-{dt}: {', '.join(pr.classes)}")
    assert pr.classes == [f"conv_igemm<{DT_TAG[dt]},5x5,s1,MT{mt}>"]
    same(y.cpu(), b["want"], "y")
    same(x.cpu(), b["x"], "x after the call")
    for name, (t, ref) in keep.items():
        same(t.cpu(), ref, name + " after the call")


@pytest.mark.parametrize("c,mt,dt", _params(WGRAD_CASES))
def test_mdsr_wgrad_exact(ops, c, mt, dt):
    from srcgan_amd import _native as N
    b, T = built(c), TDT[dt]
    CE.check_exact(c["name"], dt, b["bound"] + 8, b["val"], b["want"], CE.F32(c["alpha"]), f32_out=True)
    x, dy = b["x"].to(T).cuda(), b["dy"].to(T).cuda()
    grad = b["grad0"].float().cuda()
    planned = N.lib().srcgan_conv_wgrad_nsplit(2, HW[0], HW[1], c["cout"], c["cin"], 1)
    assert planned == 8          # 2 images x 2 row tiles x 2 tile columns: the planner's own split count is above 1 and uneven against 3
    with guarded_slabs(NAN, "cuda") as g, Prof() as pr:           # the slab's contents on entry are unspecified
        ops.conv_wgrad(dy, x, grad, kh=5, kw=5, stride=1, Cout=c["cout"], Cin=c["cin"], pad=c["pad"], layout=b["layout"], nsplit=c["nsplit"],
                       accumulate=c["accumulate"])
        torch.cuda.synchronize()
        assert g.calls == 1
    print(f"[class] {c['name']}-{dt}: {', '.join(pr.classes)}")
    assert pr.classes == [f"conv_wgrad<{DT_TAG[dt]},5x5,s1,MT{mt}>"]
    same(x.cpu(), b["x"], "x after the call")
    same(dy.cpu(), b["dy"], "dy after the call")
    same(grad.cpu(), b["want"], "grad")


@pytest.mark.parametrize("cout", [64, 32])
@pytest.mark.parametrize("dt", DTS)
def test_mdsr_bias_gradient_through_the_column_reduce(ops, dt, cout):
    """srcgan_conv_wgrad fuses the bias gradient for 3x3 kernels only (and says so); for the 5x5 convolutions the executor sums dy over
    the pixels with srcgan_col_reduce.  Integers: bit-equal to float64, dy a channel slice of a wider buffer."""
    from srcgan_amd import _native as N
    g = CE.gen(f"mdsr_5x5_bias_{cout}")
    dy = CE.ints((2, HW[0], HW[1], cout + 32), -4, 4, g)
    want = dy[..., 32:].sum((0, 1, 2))
    got = ops.col_sum(dy.to(TDT[dt]).cuda(), cout, 32)
    torch.cuda.synchronize()
    same(got.cpu(), want, "bias gradient")
    d = N.WgradDesc()
    x = torch.zeros(2, HW[0], HW[1], cout, dtype=TDT[dt], device="cuda")
    slab, grad = torch.empty(1 << 20, dtype=torch.uint8, device="cuda"), torch.empty(cout * cout * 25, device="cuda")
    d.dy, d.x, d.slab, d.grad, d.bias_grad = x.data_ptr(), x.data_ptr(), slab.data_ptr(), grad.data_ptr(), got.data_ptr()
    d.dtype, d.kh, d.kw, d.stride, d.nsplit = N.dtype_id(TDT[dt]), 5, 5, 1, 1
    d.B, d.H, d.W, d.Cin, d.x_cs, d.OH, d.OW, d.Cout, d.dy_cs, d.pad_y, d.pad_x = 2, HW[0], HW[1], cout, cout, HW[0], HW[1], cout, cout, 2, 2
    assert N.lib().srcgan_conv_wgrad(C.byref(d), None) != 0 and b"3x3 kernels only" in N.lib().srcgan_last_error()
