"""GPU, C ABI, bit-exact: the kernels of the frozen VGG feature path (srcgan_amd/csrc/vgg_loss.hip) on small-integer data, which every
compute dtype holds exactly -- srcgan_maxpool2_nhwc / _bwd_nhwc against float64 F.max_pool2d and its autograd gradient,
srcgan_feat_loss_fwd / _bwd against float64 sums.  Padding channels [C, cs) carry a sentinel that must survive every call."""
import pytest
import torch
import torch.nn.functional as F

from srcgan_amd import _native as N

pytestmark = pytest.mark.gpu

DTYPES = [("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)]
POOL_SHAPES = [(1, 2, 2, 8, 8), (2, 5, 7, 64, 64), (1, 6, 9, 136, 144)]       # B, H, W, C, channel stride
SENTINEL = 77.0


def _records(x_nchw, cs, td):
    """[B,C,H,W] float64 -> device NHWC records of stride cs, padding channels = SENTINEL"""
    B, C, H, W = x_nchw.shape
    buf = torch.full((B, H, W, cs), SENTINEL, dtype=td)
    buf[..., :C] = x_nchw.permute(0, 2, 3, 1).to(td)
    return buf.cuda()


def _nchw(buf, C):
    return buf[..., :C].permute(0, 3, 1, 2).double().cpu()


def _pool_input(B, H, W, C, seed, nonneg=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B, C, H, W), generator=g).double()
    for p in range(4):                                  # window (0, 0), channel p: equal maxima at positions p .. 3 -> the first one, p, wins
        w = torch.full((4,), -3.0)
        w[p:] = 3.0
        x[:, p, 0:2, 0:2] = w.reshape(2, 2)
    x[:, 4, 0:2, 0:2] = 0.0                             # all-zero window
    x[:, 5, 0:2, 0:2] = torch.tensor([[-1.0, -2.0], [-3.0, -1.0]])       # negative-only window with a tie
    return x.clamp_min(0) if nonneg else x


def _run_pool(x, dy, cs, dname, td, relu_mask):
    lib, dt = N.lib(), N.dtype_id(dname)
    B, C, H, W = x.shape
    xb, dyb = _records(x, cs, td), _records(dy, cs, td)
    yb = torch.full((B, H // 2, W // 2, cs), SENTINEL, dtype=td, device="cuda")
    dxb = torch.full((B, H, W, cs), SENTINEL, dtype=td, device="cuda")
    st = N.stream_ptr()
    N.check(lib.srcgan_maxpool2_nhwc(xb.data_ptr(), cs, yb.data_ptr(), cs, B, H, W, C, dt, st), "srcgan_maxpool2_nhwc")
    N.check(lib.srcgan_maxpool2_bwd_nhwc(dyb.data_ptr(), cs, xb.data_ptr(), cs, dxb.data_ptr(), cs, B, H, W, C, relu_mask, dt, st), "srcgan_maxpool2_bwd_nhwc")
    torch.cuda.synchronize()
    for buf in (yb, dxb):
        assert bool((buf[..., C:] == SENTINEL).all()), "padding channels were written"
    return _nchw(yb, C), _nchw(dxb, C), yb, dxb


@pytest.mark.parametrize("dname,td", DTYPES)
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_forward_and_backward_are_exact(dname, td, shape):
    B, H, W, C, cs = shape
    x = _pool_input(B, H, W, C, seed=H * W)
    dy = torch.randint(-4, 5, (B, C, H // 2, W // 2), generator=torch.Generator().manual_seed(1)).double()
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    yr.backward(dy)
    y, dx, yb, dxb = _run_pool(x, dy, cs, dname, td, 0)
    assert torch.equal(y, yr.detach())
    assert torch.equal(dx, xr.grad)
    assert bool((dx[:, :, 2 * (H // 2):, :] == 0).all()) and bool((dx[:, :, :, 2 * (W // 2):] == 0).all())      # the dropped odd row / column
    # relu_mask = 1 on the same (signed) data: the gradient survives only where the window's maximum is > 0
    _, dxm, _, _ = _run_pool(x, dy, cs, dname, td, 1)
    assert torch.equal(dxm, xr.grad * (x > 0))
    assert bool((dxm[:, 5, 0:2, 0:2] == 0).all()) and bool((dxm[:, 4, 0:2, 0:2] == 0).all())
    # two runs, identical bits
    _, _, yb2, dxb2 = _run_pool(x, dy, cs, dname, td, 0)
    assert torch.equal(yb.view(torch.uint8), yb2.view(torch.uint8)) and torch.equal(dxb.view(torch.uint8), dxb2.view(torch.uint8))


@pytest.mark.parametrize("dname,td", DTYPES)
def test_maxpool_backward_with_relu_mask_is_autograd_through_relu(dname, td):
    """x = relu(z) is what the forward stored; relu_mask = 1 gives d / dz of max_pool2d(relu(z))"""
    B, H, W, C, cs = 2, 5, 7, 64, 64
    z = _pool_input(B, H, W, C, seed=5).requires_grad_(True)
    dy = torch.randint(-4, 5, (B, C, H // 2, W // 2), generator=torch.Generator().manual_seed(2)).double()
    F.max_pool2d(F.relu(z), 2, 2).backward(dy)
    _, dx, _, _ = _run_pool(z.detach().clamp_min(0), dy, cs, dname, td, 1)
    assert torch.equal(dx, z.grad)


FEAT_SHAPES = [(37, 13, 16), (37, 13, 13), (300, 64, 64), (5, 136, 144)]       # npix, C, channel stride


def _feat_inputs(npix, C, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (1, C, npix, 1), generator=g).double()
    b = torch.randint(-3, 4, (1, C, npix, 1), generator=g).double()
    b[:, ::3] = a[:, ::3]                               # a == b: gradient 0 (sign(0) = 0)
    return a, b


@pytest.mark.parametrize("dname,td", DTYPES)
@pytest.mark.parametrize("shape", FEAT_SHAPES)
@pytest.mark.parametrize("kind", [0, 1])
def test_feat_loss_forward_and_backward_are_exact(dname, td, shape, kind):
    lib, dt = N.lib(), N.dtype_id(dname)
    npix, C, cs = shape
    a, b = _feat_inputs(npix, C, seed=npix + C)
    ab, bb = _records(a, cs, td), _records(b, cs, td)
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.srcgan_loss_scratch_floats(), dtype=torch.float32, device="cuda")
    st = N.stream_ptr()
    for k in range(2):
        N.check(lib.srcgan_feat_loss_fwd(kind, ab.data_ptr(), cs, bb.data_ptr(), cs, npix, C, dt, out[k:].data_ptr(), scratch.data_ptr(), st), "srcgan_feat_loss_fwd")
    d = a - b
    want = float(d.abs().sum() if kind == 0 else (d * d).sum())
    got = out.cpu()
    assert float(got[0]) == want and float(got[1]) == want
    grad = 0.5 * (torch.sign(d) if kind == 0 else 2 * d)
    g0 = torch.randint(-2, 3, a.shape, generator=torch.Generator().manual_seed(3)).double()
    for accumulate in (0, 1):
        gb = _records(g0, cs, td)
        N.check(lib.srcgan_feat_loss_bwd(kind, ab.data_ptr(), cs, bb.data_ptr(), cs, gb.data_ptr(), cs, accumulate, 0.5, npix, C, dt, st), "srcgan_feat_loss_bwd")
        torch.cuda.synchronize()
        assert bool((gb[..., C:] == SENTINEL).all()), "padding channels were written"
        assert torch.equal(_nchw(gb, C), grad + (g0 if accumulate else 0))
    assert bool((grad[:, ::3] == 0).all())


def test_feat_loss_forward_is_deterministic_on_real_data():
    lib = N.lib()
    npix, C = 4099, 72
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(npix, C, generator=g).cuda(), torch.randn(npix, C, generator=g).cuda()
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.srcgan_loss_scratch_floats(), dtype=torch.float32, device="cuda")
    for k in range(2):
        N.check(lib.srcgan_feat_loss_fwd(0, a.data_ptr(), C, b.data_ptr(), C, npix, C, N.F32, out[k:].data_ptr(), scratch.data_ptr(), N.stream_ptr()), "srcgan_feat_loss_fwd")
    got = out.cpu()
    assert got[0].view(torch.int32) == got[1].view(torch.int32)
    ref = float((a.double() - b.double()).abs().sum())
    assert abs(float(got[0]) - ref) <= 1e-5 * ref       # f32 partial sums of ~1e3 terms each: far inside 1e-5
