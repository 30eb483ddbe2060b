"""GPU: the multi-frame losses L1Loss3D, DSSIMLoss3D and VGG16Loss3D on [nb,ch,frame,row,col] tensors.

L1 / DSSIM: the reference's fixture (tests/golden/losses3d.npz, gates of test_gpu_dssim.py::test_golden_parity), and the structure the
shared device code promises -- the gradient of frame f has the bits of the 2-D DSSIMLoss of that frame at upstream 1 / F, F = 1 is the 2-D
loss, two calls give the same bits, frames that start past 2^31 bytes are addressed in 64 bits.  VGG16Loss3D: the float64 restatement of
tests/losses3d_ref.py at the gates of test_gpu_vgg_loss.py (F32_TOL; 16-bit: 1.5 x the storage emulation's error + 5e-3), chunked against
unchunked, no_grad, and the peak memory of the chunked pass against a bound made of the library's own size functions.
tests/test_losses3d_teeth.py shows what the fixture comparison notices."""
import ctypes as C
import functools

import pytest
import torch

import losses3d_ref as L
import vgg_ref as R
from conftest import load_golden, rel_err
from net_checks import F32_TOL, bound16

pytestmark = pytest.mark.gpu

CASES = ["mixed_ranges", "tiles", "single_window", "strip"]
VGG_SHAPES = [(2, 3, 2, 20, 28), (1, 1, 3, 32, 32)]          # pools floor 5x7 -> 2x3, H*W a multiple of 4; gray replication, F = 3
STORE = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _crit(key):
    from srcgan_amd import L1Loss3D, DSSIMLoss3D
    return {"l1": L1Loss3D, "dssim": DSSIMLoss3D}[key]()


def _native(crit, x, t, target_grad=True, scale=None):
    """-> (loss, dx, dt) on the device; dt is None when the target does not require grad."""
    x = x.detach().clone().requires_grad_(True)
    t = t.detach().clone().requires_grad_(target_grad)
    loss = crit(x, t)
    (loss if scale is None else loss * scale).backward()
    return loss.detach(), x.grad, t.grad


def _fixture(case):
    g = load_golden("losses3d")
    return g, torch.from_numpy(g[f"{case}/x"]).float().cuda(), torch.from_numpy(g[f"{case}/t"]).float().cuda()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ L1Loss3D / DSSIMLoss3D
@pytest.mark.parametrize("key", ["dssim", "l1"])
@pytest.mark.parametrize("case", CASES)
def test_golden_parity(case, key):
    g, x, t = _fixture(case)
    loss, dx, dt = _native(_crit(key), x, t)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    e = abs(float(loss) - float(g[f"{case}/{key}/loss"])), rel_err(dx.cpu(), g[f"{case}/{key}/dx"]), rel_err(dt.cpu(), g[f"{case}/{key}/dt"])
    print(f"{case} {key}: |loss - fixture| {e[0]:.3e}, dx {e[1]:.3e}, dt {e[2]:.3e}")
    assert e[0] < 1e-5
    assert e[1] < 1e-3
    assert e[2] < 1e-3
    # the dx-only variant (target without grad) gives the same input gradient
    _, dx1, dt1 = _native(_crit(key), x, t, target_grad=False)
    assert dt1 is None
    assert rel_err(dx1.cpu(), dx.cpu()) < 1e-5


def test_frame_gradients_have_the_bits_of_the_2d_loss():
    """mixed_ranges, F = 4 (1 / F exact): dx[:, :, f] and dt[:, :, f] are the 2-D DSSIMLoss of the contiguous copy of frame f,
    backpropagated from loss * 0.25 -- with that frame's own range -- and the loss is the mean of the per-frame losses."""
    from srcgan_amd import DSSIMLoss
    _, x, t = _fixture("mixed_ranges")
    loss, dx, dt = _native(_crit("dssim"), x, t)
    per = []
    for f in range(x.shape[2]):
        lf, dxf, dtf = _native(DSSIMLoss(), x[:, :, f].contiguous(), t[:, :, f].contiguous(), scale=0.25)
        per.append(float(lf))
        assert _bits(dx[:, :, f], dxf), f
        assert _bits(dt[:, :, f], dtf), f
    mean = sum(per) / len(per)
    assert abs(float(loss) - mean) <= 1e-6 * abs(mean)


@pytest.mark.parametrize("case", ["tiles", "strip"])
def test_one_frame_is_the_2d_loss(case):
    from srcgan_amd import DSSIMLoss
    _, x, t = _fixture(case)
    x2, t2 = x[:, :, 1].contiguous(), t[:, :, 1].contiguous()
    loss, dx, dt = _native(_crit("dssim"), x2.unsqueeze(2), t2.unsqueeze(2))
    l2, dx2, dt2 = _native(DSSIMLoss(), x2, t2)
    assert _bits(loss, l2)
    assert _bits(dx[:, :, 0], dx2) and _bits(dt[:, :, 0], dt2)


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_vgg_one_frame_is_the_2d_loss(dname):
    """VGG16Loss on [2,3,20,28] and VGG16Loss3D on the same data as [2,3,1,20,28] reach one native path: the same bits."""
    from srcgan_amd import VGG16Loss, VGG16Loss3D
    sd, out, tgt, _, _ = L.case(VGG_SHAPES[0])
    o2, t2 = out[:, :, 0].contiguous().cuda(), tgt[:, :, 0].contiguous().cuda()
    got = []
    for crit, o, t in ((VGG16Loss(weights=sd, dtype=dname), o2, t2), (VGG16Loss3D(weights=sd, dtype=dname), o2.unsqueeze(2), t2.unsqueeze(2))):
        o = o.clone().requires_grad_(True)
        loss = crit(o, t)
        loss.backward()
        with torch.no_grad():
            got.append((loss.detach(), o.grad, crit(o, t)))
    (l2, dx2, n2), (l3, dx3, n3) = got
    assert tuple(dx2.shape) == (2, 3, 20, 28) and tuple(dx3.shape) == (2, 3, 1, 20, 28)
    assert _bits(l3, l2) and _bits(dx3[:, :, 0], dx2) and _bits(n3, n2)


def test_deterministic():
    _, x, t = _fixture("mixed_ranges")           # B = 2, C = 3, F = 4, every frame different
    a, b = _native(_crit("dssim"), x, t), _native(_crit("dssim"), x, t)
    for u, v in zip(a, b):
        assert _bits(u, v)


def test_other_float_dtypes_compute_in_f32():
    _, x, t = _fixture("tiles")
    for key in ("dssim", "l1"):
        loss, dx, dt = _native(_crit(key), x.half(), t.bfloat16())
        l32, dx32, dt32 = _native(_crit(key), x.half().float(), t.bfloat16().float())
        assert loss.dtype == torch.float32 and torch.equal(loss, l32)
        assert dx.dtype == torch.float16 and dt.dtype == torch.bfloat16
        assert torch.equal(dx, dx32.half()) and torch.equal(dt, dt32.bfloat16())


def test_non_contiguous_stack_takes_the_contiguous_copy():
    _, x, t = _fixture("tiles")
    xp = x.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)          # same values, frame-major memory
    assert not xp.is_contiguous()
    a, b = _native(_crit("dssim"), xp, t), _native(_crit("dssim"), x, t)
    for u, v in zip(a, b):
        assert _bits(u, v)


def test_beyond_2g_bytes_per_frame():
    """1 x 1 x 2 x 23171 x 23171 f32: one frame is 2^31 + 97316 bytes, so frame 1 starts past 2^31 bytes.  Its gradient has the bits of
    the 2-D loss on that frame."""
    from srcgan_amd import DSSIMLoss
    n = 23171
    assert n * n > 2 ** 29
    g = torch.Generator(device="cuda").manual_seed(5)
    t = torch.rand((1, 1, 2, n, n), device="cuda", generator=g)
    x = torch.randn((1, 1, 2, n, n), device="cuda", generator=g).mul_(0.1).add_(t).clamp_(0, 1)
    x[:, :, 0].mul_(255)                           # frame 0 in 0..255: a range read from the wrong frame would show
    x.requires_grad_(True)
    loss = _crit("dssim")(x, t)
    loss.backward()
    dx1 = x.grad[:, :, 1].clone()
    x.grad = None
    x1 = x.detach()[:, :, 1].clone().requires_grad_(True)
    l1 = DSSIMLoss()(x1, t[:, :, 1].contiguous())
    (l1 * 0.5).backward()
    assert _bits(dx1, x1.grad)
    assert float(dx1.abs().max()) > 0


def test_gradient_into_a_generator():
    """one backward() through DSSIMLoss3D of torch.stack(generator outputs, dim=2) against the per-frame composition of the 2-D loss"""
    from srcgan_amd import RDDBNet, DSSIMLoss
    torch.manual_seed(0)
    net = RDDBNet(3, 3, 2, nb=1, dtype="fp32").cuda()
    xs = [torch.rand(2, 3, 24, 20, device="cuda") for _ in range(3)]
    t = torch.rand(2, 3, 3, 48, 40, device="cuda")
    _crit("dssim")(torch.stack([net(x) for x in xs], dim=2), t).backward()
    got = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    (sum(DSSIMLoss()(net(x), t[:, :, f].contiguous()) for f, x in enumerate(xs)) / 3).backward()
    for k, p in net.named_parameters():
        assert float(got[k].abs().max()) > 0, k
        e = float((got[k].double() - p.grad.double()).norm() / p.grad.double().norm())
        assert e < 1e-5, (k, e)


# ------------------------------------------------------------------------------------------------ VGG16Loss3D
def _vgg(sd, dtype, **kw):
    from srcgan_amd import VGG16Loss3D
    return VGG16Loss3D(weights=sd, dtype=dtype, **kw)


def _vgg_native(shape, dtype, **kw):
    sd, out, tgt, _, _ = L.case(shape)
    o = out.cuda().requires_grad_(True)
    loss = _vgg(sd, dtype, **kw)(o, tgt.cuda())
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    assert o.grad.shape == out.shape
    return float(loss.detach()), o.grad.cpu()


@functools.lru_cache(maxsize=None)
def _emulated(shape, dname):
    """(loss error, gradient error) against float64 of the float64 composition that stores in the 16-bit dtype"""
    sd, out, tgt, loss, grad = L.case(shape)
    return R.errors(*L.vgg16_3d(out, tgt, sd, store=STORE[dname]), loss, grad)


@pytest.mark.parametrize("shape", VGG_SHAPES)
def test_vgg_fp32_loss_and_gradient_vs_float64(shape):
    _, _, _, loss, grad = L.case(shape)
    e_loss, e_grad = R.errors(*_vgg_native(shape, "fp32"), loss, grad)
    print(f"{shape} fp32: loss error {e_loss:.3e}, gradient error {e_grad:.3e}")
    assert e_loss <= F32_TOL and e_grad <= F32_TOL


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", VGG_SHAPES)
def test_vgg_16bit_loss_and_gradient_vs_storage_emulation(shape, dname):
    _, _, _, loss, grad = L.case(shape)
    f_loss, f_grad = _emulated(shape, dname)
    e_loss, e_grad = R.errors(*_vgg_native(shape, dname), loss, grad)
    print(f"{shape} {dname}: loss error {e_loss:.3e} (emulation {f_loss:.3e}), gradient error {e_grad:.3e} (emulation {f_grad:.3e})")
    assert e_loss <= bound16(f_loss) and e_grad <= bound16(f_grad)


@pytest.mark.parametrize("shape", VGG_SHAPES)
def test_vgg_chunked_agrees_with_one_pass(shape):
    l1, g1 = _vgg_native(shape, "fp32", frames_per_pass=1)
    la, ga = _vgg_native(shape, "fp32")
    assert abs(l1 - la) <= 1e-6 * abs(la)
    assert float((g1.double() - ga.double()).norm() / ga.double().norm()) <= 1e-6
    if shape[2] == 3:            # a last chunk shorter than the others
        l2, g2 = _vgg_native(shape, "fp32", frames_per_pass=2)
        assert abs(l2 - la) <= 1e-6 * abs(la)
        assert float((g2.double() - ga.double()).norm() / ga.double().norm()) <= 1e-6


@pytest.mark.parametrize("fpp", [None, 1])
def test_vgg_no_grad_gives_the_same_loss(fpp):
    sd, out, tgt, _, _ = L.case(VGG_SHAPES[1])
    m = _vgg(sd, "fp32", frames_per_pass=fpp)
    o, t = out.cuda(), tgt.cuda()
    with torch.no_grad():
        l0 = m(o, t)
    l1 = m(o.clone().requires_grad_(True), t)
    assert not l0.requires_grad and l1.requires_grad
    assert abs(float(l0) - float(l1.detach())) <= 1e-6 * abs(float(l1.detach()))


def test_vgg_upstream_scalar_and_second_backward():
    sd, out, tgt, _, grad = L.case(VGG_SHAPES[1])
    o = out.cuda().requires_grad_(True)
    loss = _vgg(sd, "fp32", frames_per_pass=2)(o, tgt.cuda())
    (loss * 3.0).backward(retain_graph=True)
    assert float((o.grad.cpu().double() - 3.0 * grad).norm() / (3.0 * grad).norm()) <= F32_TOL
    with pytest.raises(RuntimeError):
        loss.backward()


def test_vgg_memory_follows_the_chunk():
    """F = 4 frames, one per pass: the peak over forward and backward() stays below one chunk's workspace and backward scratch (the
    library's own size functions for nb images) + 4 x the 5-D tensor + 1 MiB, and below the peak of the one-pass form."""
    from srcgan_amd import _native as N
    shape = (2, 3, 4, 64, 64)
    sd = R.seeded_state(0)
    g = torch.Generator().manual_seed(3)
    out, tgt = torch.rand(shape, generator=g).cuda(), torch.rand(shape, generator=g).cuda()

    def run(fpp):
        m = _vgg(sd, "bf16", frames_per_pass=fpp)
        o = out.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m(o, tgt).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    peak1, peak_all = run(1), run(None)
    cfg = N.VggLossCfg(0, shape[0], shape[3], shape[4], N.BF16)
    lib = N.lib()
    bound = lib.srcgan_vggloss_ws_bytes(C.byref(cfg)) + lib.srcgan_vggloss_bwd_scratch_bytes(C.byref(cfg)) + 4 * out.numel() * 4 + (1 << 20)
    print(f"peak allocation: one frame per pass {peak1} B (bound {bound} B), all frames in one pass {peak_all} B")
    assert peak1 <= bound
    assert peak1 < peak_all
