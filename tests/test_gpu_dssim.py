"""GPU: srcgan_amd.DSSIMLoss (native forward = range + SSIM tile kernels + fold; native fused backward, metrics.hip dssim_bwd_k)
against the reference's DSSIM fixture, the CPU oracle through autograd, and its own structure: locality of the stencil at full
size, batch slices, determinism, 64-bit indexing past 2^31 bytes per tensor, and the gradient it feeds into a generator."""
import pytest
import torch

import oracle
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

CASES = ["rgb01", "gray255", "tanh", "single", "strip_row", "strip_col"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _native(x, t, target_grad=True):
    """-> (loss, dx, dt) of DSSIMLoss on device; dt is None when the target does not require grad."""
    from srcgan_amd import DSSIMLoss
    x = x.detach().clone().requires_grad_(True)
    t = t.detach().clone().requires_grad_(target_grad)
    loss = DSSIMLoss()(x, t)
    loss.backward()
    return loss.detach(), x.grad, t.grad


def _oracle(x, t):
    x = x.detach().cpu().float().requires_grad_(True)
    t = t.detach().cpu().float().requires_grad_(True)
    loss = (1.0 - oracle.metric_ssim(x, t)) / 2.0
    loss.backward()
    return loss.detach(), x.grad, t.grad


def _n(x):
    B, C, H, W = x.shape
    return B * C * (H - 10) * (W - 10)


def _pair(shape, seed, noise=0.1):
    """target uniform in [0, 1), prediction = target + noise clamped to [0, 1] (dynamic range L = 1)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.rand(shape, device="cuda", generator=g)
    x = (t + noise * torch.randn(shape, device="cuda", generator=g)).clamp_(0, 1)
    return x, t


@pytest.mark.parametrize("case", CASES)
def test_golden_parity(case):
    g = load_golden("dssim")
    x, t = torch.from_numpy(g[f"{case}/x"]).float().cuda(), torch.from_numpy(g[f"{case}/t"]).float().cuda()
    loss, dx, dt = _native(x, t)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    assert abs(float(loss) - float(g[f"{case}/loss"])) < 1e-5
    assert rel_err(dx.cpu(), g[f"{case}/dx"]) < 1e-3
    assert rel_err(dt.cpu(), g[f"{case}/dt"]) < 1e-3
    # the dx-only kernel variant (target without grad) gives the same input gradient
    _, dx1, dt1 = _native(x, t, target_grad=False)
    assert dt1 is None
    assert rel_err(dx1.cpu(), dx.cpu()) < 1e-5


def test_golden_near_one_against_f64():
    g = load_golden("dssim")
    x, t = torch.from_numpy(g["near/x"]).float().cuda(), torch.from_numpy(g["near/t"]).float().cuda()
    loss, dx, dt = _native(x, t)
    assert abs(float(loss) - float(g["near/loss"])) < 1e-5
    assert rel_err(dx.cpu(), g["near/dx"]) < float(g["near/gate_dx"])
    assert rel_err(dt.cpu(), g["near/dt"]) < float(g["near/gate_dt"])


def test_oracle_autograd_parity_correlated():
    g = torch.Generator().manual_seed(7)
    base = torch.nn.functional.avg_pool2d(torch.rand(2, 3, 264, 264, generator=g), 9, 1)      # smooth, correlated over windows
    t = base.clone()
    x = (0.8 * base + 0.1 + 0.05 * torch.randn(base.shape, generator=g)).clamp(0, 1)
    loss, dx, dt = _native(x.cuda(), t.cuda())
    rl, rdx, rdt = _oracle(x, t)
    assert abs(float(loss) - float(rl)) < 1e-5
    assert rel_err(dx.cpu(), rdx) < 1e-3
    assert rel_err(dt.cpu(), rdt) < 1e-3


@pytest.fixture(scope="module")
def full():
    x, t = _pair((16, 3, 1024, 1024), seed=3)
    loss, dx, dt = _native(x, t)
    return x, t, loss, dx, dt


def test_full_size_locality(full):
    """The gradient of an interior 128x128 region depends only on pixels within 10 of it: a crop with a 20-pixel margin gives the
    same gradient once both are scaled by their window-position counts."""
    x, t, _, dx, dt = full
    r0, c0, m = 448, 576, 20
    xc = x[:, :, r0 - m:r0 + 128 + m, c0 - m:c0 + 128 + m].contiguous()
    tc = t[:, :, r0 - m:r0 + 128 + m, c0 - m:c0 + 128 + m].contiguous()
    _, cdx, cdt = _native(xc, tc)
    big = lambda d: d[:, :, r0:r0 + 128, c0:c0 + 128].double() * _n(x)
    crop = lambda d: d[:, :, m:m + 128, m:m + 128].double() * _n(xc)
    assert rel_err(big(dx), crop(cdx)) < 1e-5
    assert rel_err(big(dt), crop(cdt)) < 1e-5


def test_batch_slices(full):
    x, t, loss, dx, dt = full
    losses = []
    for i in range(x.shape[0]):
        li, dxi, dti = _native(x[i:i + 1], t[i:i + 1])
        losses.append(float(li))
        assert rel_err(dx[i:i + 1], dxi / x.shape[0]) < 1e-6, i
        assert rel_err(dt[i:i + 1], dti / x.shape[0]) < 1e-6, i
    mean = sum(losses) / len(losses)
    assert abs(float(loss) - mean) <= 1e-6 * abs(mean)


def test_deterministic(full):
    x, t, loss, dx, dt = full
    loss2, dx2, dt2 = _native(x, t)
    assert torch.equal(loss, loss2)
    assert torch.equal(dx, dx2)
    assert torch.equal(dt, dt2)


def test_beyond_2g_bytes_per_tensor():
    """48x3x2048x2048 f32 is 2.4 GB per tensor: the bottom-right corner of the last image lies past 2^31 elements' bytes."""
    x, t = _pair((48, 3, 2048, 2048), seed=5)
    assert x.numel() * 4 > 2 ** 31
    _, dx, dt = _native(x, t)
    m = 20
    xc = x[-2:, :, -(128 + m):, -(128 + m):].contiguous()
    tc = t[-2:, :, -(128 + m):, -(128 + m):].contiguous()
    _, cdx, cdt = _native(xc, tc)
    big = lambda d: d[-2:, :, -128:, -128:].double() * _n(x)
    crop = lambda d: d[:, :, m:, m:].double() * _n(xc)
    assert rel_err(big(dx), crop(cdx)) < 1e-5
    assert rel_err(big(dt), crop(cdt)) < 1e-5


def test_other_float_dtypes_compute_in_f32():
    x, t = _pair((2, 3, 40, 36), seed=9)
    x, t = x.half(), t.bfloat16()
    loss, dx, dt = _native(x, t)
    l32, dx32, dt32 = _native(x.float(), t.float())
    assert loss.dtype == torch.float32 and torch.equal(loss, l32)
    assert dx.dtype == torch.float16 and dt.dtype == torch.bfloat16
    assert torch.equal(dx, dx32.half()) and torch.equal(dt, dt32.bfloat16())


def test_gradient_into_a_generator():
    from srcgan_amd import RDDBNet, DSSIMLoss
    torch.manual_seed(0)
    net = RDDBNet(3, 3, 2, nb=1, dtype="fp32").cuda()
    x = torch.rand(2, 3, 24, 20, device="cuda")
    t = torch.rand(2, 3, 48, 40, device="cuda")
    DSSIMLoss()(net(x), t).backward()
    got = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    y = net(x)
    _, g_ref, _ = _oracle(y, t)
    y.backward(g_ref.cuda())
    for k, p in net.named_parameters():
        assert rel_err(got[k].cpu(), p.grad.cpu()) < 1e-3, k
