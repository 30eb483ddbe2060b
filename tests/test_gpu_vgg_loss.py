"""losses.VGG16Loss / losses.PerceptionLoss against the float64 compositions of tests/vgg_ref.py (reference src/losses.py:376-393,
464-468), with seeded weights.  GPU tests carry the `gpu` mark one by one: the interface tests at the end need no GPU.

Gates.  fp32: loss (relative) and d loss / d output (relative L2: isolated sign / ReLU / argmax flips move single elements) within
F32_TOL = 1e-3, the f32 parity gate of tests/test_gpu_modules.py.  bf16 / fp16: the yardstick of test_resdeconv_bf16_vs_oracle -- the
native error against float64 is at most 1.5 x the error of the same float64 composition with the input, the conv weights and every
activation stored in that dtype, + 5e-3.  tests/test_vgg_teeth.py shows what these comparisons notice."""
import functools
import subprocess
import sys

import pytest
import torch

import vgg_ref as R
from conftest import rel_err
from net_checks import F32_TOL, bound16

gpu = pytest.mark.gpu
SHAPES = [(2, 3, 20, 28), (1, 1, 32, 32), (1, 3, 16, 16)]      # pools floor 5x7 -> 2x3; gray replication; the smallest VGG19 size
BIG = (1, 3, 272, 272)                                         # 4 N_1 = 4 * 64 * 272^2 > 2^24 ((1,3,256,256) gives exactly 2^24)
STORE = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _module(kind, sd, dtype, **kw):
    from srcgan_amd import VGG16Loss, PerceptionLoss
    return VGG16Loss(weights=sd, dtype=dtype, **kw) if kind == 0 else PerceptionLoss(weights=sd, dtype=dtype, **kw).cuda()


def _native(kind, shape, dtype):
    sd, out, tgt, _, _ = R.case(kind, shape)
    m = _module(kind, sd, dtype)
    o = out.cuda().requires_grad_(True)
    loss = m(o, tgt.cuda())
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    assert o.grad.shape == out.shape
    return float(loss.detach()), o.grad.cpu()


@functools.lru_cache(maxsize=None)
def _emulated(kind, shape, dname):
    """(loss error, gradient error) against float64 of the float64 composition that stores in the 16-bit dtype"""
    sd, out, tgt, loss, grad = R.case(kind, shape)
    le, ge = R.loss_and_grad(out, tgt, sd, kind, store=STORE[dname])
    return R.errors(le, ge, loss, grad)


@gpu
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_loss_and_gradient_vs_float64(kind, shape):
    _, _, _, loss, grad = R.case(kind, shape)
    e_loss, e_grad = R.errors(*_native(kind, shape, "fp32"), loss, grad)
    print(f"kind {kind} {shape} fp32: loss error {e_loss:.3e}, gradient error {e_grad:.3e}")
    assert e_loss <= F32_TOL and e_grad <= F32_TOL


@gpu
@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_16bit_loss_and_gradient_vs_storage_emulation(kind, shape, dname):
    _, _, _, loss, grad = R.case(kind, shape)
    f_loss, f_grad = _emulated(kind, shape, dname)
    e_loss, e_grad = R.errors(*_native(kind, shape, dname), loss, grad)
    print(f"kind {kind} {shape} {dname}: loss error {e_loss:.3e} (emulation {f_loss:.3e}), gradient error {e_grad:.3e} (emulation {f_grad:.3e})")
    assert e_loss <= bound16(f_loss) and e_grad <= bound16(f_grad)


@gpu
def test_fp16_gradient_survives_at_a_training_size():
    """With 1 / (4 N) applied at the taps, fp16 gradients of this size are subnormal or zero from the first tap on (1 / (4 N_1) = 2^-24.2).
    They travel at unit scale instead: dx is non-zero and meets the 16-bit bound."""
    _, _, _, loss, grad = R.case(0, BIG)
    f_loss, f_grad = _emulated(0, BIG, "fp16")
    got_loss, got_grad = _native(0, BIG, "fp16")
    e_loss, e_grad = R.errors(got_loss, got_grad, loss, grad)
    nz = float((got_grad != 0).double().mean())
    print(f"{BIG} fp16: loss error {e_loss:.3e} (emulation {f_loss:.3e}), gradient error {e_grad:.3e} (emulation {f_grad:.3e}), non-zero {nz:.3f} "
          f"(float64: {float((grad != 0).double().mean()):.3f}), max |dx| {float(got_grad.abs().max()):.3e}")
    assert float(got_grad.abs().max()) > 0 and nz >= 0.9 * float((grad != 0).double().mean())
    assert e_loss <= bound16(f_loss) and e_grad <= bound16(f_grad)


@gpu
def test_espcn_under_vgg_plus_l1_parameter_gradients():
    """one backward() through L1 + VGG16Loss into a native generator: every parameter gradient against the float64 composition"""
    from srcgan_amd import ESPCN, L1Loss
    torch.manual_seed(11)
    net = ESPCN(1, 1, 2, dtype="fp32").cuda()
    sd = R.seeded_state(0, seed=1)
    vgg = _module(0, sd, "fp32")
    g = torch.Generator().manual_seed(12)
    x, t = torch.rand(1, 1, 16, 16, generator=g), torch.rand(1, 1, 32, 32, generator=g)
    y = net(x.cuda())
    (vgg(y, t.cuda()) + L1Loss()(y, t.cuda())).backward()
    ref = {k: p.detach().cpu().double().requires_grad_(True) for k, p in net.named_parameters()}
    yr = R.espcn_forward(ref, x.double(), 2)
    (R.vgg_loss(yr, t.double(), sd, 0) + torch.nn.functional.l1_loss(yr, t.double())).backward()
    rows = {k: rel_err(p.grad, ref[k].grad) for k, p in net.named_parameters()}
    print("ESPCN under VGG16Loss + L1, parameter gradient errors:", {k: f"{v:.2e}" for k, v in rows.items()})
    assert rel_err(y, yr) <= F32_TOL
    for k, e in rows.items():
        assert e <= F32_TOL, (k, e)


@gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_no_grad_gives_the_same_bits_in_less_memory(kind):
    sd, out, tgt, _, _ = R.case(kind, SHAPES[0])
    m = _module(kind, sd, "bf16")
    o, t = out.cuda(), tgt.cuda()

    def run(grad):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.set_grad_enabled(grad):
            loss = m(o.clone().requires_grad_(grad), t)
        torch.cuda.synchronize()
        return loss.detach().cpu(), torch.cuda.max_memory_allocated() - base

    (l0, peak0), (l1, peak1) = run(False), run(True)
    print(f"kind {kind}: peak allocation no_grad {peak0} B, grad mode {peak1} B")
    assert l0.view(torch.int32) == l1.view(torch.int32)
    assert peak0 < peak1


@gpu
def test_second_backward_is_refused():
    sd, out, tgt, _, _ = R.case(0, SHAPES[2])
    o = out.cuda().requires_grad_(True)
    loss = _module(0, sd, "fp32")(o, tgt.cuda())
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError):
        loss.backward()


# ------------------------------------------------------------------------------------------------ interface (no GPU)
def test_state_dict_keys_are_the_references():
    from srcgan_amd import VGG16Loss, PerceptionLoss
    a, b = VGG16Loss(weights=R.seeded_state(0)), PerceptionLoss(weights=R.seeded_state(1))
    assert list(a.state_dict()) == R.VGG16LOSS_KEYS and list(b.state_dict()) == R.PERCEPTION_KEYS
    assert repr(a) == "VGG16"
    for m in (a, b):
        assert all(isinstance(p, torch.nn.Parameter) and not p.requires_grad for p in m.parameters())


def test_weights_load_from_torchvision_keys_reference_keys_and_a_path(tmp_path):
    from srcgan_amd import VGG16Loss, PerceptionLoss
    sd = R.seeded_state(0)
    full = dict(sd)
    full["classifier.0.weight"] = torch.zeros(2, 2)               # a whole torchvision checkpoint carries more than the prefix
    torch.save(full, tmp_path / "vgg16.pth")
    want = R.to_slice_keys(sd)
    for m in (VGG16Loss(weights=full), VGG16Loss(weights=want), VGG16Loss(weights=str(tmp_path / "vgg16.pth"))):
        got = m.state_dict()
        assert all(torch.equal(got[k].cpu(), want[k]) for k in want)
    with pytest.warns(UserWarning, match="default initialisation"):
        m = VGG16Loss()
    m.load_state_dict(want)                                        # a checkpoint of the reference loss
    assert torch.equal(m.state_dict()["slice3.12.weight"].cpu(), want["slice3.12.weight"])
    sd19 = R.seeded_state(1)
    assert torch.equal(PerceptionLoss(weights=sd19).state_dict()["features.34.bias"], sd19["features.34.bias"])
    with pytest.raises(KeyError):
        PerceptionLoss(weights=sd)                                 # a VGG16 prefix lacks features.16 ...


def test_refusals():
    from srcgan_amd import VGG16Loss, PerceptionLoss
    with pytest.raises(NotImplementedError, match="frozen"):
        VGG16Loss(requires_grad=True, weights=R.seeded_state(0))
    with pytest.raises(NotImplementedError, match="feature_layer"):
        PerceptionLoss(feature_layer=26, weights=R.seeded_state(1))
    m = VGG16Loss(weights=R.seeded_state(0))
    with pytest.raises((NotImplementedError, ValueError), match="target"):
        m(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16, requires_grad=True))
    with pytest.raises(ValueError):
        m(torch.rand(1, 2, 16, 16), torch.rand(1, 2, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.cpu()(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16))


def test_planner_sizes_are_those_of_a_frozen_plan():
    """host-only queries: parameter counts, a backward scratch of exactly two gradient buffers of the largest tensor (no split-K slab, no
    column-reduce scratch), a no_grad workspace below the training one, refused sizes"""
    import ctypes as C
    from srcgan_amd import _native as N
    lib = N.lib()
    for kind, nparams in ((0, 20), (1, 32)):
        for dt, esz in ((N.F32, 4), (N.BF16, 2)):
            cfg = N.VggLossCfg(kind, 2, 20, 28, dt)
            assert lib.srcgan_vggloss_num_params(C.byref(cfg)) == nparams
            largest = 2 * 20 * 28 * 64 * esz                      # relu1_1 / relu1_2, a multiple of the 256-byte slot alignment
            assert lib.srcgan_vggloss_bwd_scratch_bytes(C.byref(cfg)) == 2 * largest + 256
            assert 0 < lib.srcgan_vggloss_infer_ws_bytes(C.byref(cfg)) < lib.srcgan_vggloss_ws_bytes(C.byref(cfg))
    assert lib.srcgan_vggloss_ws_bytes(C.byref(N.VggLossCfg(1, 1, 8, 16, N.F32))) == 0
    assert b"at least 16" in lib.srcgan_last_error()
    assert lib.srcgan_vggloss_ws_bytes(C.byref(N.VggLossCfg(2, 1, 32, 32, N.F32))) == 0


def test_importing_the_losses_does_not_import_torchvision():
    code = "import sys; import srcgan_amd.losses; import srcgan_amd; assert 'torchvision' not in sys.modules, 'torchvision was imported'"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=R.__file__.rsplit("/tests/", 1)[0])
    assert r.returncode == 0, r.stderr
