"""GPU: FLoss, CELoss, ConLoss and CrossLoss and the kernels under them (csrc/class_losses.hip) against the float64 restatement of
tests/class_losses_ref.py.  Loss and every gradient element within K_RECORDED * 2^-24 * N (N = the sum of the absolute values of the
quantity's own terms; an element with N = 0 must be exactly 0), on the grid of class_losses_ref (``grid``):

  flat kernels (focal, BCE)   n = 1; 3*1*5*7 = 105 (one block, n % 4 != 0); 2*1*33*65 (blocks and a tail); GRID + 5, where
                              GRID = 2 097 152 elements is what the backward's grid (CL_BWD_BLOCKS = 2048 blocks * 256 threads * 4) and
                              the forward's (CL_FWD_BLOCKS = 1024 blocks * 512 threads * 4) cover in one pass: both loop, both have a tail
  multi-class focal           3*4*5*7, 2*5*33*65
  NLL (N, C, S)               (1,2,1), (3,4,35), (2,5,4291) (S odd: rows misaligned), (2,3,1028) (the 16-byte path), maximum in the first /
                              last channel
  batch range (nb, M)         (1,7) (exactly 0), (2,105), (5,4291), (16,33), (3,1028) (the 16-byte path)
  shifted L1 (nb, S)          (2,105) (target + S misaligned), (3,1), (4,4290), (3,1028) (the 16-byte path)

and on the fixture of the reference's own float32 results (tests/golden/class_losses.npz), the clamp edges and the ties included.
Observed maxima (units of 2^-24 N) are printed by the last test."""
import ctypes as C

import numpy as np
import pytest
import torch

import class_losses_ref as R
from conftest import load_golden
from test_class_losses_host import FIXTURE, fixture_inputs

pytestmark = pytest.mark.gpu
OBSERVED = {q: 0.0 for q in R.QUANTITIES}
_REF = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _reference(key, fn, inp, kw, gout=1.0):
    """The float64 restatement of one case, computed once and shared."""
    k = (key, gout)
    if k not in _REF:
        _REF[k] = fn(*inp, gout=gout, **kw)
    return _REF[k]


def _criterion(q, kw):
    from srcgan_amd import losses
    if q == "focal":
        return losses.FLoss(gamma=kw.get("gamma", 2.0), size_average=kw.get("mean", True))
    return {"bce": losses.CELoss, "nll": losses.CELoss, "range": losses.ConLoss, "cross": losses.CrossLoss}[q]()


def _run(q, inp, kw, factor=None):
    """Forward and backward through the public class -> (loss, gradient) as numpy."""
    x = _dev(inp[0]).requires_grad_(True)
    loss = _criterion(q, kw)(x, *[_dev(a) for a in inp[1:]])
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    (loss if factor is None else factor * loss).backward()
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy()


def _check(q, tag, loss, grad, ref, against=None):
    """``against``: (loss, gradient) to compare with in place of the restatement's own (the reference's float32 results)."""
    want_loss, want_grad = (ref["loss"], ref["grad"]) if against is None else against
    grad = grad.reshape(ref["grad"].shape)
    ul = R.units(loss, want_loss, ref["Nloss"])
    ug = R.units(grad, np.asarray(want_grad).reshape(grad.shape), ref["Ngrad"])
    print(f"[class_losses] {tag}: loss {ul:.2f} of K = {R.K_RECORDED[q + '_loss']:.0f}, gradient {ug:.2f} of K = {R.K_RECORDED[q + '_grad']:.0f}")
    OBSERVED[q + "_loss"], OBSERVED[q + "_grad"] = max(OBSERVED[q + "_loss"], ul), max(OBSERVED[q + "_grad"], ug)
    assert ul <= R.K_RECORDED[q + "_loss"], (tag, ul)
    assert ug <= R.K_RECORDED[q + "_grad"], (tag, ug)
    assert np.all(grad[ref["Ngrad"] == 0] == 0), tag            # the zeros are exact zeros
    assert np.all(np.isfinite(grad)), tag


GRID_CASES = list(R.grid())
GRID_IDS = [f"{q}-{'x'.join(str(v) for v in inp[0].shape)}" + "".join(f"-{k}{v}" for k, v in kw.items()) + f"-{i}"
            for i, (q, _, inp, kw) in enumerate(GRID_CASES)]


@pytest.mark.parametrize("idx", range(len(GRID_CASES)), ids=GRID_IDS)
def test_grid_against_float64(idx):
    q, fn, inp, kw = GRID_CASES[idx]
    ref = _reference(idx, fn, inp, kw)
    loss, grad = _run(q, inp, kw)
    _check(q, GRID_IDS[idx], loss, grad, ref)
    loss2, grad2 = _run(q, inp, kw)                              # fixed summation order: the same bits again
    assert loss.tobytes() == loss2.tobytes() and grad.tobytes() == grad2.tobytes()


def test_single_sample_range_is_exactly_zero():
    loss, grad = _run("range", (R.range_inputs((1, 7)),), {})
    assert float(loss) == 0.0 and np.all(grad == 0) and grad.shape == (1, 7)


@pytest.mark.parametrize("idx", [1, 5, 7, 9, 12, 16, 21, 26], ids=lambda i: GRID_IDS[i])
def test_upstream_gradient_scales(idx):
    """(3 * loss).backward(): the upstream gradient is read from device memory and scales every element."""
    q, fn, inp, kw = GRID_CASES[idx]
    ref = _reference(idx, fn, inp, kw, gout=3.0)
    loss, grad = _run(q, inp, kw, factor=3.0)
    _check(q, GRID_IDS[idx] + " gout=3", loss, grad, ref)


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_fixture_against_the_reference(name):
    """The reference's own float32 loss and output.grad, the clamp edges and the ties element by element, at the same bound."""
    z = load_golden("class_losses")
    q, fn, kw = FIXTURE[name]
    inp = fixture_inputs(z, name)
    ref = _reference("fixture/" + name, fn, inp, kw)
    loss, grad = _run(q, inp, kw)
    _check(q, "fixture " + name, loss, grad, ref, against=(z[name + "/loss"], z[name + "/dx"]))
    assert np.array_equal(grad.reshape(z[name + "/dx"].shape) == 0, z[name + "/dx"] == 0)          # zero exactly where the reference is
    _check(q, "fixture " + name + " (float64)", loss, grad, ref)


def test_bce_outside_the_unit_interval_is_nan():
    from srcgan_amd import losses
    x, t = _dev(np.array([[1.5], [0.5], [-0.25]])), _dev(np.array([[1.0], [0.0], [0.0]]))
    assert torch.isnan(losses.CELoss()(x, t)).item()


def test_range_nan_reaches_the_loss():
    from srcgan_amd import losses
    f = R.range_inputs((5, 33))
    f[2, 17] = np.nan
    assert torch.isnan(losses.ConLoss()(_dev(f))).item()
    f = R.range_inputs((5, 33))
    f[0, 4] = np.nan
    assert torch.isnan(losses.ConLoss()(_dev(f))).item()


def test_other_dtypes_compute_in_f32_and_return_their_own_gradient_dtype():
    from srcgan_amd import losses
    x, t = R.flat_inputs((3, 1, 5, 7))
    ref = R.focal(x, t)
    xh = _dev(x).half().requires_grad_(True)
    loss = losses.FLoss()(xh, _dev(t).half())
    loss.backward()
    assert loss.dtype == torch.float32 and xh.grad.dtype == torch.float16
    assert R.units(loss.detach().cpu().numpy(), ref["loss"], ref["Nloss"]) <= R.K_RECORDED["focal_loss"]
    with torch.no_grad():
        assert losses.FLoss()(_dev(x), _dev(t)).cpu().numpy().tobytes() == loss.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ the kernels through ctypes
def _kernel_calls(q, x, t, kw, out, scratch, gout, dx):
    """(forward call, backward call) of one kernel pair on device tensors."""
    from srcgan_amd import _native as N
    lib, st = N.lib(), N.stream_ptr(x.device)
    xp, tp = x.data_ptr(), (None if t is None else t.data_ptr())
    if q == "focal":
        cfg = (x.numel(), int(kw["binary"]), float(kw.get("gamma", 2.0)), int(kw.get("mean", True)))
        return (lambda: lib.srcgan_focal_fwd(xp, tp, *cfg, out.data_ptr(), scratch.data_ptr(), st),
                lambda: lib.srcgan_focal_bwd(xp, tp, *cfg, gout.data_ptr(), dx.data_ptr(), st))
    if q == "bce":
        return (lambda: lib.srcgan_bce_fwd(xp, tp, x.numel(), out.data_ptr(), scratch.data_ptr(), st),
                lambda: lib.srcgan_bce_bwd(xp, tp, x.numel(), gout.data_ptr(), dx.data_ptr(), st))
    if q == "nll":
        dims = (x.shape[0], x.shape[1], x.numel() // (x.shape[0] * x.shape[1]))
        return (lambda: lib.srcgan_nll_argmax_fwd(xp, tp, *dims, out.data_ptr(), scratch.data_ptr(), st),
                lambda: lib.srcgan_nll_argmax_bwd(xp, tp, *dims, gout.data_ptr(), dx.data_ptr(), st))
    dims = (x.shape[0], x.numel() // x.shape[0])
    if q == "range":
        return (lambda: lib.srcgan_batch_range_fwd(xp, *dims, out.data_ptr(), scratch.data_ptr(), st),
                lambda: lib.srcgan_batch_range_bwd(xp, *dims, gout.data_ptr(), dx.data_ptr(), st))
    return (lambda: lib.srcgan_cross_l1_fwd(xp, tp, *dims, out.data_ptr(), scratch.data_ptr(), st),
            lambda: lib.srcgan_cross_l1_bwd(xp, tp, *dims, gout.data_ptr(), dx.data_ptr(), st))


def _offset(a, off, extra=0):
    """A device copy of ``a`` whose first element lies ``off`` floats past a 16-byte boundary (``extra`` spare floats behind it)."""
    buf = torch.full((a.size + off + extra + 8,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1))
    return v.view(a.shape), buf


@pytest.mark.parametrize("idx", [1, 2, 4, 8, 12, 16, 17, 18, 23, 24, 26, 28, 29], ids=lambda i: GRID_IDS[i])
@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 1, 1), (3, 3, 3), (0, 2, 0), (1, 0, 3)], ids=str)
def test_kernels_write_every_element_once_at_every_alignment(idx, offs):
    """Straight through the C entry points: the gradient buffer is NaN before the call and NaN around it afterwards, the result is within
    the bound whatever 16-byte phase the three pointers have (equal phases: head, 16-byte body, tail; unequal: element by element), and
    a second call gives the same bits."""
    from srcgan_amd import _native as N
    q, fn, inp, kw = GRID_CASES[idx]
    ref = _reference(idx, fn, inp, kw, gout=3.0)
    kw = dict(kw, binary=inp[0].shape[1] == 1)
    x, _ = _offset(inp[0], offs[0])
    t = _offset(inp[1], offs[1])[0] if len(inp) > 1 else None
    n = x.numel()
    dx, buf = _offset(np.full(inp[0].shape, np.nan, np.float32), offs[2])
    out, gout = torch.full((), float("nan"), device="cuda"), torch.full((), 3.0, device="cuda")
    scratch = torch.empty(N.lib().srcgan_loss_scratch_floats(), dtype=torch.float32, device="cuda")
    fwd, bwd = _kernel_calls(q, x, t, kw, out, scratch, gout, dx)
    N.check(fwd(), "forward")
    N.check(bwd(), "backward")
    loss, grad, whole = out.cpu().numpy(), dx.cpu().numpy(), buf.cpu().numpy()
    assert not np.isnan(grad).any()
    assert np.isnan(whole[:offs[2]]).all() and np.isnan(whole[offs[2] + n:]).all()                   # nothing written outside
    _check(q, f"kernel {GRID_IDS[idx]} offsets {offs}", loss, grad, ref)
    dx.fill_(float("nan"))
    out.fill_(float("nan"))
    N.check(fwd(), "forward")
    N.check(bwd(), "backward")
    assert out.cpu().numpy().tobytes() == loss.tobytes() and dx.cpu().numpy().tobytes() == grad.tobytes()


def test_kernels_refuse_bad_arguments():
    from srcgan_amd import _native as N
    lib = N.lib()
    x = torch.rand(2, 8, device="cuda")
    out, scratch = torch.empty((), device="cuda"), torch.empty(lib.srcgan_loss_scratch_floats(), device="cuda")
    assert lib.srcgan_cross_l1_fwd(x.data_ptr(), x.data_ptr(), 1, 8, out.data_ptr(), scratch.data_ptr(), None) != 0
    assert b"nb >= 2" in lib.srcgan_last_error()
    assert lib.srcgan_focal_fwd(x.data_ptr(), x.data_ptr(), 0, 1, 2.0, 1, out.data_ptr(), scratch.data_ptr(), None) != 0
    assert lib.srcgan_nll_argmax_fwd(x.data_ptr(), None, 1, 2, 8, out.data_ptr(), scratch.data_ptr(), None) != 0
    assert lib.srcgan_batch_range_bwd(x.data_ptr(), 0, 8, out.data_ptr(), x.data_ptr(), None) != 0


def test_zz_report_observed_maxima():
    print("[class_losses] observed maxima in units of 2^-24 N:", {q: round(v, 2) for q, v in OBSERVED.items()})
    print("[class_losses] K_RECORDED:", R.K_RECORDED)
    for q, v in OBSERVED.items():
        assert v <= R.K_RECORDED[q]
