"""GPU: srcgan_amd.NearestSelector / NearestL1Loss (shift_select.hip: one-pass shift search, device-side selection, window gather,
fused L1 backward) against tests/nearest_ref.py's float64 restatement and the reference's fixture (tests/golden/nearest_selector.npz).

Integer operands in {0..15} make every partial sum an exact integer below 2^24, so the sums, the selection, the crops and the
gradients are compared bit for bit; float operands go through the project's fp32 gate (rel_err <= 1e-3) with an exact selection,
which the margin condition of tests/test_nearest_teeth.py guarantees.  The comparison functions at the top are the ones
test_nearest_teeth.py turns on single-mistake variants of the restatement."""
import functools

import numpy as np
import pytest
import torch

import nearest_ref as R
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

GATE = 1e-3
NAMES = list(R.SHAPES)


# --------------------------------------------------------------------------- comparisons (shared with test_nearest_teeth.py)
def same_values(got, want):
    """shape and every value equal (float64 on both sides: bit for bit for f32 results of exact integer sums)"""
    got, want = torch.as_tensor(np.asarray(got)), torch.as_tensor(np.asarray(want))
    return got.shape == want.shape and torch.equal(got.double(), want.double())


def within_gate(got, want):
    got, want = torch.as_tensor(np.asarray(got)), torch.as_tensor(np.asarray(want))
    return got.shape == want.shape and bool(torch.isfinite(got.double()).all()) and rel_err(got, want) <= GATE


def within_one_ulp(got, want64):
    want = np.float32(want64)
    return abs(float(got) - float(want)) <= float(np.spacing(want))


# --------------------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=None)
def int_ref(name):
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t = R.int_case(name, 100 + NAMES.index(name))
    ref = R.l1(o.numpy(), t.numpy(), shift, stride)
    ref["out_"], ref["tgt_"], _ = R.crops(o.numpy(), t.numpy(), shift, stride, ref["sel"])
    return o, t, ref


@functools.lru_cache(maxsize=None)
def float_ref(name):
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, planted = R.float_case(name, R.FLOAT_SEEDS[name])
    return o, t, planted, R.l1(o.numpy(), t.numpy(), shift, stride)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _search(o, t, shift, stride, want_loss=False):
    """the kernel's own (diff, sel, loss) for the loss's crop size"""
    from srcgan_amd import losses
    dims = losses._shift_check("test", o, t, shift, stride)
    return losses._shift_search(o.contiguous(), t.contiguous(), dims, shift, stride, want_loss)


def _fused(o, t, shift, stride, target_grad=True):
    from srcgan_amd import NearestL1Loss
    o = o.detach().clone().requires_grad_(True)
    t = t.detach().clone().requires_grad_(target_grad)
    loss = NearestL1Loss(shift, stride)(o, t)
    loss.backward()
    return loss.detach(), o.grad, t.grad


def _l1_on_crops(out_, tgt_, sel, full_shape, shift, stride):
    """the existing native L1Loss on the contiguous crops, its gradients zero-padded / placed at each sample's window"""
    from srcgan_amd import L1Loss
    a = torch.as_tensor(out_).float().cuda().contiguous().requires_grad_(True)
    b = torch.as_tensor(tgt_).float().cuda().contiguous().requires_grad_(True)
    loss = L1Loss()(a, b)
    loss.backward()
    sd, ch, cw, _ = R.geometry(full_shape[2], full_shape[3], shift, stride)
    do, dt = torch.zeros(full_shape, device="cuda"), torch.zeros(full_shape, device="cuda")
    do[:, :, sd:sd + ch, sd:sd + cw] = a.grad
    for i, (r, c) in enumerate(np.asarray(sel)):
        dt[i, :, r * stride:r * stride + ch, c * stride:c * stride + cw] = b.grad[i]
    return loss.detach(), do, dt


# --------------------------------------------------------------------------- integer operands: everything exact
@pytest.mark.parametrize("name", NAMES)
def test_integer_operands_are_exact(name):
    from srcgan_amd import NearestSelector
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, ref = int_ref(name)
    og, tg = o.cuda(), t.cuda()
    sd, ch, cw, n = R.geometry(H, W, shift, stride)
    assert ref["diff"].max() < 2 ** 24
    ns = NearestSelector(shift, stride)
    diff = ns.shift_diff(og, tg, ch, cw)
    assert diff.dtype == torch.float32 and diff.is_cuda
    assert same_values(diff.cpu(), ref["diff"])
    kdiff, ksel, _ = _search(og, tg, shift, stride)
    assert ksel.dtype == torch.int32 and same_values(ksel.cpu(), ref["sel"]) and torch.equal(kdiff, diff)
    sel64 = NearestSelector.unravel_index(diff, n)
    assert sel64.dtype == torch.int64 and same_values(sel64.cpu(), ref["sel"])
    out_, tgt_ = ns.crop(og, tg)
    assert same_values(out_.cpu(), ref["out_"]) and same_values(tgt_.cpu(), ref["tgt_"])
    assert tgt_.is_contiguous() and not tgt_.requires_grad
    # the slice itself, on the device
    for b, (r, c) in enumerate(ref["sel"]):
        assert torch.equal(tgt_[b], tg[b, :, r * stride:r * stride + ch, c * stride:c * stride + cw])


@pytest.mark.parametrize("name", NAMES)
def test_fused_loss_equals_l1_on_the_crops(name):
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, ref = int_ref(name)
    loss, do, dt = _fused(o.cuda(), t.cuda(), shift, stride)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    print(f"[nearest] {name}: fused {float(loss):.9g} f64 {ref['loss']:.12g}")
    assert within_one_ulp(loss, ref["loss"])
    l1, do_ref, dt_ref = _l1_on_crops(ref["out_"], ref["tgt_"], ref["sel"], o.shape, shift, stride)
    assert abs(float(l1) - ref["loss"]) <= 1e-6 * ref["loss"]          # sum * f32(1/N): two roundings, not the fused sum / N
    assert torch.equal(do, do_ref) and torch.equal(dt, dt_ref)
    assert within_gate(do.cpu(), ref["dout"]) and within_gate(dt.cpu(), ref["dtgt"])
    _, do1, dt1 = _fused(o.cuda(), t.cuda(), shift, stride, target_grad=False)
    assert dt1 is None and torch.equal(do1, do)


def test_constant_target_ties_select_the_first_candidate():
    from srcgan_amd import NearestSelector
    B, C, H, W, shift, stride = R.SHAPES["nonsquare"]
    o = R.int_case("nonsquare", 7)[0].cuda()
    t = torch.full_like(o, 3.0)
    diff, sel, _ = _search(o, t, shift, stride)
    assert bool((diff == diff[:, :1]).all()) and same_values(sel.cpu(), np.zeros((B, 2)))
    out_, tgt_ = NearestSelector(shift, stride).crop(o, t)
    assert tgt_.shape == out_.shape and bool((tgt_ == 3.0).all())


# --------------------------------------------------------------------------- float operands: the fp32 gate, exact selection
@pytest.mark.parametrize("name", NAMES)
def test_float_operands_within_the_gate(name):
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, planted, ref = float_ref(name)
    assert same_values(ref["sel"], planted.numpy())
    diff, sel, loss = _search(o.cuda(), t.cuda(), shift, stride, want_loss=True)
    e_diff, e_loss = rel_err(diff.cpu(), ref["diff"]), abs(float(loss) - ref["loss"]) / ref["loss"]
    print(f"[nearest] {name}: diff rel_err {e_diff:.3g} loss rel {e_loss:.3g}")
    assert within_gate(diff.cpu(), ref["diff"]) and e_loss <= GATE
    assert same_values(sel.cpu(), ref["sel"])
    floss, do, dt = _fused(o.cuda(), t.cuda(), shift, stride)
    assert torch.equal(floss, loss)
    assert within_gate(do.cpu(), ref["dout"]) and within_gate(dt.cpu(), ref["dtgt"])


@pytest.mark.parametrize("case", ["golden", "stride2", "shift3", "nonsquare"])
def test_reference_fixture(case):
    from srcgan_amd import L1Loss, NearestSelector
    g = load_golden("nearest_selector")
    shift, stride = (int(v) for v in g[f"{case}/cfg"])
    x, t = torch.from_numpy(g[f"{case}/x"]).float().cuda(), torch.from_numpy(g[f"{case}/t"]).float().cuda()
    sd, ch, cw, n = R.geometry(x.shape[2], x.shape[3], shift, stride)
    ns = NearestSelector(shift, stride)
    diff = ns.shift_diff(x, t, ch, cw)
    print(f"[nearest] fixture {case}: diff rel_err {rel_err(diff.cpu(), g[f'{case}/diff']):.3g}")
    assert within_gate(diff.cpu(), g[f"{case}/diff"])
    if case == "golden":
        assert torch.argmin(diff, dim=1).tolist() == [3, 10, 13]
    if f"{case}/sel" not in g:
        return
    assert same_values(NearestSelector.unravel_index(diff, n).cpu(), g[f"{case}/sel"])
    xr = x.clone().requires_grad_(True)
    out_, tgt_ = ns.crop(xr, t)
    assert same_values(out_.detach().cpu(), g[f"{case}/out_"]) and same_values(tgt_.cpu(), g[f"{case}/tgt_"])
    loss = L1Loss()(out_, tgt_)
    loss.backward()
    assert abs(float(loss.detach()) - float(g[f"{case}/loss"])) <= GATE * float(g[f"{case}/loss"])
    assert rel_err(xr.grad.cpu(), g[f"{case}/dx"]) <= 1e-6           # signs exact, one scalar 1/N within an ulp
    floss, do, _ = _fused(x, t, shift, stride, target_grad=False)
    assert abs(float(floss) - float(g[f"{case}/loss"])) <= GATE * float(g[f"{case}/loss"])
    assert torch.equal(do, xr.grad)
    # float16 inputs compute in f32 (the values are float16-representable: same bits) and get float16 gradients
    hloss, hdo, hdt = _fused(x.half(), t.half(), shift, stride)
    assert torch.equal(hloss, floss) and hdo.dtype == torch.float16 and hdt.dtype == torch.float16
    assert torch.equal(hdo, do.half())


# --------------------------------------------------------------------------- the two forms, determinism, no synchronisation
def test_crop_is_a_view_and_its_gradient_is_the_fused_one():
    from srcgan_amd import L1Loss, NearestSelector
    name = "tiles"
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, _, ref = float_ref(name)
    x = o.cuda().requires_grad_(True)
    out_, tgt_ = NearestSelector(shift, stride).crop(x, t.cuda())
    assert out_._base is x and out_.untyped_storage().data_ptr() == x.untyped_storage().data_ptr()
    assert out_.requires_grad and not tgt_.requires_grad
    loss = L1Loss()(out_, tgt_)
    loss.backward()
    floss, do, _ = _fused(o.cuda(), t.cuda(), shift, stride, target_grad=False)
    assert torch.equal(x.grad, do)
    assert abs(float(loss.detach()) - float(floss)) <= GATE * float(floss)


def test_two_calls_give_the_same_bits():
    name = "tiles"
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, _, _ = float_ref(name)
    a = _search(o.cuda(), t.cuda(), shift, stride, want_loss=True)
    b = _search(o.cuda(), t.cuda(), shift, stride, want_loss=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    fa, fb = _fused(o.cuda(), t.cuda(), shift, stride), _fused(o.cuda(), t.cuda(), shift, stride)
    assert all(torch.equal(p, q) for p, q in zip(fa, fb))


def test_neither_form_synchronises():
    from srcgan_amd import L1Loss, NearestL1Loss, NearestSelector
    name = "nonsquare"
    B, C, H, W, shift, stride = R.SHAPES[name]
    o, t, _, ref = float_ref(name)
    x1, x2, tg = o.cuda().requires_grad_(True), o.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        l1 = NearestL1Loss(shift, stride)(x1, tg)
        l1.backward()
        l2 = L1Loss()(*NearestSelector(shift, stride).crop(x2, tg.detach()))
        l2.backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(x1.grad, x2.grad) and abs(float(l1.detach()) - ref["loss"]) <= GATE * ref["loss"]


# --------------------------------------------------------------------------- refusals come from the library, before any launch
def test_library_refusals():
    from srcgan_amd import NearestL1Loss, NearestSelector
    x = torch.zeros(1, 1, 24, 24, device="cuda")
    with pytest.raises(RuntimeError, match="shift=5 is not supported.*kept in registers"):
        NearestL1Loss(shift=5)(x, x)
    with pytest.raises(RuntimeError, match="shift=5 is not supported"):
        NearestSelector(shift=5).crop(x, x)
    y = torch.zeros(1, 1, 164, 164, device="cuda")
    with pytest.raises(RuntimeError, match="does not fit in LDS"):
        NearestL1Loss(shift=2, stride=40)(y, y)
    with pytest.raises(RuntimeError, match="does not fit in LDS"):
        NearestSelector(shift=2, stride=40).shift_diff(y, y, 4, 4)
