"""GPU: every public front end that takes a user tensor, on the forms of tests/input_forms.py (a contiguous view at a 4-byte phase, a
batch slice, a W-sliced view, channels-last, a stride-0 expand, bf16 / fp16, a non-leaf that requires grad) against the same call on a
fresh contiguous f32 clone: the same bits out, the clone's gradient placed into the view's base, the caller's tensors unchanged.  The
flat reductions, whose summation order follows the pointer phase, are held to equality on the 1/16 grid and to their float64 bound on
reals (the table names them and says why)."""
import numpy as np
import pytest
import torch

import input_forms as F

pytestmark = pytest.mark.gpu
PASSTHROUGH = {"NearestSelector.crop": (0,)}         # outputs that are views of the user's own tensor keep its dtype
_MADE = {}


def _subject(name):
    if name not in _MADE:
        _MADE[name] = F.BY_NAME[name].make()
    return _MADE[name]


def _flat(out):
    if isinstance(out, dict):
        return [out[k] for k in sorted(out)]
    return list(out) if isinstance(out, (tuple, list)) else [out]


def _run(s, fn, tensors):
    """-> (outputs, gradients of s.grad's arguments w.r.t. the given leaves or None).  The upstream gradient is 3 for a scalar and a
    fixed pattern for a tensor."""
    outs = _flat(fn(*tensors))
    if s.grad:
        y = outs[0]
        w = torch.full_like(y, 3.0) if y.dim() == 0 else ((torch.arange(y.numel(), device=y.device) % 7).float() - 3).view(y.shape)
        y.backward(w)
    return [o.detach() for o in outs]


def _inputs(s, form, grid):
    vals = [F.values(shape, 10 * i + 1, grid, s.lo, s.hi, s.u8) for i, shape in enumerate(s.shapes)]
    if form == "expand":
        vals = [v.narrow(s.cdim, 0, 1).expand(v.shape).contiguous() for v in vals]
    return vals


def _one(s, fn, form, grid):
    vals = _inputs(s, form, grid)
    forms = [F.Form(form, v, s.cdim) for v in vals]
    clones = [f.clone().requires_grad_(i in s.grad) for i, f in enumerate(forms)]
    want = _run(s, fn, clones)
    # what requires grad: the arguments whose gradient is checked, else (the front end detaches) the first
    views = [f.view(i in s.grad or (not s.grad and i == 0 and form == "nonleaf")) for i, f in enumerate(forms)]
    if form == "phase4":
        assert all(v.data_ptr() % 16 == (4 if not s.u8 else 1) and v.is_contiguous() for v in views)
    if form == "wslice":
        assert not any(v.is_contiguous() for v in views)
    got = _run(s, fn, views)
    phases = [v.data_ptr() % 16 for v in views]
    return forms, clones, want, got, phases


@pytest.mark.parametrize("name,form", F.CASES, ids=[f"{n}-{f}" for n, f in F.CASES])
def test_form_matches_the_contiguous_clone(name, form):
    s, fn = F.BY_NAME[name], _subject(name)
    if form in ("bf16", "fp16") and s.refuse16 is not None:
        exc, words = s.refuse16
        vals = _inputs(s, form, True)
        with pytest.raises(exc, match=words):
            fn(*[F.Form(form, v, s.cdim).view(False) for v in vals])
        return
    exempt_here = s.exempt is not None and form in F.PHASE_FORMS
    datasets = [True] if form in ("bf16", "fp16") else ([True, False] if exempt_here else [False])
    for grid in datasets:
        forms, clones, want, got, phases = _one(s, fn, form, grid)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape, (name, form, k, g.shape, w.shape)
            if g.dtype != w.dtype:
                assert k in PASSTHROUGH.get(name, ()), (name, form, k, g.dtype, w.dtype)
                g = g.float()
            if exempt_here and k == 0 and not (grid and s.exact_on_grid):
                arrays = [c.detach().cpu().numpy() for c in clones]
                ref, allowed = s.bound(arrays, phases)
                ref0, allowed0 = s.bound(arrays, [0] * len(phases))
                err, err0 = abs(float(g) - ref), abs(float(w) - ref0)
                print(f"[input_forms] {name} {form} {'grid' if grid else 'reals'}: view {err:.3e} of {allowed:.3e}, clone {err0:.3e} of {allowed0:.3e}")
                assert err <= allowed and err0 <= allowed0, (name, form, float(g), float(w), ref)
            else:
                assert torch.equal(g, w), (name, form, k, "grid" if grid else "reals", (g.double() - w.double()).abs().max().item())
        for i in s.grad:
            gb, gc = forms[i].base.grad, clones[i].grad
            assert gc is not None and gb is not None, (name, form, i)
            assert gb.shape == forms[i].base.shape and gb.dtype == forms[i].base.dtype
            exp = forms[i].expected_grad(gc)
            assert torch.equal(gb, exp), (name, form, i, (gb.double() - exp.double()).abs().max().item())
        for f in forms:
            assert f.unchanged(), (name, form)


def test_to_nchw_reads_a_channel_slice_as_the_slice():
    """The defect this file was written for: ``ops.to_nchw`` took ``data_ptr()`` of a strided NHWC view and read it as if dense."""
    from srcgan_amd import ops
    big = F.values((2, 5, 7, 12), 3, False)
    v = big[..., 2:10]
    assert not v.is_contiguous()
    assert torch.equal(ops.to_nchw(v), v.permute(0, 3, 1, 2).contiguous())
    assert torch.equal(ops.to_nchw(v, 3, 1), v[..., 1:4].permute(0, 3, 1, 2).contiguous())


def test_every_subject_of_the_issue_is_in_the_table():
    from srcgan_amd import losses
    names = {s.name.split("-")[0].split(".")[0] for s in F.SUBJECTS} | {s.name for s in F.SUBJECTS}
    for cls in losses.__all__:
        assert cls in names, cls
    for n in ("metrics.AE", "metrics.MSE", "metrics.PSNR", "metrics.SSIM", "metrics.score_scene", "ops.rgb_to_gray", "ops.bilinear_down",
              "ops.bilinear_up", "ops.nearest_resize", "ops.to_nhwc", "ops.to_nchw", "data.arr2gray", "data.arr2rgb", "data.arr2lab",
              "data.arr2ab", "data.lab2img", "infer.upscale_scene", "RDDBNet", "NLayerDiscriminator", "ESPCN", "EDSR"):
        assert n in names, n
    for s in F.SUBJECTS:
        assert (s.exempt is None) == (s.bound is None), s.name
