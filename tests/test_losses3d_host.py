"""CPU: the interface of L1Loss3D / DSSIMLoss3D / VGG16Loss3D -- names, reprs, exports, the shape errors and refusals raised before any
launch, VGG16Loss3D's parameters -- and the new C symbols in the header and in the ctypes table."""
import os
import re

import pytest
import torch

import vgg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["srcgan_dssim3d_scratch_floats", "srcgan_dssim3d_loss_fwd", "srcgan_dssim3d_loss_bwd",
               "srcgan_vggloss_forward_frames", "srcgan_vggloss_backward_frames", "srcgan_vggloss_infer_frames"]


def _vgg3d(**kw):
    from srcgan_amd import VGG16Loss3D
    return VGG16Loss3D(cuda=False, weights=R.seeded_state(0), **kw)


def test_names_reprs_and_exports():
    import srcgan_amd
    from srcgan_amd import losses
    for name, rep in (("L1Loss3D", "L13D"), ("DSSIMLoss3D", "DSSIM3D"), ("VGG16Loss3D", "VGG163D")):
        assert getattr(srcgan_amd, name) is getattr(losses, name)
        assert name in srcgan_amd.__all__ and name in losses.__all__
        m = _vgg3d() if name == "VGG16Loss3D" else getattr(srcgan_amd, name)()
        assert repr(m) == rep
    assert list(srcgan_amd.L1Loss3D().parameters()) == [] and list(srcgan_amd.DSSIMLoss3D().parameters()) == []


@pytest.mark.parametrize("xs, ts", [
    ((1, 3, 16, 16), (1, 3, 16, 16)),                # 4-D
    ((1, 3, 2, 16, 16), (1, 3, 2, 16, 17)),          # mismatched shapes
    ((1, 3, 2, 16, 16), (1, 3, 3, 16, 16)),
])
def test_shape_errors_common(xs, ts):
    from srcgan_amd import L1Loss3D, DSSIMLoss3D
    for m in (L1Loss3D(), DSSIMLoss3D(), _vgg3d()):
        for dev in ("cpu", "meta"):
            with pytest.raises(ValueError):
                m(torch.empty(xs, device=dev), torch.empty(ts, device=dev))


@pytest.mark.parametrize("shape", [(1, 3, 2, 10, 16), (1, 3, 2, 16, 10)])
def test_dssim3d_needs_11_by_11(shape):
    from srcgan_amd import DSSIMLoss3D
    with pytest.raises(ValueError, match="11x11"):
        DSSIMLoss3D()(torch.empty(shape), torch.empty(shape))


@pytest.mark.parametrize("shape", [(1, 3, 2, 7, 16), (1, 3, 2, 16, 7), (1, 2, 2, 16, 16)])
def test_vgg3d_shape_limits(shape):
    with pytest.raises(ValueError):
        _vgg3d()(torch.empty(shape), torch.empty(shape))


def test_cpu_inputs_have_no_fallback():
    from srcgan_amd import L1Loss3D, DSSIMLoss3D
    x, t = torch.rand(1, 3, 2, 16, 16), torch.rand(1, 3, 2, 16, 16)
    for m in (L1Loss3D(), DSSIMLoss3D(), _vgg3d()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x, t)


def test_vgg3d_construction_is_vgg16loss():
    from srcgan_amd import VGG16Loss, VGG16Loss3D
    with pytest.raises(NotImplementedError, match="frozen"):
        VGG16Loss3D(requires_grad=True, cuda=False, weights=R.seeded_state(0))
    with pytest.raises(ValueError):
        _vgg3d(frames_per_pass=0)
    a, b = _vgg3d(frames_per_pass=2), VGG16Loss(cuda=False, weights=R.seeded_state(0))
    assert a.frames_per_pass == 2 and _vgg3d().frames_per_pass is None
    assert list(a.state_dict()) == list(b.state_dict()) == R.VGG16LOSS_KEYS
    assert all(not p.requires_grad for p in a.parameters())
    for k, v in b.state_dict().items():
        assert torch.equal(a.state_dict()[k], v)
    a.load_state_dict(R.to_slice_keys(R.seeded_state(0, seed=3)))        # a checkpoint of the reference loss loads
    with pytest.warns(UserWarning, match="no weights given"):
        VGG16Loss3D(cuda=False)


def test_vgg3d_target_branch_is_frozen():
    x = torch.rand(1, 3, 2, 16, 16)
    with pytest.raises(NotImplementedError, match="frozen"):
        _vgg3d()(x, x.clone().requires_grad_(True))


def test_new_symbols_in_header_and_ctypes_table():
    from srcgan_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srcgan_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(srcgan_[a-z0-9_]+)\s*\(", text))
    for s in NEW_SYMBOLS:
        assert s in declared and s in _native.SIGNATURES, s
    # they are the only entry points of these losses: a 4-D tensor is F = 1
    for s in [f"srcgan_dssim_loss_{d}" for d in ("fwd", "bwd")] + [f"srcgan_vggloss_{d}" for d in ("forward", "infer", "backward")]:
        assert s not in declared and s not in _native.SIGNATURES, s
