"""Host (no GPU): SRDenseNetA / SRDenseNetB -- a CPU restatement of both forwards built from torch.nn.functional, checked against
the reference's fixtures (tests/golden/srdense_*.npz, made by tests/golden/make_golden_srdense.py); the parameter holders' keys,
shapes and seeded weights; the native planner's sizes and its refusals.

The fixtures hold a 64-bucket count sketch of every seeded weight instead of the weight (make_golden_srdense.py explains it):
equal tensors have bit-equal sketches, so the holders are checked for the reference's initialisation bit for bit, and the
restatement then runs on the holders' state_dict.  The 2.4 MB gradient of ``deconv.0.weight`` is stored as its sketch plus its
first output-channel slice; both are compared, the sketch by the relative error of the two sketch vectors (it estimates the
relative L2 error of the tensors)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err
from net_ref import run_l1, sketch

TAGS = ["srdense_a_x2", "srdense_a_x4", "srdense_b_x2", "srdense_b_x4"]
BIG = "deconv.0.weight"


def expected_keys(num_blocks, num_layers):
    """state_dict keys in the reference's order (model/model.py:675-708)."""
    names = ["conv_first", "conv.conv"]
    names += [f"dense_blocks.{i}.block.{j}.conv" for i in range(num_blocks) for j in range(num_layers)]
    names += ["bottleneck.0", "deconv.0", "reconstruction", "conv_last"]
    return [f"{n}.{s}" for n in names for s in ("weight", "bias")]


def restate(sd, x, kind, num_blocks, num_layers, up, store=None):
    """Both forwards from a state_dict (kind 'a': SRDenseNetA, 'b': SRDenseNetB), in the dtype of x.  ``store``: rounding applied to
    every stored activation and to the convolution weights (the storage-rounding yardstick of the 16-bit modes); biases stay exact."""
    rnd = store if store is not None else (lambda v: v)
    w = lambda k: rnd(sd[k + ".weight"].to(x.dtype))
    b = lambda k: sd[k + ".bias"].to(x.dtype)
    conv = lambda v, k, **kw: F.conv2d(v, w(k), b(k), **kw)
    h = rnd(conv(rnd(x), "conv_first", padding=1))
    h = rnd(F.relu(conv(h, "conv.conv", padding=1)))
    for i in range(num_blocks):
        cat = rnd(F.relu(conv(h, f"dense_blocks.{i}.block.0.conv", padding=1)))
        for j in range(1, num_layers):
            cat = torch.cat([cat, rnd(F.relu(conv(cat, f"dense_blocks.{i}.block.{j}.conv", padding=1)))], 1)
        h = torch.cat([h, cat], 1)
    h = rnd(F.relu(conv(h, "bottleneck.0")))
    for _ in range({2: 1, 4: 2}[up]):
        if kind == "a":
            h = rnd(F.relu(F.conv_transpose2d(h, w("deconv.0"), b("deconv.0"), stride=2, padding=1, output_padding=1)))
        else:
            h = rnd(F.relu(conv(h, "deconv.0", stride=2, padding=1)))
    h = rnd(conv(h, "reconstruction", padding=1))
    return conv(h, "conv_last", padding=1)


def restate_run(sd, x, t, kind, nb, nl, up, dtype=torch.float64, store=None):
    """-> (y, loss, dx, {name: grad}) of the restatement under the fixtures' L1 loss."""
    return run_l1(lambda p, xx: restate(p, xx, kind, nb, nl, up, store), sd, x, t, dtype=dtype, missing="absent")


def build_from_fixture(g, tag, dtype=None):
    """The project's module for a fixture, constructed under the fixture's seed (on the CPU: parameter holders only)."""
    import srcgan_amd as S
    ic, oc, growth, nb, nl, up = [int(v) for v in g["cfg"]]
    cls = S.SRDenseNetA if "_a_" in tag else S.SRDenseNetB
    torch.manual_seed(int(g["seed"]))
    return cls(ic, oc, growth_rate=growth, num_blocks=nb, num_layers=nl, mode=f"x{up}", dtype=dtype), ("a" if "_a_" in tag else "b", nb, nl, up)


def check_grads(g, grads, tol, err=rel_err, transposed=True):
    """Every stored gradient of fixture g against ``grads`` (name -> tensor); the large tensor by slice and sketch."""
    for k in [str(n) for n in g["names"]]:
        if k == BIG:
            sl = grads[k][:, 0] if transposed else grads[k][0]
            assert err(sl, g["gslice/" + k]) < tol, k
            assert err(sketch(grads[k]), g["gsketch/" + k]) < tol, k
        else:
            assert err(grads[k], g["grad/" + k]) < tol, k


@pytest.mark.parametrize("tag", TAGS)
def test_holders_have_the_reference_keys_shapes_and_seeded_weights(tag):
    g = load_golden(tag)
    net, (_, nb, nl, _) = build_from_fixture(g, tag)
    sd = net.state_dict()
    assert list(sd) == [str(n) for n in g["names"]] == expected_keys(nb, nl)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(int(n) for n in g["wshape/" + k]), k
        assert np.array_equal(sketch(v), g["wsketch/" + k]), k        # bit for bit
    assert [k for k, _ in net.named_parameters()] == list(sd)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference(tag):
    g = load_golden(tag)
    net, (kind, nb, nl, up) = build_from_fixture(g, tag)
    y, loss, dx, grads = restate_run(net.state_dict(), g["x"], g["t"], kind, nb, nl, up, dtype=torch.float32)
    assert rel_err(y, g["y"]) < 1e-5 and abs(float(loss) - float(g["loss"])) < 1e-5
    assert rel_err(dx, g["dx"]) < 1e-5
    check_grads(g, grads, 1e-5, transposed=kind == "a")
    y64, loss64, dx64, _ = restate_run(net.state_dict(), g["x"], g["t"], kind, nb, nl, up)
    assert rel_err(y64, g["y64"]) < 1e-9 and rel_err(dx64, g["dx64"]) < 1e-9 and abs(float(loss64) - float(g["loss64"])) < 1e-12


def test_default_parameter_count_matches_the_restatements_keys():
    import srcgan_amd as S
    from srcgan_amd import _native as N
    for cls, kind in ((S.SRDenseNetA, 0), (S.SRDenseNetB, 1)):
        net = cls(1, 3)
        keys = expected_keys(8, 8)
        assert list(net.state_dict()) == keys and len(keys) == 2 * (2 + 64 + 4)
        cfg = N.SrDenseCfg(kind, 1, 3, 1, 8, 8, N.F32, 16, 8, 8, 2)
        assert N.lib().srcgan_srdense_num_params(C.byref(cfg)) == len(keys)
        assert net.bottleneck[0].weight.shape == (256, 1152, 1, 1)


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("kind,shape,up", [(0, (2, 5, 7), 2), (0, (2, 5, 7), 4), (1, (2, 13, 18), 2), (1, (1, 10, 14), 4)])
@pytest.mark.parametrize("widths", [(16, 2, 2), (16, 8, 8)])
def test_planner_sizes(kind, shape, up, widths, dtype):
    from srcgan_amd import _native as N
    lib = N.lib()
    B, H, W = shape
    cfg = N.SrDenseCfg(kind, 3, 1, B, H, W, dtype, *widths, up)
    ws, iws, scr = lib.srcgan_srdense_ws_bytes(C.byref(cfg)), lib.srcgan_srdense_infer_ws_bytes(C.byref(cfg)), lib.srcgan_srdense_bwd_scratch_bytes(C.byref(cfg))
    assert ws > 0 and iws > 0 and scr > 0, lib.srcgan_last_error()
    assert iws <= ws
    oh, ow = C.c_int(), C.c_int()
    assert lib.srcgan_srdense_out_hw(C.byref(cfg), C.byref(oh), C.byref(ow)) == 0
    if kind == 0:
        assert (oh.value, ow.value) == (H * up, W * up)
    else:
        for _ in range(up // 2):
            H, W = (H + 1) // 2, (W + 1) // 2
        assert (oh.value, ow.value) == (H, W)


def test_refusals():
    import srcgan_amd as S
    from srcgan_amd import _native as N
    net = S.SRDenseNetA(1, 3, num_blocks=2, num_layers=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.rand(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.SRDenseNetB(3, 1, num_blocks=2, num_layers=2)(torch.rand(1, 3, 4, 4))
    with pytest.raises(NotImplementedError, match="nb_channel must be 1"):
        S.SRDenseNetA(1, 3, nb_channel=2)
    with pytest.raises(ValueError, match="growth_rate must be a multiple of 8"):
        S.SRDenseNetA(1, 3, growth_rate=12)
    with pytest.raises(ValueError, match="multiple of the 64-byte K chunk"):
        S.SRDenseNetB(3, 1, growth_rate=8, num_blocks=2, num_layers=3, dtype="bf16")       # 24-channel slice offsets, 32-channel chunks
    with pytest.raises(NotImplementedError, match="mode"):
        S.SRDenseNetA(1, 3, mode="x3")
    cfg = N.SrDenseCfg(1, 3, 1, 1, 1, 8, N.F32, 16, 2, 2, 2)          # SRDenseNetB on a one-pixel-high image
    assert N.lib().srcgan_srdense_ws_bytes(C.byref(cfg)) == 0 and b"H, W >= 2" in N.lib().srcgan_last_error()


def test_exported_and_registered():
    import srcgan_amd as S
    from srcgan_amd.train import MODEL_REGISTRY
    assert MODEL_REGISTRY["SRDenseNetA"] is S.SRDenseNetA and MODEL_REGISTRY["SRDenseNetB"] is S.SRDenseNetB
    assert "SRDenseNetA" in S.__all__ and "SRDenseNetB" in S.__all__
