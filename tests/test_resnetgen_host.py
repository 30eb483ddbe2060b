"""CPU: the native ResnetGenerator / define_G without a GPU -- the reference's state_dict keys in its order, its seeded weights (the
fixtures' sketches), define_G's routing, every refusal with its message, the planners' answers and receptive_halo's refusal."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import resnetgen_ref as R
import srcgan_amd
from conftest import load_golden
from srcgan_amd import _native as N
from test_resnetgen_ref import FIXTURES, native

IN = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)


@pytest.mark.parametrize("tag", FIXTURES)
def test_keys_order_and_seeded_weights_match_the_fixture(tag):
    z = load_golden(tag)
    sd = native(z).state_dict()
    assert list(sd) == [str(n) for n in z["names"]]
    assert len(sd) == {"resnetgen_1to3": 36, "resnetgen_3to1": 48}[tag]
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(int(s) for s in z["wshape/" + k]), k
        assert np.array_equal(R.sketch(v.numpy()), z["wsketch/" + k]), k


def test_the_holder_is_the_reference_sequential():
    m = srcgan_amd.ResnetGenerator(1, 3, 16, norm_layer=IN, n_blocks=6)
    assert isinstance(m.model, nn.Sequential) and len(m.model) == 25
    assert isinstance(m.model[0], nn.ReflectionPad2d) and isinstance(m.model[22], nn.ReflectionPad2d) and isinstance(m.model[24], nn.Tanh)
    assert isinstance(m.model[16], nn.ConvTranspose2d) and m.model[16].weight.shape == (64, 32, 3, 3)
    assert list(m.state_dict()) == R.names(6)
    assert [k for k, _ in m.named_parameters()] == R.names(6)
    z = srcgan_amd.ResnetGenerator(3, 1, 32, norm_layer=nn.InstanceNorm2d, n_blocks=2, padding_type="zero")
    assert list(z.state_dict()) == R.names(2, "zero") and len(z.model[10].conv_block) == 5
    assert list(srcgan_amd.ResnetGenerator(1, 1, 16, norm_layer=IN, n_blocks=0).state_dict()) == R.names(0)


def test_define_G_routes():
    a = srcgan_amd.define_G(1, 3, 16, "resnet_9blocks", "instance", False, "normal", 0.02)
    b = srcgan_amd.define_G(3, 1, 16, "resnet_6blocks", norm="instance")
    assert isinstance(a, srcgan_amd.ResnetGenerator) and a._cfg == (1, 3, 16, 9, 0) and len(a.state_dict()) == 48
    assert isinstance(b, srcgan_amd.ResnetGenerator) and b._cfg == (3, 1, 16, 6, 0)
    assert all(float(p.detach().abs().max()) == 0.0 for k, p in a.named_parameters() if k.endswith("bias"))         # init_weights: biases zero
    assert 0.015 < float(a.model[1].weight.detach().std()) < 0.025                                                   # N(0, 0.02)
    for name in ("unet_128", "unet_256"):
        with pytest.raises(NotImplementedError, match="UnetGenerator is not native"):
            srcgan_amd.define_G(1, 3, 16, name, "instance")
    with pytest.raises(NotImplementedError, match=r"Generator model name \[resnet_3blocks\] is not recognized"):
        srcgan_amd.define_G(1, 3, 16, "resnet_3blocks", "instance")
    with pytest.raises(NotImplementedError, match=r"normalization layer \[layer\] is not found"):
        srcgan_amd.define_G(1, 3, 16, "resnet_9blocks", "layer")
    with pytest.raises(NotImplementedError, match="BatchNorm2d"):             # define_G's own default, norm='batch'
        srcgan_amd.define_G(1, 3, 16, "resnet_9blocks")
    with pytest.raises(NotImplementedError, match=r"initialization method \[uniform\] is not implemented"):
        srcgan_amd.define_G(1, 3, 16, "resnet_6blocks", "instance", init_type="uniform")
    part = srcgan_amd.get_norm_layer("instance")
    assert part.func is nn.InstanceNorm2d and part.keywords == dict(affine=False, track_running_stats=False)
    assert srcgan_amd.get_norm_layer("batch").func is nn.BatchNorm2d
    assert isinstance(srcgan_amd.get_norm_layer("none")(16), nn.Module)
    net = nn.Sequential(nn.Conv2d(2, 2, 1), nn.BatchNorm2d(2))
    assert srcgan_amd.init_net(net, "xavier", 0.5) is net and float(net[0].bias.detach().abs().max()) == 0.0
    assert abs(float(net[1].weight.detach().mean()) - 1.0) < 2.0 and float(net[1].bias.detach().abs().max()) == 0.0        # BatchNorm2d: N(1, gain), 0


@pytest.mark.parametrize("kw, what", [
    (dict(), "BatchNorm2d"),                                                  # the class default, as in the reference
    (dict(norm_layer=nn.BatchNorm2d), "BatchNorm2d"),
    (dict(norm_layer=functools.partial(nn.BatchNorm2d, affine=True, track_running_stats=True)), "BatchNorm2d"),
    (dict(norm_layer=srcgan_amd.get_norm_layer("none")), "identity norm"),
    (dict(norm_layer=functools.partial(nn.InstanceNorm2d, affine=True)), "affine=True"),
    (dict(norm_layer=IN, padding_type="replicate"), "'replicate'"),
    (dict(norm_layer=IN, padding_type="circular"), r"padding \[circular\] is not implemented"),
    (dict(norm_layer=IN, use_dropout=True), "use_dropout=True"),
])
def test_options_that_are_not_native_raise_and_name_the_option(kw, what):
    with pytest.raises(NotImplementedError, match=what):
        srcgan_amd.ResnetGenerator(1, 3, 16, **kw)


def _cfg(in_ch=1, out_ch=3, B=2, H=8, W=12, dtype=0, ngf=16, n_blocks=6, padding=0):
    return N.ResnetGenCfg(in_ch, out_ch, B, H, W, dtype, ngf, n_blocks, padding)


@pytest.mark.parametrize("kw, what", [
    (dict(H=10), "multiples of 4"), (dict(W=6), "multiples of 4"), (dict(H=4), "at least 8"), (dict(H=9), "multiples of 4"),
    (dict(ngf=24), "multiple of 16"), (dict(ngf=0), "multiple of 16"),
    (dict(in_ch=0), "1..8"), (dict(in_ch=9), "1..8"), (dict(out_ch=0), "1..8"), (dict(out_ch=9), "1..8"),
    (dict(n_blocks=-1), "n_blocks"), (dict(padding=2), "padding"), (dict(dtype=7), "dtype"), (dict(B=0), "B/H/W"),
])
def test_the_planner_refuses_with_a_message(kw, what):
    lib, c = N.lib(), _cfg(**kw)
    assert lib.srcgan_resnetgen_num_params(C.byref(c)) == -1
    assert what in lib.srcgan_last_error().decode()
    assert lib.srcgan_resnetgen_ws_bytes(C.byref(c)) == 0 and lib.srcgan_resnetgen_bwd_scratch_bytes(C.byref(c)) == 0
    assert lib.srcgan_resnetgen_infer_ws_bytes(C.byref(c)) == 0 and lib.srcgan_resnetgen_infer_act_bytes(C.byref(c)) == 0
    assert lib.srcgan_resnetgen_infer_plan(C.byref(c), None, 0) == -1


def test_class_level_refusals_come_from_the_planner():
    with pytest.raises(ValueError, match="ngf = 24 must be a multiple of 16"):
        srcgan_amd.ResnetGenerator(1, 3, 24, norm_layer=IN)
    with pytest.raises(ValueError, match="must be in 1..8"):
        srcgan_amd.ResnetGenerator(9, 3, 16, norm_layer=IN)


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("n_blocks, padding", [(6, 0), (9, 0), (0, 0), (2, 1)])
def test_planners_answer_on_the_cpu(dtype, n_blocks, padding):
    lib, c = N.lib(), _cfg(dtype=dtype, n_blocks=n_blocks, padding=padding)
    assert lib.srcgan_resnetgen_num_params(C.byref(c)) == 2 * (6 + 2 * n_blocks) == len(R.names(n_blocks))
    ws, scr = lib.srcgan_resnetgen_ws_bytes(C.byref(c)), lib.srcgan_resnetgen_bwd_scratch_bytes(C.byref(c))
    iws, iact = lib.srcgan_resnetgen_infer_ws_bytes(C.byref(c)), lib.srcgan_resnetgen_infer_act_bytes(C.byref(c))
    assert ws > 0 and scr > 0 and 0 < iact < iws < ws and ws % 256 == 0 and iws % 256 == 0
    # ops: 3 stem pairs, per block 2 convolutions + 2 norms (+ 2 pads), 2 x (deconv + norm), and pad / pad + conv + tanh around them
    nops = 1 + 6 + n_blocks * (4 if padding else 6) + 4 + 3
    assert lib.srcgan_resnetgen_infer_plan(C.byref(c), None, 0) == nops
    r = (C.c_size_t * (6 * nops))()
    assert lib.srcgan_resnetgen_infer_plan(C.byref(c), r, nops) == nops
    for k in range(nops):                                  # an op's output slot never overlaps its operands
        (i0, ib, r0, rb, o0, ob) = r[6 * k:6 * k + 6]
        assert ob > 0 and ib > 0 and (o0 + ob <= i0 or i0 + ib <= o0) and (rb == 0 or o0 + ob <= r0 or r0 + rb <= o0)
        assert o0 + ob <= iact


def test_inference_memory_does_not_grow_with_the_depth():
    lib = N.lib()
    a, b = (lib.srcgan_resnetgen_infer_act_bytes(C.byref(_cfg(H=32, W=32, ngf=64, n_blocks=n, dtype=1))) for n in (2, 9))
    assert a == b
    t2, t9 = (lib.srcgan_resnetgen_ws_bytes(C.byref(_cfg(H=32, W=32, ngf=64, n_blocks=n, dtype=1))) for n in (2, 9))
    assert t9 > t2


def test_receptive_halo_refuses_and_the_scale_is_one():
    from srcgan_amd import infer
    m = srcgan_amd.ResnetGenerator(1, 3, 16, norm_layer=IN, n_blocks=1)
    with pytest.raises(ValueError, match="normalisation layers whose per-image statistics make tiles inexact"):
        srcgan_amd.receptive_halo(m)
    assert infer._scale(m) == 1


def test_a_cpu_tensor_is_refused_not_run_on_a_fallback():
    m = srcgan_amd.ResnetGenerator(1, 3, 16, norm_layer=IN, n_blocks=1)
    with pytest.raises((RuntimeError, ValueError)):
        m(torch.zeros(1, 1, 8, 8))
