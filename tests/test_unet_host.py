"""CPU: the native UnetGenerator without a GPU -- the reference's nested state_dict keys in its order, its seeded weights (the fixtures'
sketches), every refusal with its message, the planners' answers, receptive_halo's refusal, the exports and the header, and define_G's
standing refusal that names the replacement."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import srcgan_amd
import unet_ref as R
from conftest import load_golden
from srcgan_amd import _native as N
from test_unet_ref import FIXTURES, native

IN = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)


@pytest.mark.parametrize("tag", FIXTURES)
def test_keys_order_and_seeded_weights_match_the_fixture(tag):
    z = load_golden(tag)
    sd = native(z).state_dict()
    assert list(sd) == [str(n) for n in z["names"]]
    assert len(sd) == {"unet_d5_1to3": 20, "unet_d6_3to1": 24}[tag]
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(int(s) for s in z["wshape/" + k]), k
        assert np.array_equal(R.sketch(v.numpy()), z["wsketch/" + k]), k


def test_the_holder_nests_as_the_reference_does():
    m = srcgan_amd.UnetGenerator(1, 3, 5, 16, norm_layer=IN)
    assert list(m.state_dict()) == R.names(5) and [k for k, _ in m.named_parameters()] == R.names(5)
    assert list(m.state_dict())[:3] == ["model.model.0.weight", "model.model.0.bias", "model.model.1.model.1.weight"]
    assert list(m.state_dict())[4] == "model.model.1.model.3.model.1.weight" and list(m.state_dict())[-1] == "model.model.3.bias"
    outer = m.model.model
    assert isinstance(outer, nn.Sequential) and len(outer) == 5 and isinstance(outer[0], nn.Conv2d) and isinstance(outer[4], nn.Tanh)
    assert outer[0].weight.shape == (16, 1, 4, 4) and isinstance(outer[3], nn.ConvTranspose2d) and outer[3].weight.shape == (32, 3, 4, 4)
    mid = outer[1].model
    assert len(mid) == 7 and isinstance(mid[0], nn.LeakyReLU) and mid[0].negative_slope == 0.2 and isinstance(mid[2], nn.InstanceNorm2d)
    assert mid[1].weight.shape == (32, 16, 4, 4) and mid[5].weight.shape == (64, 16, 4, 4)
    inner = mid[3].model[3].model[3].model
    assert len(inner) == 5 and inner[1].weight.shape == (128, 128, 4, 4) and inner[3].weight.shape == (128, 128, 4, 4)         # C_n inputs, not 2 C_n
    assert isinstance(inner[4], nn.InstanceNorm2d) and not any(isinstance(l, nn.InstanceNorm2d) for l in inner[:4])            # no down norm
    with pytest.raises(NotImplementedError, match="parameter holder"):         # the inner blocks have no native forward
        outer[1](torch.zeros(1, 16, 16, 16))
    # seven levels, ngf 64: unet_128's widths
    w = [tuple(v.shape) for k, v in srcgan_amd.UnetGenerator(3, 3, 7, 64, norm_layer=nn.InstanceNorm2d).state_dict().items() if k.endswith("weight")]
    assert [s[0] for s in w[:7]] == [64, 128, 256, 512, 512, 512, 512] and [s[:2] for s in w[7:]] == [(512, 512), (1024, 512), (1024, 512), (1024, 256), (512, 128), (256, 64), (128, 3)]


def test_init_net_works_on_it_and_the_replacement_line_builds_the_class():
    torch.manual_seed(0)
    m = srcgan_amd.init_net(srcgan_amd.UnetGenerator(1, 3, 7, 16, norm_layer=srcgan_amd.get_norm_layer("instance")), "normal", 0.02)
    assert isinstance(m, srcgan_amd.UnetGenerator) and m._cfg == (1, 3, 16, 7) and len(m.state_dict()) == 28 == len(R.names(7))
    assert all(float(p.detach().abs().max()) == 0.0 for k, p in m.named_parameters() if k.endswith("bias"))
    assert 0.015 < float(m.model.model[0].weight.detach().std()) < 0.025


def test_define_G_still_refuses_and_names_the_replacement():
    for name, nd in (("unet_128", 7), ("unet_256", 8)):
        with pytest.raises(NotImplementedError, match="UnetGenerator is not native") as e:
            srcgan_amd.define_G(1, 3, 16, name, "instance")
        assert f"init_net(UnetGenerator(input_nc, output_nc, {nd}, ngf, norm_layer=get_norm_layer(norm)), init_type, init_gain)" in str(e.value)
    assert "init_net(UnetGenerator(" in srcgan_amd.define_G.__doc__


@pytest.mark.parametrize("kw, what", [
    (dict(), "BatchNorm2d"),                                                  # the class default, as in the reference
    (dict(norm_layer=nn.BatchNorm2d), "BatchNorm2d"),
    (dict(norm_layer=functools.partial(nn.BatchNorm2d, affine=True, track_running_stats=True)), "BatchNorm2d"),
    (dict(norm_layer=srcgan_amd.get_norm_layer("none")), "identity norm"),
    (dict(norm_layer=functools.partial(nn.InstanceNorm2d, affine=True)), "affine=True"),
    (dict(norm_layer=functools.partial(nn.InstanceNorm2d, track_running_stats=True)), "track_running_stats=True"),
    (dict(norm_layer=IN, use_dropout=True), "use_dropout=True"),
])
def test_options_that_are_not_native_raise_and_name_the_option(kw, what):
    with pytest.raises(NotImplementedError, match=what):
        srcgan_amd.UnetGenerator(1, 3, 5, 16, **kw)


def _cfg(in_ch=1, out_ch=3, B=2, H=32, W=32, dtype=0, ngf=16, num_downs=5):
    return N.UnetCfg(in_ch, out_ch, B, H, W, dtype, ngf, num_downs)


@pytest.mark.parametrize("kw, what", [
    (dict(num_downs=4, H=16, W=16), "num_downs = 4 must be at least 5"), (dict(H=48), "multiples of 2^num_downs = 32"),
    (dict(W=16), "multiples of 2^num_downs"), (dict(H=0), "B/H/W"), (dict(num_downs=6), "multiples of 2^num_downs = 64"),
    (dict(ngf=24), "multiple of 16"), (dict(ngf=0), "multiple of 16"), (dict(ngf=48), "multiple of 16"),
    (dict(in_ch=0), "1..8"), (dict(in_ch=9), "1..8"), (dict(out_ch=0), "1..8"), (dict(out_ch=9), "1..8"), (dict(dtype=7), "dtype"),
])
def test_the_planner_refuses_with_a_message(kw, what):
    lib, c = N.lib(), _cfg(**kw)
    assert lib.srcgan_unet_num_params(C.byref(c)) == -1
    assert what in lib.srcgan_last_error().decode()
    assert lib.srcgan_unet_ws_bytes(C.byref(c)) == 0 and lib.srcgan_unet_bwd_scratch_bytes(C.byref(c)) == 0
    assert lib.srcgan_unet_infer_ws_bytes(C.byref(c)) == 0 and lib.srcgan_unet_infer_act_bytes(C.byref(c)) == 0
    assert lib.srcgan_unet_infer_plan(C.byref(c), None, 0) == -1


def test_class_level_refusals_come_from_the_planner():
    with pytest.raises(ValueError, match="num_downs = 4 must be at least 5"):
        srcgan_amd.UnetGenerator(1, 3, 4, 16, norm_layer=IN)
    with pytest.raises(ValueError, match="ngf = 24 must be a multiple of 16"):
        srcgan_amd.UnetGenerator(1, 3, 5, 24, norm_layer=IN)
    with pytest.raises(ValueError, match="must be in 1..8"):
        srcgan_amd.UnetGenerator(9, 3, 5, 16, norm_layer=IN)
    with pytest.raises(ValueError, match="must be in 1..8"):
        srcgan_amd.UnetGenerator(1, 9, 5, 16, norm_layer=IN)


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("n, side", [(5, 32), (6, 64), (7, 128)])
def test_planners_answer_on_the_cpu(dtype, n, side):
    lib, c = N.lib(), _cfg(dtype=dtype, num_downs=n, H=side, W=2 * side)
    assert lib.srcgan_unet_num_params(C.byref(c)) == 4 * n == len(R.names(n))
    ws, scr = lib.srcgan_unet_ws_bytes(C.byref(c)), lib.srcgan_unet_bwd_scratch_bytes(C.byref(c))
    iws, iact = lib.srcgan_unet_infer_ws_bytes(C.byref(c)), lib.srcgan_unet_infer_act_bytes(C.byref(c))
    assert ws > 0 and scr > 0 and 0 < iact < iws < ws and ws % 256 == 0 and iws % 256 == 0
    # ops: n down convolutions, the outermost ReLU, n - 2 two-output norms, n transposed convolutions, n - 1 up norms, tanh
    nops = n + 1 + (n - 2) + n + (n - 1) + 1
    assert lib.srcgan_unet_infer_plan(C.byref(c), None, 0) == nops
    r = (C.c_size_t * (6 * nops))()
    assert lib.srcgan_unet_infer_plan(C.byref(c), r, nops) == nops
    for k in range(nops):                                  # an op's output slot never overlaps its operands
        (i0, ib, r0, rb, o0, ob) = r[6 * k:6 * k + 6]
        assert ob > 0 and ib > 0 and (o0 + ob <= i0 or i0 + ib <= o0) and rb == 0
        assert o0 + ob <= iact


def test_the_skip_buffers_stay_alive_until_their_transposed_convolution():
    """slot plan at five levels: the skip buffer R_l is the output of the ReLU / of the up norm at level l and the input of level l's
    transposed convolution; between its first writer and that reader no other op's output may land in it"""
    lib, c, n = N.lib(), _cfg(dtype=1), 5
    nops = lib.srcgan_unet_infer_plan(C.byref(c), None, 0)
    r = (C.c_size_t * (6 * nops))()
    lib.srcgan_unet_infer_plan(C.byref(c), r, nops)
    ops = [tuple(r[6 * k:6 * k + 6]) for k in range(nops)]
    # op order: conv, relu, (conv, norm_skip) x (n - 2), conv, (deconv, norm) x (n - 1), deconv, tanh
    first_up = 2 + 2 * (n - 2) + 1
    deconvs = [first_up + 2 * j for j in range(n)]
    relu_out = ops[1][4:6]
    assert relu_out == ops[deconvs[-1]][0:2]               # R_1: written by the ReLU, read by the last transposed convolution
    for k in range(2, deconvs[-1]):
        o0, ob = ops[k][4:6]
        assert o0 + ob <= relu_out[0] or relu_out[0] + relu_out[1] <= o0 or (o0, ob) == tuple(relu_out), k
    for j in range(1, n - 1):                              # the up norm at level l writes into the buffer the deconv of level l reads
        assert ops[deconvs[j] - 1][4:6] == ops[deconvs[j]][0:2]


def test_receptive_halo_refuses_and_the_scale_is_one():
    from srcgan_amd import infer
    m = srcgan_amd.UnetGenerator(1, 3, 5, 16, norm_layer=IN)
    with pytest.raises(ValueError, match="normalisation layers whose per-image statistics make tiles inexact"):
        srcgan_amd.receptive_halo(m)
    assert infer._scale(m) == 1 and m.num_downs == 5


def test_exports_and_header_declarations():
    from srcgan_amd import model
    assert "UnetGenerator" in model.__all__ and "UnetGenerator" in srcgan_amd.__all__ and srcgan_amd.UnetGenerator is model.UnetGenerator
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "srcgan_amd.h")) as f:
        header = f.read()
    for sym in ("srcgan_in_skip_forward", "srcgan_relu_nhwc", "srcgan_unet_num_params", "srcgan_unet_ws_bytes", "srcgan_unet_bwd_scratch_bytes",
                "srcgan_unet_forward", "srcgan_unet_backward", "srcgan_unet_infer_ws_bytes", "srcgan_unet_infer_act_bytes", "srcgan_unet_infer_plan",
                "srcgan_unet_infer"):
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in N.SIGNATURES and hasattr(N.lib(), sym), sym
    assert "typedef struct srcgan_unet_cfg" in header
    assert [f[0] for f in N.UnetCfg._fields_] == ["in_ch", "out_ch", "B", "H", "W", "dtype", "ngf", "num_downs"]


def test_a_cpu_tensor_is_refused_not_run_on_a_fallback():
    m = srcgan_amd.UnetGenerator(1, 3, 5, 16, norm_layer=IN)
    with pytest.raises((RuntimeError, ValueError)):
        m(torch.zeros(1, 1, 32, 32))
