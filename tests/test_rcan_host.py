"""CPU: RCAN through the C ABI's host code and the Python class -- parameter count and order, refused configurations, the inference
planner's ranges and depth-independent activation size, the seeded weights, and what infer.py knows about the network.  Also pins
tests/rcan_ref.py (our float64 restatement) to the three reference fixtures, so the GPU tests never need the reference."""
import ctypes as C

import numpy as np
import pytest
import torch

import rcan_ref
from conftest import load_golden, rel_l2
from rcan_ref import sketch

FIXTURES = ("rcan_x2", "rcan_x3", "rcan_x4")


@pytest.fixture(scope="module")
def lib():
    from srcgan_amd import _native as N
    return N.lib()


def make(z, **kw):
    import srcgan_amd
    ng, nb, F, red, scale = (int(v) for v in z["cfg"])
    torch.manual_seed(int(z["seed"]))
    return srcgan_amd.RCAN(n_resgroups=ng, n_resblocks=nb, n_feats=F, reduction=red, scale=scale, rgb_range=1, **kw)


def cfg_of(N, groups=2, blocks=2, feats=32, reduction=8, scale=2, colors=3, B=2, H=9, W=7, dtype=None):
    return N.RcanCfg(colors, colors, B, H, W, N.F32 if dtype is None else dtype, groups, blocks, feats, reduction, scale)


@pytest.mark.parametrize("tag", FIXTURES)
def test_parameter_count_names_and_order(lib, tag):
    from srcgan_amd import _native as N
    z = load_golden(tag)
    m = make(z)
    names = [str(n) for n in z["names"]]
    assert list(m.state_dict().keys()) == names
    assert [k for k, _ in m.named_parameters()] == names                     # parameters() order = what the native planner indexes
    cfg = cfg_of(N, scale=int(z["cfg"][4]))
    assert lib.srcgan_rcan_num_params(C.byref(cfg)) == len(names)
    assert [k for k, p in m.named_parameters() if not p.requires_grad] == [str(n) for n in z["frozen"]]
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(z["wshape/" + k])


@pytest.mark.parametrize("tag", FIXTURES)
def test_same_seed_same_weights(tag):
    z = load_golden(tag)
    m = make(z)
    for k, v in m.state_dict().items():
        assert np.array_equal(sketch(v.numpy()), z["wsketch/" + k]), k


@pytest.mark.parametrize("kw, word", [(dict(colors=1), b"n_colors"), (dict(scale=5), b"scale"), (dict(feats=24), b"n_feats"),
                                      (dict(feats=32, reduction=33), b"reduction")])
def test_refused_configurations_name_the_entry_point(lib, kw, word):
    from srcgan_amd import _native as N
    cfg = cfg_of(N, **kw)
    for fn, bad in ((lib.srcgan_rcan_num_params, -1), (lib.srcgan_rcan_ws_bytes, 0), (lib.srcgan_rcan_infer_ws_bytes, 0)):
        assert fn(C.byref(cfg)) == bad
        err = lib.srcgan_last_error()
        assert b"srcgan_rcan" in err and word in err, err


def test_constructor_refuses_what_the_planner_refuses():
    import srcgan_amd
    for kw in (dict(n_colors=1), dict(scale=5), dict(n_feats=24), dict(n_feats=32, reduction=64)):
        with pytest.raises(ValueError, match="srcgan_rcan"):
            srcgan_amd.RCAN(n_resgroups=1, n_resblocks=1, **{"n_feats": 32, "reduction": 8, **kw})


def test_args_object_and_scale_list():
    import types
    import srcgan_amd
    args = types.SimpleNamespace(n_resgroups=1, n_resblocks=1, n_feats=16, reduction=4, scale=[3, 2], rgb_range=1, n_colors=3, res_scale=0.5)
    m = srcgan_amd.RCAN(args)
    assert m.scale == 3 and m.res_scale == 0.5
    assert torch.equal(m.sub_mean.bias, -torch.tensor([0.4488, 0.4371, 0.4040])) and m.add_mean.weight.grad is None


@pytest.mark.parametrize("scale", [2, 3, 4, 8])
def test_infer_plan_outputs_overlap_no_operand(lib, scale):
    from srcgan_amd import _native as N
    cfg = cfg_of(N, groups=3, blocks=3, scale=scale, dtype=N.BF16)
    n = lib.srcgan_rcan_infer_plan(C.byref(cfg), None, 0)
    assert n == 2 + 1 + 3 * (3 * 3 + 1) + 1 + (2 if scale == 3 else 2 * {2: 1, 4: 2, 8: 3}[scale]) + 1
    r = (C.c_size_t * (6 * n))()
    assert lib.srcgan_rcan_infer_plan(C.byref(cfg), r, n) == n
    act = lib.srcgan_rcan_infer_act_bytes(C.byref(cfg))
    for k in range(n):
        io, ib, ro, rb, oo, ob = r[6 * k:6 * k + 6]
        assert ob > 0 and oo + ob <= act
        assert oo + ob <= io or io + ib <= oo, k
        if rb:
            assert oo + ob <= ro or ro + rb <= oo, k


def test_infer_activation_bytes_do_not_grow_with_depth(lib):
    from srcgan_amd import _native as N
    act = {gb: lib.srcgan_rcan_infer_act_bytes(C.byref(cfg_of(N, groups=gb[0], blocks=gb[1], feats=64, reduction=16, B=2, H=24, W=20, dtype=N.BF16)))
           for gb in ((1, 1), (2, 2), (3, 5), (10, 20))}
    assert act[(2, 2)] == act[(3, 5)] == act[(10, 20)] > 0
    assert 0 < act[(1, 1)] <= act[(2, 2)]
    train = lib.srcgan_rcan_ws_bytes(C.byref(cfg_of(N, groups=10, blocks=20, feats=64, reduction=16, B=2, H=24, W=20, dtype=N.BF16)))
    assert act[(10, 20)] < train / 10


def test_exported_and_known_to_infer():
    import srcgan_amd
    from srcgan_amd import infer, model, train
    assert "RCAN" in srcgan_amd.__all__ and "RCAN" in model.__all__ and srcgan_amd.RCAN is model.RCAN
    assert "RCAN" not in train.MODEL_REGISTRY
    for scale in (2, 3, 4):
        m = srcgan_amd.RCAN(n_resgroups=1, n_resblocks=1, n_feats=16, reduction=4, scale=scale)
        assert infer._scale(m) == scale
        with pytest.raises(ValueError, match="pass halo="):
            infer.receptive_halo(m)


def test_tolerant_loader():
    import srcgan_amd
    m = srcgan_amd.RCAN(n_resgroups=1, n_resblocks=1, n_feats=16, reduction=4, scale=2)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    before = m.tail[0][0].weight.detach().clone()
    sd["tail.0.0.weight"] = torch.zeros(144, 16, 3, 3)                       # a x3 checkpoint's up-sampler
    sd["head.0.bias"] = torch.full((16,), 2.0)
    sd["sub_mean.bias"] = torch.tensor([-1.0, -2.0, -3.0])
    m.load_state_dict(sd)
    assert torch.equal(m.tail[0][0].weight, before) and bool((m.head[0].bias == 2).all())
    assert torch.equal(m.sub_mean.bias, torch.tensor([-1.0, -2.0, -3.0])) and not m.sub_mean.bias.requires_grad
    sd["head.0.weight"] = torch.zeros(16, 2, 3, 3)                           # (a size-1 axis would broadcast, there as here)
    with pytest.raises(RuntimeError, match="head.0.weight"):
        m.load_state_dict(sd)
    with pytest.raises(KeyError):
        m.load_state_dict({"nope": torch.zeros(1)}, strict=True)


@pytest.mark.parametrize("tag", FIXTURES)
def test_rcan_ref_matches_the_fixture_in_float64(tag):
    z = load_golden(tag)
    m = make(z)
    ng, nb, F, red, scale = (int(v) for v in z["cfg"])
    y, loss, dx, g = rcan_ref.run(m.state_dict(), torch.from_numpy(z["x"]), torch.from_numpy(z["t"]), ng, nb, scale)
    assert rel_l2(y, z["y64"]) < 1e-5 and abs(float(loss) - float(z["loss64"])) < 1e-5 * float(z["loss64"]) and rel_l2(dx, z["dx64"]) < 1e-5
    assert set(g) == {k for k in map(str, z["names"]) if k not in set(map(str, z["frozen"]))}
    for k, v in g.items():
        if "grad64/" + k in z:
            assert rel_l2(v, z["grad64/" + k]) < 1e-5, k
        else:
            assert rel_l2(sketch(v.numpy()), z["gsketch64/" + k]) < 1e-5 and rel_l2(v[0], z["gslice64/" + k]) < 1e-5, k
