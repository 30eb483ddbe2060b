"""CPU: DDBPN through the C ABI's host code and the Python class -- parameter count and order, refused configurations, the inference
planner's ranges, the seeded weights, what infer.py knows about the network (scale, a sufficient receptive radius), and the
stride-1 forms of the projections against F.conv2d / F.conv_transpose2d.  Also pins tests/ddbpn_ref.py (our float64 restatement) to
the three reference fixtures, so the GPU tests never need the reference."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddbpn_ref
from conftest import load_golden, rel_l2
from ddbpn_ref import sketch

FIXTURES = ("ddbpn_x2", "ddbpn_x4", "ddbpn_x8")


@pytest.fixture(scope="module")
def lib():
    from srcgan_amd import _native as N
    return N.lib()


def make(z, **kw):
    import srcgan_amd
    torch.manual_seed(int(z["seed"]))
    return srcgan_amd.DDBPN(scale=int(z["scale"]), rgb_range=1, **kw)


def cfg_of(N, scale=2, colors=3, B=2, H=7, W=5, dtype=None):
    return N.DdbpnCfg(colors, colors, B, H, W, N.F32 if dtype is None else dtype, scale)


@pytest.mark.parametrize("tag", FIXTURES)
def test_parameter_count_names_order_and_seeded_weights(lib, tag):
    from srcgan_amd import _native as N
    z = load_golden(tag)
    m = make(z)
    names = [str(n) for n in z["names"]]
    assert list(m.state_dict().keys()) == names and len(names) == 135
    assert [k for k, _ in m.named_parameters()] == [str(n) for n in z["params"]] == names      # parameters() order = what the planner indexes
    assert lib.srcgan_ddbpn_num_params(C.byref(cfg_of(N, scale=int(z["scale"])))) == len(names)
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad]
    assert frozen == [str(n) for n in z["frozen"]] == list(ddbpn_ref.FROZEN)
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(z["wshape/" + k]), k
        assert np.array_equal(sketch(v.numpy()), z["wsketch/" + k]), k


@pytest.mark.parametrize("kw, word", [(dict(colors=1), b"n_colors"), (dict(scale=3), b"scale"), (dict(scale=16), b"scale")])
def test_refused_configurations_name_the_entry_point(lib, kw, word):
    from srcgan_amd import _native as N
    cfg = cfg_of(N, **kw)
    for fn, bad in ((lib.srcgan_ddbpn_num_params, -1), (lib.srcgan_ddbpn_ws_bytes, 0), (lib.srcgan_ddbpn_bwd_scratch_bytes, 0),
                    (lib.srcgan_ddbpn_infer_ws_bytes, 0), (lib.srcgan_ddbpn_infer_act_bytes, 0)):
        assert fn(C.byref(cfg)) == bad
        err = lib.srcgan_last_error()
        assert b"srcgan_ddbpn" in err and word in err, err


def test_constructor_refuses_what_the_planner_refuses_and_takes_args():
    import types
    import srcgan_amd
    for kw in (dict(n_colors=1), dict(scale=3)):
        with pytest.raises(ValueError, match="srcgan_ddbpn"):
            srcgan_amd.DDBPN(**kw)
    m = srcgan_amd.DDBPN(types.SimpleNamespace(scale=[4, 2], rgb_range=1, n_colors=3))
    assert m.scale == 4 and m.depth == 6
    assert torch.equal(m.sub_mean.bias, -torch.tensor([0.4488, 0.4371, 0.4040])) and torch.equal(m.add_mean.bias, torch.tensor([0.4488, 0.4371, 0.4040]))
    assert isinstance(m.initial[1], torch.nn.PReLU) and m.upmodules[1].bottleneck is None and m.upmodules[2].bottleneck is not None
    assert m.downmodules[0].bottleneck is None and isinstance(m.upmodules[0].conv_1[0], torch.nn.ConvTranspose2d)
    assert isinstance(m.downmodules[0].conv_1[0], torch.nn.Conv2d) and m.upmodules[0].conv_1[0].kernel_size == (8, 8)


def test_symbols_are_declared_bound_and_exported(lib):
    import os
    import srcgan_amd
    from srcgan_amd import _native as N, build, model
    header = open(os.path.join(os.path.dirname(srcgan_amd.__file__), "..", "include", "srcgan_amd.h")).read()
    want = ["srcgan_s2d_shift", "srcgan_d2s_shift", "srcgan_prelu_forward", "srcgan_prelu_backward", "srcgan_prelu_scratch_floats"]
    want += ["srcgan_ddbpn_" + s for s in ("num_params", "ws_bytes", "bwd_scratch_bytes", "forward", "backward", "infer_ws_bytes", "infer_act_bytes",
                                           "infer_plan", "infer")]
    for name in want:
        assert name in N.SIGNATURES and re.search(r"\b%s\(" % name, header) and getattr(lib, name) is not None, name
    assert "back_proj.hip" in build.SOURCES
    assert "DDBPN" in srcgan_amd.__all__ and "DDBPN" in model.__all__ and srcgan_amd.DDBPN is model.DDBPN


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_stride_1_forms_reproduce_the_projections_in_float64(scale):
    k, s, p = ddbpn_ref.PROJ[scale]
    g = torch.Generator().manual_seed(scale)
    h, w, ci, co = 5, 3, 3, 5                       # odd sizes, unequal channel counts
    x_hr = torch.randn(2, ci, s * h, s * w, generator=g, dtype=torch.float64)
    x_lr = torch.randn(2, ci, h, w, generator=g, dtype=torch.float64)
    wd = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64)
    wu = torch.randn(ci, co, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(co, generator=g, dtype=torch.float64)
    down, up = F.conv2d(x_hr, wd, b, stride=s, padding=p), F.conv_transpose2d(x_lr, wu, b, stride=s, padding=p)
    assert (ddbpn_ref.down_s1(x_hr, wd, b, scale) - down).abs().max() < 1e-12
    assert (ddbpn_ref.up_s1(x_lr, wu, b, scale) - up).abs().max() < 1e-12
    # gather and crop are each other's adjoint, and the crop undoes the gather
    T, shift, Hg, Wg, _, _ = ddbpn_ref.geometry(scale, h, w)
    gx = ddbpn_ref.s2d_shift(x_hr, s, shift, Hg, Wg)
    gr = torch.randn(gx.shape, generator=g, dtype=torch.float64)
    assert torch.equal(ddbpn_ref.d2s_shift(gx, ci, s, shift, s * h, s * w), x_hr)
    assert abs(float((gx * gr).sum() - (x_hr * ddbpn_ref.d2s_shift(gr, ci, s, shift, s * h, s * w)).sum())) < 1e-9


def test_prelu_backward_formula_is_autograd_s():
    g = torch.Generator().manual_seed(1)
    z = torch.randn(2, 5, 4, 3, generator=g, dtype=torch.float64)
    z[0, :, 1, 1] = 0.0
    a = torch.tensor([0.0, -0.2, 1.25, 0.25, 1.0], dtype=torch.float64, requires_grad=True)
    bias = torch.randn(5, generator=g, dtype=torch.float64).requires_grad_(True)
    zz = z.clone().requires_grad_(True)
    dy = torch.randn(z.shape, generator=g, dtype=torch.float64)
    F.prelu(zz + bias.view(1, -1, 1, 1), a).backward(dy)
    dz, da, db = ddbpn_ref.prelu_backward(dy, z, a.detach(), bias.detach())
    assert torch.allclose(dz, zz.grad, atol=1e-14) and torch.allclose(da, a.grad, atol=1e-12) and torch.allclose(db, bias.grad, atol=1e-12)
    assert torch.equal(ddbpn_ref.prelu_forward(z, a.detach(), bias=bias.detach()), F.prelu(z + bias.detach().view(1, -1, 1, 1), a.detach()))


@pytest.mark.parametrize("tag", FIXTURES)
def test_ddbpn_ref_matches_the_fixture_in_float64(tag):
    z = load_golden(tag)
    m = make(z)
    assert ddbpn_ref.set_slopes(m, int(z["seed"])) == 43
    x, t, scale = torch.from_numpy(z["x"]), torch.from_numpy(z["t"]), int(z["scale"])
    for s1 in (False, True):
        y, loss, dx, g = ddbpn_ref.run(m.state_dict(), x, t, scale, s1=s1)
        assert rel_l2(y, z["y64"]) < 1e-5 and abs(float(loss) - float(z["loss64"])) < 1e-5 * float(z["loss64"]) and rel_l2(dx, z["dx64"]) < 1e-5
        assert set(g) == {k for k in map(str, z["names"]) if k not in set(map(str, z["frozen"]))}
        for k, v in g.items():
            if "grad64/" + k in z:
                assert rel_l2(v, z["grad64/" + k]) < 1e-5, k
            else:
                first = v[0] if v[0].numel() <= 256 else v[0, 0]
                assert rel_l2(sketch(v.numpy()), z["gsketch64/" + k]) < 1e-5 and rel_l2(first, z["gslice64/" + k]) < 1e-5, k


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_infer_plan_is_inside_the_activation_part_and_live_ranges_are_disjoint(lib, scale):
    from srcgan_amd import _native as N
    cfg = cfg_of(N, scale=scale, dtype=N.BF16)
    n = lib.srcgan_ddbpn_infer_plan(C.byref(cfg), None, 0)
    # sub_mean, initial (4), per module 3 projections of 2 (up) or 3 (down) ops -- up-module: 2 + 3 + 2, down-module: 3 + 2 + 3 -- and
    # 2 per bottleneck, reconstruction, add_mean
    assert n == 1 + 4 + 6 * 7 + 5 * 8 + 8 * 2 + 2
    r = (C.c_size_t * (6 * n))()
    assert lib.srcgan_ddbpn_infer_plan(C.byref(cfg), r, n) == n
    act = lib.srcgan_ddbpn_infer_act_bytes(C.byref(cfg))
    assert 0 < act < lib.srcgan_ddbpn_infer_ws_bytes(C.byref(cfg))
    ops = [tuple(r[6 * k:6 * k + 6]) for k in range(n)]
    overlap = lambda a, b: a[1] and b[1] and a[0] < b[0] + b[1] and b[0] < a[0] + a[1]
    for k, (io, ib, ro, rb, oo, ob) in enumerate(ops):
        assert ob > 0 and oo + ob <= act and io + ib <= act and ro + rb <= act       # whichever slot a tensor got, it lies inside `act`
        assert not overlap((oo, ob), (io, ib)) and not overlap((oo, ob), (ro, rb)), k
    # a tensor (= a range written by some op, or the input) that is read after op k and was last written before it is alive across k:
    # op k's output may not touch it, unless it IS that tensor (a slice of a concatenation buffer written in place)
    for k, (_, _, _, _, oo, ob) in enumerate(ops):
        for j in range(k + 1, n):
            for q in ((ops[j][0], ops[j][1]), (ops[j][2], ops[j][3])):
                if not q[1] or q == (oo, ob) or not overlap((oo, ob), q):
                    continue
                rewritten = any((ops[i][4], ops[i][5]) == q for i in range(k + 1, j))
                assert rewritten, (k, j, q)
    # the activation part is a function of the shapes alone: same for both 16-bit types, and below the training workspace
    assert act == lib.srcgan_ddbpn_infer_act_bytes(C.byref(cfg_of(N, scale=scale, dtype=N.F16)))
    assert act < lib.srcgan_ddbpn_ws_bytes(C.byref(cfg))


def test_infer_knows_the_scale_and_a_radius():
    import srcgan_amd
    from srcgan_amd import infer
    for scale in (2, 4, 8):
        m = srcgan_amd.DDBPN(scale=scale)
        assert infer._scale(m) == scale
        assert infer.receptive_halo(m) == infer._ddbpn_halo(scale) > 0


@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("axis", [2, 3])
def test_receptive_halo_is_sufficient_on_the_restatement(scale, axis):
    """A perturbation of every input pixel farther than the radius from pixel c leaves the s output rows (columns) of c bit-identical."""
    from srcgan_amd import infer
    import srcgan_amd
    r = infer._ddbpn_halo(scale)
    torch.manual_seed(11)
    m = srcgan_amd.DDBPN(scale=scale, rgb_range=1)
    ddbpn_ref.set_slopes(m, 11)
    sd = {k: v.double() for k, v in m.state_dict().items()}
    n, c = 2 * r + 5, r + 2
    shape = [1, 3, 3, 3]
    shape[axis] = n
    g = torch.Generator().manual_seed(12)
    x = torch.rand(*shape, generator=g, dtype=torch.float64)
    x2 = x.clone()
    far = [i for i in range(n) if abs(i - c) > r]
    assert far[0] == 0 and far[-1] == n - 1 and len(far) == 4
    x2.index_copy_(axis, torch.tensor(far), torch.rand(*[len(far) if d == axis else shape[d] for d in range(4)], generator=g, dtype=torch.float64))
    with torch.no_grad():
        y, y2 = ddbpn_ref.forward(sd, x, scale), ddbpn_ref.forward(sd, x2, scale)
    rows = torch.arange(scale * c, scale * (c + 1))
    assert torch.equal(y.index_select(axis, rows), y2.index_select(axis, rows))
    assert not torch.equal(y, y2)
