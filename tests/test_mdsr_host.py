"""CPU: MDSR and VDSR through the C ABI's host code and the Python classes -- exports, parameter count and order, the seeded weights
(creation order against registration order), both constructor forms, ``url``, refused configurations, no CPU fallback, what infer.py
knows about the networks, the inference planner's answers (slots that do not grow with the depth, outputs that never alias their
operands, ranges inside the activation part) and the price of a branch off the graph: nothing."""
import ctypes as C
import re
import types

import numpy as np
import pytest
import torch

import mdsr_ref
from conftest import load_golden
from mdsr_ref import sketch
from test_mdsr_ref import FIXTURES, native

STEMS = ("mdsr", "vdsr")
ENTRIES = ("num_params", "ws_bytes", "bwd_scratch_bytes", "forward", "backward", "infer_ws_bytes", "infer_act_bytes", "infer_plan", "infer")


@pytest.fixture(scope="module")
def lib():
    from srcgan_amd import _native as N
    return N.lib()


def mcfg(N, scales=(2, 3, 4), idx=0, n=2, F=32, B=2, H=8, W=6, dtype=None, colors=(3, 3), nscale=None):
    return N.MdsrCfg(colors[0], colors[1], B, H, W, N.F32 if dtype is None else dtype, n, F, len(scales) if nscale is None else nscale,
                     (C.c_int * 4)(*scales), idx)


def vcfg(N, n=4, F=32, B=2, H=8, W=6, dtype=None, colors=3):
    return N.VdsrCfg(colors, B, H, W, N.F32 if dtype is None else dtype, n, F)


def test_symbols_are_declared_bound_and_exported(lib):
    import os
    import srcgan_amd
    from srcgan_amd import _native as N, model, train
    header = open(os.path.join(os.path.dirname(srcgan_amd.__file__), "..", "include", "srcgan_amd.h")).read()
    for stem in STEMS:
        for s in ENTRIES:
            name = f"srcgan_{stem}_{s}"
            assert name in N.SIGNATURES and re.search(r"\b%s\(" % name, header) and getattr(lib, name) is not None, name
        assert N.SIGNATURES[f"srcgan_{stem}_forward"][1][1:] == N.SIGNATURES["srcgan_rcan_forward"][1][1:]          # the signatures _OpListFn drives
        assert N.SIGNATURES[f"srcgan_{stem}_backward"][1][1:] == N.SIGNATURES["srcgan_rcan_backward"][1][1:]
    assert re.search(r"typedef struct srcgan_mdsr_cfg \{[^}]*int scales\[4\];[^}]*int scale_idx;", header)
    assert C.sizeof(N.MdsrCfg) == 14 * 4 and C.sizeof(N.VdsrCfg) == 7 * 4
    for name in ("MDSR", "VDSR"):
        assert name in srcgan_amd.__all__ and name in model.__all__ and getattr(srcgan_amd, name) is getattr(model, name)
        assert name not in train.MODEL_REGISTRY          # the CLI builds Model(in, out, up): an args network is not reachable from it


@pytest.mark.parametrize("tag", FIXTURES)
def test_parameter_count_names_order_and_seeded_weights(lib, tag):
    """The reference creates head, pre_process, body, upsample, tail (mdsr.py:25-45) and registers pre_process, upsample, head, body,
    tail (:27, 41, 47-49): the sketches are those of ITS seeded weights, so they hold the creation order, ``names`` the other one."""
    from srcgan_amd import _native as N
    z = load_golden(tag)
    m = native(z, tag)
    names = [str(n) for n in z["names"]]
    assert list(m.state_dict().keys()) == names and [k for k, _ in m.named_parameters()] == names
    assert [k for k, p in m.named_parameters() if not p.requires_grad] == [str(k) for k in z["frozen"]] == ["sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias"]
    if tag == "vdsr":
        assert len(names) == 12 == lib.srcgan_vdsr_num_params(C.byref(vcfg(N)))
    else:
        assert len(names) == 50 == lib.srcgan_mdsr_num_params(C.byref(mcfg(N, idx=int(z["cfg"][3]))))
    for k, v in m.state_dict().items():
        assert list(v.shape) == [int(s) for s in z["wshape/" + k]], k
        assert np.array_equal(sketch(v.numpy()), z["wsketch/" + k]), k          # bit for bit the reference's seeded weights


def test_parameter_counts(lib):
    from srcgan_amd import _native as N
    # the issue's count for scale = [2, 3, 4], n = 16: 4 + 3 * 8 + (2 + 2 + 4) + 2 + (4 * 16 + 2) + 2
    for idx in range(3):
        assert lib.srcgan_mdsr_num_params(C.byref(mcfg(N, n=16, F=64, idx=idx))) == 106 == len(mdsr_ref.mdsr_names(16, [2, 3, 4]))
    assert lib.srcgan_mdsr_num_params(C.byref(mcfg(N, scales=(8, 2), n=80, F=64))) == 4 + 16 + 8 + 2 + 322 + 2 == len(mdsr_ref.mdsr_names(80, [8, 2]))
    assert lib.srcgan_mdsr_num_params(C.byref(mcfg(N, scales=(3,), n=1))) == 4 + 8 + 2 + 2 + 6 + 2
    assert lib.srcgan_vdsr_num_params(C.byref(vcfg(N, n=20, F=64))) == 44 == len(mdsr_ref.vdsr_names(20))
    assert lib.srcgan_vdsr_num_params(C.byref(vcfg(N, n=2))) == 8


def test_both_constructor_forms_and_url():
    import srcgan_amd
    a = srcgan_amd.MDSR(types.SimpleNamespace(n_resblocks=16, n_feats=64, scale=[2, 3, 4], rgb_range=255, n_colors=3))
    assert a.url == "https://cv.snu.ac.kr/research/EDSR/models/mdsr_baseline-a00cab12.pt" and a.scale_idx == 0 and a.scale == [2, 3, 4]
    assert len(a.pre_process) == 3 == len(a.upsample) and len(a.body) == 17 and len(a.upsample[2]) == 4 and len(a.upsample[1]) == 2
    assert a.pre_process[1][0].body[0].kernel_size == (5, 5) and a.pre_process[1][0].body[0].padding == (2, 2) and a.body[0].body[2].kernel_size == (3, 3)
    assert a.upsample[1][0].out_channels == 9 * 64 and a.head[0].in_channels == 3 and a.tail[0].out_channels == 3
    assert list(a.state_dict().keys()) == mdsr_ref.mdsr_names(16, [2, 3, 4]) and len(list(a.parameters())) == 106
    assert torch.equal(a.sub_mean.bias, -255 * torch.tensor([0.4488, 0.4371, 0.4040])) and torch.equal(a.add_mean.weight.flatten(), torch.eye(3).flatten())
    a.set_scale(2)
    assert a.scale_idx == 2
    b = srcgan_amd.MDSR(n_resblocks=3, n_feats=48, scale=(4, 8), rgb_range=1, dtype="bf16")
    assert b.url is None and b.compute_dtype == "bf16" and len(b.upsample[1]) == 6           # a size the reference refuses with KeyError
    assert list(b.state_dict().keys()) == mdsr_ref.mdsr_names(3, [4, 8])
    assert srcgan_amd.MDSR(n_resblocks=80, scale=2).url.endswith("mdsr-4a78bedf.pt")
    assert srcgan_amd.MDSR().n_resblocks == 16 and srcgan_amd.MDSR().scale == [2, 3, 4]
    v = srcgan_amd.VDSR(types.SimpleNamespace(n_resblocks=20, n_feats=64, rgb_range=255, n_colors=3))
    assert v.url == "" and len(v.body) == 20 and len(v.body[0]) == 2 and len(v.body[19]) == 1 and v.body[19][0].out_channels == 3
    assert list(v.state_dict().keys()) == mdsr_ref.vdsr_names(20)
    assert srcgan_amd.VDSR(n_resblocks=4, n_feats=32).url is None and srcgan_amd.VDSR().n_resblocks == 20


MDSR_REFUSALS = [(dict(colors=(1, 3)), b"n_colors must be 3"), (dict(colors=(3, 1)), b"n_colors must be 3"), (dict(scales=(), nscale=0), b"nscale = 0 must be in 1..4"),
                 (dict(nscale=5), b"nscale = 5 must be in 1..4"), (dict(scales=(2, 5)), b"scales[1] = 5 must be 2, 3, 4 or 8"),
                 (dict(scales=(1,)), b"scales[0] = 1 must be 2, 3, 4 or 8"), (dict(idx=3), b"scale_idx = 3 must be in [0, nscale = 3)"),
                 (dict(idx=-1), b"scale_idx = -1 must be in"), (dict(F=40), b"n_feats = 40 must be a multiple of 16"), (dict(F=0), b"n_feats = 0 must be a multiple of 16"),
                 (dict(F=2048), b"at most 1024"), (dict(n=0), b"n_resblocks = 0 must be in 1..100000"), (dict(dtype=7), b"bad dtype"), (dict(H=0), b"bad B/H/W")]
VDSR_REFUSALS = [(dict(colors=1), b"n_colors must be 3"), (dict(n=1), b"n_resblocks = 1 must be in 2..100000"), (dict(F=24), b"n_feats = 24 must be a multiple of 16"),
                 (dict(F=1040), b"at most 1024"), (dict(dtype=-1), b"bad dtype"), (dict(B=0), b"bad B/H/W")]


@pytest.mark.parametrize("stem, kw, word", [("mdsr", k, w) for k, w in MDSR_REFUSALS] + [("vdsr", k, w) for k, w in VDSR_REFUSALS])
def test_refused_configurations_name_the_entry_point_and_the_limit(lib, stem, kw, word):
    from srcgan_amd import _native as N
    cfg = (mcfg if stem == "mdsr" else vcfg)(N, **kw)
    f = lambda s: getattr(lib, f"srcgan_{stem}_{s}")
    for s, bad in (("num_params", -1), ("ws_bytes", 0), ("bwd_scratch_bytes", 0), ("infer_ws_bytes", 0), ("infer_act_bytes", 0)):
        assert f(s)(C.byref(cfg)) == bad
        err = lib.srcgan_last_error()
        assert f"srcgan_{stem}".encode() in err and word in err, err
    assert f("infer_plan")(C.byref(cfg), None, 0) == -1
    # the drivers refuse before anything is touched: the pointers are never read
    assert f("forward")(C.byref(cfg), None, None, None, None, None) != 0 and word in lib.srcgan_last_error()
    assert f("backward")(C.byref(cfg), None, None, None, None, None, None, None) != 0 and word in lib.srcgan_last_error()
    assert f("infer")(C.byref(cfg), None, None, None, None, None) != 0 and word in lib.srcgan_last_error()


def test_constructor_refusals():
    import srcgan_amd
    for cls in (srcgan_amd.MDSR, srcgan_amd.VDSR):
        with pytest.raises(ValueError, match="n_colors = 1"):
            cls(n_colors=1)
        with pytest.raises(ValueError, match="n_feats = 40 must be a multiple of 16"):
            cls(n_feats=40)
    with pytest.raises(ValueError, match="srcgan_mdsr: scales\\[1\\] = 6"):
        srcgan_amd.MDSR(scale=[2, 6])
    with pytest.raises(ValueError, match="srcgan_mdsr: nscale = 5"):
        srcgan_amd.MDSR(scale=[2, 3, 4, 8, 2])
    with pytest.raises(ValueError, match="srcgan_vdsr: n_resblocks = 1"):
        srcgan_amd.VDSR(n_resblocks=1)


def test_no_cpu_fallback():
    import srcgan_amd
    for m in (srcgan_amd.MDSR(n_resblocks=1, n_feats=16), srcgan_amd.VDSR(n_resblocks=2, n_feats=16)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.rand(1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        srcgan_amd.MDSR(n_resblocks=1, n_feats=16).pre_process[0][0](torch.rand(1, 16, 8, 8))
    m = srcgan_amd.MDSR(n_resblocks=1, n_feats=16, scale=(2, 3))
    m.set_scale(2)
    with pytest.raises(IndexError, match="scale_idx = 2"):
        m(torch.rand(1, 3, 8, 8))


def test_infer_knows_the_scale_and_the_radius():
    import srcgan_amd
    from srcgan_amd import infer
    for n in (1, 2, 16):
        m = srcgan_amd.MDSR(n_resblocks=n, n_feats=16, scale=(2, 3, 4, 8))
        for idx, s in enumerate((2, 3, 4, 8)):
            m.set_scale(idx)
            assert infer._scale(m) == s and infer.receptive_halo(m) == 2 * n + 12
    assert infer.receptive_halo(srcgan_amd.MDSR()) == 44
    for n in (2, 5, 20):
        v = srcgan_amd.VDSR(n_resblocks=n, n_feats=16)
        assert infer._scale(v) == 1 and infer.receptive_halo(v) == n
    # both are whole networks of a chain's halo sum
    assert infer._chain_halo([srcgan_amd.MDSR(n_resblocks=1, n_feats=16, scale=2), srcgan_amd.VDSR(n_resblocks=4, n_feats=16)]) == 14 + 2


def _plan(lib, stem, cfg):
    n = getattr(lib, f"srcgan_{stem}_infer_plan")(C.byref(cfg), None, 0)
    r = (C.c_size_t * (6 * n))()
    assert getattr(lib, f"srcgan_{stem}_infer_plan")(C.byref(cfg), r, n) == n
    return [tuple(r[6 * k:6 * k + 6]) for k in range(n)]


@pytest.mark.parametrize("stem, kw, nops", [("mdsr", dict(idx=0), 15), ("mdsr", dict(idx=1), 15), ("mdsr", dict(idx=2), 17), ("mdsr", dict(scales=(8,), n=1), 17),
                                            ("vdsr", dict(), 6), ("vdsr", dict(n=2), 4)])
def test_infer_plan_outputs_never_alias_their_operands(lib, stem, kw, nops):
    from srcgan_amd import _native as N
    make = mcfg if stem == "mdsr" else vcfg
    cfg = make(N, dtype=N.BF16, **kw)
    ops = _plan(lib, stem, cfg)
    # MDSR: sub_mean, head, 4 + 2 n + 1 trunk convolutions, (conv, shuffle) per stage, tail, add_mean; VDSR: sub_mean, n convolutions, add_mean
    assert len(ops) == nops
    act = getattr(lib, f"srcgan_{stem}_infer_act_bytes")(C.byref(cfg))
    assert 0 < act < getattr(lib, f"srcgan_{stem}_infer_ws_bytes")(C.byref(cfg))
    overlap = lambda a, b: a[1] and b[1] and a[0] < b[0] + b[1] and b[0] < a[0] + a[1]
    for k, (io, ib, ro, rb, oo, ob) in enumerate(ops):
        assert ob > 0 and ib > 0 and oo + ob <= act and io + ib <= act and ro + rb <= act          # every range inside the activation part
        assert not overlap((oo, ob), (io, ib)) and not overlap((oo, ob), (ro, rb)), k
    # a range read after op k and last written before it is alive across k: op k's output may not touch it
    for k, (_, _, _, _, oo, ob) in enumerate(ops):
        for j in range(k + 1, len(ops)):
            for q in ((ops[j][0], ops[j][1]), (ops[j][2], ops[j][3])):
                if not q[1] or not overlap((oo, ob), q):
                    continue
                assert any((ops[i][4], ops[i][5]) == q for i in range(k, j)), (k, j, q)
    assert act == getattr(lib, f"srcgan_{stem}_infer_act_bytes")(C.byref(make(N, dtype=N.F16, **kw)))
    if stem == "vdsr":          # the sub_mean output is read by the first and by the last convolution
        assert (ops[-2][2], ops[-2][3]) == (ops[0][4], ops[0][5]) == (ops[1][0], ops[1][1])
    else:                       # the body's last convolution adds the pre_process output (op 5), not the head's (op 1)
        last_body = 6 + 2 * kw.get("n", 2)
        assert (ops[last_body][2], ops[last_body][3]) == (ops[5][4], ops[5][5]) != (ops[1][4], ops[1][5])


def test_inference_slots_do_not_grow_with_the_depth(lib):
    from srcgan_amd import _native as N
    act = lambda n, **kw: lib.srcgan_mdsr_infer_act_bytes(C.byref(mcfg(N, n=n, **kw)))
    for kw in (dict(idx=0), dict(idx=2, F=64, dtype=N.BF16, H=48, W=48)):
        assert act(2, **kw) == act(6, **kw) == act(80, **kw) > 0
    vact = lambda n, **kw: lib.srcgan_vdsr_infer_act_bytes(C.byref(vcfg(N, n=n, **kw)))
    assert vact(3) == vact(4) == vact(20) == vact(200) > 0
    big = mcfg(N, n=16, F=64, B=2, H=48, W=48, dtype=N.BF16)
    feat = 2 * 48 * 48 * 64 * 2
    # x2: the pre_process output and three rotating features, the 4 F tensor and its shuffle (4 feature sizes each), image-sized tensors and
    # scratch (under 4 more); the training plan keeps all 39 trunk features
    assert 12 * feat < lib.srcgan_mdsr_infer_act_bytes(C.byref(big)) < 16 * feat < 40 * feat < lib.srcgan_mdsr_ws_bytes(C.byref(big))


@pytest.mark.parametrize("dtype", ["F32", "BF16"])
def test_a_branch_off_the_graph_costs_nothing(lib, dtype):
    """every size of {scales = {2, 3, 4}, scale_idx = k} equals that of {scales = {scales[k]}, scale_idx = 0}"""
    from srcgan_amd import _native as N
    dt = getattr(N, dtype)
    sizes = lambda cfg: tuple(getattr(lib, "srcgan_mdsr_" + s)(C.byref(cfg)) for s in ("ws_bytes", "bwd_scratch_bytes", "infer_ws_bytes", "infer_act_bytes"))
    seen = set()
    for k, s in enumerate((2, 3, 4)):
        many, one = mcfg(N, idx=k, n=3, F=64, H=11, W=37, dtype=dt), mcfg(N, scales=(s,), idx=0, n=3, F=64, H=11, W=37, dtype=dt)
        assert sizes(many) == sizes(one) and all(v > 0 for v in sizes(many))
        assert _plan(lib, "mdsr", many) == _plan(lib, "mdsr", one)
        assert lib.srcgan_mdsr_num_params(C.byref(many)) == 4 + 24 + 8 + 2 + 14 + 2 > lib.srcgan_mdsr_num_params(C.byref(one))
        seen.add(sizes(many))
    assert len(seen) == 3           # and the three branches differ from each other
    # four scales against one: still the one branch's sizes
    assert sizes(mcfg(N, scales=(8, 4, 3, 2), idx=3, F=64, dtype=dt)) == sizes(mcfg(N, scales=(2,), F=64, dtype=dt))
