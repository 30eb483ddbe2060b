"""CPU: the inference planner of the op-list networks (ResDeconv, ESPCN, SRCNN, EDSR: srcgan_resdeconv_infer_* / srcgan_srnet_infer_*)
-- exported and declared, rejects what the training planner rejects, its activation part does not grow with the depth, it is smaller
than the training workspace, the folded tail drops the 64-channel full-resolution tensor, and no op's output slot overlaps one of
its operands.  Pure host code: no compute call is made."""
import ctypes as C
import re
import subprocess

import pytest

from test_abi import header_symbols

NEW = ("srcgan_resdeconv_infer_ws_bytes", "srcgan_resdeconv_infer_act_bytes", "srcgan_resdeconv_infer_plan", "srcgan_resdeconv_infer",
       "srcgan_srnet_infer_ws_bytes", "srcgan_srnet_infer_act_bytes", "srcgan_srnet_infer_plan", "srcgan_srnet_infer",
       "srcgan_fold_tail_pack_bytes", "srcgan_fold_tail_pack")
DTYPES = pytest.mark.parametrize("dtype", [0, 1, 2], ids=["f32", "bf16", "fp16"])
LAYERS = ([1, 1, 1, 1], [2, 2, 2, 2], [3, 4, 6, 3])


@pytest.fixture(scope="module")
def lib():
    from srcgan_amd import build
    path = build.build(verbose=False)
    from srcgan_amd import _native as N
    return N.lib(), path


def _rd(layers=(2, 2, 2, 2), out_ch=3, B=2, H=32, W=48, dtype=0, norm=0):
    from srcgan_amd import _native as N
    return N.ResDeconvCfg(3, out_ch, B, H, W, dtype, (C.c_int * 4)(*layers), norm)


def _sr(kind=2, in_ch=3, out_ch=3, up=2, base=64, B=2, H=32, W=48, dtype=0, nres=4):
    from srcgan_amd import _native as N
    return N.SrNetCfg(kind, in_ch, out_ch, up, base, B, H, W, dtype, nres)


def test_new_symbols_are_declared_bound_and_exported(lib):
    from srcgan_amd import _native as N
    _, path = lib
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (srcgan_[a-z0-9_]+)", out))
    for s in NEW:
        assert s in header_symbols() and s in N.SIGNATURES and s in exported, s


@DTYPES
def test_edsr_activation_workspace_does_not_depend_on_depth(lib, dtype):
    l, _ = lib
    a = [l.srcgan_srnet_infer_act_bytes(C.byref(_sr(nres=n, dtype=dtype))) for n in (1, 4, 50)]
    assert a[0] > 0 and a[0] == a[1] == a[2], a
    # ... while the packed weights and the training workspace do grow
    w = [l.srcgan_srnet_infer_ws_bytes(C.byref(_sr(nres=n, dtype=dtype))) for n in (1, 4, 50)]
    t = [l.srcgan_srnet_ws_bytes(C.byref(_sr(nres=n, dtype=dtype))) for n in (1, 4, 50)]
    assert w[0] < w[1] < w[2] and t[0] < t[1] < t[2]


@DTYPES
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("norm", [0, 1], ids=["GN", "IN"])
def test_resdeconv_activation_workspace_does_not_depend_on_depth(lib, fold, norm, dtype):
    l, _ = lib
    a = [l.srcgan_resdeconv_infer_act_bytes(C.byref(_rd(layers=ly, dtype=dtype, norm=norm)), fold) for ly in LAYERS]
    assert a[0] > 0 and a[0] == a[1] == a[2], a
    w = [l.srcgan_resdeconv_infer_ws_bytes(C.byref(_rd(layers=ly, dtype=dtype, norm=norm)), fold) for ly in LAYERS]
    assert w[0] < w[1] < w[2]


@DTYPES
@pytest.mark.parametrize("layers", LAYERS, ids=["r10", "r18", "r34"])
def test_resdeconv_ordering(lib, layers, dtype):
    l, _ = lib
    c = _rd(layers=layers, dtype=dtype)
    train = l.srcgan_resdeconv_ws_bytes(C.byref(c))
    for fold in (0, 1):
        assert 0 < l.srcgan_resdeconv_infer_act_bytes(C.byref(c), fold) < l.srcgan_resdeconv_infer_ws_bytes(C.byref(c), fold) < train
    a0, a1 = (l.srcgan_resdeconv_infer_act_bytes(C.byref(c), f) for f in (0, 1))
    # the fold removes exactly the tensor between deconv13 and pred: B x H x W x 64 elements (2 x 32 x 48 here)
    esz = 4 if dtype == 0 else 2
    assert a1 < a0 and a0 - a1 == 2 * 32 * 48 * 64 * esz


@DTYPES
def test_edsr_ordering(lib, dtype):
    l, _ = lib
    c = _sr(nres=50, dtype=dtype)
    assert 0 < l.srcgan_srnet_infer_ws_bytes(C.byref(c)) < l.srcgan_srnet_ws_bytes(C.byref(c))
    # the cases of the GPU memory tests: the EDSR inference workspace is under a third of the training one
    c = _sr(nres=50, dtype=1, B=2, H=64, W=64)
    assert l.srcgan_srnet_infer_ws_bytes(C.byref(c)) < l.srcgan_srnet_ws_bytes(C.byref(c)) / 3


def test_bad_configurations_return_zero_and_say_why(lib):
    l, _ = lib
    for c in (_rd(H=40), _rd(norm=2), _rd(B=0), _rd(dtype=7), _rd(layers=[2, 2, 0, 2]), _rd(out_ch=9)):
        assert l.srcgan_resdeconv_ws_bytes(C.byref(c)) == 0
        want = l.srcgan_last_error()
        assert want
        for fold in (0, 1):
            for fn in (l.srcgan_resdeconv_infer_ws_bytes, l.srcgan_resdeconv_infer_act_bytes):
                assert fn(C.byref(c), fold) == 0 and l.srcgan_last_error() == want
            assert l.srcgan_resdeconv_infer_plan(C.byref(c), fold, None, 0) == -1
    ok = _rd()
    assert l.srcgan_resdeconv_infer_ws_bytes(C.byref(ok), 2) == 0 and b"fold_tail" in l.srcgan_last_error()
    for c in (_sr(kind=3), _sr(base=60), _sr(up=3), _sr(nres=0), _sr(in_ch=9), _sr(B=0), _sr(kind=0, up=9)):
        assert l.srcgan_srnet_ws_bytes(C.byref(c)) == 0
        want = l.srcgan_last_error()
        assert want
        for fn in (l.srcgan_srnet_infer_ws_bytes, l.srcgan_srnet_infer_act_bytes):
            assert fn(C.byref(c)) == 0 and l.srcgan_last_error() == want
        assert l.srcgan_srnet_infer_plan(C.byref(c), None, 0) == -1
    assert l.srcgan_srnet_infer_ws_bytes(C.byref(_sr())) > 0


def _ranges(l, kind, c, fold=0):
    """[(in_off, in_bytes, res_off, res_bytes, out_off, out_bytes)] per op, and the activation bytes of the plan."""
    if kind == "rd":
        n = l.srcgan_resdeconv_infer_plan(C.byref(c), fold, None, 0)
        buf = (C.c_size_t * (6 * n))()
        assert n > 0 and l.srcgan_resdeconv_infer_plan(C.byref(c), fold, buf, n) == n
        act = l.srcgan_resdeconv_infer_act_bytes(C.byref(c), fold)
    else:
        n = l.srcgan_srnet_infer_plan(C.byref(c), None, 0)
        buf = (C.c_size_t * (6 * n))()
        assert n > 0 and l.srcgan_srnet_infer_plan(C.byref(c), buf, n) == n
        act = l.srcgan_srnet_infer_act_bytes(C.byref(c))
    return [tuple(buf[6 * k:6 * k + 6]) for k in range(n)], act


def _plans(dtype):
    for ly in LAYERS:
        for norm in (0, 1):
            for fold in (0, 1):
                yield f"resdeconv{ly}/norm{norm}/fold{fold}", "rd", _rd(layers=ly, dtype=dtype, norm=norm), fold
    yield "resdeconv 16x16", "rd", _rd(B=1, H=16, W=16, out_ch=2, dtype=dtype), 1
    for n in (1, 4, 50):
        for up in (1, 2, 4):
            yield f"edsr{n}x{up}", "sr", _sr(nres=n, up=up, dtype=dtype), 0
    yield "espcn", "sr", _sr(kind=0, in_ch=1, out_ch=1, up=2, dtype=dtype), 0
    yield "espcn x3", "sr", _sr(kind=0, up=3, H=19, W=35, dtype=dtype), 0
    yield "srcnn", "sr", _sr(kind=1, up=1, H=19, W=35, dtype=dtype), 0


@DTYPES
def test_no_output_aliases_an_operand_and_every_tensor_is_inside_the_activation_part(lib, dtype):
    l, _ = lib

    def apart(a, an, b, bn):
        return bn == 0 or a + an <= b or b + bn <= a

    for name, kind, c, fold in _plans(dtype):
        ops, act = _ranges(l, kind, c, fold)
        for k, (i, ib, r, rb, o, ob) in enumerate(ops):
            assert ib > 0 and ob > 0 and i % 256 == 0 and o % 256 == 0, (name, k)
            assert apart(o, ob, i, ib) and apart(o, ob, r, rb), (name, k)
            assert i + ib <= act and r + rb <= act and o + ob <= act, (name, k)
        # a tensor that is read later is not overwritten in between: the output of op k is still where op j > k reads it, i.e. no op
        # between them writes into that range.  Consumers are identified by range; a range that is rewritten ends the search.
        for k, (_, _, _, _, o, ob) in enumerate(ops):
            readers = [j for j in range(k + 1, len(ops)) if (ops[j][0], ops[j][1]) == (o, ob) or (ops[j][2], ops[j][3]) == (o, ob)]
            if not readers:
                continue
            first = readers[0]                    # the producer's first consumer: nothing may write the slot before it
            for j in range(k + 1, first):
                assert apart(ops[j][4], ops[j][5], o, ob), (name, k, j)


def test_folded_plan_has_no_full_resolution_64_channel_tensor(lib):
    l, _ = lib
    c = _rd(dtype=1)
    full64 = 2 * 32 * 48 * 64 * 2
    plain, _ = _ranges(l, "rd", c, 0)
    fold, _ = _ranges(l, "rd", c, 1)
    assert len(fold) == len(plain) - 1
    assert any(op[5] == full64 for op in plain)
    assert all(op[1] < full64 and op[5] < full64 for op in fold)

