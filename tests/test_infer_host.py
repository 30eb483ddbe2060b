"""CPU: the inference planner of the RRDB generators (srcgan_rddbnet_infer_ws_bytes) -- exported and declared, rejects what the
training planner rejects, does not grow with the trunk depth, and stays under a cap computed from the tensor shapes.  Pure host
code: no compute call is made."""
import ctypes as C
import re
import subprocess

import pytest

from test_abi import header_symbols

MIB = 1 << 20
NEW = ("srcgan_rddbnet_infer_ws_bytes", "srcgan_rddbnet_infer")


@pytest.fixture(scope="module")
def lib():
    from srcgan_amd import build
    path = build.build(verbose=False)
    from srcgan_amd import _native as N
    return N.lib(), path


def _cfg(in_ch=3, out_ch=3, up=1, nf=64, nb=3, gc=32, B=2, H=48, W=40, dtype=0, down=0, legacy=0):
    from srcgan_amd import _native as N
    return N.RddbCfg(in_ch, out_ch, up, nf, nb, gc, B, H, W, dtype, down, legacy)


def _act(l, c):
    """The activation part of the inference workspace."""
    return l.srcgan_rddbnet_infer_ws_bytes(C.byref(c)) - l.srcgan_rddbnet_wpack_bytes(C.byref(c))


# name -> cfg keywords: every family the planner serves
FAMILIES = {
    "rddbnet_x1": dict(up=1), "rddbnet_x2": dict(up=2), "rddbnet_x4": dict(up=4), "rddbnet_x8": dict(up=8),
    "rddbneta_d2": dict(up=1, down=2), "rddbneta_d4": dict(up=1, down=4),
    "srdn": dict(up=1, legacy=3),
    "rddbnetb_x2": dict(up=2, legacy=1), "rddbnetb_x4": dict(up=4, legacy=1),
}


def test_new_symbols_are_declared_bound_and_exported(lib):
    from srcgan_amd import _native as N
    _, path = lib
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (srcgan_[a-z0-9_]+)", out))
    for s in NEW:
        assert s in header_symbols() and s in N.SIGNATURES and s in exported, s


def test_infer_planner_rejects_what_the_training_planner_rejects(lib):
    l, _ = lib
    bad = [_cfg(nf=60), _cfg(gc=12), _cfg(up=3), _cfg(up=2, down=2), _cfg(nb=0), _cfg(B=0), _cfg(in_ch=9), _cfg(dtype=7),
           _cfg(legacy=4), _cfg(legacy=1, up=1), _cfg(legacy=3, up=2), _cfg(down=4, H=50), _cfg(legacy=2, up=8)]
    for c in bad:
        assert l.srcgan_rddbnet_ws_bytes(C.byref(c)) == 0
        want = l.srcgan_last_error()
        assert want
        assert l.srcgan_rddbnet_infer_ws_bytes(C.byref(c)) == 0
        assert l.srcgan_last_error() == want
    ok = _cfg(up=2)
    assert l.srcgan_rddbnet_infer_ws_bytes(C.byref(ok)) > 0


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_activation_workspace_does_not_depend_on_depth(lib, name, dtype):
    l, _ = lib
    a = [_act(l, _cfg(nb=nb, dtype=dtype, **FAMILIES[name])) for nb in (1, 23, 64)]
    assert a[0] > 0 and a[0] == a[1] == a[2], a
    # ... while the training workspace does grow
    t = [l.srcgan_rddbnet_ws_bytes(C.byref(_cfg(nb=nb, dtype=dtype, **FAMILIES[name]))) for nb in (1, 23)]
    assert t[1] > t[0]


def _cap(c):
    """Upper bound from shapes alone: 4 dense buffers' worth of trunk pixels, 4 nf-channel trunk tensors, the input and output
    images at 8 padded channels, every materialised tensor at another resolution once, and 1 MiB for alignment."""
    e = 4 if c.dtype == 0 else 2
    ndn = max(c.down, 1).bit_length() - 1
    Ht, Wt = c.H >> ndn, c.W >> ndn
    P = c.B * Ht * Wt
    f = c.up if c.down == 0 else 1
    HO, WO = Ht * f, Wt * f
    cap = 4 * (c.nf + 4 * c.gc) * e * P + 4 * c.nf * e * P
    cap += 8 * e * c.B * c.H * c.W + 8 * e * c.B * HO * WO
    stages = []                                   # pixel counts of the nf-channel tensors that are not at the trunk's resolution
    if c.legacy in (1, 2):
        h, w = Ht, Wt
        if c.legacy == 1:
            ops = [0, 1, 0, 1] if c.up == 4 else [0, 1, 1]
            ops += [1] * 8
        else:
            ops = [0, 1] * (c.up.bit_length() - 1) + ([1] if c.up == 1 else []) + [1, 1]
        for conv in ops:
            if not conv:
                h, w = 2 * h, 2 * w
            stages.append(c.B * h * w)
    elif c.legacy == 0:
        stages += [P << (2 * s) for s in range(1, f.bit_length())]          # up-sampler stage outputs
        stages += [c.B * (c.H >> s) * (c.W >> s) for s in range(ndn)]       # conv_first at HR and the down stages above the trunk
    return cap + sum(c.nf * e * s for s in stages) + MIB


@pytest.mark.parametrize("dtype", [0, 1, 2], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(FAMILIES) + ["legacy_x1", "legacy_x4", "narrow_x4", "odd_x2"])
def test_activation_workspace_is_under_the_shape_cap(lib, name, dtype):
    l, _ = lib
    extra = {"legacy_x1": dict(up=1, legacy=2), "legacy_x4": dict(up=4, legacy=2), "narrow_x4": dict(up=4, nf=16, gc=8),
             "odd_x2": dict(up=2, H=19, W=35, B=3)}
    kw = {**FAMILIES, **extra}[name]
    for nb in (1, 23):
        c = _cfg(nb=nb, dtype=dtype, **kw)
        a = _act(l, c)
        assert 0 < a <= _cap(c), (a, _cap(c))


def test_bench_configuration(lib, capsys):
    """bf16, B = 16, 256x256 -> x4, nb = 23: the training workspace is 32.4 GB; the inference workspace must be under a fifth."""
    l, _ = lib
    c = _cfg(up=4, nb=23, B=16, H=256, W=256, dtype=1)
    train, infer = l.srcgan_rddbnet_ws_bytes(C.byref(c)), l.srcgan_rddbnet_infer_ws_bytes(C.byref(c))
    with capsys.disabled():
        print(f"\nbench cfg: training workspace {train / 1e9:.2f} GB, inference workspace {infer / 1e9:.2f} GB "
              f"(activations {_act(l, c) / 1e9:.2f} GB, cap {_cap(c) / 1e9:.2f} GB)")
    assert 0 < infer < train / 5
    assert _act(l, c) <= _cap(c)
    # one 3 x 2048 x 2048 -> 8192 x 8192 scene has 4 x the pixels
    s = _cfg(up=4, nb=23, B=1, H=2048, W=2048, dtype=1)
    assert l.srcgan_rddbnet_infer_ws_bytes(C.byref(s)) < l.srcgan_rddbnet_ws_bytes(C.byref(s)) / 5


# ---- parameter layout questions the native planner answers (srcgan_rddbnet_num_rrdb / srcgan_rddbnet_phase_params)
LAYOUT = {**{k: FAMILIES[k] for k in ("rddbnet_x1", "rddbnet_x4", "rddbneta_d2", "rddbneta_d4", "srdn", "rddbnetb_x2", "rddbnetb_x4")},
          "legacy_x1": dict(up=1, legacy=2), "legacy_x4": dict(up=4, legacy=2)}


def _phase(l, c, lo, hi):
    first, end = C.c_int(-1), C.c_int(-1)
    rc = l.srcgan_rddbnet_phase_params(C.byref(c), lo, hi, C.byref(first), C.byref(end))
    return rc, first.value, end.value


def test_layout_symbols_are_declared_bound_and_exported(lib):
    from srcgan_amd import _native as N
    _, path = lib
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (srcgan_[a-z0-9_]+)", out))
    for s in ("srcgan_rddbnet_num_rrdb", "srcgan_rddbnet_phase_params"):
        assert s in header_symbols() and s in N.SIGNATURES and s in exported, s


@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("name", sorted(LAYOUT))
def test_phase_ranges_tile_the_parameters(lib, name, nb):
    l, _ = lib
    kw = LAYOUT[name]
    c = _cfg(nb=nb, **kw)
    n, nrr = l.srcgan_rddbnet_num_params(C.byref(c)), l.srcgan_rddbnet_num_rrdb(C.byref(c))
    assert n > 0 and nrr == {0: nb, 1: nb, 2: 0, 3: 2 * nb}[kw.get("legacy", 0)]
    assert _phase(l, c, 0, nrr) == (0, 0, n)                    # one phase (also the network without a trunk): everything
    # every gap-free descending cut list: its ranges tile [0, n) exactly once, last phase first
    for mask in range(1 << max(nrr - 1, 0)):
        cuts = [0] + [k for k in range(1, nrr) if mask >> (k - 1) & 1]
        hi, want_end = nrr, n
        for lo in sorted(cuts, reverse=True):
            rc, first, end = _phase(l, c, lo, hi)
            assert rc == 0 and 0 <= first < end == want_end, (cuts, lo, hi, first, end)
            hi, want_end = lo, first
        assert want_end == 0, cuts


@pytest.mark.parametrize("down", [0, 2, 4])
def test_phase_ranges_of_the_plain_order(lib, down):
    """conv_first (2), the down stages (2 each), 30 parameters per RRDB, then trunk_conv / up-sampler / conv_last."""
    l, _ = lib
    nb = 5
    c = _cfg(nb=nb, up=1 if down else 2, down=down)
    n = l.srcgan_rddbnet_num_params(C.byref(c))
    p_rdb0 = 2 + 2 * (down.bit_length() - 1 if down else 0)
    assert l.srcgan_rddbnet_num_rrdb(C.byref(c)) == nb
    for lo in range(nb + 1):
        for hi in range(lo, nb + 1):
            want = (0, 0 if lo == 0 else p_rdb0 + 30 * lo, n if hi == nb else p_rdb0 + 30 * hi)
            assert _phase(l, c, lo, hi) == want, (lo, hi)


def test_layout_functions_reject_bad_input(lib):
    l, _ = lib
    for c in (_cfg(nf=60), _cfg(legacy=4), _cfg(up=2, down=2)):
        assert l.srcgan_rddbnet_ws_bytes(C.byref(c)) == 0
        want = l.srcgan_last_error()
        assert want
        assert l.srcgan_rddbnet_num_rrdb(C.byref(c)) == -1 and l.srcgan_last_error() == want
        assert _phase(l, c, 0, 1)[0] != 0 and l.srcgan_last_error() == want
    ok = _cfg(nb=3, up=2)
    for lo, hi in ((-1, 2), (2, 1), (0, 4), (4, 4)):
        assert _phase(l, ok, lo, hi) == (1, -1, -1), (lo, hi)
        assert b"outside [0,3)" in l.srcgan_last_error()
    legacy = _cfg(up=2, legacy=2)                               # no trunk: [0, 0) is the only range
    assert _phase(l, legacy, 0, 1)[0] != 0 and l.srcgan_last_error()
    assert l.srcgan_rddbnet_phase_params(C.byref(ok), 0, 3, None, None) != 0 and l.srcgan_last_error()
