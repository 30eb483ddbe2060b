"""Host: the D4 view numbering of the geometric self-ensemble (tests/d4_ref.py, the restatement the GPU tests use) against numpy's
named transforms, with teeth; the ``ensemble=`` argument check of both scene drivers; and the argument checks of the two native
entry points, none of which launches anything."""
import ctypes as C

import numpy as np
import pytest
import torch

import d4_ref as R
from srcgan_amd import ESPCN, SRCNN, cascade_scene, upscale_scene

NAMED = {0: lambda m: m, 2: np.flipud, 4: np.fliplr, 6: lambda m: np.flip(m, (0, 1)), 1: np.transpose,
         3: lambda m: np.rot90(m, 1), 5: lambda m: np.rot90(m, 3), 7: lambda m: np.flip(np.transpose(m), (0, 1))}


def _asym(h, w):
    return np.random.default_rng(h * 100 + w).standard_normal((h, w)).astype(np.float32)


@pytest.mark.parametrize("op", range(8))
def test_each_op_is_the_named_transform(op):
    for h, w in [(5, 7), (4, 4), (1, 6)]:
        m = _asym(h, w)
        v = R.view(m, op)
        assert v.shape == R.view_shape(op, h, w) == NAMED[op](m).shape
        assert np.array_equal(v, NAMED[op](m)), op
        t = torch.from_numpy(m)
        assert np.array_equal(R.torch_view(t, op).numpy(), v), op
        assert np.array_equal(R.torch_fold(torch.from_numpy(v), op).numpy(), m), op
        batched = np.stack([m, 2 * m])[None]                                     # leading axes are carried along
        assert np.array_equal(R.view(batched, op)[0, 1], 2 * v)


def test_the_eight_views_are_distinct_and_the_sets_are_as_documented():
    m = _asym(6, 6)
    views = [R.view(m, op) for op in range(8)]
    for i in range(8):
        for j in range(i + 1, 8):
            assert not np.array_equal(views[i], views[j]), (i, j)
    assert R.OPS == {1: (0,), 2: (0, 4), 4: (0, 2, 4, 6), 8: (0, 1, 2, 3, 4, 5, 6, 7)}
    from srcgan_amd import infer
    assert infer.ENSEMBLE_OPS == R.OPS
    assert all(not op & 1 for op in R.OPS[4])                                    # flips only: no tile changes its shape


@pytest.mark.parametrize("op", range(8))
def test_fold_inverts_view_on_non_square_arrays(op):
    for h, w in [(5, 7), (33, 2)]:
        m = _asym(h, w)
        assert np.array_equal(R.fold(R.view(m, op), op, h, w), m)


def test_teeth_swapped_rotations_and_exchanged_extents():
    m = _asym(6, 6)                                                              # square: only the orientation can tell them apart
    assert not np.array_equal(R.fold(R.view(m, 3), 5, 6, 6), m)
    assert not np.array_equal(R.fold(R.view(m, 5), 3, 6, 6), m)
    assert not np.array_equal(R.torch_fold(R.torch_view(torch.from_numpy(m), 3), 5).numpy(), m)
    n = _asym(5, 7)
    for op in (1, 3, 5, 7):
        with pytest.raises(ValueError, match="does not fold"):
            R.fold(R.view(n, op), op, 7, 5)                                      # (ah, aw) exchanged
    # a transposed view taken for an untransposed one of the exchanged extents has the right shape and the wrong content
    assert R.view(n, 1).shape == (7, 5) and not np.array_equal(R.fold(R.view(n, 1), 0, 7, 5), n.reshape(7, 5))


def test_teeth_the_order_of_the_sum_is_part_of_the_result():
    big = np.float32(2.0 ** 24)
    vals = [big, 1.0, 1.0, -big]                                                 # 2^24 + 1 is no f32: in this order both ones are lost
    a = R.average([np.full((2, 2), v, np.float32) for v in vals])
    b = R.average([np.full((2, 2), v, np.float32) for v in (vals[1], vals[2], vals[0], vals[3])])
    assert float(a[0, 0]) == 0.0 and float(b[0, 0]) == 0.5
    t = [torch.full((2, 2), float(v)) for v in vals]
    assert np.array_equal(R.torch_average(t).numpy(), a)
    x = np.random.default_rng(3).standard_normal((8, 3, 3)).astype(np.float32) * np.float32(1e3)
    assert not np.array_equal(R.average(list(x)), R.average(list(x[::-1])))      # and on ordinary data bits move too
    assert np.array_equal(R.average(list(x)), ((((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]) + x[6] + x[7]) * np.float32(0.125))


@pytest.mark.parametrize("bad", [0, 3, 5, 6, 16, -1, True, "8", None])
def test_ensemble_values_are_checked_before_the_device(bad):
    """CPU tensors: the ValueError comes first, the no-CPU-fallback RuntimeError only for an allowed value."""
    net = ESPCN(1, 1, 2)
    with pytest.raises(ValueError, match="ensemble must be 1, 2, 4 or 8"):
        upscale_scene(net, torch.zeros(1, 1, 20, 20), up=2, tile=16, ensemble=bad)
    with pytest.raises(ValueError, match="ensemble must be 1, 2, 4 or 8"):
        cascade_scene(net, SRCNN(1, 3, 1, 16), torch.zeros(20, 20, dtype=torch.uint8), up=2, tile=16, ensemble=bad)


@pytest.mark.parametrize("good", [1, 2, 4, 8])
def test_allowed_ensemble_values_reach_the_device_check(good):
    net = ESPCN(1, 1, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        upscale_scene(net, torch.zeros(1, 1, 20, 20), up=2, tile=16, ensemble=good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cascade_scene(net, SRCNN(1, 3, 1, 16), torch.zeros(20, 20, dtype=torch.uint8), up=2, tile=16, ensemble=good)


def test_wrappers_have_no_cpu_fallback():
    from srcgan_amd import infer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        infer.tile_gather_d4(torch.zeros(1, 1, 8, 8), "f32", 1, [(0, 0)], 4, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        infer.d4_accumulate(torch.zeros(1, 1, 4, 6), torch.zeros(1, 1, 6, 4), 1, True, 1.0)


def test_native_entry_points_reject_bad_arguments():
    from srcgan_amd import _native as N, build
    build.build(verbose=False)                      # a no-op when the library is up to date
    lib = N.lib()
    org = (C.c_int * 2)(0, 0)
    p, q = 4096, 1 << 30                            # never dereferenced: every call below is refused before any launch

    def refused(rc, word, who):
        assert rc != 0
        msg = lib.srcgan_last_error().decode()
        assert msg.startswith(who + ": ") and word in msg, msg

    g = "srcgan_tile_gather_d4"
    refused(lib.srcgan_tile_gather_d4(None, 0, 3, 8, 8, 1, p, 1, 4, 4, org, 1, None), "null", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 1, None, 1, 4, 4, org, 1, None), "null", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 1, p, 1, 4, 4, None, 1, None), "null", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 1, p, 1, 4, 4, org, 8, None), "op = 8", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 1, p, 1, 4, 4, org, -1, None), "op = -1", g)
    refused(lib.srcgan_tile_gather_d4(p, 3, 3, 8, 8, 1, p, 1, 4, 4, org, 1, None), "src_kind = 3", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 9, 8, 8, 1, p, 1, 4, 4, org, 1, None), "C = 9", g)
    refused(lib.srcgan_tile_gather_d4(p, 1, 2, 8, 8, 1, p, 1, 4, 4, org, 1, None), "C = 2", g)
    refused(lib.srcgan_tile_gather_d4(p, 2, 1, 8, 8, 1, p, 1, 4, 4, org, 1, None), "C = 1", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 0, p, 1, 4, 4, org, 1, None), "s = 0", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 1, p, 1, 1 << 20, 4, org, 1, None), "launch limit", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 1, p, 1, 4, 1 << 20, org, 1, None), "launch limit", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 1, p, 1, 4, 4, (C.c_int * 2)(8, 0), 1, None), "outside", g)
    refused(lib.srcgan_tile_gather_d4(p, 0, 3, 8, 8, 2, p, 1, 4, 4, (C.c_int * 2)(0, 16), 1, None), "outside", g)
    a = "srcgan_d4_accumulate"
    refused(lib.srcgan_d4_accumulate(None, q, 3, 4, 6, 1, 1, 1.0, None), "null", a)
    refused(lib.srcgan_d4_accumulate(p, None, 3, 4, 6, 1, 1, 1.0, None), "null", a)
    refused(lib.srcgan_d4_accumulate(p, q, 3, 4, 6, 8, 1, 1.0, None), "op = 8", a)
    refused(lib.srcgan_d4_accumulate(p, q, 3, 4, 6, -1, 1, 1.0, None), "op = -1", a)
    refused(lib.srcgan_d4_accumulate(p, q, 0, 4, 6, 1, 1, 1.0, None), "bad extents", a)
    refused(lib.srcgan_d4_accumulate(p, q, 3, 0, 6, 1, 1, 1.0, None), "bad extents", a)
    refused(lib.srcgan_d4_accumulate(p, q, 3, 4, 1 << 20, 1, 1, 1.0, None), "launch limit", a)
    refused(lib.srcgan_d4_accumulate(p, q, 3, 4, 6, 1, 1, float("nan"), None), "finite", a)
    refused(lib.srcgan_d4_accumulate(p, q, 3, 4, 6, 1, 1, float("inf"), None), "finite", a)
    refused(lib.srcgan_d4_accumulate(p, p, 3, 4, 6, 1, 0, 1.0, None), "alias", a)
    refused(lib.srcgan_d4_accumulate(p, p + 3 * 4 * 6 * 4 - 4, 3, 4, 6, 1, 0, 1.0, None), "alias", a)       # the last element overlaps


def test_the_three_gather_symbols_share_their_checks():
    from srcgan_amd import _native as N, build
    build.build(verbose=False)
    lib = N.lib()
    p = 4096
    rc = lib.srcgan_tile_gather_ex(p, 1, 2, 8, 8, 1, p, 1, 4, 4, (C.c_int * 2)(0, 0), None)
    ex = lib.srcgan_last_error().decode().partition(": ")
    rc4 = lib.srcgan_tile_gather_d4(p, 1, 2, 8, 8, 1, p, 1, 4, 4, (C.c_int * 2)(0, 0), 5, None)
    d4 = lib.srcgan_last_error().decode().partition(": ")
    assert rc != 0 and rc4 != 0 and (ex[0], d4[0]) == ("srcgan_tile_gather_ex", "srcgan_tile_gather_d4") and ex[2] == d4[2]
