"""CPU: the checks of tests/test_gpu_workspace_hygiene.py have teeth.  Three small fake "drivers" written in torch obtain their workspace
through ``srcgan_amd._native.workspace`` and their gradient buffer through ``srcgan_amd.model._GradArena``, the way the native drivers'
host code does, under tests/ws_guard.py with device "cpu".  Each has one of the faults the GPU test exists to catch -- a float read that
was never written, four bytes written past the end of the region, one gradient element left unwritten -- and a corrected twin: the checks
fail for the first and pass for the second."""
import pytest
import torch

import ws_guard as WG
from ws_guard import NAN, STALE, ZERO, guarded, run_fills

N_IN = 24


def _x(scale):
    return torch.arange(1, N_IN + 1, dtype=torch.float32) * 0.25 * scale


def _check(guard):
    if guard is not None:
        guard.check()


def driver_sum(read):
    """y = sum of 2 x, staged through a float workspace of N_IN + 8 floats; ``read`` floats of it are summed (N_IN were written)"""
    def compute(guard, scale):
        from srcgan_amd import _native as N
        ws = N.workspace(4 * (N_IN + 8), "cpu").view(torch.float32)
        ws[:N_IN] = 2.0 * _x(scale)
        y = ws[:read].sum().reshape(1).clone()
        _check(guard)
        return {"y": y}
    return compute


def driver_overrun(extra):
    """writes x into a workspace of N_IN floats, and ``extra`` bytes beyond its end (through the storage, as a kernel with a wrong bound would)"""
    def compute(guard, scale):
        from srcgan_amd import _native as N
        ws = N.workspace(4 * N_IN, "cpu")
        ws.view(torch.float32)[:] = _x(scale)
        if extra:
            past = torch.empty(0, dtype=torch.uint8).set_(ws.untyped_storage(), ws.storage_offset() + ws.numel(), (extra,), (1,))
            past.fill_(0x3C)
        y = ws.view(torch.float32).sum().reshape(1).clone()
        _check(guard)
        return {"y": y}
    return compute


def driver_grads(skip):
    """the "backward" of sum(w * x): dw = x, written into a _GradArena -- all but the last ``skip`` elements of the second parameter"""
    params = [torch.zeros(8), torch.zeros(4, 4)]

    def compute(guard, scale):
        from srcgan_amd import model as M
        arena = M._GradArena(params, [True, True])
        x = _x(scale)
        arena.views[0].copy_(x[:8])
        arena.views[1].reshape(-1)[:16 - skip] = x[8:24 - skip]
        _check(guard)
        return {"dw0": arena.views[0].clone(), "dw1": arena.views[1].clone()}
    return compute


def test_read_of_an_unwritten_float_is_caught():
    with pytest.raises(AssertionError, match="non-finite|differs"):
        run_fills(driver_sum(N_IN + 1), "cpu", expected=[("workspace", 4 * (N_IN + 8))])
    runs = run_fills(driver_sum(N_IN), "cpu", expected=[("workspace", 4 * (N_IN + 8))])
    assert set(runs) == {"stock", "ZERO", "NAN", "STALE"} and float(runs["NAN"]["y"]) == float(2.0 * _x(1.0).sum())


def test_each_fill_alone_sees_the_unwritten_float_where_it_can():
    """ZERO hides it (that is the idle card's benign page), NAN and STALE do not"""
    faulty, want = driver_sum(N_IN + 1), float(2.0 * _x(1.0).sum())
    with guarded(ZERO, "cpu") as g:
        assert float(faulty(g, 1.0)["y"]) == want
    with guarded(NAN, "cpu") as g:
        with pytest.raises(AssertionError, match="non-finite"):
            WG.assert_finite(faulty(g, 1.0), "NAN")
    with guarded(ZERO, "cpu") as prev:
        driver_sum(N_IN)(prev, -3.0)
        prev.allocs[0].view.view(torch.float32)[N_IN:] = 7.0           # the previous user of the buffer wrote more of it
    with guarded(STALE, "cpu", previous=prev) as g:
        assert float(faulty(g, 1.0)["y"]) == want + 7.0


def test_four_bytes_past_the_end_are_caught():
    # no stock run: past a plain torch.empty there is no storage to write to
    with pytest.raises(AssertionError, match=r"guard past allocation .*offset 96 "):
        run_fills(driver_overrun(4), "cpu", stock=False)
    run_fills(driver_overrun(0), "cpu", expected=[("workspace", 4 * N_IN)])


def test_an_over_write_in_front_of_the_region_is_caught():
    with guarded(NAN, "cpu") as g:
        from srcgan_amd import _native as N
        ws = N.workspace(64, "cpu")
        g.check()
        torch.empty(0, dtype=torch.uint8).set_(ws.untyped_storage(), ws.storage_offset() - 2, (2,), (1,)).fill_(0)
        with pytest.raises(AssertionError, match=r"guard before allocation .*offset -2 "):
            g.check()


def test_an_unwritten_gradient_element_is_caught():
    expected = [("grad_arena", 4 * 24)]
    with pytest.raises(AssertionError, match="dw1"):
        run_fills(driver_grads(1), "cpu", expected=expected)
    runs = run_fills(driver_grads(0), "cpu", expected=expected)
    assert torch.equal(runs["STALE"]["dw1"].reshape(-1), _x(1.0)[8:])


def test_an_allocation_the_patch_does_not_see_is_caught():
    """assertion 4 of the GPU test: a workspace allocated some other way leaves the recorded set short of the planners' answer"""
    def bypass(guard, scale):
        ws = torch.zeros(4 * N_IN, dtype=torch.uint8).view(torch.float32)
        ws[:] = _x(scale)
        return {"y": ws.sum().reshape(1)}
    with pytest.raises(AssertionError, match="planners answer"):
        run_fills(bypass, "cpu", expected=[("workspace", 4 * N_IN)])


def test_the_patches_are_restored_and_keep_the_originals_behaviour():
    from srcgan_amd import _native as N
    from srcgan_amd import model as M
    stock = (N.workspace, M._GradArena, M._PackState.opts)
    with pytest.raises(ZeroDivisionError):
        with guarded(NAN, "cpu") as g:
            assert N.workspace is not stock[0] and issubclass(M._GradArena, stock[1]) and M._GradArena is not stock[1]
            ws = N.workspace(100, "cpu")
            assert ws.dtype == torch.uint8 and ws.numel() == 100 and ws.data_ptr() % 4096 == g.allocs[0].parent.data_ptr() % 4096
            assert bool((ws == 0xFF).all()) and WG.G % 4096 == 0
            arena = M._GradArena([torch.zeros(3), torch.zeros(2, 2), torch.zeros(5)], [True, False, True])
            assert arena.flat.numel() == 8 and arena.views[1] is None and arena.views[2].shape == (5,) and arena.offsets == [0, 3, 3, 8]
            assert bool(torch.isnan(arena.flat).all()) and arena.views[2].data_ptr() == arena.flat.data_ptr() + 12
            assert [a.kind for a in g.allocs] == ["workspace", "grad_arena"] and g.allocs[0].tag.endswith("test_the_patches_are_restored_and_keep_the_originals_behaviour")
            1 / 0
    assert (N.workspace, M._GradArena, M._PackState.opts) == stock


def test_a_rejected_plan_raises_as_in_the_original():
    from srcgan_amd import _native as N
    with guarded(ZERO, "cpu"):
        with pytest.raises(RuntimeError):
            N.workspace(0, "cpu")


def test_guarded_slabs_redirect_the_descriptor_and_check_after_the_call(monkeypatch):
    """a fake srcgan_conv_wgrad that clears its slab: four bytes too many are caught, the exact size passes, the entry points come back"""
    import ctypes as C
    from srcgan_amd import _native as N
    lib = N.lib()
    real = lib.srcgan_conv_wgrad
    d = N.WgradDesc()
    d.Cout, d.Cin, d.kh, d.kw, d.nsplit = 32, 16, 3, 3, 2
    need = int(lib.srcgan_conv_wgrad_slab_bytes(32, 16, 3, 3, 2))
    assert need > 0
    own = torch.zeros(8, dtype=torch.uint8)
    seen = []

    def fake(over):
        def call(dref, stream):
            seen.append(dref._obj.slab)
            C.memset(dref._obj.slab, 0, need + over)
            return 0
        return call

    for over, ok in ((0, True), (4, False)):
        d.slab = own.data_ptr()
        monkeypatch.setattr(lib, "srcgan_conv_wgrad", fake(over))
        with WG.guarded_slabs(NAN, "cpu") as g:
            if ok:
                assert lib.srcgan_conv_wgrad(C.byref(d), None) == 0
            else:
                with pytest.raises(AssertionError, match=rf"guard past allocation 'srcgan_conv_wgrad slab' .*offset {need} "):
                    lib.srcgan_conv_wgrad(C.byref(d), None)
        assert g.calls == 1 and seen[-1] != own.data_ptr() and not own.any()
    monkeypatch.setattr(lib, "srcgan_conv_wgrad", real)
    assert lib.srcgan_conv_wgrad is real


def test_stale_refuses_a_size_the_previous_block_never_had():
    from srcgan_amd import _native as N
    with guarded(ZERO, "cpu") as prev:
        N.workspace(64, "cpu")
    with guarded(STALE, "cpu", previous=prev):
        with pytest.raises(AssertionError, match="never allocated"):
            N.workspace(128, "cpu")
