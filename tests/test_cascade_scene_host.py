"""CPU: the argument checks of ``cascade_scene`` and the plan it runs -- the Const variants plan on the up-sampled grid.  No GPU."""
import pytest
import torch

from srcgan_amd import ESPCN, SRCNN, SRDN, RDDBNet, ResDeconv, cascade_scene, plan_tiles
from srcgan_amd import infer


def _gray(h=20, w=24):
    return torch.zeros(h, w, dtype=torch.uint8)


def test_cascade_scene_is_exported():
    import srcgan_amd
    assert srcgan_amd.cascade_scene is infer.cascade_scene and "cascade_scene" in srcgan_amd.__all__ and "cascade_scene" in infer.__all__


def test_const_needs_a_size_preserving_sr_network():
    col = SRCNN(1, 3, 1, 16)
    with pytest.raises(ValueError, match="size-preserving"):
        cascade_scene(RDDBNet(1, 1, 2, nf=16, nb=1, gc=8), col, _gray(), up=2, const=True)
    with pytest.raises(ValueError, match="size-preserving"):
        cascade_scene(ESPCN(1, 1, 2), col, _gray(), up=2, const=True, halo=4)
    with pytest.raises(ValueError, match="size-preserving"):
        cascade_scene(torch.nn.Conv2d(1, 1, 3, padding=1), col, _gray(), up=2, const=True, halo=4)      # unknown module: scale unknown


def test_wrong_space_out_blend_and_scene_are_refused():
    sr, col = SRCNN(1, 1, 1, 16), SRCNN(1, 3, 1, 16)
    with pytest.raises(ValueError, match="space"):
        cascade_scene(sr, col, _gray(), up=2, const=True, space="yuv")
    with pytest.raises(ValueError, match="out"):
        cascade_scene(sr, col, _gray(), up=2, const=True, out="f16")
    with pytest.raises(ValueError, match="blend"):
        cascade_scene(sr, col, _gray(), up=2, const=True, blend="average")
    with pytest.raises(ValueError, match="exact mode"):
        cascade_scene(sr, col, _gray(), up=2, const=True, blend="feather")                 # halo=None with feather
    with pytest.raises(TypeError, match="modules"):
        cascade_scene([sr], col, _gray(), up=2)
    for bad in (torch.zeros(20, 24, 2, dtype=torch.uint8), torch.zeros(1, 3, 20, 24), torch.zeros(2, 1, 20, 24), torch.zeros(20, 24)):
        with pytest.raises(ValueError, match="scene must be"):
            cascade_scene(sr, col, bad, up=2, const=True)


def test_exact_mode_refuses_normalisation_layers():
    with pytest.raises(ValueError, match="normalisation"):
        cascade_scene(SRCNN(1, 1, 1, 16), ResDeconv(1, 2), _gray(32, 32), up=2, const=True, space="lab", halo=None)
    with pytest.raises(ValueError, match="normalisation"):
        cascade_scene(ESPCN(1, 1, 2), ResDeconv(1, 3), torch.zeros(1, 1, 32, 32), up=2)
    with pytest.raises(ValueError, match="would not be exact"):
        cascade_scene(ESPCN(1, 1, 2), SRCNN(1, 3, 1, 16), _gray(40, 56), up=2, tile=16, multiple=16)


def test_cpu_scene_has_no_fallback():
    sr, col = SRCNN(1, 1, 1, 16), SRCNN(1, 2, 1, 16)
    for scene in (_gray(), torch.zeros(20, 24, 3, dtype=torch.uint8), torch.zeros(1, 1, 20, 24)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cascade_scene(sr, col, scene, up=2, const=True, space="lab", tile=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cascade_scene(SRDN(1, 1, 2, nf=16, nb=1, gc=8), ResDeconv(1, 2), _gray(), up=2, const=True, space="lab", tile=32, halo=8,
                      multiple=16, blend="feather")


def test_const_plan_is_made_on_the_upsampled_grid():
    sr, col = SRCNN(1, 1, 1, 16), SRCNN(1, 2, 1, 16)
    H, W, up = 24, 26, 2
    plan = infer._cascade_plan(sr, col, H, W, up=up, const=True, tile=16, halo=None, multiple=1)
    assert (plan.H, plan.W) == (H * up, W * up)
    assert plan.halo == 12                                             # SRCNN 6 + SRCNN 6 at scale 1: the interpolation adds nothing
    ref = plan_tiles(H * up, W * up, 16, 12, 1)
    assert plan.tiles == ref.tiles and plan.classes == ref.classes
    assert len(plan.tiles) == 3 * 4                                    # 48 x 52 in cores of 16
    # an explicit halo and a multiple are on that grid too
    plan = infer._cascade_plan(SRDN(1, 1, 2, nf=16, nb=1, gc=8), ResDeconv(1, 2), 24, 24, up=2, const=True, tile=32, halo=8, multiple=16)
    assert (plan.H, plan.W, plan.halo) == (48, 48, 8)
    assert all(t.th % 16 == 0 and t.tw % 16 == 0 for t in plan.tiles) and plan.overruns
    # const=False: the scene's own grid, the second network's radius shrunk by the first one's scale (ESPCN 6 + ceil(6 / 2))
    plan = infer._cascade_plan(ESPCN(1, 1, 2), col, H, W, up=up, const=False, tile=16, halo=None, multiple=1)
    assert (plan.H, plan.W, plan.halo) == (H, W, 9)


def test_native_entry_points_reject_bad_arguments():
    import ctypes as C
    from srcgan_amd import _native as N, build
    build.build(verbose=False)                      # a no-op when the library is up to date
    lib = N.lib()
    org = (C.c_int * 2)(0, 0)
    rect = (C.c_int * 10)(0, 0, 0, 4, 0, 4, 0, 0, 0, 0)
    p = 4096                                        # never dereferenced: every call below is refused before any launch

    def refused(rc, word):
        assert rc != 0
        msg = lib.srcgan_last_error().decode()
        assert word in msg, msg

    refused(lib.srcgan_tile_gather_ex(None, 0, 1, 8, 8, 2, p, 1, 4, 4, org, None), "null")
    refused(lib.srcgan_tile_gather_ex(p, 0, 1, 8, 8, 2, None, 1, 4, 4, org, None), "null")
    refused(lib.srcgan_tile_gather_ex(p, 0, 1, 8, 8, 2, p, 1, 4, 4, None, None), "null")
    refused(lib.srcgan_tile_gather_ex(p, 3, 1, 8, 8, 2, p, 1, 4, 4, org, None), "src_kind = 3")
    refused(lib.srcgan_tile_gather_ex(p, 0, 9, 8, 8, 2, p, 1, 4, 4, org, None), "C = 9")
    refused(lib.srcgan_tile_gather_ex(p, 1, 2, 8, 8, 2, p, 1, 4, 4, org, None), "C = 2")
    refused(lib.srcgan_tile_gather_ex(p, 2, 1, 8, 8, 2, p, 1, 4, 4, org, None), "C = 1")
    refused(lib.srcgan_tile_gather_ex(p, 2, 3, 8, 8, 0, p, 1, 4, 4, org, None), "s = 0")
    refused(lib.srcgan_tile_gather_ex(p, 2, 3, 1 << 20, 8, 1 << 12, p, 1, 4, 4, org, None), "2^30")
    refused(lib.srcgan_tile_gather_ex(p, 0, 1, 8, 8, 2, p, 1, 4, 1 << 20, org, None), "launch limit")
    refused(lib.srcgan_tile_gather_ex(p, 0, 1, 8, 8, 2, p, 1, 4, 4, (C.c_int * 2)(16, 0), None), "outside")      # 15 is the last row at s = 2
    refused(lib.srcgan_tile_gather_ex(p, 0, 1, 8, 8, 1, p, 1, 4, 4, (C.c_int * 2)(0, 8), None), "outside")
    refused(lib.srcgan_tile_scatter_u8(None, 3, None, 0, p, 8, 8, 2, 1, 4, 4, rect, 0, None), "null")
    refused(lib.srcgan_tile_scatter_u8(p, 3, None, 0, None, 8, 8, 2, 1, 4, 4, rect, 0, None), "null")
    refused(lib.srcgan_tile_scatter_u8(p, 3, None, 0, p, 8, 8, 2, 1, 4, 4, None, 0, None), "null")
    refused(lib.srcgan_tile_scatter_u8(p, 3, None, 0, p, 8, 8, 2, 1, 4, 4, rect, 2, None), "mode = 2")
    refused(lib.srcgan_tile_scatter_u8(p, 2, None, 0, p, 8, 8, 2, 1, 4, 4, rect, 0, None), "mode 0")
    refused(lib.srcgan_tile_scatter_u8(p, 3, p, 2, p, 8, 8, 2, 1, 4, 4, rect, 0, None), "mode 0")
    refused(lib.srcgan_tile_scatter_u8(p, 1, None, 2, p, 8, 8, 2, 1, 4, 4, rect, 1, None), "mode 1")
    refused(lib.srcgan_tile_scatter_u8(p, 1, p, 3, p, 8, 8, 2, 1, 4, 4, rect, 1, None), "mode 1")
    refused(lib.srcgan_tile_scatter_u8(p, 3, None, 0, p, 8, 8, 0, 1, 4, 4, rect, 0, None), "up = 0")
    refused(lib.srcgan_tile_scatter_u8(p, 3, None, 0, p, 8, 8, 2, 1, 1 << 14, 4, rect, 0, None), "launch limit")
    refused(lib.srcgan_tile_scatter_u8(p, 3, None, 0, p, 8, 8, 2, 1, 4, 4, (C.c_int * 10)(0, 0, 0, 4, 0, 9, 0, 0, 0, 0), 0, None), "leaves")
    refused(lib.srcgan_tile_scatter_u8(p, 3, None, 0, p, 8, 8, 2, 1, 4, 4, (C.c_int * 10)(0, 0, 0, 4, 0, 4, 0, 0, 2, 0), 0, None), "no ramps")
