"""CPU: the tile plan of srcgan_amd.infer (partition, halo, multiples, feather weights), the receptive radii against the float64
oracle (a crop-stitched tiling must equal the whole-scene forward), and the argument checks of the new entry points.  No GPU."""
import ctypes as C
import itertools

import pytest
import torch

import oracle
from net_ref import stitch
from srcgan_amd import infer
from srcgan_amd import ESPCN, SRCNN, EDSR, RDDBNet, RDDBNetB, ResDeconv, plan_tiles, receptive_halo, upscale_scene

SCENES = [(16, 16), (37, 53), (45, 70)]
PLANS = list(itertools.product(SCENES, (4, 16, 64), (0, 3, 20), (1, 8)))


@pytest.mark.parametrize("hw,tile,halo,multiple", PLANS)
def test_plan_properties(hw, tile, halo, multiple):
    H, W = hw
    plan = plan_tiles(H, W, tile, halo, multiple)
    cover = torch.zeros(H, W, dtype=torch.int32)
    for t in plan.tiles:
        cy0, cy1, cx0, cx1 = t.core
        cover[cy0:cy1, cx0:cx1] += 1
        # the tile holds its core plus the halo, or reaches the border
        assert t.y0 <= max(cy0 - halo, 0) and t.x0 <= max(cx0 - halo, 0)
        assert t.y0 + t.th >= min(cy1 + halo, H) and t.x0 + t.tw >= min(cx1 + halo, W)
        assert 0 <= t.y0 < H and 0 <= t.x0 < W
        assert t.th % multiple == 0 and t.tw % multiple == 0
        if multiple == 1:
            assert t.y0 + t.th <= H and t.x0 + t.tw <= W
        # a feathered write-back stays inside the tile and inside the scene
        sy0, sy1, sx0, sx1 = t.support
        assert max(t.y0, 0) <= sy0 <= cy0 and cy1 <= sy1 <= min(t.y0 + t.th, H)
        assert max(t.x0, 0) <= sx0 <= cx0 and cx1 <= sx1 <= min(t.x0 + t.tw, W)
        assert t.ramps[0] + t.ramps[1] <= sy1 - sy0 and t.ramps[2] + t.ramps[3] <= sx1 - sx0
    assert int(cover.min()) == 1 and int(cover.max()) == 1          # cores: every pixel exactly once
    # classes: every tile in exactly one, shapes equal, indices in running order
    seen = [i for idx in plan.classes.values() for i in idx]
    assert seen == list(range(len(plan.tiles)))
    for (th, tw), idx in plan.classes.items():
        assert all((plan.tiles[i].th, plan.tiles[i].tw) == (th, tw) for i in idx)
    # feather weights: a partition of unity, at most 4 tiles at a pixel (one f32 rounding each) -> 1e-6
    for up in (1, 2):
        total = torch.zeros(H * up, W * up, dtype=torch.float64)
        count = torch.zeros(H * up, W * up, dtype=torch.int32)
        for t in plan.tiles:
            sy0, sy1, sx0, sx1 = t.support
            w = plan.weights(t, up)
            assert w.dtype == torch.float32 and tuple(w.shape) == ((sy1 - sy0) * up, (sx1 - sx0) * up)
            assert float(w.min()) > 0.0 and float(w.max()) <= 1.0
            total[sy0 * up:sy1 * up, sx0 * up:sx1 * up] += w.double()
            count[sy0 * up:sy1 * up, sx0 * up:sx1 * up] += 1
        assert int(count.max()) <= 4 and int(count.min()) >= 1
        assert float((total - 1.0).abs().max()) <= 1e-6


def test_plan_ramps_are_as_wide_as_the_halo_allows():
    plan = plan_tiles(40, 56, 16, 8, 8)
    interior = [t for t in plan.tiles if t.core == (16, 32, 16, 32)][0]
    assert interior.ramps == (16, 16, 16, 16) and interior.support == (8, 40, 8, 40)
    assert plan_tiles(40, 56, 16, 0).tiles[0].ramps == (0, 0, 0, 0)
    assert plan_tiles(64, 64, 16, 3, 8).overruns and not plan_tiles(37, 53, 16, 3, 1).overruns
    assert len(plan_tiles(37, 53, 4, 0).tiles) == 140


def _sd64(net):
    return {k: v.detach().double() for k, v in net.state_dict().items()}


def _halo_cases():
    torch.manual_seed(5)
    cases = []
    for up in (2, 4):
        sd = {k: v.double() for k, v in oracle.rddbnet_state(3, 3, up, 8, 1, 8, seed=3).items()}
        cases.append((f"rddbnet_x{up}", RDDBNet(3, 3, up, nf=8, nb=1, gc=8), 3, up, (lambda s, u: lambda x: oracle.rddbnet_forward(s, x, u))(sd, up)))
    for up in (2, 3):
        net = ESPCN(1, 1, up, base_kernel=8)
        cases.append((f"espcn_x{up}", net, 1, up, (lambda s, u: lambda x: oracle.espcn_forward(s, x, u))(_sd64(net), up)))
    net = SRCNN(1, 1, 2, base_kernel=8)
    cases.append(("srcnn", net, 1, 1, (lambda s: lambda x: oracle.srcnn_forward(s, x))(_sd64(net))))
    net = RDDBNetB(3, 3, 8, nb=1, gc=8, mode="x2")
    cases.append(("rddbnetb_x2", net, 3, 2, (lambda s: lambda x: oracle.rddbnetb_forward(s, x, "x2"))(_sd64(net))))
    return cases


@pytest.mark.parametrize("case", _halo_cases(), ids=lambda c: c[0])
def test_receptive_halo_is_sufficient_in_float64(case):
    """Crop-stitched tiles with halo = receptive_halo(net) == the whole-scene forward, <= 1e-10 relative in float64 (rounding over ~20
    layers stays orders below; a missing halo pixel is a real dependency).  One pixel less is NOT enough: the radius is tight."""
    name, net, in_ch, up, forward = case
    torch.manual_seed(7)
    x = torch.rand(1, in_ch, 40, 56, dtype=torch.float64)
    halo = receptive_halo(net)
    with torch.no_grad():
        whole = forward(x)
        tiled = stitch(forward, x, up, 16, halo)
        short = stitch(forward, x, up, 16, halo - 1)
    assert tuple(whole.shape[2:]) == (40 * up, 56 * up)
    rel = float((tiled - whole).abs().max() / whole.abs().max())
    rel_short = float((short - whole).abs().max() / whole.abs().max())
    print(f"{name}: halo {halo}: rel {rel:.3e}; halo {halo - 1}: rel {rel_short:.3e}")
    assert rel <= 1e-10
    assert rel_short > 1e-10


def test_receptive_halo_values_and_refusals():
    assert receptive_halo(RDDBNet(3, 3, 4, nf=8, nb=1, gc=8)) == 18
    assert receptive_halo(RDDBNet(3, 3, 4, nf=8, nb=23, gc=8)) == 15 * 23 + 3
    assert receptive_halo(ESPCN(1, 1, 2)) == 6 and receptive_halo(SRCNN(1, 1, 2)) == 6
    assert receptive_halo(RDDBNetB(3, 3, 8, nb=2, gc=8, mode="x2")) == 38
    assert receptive_halo(RDDBNetB(3, 3, 8, nb=2, gc=8, mode="x4")) == 35
    with pytest.raises(ValueError, match="normalisation"):
        receptive_halo(ResDeconv(1, 3))
    with pytest.raises(ValueError, match="normalisation"):
        receptive_halo(EDSR(3, 3, 2, num_residuals=1))
    with pytest.raises(ValueError, match="halo="):
        receptive_halo(torch.nn.Conv2d(3, 3, 3))
    assert infer._chain_halo([ESPCN(1, 1, 2), SRCNN(1, 1, 2)]) == 6 + 3          # SRCNN's 6 HR pixels behind an x2 stage


def test_upscale_scene_argument_checks():
    net = ESPCN(1, 1, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        upscale_scene(net, torch.zeros(1, 1, 20, 20), up=2, tile=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        upscale_scene([net], torch.zeros(20, 20, 1, dtype=torch.uint8), up=2, tile=16, halo=4, blend="feather", out="u8")
    with pytest.raises(ValueError, match="normalisation"):
        upscale_scene([net, ResDeconv(1, 3)], torch.zeros(1, 1, 32, 32), up=2, tile=16, blend="crop", halo=None)
    with pytest.raises(ValueError, match="exact mode"):
        upscale_scene(net, torch.zeros(1, 1, 20, 20), up=2, tile=16, blend="feather")
    with pytest.raises(ValueError, match="blend"):
        upscale_scene(net, torch.zeros(1, 1, 20, 20), up=2, blend="average")


def test_native_entry_points_reject_bad_arguments():
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

    refused(lib.srcgan_tile_gather(None, 0, 3, 8, 8, p, 1, 4, 4, org, None), "null")
    refused(lib.srcgan_tile_gather(p, 0, 3, 8, 8, None, 1, 4, 4, org, None), "null")
    refused(lib.srcgan_tile_gather(p, 0, 3, 8, 8, p, 1, 4, 4, None, None), "null")
    refused(lib.srcgan_tile_gather(p, 0, 0, 8, 8, p, 1, 4, 4, org, None), "C = 0")
    refused(lib.srcgan_tile_gather(p, 0, 9, 8, 8, p, 1, 4, 4, org, None), "C = 9")
    refused(lib.srcgan_tile_gather(p, 1, 2, 8, 8, p, 1, 4, 4, org, None), "C = 2")
    refused(lib.srcgan_tile_gather(p, 0, 3, 8, 8, p, 1, 4, 1 << 20, org, None), "launch limit")
    refused(lib.srcgan_tile_gather(p, 0, 3, 8, 8, p, 1, 4, 4, (C.c_int * 2)(8, 0), None), "outside")
    refused(lib.srcgan_tile_scatter(None, p, 3, 8, 8, 2, 1, 4, 4, rect, 0, None), "null")
    refused(lib.srcgan_tile_scatter(p, None, 3, 8, 8, 2, 1, 4, 4, rect, 0, None), "null")
    refused(lib.srcgan_tile_scatter(p, p, 3, 8, 8, 2, 1, 4, 4, None, 0, None), "null")
    refused(lib.srcgan_tile_scatter(p, p, 0, 8, 8, 2, 1, 4, 4, rect, 0, None), "C = 0")
    refused(lib.srcgan_tile_scatter(p, p, 9, 8, 8, 2, 1, 4, 4, rect, 0, None), "C = 9")
    refused(lib.srcgan_tile_scatter(p, p, 3, 8, 8, 0, 1, 4, 4, rect, 0, None), "up = 0")
    refused(lib.srcgan_tile_scatter(p, p, 3, 8, 8, 2, 1, 1 << 14, 4, rect, 0, None), "launch limit")
    refused(lib.srcgan_tile_scatter(p, p, 3, 8, 8, 2, 1, 4, 4, (C.c_int * 10)(0, 0, 0, 4, 0, 9, 0, 0, 0, 0), 0, None), "leaves")
    refused(lib.srcgan_tile_scatter(p, p, 3, 8, 8, 2, 1, 4, 4, (C.c_int * 10)(0, 0, 0, 4, 0, 4, 2, 0, 0, 0), 0, None), "crop mode")
    refused(lib.srcgan_planes_to_u8hwc(None, p, 3, 64, None), "null")
    refused(lib.srcgan_planes_to_u8hwc(p, None, 3, 64, None), "null")
    refused(lib.srcgan_planes_to_u8hwc(p, p, 0, 64, None), "C = 0")
    refused(lib.srcgan_planes_to_u8hwc(p, p, 9, 64, None), "C = 9")


def test_native_entry_points_share_their_checks():
    """One bad argument list is refused by both write-back symbols, and one by both gather symbols, in the same words after each
    symbol's own name.  Nothing launches: the dummy pointer is never dereferenced."""
    from srcgan_amd import _native as N, build
    build.build(verbose=False)
    lib = N.lib()
    p = 4096

    def message(rc):
        assert rc != 0
        name, _, text = lib.srcgan_last_error().decode().partition(": ")
        return name, text

    # 8x8 scene, up = 2, one 4x4 tile at (2, 2); a rectangle is (y0, x0, sy0, sy1, sx0, sx1, ny_lo, ny_hi, nx_lo, nx_hi)
    for rect, word in [((2, 2, 2, 6, 2, 7, 0, 0, 0, 0), "leaves"),                   # one column past the tile
                       ((2, 2, 1, 6, 2, 6, 0, 0, 0, 0), "leaves"),                   # one row above the tile
                       ((6, 6, 6, 9, 6, 8, 0, 0, 0, 0), "leaves"),                   # inside the tile, one row below the scene
                       ((2, 2, 2, 6, 2, 6, 3, 2, 0, 0), "overlap"),                  # 3 + 2 ramp rows in a rectangle of 4
                       ((2, 2, 2, 6, 2, 6, 0, 0, -1, 0), "overlap"),
                       ((2, 2, 2, 6, 2, 6, 2, 0, 0, 0), "no ramps")]:                # crop mode
        r = (C.c_int * 10)(*rect)
        f32 = message(lib.srcgan_tile_scatter(p, p, 3, 8, 8, 2, 1, 4, 4, r, 0, None))
        u8 = message(lib.srcgan_tile_scatter_u8(p, 3, None, 0, p, 8, 8, 2, 1, 4, 4, r, 0, None))
        assert (f32[0], u8[0]) == ("srcgan_tile_scatter", "srcgan_tile_scatter_u8") and f32[1] == u8[1] and word in f32[1], (rect, f32, u8)
    for args, word in [(dict(up=0), "up = 0"), (dict(H=0), "bad extents"), (dict(th=1 << 14), "launch limit")]:
        H, up, th = ({"H": 8, "up": 2, "th": 4, **args}[k] for k in ("H", "up", "th"))
        r = (C.c_int * 10)(0, 0, 0, 4, 0, 4, 0, 0, 0, 0)
        f32 = message(lib.srcgan_tile_scatter(p, p, 3, H, 8, up, 1, th, 4, r, 0, None))
        u8 = message(lib.srcgan_tile_scatter_u8(p, 3, None, 0, p, H, 8, up, 1, th, 4, r, 0, None))
        assert f32[1] == u8[1] and word in f32[1], (args, f32, u8)

    # the gather, s = 1: (kind = src_u8, C, H, th, origins)
    org = (C.c_int * 2)(0, 0)
    for kind, Cc, H, th, o, word in [(0, 3, 8, 4, None, "null"), (0, 9, 8, 4, org, "C = 9"), (1, 2, 8, 4, org, "C = 2"), (0, 3, 0, 4, org, "bad extents"),
                                     (1, 3, 8, 1 << 20, org, "launch limit"), (0, 3, 8, 4, (C.c_int * 2)(0, 8), "outside"),
                                     (1, 1, 8, 4, (C.c_int * 2)(-1, 0), "outside")]:
        plain = message(lib.srcgan_tile_gather(p, kind, Cc, H, 8, p, 1, th, 4, o, None))
        ex = message(lib.srcgan_tile_gather_ex(p, kind, Cc, H, 8, 1, p, 1, th, 4, o, None))
        assert (plain[0], ex[0]) == ("srcgan_tile_gather", "srcgan_tile_gather_ex") and plain[1] == ex[1] and word in plain[1], (word, plain, ex)
