"""GPU: whole-scene inference (srcgan_amd.infer).  The gather / write-back kernels against torch slicing (bit-exact where they copy),
the feathered blend against a torch re-implementation in tile order, the u8 conversion, and ``upscale_scene`` end to end: exact mode
against the whole-image forward (fp32, bf16) and the ESPCN -> ResDeconv cascade in feather mode against a test-side re-implementation
of the same plan.  Shapes are small and chosen so that ragged edges, misaligned rows, tiles past the edge and launch chunking occur."""
import pytest
import torch
import torch.nn.functional as F

import oracle
from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu

SCENES = [(37, 53), (64, 64)]
PLANS = [(4, 0, 1), (16, 3, 1), (16, 3, 8)]


@pytest.fixture(scope="module")
def infer():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import infer as m
    return m


def _planes(C, H, W, kind, seed=0):
    """-> (scene as the entry point takes it, on the device; its f32 [C,H,W] planes on the host)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "u8":
        u8 = torch.randint(0, 256, (H, W, C), dtype=torch.uint8, generator=g)
        return u8.cuda(), (u8.double() / 255.0).float().permute(2, 0, 1).contiguous()
    f = torch.rand(1, C, H, W, generator=g) * 2 - 0.5
    return f.cuda(), f[0].clone()


class Tile4:
    """a 4x4 rectangle at (y0, x0), for ``_ref_tile``"""
    th = tw = 4

    def __init__(self, y0, x0):
        self.y0, self.x0 = y0, x0


def _ref_tile(planes, t):
    """torch slicing; what passes the right / bottom edge is edge replication"""
    _, H, W = planes.shape
    y1, x1 = min(t.y0 + t.th, H), min(t.x0 + t.tw, W)
    s = planes[None, :, t.y0:y1, t.x0:x1]
    return F.pad(s, (0, t.x0 + t.tw - x1, 0, t.y0 + t.th - y1), mode="replicate")[0]


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw", SCENES)
def test_gather_equals_torch_slicing_bit_exact(infer, hw, C, kind):
    H, W = hw
    scene, planes = _planes(C, H, W, kind)
    for tile, halo, multiple in PLANS:
        plan = infer.plan_tiles(H, W, tile, halo, multiple)
        if (hw, tile) == ((37, 53), 4):
            # 140 tiles; the shape classes hold at most 117, so all 140 origins also go through ONE call at the common 4x4 shape
            # (more than the 128 a launch carries: chunking), where the ragged right / bottom tiles pass the edge
            assert len(plan.tiles) == 140
            got = infer.tile_gather(scene, [(t.y0, t.x0) for t in plan.tiles], 4, 4).cpu()
            ref = torch.stack([_ref_tile(planes, Tile4(t.y0, t.x0)) for t in plan.tiles])
            assert got.shape == ref.shape and torch.equal(got, ref), (hw, C, kind, "140 origins in one call")
        if (hw, multiple) == ((64, 64), 8):
            assert plan.overruns                                                     # right and bottom tiles pass the edge
        for (th, tw), idx in plan.classes.items():
            got = infer.tile_gather(scene, [(plan.tiles[i].y0, plan.tiles[i].x0) for i in idx], th, tw).cpu()
            ref = torch.stack([_ref_tile(planes, plan.tiles[i]) for i in idx])
            assert got.shape == ref.shape and torch.equal(got, ref), (hw, C, kind, tile, halo, multiple, th, tw)


def test_gather_u8_mapping_is_arr2rgb(infer):
    from srcgan_amd import data
    u8 = torch.arange(256, dtype=torch.uint8).repeat(3)[:16 * 16 * 3].reshape(16, 16, 3).contiguous().cuda()
    got = infer.tile_gather(u8, [(0, 0)], 16, 16)[0]
    assert torch.equal(got, data.arr2rgb(u8))
    # a misaligned f32 scene pointer takes the scalar path and gives the same bits as the aligned one
    base = torch.rand(3 * 64 * 64 + 1, device="cuda")
    off = base[1:].view(3, 64, 64)
    assert off.data_ptr() % 16 != 0
    assert torch.equal(infer.tile_gather(off, [(16, 16), (48, 44)], 24, 24), infer.tile_gather(off.clone(), [(16, 16), (48, 44)], 24, 24))


def test_gather_f32_vector_load_path(infer):
    """The f32, s = 1 gather takes a unit as one 16-byte load where the scene is aligned (base and pitch), x0 % 4 == 0 and the unit
    lies inside the row: x0 = 0, 4 take it, x0 = 3 does not, x0 = 20 takes it for the first unit of a row and replicates the edge in
    the second (20 + 4 + 3 >= W = 24); the same scene one float further on never takes it.  All equal torch slicing, bit for bit,
    through ``tile_gather`` and through ``tile_gather_ex``."""
    C, H, W, T = 3, 20, 24, 8
    base = torch.rand(C * H * W + 1, generator=torch.Generator().manual_seed(7)) * 2 - 0.5
    origins = [(0, 0), (5, 4), (13, 3), (12, 20)]                                    # y0 = 13: the last row is replicated too
    for off in (0, 1):
        planes = base[off:off + C * H * W].view(C, H, W)
        scene = base.cuda()[off:off + C * H * W].view(C, H, W)
        assert (scene.data_ptr() % 16 == 0) == (off == 0) and scene.is_contiguous()
        ref = torch.stack([_ref_tile(planes, type("T", (), dict(y0=y0, x0=x0, th=T, tw=T))) for y0, x0 in origins])
        assert torch.equal(infer.tile_gather(scene, origins, T, T).cpu(), ref), off
        assert torch.equal(infer.tile_gather_ex(scene, "f32", 1, origins, T, T).cpu(), ref), off


def _hr_tiles(plan, idx, C, up, seed, ones=False):
    th, tw = plan.tiles[idx[0]].th, plan.tiles[idx[0]].tw
    if ones:
        return torch.ones(len(idx), C, th * up, tw * up)
    return torch.rand(len(idx), C, th * up, tw * up, generator=torch.Generator().manual_seed(seed)) - 0.25


GUARD = 3          # rows allocated around the destination scene


def _guarded(C, SH, SW, fill):
    buf = torch.full((C * SH * SW + 2 * GUARD * SW,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD * SW:GUARD * SW + C * SH * SW].view(C, SH, SW)


@pytest.mark.parametrize("up", [1, 2, 4])
@pytest.mark.parametrize("hw", SCENES)
def test_crop_scatter_equals_torch_slicing_bit_exact(infer, hw, up):
    H, W = hw
    C, sentinel = 3, -77.0
    for tile, halo, multiple in PLANS:
        plan = infer.plan_tiles(H, W, tile, halo, multiple)
        buf, dst = _guarded(C, H * up, W * up, sentinel)
        ref = torch.full((C, H * up, W * up), sentinel)
        for k, ((th, tw), idx) in enumerate(plan.classes.items()):
            tiles = _hr_tiles(plan, idx, C, up, seed=k)
            infer.tile_scatter(tiles.cuda(), dst, up, plan.rects(idx, False), False)
            for n, i in enumerate(idx):
                t = plan.tiles[i]
                cy0, cy1, cx0, cx1 = t.core
                ref[:, cy0 * up:cy1 * up, cx0 * up:cx1 * up] = tiles[n, :, (cy0 - t.y0) * up:(cy1 - t.y0) * up, (cx0 - t.x0) * up:(cx1 - t.x0) * up]
        got = dst.cpu()
        assert not bool((ref == sentinel).any())                       # the reference itself covers the scene
        assert torch.equal(got, ref), (hw, up, tile, halo, multiple)   # bit-exact; hence no sentinel left inside the scene
        guard = buf.cpu()
        n = GUARD * W * up
        assert bool((guard[:n] == sentinel).all()) and bool((guard[-n:] == sentinel).all())


def _ref_feather(plan, tiles_by_class, C, up):
    """scene += w * tile in tile order, f32, w = wy * wx rounded once (torch on the host)"""
    ref = torch.zeros(C, plan.H * up, plan.W * up)
    for idx, tiles in tiles_by_class:
        for n, i in enumerate(idx):
            t = plan.tiles[i]
            sy0, sy1, sx0, sx1 = t.support
            part = tiles[n, :, (sy0 - t.y0) * up:(sy1 - t.y0) * up, (sx0 - t.x0) * up:(sx1 - t.x0) * up]
            ref[:, sy0 * up:sy1 * up, sx0 * up:sx1 * up] += plan.weights(t, up)[None] * part
    return ref


@pytest.mark.parametrize("up", [1, 2, 4])
@pytest.mark.parametrize("hw", SCENES)
def test_feather_scatter(infer, hw, up):
    """All-ones tiles blend to 1 within 1e-6; random tiles equal the torch re-implementation within 1e-6 * max|ref| (a fused
    multiply-add saves one rounding per addition, at most 4 additions per pixel); two runs give the same bits; guard rows untouched."""
    H, W = hw
    C = 2
    for tile, halo, multiple in [(16, 3, 1), (16, 3, 8), (16, 8, 8), (4, 0, 1)]:
        plan = infer.plan_tiles(H, W, tile, halo, multiple)
        runs = []
        for ones in (True, False, False):
            buf, dst = _guarded(C, H * up, W * up, 0.0)
            tiles_by_class = []
            for k, ((th, tw), idx) in enumerate(plan.classes.items()):
                tiles = _hr_tiles(plan, idx, C, up, seed=10 + k, ones=ones)
                tiles_by_class.append((idx, tiles))
                infer.tile_scatter(tiles.cuda(), dst, up, plan.rects(idx, True), True)
            got = dst.cpu()
            if ones:
                err = float((got - 1.0).abs().max())
                print(f"{hw} up {up} plan {(tile, halo, multiple)}: ones err {err:.3e}")
                assert err <= 1e-6
            else:
                ref = _ref_feather(plan, tiles_by_class, C, up)
                err = float((got - ref).abs().max() / ref.abs().max())
                print(f"{hw} up {up} plan {(tile, halo, multiple)}: random err {err:.3e}")
                assert err <= 1e-6
                runs.append(got)
            guard = buf.cpu()
            n = GUARD * W * up
            assert bool((guard[:n] == 0).all()) and bool((guard[-n:] == 0).all())
        assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("chw", [(3, 37, 53), (1, 37, 53), (3, 16, 24), (1, 64, 64), (4, 5, 7)])
def test_planes_to_u8hwc(infer, chw):
    C, H, W = chw
    g = torch.Generator().manual_seed(3)
    v = torch.rand(C, H, W, generator=g) * 1.5 - 0.25                  # negatives and values above 1
    k = torch.randint(0, 256, (C, H, W), generator=g).float() / 255.0   # exact k / 255 as f32 division gives them
    v = torch.where(torch.rand(C, H, W, generator=g) < 0.4, k, v)
    v.view(-1)[:6] = torch.tensor([0.0, 1.0, -0.0, 2.0, -3.0, 254.999 / 255.0])[:min(6, v.numel())]
    got = infer.planes_to_u8hwc(v.cuda()).cpu()
    ref = v.clamp(0, 1).mul(255).floor().to(torch.uint8).permute(1, 2, 0).contiguous()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, C)
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ end to end
def _nets(name, dtype="fp32"):
    from srcgan_amd import ESPCN, SRCNN, RDDBNet, RDDBNetB
    torch.manual_seed(21)
    if name == "rddbnet":
        sd = oracle.rddbnet_state(3, 3, 4, 16, 1, 16, seed=11)
        net = RDDBNet(3, 3, 4, nf=16, nb=1, gc=16, dtype=dtype)
        net.load_state_dict(sd)
        return net.cuda(), 3, 4, sd
    if name == "rddbnetb":
        return RDDBNetB(3, 3, 16, nb=1, gc=16, mode="x2", dtype=dtype).cuda(), 3, 2, None
    if name == "espcn":
        return ESPCN(1, 1, 2, dtype=dtype).cuda(), 1, 2, None
    return SRCNN(1, 1, 2, dtype=dtype).cuda(), 1, 1, None


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", ["rddbnet", "rddbnetb", "espcn", "srcnn"])
def test_exact_mode_equals_whole_image_fp32(infer, name, batch):
    """``upscale_scene`` (tile 16, halo = receptive radius, crop) against the same module's whole-image ``no_grad`` forward; gate: the
    project's fp32 gate rel_err < 1e-3.  Observed on an MI355X: see the printed value (not yet measured when this was written)."""
    net, in_ch, up, sd = _nets(name)
    x = torch.rand(1, in_ch, 45, 70, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        whole = net.eval()(x.cuda()).cpu()
    got = infer.upscale_scene(net, x.cuda(), up=up, tile=16, batch=batch).cpu()
    assert got.shape == whole.shape == (1, whole.shape[1], 45 * up, 70 * up)
    err = rel_err(got, whole)
    print(f"{name} batch {batch}: tiled vs whole-image rel_err {err:.3e}")
    assert err < 1e-3
    if sd is not None:
        ref = oracle.rddbnet_forward(sd, x, up)
        err_o = rel_err(got, ref)
        print(f"{name} batch {batch}: tiled vs oracle rel_err {err_o:.3e}")
        assert err_o < 1e-3


def test_exact_mode_bf16(infer):
    """The RDDBNet case in bf16, tiled against whole-image bf16; gate: rel_l2 < 2e-2, the bf16 gate of test_gpu_fullsize.py.
    Observed on an MI355X: see the printed value (not yet measured when this was written)."""
    net, in_ch, up, _ = _nets("rddbnet", dtype="bf16")
    x = torch.rand(1, in_ch, 45, 70, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        whole = net.eval()(x.cuda()).cpu()
    got = infer.upscale_scene(net, x.cuda(), up=up, tile=16, batch=3).cpu()
    err = rel_l2(got, whole)
    print(f"rddbnet bf16: tiled vs whole-image rel_l2 {err:.3e}")
    assert err < 2e-2


def test_exact_mode_refuses_what_would_not_be_exact(infer):
    from srcgan_amd import ESPCN, ResDeconv
    sr = ESPCN(1, 1, 2).cuda()
    x = torch.rand(1, 1, 40, 56, device="cuda")
    with pytest.raises(ValueError, match="normalisation"):
        infer.upscale_scene([sr, ResDeconv(1, 3).cuda()], x, up=2, tile=16)
    with pytest.raises(ValueError, match="would not be exact"):
        infer.upscale_scene(sr, x, up=2, tile=16, multiple=16)          # 40 = 16 + 16 + 8: the last tile passes the bottom edge
    with pytest.raises(ValueError, match="up = 4"):
        infer.upscale_scene(sr, x, up=4, tile=16)


def test_cascade_feather_mode(infer):
    """[ESPCN(1,1,2), ResDeconv(1,3)] on a 40x56 gray u8 scene, tile 16, halo 8, multiple 8 (HR tiles: multiples of 16), u8 output,
    against a re-implementation of the same plan: slice, pad with replication, the same native modules per tile, blend in torch in
    tile order.  Allowance: at most 1 u8 step on at most 0.1 % of the values -- the floor of a value that the blend's rounding (fused
    multiply-add against multiply then add: <= 4 roundings of ~6e-8) moved across a k/255 boundary.  Checked on the host with random
    data before relying on it: torch's blend against the same blend with fma-style rounding (products and sums in float64, one
    rounding to f32 per addition) differed by one step on 12 of 5 376 000 values over 200 random trials of this plan, at worst 1 of
    26 880 values (3.7e-5) in one trial, never by more than one step: inside the 0.1 % allowance."""
    from srcgan_amd import ESPCN, ResDeconv
    torch.manual_seed(9)
    sr, col = ESPCN(1, 1, 2).cuda().eval(), ResDeconv(1, 3).cuda().eval()
    H, W, up = 40, 56, 2
    u8 = torch.randint(0, 256, (H, W, 1), dtype=torch.uint8, generator=torch.Generator().manual_seed(6))
    got = infer.upscale_scene([sr, col], u8.cuda(), up=up, tile=16, halo=8, multiple=8, batch=2, blend="feather", out="u8").cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (80, 112, 3)
    again = infer.upscale_scene([sr, col], u8.cuda(), up=up, tile=16, halo=8, multiple=8, batch=2, blend="feather", out="u8").cpu()
    assert torch.equal(got, again)
    plan = infer.plan_tiles(H, W, 16, 8, 8)
    planes = (u8.double() / 255.0).float().permute(2, 0, 1).contiguous()
    ref = torch.zeros(3, H * up, W * up)
    with torch.no_grad():
        for (th, tw), idx in plan.classes.items():
            for b0 in range(0, len(idx), 2):                                   # the same batches: GroupNorm is per image, batching is not
                ids = idx[b0:b0 + 2]
                xb = torch.stack([_ref_tile(planes, plan.tiles[i]) for i in ids]).cuda()
                yb = col(sr(xb)).cpu()
                for n, i in enumerate(ids):
                    t = plan.tiles[i]
                    sy0, sy1, sx0, sx1 = t.support
                    part = yb[n, :, (sy0 - t.y0) * up:(sy1 - t.y0) * up, (sx0 - t.x0) * up:(sx1 - t.x0) * up]
                    ref[:, sy0 * up:sy1 * up, sx0 * up:sx1 * up] += plan.weights(t, up)[None] * part
    ref8 = ref.clamp(0, 1).mul(255).floor().to(torch.uint8).permute(1, 2, 0)
    diff = (got.int() - ref8.int()).abs()
    share = float((diff > 0).float().mean())
    print(f"cascade: max u8 step {int(diff.max())}, share of differing values {share:.2e}")
    assert int(diff.max()) <= 1
    assert share <= 1e-3
