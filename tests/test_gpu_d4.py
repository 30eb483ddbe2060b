"""GPU: the geometric self-ensemble of the scene drivers (``ensemble=``).  The view gather and the fold are compared BIT FOR BIT with
torch's flips and transpositions of what the plain gather returns (tests/d4_ref.py, tied to the index mapping by
tests/test_d4_host.py); the drivers bit for bit with a torch re-implementation of the same plan in crop mode, within the existing
allowance in feather mode, within the fp32 gate with the whole-image ensemble, and -- independently of any re-implementation -- with
themselves on a network made equivariant.  Shapes are small: more than one 32 x 32 LDS block per axis, extents that are no multiple
of 32 or of 4, th != tw, odd origins, tiles past the edge, more origins than one launch carries."""
import pytest
import torch
import torch.nn.functional as F

import d4_ref as R
import oracle
from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import data, infer
    return infer, data


# ------------------------------------------------------------------------------------------------ 1. the view gather
KINDS = ["f32c1", "f32c3", "u8c1", "u8c3", "u8gray"]
TILE_SHAPES = [(24, 24), (16, 40), (33, 65)]            # one block; two blocks along W, 16-byte stores; ragged blocks, scalar stores


def _scene(kind, H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    if kind.startswith("f32"):
        return (torch.rand(1, int(kind[-1]), H, W, generator=g) * 2 - 0.5).cuda(), "f32"
    u8 = torch.randint(0, 256, (H, W, 1 if kind == "u8c1" else 3), dtype=torch.uint8, generator=g).cuda()
    return u8, "u8rgb2gray" if kind == "u8gray" else "u8"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hw", [(37, 53), (70, 96)])
def test_gather_d4_equals_the_transformed_gather_bit_exact(mods, hw, kind):
    infer, _ = mods
    H, W = hw
    scene, k = _scene(kind, H, W)
    for s in (1, 2):
        OH, OW = H * s, W * s
        for th, tw in TILE_SHAPES:
            origins = [(0, 0), (3, 5), (max(OH - th, 0), max(OW - tw, 0) | 1), (OH - 5, OW - 7)]   # odd x0; the last two pass the edge
            win = infer.tile_gather_ex(scene, k, s, origins, th, tw)
            for op in range(8):
                got = infer.tile_gather_d4(scene, k, s, origins, th, tw, op)
                ref = R.torch_view(win, op)
                assert tuple(got.shape) == (4, win.shape[1], *R.view_shape(op, th, tw)) == tuple(ref.shape)
                assert torch.equal(got, ref), (hw, kind, s, th, tw, op)
            assert torch.equal(infer.tile_gather_d4(scene, k, s, origins, th, tw, 0), win)


def test_gather_d4_chunks_its_origins(mods):
    infer, _ = mods
    for kind, s in (("f32c3", 1), ("u8gray", 2)):
        scene, k = _scene(kind, 70, 96)
        many = [((7 * i) % (70 * s), (11 * i) % (96 * s)) for i in range(140)]     # more than one launch carries
        win = infer.tile_gather_ex(scene, k, s, many, 16, 40)
        for op in range(8):
            assert torch.equal(infer.tile_gather_d4(scene, k, s, many, 16, 40, op), R.torch_view(win, op)), (kind, op)


def test_wrappers_refuse_bad_arguments(mods):
    infer, _ = mods
    u8 = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="op = 8"):
        infer.tile_gather_d4(u8, "u8", 1, [(0, 0)], 4, 4, 8)
    with pytest.raises(RuntimeError, match="outside"):
        infer.tile_gather_d4(u8, "u8rgb2gray", 2, [(16, 0)], 4, 4, 1)
    with pytest.raises(ValueError, match="kind"):
        infer.tile_gather_d4(u8, "rgb", 1, [(0, 0)], 4, 4, 1)
    with pytest.raises(TypeError, match="takes float32"):
        infer.tile_gather_d4(u8, "f32", 1, [(0, 0)], 4, 4, 1)
    v, acc = torch.zeros(1, 2, 4, 6, device="cuda"), torch.zeros(1, 2, 6, 4, device="cuda")
    with pytest.raises(ValueError, match="does not fold"):
        infer.d4_accumulate(v, acc, 0, True, 1.0)
    with pytest.raises(RuntimeError, match="op = 9"):
        infer.d4_accumulate(v, acc, 9, True, 1.0)
    with pytest.raises(RuntimeError, match="alias"):
        infer.d4_accumulate(v, v, 0, False, 1.0)
    with pytest.raises(TypeError, match="contiguous float32"):
        infer.d4_accumulate(v.double(), acc, 1, True, 1.0)


# ------------------------------------------------------------------------------------------------ 2. the fold
GUARD = 64                                                # floats around the accumulator


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("ahw", [(24, 24), (32, 80), (66, 130)])
def test_fold_equals_the_sequential_f32_average_bit_exact(mods, ahw, shift):
    """The accumulator lies between sentinels; ``shift`` moves it off 16-byte alignment (scalar path, the same bits)."""
    infer, _ = mods
    ah, aw = ahw
    T, C = 2, 3
    n = T * C * ah * aw
    g = torch.Generator().manual_seed(ah + aw)
    for V, ops in R.OPS.items():
        if V == 1:
            continue
        views = [((torch.rand(T, C, *R.view_shape(op, ah, aw), generator=g) - 0.5) * 1000.0).cuda() for op in ops]
        ref = R.torch_average([R.torch_fold(v, op) for v, op in zip(views, ops)])
        runs = []
        for _ in range(2):
            buf = torch.full((n + 2 * GUARD + 4,), -7.25, device="cuda")          # `first` must not read what is there
            acc = buf[GUARD + shift:GUARD + shift + n].view(T, C, ah, aw)
            assert acc.data_ptr() % 16 == 4 * shift
            for k, (v, op) in enumerate(zip(views, ops)):
                infer.d4_accumulate(v, acc, op, k == 0, 1.0 / V if k == V - 1 else 1.0)
            assert torch.equal(acc, ref), (ahw, shift, V)
            host = buf.cpu()
            assert bool((host[:GUARD + shift] == -7.25).all()) and bool((host[GUARD + shift + n:] == -7.25).all())
            runs.append(acc.clone())
        assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------ 3-8. the drivers
def _ref_tile(planes, y0, x0, th, tw):
    """torch slicing of f32 [C,H,W]; what passes the right / bottom edge is edge replication"""
    _, H, W = planes.shape
    y1, x1 = min(y0 + th, H), min(x0 + tw, W)
    return F.pad(planes[None, :, y0:y1, x0:x1], (0, x0 + tw - x1, 0, y0 + th - y1), mode="replicate")[0]


def _ref_ensemble(infer, plan, planes, chain, ensemble, batch, up, feather=False):
    """The same plan in torch: the same tile batches (sliced from the f32 ``planes`` [C,H,W]), torch flips and transpositions, the
    same native modules per view (``chain(x)`` -> the tensors written back), a sequential f32 sum, x 1 / V, then the crop (or the
    feathered blend in tile order, on the host).  -> f32 [planes written, H*up, W*up]."""
    ops, out = R.OPS[ensemble], None
    with torch.no_grad():
        for (th, tw), idx in plan.classes.items():
            for b0 in range(0, len(idx), batch):
                ids = idx[b0:b0 + batch]
                x = torch.stack([_ref_tile(planes, plan.tiles[i].y0, plan.tiles[i].x0, th, tw) for i in ids]).cuda()
                per_view = [[R.torch_fold(t.contiguous().float(), op) for t in chain(R.torch_view(x, op))] for op in ops]
                y = torch.cat([R.torch_average([pv[j] for pv in per_view]) if ensemble > 1 else per_view[0][j]
                               for j in range(len(per_view[0]))], 1).cpu()
                if out is None:
                    out = torch.zeros(y.shape[1], plan.H * up, plan.W * up)
                for n, i in enumerate(ids):
                    t = plan.tiles[i]
                    sy0, sy1, sx0, sx1 = t.support if feather else t.core
                    part = y[n, :, (sy0 - t.y0) * up:(sy1 - t.y0) * up, (sx0 - t.x0) * up:(sx1 - t.x0) * up]
                    if feather:
                        out[:, sy0 * up:sy1 * up, sx0 * up:sx1 * up] += plan.weights(t, up)[None] * part
                    else:
                        out[:, sy0 * up:sy1 * up, sx0 * up:sx1 * up] = part
    return out


@pytest.fixture(scope="module")
def rddb(mods):
    """RDDBNet(3,3,4,nf=16,nb=1,gc=16) fp32 on a 45x70 scene, tile 16, exact mode, batch 3: the network, the scene and the
    ``ensemble=8`` result, computed once."""
    infer, _ = mods
    from srcgan_amd import RDDBNet
    sd = oracle.rddbnet_state(3, 3, 4, 16, 1, 16, seed=11)
    net = RDDBNet(3, 3, 4, nf=16, nb=1, gc=16)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    x = torch.rand(1, 3, 45, 70, generator=torch.Generator().manual_seed(4)).cuda()
    got = infer.upscale_scene(net, x, up=4, tile=16, batch=3, ensemble=8, out="f32")
    return net, x, sd, got


def test_upscale_scene_rddbnet_ensemble8_equals_the_plan_in_torch(mods, rddb):
    infer, _ = mods
    net, x, _, got = rddb
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 180, 280)
    plan = infer.plan_tiles(45, 70, 16, infer.receptive_halo(net))
    assert any(th != tw for th, tw in plan.classes)                              # transposed views do change the batch shape
    ref = _ref_ensemble(infer, plan, x[0].cpu(), lambda v: [net(v)], 8, 3, 4)
    assert torch.equal(got[0].cpu(), ref)


@pytest.mark.parametrize("ensemble", [2, 4])
def test_upscale_scene_espcn_equals_the_plan_in_torch(mods, ensemble):
    infer, _ = mods
    from srcgan_amd import ESPCN
    torch.manual_seed(21)
    net = ESPCN(1, 1, 2).cuda().eval()
    x = torch.rand(1, 1, 45, 70, generator=torch.Generator().manual_seed(5)).cuda()
    got = infer.upscale_scene(net, x, up=2, tile=16, batch=2, ensemble=ensemble)
    ref = _ref_ensemble(infer, infer.plan_tiles(45, 70, 16, 6), x[0].cpu(), lambda v: [net(v)], ensemble, 2, 2)
    assert tuple(got.shape) == (1, 1, 90, 140) and torch.equal(got[0].cpu(), ref)


@pytest.fixture(scope="module")
def cascade(mods):
    """[ESPCN(1,1,2), ResDeconv(1,3)] (and a ResDeconv(1,2) for LAB) on a 40x56 gray u8 scene: tile 16, halo 8, multiple 8 (HR tiles:
    multiples of 16), batch 2 -- the plan of test_cascade_feather_mode."""
    from srcgan_amd import ESPCN, ResDeconv
    torch.manual_seed(9)
    sr, col, col_ab = ESPCN(1, 1, 2).cuda().eval(), ResDeconv(1, 3).cuda().eval(), ResDeconv(1, 2).cuda().eval()
    u8 = torch.randint(0, 256, (40, 56, 1), dtype=torch.uint8, generator=torch.Generator().manual_seed(6))
    planes = (u8.double() / 255.0).float().permute(2, 0, 1).contiguous()
    return sr, col, col_ab, u8.cuda(), planes, dict(up=2, tile=16, halo=8, multiple=8, batch=2)


def test_cascade_scene_ensemble8_equals_the_plan_in_torch(mods, cascade):
    infer, _ = mods
    sr, col, col_ab, u8, planes, kw = cascade
    plan = infer.plan_tiles(40, 56, 16, 8, 8)
    assert any(th != tw for th, tw in plan.classes)
    got = infer.cascade_scene(sr, col, u8, blend="crop", ensemble=8, out="f32", **kw)
    ref = _ref_ensemble(infer, plan, planes, lambda v: [col(sr(v))], 8, 2, 2)
    assert tuple(got.shape) == (1, 3, 80, 112) and torch.equal(got[0].cpu(), ref)
    lab = infer.cascade_scene(sr, col_ab, u8, space="lab", blend="crop", ensemble=8, out="f32", **kw)

    def both(v):
        l = sr(v)
        return [l, col_ab(l)]
    assert torch.equal(lab[0].cpu(), _ref_ensemble(infer, plan, planes, both, 8, 2, 2))      # L and ab are folded and averaged alike


@pytest.mark.parametrize("space", ["rgb", "lab"])
def test_cascade_u8_output_is_the_converted_f32_ensemble(mods, cascade, space):
    """The average is taken before the 8-bit conversion (and before lab2img): the fused u8 write-back of the averaged tiles equals
    the project's own conversion of the ``out="f32"`` ensemble result, the comparison test_gpu_cascade_scene.py makes at ensemble=1."""
    infer, data = mods
    sr, col, col_ab, u8, planes, kw = cascade
    c = col_ab if space == "lab" else col
    f32 = infer.cascade_scene(sr, c, u8, space=space, blend="crop", ensemble=8, out="f32", **kw)
    got = infer.cascade_scene(sr, c, u8, space=space, blend="crop", ensemble=8, out="u8", **kw)
    ref = data.lab2img(f32[0]) if space == "lab" else infer.planes_to_u8hwc(f32)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (80, 112, 3) and torch.equal(got, ref)


def test_cascade_feather_mode_ensemble4(mods, cascade):
    """Feathered, u8, ``ensemble=4``: reproducible bit for bit, and within the allowance of test_cascade_feather_mode (at most 1 u8
    step on at most 0.1 % of the values, checked on the host there for the blend's fma-against-multiply-add rounding) of the plan in
    torch; the allowance carries over because the averaged tile that enters the blend is bit-identical to the reference's.
    Observed on an MI355X: no differing value."""
    infer, _ = mods
    sr, col, col_ab, u8, planes, kw = cascade
    got = infer.cascade_scene(sr, col, u8, blend="feather", out="u8", ensemble=4, **kw)
    again = infer.cascade_scene(sr, col, u8, blend="feather", out="u8", ensemble=4, **kw)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (80, 112, 3) and torch.equal(got, again)
    ref = _ref_ensemble(infer, infer.plan_tiles(40, 56, 16, 8, 8), planes, lambda v: [col(sr(v))], 4, 2, 2, feather=True)
    ref8 = ref.clamp(0, 1).mul(255).floor().to(torch.uint8).permute(1, 2, 0)
    diff = (got.cpu().int() - ref8.int()).abs()
    share = float((diff > 0).float().mean())
    print(f"cascade ensemble 4: max u8 step {int(diff.max())}, share of differing values {share:.2e}")
    assert int(diff.max()) <= 1
    assert share <= 1e-3


def _whole_ensemble(net, x, ensemble):
    with torch.no_grad():
        outs = [R.torch_fold(net(R.torch_view(x, op)).float(), op).double() for op in R.OPS[ensemble]]
    return (sum(outs) / len(outs)).cpu()


def test_exact_mode_equals_the_whole_image_ensemble_fp32(mods, rddb):
    """Tiled ``ensemble=8`` against the mean over g of g^-1(net(g(x))) on the whole image; gate: the project's fp32 gate rel_err < 1e-3
    (test_exact_mode_equals_whole_image_fp32).  Observed on an MI355X: 1.2e-7 (the value is printed)."""
    net, x, _, got = rddb
    err = rel_err(got, _whole_ensemble(net, x, 8))
    print(f"rddbnet ensemble 8: tiled vs whole-image ensemble rel_err {err:.3e}")
    assert err < 1e-3


def test_an_equivariant_network_is_its_own_ensemble(mods, rddb):
    """Every 3x3 kernel replaced by its mean over its eight transforms and every k2 s2 transposed-convolution kernel by its mean over
    its four taps: the network commutes with D4, so every folded view is the plain output up to fp32 rounding and ``ensemble=8``
    agrees with ``ensemble=1`` at the fp32 gate rel_err < 1e-3 -- which a fold with a wrong orientation would miss by the size of the
    signal.  Pins the fold without the torch re-implementation.  Observed on an MI355X: 6.2e-7 (the value is printed)."""
    infer, _ = mods
    from srcgan_amd import RDDBNet
    _, x, sd, _ = rddb
    sym = {}
    for k, w in sd.items():
        w = w.clone()
        if w.dim() == 4 and tuple(w.shape[-2:]) == (3, 3):
            w = sum(R.torch_view(w, op) for op in range(8)) / 8.0
        elif w.dim() == 4 and tuple(w.shape[-2:]) == (2, 2):
            w = w.mean((-2, -1), keepdim=True).expand_as(w).contiguous()
        sym[k] = w
    net = RDDBNet(3, 3, 4, nf=16, nb=1, gc=16)
    net.load_state_dict(sym)
    net = net.cuda().eval()
    one = infer.upscale_scene(net, x, up=4, tile=16, batch=3, ensemble=1)
    eight = infer.upscale_scene(net, x, up=4, tile=16, batch=3, ensemble=8)
    err = rel_err(eight, one)
    print(f"equivariant rddbnet: ensemble 8 vs ensemble 1 rel_err {err:.3e}")
    assert err < 1e-3
    assert rel_err(one.flip(-1), one) > 0.1                                      # the output is no symmetric image: the gate can tell


def test_ensemble_1_is_the_call_without_the_argument(mods, rddb, cascade):
    infer, _ = mods
    net, x, _, _ = rddb
    assert torch.equal(infer.upscale_scene(net, x, up=4, tile=16, batch=3, ensemble=1), infer.upscale_scene(net, x, up=4, tile=16, batch=3))
    sr, col, col_ab, u8, planes, kw = cascade
    for extra in (dict(blend="crop", out="u8"), dict(blend="feather", out="f32"), dict(space="lab", blend="crop", out="u8")):
        c = col_ab if extra.get("space") == "lab" else col
        assert torch.equal(infer.cascade_scene(sr, c, u8, ensemble=1, **extra, **kw), infer.cascade_scene(sr, c, u8, **extra, **kw)), extra


def test_memory_follows_the_tile_batch_under_the_ensemble(mods):
    """As test_gpu_cascade_scene.py::test_memory_follows_the_tile_batch, with ``ensemble=8``: crop / u8, SRCNN networks, const, x2, LR
    colour scenes of 256x256 and 512x512 (tile 64, halo 8 on the up-sampled grid: both plans hold the same tile classes, and a class
    and its transpose are both among them or both run in both).  Nothing but the input scene and the u8 result may scale with the
    scene: peak(big) - peak(small) <= delta(input bytes + output bytes) + 1 MiB, the 1 MiB for allocator rounding only.  Eight
    scene-sized f32 results, or one, would break it: a single f32 [3,1024,1024] image grows by 9 MiB between the two scenes."""
    infer, _ = mods
    from srcgan_amd import SRCNN
    torch.manual_seed(31)
    sr, col = SRCNN(1, 1, 1, 16).cuda().eval(), SRCNN(1, 2, 1, 16).cuda().eval()
    kw = dict(up=2, space="lab", const=True, tile=64, halo=8, batch=4, blend="crop", out="u8", ensemble=8)
    sizes = [(256, 256), (512, 512)]
    plans = [infer._cascade_plan(sr, col, h, w, up=2, const=True, tile=64, halo=8, multiple=1) for h, w in sizes]
    assert set(plans[0].classes) == set(plans[1].classes) and len(plans[1].tiles) > len(plans[0].tiles)
    warm = torch.randint(0, 256, (*sizes[0], 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    infer.cascade_scene(sr, col, warm, **kw)                                   # whatever the modules cache exists before measuring
    del warm
    peaks, io = [], []
    for h, w in sizes:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        scene = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
        res = infer.cascade_scene(sr, col, scene, **kw)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        io.append(scene.numel() + res.numel())
        assert tuple(res.shape) == (2 * h, 2 * w, 3) and res.dtype == torch.uint8
        del scene, res
    d_peak, d_io = peaks[1] - peaks[0], io[1] - io[0]
    print(f"ensemble 8: peak above the baseline: {peaks[0]} B, {peaks[1]} B; delta {d_peak} B; delta(input + output) {d_io} B")
    assert d_peak <= d_io + (1 << 20)
