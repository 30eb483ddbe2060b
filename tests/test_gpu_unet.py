"""GPU: the native UnetGenerator against the two reference fixtures (fp32, 1e-3 ``rel_err``, the project's fp32 gate, on y, loss, dx and
every live gradient), against our float64 restatement at ngf = 64 (512-channel levels, 1024-channel skip buffers), at seven levels on
128 x 128 (``unet_128``'s graph) and on a batch of wide three-channel images, in the 16-bit modes against the storage emulation, its no_grad
path, and whole-scene inference through upscale_scene and cascade_scene.

Dead biases.  Every bias in front of an InstanceNorm (all but the first and last down convolution's and the last transposed one's) has a
gradient that is zero in exact arithmetic, so it is held in the absolute measure unet_ref.dead_ratio = max|g_b| / max|g_w| of its layer:
fp32 at 1e-3 (the fp32 gate in absolute form; the reference's own float32 run sits at 3e-6 on these fixtures), the 16-bit modes at 1.5 x the
emulation's own ratio + 5e-3.  Observed values are printed (pytest -s)."""
import functools

import pytest
import torch
import torch.nn as nn

import unet_ref as R
from conftest import load_golden, rel_err
from net_checks import F32_TOL, STORE, bound16, check_16bit, check_fp32, check_no_grad_bits, check_one_tile_scene, step
from test_unet_ref import FIXTURES, native

pytestmark = pytest.mark.gpu
IN = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)


def report(who, e, dead):
    worst = sorted(((v, k) for k, v in e.items() if k.startswith("grad ")), reverse=True)
    kd = max(dead, key=dead.get) if dead else None
    print(f"[unet] {who}: y {e['y']:.2e} loss {e['loss']:.2e} dx {e['dx']:.2e} worst live grads {[(f'{v:.2e}', k[5:]) for v, k in worst[:3]]} "
          f"worst dead-bias ratio {dead[kd] if dead else 0.0:.2e} ({kd})")
    return worst


@pytest.mark.parametrize("tag", FIXTURES)
def test_fp32_against_the_reference_fixture(tag):
    z = load_golden(tag)
    m = native(z).cuda()
    assert list(m.state_dict().keys()) == [str(n) for n in z["names"]]
    y, loss, dx, g = step(m, torch.from_numpy(z["x"]), torch.from_numpy(z["t"]))
    assert tuple(y.shape) == tuple(z["y"].shape) and list(g) == [str(n) for n in z["names"]]
    e, dead = R.fixture_errors(z, y, loss, dx, g, "", measure=rel_err)
    worst = report(f"{tag} fp32 vs reference", e, dead)
    assert e["y"] < F32_TOL and e["loss"] < F32_TOL and e["dx"] < F32_TOL
    assert worst[0][0] < F32_TOL, worst[:3]
    assert sorted(dead) == sorted(R.dead_biases(int(z["cfg"][3]))) and max(dead.values()) <= 1e-3, dead
    assert all(torch.isfinite(v).all() for v in g.values())


def _case(cin, cout, shape, dtype, seed, n=5, ngf=16):
    import srcgan_amd
    torch.manual_seed(seed)
    m = srcgan_amd.UnetGenerator(cin, cout, n, ngf, norm_layer=IN, dtype=dtype)        # torch's default initialisation: no bias is zero
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(*shape, generator=g)
    t = torch.rand(shape[0], cout, *shape[2:], generator=g) * 2 - 1
    return m.cuda(), x, t


def dead_ratios(g, n):
    return {k: R.dead_ratio(g, k) for k in R.dead_biases(n)}


# ngf 64 at five levels: 512-channel levels, 1024-channel skip buffers, several K chunks, a 1 x 1 bottleneck; seven levels at ngf 16 on
# 128 x 128: unet_128's graph, three 128-channel levels of 4 x 4 and below; (2, 3, 32, 96): a batch, three colours in, 1 x 3 at the bottom
@pytest.mark.parametrize("cin, cout, shape, n, ngf", [(1, 1, (1, 1, 32, 32), 5, 64), (1, 3, (1, 1, 128, 128), 7, 16), (3, 2, (2, 3, 32, 96), 5, 16)])
def test_fp32_against_the_float64_restatement(cin, cout, shape, n, ngf):
    m, x, t = _case(cin, cout, shape, "fp32", 3, n=n, ngf=ngf)
    got = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    assert list(sd) == R.names(n)
    dead = dead_ratios(got[3], n)
    check_fp32("unet", f"{shape} d{n} ngf{ngf}", got, R.run(sd, x, t, n), names="list", skip=tuple(dead),
               tail=f" worst dead-bias ratio {max(dead.values()):.2e}")
    assert max(dead.values()) <= 1e-3, dead


_REF16 = {}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_modes_against_the_storage_emulation(dtype):
    """net_checks.bound16 on the live tensors, with its static loss scale of 1024; the dead biases in the same form on their absolute
    measure, against a yardstick of their own.

    A dead bias's gradient is the sum over the pixels of a gradient tensor the native backward stores in the 16-bit type; in exact
    arithmetic the sum is zero, and what is left is the rounding of that storage -- about 2^-9 (bf16) of the tensor's size, which at the
    16- and 32-channel levels is several 1e-3 of the layer's largest weight gradient.  The forward-only emulation leaves 1e-15 there: it
    compares unlike things.  So the yardstick is the emulation that also rounds those gradient tensors (unet_ref.run(round_grads=True);
    its figures on the CPU for this case: bf16 7.1e-3, fp16 1.2e-3, the same biases worst), in bound16's form."""
    n, shape, scale_loss = 5, (2, 1, 32, 64), 1024.0
    m, x, t = _case(1, 3, shape, dtype, 5)
    got = step(m, x, t, scale_loss)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    if "ref" not in _REF16:          # the float64 run is the same for both 16-bit types (same seed, same weights)
        _REF16["ref"] = R.run(sd, x, t, n, loss_scale=scale_loss)
    emu = R.run(sd, x, t, n, store=STORE[dtype], loss_scale=scale_loss)
    emu_g = R.run(sd, x, t, n, store=STORE[dtype], loss_scale=scale_loss, round_grads=True)
    dnat, demu = dead_ratios(got[3], n), dead_ratios(emu_g[3], n)
    check_16bit("unet", "", dtype, got, _REF16["ref"], emu, names="list", skip=tuple(dnat),
                tails=tuple(f" worst dead-bias ratio {max(d.values()):.2e}" for d in (dnat, demu)))
    assert max(dnat.values()) <= bound16(max(demu.values())), (dnat, demu)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_no_grad_path_has_the_bits_of_the_training_forward(dtype):
    m, x, _ = _case(1, 3, (2, 1, 32, 64), dtype, 7)
    y = check_no_grad_bits(m, x)
    assert tuple(y.shape) == (2, 3, 32, 64) and float(y.detach().abs().max()) <= 1.0


def test_the_input_gradient_is_optional_and_changes_nothing():
    """without requires_grad on x the first layer's input gradient is skipped; the parameter gradients keep their bits"""
    m, x, t = _case(3, 1, (1, 3, 32, 32), "fp32", 11)
    _, _, _, g = step(m, x, t)
    for p in m.parameters():
        p.grad = None
    torch.nn.functional.l1_loss(m(x.cuda()), t.cuda()).backward()
    assert all(torch.equal(p.grad.cpu(), g[k]) for k, p in m.named_parameters())


def test_upscale_scene_on_one_tile_equals_the_forward():
    from srcgan_amd import infer
    m, _, _ = _case(3, 3, (1, 3, 32, 32), "bf16", 9)
    scene = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(10)).cuda()
    check_one_tile_scene(m, scene, 1, (1, 3, 32, 32))
    with pytest.raises(ValueError, match=r"up = 2"):
        infer.upscale_scene(m, scene, up=2, tile=32, halo=8, blend="feather")
    with pytest.raises(ValueError, match="per-image statistics make tiles inexact"):          # exact mode: halo=None
        infer.upscale_scene(m, scene, up=1, tile=32)


def test_feathered_tiles_equal_the_same_plan_stitched_in_torch():
    """two tiles of different widths, every extent a multiple of 2^num_downs = 32 (``multiple=32`` with halo 32): the module's own no_grad
    outputs on the plan's tiles, blended with the plan's weights in torch, within the feather scatter's 1e-6 of max|ref|
    (tests/test_gpu_infer_scene.py); a plan with an extent that is no multiple reaches the user as the planner's refusal"""
    from srcgan_amd import infer
    m, _, _ = _case(1, 3, (1, 1, 32, 32), "bf16", 15)
    scene = torch.rand(1, 1, 32, 96, generator=torch.Generator().manual_seed(16)).cuda()
    plan = infer.plan_tiles(32, 96, 64, 32, 32)
    assert len(plan.tiles) == 2 and all(t.th % 32 == 0 and t.tw % 32 == 0 for t in plan.tiles) and len({t.tw for t in plan.tiles}) == 2
    got = infer.upscale_scene(m, scene, up=1, tile=64, halo=32, blend="feather", multiple=32)
    ref = torch.zeros(3, 32, 96)
    with torch.no_grad():
        for t in plan.tiles:
            y = m(scene[:, :, t.y0:t.y0 + t.th, t.x0:t.x0 + t.tw])[0].cpu()
            sy0, sy1, sx0, sx1 = t.support
            ref[:, sy0:sy1, sx0:sx1] += plan.weights(t, 1)[None] * y[:, sy0 - t.y0:sy1 - t.y0, sx0 - t.x0:sx1 - t.x0]
    err = float((got[0].cpu() - ref).abs().max() / ref.abs().max())
    print(f"[unet] feathered two-tile scene vs the plan stitched in torch: {err:.2e}")
    assert tuple(got.shape) == (1, 3, 32, 96) and err <= 1e-6
    assert torch.equal(got, infer.upscale_scene(m, scene, up=1, tile=64, halo=32, blend="feather", multiple=32))
    with pytest.raises(Exception, match="multiples of 2\\^num_downs"):          # 48-pixel tiles
        infer.upscale_scene(m, scene, up=1, tile=16, halo=16, blend="feather", multiple=16)


def test_cascade_scene_accepts_the_network_as_colouriser():
    import srcgan_amd
    torch.manual_seed(12)
    sr = srcgan_amd.SRCNN(1, 1, 1, 32, dtype="bf16").cuda()
    col, _, _ = _case(1, 3, (1, 1, 32, 32), "bf16", 13)
    scene = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(14)).cuda()
    out = srcgan_amd.cascade_scene(sr, col, scene, up=1, tile=32, halo=8, blend="feather", out="f32")
    with torch.no_grad():
        want = col(sr(scene))
    assert tuple(out.shape) == (1, 3, 32, 32) and torch.isfinite(out).all() and torch.equal(out, want)
