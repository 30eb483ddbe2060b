"""GPU: the native DDBPN against the reference fixtures (fp32, 1e-3 ``rel_err`` as tests/test_gpu_modules.py uses), against our
float64 restatement at one further shape per scale, in the 16-bit modes against the storage emulation, its no_grad path, and whole-scene
inference through upscale_scene (one tile; exact mode on a 2 x 2-tile plan).  Observed values are printed (pytest -s).

The figures measured on an MI355X are in DESIGN 3.9."""
import pytest
import torch

import ddbpn_ref
from conftest import load_golden, rel_err, rel_l2
from ddbpn_ref import sketch

pytestmark = pytest.mark.gpu
F32_TOL = 1e-3
FIXTURES = ("ddbpn_x2", "ddbpn_x4", "ddbpn_x8")
STORE = {"bf16": torch.bfloat16, "fp16": torch.float16}


def step(m, x, t, loss_scale=1.0):
    """forward, L1 loss (times loss_scale), backward -> (y, loss, dx, {name: grad}) on the CPU"""
    for p in m.parameters():
        p.grad = None
    x = x.detach().cuda().requires_grad_(True)
    y = m(x)
    loss = torch.nn.functional.l1_loss(y, t.cuda()) * loss_scale
    loss.backward()
    return y.detach().cpu(), float(loss.detach()), x.grad.cpu(), {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("tag", FIXTURES)
def test_fp32_against_the_reference_fixture(tag):
    import srcgan_amd
    z = load_golden(tag)
    torch.manual_seed(int(z["seed"]))
    m = srcgan_amd.DDBPN(scale=int(z["scale"]), rgb_range=1)
    ddbpn_ref.set_slopes(m, int(z["seed"]))
    m = m.cuda()
    assert list(m.state_dict().keys()) == [str(n) for n in z["names"]]
    y, loss, dx, g = step(m, torch.from_numpy(z["x"]), torch.from_numpy(z["t"]))
    frozen = [str(n) for n in z["frozen"]]
    assert all(m.get_parameter(k).grad is None and not m.get_parameter(k).requires_grad for k in frozen) and len(frozen) == 4
    assert set(g) == {k for k in map(str, z["names"]) if k not in frozen}
    errs = []
    for k, v in g.items():
        if "grad/" + k in z:
            errs.append((rel_err(v, z["grad/" + k]), k))
        else:       # a large tensor: its sketch (whose relative error estimates the tensor's relative L2 error) and its first slice
            first = v[0] if v[0].numel() <= 256 else v[0, 0]
            errs.append((max(rel_err(sketch(v.numpy()), z["gsketch/" + k]), rel_err(first, z["gslice/" + k])), k))
    errs.sort(reverse=True)
    print(f"[ddbpn] {tag} fp32 vs reference: y {rel_err(y, z['y']):.2e} loss {abs(loss - float(z['loss'])) / float(z['loss']):.2e} "
          f"dx {rel_err(dx, z['dx']):.2e} worst grads {[(f'{e:.2e}', k) for e, k in errs[:3]]}")
    assert rel_err(y, z["y"]) < F32_TOL and abs(loss - float(z["loss"])) < F32_TOL * float(z["loss"]) and rel_err(dx, z["dx"]) < F32_TOL
    assert errs[0][0] < F32_TOL, errs[:3]


def _case(scale, shape, dtype, seed):
    import srcgan_amd
    torch.manual_seed(seed)
    m = srcgan_amd.DDBPN(scale=scale, rgb_range=1, dtype=dtype)
    ddbpn_ref.set_slopes(m, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(*shape, generator=g)
    t = torch.rand(shape[0], 3, shape[2] * scale, shape[3] * scale, generator=g)
    return m.cuda(), x, t


# a further shape per scale: more than one 32-pixel tile column at HR, odd sizes, and a batch the fixtures do not have
@pytest.mark.parametrize("scale, shape", [(2, (3, 3, 19, 9)), (4, (2, 3, 9, 11)), (8, (2, 3, 5, 3))])
def test_fp32_against_the_float64_restatement(scale, shape):
    m, x, t = _case(scale, shape, "fp32", 3)
    y, loss, dx, g = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    yr, lr, dxr, gr = ddbpn_ref.run(sd, x, t, scale)
    errs = sorted(((rel_err(g[k], gr[k]), k) for k in gr), reverse=True)
    print(f"[ddbpn] x{scale} {shape} fp32 vs float64: y {rel_err(y, yr):.2e} loss {abs(loss - float(lr)) / float(lr):.2e} dx {rel_err(dx, dxr):.2e} "
          f"worst grads {[(f'{e:.2e}', k) for e, k in errs[:3]]}")
    assert set(g) == set(gr)
    assert rel_err(y, yr) < F32_TOL and abs(loss - float(lr)) < F32_TOL * float(lr) and rel_err(dx, dxr) < F32_TOL and errs[0][0] < F32_TOL


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_modes_against_the_storage_emulation(dtype, scale):
    """The yardstick of test_gpu_rcan.py: against float64, the native relative L2 error may not exceed 1.5 x the error of the float64
    restatement with 16-bit STORAGE (+ 5e-3), on y, dx and the worst parameter gradient.

    The loss carries a static scale of 1024, as 16-bit training does: the native backward stores its gradient tensors in the 16-bit type,
    the emulation rounds the forward only.  The mean-reduced L1 loss hands 1 / N = 2.2e-4 (x4: N = 4608) to every output element; two
    layers of weights around 0.02 further in, the gradients lie below float16's smallest normal number 2^-14 = 6.1e-5, where only a few
    bits are left.  Without the scale the x4 float16 case measured 0.040 on downmodules.4.conv_2.0.weight against a bound of 0.037 on an
    MI355X (the emulation with its gradients rounded to float16 too gives 0.138 for that tensor on the CPU); with it, that emulation
    returns to the forward-only figures, so the rule compares like with like."""
    shape, scale_loss = (2, 3, 8, 6), 1024.0
    m, x, t = _case(scale, shape, dtype, 5)
    y, loss, dx, g = step(m, x, t, scale_loss)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    yr, _, dxr, gr = ddbpn_ref.run(sd, x, t, scale, loss_scale=scale_loss)
    ye, _, dxe, ge = ddbpn_ref.run(sd, x, t, scale, store=STORE[dtype], loss_scale=scale_loss)
    nat = sorted(((rel_l2(g[k], gr[k]), k) for k in gr), reverse=True)
    emu = sorted(((rel_l2(ge[k], gr[k]), k) for k in gr), reverse=True)
    print(f"[ddbpn] x{scale} {dtype} native vs float64: y {rel_l2(y, yr):.4f} dx {rel_l2(dx, dxr):.4f} worst grads {nat[:2]}")
    print(f"[ddbpn] x{scale} {dtype} storage emulation vs float64: y {rel_l2(ye, yr):.4f} dx {rel_l2(dxe, dxr):.4f} worst grads {emu[:2]}")
    bound = lambda e: 1.5 * e + 5e-3
    assert all(torch.isfinite(v).all() for v in g.values())
    assert rel_l2(y, yr) < bound(rel_l2(ye, yr))
    assert rel_l2(dx, dxr) < bound(rel_l2(dxe, dxr))
    assert nat[0][0] < bound(emu[0][0])


@pytest.mark.parametrize("scale, dtype", [(2, "bf16"), (4, "fp32"), (8, "fp16")])
def test_no_grad_path_has_the_bits_of_the_training_forward(scale, dtype):
    m, x, t = _case(scale, (2, 3, 7, 6), dtype, 7)
    x = x.cuda()
    y = m(x)
    assert y.grad_fn is not None
    with torch.no_grad():
        yi = m(x)
    assert yi.grad_fn is None and not yi.requires_grad and torch.equal(yi, y.detach())
    y.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="twice"):
        y.sum().backward()


def test_upscale_scene_on_one_tile_equals_the_forward():
    from srcgan_amd import infer
    m, _, _ = _case(2, (1, 3, 8, 8), "bf16", 9)
    scene = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(10)).cuda()
    assert len(infer.plan_tiles(32, 32, 32, 8, 1).tiles) == 1
    with torch.no_grad():
        whole = m(scene)
    got = infer.upscale_scene(m, scene, up=2, tile=32, halo=8, blend="feather")
    assert tuple(got.shape) == (1, 3, 64, 64) and torch.equal(got, whole)


def test_exact_mode_on_a_2x2_tile_plan_equals_the_whole_image_forward():
    """``upscale_scene`` with halo = receptive_halo (crop) against the same module's whole-image no_grad forward; gate: the exact-mode
    tests' fp32 gate, rel_err < 1e-3 (tests/test_gpu_infer_scene.py).  The tiles' convolutions see other tile shapes than the whole
    image's, so the bits may differ; the value is printed."""
    from srcgan_amd import infer
    m, _, _ = _case(4, (1, 3, 8, 8), "fp32", 13)
    scene = torch.rand(1, 3, 24, 20, generator=torch.Generator().manual_seed(14)).cuda()
    halo = infer.receptive_halo(m)
    assert len(infer.plan_tiles(24, 20, 12, halo, 1).tiles) == 4
    with torch.no_grad():
        whole = m(scene)
    got = infer.upscale_scene(m, scene, up=4, tile=12)
    err = rel_err(got, whole)
    print(f"[ddbpn] x4 exact mode, 2 x 2 tiles, halo {halo}: tiled vs whole-image rel_err {err:.3e}")
    assert tuple(got.shape) == (1, 3, 96, 80) and err < 1e-3
