"""GPU: the native RCAN against the reference fixtures (fp32, 1e-3 ``rel_err`` as tests/test_gpu_modules.py uses), against our
float64 restatement at the default width and on a ragged pool, in the 16-bit modes against the storage emulation, its no_grad path, and
whole-scene inference through upscale_scene (one tile; ensemble=8).  Observed values are printed (pytest -s).

The figures measured on an MI355X are in DESIGN 3.8."""
import pytest
import torch

import d4_ref
import rcan_ref
from conftest import load_golden, rel_err, rel_l2

pytestmark = pytest.mark.gpu
F32_TOL = 1e-3
FIXTURES = ("rcan_x2", "rcan_x3", "rcan_x4")
STORE = {"bf16": torch.bfloat16, "fp16": torch.float16}


def build(z, dtype="fp32"):
    import srcgan_amd
    ng, nb, F, red, scale = (int(v) for v in z["cfg"])
    torch.manual_seed(int(z["seed"]))
    return srcgan_amd.RCAN(n_resgroups=ng, n_resblocks=nb, n_feats=F, reduction=red, scale=scale, rgb_range=1, dtype=dtype).cuda()


def step(m, x, t):
    """forward, L1 loss, backward -> (y, loss, dx, {name: grad}) on the CPU"""
    for p in m.parameters():
        p.grad = None
    x = x.detach().cuda().requires_grad_(True)
    y = m(x)
    loss = torch.nn.functional.l1_loss(y, t.cuda())
    loss.backward()
    return y.detach().cpu(), float(loss.detach()), x.grad.cpu(), {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("tag", FIXTURES)
def test_fp32_against_the_reference_fixture(tag):
    z = load_golden(tag)
    m = build(z)
    assert list(m.state_dict().keys()) == [str(n) for n in z["names"]]
    y, loss, dx, g = step(m, torch.from_numpy(z["x"]), torch.from_numpy(z["t"]))
    frozen = [str(n) for n in z["frozen"]]
    assert all(getattr(m.get_parameter(k), "grad") is None and not m.get_parameter(k).requires_grad for k in frozen) and len(frozen) == 4
    assert set(g) == {k for k in map(str, z["names"]) if k not in frozen}
    errs = sorted(((rel_err(v, z["grad/" + k]), k) for k, v in g.items()), reverse=True)
    print(f"[rcan] {tag} fp32 vs reference: y {rel_err(y, z['y']):.2e} loss {abs(loss - float(z['loss'])) / float(z['loss']):.2e} "
          f"dx {rel_err(dx, z['dx']):.2e} worst grads {[(f'{e:.2e}', k) for e, k in errs[:3]]}")
    assert rel_err(y, z["y"]) < F32_TOL and abs(loss - float(z["loss"])) < F32_TOL * float(z["loss"]) and rel_err(dx, z["dx"]) < F32_TOL
    assert errs[0][0] < F32_TOL, errs[:3]


def _case(groups, blocks, feats, reduction, scale, shape, dtype, seed):
    import srcgan_amd
    torch.manual_seed(seed)
    m = srcgan_amd.RCAN(n_resgroups=groups, n_resblocks=blocks, n_feats=feats, reduction=reduction, scale=scale, rgb_range=1, dtype=dtype).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(*shape, generator=g)
    t = torch.rand(shape[0], 3, shape[2] * scale, shape[3] * scale, generator=g)
    return m, x, t


@pytest.mark.parametrize("name, cfg", [("default width", (1, 2, 64, 16, 2, (2, 3, 8, 8))), ("ragged pool", (2, 2, 32, 8, 2, (2, 3, 5, 7)))])
def test_fp32_against_the_float64_restatement(name, cfg):
    m, x, t = _case(*cfg, "fp32", 3)
    y, loss, dx, g = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    yr, lr, dxr, gr = rcan_ref.run(sd, x, t, cfg[0], cfg[1], cfg[4])
    errs = sorted(((rel_err(g[k], gr[k]), k) for k in gr), reverse=True)
    print(f"[rcan] {name} fp32 vs float64: y {rel_err(y, yr):.2e} loss {abs(loss - float(lr)) / float(lr):.2e} dx {rel_err(dx, dxr):.2e} "
          f"worst grads {[(f'{e:.2e}', k) for e, k in errs[:3]]}")
    assert set(g) == set(gr)
    assert rel_err(y, yr) < F32_TOL and abs(loss - float(lr)) < F32_TOL * float(lr) and rel_err(dx, dxr) < F32_TOL and errs[0][0] < F32_TOL


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_modes_against_the_storage_emulation(dtype):
    """The yardstick of test_gpu_modules.py::test_rddbnet_nb23_bf16_vs_oracle: against float64, the native relative L2 error may not
    exceed 1.5 x the error of the float64 restatement with 16-bit STORAGE (+ 5e-3), on y, dx and the worst parameter gradient."""
    cfg = (2, 2, 32, 8, 2, (2, 3, 12, 10))
    m, x, t = _case(*cfg, dtype, 5)
    y, loss, dx, g = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    yr, _, dxr, gr = rcan_ref.run(sd, x, t, cfg[0], cfg[1], cfg[4])
    ye, _, dxe, ge = rcan_ref.run(sd, x, t, cfg[0], cfg[1], cfg[4], store=STORE[dtype])
    nat = sorted(((rel_l2(g[k], gr[k]), k) for k in gr), reverse=True)
    emu = sorted(((rel_l2(ge[k], gr[k]), k) for k in gr), reverse=True)
    print(f"[rcan] {dtype} native vs float64: y {rel_l2(y, yr):.4f} dx {rel_l2(dx, dxr):.4f} worst grads {nat[:2]}")
    print(f"[rcan] {dtype} storage emulation vs float64: y {rel_l2(ye, yr):.4f} dx {rel_l2(dxe, dxr):.4f} worst grads {emu[:2]}")
    bound = lambda e: 1.5 * e + 5e-3
    assert all(torch.isfinite(v).all() for v in g.values())
    assert rel_l2(y, yr) < bound(rel_l2(ye, yr))
    assert rel_l2(dx, dxr) < bound(rel_l2(dxe, dxr))
    assert nat[0][0] < bound(emu[0][0])


def test_no_grad_path_has_the_bits_of_the_training_forward():
    m, x, t = _case(2, 2, 32, 8, 3, (2, 3, 7, 6), "bf16", 7)
    x = x.cuda()
    y = m(x)
    assert y.grad_fn is not None
    with torch.no_grad():
        yi = m(x)
    assert yi.grad_fn is None and not yi.requires_grad and torch.equal(yi, y.detach())
    y.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="twice"):
        y.sum().backward()


@pytest.fixture(scope="module")
def scene_net():
    m, _, _ = _case(1, 2, 32, 8, 2, (1, 3, 8, 8), "bf16", 9)
    scene = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(10)).cuda()
    return m.eval(), scene


def test_upscale_scene_on_one_tile_equals_the_forward(scene_net):
    from srcgan_amd import infer
    m, scene = scene_net
    assert len(infer.plan_tiles(32, 32, 32, 8, 1).tiles) == 1
    with torch.no_grad():
        whole = m(scene)
    got = infer.upscale_scene(m, scene, up=2, tile=32, halo=8, blend="feather")
    assert tuple(got.shape) == (1, 3, 64, 64) and torch.equal(got, whole)
    with pytest.raises(ValueError, match="halo="):
        infer.upscale_scene(m, scene, up=2, tile=32)


def test_ensemble8_is_the_d4_average_of_eight_native_forwards(scene_net):
    from srcgan_amd import infer
    m, scene = scene_net
    got = infer.upscale_scene(m, scene, up=2, tile=32, halo=8, blend="feather", ensemble=8)
    with torch.no_grad():
        folded = [d4_ref.torch_fold(m(d4_ref.torch_view(scene, op)).float(), op) for op in d4_ref.OPS[8]]
    assert torch.equal(got, d4_ref.torch_average(folded))
