"""GPU: the native RCAN against the reference fixtures (fp32, 1e-3 ``rel_err`` as tests/test_gpu_modules.py uses), against our
float64 restatement at the default width and on a ragged pool, in the 16-bit modes against the storage emulation, its no_grad path, and
whole-scene inference through upscale_scene (one tile; ensemble=8).  Observed values are printed (pytest -s).

The figures measured on an MI355X are in DESIGN 3.8."""
import pytest
import torch

import d4_ref
import rcan_ref
from conftest import load_golden, rel_err
from net_checks import F32_TOL, STORE, check_16bit, check_fp32, check_no_grad_bits, check_one_tile_scene, step

pytestmark = pytest.mark.gpu
FIXTURES = ("rcan_x2", "rcan_x3", "rcan_x4")


def build(z, dtype="fp32"):
    import srcgan_amd
    ng, nb, F, red, scale = (int(v) for v in z["cfg"])
    torch.manual_seed(int(z["seed"]))
    return srcgan_amd.RCAN(n_resgroups=ng, n_resblocks=nb, n_feats=F, reduction=red, scale=scale, rgb_range=1, dtype=dtype).cuda()


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
    got = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    check_fp32("rcan", name, got, rcan_ref.run(sd, x, t, cfg[0], cfg[1], cfg[4]), names="set")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_modes_against_the_storage_emulation(dtype):
    cfg = (2, 2, 32, 8, 2, (2, 3, 12, 10))
    m, x, t = _case(*cfg, dtype, 5)
    got = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    ref, emu = rcan_ref.run(sd, x, t, cfg[0], cfg[1], cfg[4]), rcan_ref.run(sd, x, t, cfg[0], cfg[1], cfg[4], store=STORE[dtype])
    check_16bit("rcan", "", dtype, got, ref, emu, names="set")


def test_no_grad_path_has_the_bits_of_the_training_forward():
    m, x, _ = _case(2, 2, 32, 8, 3, (2, 3, 7, 6), "bf16", 7)
    check_no_grad_bits(m, x)


@pytest.fixture(scope="module")
def scene_net():
    m, _, _ = _case(1, 2, 32, 8, 2, (1, 3, 8, 8), "bf16", 9)
    scene = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(10)).cuda()
    return m.eval(), scene


def test_upscale_scene_on_one_tile_equals_the_forward(scene_net):
    from srcgan_amd import infer
    m, scene = scene_net
    check_one_tile_scene(m, scene, 2, (1, 3, 64, 64))
    with pytest.raises(ValueError, match="halo="):
        infer.upscale_scene(m, scene, up=2, tile=32)


def test_ensemble8_is_the_d4_average_of_eight_native_forwards(scene_net):
    from srcgan_amd import infer
    m, scene = scene_net
    got = infer.upscale_scene(m, scene, up=2, tile=32, halo=8, blend="feather", ensemble=8)
    with torch.no_grad():
        folded = [d4_ref.torch_fold(m(d4_ref.torch_view(scene, op)).float(), op) for op in d4_ref.OPS[8]]
    assert torch.equal(got, d4_ref.torch_average(folded))
