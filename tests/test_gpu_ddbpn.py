"""GPU: the native DDBPN against the reference fixtures (fp32, 1e-3 ``rel_err`` as tests/test_gpu_modules.py uses), against our
float64 restatement at one further shape per scale, in the 16-bit modes against the storage emulation, its no_grad path, and whole-scene
inference through upscale_scene (one tile; exact mode on a 2 x 2-tile plan).  Observed values are printed (pytest -s).

The figures measured on an MI355X are in DESIGN 3.9."""
import pytest
import torch

import ddbpn_ref
from conftest import load_golden, rel_err
from ddbpn_ref import sketch
from net_checks import F32_TOL, STORE, check_16bit, check_exact_tiles, check_fp32, check_no_grad_bits, check_one_tile_scene, step

pytestmark = pytest.mark.gpu
FIXTURES = ("ddbpn_x2", "ddbpn_x4", "ddbpn_x8")


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
    got = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    check_fp32("ddbpn", f"x{scale} {shape}", got, ddbpn_ref.run(sd, x, t, scale), names="set")


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_modes_against_the_storage_emulation(dtype, scale):
    """net_checks.bound16, with the static loss scale of 1024 it explains"""
    shape, scale_loss = (2, 3, 8, 6), 1024.0
    m, x, t = _case(scale, shape, dtype, 5)
    got = step(m, x, t, scale_loss)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    ref, emu = ddbpn_ref.run(sd, x, t, scale, loss_scale=scale_loss), ddbpn_ref.run(sd, x, t, scale, store=STORE[dtype], loss_scale=scale_loss)
    check_16bit("ddbpn", f"x{scale}", dtype, got, ref, emu, names="set")


@pytest.mark.parametrize("scale, dtype", [(2, "bf16"), (4, "fp32"), (8, "fp16")])
def test_no_grad_path_has_the_bits_of_the_training_forward(scale, dtype):
    m, x, _ = _case(scale, (2, 3, 7, 6), dtype, 7)
    check_no_grad_bits(m, x)


def test_upscale_scene_on_one_tile_equals_the_forward():
    m, _, _ = _case(2, (1, 3, 8, 8), "bf16", 9)
    scene = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(10)).cuda()
    check_one_tile_scene(m, scene, 2, (1, 3, 64, 64))


def test_exact_mode_on_a_2x2_tile_plan_equals_the_whole_image_forward():
    m, _, _ = _case(4, (1, 3, 8, 8), "fp32", 13)
    scene = torch.rand(1, 3, 24, 20, generator=torch.Generator().manual_seed(14)).cuda()
    check_exact_tiles("ddbpn", m, scene, 4, 12, 4, (1, 3, 96, 80))
