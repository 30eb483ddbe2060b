"""GPU: the native VDSR against the reference fixture (fp32, 1e-3 ``rel_err``, the project's fp32 gate), against our float64 restatement
at n_feats = 64 on shapes with a tile seam in both directions, in the 16-bit modes against the storage emulation, its no_grad path, and
whole-scene inference through upscale_scene (one tile; exact mode on a 2 x 2-tile plan).  VDSR has no scales: its output has the
input's size.  Observed values are printed (pytest -s).

The figures measured on an MI355X are in DESIGN 3.12."""
import pytest
import torch

import mdsr_ref
from conftest import load_golden, rel_err
from net_checks import STORE, check_16bit, check_exact_tiles, check_fixture, check_fp32, check_no_grad_bits, check_one_tile_scene, step
from test_mdsr_ref import native

pytestmark = pytest.mark.gpu


def test_fp32_against_the_reference_fixture():
    z = load_golden("vdsr")
    m = native(z, "vdsr").cuda()
    assert list(m.state_dict().keys()) == [str(n) for n in z["names"]]
    y, loss, dx, g = step(m, torch.from_numpy(z["x"]), torch.from_numpy(z["t"]))
    assert tuple(y.shape) == tuple(z["x"].shape)
    assert list(g) == mdsr_ref.fixture_grad_names(z) and len(z["nograd"]) == 0
    assert {k for k, p in m.named_parameters() if p.grad is None} == {str(k) for k in z["frozen"]}
    check_fixture("mdsr", "vdsr fp32 vs reference", mdsr_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err))


def _case(shape, dtype, seed, n_resblocks=4, n_feats=64):
    import srcgan_amd
    torch.manual_seed(seed)
    m = srcgan_amd.VDSR(n_resblocks=n_resblocks, n_feats=n_feats, rgb_range=1, dtype=dtype)
    g = torch.Generator().manual_seed(seed + 1)
    return m.cuda(), torch.rand(*shape, generator=g), torch.rand(*shape, generator=g)


# n_resblocks = 2 is the shortest network: the first convolution's output feeds the one that adds the skip
@pytest.mark.parametrize("n, shape", [(4, (2, 3, 11, 37)), (2, (3, 3, 19, 9))])
def test_fp32_against_the_float64_restatement(n, shape):
    m, x, t = _case(shape, "fp32", 3, n_resblocks=n)
    got = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    check_fp32("mdsr", f"vdsr r{n} {shape}", got, mdsr_ref.vdsr_run(sd, x, t, n), names="list")


_REF16 = {}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_modes_against_the_storage_emulation(dtype):
    shape, scale_loss = (2, 3, 9, 7), 1024.0
    m, x, t = _case(shape, dtype, 5)
    got = step(m, x, t, scale_loss)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    if "ref" not in _REF16:          # the float64 run is the same for both 16-bit types (same seed, same weights)
        _REF16["ref"] = mdsr_ref.vdsr_run(sd, x, t, 4, loss_scale=scale_loss)
    check_16bit("mdsr", "vdsr", dtype, got, _REF16["ref"], mdsr_ref.vdsr_run(sd, x, t, 4, store=STORE[dtype], loss_scale=scale_loss), names="list")


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_no_grad_path_has_the_bits_of_the_training_forward(dtype):
    m, x, _ = _case((2, 3, 7, 6), dtype, 7)
    assert tuple(check_no_grad_bits(m, x).shape) == (2, 3, 7, 6)


def test_upscale_scene_on_one_tile_equals_the_forward():
    from srcgan_amd import infer
    m, _, _ = _case((1, 3, 8, 8), "bf16", 9, n_feats=32)
    scene = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(10)).cuda()
    check_one_tile_scene(m, scene, 1, (1, 3, 32, 32))
    with pytest.raises(ValueError, match=r"up = 2"):
        infer.upscale_scene(m, scene, up=2, tile=32, halo=8, blend="feather")


def test_exact_mode_on_a_2x2_tile_plan_equals_the_whole_image_forward():
    """receptive_halo = n_resblocks = 4"""
    m, _, _ = _case((1, 3, 8, 8), "fp32", 13, n_feats=32)
    scene = torch.rand(1, 3, 24, 20, generator=torch.Generator().manual_seed(14)).cuda()
    check_exact_tiles("vdsr", m, scene, 1, 12, 4, (1, 3, 24, 20), halo=4)
