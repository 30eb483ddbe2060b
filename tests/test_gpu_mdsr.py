"""GPU: the native MDSR against the three reference fixtures (fp32, 1e-3 ``rel_err``, the project's fp32 gate; the set of parameters with
a gradient is the fixture's), against our float64 restatement at n_feats = 64 -- the 5x5 multi-chunk path and a tile seam in both
directions -- once per scale_idx, in the 16-bit modes against the storage emulation, ``set_scale`` on one instance, its no_grad path,
and whole-scene inference through upscale_scene (one tile; exact mode on a 2 x 2-tile plan).  Observed values are printed (pytest -s).

The figures measured on an MI355X are in DESIGN 3.12."""
import pytest
import torch

import mdsr_ref
from conftest import load_golden, rel_err
from net_checks import STORE, check_16bit, check_exact_tiles, check_fixture, check_fp32, check_no_grad_bits, check_one_tile_scene, step
from test_mdsr_ref import MDSR_FIXTURES, native

pytestmark = pytest.mark.gpu
SCALES = [2, 3, 4]


@pytest.mark.parametrize("tag", MDSR_FIXTURES)
def test_fp32_against_the_reference_fixture(tag):
    z = load_golden(tag)
    m = native(z, tag).cuda()
    assert list(m.state_dict().keys()) == [str(n) for n in z["names"]]
    y, loss, dx, g = step(m, torch.from_numpy(z["x"]), torch.from_numpy(z["t"]))
    assert list(g) == mdsr_ref.fixture_grad_names(z)
    assert {k for k, p in m.named_parameters() if p.grad is None} == {str(k) for k in z["nograd"]} | {str(k) for k in z["frozen"]}
    check_fixture("mdsr", f"{tag} fp32 vs reference", mdsr_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err))


def _case(idx, shape, dtype, seed, n_resblocks=2, n_feats=64, scales=SCALES):
    import srcgan_amd
    torch.manual_seed(seed)
    m = srcgan_amd.MDSR(n_resblocks=n_resblocks, n_feats=n_feats, scale=scales, rgb_range=1, dtype=dtype)
    m.set_scale(idx)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(*shape, generator=g)
    t = torch.rand(shape[0], 3, shape[2] * scales[idx], shape[3] * scales[idx], generator=g)
    return m.cuda(), x, t


# n_feats = 64: two K chunks per tap in the 16-bit types and four in fp32 on the 64-row tile of the 5x5 kernel; 37 columns and 11 / 19 rows:
# a 32-pixel tile seam and an 8-row tile seam at LR; odd sizes, a batch the fixtures do not have
@pytest.mark.parametrize("idx, shape", [(0, (2, 3, 11, 37)), (1, (3, 3, 19, 9)), (2, (2, 3, 11, 37))])
def test_fp32_against_the_float64_restatement(idx, shape):
    m, x, t = _case(idx, shape, "fp32", 3)
    got = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    check_fp32("mdsr", f"x{SCALES[idx]} {shape}", got, mdsr_ref.mdsr_run(sd, x, t, 2, SCALES, idx), names="list")


_REF16 = {}


@pytest.mark.parametrize("idx", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_modes_against_the_storage_emulation(dtype, idx):
    """net_checks.bound16, with its static loss scale of 1024"""
    shape, scale_loss = (2, 3, 9, 7), 1024.0
    m, x, t = _case(idx, shape, dtype, 5)
    got = step(m, x, t, scale_loss)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    if idx not in _REF16:           # the float64 run is the same for both 16-bit types (same seed, same weights)
        _REF16[idx] = mdsr_ref.mdsr_run(sd, x, t, 2, SCALES, idx, loss_scale=scale_loss)
    emu = mdsr_ref.mdsr_run(sd, x, t, 2, SCALES, idx, store=STORE[dtype], loss_scale=scale_loss)
    check_16bit("mdsr", f"x{SCALES[idx]}", dtype, got, _REF16[idx], emu, names="list")


def _branch_off(m, idx):
    return {k for k, _ in m.named_parameters() if any(k.startswith(f"{part}.{j}.") for part in ("pre_process", "upsample") for j in range(3) if j != idx)}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_set_scale_on_one_instance(dtype):
    """idx 0, then 2, then 0 again: the third run has the bits of the first; after each run exactly the branches off the graph (and the
    frozen shifts) have no gradient; an optimiser step in between leaves their weights untouched."""
    m, x, _ = _case(0, (2, 3, 9, 7), dtype, 11)
    frozen = {"sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias"}
    runs = []
    for idx in (0, 2, 0):
        m.set_scale(idx)
        t = torch.rand(2, 3, 9 * SCALES[idx], 7 * SCALES[idx], generator=torch.Generator().manual_seed(20 + idx))
        runs.append(step(m, x, t))
        assert tuple(runs[-1][0].shape) == tuple(t.shape)
        assert {k for k, p in m.named_parameters() if p.grad is None} == _branch_off(m, idx) | frozen
        assert list(runs[-1][3]) == mdsr_ref.mdsr_branch(2, SCALES, idx)
    a, b = runs[0], runs[2]
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2]) and all(torch.equal(a[3][k], b[3][k]) for k in a[3])
    assert not torch.equal(runs[1][0][..., :18, :14], a[0])
    # an optimiser step at idx 2 (the gradients of the last run are those of idx 0: take a fresh one)
    m.set_scale(2)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.1)
    step(m, x, torch.rand(2, 3, 36, 28, generator=torch.Generator().manual_seed(22)))
    opt.step()
    after = m.state_dict()
    moved = {k for k in before if not torch.equal(before[k], after[k])}
    assert moved == set(mdsr_ref.mdsr_branch(2, SCALES, 2)), sorted(moved ^ set(mdsr_ref.mdsr_branch(2, SCALES, 2)))


@pytest.mark.parametrize("idx, dtype", [(0, "bf16"), (1, "fp32"), (2, "fp16")])
def test_no_grad_path_has_the_bits_of_the_training_forward(idx, dtype):
    m, x, _ = _case(idx, (2, 3, 7, 6), dtype, 7)
    check_no_grad_bits(m, x)


def test_upscale_scene_on_one_tile_equals_the_forward():
    from srcgan_amd import infer
    m, _, _ = _case(1, (1, 3, 8, 8), "bf16", 9, n_resblocks=1, n_feats=32)
    scene = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(10)).cuda()
    check_one_tile_scene(m, scene, 3, (1, 3, 96, 96))
    with pytest.raises(ValueError, match=r"not to 64x64 \(up = 2\)"):          # an ``up`` that disagrees with the active scale
        infer.upscale_scene(m, scene, up=2, tile=32, halo=8, blend="feather")
    got8 = infer.upscale_scene(m, scene, up=3, tile=32, halo=8, blend="feather", ensemble=8)
    assert tuple(got8.shape) == (1, 3, 96, 96) and bool(torch.isfinite(got8).all())


@pytest.mark.parametrize("idx", [0, 2])
def test_exact_mode_on_a_2x2_tile_plan_equals_the_whole_image_forward(idx):
    """n_resblocks = 1 keeps the halo at 14"""
    m, _, _ = _case(idx, (1, 3, 8, 8), "fp32", 13, n_resblocks=1, n_feats=32)
    s = SCALES[idx]
    scene = torch.rand(1, 3, 24, 20, generator=torch.Generator().manual_seed(14)).cuda()
    check_exact_tiles("mdsr", m, scene, s, 12, 4, (1, 3, 24 * s, 20 * s), halo=14)
