"""GPU: the native RDN against the three reference fixtures (fp32, 1e-3 ``rel_err``, the project's fp32 gate), against our float64
restatement at one further shape per configuration, in the 16-bit modes against the storage emulation, its no_grad path, whole-scene
inference through upscale_scene (one tile; exact mode on a 2 x 2-tile plan), and the weight gradient of a K slice of GFF.0 directly.
Observed values are printed (pytest -s).

The figures measured on an MI355X are in DESIGN 3.11."""
import pytest
import torch

import conv_exact as CE
import rdn_ref
from conftest import load_golden, rel_err
from net_checks import STORE, check_16bit, check_exact_tiles, check_fixture, check_fp32, check_no_grad_bits, check_one_tile_scene, step
from ws_guard import NAN, Guard, guarded_slabs

pytestmark = pytest.mark.gpu
FIXTURES = ("rdn_a_x2", "rdn_b_x3", "rdn_a_x4_gray")


@pytest.mark.parametrize("tag", FIXTURES)
def test_fp32_against_the_reference_fixture(tag):
    import srcgan_amd
    z = load_golden(tag)
    torch.manual_seed(int(z["seed"]))
    m = srcgan_amd.RDN(scale=int(z["scale"]), G0=int(z["G0"]), RDNconfig=str(z["config"]), n_colors=int(z["n_colors"])).cuda()
    assert list(m.state_dict().keys()) == [str(n) for n in z["names"]]
    y, loss, dx, g = step(m, torch.from_numpy(z["x"]), torch.from_numpy(z["t"]))
    assert list(g) == [str(n) for n in z["names"]]
    check_fixture("rdn", f"{tag} fp32 vs reference", rdn_ref.fixture_errors(z, y, loss, dx, g, "", measure=rel_err))


def _case(config, scale, shape, dtype, seed, G0=64):
    import srcgan_amd
    torch.manual_seed(seed)
    m = srcgan_amd.RDN(scale=scale, G0=G0, RDNconfig=config, n_colors=shape[1], dtype=dtype)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(*shape, generator=g)
    t = torch.rand(shape[0], shape[1], shape[2] * scale, shape[3] * scale, generator=g)
    return m.cuda(), x, t


# a further shape per configuration: more than one 32-pixel tile column at HR, odd sizes, and a batch the fixtures do not have
@pytest.mark.parametrize("config, scale, shape", [("A", 2, (3, 3, 19, 9)), ("B", 2, (2, 3, 9, 11))])
def test_fp32_against_the_float64_restatement(config, scale, shape):
    m, x, t = _case(config, scale, shape, "fp32", 3)
    got = step(m, x, t)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    check_fp32("rdn", f"'{config}' x{scale} {shape}", got, rdn_ref.run(sd, x, t, config, scale), names="set")


_REF16 = {}


def _ref16(config, scale, sd, x, t, dtype, loss_scale):
    """the float64 run is the same for both 16-bit types (same seed, same weights): computed once per configuration"""
    if (config, scale) not in _REF16:
        _REF16[(config, scale)] = rdn_ref.run(sd, x, t, config, scale, loss_scale=loss_scale)
    return _REF16[(config, scale)], rdn_ref.run(sd, x, t, config, scale, store=STORE[dtype], loss_scale=loss_scale)


@pytest.mark.parametrize("config, scale", [("A", 2), ("B", 3)])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_modes_against_the_storage_emulation(dtype, config, scale):
    """net_checks.bound16, with its static loss scale of 1024.  The emulation rounds GFF.0's running sum after every block, as the
    native plan does."""
    shape, scale_loss = (2, 3, 8, 6), 1024.0
    m, x, t = _case(config, scale, shape, dtype, 5)
    got = step(m, x, t, scale_loss)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    check_16bit("rdn", f"'{config}' x{scale}", dtype, got, *_ref16(config, scale, sd, x, t, dtype, scale_loss), names="set")


@pytest.mark.parametrize("config, scale, dtype, colors", [("A", 2, "bf16", 3), ("B", 3, "fp32", 3), ((2, 3, 32), 4, "fp16", 1)])
def test_no_grad_path_has_the_bits_of_the_training_forward(config, scale, dtype, colors):
    m, x, _ = _case(config, scale, (2, colors, 7, 6), dtype, 7)
    check_no_grad_bits(m, x)


def test_upscale_scene_on_one_tile_equals_the_forward():
    m, _, _ = _case((2, 3, 32), 2, (1, 3, 8, 8), "bf16", 9)
    scene = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(10)).cuda()
    check_one_tile_scene(m, scene, 2, (1, 3, 64, 64))


def test_exact_mode_on_a_2x2_tile_plan_equals_the_whole_image_forward():
    m, _, _ = _case((2, 3, 32), 3, (1, 3, 8, 8), "fp32", 13, G0=32)
    scene = torch.rand(1, 3, 24, 20, generator=torch.Generator().manual_seed(14)).cuda()
    check_exact_tiles("rdn", m, scene, 3, 12, 4, (1, 3, 72, 60), halo=11)


# ------------------------------------------------------------------------------------------------ the weight gradient of a K slice
KS_D, KS_G0 = 3, 64          # GFF.0 of a 3-block network: [64][192][1][1]; slice d owns columns [64 d, 64 d + 64)


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("dt", CE.DTS)
def test_k_slice_weight_gradient_lands_in_its_columns(dt, d, accumulate):
    """srcgan_conv_wgrad's split-K reduce scatters through (sr, sk, sty, stx, off); with sr = D G0, off = d G0 it writes slice d's
    [G0][G0] gradient into columns [d G0, (d + 1) G0) of the [G0][D G0] gradient of GFF.0 -- the call the RDN backward makes once per
    block.  Small-integer operands (tests/conv_exact.py): bit-equal to float64.  The destination sits between guards; stored into a
    NaN-filled tensor, every column outside the slice keeps its NaN bits; accumulated onto integers, every column outside keeps its value."""
    from srcgan_amd import ops
    T, G0, D = CE.TDT[dt], KS_G0, KS_D
    c = CE.wgrad_case(f"rdn_gff_kslice{d}", k=(1, 1), pad=(0, 0), cin=G0, cout=G0, hw=(9, 7), x_cs=256, dy_cs=G0)
    b = CE.build_wgrad(c)
    CE.check_exact(c["name"], dt, b["bound"] + 8, b["val"], b["val"], 1.0, f32_out=True)
    val = b["val"].reshape(G0, G0)
    guard = Guard(NAN, "cuda")
    grad = guard.carve("GFF.0.weight.grad", "grad", G0 * D * G0 * 4).view(torch.float32).view(G0, D * G0)
    old = CE.ints((G0, D * G0), -4, 4, CE.gen("rdn_gff_kslice_old")) if accumulate else None
    if accumulate:
        grad.copy_(old.float())
    before = grad.clone()
    x, dy = b["x"].to(T).cuda(), b["dy"].to(T).cuda()
    with guarded_slabs(NAN, "cuda") as gs:
        ops.conv_wgrad(dy, x, grad, kh=1, kw=1, stride=1, Cout=G0, Cin=G0, pad=(0, 0), layout=(D * G0, 1, 1, 1, d * G0), accumulate=accumulate)
        torch.cuda.synchronize()
        assert gs.calls == 1
    guard.check()
    cols = slice(d * G0, (d + 1) * G0)
    want = val + old[:, cols] if accumulate else val
    assert torch.equal(grad[:, cols].cpu().double(), want), "the slice's columns"
    outside = torch.ones(D * G0, dtype=torch.bool)
    outside[cols] = False
    assert torch.equal(grad[:, outside.cuda()].contiguous().view(torch.int32), before[:, outside.cuda()].contiguous().view(torch.int32)), "columns outside the slice"
    assert torch.equal(x.cpu().double(), b["x"]) and torch.equal(dy.cpu().double(), b["dy"])
