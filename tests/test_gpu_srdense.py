"""GPU: SRDenseNetA / SRDenseNetB and their up-sampler kernel (ConvTranspose2d k3 s2 p1 output_padding 1, four parities in one
launch: csrc/deconv_k3s2.hip).  Observed errors are printed (pytest -s).

16-bit gates have the form of the existing bf16 module tests: relative L2 against a float64 evaluation may not exceed 1.5 x the
error of the same float64 evaluation with storage rounded to the format, plus 5e-3."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err, rel_l2
from net_checks import F32_TOL, bound16 as bound, check_no_grad_bits
from test_srdense_host import BIG, TAGS, build_from_fixture, check_grads, restate_run, sketch

pytestmark = pytest.mark.gpu

TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", [(1, 32, 32, 1, 1), (3, 64, 32, 5, 7), (2, 256, 256, 4, 33)], ids=lambda s: "x".join(map(str, s)))
def test_deconv3x3s2_kernel(shape, dtype):
    from srcgan_amd import ops
    B, cin, cout, H, W = shape
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, cin, H, W, generator=gen)
    w = torch.randn(cin, cout, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    ref = lambda xx, ww: F.relu(F.conv_transpose2d(xx.double(), ww.double(), b.double(), stride=2, padding=1, output_padding=1))
    y64 = ref(x, w)
    td = TORCH_DT[dtype]
    y = ops.to_nchw(ops.deconv3x3s2(ops.to_nhwc(x.cuda(), dtype=dtype), w.cuda(), b.cuda(), relu=True)).cpu()
    assert y.shape == y64.shape == (B, cout, 2 * H, 2 * W) and torch.isfinite(y).all()
    y64r = ref(x.to(td), w.to(td)) if dtype != "fp32" else None
    for a in (0, 1):
        for c in (0, 1):          # each output parity on its own: one wrong parity cannot hide in a mean
            got, want = y[:, :, a::2, c::2], y64[:, :, a::2, c::2]
            if dtype == "fp32":
                e = rel_err(got, want)
                print(f"deconv3x3s2 {shape} fp32 parity ({a},{c}): rel_err {e:.3e}")
                assert e < F32_TOL
            else:
                e, fmt = rel_l2(got, want), rel_l2(y64r[:, :, a::2, c::2], want)
                print(f"deconv3x3s2 {shape} {dtype} parity ({a},{c}): rel L2 {e:.3e}, rounded-input f64 {fmt:.3e}")
                assert e < bound(fmt)


# ------------------------------------------------------------------------------------------------ 2. module parity, f32
def _run(net, g, device="cuda"):
    x = torch.from_numpy(g["x"]).to(device).requires_grad_(True)
    y = net(x)
    loss = F.l1_loss(y, torch.from_numpy(g["t"]).to(device))
    loss.backward()
    return y.detach().cpu(), float(loss), x.grad.cpu(), {k: p.grad.cpu() for k, p in net.named_parameters()}


@pytest.mark.parametrize("tag", TAGS)
def test_module_golden_f32(tag):
    g = load_golden(tag)
    net, (kind, _, _, _) = build_from_fixture(g, tag, dtype="fp32")
    y, loss, dx, grads = _run(net.cuda(), g)
    errs = {k: rel_err(grads[k], g["grad/" + k]) for k in grads if k != BIG}
    errs[BIG + " (slice)"] = rel_err(grads[BIG][:, 0] if kind == "a" else grads[BIG][0], g["gslice/" + BIG])
    errs[BIG + " (sketch)"] = rel_err(sketch(grads[BIG]), g["gsketch/" + BIG])
    print(f"{tag} fp32: y {rel_err(y, g['y']):.3e} dx {rel_err(dx, g['dx']):.3e} loss diff {abs(loss - float(g['loss'])):.2e} worst grad {max(errs.items(), key=lambda kv: kv[1])}")
    assert rel_err(y, g["y"]) < F32_TOL
    assert abs(loss - float(g["loss"])) < 1e-5
    assert rel_err(dx, g["dx"]) < F32_TOL
    check_grads(g, grads, F32_TOL, transposed=kind == "a")


# ------------------------------------------------------------------------------------------------ 3. perf dtypes
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("tag", ["srdense_a_x2", "srdense_b_x2"])
def test_module_16bit_vs_storage_rounding(tag, dtype):
    g = load_golden(tag)
    net, (kind, nb, nl, up) = build_from_fixture(g, tag, dtype=dtype)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    td = TORCH_DT[dtype]
    yr, _, dxr, gr = restate_run(sd, g["x"], g["t"], kind, nb, nl, up)
    ye, _, dxe, ge = restate_run(sd, g["x"], g["t"], kind, nb, nl, up, store=lambda v: v.to(td).to(v.dtype))
    y, _, dx, gg = _run(net.cuda(), g)
    worst = max(rel_l2(gg[k], gr[k]) for k in gg)
    fmt = max(rel_l2(ge[k], gr[k]) for k in gg)
    print(f"{tag} {dtype}: y {rel_l2(y, yr):.4f} (format {rel_l2(ye, yr):.4f}) dx {rel_l2(dx, dxr):.4f} (format {rel_l2(dxe, dxr):.4f}) "
          f"worst grad {worst:.4f} (format {fmt:.4f})")
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert rel_l2(y, yr) < bound(rel_l2(ye, yr))
    assert rel_l2(dx, dxr) < bound(rel_l2(dxe, dxr))
    assert worst < bound(fmt)


# ------------------------------------------------------------------------------------------------ 4. inference
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("tag", TAGS)
def test_inference_equals_the_training_forward_bit_for_bit(tag, dtype):
    g = load_golden(tag)
    net, _ = build_from_fixture(g, tag, dtype=dtype)
    net = net.cuda()
    x = torch.from_numpy(g["x"]).cuda()
    net(x)                                       # warm: pack-cache tables and kernel attributes are allocated once
    with torch.no_grad():
        net(x)
    torch.cuda.synchronize()

    def peak(fn):
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    yt, mt = peak(lambda: net(x).detach())
    with torch.no_grad():
        yi, mi = peak(lambda: net(x))
    assert yi.grad_fn is None and torch.isfinite(yi).all()
    assert torch.equal(yi, yt)
    print(f"{tag} {dtype}: peak bytes no_grad {mi}, grad mode {mt}")
    assert mi <= mt
    check_no_grad_bits(net, x)                   # behind the measurement: its backward leaves gradients allocated


# ------------------------------------------------------------------------------------------------ 5. defaults (16, 8, 8)
def test_defaults_f32():
    """The widest concatenation (1152 channels into the bottleneck).  The input gradient runs through 66 ReLU layers and is gated at
    max(F32_TOL, 3 x the restatement's own f32-vs-f64 error), the project's rule for deep stacks."""
    import srcgan_amd as S
    torch.manual_seed(2)
    net = S.SRDenseNetA(1, 3, dtype="fp32")
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(3)
    g = {"x": torch.rand(1, 1, 8, 8, generator=gen).numpy(), "t": torch.rand(1, 3, 16, 16, generator=gen).numpy()}
    y64, _, dx64, g64 = restate_run(sd, g["x"], g["t"], "a", 8, 8, 2)
    _, _, dx32, _ = restate_run(sd, g["x"], g["t"], "a", 8, 8, 2, dtype=torch.float32)
    y, _, dx, grads = _run(net.cuda(), g)
    own = rel_err(dx32, dx64)
    worst = max((rel_err(grads[k], g64[k]), k) for k in grads)
    print(f"defaults fp32: y {rel_err(y, y64):.3e} dx {rel_err(dx, dx64):.3e} (restatement f32 vs f64 {own:.3e}) worst grad {worst}")
    assert rel_err(y, y64) < F32_TOL
    assert rel_err(dx, dx64) < max(F32_TOL, 3 * own)
    assert worst[0] < F32_TOL
