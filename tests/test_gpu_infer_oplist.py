"""GPU: the inference path of the op-list networks (ResDeconv, ESPCN, SRCNN, EDSR under ``torch.no_grad()`` ->
srcgan_resdeconv_infer / srcgan_srnet_infer on the slot-planned workspace).  Without the folded tail it launches the kernels of
the training forward in the same order, so its claim is BIT equality with the grad-mode forward.  ResDeconv's module path folds
deconv13 and pred into four parity 2x2 convolutions: equal in real arithmetic, so it is held to the fp32 gate against the
reference's goldens and, in the 16-bit modes, to the error of the unfolded forward."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3
MIB = 1 << 20
DTYPES = ["fp32", "bf16", "fp16"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _both(net, x):
    """(inference output, grad-mode output) of one module on one input."""
    assert torch.is_grad_enabled()
    with torch.no_grad():
        yi = net(x)
    yt = net(x)
    assert yt.grad_fn is not None and yi.grad_fn is None and not yi.requires_grad
    return yi, yt.detach()


def _l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------------------------------------ ESPCN / SRCNN / EDSR
SR_CASES = [("espcn", (1, 1, 2), {}), ("espcn", (3, 3, 3), {}), ("srcnn", (3, 3, 1), {})] + \
           [("edsr", (3, 3, up), dict(num_residuals=n)) for n in (2, 5) for up in (1, 2, 4)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,args,kw", SR_CASES, ids=[f"{k}-{'-'.join(map(str, a))}" + "".join(f"-n{v}" for v in w.values()) for k, a, w in SR_CASES])
def test_sr_inference_equals_the_training_forward_bit_for_bit(kind, args, kw, dtype):
    import srcgan_amd as S
    torch.manual_seed(11)
    net = {"espcn": S.ESPCN, "srcnn": S.SRCNN, "edsr": S.EDSR}[kind](*args, dtype=dtype, **kw).cuda()
    torch.manual_seed(5)
    x = torch.rand(2, args[0], 19, 35, device="cuda")
    yi, yt = _both(net, x)
    assert yi.shape == yt.shape and torch.isfinite(yi).all()
    assert torch.equal(yi, yt)
    with torch.no_grad():                       # a second pass over warm buffers, and an input that requires grad, change nothing
        assert torch.equal(net(x), yt)
        assert torch.equal(net(x.clone().requires_grad_(True)), yt)
    net.eval()                                  # eval() alone keeps the autograd path
    assert net(x).grad_fn is not None


# ------------------------------------------------------------------------------------------------ ResDeconv
def _resdeconv_infer(net, x, fold):
    """srcgan_resdeconv_infer through ctypes, on the module's parameters."""
    from srcgan_amd import _native as N
    lib = N.lib()
    if net.src_ch == 1:
        x = torch.cat([x, x, x], dim=1)
    x = x.contiguous().float()
    B, _, H, W = x.shape
    cfg = N.ResDeconvCfg(3, net.tar_ch, B, H, W, N.dtype_id(net.compute_dtype), (C.c_int * 4)(*net.layers_cfg), 1 if net.BN == "IN" else 0)
    plist = [p.detach().contiguous() for p in net.parameters()]
    ws = N.workspace(lib.srcgan_resdeconv_infer_ws_bytes(C.byref(cfg), fold), x.device)
    y = torch.empty(B, net.tar_ch, H, W, dtype=torch.float32, device=x.device)
    N.check(lib.srcgan_resdeconv_infer(C.byref(cfg), x.data_ptr(), N.ptr_array(plist), ws.data_ptr(), y.data_ptr(), fold,
                                       N.stream_ptr(x.device)), "srcgan_resdeconv_infer")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layers", [[2, 2, 2, 2], [3, 4, 6, 3]], ids=["r18", "r34"])
@pytest.mark.parametrize("BN", ["GN", "IN"])
def test_resdeconv_unfolded_inference_equals_the_training_forward_bit_for_bit(BN, layers, dtype):
    """16 x 16 is the smallest legal input: the tail's half-resolution grid is 8 x 8 there, every border case occurs."""
    from srcgan_amd import ResDeconv
    for src, tar, shape in ((1, 3, (2, 1, 32, 48)), (3, 2, (1, 3, 16, 16))):
        torch.manual_seed(11)
        net = ResDeconv(src, tar, None, layers, BN, dtype=dtype).cuda()
        torch.manual_seed(5)
        x = torch.rand(*shape, device="cuda")
        yt = net(x).detach()
        assert torch.isfinite(yt).all()
        assert torch.equal(_resdeconv_infer(net, x, 0), yt)
        assert torch.equal(_resdeconv_infer(net, x, 0), yt)        # warm


def _compose_f64(dec, pred):
    """Wc[a][b][dy][dx][t][c] in float64 from deconv13.weight [64(c), 64(m), 2, 2] and pred.weight [tar, 64(m), 3, 3]: tap (u, v) of
    output pixel (2i + a, 2j + b) reads full-resolution pixel (2i + a + u - 1, 2j + b + v - 1), i.e. sub-position
    ((a + u - 1) mod 2, (b + v - 1) mod 2) of half-resolution pixel (i + floor((a + u - 1) / 2), j + floor((b + v - 1) / 2)); the window
    of parity (a, b) starts at (i + a - 1, j + b - 1)."""
    dec, pred = dec.astype(np.float64), pred.astype(np.float64)
    Wc = np.zeros((2, 2, 2, 2, pred.shape[0], 64))
    for a in range(2):
        for b in range(2):
            for u in range(3):
                for v in range(3):
                    hy, p = divmod(a + u - 1, 2)
                    hx, q = divmod(b + v - 1, 2)
                    Wc[a, b, hy - (a - 1), hx - (b - 1)] += np.einsum("tm,cm->tc", pred[:, :, u, v], dec[:, :, p, q])
    return Wc


def test_the_composition_formula_against_the_two_layers_in_float64():
    """CPU arithmetic: the derivation itself, borders included -- four parity 2x2 convolutions with Wc on a zero-padded input
    against conv2d(conv_transpose2d(h)) in float64."""
    rng = np.random.default_rng(3)
    dec, pred = rng.standard_normal((64, 64, 2, 2)), rng.standard_normal((3, 64, 3, 3))
    h = rng.standard_normal((1, 64, 5, 6))
    ref = torch.nn.functional.conv2d(torch.nn.functional.conv_transpose2d(torch.from_numpy(h), torch.from_numpy(dec), stride=2),
                                     torch.from_numpy(pred), padding=1).numpy()
    Wc = _compose_f64(dec, pred)
    hp = np.pad(h, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(ref)
    for a in range(2):
        for b in range(2):
            for dy in range(2):
                for dx in range(2):
                    win = hp[0, :, a + dy:a + dy + 5, b + dx:b + dx + 6]          # padded index of (i + a - 1 + dy) is i + a + dy
                    out[0, :, a::2, b::2] += np.einsum("tc,cij->tij", Wc[a, b, dy, dx], win)
    assert np.abs(out - ref).max() <= 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize("tar", [1, 2, 3])
def test_composed_weights_against_float64(tar):
    """The kernel's f32 pack Wp[parity][chunk (4)][tap][row (32)][k (16)] against the float64 sums.  Bound: relative L2 <= 1e-6 -- f32
    accumulation of at most 9 * 64 products (2^-24 per rounding, random signs)."""
    from srcgan_amd import _native as N
    lib = N.lib()
    g = torch.Generator().manual_seed(20 + tar)
    dec, pred = torch.randn(64, 64, 2, 2, generator=g).cuda(), torch.randn(tar, 64, 3, 3, generator=g).cuda()
    nbytes = lib.srcgan_fold_tail_pack_bytes(N.F32)
    assert nbytes == 4 * 4 * 4 * 32 * 16 * 4
    wp = torch.full((nbytes // 4,), float("nan"), device="cuda")
    N.check(lib.srcgan_fold_tail_pack(dec.data_ptr(), pred.data_ptr(), wp.data_ptr(), tar, N.F32, N.stream_ptr(wp.device)), "srcgan_fold_tail_pack")
    got = wp.cpu().numpy().astype(np.float64).reshape(4, 4, 4, 32, 16)            # [parity][chunk][tap][row][k]
    got = got.transpose(0, 2, 3, 1, 4).reshape(2, 2, 2, 2, 32, 64)                # [a][b][dy][dx][row][c]
    assert np.isfinite(got).all() and not got[..., tar:, :].any()                 # rows past tar_ch are zero
    want = _compose_f64(dec.cpu().numpy(), pred.cpu().numpy())
    err = np.linalg.norm(got[..., :tar, :] - want) / np.linalg.norm(want)
    print(f"composed weights tar_ch={tar}: relative L2 {err:.3e}")
    assert err <= 1e-6
    for a in range(2):                                                            # ... and tap by tap: a swapped pair of taps cannot hide
        for b in range(2):
            for t in range(4):
                w = want[a, b, t >> 1, t & 1]
                assert np.linalg.norm(got[a, b, t >> 1, t & 1, :tar] - w) <= 1e-6 * np.linalg.norm(w), (a, b, t)


@pytest.mark.parametrize("tag", ["resdeconv_gray", "resdeconv_rgb", "resdeconv_in", "resdeconv_r34"])
def test_resdeconv_goldens_under_no_grad(tag):
    """The folded tail against the reference's own output, fp32 gate.  Printed, not gated: the distance to the grad-mode forward
    (the two differ by the rounding of the composed weights and of one 64-channel tensor)."""
    from test_oracle_golden import _resdeconv_from_cfg
    g = load_golden(tag)
    net = _resdeconv_from_cfg(g, dtype="fp32").cuda()
    yi, yt = _both(net, torch.from_numpy(g["x"]).cuda())
    print(f"{tag}: folded vs reference {rel_err(yi.cpu(), g['y']):.3e}, folded vs grad-mode forward {rel_err(yi, yt):.3e}")
    assert rel_err(yi.cpu(), g["y"]) < F32_TOL


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_folded_tail_is_no_worse_than_the_unfolded_one_in_16_bit(dtype):
    """e_fold <= 1.25 e_plain, both relative L2 against the fp32 native output: the fold removes one rounding of a 64-channel tensor
    (and adds one of the composed weights), so it should not be worse; the margin covers a single unlucky input."""
    from srcgan_amd import ResDeconv
    torch.manual_seed(11)
    net = ResDeconv(1, 3, dtype="fp32").cuda()
    torch.manual_seed(5)
    x = torch.rand(2, 1, 32, 48, device="cuda")
    y32 = net(x).detach()
    net.compute_dtype = dtype
    yi, yt = _both(net, x)
    e_fold, e_plain = _l2(yi, y32), _l2(yt, y32)
    print(f"{dtype}: e_fold {e_fold:.4e} e_plain {e_plain:.4e} ratio {e_fold / e_plain:.3f}")
    assert torch.equal(_resdeconv_infer(net, x, 1), yi)                          # the module path IS fold_tail = 1
    assert e_fold <= 1.25 * e_plain


def _warm_peak(net, x):
    """(peak extra bytes during a warm no_grad call, bytes left afterwards, output bytes)."""
    with torch.no_grad():
        y = net(x)                                  # first call: job tables are staged here
    ybytes = y.numel() * 4
    del y
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        y = net(x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    after = torch.cuda.memory_allocated() - before
    assert torch.isfinite(y).all()
    return peak, after, ybytes


def test_edsr_inference_workspace_is_what_the_planner_says_and_is_given_back():
    from srcgan_amd import EDSR, _native as N
    torch.manual_seed(11)
    net = EDSR(3, 3, 2, num_residuals=50, dtype="bf16").cuda()
    peak, after, ybytes = _warm_peak(net, torch.rand(2, 3, 64, 64, device="cuda"))
    cfg = N.SrNetCfg(2, 3, 3, 2, 64, 2, 64, 64, N.BF16, 50)
    infer, train = N.lib().srcgan_srnet_infer_ws_bytes(C.byref(cfg)), N.lib().srcgan_srnet_ws_bytes(C.byref(cfg))
    print(f"EDSR-50: peak {peak / MIB:.1f} MiB, planner: inference {infer / MIB:.1f} MiB, training {train / MIB:.1f} MiB, y {ybytes / MIB:.1f} MiB")
    assert peak <= infer + ybytes + MIB
    assert ybytes <= after <= ybytes + 512          # the caching allocator rounds a block to 512 bytes
    assert infer < train / 3


def test_resdeconv_inference_workspace_is_what_the_planner_says_and_is_given_back():
    from srcgan_amd import ResDeconv, _native as N
    torch.manual_seed(11)
    net = ResDeconv(1, 3, dtype="bf16").cuda()
    peak, after, ybytes = _warm_peak(net, torch.rand(2, 1, 128, 128, device="cuda"))
    cfg = N.ResDeconvCfg(3, 3, 2, 128, 128, N.BF16, (C.c_int * 4)(2, 2, 2, 2), 0)
    infer, train = N.lib().srcgan_resdeconv_infer_ws_bytes(C.byref(cfg), 1), N.lib().srcgan_resdeconv_ws_bytes(C.byref(cfg))
    print(f"ResDeconv: peak {peak / MIB:.1f} MiB, planner: inference {infer / MIB:.1f} MiB, training {train / MIB:.1f} MiB, y {ybytes / MIB:.1f} MiB")
    assert peak <= infer + ybytes + MIB             # (the 3-channel replica of the gray input is inside the MiB)
    assert ybytes <= after <= ybytes + 512
    assert infer < train


def test_the_composed_pack_follows_both_of_its_sources():
    from srcgan_amd import ResDeconv
    torch.manual_seed(11)
    net = ResDeconv(1, 3, dtype="fp32").cuda()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    x = torch.rand(2, 1, 32, 32, device="cuda")

    def infer():
        with torch.no_grad():
            return net(x)

    prev = infer()
    assert rel_err(prev, net(x)) < F32_TOL
    for w in (net.deconv13.weight, net.pred.weight):
        w.data.mul_(0.5)
        y = infer()
        assert not torch.equal(y, prev)
        assert rel_err(y, net(x)) < F32_TOL
        prev = y
    net(x).abs().mean().backward()
    opt.step()
    y = infer()
    assert not torch.equal(y, prev)
    assert rel_err(y, net(x)) < F32_TOL
    assert torch.equal(infer(), y)


def test_cascade_scoring_loop_runs_on_the_inference_path():
    """metrics.evaluate_cascade (no_grad) against the same loop on the networks' grad-mode outputs."""
    from srcgan_amd import ESPCN, ResDeconv, metrics as M, ops
    torch.manual_seed(1)
    sr, cn = ESPCN(1, 1, 2).cuda(), ResDeconv(1, 3).cuda()
    batches = [{"src": torch.rand(1, 1, 64, 64), "tar": torch.rand(1, 3, 64, 64)} for _ in range(2)]
    M.evaluate_cascade(sr, cn, batches, up=2)                   # warm: job tables
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    perf, outs = M.evaluate_cascade(sr, cn, batches, up=2)
    assert all(o.grad_fn is None and o.shape == (1, 3, 64, 64) for o in outs)
    del outs
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before              # no workspace is left behind
    evs = [M.MSE(), M.PSNR(), M.AE(), M.SSIM()]
    want = {repr(e): [] for e in evs}
    for s in batches:
        realB = s["tar"].cuda()
        fake = cn(sr(ops.nearest_resize(ops.rgb_to_gray(realB), 0.5)))
        assert fake.grad_fn is not None
        for e in evs:
            want[repr(e)].append(e(fake.detach(), realB).item())
    for k, v in want.items():
        w = sum(v) / len(v)
        assert np.isfinite(perf[k]) and abs(perf[k] - w) <= 1e-3 * abs(w), (k, perf[k], w)


def test_scene_sized_pass():
    """ResDeconv(1, 3), bf16, 1 x 1 x 2048 x 2048 under no_grad: finite, right shape, peak memory within the planner's figure, and a
    256 x 256 interior crop against the fp32 native result.  GroupNorm's statistics span the whole image, so the crop cannot be
    recomputed on its own: the fp32 reference is a no_grad pass of the same module in fp32 at the full size, and the assertion is
    the one of the small 16-bit test -- the crop's error is at most 1.25 x that of the grad-mode bf16 forward at the same size."""
    from srcgan_amd import ResDeconv, _native as N
    torch.manual_seed(11)
    net = ResDeconv(1, 3, dtype="bf16").cuda()
    torch.manual_seed(9)
    x = torch.rand(1, 1, 2048, 2048, device="cuda")
    peak, after, ybytes = _warm_peak(net, x)
    cfg = N.ResDeconvCfg(3, 3, 1, 2048, 2048, N.BF16, (C.c_int * 4)(2, 2, 2, 2), 0)
    infer = N.lib().srcgan_resdeconv_infer_ws_bytes(C.byref(cfg), 1)
    assert peak <= infer + ybytes + 3 * x.numel() * 4 + MIB     # + the 3-channel replica of the gray input
    crop = (slice(None), slice(None), slice(896, 1152), slice(896, 1152))
    with torch.no_grad():
        yi = net(x)
        assert yi.shape == (1, 3, 2048, 2048) and torch.isfinite(yi).all()
        yi = yi[crop].clone()
        net.compute_dtype = "fp32"
        y32 = net(x)[crop].clone()
    net.compute_dtype = "bf16"
    yt = net(x).detach()[crop].clone()
    e_fold, e_plain = _l2(yi, y32), _l2(yt, y32)
    print(f"scene: peak {peak / MIB:.0f} MiB (planner {infer / MIB:.0f} MiB), crop e_fold {e_fold:.4e} e_plain {e_plain:.4e}")
    assert e_fold <= 1.25 * e_plain
