"""CPU: score_scene's fixture, float64 restatement, host-only planner queries and argument checks (no kernel is launched).

``ref64`` restates the four reference formulas (src/metrics.py:22-33, 50, 67-68, 91-144) for a batch of one image; it reproduces the
reference-generated ``ref64/*`` of tests/golden/scene_score.npz and serves the GPU tests (tests/test_gpu_scene_score.py) for
generated shapes, at float32 as well to supply the reference's own f32-vs-f64 error."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

QS = ("MSE", "PSNR", "AE", "SSIM", "CS")
CASES = ["s11x11x3", "s11x75x1", "s43x75x3", "s97x139x3", "s97x139x1"]
BIG = ["s43x75x3", "s97x139x3", "s97x139x1"]          # both edges exceed 21: the 10-pixel border is not the whole scene


def planes(x):
    """u8 [H,W] / [H,W,C] -> f32 [1,C,H,W] with v / 255 (quotient in double, one rounding); f32 [1,C,H,W] as is."""
    x = torch.as_tensor(x)
    if x.dtype == torch.uint8:
        if x.dim() == 2:
            x = x.unsqueeze(2)
        return (x.double() / 255.0).float().permute(2, 0, 1).unsqueeze(0).contiguous()
    assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1
    return x


def ref64(pred, target, dtype=torch.float64, crop_border=False, shift=0):
    """The reference's MSE / PSNR / AE / SSIM / CS of one image pair, evaluated in ``dtype`` -> {name: float}.
    ``crop_border`` / ``shift`` are deliberate mistakes for the teeth tests: leave the last 10 rows and columns out of MSE and AE;
    move the SSIM window grid by ``shift`` pixels."""
    p, t = planes(pred).to(dtype).cpu(), planes(target).to(dtype).cpu()
    L = (255 if float(p.max()) > 128 else 1) - (-1 if float(p.min()) < -0.5 else 0)
    pm, tm = (p[..., :-10, :-10], t[..., :-10, :-10]) if crop_border else (p, t)
    mse = ((pm - tm) ** 2).mean()
    dot = (pm * tm).sum(1)
    ae = (180 / math.pi * torch.acos(dot / (torch.sqrt((pm * pm).sum(1)) * torch.sqrt((tm * tm).sum(1)) + 1e-6))).mean()
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], dtype=torch.float32)          # the reference's f32 window
    g = (g / g.sum()).unsqueeze(1)
    ch = p.shape[1]
    win = g.mm(g.t()).expand(ch, 1, 11, 11).contiguous().to(dtype)
    ps, ts = (p[..., shift:, shift:], t[..., shift:, shift:]) if shift else (p, t)
    conv = lambda z: F.conv2d(z, win, groups=ch)
    m1, m2 = conv(ps), conv(ts)
    s1, s2, s12 = conv(ps * ps) - m1 * m1, conv(ts * ts) - m2 * m2, conv(ps * ts) - m1 * m2
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    v1, v2 = 2.0 * s12 + C2, s1 + s2 + C2
    ssim = ((2 * m1 * m2 + C1) * v1) / ((m1 * m1 + m2 * m2 + C1) * v2)
    return {"MSE": float(mse), "PSNR": float(10 * torch.log10(1 / mse)), "AE": float(ae), "SSIM": float(ssim.mean()), "CS": float((v1 / v2).mean())}


def tolerances(r64, r32):
    """Per quantity: max(1e-4, 3 x the reference's own f32-vs-f64 relative error) -- the project's widening rule (README)."""
    return {q: max(1e-4, 3 * abs(r32[q] - r64[q]) / abs(r64[q])) for q in r64}


def rel(a, b):
    return abs(a - b) / abs(b)


def make_pair(H, W, C, seed):
    """Seeded data of the fixture's kind -> (pred, target) u8 [H,W,C]: smooth target, prediction = target + noise of 12 levels, a
    block of zeros in the prediction and a smaller one in the target, the prediction's last 10 rows and columns inverted."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(1, C, max(2, H // 8 + 2), max(2, W // 8 + 2), generator=g)
    field = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0]
    target = (field * 215 + 20).round().clamp(0, 255)
    pred = (target + 12.0 * torch.randn(C, H, W, generator=g)).round().clamp(0, 255)
    y0, x0 = H // 4, W // 4
    pred[:, y0:y0 + max(2, H // 5), x0:x0 + max(2, W // 5)] = 0
    target[:, y0:y0 + max(1, H // 10), x0:x0 + max(1, W // 10)] = 0
    pred[:, H - 10:, :] = 255 - pred[:, H - 10:, :]
    pred[:, :, W - 10:] = 255 - pred[:, :, W - 10:]
    hwc = lambda z: z.permute(1, 2, 0).contiguous().to(torch.uint8)
    return hwc(pred), hwc(target)


def golden_case(g, name):
    pred, target = torch.from_numpy(g[f"{name}/pred"]), torch.from_numpy(g[f"{name}/target"])
    r64 = {q: float(g[f"{name}/ref64/{q}"]) for q in QS}
    r32 = {q: float(g[f"{name}/ref32/{q}"]) for q in QS}
    return pred, target, r64, r32


@pytest.fixture(scope="module")
def fixture_npz():
    return load_golden("scene_score")


@pytest.mark.parametrize("name", CASES)
def test_ref64_reproduces_the_fixture(fixture_npz, name):
    pred, target, r64, r32 = golden_case(fixture_npz, name)
    mine = ref64(pred, target)
    for q in QS:
        assert rel(mine[q], r64[q]) <= 1e-12, (q, mine[q], r64[q])
    mine32 = ref64(pred, target, dtype=torch.float32)
    tol = tolerances(r64, r32)
    for q in QS:          # the f32 evaluation stands in for the reference's f32 run on generated shapes: it is as close to ref64
        assert rel(mine32[q], r64[q]) <= tol[q], (q, mine32[q], r64[q])


@pytest.mark.parametrize("name", BIG)
def test_fixture_has_teeth(fixture_npz, name):
    pred, target, r64, r32 = golden_case(fixture_npz, name)
    tol = tolerances(r64, r32)
    cropped = ref64(pred, target, crop_border=True)
    assert rel(cropped["MSE"], r64["MSE"]) > 100 * tol["MSE"]
    assert rel(cropped["AE"], r64["AE"]) > 100 * tol["AE"]
    shifted = ref64(pred, target, shift=1)
    assert rel(shifted["SSIM"], r64["SSIM"]) > tol["SSIM"]


def _lib():
    from srcgan_amd import build, _native as N
    build.build(verbose=False)
    return N.lib()


def test_tile_edge():
    assert 16 <= _lib().srcgan_scene_score_tile() <= 64


def test_ws_bytes():
    lib = _lib()
    assert lib.srcgan_scene_score_ws_bytes(11, 11, 1) > 0
    for H, W, Cc in ((256, 256, 1), (8192, 8192, 3), (40000, 40000, 3)):          # the last: tiles x bytes per tile needs 64-bit arithmetic
        ws = lib.srcgan_scene_score_ws_bytes(H, W, Cc)
        assert 0 < ws <= H * W * Cc // 16, (H, W, Cc, ws)
    T = lib.srcgan_scene_score_tile()
    tiles = lambda n: -(-(n - 10) // T)
    assert lib.srcgan_scene_score_ws_bytes(40000, 40000, 3) >= tiles(40000) ** 2 * 16          # not truncated: four f32 partials per tile
    for bad in ((10, 64, 3), (64, 10, 3), (64, 64, 2)):
        assert lib.srcgan_scene_score_ws_bytes(*bad) == 0
        assert b"srcgan_scene_score" in lib.srcgan_last_error()


def test_score_scene_is_exported():
    import srcgan_amd
    from srcgan_amd import metrics as M
    assert "score_scene" in srcgan_amd.__all__ and "score_scene" in M.__all__
    assert srcgan_amd.score_scene is M.score_scene


@pytest.mark.parametrize("pred, target, msg", [
    (torch.zeros(32, 32, 3, dtype=torch.uint8), torch.zeros(32, 32, 3, dtype=torch.uint8), "cpu"),
    (torch.zeros(1, 3, 32, 32), torch.zeros(32, 32, 3, dtype=torch.uint8), "cpu"),
    (torch.zeros(32, 32, 3, dtype=torch.uint8), torch.zeros(32, 33, 3, dtype=torch.uint8), "target is"),
    (torch.zeros(32, 32, 3, dtype=torch.uint8), torch.zeros(1, 1, 32, 32), "target is"),
    (torch.zeros(32, 32, 2, dtype=torch.uint8), torch.zeros(32, 32, 2, dtype=torch.uint8), "C must be 1 or 3"),
    (torch.zeros(1, 2, 32, 32), torch.zeros(1, 2, 32, 32), "C must be 1 or 3"),
    (torch.zeros(10, 32, 3, dtype=torch.uint8), torch.zeros(10, 32, 3, dtype=torch.uint8), "at least 11x11"),
    (torch.zeros(1, 1, 32, 10), torch.zeros(1, 1, 32, 10), "at least 11x11"),
    (torch.zeros(32, 32, 3, dtype=torch.int32), torch.zeros(32, 32, 3, dtype=torch.uint8), "pred must be"),
    (torch.zeros(32, 32, 3, dtype=torch.uint8), torch.zeros(32, 32, 3, dtype=torch.float32), "target must be"),
    (torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32), "pred must be"),
    (torch.zeros(32, dtype=torch.uint8), torch.zeros(32, dtype=torch.uint8), "pred must be"),
])
def test_score_scene_rejects(pred, target, msg):
    """CPU tensors, mismatched shapes, C = 2, H or W = 10, a wrong dtype, a batch of two, a wrong rank: ValueError before any launch
    (the tensors here are all on the CPU; the device is checked last, so every other message is reached first)."""
    from srcgan_amd import score_scene
    with pytest.raises(ValueError, match=msg):
        score_scene(pred, target)
