"""GPU: srcgan_amd.score_scene (csrc/scene_score.hip) against the reference-generated fixture tests/golden/scene_score.npz and the
float64 restatement of tests/test_scene_score_host.py.

Tolerance, per quantity: |native - ref64| / |ref64| <= max(1e-4, 3 x the reference's own f32-vs-f64 relative error) -- 1e-4 is what
tests/test_gpu_harness.py holds the existing metric kernels to, the widening is the README's rule.  Every test prints its observed
figures before it asserts."""
import math

import pytest
import torch

from conftest import load_golden
from test_scene_score_host import CASES, QS, golden_case, make_pair, planes, ref64, rel, tolerances

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import score_scene
    return score_scene


@pytest.fixture(scope="module")
def fixture_npz():
    return load_golden("scene_score")


def vals(d):
    assert all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for v in d.values())
    return {k: float(v) for k, v in d.items()}


def check(got, r64, tol, what):
    worst = {q: rel(got[q], r64[q]) for q in QS}
    print(what, " ".join(f"{q} {worst[q]:.2e}/{tol[q]:.1e}" for q in QS))
    for q in QS:
        assert worst[q] <= tol[q], (what, q, got[q], r64[q], tol[q])


def forms(u8):
    return {"u8": u8.cuda(), "f32": planes(u8).cuda()}


# ------------------------------------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("name", CASES)
def test_fixture_all_kind_combinations(S, fixture_npz, name):
    pred, target, r64, r32 = golden_case(fixture_npz, name)
    tol = tolerances(r64, r32)
    p, t = forms(pred), forms(target)
    if pred.shape[2] == 1:
        p["u8"] = p["u8"][:, :, 0].contiguous()          # the [H,W] form of a gray scene
    res = {}
    for kp in ("u8", "f32"):
        for kt in ("u8", "f32"):
            d = S(p[kp], t[kt], full=True)
            assert set(d) == {"MSE", "PSNR", "AE", "SSIM", "CS"} and set(S(p[kp], t[kt])) == {"MSE", "PSNR", "AE", "SSIM"}
            res[kp, kt] = vals(d)
            check(res[kp, kt], r64, tol, f"{name} {kp}/{kt}")
    base = res["u8", "u8"]
    for key, r in res.items():
        for q in QS:
            assert rel(r[q], base[q]) <= tol[q], (key, q)


# ------------------------------------------------------------------------------------------------ 2. tile seams
def _seam_case(i):
    """case i of 12: the six edge lengths below, paired so that each appears on each axis twice, C alternating"""
    from srcgan_amd import _native as N
    T = N.lib().srcgan_scene_score_tile()
    e = [T + 9, T + 10, T + 11, 2 * T + 10, 2 * T + 11, 3 * T + 13]
    return (e[i], e[(i + 3) % 6], (1, 3)[i % 2]) if i < 6 else (e[i - 6], e[(i - 4) % 6], (3, 1)[i % 2])


@pytest.mark.parametrize("i", range(12))
def test_tile_seams(S, i):
    """every edge length of {T+9, T+10, T+11, 2T+10, 2T+11, 3T+13} on each axis, with C = 1 and C = 3: a last tile of one position,
    a full last tile, one position into the next tile, two and three tiles"""
    H, W, C = _seam_case(i)
    pred, target = make_pair(H, W, C, 7 * H + W)
    r64, r32 = ref64(pred, target), ref64(pred, target, dtype=torch.float32)
    check(vals(S(pred.cuda(), target.cuda(), full=True)), r64, tolerances(r64, r32), f"seam {H}x{W}x{C}")


# ------------------------------------------------------------------------------------------------ 3. misaligned base
@pytest.mark.parametrize("C", [1, 3])
def test_misaligned_u8_views_are_bit_equal(S, C):
    H, W = 53, 45                                    # W * C odd: every row starts at another offset in its dword
    pred, target = make_pair(H, W, C, 3)
    n = H * W * C
    want = vals(S(pred.cuda(), target.cuda(), full=True))
    for op, ot in ((1, 0), (2, 3), (3, 1), (0, 2)):
        bp, bt = torch.zeros(n + 8, dtype=torch.uint8, device="cuda"), torch.full((n + 8,), 255, dtype=torch.uint8, device="cuda")
        vp, vt = bp[op:op + n].view(H, W, C), bt[ot:ot + n].view(H, W, C)
        vp.copy_(pred); vt.copy_(target)
        assert vp.is_contiguous() and vp.storage_offset() == op and vp.data_ptr() % 4 == op and vt.data_ptr() % 4 == ot
        assert vals(S(vp, vt, full=True)) == want, (op, ot)


# ------------------------------------------------------------------------------------------------ 4. range selection
def test_range_selection_follows_the_prediction(S, fixture_npz):
    pred, target, _, _ = golden_case(fixture_npz, "s97x139x3")
    p, t = planes(pred), planes(target)
    for what, f in (("L=255", lambda z: z * 255), ("L=2", lambda z: z * 2 - 1)):
        pp, tt = f(p), f(t)
        r64, r32 = ref64(pp, tt), ref64(pp, tt, dtype=torch.float32)
        check(vals(S(pp.cuda(), tt.cuda(), full=True)), r64, tolerances(r64, r32), what)
    assert float(p.max() * 255) > 128 and float((p * 2 - 1).min()) < -0.5
    # a u8 prediction is in [0, 1]: the same numbers as its f32 copy, whose range pass finds L = 1
    a, b = vals(S(pred.cuda(), target.cuda(), full=True)), vals(S(p.cuda(), target.cuda(), full=True))
    assert a == b


# ------------------------------------------------------------------------------------------------ 5. identity
def test_identity(S):
    x = torch.randint(0, 256, (70, 83, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
    d = vals(S(x, x.clone(), full=True))
    print("identity", d)
    assert d["MSE"] == 0.0 and d["PSNR"] == math.inf and abs(d["SSIM"] - 1) <= 1e-6 and abs(d["CS"] - 1) <= 1e-6


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_determinism_and_side_stream(S):
    pred, target = make_pair(150, 201, 3, 11)
    p, t = pred.cuda(), planes(target).cuda()
    a, b = vals(S(p, t, full=True)), vals(S(p, t, full=True))
    assert a == b
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = S(p, t, full=True)
    side.synchronize()
    assert vals(c) == a


# ------------------------------------------------------------------------------------------------ 7. the existing kernels
def test_agrees_with_the_existing_metric_kernels(S, fixture_npz):
    from srcgan_amd import metrics as M
    pred, target, _, _ = golden_case(fixture_npz, "s97x139x3")
    p, t = planes(pred).cuda(), planes(target).cuda()
    r64, r32 = ref64(p.cpu(), t.cpu()), ref64(p.cpu(), t.cpu(), dtype=torch.float32)
    s, cs = M.SSIM()(p, t, full=True)
    old = {"MSE": float(M.MSE()(p, t)), "PSNR": float(M.PSNR()(p, t)), "AE": float(M.AE()(p, t)[0]), "SSIM": float(s), "CS": float(cs)}
    check(vals(S(p, t, full=True)), old, tolerances(r64, r32), "vs M.*")


# ------------------------------------------------------------------------------------------------ 8. memory
def test_memory_is_the_workspace(S):
    from srcgan_amd import _native as N
    H, W, C = 1024, 1536, 3
    g = torch.Generator().manual_seed(4)
    p = torch.randint(0, 256, (H, W, C), dtype=torch.uint8, generator=g).cuda()
    t = torch.randint(0, 256, (H, W, C), dtype=torch.uint8, generator=g).cuda()
    ws = N.lib().srcgan_scene_score_ws_bytes(H, W, C)
    assert 0 < ws <= H * W * C // 16
    S(p, t)                                          # first call: code objects loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    d = S(p, t, full=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("memory rise", rise, "ws", ws)
    assert rise <= ws + 4096 and math.isfinite(float(d["SSIM"]))


# ------------------------------------------------------------------------------------------------ 9. 64-bit offsets
def test_offsets_past_2_to_31(S):
    """u8 26760 x 26760 x 3 = 2.148e9 elements per scene (> 2^31), zeros; the prediction's last 16 rows are 255.  MSE = 16 / 26760;
    every pixel's angle is acos(0 / (0 + eps)) = 90 degrees.  A 32-bit offset would wrap long before the last rows."""
    n = 26760
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 1024 ** 3:
        pytest.skip("needs 6 GB of free device memory")
    assert n * n * 3 > 2 ** 31
    p = torch.zeros(n, n, 3, dtype=torch.uint8, device="cuda")
    t = torch.zeros(n, n, 3, dtype=torch.uint8, device="cuda")
    p[n - 16:] = 255
    d = vals(S(p, t, full=True))
    del p, t
    print("2^31", d)
    assert rel(d["MSE"], 16 / n) <= 1e-9
    assert abs(d["AE"] - 90.0) <= 1e-4 * 90.0
    assert math.isfinite(d["SSIM"]) and 0.0 <= d["SSIM"] <= 1.0


# ------------------------------------------------------------------------------------------------ 10. end to end
def test_scores_a_cascade_scene_picture(S):
    from srcgan_amd import RDDBNet, SRCNN, cascade_scene
    torch.manual_seed(31)
    sr, col = RDDBNet(1, 1, 2, nf=16, nb=1, gc=8).cuda().eval(), SRCNN(1, 3, 1, 16).cuda().eval()
    g = torch.Generator().manual_seed(5)
    scene = torch.randint(0, 256, (24, 26), dtype=torch.uint8, generator=g).cuda()
    pic = cascade_scene(sr, col, scene, up=2, tile=16, halo=None, batch=2, out="u8")
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (48, 52, 3)
    target = torch.randint(0, 256, (48, 52, 3), dtype=torch.uint8, generator=g).cuda()
    pf, tf = planes(pic.cpu()), planes(target.cpu())
    r64, r32 = ref64(pf, tf), ref64(pf, tf, dtype=torch.float32)
    tol = tolerances(r64, r32)
    a, b = vals(S(pic, target, full=True)), vals(S(pf.cuda(), tf.cuda(), full=True))
    check(a, b, tol, "u8 picture vs its f32 copy")
    check(a, r64, tol, "u8 picture vs ref64")
