"""GPU: every whole-network driver (csrc/nets.hip, csrc/oplist.hip, the VGG feature path, score_scene) on poisoned, guarded workspaces.

Each case builds its module with seeded weights and runs one computation -- forward, a loss, backward, and the no-grad forward -- on the
same inputs on stock allocation and under tests/ws_guard.py's ZERO, NAN and STALE fills (STALE: the buffers a run of the same network on
-3 x left behind).  It asserts

  1. bit equality of y, the loss, x.grad, every parameter's gradient (and the BatchNorm buffers) across the four runs,
  2. that all of them are finite,
  3. intact guards after the forward, after the backward and after the inference call,
  4. that the allocations the patch recorded are the ones the planners answer for the configuration (*_ws_bytes, *_bwd_scratch_bytes,
     *_infer_ws_bytes, *_wpack_bytes) plus one gradient arena -- a workspace allocated some other way would leave this test blind.

No tolerance and no reference: the numbers are the business of the fixture and float64 tests at these same configurations, and the stock
run being bit-equal to the poisoned ones ties the two together.  tests/test_ws_guard_teeth.py shows on the CPU what these checks notice."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import oracle
from conftest import load_golden, sub
from ws_guard import assert_bit_equal, run_fills

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _chk(guard):
    if guard is not None:
        guard.check()


def _l1(y, t):
    return F.l1_loss(y, t)


def _lsgan_real(y, t):
    return (y - 1.0).square().mean()


# ------------------------------------------------------------------------------------------------ planners
def _lib():
    from srcgan_amd import _native as N
    return N, N.lib()


def _plan_rddb(net, x):
    from srcgan_amd import RDDBNetA, SRDN
    N, _ = _lib()
    B, _, H, W = x.shape
    dt = N.dtype_id(net.compute_dtype)
    if isinstance(net, SRDN):
        down, legacy = 0, 3
    elif hasattr(net, "_legacy"):
        down, legacy = 0, net._legacy
    else:
        down, legacy = (net._down() if isinstance(net, RDDBNetA) else 0), 0
    return "rddbnet", N.RddbCfg(*net._cfg, B, H, W, dt, down, legacy), ()


def _plan_nlayerd(net, x):
    N, _ = _lib()
    B, _, H, W = x.shape
    return "nlayerd", N.NLayerDCfg(*net._cfg, B, H, W, N.dtype_id(net.compute_dtype), 1, net._norm), ()


def _plan_oplist(net, x):
    import srcgan_amd as S
    from srcgan_amd import model as M
    N, _ = _lib()
    dt = N.dtype_id(net.compute_dtype)
    if isinstance(net, S.ResDeconv):
        x3 = torch.cat([x, x, x], 1) if net.src_ch == 1 else x
        return "resdeconv", M._resdeconv_cfg(x3, (net.tar_ch, dt, net.layers_cfg, 1 if net.BN == "IN" else 0))[0], (1,)
    if isinstance(net, S.EDSR):
        return "srnet", M._srnet_cfg(x, (*net._cfg, dt, net._nres))[0], ()
    if isinstance(net, (S.ESPCN, S.SRCNN)):
        return "srnet", M._srnet_cfg(x, (*net._cfg, dt))[0], ()
    if isinstance(net, S.SRDenseNetA):
        return "srdense", M._srdense_cfg(x, (*net._cfg, dt))[0], ()
    if isinstance(net, S.RCAN):
        return "rcan", M._rcan_cfg(x, (*net._cfg, dt))[0], ()
    assert isinstance(net, S.DDBPN), type(net)
    return "ddbpn", M._ddbpn_cfg(x, (*net._cfg, dt))[0], ()


def _sizes(stem, cfg, infer_extra, *, infer, wpack, fold0=False):
    """[(kind, bytes)] the planners answer for one training step (and the inference call) of one network"""
    _, lib = _lib()
    f = lambda name, *a: int(getattr(lib, f"srcgan_{stem}_{name}")(C.byref(cfg), *a))
    out = [("workspace", f("ws_bytes")), ("workspace", f("bwd_scratch_bytes"))]
    if infer:
        out.append(("workspace", f("infer_ws_bytes", *infer_extra)))
    if fold0:
        out.append(("workspace", f("infer_ws_bytes", 0)))
    if wpack:
        out.append(("wpack", f("wpack_bytes")))
    assert all(n > 0 for _, n in out), out
    return out


# ------------------------------------------------------------------------------------------------ one network, four fills
class _EveryRrdb:
    """A data-parallel hook that cuts the generator's backward at every RRDB and does nothing else."""

    def cuts(self, cfg, nrr, params):
        return list(range(nrr))

    def phase_done(self, arena, params, first, end, last):
        pass


def _network_case(net, x, t, plan, *, loss=_l1, infer=True, fold0=False, hook=None):
    """-> (compute, expected) for ws_guard.run_fills: a training step and the no-grad forward of ``net`` on ``x``"""
    from srcgan_amd import model as M
    net = net.to(DEV)
    x, t = x.to(DEV), t.to(DEV)
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    stem, cfg, infer_extra = plan(net, x)

    def compute(guard, scale):
        with torch.no_grad():                               # the same starting state for every run
            for k, v in net.state_dict().items():
                v.copy_(sd0[k])
        for p in net.parameters():
            p.grad = None
        if hasattr(net, "_pack"):
            net._pack = M._PackState()
        net.train()
        xg = (x * scale).requires_grad_(True)
        M._phase_hook = hook
        try:
            y = net(xg)
            _chk(guard)
            lv = loss(y, t)
            lv.backward()
            _chk(guard)
        finally:
            M._phase_hook = None
        res = {"y": y.detach().clone(), "loss": lv.detach().clone(), "dx": xg.grad.clone()}
        for k, p in net.named_parameters():
            res["grad/" + k] = None if p.grad is None else p.grad.clone()
        for k, b in net.named_buffers():
            res["buffer/" + k] = b.detach().clone()
        if infer:
            with torch.no_grad():
                res["y_infer"] = net(xg.detach()).clone()
            _chk(guard)
        if fold0:
            from test_gpu_infer_oplist import _resdeconv_infer
            res["y_infer_fold0"] = _resdeconv_infer(net, xg.detach(), 0).clone()
            _chk(guard)
        return res

    def expected():                                         # after the stock run: the arena holds the parameters that got a gradient
        arena = 4 * sum(p.numel() for p in net.parameters() if p.grad is not None)
        return _sizes(stem, cfg, infer_extra, infer=infer, wpack=hasattr(net, "_pack"), fold0=fold0) + [("grad_arena", arena)]

    return compute, expected


def _run(net, x, t, plan, **kw):
    compute, expected = _network_case(net, x, t, plan, **kw)
    runs = run_fills(compute, DEV, expected=expected)
    assert any(k.startswith("grad/") and v is not None for k, v in runs["stock"].items())
    return runs, compute


def _fixture_xt(g):
    return torch.from_numpy(g["x"]), torch.from_numpy(g["t"])


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ csrc/nets.hip: the RRDB generators
FAMILY = {}         # test name -> the C stems (srcgan_<stem>_ws_bytes) its cases drive; read by test_the_case_table_names_every_family


def drives(*stems):
    def mark(fn):
        FAMILY[fn.__name__] = stems
        return fn
    return mark


@drives("rddbnet")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["rddbnet_x2_w32", "rddbnet_x4"])
def test_rddbnet_fixtures(tag, dtype):
    from srcgan_amd import RDDBNet
    g = load_golden(tag)
    ic, oc, up, nf, nb, gc = [int(v) for v in g["cfg"]]
    net = RDDBNet(ic, oc, up, nf=nf, nb=nb, gc=gc, dtype=dtype)
    net.load_state_dict(sub(g, "sd/"), strict=True)
    _run(net, *_fixture_xt(g), _plan_rddb)


def _ragged(dtype):
    """in 3, out 3, x2, nf 64, gc 32, nb 2 on 3 x 3 x 5 x 7: one ragged 32 x 16 tile, and cin 64 ... 192 of the dense block at real width"""
    from srcgan_amd import RDDBNet
    net = RDDBNet(3, 3, 2, nf=64, nb=2, gc=32, dtype=dtype)
    net.load_state_dict(oracle.rddbnet_state(3, 3, 2, 64, 2, 32, seed=21), strict=True)
    return net, _rand((3, 3, 5, 7), 22), _rand((3, 3, 10, 14), 23)


@drives("rddbnet")
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_rddbnet_ragged_batch(dtype):
    _run(*_ragged(dtype), _plan_rddb)


@drives("rddbnet")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rddbnet_staged_backward(dtype):
    """the ragged case with the backward cut at every RRDB: bit-equal across fills, and to the single-phase backward"""
    net, x, t = _ragged(dtype)
    runs, _ = _run(net, x, t, _plan_rddb, hook=_EveryRrdb())
    single, _ = _network_case(net, x, t, _plan_rddb)
    assert_bit_equal({"single phase": single(None, 1.0), "staged": runs["stock"]})


@drives("rddbnet")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("down", [2, 4])
def test_rddbneta(down, dtype):
    """the configuration of test_gpu_modules.py::test_rddbneta_vs_oracle_f32, and the same with two stride-2 stages"""
    from srcgan_amd import RDDBNetA
    net = RDDBNetA(3, 3, down, nf=32, nb=1, gc=16, dtype=dtype)
    net.load_state_dict(oracle.rddbneta_state(3, 3, down, 32, 1, 16, seed=2))
    _run(net, _rand((2, 3, 24, 40), 3), _rand((2, 3, 24 // down, 40 // down), 4), _plan_rddb)


@drives("rddbnet")
@pytest.mark.parametrize("tag", ["rddbnetb_x2", "legacy_rddbnet_x1", "legacy_rddbnet_x4", "srdn_nb2"])
def test_legacy_generators_and_srdn(tag):
    from srcgan_amd import RDDBNetB, LegacyRDDBNet, SRDN
    g = load_golden(tag)
    cfg = [int(v) for v in g["cfg"]]
    if tag.startswith("srdn"):
        net = SRDN(*cfg, dtype="fp32")
    else:
        ic, oc, nf, nb, gc, up = cfg
        net = (RDDBNetB if tag.startswith("rddbnetb") else LegacyRDDBNet)(ic, oc, nf, nb, gc, f"x{up}", dtype="fp32")
    net.load_state_dict(sub(g, "sd/"), strict=True)
    runs, _ = _run(net, *_fixture_xt(g), _plan_rddb)
    assert any(v is None for k, v in runs["stock"].items() if k.startswith("grad/"))       # off-graph parameters stay None in every run


# ------------------------------------------------------------------------------------------------ csrc/nets.hip: the PatchGAN
def _patchgan(tag, dtype, norm_layer=torch.nn.BatchNorm2d):
    from srcgan_amd import NLayerDiscriminator
    g = load_golden(tag)
    ic, ndf, nl = [int(v) for v in g["cfg"]]
    net = NLayerDiscriminator(ic, ndf, nl, norm_layer=norm_layer, dtype=dtype)
    net.load_state_dict(sub(g, "sd/"), strict=True)
    x = torch.from_numpy(g["x"])
    return net, x, x.new_zeros(1)


@drives("nlayerd")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["nlayerd_2", "nlayerd_3", "ndf16_70x54"])
def test_patchgan_batchnorm(tag, dtype):
    """running_mean, running_var and num_batches_tracked are compared with everything else (the buffers of the results)"""
    from srcgan_amd import NLayerDiscriminator
    if tag == "ndf16_70x54":
        net = NLayerDiscriminator(3, 16, 3, dtype=dtype)
        net.load_state_dict(oracle.nlayer_d_state(3, 16, 3, seed=31), strict=True)
        x, t = _rand((2, 3, 70, 54), 32), torch.zeros(1)
    else:
        net, x, t = _patchgan(tag, dtype)
    runs, _ = _run(net, x, t, _plan_nlayerd, loss=_lsgan_real, infer=False)
    tracked = [k for k in runs["stock"] if k.endswith("num_batches_tracked")]
    assert tracked and all(int(runs[r][k]) >= 1 for r in runs for k in tracked)
    assert any(k.endswith("running_var") for k in runs["stock"])


@drives("nlayerd")
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_patchgan_instancenorm(dtype):
    _run(*_patchgan("nlayerd_in", dtype, torch.nn.InstanceNorm2d), _plan_nlayerd, loss=_lsgan_real, infer=False)


# ------------------------------------------------------------------------------------------------ csrc/oplist.hip
@drives("resdeconv")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["resdeconv_gray", "resdeconv_in"])
def test_resdeconv(tag, dtype):
    """training step, the module's no-grad path (fold_tail = 1) and srcgan_resdeconv_infer with fold_tail = 0"""
    from test_oracle_golden import _resdeconv_from_cfg
    g = load_golden(tag)
    _run(_resdeconv_from_cfg(g, dtype=dtype), *_fixture_xt(g), _plan_oplist, fold0=True)


@drives("srnet")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["espcn_x2", "espcn_x3", "srcnn", "edsr_x2"])
def test_small_sr_models(tag, dtype):
    from srcgan_amd import ESPCN, SRCNN, EDSR
    g = load_golden(tag)
    cfg = [int(v) for v in g["cfg"]]
    net = EDSR(*cfg, dtype=dtype) if tag.startswith("edsr") else (SRCNN if tag == "srcnn" else ESPCN)(*cfg[:3], dtype=dtype)
    net.load_state_dict(sub(g, "sd/"), strict=True)
    _run(net, *_fixture_xt(g), _plan_oplist)


@drives("srdense")
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("tag", ["srdense_a_x2", "srdense_b_x2"])
def test_srdensenet(tag, dtype):
    from test_srdense_host import build_from_fixture
    g = load_golden(tag)
    _run(build_from_fixture(g, tag, dtype=dtype)[0], *_fixture_xt(g), _plan_oplist)


@drives("rcan")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["rcan_x2", "ragged pool"])
def test_rcan(case, dtype):
    import test_gpu_rcan as T
    if case == "rcan_x2":
        z = load_golden(case)
        net, (x, t) = T.build(z, dtype), _fixture_xt(z)
    else:
        net, x, t = T._case(2, 2, 32, 8, 2, (2, 3, 5, 7), dtype, 3)
    _run(net, x, t, _plan_oplist)


@drives("ddbpn")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["ddbpn_x2", "x8 on 2x3x5x3"])
def test_ddbpn(case, dtype):
    import ddbpn_ref
    import srcgan_amd
    if case == "ddbpn_x2":
        z = load_golden(case)
        scale, seed, (x, t) = int(z["scale"]), int(z["seed"]), _fixture_xt(z)
    else:
        scale, seed = 8, 3
        x, t = _rand((2, 3, 5, 3), 4), _rand((2, 3, 40, 24), 5)
    torch.manual_seed(seed)
    net = srcgan_amd.DDBPN(scale=scale, rgb_range=1, dtype=dtype)
    ddbpn_ref.set_slopes(net, seed)
    _run(net, x, t, _plan_oplist)


# ------------------------------------------------------------------------------------------------ the VGG feature path (losses.py)
def _vgg_case(kind, dtype):
    import vgg_ref as R
    from srcgan_amd import VGG16Loss, PerceptionLoss
    from test_gpu_vgg_loss import SHAPES
    shape = min(SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3])
    sd, out, tgt = R.make_case(kind, shape, R.CASE_SEEDS.get((kind, shape), 0))
    m = VGG16Loss(weights=sd, dtype=dtype) if kind == 0 else PerceptionLoss(weights=sd, dtype=dtype).cuda()
    return m, out.to(DEV), tgt.to(DEV)


def _vgg_sizes(kind, B, H, W, dtype, times=1):
    N, lib = _lib()
    cfg = N.VggLossCfg(kind, B, H, W, N.dtype_id(dtype))
    names = ("srcgan_vggloss_ws_bytes", "srcgan_vggloss_bwd_scratch_bytes", "srcgan_vggloss_infer_ws_bytes")
    return [("workspace", int(getattr(lib, n)(C.byref(cfg)))) for n in names] * times


def _loss_compute(m, out, tgt):
    def compute(guard, scale):
        o = (out * scale).requires_grad_(True)
        lv = m(o, tgt)
        _chk(guard)
        lv.backward()
        _chk(guard)
        with torch.no_grad():
            li = m(o.detach(), tgt)
        _chk(guard)
        return {"loss": lv.detach().clone(), "dx": o.grad.clone(), "loss_no_grad": li.clone()}
    return compute


@drives("vggloss")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", [0, 1], ids=["VGG16Loss", "PerceptionLoss"])
def test_vgg_losses(kind, dtype):
    m, out, tgt = _vgg_case(kind, dtype)
    B, _, H, W = out.shape
    run_fills(_loss_compute(m, out, tgt), DEV, expected=_vgg_sizes(kind, B, H, W, dtype))


@drives("vggloss")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_vgg16loss3d_reuses_its_workspace_per_chunk(dtype):
    """F = 2 frames, one per pass: the second chunk's workspace and scratch are allocated after the first chunk's were released"""
    import vgg_ref as R
    from srcgan_amd import VGG16Loss3D
    m = VGG16Loss3D(weights=R.seeded_state(0, seed=1), dtype=dtype, frames_per_pass=1)
    out, tgt = _rand((1, 3, 2, 16, 16), 41).to(DEV), _rand((1, 3, 2, 16, 16), 42).to(DEV)
    run_fills(_loss_compute(m, out, tgt), DEV, expected=_vgg_sizes(0, 1, 16, 16, dtype, times=2))


# ------------------------------------------------------------------------------------------------ score_scene (metrics.py)
@drives("scene_score")
@pytest.mark.parametrize("form", ["u8", "f32"])
def test_score_scene(form):
    from srcgan_amd import score_scene
    from test_scene_score_host import CASES, golden_case, planes
    _, lib = _lib()
    z = load_golden("scene_score")
    name = min(CASES, key=lambda n: golden_case(z, n)[0].numel())
    pred, target, _, _ = golden_case(z, name)
    H, W, Cc = pred.shape
    p, t = (pred.to(DEV), target.to(DEV)) if form == "u8" else (planes(pred).to(DEV), planes(target).to(DEV))

    def compute(guard, scale):
        d = score_scene(p if scale == 1.0 else p.flip(-1).contiguous(), t, full=True)       # the STALE block's earlier run: another scene
        _chk(guard)
        return {k: v.clone() for k, v in d.items()}

    runs = run_fills(compute, DEV, expected=[("workspace", int(lib.srcgan_scene_score_ws_bytes(H, W, Cc)))])
    assert set(runs["NAN"]) == {"MSE", "PSNR", "AE", "SSIM", "CS"}


# ------------------------------------------------------------------------------------------------ no family arrives uncovered
def test_the_case_table_names_every_family():
    """every stem with a srcgan_<stem>_ws_bytes symbol has at least one case above"""
    from srcgan_amd import _native as N
    stems = {n[len("srcgan_"):-len("_ws_bytes")] for n in N.SIGNATURES if n.endswith("_ws_bytes") and not n.endswith("_infer_ws_bytes")}
    covered = {s for v in FAMILY.values() for s in v}
    assert stems and stems <= covered, sorted(stems - covered)
    assert all(name in globals() for name in FAMILY)
