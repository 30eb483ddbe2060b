"""GPU: the generators' inference path (forward under ``torch.no_grad()`` -> srcgan_rddbnet_infer on the rolling workspace).
It launches the kernels of the training forward in the same order, so its claim is BIT equality with the grad-mode forward; on
its own it must meet the fp32 gate against the reference's goldens, give its workspace back, and follow weight updates."""
import ctypes as C

import pytest
import torch

from conftest import load_golden, sub, rel_err

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3
MIB = 1 << 20


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


def _make(kind, dtype, **kw):
    import srcgan_amd as S
    torch.manual_seed(11)
    nf, gc, nb = kw.get("nf", 64), kw.get("gc", 32), kw.get("nb", 1)
    if kind == "rddbnet":
        net = S.RDDBNet(3, 3, kw["up"], nf=nf, nb=nb, gc=gc, dtype=dtype)
    elif kind == "rddbneta":
        net = S.RDDBNetA(3, 3, kw["down"], nf=nf, nb=nb, gc=gc, dtype=dtype)
    elif kind == "rddbnetb":
        net = S.RDDBNetB(3, 3, nf, nb, gc, f"x{kw['up']}", dtype=dtype)
    elif kind == "legacy":
        net = S.LegacyRDDBNet(3, 3, nf, nb, gc, f"x{kw['up']}", dtype=dtype)
    else:
        net = S.SRDN(3, 3, 1, nf=nf, nb=nb, gc=gc, dtype=dtype)
    return net.cuda()


CASES = [("rddbnet", dict(up=1, nb=1)), ("rddbnet", dict(up=2, nb=3)), ("rddbnet", dict(up=4, nb=1)), ("rddbnet", dict(up=4, nb=3)),
         ("rddbnet", dict(up=2, nb=3, nf=16, gc=8)), ("rddbnet", dict(up=4, nb=1, nf=16, gc=8)),
         ("rddbneta", dict(down=2, nb=3)), ("rddbneta", dict(down=4, nb=1, nf=16, gc=8)),
         ("rddbnetb", dict(up=2, nb=1)), ("rddbnetb", dict(up=4, nb=3)),
         ("legacy", dict(up=1, nb=1)), ("legacy", dict(up=2, nb=1)), ("legacy", dict(up=4, nb=3)),
         ("srdn", dict(nb=1)), ("srdn", dict(nb=3)), ("srdn", dict(nb=3, nf=16, gc=8))]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("kind,kw", CASES, ids=[f"{k}-" + "-".join(f"{a}{b}" for a, b in v.items()) for k, v in CASES])
def test_inference_equals_the_training_forward_bit_for_bit(kind, kw, dtype):
    net = _make(kind, dtype, **kw)
    torch.manual_seed(5)
    hw = (20, 36) if kind == "rddbneta" else (19, 35)          # RDDBNetA wants H, W divisible by its down factor
    x = torch.rand(2, 3, *hw, device="cuda")
    yi, yt = _both(net, x)
    assert yi.shape == yt.shape and torch.isfinite(yi).all()
    assert torch.equal(yi, yt)
    # a second pass over warm buffers, and an input that requires grad, change nothing
    with torch.no_grad():
        assert torch.equal(net(x.clone().requires_grad_(True)), yt)


def test_inference_of_an_empty_batch():
    net = _make("rddbnet", "fp32", up=2)
    x = torch.rand(0, 3, 8, 12, device="cuda")
    yi, yt = _both(net, x)
    assert yi.shape == yt.shape == (0, 3, 16, 24)


def test_eval_mode_plays_no_part():
    net = _make("rddbnet", "bf16", up=2, nb=1)
    x = torch.rand(1, 3, 16, 16, device="cuda")
    y = net(x).detach()
    net.eval()
    assert net(x).grad_fn is not None                      # eval() alone keeps the autograd path
    with torch.no_grad():
        assert torch.equal(net(x), y)
    net.train()
    with torch.no_grad():
        assert torch.equal(net(x), y)


@pytest.mark.parametrize("tag", ["rddbnet_x2", "rddbnet_x4", "rddbnet_x2_w32"])
def test_rddbnet_goldens_under_no_grad(tag):
    from srcgan_amd import RDDBNet
    g = load_golden(tag)
    ic, oc, up, nf, nb, gc = [int(v) for v in g["cfg"]]
    net = RDDBNet(ic, oc, up, nf=nf, nb=nb, gc=gc, dtype="fp32")
    net.load_state_dict(sub(g, "sd/"), strict=True)
    with torch.no_grad():
        y = net.cuda()(torch.from_numpy(g["x"]).cuda())
    assert rel_err(y.cpu(), g["y"]) < F32_TOL


@pytest.mark.parametrize("tag,kind", [("rddbnetb_x2", "B"), ("rddbnetb_x4", "B"), ("legacy_rddbnet_x1", "L"),
                                      ("legacy_rddbnet_x2", "L"), ("legacy_rddbnet_x4", "L")])
def test_legacy_goldens_under_no_grad(tag, kind):
    from srcgan_amd import RDDBNetB, LegacyRDDBNet
    g = load_golden(tag)
    ic, oc, nf, nb, gc, up = [int(v) for v in g["cfg"]]
    net = (RDDBNetB if kind == "B" else LegacyRDDBNet)(ic, oc, nf, nb, gc, f"x{up}", dtype="fp32")
    net.load_state_dict(sub(g, "sd/"), strict=True)
    with torch.no_grad():
        y = net.cuda()(torch.from_numpy(g["x"]).cuda())
    assert rel_err(y.cpu(), g["y"]) < F32_TOL


@pytest.mark.parametrize("tag", ["srdn_nb1", "srdn_nb2"])
def test_srdn_goldens_under_no_grad(tag):
    from srcgan_amd import SRDN
    g = load_golden(tag)
    net = SRDN(*[int(v) for v in g["cfg"]], dtype="fp32")
    net.load_state_dict(sub(g, "sd/"), strict=True)
    with torch.no_grad():
        y = net.cuda()(torch.from_numpy(g["x"]).cuda())
    assert rel_err(y.cpu(), g["y"]) < F32_TOL


def test_inference_workspace_is_what_the_planner_says_and_is_given_back():
    """nb = 23, bf16, B = 2, 128 x 128 -> x4: the training workspace is ~1 GB here, the inference workspace ~0.2 GB."""
    from srcgan_amd import _native as N
    net = _make("rddbnet", "bf16", up=4, nb=23)
    x = torch.rand(2, 3, 128, 128, device="cuda")
    with torch.no_grad():
        y = net(x)                                          # first call: the persistent weight pack and its tables are made here
    ybytes = y.numel() * 4
    del y
    cfg = N.RddbCfg(3, 3, 4, 64, 23, 32, 2, 128, 128, N.BF16, 0, 0)
    infer = N.lib().srcgan_rddbnet_infer_ws_bytes(C.byref(cfg))
    train = N.lib().srcgan_rddbnet_ws_bytes(C.byref(cfg))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        y = net(x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    after = torch.cuda.memory_allocated() - before
    print(f"peak {peak / MIB:.1f} MiB, planner: inference {infer / MIB:.1f} MiB, training {train / MIB:.1f} MiB, y {ybytes / MIB:.1f} MiB")
    assert peak <= infer + ybytes + MIB
    assert after <= ybytes + 512 and after >= ybytes        # the caching allocator rounds a block to 512 bytes
    assert infer < train / 3


def test_inference_follows_weight_updates():
    """The inference path shares the persistent weight pack and its guard words with the training forward: whatever changes the
    weights between two calls, each call computes with the weights of its moment."""
    net = _make("rddbnet", "bf16", up=2, nb=2)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    x = torch.rand(2, 3, 24, 24, device="cuda")

    def infer():
        with torch.no_grad():
            return net(x)

    y0 = net(x)
    assert torch.equal(infer(), y0.detach())
    w = net.RRDB_trunk[1].RDB2.conv3.weight
    w.data.mul_(0.5)
    y1 = infer()
    assert not torch.equal(y1, y0.detach())
    assert torch.equal(y1, net(x).detach())
    y0.abs().mean().backward()                               # gradients at the first weights: any non-trivial update will do
    opt.step()
    y2 = infer()
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, net(x).detach())
    assert torch.equal(infer(), y2)


def test_scene_sized_pass():
    """1 x 3 x 1024 x 1024 -> 4096 x 4096 at nb = 23, bf16: the inference pass equals the grad-mode forward (whose 32.4 GB
    workspace fits on the card) bit for bit, on 4.5 GB."""
    net = _make("rddbnet", "bf16", up=4, nb=23)
    torch.manual_seed(9)
    x = torch.rand(1, 3, 1024, 1024, device="cuda")
    with torch.no_grad():
        yi = net(x)
    torch.cuda.synchronize()
    yt = net(x).detach()
    assert yi.shape == (1, 3, 4096, 4096) and torch.isfinite(yi).all()
    assert torch.equal(yi, yt)
