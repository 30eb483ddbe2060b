"""GPU: the gray configurations of the cycle harness (reference src/train.py:166-180, 251-260).

1. the two fused preprocessing kernels against the composition of the existing ones, bit for bit, and against CPU F.interpolate;
2. one ``net == 'SRdens'`` step in fp32 against tests/golden/cycle_srdens.npz, which the REFERENCE's own
   ``train.SRCycleGAN.optimize_parameters`` produced (tests/golden/make_golden_cycle_gray.py) -- the first cycle step pinned by the
   reference itself rather than by the oracle's restatement;
3. the gray fallback branch (RRDB generators) runs -- parity unpinned, see the test;
4. the 'SRdens' step in bf16 against the native fp32 step;
5. the default ``net == '1'`` branch gives the losses of the pre-existing code path bit for bit.

Gates: tensors ``F32_TOL`` and losses 1e-3 (test_gpu_harness.py::test_cycle_step_vs_oracle, test_gpu_modules.py::
test_paired_step_golden_f32), gradient fingerprints as test_gpu_modules.py::test_resdeconv_golden_f32."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err
from test_cycle_gray_host import NETS, fill_by_recipe, fingerprint, nets_of, srdens_harness

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3
LOSSES = ("loss_D_A", "loss_G_A", "loss_cycle_A", "loss_iden_A", "loss_D_B", "loss_G_B", "loss_cycle_B", "loss_iden_B", "loss_G")
IMAGES = ("fake_B", "fake_A", "recl_A", "recl_B", "iden_A", "iden_B")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _cpu_gray(x):
    return 0.2125 * x[:, :1] + 0.7154 * x[:, 1:2] + 0.0721 * x[:, 2:3]                 # train.py:252


# ------------------------------------------------------------------------------------------------ 1. kernels vs composition
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("shape", [(1, 3, 8, 8), (2, 3, 12, 20), "ragged", "big"])
def test_gray_nearest_down_equals_composition(s, shape):
    """``ragged`` = (3, 3, 4s, 6s): output 4 x 6, a width that is no multiple of 4.  ``big`` = (1, 3, 736s, 720s): 529 920 output
    pixels, more than one pass of the grid covers (2048 blocks x 256), so the grid-stride loop runs more than once.  This is the
    size at which a contracted gray expression shows: the compiler's second loop version fused other products than its first, in
    ``rgb_to_gray_k`` as well, so ``sg_gray`` now forbids contraction.  Against the CPU the gate is the 1e-6 of test_gpu_kernels.py's
    preprocessing test."""
    from srcgan_amd import ops
    shape = {"ragged": (3, 3, 4 * s, 6 * s), "big": (1, 3, 736 * s, 720 * s)}.get(shape, shape)
    x = _rand(*shape, seed=s)
    xg = x.cuda().requires_grad_(True)
    y = ops.gray_nearest_down(xg, s)
    assert y.shape == (shape[0], 1, shape[2] // s, shape[3] // s) and y.dtype == torch.float32
    assert y.grad_fn is None and not y.requires_grad
    assert torch.equal(y, ops.nearest_resize(ops.rgb_to_gray(x.cuda()), 1.0 / s))
    assert rel_err(y.cpu(), F.interpolate(_cpu_gray(x), scale_factor=1.0 / s)) < 1e-6


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("shape", [(1, 1, 8, 8), (2, 1, 12, 20), (3, 1, 4, 6), (3, 1, 4, 5), (2, 1, 5, 7), "big", "big_odd"])
def test_rep3_nearest_up_equals_composition(s, shape):
    """Odd widths with s = 2 give output rows of 10, 14, ... floats, not 16-byte aligned: the scalar-store kernel; every other case
    takes the 16-byte vector stores (s = 2: two source pixels per vector, s = 4: one).  ``big`` = (1, 1, 736, 2880 / s) and
    ``big_odd`` = (1, 1, 736, 721) have more than 2048 x 256 work items in the vector and in the scalar kernel: the grid-stride loop
    runs more than once."""
    from srcgan_amd import ops
    shape = {"big": (1, 1, 736, 2880 // s), "big_odd": (1, 1, 736, 721)}.get(shape, shape)
    x = _rand(*shape, seed=10 + s)
    xg = x.cuda().requires_grad_(True)
    y = ops.rep3_nearest_up(xg, s)
    assert y.shape == (shape[0], 3, s * shape[2], s * shape[3]) and y.dtype == torch.float32
    assert y.grad_fn is None and not y.requires_grad
    assert torch.equal(y, ops.nearest_resize(torch.cat([x, x, x], 1).cuda(), s))
    assert torch.equal(y.cpu(), F.interpolate(torch.cat([x, x, x], 1), scale_factor=s))


def test_ops_take_non_contiguous_views():
    from srcgan_amd import ops
    big = _rand(2, 4, 16, 24, seed=5).cuda()
    x = big[:, 1:4, :, 4:20]
    assert torch.equal(ops.gray_nearest_down(x, 2), ops.gray_nearest_down(x.contiguous(), 2))
    a = big[:, :1, 2:9, 1:12]
    assert torch.equal(ops.rep3_nearest_up(a, 2), ops.rep3_nearest_up(a.contiguous(), 2))


# ------------------------------------------------------------------------------------------------ 2. step vs the reference's train.py
def _run_srdens(dtype):
    g = load_golden("cycle_srdens")
    m = srdens_harness("cuda", dtype)
    fill_by_recipe(nets_of(m), int(g["s"]))
    before = {n: {k: fingerprint(v) for k, v in net.state_dict().items()} for n, net in zip(NETS, nets_of(m))}
    m.optimize_parameters(torch.from_numpy(g["realA"]).cuda(), torch.from_numpy(g["realB"]).cuda())
    torch.cuda.synchronize()
    return g, m, before


@pytest.fixture(scope="module")
def step32():
    return _run_srdens("fp32")


def test_srdens_step_images_and_losses_vs_reference(step32):
    g, m, _ = step32
    assert rel_err(m.real_B_Gray.cpu(), g["real_B_Gray"]) < 1e-6
    assert torch.equal(m.real_A_RGB.cpu(), torch.from_numpy(g["real_A_RGB"]))
    for k in IMAGES:
        e = rel_err(getattr(m, k).cpu(), g[k])
        print(f"{k}: rel_err {e:.3e}")
        assert e < F32_TOL, (k, e)
    for k in LOSSES:
        mine, ref = float(getattr(m, k)), float(g[k])
        print(f"{k}: native {mine:.7f} reference {ref:.7f} (reference float64 {float(g[k + '_64']):.7f})")
        assert abs(mine - ref) < 1e-3 * max(1.0, abs(ref)), (k, mine, ref)
    assert abs(float(m.loss_D_A) + float(m.loss_D_B) - float(g["loss_D"])) < 1e-3 * max(1.0, abs(float(g["loss_D"])))


def test_srdens_step_gradients_vs_reference(step32):
    """After the step the generators' ``.grad`` is loss_G's gradient and the discriminators' is loss_D_*'s.  Full gradients of the
    small tensors at F32_TOL; every parameter's gradient fingerprint at the gates of test_resdeconv_golden_f32."""
    g, m, _ = step32
    worst = {}
    for n, net in zip(NETS, nets_of(m)):
        params = dict(net.named_parameters())
        assert list(params) == [str(k) for k in g[f"pnames/{n}"]]
        full = [k[len(f"grad/{n}/"):] for k in g if k.startswith(f"grad/{n}/")]
        assert len(full) == 6
        for k in full:
            e = rel_err(params[k].grad.cpu(), g[f"grad/{n}/{k}"])
            worst[n] = max(worst.get(n, 0.0), e)
            assert e < F32_TOL, (n, k, e)
        for k, p in params.items():
            assert p.grad is not None, (n, k)
            ref, mine = g[f"gfp/{n}/{k}"], fingerprint(p.grad)
            assert abs(mine[0] - ref[0]) <= 1e-3 * max(1.0, np.sqrt(ref[1])), (n, k, mine[0], ref[0])
            assert abs(mine[1] - ref[1]) <= 2e-3 * max(ref[1], 1e-12), (n, k, mine[1], ref[1])
    print("worst full-gradient rel_err per network", worst, "reference f32 vs f64", float(g["ref_f32_vs_f64"]))


def test_srdens_step_updates_vs_reference(step32):
    """Post-step weights and the discriminators' BatchNorm running statistics.  Each discriminator runs three times per step (once
    frozen inside backward_G, twice in backward_D_*), so ``num_batches_tracked`` is 3 and the running statistics are three updates old.

    Weight fingerprints at the gradient-fingerprint gates.  The update itself is checked through the change of each tensor's sum:
    Adam's first step moves an element by lr * g / (|g| + 1e-8), within [-lr, lr]; an element whose gradient is at rounding level may
    land on either side, moving the sum by at most 2 lr, so the two changes of the sum agree to a small fraction of lr * numel unless
    the step is missing, doubled or scaled wrongly -- gate 0.05 * lr * numel, i.e. one element in 40 on the other side."""
    g, m, before = step32
    for n, net in zip(NETS, nets_of(m)):
        lr = m.optimizer_G.param_groups[0]["lr"] if n.startswith("G_") else m.optimizer_D.param_groups[0]["lr"]
        pnames = {k for k, _ in net.named_parameters()}
        for k, v in net.state_dict().items():
            ref, mine = g[f"wfp1/{n}/{k}"], fingerprint(v)
            assert abs(mine[0] - ref[0]) <= 1e-3 * max(1.0, np.sqrt(ref[1])), (n, k, mine[0], ref[0])
            assert abs(mine[1] - ref[1]) <= 2e-3 * max(ref[1], 1e-12), (n, k, mine[1], ref[1])
            if k in pnames:
                d_mine, d_ref = mine[0] - before[n][k][0], ref[0] - g[f"wfp/{n}/{k}"][0]
                assert abs(d_mine - d_ref) <= 0.05 * lr * v.numel(), (n, k, d_mine, d_ref)
                assert not np.array_equal(mine, before[n][k]), (n, k, "parameter did not move")
        if n.startswith("D_"):
            sd = net.state_dict()
            stats = [k[len(f"bn1/{n}/"):] for k in g if k.startswith(f"bn1/{n}/")]
            assert len(stats) == 6
            for k in stats:
                if k.endswith("num_batches_tracked"):
                    assert int(sd[k]) == int(g[f"bn1/{n}/{k}"]) == 3, (n, k)
                else:
                    e = rel_err(sd[k].cpu(), g[f"bn1/{n}/{k}"])
                    assert e < F32_TOL, (n, k, e)


# ------------------------------------------------------------------------------------------------ 3. gray fallback branch
def test_gray_fallback_branch_runs():
    """``net == '0'`` (train.py:176-180): RDDBNetB(1, 3) / RDDBNetA(3, 1) and discriminators on 3 / 1 channels, small widths.
    PARITY UNPINNED: the reference ships no source for RDDBNetA, so its own train.py cannot run this branch and no fixture can come
    from it (VERDICT a10); what is checked is that the step runs, every loss is finite and every parameter on the graph gets a
    gradient -- ``upconv2`` of an x2 RDDBNetB is not on the graph and stays None, as in the reference."""
    from srcgan_amd import train as T
    losses = {}
    for lam in (1.0, 0.0):
        opt = T.CycleParams(device="cuda")
        opt.net, opt.G_A, opt.dtype, opt.lambda_identity = "0", "RDDBNetB", "fp32", lam
        opt.nf, opt.nb, opt.gc, opt.ndf = 16, 1, 8, 16
        torch.manual_seed(4)
        m = T.SRCycleGAN(opt)
        m.optimize_parameters(_rand(2, 1, 24, 20, seed=1).cuda(), _rand(2, 3, 48, 40, seed=2).cuda())
        assert m.real_B_Gray.shape == (2, 1, 24, 20) and m.real_A_RGB.shape == (2, 3, 48, 40)
        assert m.fake_B.shape == m.recl_B.shape == m.iden_A.shape == (2, 3, 48, 40)
        assert m.fake_A.shape == m.recl_A.shape == m.iden_B.shape == (2, 1, 24, 20)
        for k in LOSSES:
            assert np.isfinite(float(getattr(m, k))), (lam, k)
        for n, net in zip(NETS, nets_of(m)):
            for k, p in net.named_parameters():
                if n == "G_A" and k.startswith("upconv2."):
                    assert p.grad is None, k
                else:
                    assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (lam, n, k)
        losses[lam] = m
    assert float(losses[0.0].loss_iden_A) == 0.0 and float(losses[0.0].loss_iden_B) == 0.0
    assert float(losses[1.0].loss_iden_A) > 0.0 and float(losses[1.0].loss_iden_B) > 0.0
    # the generators see identical weights and inputs in both runs: everything in front of the first optimiser step agrees
    assert torch.equal(losses[0.0].fake_B, losses[1.0].fake_B) and torch.equal(losses[0.0].loss_cycle_A, losses[1.0].loss_cycle_A)


# ------------------------------------------------------------------------------------------------ 4. bf16
def test_srdens_step_bf16_vs_fp32(step32):
    """The same step with bf16 storage against the native fp32 step.  tests/test_gpu_trajectory.py bounds a bf16 loss curve by 6 % (L1
    losses) and 10 % (GAN and discriminator losses) of the fp32 curve; a single step is a curve of length one.  The observed figures
    are printed and recorded in DESIGN.md section 3.3."""
    _, m32, _ = step32
    _, m16, _ = _run_srdens("bf16")
    for k in LOSSES:
        a, b = float(getattr(m16, k)), float(getattr(m32, k))
        dev = abs(a - b) / abs(b)
        print(f"{k}: bf16 {a:.6f} fp32 {b:.6f} deviation {dev:.3e}")
        assert np.isfinite(a)
        assert dev < (0.06 if ("cycle" in k or "iden" in k) else 0.10), (k, a, b)


# ------------------------------------------------------------------------------------------------ 5. default branch untouched
def test_default_branch_equals_the_previous_code_path():
    """``net == '1'``: a harness built and run through a restatement of the construction and forward() that preceded the ``net`` switch
    gives the same losses bit for bit, from one seed and the same inputs (two steps: the second runs on updated weights)."""
    from srcgan_amd import ops, train as T
    from srcgan_amd.model import NLayerDiscriminator, RDDBNet, RDDBNetA
    from srcgan_amd.losses import GANLoss, L1Loss
    from srcgan_amd.optim import Adam

    class Previous(T.SRCycleGAN):
        def __init__(self, opt):
            self.opt = opt
            up = self.up = 2 if opt.mode == "x2" else 4
            dev = opt.device
            self.netG_A = RDDBNet(3, 3, up, nf=opt.nf, nb=opt.nb, gc=opt.gc, dtype=opt.dtype).to(dev)
            self.netG_B = RDDBNetA(3, 3, up, nf=opt.nf, nb=opt.nb, gc=opt.gc, dtype=opt.dtype).to(dev)
            self.netD_A = NLayerDiscriminator(3, opt.ndf, opt.n_layers, dtype=opt.dtype).to(dev)
            self.netD_B = NLayerDiscriminator(3, opt.ndf, opt.n_layers, dtype=opt.dtype).to(dev)
            self.fake_A_pool, self.fake_B_pool = T.ImagePool(opt.pool_size), T.ImagePool(opt.pool_size)
            self.criterionGAN = GANLoss("lsgan", device=dev)
            self.criterionCycle, self.criterionIdt = L1Loss(), L1Loss()
            self.optimizer_G = Adam(itertools.chain(self.netG_A.parameters(), self.netG_B.parameters()), lr=opt.lr, betas=(opt.beta1, 0.999))
            self.optimizer_D = Adam(itertools.chain(self.netD_A.parameters(), self.netD_B.parameters()), lr=1e-5, betas=(opt.beta1, 0.999))

        def forward(self, realA, realB):
            self.real_A, self.real_B = realA, realB
            self.fake_B = self.netG_A(self.real_A)
            self.recl_A = self.netG_B(self.fake_B)
            self.fake_A = self.netG_B(self.real_B)
            self.recl_B = self.netG_A(self.fake_A)
            self.real_B_Gray = ops.nearest_resize(self.real_B, 1.0 / self.up)
            self.iden_A = self.netG_A(self.real_B_Gray)
            self.real_A_RGB = ops.nearest_resize(self.real_A, self.up)
            self.iden_B = self.netG_B(self.real_A_RGB)

    runs = []
    for cls in (T.SRCycleGAN, Previous):
        opt = T.CycleParams(device="cuda")
        assert opt.net == "1"
        opt.nf, opt.nb, opt.gc, opt.ndf, opt.dtype = 16, 1, 8, 16, "fp32"
        torch.manual_seed(3)
        m = cls(opt)
        out = []
        for step in range(2):
            m.optimize_parameters(_rand(2, 3, 24, 20, seed=20 + step).cuda(), _rand(2, 3, 48, 40, seed=30 + step).cuda())
            out += [getattr(m, k).detach().clone() for k in LOSSES] + [m.iden_A.detach().clone(), m.iden_B.detach().clone()]
        runs.append((m, out))
    (new, a), (old, b) = runs
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    for na, nb in zip(nets_of(new), nets_of(old)):
        assert all(torch.equal(u, v) for u, v in zip(na.state_dict().values(), nb.state_dict().values()))
