"""Host (no GPU): the gray configurations of the cycle harness (reference src/train.py:166-180, 251-260) -- which classes and channel
counts ``SRCycleGAN`` builds for ``net == 'SRdens'`` and for the gray fallback, that the default stays ``net == '1'``, that the
parameter holders' key order and the weight recipe of tests/golden/make_golden_cycle_gray.py reproduce the fixture's fingerprints
(tests/golden/cycle_srdens.npz, made by the REFERENCE's own train.SRCycleGAN), the refusals of the two preprocessing ops and of
the harness, and the checkpoint names of train.py:407-408.

``fill_by_recipe`` / ``fingerprint`` restate the fixture script's recipe; tests/test_gpu_cycle_gray.py imports them from here."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import load_golden

NETS = ("G_A", "G_B", "D_A", "D_B")


def nets_of(m):
    return (m.netG_A, m.netG_B, m.netD_A, m.netD_B)


def fingerprint(t):
    t = t.detach().double().reshape(-1).cpu()
    return np.array([float(t.sum()), float((t * t).sum()), *[float(v) for v in t[:4]]])


def fill_by_recipe(nets, seed):
    """torch.manual_seed(seed); nets in the given order, each in state_dict() order: 0.05 * randn(shape), a BatchNorm weight
    1 + 0.05 * randn(shape); running statistics and num_batches_tracked untouched.  The values are drawn on the CPU."""
    torch.manual_seed(seed)
    for net in nets:
        for key, t in net.state_dict().items():
            leaf = key.rsplit(".", 1)[-1]
            if leaf in ("running_mean", "running_var", "num_batches_tracked"):
                continue
            owner = net.get_submodule(key.rsplit(".", 1)[0]) if "." in key else net
            v = 0.05 * torch.randn(tuple(t.shape))
            if isinstance(owner, nn.BatchNorm2d) and leaf == "weight":
                v = 1.0 + v
            with torch.no_grad():
                t.copy_(v)


def srdens_harness(device, dtype="fp32"):
    from srcgan_amd import train as T
    opt = T.CycleParams(device=device)
    opt.net, opt.dtype = "SRdens", dtype
    return T.SRCycleGAN(opt)


@pytest.fixture(scope="module")
def g():
    return load_golden("cycle_srdens")


@pytest.fixture(scope="module")
def srdens_cpu():
    return srdens_harness("cpu")


def test_defaults_keep_the_three_channel_branch():
    from srcgan_amd import train as T
    opt = T.CycleParams(device="cpu")
    assert opt.net == "1"
    assert (opt.num_blocks, opt.num_layers, opt.ndf, opt.n_layers) == (2, 2, 64, 2)


def test_srdens_branch_builds_the_reference_classes(srdens_cpu):
    from srcgan_amd import SRDenseNetA, SRDenseNetB, NLayerDiscriminator
    m = srdens_cpu
    assert type(m.netG_A) is SRDenseNetA and type(m.netG_B) is SRDenseNetB
    assert type(m.netD_A) is NLayerDiscriminator and type(m.netD_B) is NLayerDiscriminator
    # (kind, in, out, growth, num_blocks, num_layers, up)
    assert m.netG_A._cfg == (0, 1, 3, 16, 2, 2, 2) and m.netG_B._cfg == (1, 3, 1, 16, 2, 2, 2)
    assert m.netD_A._cfg == (3, 64, 2) and m.netD_B._cfg == (1, 64, 2)
    assert m.netG_A.conv_first.in_channels == 1 and m.netG_A.conv_last.out_channels == 3
    assert m.netG_B.conv_first.in_channels == 3 and m.netG_B.conv_last.out_channels == 1
    assert all(n.compute_dtype == "fp32" for n in nets_of(m))
    # the two Adam optimisers as in the '1' branch: generators lr, discriminators 1e-5, betas (0.5, 0.999)
    assert m.optimizer_G.param_groups[0]["lr"] == 1e-4 and m.optimizer_D.param_groups[0]["lr"] == 1e-5
    assert m.optimizer_G.param_groups[0]["betas"] == m.optimizer_D.param_groups[0]["betas"] == (0.5, 0.999)
    n_g = sum(1 for _ in m.netG_A.parameters()) + sum(1 for _ in m.netG_B.parameters())
    assert len(m.optimizer_G.param_groups[0]["params"]) == n_g


def test_srdens_dtype_and_depth_are_passed_through():
    from srcgan_amd import train as T
    opt = T.CycleParams(device="cpu")
    opt.net, opt.dtype, opt.num_blocks, opt.num_layers, opt.ndf, opt.mode = "SRdens", "bf16", 1, 4, 16, "x4"
    m = T.SRCycleGAN(opt)
    assert m.netG_A._cfg == (0, 1, 3, 16, 1, 4, 4) and m.netG_B._cfg == (1, 3, 1, 16, 1, 4, 4)
    assert m.netD_A._cfg == (3, 16, 2) and m.netD_B._cfg == (1, 16, 2)
    assert all(n.compute_dtype == "bf16" for n in nets_of(m))


@pytest.mark.parametrize("g_a", ["RDDBNetB", "RDDBNet"])
def test_gray_fallback_branch_builds_the_rrdb_generators(g_a):
    """train.py:176-180 (any other ``net``): RDDBNetB(1, 3, 64, nb=3, mode) / RDDBNetA(3, 1, 64, nb=3, mode) and the two
    discriminators on 3 and 1 channels; G_A follows the existing ``opt.G_A`` switch."""
    from srcgan_amd import train as T, RDDBNet, RDDBNetA, RDDBNetB, NLayerDiscriminator
    opt = T.CycleParams(device="cpu")
    opt.net, opt.G_A = "0", g_a
    m = T.SRCycleGAN(opt)
    assert type(m.netG_A) is (RDDBNetB if g_a == "RDDBNetB" else RDDBNet) and type(m.netG_B) is RDDBNetA
    assert type(m.netD_A) is NLayerDiscriminator and type(m.netD_B) is NLayerDiscriminator
    assert tuple(m.netG_A.conv_first.weight.shape) == (64, 1, 3, 3) and m.netG_A.conv_last.weight.shape[0] == 3
    assert m.netG_B.conv_first.weight.shape[1] == 3 and m.netG_B.conv_last.weight.shape[0] == 1
    assert sum(1 for k in m.netG_A.state_dict() if k.startswith("RRDB_trunk.") and k.endswith("RDB1.conv1.weight")) == 3
    assert m.netD_A._cfg == (3, 64, 2) and m.netD_B._cfg == (1, 64, 2)


def test_default_branch_channels_unchanged():
    from srcgan_amd import train as T, RDDBNet, RDDBNetA
    opt = T.CycleParams(device="cpu")
    opt.nf, opt.nb, opt.gc, opt.ndf = 16, 1, 8, 16
    m = T.SRCycleGAN(opt)
    assert type(m.netG_A) is RDDBNet and type(m.netG_B) is RDDBNetA
    assert m.netG_A.conv_first.weight.shape[1] == 3 and m.netG_B.conv_last.weight.shape[0] == 3
    assert m.netD_A._cfg == (3, 16, 2) and m.netD_B._cfg == (3, 16, 2)


def test_state_dict_keys_equal_the_fixture(g, srdens_cpu):
    for n, net in zip(NETS, nets_of(srdens_cpu)):
        assert list(net.state_dict()) == [str(k) for k in g[f"keys/{n}"]], n
        assert [k for k, _ in net.named_parameters()] == [str(k) for k in g[f"pnames/{n}"]], n


def test_fill_recipe_reproduces_the_fixture_weights(g, srdens_cpu):
    """The same float32 values: the first four bit for bit; the two sums are float64 sums of up to 6e5 equal values whose order
    depends on the thread count, so they may differ by 6e5 * 2^-53 = 7e-11 of the sum of magnitudes -- gate 1e-9."""
    fill_by_recipe(nets_of(srdens_cpu), int(g["s"]))
    for n, net in zip(NETS, nets_of(srdens_cpu)):
        for k, v in net.state_dict().items():
            mine, ref = fingerprint(v), g[f"wfp/{n}/{k}"]
            assert np.array_equal(mine[2:], ref[2:]), (n, k)
            assert abs(mine[0] - ref[0]) <= 1e-9 * max(1.0, float(v.double().abs().sum())), (n, k)
            assert abs(mine[1] - ref[1]) <= 1e-9 * max(ref[1], 1e-300), (n, k)


def test_fixture_seed_condition_and_contents(g):
    assert 0.0 <= float(g["ref_f32_vs_f64"]) <= 1e-4
    assert g["realA"].shape == (2, 1, 24, 20) and g["realB"].shape == (2, 3, 48, 40)
    assert g["real_B_Gray"].shape == g["realA"].shape and g["real_A_RGB"].shape == g["realB"].shape
    for n in ("D_A", "D_B"):
        assert int(g[f"bn1/{n}/model.3.num_batches_tracked"]) == int(g[f"bn1/{n}/model.6.num_batches_tracked"]) == 3
    assert float(g["loss_D"]) == pytest.approx(float(g["loss_D_A"]) + float(g["loss_D_B"]))


@pytest.mark.parametrize("s", [0, 1, 3, 8, -2, 2.0, "2", True])
def test_ops_refuse_other_scales(s):
    from srcgan_amd import ops
    with pytest.raises(ValueError, match="s must be 2 or 4"):
        ops.gray_nearest_down(torch.zeros(1, 3, 8, 8), s)
    with pytest.raises(ValueError, match="s must be 2 or 4"):
        ops.rep3_nearest_up(torch.zeros(1, 1, 8, 8), s)


def test_ops_refuse_bad_shapes():
    from srcgan_amd import ops
    for bad in (torch.zeros(1, 1, 8, 8), torch.zeros(3, 8, 8), torch.zeros(1, 4, 8, 8)):
        with pytest.raises(ValueError, match=r"expects \[B,3,H,W\]"):
            ops.gray_nearest_down(bad, 2)
    for bad in (torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8)):
        with pytest.raises(ValueError, match=r"expects \[B,1,H,W\]"):
            ops.rep3_nearest_up(bad, 2)
    with pytest.raises(ValueError, match="must divide H and W"):
        ops.gray_nearest_down(torch.zeros(1, 3, 8, 6), 4)
    with pytest.raises(ValueError, match="must divide H and W"):
        ops.gray_nearest_down(torch.zeros(1, 3, 7, 8), 2)
    # well-formed arguments on the CPU: no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gray_nearest_down(torch.zeros(1, 3, 8, 8), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rep3_nearest_up(torch.zeros(1, 1, 4, 4), 2)


@pytest.mark.parametrize("a,b", [((2, 3, 8, 8), (2, 3, 16, 16)), ((2, 1, 8, 8), (2, 1, 16, 16)), ((2, 1, 8, 8), (2, 3, 16, 12)),
                                 ((2, 1, 8, 8), (1, 3, 16, 16)), ((2, 1, 8, 8), (2, 3, 32, 32))])
def test_gray_harness_refuses_other_shapes_naming_both(srdens_cpu, a, b):
    with pytest.raises(ValueError) as e:
        srdens_cpu.forward(torch.zeros(*a), torch.zeros(*b))
    assert str(a) in str(e.value) and str(b) in str(e.value)


def test_cycle_checkpoint_names_round_trip(tmp_path, srdens_cpu):
    from srcgan_amd import data as D
    assert D.cycle_checkpoint_name("A2B", "x2", 5) == "netG_A2B_SRtask_x2_0005.pth"
    assert D.cycle_checkpoint_name("B2A", "x4", 125) == "netG_B2A_SRtask_x4_0125.pth"
    for direction in ("A2B", "B2A"):
        for mode in ("x2", "x4"):
            for epoch in (0, 5, 9999):
                name = D.cycle_checkpoint_name(direction, mode, epoch)
                assert D.parse_cycle_checkpoint_name(os.path.join("./checkpoints", name)) == (direction, mode, epoch)
    for bad in ("netG_A2C_SRtask_x2_0005.pth", "netG_A2B_x2_0005.pth", "RDDBNet_A2C_x2_0025.pth", "netG_A2B_SRtask_x3_0005.pth",
                "netG_A2B_SRtask_x2_last.pth"):
        with pytest.raises(ValueError):
            D.parse_cycle_checkpoint_name(bad)
    with pytest.raises(ValueError):
        D.cycle_checkpoint_name("A2C", "x2", 1)
    with pytest.raises(ValueError):
        D.parse_checkpoint_name("netG_A2B_SRtask_x2_0005.pth")       # the cascade parser does not read the cycle's names
    pa, pb = D.save_cycle_checkpoints(srdens_cpu, srdens_cpu.opt, 5, root=str(tmp_path))
    assert (os.path.basename(pa), os.path.basename(pb)) == ("netG_A2B_SRtask_x2_0005.pth", "netG_B2A_SRtask_x2_0005.pth")
    for path, net in ((pa, srdens_cpu.netG_A), (pb, srdens_cpu.netG_B)):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        assert list(sd) == list(net.state_dict())
        assert all(torch.equal(sd[k], v) for k, v in net.state_dict().items())
