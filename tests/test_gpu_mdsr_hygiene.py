"""GPU: the MDSR and VDSR drivers (csrc/oplist.hip, mdsr_plan / vdsr_plan) on poisoned, guarded workspaces -- the cases
tests/test_gpu_workspace_hygiene.py would hold for these families, with that file's machinery: forward + L1 loss + backward and the
no_grad forward (``srcgan_<stem>_infer``) on stock allocation and on guarded workspaces, gradient arenas and packs filled with zeros, with
NaN and with the bytes a run on -3 x left behind.  Results are bit-equal and finite across the four runs, the guards stay intact, and
the allocations recorded are the planners' answers (``_ws_bytes``, ``_bwd_scratch_bytes``, ``_infer_ws_bytes``, one gradient arena).

MDSR runs at two scale_idx of one scale list: the gradient arena holds the parameters of the branch on the graph and nothing of the
others (their gradient stays None in all four runs), and the planners answer for that branch alone.

That file's last test wants every family with a ``srcgan_<stem>_ws_bytes`` symbol to have a case in its table; the cases below enter
themselves there (``drives``), which they can do only where both files are collected -- as they are in a run of the suite."""
import pytest
import torch

import test_gpu_workspace_hygiene as H

pytestmark = pytest.mark.gpu
SCALES = (2, 3, 4)


def _plan_mdsr(net, x):
    from srcgan_amd import model as M, _native as N
    return "mdsr", M._mdsr_cfg(x, (net.n_resblocks, net.n_feats, tuple(net.scale), int(net.scale_idx), N.dtype_id(net.compute_dtype)))[0], ()


def _plan_vdsr(net, x):
    from srcgan_amd import model as M, _native as N
    return "vdsr", M._vdsr_cfg(x, (net.n_resblocks, net.n_feats, N.dtype_id(net.compute_dtype)))[0], ()


@H.drives("mdsr")
def mdsr_hygiene_case(dtype, idx):
    import srcgan_amd
    torch.manual_seed(3)
    net = srcgan_amd.MDSR(n_resblocks=2, n_feats=64, scale=SCALES, rgb_range=1, dtype=dtype)
    net.set_scale(idx)
    s = SCALES[idx]
    x, t = H._rand((2, 3, 8, 6), 4), H._rand((2, 3, 8 * s, 6 * s), 5)
    runs, _ = H._run(net, x, t, _plan_mdsr)
    on = {k for k, _ in net.named_parameters() if "mean" not in k and not any(k.startswith(f"{part}.{j}.") for part in ("pre_process", "upsample")
                                                                                  for j in range(3) if j != idx)}
    for name, run in runs.items():
        assert {k[5:] for k, v in run.items() if k.startswith("grad/") and v is not None} == on, name
    return runs


@H.drives("vdsr")
def vdsr_hygiene_case(dtype):
    import srcgan_amd
    torch.manual_seed(3)
    net = srcgan_amd.VDSR(n_resblocks=4, n_feats=64, rgb_range=1, dtype=dtype)
    x, t = H._rand((2, 3, 8, 6), 4), H._rand((2, 3, 8, 6), 5)
    runs, _ = H._run(net, x, t, _plan_vdsr)
    assert all((runs["stock"]["grad/" + k] is not None) == p.requires_grad for k, p in net.named_parameters())
    return runs


H.mdsr_hygiene_case, H.vdsr_hygiene_case = mdsr_hygiene_case, vdsr_hygiene_case         # the table's names are looked up in that module


@pytest.mark.parametrize("idx", [0, 2])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_mdsr(dtype, idx):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    mdsr_hygiene_case(dtype, idx)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_vdsr(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    vdsr_hygiene_case(dtype)
