"""GPU: the RDN driver (csrc/oplist.hip, rdn_plan) on poisoned, guarded workspaces -- the case tests/test_gpu_workspace_hygiene.py would
hold for this family, with that file's machinery: forward + L1 loss + backward and the no_grad forward of 'A' x2 at 2x3x8x6 on stock
allocation and on guarded workspaces, gradient arenas and packs filled with zeros, with NaN and with the bytes a run on -3 x left behind.
Results are bit-equal and finite across the four runs, the guards stay intact, and the allocations recorded are the planners' answers
(srcgan_rdn_ws_bytes, _bwd_scratch_bytes, _infer_ws_bytes, one gradient arena).

That file's last test wants every family with a ``srcgan_<stem>_ws_bytes`` symbol to have a case in its table; the case below enters
itself there (``drives("rdn")``), which it can do only where both files are collected -- as they are in a run of the suite."""
import pytest
import torch

import test_gpu_workspace_hygiene as H

pytestmark = pytest.mark.gpu


def _plan_rdn(net, x):
    from srcgan_amd import model as M, _native as N
    return "rdn", M._rdn_cfg(x, (*net._cfg, N.dtype_id(net.compute_dtype)))[0], ()


@H.drives("rdn")
def rdn_hygiene_case(dtype):
    import srcgan_amd
    torch.manual_seed(3)
    net = srcgan_amd.RDN(scale=2, G0=64, RDNconfig="A", dtype=dtype)
    x, t = H._rand((2, 3, 8, 6), 4), H._rand((2, 3, 16, 12), 5)
    runs, _ = H._run(net, x, t, _plan_rdn)
    assert all(runs["stock"]["grad/" + k] is not None for k, _ in net.named_parameters())
    return runs


H.rdn_hygiene_case = rdn_hygiene_case         # the table's names are looked up in that module


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rdn(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rdn_hygiene_case(dtype)
