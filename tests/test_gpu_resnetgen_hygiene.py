"""GPU: the ResnetGenerator driver (csrc/oplist.hip, resnetgen_plan) on poisoned, guarded workspaces -- the case
tests/test_gpu_workspace_hygiene.py would hold for this family, with that file's machinery: forward + L1 loss + backward and the
no_grad forward (``srcgan_resnetgen_infer``) on stock allocation and on guarded workspaces, gradient arenas and packs filled with zeros,
with NaN and with the bytes a run on -3 x left behind.  Results are bit-equal and finite across the four runs, the guards stay intact,
and the allocations recorded are the planners' answers (``_ws_bytes``, ``_bwd_scratch_bytes``, ``_infer_ws_bytes``, one gradient arena).

Both padding types run: 'reflect' materialises its padded tensors (their borders are written by the pad kernel alone, so a stale or NaN
border would show), 'zero' leaves them out.

That file's last test wants every family with a ``srcgan_<stem>_ws_bytes`` symbol to have a case in its table; the case below enters
itself there (``drives``), which it can do only where both files are collected -- as they are in a run of the suite."""
import functools

import pytest
import torch
import torch.nn as nn

import test_gpu_workspace_hygiene as H

pytestmark = pytest.mark.gpu


def _plan(net, x):
    from srcgan_amd import model as M, _native as N
    return "resnetgen", M._resnetgen_cfg(x, (*net._cfg, N.dtype_id(net.compute_dtype)))[0], ()


@H.drives("resnetgen")
def resnetgen_hygiene_case(dtype, padding):
    import srcgan_amd
    torch.manual_seed(3)
    norm = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
    net = srcgan_amd.ResnetGenerator(1, 3, 16, norm_layer=norm, n_blocks=2, padding_type=padding, dtype=dtype)
    x, t = H._rand((2, 1, 12, 8), 4), H._rand((2, 3, 12, 8), 5)
    runs, _ = H._run(net, x, t, _plan)
    assert all(runs["stock"]["grad/" + k] is not None for k, _ in net.named_parameters())
    return runs


H.resnetgen_hygiene_case = resnetgen_hygiene_case         # the table's names are looked up in that module


@pytest.mark.parametrize("padding", ["reflect", "zero"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_resnetgen(dtype, padding):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    resnetgen_hygiene_case(dtype, padding)
