"""GPU: the UnetGenerator driver (csrc/oplist.hip, unet_plan) on poisoned, guarded workspaces -- the case
tests/test_gpu_workspace_hygiene.py would hold for this family, with that file's machinery: forward + L1 loss + backward and the
no_grad forward (``srcgan_unet_infer``) on stock allocation and on guarded workspaces, gradient arenas and packs filled with zeros,
with NaN and with the bytes a run on -3 x left behind.  Results are bit-equal and finite across the four runs, the guards stay intact,
and the allocations recorded are the planners' answers (``_ws_bytes``, ``_bwd_scratch_bytes``, ``_infer_ws_bytes``, one gradient arena).

The skip buffers are written by halves, by two different ops: a half nobody wrote, or a padded channel of the 3-channel output the four
parity launches leave out, would show as NaN or as a stale value.  Five levels on 32 x 64 (1 x 2 at the bottom) and six on 64 x 64.

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
    return "unet", M._unet_cfg(x, (*net._cfg, N.dtype_id(net.compute_dtype)))[0], ()


@H.drives("unet")
def unet_hygiene_case(dtype, n, shape):
    import srcgan_amd
    torch.manual_seed(3)
    norm = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
    net = srcgan_amd.UnetGenerator(shape[1], 3, n, 16, norm_layer=norm, dtype=dtype)
    x, t = H._rand(shape, 4), H._rand((shape[0], 3, *shape[2:]), 5)
    runs, _ = H._run(net, x, t, _plan)
    assert all(runs["stock"]["grad/" + k] is not None for k, _ in net.named_parameters())
    return runs


H.unet_hygiene_case = unet_hygiene_case         # the table's names are looked up in that module


@pytest.mark.parametrize("n, shape", [(5, (2, 1, 32, 64)), (6, (1, 3, 64, 64))])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_unet(dtype, n, shape):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    unet_hygiene_case(dtype, n, shape)
