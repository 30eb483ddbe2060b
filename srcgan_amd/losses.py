"""Loss modules of the hot path with the reference's class names and call signatures.

  L1Loss / MSELoss / PSNRLoss  <- reference src/losses.py:95-105,123-133,136-147
  GANLoss                      <- reference src/train.py:67-128 (only 'lsgan' is ever constructed, :186)
  DSSIMLoss                    <- reference src/losses.py:170-180 (on SSIM, :20-93)
  VGG16Loss / PerceptionLoss   <- reference src/losses.py:344-393, 455-470 (frozen VGG16 / VGG19 features; weights come from the caller)
  NearestSelector              <- reference src/losses.py:199-255 (shift search + crops); NearestL1Loss = its use with L1Loss (:522), fused
  L1Loss3D / DSSIMLoss3D / VGG16Loss3D <- reference src/losses.py:107-120, 183-196, 396-453 (means over the frames of [nb,ch,frame,row,col])
  CELoss / ConLoss / CrossLoss / FLoss <- reference src/losses.py:150-167, 258-274, 277-293, 296-341

Each forward is one native two-stage reduction (wavefront shuffles + fixed-order final sum,
elementwise.hip) returning a 0-dim device tensor; backward is one fused elementwise kernel
(sign(a-b)/N or 2(a-b)/N times the upstream gradient read from device memory -> no host sync).
DSSIMLoss reuses the SSIM metric's range and tile kernels plus one fold for its forward; its backward is one fused
stencil pass (metrics.hip, dssim_bwd_k) that recomputes the window statistics per output tile.
The perceptual losses run a frozen VGG feature extractor on the op-list executor (oplist.hip, srcgan_vggloss_*): one native forward
over both branches and one native backward that carries input gradients only.
The shift search (shift_select.hip) reads both tensors once, accumulates every candidate offset in registers and leaves the selection on
the device; NearestL1Loss takes its value from the search and never materialises a crop.
The multi-frame losses read and write the 5-D layout in place: DSSIMLoss3D runs the SSIM kernels with a frame dimension in the grid and one
dynamic range per frame, VGG16Loss3D packs chunks of frames as images straight from the 5-D tensor and runs each chunk's backward at once.
Their native entry points (srcgan_dssim3d_*, srcgan_vggloss_*_frames) also serve the 4-D classes, for which a tensor is one frame.
The classification-style losses (class_losses.hip) are one pass over their inputs forward and one backward each: the focal loss takes
its powers by multiplication (integer gamma) or from the logarithms of its own formula, the multi-class cross-entropy finds the target's
arg-max while it reads it, ConLoss recomputes the extreme samples in its backward, CrossLoss addresses the shifted target in place.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import torch
import torch.nn as nn

from . import _native as N

__all__ = ["L1Loss", "MSELoss", "PSNRLoss", "GANLoss", "DSSIMLoss", "VGG16Loss", "PerceptionLoss", "NearestSelector", "NearestL1Loss",
           "L1Loss3D", "DSSIMLoss3D", "VGG16Loss3D", "FLoss", "CELoss", "ConLoss", "CrossLoss"]

_K_L1, _K_MSE, _K_LABEL, _K_BCE, _K_SIGNED = 0, 1, 2, 3, 4       # srcgan_loss_fwd kinds; >= 2: scalar label instead of a target tensor


def _as_f32(t: torch.Tensor, what: str) -> torch.Tensor:
    N.require_cuda(t, what)
    return t.detach().contiguous().float()


class _MeanLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, label, a, b):
        lib = N.lib()
        a32 = _as_f32(a, "loss input")
        b32 = None
        if kind < _K_LABEL:
            if b.shape != a.shape:
                raise ValueError(f"loss: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
            b32 = _as_f32(b, "loss target")
        out = torch.empty((), dtype=torch.float32, device=a.device)
        scratch = torch.empty(lib.srcgan_loss_scratch_floats(), dtype=torch.float32, device=a.device)
        N.check(lib.srcgan_loss_fwd(kind, a32.data_ptr(), None if b32 is None else b32.data_ptr(), float(label),
                                    a32.numel(), out.data_ptr(), scratch.data_ptr(), N.stream_ptr(a.device)), "srcgan_loss_fwd")
        ctx.kind, ctx.label = kind, float(label)
        ctx.save_for_backward(a32, b32 if b32 is not None else a32.new_empty(0))
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = N.lib()
        a32, b32 = ctx.saved_tensors
        has_b = ctx.kind < _K_LABEL
        gout = gout.contiguous().float()
        da = db = None
        st = N.stream_ptr(a32.device)
        if ctx.needs_input_grad[2]:
            da = torch.empty_like(a32)
            N.check(lib.srcgan_loss_bwd(ctx.kind, a32.data_ptr(), b32.data_ptr() if has_b else None, ctx.label, a32.numel(),
                                        gout.data_ptr(), 1.0, da.data_ptr(), st), "srcgan_loss_bwd")
        if has_b and ctx.needs_input_grad[3]:
            db = torch.empty_like(b32)
            N.check(lib.srcgan_loss_bwd(ctx.kind, a32.data_ptr(), b32.data_ptr(), ctx.label, a32.numel(),
                                        gout.data_ptr(), -1.0, db.data_ptr(), st), "srcgan_loss_bwd")
        return None, None, da, db


class _DSSIMFn(torch.autograd.Function):
    """DSSIM of [B,C,H,W] (one frame) or [B,C,F,H,W] tensors; the gradients come back in the input's own shape."""

    @staticmethod
    def forward(ctx, output, target):
        lib = N.lib()
        p32, t32 = _as_f32(output, "DSSIM loss output"), _as_f32(target, "DSSIM loss target")
        B, Cc, H, W = p32.shape[0], p32.shape[1], p32.shape[-2], p32.shape[-1]
        Fr = p32.shape[2] if p32.dim() == 5 else 1
        dev = p32.device
        nfl = lib.srcgan_dssim3d_scratch_floats(B, Cc, Fr, H, W)
        if nfl <= 0:
            raise RuntimeError(f"srcgan_amd: srcgan_dssim3d_scratch_floats refused the shape {tuple(p32.shape)}")
        out = torch.empty((), dtype=torch.float32, device=dev)
        rng = torch.empty((Fr, 2), dtype=torch.float32, device=dev)
        scratch = torch.empty(nfl, dtype=torch.float32, device=dev)
        N.check(lib.srcgan_dssim3d_loss_fwd(p32.data_ptr(), t32.data_ptr(), B, Cc, Fr, H, W, out.data_ptr(), rng.data_ptr(),
                                            scratch.data_ptr(), N.stream_ptr(dev)), "srcgan_dssim3d_loss_fwd")
        ctx.dims = (B, Cc, Fr, H, W)
        ctx.dtypes = (output.dtype, target.dtype)
        ctx.save_for_backward(p32, t32, rng)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = N.lib()
        p32, t32, rng = ctx.saved_tensors
        gout = gout.contiguous().float()
        dp = torch.empty_like(p32)                       # the kernel always produces the output's gradient
        dt = torch.empty_like(t32) if ctx.needs_input_grad[1] else None
        N.check(lib.srcgan_dssim3d_loss_bwd(p32.data_ptr(), t32.data_ptr(), *ctx.dims, rng.data_ptr(), gout.data_ptr(),
                                            dp.data_ptr(), None if dt is None else dt.data_ptr(), N.stream_ptr(p32.device)),
                "srcgan_dssim3d_loss_bwd")
        dp = dp.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None
        return dp, None if dt is None else dt.to(ctx.dtypes[1])


def _check_5d(name, output, target):
    if output.dim() != 5 or target.dim() != 5 or output.shape != target.shape:
        raise ValueError(f"{name}: expected two [nb,ch,frame,row,col] tensors of one shape, got {tuple(output.shape)} and {tuple(target.shape)}")
    if output.numel() == 0:
        raise ValueError(f"{name}: empty input {tuple(output.shape)}")


class L1Loss(nn.Module):
    """mean |output - target| (losses.py:95-105)."""

    def __repr__(self):
        return "L1"

    def forward(self, output, target):
        return _MeanLossFn.apply(_K_L1, 0.0, output, target)


class MSELoss(nn.Module):
    """mean (output - target)^2 (losses.py:123-133)."""

    def __repr__(self):
        return "MSE"

    def forward(self, output, target):
        return _MeanLossFn.apply(_K_MSE, 0.0, output, target)


class PSNRLoss(nn.Module):
    """10*log10(1/mse), peak 1.0 (losses.py:136-147).  Validation metric: no gradient."""

    def __repr__(self):
        return "PSNR"

    def forward(self, output, target):
        lib = N.lib()
        mse = _MeanLossFn.apply(_K_MSE, 0.0, output.detach(), target.detach())
        out = torch.empty_like(mse)
        N.check(lib.srcgan_psnr_from_mse(mse.data_ptr(), out.data_ptr(), N.stream_ptr(mse.device)), "srcgan_psnr_from_mse")
        return out


class GANLoss(nn.Module):
    """GAN objective with the reference's interface (train.py:67-128): 'lsgan' = MSE against the scalar label (the only mode a
    reference script constructs, train.py:186), 'vanilla' = BCE-with-logits against it, 'wgangp' = -mean(prediction) for real,
    +mean for fake.  The label is folded into the reduction kernel as an immediate instead of ``expand_as``.  'DSSIM' (the
    reference wires ``losses.DSSIMLoss`` there) is outside the native path and refused."""

    _KINDS = {"lsgan": _K_LABEL, "vanilla": _K_BCE, "wgangp": _K_SIGNED}

    def __init__(self, gan_mode, device=None, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        self.register_buffer("real_label", torch.tensor(target_real_label, device=device))
        self.register_buffer("fake_label", torch.tensor(target_fake_label, device=device))
        self._real, self._fake = float(target_real_label), float(target_fake_label)
        self.gan_mode = gan_mode
        if gan_mode not in self._KINDS:
            if gan_mode == "DSSIM":
                raise NotImplementedError("gan mode DSSIM is outside the native hot path (no reference script selects it)")
            raise NotImplementedError("gan mode %s not implemented" % gan_mode)

    def get_target_tensor(self, prediction, target_is_real):
        return (self.real_label if target_is_real else self.fake_label).expand_as(prediction)

    def forward(self, prediction, target_is_real):
        kind = self._KINDS[self.gan_mode]
        if kind == _K_SIGNED:
            return _MeanLossFn.apply(kind, -1.0 if target_is_real else 1.0, prediction, None)
        return _MeanLossFn.apply(kind, self._real if target_is_real else self._fake, prediction, None)


class DSSIMLoss(nn.Module):
    """(1 - SSIM(output, target)) / 2 (losses.py:170-180): the SSIM of ``metrics.SSIM`` (11x11 gaussian sigma 1.5 "valid"
    depth-wise windows, dynamic range from the prediction), averaged over every window position of every image and channel.
    Inputs are [B,C,H,W] CUDA tensors with H, W >= 11 (other float dtypes compute in f32); the gradient reaches the target only
    when it requires one.  Returns a 0-dim f32 device tensor; forward and backward never synchronise with the host."""

    def __repr__(self):
        return "DSSIM"

    def forward(self, output, target):
        if output.dim() != 4 or target.dim() != 4 or output.shape != target.shape:
            raise ValueError(f"DSSIMLoss: expected two [B,C,H,W] tensors of one shape, got {tuple(output.shape)} and {tuple(target.shape)}")
        if output.shape[2] < 11 or output.shape[3] < 11:
            raise ValueError(f"DSSIMLoss: images must be at least 11x11 (valid 11x11 windows), got {tuple(output.shape)}")
        N.require_cuda(output, "DSSIMLoss output")
        N.require_cuda(target, "DSSIMLoss target")
        return _DSSIMFn.apply(output, target)


class L1Loss3D(nn.Module):
    """Mean over the frames of ``[nb,ch,frame,row,col]`` inputs of the per-frame L1 mean (losses.py:107-120).  Every frame has the same
    element count, so the mean of the per-frame means is the mean over the whole tensor: this is ``L1Loss``'s reduction and backward
    kernel (``srcgan_loss_fwd`` / ``_bwd``, kind L1) on the flat 5-D tensor -- no frame loop, no slice copies, no new kernel."""

    def __repr__(self):
        return "L13D"

    def forward(self, output, target):
        _check_5d("L1Loss3D", output, target)
        N.require_cuda(output, "L1Loss3D output")
        N.require_cuda(target, "L1Loss3D target")
        return _MeanLossFn.apply(_K_L1, 0.0, output, target)


class DSSIMLoss3D(nn.Module):
    """Mean over the frames f of ``DSSIMLoss(output[:, :, f], target[:, :, f])`` (losses.py:183-196) in one autograd Function.  Like the
    reference's loop, every frame takes the dynamic range of its own prediction (min / max over that frame of the whole batch), so a
    stack that mixes 0..1, 0..255 and -1..1 frames is not the 2-D loss of the frames folded into the batch.  Inputs are
    [nb,ch,frame,row,col] CUDA tensors with row, col >= 11 (other float dtypes compute in f32); the kernels address the 5-D layout
    directly (one range launch, one SSIM launch and one fused backward pass for all frames, no per-frame copy).  The gradient reaches
    the target only when it requires one.  Returns a 0-dim f32 device tensor; forward and backward never synchronise with the host.
    The gradient of frame f has the bits of ``DSSIMLoss`` on that frame at upstream ``gout * (1 / frame)``."""

    def __repr__(self):
        return "DSSIM3D"

    def forward(self, output, target):
        _check_5d("DSSIMLoss3D", output, target)
        if output.shape[3] < 11 or output.shape[4] < 11:
            raise ValueError(f"DSSIMLoss3D: frames must be at least 11x11 (valid 11x11 windows), got {tuple(output.shape)}")
        N.require_cuda(output, "DSSIMLoss3D output")
        N.require_cuda(target, "DSSIMLoss3D target")
        return _DSSIMFn.apply(output, target)


# ------------------------------------------------------------------------------------------------ classification-style losses
def _check_pair(name, output, target, min_dim=2, dims=None, min_batch=1):
    """Shape, emptiness and frozen-target checks of the two-tensor class losses, then the device check."""
    ok = output.dim() == target.dim() and output.shape == target.shape and (output.dim() == dims if dims else output.dim() >= min_dim)
    if not ok:
        want = f"{dims}-D" if dims else f"at least {min_dim}-D"
        raise ValueError(f"{name}: expected two {want} tensors of one shape, got {tuple(output.shape)} and {tuple(target.shape)}")
    if output.numel() == 0:
        raise ValueError(f"{name}: empty input {tuple(output.shape)}")
    if output.shape[0] < min_batch:
        raise ValueError(f"{name}: needs at least two samples (sample b is compared with sample b+1), got {tuple(output.shape)}")
    if target.requires_grad:
        raise ValueError(f"{name}: the native backward produces the output's gradient only: detach the target")
    N.require_cuda(output, f"{name} output")
    N.require_cuda(target, f"{name} target")


def _loss_buffers(dev):
    return (torch.empty((), dtype=torch.float32, device=dev),
            torch.empty(N.lib().srcgan_loss_scratch_floats(), dtype=torch.float32, device=dev))


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, gamma, mean):
        lib = N.lib()
        o32, t32 = _as_f32(output, "FLoss output"), _as_f32(target, "FLoss target")
        out, scratch = _loss_buffers(o32.device)
        ctx.cfg = (int(o32.shape[1] == 1), float(gamma), int(bool(mean)))
        N.check(lib.srcgan_focal_fwd(o32.data_ptr(), t32.data_ptr(), o32.numel(), *ctx.cfg, out.data_ptr(), scratch.data_ptr(),
                                     N.stream_ptr(o32.device)), "srcgan_focal_fwd")
        ctx.in_dtype = output.dtype
        ctx.save_for_backward(o32, t32)
        return out

    @staticmethod
    def backward(ctx, gout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        o32, t32 = ctx.saved_tensors
        gout = gout.contiguous().float()
        do = torch.empty_like(o32)
        N.check(N.lib().srcgan_focal_bwd(o32.data_ptr(), t32.data_ptr(), o32.numel(), *ctx.cfg, gout.data_ptr(), do.data_ptr(),
                                         N.stream_ptr(o32.device)), "srcgan_focal_bwd")
        return do.to(ctx.in_dtype), None, None, None


class _CEFn(torch.autograd.Function):
    @staticmethod
    def _dims(o32):
        n, c = int(o32.shape[0]), int(o32.shape[1])
        return n, c, o32.numel() // (n * c)

    @staticmethod
    def forward(ctx, output, target):
        lib = N.lib()
        o32, t32 = _as_f32(output, "CELoss output"), _as_f32(target, "CELoss target")
        out, scratch = _loss_buffers(o32.device)
        st = N.stream_ptr(o32.device)
        if o32.shape[1] == 1:
            N.check(lib.srcgan_bce_fwd(o32.data_ptr(), t32.data_ptr(), o32.numel(), out.data_ptr(), scratch.data_ptr(), st), "srcgan_bce_fwd")
        else:
            N.check(lib.srcgan_nll_argmax_fwd(o32.data_ptr(), t32.data_ptr(), *_CEFn._dims(o32), out.data_ptr(), scratch.data_ptr(), st),
                    "srcgan_nll_argmax_fwd")
        ctx.in_dtype = output.dtype
        ctx.save_for_backward(o32, t32)
        return out

    @staticmethod
    def backward(ctx, gout):
        if not ctx.needs_input_grad[0]:
            return None, None
        lib = N.lib()
        o32, t32 = ctx.saved_tensors
        gout = gout.contiguous().float()
        do = torch.empty_like(o32)
        st = N.stream_ptr(o32.device)
        if o32.shape[1] == 1:
            N.check(lib.srcgan_bce_bwd(o32.data_ptr(), t32.data_ptr(), o32.numel(), gout.data_ptr(), do.data_ptr(), st), "srcgan_bce_bwd")
        else:
            N.check(lib.srcgan_nll_argmax_bwd(o32.data_ptr(), t32.data_ptr(), *_CEFn._dims(o32), gout.data_ptr(), do.data_ptr(), st),
                    "srcgan_nll_argmax_bwd")
        return do.to(ctx.in_dtype), None


class _ConFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats):
        f32 = _as_f32(feats, "ConLoss feats")
        out, scratch = _loss_buffers(f32.device)
        nb = int(f32.shape[0])
        N.check(N.lib().srcgan_batch_range_fwd(f32.data_ptr(), nb, f32.numel() // nb, out.data_ptr(), scratch.data_ptr(),
                                               N.stream_ptr(f32.device)), "srcgan_batch_range_fwd")
        ctx.in_dtype = feats.dtype
        ctx.save_for_backward(f32)
        return out

    @staticmethod
    def backward(ctx, gout):
        f32, = ctx.saved_tensors
        gout = gout.contiguous().float()
        df = torch.empty_like(f32)
        nb = int(f32.shape[0])
        N.check(N.lib().srcgan_batch_range_bwd(f32.data_ptr(), nb, f32.numel() // nb, gout.data_ptr(), df.data_ptr(),
                                               N.stream_ptr(f32.device)), "srcgan_batch_range_bwd")
        return df.to(ctx.in_dtype)


class _CrossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target):
        o32, t32 = _as_f32(output, "CrossLoss output"), _as_f32(target, "CrossLoss target")
        out, scratch = _loss_buffers(o32.device)
        nb = int(o32.shape[0])
        N.check(N.lib().srcgan_cross_l1_fwd(o32.data_ptr(), t32.data_ptr(), nb, o32.numel() // nb, out.data_ptr(), scratch.data_ptr(),
                                            N.stream_ptr(o32.device)), "srcgan_cross_l1_fwd")
        ctx.in_dtype = output.dtype
        ctx.save_for_backward(o32, t32)
        return out

    @staticmethod
    def backward(ctx, gout):
        if not ctx.needs_input_grad[0]:
            return None, None
        o32, t32 = ctx.saved_tensors
        gout = gout.contiguous().float()
        do = torch.empty_like(o32)
        nb = int(o32.shape[0])
        N.check(N.lib().srcgan_cross_l1_bwd(o32.data_ptr(), t32.data_ptr(), nb, o32.numel() // nb, gout.data_ptr(), do.data_ptr(),
                                            N.stream_ptr(o32.device)), "srcgan_cross_l1_bwd")
        return do.to(ctx.in_dtype), None


class FLoss(nn.Module):
    """Focal loss (losses.py:296-341), ``FLoss(gamma=2., weight=None, size_average=True)``; ``weight`` is stored and unused, as in the
    reference.  With o = clamp(output, 1e-6, 1 - 1e-6) (float32 bounds): ``target.shape[1] == 1`` selects the binary form
    ``-0.9 (1-o)^gamma t log o - 0.1 o^gamma (1-t) log(1-o)`` (alpha = 0.1), anything else ``-(1-o)^gamma t log o``; the mean (or, with
    ``size_average=False``, the sum) runs over every element, channels included.  Inputs: two CUDA tensors of one shape, at least 2-D
    (other float dtypes compute in f32).  One pass forward, one backward (srcgan_focal_*); the gradient reaches ``output`` only, is
    clamp's (zero outside [1e-6, 1 - 1e-6], bounds included), and a target that requires grad is refused."""

    def __init__(self, gamma=2., weight=None, size_average=True):
        super().__init__()
        self.gamma = gamma
        self.weight = weight
        self.size_average = size_average

    def __repr__(self):
        return "Focal"

    def forward(self, output, target):
        _check_pair("FLoss", output, target)
        return _FocalFn.apply(output, target, self.gamma, self.size_average)


class CELoss(nn.Module):
    """Cross-entropy (losses.py:150-167).  ``target.shape[1] == 1``: ``nn.BCELoss`` (mean, logarithms clamped at -100) between two tensors
    (srcgan_bce_*).  Otherwise ``nn.NLLLoss(log(output), argmax(target, dim=1))``: the mean over the batch and spatial positions of
    ``-log output[n, k, s]`` at the first maximum k of the target's channels (srcgan_nll_argmax_*, one pass over both tensors; no index
    tensor, no log tensor).  Inputs: two CUDA tensors of one shape, at least 2-D.  The gradient reaches ``output`` only; a target that
    requires grad is refused.  Outputs outside [0, 1] give NaN (the reference asserts on the host instead)."""

    def __repr__(self):
        return "CE"

    def forward(self, output, target):
        _check_pair("CELoss", output, target)
        return _CEFn.apply(output, target)


class ConLoss(nn.Module):
    """Consistency of the samples within a batch (losses.py:258-274): the mean over the positions of ``(max_b feats - min_b feats)^2``.
    ``forward(feats)``: a CUDA tensor of any dimension >= 1, the batch first.  The gradient goes to the first maximum's and the first
    minimum's sample of every position (lowest batch index on ties, as the reference on the CPU); srcgan_batch_range_* recompute the
    indices in the backward and keep no index tensor."""

    def __repr__(self):
        return "ConLoss"

    def forward(self, feats):
        if feats.dim() < 1:
            raise ValueError(f"ConLoss: expected a tensor with a batch dimension, got {tuple(feats.shape)}")
        if feats.numel() == 0:
            raise ValueError(f"ConLoss: empty input {tuple(feats.shape)}")
        N.require_cuda(feats, "ConLoss feats")
        return _ConFn.apply(feats)


class CrossLoss(nn.Module):
    """Cross comparison between the samples of a batch (losses.py:277-293): ``L1Loss(output[:nb-1], target[1:])`` on [nb,ch,row,col] CUDA
    tensors of one shape, without the two slice copies (srcgan_cross_l1_*; any ch*row*col, whatever the alignment of ``target[1]``).
    The gradient reaches ``output`` only (zeros for the last sample); a target that requires grad is refused.

    Deviation from the reference: ``nb == 1`` is a ``ValueError`` here; the reference takes the mean of an empty tensor and returns NaN."""

    def __repr__(self):
        return "CrossLoss"

    def forward(self, output, target):
        _check_pair("CrossLoss", output, target, dims=4, min_batch=2)
        return _CrossFn.apply(output, target)


# ------------------------------------------------------------------------------------------------ shift-tolerant pixel loss
def _shift_check(name, output, target, shift, stride, crop=None):
    """Shape checks of the shift search, before any launch -> (B, C, H, W, crop_h, crop_w)."""
    if not (isinstance(shift, int) and isinstance(stride, int) and shift >= 1 and stride >= 1):
        raise ValueError(f"{name}: shift and stride must be integers >= 1, got shift={shift!r} stride={stride!r}")
    if output.dim() != 4 or target.dim() != 4 or output.shape != target.shape:
        raise ValueError(f"{name}: expected two [B,C,H,W] tensors of one shape, got {tuple(output.shape)} and {tuple(target.shape)}")
    B, Cc, H, W = (int(v) for v in output.shape)
    ch, cw = (H - 2 * shift * stride, W - 2 * shift * stride) if crop is None else (int(crop[0]), int(crop[1]))
    if ch < 1 or cw < 1 or B < 1 or Cc < 1:
        raise ValueError(f"{name}: empty crop {ch} x {cw} of a {tuple(output.shape)} tensor (shift={shift}, stride={stride})")
    if (2 * shift - 1) * stride + ch > H or (2 * shift - 1) * stride + cw > W:
        raise ValueError(f"{name}: the shifted {ch} x {cw} crops leave the {H} x {W} image (shift={shift}, stride={stride})")
    N.require_cuda(output, f"{name} output")
    N.require_cuda(target, f"{name} target")
    return B, Cc, H, W, ch, cw


def _shift_search(o32, t32, dims, shift, stride, want_loss):
    """srcgan_shift_search on contiguous f32 tensors -> (diff [B,n*n] f32, sel [B,2] int32, loss or None), all on the device."""
    lib = N.lib()
    B, Cc, H, W, ch, cw = dims
    dev = o32.device
    nfl = lib.srcgan_shift_search_scratch_floats(B, Cc, H, W, shift, stride, ch, cw)
    if nfl == 0:
        N.check(1, "srcgan_shift_search")
    scratch = torch.empty(nfl, dtype=torch.float32, device=dev)
    diff = torch.empty((B, 4 * shift * shift), dtype=torch.float32, device=dev)
    sel = torch.empty((B, 2), dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
    N.check(lib.srcgan_shift_search(o32.data_ptr(), t32.data_ptr(), B, Cc, H, W, shift, stride, ch, cw, diff.data_ptr(), sel.data_ptr(),
                                    None if loss is None else loss.data_ptr(), scratch.data_ptr(), N.stream_ptr(dev)), "srcgan_shift_search")
    return diff, sel, loss


class NearestSelector(object):
    """Shift search of the reference (losses.py:199-255), ``NearestSelector(shift=2, stride=1, criter='l1')``: per sample, the centre
    crop of ``output`` is compared with ``target`` shifted by each of ``(2*shift)**2`` offsets ``(i*stride, j*stride)`` and the offset of
    the smallest L1 sum is kept.  ``crop(output, target)`` -> ``(output_, target_)``: ``output_`` is the autograd slice view
    ``output[:, :, sd:sd+ch, sd:sd+cw]`` (sd = shift*stride, ch = H - 2 sd, cw = W - 2 sd), ``target_`` the f32 copy of each sample's best
    window, detached like the reference's search.  ``shift_diff`` returns the ``[B, (2*shift)**2]`` f32 sums.  [B,C,H,W] CUDA tensors
    (other float dtypes compute in f32); shift <= 4.

    Deviations from the reference, all deliberate:
      * ``unravel_index`` uses integer (floor) division.  The reference writes ``index / cols``, which is true division on current
        torch, so its ``crop`` raises ``TypeError: only integer tensors of a single element can be converted to an index``.
      * the target window's column extent is ``cw``; the reference writes ``crop_row`` there (losses.py:254), equal for square images and
        a shape error otherwise.
      * the selection is never read on the host: the search, the selection and the copy of the window are device work
        (shift_select.hip), so ``crop`` does not synchronise."""

    def __init__(self, shift=2, stride=1, criter='l1'):
        self.shift = shift
        self.stride = stride
        self.criter = criter

    def __repr__(self):
        return "NS"

    @staticmethod
    def unravel_index(tensor, cols):
        """[nb, rows*cols] -> [nb, 2] int64 (row, column) of each row's first minimum."""
        index = torch.argmin(tensor, dim=1).view(-1, 1)
        return torch.cat([index // cols, index % cols], dim=1)

    def shift_diff(self, output, target, crop_row, crop_col):
        dims = _shift_check("NearestSelector", output, target, self.shift, self.stride, (crop_row, crop_col))
        return _shift_search(_as_f32(output, "NearestSelector output"), _as_f32(target, "NearestSelector target"), dims, self.shift,
                             self.stride, False)[0]

    def crop(self, output, target):
        dims = _shift_check("NearestSelector", output, target, self.shift, self.stride)
        B, Cc, H, W, ch, cw = dims
        lib = N.lib()
        t32 = _as_f32(target, "NearestSelector target")
        _, sel, _ = _shift_search(_as_f32(output, "NearestSelector output"), t32, dims, self.shift, self.stride, False)
        target_ = torch.empty((B, Cc, ch, cw), dtype=torch.float32, device=t32.device)
        N.check(lib.srcgan_shift_gather(t32.data_ptr(), sel.data_ptr(), B, Cc, H, W, self.shift, self.stride, ch, cw, target_.data_ptr(),
                                        N.stream_ptr(t32.device)), "srcgan_shift_gather")
        sd = self.shift * self.stride
        return output[:, :, sd:sd + ch, sd:sd + cw], target_


class _NearestL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, shift, stride, dims):
        o32, t32 = _as_f32(output, "NearestL1Loss output"), _as_f32(target, "NearestL1Loss target")
        _, sel, loss = _shift_search(o32, t32, dims, shift, stride, True)
        ctx.cfg = (shift, stride, dims)
        ctx.dtypes = (output.dtype, target.dtype)
        ctx.save_for_backward(o32, t32, sel)
        return loss

    @staticmethod
    def backward(ctx, gout):
        lib = N.lib()
        o32, t32, sel = ctx.saved_tensors
        shift, stride, (B, Cc, H, W, ch, cw) = ctx.cfg
        gout = gout.contiguous().float()
        do = torch.empty_like(o32)                       # the kernel always produces the output's gradient
        dt = torch.empty_like(t32) if ctx.needs_input_grad[1] else None
        N.check(lib.srcgan_shift_l1_bwd(o32.data_ptr(), t32.data_ptr(), sel.data_ptr(), B, Cc, H, W, shift, stride, ch, cw, gout.data_ptr(),
                                        do.data_ptr(), None if dt is None else dt.data_ptr(), N.stream_ptr(o32.device)), "srcgan_shift_l1_bwd")
        do = do.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None
        return do, None if dt is None else dt.to(ctx.dtypes[1]), None, None, None


class NearestL1Loss(nn.Module):
    """``L1Loss()(*NearestSelector(shift, stride).crop(output, target))`` (losses.py:522) in one autograd Function: the forward is the
    shift search itself (the loss is the sum of the per-sample minima over B*C*ch*cw), the backward one kernel that writes the full-size
    gradients; no crop is materialised.  As in ``NearestSelector.crop`` the selection carries no gradient; the gradient reaches the
    target (at each sample's selected window) only when the target requires one.  Returns a 0-dim f32 device tensor; forward and
    backward never synchronise with the host."""

    def __init__(self, shift=2, stride=1):
        super().__init__()
        self.shift = shift
        self.stride = stride

    def __repr__(self):
        return "NSL1"

    def forward(self, output, target):
        dims = _shift_check("NearestL1Loss", output, target, self.shift, self.stride)
        return _NearestL1Fn.apply(output, target, self.shift, self.stride, dims)


# ------------------------------------------------------------------------------------------------ perceptual losses
# torchvision's `features` layouts: 'M' = MaxPool2d(2, 2), a number = Conv2d(., n, 3, padding=1) followed by ReLU(inplace=True)
_VGG16_FEATURES = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512)                                  # features[0:23]
_VGG19_FEATURES = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512)     # features[0:36]
_VGG16_SLICES = ((0, 4), (4, 9), (9, 16), (16, 23))       # losses.py:354-361


def _vgg_layers(layout):
    """[(features index, module)] of a torchvision VGG `features` layout."""
    out, cin = [], 3
    for v in layout:
        if v == "M":
            out.append((len(out), nn.MaxPool2d(kernel_size=2, stride=2)))
        else:
            out.append((len(out), nn.Conv2d(cin, v, kernel_size=3, padding=1)))
            out.append((len(out), nn.ReLU(inplace=True)))
            cin = v
    return out


def _load_vgg_weights(module, weights, rename):
    """``weights``: a state dict under the module's own keys or torchvision's ``features.N.*`` keys (anything else in it, such as
    the classifier, is ignored), or a local path to one saved with ``torch.save``."""
    if isinstance(weights, (str, os.PathLike)):
        weights = torch.load(os.fspath(weights), map_location="cpu")
    if not hasattr(weights, "items"):
        raise TypeError(f"{type(module).__name__}: weights must be a state dict or a local path to one, got {type(weights).__name__}")
    own = module.state_dict()
    picked = {}
    for k, v in weights.items():
        k = k if k in own else rename.get(k)
        if k in own:
            picked[k] = v
    missing = [k for k in own if k not in picked]
    if missing:
        raise KeyError(f"{type(module).__name__}: weights lack {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    module.load_state_dict(picked)


def _vgg_infer(kind, dtype, o32, t32, nb, Fr, f0, k, params, out):
    """The no-grad loss of frames [f0, f0 + k) of two f32 [nb, C, Fr, H, W] tensors (a [nb, C, H, W] tensor is Fr = 1) -> ``out``."""
    lib = N.lib()
    cfg = N.VggLossCfg(kind, nb * k, o32.shape[-2], o32.shape[-1], dtype)
    ws = N.workspace(lib.srcgan_vggloss_infer_ws_bytes(C.byref(cfg)), o32.device)
    N.check(lib.srcgan_vggloss_infer_frames(C.byref(cfg), o32.data_ptr(), t32.data_ptr(), o32.shape[1], Fr, f0, k, params, ws.data_ptr(),
                                            out.data_ptr(), N.stream_ptr(o32.device)), "srcgan_vggloss_infer_frames")


class _VggLossFn(torch.autograd.Function):
    """One native forward over both branches and one native backward w.r.t. ``output``; the parameters are frozen."""

    @staticmethod
    def forward(ctx, output, target, kind, dtype, plist):
        lib = N.lib()
        o32, t32 = _as_f32(output, "perceptual loss output"), _as_f32(target, "perceptual loss target")
        B, _, H, W = o32.shape
        cfg = N.VggLossCfg(kind, B, H, W, dtype)
        ws = N.workspace(lib.srcgan_vggloss_ws_bytes(C.byref(cfg)), o32.device)
        out = torch.empty((), dtype=torch.float32, device=o32.device)
        N.check(lib.srcgan_vggloss_forward_frames(C.byref(cfg), o32.data_ptr(), t32.data_ptr(), 3, 1, 0, 1, N.ptr_array(plist), ws.data_ptr(),
                                                  out.data_ptr(), N.stream_ptr(o32.device)), "srcgan_vggloss_forward_frames")
        ctx.cfg, ctx.ws, ctx.plist, ctx.in_dtype = cfg, ws, plist, output.dtype
        return out

    @staticmethod
    def backward(ctx, gout):
        lib, cfg = N.lib(), ctx.cfg
        if ctx.ws is None:
            raise RuntimeError("perceptual loss: backward called a second time (the workspace of the forward is released by the first)")
        gout = gout.contiguous().float()
        dev = ctx.ws.device
        scratch = N.workspace(lib.srcgan_vggloss_bwd_scratch_bytes(C.byref(cfg)), dev)
        dout = torch.empty((cfg.B, 3, cfg.H, cfg.W), dtype=torch.float32, device=dev)
        N.check(lib.srcgan_vggloss_backward_frames(C.byref(cfg), gout.data_ptr(), 1.0, 3, 1, 0, 1, N.ptr_array(ctx.plist), ctx.ws.data_ptr(),
                                                   scratch.data_ptr(), dout.data_ptr(), N.stream_ptr(dev)), "srcgan_vggloss_backward_frames")
        ctx.ws = None
        return dout.to(ctx.in_dtype), None, None, None, None


class _VggLossBase(nn.Module):
    _kind = 0

    def _init_weights(self, weights, rename):
        for p in self.parameters():
            p.requires_grad = False
        if weights is None:
            warnings.warn(f"{type(self).__name__}: no weights given -- the feature extractor keeps its seeded default initialisation. Nothing is "
                          "downloaded here: pass weights= (a torchvision VGG state dict or a local path to one) for the pretrained loss.", stacklevel=3)
        else:
            _load_vgg_weights(self, weights, rename)

    def _checked_params(self, name, output, target):
        """The channel, frozen-target and device checks of a forward (after its shape checks) -> the parameter list."""
        if output.shape[1] not in (1, 3):
            raise ValueError(f"{name}: inputs must have 1 or 3 channels, got {output.shape[1]}")
        if target.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f"{name}: the target branch is frozen (it keeps no activations): detach the target")
        N.require_cuda(output, f"{name} output")
        N.require_cuda(target, f"{name} target")
        plist = tuple(p.detach() for p in self.parameters())
        for p in plist:
            if p.device != output.device or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"{name}: parameters must be contiguous float32 tensors on {output.device} (move the loss with .to(device))")
        return plist

    def forward(self, output, target):
        name = type(self).__name__
        if output.dim() != 4 or target.dim() != 4 or output.shape != target.shape:
            raise ValueError(f"{name}: expected two [B,C,H,W] tensors of one shape, got {tuple(output.shape)} and {tuple(target.shape)}")
        plist = self._checked_params(name, output, target)
        if output.shape[1] == 1:       # losses.py:378-380: autograd sums the three gradients
            output = torch.cat([output, output, output], dim=1)
            target = torch.cat([target, target, target], dim=1)
        if torch.is_grad_enabled() and output.requires_grad:
            return _VggLossFn.apply(output, target, self._kind, self._dtype, plist)
        o32, t32 = _as_f32(output, f"{name} output"), _as_f32(target, f"{name} target")
        out = torch.empty((), dtype=torch.float32, device=o32.device)
        _vgg_infer(self._kind, self._dtype, o32, t32, o32.shape[0], 1, 0, 1, N.ptr_array(plist), out)
        return out


class VGG16Loss(_VggLossBase):
    """Mean over relu1_2, relu2_2, relu3_3, relu4_3 of the L1 distance between the VGG16 features of ``output`` and ``target``
    (losses.py:344-393).  ``VGG16Loss(requires_grad=False, cuda=True, *, weights=None, dtype=None)``; the parameters are frozen
    ``nn.Parameter``s under the reference's keys (``slice1.0.weight`` ... ``slice4.21.bias``), so a checkpoint of the reference loss
    loads with ``load_state_dict``.  ``weights``: that state dict, torchvision's ``vgg16`` state dict (``features.N.*``), or a local
    path to either; nothing is downloaded, and without weights the seeded default initialisation stays (with a warning).
    ``forward(output, target)``: [B,1|3,H,W] CUDA tensors, H, W >= 8 -> 0-dim f32 device tensor; the gradient reaches ``output`` only.
    Under ``no_grad`` (or when ``output`` needs no gradient) both branches run on slot-planned workspaces (same bits)."""
    _kind = 0

    def __init__(self, requires_grad=False, cuda=True, *, weights=None, dtype=None):
        super().__init__()
        if requires_grad:
            raise NotImplementedError(f"{type(self).__name__}: the native feature extractor is frozen (no weight-gradient launches): requires_grad=True is not implemented")
        self._dtype = N.dtype_id(dtype)
        layers = _vgg_layers(_VGG16_FEATURES)
        rename = {}
        for k, (lo, hi) in enumerate(_VGG16_SLICES):
            seq = nn.Sequential()
            for idx, m in layers[lo:hi]:
                seq.add_module(str(idx), m)
                for leaf in ("weight", "bias"):
                    rename[f"features.{idx}.{leaf}"] = f"slice{k + 1}.{idx}.{leaf}"
            setattr(self, f"slice{k + 1}", seq)
        self._init_weights(weights, rename)
        if cuda and torch.cuda.is_available():
            self.cuda()

    def __repr__(self):
        return "VGG16"


class _VggFramesFn(torch.autograd.Function):
    """Carries the gradient that ``VGG16Loss3D.forward`` has already computed chunk by chunk: backward only scales it."""

    @staticmethod
    def forward(ctx, output, loss, grad):
        ctx.grad, ctx.in_dtype = grad, output.dtype
        return loss.clone()

    @staticmethod
    def backward(ctx, gout):
        if ctx.grad is None:
            raise RuntimeError("perceptual loss: backward called a second time (the stored gradient is released by the first)")
        grad, ctx.grad = ctx.grad, None
        return (grad * gout.float()).to(ctx.in_dtype), None, None      # the f32 gradient, scaled, cast once to a 16-bit input's dtype


class VGG16Loss3D(VGG16Loss):
    """Mean over the frames f of ``VGG16Loss(output[:, :, f], target[:, :, f])`` (losses.py:396-453).
    ``VGG16Loss3D(requires_grad=False, cuda=True, *, weights=None, dtype=None, frames_per_pass=None)``: parameters, keys and weight
    loading are ``VGG16Loss``'s.  ``forward(output, target)``: [nb,1|3,frame,row,col] CUDA tensors, row, col >= 8 -> 0-dim f32 device
    tensor; the target branch is frozen.  Every per-frame mean has the same count, so the value is the four-tap loss of the frames taken
    as a batch: frames run in chunks of ``frames_per_pass`` (``None``: all in one pass) as nb * chunk images that the native pack reads
    straight from the 5-D tensor (a gray plane is replicated to three channels inside the pack, its three gradients summed in the
    unpack), and the loss is the fixed-order sum of the chunks' shares.

    When ``output`` requires grad, each chunk's native backward runs right after its forward (unit upstream scalar, the chunk's share
    as scale) into that chunk's frames of one 5-D gradient buffer, and the chunk's workspace is released before the next chunk: peak
    memory follows one chunk, not the frame count.  ``backward()`` then only multiplies the stored gradient by the upstream scalar; a
    second ``backward()`` raises, like ``VGG16Loss``.  Under ``no_grad`` (or when ``output`` needs no gradient) the slot-planned
    inference path runs per chunk."""

    def __init__(self, requires_grad=False, cuda=True, *, weights=None, dtype=None, frames_per_pass=None):
        if frames_per_pass is not None and not (isinstance(frames_per_pass, int) and frames_per_pass >= 1):
            raise ValueError(f"VGG16Loss3D: frames_per_pass must be None or an integer >= 1, got {frames_per_pass!r}")
        super().__init__(requires_grad, cuda, weights=weights, dtype=dtype)
        self.frames_per_pass = frames_per_pass

    def __repr__(self):
        return "VGG163D"

    def forward(self, output, target):
        name = "VGG16Loss3D"
        _check_5d(name, output, target)
        Bt, Cin, Fr, H, W = (int(v) for v in output.shape)
        if H < 8 or W < 8:
            raise ValueError(f"{name}: frames must be at least 8x8 (three max-pools), got {tuple(output.shape)}")
        plist = self._checked_params(name, output, target)
        lib, dev = N.lib(), output.device
        o32, t32 = _as_f32(output, f"{name} output"), _as_f32(target, f"{name} target")
        need_grad = torch.is_grad_enabled() and output.requires_grad
        params, st = N.ptr_array(plist), N.stream_ptr(dev)
        step = Fr if self.frames_per_pass is None else min(self.frames_per_pass, Fr)
        grad = torch.empty_like(o32) if need_grad else None
        one = torch.ones((), dtype=torch.float32, device=dev) if need_grad else None
        part = torch.empty((), dtype=torch.float32, device=dev)
        total = torch.zeros((), dtype=torch.float32, device=dev)
        for f0 in range(0, Fr, step):
            k = min(step, Fr - f0)
            share = k / Fr
            if need_grad:
                cfg = N.VggLossCfg(self._kind, Bt * k, H, W, self._dtype)
                ws = N.workspace(lib.srcgan_vggloss_ws_bytes(C.byref(cfg)), dev)
                N.check(lib.srcgan_vggloss_forward_frames(C.byref(cfg), o32.data_ptr(), t32.data_ptr(), Cin, Fr, f0, k, params, ws.data_ptr(),
                                                          part.data_ptr(), st), "srcgan_vggloss_forward_frames")
                scratch = N.workspace(lib.srcgan_vggloss_bwd_scratch_bytes(C.byref(cfg)), dev)
                N.check(lib.srcgan_vggloss_backward_frames(C.byref(cfg), one.data_ptr(), share, Cin, Fr, f0, k, params, ws.data_ptr(),
                                                           scratch.data_ptr(), grad.data_ptr(), st), "srcgan_vggloss_backward_frames")
                del ws, scratch               # the next chunk's workspace reuses this memory
            else:
                _vgg_infer(self._kind, self._dtype, o32, t32, Bt, Fr, f0, k, params, part)
            total = total + part * share      # stream-ordered: `part` is rewritten by the next chunk only after this read
        if not need_grad:
            return total
        return _VggFramesFn.apply(output, total, grad)


class PerceptionLoss(_VggLossBase):
    """MSE between the VGG19 ``features[:35]`` (conv5_4, before its ReLU) of ``input`` and ``target`` (losses.py:455-470).
    ``PerceptionLoss(feature_layer=35, *, weights=None, dtype=None)``; frozen parameters under ``features.0.weight`` ...
    ``features.34.bias`` (the reference's and torchvision's keys).  H, W >= 16.  Otherwise as ``VGG16Loss``; like the reference it is not
    moved to a device by its constructor and keeps nn.Module's repr."""
    _kind = 1

    def __init__(self, feature_layer=35, *, weights=None, dtype=None):
        super().__init__()
        if feature_layer != 35:
            raise NotImplementedError(f"PerceptionLoss: the native plan is vgg19.features[:35] (the reference's default); feature_layer={feature_layer} is not implemented")
        self._dtype = N.dtype_id(dtype)
        self.features = nn.Sequential()
        for idx, m in _vgg_layers(_VGG19_FEATURES)[:35]:
            self.features.add_module(str(idx), m)
        self._init_weights(weights, {})

