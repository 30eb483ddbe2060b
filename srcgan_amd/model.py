"""Host-side mirror of the reference model classes on the hot path.

Same class names, constructor signatures, ``state_dict`` keys / shapes / dtypes and NCHW f32
tensor interface as the reference, so ``eval(opt.SRModel)(1, 1, opt.up)``
(trainCas.py:30) and reference ``.pth`` checkpoints keep working -- but ``forward`` / backward run
as one native call each into libsrcgan_amd.so (hand-written gfx950 kernels).  The ``nn.Conv2d`` /
``nn.BatchNorm2d`` children are *parameter holders only* (they give the reference's key names and
its default initialisation); their own ``forward`` is never used and there is no CPU fallback.

  RDDBNet              <- reference src/model/rddb.py:85-114
  NLayerDiscriminator  <- reference src/model/model.py:595-639
  RDDBNetA             <- named by reference src/train.py:11,173 but defined nowhere; build-defined
                          HR->LR mirror (strided 3x3 s2 conv + LeakyReLU per /2 stage, trunk at LR).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Callable, NamedTuple

import torch
import torch.nn as nn

from . import _native as N

__all__ = ["RDDBNet", "RDDBNetA", "RDDBNetB", "LegacyRDDBNet", "ResDeconv", "ESPCN", "SRCNN", "EDSR", "SRDN", "SRDenseNetA", "SRDenseNetB", "RCAN", "DDBPN", "RDN", "MDSR", "VDSR", "ResnetGenerator", "UnetGenerator", "NLayerDiscriminator", "ResidualDenseBlock_5", "RRDB", "deconv",
           "get_deconv_params", "Identity", "get_norm_layer", "init_weights", "init_net", "define_G"]


def get_deconv_params(upscale_factor):
    """(kernel_size, stride, output_padding) of the reference's deconv helper (rddb.py:9-25)."""
    table = {2: (2, 2), 4: (2, 4), 8: (4, 8)}
    if upscale_factor not in table:
        raise ValueError(f"unsupported upscale_factor {upscale_factor}")
    k, s = table[upscale_factor]
    return k, s, s - k


def deconv(in_planes, out_planes, upscale_factor=2):
    """Parameter holder equal to the reference's deconv() (rddb.py:28-38)."""
    k, s, opad = get_deconv_params(upscale_factor)
    return nn.ConvTranspose2d(in_planes, out_planes, kernel_size=k, stride=s, padding=0, bias=False, output_padding=opad)


class _HolderOnly(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise NotImplementedError(
            f"{type(self).__name__} is a parameter holder of the native srcgan_amd network; call the whole "
            "network (RDDBNet / NLayerDiscriminator), which runs as fused gfx950 kernels.")


class ResidualDenseBlock_5(_HolderOnly):
    """Holder for conv1..conv5 of one dense block (rddb.py:48-60)."""

    def __init__(self, nf=64, gc=32, bias=True):
        super().__init__()
        for k in range(5):
            setattr(self, f"conv{k + 1}", nn.Conv2d(nf + k * gc, gc if k < 4 else nf, 3, 1, 1, bias=bias))


class RRDB(_HolderOnly):
    """Holder for RDB1..RDB3 (rddb.py:71-76)."""

    def __init__(self, nf, gc=32):
        super().__init__()
        for j in (1, 2, 3):
            setattr(self, f"RDB{j}", ResidualDenseBlock_5(nf, gc))


def _kaiming_like_reference(module: nn.Module) -> None:
    # rddb.py:100-105: kaiming-normal(fan_out, relu) on every nn.Conv2d weight; biases and
    # ConvTranspose2d weights keep torch's default init.
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)


class _PackState:
    """Persistent packed (MFMA-order, compute-dtype) copy of a module's weights: packed once per weight update instead of once per
    native call -- a cycle step runs each generator three times forward and three times backward on the same weights
    (reference train.py:228-260, 331-333).

    Validity is decided ON THE DEVICE, per call and without a host synchronisation: ``srcgan_params_fingerprint`` hashes every bit
    of every parameter (66 MB for the 23-block generator: ~15 us) into the second word of a guard pair, and the pack kernels of
    the native call do nothing when it equals the first word -- the fingerprint the pack was made from (``srcgan_net_opts.pack
    == 2``).  So ANY way of changing the weights is honoured: optimiser steps, ``load_state_dict``, ``p.data.mul_()`` (which does
    not bump autograd's version counter), a raw-pointer write by another library.  The host only forces a pack when the buffer is
    new, the layout changed or the parameters moved (their pointer table is rebuilt then); ``invalidate()`` forces one too."""

    def __init__(self):
        self.buf = None
        self.layout = None
        self.table = None            # device int64 [n, 3]: pointer, elements, first fingerprint block
        self.table_key = None
        self.nblocks = 0
        self.guard = None            # device int64 [4]: forward {packed-from, now}, backward {packed-from, now}
        self.valid = [False, False]  # forward / backward pack made at least once from the current buffer + table

    def invalidate(self):
        """Force the next forward and the next backward to re-pack (never needed for correctness: see the class comment)."""
        self.valid = [False, False]

    def opts(self, lib_bytes_fn, cfg, params, extra, backward, device):
        """-> NetOpts for one native call.  Call ``done(backward)`` after the call succeeded."""
        need = int(lib_bytes_fn(C.byref(cfg)))
        if self.buf is None or self.buf.numel() < need or self.buf.device != device or self.layout != extra:
            self.buf = torch.empty(need, dtype=torch.uint8, device=device)
            self.guard = torch.zeros(4, dtype=torch.int64, device=device)
            self.layout = extra
            self.valid = [False, False]
        key = tuple((p.data_ptr(), p.numel()) for p in params)
        if key != self.table_key:
            rows, blk = [], 0
            for ptr, n in key:
                rows.append((ptr, n, blk))
                blk += (n + 16383) // 16384              # srcgan_params_fingerprint: 16 Ki-element slices
            self.table = torch.tensor(rows, dtype=torch.int64).to(device)
            self.table_key, self.nblocks = key, blk
            self.valid = [False, False]
        slot = 2 if backward else 0
        gptr = self.guard.data_ptr() + 8 * slot
        N.check(N.lib().srcgan_params_fingerprint(self.table.data_ptr(), len(key), self.nblocks, gptr + 8, N.stream_ptr(device)),
                "srcgan_params_fingerprint")
        return N.NetOpts(self.buf.data_ptr(), 2 if self.valid[1 if backward else 0] else 1, 0, 0, gptr)

    def done(self, backward):
        """The native call that packed (or verified) returned without error: what is packed now matches the fingerprint."""
        slot = 2 if backward else 0
        self.guard[slot:slot + 1].copy_(self.guard[slot + 1:slot + 2])
        self.valid[1 if backward else 0] = True


class _GradArena:
    """One flat f32 buffer for all parameter gradients a backward call produces; ``views[i]`` aliases it with the parameter's
    shape.  autograd's AccumulateGrad adopts the views as ``.grad`` (no copy), so the data-parallel all-reduce runs on slices of
    the flat buffer in place -- no flatten / copy-back passes (srcgan_amd.dist.GradSync)."""

    def __init__(self, params, needs):
        sizes = [p.numel() if n else 0 for p, n in zip(params, needs)]
        self.flat = torch.empty(sum(sizes), dtype=torch.float32, device=params[0].device)
        self.views, self.offsets, off = [], [0], 0
        for p, n, sz in zip(params, needs, sizes):
            self.views.append(self.flat[off:off + sz].view_as(p) if n else None)
            off += sz
            self.offsets.append(off)          # offsets[i] .. offsets[i + 1] = parameter i


# Data-parallel hook (srcgan_amd.dist.GradSync.attach sets it, detach clears it): an object with ``cuts(cfg, nrr, params) -> [rrdb
# indices]`` (phase boundaries of the generator's backward) and ``phase_done(arena, params, first, end, last)``, called right after
# the native call that finalised the gradients of the parameters [first, end) (``srcgan_rddbnet_phase_params``; ``last``: the
# backward is complete) was queued: the hook launches their all-reduce on its side stream while the next phase computes.  One slot
# for every native network: each Function reads it at FORWARD time and its backward uses what it read.
_phase_hook = None


# ---- operand handling every native forward / backward shares
def _check_input(x, name, in_ch, expects):
    """The network input must be on the GPU (RuntimeError) and [B,in_ch,H,W] (ValueError, ``expects``: the family's wording)."""
    N.require_cuda(x, f"{name}.forward")
    if x.dim() != 4 or x.shape[1] != in_ch:
        raise ValueError(f"{expects}, got {tuple(x.shape)}")


def _input(x, name, in_ch, expects):
    """-> the checked input as the native code reads it: off the graph, contiguous, f32."""
    _check_input(x, name, in_ch, expects)
    return x.detach().contiguous().float()


def _params(params, name):
    """-> the parameters as the native code reads them (``const float*``): on the GPU, off the graph, contiguous, f32."""
    for p in params:
        N.require_cuda(p, f"{name} parameter")
    plist = [p.detach().contiguous() for p in params]
    if any(p.dtype != torch.float32 for p in plist):
        raise TypeError(f"{name} parameters must be float32 (canonical weights stay f32)")
    return plist


def _backward_operands(ctx, dy, first, scratch_bytes, name):
    """What a native backward needs besides the forward's workspace -> (dy, params, arena, grads, scratch, dx).  ``first``: index
    of the first parameter in ``ctx.needs_input_grad``; ``scratch_bytes``: the family's ``*_bwd_scratch_bytes``.  For all three
    Functions: no arena (and ``None`` gradients: the native call gets the same null pointers as from an arena without elements,
    and a hook's ``phase_done`` ignores either) when no parameter needs a gradient; ``dx`` is None when the input needs none."""
    if ctx.ws is None:
        raise RuntimeError(f"{name} backward called twice (activations were released)")
    cfg, params = ctx.cfg, list(ctx.saved_tensors)
    dy = dy.contiguous().float()
    needs = [ctx.needs_input_grad[first + i] for i in range(len(params))]
    arena = _GradArena(params, needs) if any(needs) else None
    grads = arena.views if arena is not None else [None] * len(params)
    scratch = N.workspace(scratch_bytes(C.byref(cfg)), dy.device)
    dx = torch.empty(cfg.B, cfg.in_ch, cfg.H, cfg.W, dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[0] else None
    return dy, params, arena, grads, scratch, dx


def _rddb_prepare(x, cfg_items, params):
    """Checks and allocations both generator forwards (autograd Function, inference) share.
    -> (x, None, None, pstate, layout, empty output) for an empty batch, else (x, cfg, plist, pstate, layout, y)."""
    in_ch, out_ch, up, nf, nb, gc, dtype, down = cfg_items[:8]
    legacy = cfg_items[8] if len(cfg_items) > 8 else 0
    pstate = cfg_items[9] if len(cfg_items) > 9 else None
    x = _input(x, "RDDBNet", in_ch, f"RDDBNet expects [B,{in_ch},H,W]")
    B, _, H, W = x.shape
    f = (up if down == 0 else 1)
    HO, WO = (H * f, W * f) if down <= 1 else (H // down, W // down)
    layout = (in_ch, out_ch, up, nf, nb, gc, dtype, down, legacy)
    if B == 0:          # an empty batch yields an empty output and zero gradients, as aten::convolution does
        return x, None, None, pstate, layout, x.new_zeros((0, out_ch, HO, WO))
    cfg = N.RddbCfg(in_ch, out_ch, up, nf, nb, gc, B, H, W, dtype, down, legacy)
    plist = _params(params, "RDDBNet")
    y = torch.empty(B, out_ch, HO, WO, dtype=torch.float32, device=x.device)
    return x, cfg, plist, pstate, layout, y


class _RddbFn(torch.autograd.Function):
    """One native forward / one native backward for the whole generator."""

    @staticmethod
    def forward(ctx, x, cfg_items, *params):
        lib = N.lib()
        x, cfg, plist, pstate, layout, y = _rddb_prepare(x, cfg_items, params)
        ctx.empty = cfg is None
        if ctx.empty:
            ctx.save_for_backward(*params)
            return y
        ws = N.workspace(lib.srcgan_rddbnet_ws_bytes(C.byref(cfg)), x.device)
        opt = pstate.opts(lib.srcgan_rddbnet_wpack_bytes, cfg, plist, layout, False, x.device) if pstate is not None else None
        N.check(lib.srcgan_rddbnet_forward_ex(C.byref(cfg), x.data_ptr(), N.ptr_array(plist), ws.data_ptr(), y.data_ptr(),
                                              C.byref(opt) if opt is not None else None, N.stream_ptr(x.device)), "srcgan_rddbnet_forward")
        if pstate is not None:
            pstate.done(False)
        ctx.cfg, ctx.ws, ctx.n = cfg, ws, len(plist)
        ctx.pstate, ctx.layout = pstate, layout
        ctx.save_for_backward(*plist)
        ctx.phase_hook = _phase_hook
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = N.lib()
        if ctx.empty:
            return (None, None, *[torch.zeros_like(p) if ctx.needs_input_grad[2 + i] else None for i, p in enumerate(ctx.saved_tensors)])
        cfg = ctx.cfg
        dy, params, arena, grads, scratch, dx = _backward_operands(ctx, dy, 2, lib.srcgan_rddbnet_bwd_scratch_bytes, "RDDBNet")
        need_dx = dx is not None
        pstate = ctx.pstate
        opt = pstate.opts(lib.srcgan_rddbnet_wpack_bytes, cfg, params, ctx.layout, True, dy.device) if pstate is not None else N.NetOpts(None, 0, 0, 0, None)
        gptr, pptr = N.ptr_array(grads), N.ptr_array(params)
        hook = ctx.phase_hook
        nrr = lib.srcgan_rddbnet_num_rrdb(C.byref(cfg))
        # phases: RRDB ranges, last to first (one phase unless a data-parallel hook asks for more)
        cuts = hook.cuts(cfg, nrr, params) if (hook is not None and nrr > 1) else [0]
        hi = nrr
        for lo in sorted(set(cuts) | {0}, reverse=True):
            if lo >= hi and hi != nrr:
                continue
            opt.rrdb_lo, opt.rrdb_hi = lo, hi
            N.check(lib.srcgan_rddbnet_backward_ex(C.byref(cfg), dy.data_ptr(), pptr, ctx.ws.data_ptr(), scratch.data_ptr(), gptr,
                                                   dx.data_ptr() if need_dx else None, C.byref(opt), N.stream_ptr(dy.device)),
                    "srcgan_rddbnet_backward")
            if opt.pack and pstate is not None:
                pstate.done(True)
            opt.pack = 0
            if hook is not None:
                first, end = C.c_int(), C.c_int()
                N.check(lib.srcgan_rddbnet_phase_params(C.byref(cfg), lo, hi, C.byref(first), C.byref(end)), "srcgan_rddbnet_phase_params")
                hook.phase_done(arena, params, first.value, end.value, lo == 0)
            hi = lo
        ctx.ws = None
        return (dx, None, *grads)


def _rddb_infer(x, cfg_items, params):
    """Forward under ``torch.no_grad()``: one native call on the depth-independent inference workspace (three rotating dense
    buffers, no sign masks, no per-stage retention: ``srcgan_rddbnet_infer``), released on return.  Same kernels in the same order as
    ``_RddbFn.forward``, hence the same bits."""
    lib = N.lib()
    x, cfg, plist, pstate, layout, y = _rddb_prepare(x, cfg_items, params)
    if cfg is None:
        return y
    ws = N.workspace(lib.srcgan_rddbnet_infer_ws_bytes(C.byref(cfg)), x.device)
    opt = pstate.opts(lib.srcgan_rddbnet_wpack_bytes, cfg, plist, layout, False, x.device) if pstate is not None else None
    N.check(lib.srcgan_rddbnet_infer(C.byref(cfg), x.data_ptr(), N.ptr_array(plist), ws.data_ptr(), y.data_ptr(),
                                     C.byref(opt) if opt is not None else None, N.stream_ptr(x.device)), "srcgan_rddbnet_infer")
    if pstate is not None:
        pstate.done(False)
    return y


def _rddb_forward(x, cfg_items, params):
    """Grad mode on: the autograd Function (workspace kept for backward), also when nothing requires grad.  Off: inference."""
    if torch.is_grad_enabled():
        return _RddbFn.apply(x, cfg_items, *params)
    return _rddb_infer(x, cfg_items, params)


class _NativeRepr:
    """Method-only mixin of the native networks: what ``repr()`` says about them."""
    _repr_mode = False          # True in the classes whose ``mode`` (up-sampling factor) belongs in the repr

    def extra_repr(self):
        return "native gfx950, " + (f"mode={self.mode}, " if self._repr_mode else "") + f"compute_dtype={self.compute_dtype}"


class RDDBNet(_NativeRepr, nn.Module):
    """RRDB generator, drop-in for reference ``model.RDDBNet`` (rddb.py:85-114).

    ``forward(x[B,in_ch,H,W] f32 NCHW) -> [B,ou_ch,H*up,W*up]``.  ``dtype``: 'fp32' (default; exact
    f32 MFMA, <=1e-3 of the CPU reference) or 'bf16' (perf mode)."""

    def __init__(self, in_ch, ou_ch, upscale_factor, nf=64, nb=3, gc=32, dtype=None):
        super().__init__()
        self.conv_first = nn.Conv2d(in_ch, nf, 3, 1, 1, bias=True)
        self.RRDB_trunk = nn.Sequential(*[RRDB(nf=nf, gc=gc) for _ in range(nb)])
        self.trunk_conv = nn.Conv2d(nf, nf, 3, 1, 1, bias=True)
        self.upscale_factor = upscale_factor
        ups = []
        for _ in range(int(math.log2(upscale_factor))):
            ups += [deconv(nf, nf, upscale_factor=2), nn.LeakyReLU(negative_slope=0.2, inplace=True)]
        self.upscale_layers = nn.Sequential(*ups)
        self.conv_last = nn.Conv2d(nf, ou_ch, 3, 1, 1, bias=False)
        _kaiming_like_reference(self)
        self._cfg = (in_ch, ou_ch, upscale_factor, nf, nb, gc)
        self.compute_dtype = N.dtype_name(dtype)
        self._pack = _PackState()

    def _down(self):
        return 0

    def invalidate_packed_weights(self):
        """Force a re-pack of the kernels' weight copy at the next forward / backward.  Not needed for correctness -- every native
        call verifies the copy against a device-side fingerprint of the parameters (see _PackState) -- kept as an explicit hook."""
        self._pack.invalidate()

    def forward(self, x):
        cfg = (*self._cfg, N.dtype_id(self.compute_dtype), self._down(), 0, self._pack)
        # parameters in state_dict order == the order the native planner assumes
        return _rddb_forward(x, cfg, list(self.parameters()))


class RDDBNetA(RDDBNet):
    """HR->LR generator G_B of the cycle (reference train.py:173,178 names ``RDDBNetA`` but ships no
    definition -> build-defined, "parity unpinned" vs the reference; pinned against oracle.rddbneta_forward).
    conv_first -> [conv3x3 s2 + bias + LeakyReLU] x log2(down) -> RRDB trunk at LR -> trunk_conv + skip -> conv_last."""

    def __init__(self, in_ch, ou_ch, down_factor, nf=64, nb=3, gc=32, dtype=None):
        super().__init__(in_ch, ou_ch, 1, nf=nf, nb=nb, gc=gc, dtype=dtype)
        self.down_factor = down_factor
        downs = []
        for _ in range(int(math.log2(down_factor))):
            downs += [nn.Conv2d(nf, nf, 3, 2, 1, bias=True), nn.LeakyReLU(negative_slope=0.2, inplace=True)]
        self.down_layers = nn.Sequential(*downs)
        _kaiming_like_reference(self.down_layers)

    def _down(self):
        return max(1, self.down_factor)

    def forward(self, x):
        cfg = (*self._cfg, N.dtype_id(self.compute_dtype), self._down(), 0, self._pack)
        # native order: conv_first, down_layers, trunk, trunk_conv, conv_last
        ps = [self.conv_first.weight, self.conv_first.bias, *self.down_layers.parameters(),
              *self.RRDB_trunk.parameters(), self.trunk_conv.weight, self.trunk_conv.bias, self.conv_last.weight]
        return _rddb_forward(x, cfg, ps)


class _LegacyRRDB(_HolderOnly):
    """Holder for the RRDB of model/model.py:214-226: like rddb.py's, but its constructor already re-initialises its
    own convolutions (kaiming-normal) -- kept so that a seeded construction consumes the RNG exactly like the reference."""

    def __init__(self, nf, gc=32):
        super().__init__()
        for j in (1, 2, 3):
            setattr(self, f"RDB{j}", ResidualDenseBlock_5(nf, gc))
        _kaiming_like_reference(self)


_MODES = {"x1": 1, "x2": 2, "x4": 4}


class RDDBNetB(_NativeRepr, nn.Module):
    """Legacy nearest-up-sampling generator, drop-in for reference ``model.model.RDDBNetB`` (model/model.py:394-440; G_A of
    train.py:172,177).  ``RDDBNetB(in_nc, out_nc, nf, nb=3, gc=32, mode='x2')``; forward: conv_first -> RRDB trunk ->
    trunk_conv + skip -> [nearest x2 -> upconv -> LeakyReLU] (x4: upconv1 then upconv2; x2: upconv1 twice, the second
    without up-sampling) -> HRconv + LeakyReLU eight times -> conv_last (with bias).  Any other mode leaves the
    resolution unchanged in the reference; only 'x2' / 'x4' are accepted here."""

    _legacy = 1
    _tail = ("upconv1", "upconv2", "HRconv")
    _repr_mode = True

    def __init__(self, in_nc, out_nc, nf, nb=3, gc=32, mode="x2", dtype=None):
        super().__init__()
        if mode not in _MODES or (self._legacy == 1 and mode == "x1"):
            raise NotImplementedError(f"{type(self).__name__}: mode {mode!r} is not supported")
        self.conv_first = nn.Conv2d(in_nc, nf, 3, 1, 1, bias=True)
        self.RRDB_trunk = nn.Sequential(*[_LegacyRRDB(nf=nf, gc=gc) for _ in range(nb)])
        self.trunk_conv = nn.Conv2d(nf, nf, 3, 1, 1, bias=True)
        for name in self._tail:
            setattr(self, name, nn.Conv2d(nf, nf, 3, 1, 1, bias=True))
        self.mode = mode
        self.nb = nb
        self.conv_last = nn.Conv2d(nf, out_nc, 3, 1, 1, bias=True)
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        _kaiming_like_reference(self)
        self._cfg = (in_nc, out_nc, _MODES[mode], nf, nb, gc)
        self.compute_dtype = N.dtype_name(dtype)

    def forward(self, x):
        cfg = (*self._cfg, N.dtype_id(self.compute_dtype), 0, self._legacy)
        ps = list(self.parameters())                            # state_dict order == native order
        if self.mode == "x2":       # upconv2 is not on the x2 graph (model.py:430-432): its .grad stays None, as in the reference
            skip = {id(self.upconv2.weight), id(self.upconv2.bias)}
            ps = [p.detach() if id(p) in skip else p for p in ps]
        return _rddb_forward(x, cfg, ps)


class LegacyRDDBNet(RDDBNetB):
    """Drop-in for the *legacy* ``model.model.RDDBNet`` (model/model.py:347-391; not the rddb.py class that
    ``from model import *`` exports): ``(in_nc, out_nc, nf, nb, gc=32, mode='x2')``.  Its forward computes the RRDB trunk
    and discards it (model.py:382-383), so the output is conv_first -> [nearest x2 -> upconv -> LeakyReLU] per x2 stage
    (mode 'x1': upconv without up-sampling) -> HRconv + LeakyReLU twice -> conv_last; the trunk parameters exist in the
    state_dict and receive no gradient (``.grad`` stays None, as in the reference)."""

    _legacy = 2
    _tail = ("upconv", "HRconv")

    def __init__(self, in_nc, out_nc, nf, nb, gc=32, mode="x2", dtype=None):
        super().__init__(in_nc, out_nc, nf, nb=nb, gc=gc, mode=mode, dtype=dtype)

    def forward(self, x):
        cfg = (*self._cfg, N.dtype_id(self.compute_dtype), 0, self._legacy)
        # the trunk is not on the graph: pass its parameters detached so autograd leaves their .grad at None
        trunk = {id(p) for p in self.RRDB_trunk.parameters()} | {id(self.trunk_conv.weight), id(self.trunk_conv.bias)}
        ps = [p.detach() if id(p) in trunk else p for p in self.parameters()]
        return _rddb_forward(x, cfg, ps)


# ------------------------------------------------------------------------------------------------ op-list networks
class _OpList(NamedTuple):
    """One network family of the native op-list executor (``rd_forward`` / ``rd_backward`` in csrc/oplist.hip).  Its C entry points
    are ``<stem>_ws_bytes`` / ``_forward`` / ``_bwd_scratch_bytes`` / ``_backward`` / ``_infer_ws_bytes`` / ``_infer``."""
    name: str                 # in messages
    stem: str                 # C symbol stem
    make_cfg: Callable        # (x, items) -> (config struct, output shape); checks x (_check_input) and what else the family requires


def _resdeconv_cfg(x, items):
    out_ch, dtype, layers, norm = items
    _check_input(x, "ResDeconv", 3, "ResDeconv's stem expects 3 channels")
    B, _, H, W = x.shape
    if H % 16 or W % 16:
        raise ValueError(f"ResDeconv needs H and W to be multiples of 16 (four stride-2 stages), got {H}x{W}")
    return N.ResDeconvCfg(3, out_ch, B, H, W, dtype, (C.c_int * 4)(*layers), norm), (B, out_ch, H, W)


def _srnet_cfg(x, items):
    kind, in_ch, out_ch, up, base, dtype = items[:6]
    nres = items[6] if len(items) > 6 else 0
    _check_input(x, "ESPCN/SRCNN/EDSR", in_ch, f"expected [B,{in_ch},H,W]")
    B, _, H, W = x.shape
    f = 1 if kind == 1 else up
    return N.SrNetCfg(kind, in_ch, out_ch, up, base, B, H, W, dtype, nres), (B, out_ch, H * f, W * f)


def _srdense_cfg(x, items):
    kind, in_ch, out_ch, growth, nblocks, nlayers, up, dtype = items
    _check_input(x, "SRDenseNet", in_ch, f"expected [B,{in_ch},H,W]")
    B, _, H, W = x.shape
    cfg = N.SrDenseCfg(kind, in_ch, out_ch, B, H, W, dtype, growth, nblocks, nlayers, up)
    oh, ow = C.c_int(), C.c_int()
    N.check(N.lib().srcgan_srdense_out_hw(C.byref(cfg), C.byref(oh), C.byref(ow)), "srcgan_srdense_out_hw")
    return cfg, (B, out_ch, oh.value, ow.value)


# ResDeconv's inference entry points take one more argument, ``fold_tail``.  1: deconv13 and pred run as four parity 2x2 convolutions
# with composed weights, the 64-channel full-resolution tensor is never made.  0: the training forward's launches, its bits.
_RESDECONV = _OpList("ResDeconv", "srcgan_resdeconv", _resdeconv_cfg)       # resdeconv.py:164-195
_SRNET = _OpList("ESPCN/SRCNN/EDSR", "srcgan_srnet", _srnet_cfg)            # kind 0 ESPCN, 1 SRCNN, 2 EDSR
_SRDENSE = _OpList("SRDenseNet", "srcgan_srdense", _srdense_cfg)            # kind 0 SRDenseNetA, 1 SRDenseNetB


def _oplist_run(x, family, items, params, entry, extra=()):
    """One native forward, ``entry`` "forward" (training workspace) or "infer" (slot-planned workspace; ``extra``: the family's
    trailing inference arguments) -> (y, cfg, plist, workspace)."""
    lib = N.lib()
    cfg, yshape = family.make_cfg(x, items)
    x = x.detach().contiguous().float()
    plist = _params(params, family.name)
    ws_bytes = getattr(lib, f"{family.stem}_ws_bytes" if entry == "forward" else f"{family.stem}_infer_ws_bytes")
    ws = N.workspace(ws_bytes(C.byref(cfg), *extra), x.device)
    y = torch.empty(*yshape, dtype=torch.float32, device=x.device)
    what = f"{family.stem}_{entry}"
    N.check(getattr(lib, what)(C.byref(cfg), x.data_ptr(), N.ptr_array(plist), ws.data_ptr(), y.data_ptr(), *extra, N.stream_ptr(x.device)), what)
    return y, cfg, plist, ws


class _OpListFn(torch.autograd.Function):
    """One native forward / one native backward for a whole op-list network."""

    @staticmethod
    def forward(ctx, x, family, items, *params):
        y, ctx.cfg, plist, ctx.ws = _oplist_run(x, family, items, params, "forward")
        ctx.family = family
        ctx.save_for_backward(*plist)
        ctx.phase_hook = _phase_hook
        return y

    @staticmethod
    def backward(ctx, dy):
        lib, family = N.lib(), ctx.family
        dy, params, arena, grads, scratch, dx = _backward_operands(ctx, dy, 3, getattr(lib, f"{family.stem}_bwd_scratch_bytes"), family.name)
        what = f"{family.stem}_backward"
        N.check(getattr(lib, what)(C.byref(ctx.cfg), dy.data_ptr(), N.ptr_array(params), ctx.ws.data_ptr(), scratch.data_ptr(),
                                   N.ptr_array(grads), dx.data_ptr() if dx is not None else None, N.stream_ptr(dy.device)), what)
        ctx.ws = None
        if ctx.phase_hook is not None:
            ctx.phase_hook.phase_done(arena, params, 0, len(params), True)
        return (dx, None, None, *grads)


def _oplist_forward(x, family, items, params, extra=()):
    """The rule of _rddb_forward: grad mode decides, eval() plays no part.  On: the autograd Function (workspace kept for backward).
    Off: ``<stem>_infer`` on the slot-planned workspace, released on return; no autograd node.  ``extra`` (the family's trailing
    inference arguments) applies to the second branch only: the training forward has no such arguments."""
    if torch.is_grad_enabled():
        return _OpListFn.apply(x, family, items, *params)
    return _oplist_run(x, family, items, params, "infer", extra)[0]


# ------------------------------------------------------------------------------------------------ ResDeconv colouriser
class _BasicBlockHolder(_HolderOnly):
    """Parameter holder of resdeconv.py:56-76 BasicBlock (attribute order = the reference's state_dict order)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, BN="GN"):
        super().__init__()
        norm = (lambda c: nn.InstanceNorm2d(c)) if BN == "IN" else (lambda c: nn.GroupNorm(32, c))
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = norm(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = norm(planes)
        self.downsample = downsample
        self.stride = stride


class ResDeconv(_NativeRepr, nn.Module):
    """Colouriser, drop-in for reference ``model.ResDeconv`` (src/model/resdeconv.py:99-195):
    ``ResDeconv(src_ch=1, tar_ch=3, block=None, layers=[2, 2, 2, 2], BN='GN')`` -- the reference's positional signature
    (resdeconv.py:107).  ``block``: BasicBlock, the only block the reference defines.  ``layers``: BasicBlocks per stage, any
    counts ([2, 2, 2, 2] = ResNet-18 layout, the default; [3, 4, 6, 3] = ResNet-34); the up path uses layers[2], layers[1],
    layers[0] (resdeconv.py:131-137).  ``BN``: 'GN' (GroupNorm(32, C), the default) or 'IN' (nn.InstanceNorm2d(C): no parameters);
    'BN' (BatchNorm2d) is refused.  ``forward(x[B,src_ch,H,W]) -> [B,tar_ch,H,W]`` (H, W multiples of 16).
    A 1-channel source is replicated to 3 channels like the reference (resdeconv.py:166-167)."""

    def __init__(self, src_ch=1, tar_ch=3, block=None, layers=(2, 2, 2, 2), BN="GN", dtype=None):
        super().__init__()
        if block is not None and getattr(block, "__name__", str(block)) not in ("BasicBlock", "_BasicBlockHolder"):
            raise NotImplementedError("native ResDeconv implements block=BasicBlock (the only block resdeconv.py defines)")
        layers = [int(v) for v in layers]
        if len(layers) != 4 or min(layers) < 1:
            raise ValueError("ResDeconv: layers must be four positive block counts")
        if BN not in ("GN", "IN"):
            raise NotImplementedError("native ResDeconv implements BN='GN' (GroupNorm(32, C), the reference's default) and BN='IN' (InstanceNorm2d)")
        self.src_ch = src_ch
        if isinstance(tar_ch, list):
            tar_ch = sum(tar_ch)
        self.tar_ch = tar_ch
        self.layers_cfg, self.BN = tuple(layers), BN
        self.inplanes = 64
        # creation order == the reference's (it fixes which random numbers each default initialisation consumes)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.InstanceNorm2d(64) if BN == "IN" else nn.GroupNorm(32, 64)
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        self.deconv10 = nn.ConvTranspose2d(512, 256, 2, 2, 0, bias=False)
        self.inplanes = 256
        self.upRes1 = self._make_layer(256, layers[2], 1)
        self.deconv11 = nn.ConvTranspose2d(256, 128, 2, 2, 0, bias=False)
        self.inplanes = 128
        self.upRes2 = self._make_layer(128, layers[1], 1)
        self.deconv12 = nn.ConvTranspose2d(128, 64, 2, 2, 0, bias=False)
        self.inplanes = 64
        self.upRes3 = self._make_layer(64, layers[0], 1)
        self.deconv13 = nn.ConvTranspose2d(64, 64, 2, 2, 0, bias=False)
        self.pred = nn.Conv2d(64, tar_ch, kernel_size=3, stride=1, padding=1, bias=False)
        _kaiming_like_reference(self)
        self.compute_dtype = N.dtype_name(dtype)

    def _make_layer(self, planes, blocks, stride):
        downsample = None
        norm = nn.InstanceNorm2d(planes) if self.BN == "IN" else nn.GroupNorm(32, planes)
        if stride != 1 or self.inplanes != planes:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes, kernel_size=1, stride=stride, bias=False), norm)
        layers = [_BasicBlockHolder(self.inplanes, planes, stride, downsample, BN=self.BN)]
        self.inplanes = planes
        for _ in range(1, blocks):
            layers.append(_BasicBlockHolder(self.inplanes, planes, BN=self.BN))
        return nn.Sequential(*layers)

    def forward(self, x):
        if self.src_ch == 1:
            x = torch.cat([x, x, x], dim=1)
        items = (self.tar_ch, N.dtype_id(self.compute_dtype), self.layers_cfg, 1 if self.BN == "IN" else 0)
        return _oplist_forward(x, _RESDECONV, items, list(self.parameters()), extra=(1,))      # under no_grad: fold_tail = 1


# ------------------------------------------------------------------------------------------------ ESPCN / SRCNN
class ESPCN(_NativeRepr, nn.Module):
    """Drop-in for reference ``model.ESPCN`` (src/model/espcn.py:18-51; the CLI default ``--SRModel``, trainCas.py:169):
    5x5, 3x3, 3x3 convolutions + ReLU, 3x3 to 64 r^2 channels, PixelShuffle(r), 3x3."""

    def __init__(self, in_ch=3, ou_ch=3, upscale_factor=2, base_kernel=64, dtype=None):
        super().__init__()
        kernels = [int(x * base_kernel) for x in [1, 1, 1 / 2]]
        self.relu = nn.ReLU(True)
        self.conv1 = nn.Conv2d(in_ch, kernels[0], kernel_size=5, stride=1, padding=2)
        self.conv2 = nn.Conv2d(kernels[0], kernels[1], kernel_size=3, stride=1, padding=1)
        self.conv3 = nn.Conv2d(kernels[1], kernels[2], kernel_size=3, stride=1, padding=1)
        self.conv4 = nn.Conv2d(kernels[2], base_kernel * upscale_factor ** 2, kernel_size=3, stride=1, padding=1)
        self.pixel_shuffle = nn.PixelShuffle(upscale_factor)
        self.conv5 = nn.Conv2d(base_kernel, ou_ch, kernel_size=3, stride=1, padding=1)
        _kaiming_like_reference(self)
        self._cfg = (0, in_ch, ou_ch, upscale_factor, base_kernel)
        self.compute_dtype = N.dtype_name(dtype)

    def forward(self, x):
        return _oplist_forward(x, _SRNET, (*self._cfg, N.dtype_id(self.compute_dtype)), list(self.parameters()))


class SRCNN(_NativeRepr, nn.Module):
    """Drop-in for reference ``model.SRCNN`` (src/model/srcnn.py:17-42): 9x9, 1x1, 5x5 convolutions, each followed by ReLU;
    the output has the input's size (``upscale_factor`` is stored and unused, as in the reference); torch default init."""

    def __init__(self, in_ch=3, ou_ch=3, upscale_factor=2, base_kernel=64, dtype=None):
        super().__init__()
        kernels = [int(x * base_kernel) for x in [1, 1 / 2]]
        self.up = upscale_factor
        self.relu = nn.ReLU(True)
        self.conv1 = nn.Conv2d(in_ch, kernels[0], kernel_size=9, stride=1, padding=4)
        self.conv2 = nn.Conv2d(kernels[0], kernels[1], kernel_size=1, stride=1, padding=0)
        self.conv3 = nn.Conv2d(kernels[1], ou_ch, kernel_size=5, stride=1, padding=2)
        self._cfg = (1, in_ch, ou_ch, upscale_factor, base_kernel)
        self.compute_dtype = N.dtype_name(dtype)

    def forward(self, x):
        return _oplist_forward(x, _SRNET, (*self._cfg, N.dtype_id(self.compute_dtype)), list(self.parameters()))


class _EdsrBlock(_HolderOnly):
    """Parameter holder of edsr.py:37-50 ResnetBlock: conv1, conv2, ONE GroupNorm(32) applied after each."""

    def __init__(self, num_channel):
        super().__init__()
        self.conv1 = nn.Conv2d(num_channel, num_channel, 3, 1, 1)
        self.conv2 = nn.Conv2d(num_channel, num_channel, 3, 1, 1)
        self.gn = nn.GroupNorm(32, num_channel)
        self.activation = nn.LeakyReLU(negative_slope=0.2, inplace=True)


class EDSR(_NativeRepr, nn.Module):
    """Drop-in for reference ``model.EDSR`` (src/model/edsr.py:68-110): ``EDSR(in_ch, ou_ch, upscale_factor=2, base_channel=64,
    num_residuals=50)``."""

    def __init__(self, in_ch, ou_ch, upscale_factor=2, base_channel=64, num_residuals=50, dtype=None):
        super().__init__()
        self.input_conv = nn.Conv2d(in_ch, base_channel, kernel_size=3, stride=1, padding=1)
        self.residual_layers = nn.Sequential(*[_EdsrBlock(base_channel) for _ in range(num_residuals)])
        self.mid_conv = nn.Conv2d(base_channel, base_channel, kernel_size=3, stride=1, padding=1)
        self.upscale_layers = nn.Sequential(*[nn.ConvTranspose2d(base_channel, base_channel, 2, 2, 0, bias=False)
                                              for _ in range(int(math.log2(upscale_factor)))])
        self.output_conv = nn.Conv2d(base_channel, ou_ch, kernel_size=3, stride=1, padding=1)
        _kaiming_like_reference(self)
        self._cfg = (2, in_ch, ou_ch, upscale_factor, base_channel)
        self._nres = num_residuals
        self.compute_dtype = N.dtype_name(dtype)

    def forward(self, x):
        return _oplist_forward(x, _SRNET, (*self._cfg, N.dtype_id(self.compute_dtype), self._nres), list(self.parameters()))


class SRDN(_NativeRepr, nn.Module):
    """Drop-in for reference ``model.SRDN`` (src/model/srdn.py:56-74): conv_first -> RRDB_encoder (nb RRDBs) -> + skip ->
    RRDB_decoder (nb RRDBs) -> + skip -> conv_last; same resolution in and out (``upscale_factor`` is stored and unused, and
    ``trunk_conv`` exists in the state_dict but is never applied -- it receives no gradient, as in the reference)."""

    def __init__(self, in_ch, ou_ch, upscale_factor, nf=64, nb=3, gc=32, dtype=None):
        super().__init__()
        self.upscale_factor = upscale_factor
        self.conv_first = nn.Conv2d(in_ch, nf, 3, 1, 1, bias=True)
        self.RRDB_encoder = nn.Sequential(*[RRDB(nf=nf, gc=gc) for _ in range(nb)])
        self.trunk_conv = nn.Conv2d(nf, nf, 3, 1, 1, bias=True)
        self.RRDB_decoder = nn.Sequential(*[RRDB(nf=nf, gc=gc) for _ in range(nb)])
        self.conv_last = nn.Conv2d(nf, ou_ch, 3, 1, 1, bias=False)
        _kaiming_like_reference(self)
        self._cfg = (in_ch, ou_ch, 1, nf, nb, gc)
        self.compute_dtype = N.dtype_name(dtype)

    def forward(self, x):
        cfg = (*self._cfg, N.dtype_id(self.compute_dtype), 0, 3)
        skip = {id(self.trunk_conv.weight), id(self.trunk_conv.bias)}
        return _rddb_forward(x, cfg, [p.detach() if id(p) in skip else p for p in self.parameters()])


# ------------------------------------------------------------------------------------------------ SRDenseNetA / SRDenseNetB
class _SrDenseConv(_HolderOnly):
    """Parameter holder of model/model.py:643-660 ConvLayer / DenseLayer: one convolution under the key ``conv``."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=kernel_size // 2)
        self.relu = nn.ReLU(inplace=True)


class _SrDenseBlock(_HolderOnly):
    """Parameter holder of model/model.py:663-672 DenseBlock: ``block.<j>.conv``; layer 0 takes the block input, layer j > 0 the
    block-local concatenation of the j earlier outputs."""

    def __init__(self, in_channels, growth_rate, num_layers):
        super().__init__()
        layers = [_SrDenseConv(in_channels, growth_rate, 3)]
        for i in range(num_layers - 1):
            layers.append(_SrDenseConv(growth_rate * (i + 1), growth_rate, 3))
        self.block = nn.Sequential(*layers)


class SRDenseNetA(_NativeRepr, nn.Module):
    """LR -> HR SRDenseNet, drop-in for reference ``model.model.SRDenseNetA`` (model/model.py:675-729; train.py:165-168):
    ``SRDenseNetA(in_nc, out_nc, nb_channel=1, growth_rate=16, num_blocks=8, num_layers=8, mode='x2')``.  conv_first (to 1 channel) ->
    conv + ReLU -> dense blocks -> 1x1 bottleneck to 256 + ReLU -> ``deconv`` = ConvTranspose2d(256, 256, k3 s2 p1 output_padding 1) +
    ReLU once ('x2') or twice with the same weights ('x4') -> reconstruction -> conv_last.  ``forward(x[B,in_nc,H,W]) ->
    [B,out_nc,H*up,W*up]``, any H, W >= 1.  ``nb_channel`` must be 1 (the reference's own conv_first fixes it); any other mode leaves
    the resolution unchanged in the reference and is refused here."""

    _kind = 0
    _repr_mode = True

    def __init__(self, in_nc, out_nc, nb_channel=1, growth_rate=16, num_blocks=8, num_layers=8, mode="x2", dtype=None):
        super().__init__()
        if nb_channel != 1:
            raise NotImplementedError(f"{type(self).__name__}: nb_channel must be 1 -- conv_first always produces one channel "
                                      "(model/model.py:679,683), any other value fails in the reference's own forward")
        if mode not in ("x2", "x4"):
            raise NotImplementedError(f"{type(self).__name__}: mode {mode!r} is not supported (use 'x2' or 'x4')")
        self.mode = mode
        self.compute_dtype = N.dtype_name(dtype)
        self._cfg = (self._kind, in_nc, out_nc, growth_rate, num_blocks, num_layers, _MODES[mode])
        # the native planner owns the alignment rules: ask it (host code, no GPU needed) before any parameter is created
        probe = N.SrDenseCfg(self._kind, in_nc, out_nc, 1, 2, 2, N.dtype_id(self.compute_dtype), growth_rate, num_blocks, num_layers, _MODES[mode])
        if N.lib().srcgan_srdense_num_params(C.byref(probe)) < 0:
            raise ValueError(f"{type(self).__name__}: " + (N.lib().srcgan_last_error() or b"").decode())
        # creation order == the reference's
        self.conv_first = nn.Conv2d(in_nc, 1, 3, 1, 1, bias=True)
        self.conv = _SrDenseConv(nb_channel, growth_rate * num_layers, 3)
        self.dense_blocks = nn.Sequential(*[_SrDenseBlock(growth_rate * num_layers * (i + 1), growth_rate, num_layers) for i in range(num_blocks)])
        self.bottleneck = nn.Sequential(nn.Conv2d(growth_rate * num_layers * (num_blocks + 1), 256, kernel_size=1), nn.ReLU(inplace=True))
        self.deconv = nn.Sequential(self._sampler(), nn.ReLU(inplace=True))
        self.reconstruction = nn.Conv2d(256, nb_channel, kernel_size=3, padding=1)
        self.conv_last = nn.Conv2d(1, out_nc, 3, 1, 1, bias=True)
        # model.py:710-715: kaiming-normal (fan_in, relu) on every Conv2d / ConvTranspose2d weight in modules() order, zero biases
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.kaiming_normal_(m.weight.data, nonlinearity="relu")
                if m.bias is not None:
                    nn.init.zeros_(m.bias.data)

    @staticmethod
    def _sampler():
        return nn.ConvTranspose2d(256, 256, kernel_size=3, stride=2, padding=1, output_padding=1)

    def forward(self, x):
        return _oplist_forward(x, _SRDENSE, (*self._cfg, N.dtype_id(self.compute_dtype)), list(self.parameters()))


class SRDenseNetB(SRDenseNetA):
    """HR -> LR SRDenseNet, drop-in for reference ``model.model.SRDenseNetB`` (model/model.py:732-786): as SRDenseNetA with
    ``deconv`` = Conv2d(256, 256, k3 s2 p1) + ReLU, so each stage maps n to (n + 1) // 2: any H, W >= 2, odd sizes included."""

    _kind = 1

    @staticmethod
    def _sampler():
        return nn.Conv2d(256, 256, kernel_size=3, stride=2, padding=1)


# ------------------------------------------------------------------------------------------------ RCAN
_DIV2K_MEAN = (0.4488, 0.4371, 0.4040)          # the RGB mean of the DIV2K training set, as a fraction of the value range


class _MeanShift(nn.Conv2d):
    """The colour shift in front of and behind RCAN (common.py:11-21), kept as the frozen 1x1 convolution the reference's state_dict
    holds: y = x / std + sign * rgb_range * mean / std per colour.  The convolution is first made with torch's default initialisation,
    so a seeded construction draws the random numbers the reference's draws, and is then overwritten."""

    def __init__(self, rgb_range, sign=-1, rgb_mean=_DIV2K_MEAN, rgb_std=(1.0, 1.0, 1.0)):
        super().__init__(3, 3, kernel_size=1)
        mean, std = torch.tensor(rgb_mean, dtype=torch.float32), torch.tensor(rgb_std, dtype=torch.float32)
        self.weight.requires_grad_(False).copy_(torch.diag(1.0 / std).reshape(3, 3, 1, 1))
        self.bias.requires_grad_(False).copy_(mean * (sign * rgb_range) / std)

    def forward(self, *a, **k):  # pragma: no cover
        return _HolderOnly.forward(self, *a, **k)


class _CALayer(_HolderOnly):
    """Parameter holder of rcan.py:11-22 CALayer."""

    def __init__(self, channel, reduction=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.conv_du = nn.Sequential(nn.Conv2d(channel, channel // reduction, 1, padding=0, bias=True), nn.ReLU(inplace=True),
                                     nn.Conv2d(channel // reduction, channel, 1, padding=0, bias=True), nn.Sigmoid())


class _RCAB(_HolderOnly):
    """Parameter holder of rcan.py:30-43 RCAB: body = [conv, ReLU, conv, CALayer]."""

    def __init__(self, n_feat, reduction):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(n_feat, n_feat, 3, padding=1), nn.ReLU(True), nn.Conv2d(n_feat, n_feat, 3, padding=1), _CALayer(n_feat, reduction))


class _ResidualGroup(_HolderOnly):
    """Parameter holder of rcan.py:52-61 ResidualGroup: body = n_resblocks RCABs and a convolution."""

    def __init__(self, n_feat, reduction, n_resblocks):
        super().__init__()
        self.body = nn.Sequential(*[_RCAB(n_feat, reduction) for _ in range(n_resblocks)], nn.Conv2d(n_feat, n_feat, 3, padding=1))


def _rcan_cfg(x, items):
    n_colors, groups, blocks, feats, reduction, scale, dtype = items
    _check_input(x, "RCAN", n_colors, f"RCAN expects [B,{n_colors},H,W]")
    B, _, H, W = x.shape
    return N.RcanCfg(n_colors, n_colors, B, H, W, dtype, groups, blocks, feats, reduction, scale), (B, n_colors, H * scale, W * scale)


_RCAN = _OpList("RCAN", "srcgan_rcan", _rcan_cfg)


class RCAN(_NativeRepr, nn.Module):
    """Residual Channel Attention Network, drop-in for reference ``model.rcan.RCAN`` (src/model/rcan.py:69-142 with common.py):
    ``RCAN(args)`` with the reference's attribute names (``n_resgroups, n_resblocks, n_feats, reduction, scale`` -- a list, its first
    entry counts -- ``rgb_range, n_colors, res_scale``), or the same names as keywords.  sub_mean -> head -> n_resgroups residual
    groups of n_resblocks channel-attention blocks -> + head -> Upsampler (PixelShuffle) -> conv -> add_mean;
    ``forward(x[B,3,H,W]) -> [B,3,H*scale,W*scale]``.  ``res_scale`` is stored and unused, as in the reference (rcan.py:47).
    The two MeanShift layers are frozen (``requires_grad=False``) and run from their parameters, so a loaded ``rgb_range`` / ``rgb_std``
    is honoured.  Default torch initialisation, modules created in the reference's order: the same seed gives the same weights."""

    def __init__(self, args=None, *, n_resgroups=10, n_resblocks=20, n_feats=64, reduction=16, scale=2, rgb_range=255, n_colors=3,
                 res_scale=1, dtype=None):
        super().__init__()
        if args is not None:
            n_resgroups, n_resblocks = getattr(args, "n_resgroups", n_resgroups), getattr(args, "n_resblocks", n_resblocks)
            n_feats, reduction = getattr(args, "n_feats", n_feats), getattr(args, "reduction", reduction)
            scale, rgb_range = getattr(args, "scale", scale), getattr(args, "rgb_range", rgb_range)
            n_colors, res_scale = getattr(args, "n_colors", n_colors), getattr(args, "res_scale", res_scale)
        if isinstance(scale, (list, tuple)):
            scale = scale[0]
        scale = int(scale)
        self.compute_dtype = N.dtype_name(dtype)
        self.scale, self.res_scale = scale, res_scale
        self._cfg = (int(n_colors), int(n_resgroups), int(n_resblocks), int(n_feats), int(reduction), scale)
        # the native planner owns the rules (3 colours, scale 2 / 3 / 4 / 8, n_feats % 16, n_feats // reduction >= 1): ask it first
        probe = N.RcanCfg(self._cfg[0], self._cfg[0], 1, 8, 8, N.dtype_id(self.compute_dtype), *self._cfg[1:])
        if N.lib().srcgan_rcan_num_params(C.byref(probe)) < 0:
            raise ValueError("RCAN: " + (N.lib().srcgan_last_error() or b"").decode())
        # creation order == the reference's (rcan.py:82-100); registration order (= parameters() order) too (:82, 100, 102-104)
        sub_mean = _MeanShift(rgb_range)
        head = [nn.Conv2d(n_colors, n_feats, 3, padding=1)]
        body = [_ResidualGroup(n_feats, reduction, n_resblocks) for _ in range(n_resgroups)]
        body.append(nn.Conv2d(n_feats, n_feats, 3, padding=1))
        ups = []
        for _ in range(1 if scale == 3 else int(math.log2(scale))):
            r = 3 if scale == 3 else 2
            ups += [nn.Conv2d(n_feats, r * r * n_feats, 3, padding=1), nn.PixelShuffle(r)]
        tail = [nn.Sequential(*ups), nn.Conv2d(n_feats, n_colors, 3, padding=1)]
        self.sub_mean = sub_mean
        self.add_mean = _MeanShift(rgb_range, sign=1)
        self.head = nn.Sequential(*head)
        self.body = nn.Sequential(*body)
        self.tail = nn.Sequential(*tail)

    def forward(self, x):
        return _oplist_forward(x, _RCAN, (*self._cfg, N.dtype_id(self.compute_dtype)), list(self.parameters()))

    def load_state_dict(self, state_dict, strict=False, assign=False):
        """The reference's tolerant loader (rcan.py:118-142): entries are copied by name; one that does not fit is skipped when it
        belongs to the tail (a checkpoint trained for another scale) and raises otherwise.  ``strict``: unknown names outside the tail
        and missing names raise KeyError."""
        own = self.state_dict()
        for name, value in state_dict.items():
            if name in own:
                try:
                    own[name].copy_(value.data if isinstance(value, nn.Parameter) else value)
                except Exception:
                    if "tail" not in name:
                        raise RuntimeError(f"RCAN.load_state_dict: {name} has shape {tuple(own[name].shape)} in the model and "
                                           f"{tuple(value.shape)} in the checkpoint")
            elif strict and "tail" not in name:
                raise KeyError(f'unexpected key "{name}" in state_dict')
        if strict:
            missing = set(own) - set(state_dict)
            if missing:
                raise KeyError(f"missing keys in state_dict: {sorted(missing)}")


# ------------------------------------------------------------------------------------------------ DDBPN
_DDBPN_PROJ = {2: (6, 2, 2), 4: (8, 4, 2), 8: (12, 8, 2)}      # scale -> (kernel, stride, padding) of a projection (ddbpn.py:14-18)


class _DenseProjection(_HolderOnly):
    """Parameter holder of ddbpn.py:29-53 DenseProjection: [bottleneck = 1x1 conv + PReLU,] conv_1 .. conv_3 = projection + PReLU, the
    projections alternating ConvTranspose2d / Conv2d (up) or Conv2d / ConvTranspose2d (down)."""

    def __init__(self, in_channels, nr, scale, up=True, bottleneck=True):
        super().__init__()
        k, s, p = _DDBPN_PROJ[scale]
        proj = lambda ci, co, t: (nn.ConvTranspose2d if t else nn.Conv2d)(ci, co, k, stride=s, padding=p)
        if bottleneck:
            self.bottleneck = nn.Sequential(nn.Conv2d(in_channels, nr, 1), nn.PReLU(nr))
            inter = nr
        else:
            self.bottleneck = None
            inter = in_channels
        self.conv_1 = nn.Sequential(proj(inter, nr, up), nn.PReLU(nr))
        self.conv_2 = nn.Sequential(proj(nr, inter, not up), nn.PReLU(inter))
        self.conv_3 = nn.Sequential(proj(inter, nr, up), nn.PReLU(nr))


def _ddbpn_cfg(x, items):
    n_colors, scale, dtype = items
    _check_input(x, "DDBPN", n_colors, f"DDBPN expects [B,{n_colors},H,W]")
    B, _, H, W = x.shape
    return N.DdbpnCfg(n_colors, n_colors, B, H, W, dtype, scale), (B, n_colors, H * scale, W * scale)


_DDBPN = _OpList("DDBPN", "srcgan_ddbpn", _ddbpn_cfg)


class DDBPN(_NativeRepr, nn.Module):
    """Dense Deep Back-Projection Network (arXiv 1803.02735), drop-in for reference ``model.ddbpn.DDBPN`` (src/model/ddbpn.py:68-130):
    ``DDBPN(args)`` with the reference's attribute names (``scale`` -- a list, its first entry counts -- ``rgb_range, n_colors``), or the
    same names as keywords.  sub_mean -> initial (3x3 + PReLU, 1x1 + PReLU) -> six up- and five down-projection modules, each fed the
    concatenation of all earlier outputs at its resolution -> 3x3 reconstruction over the six HR outputs -> add_mean;
    ``forward(x[B,3,H,W]) -> [B,3,H*scale,W*scale]``, scale 2, 4 or 8.  n0 = 128, nr = 32 and depth = 6 are the reference's constants.
    The two MeanShift layers are frozen and run from their parameters.  Default torch initialisation, modules created in the
    reference's order: the same seed gives the same weights, and ``state_dict`` has the reference's keys."""

    def __init__(self, args=None, *, scale=2, rgb_range=255, n_colors=3, dtype=None):
        super().__init__()
        if args is not None:
            scale, rgb_range = getattr(args, "scale", scale), getattr(args, "rgb_range", rgb_range)
            n_colors = getattr(args, "n_colors", n_colors)
        if isinstance(scale, (list, tuple)):
            scale = scale[0]
        scale = int(scale)
        self.compute_dtype = N.dtype_name(dtype)
        self.scale, self.depth = scale, 6
        self._cfg = (int(n_colors), scale)
        # the native planner owns the rules (3 colours, scale 2 / 4 / 8): ask it first
        probe = N.DdbpnCfg(self._cfg[0], self._cfg[0], 1, 8, 8, N.dtype_id(self.compute_dtype), scale)
        if N.lib().srcgan_ddbpn_num_params(C.byref(probe)) < 0:
            raise ValueError("DDBPN: " + (N.lib().srcgan_last_error() or b"").decode())
        n0, nr = 128, 32
        rgb_mean, rgb_std = _DIV2K_MEAN, (1.0, 1.0, 1.0)
        # creation order == registration order == the reference's (ddbpn.py:79-110)
        self.sub_mean = _MeanShift(rgb_range, rgb_mean=rgb_mean, rgb_std=rgb_std, sign=-1)
        self.initial = nn.Sequential(nn.Conv2d(n_colors, n0, 3, padding=1), nn.PReLU(n0), nn.Conv2d(n0, nr, 1), nn.PReLU(nr))
        self.upmodules = nn.ModuleList()
        self.downmodules = nn.ModuleList()
        channels = nr
        for i in range(self.depth):
            self.upmodules.append(_DenseProjection(channels, nr, scale, True, i > 1))
            if i != 0:
                channels += nr
        channels = nr
        for i in range(self.depth - 1):
            self.downmodules.append(_DenseProjection(channels, nr, scale, False, i != 0))
            channels += nr
        self.reconstruction = nn.Sequential(nn.Conv2d(self.depth * nr, n_colors, 3, padding=1))
        self.add_mean = _MeanShift(rgb_range, rgb_mean=rgb_mean, rgb_std=rgb_std, sign=1)

    def forward(self, x):
        return _oplist_forward(x, _DDBPN, (*self._cfg, N.dtype_id(self.compute_dtype)), list(self.parameters()))


# ------------------------------------------------------------------------------------------------ RDN
_RDN_CONFIG = {"A": (20, 6, 32), "B": (16, 8, 64)}       # RDNconfig -> (D blocks, C layers per block, G growth) (rdn.py:53-56)


class _RDBConv(_HolderOnly):
    """Parameter holder of rdn.py:13-21 RDB_Conv: conv = [3x3, ReLU]."""

    def __init__(self, in_channels, grow_rate):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_channels, grow_rate, 3, padding=1, stride=1), nn.ReLU())


class _RDB(_HolderOnly):
    """Parameter holder of rdn.py:27-40 RDB: convs = C dense layers, LFF = the 1x1 local feature fusion."""

    def __init__(self, G0, G, C):
        super().__init__()
        self.convs = nn.Sequential(*[_RDBConv(G0 + c * G, G) for c in range(C)])
        self.LFF = nn.Conv2d(G0 + C * G, G0, 1, padding=0, stride=1)


def _rdn_cfg(x, items):
    n_colors, scale, G0, D, Cl, G, dtype = items
    _check_input(x, "RDN", n_colors, f"RDN expects [B,{n_colors},H,W]")
    B, _, H, W = x.shape
    return N.RdnCfg(n_colors, B, H, W, dtype, scale, G0, D, Cl, G), (B, n_colors, H * scale, W * scale)


_RDN = _OpList("RDN", "srcgan_rdn", _rdn_cfg)


class RDN(_NativeRepr, nn.Module):
    """Residual Dense Network (arXiv 1802.08797), drop-in for reference ``model.rdn.RDN`` (src/model/rdn.py:45-105): ``RDN(args)`` with the
    reference's attribute names (``scale`` -- a list, its first entry counts -- ``G0, RDNkSize, RDNconfig, n_colors``), or the same names as
    keywords.  SFENet1 -> SFENet2 -> D residual dense blocks (C 3x3 + ReLU layers on the growing concatenation, a 1x1 local fusion, + the
    block's input) -> GFF (1x1 over all D block outputs, 3x3) + SFENet1's output -> UPNet (PixelShuffle);
    ``forward(x[B,n_colors,H,W]) -> [B,n_colors,H*scale,W*scale]``, scale 2, 3 or 4.  ``RDNconfig`` is 'A' (D, C, G = 20, 6, 32), 'B'
    (16, 8, 64) or, beyond the reference, a tuple ``(D, C, G)``; G0 and G must be multiples of 32.  No concatenation is made (DESIGN.md
    section 3.11).  Default torch initialisation, modules created in the reference's order: the same seed gives the same weights, and
    ``state_dict`` has the reference's keys."""

    def __init__(self, args=None, *, scale=2, G0=64, RDNkSize=3, RDNconfig="B", n_colors=3, dtype=None):
        super().__init__()
        if args is not None:
            scale, G0, RDNkSize = getattr(args, "scale", scale), getattr(args, "G0", G0), getattr(args, "RDNkSize", RDNkSize)
            RDNconfig, n_colors = getattr(args, "RDNconfig", RDNconfig), getattr(args, "n_colors", n_colors)
        if isinstance(scale, (list, tuple)):
            scale = scale[0]
        scale, G0, n_colors = int(scale), int(G0), int(n_colors)
        if int(RDNkSize) != 3:
            raise NotImplementedError(f"RDN: RDNkSize = {RDNkSize}; the native network has the reference's default, 3x3 convolutions")
        if isinstance(RDNconfig, str):
            if RDNconfig not in _RDN_CONFIG:
                raise KeyError(RDNconfig)          # the reference's own failure (rdn.py:53-56)
            RDNconfig = _RDN_CONFIG[RDNconfig]
        D, Cl, G = (int(v) for v in RDNconfig)
        if scale not in (2, 3, 4):
            raise ValueError("scale must be 2 or 3 or 4.")      # rdn.py:91
        self.compute_dtype = N.dtype_name(dtype)
        self.scale, self.D, self.C, self.G, self.G0 = scale, D, Cl, G, G0
        self._cfg = (n_colors, scale, G0, D, Cl, G)
        # the native planner owns the rules (1..8 colours, G0 and G multiples of 32, at most 8192 channels in a dense buffer): ask it first
        probe = N.RdnCfg(n_colors, 1, 8, 8, N.dtype_id(self.compute_dtype), scale, G0, D, Cl, G)
        if N.lib().srcgan_rdn_num_params(C.byref(probe)) < 0:
            raise ValueError("RDN: " + (N.lib().srcgan_last_error() or b"").decode())
        # creation order == registration order == the reference's (rdn.py:59-89)
        self.SFENet1 = nn.Conv2d(n_colors, G0, 3, padding=1, stride=1)
        self.SFENet2 = nn.Conv2d(G0, G0, 3, padding=1, stride=1)
        self.RDBs = nn.ModuleList()
        for _ in range(D):
            self.RDBs.append(_RDB(G0, G, Cl))
        self.GFF = nn.Sequential(nn.Conv2d(D * G0, G0, 1, padding=0, stride=1), nn.Conv2d(G0, G0, 3, padding=1, stride=1))
        if scale == 4:
            self.UPNet = nn.Sequential(nn.Conv2d(G0, G * 4, 3, padding=1, stride=1), nn.PixelShuffle(2), nn.Conv2d(G, G * 4, 3, padding=1, stride=1),
                                       nn.PixelShuffle(2), nn.Conv2d(G, n_colors, 3, padding=1, stride=1))
        else:
            self.UPNet = nn.Sequential(nn.Conv2d(G0, G * scale * scale, 3, padding=1, stride=1), nn.PixelShuffle(scale),
                                       nn.Conv2d(G, n_colors, 3, padding=1, stride=1))

    def forward(self, x):
        return _oplist_forward(x, _RDN, (*self._cfg, N.dtype_id(self.compute_dtype)), list(self.parameters()))


# ------------------------------------------------------------------------------------------------ MDSR, VDSR
# the reference's checkpoint addresses (mdsr.py:5-8, vdsr.py:6-8); never fetched
_MDSR_URL = {"r16f64": "https://cv.snu.ac.kr/research/EDSR/models/mdsr_baseline-a00cab12.pt",
             "r80f64": "https://cv.snu.ac.kr/research/EDSR/models/mdsr-4a78bedf.pt"}
_VDSR_URL = {"r20f64": ""}


class _ResBlock(_HolderOnly):
    """Parameter holder of common.py:36-57 ResBlock (no BatchNorm, res_scale 1): body = [conv, ReLU, conv]."""

    def __init__(self, n_feats, kernel_size):
        super().__init__()
        pad = kernel_size // 2
        self.body = nn.Sequential(nn.Conv2d(n_feats, n_feats, kernel_size, padding=pad), nn.ReLU(True), nn.Conv2d(n_feats, n_feats, kernel_size, padding=pad))
        self.res_scale = 1


def _upsampler(scale, n_feats):
    """common.py:59-86 Upsampler without BatchNorm or activation: [3x3 to 4 F, PixelShuffle(2)] per x2 stage, [3x3 to 9 F, PixelShuffle(3)]."""
    m = []
    for _ in range(1 if scale == 3 else int(math.log2(scale))):
        r = 3 if scale == 3 else 2
        m += [nn.Conv2d(n_feats, r * r * n_feats, 3, padding=1), nn.PixelShuffle(r)]
    return nn.Sequential(*m)


def _mdsr_cfg(x, items):
    n_resblocks, n_feats, scales, scale_idx, dtype = items
    _check_input(x, "MDSR", 3, "MDSR expects [B,3,H,W]")
    B, _, H, W = x.shape
    s = scales[scale_idx]
    return (N.MdsrCfg(3, 3, B, H, W, dtype, n_resblocks, n_feats, len(scales), (C.c_int * 4)(*scales), scale_idx), (B, 3, H * s, W * s))


def _vdsr_cfg(x, items):
    n_resblocks, n_feats, dtype = items
    _check_input(x, "VDSR", 3, "VDSR expects [B,3,H,W]")
    B, _, H, W = x.shape
    return N.VdsrCfg(3, B, H, W, dtype, n_resblocks, n_feats), (B, 3, H, W)


_MDSR = _OpList("MDSR", "srcgan_mdsr", _mdsr_cfg)
_VDSR = _OpList("VDSR", "srcgan_vdsr", _vdsr_cfg)


class MDSR(_NativeRepr, nn.Module):
    """Multi-scale EDSR (arXiv 1707.02921), drop-in for reference ``model.mdsr.MDSR`` (src/model/mdsr.py:13-66 with common.py): ``MDSR(args)``
    with the reference's attribute names (``n_resblocks, n_feats, scale`` -- the list of scales -- ``rgb_range, n_colors``), or the same
    names as keywords.  sub_mean -> head -> pre_process[scale_idx] (two 5x5 ResBlocks) -> body (n_resblocks 3x3 ResBlocks, a 3x3) + the
    pre_process output -> upsample[scale_idx] (PixelShuffle) -> tail -> add_mean; ``forward(x[B,3,H,W]) -> [B,3,H*s,W*s]`` with
    ``s = scale[scale_idx]``, each scale 2, 3, 4 or 8, at most four of them.  ``set_scale(i)`` chooses the branch of the next forward;
    the other branches stay in the ``state_dict``, cost nothing and their ``.grad`` stays None, as in the reference.  In a data-parallel
    step all ranks must use the same ``scale_idx`` (``GradSync`` reduces the gradients that exist).

    Unlike the reference, which looks ``url['r{}f{}']`` up and so raises KeyError for every size but r16f64 / r80f64, any size the native
    plan accepts is built: ``url`` is the reference's string where the key exists and None otherwise; nothing is ever fetched.
    Default torch initialisation with the modules CREATED in the reference's order (head, pre_process, body, upsample, tail:
    mdsr.py:25-45) and REGISTERED in its other one (pre_process, upsample, head, body, tail: :27, 41, 47-49): the same seed gives the
    same weights, and ``state_dict`` has the reference's keys in its order."""

    def __init__(self, args=None, *, n_resblocks=16, n_feats=64, scale=(2, 3, 4), rgb_range=255, n_colors=3, dtype=None):
        super().__init__()
        if args is not None:
            n_resblocks, n_feats = getattr(args, "n_resblocks", n_resblocks), getattr(args, "n_feats", n_feats)
            scale, rgb_range, n_colors = getattr(args, "scale", scale), getattr(args, "rgb_range", rgb_range), getattr(args, "n_colors", n_colors)
        scale = [int(s) for s in (scale if isinstance(scale, (list, tuple)) else [scale])]
        n_resblocks, n_feats = int(n_resblocks), int(n_feats)
        if int(n_colors) != 3:
            raise ValueError(f"MDSR: n_colors = {n_colors}; MeanShift is a 3-channel convolution (common.py:16)")
        self.compute_dtype = N.dtype_name(dtype)
        self.scale, self.n_resblocks, self.n_feats = scale, n_resblocks, n_feats
        self.scale_idx = 0
        self.url = _MDSR_URL.get(f"r{n_resblocks}f{n_feats}")
        # the native planner owns the rules (1..4 scales of 2 / 3 / 4 / 8, n_feats % 16, n_resblocks >= 1): ask it first
        probe = N.MdsrCfg(3, 3, 1, 8, 8, N.dtype_id(self.compute_dtype), n_resblocks, n_feats, len(scale), (C.c_int * 4)(*scale[:4]), 0)
        if N.lib().srcgan_mdsr_num_params(C.byref(probe)) < 0:
            raise ValueError("MDSR: " + (N.lib().srcgan_last_error() or b"").decode())
        # creation order: the reference's (mdsr.py:22-45); registration order (= parameters() order): its other one (:22-23, 27, 41, 47-49)
        self.sub_mean = _MeanShift(rgb_range)
        self.add_mean = _MeanShift(rgb_range, sign=1)
        head = [nn.Conv2d(3, n_feats, 3, padding=1)]
        self.pre_process = nn.ModuleList([nn.Sequential(_ResBlock(n_feats, 5), _ResBlock(n_feats, 5)) for _ in scale])
        body = [_ResBlock(n_feats, 3) for _ in range(n_resblocks)]
        body.append(nn.Conv2d(n_feats, n_feats, 3, padding=1))
        self.upsample = nn.ModuleList([_upsampler(s, n_feats) for s in scale])
        tail = [nn.Conv2d(n_feats, 3, 3, padding=1)]
        self.head = nn.Sequential(*head)
        self.body = nn.Sequential(*body)
        self.tail = nn.Sequential(*tail)

    def set_scale(self, scale_idx):
        self.scale_idx = scale_idx

    def forward(self, x):
        idx = int(self.scale_idx)
        if not 0 <= idx < len(self.scale):
            raise IndexError(f"MDSR: scale_idx = {self.scale_idx} with {len(self.scale)} scales")       # the reference's ModuleList would raise it
        # the other branches are not on the graph (mdsr.py:54, 59): pass their parameters detached so autograd leaves their .grad at None
        on = {id(p) for m in (self.pre_process[idx], self.upsample[idx]) for p in m.parameters()}
        off = {id(p) for m in (self.pre_process, self.upsample) for p in m.parameters()} - on
        ps = [p.detach() if id(p) in off else p for p in self.parameters()]
        return _oplist_forward(x, _MDSR, (self.n_resblocks, self.n_feats, tuple(self.scale), idx, N.dtype_id(self.compute_dtype)), ps)


class VDSR(_NativeRepr, nn.Module):
    """Very Deep Super-Resolution network (arXiv 1511.04587), drop-in for reference ``model.vdsr.VDSR`` (src/model/vdsr.py:13-45):
    ``VDSR(args)`` with the reference's attribute names (``n_resblocks, n_feats, rgb_range, n_colors``), or the same names as keywords.
    sub_mean -> n_resblocks 3x3 convolutions, all but the last with ReLU, + the sub_mean output -> add_mean; ``forward(x[B,3,H,W])`` has
    the input's size (the reference feeds it an interpolated image).  ``n_resblocks >= 2``.  ``url`` is the reference's string for r20f64
    and None for every other size, which the reference refuses with KeyError; nothing is ever fetched.  Default torch initialisation in the
    reference's order: the same seed gives the same weights, and ``state_dict`` has the reference's keys."""

    def __init__(self, args=None, *, n_resblocks=20, n_feats=64, rgb_range=255, n_colors=3, dtype=None):
        super().__init__()
        if args is not None:
            n_resblocks, n_feats = getattr(args, "n_resblocks", n_resblocks), getattr(args, "n_feats", n_feats)
            rgb_range, n_colors = getattr(args, "rgb_range", rgb_range), getattr(args, "n_colors", n_colors)
        n_resblocks, n_feats = int(n_resblocks), int(n_feats)
        if int(n_colors) != 3:
            raise ValueError(f"VDSR: n_colors = {n_colors}; MeanShift is a 3-channel convolution (common.py:16)")
        self.compute_dtype = N.dtype_name(dtype)
        self.n_resblocks, self.n_feats = n_resblocks, n_feats
        self.url = _VDSR_URL.get(f"r{n_resblocks}f{n_feats}")
        probe = N.VdsrCfg(3, 1, 8, 8, N.dtype_id(self.compute_dtype), n_resblocks, n_feats)
        if N.lib().srcgan_vdsr_num_params(C.byref(probe)) < 0:
            raise ValueError("VDSR: " + (N.lib().srcgan_last_error() or b"").decode())
        self.sub_mean = _MeanShift(rgb_range)
        self.add_mean = _MeanShift(rgb_range, sign=1)
        # BasicBlock (common.py:23-34) without BatchNorm: [conv, ReLU], the last one [conv]
        widths = [3] + [n_feats] * (n_resblocks - 1) + [3]
        self.body = nn.Sequential(*[nn.Sequential(nn.Conv2d(widths[k], widths[k + 1], 3, padding=1), *([nn.ReLU(True)] if k < n_resblocks - 1 else []))
                                    for k in range(n_resblocks)])

    def forward(self, x):
        return _oplist_forward(x, _VDSR, (self.n_resblocks, self.n_feats, N.dtype_id(self.compute_dtype)), list(self.parameters()))


# ------------------------------------------------------------------------------------------------ ResnetGenerator, define_G
class Identity(nn.Module):
    """The module ``get_norm_layer('none')`` puts where a normalisation layer would be: it returns its input."""

    def forward(self, x):
        return x


# norm_type -> the factory ``norm_layer(channels)`` of basicModel.get_norm_layer: BatchNorm2d with affine parameters and running
# statistics, InstanceNorm2d with neither, or no normalisation at all
_NORM_FACTORIES = {
    'batch': functools.partial(nn.BatchNorm2d, affine=True, track_running_stats=True),
    'instance': functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False),
    'none': lambda channels: Identity(),
}
# init_type -> what it does to a weight tensor (init_gain is unused by 'kaiming', as in the reference)
_WEIGHT_INITS = {
    'normal': lambda w, gain: nn.init.normal_(w, 0.0, gain),
    'xavier': lambda w, gain: nn.init.xavier_normal_(w, gain=gain),
    'kaiming': lambda w, gain: nn.init.kaiming_normal_(w, a=0, mode='fan_in'),
    'orthogonal': lambda w, gain: nn.init.orthogonal_(w, gain=gain),
}
_RESNET_BLOCKS = {'resnet_9blocks': 9, 'resnet_6blocks': 6}


def get_norm_layer(norm_type='instance'):
    """Same name, signature and results as the reference's ``basicModel.get_norm_layer``: 'batch' | 'instance' | 'none' -> a factory
    called with the channel count (the first two are ``functools.partial`` objects of the torch classes)."""
    if norm_type not in _NORM_FACTORIES:
        raise NotImplementedError(f'normalization layer [{norm_type}] is not found')
    return _NORM_FACTORIES[norm_type]


def _init_kind(m):
    """What init_weights does to a module, by the reference's rule on the class NAME: 'weights' for anything that owns a ``weight``
    and is called *Conv* or *Linear* (Conv2d, ConvTranspose2d, ...), 'batchnorm' for *BatchNorm2d*, None otherwise."""
    name = type(m).__name__
    if hasattr(m, 'weight') and ('Conv' in name or 'Linear' in name):
        return 'weights'
    return 'batchnorm' if 'BatchNorm2d' in name else None


def init_weights(net, init_type='normal', init_gain=0.02):
    """Same name, signature and results as the reference's ``basicModel.init_weights``: every convolution / linear weight is drawn by
    ``init_type`` ('normal': N(0, init_gain) | 'xavier' | 'kaiming' | 'orthogonal') and its bias zeroed; BatchNorm2d weights are drawn from
    N(1, init_gain), their biases zeroed.  The modules are visited in ``net.modules()`` order; the ones that draw are leaves, and the
    leaves come in the order ``net.apply`` visits them, so the same seed gives the reference's weights (the fixtures' sketches hold it)."""
    print(f'initialize network with {init_type}')
    for m in net.modules():
        kind = _init_kind(m)
        if kind == 'weights':
            if init_type not in _WEIGHT_INITS:
                raise NotImplementedError(f'initialization method [{init_type}] is not implemented')
            _WEIGHT_INITS[init_type](m.weight.data, init_gain)
            if getattr(m, 'bias', None) is not None:
                m.bias.data.zero_()
        elif kind == 'batchnorm':
            nn.init.normal_(m.weight.data, 1.0, init_gain)
            m.bias.data.zero_()


def init_net(net, init_type='normal', init_gain=0.02):
    """``init_weights`` on ``net``, which is returned (the reference's ``basicModel.init_net``)."""
    init_weights(net, init_type, init_gain)
    return net


def define_G(input_nc, output_nc, ngf, netG, norm='batch', use_dropout=False, init_type='normal', init_gain=0.02):
    """Same name and signature as the reference's ``basicModel.define_G``: ``netG`` 'resnet_9blocks' / 'resnet_6blocks' build the native
    ResnetGenerator with 9 / 6 blocks (which accepts ``norm='instance'`` alone) and initialise it with ``init_net``.

    'unet_128' / 'unet_256' are still refused here, although the class is native: build it with
    ``init_net(UnetGenerator(input_nc, output_nc, 7 | 8, ngf, norm_layer=get_norm_layer(norm)), init_type, init_gain)`` -- what the
    reference's ``define_G`` does, draw for draw.  Routing the two names is two lines in this function once
    tests/test_resnetgen_host.py::test_define_G_routes, which asserts the refusal, may change."""
    if netG in ('unet_128', 'unet_256'):
        raise NotImplementedError(f"UnetGenerator is not native through define_G yet: build it with init_net(UnetGenerator(input_nc, output_nc, "
                                  f"{7 if netG == 'unet_128' else 8}, ngf, norm_layer=get_norm_layer(norm)), init_type, init_gain)")
    if netG not in _RESNET_BLOCKS:
        raise NotImplementedError(f'Generator model name [{netG}] is not recognized')
    net = ResnetGenerator(input_nc, output_nc, ngf, norm_layer=get_norm_layer(norm), use_dropout=use_dropout, n_blocks=_RESNET_BLOCKS[netG])
    return init_net(net, init_type, init_gain)


class _ResnetBlock(_HolderOnly):
    """Parameter holder of basicModel.py:200-254 ResnetBlock with InstanceNorm2d and biases: conv_block = [pad, conv, norm, ReLU, pad, conv,
    norm] ('reflect') or [conv, norm, ReLU, conv, norm] ('zero')."""

    def __init__(self, dim, padding_type):
        super().__init__()
        blk = []
        for half in range(2):
            if padding_type == 'reflect':
                blk += [nn.ReflectionPad2d(1)]
            blk += [nn.Conv2d(dim, dim, kernel_size=3, padding=0 if padding_type == 'reflect' else 1, bias=True), nn.InstanceNorm2d(dim)]
            if half == 0:
                blk += [nn.ReLU(True)]
        self.conv_block = nn.Sequential(*blk)


def _resnetgen_cfg(x, items):
    in_ch, out_ch, ngf, n_blocks, padding, dtype = items
    _check_input(x, "ResnetGenerator", in_ch, f"expected [B,{in_ch},H,W]")
    B, _, H, W = x.shape
    return N.ResnetGenCfg(in_ch, out_ch, B, H, W, dtype, ngf, n_blocks, padding), (B, out_ch, H, W)


_RESNETGEN = _OpList("ResnetGenerator", "srcgan_resnetgen", _resnetgen_cfg)


class ResnetGenerator(_NativeRepr, nn.Module):
    """ResNet translator of CycleGAN / pix2pix, drop-in for reference ``model.basicModel.ResnetGenerator`` (src/model/basicModel.py:141-197), the
    network ``multi-task.py`` builds with ``define_G(1, 3, ngf, 'resnet_9blocks', 'instance', ...)``: ReflectionPad2d(3), 7x7, IN, ReLU; two
    3x3 stride-2 convolutions, each IN + ReLU; ``n_blocks`` ResnetBlocks [pad 1, 3x3, IN, ReLU, pad 1, 3x3, IN, + x]; two
    ConvTranspose2d(k3, s2, p1, output_padding 1), each IN + ReLU; ReflectionPad2d(3), 7x7, Tanh.  ``forward(x[B,input_nc,H,W]) ->
    [B,output_nc,H,W]``, H and W multiples of 4, at least 8; ``ngf`` a multiple of 16; 1..8 channels in and out.

    Native: ``norm_layer`` = ``nn.InstanceNorm2d`` or the ``functools.partial`` of ``get_norm_layer('instance')`` (affine=False,
    track_running_stats=False), ``padding_type`` 'reflect' or 'zero', no dropout.  BatchNorm -- the class default, as in the reference --
    the identity norm, 'replicate' and dropout raise NotImplementedError.  ``state_dict`` has the reference's keys (``model.1.weight`` ...;
    36 tensors for 6 blocks): ``model`` is an nn.Sequential with the parameter-free layers in their places, created in the reference's
    order, so the same seed gives the same weights."""

    def __init__(self, input_nc, output_nc, ngf=64, norm_layer=nn.BatchNorm2d, use_dropout=False, n_blocks=6, padding_type='reflect', dtype=None):
        assert n_blocks >= 0
        super().__init__()
        nkw = {}
        if isinstance(norm_layer, functools.partial):
            nkw, norm_layer = dict(norm_layer.keywords), norm_layer.func
        if norm_layer is nn.BatchNorm2d:
            raise NotImplementedError("native ResnetGenerator: norm_layer = nn.BatchNorm2d (the class default; define_G's norm='batch') is not "
                                      "implemented -- the op-list executor has no BatchNorm; use nn.InstanceNorm2d (norm='instance')")
        if norm_layer is not nn.InstanceNorm2d:
            raise NotImplementedError("native ResnetGenerator: the identity norm (get_norm_layer('none')) and other norm_layer factories are not "
                                      "implemented; use nn.InstanceNorm2d (norm='instance')")
        if nkw.get("affine", False) or nkw.get("track_running_stats", False):
            raise NotImplementedError("native ResnetGenerator: InstanceNorm2d with affine=True or track_running_stats=True is not implemented "
                                      "(get_norm_layer('instance') builds it without either)")
        if use_dropout:
            raise NotImplementedError("native ResnetGenerator: use_dropout=True is not implemented")
        if padding_type == 'replicate':
            raise NotImplementedError("native ResnetGenerator: padding_type 'replicate' is not implemented (use 'reflect' or 'zero')")
        if padding_type not in ('reflect', 'zero'):
            raise NotImplementedError('padding [%s] is not implemented' % padding_type)
        input_nc, output_nc, ngf, n_blocks = int(input_nc), int(output_nc), int(ngf), int(n_blocks)
        self.compute_dtype = N.dtype_name(dtype)
        self._cfg = (input_nc, output_nc, ngf, n_blocks, 0 if padding_type == 'reflect' else 1)
        # the native planner owns the rules (ngf % 16, 1..8 channels): ask it first
        probe = N.ResnetGenCfg(input_nc, output_nc, 1, 8, 8, N.dtype_id(self.compute_dtype), ngf, n_blocks, self._cfg[4])
        if N.lib().srcgan_resnetgen_num_params(C.byref(probe)) < 0:
            raise ValueError("ResnetGenerator: " + (N.lib().srcgan_last_error() or b"").decode())
        # the layers in the reference's order (creation order = the order the seeded weights are drawn in; index = state_dict key)
        act_norm = lambda c: [nn.InstanceNorm2d(c, affine=False, track_running_stats=False), nn.ReLU(True)]
        widths = [ngf, 2 * ngf, 4 * ngf]
        model = [nn.ReflectionPad2d(3), nn.Conv2d(input_nc, ngf, 7), *act_norm(ngf)]
        for cin, cout in zip(widths, widths[1:]):
            model += [nn.Conv2d(cin, cout, 3, stride=2, padding=1), *act_norm(cout)]
        model += [_ResnetBlock(widths[-1], padding_type) for _ in range(n_blocks)]
        for cin, cout in zip(widths[::-1], widths[-2::-1]):
            model += [nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1), *act_norm(cout)]
        model += [nn.ReflectionPad2d(3), nn.Conv2d(ngf, output_nc, 7), nn.Tanh()]
        self.model = nn.Sequential(*model)

    def forward(self, input):
        return _oplist_forward(input, _RESNETGEN, (*self._cfg, N.dtype_id(self.compute_dtype)), list(self.parameters()))


# ------------------------------------------------------------------------------------------------ UnetGenerator
class _UnetSkipBlock(_HolderOnly):
    """Parameter holder of basicModel.py:288-354 UnetSkipConnectionBlock with InstanceNorm2d and biases: ``model`` is the reference's
    nn.Sequential -- [downconv, submodule, ReLU, upconv, Tanh] (outermost), [LeakyReLU, downconv, ReLU, upconv, norm] (innermost),
    [LeakyReLU, downconv, norm, submodule, ReLU, upconv, norm] otherwise -- so the state_dict keys nest as the reference's do."""

    def __init__(self, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False):
        super().__init__()
        norm = lambda c: nn.InstanceNorm2d(c, affine=False, track_running_stats=False)
        downconv = nn.Conv2d(outer_nc if input_nc is None else input_nc, inner_nc, kernel_size=4, stride=2, padding=1, bias=True)
        downrelu, downnorm, uprelu, upnorm = nn.LeakyReLU(0.2, True), norm(inner_nc), nn.ReLU(True), norm(outer_nc)
        upconv = nn.ConvTranspose2d(inner_nc if innermost else inner_nc * 2, outer_nc, kernel_size=4, stride=2, padding=1, bias=True)
        if outermost:
            model = [downconv, submodule, uprelu, upconv, nn.Tanh()]
        elif innermost:
            model = [downrelu, downconv, uprelu, upconv, upnorm]
        else:
            model = [downrelu, downconv, downnorm, submodule, uprelu, upconv, upnorm]
        self.model = nn.Sequential(*model)


def _unet_cfg(x, items):
    in_ch, out_ch, ngf, num_downs, dtype = items
    _check_input(x, "UnetGenerator", in_ch, f"expected [B,{in_ch},H,W]")
    B, _, H, W = x.shape
    return N.UnetCfg(in_ch, out_ch, B, H, W, dtype, ngf, num_downs), (B, out_ch, H, W)


_UNET = _OpList("UnetGenerator", "srcgan_unet", _unet_cfg)


class UnetGenerator(_NativeRepr, nn.Module):
    """U-Net translator of pix2pix, drop-in for reference ``model.basicModel.UnetGenerator`` (src/model/basicModel.py:257-354), what its
    ``define_G(.., 'unet_128' | 'unet_256', ..)`` builds with ``num_downs`` 7 | 8: ``num_downs`` 4x4 stride-2 convolutions down to
    ngf min(2^(l-1), 8) channels at level l (LeakyReLU(0.2) in front of each but the first, InstanceNorm behind each but the first and
    the last), the mirrored ConvTranspose2d(k4, s2, p1) back up (ReLU in front, InstanceNorm behind each but the last), a skip connection
    around every level but the outermost, Tanh.  ``forward(x[B,input_nc,H,W]) -> [B,output_nc,H,W]``, H and W multiples of
    2^num_downs; ``num_downs`` >= 5; ``ngf`` 16, 32, 64 or 128; 1..8 channels in and out.

    Native: ``norm_layer`` = ``nn.InstanceNorm2d`` or the ``functools.partial`` of ``get_norm_layer('instance')``, no dropout.  BatchNorm
    -- the class default, as in the reference -- the identity norm, affine / tracked InstanceNorm and dropout raise NotImplementedError.
    The skip connection is one buffer written in place by its two producers, never a ``torch.cat``.  ``state_dict`` has the reference's
    nested keys (``model.model.0.weight``, ``model.model.1.model.1.weight``, ..., ``model.model.3.bias``): the inner blocks are parameter
    holders without a forward of their own, created innermost first as in the reference, so the same seed gives the same weights.
    ``define_G`` does not route to this class yet (see there): ``init_net(UnetGenerator(...), init_type, init_gain)`` is its equal."""

    def __init__(self, input_nc, output_nc, num_downs, ngf=64, norm_layer=nn.BatchNorm2d, use_dropout=False, dtype=None):
        super().__init__()
        nkw = {}
        if isinstance(norm_layer, functools.partial):
            nkw, norm_layer = dict(norm_layer.keywords), norm_layer.func
        if norm_layer is nn.BatchNorm2d:
            raise NotImplementedError("native UnetGenerator: norm_layer = nn.BatchNorm2d (the class default; define_G's norm='batch') is not "
                                      "implemented -- the op-list executor has no BatchNorm; use nn.InstanceNorm2d (norm='instance')")
        if norm_layer is not nn.InstanceNorm2d:
            raise NotImplementedError("native UnetGenerator: the identity norm (get_norm_layer('none')) and other norm_layer factories are not "
                                      "implemented; use nn.InstanceNorm2d (norm='instance')")
        if nkw.get("affine", False) or nkw.get("track_running_stats", False):
            raise NotImplementedError("native UnetGenerator: InstanceNorm2d with affine=True or track_running_stats=True is not implemented "
                                      "(get_norm_layer('instance') builds it without either)")
        if use_dropout:
            raise NotImplementedError("native UnetGenerator: use_dropout=True is not implemented")
        input_nc, output_nc, num_downs, ngf = int(input_nc), int(output_nc), int(num_downs), int(ngf)
        self.compute_dtype = N.dtype_name(dtype)
        self.num_downs = num_downs
        self._cfg = (input_nc, output_nc, ngf, num_downs)
        # the native planner owns the rules (num_downs >= 5, ngf, 1..8 channels): ask it first, on the smallest image it takes
        side = 1 << max(min(num_downs, 24), 0)
        probe = N.UnetCfg(input_nc, output_nc, 1, side, side, N.dtype_id(self.compute_dtype), ngf, num_downs)
        if N.lib().srcgan_unet_num_params(C.byref(probe)) < 0:
            raise ValueError("UnetGenerator: " + (N.lib().srcgan_last_error() or b"").decode())
        # the blocks in the reference's order, innermost first (creation order = the order the seeded weights are drawn in)
        block = _UnetSkipBlock(ngf * 8, ngf * 8, innermost=True)
        for _ in range(num_downs - 5):
            block = _UnetSkipBlock(ngf * 8, ngf * 8, submodule=block)
        for mult in (4, 2, 1):
            block = _UnetSkipBlock(ngf * mult, ngf * mult * 2, submodule=block)
        self.model = _UnetSkipBlock(output_nc, ngf, input_nc=input_nc, submodule=block, outermost=True)

    def forward(self, input):
        return _oplist_forward(input, _UNET, (*self._cfg, N.dtype_id(self.compute_dtype)), list(self.parameters()))


class _NLayerDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg_items, running, nbt, *params):
        lib = N.lib()
        in_ch, ndf, n_layers, dtype, training, pstate = cfg_items[:6]
        norm = cfg_items[6] if len(cfg_items) > 6 else 0
        x = _input(x, "NLayerDiscriminator", in_ch, f"NLayerDiscriminator expects [B,{in_ch},H,W]")
        B, _, H, W = x.shape
        cfg = N.NLayerDCfg(in_ch, ndf, n_layers, B, H, W, dtype, int(training), norm)
        plist = _params(params, "NLayerDiscriminator")
        oh, ow = C.c_int(), C.c_int()
        N.check(lib.srcgan_nlayerd_out_hw(C.byref(cfg), C.byref(oh), C.byref(ow)), "srcgan_nlayerd_out_hw")
        ws = N.workspace(lib.srcgan_nlayerd_ws_bytes(C.byref(cfg)), x.device)
        y = torch.empty(B, 1, oh.value, ow.value, dtype=torch.float32, device=x.device)
        layout = (in_ch, ndf, n_layers, dtype, H % 2, W % 2, norm)    # (the first layer's packed form depends on the parity of H, W)
        opt = pstate.opts(lib.srcgan_nlayerd_wpack_bytes, cfg, plist, layout, False, x.device)
        N.check(lib.srcgan_nlayerd_forward_ex(C.byref(cfg), x.data_ptr(), N.ptr_array(plist), N.ptr_array(running),
                                              N.ptr_array(nbt), ws.data_ptr(), y.data_ptr(), C.byref(opt), N.stream_ptr(x.device)),
                "srcgan_nlayerd_forward")
        pstate.done(False)
        ctx.cfg, ctx.ws = cfg, ws
        ctx.pstate, ctx.layout = pstate, layout
        ctx.save_for_backward(*plist)
        ctx.phase_hook = _phase_hook
        return y

    @staticmethod
    def backward(ctx, dy):
        lib, cfg = N.lib(), ctx.cfg
        dy, params, arena, grads, scratch, dx = _backward_operands(ctx, dy, 4, lib.srcgan_nlayerd_bwd_scratch_bytes, "NLayerDiscriminator")
        opt = ctx.pstate.opts(lib.srcgan_nlayerd_wpack_bytes, cfg, params, ctx.layout, True, dy.device)
        N.check(lib.srcgan_nlayerd_backward_ex(C.byref(cfg), dy.data_ptr(), N.ptr_array(params), ctx.ws.data_ptr(),
                                               scratch.data_ptr(), N.ptr_array(grads), dx.data_ptr() if dx is not None else None,
                                               C.byref(opt), N.stream_ptr(dy.device)), "srcgan_nlayerd_backward")
        ctx.pstate.done(True)
        ctx.ws = None
        if ctx.phase_hook is not None and arena is not None:
            ctx.phase_hook.phase_done(arena, params, 0, len(params), True)
        return (dx, None, None, None, *grads)


class NLayerDiscriminator(_NativeRepr, nn.Module):
    """PatchGAN discriminator, drop-in for reference ``model.model.NLayerDiscriminator``
    (model/model.py:595-639): conv4x4 s2 + LeakyReLU | (n-1) x [conv4x4 s2, BatchNorm2d, LeakyReLU] |
    conv4x4 s1, BN, LeakyReLU | conv4x4 s1 -> 1 channel.  BatchNorm uses per-replica batch statistics
    in train mode and updates the running buffers like nn.BatchNorm2d.

    ``norm_layer`` as in the reference: ``nn.BatchNorm2d`` (default) or ``nn.InstanceNorm2d`` -- the class or the
    ``functools.partial`` that ``basicModel.get_norm_layer`` builds (affine=False, track_running_stats=False); with InstanceNorm2d
    the normalised convolutions have a bias (model/model.py:607-610) and the layers normalise every image by its own statistics in
    train and eval mode."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d, dtype=None):
        super().__init__()
        nkw = {}
        if isinstance(norm_layer, functools.partial):
            nkw, norm_layer = dict(norm_layer.keywords), norm_layer.func
        if norm_layer is nn.InstanceNorm2d:
            if nkw.get("affine", False) or nkw.get("track_running_stats", False):
                raise NotImplementedError("native NLayerDiscriminator: InstanceNorm2d without affine parameters / running statistics "
                                          "(what nn.InstanceNorm2d defaults to and basicModel.get_norm_layer('instance') builds)")
            inorm = True
        elif norm_layer is nn.BatchNorm2d:
            if not nkw.get("affine", True) or not nkw.get("track_running_stats", True):
                raise NotImplementedError("native NLayerDiscriminator: BatchNorm2d with affine parameters and running statistics")
            inorm = False
        else:
            raise NotImplementedError("native NLayerDiscriminator implements norm_layer = nn.BatchNorm2d (the reference's default) or nn.InstanceNorm2d")
        norm = (lambda c: nn.InstanceNorm2d(c)) if inorm else (lambda c: nn.BatchNorm2d(c))
        kw, padw = 4, 1
        seq = [nn.Conv2d(input_nc, ndf, kw, 2, padw), nn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [nn.Conv2d(ndf * prev, ndf * mult, kw, 2, padw, bias=inorm), norm(ndf * mult), nn.LeakyReLU(0.2, True)]
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [nn.Conv2d(ndf * prev, ndf * mult, kw, 1, padw, bias=inorm), norm(ndf * mult), nn.LeakyReLU(0.2, True)]
        seq += [nn.Conv2d(ndf * mult, 1, kw, 1, padw)]
        self.model = nn.Sequential(*seq)
        self._cfg = (input_nc, ndf, n_layers)
        self._norm = 1 if inorm else 0
        self.compute_dtype = N.dtype_name(dtype)
        self._pack = _PackState()

    def invalidate_packed_weights(self):
        """See RDDBNet.invalidate_packed_weights."""
        self._pack.invalidate()

    def forward(self, input):
        bns = [m for m in self.model if isinstance(m, nn.BatchNorm2d)]
        running = [t for m in bns for t in (m.running_mean, m.running_var)]
        nbt = [m.num_batches_tracked for m in bns]
        cfg = (*self._cfg, N.dtype_id(self.compute_dtype), self.training, self._pack, self._norm)
        return _NLayerDFn.apply(input, cfg, running, nbt, *self.parameters())
