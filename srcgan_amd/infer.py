"""Whole-scene inference: super-resolve (and colourise) an image too large, or too oddly sized, for one forward.

The scene stays on the device (u8 HWC or f32 NCHW).  ``plan_tiles`` cuts it into cores that partition it, each read with a halo;
``srcgan_tile_gather`` collects up to ``batch`` tiles of one shape into an NCHW f32 batch, the generators run on it under
``no_grad`` (their inference workspaces, sized by the tile batch and not by the scene), and ``srcgan_tile_scatter`` writes the HR
tiles back -- by crop, or by a feathered blend whose ramps the plan defines.  Everything on the hot path is native (csrc/tiles.hip
and the generators' own kernels); there is no CPU fallback.

``cascade_scene`` is the reference's product, the gray LR scene -> super-resolution -> colourisation -> 8-bit RGB cascade of
testCas.py / testCasConst.py / testCasLAB.py / testCasConstLAB.py, on the same plan: the gray conversion of a colour scene and the
Const variants' bilinear up-sampling happen inside the gather (``srcgan_tile_gather_ex``, the one gather both drivers call: the
plain ``srcgan_tile_gather`` is its ``s = 1`` case with the kind taken from the dtype), the LAB variants keep the L tile of the
first network next to the ab tile of the second, and in crop mode the 8-bit conversion happens inside the write-back
(``srcgan_tile_scatter_u8``) -- no f32 scene is made on the way.

``ensemble=`` on both drivers is the geometric self-ensemble: every tile batch runs under 2, 4 or 8 flips / rotations made inside the
gather (``srcgan_tile_gather_d4``), and the outputs are folded back and averaged in f32 (``srcgan_d4_accumulate``) before the
write-back -- the plan, the sinks and the memory rule (nothing scene-sized beyond the result) stay as they are.

Two modes:
  exact    ``halo=None``: the halo is the receptive radius of the chain (``receptive_halo``), tiles are cropped to their cores, and
           the result is the whole-image forward's (networks without normalisation layers only).
  blended  an explicit ``halo`` and ``blend="feather"``: for chains with per-image statistics (ResDeconv's GroupNorm), where no halo
           makes tiles exact; neighbouring tiles are cross-faded over ``2 * min(halo, tile // 2)`` pixels around each core boundary.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _native as N
from . import model as M

__all__ = ["plan_tiles", "receptive_halo", "upscale_scene", "cascade_scene", "TilePlan", "Tile"]


# ------------------------------------------------------------------------------------------------ the plan (pure Python)
@dataclass(frozen=True)
class Tile:
    """One tile, in LR pixels.  ``y0, x0, th, tw``: the gathered rectangle (it may pass the right / bottom edge: the gather replicates
    the edge there).  ``core`` = (cy0, cy1, cx0, cx1): the cores of all tiles partition the scene.  ``support`` = (sy0, sy1, sx0, sx1):
    what a feathered write-back touches, the core widened by half a ramp on every side that has a neighbour.  ``ramps`` = (ny_lo, ny_hi,
    nx_lo, nx_hi): the ramp lengths at the low / high end of the support (0 at the scene border)."""
    y0: int
    x0: int
    th: int
    tw: int
    core: Tuple[int, int, int, int]
    support: Tuple[int, int, int, int]
    ramps: Tuple[int, int, int, int]


@dataclass
class TilePlan:
    """``tiles``: every tile, ordered class by class (classes in order of first appearance, row-major inside a class) -- the order
    ``upscale_scene`` runs and blends them in, so "tile order" below always means the index into this list.  ``classes``: tile shape
    (th, tw) -> indices into ``tiles``."""
    H: int
    W: int
    tile: int
    halo: int
    multiple: int
    tiles: List[Tile] = field(default_factory=list)
    classes: Dict[Tuple[int, int], List[int]] = field(default_factory=dict)

    @property
    def overruns(self) -> bool:
        """Some tile passes the right / bottom edge (possible with ``multiple > 1`` only)."""
        return any(t.y0 + t.th > self.H or t.x0 + t.tw > self.W for t in self.tiles)

    @staticmethod
    def axis_weights(n: int, n_lo: int, n_hi: int) -> torch.Tensor:
        """f32 weights of one axis of a support of ``n`` (HR) pixels: ``(j + 0.5) / n_lo`` over the first ``n_lo``, ``1 - (j + 0.5) /
        n_hi`` over the last ``n_hi``, 1 between -- the arithmetic of the scatter kernel, rounding for rounding."""
        w = torch.ones(n, dtype=torch.float32)
        if n_lo:
            w[:n_lo] = (torch.arange(n_lo, dtype=torch.float32) + 0.5) / float(n_lo)
        if n_hi:
            w[n - n_hi:] = 1.0 - (torch.arange(n_hi, dtype=torch.float32) + 0.5) / float(n_hi)
        return w

    def weights(self, t: Tile, up: int = 1) -> torch.Tensor:
        """[support height * up, support width * up] f32 feather weights of one tile: the outer product of its two axis ramps.  Over
        all tiles they sum to 1 at every pixel (a partition of unity up to f32 rounding)."""
        sy0, sy1, sx0, sx1 = t.support
        wy = self.axis_weights((sy1 - sy0) * up, t.ramps[0] * up, t.ramps[1] * up)
        wx = self.axis_weights((sx1 - sx0) * up, t.ramps[2] * up, t.ramps[3] * up)
        return wy[:, None] * wx[None, :]

    def rects(self, idx: Sequence[int], feather: bool):
        """The 10-int records ``srcgan_tile_scatter`` takes (crop mode: the core, no ramps)."""
        out = []
        for i in idx:
            t = self.tiles[i]
            out += [t.y0, t.x0, *(t.support if feather else t.core), *(t.ramps if feather else (0, 0, 0, 0))]
        return out


def _axis(L: int, tile: int, halo: int, multiple: int):
    """One axis: [(start, extent, core0, core1, support0, support1, ramp_lo, ramp_hi)].  The ramp between two neighbours is centred on
    their core boundary B and spans [B - r, B + r), r = min(halo, tile // 2, length of the following core): inside both tiles (r <=
    halo), inside the scene, and never meeting the next boundary's ramp (every core that has ramps at both ends is a full one, and
    tile >= 2 (tile // 2)) -- so at most two tiles per axis carry weight at any pixel."""
    cores = [(c0, min(c0 + tile, L)) for c0 in range(0, L, tile)]
    r = [min(halo, tile // 2, cores[k + 1][1] - cores[k + 1][0]) for k in range(len(cores) - 1)]
    out = []
    for k, (c0, c1) in enumerate(cores):
        s = max(c0 - halo, 0)
        n = min(c1 + halo, L) - s
        n = -(-n // multiple) * multiple
        r_lo = r[k - 1] if k > 0 else 0
        r_hi = r[k] if k < len(cores) - 1 else 0
        out.append((s, n, c0, c1, c0 - r_lo, c1 + r_hi, 2 * r_lo, 2 * r_hi))
    return out


def plan_tiles(H: int, W: int, tile: int, halo: int, multiple: int = 1) -> TilePlan:
    """Cut an H x W scene into tiles.  Cores of ``tile`` x ``tile`` pixels (ragged at the right / bottom) partition the scene; a tile is
    its core plus ``halo`` on every side, clipped at the scene border -- a clipped side sees the network's own zero padding, exactly
    as the whole image does.  ``multiple > 1`` rounds every tile extent up to that multiple (towards the right / bottom); where that
    passes the edge the gather replicates the edge pixel and the scatter drops the excess."""
    if min(H, W, tile, multiple) < 1 or halo < 0:
        raise ValueError(f"plan_tiles: need H, W, tile, multiple >= 1 and halo >= 0, got {(H, W, tile, halo, multiple)}")
    plan = TilePlan(H, W, tile, halo, multiple)
    by_class: Dict[Tuple[int, int], List[Tile]] = {}
    for (y0, th, cy0, cy1, sy0, sy1, ny_lo, ny_hi) in _axis(H, tile, halo, multiple):
        for (x0, tw, cx0, cx1, sx0, sx1, nx_lo, nx_hi) in _axis(W, tile, halo, multiple):
            by_class.setdefault((th, tw), []).append(
                Tile(y0, x0, th, tw, (cy0, cy1, cx0, cx1), (sy0, sy1, sx0, sx1), (ny_lo, ny_hi, nx_lo, nx_hi)))
    for shape, ts in by_class.items():
        plan.classes[shape] = list(range(len(plan.tiles), len(plan.tiles) + len(ts)))
        plan.tiles += ts
    return plan


# ------------------------------------------------------------------------------------------------ receptive radii
def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _scale(net) -> Optional[int]:
    """Output pixels per input pixel of a known generator (None: unknown module)."""
    if isinstance(net, (M.RDDBNetA, M.SRDenseNetB)):
        return None                                     # HR -> LR networks: not an up-scaling chain
    if isinstance(net, M.SRDenseNetA):
        return M._MODES[net.mode]
    if isinstance(net, M.RDDBNetB):                     # and LegacyRDDBNet
        return M._MODES[net.mode]
    if isinstance(net, M.RDDBNet):
        return int(net.upscale_factor)
    if isinstance(net, (M.ESPCN, M.EDSR)):
        return int(net._cfg[3])
    if isinstance(net, (M.SRCNN, M.SRDN, M.ResDeconv)):
        return 1
    if isinstance(net, (M.RCAN, M.DDBPN, M.RDN)):
        return int(net.scale)
    if isinstance(net, M.MDSR):
        return int(net.scale[net.scale_idx])            # the branch ``set_scale`` chose
    if isinstance(net, M.VDSR):
        return 1                                        # three colours in and out: a ``cascade_scene(const=True)`` SR network on 3-channel input only
    if isinstance(net, M.ResnetGenerator):
        return 1                                        # a translator: the output has the input's size (H, W multiples of 4)
    if isinstance(net, M.UnetGenerator):
        return 1                                        # a translator: the output has the input's size (H, W multiples of 2^num_downs)
    return None


def _ddbpn_halo(scale: int) -> int:
    """DDBPN's receptive radius in input pixels, by propagating index intervals backwards through its graph (ddbpn.py:112-130).

    A projection has (k, s, p) = (6, 2, 2), (8, 4, 2) or (12, 8, 2).  Up (ConvTranspose2d): HR pixel o reads the LR pixels i with
    0 <= o + p - s i <= k - 1, so an HR interval [a, b] needs U[a, b] = [ceil((a + p - k + 1) / s), floor((b + p) / s)].  Down (Conv2d):
    LR pixel q reads HR [s q - p, s q - p + k - 1], so D[a, b] = [s a - p, s b - p + k - 1].  PReLU and the 1x1 bottleneck spread
    nothing.  An up-module computes a_0 = up(x), e = down(a_0) - x, out = a_0 + up(e) (:59-64): ``out`` on I needs x on
    U(I + D(U(I))), where + is the interval hull; a down-module likewise needs D(I + U(D(I))).  The walk starts from one HR pixel o
    widened by the 3x3 reconstruction, visits the eleven modules in reverse order -- every module's need is added to each slice of
    the concatenation it reads -- and ends at the initial 1x1 (0) and 3x3 (1) convolutions.  The radius is the largest distance
    between the needed interval's ends and the LR pixel o // s that owns o, over the s phases of o (the graph is periodic in s)."""
    k, s, p = M._DDBPN_PROJ[scale]
    depth = 6
    hull = lambda a, b: b if a is None else (a if b is None else (min(a[0], b[0]), max(a[1], b[1])))
    U = lambda I: (-((-(I[0] + p - k + 1)) // s), (I[1] + p) // s)
    D = lambda I: (s * I[0] - p, s * I[1] - p + k - 1)
    up_mod = lambda I: U(hull(I, D(U(I))))
    down_mod = lambda I: D(hull(I, U(D(I))))
    radius = 0
    for o in range(s):
        need_h = [(o - 1, o + 1)] * depth                      # reconstruction: 3x3 over all six HR outputs
        need_l = [None] * (depth - 1)
        x0 = None
        for j in range(depth - 1):                              # the last up-module reads l_0 .. l_4
            need_l[j] = hull(need_l[j], up_mod(need_h[depth - 1]))
        for i in range(depth - 2, -1, -1):
            d = down_mod(need_l[i])                             # down-module i reads h_0 .. h_i
            for j in range(i + 1):
                need_h[j] = hull(need_h[j], d)
            u = up_mod(need_h[i])                               # up-module i reads x (i = 0) or l_0 .. l_{i-1}
            if i == 0:
                x0 = hull(x0, u)
            for j in range(i):
                need_l[j] = hull(need_l[j], u)
        lo, hi = x0[0] - 1, x0[1] + 1                           # initial: 1x1 (0), 3x3 (1)
        radius = max(radius, (o // s) - lo, hi - (o // s))
    return radius


def receptive_halo(net) -> int:
    """Receptive radius of a generator in INPUT pixels: the halo at which a cropped tile equals the whole-image forward.

    Every 3x3 p1 convolution spreads 1 pixel at its own resolution (k x k: k // 2); LeakyReLU / ReLU, 1x1 convolutions, the k2 s2
    transposed convolutions, PixelShuffle and nearest up-sampling spread nothing; r pixels at a resolution ``s`` times the input's
    cost ceil(r / s) input pixels.  Citations are into the reference (src/model/...):

      RDDBNet        15 nb + 3      conv_first (rddb.py:89) 1; five 3x3 per dense block (rddb.py:52-58), three blocks per RRDB
                                    (rddb.py:71-82): 15 per RRDB; trunk_conv (rddb.py:91) 1; deconv k2 s2 + LeakyReLU (rddb.py:28-38,
                                    93-97) 0; conv_last at HR (rddb.py:98): 1 HR pixel = 1 input pixel
      RDDBNetB       15 nb + 8 (x2), 15 nb + 5 (x4)
                                    conv_first, trunk, trunk_conv (model.py:400-402, 418-424) 15 nb + 2; x2: nearest x2, upconv1 twice
                                    (model.py:429-430), HRconv eight times and conv_last (model.py:431-439): 11 HR pixels = 6 input
                                    pixels; x4: upconv1 at 2x (model.py:426) 1, then upconv2, 8 HRconv, conv_last at 4x: 10 -> 5 at 2x,
                                    6 at 2x in all = 3 input pixels
      LegacyRDDBNet  3 (x2, x4), 5 (x1)
                                    the trunk is computed and discarded (model.py:381-382): conv_first (model.py:352) 1; x2: upconv,
                                    HRconv twice, conv_last at 2x (model.py:386, 390-391): 4 -> 2; x4: upconv at 2x, then upconv, 2 HRconv,
                                    conv_last at 4x (model.py:383-384): 4 -> 2 at 2x, 3 at 2x in all -> 2; x1 (model.py:388): 4 at 1x
      ESPCN          6              conv1 5x5 (espcn.py:27) 2; conv2, conv3, conv4 3x3 (espcn.py:29-33) 3; PixelShuffle (espcn.py:35) 0;
                                    conv5 3x3 at HR (espcn.py:36): 1 HR pixel = 1 input pixel
      SRCNN          6              conv1 9x9 (srcnn.py:25) 4; conv2 1x1 (srcnn.py:27) 0; conv3 5x5 (srcnn.py:29) 2
      SRDenseNetA    blocks * layers + 4
                                    conv_first (model.py:679) 1; conv (model.py:643-646) 1; one 3x3 per dense layer (model.py:653-672);
                                    bottleneck 1x1 (model.py:693) 0; ConvTranspose2d k3 s2 p1 op1 (model.py:699): output 2i reads input i,
                                    output 2i + 1 reads i and i + 1; reconstruction and conv_last at HR (model.py:704-706) 2 HR pixels:
                                    HR [2c - 2, 2c + 3] reads inputs [c - 1, c + 2] (x4, the sampler applied twice: [c - 1, c + 2] too): 2
      SRDenseNetB    blocks * layers + 7 (x2), + 13 (x4)
                                    as A up to the bottleneck: blocks * layers + 2; Conv2d k3 s2 p1 (model.py:756): output o reads inputs
                                    2o - 1 .. 2o + 1; reconstruction and conv_last (model.py:761-763) 2 output pixels: x2 2 * 2 + 1 = 5
                                    input pixels, x4 2 * (2 * 2 + 1) + 1 = 11.  (An HR -> LR network: ``upscale_scene`` does not run it.)

      DDBPN          by interval propagation through its eleven projection modules: ``_ddbpn_halo`` holds the derivation
      RDN            D C + 5        SFENet1, SFENet2 (rdn.py:59-60) 2; one 3x3 per dense layer (rdn.py:18-20, 35-37): C per block, D blocks;
                                    LFF and GFF.0 1x1 (rdn.py:40, 71) 0; GFF.1 (rdn.py:72) 1; UPNet.0 (rdn.py:78, 84) 1; PixelShuffle 0; x2 / x3:
                                    the last convolution at HR (rdn.py:80): 1 HR pixel = 1 input pixel; x4: UPNet.2 at 2x (rdn.py:86) 1 and
                                    the last convolution at 4x (rdn.py:88) 1 -> 1 at 2x: 2 pixels at 2x = 1 input pixel.  'A': 125, 'B': 133
      MDSR           2 n_resblocks + 12
                                    MeanShift 1x1 (common.py:16) 0; head (mdsr.py:25) 1; pre_process: two ResBlocks of two 5x5 (mdsr.py:27-32,
                                    common.py:43-44) 4 * 2 = 8; body: two 3x3 per ResBlock and one 3x3 (mdsr.py:34-39) 2 n_resblocks + 1; the
                                    skips spread nothing; Upsampler (common.py:63-82): its first 3x3 at LR 1; x2 / x3: the tail at HR
                                    (mdsr.py:45): 1 HR pixel = 1 input pixel; x4: a 3x3 at 2x and the tail at 4x: 1 -> 1 at 2x, 2 at 2x = 1
                                    input pixel; x8: one level more, again 1: the sampler and the tail cost 2 at every scale.  r16: 44
      VDSR           n_resblocks    one 3x3 per BasicBlock (vdsr.py:24-35), all at the input's resolution; the skip spreads nothing.  r20: 20

    Networks with normalisation layers (ResDeconv, EDSR, ResnetGenerator, UnetGenerator: GroupNorm / InstanceNorm statistics are taken over the whole image), RCAN
    (its channel attention pools over the whole image) and unknown modules raise ValueError: no halo makes their tiles exact, so pass ``halo=`` explicitly and blend."""
    name = type(net).__name__
    if isinstance(net, (M.ResDeconv, M.EDSR, M.ResnetGenerator, M.UnetGenerator)):
        raise ValueError(f"receptive_halo: {name} has normalisation layers whose per-image statistics make tiles inexact at any halo; "
                         "pass halo= explicitly (and blend='feather')")
    if isinstance(net, M.RCAN):
        raise ValueError(f"receptive_halo: {name} gates its channels by a global average pool (rcan.py:24-27) whose per-image value makes "
                         "tiles inexact at any halo; pass halo= explicitly (and blend='feather')")
    if isinstance(net, M.DDBPN):
        return _ddbpn_halo(net.scale)
    if isinstance(net, M.RDN):
        return net.D * net.C + 5
    if isinstance(net, M.MDSR):
        return 2 * net.n_resblocks + 12
    if isinstance(net, M.VDSR):
        return net.n_resblocks
    if isinstance(net, M.LegacyRDDBNet):
        return 5 if net.mode == "x1" else 3
    if isinstance(net, M.RDDBNetB):
        return 15 * net.nb + (8 if net.mode == "x2" else 5)
    if isinstance(net, M.SRDenseNetA):                  # and SRDenseNetB
        _, _, _, growth, nblocks, nlayers, up = net._cfg
        trunk = nblocks * nlayers
        if isinstance(net, M.SRDenseNetB):
            return trunk + (7 if up == 2 else 13)
        return trunk + 4
    if isinstance(net, M.RDDBNet) and not isinstance(net, M.RDDBNetA):
        return 15 * net._cfg[4] + 3
    if isinstance(net, (M.ESPCN, M.SRCNN)):
        return 6
    raise ValueError(f"receptive_halo: no receptive radius is known for {name} (an unknown module may hold per-image statistics, which "
                     "make tiles inexact); pass halo= explicitly")


def _chain_halo(nets) -> int:
    """Summed receptive radius of a chain in pixels of its input: a later network's radius shrinks by the scale in front of it."""
    total, scale = 0, 1
    for net in nets:
        r = receptive_halo(net)
        total += _cdiv(r, scale)
        s = _scale(net)
        if s is None:
            raise ValueError(f"upscale_scene: {type(net).__name__} is not an up-scaling generator")
        scale *= s
    return total


# ------------------------------------------------------------------------------------------------ native calls
def _int_array(values):
    return (C.c_int * len(values))(*values)


_KINDS = {"f32": 0, "u8": 1, "u8rgb2gray": 2}


def _gather(who: str, scene: torch.Tensor, lay, kind: str, s: int, origins, th: int, tw: int, op: Optional[int] = None) -> torch.Tensor:
    """The one native gather call; ``lay`` = ``N.scene_layout(scene)``, already checked against ``kind`` by the caller.  ``op`` given:
    ``srcgan_tile_gather_d4``, whose tiles are ``tw`` x ``th`` for a transposing ``op``."""
    _, sc, Cc, H, W = lay
    if not sc.is_contiguous():
        raise ValueError(f"{who}: the scene must be contiguous")
    T = len(origins)
    vh, vw = (tw, th) if op is not None and op & 1 else (th, tw)
    out = torch.empty(T, 1 if kind == "u8rgb2gray" else Cc, vh, vw, dtype=torch.float32, device=scene.device)
    flat = _int_array([int(v) for yx in origins for v in yx])
    args = (sc.data_ptr(), _KINDS[kind], Cc, H, W, int(s), out.data_ptr(), T, th, tw, flat)
    if op is None:
        N.check(N.lib().srcgan_tile_gather_ex(*args, N.stream_ptr(scene.device)), who)
    else:
        N.check(N.lib().srcgan_tile_gather_d4(*args, int(op), N.stream_ptr(scene.device)), who)
    return out


def tile_gather(scene: torch.Tensor, origins, th: int, tw: int) -> torch.Tensor:
    """``srcgan_tile_gather``: scene u8 [H,W,C] / [H,W] or f32 [C,H,W] / [1,C,H,W] on the device, origins [(y0, x0)] -> f32
    [T,C,th,tw]; coordinates are clamped to the scene (edge replication past the right / bottom edge)."""
    N.require_cuda(scene, "tile_gather")
    lay = N.scene_layout(scene)
    if lay is None:
        raise TypeError(f"tile_gather: the scene must be uint8 (HWC) or float32 (NCHW), got {scene.dtype} {tuple(scene.shape)}")
    return _gather("tile_gather", scene, lay, lay[0], 1, origins, th, tw)


def tile_gather_ex(scene: torch.Tensor, kind: str, s: int, origins, th: int, tw: int) -> torch.Tensor:
    """``srcgan_tile_gather_ex``: ``tile_gather`` of the scene converted (``kind``: "f32" planes, "u8" HWC v / 255, "u8rgb2gray" u8
    [H,W,3] -> one gray plane as ``data.arr2gray``) and up-sampled ``s`` times bilinearly (as ``ops.bilinear_up``), evaluated on the
    fly; origins are on the up-sampled grid.  Bit-identical to ``tile_gather`` of the materialised scene."""
    N.require_cuda(scene, "tile_gather_ex")
    return _gather("tile_gather_ex", scene, _kind_layout("tile_gather_ex", scene, kind), kind, s, origins, th, tw)


def _kind_layout(who: str, scene: torch.Tensor, kind: str):
    """``N.scene_layout(scene)``, checked against an explicit ``kind``."""
    if kind not in _KINDS:
        raise ValueError(f"{who}: kind must be one of {sorted(_KINDS)}, got {kind!r}")
    lay = N.scene_layout(scene)
    if lay is None or lay[0] != ("f32" if kind == "f32" else "u8"):
        raise TypeError(f"{who}: kind {kind!r} takes " + ("float32 [C,H,W] / [1,C,H,W]" if kind == "f32" else "uint8 [H,W] / [H,W,C]")
                        + f", got {scene.dtype} {tuple(scene.shape)}")
    return lay


def tile_gather_d4(scene: torch.Tensor, kind: str, s: int, origins, th: int, tw: int, op: int) -> torch.Tensor:
    """``srcgan_tile_gather_d4``: the ``op`` view (``ENSEMBLE_OPS``: bit 0 transposes, bit 1 mirrors rows, bit 2 mirrors columns) of
    every ``th`` x ``tw`` window ``tile_gather_ex`` returns -> f32 [T,C,th,tw], or [T,C,tw,th] for a transposing ``op``.  Bit-identical
    to transforming ``tile_gather_ex``'s output; ``op = 0`` is ``tile_gather_ex``."""
    N.require_cuda(scene, "tile_gather_d4")
    return _gather("tile_gather_d4", scene, _kind_layout("tile_gather_d4", scene, kind), kind, s, origins, th, tw, op)


def d4_accumulate(view: torch.Tensor, acc: torch.Tensor, op: int, first: bool, scale: float) -> None:
    """``srcgan_d4_accumulate``: fold ``view``, f32 [T,C,Hv,Wv] in the orientation of ``op``, back to the identity orientation into
    ``acc``, f32 [T,C,ah,aw] ((Hv, Wv) = (aw, ah) for a transposing ``op``): ``acc = ((0 if first else acc) + folded view) * scale`` in
    f32, one addition and one multiplication.  ``first`` does not read ``acc``."""
    N.require_cuda(view, "d4_accumulate")
    N.require_cuda(acc, "d4_accumulate")
    for t in (view, acc):
        if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
            raise TypeError("d4_accumulate: view and accumulator must be contiguous float32 [T,C,H,W]")
    T, Cc, ah, aw = acc.shape
    if tuple(view.shape) != (T, Cc, *((aw, ah) if int(op) & 1 else (ah, aw))):
        raise ValueError(f"d4_accumulate: a view {tuple(view.shape)} under op = {op} does not fold into {tuple(acc.shape)}")
    N.check(N.lib().srcgan_d4_accumulate(view.data_ptr(), acc.data_ptr(), T * Cc, ah, aw, int(op), int(bool(first)), float(scale),
                                         N.stream_ptr(acc.device)), "srcgan_d4_accumulate")


def tile_scatter(tiles: torch.Tensor, dst: torch.Tensor, up: int, rects, feather: bool) -> None:
    """``srcgan_tile_scatter``: tiles f32 [T,C,th*up,tw*up] into dst f32 [C,H*up,W*up]; ``rects`` as ``TilePlan.rects`` builds them.
    Feather mode adds into ``dst`` (zero it first), tile after tile in the order given."""
    N.require_cuda(tiles, "tile_scatter")
    N.require_cuda(dst, "tile_scatter")
    if tiles.dtype != torch.float32 or dst.dtype != torch.float32 or not tiles.is_contiguous() or not dst.is_contiguous():
        raise TypeError("tile_scatter: tiles and destination must be contiguous float32")
    d = dst if dst.dim() == 3 else dst[0]
    T, Cc, TH, TW = tiles.shape
    if up < 1 or TH % up or TW % up or d.shape[0] != Cc or d.shape[1] % up or d.shape[2] % up:
        raise ValueError(f"tile_scatter: tiles {tuple(tiles.shape)} / scene {tuple(d.shape)} do not fit up = {up}")
    if len(rects) != 10 * T:
        raise ValueError("tile_scatter: 10 integers per tile expected")
    N.check(N.lib().srcgan_tile_scatter(tiles.data_ptr(), d.data_ptr(), Cc, d.shape[1] // up, d.shape[2] // up, up, T, TH // up, TW // up,
                                        _int_array([int(v) for v in rects]), int(bool(feather)), N.stream_ptr(dst.device)),
            "srcgan_tile_scatter")


def planes_to_u8hwc(planes: torch.Tensor) -> torch.Tensor:
    """f32 [C,H,W] / [1,C,H,W] on the device -> u8 [H,W,C]: ``floor(clamp(v, 0, 1) * 255)``.  For values in [0, 1] this is the
    reference's ``tensor2image`` (test.py:38, visCas.py:28: ``* 255`` then ``astype(uint8)``).  Deviation: out-of-range values
    SATURATE (below 0 -> 0, above 1 -> 255) where the reference's uint8 cast wraps around."""
    N.require_cuda(planes, "planes_to_u8hwc")
    p = planes if planes.dim() == 3 else planes[0]
    if p.dtype != torch.float32 or not p.is_contiguous():
        raise TypeError("planes_to_u8hwc: contiguous float32 planes expected")
    Cc, H, W = p.shape
    out = torch.empty(H, W, Cc, dtype=torch.uint8, device=p.device)
    N.check(N.lib().srcgan_planes_to_u8hwc(p.data_ptr(), out.data_ptr(), Cc, H * W, N.stream_ptr(p.device)), "srcgan_planes_to_u8hwc")
    return out


def tile_scatter_u8(tiles_a: torch.Tensor, tiles_b: Optional[torch.Tensor], dst: torch.Tensor, up: int, rects) -> None:
    """``srcgan_tile_scatter_u8``: crop-mode write-back into dst u8 [H*up,W*up,3] with the conversion fused into the store.
    ``tiles_b is None``: ``tiles_a`` f32 [T,3,th*up,tw*up] RGB planes, bytes as ``planes_to_u8hwc``; else ``tiles_a`` [T,1,..] is L and
    ``tiles_b`` [T,2,..] is ab (normalised LAB), bytes as ``data.lab2img``.  ``rects``: ``TilePlan.rects(idx, False)``."""
    N.require_cuda(tiles_a, "tile_scatter_u8")
    N.require_cuda(dst, "tile_scatter_u8")
    for t in (tiles_a, tiles_b):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous()):
            raise TypeError("tile_scatter_u8: tiles must be contiguous float32 [T,C,TH,TW]")
    if dst.dtype != torch.uint8 or dst.dim() != 3 or dst.shape[2] != 3 or not dst.is_contiguous():
        raise TypeError("tile_scatter_u8: the destination must be contiguous uint8 [H,W,3]")
    T, Ca, TH, TW = tiles_a.shape
    Cb = 0 if tiles_b is None else tiles_b.shape[1]
    if tiles_b is not None and (tiles_b.shape[0], tiles_b.shape[2], tiles_b.shape[3]) != (T, TH, TW):
        raise ValueError(f"tile_scatter_u8: L tiles {tuple(tiles_a.shape)} and ab tiles {tuple(tiles_b.shape)} do not match")
    if up < 1 or TH % up or TW % up or dst.shape[0] % up or dst.shape[1] % up:
        raise ValueError(f"tile_scatter_u8: tiles {tuple(tiles_a.shape)} / scene {tuple(dst.shape)} do not fit up = {up}")
    if len(rects) != 10 * T:
        raise ValueError("tile_scatter_u8: 10 integers per tile expected")
    N.check(N.lib().srcgan_tile_scatter_u8(tiles_a.data_ptr(), Ca, None if tiles_b is None else tiles_b.data_ptr(), Cb, dst.data_ptr(),
                                           dst.shape[0] // up, dst.shape[1] // up, up, T, TH // up, TW // up,
                                           _int_array([int(v) for v in rects]), 0 if tiles_b is None else 1, N.stream_ptr(dst.device)),
            "srcgan_tile_scatter_u8")


# ------------------------------------------------------------------------------------------------ the drivers
# The views of the geometric self-ensemble: elements of the dihedral group D4 numbered op = 0..7, bit 0 transposes, bit 1 mirrors the
# view's rows, bit 2 its columns (include/srcgan_amd.h states the index mapping).  ensemble=4 is the flips only: no tile changes shape.
ENSEMBLE_OPS = {1: (0,), 2: (0, 4), 4: (0, 2, 4, 6), 8: tuple(range(8))}


def _check_options(who: str, up: int, batch: int, blend: str, out: str, halo: Optional[int], ensemble: int = 1) -> None:
    if ensemble not in ENSEMBLE_OPS or isinstance(ensemble, bool):
        raise ValueError(f"{who}: ensemble must be 1, 2, 4 or 8, got {ensemble!r}")
    if blend not in ("crop", "feather"):
        raise ValueError(f"{who}: blend must be 'crop' or 'feather', got {blend!r}")
    if out not in ("f32", "u8"):
        raise ValueError(f"{who}: out must be 'f32' or 'u8', got {out!r}")
    if up < 1 or batch < 1:
        raise ValueError(f"{who}: up and batch must be >= 1")
    if halo is None and blend != "crop":
        raise ValueError(f"{who}: halo=None is the exact mode and needs blend='crop'")


def _scene_plan(who: str, nets, H: int, W: int, tile: int, halo: Optional[int], multiple: int) -> TilePlan:
    """The plan of an H x W grid.  ``halo=None`` is the exact mode: the summed receptive radius of ``nets`` (ValueError for chains with
    normalisation layers / unknown modules), refused where a tile would pass the edge."""
    exact = halo is None
    plan = plan_tiles(H, W, tile, _chain_halo(nets) if exact else halo, multiple)
    if exact and plan.overruns:
        raise ValueError(f"{who}: with this `multiple` a tile passes the scene's edge and sees replicated pixels where the whole "
                         "image sees zero padding, so exact mode would not be exact; use multiple=1 or pass halo= explicitly")
    return plan


def _view_gather(scene: torch.Tensor, kind: str, s: int):
    """``gather(origins, th, tw, op)`` of the drivers: the plain gather for ``op=None``, the view ``op`` otherwise."""
    def gather(origins, th, tw, op):
        if op is None:
            return tile_gather_ex(scene, kind, s, origins, th, tw)
        return tile_gather_d4(scene, kind, s, origins, th, tw, op)
    return gather


def _run_views(ops, origins, th: int, tw: int, gather, forward) -> List[torch.Tensor]:
    """One tile batch under the self-ensemble: for each op in turn (ascending, the identity first) gather the batch under that view,
    run the chain on it (a transposing view is a ``tw`` x ``th`` batch) and fold what it returns back into one f32 accumulator per
    tensor -- ``acc = v0; acc = acc + v1; ...``, the last addition scaled by ``1 / V``.  One view's tensors are alive at a time."""
    accs = None
    for k, op in enumerate(ops):
        x = gather(origins, th, tw, op)
        views = [t.contiguous().float() for t in forward(x, *((tw, th) if op & 1 else (th, tw)))]
        if accs is None:
            accs = [torch.empty_like(v) for v in views]         # op 0 comes first: its tensors have the identity's shape
        for v, acc in zip(views, accs):
            d4_accumulate(v, acc, op, k == 0, 1.0 / len(ops) if k == len(ops) - 1 else 1.0)
        del x, views
    return accs


def _run_tiles(nets, plan: TilePlan, batch: int, feather: bool, gather, forward, sink, hr, u8: bool = False, ensemble: int = 1) -> torch.Tensor:
    """The tile loop of both drivers, class by class in batches of ``batch``: ``gather(origins, th, tw, op)`` -> the input batch
    (``op=None``: the plain gather); ``forward(x, th, tw)`` -> the tensors to write back (shape-checked by the caller);
    ``sink(tensors, result, rects)`` writes them.  ``ensemble > 1``: the tensors are the averages over the views (``_run_views``).
    The result is made when the first batch is there: f32 [1, planes of all written tensors, *hr], or u8 [*hr, 3] with ``u8``; zeroed
    for a feathered blend, which adds into it.  Under ``no_grad`` with ``nets`` in ``eval()``."""
    result = None
    ops = ENSEMBLE_OPS[ensemble]
    with torch.no_grad():
        for net in nets:
            net.eval()
        for (th, tw), idx in plan.classes.items():
            for b0 in range(0, len(idx), batch):
                ids = idx[b0:b0 + batch]
                origins = [(plan.tiles[i].y0, plan.tiles[i].x0) for i in ids]
                if ensemble == 1:
                    x = gather(origins, th, tw, None)
                    tensors = [t.contiguous().float() for t in forward(x, th, tw)]
                    del x
                else:
                    tensors = _run_views(ops, origins, th, tw, gather, forward)
                if result is None:
                    shape = (*hr, 3) if u8 else (1, sum(t.shape[1] for t in tensors), *hr)
                    result = (torch.zeros if feather else torch.empty)(shape, dtype=torch.uint8 if u8 else torch.float32, device=tensors[0].device)
                sink(tensors, result, plan.rects(ids, feather))
                del tensors                             # nothing of this batch is held while the next one runs
    return result


def upscale_scene(nets, scene: torch.Tensor, *, up: int, tile: int = 512, halo: Optional[int] = None, batch: int = 1,
                  blend: str = "crop", out: str = "f32", multiple: int = 1, ensemble: int = 1) -> torch.Tensor:
    """Run ``nets`` (a module, or a sequence applied in order, e.g. ``[sr, colouriser]``) over a whole scene, tile by tile.

    ``scene``: a device tensor, u8 [H,W,C] (C = 1 or 3; mapped v / 255 like ``data.arr2rgb``) or f32 [1,C,H,W].  ``up``: output pixels
    per scene pixel of the whole chain.  ``tile``: core size; ``halo``: context read around each core -- ``None`` means EXACT mode: the
    summed receptive radius of the chain (``receptive_halo``), which needs ``blend="crop"`` and a chain without normalisation layers,
    and then equals the whole-image forward.  ``blend``: "crop" (each tile writes its core) or "feather" (neighbours are cross-faded
    over linear ramps, accumulated in f32 in tile order: bitwise reproducible).  ``multiple``: round tile extents up to a multiple (16
    / up of the first stage for a ResDeconv behind it).  ``out``: "f32" -> [1,C',H*up,W*up], "u8" -> u8 [H*up,W*up,C']
    (``planes_to_u8hwc``).  ``ensemble``: 1, 2, 4 or 8 -- the geometric self-ensemble (the "+" variants of EDSR / RCAN): every tile
    batch runs under the views ``ENSEMBLE_OPS[ensemble]`` (2: identity and the mirror image; 4: the four flips, tile shapes unchanged;
    8: all of D4), each output is folded back and the outputs are averaged in f32, in op order, BEFORE the write-back -- so before
    the blend and before any 8-bit conversion.  Views are made per tile inside the gather (``tile_gather_d4``) on the unchanged plan;
    in exact mode the result is the mean over ``g`` of ``g^-1(whole-image forward of g(scene))``.  1 is the path without it.

    Runs under ``no_grad`` with the modules in ``eval()``.  Extra memory: one tile batch's inference workspace and its input / output
    tensors (with ``ensemble > 1`` one f32 accumulator per written tensor more), next to the input and output scenes -- independent
    of the scene size."""
    nets = list(nets) if isinstance(nets, (list, tuple)) else [nets]
    if not nets or not all(isinstance(n, nn.Module) for n in nets):
        raise TypeError("upscale_scene: nets must be a module or a sequence of modules")
    _check_options("upscale_scene", up, batch, blend, out, halo, ensemble)
    lay = N.scene_layout(scene)
    if lay is None or (lay[0] == "f32" and scene.dim() != 4):
        raise ValueError(f"upscale_scene: the scene must be u8 [H,W,C] or f32 [1,C,H,W], got {scene.dtype} {tuple(scene.shape)}")
    kind, _, _, H, W = lay
    plan = _scene_plan("upscale_scene", nets, H, W, tile, halo, multiple)
    N.require_cuda(scene, "upscale_scene")
    feather = blend == "feather"
    scene = scene.contiguous()

    def forward(x, th, tw):
        n = x.shape[0]
        for net in nets:
            x = net(x)
        if x.dim() != 4 or x.shape[0] != n or tuple(x.shape[2:]) != (th * up, tw * up):
            raise ValueError(f"upscale_scene: the chain maps a {th}x{tw} tile to {tuple(x.shape)}, not to {th * up}x{tw * up} (up = {up})")
        return [x]

    result = _run_tiles(nets, plan, batch, feather, _view_gather(scene, kind, 1), forward,
                        lambda ts, res, rects: tile_scatter(ts[0], res, up, rects, feather), (H * up, W * up), ensemble=ensemble)
    return planes_to_u8hwc(result) if out == "u8" else result


# ------------------------------------------------------------------------------------------------ the cascade
def _cascade_plan(netG_A2C, netG_C2B, H: int, W: int, *, up: int, const: bool, tile: int, halo: Optional[int], multiple: int) -> TilePlan:
    """The plan ``cascade_scene`` runs (pure Python).  ``const``: the first network is size-preserving and sees the scene up-sampled
    by ``up`` inside the gather, so the plan -- tiles, halo, ``multiple`` -- is made on the H*up x W*up grid and the chain's own scale
    is 1; the interpolation reads the scene itself and adds nothing to the halo.  Otherwise the plan is on the scene's own grid, as in
    ``upscale_scene``.  ``halo=None``: the summed receptive radius of both networks (refused for normalisation layers)."""
    if const and _scale(netG_A2C) != 1:
        raise ValueError(f"cascade_scene: const=True needs a size-preserving netG_A2C (SRCNN, SRDN), got {type(netG_A2C).__name__}"
                         + ("" if _scale(netG_A2C) is None else f" with scale {_scale(netG_A2C)}"))
    g = up if const else 1
    return _scene_plan("cascade_scene", [netG_A2C, netG_C2B], H * g, W * g, tile, halo, multiple)


def cascade_scene(netG_A2C, netG_C2B, scene: torch.Tensor, *, up: int, space: str = "rgb", const: bool = False, tile: int = 512,
                  halo: Optional[int] = None, batch: int = 1, blend: str = "crop", out: str = "u8", multiple: int = 1,
                  ensemble: int = 1) -> torch.Tensor:
    """The reference's cascade over a whole LR scene: gray -> ``netG_A2C`` (super-resolution) -> ``netG_C2B`` (colourisation) -> picture.

        testCas.py          cascade_scene(sr, col, scene, up=up)
        testCasLAB.py       cascade_scene(sr, col, scene, up=up, space="lab")
        testCasConst.py     cascade_scene(sr, col, scene, up=up, const=True)
        testCasConstLAB.py  cascade_scene(sr, col, scene, up=up, const=True, space="lab")

    (The test scripts make their LR input by down-sampling the HR target; here ``scene`` IS the LR input.)

    ``scene``: a device tensor -- u8 [H,W] / [H,W,1] gray (v / 255), u8 [H,W,3] colour (converted to gray with the arithmetic of
    ``data.arr2gray``) or f32 [1,1,H,W].  ``const``: ``netG_A2C`` is size-preserving and sees the gray scene up-sampled bilinearly by
    ``up`` (trainCasConst.py:89-92); the up-sampling happens inside the tile gather and tiles, halo and ``multiple`` are planned on the
    H*up x W*up grid.  ``space``: "rgb" -- ``netG_C2B`` returns the 3 image planes; "lab" -- it returns the 2 chroma planes and the
    image is normalised LAB, cat(L tile of ``netG_A2C``, ab tile), converted as ``data.lab2img`` for ``out="u8"``.  ``out``: "u8" ->
    u8 [H*up,W*up,3] RGB; "f32" -> f32 [1,3,H*up,W*up], RGB planes or normalised LAB planes.  ``tile, halo, batch, blend, multiple``:
    as in ``upscale_scene`` (``halo=None``: exact mode over both networks' receptive radii, crop only, no normalisation layers).
    ``ensemble``: as in ``upscale_scene``; the whole cascade runs per view, and in LAB mode both the L tile and the ab tile are folded
    and averaged in f32 before the non-linear ``lab2img``.

    Memory: with ``blend="crop", out="u8"`` nothing scene-sized is allocated but the u8 result (the conversion is fused into the
    write-back); ``blend="feather"`` accumulates in ONE f32 [3,H*up,W*up] buffer (L into plane 0, ab into planes 1-2) converted once at
    the end; ``out="f32"`` allocates the f32 result.  Everything else follows the tile batch, the accumulators of ``ensemble > 1`` included."""
    if not isinstance(netG_A2C, nn.Module) or not isinstance(netG_C2B, nn.Module):
        raise TypeError("cascade_scene: netG_A2C and netG_C2B must be modules")
    if space not in ("rgb", "lab"):
        raise ValueError(f"cascade_scene: space must be 'rgb' or 'lab', got {space!r}")
    _check_options("cascade_scene", up, batch, blend, out, halo, ensemble)
    lay = N.scene_layout(scene)
    if lay is None or not (lay[2] in (1, 3) if lay[0] == "u8" else scene.dim() == 4 and lay[2] == 1):
        raise ValueError(f"cascade_scene: the scene must be u8 [H,W], [H,W,1], [H,W,3] or f32 [1,1,H,W], got {scene.dtype} {tuple(scene.shape)}")
    kind, _, Cc, H, W = lay
    if Cc == 3:
        kind = "u8rgb2gray"
    plan = _cascade_plan(netG_A2C, netG_C2B, H, W, up=up, const=const, tile=tile, halo=halo, multiple=multiple)
    N.require_cuda(scene, "cascade_scene")
    s, cu = (up, 1) if const else (1, up)               # up-sampling inside the gather; scale of the chain on the plan's grid
    lab, feather, fused = space == "lab", blend == "feather", blend == "crop" and out == "u8"
    want = 2 if lab else 3
    scene = scene.contiguous()

    def forward(x, th, tw):
        l = netG_A2C(x)
        if l.dim() != 4 or l.shape[0] != x.shape[0] or tuple(l.shape[2:]) != (th * cu, tw * cu):
            raise ValueError(f"cascade_scene: netG_A2C maps a {th}x{tw} tile to {tuple(l.shape)}, not to {th * cu}x{tw * cu} "
                             f"(up = {up}, const = {const})")
        if lab and l.shape[1] != 1:
            raise ValueError(f"cascade_scene: space='lab' needs a 1-plane netG_A2C (L), got {l.shape[1]} planes")
        c = netG_C2B(l)
        if c.dim() != 4 or c.shape[0] != x.shape[0] or tuple(c.shape[2:]) != tuple(l.shape[2:]):
            raise ValueError(f"cascade_scene: netG_C2B maps {tuple(l.shape)} to {tuple(c.shape)}; a size-preserving colouriser is expected")
        if c.shape[1] != want:
            raise ValueError(f"cascade_scene: space={space!r} needs a colouriser with {want} output planes, got {c.shape[1]}")
        return [l, c] if lab else [c]

    if fused:
        def sink(ts, res, rects):
            tile_scatter_u8(ts[0], ts[1] if lab else None, res, cu, rects)
    elif lab:                                           # L -> plane 0, ab -> planes 1-2 of the same buffer, through offset pointers
        def sink(ts, res, rects):
            tile_scatter(ts[0], res[0, 0:1], cu, rects, feather)
            tile_scatter(ts[1], res[0, 1:3], cu, rects, feather)
    else:
        def sink(ts, res, rects):
            tile_scatter(ts[0], res, cu, rects, feather)

    result = _run_tiles([netG_A2C, netG_C2B], plan, batch, feather, _view_gather(scene, kind, s), forward, sink, (H * up, W * up), u8=fused,
                        ensemble=ensemble)
    if fused or out == "f32":
        return result
    if lab:
        from .data import lab2img
        return lab2img(result[0])
    return planes_to_u8hwc(result)
