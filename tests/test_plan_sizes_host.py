"""CPU: what the planners of nets.hip and oplist.hip answer -- parameter counts, output sizes, workspace / scratch / packed-weight bytes -- pinned
as literal numbers.  Pure host code: no compute call is made.

The literals are the answers of the library built from the commit BEFORE the discriminator got its per-layer plan and the three
networks their shared stride-2 input-gradient helper (commit 6f71cb0): that commit was exported to a scratch directory, built with
`python -m srcgan_amd.build`, and `collect()` below was run against its library (SRCGAN_AMD_LIB) and printed.  Every value must
stay EQUAL, with one exception that only shrinks: the packed input-gradient weights of RDDBNetA's down stages (3x3 s2 p1,
nf -> nf) are now sized for the taps their four parity packs hold (1 + 2 + 2 + 4 = 9) instead of 4 x 4 = 16, which saves seven
one-tap nf x nf packs per stage in srcgan_rddbnet_wpack_bytes and in the two workspace sizes that contain it (RDDB_DOWN_PARENT)."""
import ctypes as C
import itertools

import pytest


@pytest.fixture(scope="module")
def lib():
    from srcgan_amd import build
    build.build(verbose=False)
    from srcgan_amd import _native as N
    return N.lib()


def _err(l):
    return l.srcgan_last_error().decode()


# ---- NLayerDiscriminator: key = (in_ch, ndf, n_layers, B, H, W, dtype, norm)
D_GRID = [(i, ndf, nl, B, H, W, dt, norm)
          for i, ndf, nl, B, (H, W), dt, norm in itertools.product((1, 3), (16, 64), (1, 3, 5), (1, 4), ((64, 64), (70, 54), (63, 65)),
                                                                   (0, 1), (0, 1))]


def d_answer(l, key):
    """(num_params, out_h, out_w, ws_bytes, bwd_scratch_bytes, wpack_bytes), or the planner's error text."""
    from srcgan_amd import _native as N
    in_ch, ndf, nl, B, H, W, dt, norm = key
    c = N.NLayerDCfg(in_ch, ndf, nl, B, H, W, dt, 1, norm)
    n = l.srcgan_nlayerd_num_params(C.byref(c))
    if n < 0:
        want = _err(l)
        oh, ow = C.c_int(-1), C.c_int(-1)
        assert l.srcgan_nlayerd_out_hw(C.byref(c), C.byref(oh), C.byref(ow)) != 0 and _err(l) == want
        for f in (l.srcgan_nlayerd_ws_bytes, l.srcgan_nlayerd_bwd_scratch_bytes, l.srcgan_nlayerd_wpack_bytes):
            assert f(C.byref(c)) == 0 and _err(l) == want
        return want
    oh, ow = C.c_int(-1), C.c_int(-1)
    assert l.srcgan_nlayerd_out_hw(C.byref(c), C.byref(oh), C.byref(ow)) == 0
    return (n, oh.value, ow.value, l.srcgan_nlayerd_ws_bytes(C.byref(c)), l.srcgan_nlayerd_bwd_scratch_bytes(C.byref(c)),
            l.srcgan_nlayerd_wpack_bytes(C.byref(c)))


# ---- ResDeconv: key = (layers, norm, dtype); B = 2, 64x48, 3 -> 2 channels
RD_GRID = [(layers, norm, dt) for layers in ((2, 2, 2, 2), (3, 4, 6, 3)) for norm in (0, 1) for dt in (0, 1)]


def rd_answer(l, key):
    from srcgan_amd import _native as N
    layers, norm, dt = key
    c = N.ResDeconvCfg(3, 2, 2, 64, 48, dt, (C.c_int * 4)(*layers), norm)
    return (l.srcgan_resdeconv_num_params(C.byref(c)), l.srcgan_resdeconv_ws_bytes(C.byref(c)), l.srcgan_resdeconv_bwd_scratch_bytes(C.byref(c)))


# ---- ESPCN / SRCNN / EDSR: key = (kind, up, dtype); 3 -> 3 channels, base 64, B = 2, 32x24, EDSR with 4 residual blocks
SR_GRID = [(kind, up, dt) for kind, up in ((0, 2), (0, 4), (1, 1), (2, 2), (2, 4)) for dt in (0, 1)]


def sr_answer(l, key):
    from srcgan_amd import _native as N
    kind, up, dt = key
    c = N.SrNetCfg(kind, 3, 3, up, 64, 2, 32, 24, dt, 4)
    return (l.srcgan_srnet_num_params(C.byref(c)), l.srcgan_srnet_ws_bytes(C.byref(c)), l.srcgan_srnet_bwd_scratch_bytes(C.byref(c)))


# ---- RDDBNet / RDDBNetA: key = (down, dtype); nf 64, gc 32, nb 3, B = 2, 48x40, x2 up-sampler when there is no down factor
RDDB_GRID = [(down, dt) for down in (0, 2, 4) for dt in (0, 1)]


def rddb_answer(l, key):
    """(num_params, ws_bytes, infer_ws_bytes, bwd_scratch_bytes, wpack_bytes)"""
    from srcgan_amd import _native as N
    down, dt = key
    c = N.RddbCfg(3, 3, 1 if down else 2, 64, 3, 32, 2, 48, 40, dt, down, 0)
    return (l.srcgan_rddbnet_num_params(C.byref(c)), l.srcgan_rddbnet_ws_bytes(C.byref(c)), l.srcgan_rddbnet_infer_ws_bytes(C.byref(c)),
            l.srcgan_rddbnet_bwd_scratch_bytes(C.byref(c)), l.srcgan_rddbnet_wpack_bytes(C.byref(c)))


# ---- the op-list families (csrc/oplist.hip).  The literals are the answers of the library built from the commit BEFORE the executor
# moved into oplist.hip and its two pack-layout routines became one (commit 4ff4258), taken the same way.  Every value must stay EQUAL.
def _plan(f, cfg, *extra):
    """The full {in, res, out} x {offset, bytes} range list of an inference plan, as a flat tuple."""
    n = f(C.byref(cfg), *extra, None, 0)
    assert n > 0
    buf = (C.c_size_t * (6 * n))()
    assert f(C.byref(cfg), *extra, buf, n) == n
    return tuple(buf)


# ResDeconv: key = (layers, norm, dtype, fold_tail); B = 1, 32x32, 3 -> 2 channels
RDI_GRID = [(layers, norm, dt, fold) for layers in ((1, 1, 1, 1), (2, 1, 1, 1)) for norm in (0, 1) for dt in (0, 1) for fold in (0, 1)]


def rdi_answer(l, key):
    """(num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes, infer_act_bytes, infer_plan)"""
    from srcgan_amd import _native as N
    layers, norm, dt, fold = key
    c = N.ResDeconvCfg(3, 2, 1, 32, 32, dt, (C.c_int * 4)(*layers), norm)
    return (l.srcgan_resdeconv_num_params(C.byref(c)), l.srcgan_resdeconv_ws_bytes(C.byref(c)), l.srcgan_resdeconv_bwd_scratch_bytes(C.byref(c)),
            l.srcgan_resdeconv_infer_ws_bytes(C.byref(c), fold), l.srcgan_resdeconv_infer_act_bytes(C.byref(c), fold),
            _plan(l.srcgan_resdeconv_infer_plan, c, fold))


# ESPCN / SRCNN / EDSR: key = (kind, up, nres, dtype); 3 -> 3 channels, base 32, B = 2, 16x12.  EDSR with one block takes the spare slot.
SRI_GRID = [(kind, up, nres, dt) for kind, up, nres in ((0, 2, 0), (0, 3, 0), (1, 1, 0), (2, 1, 2), (2, 2, 1), (2, 4, 2)) for dt in (0, 1)]


def sri_answer(l, key):
    """(num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes, infer_act_bytes, infer_plan)"""
    from srcgan_amd import _native as N
    kind, up, nres, dt = key
    c = N.SrNetCfg(kind, 3, 3, up, 32, 2, 16, 12, dt, nres)
    return (l.srcgan_srnet_num_params(C.byref(c)), l.srcgan_srnet_ws_bytes(C.byref(c)), l.srcgan_srnet_bwd_scratch_bytes(C.byref(c)),
            l.srcgan_srnet_infer_ws_bytes(C.byref(c)), l.srcgan_srnet_infer_act_bytes(C.byref(c)), _plan(l.srcgan_srnet_infer_plan, c))


# SRDenseNetA / B: key = (kind, up, dtype); 1 -> 3 channels, growth 16, 2 blocks of 2 layers, B = 1, 12x8.  up = 4 applies the shared module twice.
SD_GRID = [(kind, up, dt) for kind in (0, 1) for up in (2, 4) for dt in (0, 1)]


def sd_answer(l, key):
    """(num_params, out_h, out_w, ws_bytes, bwd_scratch_bytes, infer_ws_bytes)"""
    from srcgan_amd import _native as N
    kind, up, dt = key
    c = N.SrDenseCfg(kind, 1, 3, 1, 12, 8, dt, 16, 2, 2, up)
    oh, ow = C.c_int(-1), C.c_int(-1)
    assert l.srcgan_srdense_out_hw(C.byref(c), C.byref(oh), C.byref(ow)) == 0
    return (l.srcgan_srdense_num_params(C.byref(c)), oh.value, ow.value, l.srcgan_srdense_ws_bytes(C.byref(c)),
            l.srcgan_srdense_bwd_scratch_bytes(C.byref(c)), l.srcgan_srdense_infer_ws_bytes(C.byref(c)))


# RCAN: key = (scale, dtype); 2 groups of 1 block, 16 features, reduction 4, B = 1, 10x8
RCAN_GRID = [(scale, dt) for scale in (2, 3, 4, 8) for dt in (0, 1)]


def rcan_answer(l, key):
    """(num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes, infer_act_bytes, infer_plan)"""
    from srcgan_amd import _native as N
    scale, dt = key
    c = N.RcanCfg(3, 3, 1, 10, 8, dt, 2, 1, 16, 4, scale)
    return (l.srcgan_rcan_num_params(C.byref(c)), l.srcgan_rcan_ws_bytes(C.byref(c)), l.srcgan_rcan_bwd_scratch_bytes(C.byref(c)),
            l.srcgan_rcan_infer_ws_bytes(C.byref(c)), l.srcgan_rcan_infer_act_bytes(C.byref(c)), _plan(l.srcgan_rcan_infer_plan, c))


# DDBPN: key = (scale, dtype); B = 1, 6x5.  Scale 2 is grid shift 0, scales 4 and 8 shift 2.
DDBPN_GRID = [(scale, dt) for scale in (2, 4, 8) for dt in (0, 1)]


def ddbpn_answer(l, key):
    """(num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes, infer_act_bytes, infer_plan)"""
    from srcgan_amd import _native as N
    scale, dt = key
    c = N.DdbpnCfg(3, 3, 1, 6, 5, dt, scale)
    return (l.srcgan_ddbpn_num_params(C.byref(c)), l.srcgan_ddbpn_ws_bytes(C.byref(c)), l.srcgan_ddbpn_bwd_scratch_bytes(C.byref(c)),
            l.srcgan_ddbpn_infer_ws_bytes(C.byref(c)), l.srcgan_ddbpn_infer_act_bytes(C.byref(c)), _plan(l.srcgan_ddbpn_infer_plan, c))


# VGG16Loss / PerceptionLoss: key = (kind, B, H, W, dtype)
VGG_GRID = [(kind, B, H, W, dt) for kind in (0, 1) for B, H, W in ((2, 32, 32), (1, 40, 24)) for dt in (0, 1)]


def vgg_answer(l, key):
    """(num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes)"""
    from srcgan_amd import _native as N
    kind, B, H, W, dt = key
    c = N.VggLossCfg(kind, B, H, W, dt)
    return (l.srcgan_vggloss_num_params(C.byref(c)), l.srcgan_vggloss_ws_bytes(C.byref(c)), l.srcgan_vggloss_bwd_scratch_bytes(C.byref(c)),
            l.srcgan_vggloss_infer_ws_bytes(C.byref(c)))


OPLIST = {"RDI": (RDI_GRID, rdi_answer), "SRI": (SRI_GRID, sri_answer), "SD": (SD_GRID, sd_answer), "RCAN": (RCAN_GRID, rcan_answer),
          "DDBPN": (DDBPN_GRID, ddbpn_answer), "VGG": (VGG_GRID, vgg_answer)}


def collect(l):
    """Every answer, as the literal tables below hold them."""
    out = {"D": {k: d_answer(l, k) for k in D_GRID}, "RD": {k: rd_answer(l, k) for k in RD_GRID},
           "SR": {k: sr_answer(l, k) for k in SR_GRID}, "RDDB": {k: rddb_answer(l, k) for k in RDDB_GRID}}
    out.update({name: {k: answer(l, k) for k in grid} for name, (grid, answer) in OPLIST.items()})
    return out


# (num_params, out_h, out_w, ws_bytes, bwd_scratch_bytes, wpack_bytes), or the error text of a rejected configuration
D_EXPECTED = {
    (1, 16, 1, 1, 64, 64, 0, 0): (7, 30, 30, 703232, 702976, 221440),
    (1, 16, 1, 1, 64, 64, 0, 1): (6, 30, 30, 719616, 719616, 221440),
    (1, 16, 1, 1, 64, 64, 1, 0): (7, 30, 30, 389888, 496128, 147712),
    (1, 16, 1, 1, 64, 64, 1, 1): (6, 30, 30, 406272, 512768, 147712),
    (1, 16, 1, 1, 70, 54, 0, 0): (7, 33, 25, 665600, 739840, 221440),
    (1, 16, 1, 1, 70, 54, 0, 1): (6, 33, 25, 681984, 756480, 221440),
    (1, 16, 1, 1, 70, 54, 1, 0): (7, 33, 25, 370688, 548864, 147712),
    (1, 16, 1, 1, 70, 54, 1, 1): (6, 33, 25, 387072, 565504, 147712),
    (1, 16, 1, 1, 63, 65, 0, 0): (7, 29, 30, 724480, 963840, 262400),
    (1, 16, 1, 1, 63, 65, 0, 1): (6, 29, 30, 740864, 980480, 262400),
    (1, 16, 1, 1, 63, 65, 1, 0): (7, 29, 30, 429056, 765696, 196864),
    (1, 16, 1, 1, 63, 65, 1, 1): (6, 29, 30, 445440, 782336, 196864),
    (1, 16, 1, 4, 64, 64, 0, 0): (7, 30, 30, 2145024, 2783744, 221440),
    (1, 16, 1, 4, 64, 64, 0, 1): (6, 30, 30, 2212096, 2850304, 221440),
    (1, 16, 1, 4, 64, 64, 1, 0): (7, 30, 30, 1111808, 1955328, 147712),
    (1, 16, 1, 4, 64, 64, 1, 1): (6, 30, 30, 1178880, 2021888, 147712),
    (1, 16, 1, 4, 70, 54, 0, 0): (7, 33, 25, 1994752, 2932224, 221440),
    (1, 16, 1, 4, 70, 54, 0, 1): (6, 33, 25, 2061824, 2998784, 221440),
    (1, 16, 1, 4, 70, 54, 1, 0): (7, 33, 25, 1036800, 2168832, 147712),
    (1, 16, 1, 4, 70, 54, 1, 1): (6, 33, 25, 1103872, 2235392, 147712),
    (1, 16, 1, 4, 63, 65, 0, 0): (7, 29, 30, 2108928, 3828992, 262400),
    (1, 16, 1, 4, 63, 65, 0, 1): (6, 29, 30, 2176000, 3895552, 262400),
    (1, 16, 1, 4, 63, 65, 1, 0): (7, 29, 30, 1122560, 3035136, 196864),
    (1, 16, 1, 4, 63, 65, 1, 1): (6, 29, 30, 1189632, 3101696, 196864),
    (1, 16, 3, 1, 64, 64, 0, 0): (13, 6, 6, 2188800, 842496, 1827072),
    (1, 16, 3, 1, 64, 64, 0, 1): (10, 6, 6, 2229760, 884480, 1827072),
    (1, 16, 3, 1, 64, 64, 1, 0): (13, 6, 6, 1184256, 706816, 999680),
    (1, 16, 3, 1, 64, 64, 1, 1): (10, 6, 6, 1225216, 748800, 999680),
    (1, 16, 3, 1, 70, 54, 0, 0): (13, 6, 4, 2141696, 821760, 1827072),
    (1, 16, 3, 1, 70, 54, 0, 1): (10, 6, 4, 2182656, 863744, 1827072),
    (1, 16, 3, 1, 70, 54, 1, 0): (13, 6, 4, 1160960, 696576, 999680),
    (1, 16, 3, 1, 70, 54, 1, 1): (10, 6, 4, 1201920, 738560, 999680),
    (1, 16, 3, 1, 63, 65, 0, 0): (13, 5, 6, 2203648, 829696, 1868032),
    (1, 16, 3, 1, 63, 65, 0, 1): (10, 5, 6, 2244608, 871680, 1868032),
    (1, 16, 3, 1, 63, 65, 1, 0): (13, 5, 6, 1220096, 700160, 1048832),
    (1, 16, 3, 1, 63, 65, 1, 1): (10, 5, 6, 1261056, 742144, 1048832),
    (1, 16, 3, 4, 64, 64, 0, 0): (13, 6, 6, 3264512, 3340544, 1827072),
    (1, 16, 3, 4, 64, 64, 0, 1): (10, 6, 6, 3436800, 3508480, 1827072),
    (1, 16, 3, 4, 64, 64, 1, 0): (13, 6, 6, 1728000, 2797312, 999680),
    (1, 16, 3, 4, 64, 64, 1, 1): (10, 6, 6, 1900288, 2965248, 999680),
    (1, 16, 3, 4, 70, 54, 0, 0): (13, 6, 4, 3074304, 3256064, 1827072),
    (1, 16, 3, 4, 70, 54, 0, 1): (10, 6, 4, 3246592, 3424000, 1827072),
    (1, 16, 3, 4, 70, 54, 1, 0): (13, 6, 4, 1632512, 2754816, 999680),
    (1, 16, 3, 4, 70, 54, 1, 1): (10, 6, 4, 1804800, 2922752, 999680),
    (1, 16, 3, 4, 63, 65, 0, 0): (13, 5, 6, 3201792, 3290112, 1868032),
    (1, 16, 3, 4, 63, 65, 0, 1): (10, 5, 6, 3374080, 3458048, 1868032),
    (1, 16, 3, 4, 63, 65, 1, 0): (13, 5, 6, 1725440, 2772224, 1048832),
    (1, 16, 3, 4, 63, 65, 1, 1): (10, 5, 6, 1897728, 2940160, 1048832),
    (1, 16, 5, 1, 64, 64, 0, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 16, 5, 1, 64, 64, 0, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 16, 5, 1, 64, 64, 1, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 16, 5, 1, 64, 64, 1, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 16, 5, 1, 70, 54, 0, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 16, 5, 1, 70, 54, 0, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 16, 5, 1, 70, 54, 1, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 16, 5, 1, 70, 54, 1, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 16, 5, 1, 63, 65, 0, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 16, 5, 1, 63, 65, 0, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 16, 5, 1, 63, 65, 1, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 16, 5, 1, 63, 65, 1, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 16, 5, 4, 64, 64, 0, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 16, 5, 4, 64, 64, 0, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 16, 5, 4, 64, 64, 1, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 16, 5, 4, 64, 64, 1, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 16, 5, 4, 70, 54, 0, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 16, 5, 4, 70, 54, 0, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 16, 5, 4, 70, 54, 1, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 16, 5, 4, 70, 54, 1, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 16, 5, 4, 63, 65, 0, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 16, 5, 4, 63, 65, 0, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 16, 5, 4, 63, 65, 1, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 16, 5, 4, 63, 65, 1, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 64, 1, 1, 64, 64, 0, 0): (7, 30, 30, 2927872, 3418880, 1507584),
    (1, 64, 1, 1, 64, 64, 0, 1): (6, 30, 30, 2969344, 3460864, 1507584),
    (1, 64, 1, 1, 64, 64, 1, 0): (7, 30, 30, 1532672, 2842880, 819456),
    (1, 64, 1, 1, 64, 64, 1, 1): (6, 30, 30, 1574144, 2884864, 819456),
    (1, 64, 1, 1, 70, 54, 0, 0): (7, 33, 25, 2816000, 3884288, 1507584),
    (1, 64, 1, 1, 70, 54, 0, 1): (6, 33, 25, 2857472, 3926272, 1507584),
    (1, 64, 1, 1, 70, 54, 1, 0): (7, 33, 25, 1476608, 3353856, 819456),
    (1, 64, 1, 1, 70, 54, 1, 1): (6, 33, 25, 1518080, 3395840, 819456),
    (1, 64, 1, 1, 63, 65, 0, 0): (7, 29, 30, 3009536, 3377664, 1638656),
    (1, 64, 1, 1, 63, 65, 0, 1): (6, 29, 30, 3051008, 3419648, 1638656),
    (1, 64, 1, 1, 63, 65, 1, 0): (7, 29, 30, 1606144, 2822144, 917760),
    (1, 64, 1, 1, 63, 65, 1, 1): (6, 29, 30, 1647616, 2864128, 917760),
    (1, 64, 1, 4, 64, 64, 0, 0): (7, 30, 30, 7183104, 13572352, 1507584),
    (1, 64, 1, 4, 64, 64, 0, 1): (6, 30, 30, 7353600, 13740288, 1507584),
    (1, 64, 1, 4, 64, 64, 1, 0): (7, 30, 30, 3666176, 11267840, 819456),
    (1, 64, 1, 4, 64, 64, 1, 1): (6, 30, 30, 3836672, 11435776, 819456),
    (1, 64, 1, 4, 70, 54, 0, 0): (7, 33, 25, 6734848, 15433216, 1507584),
    (1, 64, 1, 4, 70, 54, 0, 1): (6, 33, 25, 6905344, 15601152, 1507584),
    (1, 64, 1, 4, 70, 54, 1, 0): (7, 33, 25, 3441664, 13312000, 819456),
    (1, 64, 1, 4, 70, 54, 1, 1): (6, 33, 25, 3612160, 13479936, 819456),
    (1, 64, 1, 4, 63, 65, 0, 0): (7, 29, 30, 7117312, 13408256, 1638656),
    (1, 64, 1, 4, 63, 65, 0, 1): (6, 29, 30, 7287808, 13576192, 1638656),
    (1, 64, 1, 4, 63, 65, 1, 0): (7, 29, 30, 3666176, 11185920, 917760),
    (1, 64, 1, 4, 63, 65, 1, 1): (6, 29, 30, 3836672, 11353856, 917760),
    (1, 64, 3, 1, 64, 64, 0, 0): (13, 6, 6, 24682752, 9631488, 23658752),
    (1, 64, 3, 1, 64, 64, 0, 1): (10, 6, 6, 24822528, 9774848, 23658752),
    (1, 64, 3, 1, 64, 64, 1, 0): (13, 6, 6, 12617472, 9299200, 12091648),
    (1, 64, 3, 1, 64, 64, 1, 1): (10, 6, 6, 12757248, 9442560, 12091648),
    (1, 64, 3, 1, 70, 54, 0, 0): (13, 6, 4, 24525568, 9580032, 23658752),
    (1, 64, 3, 1, 70, 54, 0, 1): (10, 6, 4, 24665344, 9723392, 23658752),
    (1, 64, 3, 1, 70, 54, 1, 0): (13, 6, 4, 12538880, 9273600, 12091648),
    (1, 64, 3, 1, 70, 54, 1, 1): (10, 6, 4, 12678656, 9416960, 12091648),
    (1, 64, 3, 1, 63, 65, 0, 0): (13, 5, 6, 24735488, 9606400, 23789824),
    (1, 64, 3, 1, 63, 65, 0, 1): (10, 5, 6, 24875264, 9749760, 23789824),
    (1, 64, 3, 1, 63, 65, 1, 0): (13, 5, 6, 12676352, 9286400, 12189952),
    (1, 64, 3, 1, 63, 65, 1, 1): (10, 5, 6, 12816128, 9429760, 12189952),
    (1, 64, 3, 4, 64, 64, 0, 0): (13, 6, 6, 27721472, 38413568, 23658752),
    (1, 64, 3, 4, 64, 64, 0, 1): (10, 6, 6, 28312832, 38987008, 23658752),
    (1, 64, 3, 4, 64, 64, 1, 0): (13, 6, 6, 14161152, 37083904, 12091648),
    (1, 64, 3, 4, 64, 64, 1, 1): (10, 6, 6, 14752512, 37657344, 12091648),
    (1, 64, 3, 4, 70, 54, 0, 0): (13, 6, 4, 27089664, 38204672, 23658752),
    (1, 64, 3, 4, 70, 54, 0, 1): (10, 6, 4, 27681024, 38778112, 23658752),
    (1, 64, 3, 4, 70, 54, 1, 0): (13, 6, 4, 13843200, 36977408, 12091648),
    (1, 64, 3, 4, 70, 54, 1, 1): (10, 6, 4, 14434560, 37550848, 12091648),
    (1, 64, 3, 4, 63, 65, 0, 0): (13, 5, 6, 27539968, 38313984, 23789824),
    (1, 64, 3, 4, 63, 65, 0, 1): (10, 5, 6, 28131328, 38887424, 23789824),
    (1, 64, 3, 4, 63, 65, 1, 0): (13, 5, 6, 14103296, 37034240, 12189952),
    (1, 64, 3, 4, 63, 65, 1, 1): (10, 5, 6, 14694656, 37607680, 12189952),
    (1, 64, 5, 1, 64, 64, 0, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 64, 5, 1, 64, 64, 0, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 64, 5, 1, 64, 64, 1, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 64, 5, 1, 64, 64, 1, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 64, 5, 1, 70, 54, 0, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 64, 5, 1, 70, 54, 0, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 64, 5, 1, 70, 54, 1, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 64, 5, 1, 70, 54, 1, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 64, 5, 1, 63, 65, 0, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 64, 5, 1, 63, 65, 0, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 64, 5, 1, 63, 65, 1, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 64, 5, 1, 63, 65, 1, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 64, 5, 4, 64, 64, 0, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 64, 5, 4, 64, 64, 0, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 64, 5, 4, 64, 64, 1, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 64, 5, 4, 64, 64, 1, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (1, 64, 5, 4, 70, 54, 0, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 64, 5, 4, 70, 54, 0, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 64, 5, 4, 70, 54, 1, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 64, 5, 4, 70, 54, 1, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (1, 64, 5, 4, 63, 65, 0, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 64, 5, 4, 63, 65, 0, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 64, 5, 4, 63, 65, 1, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (1, 64, 5, 4, 63, 65, 1, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 16, 1, 1, 64, 64, 0, 0): (7, 30, 30, 703232, 702976, 221440),
    (3, 16, 1, 1, 64, 64, 0, 1): (6, 30, 30, 719616, 719616, 221440),
    (3, 16, 1, 1, 64, 64, 1, 0): (7, 30, 30, 389888, 496128, 147712),
    (3, 16, 1, 1, 64, 64, 1, 1): (6, 30, 30, 406272, 512768, 147712),
    (3, 16, 1, 1, 70, 54, 0, 0): (7, 33, 25, 665600, 739840, 221440),
    (3, 16, 1, 1, 70, 54, 0, 1): (6, 33, 25, 681984, 756480, 221440),
    (3, 16, 1, 1, 70, 54, 1, 0): (7, 33, 25, 370688, 548864, 147712),
    (3, 16, 1, 1, 70, 54, 1, 1): (6, 33, 25, 387072, 565504, 147712),
    (3, 16, 1, 1, 63, 65, 0, 0): (7, 29, 30, 724480, 963840, 262400),
    (3, 16, 1, 1, 63, 65, 0, 1): (6, 29, 30, 740864, 980480, 262400),
    (3, 16, 1, 1, 63, 65, 1, 0): (7, 29, 30, 429056, 765696, 196864),
    (3, 16, 1, 1, 63, 65, 1, 1): (6, 29, 30, 445440, 782336, 196864),
    (3, 16, 1, 4, 64, 64, 0, 0): (7, 30, 30, 2145024, 2783744, 221440),
    (3, 16, 1, 4, 64, 64, 0, 1): (6, 30, 30, 2212096, 2850304, 221440),
    (3, 16, 1, 4, 64, 64, 1, 0): (7, 30, 30, 1111808, 1955328, 147712),
    (3, 16, 1, 4, 64, 64, 1, 1): (6, 30, 30, 1178880, 2021888, 147712),
    (3, 16, 1, 4, 70, 54, 0, 0): (7, 33, 25, 1994752, 2932224, 221440),
    (3, 16, 1, 4, 70, 54, 0, 1): (6, 33, 25, 2061824, 2998784, 221440),
    (3, 16, 1, 4, 70, 54, 1, 0): (7, 33, 25, 1036800, 2168832, 147712),
    (3, 16, 1, 4, 70, 54, 1, 1): (6, 33, 25, 1103872, 2235392, 147712),
    (3, 16, 1, 4, 63, 65, 0, 0): (7, 29, 30, 2108928, 3828992, 262400),
    (3, 16, 1, 4, 63, 65, 0, 1): (6, 29, 30, 2176000, 3895552, 262400),
    (3, 16, 1, 4, 63, 65, 1, 0): (7, 29, 30, 1122560, 3035136, 196864),
    (3, 16, 1, 4, 63, 65, 1, 1): (6, 29, 30, 1189632, 3101696, 196864),
    (3, 16, 3, 1, 64, 64, 0, 0): (13, 6, 6, 2188800, 842496, 1827072),
    (3, 16, 3, 1, 64, 64, 0, 1): (10, 6, 6, 2229760, 884480, 1827072),
    (3, 16, 3, 1, 64, 64, 1, 0): (13, 6, 6, 1184256, 706816, 999680),
    (3, 16, 3, 1, 64, 64, 1, 1): (10, 6, 6, 1225216, 748800, 999680),
    (3, 16, 3, 1, 70, 54, 0, 0): (13, 6, 4, 2141696, 821760, 1827072),
    (3, 16, 3, 1, 70, 54, 0, 1): (10, 6, 4, 2182656, 863744, 1827072),
    (3, 16, 3, 1, 70, 54, 1, 0): (13, 6, 4, 1160960, 696576, 999680),
    (3, 16, 3, 1, 70, 54, 1, 1): (10, 6, 4, 1201920, 738560, 999680),
    (3, 16, 3, 1, 63, 65, 0, 0): (13, 5, 6, 2203648, 829696, 1868032),
    (3, 16, 3, 1, 63, 65, 0, 1): (10, 5, 6, 2244608, 871680, 1868032),
    (3, 16, 3, 1, 63, 65, 1, 0): (13, 5, 6, 1220096, 700160, 1048832),
    (3, 16, 3, 1, 63, 65, 1, 1): (10, 5, 6, 1261056, 742144, 1048832),
    (3, 16, 3, 4, 64, 64, 0, 0): (13, 6, 6, 3264512, 3340544, 1827072),
    (3, 16, 3, 4, 64, 64, 0, 1): (10, 6, 6, 3436800, 3508480, 1827072),
    (3, 16, 3, 4, 64, 64, 1, 0): (13, 6, 6, 1728000, 2797312, 999680),
    (3, 16, 3, 4, 64, 64, 1, 1): (10, 6, 6, 1900288, 2965248, 999680),
    (3, 16, 3, 4, 70, 54, 0, 0): (13, 6, 4, 3074304, 3256064, 1827072),
    (3, 16, 3, 4, 70, 54, 0, 1): (10, 6, 4, 3246592, 3424000, 1827072),
    (3, 16, 3, 4, 70, 54, 1, 0): (13, 6, 4, 1632512, 2754816, 999680),
    (3, 16, 3, 4, 70, 54, 1, 1): (10, 6, 4, 1804800, 2922752, 999680),
    (3, 16, 3, 4, 63, 65, 0, 0): (13, 5, 6, 3201792, 3290112, 1868032),
    (3, 16, 3, 4, 63, 65, 0, 1): (10, 5, 6, 3374080, 3458048, 1868032),
    (3, 16, 3, 4, 63, 65, 1, 0): (13, 5, 6, 1725440, 2772224, 1048832),
    (3, 16, 3, 4, 63, 65, 1, 1): (10, 5, 6, 1897728, 2940160, 1048832),
    (3, 16, 5, 1, 64, 64, 0, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 16, 5, 1, 64, 64, 0, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 16, 5, 1, 64, 64, 1, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 16, 5, 1, 64, 64, 1, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 16, 5, 1, 70, 54, 0, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 16, 5, 1, 70, 54, 0, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 16, 5, 1, 70, 54, 1, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 16, 5, 1, 70, 54, 1, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 16, 5, 1, 63, 65, 0, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 16, 5, 1, 63, 65, 0, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 16, 5, 1, 63, 65, 1, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 16, 5, 1, 63, 65, 1, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 16, 5, 4, 64, 64, 0, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 16, 5, 4, 64, 64, 0, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 16, 5, 4, 64, 64, 1, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 16, 5, 4, 64, 64, 1, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 16, 5, 4, 70, 54, 0, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 16, 5, 4, 70, 54, 0, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 16, 5, 4, 70, 54, 1, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 16, 5, 4, 70, 54, 1, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 16, 5, 4, 63, 65, 0, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 16, 5, 4, 63, 65, 0, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 16, 5, 4, 63, 65, 1, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 16, 5, 4, 63, 65, 1, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 64, 1, 1, 64, 64, 0, 0): (7, 30, 30, 2927872, 3418880, 1507584),
    (3, 64, 1, 1, 64, 64, 0, 1): (6, 30, 30, 2969344, 3460864, 1507584),
    (3, 64, 1, 1, 64, 64, 1, 0): (7, 30, 30, 1532672, 2842880, 819456),
    (3, 64, 1, 1, 64, 64, 1, 1): (6, 30, 30, 1574144, 2884864, 819456),
    (3, 64, 1, 1, 70, 54, 0, 0): (7, 33, 25, 2816000, 3884288, 1507584),
    (3, 64, 1, 1, 70, 54, 0, 1): (6, 33, 25, 2857472, 3926272, 1507584),
    (3, 64, 1, 1, 70, 54, 1, 0): (7, 33, 25, 1476608, 3353856, 819456),
    (3, 64, 1, 1, 70, 54, 1, 1): (6, 33, 25, 1518080, 3395840, 819456),
    (3, 64, 1, 1, 63, 65, 0, 0): (7, 29, 30, 3009536, 3377664, 1638656),
    (3, 64, 1, 1, 63, 65, 0, 1): (6, 29, 30, 3051008, 3419648, 1638656),
    (3, 64, 1, 1, 63, 65, 1, 0): (7, 29, 30, 1606144, 2822144, 917760),
    (3, 64, 1, 1, 63, 65, 1, 1): (6, 29, 30, 1647616, 2864128, 917760),
    (3, 64, 1, 4, 64, 64, 0, 0): (7, 30, 30, 7183104, 13572352, 1507584),
    (3, 64, 1, 4, 64, 64, 0, 1): (6, 30, 30, 7353600, 13740288, 1507584),
    (3, 64, 1, 4, 64, 64, 1, 0): (7, 30, 30, 3666176, 11267840, 819456),
    (3, 64, 1, 4, 64, 64, 1, 1): (6, 30, 30, 3836672, 11435776, 819456),
    (3, 64, 1, 4, 70, 54, 0, 0): (7, 33, 25, 6734848, 15433216, 1507584),
    (3, 64, 1, 4, 70, 54, 0, 1): (6, 33, 25, 6905344, 15601152, 1507584),
    (3, 64, 1, 4, 70, 54, 1, 0): (7, 33, 25, 3441664, 13312000, 819456),
    (3, 64, 1, 4, 70, 54, 1, 1): (6, 33, 25, 3612160, 13479936, 819456),
    (3, 64, 1, 4, 63, 65, 0, 0): (7, 29, 30, 7117312, 13408256, 1638656),
    (3, 64, 1, 4, 63, 65, 0, 1): (6, 29, 30, 7287808, 13576192, 1638656),
    (3, 64, 1, 4, 63, 65, 1, 0): (7, 29, 30, 3666176, 11185920, 917760),
    (3, 64, 1, 4, 63, 65, 1, 1): (6, 29, 30, 3836672, 11353856, 917760),
    (3, 64, 3, 1, 64, 64, 0, 0): (13, 6, 6, 24682752, 9631488, 23658752),
    (3, 64, 3, 1, 64, 64, 0, 1): (10, 6, 6, 24822528, 9774848, 23658752),
    (3, 64, 3, 1, 64, 64, 1, 0): (13, 6, 6, 12617472, 9299200, 12091648),
    (3, 64, 3, 1, 64, 64, 1, 1): (10, 6, 6, 12757248, 9442560, 12091648),
    (3, 64, 3, 1, 70, 54, 0, 0): (13, 6, 4, 24525568, 9580032, 23658752),
    (3, 64, 3, 1, 70, 54, 0, 1): (10, 6, 4, 24665344, 9723392, 23658752),
    (3, 64, 3, 1, 70, 54, 1, 0): (13, 6, 4, 12538880, 9273600, 12091648),
    (3, 64, 3, 1, 70, 54, 1, 1): (10, 6, 4, 12678656, 9416960, 12091648),
    (3, 64, 3, 1, 63, 65, 0, 0): (13, 5, 6, 24735488, 9606400, 23789824),
    (3, 64, 3, 1, 63, 65, 0, 1): (10, 5, 6, 24875264, 9749760, 23789824),
    (3, 64, 3, 1, 63, 65, 1, 0): (13, 5, 6, 12676352, 9286400, 12189952),
    (3, 64, 3, 1, 63, 65, 1, 1): (10, 5, 6, 12816128, 9429760, 12189952),
    (3, 64, 3, 4, 64, 64, 0, 0): (13, 6, 6, 27721472, 38413568, 23658752),
    (3, 64, 3, 4, 64, 64, 0, 1): (10, 6, 6, 28312832, 38987008, 23658752),
    (3, 64, 3, 4, 64, 64, 1, 0): (13, 6, 6, 14161152, 37083904, 12091648),
    (3, 64, 3, 4, 64, 64, 1, 1): (10, 6, 6, 14752512, 37657344, 12091648),
    (3, 64, 3, 4, 70, 54, 0, 0): (13, 6, 4, 27089664, 38204672, 23658752),
    (3, 64, 3, 4, 70, 54, 0, 1): (10, 6, 4, 27681024, 38778112, 23658752),
    (3, 64, 3, 4, 70, 54, 1, 0): (13, 6, 4, 13843200, 36977408, 12091648),
    (3, 64, 3, 4, 70, 54, 1, 1): (10, 6, 4, 14434560, 37550848, 12091648),
    (3, 64, 3, 4, 63, 65, 0, 0): (13, 5, 6, 27539968, 38313984, 23789824),
    (3, 64, 3, 4, 63, 65, 0, 1): (10, 5, 6, 28131328, 38887424, 23789824),
    (3, 64, 3, 4, 63, 65, 1, 0): (13, 5, 6, 14103296, 37034240, 12189952),
    (3, 64, 3, 4, 63, 65, 1, 1): (10, 5, 6, 14694656, 37607680, 12189952),
    (3, 64, 5, 1, 64, 64, 0, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 64, 5, 1, 64, 64, 0, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 64, 5, 1, 64, 64, 1, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 64, 5, 1, 64, 64, 1, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 64, 5, 1, 70, 54, 0, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 64, 5, 1, 70, 54, 0, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 64, 5, 1, 70, 54, 1, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 64, 5, 1, 70, 54, 1, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 64, 5, 1, 63, 65, 0, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 64, 5, 1, 63, 65, 0, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 64, 5, 1, 63, 65, 1, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 64, 5, 1, 63, 65, 1, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 64, 5, 4, 64, 64, 0, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 64, 5, 4, 64, 64, 0, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 64, 5, 4, 64, 64, 1, 0): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 64, 5, 4, 64, 64, 1, 1): 'nlayerd: input 64x64 too small for 5 layers',
    (3, 64, 5, 4, 70, 54, 0, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 64, 5, 4, 70, 54, 0, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 64, 5, 4, 70, 54, 1, 0): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 64, 5, 4, 70, 54, 1, 1): 'nlayerd: input 70x54 too small for 5 layers',
    (3, 64, 5, 4, 63, 65, 0, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 64, 5, 4, 63, 65, 0, 1): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 64, 5, 4, 63, 65, 1, 0): 'nlayerd: input 63x65 too small for 5 layers',
    (3, 64, 5, 4, 63, 65, 1, 1): 'nlayerd: input 63x65 too small for 5 layers',
}
# (num_params, ws_bytes, bwd_scratch_bytes)
RD_EXPECTED = {
    ((2, 2, 2, 2), 0, 0): (101, 136216832, 36888832),
    ((2, 2, 2, 2), 0, 1): (101, 68378880, 29122816),
    ((2, 2, 2, 2), 1, 0): (37, 136305920, 36888832),
    ((2, 2, 2, 2), 1, 1): (37, 68467968, 29122816),
    ((3, 4, 6, 3), 0, 0): (191, 269729024, 46522624),
    ((3, 4, 6, 3), 0, 1): (191, 135142656, 33939712),
    ((3, 4, 6, 3), 1, 0): (67, 269905152, 46522624),
    ((3, 4, 6, 3), 1, 1): (67, 135318784, 33939712),
}
# (num_params, ws_bytes, bwd_scratch_bytes)
SR_EXPECTED = {
    (0, 2, 0): (10, 5976320, 7196928),
    (0, 2, 1): (10, 3133696, 5009664),
    (0, 4, 0): (10, 18178304, 26231040),
    (0, 4, 1): (10, 9437440, 19030272),
    (1, 1, 0): (6, 1903872, 6115584),
    (1, 1, 1): (6, 1168640, 5771520),
    (2, 2, 0): (31, 11957504, 11580672),
    (2, 2, 1): (31, 6042880, 7132416),
    (2, 4, 0): (32, 18969856, 23741696),
    (2, 4, 1): (32, 9549056, 15852800),
}
# (num_params, ws_bytes, infer_ws_bytes, bwd_scratch_bytes, wpack_bytes); down = 0: the parent's answers; down = 2, 4: see RDDB_DOWN_PARENT
RDDB_EXPECTED = {
    (0, 0): (96, 50954496, 34242816, 99010816, 17899776),
    (0, 1): (96, 26190080, 17158400, 54958336, 8986880),
    (2, 0): (97, 26573056, 22149376, 27456256, 18063616),
    (2, 1): (97, 13461760, 11111680, 13739776, 9068800),
    (4, 0): (99, 21561088, 20455168, 13854976, 18358528),
    (4, 1): (99, 10852096, 10264576, 6939136, 9216256),
}
# the parent's answers where they differ
RDDB_DOWN_PARENT = {
    (2, 0): (97, 26687744, 22264064, 27456256, 18178304),
    (2, 1): (97, 13519104, 11169024, 13739776, 9126144),
    (4, 0): (99, 21790464, 20684544, 13854976, 18587904),
    (4, 1): (99, 10966784, 10379264, 6939136, 9330944),
}


def test_the_grid_reaches_both_layouts_both_norms_and_a_rejection():
    assert set(D_EXPECTED) == set(D_GRID) and len(D_GRID) == 288
    rejected = [k for k, v in D_EXPECTED.items() if isinstance(v, str)]
    assert rejected and all("too small" in D_EXPECTED[k] for k in rejected)
    ok = [k for k in D_GRID if k not in rejected]
    assert {(k[4] % 2, k[5] % 2) for k in ok} == {(0, 0), (1, 1)} and {k[7] for k in ok} == {0, 1}


@pytest.mark.parametrize("key", D_GRID, ids=lambda k: "-".join(map(str, k)))
def test_nlayerd_planner(lib, key):
    assert d_answer(lib, key) == D_EXPECTED[key]


@pytest.mark.parametrize("key", RD_GRID, ids=str)
def test_resdeconv_planner(lib, key):
    assert rd_answer(lib, key) == RD_EXPECTED[key]


@pytest.mark.parametrize("key", SR_GRID, ids=str)
def test_srnet_planner(lib, key):
    assert sr_answer(lib, key) == SR_EXPECTED[key]


@pytest.mark.parametrize("key", RDDB_GRID, ids=str)
def test_rddbnet_planner(lib, key):
    got = rddb_answer(lib, key)
    assert got == RDDB_EXPECTED[key]
    down, dt = key
    if down == 0:
        assert key not in RDDB_DOWN_PARENT
        return
    # the one permitted difference from the parent: exactly seven one-tap 64 x 64 packs per down stage, in the three sizes that
    # contain the packed weights; the other answers are the parent's
    stages = {2: 1, 4: 2}[down]
    one_tap = lib.srcgan_packed_weight_bytes(64, 64, 1, dt)
    assert one_tap == {0: 16384, 1: 8192}[dt]
    saved = stages * 7 * one_tap
    parent = RDDB_DOWN_PARENT[key]
    assert (parent[0], parent[3]) == (got[0], got[3])
    assert [parent[i] - got[i] for i in (1, 2, 4)] == [saved] * 3


# ---- the op-list families: the parent library's answers (see OPLIST above)
# (num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes, infer_act_bytes, infer_plan)
RDI_EXPECTED = {
    ((1, 1, 1, 1), 0, 0, 0): (59, 59646720, 12284160, 29622784, 774656, (
        0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0, 0, 0, 32768,
        0, 32768, 0, 0, 229376, 32768, 229376, 32768, 0, 0, 0, 32768, 163840, 65536, 0, 0, 229376, 32768, 229376, 32768, 0, 0,
        262144, 32768, 0, 32768, 262144, 32768, 229376, 32768, 229376, 32768, 0, 0, 294912, 16384, 294912, 16384, 0, 0, 311296,
        16384, 311296, 16384, 0, 0, 294912, 16384, 229376, 32768, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 294912,
        16384, 327680, 16384, 311296, 16384, 311296, 16384, 0, 0, 344064, 8192, 344064, 8192, 0, 0, 352256, 8192, 352256, 8192, 0,
        0, 344064, 8192, 311296, 16384, 0, 0, 352256, 8192, 352256, 8192, 0, 0, 360448, 8192, 344064, 8192, 360448, 8192, 352256,
        8192, 352256, 8192, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 327680, 16384, 0, 0, 294912, 16384, 294912,
        16384, 0, 0, 327680, 16384, 327680, 16384, 311296, 16384, 294912, 16384, 294912, 16384, 0, 0, 229376, 32768, 229376, 32768,
        0, 0, 262144, 32768, 262144, 32768, 0, 0, 0, 32768, 0, 32768, 0, 0, 262144, 32768, 262144, 32768, 229376, 32768, 0, 32768,
        0, 32768, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        98304, 65536, 98304, 65536, 163840, 65536, 32768, 65536, 32768, 65536, 0, 0, 368640, 262144, 368640, 262144, 0, 0, 0, 32768)),
    ((1, 1, 1, 1), 0, 0, 1): (59, 59646720, 12284160, 29352448, 512512, (
        0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0, 0, 0, 32768,
        0, 32768, 0, 0, 229376, 32768, 229376, 32768, 0, 0, 0, 32768, 163840, 65536, 0, 0, 229376, 32768, 229376, 32768, 0, 0,
        262144, 32768, 0, 32768, 262144, 32768, 229376, 32768, 229376, 32768, 0, 0, 294912, 16384, 294912, 16384, 0, 0, 311296,
        16384, 311296, 16384, 0, 0, 294912, 16384, 229376, 32768, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 294912,
        16384, 327680, 16384, 311296, 16384, 311296, 16384, 0, 0, 344064, 8192, 344064, 8192, 0, 0, 352256, 8192, 352256, 8192, 0,
        0, 344064, 8192, 311296, 16384, 0, 0, 352256, 8192, 352256, 8192, 0, 0, 360448, 8192, 344064, 8192, 360448, 8192, 352256,
        8192, 352256, 8192, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 327680, 16384, 0, 0, 294912, 16384, 294912,
        16384, 0, 0, 327680, 16384, 327680, 16384, 311296, 16384, 294912, 16384, 294912, 16384, 0, 0, 229376, 32768, 229376, 32768,
        0, 0, 262144, 32768, 262144, 32768, 0, 0, 0, 32768, 0, 32768, 0, 0, 262144, 32768, 262144, 32768, 229376, 32768, 0, 32768,
        0, 32768, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        98304, 65536, 98304, 65536, 163840, 65536, 32768, 65536, 32768, 65536, 0, 0, 0, 32768)),
    ((1, 1, 1, 1), 0, 1, 0): (59, 30016256, 11464960, 14983680, 459264, (
        0, 16384, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920,
        32768, 81920, 32768, 0, 0, 16384, 32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 0, 16384, 0, 16384,
        0, 0, 114688, 16384, 114688, 16384, 0, 0, 0, 16384, 81920, 32768, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384,
        0, 16384, 131072, 16384, 114688, 16384, 114688, 16384, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 155648, 8192, 155648, 8192,
        0, 0, 147456, 8192, 114688, 16384, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 147456, 8192, 163840, 8192, 155648,
        8192, 155648, 8192, 0, 0, 172032, 4096, 172032, 4096, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 172032, 4096, 155648, 8192, 0,
        0, 176128, 4096, 176128, 4096, 0, 0, 180224, 4096, 172032, 4096, 180224, 4096, 176128, 4096, 176128, 4096, 0, 0, 155648,
        8192, 155648, 8192, 0, 0, 163840, 8192, 163840, 8192, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 163840, 8192, 163840, 8192,
        155648, 8192, 147456, 8192, 147456, 8192, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384, 131072, 16384, 0, 0, 0,
        16384, 0, 16384, 0, 0, 131072, 16384, 131072, 16384, 114688, 16384, 0, 16384, 0, 16384, 0, 0, 81920, 32768, 81920, 32768, 0,
        0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 81920, 32768, 16384,
        32768, 16384, 32768, 0, 0, 184320, 131072, 184320, 131072, 0, 0, 0, 16384)),
    ((1, 1, 1, 1), 0, 1, 1): (59, 30016256, 11464960, 14848512, 328192, (
        0, 16384, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920,
        32768, 81920, 32768, 0, 0, 16384, 32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 0, 16384, 0, 16384,
        0, 0, 114688, 16384, 114688, 16384, 0, 0, 0, 16384, 81920, 32768, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384,
        0, 16384, 131072, 16384, 114688, 16384, 114688, 16384, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 155648, 8192, 155648, 8192,
        0, 0, 147456, 8192, 114688, 16384, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 147456, 8192, 163840, 8192, 155648,
        8192, 155648, 8192, 0, 0, 172032, 4096, 172032, 4096, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 172032, 4096, 155648, 8192, 0,
        0, 176128, 4096, 176128, 4096, 0, 0, 180224, 4096, 172032, 4096, 180224, 4096, 176128, 4096, 176128, 4096, 0, 0, 155648,
        8192, 155648, 8192, 0, 0, 163840, 8192, 163840, 8192, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 163840, 8192, 163840, 8192,
        155648, 8192, 147456, 8192, 147456, 8192, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384, 131072, 16384, 0, 0, 0,
        16384, 0, 16384, 0, 0, 131072, 16384, 131072, 16384, 114688, 16384, 0, 16384, 0, 16384, 0, 0, 81920, 32768, 81920, 32768, 0,
        0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 81920, 32768, 16384,
        32768, 16384, 32768, 0, 0, 0, 16384)),
    ((1, 1, 1, 1), 1, 0, 0): (23, 59672320, 12284160, 29626624, 778496, (
        0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0, 0, 0, 32768,
        0, 32768, 0, 0, 229376, 32768, 229376, 32768, 0, 0, 0, 32768, 163840, 65536, 0, 0, 229376, 32768, 229376, 32768, 0, 0,
        262144, 32768, 0, 32768, 262144, 32768, 229376, 32768, 229376, 32768, 0, 0, 294912, 16384, 294912, 16384, 0, 0, 311296,
        16384, 311296, 16384, 0, 0, 294912, 16384, 229376, 32768, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 294912,
        16384, 327680, 16384, 311296, 16384, 311296, 16384, 0, 0, 344064, 8192, 344064, 8192, 0, 0, 352256, 8192, 352256, 8192, 0,
        0, 344064, 8192, 311296, 16384, 0, 0, 352256, 8192, 352256, 8192, 0, 0, 360448, 8192, 344064, 8192, 360448, 8192, 352256,
        8192, 352256, 8192, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 327680, 16384, 0, 0, 294912, 16384, 294912,
        16384, 0, 0, 327680, 16384, 327680, 16384, 311296, 16384, 294912, 16384, 294912, 16384, 0, 0, 229376, 32768, 229376, 32768,
        0, 0, 262144, 32768, 262144, 32768, 0, 0, 0, 32768, 0, 32768, 0, 0, 262144, 32768, 262144, 32768, 229376, 32768, 0, 32768,
        0, 32768, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        98304, 65536, 98304, 65536, 163840, 65536, 32768, 65536, 32768, 65536, 0, 0, 368640, 262144, 368640, 262144, 0, 0, 0, 32768)),
    ((1, 1, 1, 1), 1, 0, 1): (23, 59672320, 12284160, 29356288, 516352, (
        0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0, 0, 0, 32768,
        0, 32768, 0, 0, 229376, 32768, 229376, 32768, 0, 0, 0, 32768, 163840, 65536, 0, 0, 229376, 32768, 229376, 32768, 0, 0,
        262144, 32768, 0, 32768, 262144, 32768, 229376, 32768, 229376, 32768, 0, 0, 294912, 16384, 294912, 16384, 0, 0, 311296,
        16384, 311296, 16384, 0, 0, 294912, 16384, 229376, 32768, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 294912,
        16384, 327680, 16384, 311296, 16384, 311296, 16384, 0, 0, 344064, 8192, 344064, 8192, 0, 0, 352256, 8192, 352256, 8192, 0,
        0, 344064, 8192, 311296, 16384, 0, 0, 352256, 8192, 352256, 8192, 0, 0, 360448, 8192, 344064, 8192, 360448, 8192, 352256,
        8192, 352256, 8192, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 327680, 16384, 0, 0, 294912, 16384, 294912,
        16384, 0, 0, 327680, 16384, 327680, 16384, 311296, 16384, 294912, 16384, 294912, 16384, 0, 0, 229376, 32768, 229376, 32768,
        0, 0, 262144, 32768, 262144, 32768, 0, 0, 0, 32768, 0, 32768, 0, 0, 262144, 32768, 262144, 32768, 229376, 32768, 0, 32768,
        0, 32768, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        98304, 65536, 98304, 65536, 163840, 65536, 32768, 65536, 32768, 65536, 0, 0, 0, 32768)),
    ((1, 1, 1, 1), 1, 1, 0): (23, 30041856, 11464960, 14987520, 463104, (
        0, 16384, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920,
        32768, 81920, 32768, 0, 0, 16384, 32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 0, 16384, 0, 16384,
        0, 0, 114688, 16384, 114688, 16384, 0, 0, 0, 16384, 81920, 32768, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384,
        0, 16384, 131072, 16384, 114688, 16384, 114688, 16384, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 155648, 8192, 155648, 8192,
        0, 0, 147456, 8192, 114688, 16384, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 147456, 8192, 163840, 8192, 155648,
        8192, 155648, 8192, 0, 0, 172032, 4096, 172032, 4096, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 172032, 4096, 155648, 8192, 0,
        0, 176128, 4096, 176128, 4096, 0, 0, 180224, 4096, 172032, 4096, 180224, 4096, 176128, 4096, 176128, 4096, 0, 0, 155648,
        8192, 155648, 8192, 0, 0, 163840, 8192, 163840, 8192, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 163840, 8192, 163840, 8192,
        155648, 8192, 147456, 8192, 147456, 8192, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384, 131072, 16384, 0, 0, 0,
        16384, 0, 16384, 0, 0, 131072, 16384, 131072, 16384, 114688, 16384, 0, 16384, 0, 16384, 0, 0, 81920, 32768, 81920, 32768, 0,
        0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 81920, 32768, 16384,
        32768, 16384, 32768, 0, 0, 184320, 131072, 184320, 131072, 0, 0, 0, 16384)),
    ((1, 1, 1, 1), 1, 1, 1): (23, 30041856, 11464960, 14852352, 332032, (
        0, 16384, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920,
        32768, 81920, 32768, 0, 0, 16384, 32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 0, 16384, 0, 16384,
        0, 0, 114688, 16384, 114688, 16384, 0, 0, 0, 16384, 81920, 32768, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384,
        0, 16384, 131072, 16384, 114688, 16384, 114688, 16384, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 155648, 8192, 155648, 8192,
        0, 0, 147456, 8192, 114688, 16384, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 147456, 8192, 163840, 8192, 155648,
        8192, 155648, 8192, 0, 0, 172032, 4096, 172032, 4096, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 172032, 4096, 155648, 8192, 0,
        0, 176128, 4096, 176128, 4096, 0, 0, 180224, 4096, 172032, 4096, 180224, 4096, 176128, 4096, 176128, 4096, 0, 0, 155648,
        8192, 155648, 8192, 0, 0, 163840, 8192, 163840, 8192, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 163840, 8192, 163840, 8192,
        155648, 8192, 147456, 8192, 147456, 8192, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384, 131072, 16384, 0, 0, 0,
        16384, 0, 16384, 0, 0, 131072, 16384, 131072, 16384, 114688, 16384, 0, 16384, 0, 16384, 0, 0, 81920, 32768, 81920, 32768, 0,
        0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 81920, 32768, 16384,
        32768, 16384, 32768, 0, 0, 0, 16384)),
    ((2, 1, 1, 1), 0, 0, 0): (71, 61351680, 12808448, 30212608, 774656, (
        0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0, 0, 98304,
        65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 163840, 65536, 32768, 65536, 32768,
        65536, 0, 0, 0, 32768, 0, 32768, 0, 0, 229376, 32768, 229376, 32768, 0, 0, 0, 32768, 32768, 65536, 0, 0, 229376, 32768,
        229376, 32768, 0, 0, 262144, 32768, 0, 32768, 262144, 32768, 229376, 32768, 229376, 32768, 0, 0, 294912, 16384, 294912,
        16384, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 294912, 16384, 229376, 32768, 0, 0, 311296, 16384, 311296, 16384, 0, 0,
        327680, 16384, 294912, 16384, 327680, 16384, 311296, 16384, 311296, 16384, 0, 0, 344064, 8192, 344064, 8192, 0, 0, 352256,
        8192, 352256, 8192, 0, 0, 344064, 8192, 311296, 16384, 0, 0, 352256, 8192, 352256, 8192, 0, 0, 360448, 8192, 344064, 8192,
        360448, 8192, 352256, 8192, 352256, 8192, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 327680, 16384, 0, 0,
        294912, 16384, 294912, 16384, 0, 0, 327680, 16384, 327680, 16384, 311296, 16384, 294912, 16384, 294912, 16384, 0, 0, 229376,
        32768, 229376, 32768, 0, 0, 262144, 32768, 262144, 32768, 0, 0, 0, 32768, 0, 32768, 0, 0, 262144, 32768, 262144, 32768,
        229376, 32768, 0, 32768, 0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 98304, 65536,
        98304, 65536, 0, 0, 163840, 65536, 163840, 65536, 32768, 65536, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768,
        65536, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0,
        0, 368640, 262144, 368640, 262144, 0, 0, 0, 32768)),
    ((2, 1, 1, 1), 0, 0, 1): (71, 61351680, 12808448, 29942272, 512512, (
        0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0, 0, 98304,
        65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 163840, 65536, 32768, 65536, 32768,
        65536, 0, 0, 0, 32768, 0, 32768, 0, 0, 229376, 32768, 229376, 32768, 0, 0, 0, 32768, 32768, 65536, 0, 0, 229376, 32768,
        229376, 32768, 0, 0, 262144, 32768, 0, 32768, 262144, 32768, 229376, 32768, 229376, 32768, 0, 0, 294912, 16384, 294912,
        16384, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 294912, 16384, 229376, 32768, 0, 0, 311296, 16384, 311296, 16384, 0, 0,
        327680, 16384, 294912, 16384, 327680, 16384, 311296, 16384, 311296, 16384, 0, 0, 344064, 8192, 344064, 8192, 0, 0, 352256,
        8192, 352256, 8192, 0, 0, 344064, 8192, 311296, 16384, 0, 0, 352256, 8192, 352256, 8192, 0, 0, 360448, 8192, 344064, 8192,
        360448, 8192, 352256, 8192, 352256, 8192, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 327680, 16384, 0, 0,
        294912, 16384, 294912, 16384, 0, 0, 327680, 16384, 327680, 16384, 311296, 16384, 294912, 16384, 294912, 16384, 0, 0, 229376,
        32768, 229376, 32768, 0, 0, 262144, 32768, 262144, 32768, 0, 0, 0, 32768, 0, 32768, 0, 0, 262144, 32768, 262144, 32768,
        229376, 32768, 0, 32768, 0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 98304, 65536,
        98304, 65536, 0, 0, 163840, 65536, 163840, 65536, 32768, 65536, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768,
        65536, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0,
        0, 0, 32768)),
    ((2, 1, 1, 1), 0, 1, 0): (71, 30869248, 11727104, 15278592, 459264, (
        0, 16384, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920,
        32768, 81920, 32768, 0, 0, 16384, 32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 49152, 32768, 49152,
        32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 81920, 32768, 16384, 32768, 16384, 32768, 0, 0,
        0, 16384, 0, 16384, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 0, 16384, 16384, 32768, 0, 0, 114688, 16384, 114688, 16384, 0,
        0, 131072, 16384, 0, 16384, 131072, 16384, 114688, 16384, 114688, 16384, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 155648,
        8192, 155648, 8192, 0, 0, 147456, 8192, 114688, 16384, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 147456, 8192,
        163840, 8192, 155648, 8192, 155648, 8192, 0, 0, 172032, 4096, 172032, 4096, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 172032,
        4096, 155648, 8192, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 180224, 4096, 172032, 4096, 180224, 4096, 176128, 4096, 176128,
        4096, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 163840, 8192, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 163840,
        8192, 163840, 8192, 155648, 8192, 147456, 8192, 147456, 8192, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384,
        131072, 16384, 0, 0, 0, 16384, 0, 16384, 0, 0, 131072, 16384, 131072, 16384, 114688, 16384, 0, 16384, 0, 16384, 0, 0, 16384,
        32768, 16384, 32768, 0, 0, 81920, 32768, 81920, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 81920, 32768, 81920, 32768,
        16384, 32768, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920, 32768, 81920, 32768, 0, 0, 16384,
        32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 184320, 131072, 184320, 131072, 0, 0, 0, 16384)),
    ((2, 1, 1, 1), 0, 1, 1): (71, 30869248, 11727104, 15143424, 328192, (
        0, 16384, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920,
        32768, 81920, 32768, 0, 0, 16384, 32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 49152, 32768, 49152,
        32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 81920, 32768, 16384, 32768, 16384, 32768, 0, 0,
        0, 16384, 0, 16384, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 0, 16384, 16384, 32768, 0, 0, 114688, 16384, 114688, 16384, 0,
        0, 131072, 16384, 0, 16384, 131072, 16384, 114688, 16384, 114688, 16384, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 155648,
        8192, 155648, 8192, 0, 0, 147456, 8192, 114688, 16384, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 147456, 8192,
        163840, 8192, 155648, 8192, 155648, 8192, 0, 0, 172032, 4096, 172032, 4096, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 172032,
        4096, 155648, 8192, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 180224, 4096, 172032, 4096, 180224, 4096, 176128, 4096, 176128,
        4096, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 163840, 8192, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 163840,
        8192, 163840, 8192, 155648, 8192, 147456, 8192, 147456, 8192, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384,
        131072, 16384, 0, 0, 0, 16384, 0, 16384, 0, 0, 131072, 16384, 131072, 16384, 114688, 16384, 0, 16384, 0, 16384, 0, 0, 16384,
        32768, 16384, 32768, 0, 0, 81920, 32768, 81920, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 81920, 32768, 81920, 32768,
        16384, 32768, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920, 32768, 81920, 32768, 0, 0, 16384,
        32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 0, 16384)),
    ((2, 1, 1, 1), 1, 0, 0): (27, 61378304, 12808448, 30216448, 778496, (
        0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0, 0, 98304,
        65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 163840, 65536, 32768, 65536, 32768,
        65536, 0, 0, 0, 32768, 0, 32768, 0, 0, 229376, 32768, 229376, 32768, 0, 0, 0, 32768, 32768, 65536, 0, 0, 229376, 32768,
        229376, 32768, 0, 0, 262144, 32768, 0, 32768, 262144, 32768, 229376, 32768, 229376, 32768, 0, 0, 294912, 16384, 294912,
        16384, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 294912, 16384, 229376, 32768, 0, 0, 311296, 16384, 311296, 16384, 0, 0,
        327680, 16384, 294912, 16384, 327680, 16384, 311296, 16384, 311296, 16384, 0, 0, 344064, 8192, 344064, 8192, 0, 0, 352256,
        8192, 352256, 8192, 0, 0, 344064, 8192, 311296, 16384, 0, 0, 352256, 8192, 352256, 8192, 0, 0, 360448, 8192, 344064, 8192,
        360448, 8192, 352256, 8192, 352256, 8192, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 327680, 16384, 0, 0,
        294912, 16384, 294912, 16384, 0, 0, 327680, 16384, 327680, 16384, 311296, 16384, 294912, 16384, 294912, 16384, 0, 0, 229376,
        32768, 229376, 32768, 0, 0, 262144, 32768, 262144, 32768, 0, 0, 0, 32768, 0, 32768, 0, 0, 262144, 32768, 262144, 32768,
        229376, 32768, 0, 32768, 0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 98304, 65536,
        98304, 65536, 0, 0, 163840, 65536, 163840, 65536, 32768, 65536, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768,
        65536, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0,
        0, 368640, 262144, 368640, 262144, 0, 0, 0, 32768)),
    ((2, 1, 1, 1), 1, 0, 1): (27, 61378304, 12808448, 29946112, 516352, (
        0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0,
        163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0, 0, 98304,
        65536, 98304, 65536, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 98304, 65536, 98304, 65536, 163840, 65536, 32768, 65536, 32768,
        65536, 0, 0, 0, 32768, 0, 32768, 0, 0, 229376, 32768, 229376, 32768, 0, 0, 0, 32768, 32768, 65536, 0, 0, 229376, 32768,
        229376, 32768, 0, 0, 262144, 32768, 0, 32768, 262144, 32768, 229376, 32768, 229376, 32768, 0, 0, 294912, 16384, 294912,
        16384, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 294912, 16384, 229376, 32768, 0, 0, 311296, 16384, 311296, 16384, 0, 0,
        327680, 16384, 294912, 16384, 327680, 16384, 311296, 16384, 311296, 16384, 0, 0, 344064, 8192, 344064, 8192, 0, 0, 352256,
        8192, 352256, 8192, 0, 0, 344064, 8192, 311296, 16384, 0, 0, 352256, 8192, 352256, 8192, 0, 0, 360448, 8192, 344064, 8192,
        360448, 8192, 352256, 8192, 352256, 8192, 0, 0, 311296, 16384, 311296, 16384, 0, 0, 327680, 16384, 327680, 16384, 0, 0,
        294912, 16384, 294912, 16384, 0, 0, 327680, 16384, 327680, 16384, 311296, 16384, 294912, 16384, 294912, 16384, 0, 0, 229376,
        32768, 229376, 32768, 0, 0, 262144, 32768, 262144, 32768, 0, 0, 0, 32768, 0, 32768, 0, 0, 262144, 32768, 262144, 32768,
        229376, 32768, 0, 32768, 0, 32768, 0, 0, 32768, 65536, 32768, 65536, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 98304, 65536,
        98304, 65536, 0, 0, 163840, 65536, 163840, 65536, 32768, 65536, 98304, 65536, 98304, 65536, 0, 0, 32768, 65536, 32768,
        65536, 0, 0, 163840, 65536, 163840, 65536, 0, 0, 32768, 65536, 32768, 65536, 98304, 65536, 163840, 65536, 163840, 65536, 0,
        0, 0, 32768)),
    ((2, 1, 1, 1), 1, 1, 0): (27, 30895872, 11727104, 15282432, 463104, (
        0, 16384, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920,
        32768, 81920, 32768, 0, 0, 16384, 32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 49152, 32768, 49152,
        32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 81920, 32768, 16384, 32768, 16384, 32768, 0, 0,
        0, 16384, 0, 16384, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 0, 16384, 16384, 32768, 0, 0, 114688, 16384, 114688, 16384, 0,
        0, 131072, 16384, 0, 16384, 131072, 16384, 114688, 16384, 114688, 16384, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 155648,
        8192, 155648, 8192, 0, 0, 147456, 8192, 114688, 16384, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 147456, 8192,
        163840, 8192, 155648, 8192, 155648, 8192, 0, 0, 172032, 4096, 172032, 4096, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 172032,
        4096, 155648, 8192, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 180224, 4096, 172032, 4096, 180224, 4096, 176128, 4096, 176128,
        4096, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 163840, 8192, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 163840,
        8192, 163840, 8192, 155648, 8192, 147456, 8192, 147456, 8192, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384,
        131072, 16384, 0, 0, 0, 16384, 0, 16384, 0, 0, 131072, 16384, 131072, 16384, 114688, 16384, 0, 16384, 0, 16384, 0, 0, 16384,
        32768, 16384, 32768, 0, 0, 81920, 32768, 81920, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 81920, 32768, 81920, 32768,
        16384, 32768, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920, 32768, 81920, 32768, 0, 0, 16384,
        32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 184320, 131072, 184320, 131072, 0, 0, 0, 16384)),
    ((2, 1, 1, 1), 1, 1, 1): (27, 30895872, 11727104, 15147264, 332032, (
        0, 16384, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920,
        32768, 81920, 32768, 0, 0, 16384, 32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 49152, 32768, 49152,
        32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 49152, 32768, 49152, 32768, 81920, 32768, 16384, 32768, 16384, 32768, 0, 0,
        0, 16384, 0, 16384, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 0, 16384, 16384, 32768, 0, 0, 114688, 16384, 114688, 16384, 0,
        0, 131072, 16384, 0, 16384, 131072, 16384, 114688, 16384, 114688, 16384, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 155648,
        8192, 155648, 8192, 0, 0, 147456, 8192, 114688, 16384, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 147456, 8192,
        163840, 8192, 155648, 8192, 155648, 8192, 0, 0, 172032, 4096, 172032, 4096, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 172032,
        4096, 155648, 8192, 0, 0, 176128, 4096, 176128, 4096, 0, 0, 180224, 4096, 172032, 4096, 180224, 4096, 176128, 4096, 176128,
        4096, 0, 0, 155648, 8192, 155648, 8192, 0, 0, 163840, 8192, 163840, 8192, 0, 0, 147456, 8192, 147456, 8192, 0, 0, 163840,
        8192, 163840, 8192, 155648, 8192, 147456, 8192, 147456, 8192, 0, 0, 114688, 16384, 114688, 16384, 0, 0, 131072, 16384,
        131072, 16384, 0, 0, 0, 16384, 0, 16384, 0, 0, 131072, 16384, 131072, 16384, 114688, 16384, 0, 16384, 0, 16384, 0, 0, 16384,
        32768, 16384, 32768, 0, 0, 81920, 32768, 81920, 32768, 0, 0, 49152, 32768, 49152, 32768, 0, 0, 81920, 32768, 81920, 32768,
        16384, 32768, 49152, 32768, 49152, 32768, 0, 0, 16384, 32768, 16384, 32768, 0, 0, 81920, 32768, 81920, 32768, 0, 0, 16384,
        32768, 16384, 32768, 49152, 32768, 81920, 32768, 81920, 32768, 0, 0, 0, 16384)),
}
# (num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes, infer_act_bytes, infer_plan)
SRI_EXPECTED = {
    (0, 2, 0, 0): (10, 1220864, 1323264, 848128, 612608, (
        0, 12288, 0, 0, 12288, 49152, 12288, 49152, 0, 0, 61440, 49152, 61440, 49152, 0, 0, 110592, 24576, 110592, 24576, 0, 0,
        135168, 196608, 135168, 196608, 0, 0, 331776, 196608, 331776, 196608, 0, 0, 61440, 49152)),
    (0, 2, 0, 1): (10, 733440, 1034496, 528640, 348416, (
        0, 6144, 0, 0, 6144, 24576, 6144, 24576, 0, 0, 30720, 24576, 30720, 24576, 0, 0, 55296, 12288, 55296, 12288, 0, 0, 67584,
        98304, 67584, 98304, 0, 0, 165888, 98304, 165888, 98304, 0, 0, 30720, 24576)),
    (0, 3, 0, 0): (10, 2153216, 2969856, 1645312, 1299200, (
        0, 12288, 0, 0, 12288, 49152, 12288, 49152, 0, 0, 61440, 49152, 61440, 49152, 0, 0, 110592, 24576, 110592, 24576, 0, 0,
        135168, 442368, 135168, 442368, 0, 0, 577536, 442368, 577536, 442368, 0, 0, 1019904, 110592)),
    (0, 3, 0, 1): (10, 1297152, 2404608, 1024768, 733952, (
        0, 6144, 0, 0, 6144, 24576, 6144, 24576, 0, 0, 30720, 24576, 30720, 24576, 0, 0, 55296, 12288, 55296, 12288, 0, 0, 67584,
        221184, 67584, 221184, 0, 0, 288768, 221184, 288768, 221184, 0, 0, 509952, 55296)),
    (1, 1, 0, 0): (6, 738048, 1475840, 340736, 119552, (
        0, 12288, 0, 0, 12288, 49152, 12288, 49152, 0, 0, 61440, 24576, 61440, 24576, 0, 0, 0, 12288)),
    (1, 1, 0, 1): (6, 520960, 1426688, 295680, 76544, (
        0, 6144, 0, 0, 6144, 24576, 6144, 24576, 0, 0, 30720, 12288, 30720, 12288, 0, 0, 0, 6144)),
    (2, 1, 2, 0): (18, 1030912, 713984, 482560, 242944, (
        0, 12288, 0, 0, 12288, 49152, 12288, 49152, 0, 0, 61440, 49152, 61440, 49152, 0, 0, 110592, 49152, 110592, 49152, 0, 0,
        61440, 49152, 61440, 49152, 12288, 49152, 110592, 49152, 110592, 49152, 0, 0, 61440, 49152, 61440, 49152, 0, 0, 159744,
        49152, 159744, 49152, 0, 0, 61440, 49152, 61440, 49152, 110592, 49152, 159744, 49152, 159744, 49152, 12288, 49152, 110592,
        49152, 110592, 49152, 0, 0, 0, 12288)),
    (2, 1, 2, 1): (18, 551680, 455936, 267520, 138496, (
        0, 6144, 0, 0, 6144, 24576, 6144, 24576, 0, 0, 30720, 24576, 30720, 24576, 0, 0, 55296, 24576, 55296, 24576, 0, 0, 30720,
        24576, 30720, 24576, 6144, 24576, 55296, 24576, 55296, 24576, 0, 0, 30720, 24576, 30720, 24576, 0, 0, 79872, 24576, 79872,
        24576, 0, 0, 30720, 24576, 30720, 24576, 55296, 24576, 79872, 24576, 79872, 24576, 6144, 24576, 55296, 24576, 55296, 24576,
        0, 0, 0, 6144)),
    (2, 2, 1, 0): (13, 952064, 915712, 621824, 439552, (
        0, 12288, 0, 0, 12288, 49152, 12288, 49152, 0, 0, 61440, 49152, 61440, 49152, 0, 0, 110592, 49152, 110592, 49152, 0, 0,
        61440, 49152, 61440, 49152, 12288, 49152, 110592, 49152, 110592, 49152, 12288, 49152, 61440, 49152, 61440, 49152, 0, 0,
        159744, 196608, 159744, 196608, 0, 0, 61440, 49152)),
    (2, 2, 1, 1): (13, 511744, 639232, 337152, 236800, (
        0, 6144, 0, 0, 6144, 24576, 6144, 24576, 0, 0, 30720, 24576, 30720, 24576, 0, 0, 55296, 24576, 55296, 24576, 0, 0, 30720,
        24576, 30720, 24576, 6144, 24576, 55296, 24576, 55296, 24576, 6144, 24576, 30720, 24576, 30720, 24576, 0, 0, 79872, 98304,
        79872, 98304, 0, 0, 30720, 24576)),
    (2, 4, 2, 0): (20, 2263808, 3033856, 1498368, 1225984, (
        0, 12288, 0, 0, 12288, 49152, 12288, 49152, 0, 0, 61440, 49152, 61440, 49152, 0, 0, 110592, 49152, 110592, 49152, 0, 0,
        61440, 49152, 61440, 49152, 12288, 49152, 110592, 49152, 110592, 49152, 0, 0, 61440, 49152, 61440, 49152, 0, 0, 159744,
        49152, 159744, 49152, 0, 0, 61440, 49152, 61440, 49152, 110592, 49152, 159744, 49152, 159744, 49152, 12288, 49152, 110592,
        49152, 110592, 49152, 0, 0, 208896, 196608, 208896, 196608, 0, 0, 405504, 786432, 405504, 786432, 0, 0, 208896, 196608)),
    (2, 4, 2, 1): (20, 1168128, 2192128, 775424, 630016, (
        0, 6144, 0, 0, 6144, 24576, 6144, 24576, 0, 0, 30720, 24576, 30720, 24576, 0, 0, 55296, 24576, 55296, 24576, 0, 0, 30720,
        24576, 30720, 24576, 6144, 24576, 55296, 24576, 55296, 24576, 0, 0, 30720, 24576, 30720, 24576, 0, 0, 79872, 24576, 79872,
        24576, 0, 0, 30720, 24576, 30720, 24576, 55296, 24576, 79872, 24576, 79872, 24576, 6144, 24576, 55296, 24576, 55296, 24576,
        0, 0, 104448, 98304, 104448, 98304, 0, 0, 202752, 393216, 202752, 393216, 0, 0, 104448, 98304)),
}
# (num_params, out_h, out_w, ws_bytes, bwd_scratch_bytes, infer_ws_bytes)
SD_EXPECTED = {
    (0, 2, 0): (20, 24, 16, 8229120, 8503552, 5425408),
    (0, 2, 1): (20, 24, 16, 4336896, 8224000, 2796800),
    (0, 4, 0): (20, 48, 32, 9875712, 18023680, 7072000),
    (0, 4, 1): (20, 48, 32, 5160192, 16920832, 3620096),
    (1, 2, 0): (20, 6, 4, 6002432, 5488384, 3198720),
    (1, 2, 1): (20, 6, 4, 3223808, 5404928, 1683712),
    (1, 4, 0): (20, 3, 2, 6007552, 5494528, 3203840),
    (1, 4, 1): (20, 3, 2, 3226368, 5408512, 1686272),
}
# (num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes, infer_act_bytes, infer_plan)
RCAN_EXPECTED = {
    (2, 0): (32, 585984, 307968, 315392, 112640, (
        0, 2560, 0, 0, 2560, 2560, 2560, 2560, 0, 0, 5120, 5120, 5120, 5120, 0, 0, 10240, 5120, 10240, 5120, 0, 0, 15360, 5120,
        15360, 5120, 5120, 5120, 10240, 5120, 10240, 5120, 5120, 5120, 15360, 5120, 15360, 5120, 0, 0, 10240, 5120, 10240, 5120, 0,
        0, 20480, 5120, 20480, 5120, 15360, 5120, 10240, 5120, 10240, 5120, 15360, 5120, 20480, 5120, 20480, 5120, 5120, 5120,
        15360, 5120, 15360, 5120, 0, 0, 25600, 20480, 25600, 20480, 0, 0, 46080, 20480, 46080, 20480, 0, 0, 66560, 10240, 66560,
        10240, 0, 0, 76800, 10240)),
    (2, 1): (32, 490240, 249088, 271872, 69120, (
        0, 1280, 0, 0, 1280, 1280, 1280, 1280, 0, 0, 2560, 2560, 2560, 2560, 0, 0, 5120, 2560, 5120, 2560, 0, 0, 7680, 2560, 7680,
        2560, 2560, 2560, 5120, 2560, 5120, 2560, 2560, 2560, 7680, 2560, 7680, 2560, 0, 0, 5120, 2560, 5120, 2560, 0, 0, 10240,
        2560, 10240, 2560, 7680, 2560, 5120, 2560, 5120, 2560, 7680, 2560, 10240, 2560, 10240, 2560, 2560, 2560, 7680, 2560, 7680,
        2560, 0, 0, 12800, 10240, 12800, 10240, 0, 0, 23040, 10240, 23040, 10240, 0, 0, 33280, 5120, 33280, 5120, 0, 0, 38400, 5120)),
    (3, 0): (32, 849920, 736256, 487168, 210688, (
        0, 2560, 0, 0, 2560, 2560, 2560, 2560, 0, 0, 5120, 5120, 5120, 5120, 0, 0, 10240, 5120, 10240, 5120, 0, 0, 15360, 5120,
        15360, 5120, 5120, 5120, 10240, 5120, 10240, 5120, 5120, 5120, 15360, 5120, 15360, 5120, 0, 0, 10240, 5120, 10240, 5120, 0,
        0, 20480, 5120, 20480, 5120, 15360, 5120, 10240, 5120, 10240, 5120, 15360, 5120, 20480, 5120, 20480, 5120, 5120, 5120,
        15360, 5120, 15360, 5120, 0, 0, 25600, 46080, 25600, 46080, 0, 0, 71680, 46080, 71680, 46080, 0, 0, 117760, 23040, 117760,
        23040, 0, 0, 140800, 23040)),
    (3, 1): (32, 678912, 638976, 405248, 128768, (
        0, 1280, 0, 0, 1280, 1280, 1280, 1280, 0, 0, 2560, 2560, 2560, 2560, 0, 0, 5120, 2560, 5120, 2560, 0, 0, 7680, 2560, 7680,
        2560, 2560, 2560, 5120, 2560, 5120, 2560, 2560, 2560, 7680, 2560, 7680, 2560, 0, 0, 5120, 2560, 5120, 2560, 0, 0, 10240,
        2560, 10240, 2560, 7680, 2560, 5120, 2560, 5120, 2560, 7680, 2560, 10240, 2560, 10240, 2560, 2560, 2560, 7680, 2560, 7680,
        2560, 0, 0, 12800, 23040, 12800, 23040, 0, 0, 35840, 23040, 35840, 23040, 0, 0, 58880, 11520, 58880, 11520, 0, 0, 70400,
        11520)),
    (4, 0): (34, 921856, 616704, 577536, 337920, (
        0, 2560, 0, 0, 2560, 2560, 2560, 2560, 0, 0, 5120, 5120, 5120, 5120, 0, 0, 10240, 5120, 10240, 5120, 0, 0, 15360, 5120,
        15360, 5120, 5120, 5120, 10240, 5120, 10240, 5120, 5120, 5120, 15360, 5120, 15360, 5120, 0, 0, 10240, 5120, 10240, 5120, 0,
        0, 20480, 5120, 20480, 5120, 15360, 5120, 10240, 5120, 10240, 5120, 15360, 5120, 20480, 5120, 20480, 5120, 5120, 5120,
        15360, 5120, 15360, 5120, 0, 0, 25600, 20480, 25600, 20480, 0, 0, 46080, 20480, 46080, 20480, 0, 0, 66560, 81920, 66560,
        81920, 0, 0, 148480, 81920, 148480, 81920, 0, 0, 230400, 40960, 230400, 40960, 0, 0, 271360, 40960)),
    (4, 1): (34, 676608, 445184, 421376, 181760, (
        0, 1280, 0, 0, 1280, 1280, 1280, 1280, 0, 0, 2560, 2560, 2560, 2560, 0, 0, 5120, 2560, 5120, 2560, 0, 0, 7680, 2560, 7680,
        2560, 2560, 2560, 5120, 2560, 5120, 2560, 2560, 2560, 7680, 2560, 7680, 2560, 0, 0, 5120, 2560, 5120, 2560, 0, 0, 10240,
        2560, 10240, 2560, 7680, 2560, 5120, 2560, 5120, 2560, 7680, 2560, 10240, 2560, 10240, 2560, 2560, 2560, 7680, 2560, 7680,
        2560, 0, 0, 12800, 10240, 12800, 10240, 0, 0, 23040, 10240, 23040, 10240, 0, 0, 33280, 40960, 33280, 40960, 0, 0, 74240,
        40960, 74240, 40960, 0, 0, 115200, 20480, 115200, 20480, 0, 0, 135680, 20480)),
    (8, 0): (36, 1933568, 2098944, 1515520, 1239040, (
        0, 2560, 0, 0, 2560, 2560, 2560, 2560, 0, 0, 5120, 5120, 5120, 5120, 0, 0, 10240, 5120, 10240, 5120, 0, 0, 15360, 5120,
        15360, 5120, 5120, 5120, 10240, 5120, 10240, 5120, 5120, 5120, 15360, 5120, 15360, 5120, 0, 0, 10240, 5120, 10240, 5120, 0,
        0, 20480, 5120, 20480, 5120, 15360, 5120, 10240, 5120, 10240, 5120, 15360, 5120, 20480, 5120, 20480, 5120, 5120, 5120,
        15360, 5120, 15360, 5120, 0, 0, 25600, 20480, 25600, 20480, 0, 0, 46080, 20480, 46080, 20480, 0, 0, 66560, 81920, 66560,
        81920, 0, 0, 148480, 81920, 148480, 81920, 0, 0, 230400, 327680, 230400, 327680, 0, 0, 558080, 327680, 558080, 327680, 0, 0,
        885760, 163840, 885760, 163840, 0, 0, 1049600, 163840)),
    (8, 1): (36, 1200896, 1476864, 908800, 632320, (
        0, 1280, 0, 0, 1280, 1280, 1280, 1280, 0, 0, 2560, 2560, 2560, 2560, 0, 0, 5120, 2560, 5120, 2560, 0, 0, 7680, 2560, 7680,
        2560, 2560, 2560, 5120, 2560, 5120, 2560, 2560, 2560, 7680, 2560, 7680, 2560, 0, 0, 5120, 2560, 5120, 2560, 0, 0, 10240,
        2560, 10240, 2560, 7680, 2560, 5120, 2560, 5120, 2560, 7680, 2560, 10240, 2560, 10240, 2560, 2560, 2560, 7680, 2560, 7680,
        2560, 0, 0, 12800, 10240, 12800, 10240, 0, 0, 23040, 10240, 23040, 10240, 0, 0, 33280, 40960, 33280, 40960, 0, 0, 74240,
        40960, 74240, 40960, 0, 0, 115200, 163840, 115200, 163840, 0, 0, 279040, 163840, 279040, 163840, 0, 0, 442880, 81920,
        442880, 81920, 0, 0, 524800, 81920)),
}
# (num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes, infer_act_bytes, infer_plan)
DDBPN_EXPECTED = {
    (2, 0): (135, 16581376, 1793280, 10388224, 230144, (
        0, 960, 0, 0, 1024, 960, 1024, 960, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 17408, 15360, 17408, 15360, 0, 0, 32768, 3840,
        32768, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 17408, 15360, 17408, 15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 17408,
        15360, 17408, 15360, 0, 0, 32768, 3840, 32768, 3840, 36608, 3840, 40448, 3840, 40448, 3840, 0, 0, 17408, 15360, 17408,
        15360, 2048, 15360, 44288, 92160, 44288, 92160, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 40448, 3840, 40448, 3840, 0, 0, 36608,
        3840, 36608, 3840, 0, 0, 2048, 15360, 2048, 15360, 44288, 92160, 17408, 15360, 17408, 15360, 0, 0, 2048, 15360, 2048, 15360,
        0, 0, 40448, 3840, 40448, 3840, 36608, 3840, 136448, 19200, 136448, 19200, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 17408,
        15360, 17408, 15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 36608, 3840, 36608, 3840, 136448, 19200, 40448, 3840, 40448,
        3840, 0, 0, 2048, 15360, 2048, 15360, 17408, 15360, 44288, 92160, 44288, 92160, 0, 0, 17408, 15360, 17408, 15360, 0, 0,
        2048, 15360, 2048, 15360, 0, 0, 17408, 15360, 17408, 15360, 0, 0, 40448, 3840, 40448, 3840, 0, 0, 36608, 3840, 36608, 3840,
        0, 0, 17408, 15360, 17408, 15360, 2048, 15360, 155648, 15360, 155648, 15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 40448,
        3840, 40448, 3840, 36608, 3840, 136448, 19200, 136448, 19200, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 3840, 40448,
        3840, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 155648, 15360, 155648, 15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 36608, 3840,
        36608, 3840, 40448, 3840, 32768, 3840, 32768, 3840, 0, 0, 2048, 15360, 2048, 15360, 155648, 15360, 44288, 92160, 44288,
        92160, 0, 0, 155648, 15360, 155648, 15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 155648, 15360, 155648, 15360, 0, 0, 32768,
        3840, 32768, 3840, 0, 0, 40448, 3840, 40448, 3840, 0, 0, 155648, 15360, 155648, 15360, 2048, 15360, 17408, 15360, 17408,
        15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 32768, 3840, 32768, 3840, 40448, 3840, 136448, 19200, 136448, 19200, 0, 0,
        40448, 3840, 40448, 3840, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 17408, 15360, 17408, 15360,
        0, 0, 2048, 15360, 2048, 15360, 0, 0, 40448, 3840, 40448, 3840, 32768, 3840, 36608, 3840, 36608, 3840, 0, 0, 2048, 15360,
        2048, 15360, 17408, 15360, 44288, 92160, 44288, 92160, 0, 0, 17408, 15360, 17408, 15360, 0, 0, 2048, 15360, 2048, 15360, 0,
        0, 17408, 15360, 17408, 15360, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 17408, 15360, 17408,
        15360, 2048, 15360, 155648, 15360, 155648, 15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 36608, 3840, 36608, 3840, 32768,
        3840, 136448, 19200, 136448, 19200, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 2048, 15360, 2048,
        15360, 0, 0, 155648, 15360, 155648, 15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 32768, 3840, 32768, 3840, 36608, 3840,
        40448, 3840, 40448, 3840, 0, 0, 2048, 15360, 2048, 15360, 155648, 15360, 44288, 92160, 44288, 92160, 0, 0, 155648, 15360,
        155648, 15360, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 155648, 15360, 155648, 15360, 0, 0, 40448, 3840, 40448, 3840, 0, 0,
        36608, 3840, 36608, 3840, 0, 0, 155648, 15360, 155648, 15360, 2048, 15360, 17408, 15360, 17408, 15360, 0, 0, 2048, 15360,
        2048, 15360, 0, 0, 40448, 3840, 40448, 3840, 36608, 3840, 136448, 19200, 136448, 19200, 0, 0, 36608, 3840, 36608, 3840, 0,
        0, 40448, 3840, 40448, 3840, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 17408, 15360, 17408, 15360, 0, 0, 2048, 15360, 2048,
        15360, 0, 0, 36608, 3840, 36608, 3840, 40448, 3840, 32768, 3840, 32768, 3840, 0, 0, 2048, 15360, 2048, 15360, 17408, 15360,
        44288, 92160, 44288, 92160, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 40448, 3840)),
    (2, 1): (135, 10850560, 1252096, 7694080, 145152, (
        0, 480, 0, 0, 512, 480, 512, 480, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680, 8704, 7680, 0, 0, 16384, 1920, 16384,
        1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 8704, 7680, 8704, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680, 8704,
        7680, 0, 0, 16384, 1920, 16384, 1920, 18432, 1920, 20480, 1920, 20480, 1920, 0, 0, 8704, 7680, 8704, 7680, 1024, 7680,
        22528, 46080, 22528, 46080, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 20480, 1920, 20480, 1920, 0, 0, 18432, 1920, 18432, 1920, 0,
        0, 1024, 7680, 1024, 7680, 22528, 46080, 8704, 7680, 8704, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 20480, 1920, 20480,
        1920, 18432, 1920, 68608, 9600, 68608, 9600, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680, 8704, 7680, 0, 0, 1024, 7680,
        1024, 7680, 0, 0, 18432, 1920, 18432, 1920, 68608, 9600, 20480, 1920, 20480, 1920, 0, 0, 1024, 7680, 1024, 7680, 8704, 7680,
        22528, 46080, 22528, 46080, 0, 0, 8704, 7680, 8704, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680, 8704, 7680, 0, 0,
        20480, 1920, 20480, 1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 8704, 7680, 8704, 7680, 1024, 7680, 78336, 7680, 78336,
        7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 20480, 1920, 20480, 1920, 18432, 1920, 68608, 9600, 68608, 9600, 0, 0, 18432,
        1920, 18432, 1920, 0, 0, 20480, 1920, 20480, 1920, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 78336, 7680, 78336, 7680, 0, 0, 1024,
        7680, 1024, 7680, 0, 0, 18432, 1920, 18432, 1920, 20480, 1920, 16384, 1920, 16384, 1920, 0, 0, 1024, 7680, 1024, 7680,
        78336, 7680, 22528, 46080, 22528, 46080, 0, 0, 78336, 7680, 78336, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 78336, 7680,
        78336, 7680, 0, 0, 16384, 1920, 16384, 1920, 0, 0, 20480, 1920, 20480, 1920, 0, 0, 78336, 7680, 78336, 7680, 1024, 7680,
        8704, 7680, 8704, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 16384, 1920, 16384, 1920, 20480, 1920, 68608, 9600, 68608, 9600,
        0, 0, 20480, 1920, 20480, 1920, 0, 0, 16384, 1920, 16384, 1920, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680, 8704, 7680,
        0, 0, 1024, 7680, 1024, 7680, 0, 0, 20480, 1920, 20480, 1920, 16384, 1920, 18432, 1920, 18432, 1920, 0, 0, 1024, 7680, 1024,
        7680, 8704, 7680, 22528, 46080, 22528, 46080, 0, 0, 8704, 7680, 8704, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680,
        8704, 7680, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 16384, 1920, 16384, 1920, 0, 0, 8704, 7680, 8704, 7680, 1024, 7680, 78336,
        7680, 78336, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 18432, 1920, 18432, 1920, 16384, 1920, 68608, 9600, 68608, 9600, 0,
        0, 16384, 1920, 16384, 1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 78336, 7680, 78336, 7680,
        0, 0, 1024, 7680, 1024, 7680, 0, 0, 16384, 1920, 16384, 1920, 18432, 1920, 20480, 1920, 20480, 1920, 0, 0, 1024, 7680, 1024,
        7680, 78336, 7680, 22528, 46080, 22528, 46080, 0, 0, 78336, 7680, 78336, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 78336,
        7680, 78336, 7680, 0, 0, 20480, 1920, 20480, 1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 78336, 7680, 78336, 7680, 1024,
        7680, 8704, 7680, 8704, 7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 20480, 1920, 20480, 1920, 18432, 1920, 68608, 9600, 68608,
        9600, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 20480, 1920, 20480, 1920, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680, 8704,
        7680, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 18432, 1920, 18432, 1920, 20480, 1920, 16384, 1920, 16384, 1920, 0, 0, 1024, 7680,
        1024, 7680, 8704, 7680, 22528, 46080, 22528, 46080, 0, 0, 16384, 1920, 16384, 1920, 0, 0, 20480, 1920)),
    (4, 0): (135, 31526656, 5751552, 18512128, 784640, (
        0, 960, 0, 0, 1024, 960, 1024, 960, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 17408, 15360, 17408, 15360, 0, 0, 32768, 3840,
        32768, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 126464, 61440, 126464, 61440, 0, 0,
        40448, 86016, 40448, 86016, 0, 0, 32768, 3840, 32768, 3840, 36608, 3840, 187904, 3840, 187904, 3840, 0, 0, 40448, 86016,
        40448, 86016, 126464, 61440, 191744, 368640, 191744, 368640, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 187904, 3840, 187904,
        3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 86016, 40448, 86016, 191744, 368640, 126464, 61440, 126464, 61440, 0, 0,
        40448, 86016, 40448, 86016, 0, 0, 187904, 3840, 187904, 3840, 36608, 3840, 560384, 19200, 560384, 19200, 0, 0, 40448, 86016,
        40448, 86016, 0, 0, 126464, 61440, 126464, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 36608, 3840, 36608, 3840, 560384,
        19200, 187904, 3840, 187904, 3840, 0, 0, 40448, 86016, 40448, 86016, 126464, 61440, 191744, 368640, 191744, 368640, 0, 0,
        126464, 61440, 126464, 61440, 0, 0, 579584, 61440, 579584, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 187904, 3840,
        187904, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 86016, 40448, 86016, 579584, 61440, 126464, 61440, 126464, 61440,
        0, 0, 40448, 86016, 40448, 86016, 0, 0, 187904, 3840, 187904, 3840, 36608, 3840, 560384, 19200, 560384, 19200, 0, 0, 36608,
        3840, 36608, 3840, 0, 0, 187904, 3840, 187904, 3840, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 126464, 61440, 126464, 61440,
        0, 0, 40448, 86016, 40448, 86016, 0, 0, 36608, 3840, 36608, 3840, 187904, 3840, 32768, 3840, 32768, 3840, 0, 0, 40448,
        86016, 40448, 86016, 126464, 61440, 191744, 368640, 191744, 368640, 0, 0, 126464, 61440, 126464, 61440, 0, 0, 579584, 61440,
        579584, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 187904, 3840, 187904, 3840, 0, 0,
        40448, 86016, 40448, 86016, 579584, 61440, 126464, 61440, 126464, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 32768,
        3840, 32768, 3840, 187904, 3840, 560384, 19200, 560384, 19200, 0, 0, 187904, 3840, 187904, 3840, 0, 0, 32768, 3840, 32768,
        3840, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 126464, 61440, 126464, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 187904,
        3840, 187904, 3840, 32768, 3840, 36608, 3840, 36608, 3840, 0, 0, 40448, 86016, 40448, 86016, 126464, 61440, 191744, 368640,
        191744, 368640, 0, 0, 126464, 61440, 126464, 61440, 0, 0, 579584, 61440, 579584, 61440, 0, 0, 40448, 86016, 40448, 86016, 0,
        0, 36608, 3840, 36608, 3840, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 40448, 86016, 40448, 86016, 579584, 61440, 126464, 61440,
        126464, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 36608, 3840, 36608, 3840, 32768, 3840, 560384, 19200, 560384, 19200,
        0, 0, 32768, 3840, 32768, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 126464, 61440,
        126464, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 32768, 3840, 32768, 3840, 36608, 3840, 187904, 3840, 187904, 3840, 0,
        0, 40448, 86016, 40448, 86016, 126464, 61440, 191744, 368640, 191744, 368640, 0, 0, 126464, 61440, 126464, 61440, 0, 0,
        579584, 61440, 579584, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 187904, 3840, 187904, 3840, 0, 0, 36608, 3840, 36608,
        3840, 0, 0, 40448, 86016, 40448, 86016, 579584, 61440, 126464, 61440, 126464, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0,
        187904, 3840, 187904, 3840, 36608, 3840, 560384, 19200, 560384, 19200, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 187904, 3840,
        187904, 3840, 0, 0, 40448, 86016, 40448, 86016, 0, 0, 126464, 61440, 126464, 61440, 0, 0, 40448, 86016, 40448, 86016, 0, 0,
        36608, 3840, 36608, 3840, 187904, 3840, 32768, 3840, 32768, 3840, 0, 0, 40448, 86016, 40448, 86016, 126464, 61440, 191744,
        368640, 191744, 368640, 0, 0, 17408, 15360, 17408, 15360, 0, 0, 2048, 15360)),
    (4, 1): (135, 20257536, 3456768, 13690624, 464640, (
        0, 480, 0, 0, 512, 480, 512, 480, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680, 8704, 7680, 0, 0, 16384, 1920, 16384,
        1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 63488, 30720, 63488, 30720, 0, 0, 20480,
        43008, 20480, 43008, 0, 0, 16384, 1920, 16384, 1920, 18432, 1920, 94208, 1920, 94208, 1920, 0, 0, 20480, 43008, 20480,
        43008, 63488, 30720, 96256, 184320, 96256, 184320, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 94208, 1920, 94208, 1920, 0, 0,
        18432, 1920, 18432, 1920, 0, 0, 20480, 43008, 20480, 43008, 96256, 184320, 63488, 30720, 63488, 30720, 0, 0, 20480, 43008,
        20480, 43008, 0, 0, 94208, 1920, 94208, 1920, 18432, 1920, 280576, 9600, 280576, 9600, 0, 0, 20480, 43008, 20480, 43008, 0,
        0, 63488, 30720, 63488, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 18432, 1920, 18432, 1920, 280576, 9600, 94208, 1920,
        94208, 1920, 0, 0, 20480, 43008, 20480, 43008, 63488, 30720, 96256, 184320, 96256, 184320, 0, 0, 63488, 30720, 63488, 30720,
        0, 0, 290304, 30720, 290304, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 94208, 1920, 94208, 1920, 0, 0, 18432, 1920,
        18432, 1920, 0, 0, 20480, 43008, 20480, 43008, 290304, 30720, 63488, 30720, 63488, 30720, 0, 0, 20480, 43008, 20480, 43008,
        0, 0, 94208, 1920, 94208, 1920, 18432, 1920, 280576, 9600, 280576, 9600, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 94208, 1920,
        94208, 1920, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 63488, 30720, 63488, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0,
        18432, 1920, 18432, 1920, 94208, 1920, 16384, 1920, 16384, 1920, 0, 0, 20480, 43008, 20480, 43008, 63488, 30720, 96256,
        184320, 96256, 184320, 0, 0, 63488, 30720, 63488, 30720, 0, 0, 290304, 30720, 290304, 30720, 0, 0, 20480, 43008, 20480,
        43008, 0, 0, 16384, 1920, 16384, 1920, 0, 0, 94208, 1920, 94208, 1920, 0, 0, 20480, 43008, 20480, 43008, 290304, 30720,
        63488, 30720, 63488, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 16384, 1920, 16384, 1920, 94208, 1920, 280576, 9600,
        280576, 9600, 0, 0, 94208, 1920, 94208, 1920, 0, 0, 16384, 1920, 16384, 1920, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 63488,
        30720, 63488, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 94208, 1920, 94208, 1920, 16384, 1920, 18432, 1920, 18432,
        1920, 0, 0, 20480, 43008, 20480, 43008, 63488, 30720, 96256, 184320, 96256, 184320, 0, 0, 63488, 30720, 63488, 30720, 0, 0,
        290304, 30720, 290304, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 16384, 1920, 16384,
        1920, 0, 0, 20480, 43008, 20480, 43008, 290304, 30720, 63488, 30720, 63488, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0,
        18432, 1920, 18432, 1920, 16384, 1920, 280576, 9600, 280576, 9600, 0, 0, 16384, 1920, 16384, 1920, 0, 0, 18432, 1920, 18432,
        1920, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 63488, 30720, 63488, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 16384,
        1920, 16384, 1920, 18432, 1920, 94208, 1920, 94208, 1920, 0, 0, 20480, 43008, 20480, 43008, 63488, 30720, 96256, 184320,
        96256, 184320, 0, 0, 63488, 30720, 63488, 30720, 0, 0, 290304, 30720, 290304, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0,
        94208, 1920, 94208, 1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 20480, 43008, 20480, 43008, 290304, 30720, 63488, 30720,
        63488, 30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 94208, 1920, 94208, 1920, 18432, 1920, 280576, 9600, 280576, 9600, 0,
        0, 18432, 1920, 18432, 1920, 0, 0, 94208, 1920, 94208, 1920, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 63488, 30720, 63488,
        30720, 0, 0, 20480, 43008, 20480, 43008, 0, 0, 18432, 1920, 18432, 1920, 94208, 1920, 16384, 1920, 16384, 1920, 0, 0, 20480,
        43008, 20480, 43008, 63488, 30720, 96256, 184320, 96256, 184320, 0, 0, 8704, 7680, 8704, 7680, 0, 0, 1024, 7680)),
    (8, 0): (135, 122734336, 22223616, 72407296, 2775296, (
        0, 960, 0, 0, 1024, 960, 1024, 960, 0, 0, 2048, 15360, 2048, 15360, 0, 0, 17408, 15360, 17408, 15360, 0, 0, 32768, 3840,
        32768, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 384512, 245760, 384512, 245760, 0, 0,
        40448, 344064, 40448, 344064, 0, 0, 32768, 3840, 32768, 3840, 36608, 3840, 630272, 3840, 630272, 3840, 0, 0, 40448, 344064,
        40448, 344064, 384512, 245760, 634112, 1474560, 634112, 1474560, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 630272, 3840,
        630272, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 344064, 40448, 344064, 634112, 1474560, 384512, 245760, 384512,
        245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 630272, 3840, 630272, 3840, 36608, 3840, 2108672, 19200, 2108672, 19200,
        0, 0, 40448, 344064, 40448, 344064, 0, 0, 384512, 245760, 384512, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 36608,
        3840, 36608, 3840, 2108672, 19200, 630272, 3840, 630272, 3840, 0, 0, 40448, 344064, 40448, 344064, 384512, 245760, 634112,
        1474560, 634112, 1474560, 0, 0, 384512, 245760, 384512, 245760, 0, 0, 2127872, 245760, 2127872, 245760, 0, 0, 40448, 344064,
        40448, 344064, 0, 0, 630272, 3840, 630272, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 344064, 40448, 344064,
        2127872, 245760, 384512, 245760, 384512, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 630272, 3840, 630272, 3840,
        36608, 3840, 2108672, 19200, 2108672, 19200, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 630272, 3840, 630272, 3840, 0, 0, 40448,
        344064, 40448, 344064, 0, 0, 384512, 245760, 384512, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 36608, 3840, 36608,
        3840, 630272, 3840, 32768, 3840, 32768, 3840, 0, 0, 40448, 344064, 40448, 344064, 384512, 245760, 634112, 1474560, 634112,
        1474560, 0, 0, 384512, 245760, 384512, 245760, 0, 0, 2127872, 245760, 2127872, 245760, 0, 0, 40448, 344064, 40448, 344064,
        0, 0, 32768, 3840, 32768, 3840, 0, 0, 630272, 3840, 630272, 3840, 0, 0, 40448, 344064, 40448, 344064, 2127872, 245760,
        384512, 245760, 384512, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 32768, 3840, 32768, 3840, 630272, 3840, 2108672,
        19200, 2108672, 19200, 0, 0, 630272, 3840, 630272, 3840, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 40448, 344064, 40448, 344064,
        0, 0, 384512, 245760, 384512, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 630272, 3840, 630272, 3840, 32768, 3840,
        36608, 3840, 36608, 3840, 0, 0, 40448, 344064, 40448, 344064, 384512, 245760, 634112, 1474560, 634112, 1474560, 0, 0,
        384512, 245760, 384512, 245760, 0, 0, 2127872, 245760, 2127872, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 36608,
        3840, 36608, 3840, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 40448, 344064, 40448, 344064, 2127872, 245760, 384512, 245760,
        384512, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 36608, 3840, 36608, 3840, 32768, 3840, 2108672, 19200, 2108672,
        19200, 0, 0, 32768, 3840, 32768, 3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 384512,
        245760, 384512, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 32768, 3840, 32768, 3840, 36608, 3840, 630272, 3840,
        630272, 3840, 0, 0, 40448, 344064, 40448, 344064, 384512, 245760, 634112, 1474560, 634112, 1474560, 0, 0, 384512, 245760,
        384512, 245760, 0, 0, 2127872, 245760, 2127872, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 630272, 3840, 630272,
        3840, 0, 0, 36608, 3840, 36608, 3840, 0, 0, 40448, 344064, 40448, 344064, 2127872, 245760, 384512, 245760, 384512, 245760,
        0, 0, 40448, 344064, 40448, 344064, 0, 0, 630272, 3840, 630272, 3840, 36608, 3840, 2108672, 19200, 2108672, 19200, 0, 0,
        36608, 3840, 36608, 3840, 0, 0, 630272, 3840, 630272, 3840, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 384512, 245760,
        384512, 245760, 0, 0, 40448, 344064, 40448, 344064, 0, 0, 36608, 3840, 36608, 3840, 630272, 3840, 32768, 3840, 32768, 3840,
        0, 0, 40448, 344064, 40448, 344064, 384512, 245760, 634112, 1474560, 634112, 1474560, 0, 0, 2373632, 61440, 2373632, 61440,
        0, 0, 2435072, 61440)),
    (8, 1): (135, 78905088, 13320960, 53681920, 1527552, (
        0, 480, 0, 0, 512, 480, 512, 480, 0, 0, 1024, 7680, 1024, 7680, 0, 0, 8704, 7680, 8704, 7680, 0, 0, 16384, 1920, 16384,
        1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 192512, 122880, 192512, 122880, 0, 0, 20480,
        172032, 20480, 172032, 0, 0, 16384, 1920, 16384, 1920, 18432, 1920, 315392, 1920, 315392, 1920, 0, 0, 20480, 172032, 20480,
        172032, 192512, 122880, 317440, 737280, 317440, 737280, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 315392, 1920, 315392,
        1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 20480, 172032, 20480, 172032, 317440, 737280, 192512, 122880, 192512, 122880, 0,
        0, 20480, 172032, 20480, 172032, 0, 0, 315392, 1920, 315392, 1920, 18432, 1920, 1054720, 9600, 1054720, 9600, 0, 0, 20480,
        172032, 20480, 172032, 0, 0, 192512, 122880, 192512, 122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 18432, 1920, 18432,
        1920, 1054720, 9600, 315392, 1920, 315392, 1920, 0, 0, 20480, 172032, 20480, 172032, 192512, 122880, 317440, 737280, 317440,
        737280, 0, 0, 192512, 122880, 192512, 122880, 0, 0, 1064448, 122880, 1064448, 122880, 0, 0, 20480, 172032, 20480, 172032, 0,
        0, 315392, 1920, 315392, 1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 20480, 172032, 20480, 172032, 1064448, 122880, 192512,
        122880, 192512, 122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 315392, 1920, 315392, 1920, 18432, 1920, 1054720, 9600,
        1054720, 9600, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 315392, 1920, 315392, 1920, 0, 0, 20480, 172032, 20480, 172032, 0, 0,
        192512, 122880, 192512, 122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 18432, 1920, 18432, 1920, 315392, 1920, 16384,
        1920, 16384, 1920, 0, 0, 20480, 172032, 20480, 172032, 192512, 122880, 317440, 737280, 317440, 737280, 0, 0, 192512, 122880,
        192512, 122880, 0, 0, 1064448, 122880, 1064448, 122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 16384, 1920, 16384, 1920,
        0, 0, 315392, 1920, 315392, 1920, 0, 0, 20480, 172032, 20480, 172032, 1064448, 122880, 192512, 122880, 192512, 122880, 0, 0,
        20480, 172032, 20480, 172032, 0, 0, 16384, 1920, 16384, 1920, 315392, 1920, 1054720, 9600, 1054720, 9600, 0, 0, 315392,
        1920, 315392, 1920, 0, 0, 16384, 1920, 16384, 1920, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 192512, 122880, 192512,
        122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 315392, 1920, 315392, 1920, 16384, 1920, 18432, 1920, 18432, 1920, 0, 0,
        20480, 172032, 20480, 172032, 192512, 122880, 317440, 737280, 317440, 737280, 0, 0, 192512, 122880, 192512, 122880, 0, 0,
        1064448, 122880, 1064448, 122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 16384, 1920,
        16384, 1920, 0, 0, 20480, 172032, 20480, 172032, 1064448, 122880, 192512, 122880, 192512, 122880, 0, 0, 20480, 172032,
        20480, 172032, 0, 0, 18432, 1920, 18432, 1920, 16384, 1920, 1054720, 9600, 1054720, 9600, 0, 0, 16384, 1920, 16384, 1920, 0,
        0, 18432, 1920, 18432, 1920, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 192512, 122880, 192512, 122880, 0, 0, 20480, 172032,
        20480, 172032, 0, 0, 16384, 1920, 16384, 1920, 18432, 1920, 315392, 1920, 315392, 1920, 0, 0, 20480, 172032, 20480, 172032,
        192512, 122880, 317440, 737280, 317440, 737280, 0, 0, 192512, 122880, 192512, 122880, 0, 0, 1064448, 122880, 1064448,
        122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 315392, 1920, 315392, 1920, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 20480,
        172032, 20480, 172032, 1064448, 122880, 192512, 122880, 192512, 122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 315392,
        1920, 315392, 1920, 18432, 1920, 1054720, 9600, 1054720, 9600, 0, 0, 18432, 1920, 18432, 1920, 0, 0, 315392, 1920, 315392,
        1920, 0, 0, 20480, 172032, 20480, 172032, 0, 0, 192512, 122880, 192512, 122880, 0, 0, 20480, 172032, 20480, 172032, 0, 0,
        18432, 1920, 18432, 1920, 315392, 1920, 16384, 1920, 16384, 1920, 0, 0, 20480, 172032, 20480, 172032, 192512, 122880,
        317440, 737280, 317440, 737280, 0, 0, 1187328, 30720, 1187328, 30720, 0, 0, 1218048, 30720)),
}
# (num_params, ws_bytes, bwd_scratch_bytes, infer_ws_bytes)
VGG_EXPECTED = {
    (0, 2, 32, 32, 0): (20, 66191872, 1048832, 35136000),
    (0, 2, 32, 32, 1): (20, 33403392, 524544, 17875456),
    (0, 1, 40, 24, 0): (20, 63537664, 491776, 32725504),
    (0, 1, 40, 24, 1): (20, 31932928, 246016, 16526848),
    (1, 2, 32, 32, 0): (32, 165593600, 1048832, 84746752),
    (1, 2, 32, 32, 1): (32, 83104256, 524544, 42680832),
    (1, 1, 40, 24, 0): (32, 162748928, 491776, 82287104),
    (1, 1, 40, 24, 1): (32, 81538560, 246016, 41307648),
}
OPLIST_EXPECTED = {"RDI": RDI_EXPECTED, "SRI": SRI_EXPECTED, "SD": SD_EXPECTED, "RCAN": RCAN_EXPECTED, "DDBPN": DDBPN_EXPECTED, "VGG": VGG_EXPECTED}


def test_the_oplist_grids_reach_every_planner_branch():
    assert {k[3] for k in RDI_GRID} == {0, 1} and {k[1] for k in RDI_GRID} == {0, 1}                   # fold_tail, norm
    assert {k[0] for k in SRI_GRID} == {0, 1, 2} and (2, 2, 1, 0) in SRI_GRID                           # kinds; EDSR's one-block spare slot
    assert {(k[0], k[1]) for k in SD_GRID} == {(0, 2), (0, 4), (1, 2), (1, 4)}                          # x4: the shared module
    assert {k[0] for k in RCAN_GRID} == {2, 3, 4, 8} and {k[0] for k in DDBPN_GRID} == {2, 4, 8}
    assert {k[0] for k in VGG_GRID} == {0, 1}
    for name, (grid, _) in OPLIST.items():
        assert set(OPLIST_EXPECTED[name]) == set(grid) and {k[-1] for k in grid if name != "RDI"} <= {0, 1}
        assert {(k[2] if name == "RDI" else k[-1]) for k in grid} == {0, 1}                             # both dtypes


@pytest.mark.parametrize("name,key", [(name, k) for name, (grid, _) in OPLIST.items() for k in grid], ids=lambda v: str(v).replace(" ", ""))
def test_oplist_planner(lib, name, key):
    got = OPLIST[name][1](lib, key)
    want = OPLIST_EXPECTED[name][key]
    assert got[:5] == want[:5]          # the sizes first: a short message when one moves
    assert got == want
