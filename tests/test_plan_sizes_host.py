"""CPU: what the planners of nets.hip answer -- parameter counts, output sizes, workspace / scratch / packed-weight bytes -- pinned
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


def collect(l):
    """Every answer, as the literal tables below hold them."""
    return {"D": {k: d_answer(l, k) for k in D_GRID}, "RD": {k: rd_answer(l, k) for k in RD_GRID},
            "SR": {k: sr_answer(l, k) for k in SR_GRID}, "RDDB": {k: rddb_answer(l, k) for k in RDDB_GRID}}


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
