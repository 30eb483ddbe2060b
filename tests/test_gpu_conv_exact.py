"""Direct tests of the MFMA kernels behind srcgan_conv_igemm, srcgan_conv_wgrad and srcgan_wgrad_dense.

Two kinds of assertion only (operands and references: tests/conv_exact.py):
  * exact -- small-integer operands, for which every order of f32 summation gives the same bits: `torch.equal` with a float64
    reference cast once to the storage type, on the WHOLE output buffer (sentinels around the slice, between the lattice points of a
    strided store and behind the last row must survive), the operand buffers compared with their copies afterwards;
  * per element against float64 on random reals with the production constants: |out - ref| <= eps_T |ref| + (K + 8) 2^-23 N.
Every call runs with the launch profiler on and records the kernel class (template instance) it was served by; the last test holds
the classes seen against EXPECTED_CLASSES, the list of instances reachable through the C ABI with the default environment, so a
change of dispatch that moves coverage fails here.  The case tables are plain data: tests/test_conv_exact_teeth.py runs the
generator's conditions for every case on the CPU."""
import collections
import itertools

import pytest
import torch

import conv_exact as CE
from conv_exact import conv_case, par_case, wgrad_case, dense_case, DTS, TDT
from ws_guard import NAN, guarded_slabs

pytestmark = pytest.mark.gpu

B16 = ("bf16", "fp16")
SHAPES3 = [(5, 7), (16, 33), (35, 70)]       # 32 x 16 tiles of the 3x3 kernels: one ragged tile; a one-pixel second column; all nine tile classes


# ------------------------------------------------------------------------------------------------------------------ case tables
def _conv3x3_cases():
    L = []
    # -- 3x3 stride 1, Cout <= 32 on blocked buffers (the dense-block forms): three stages + resident weights (Cin 64), resident
    #    weights (96, 128), streamed weights (160, 192); epilogue sets none / mz / sign_in / sign_out / r1 + r2 + mz
    for i, cin in enumerate((64, 96, 128, 160, 192)):
        for j, em in enumerate((0, 4, 8, 16, 7)):
            hw = SHAPES3[(i + j) % 3]
            n = f"c3b_cin{cin}_e{em}"
            if em == 0:
                L.append(conv_case(n, cin=cin, hw=hw, blocked=True, y_in_x=True, x_cs=cin + 32, y_coff=cin, act=True))
            elif em == 4:
                L.append(conv_case(n, cin=cin, hw=hw, blocked=True, bias=False, mz=True, mz_coff=32, mz_cs=64, ep_blocked=True, alpha=0.5))
            elif em == 8:
                L.append(conv_case(n, cin=cin, hw=hw, blocked=True, bias=False, sign_in=True, dts=B16))
            elif em == 16:
                L.append(conv_case(n, cin=cin, hw=hw, blocked=True, y_in_x=True, x_cs=cin + 32, y_coff=cin, act=True, sign_out=True, dts=B16))
            else:
                L.append(conv_case(n, cin=cin, hw=hw, blocked=True, alpha=0.5, r1="x", r1_coff=32, r2=True, mz=True, mz_c0=8))
    # -- the same kernels on interleaved tensors: 16-byte direct (d16), 8-byte direct (d8: y_coff % 8 == 4), row epilogue (Cout < 32),
    #    and the per-element form (Cout 3, 1; a channel stride that is no multiple of 4)
    for i, cin in enumerate((64, 128, 160)):
        hw = SHAPES3[i]
        L.append(conv_case(f"c3i_cin{cin}_d16", cin=cin, hw=hw, act=True, y_extra=(0, 0)))
        L.append(conv_case(f"c3i_cin{cin}_d8", cin=cin, hw=hw, act=True, y_coff=4, y_cs=40))
        L.append(conv_case(f"c3i_cin{cin}_mz4", cin=cin, hw=hw, mz=True, y_coff=4, y_cs=40, mz_coff=4, mz_cs=36, mz_c0=4, bias=False))
        L.append(conv_case(f"c3i_cin{cin}_co16", cin=cin, cout=16, hw=hw, y_coff=8, y_cs=32, y_extra=(3, 2), alpha=0.5))
        L.append(conv_case(f"c3i_cin{cin}_co3", cin=cin, cout=3, hw=hw, y_cs=8, act=True))
        L.append(conv_case(f"c3i_cin{cin}_odd_cs", cin=cin, hw=hw, y_coff=1, y_cs=35, r1="own", r1_cs=33, r1_coff=1, r1_cend=20))
    L.append(conv_case("c3i_cin64_co1", cin=64, cout=1, hw=(16, 33), y_cs=8))
    L.append(conv_case("c3i_cin8_co32", cin=8, hw=(16, 33), act=True))                                  # one K chunk
    L.append(conv_case("c3b_sign_in_d8", cin=64, hw=(16, 33), blocked=True, bias=False, sign_in=True, y_coff=4, y_cs=40, dts=B16))
    L.append(conv_case("c3b_sign_out_rows", cin=96, hw=(16, 33), blocked=True, y_in_x=True, x_cs=160, y_coff=104, act=True, sign_out=True, dts=B16))
    for cin in (64, 96, 160):               # the remaining epilogue forms of the sign-mask instances, at each weight-residency form
        L.append(conv_case(f"c3b_cin{cin}_sign_in_rows", cin=cin, hw=(16, 33), blocked=True, bias=False, sign_in=True, y_blocked=True, y_coff=8, y_cs=64, dts=B16))
        L.append(conv_case(f"c3b_cin{cin}_sign_out_d8", cin=cin, hw=(16, 33), blocked=True, act=True, sign_out=True, y_coff=4, y_cs=40, dts=B16))
        if cin != 64:
            L.append(conv_case(f"c3b_cin{cin}_sign_in_d8", cin=cin, hw=(5, 7), blocked=True, bias=False, sign_in=True, y_coff=4, y_cs=40, dts=B16))
        if cin != 96:
            L.append(conv_case(f"c3b_cin{cin}_sign_out_rows", cin=cin, hw=(5, 7), blocked=True, y_in_x=True, x_cs=cin + 64, y_coff=cin + 8, act=True, sign_out=True, dts=B16))
    # -- the persistent loop: more work units than 2 x CUs + 3, walked forwards and backwards
    for rev in (0, 1):
        L.append(conv_case(f"c3b_persistent_rev{rev}", cin=64, hw=(35, 70), B=CE.PERSISTENT, blocked=True, y_in_x=True, x_cs=96, y_coff=64, act=True, rev=rev))
    # -- Cout > 32: 64, and 96 for a ragged second channel tile; sets 0, 1, 3, 4, sign_in, and 5 (the EM == 7 instance) as the in-place
    #    dense-gradient form: G[0:96) += conv^T(G[96:128)), channels >= 64 times LeakyReLU'(mz)
    for i, (cout, em) in enumerate(((64, 0), (96, 0), (64, 1), (96, 3), (64, 4), (96, 4))):
        hw = SHAPES3[i % 3]
        kw = dict(cin=64, cout=cout, hw=hw)
        if em & 1:
            kw.update(r1="x", r1_coff=0, r1_cend=64, alpha=0.5)
        if em & 2:
            kw.update(r2=True, r2_cend=cout)
        if em & 4:
            kw.update(mz=True, mz_c0=32)
        L.append(conv_case(f"c3i_co{cout}_e{em}", **kw))
        L.append(conv_case(f"c3b_co{cout}_e{em}", blocked=True, **kw))
    L.append(conv_case("c3i_co64_sign_in", cin=8, cout=64, hw=(16, 33), bias=False, sign_in=True, dts=B16))
    L.append(conv_case("c3i_dgrad_accumulate", cin=32, x_coff=96, x_cs=128, cout=96, hw=(16, 33), y_in_x=True, bias=False, r1="y", r1_cend=96, beta1=1.0,
                       mz=True, mz_c0=64, mz_cs=128))
    L.append(conv_case("c3i_dgrad_accumulate_co32", cin=32, x_coff=32, x_cs=64, cout=32, hw=(16, 33), y_in_x=True, bias=False, r1="y", r1_cend=32, beta1=1.0,
                       mz=True, mz_c0=16))
    L.append(conv_case("c3i_co64_odd_cs", cin=64, cout=64, hw=(5, 7), y_coff=1, y_cs=67, act=True))
    L.append(conv_case("c3i_co64_odd_cs_e1", cin=64, cout=64, hw=(5, 7), y_coff=1, y_cs=67, r1="x", r1_cend=64, alpha=0.5))
    L.append(conv_case("c3i_co64_odd_cs_e3", cin=64, cout=64, hw=(16, 33), y_coff=1, y_cs=67, r1="x", r1_cend=64, alpha=0.5, r2=True))
    L.append(conv_case("c3i_co96_odd_cs_e5", cin=64, cout=96, hw=(5, 7), y_coff=1, y_cs=99, r1="own", r1_cend=40, mz=True, mz_c0=50))
    L.append(conv_case("c3i_co66", cin=64, cout=66, hw=(16, 33), y_cs=66, mz=True, mz_c0=3))
    # -- 3x3 stride 1 with a strided store (os = 2, oa = ob = 0, y of 2 OH x 2 OW): parity (0, 0) of the 7x7 s2 p3 input gradient
    #    (3 taps per axis, lead 1), with the caller's operands -- in-place accumulation r1 == y, the ReLU' mask with mslope 0.  At
    #    Cout == 32 in 16 bits the direct epilogue is refused and the row epilogue's strided loads and stores run
    for hw in ((5, 7), (16, 33)):
        t = f"{hw[0]}x{hw[1]}"
        L.append(conv_case(f"c3i_os2_co32_plain_{t}", cin=64, hw=hw, os=2, act=True))
        L.append(conv_case(f"c3i_os2_co32_mz_{t}", cin=64, hw=hw, os=2, bias=False, mz=True, mslope=0.0))
        L.append(conv_case(f"c3i_os2_co32_mz_r1_{t}", cin=64, hw=hw, os=2, bias=False, mz=True, mslope=0.0, r1="y", beta1=1.0))
        L.append(conv_case(f"c3i_os2_co32_mz_r1_scalar_{t}", cin=64, hw=hw, os=2, bias=False, mz=True, r1="y", beta1=1.0, y_coff=1, y_cs=35))
        L.append(conv_case(f"c3i_os2_co64_plain_{t}", cin=64, cout=64, hw=hw, os=2, act=True))
        L.append(conv_case(f"c3i_os2_co64_r1_{t}", cin=64, cout=64, hw=hw, os=2, r1="own", alpha=0.5))
        L.append(conv_case(f"c3i_os2_co72_mz_r1_{t}", cin=64, cout=72, hw=hw, os=2, bias=False, mz=True, mslope=0.0, r1="y", beta1=1.0))
        L.append(conv_case(f"c3i_os2_co72_mz_r1_scalar_{t}", cin=64, cout=72, hw=hw, os=2, bias=False, mz=True, r1="y", beta1=1.0, y_coff=1, y_cs=75))
    L.append(conv_case("c3i_os2_p11_co32", cin=64, hw=(16, 33), os=2, oa=1, ob=1, mz=True, r1="y", beta1=1.0))
    L.append(conv_case("c3b_os2_co32_mz_r1", cin=96, hw=(16, 33), os=2, blocked=True, bias=False, mz=True, mslope=0.0, r1="y", beta1=1.0))
    # -- the self-loading kernel (launch_dma), one case per reason it is taken
    L.append(conv_case("c3dma_pad0", cin=64, pad=(0, 0), hw=(18, 35), act=True))
    L.append(conv_case("c3dma_pad2", cin=64, cout=64, pad=(2, 2), hw=(5, 7), mz=True))
    L.append(conv_case("c3dma_cin48", cin=48, hw=(16, 33), act=True, dts=B16))
    L.append(conv_case("c3dma_cin24", cin=24, hw=(16, 33), act=True, dts=("fp32",)))
    L.append(conv_case("c3dma_cin48_co96", cin=48, cout=96, hw=(35, 70), r1="own", dts=B16))
    L.append(conv_case("c3dma_cin24_co96", cin=24, cout=96, hw=(35, 70), r1="own", dts=("fp32",)))
    L.append(conv_case("c3dma_xcoff_in_plane", cin=64, x_coff=8, x_cs=96, blocked=True, hw=(16, 33), mz=True))
    return L


def _generic_cases():
    """every (kh, kw, stride) of dispatch_shape at Cout <= 32 and > 32, with the padding its caller uses; shapes from the launcher's
    tile (32 columns x 8 rows, 4 rows for the PT = 1 forms): below one tile, and one pixel more than a whole number of tiles"""
    L = []
    acc = itertools.cycle([dict(y_cs=None), dict(y_coff=4, y_cs=None), dict(y_coff=1, y_cs="odd")])       # 16-byte, 4-wide only, scalar

    def add(tag, k, s, pad, cin, hw, **kw):
        for cout in (32, 72):
            a = dict(next(acc))
            yc = a.get("y_coff", 0)
            a["y_cs"] = (yc + cout + 2) if a["y_cs"] == "odd" else (yc + cout + 4 if yc else None)
            L.append(conv_case(f"g{tag}_co{cout}", k=k, s=s, pad=pad, cin=cin, cout=cout, hw=hw, **dict(a, **kw)))

    add("1x1s1", (1, 1), 1, (0, 0), 64, (9, 33), act=True)
    add("1x1s1_small", (1, 1), 1, (0, 0), 32, (3, 5), mz=True)
    add("2x2s2", (2, 2), 2, (0, 0), 64, (10, 66))                                        # dgrad of ConvTranspose2d(k2, s2): OH x OW = 5 x 33
    add("2x2s2_odd", (2, 2), 2, (0, 0), 32, (7, 9), OHW=(3, 4), r1="own")
    for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):                                         # parity classes of the 4x4 s2 p1 input gradient
        H, W = (17, 67) if a == b else (16, 66)
        add(f"2x2s1_p{a}{b}", (2, 2), 1, (1 - a, 1 - b), 64, ((H - 2) // 2 + 1, (W - 2) // 2 + 1), OHW=((H - a + 1) // 2, (W - b + 1) // 2), os=2, oa=a, ob=b,
            bias=False, mz=bool(a))
    for a, b in ((0, 1), (1, 0)):                                                         # parity classes of the 3x3 s2 p1 input gradient (1x2, 2x1 taps)
        H, W = 17, 67
        add(f"{1 + a}x{1 + b}s1_p{a}{b}", (1 + a, 1 + b), 1, (0, 0), 64, ((H - 1) // 2 + 1, (W - 1) // 2 + 1), OHW=((H - a + 1) // 2, (W - b + 1) // 2), os=2, oa=a, ob=b,
            bias=False)
    add("4x4s2", (4, 4), 2, (1, 1), 64, (11, 67), act=True)
    add("4x4s2_small", (4, 4), 2, (1, 1), 8, (5, 6))
    add("4x4s1", (4, 4), 1, (1, 1), 64, (10, 34))                                         # OH x OW = 9 x 33
    add("4x4s1_dgrad", (4, 4), 1, (2, 2), 32, (4, 6), bias=False)
    for a, b in ((0, 1), (1, 0)):                                                         # 7x7 s2 p3 input gradient: 3 or 4 taps per axis, lead 1
        add(f"{3 + a}x{3 + b}s1_p{a}{b}", (3 + a, 3 + b), 1, (1, 1), 64, (9, 34), OHW=(9, 33), os=2, oa=a, ob=b, bias=False)
    # parity (1, 1) of the 7x7 s2 p3 input gradient: 4 taps per axis, lead 1; with the caller's accumulate + ReLU' operands as well
    add("4x4s1_p11", (4, 4), 1, (1, 1), 64, (9, 34), OHW=(9, 33), os=2, oa=1, ob=1, bias=False)
    add("4x4s1_p11_mz_r1", (4, 4), 1, (1, 1), 32, (4, 6), OHW=(4, 5), os=2, oa=1, ob=1, bias=False, mz=True, mslope=0.0, r1="y", beta1=1.0)
    # 1x1 with a strided store: parity (0, 0) of the 3x3 s2 p1 input gradient and the stride-2 shortcut's gradient (accumulating), and
    # the four launches of ConvTranspose2d(k2, s2) in the op-list networks
    add("1x1s1_p00", (1, 1), 1, (0, 0), 64, (9, 33), os=2, bias=False)
    add("1x1s1_p00_mz_r1", (1, 1), 1, (0, 0), 64, (9, 33), os=2, bias=False, mz=True, mslope=0.0, r1="y", beta1=1.0)
    for a, b in ((0, 1), (1, 0), (1, 1)):
        add(f"1x1s1_p{a}{b}", (1, 1), 1, (0, 0), 64, (5, 33), os=2, oa=a, ob=b, bias=False)
    add("3x3s2", (3, 3), 2, (1, 1), 64, (9, 67), act=True)                                # OH x OW = 5 x 34
    add("3x3s2_even", (3, 3), 2, (1, 1), 32, (6, 8), r1="own")
    add("7x7s2", (7, 7), 2, (3, 3), 8, (9, 67))
    add("1x1s2", (1, 1), 2, (0, 0), 64, (17, 67))                                         # OH x OW = 9 x 34
    add("5x5s1", (5, 5), 1, (2, 2), 32, (9, 33), act=True)
    add("9x9s1", (9, 9), 1, (4, 4), 8, (9, 33))
    return L


def _par_cases():
    L = []
    for hw in ((5, 7), (9, 37)):
        L.append(par_case(f"up_general_{hw[0]}x{hw[1]}", "up1x1", cin=64, cout=32, hw=hw, act=True, bias=True))
        L.append(par_case(f"up_general64_{hw[0]}x{hw[1]}", "up1x1", cin=64, cout=64, hw=hw, act=True, y_cs=72))
        L.append(par_case(f"up_pair_{hw[0]}x{hw[1]}", "up1x1", cin=64, cout=64, hw=hw, act=True))
        L.append(par_case(f"up_general64_sign_{hw[0]}x{hw[1]}", "up1x1", cin=64, cout=64, hw=hw, act=True, y_cs=72, sign_out=True, dts=B16))
        L.append(par_case(f"up_pair_sign_{hw[0]}x{hw[1]}", "up1x1", cin=64, cout=64, hw=hw, act=True, sign_out=True, dts=B16))
    for hw, cin, cout, mz, r1 in (((16, 66), 64, 64, True, False), ((17, 67), 32, 128, True, True), ((7, 34), 40, 32, False, True), ((4, 5), 64, 32, False, False)):
        L.append(par_case(f"par4_{hw[0]}x{hw[1]}", "par4", cin=cin, cout=cout, hw=hw, mz=mz, r1=r1))
    for hw in ((1, 1), (5, 7), (4, 33)):
        L.append(par_case(f"deconv3_{hw[0]}x{hw[1]}", "deconv3", cin=64, cout=40, hw=hw, bias=True, act=True, slope=0.0))
    return L


def _wgrad_cases():
    L = []
    shapes = [((3, 3), 1, (1, 1), 32), ((2, 2), 2, (0, 0), 64), ((2, 2), 1, (1, 1), 32), ((4, 4), 2, (1, 1), 32), ((4, 4), 1, (1, 1), 32), ((3, 3), 2, (1, 1), 64),
              ((1, 1), 2, (0, 0), 64), ((1, 1), 1, (0, 0), 32), ((5, 5), 1, (2, 2), 32)]
    for k, s, pad, cin in shapes:                                 # every dispatch_wgrad shape at both row-tile heights (cot 32 / 64)
        for cout in (32, 72):
            hw = (9, 33) if s == 1 else (11, 67)                  # one pixel more than whole 8- (stride 1) or 4-row (stride 2) tiles of 32 columns
            L.append(wgrad_case(f"w{k[0]}x{k[1]}s{s}_co{cout}", k=k, s=s, pad=pad, cin=cin, cout=cout, hw=hw))
    L.append(wgrad_case("w9x9s1", k=(9, 9), s=1, pad=(4, 4), cin=3, cout=40, hw=(9, 33)))
    L.append(wgrad_case("w7x7s2", k=(7, 7), s=2, pad=(3, 3), cin=3, cout=40, hw=(11, 67)))
    # 3x3: split counts (one, one that does not divide the 2 x 2 x 2 = 8 tiles, one above them), accumulate, dyadic alpha, fused bias
    # gradient, sliced operands, a transposed layout, three image channels padded to 8
    for ns in (1, 3, 11):
        L.append(wgrad_case(f"w3x3_nsplit{ns}", cin=32, cout=32, hw=(9, 33), nsplit=ns, bias_grad=True))
    for cout in (32, 72):                                         # the stride-2 kernel carries the bias wave too
        L.append(wgrad_case(f"w3x3s2_bias_co{cout}", s=2, cin=64, cout=cout, hw=(11, 67), bias_grad=True, alpha=0.5))
    L.append(wgrad_case("w3x3_accumulate", cin=64, cout=72, hw=(5, 7), accumulate=True, alpha=0.25, bias_grad=True))
    L.append(wgrad_case("w3x3_sliced", cin=32, cout=32, hw=(9, 33), x_coff=8, x_cs=48, dy_coff=16, dy_cs=56, alpha=0.5))
    L.append(wgrad_case("w3x3_cin3", cin=3, cout=16, hw=(9, 33), nsplit=3))
    L.append(wgrad_case("w2x2s2_transposed", k=(2, 2), s=2, pad=(0, 0), cin=64, cout=64, hw=(10, 18), layout="transposed"))
    L.append(wgrad_case("w2x2s2_transposed_acc", k=(2, 2), s=2, pad=(0, 0), cin=32, cout=24, hw=(6, 10), layout="transposed", accumulate=True, alpha=0.5))
    # at most three output channels: the (tap, channel)-as-N kernels in 16 bits, and the conditions that turn them off
    L.append(wgrad_case("wc3", cin=64, cout=3, hw=(9, 33)))
    L.append(wgrad_case("wc3_co1_small", cin=32, cout=1, hw=(5, 7), nsplit=2))
    L.append(wgrad_case("wc3_off_bias", cin=64, cout=3, hw=(9, 33), bias_grad=True))
    L.append(wgrad_case("wc3_off_cin", cin=48, cout=3, hw=(9, 33)))
    L.append(wgrad_case("wc1", k=(4, 4), cin=64, cout=1, hw=(9, 33)))
    L.append(wgrad_case("wc1_off_cin", k=(4, 4), cin=16, cout=1, hw=(9, 33)))
    return L


def _dense_cases():
    L = []
    for nf, gc in ((64, 32), (16, 8)):
        for blocked in (False, True):
            for hw in ((8, 32), (9, 33)):                  # whole tiles (the `fast` kernels where they exist) and ragged ones
                L.append(dense_case(f"d{nf}_{gc}_{'b' if blocked else 'i'}_{hw[0]}x{hw[1]}", nf=nf, gc=gc, hw=hw, blocked=blocked))
    L.append(dense_case("d64_32_accumulate", hw=(8, 64), accumulate=True))
    L.append(dense_case("d64_32_no_grad", hw=(4, 32), no_grad=1, no_bias=3))
    L.append(dense_case("d16_8_no_grad_acc", nf=16, gc=8, hw=(5, 7), no_grad=0, no_bias=4, accumulate=True))
    # single-segment forms for the remaining row / column tile counts: (rows, Cin) -> MT = rows / 32, NT by Cin (16-bit)
    for rows, cin in ((32, 64), (32, 96), (32, 128), (64, 128), (96, 64), (128, 160)):
        for hw in ((8, 32), (5, 33)):
            L.append(dense_case(f"d1seg_{rows}_{cin}_{hw[0]}x{hw[1]}", hw=hw, segs=[(0, rows, cin, 1.0)]))
    return L


CONV_CASES = _conv3x3_cases() + _generic_cases()
PAR_CASES = _par_cases()
WGRAD_CASES = _wgrad_cases()
DENSE_CASES = _dense_cases()
# float64 part: one case per kernel family, the reference's constants (conv5 of RDB3: alpha 0.04, beta1 0.2, beta2 1; LeakyReLU 0.2)
REAL_CASES = [
    conv_case("r_conv3x3_ls", real=True, cin=192, cout=64, hw=(11, 34), B=1, alpha=0.04, r1="x", r1_cend=64, beta1=0.2, r2=True, beta2=1.0),
    conv_case("r_conv3x3_ls_dense", real=True, cin=128, cout=32, hw=(16, 33), blocked=True, y_in_x=True, x_cs=160, y_coff=128, act=True, slope=0.2),
    conv_case("r_conv3x3_ls_mask", real=True, cin=64, cout=32, hw=(16, 33), blocked=True, bias=False, mz=True, mslope=0.2),
    conv_case("r_conv3x3_dma", real=True, cin=64, cout=32, pad=(0, 0), hw=(18, 35), act=True, slope=0.2),
    conv_case("r_conv_igemm_4x4s2", real=True, k=(4, 4), s=2, pad=(1, 1), cin=64, cout=128, hw=(11, 67), act=True, slope=0.2),
    conv_case("r_conv_igemm_1x1", real=True, k=(1, 1), s=1, pad=(0, 0), cin=64, cout=32, hw=(9, 33), alpha=0.2, r1="own", beta1=1.0),
    par_case("r_up_pair", "up1x1", real=True, cin=64, cout=64, hw=(9, 37), act=True, slope=0.2),
    par_case("r_par4", "par4", real=True, cin=64, cout=128, hw=(17, 67), mz=True, mslope=0.2),
    par_case("r_deconv3", "deconv3", real=True, cin=64, cout=40, hw=(5, 33), bias=True, act=True, slope=0.0),
    wgrad_case("r_wgrad_3x3", real=True, cin=64, cout=32, hw=(9, 33), bias_grad=True, alpha=0.2),
    wgrad_case("r_wgrad_4x4s2", real=True, k=(4, 4), s=2, pad=(1, 1), cin=32, cout=72, hw=(11, 67)),
    wgrad_case("r_wgrad_c3", real=True, cin=64, cout=3, hw=(9, 33)),
    dense_case("r_dense", real=True, hw=(8, 32)),
    dense_case("r_dense_ragged", real=True, nf=16, gc=8, hw=(9, 33)),
]
ALL_EXACT = CONV_CASES + PAR_CASES + WGRAD_CASES + DENSE_CASES


def _params(cases):
    return [pytest.param(c, dt, id=f"{c['name']}-{dt}") for c in cases for dt in c["dts"]]


# --------------------------------------------------------------------------------------------- the classes the dispatch can reach
def _expected_classes():
    """Read off srcgan_conv_igemm's routing (conv_entry.hip), dispatch_dma / launch_ls_em / launch_ls (conv3x3_dma.hip), sg_conv_generic /
    dispatch_shape (conv_igemm.hip), sg_dgrad_s2k4 (conv_par4.hip), sg_deconv_k3s2 (deconv_k3s2.hip), srcgan_conv_wgrad / dispatch_wgrad (conv_wgrad.hip) and dispatch_wd / launch_wd
    (wgrad_dense.hip), default environment.  3x3 stride 1 always goes to conv3x3_dma.hip, so conv_igemm<.,3x3,s1,.> is not reachable."""
    E = set()
    for t in ("f32", "bf16", "f16"):
        h = t != "f32"
        # 3x3 stride 1, loader-specialised kernel.  Epilogue form: d16 / d8 = direct (16-bit, Cout == 32, sets 0 / 8 / 16), "" = row
        # epilogue (16-byte accessible), gen = per element (no sign masks)
        if h:
            for res in (",wres,s3", ",wres", ""):                      # Cin 64: three stages; resident weights (<= 4 chunks); streamed
                for em in (0, 4, 8, 16) + ((7,) if res != ",wres,s3" else ()):
                    dirs = {0: (",d16", ",d8", "", ",gen"), 8: (",d16", ",d8", ""), 16: (",d16", ",d8", "")}.get(em, ("", ",gen"))
                    E.update(f"conv3x3_ls<{t},MT1,W8+8{res},e{em}{d}>" for d in dirs)
            for em in (0, 1, 3, 4, 7):
                E.update(f"conv3x3_ls<{t},MT2,W8+4,e{em}{d}>" for d in ("", ",gen"))
            E.add(f"conv3x3_ls<{t},MT2,W8+4,e8>")
        else:
            E.update(f"conv3x3_ls<{t},MT{mt},W8+4,e7{d}>" for mt in (1, 2) for d in ("", ",gen"))
        E.update(f"conv3x3_dma<{t},MT{mt},W8+0,PT2>" for mt in (1, 2))
        for kh, kw, s in ((1, 1, 1), (2, 2, 2), (2, 2, 1), (1, 2, 1), (2, 1, 1), (4, 4, 2), (4, 4, 1), (3, 4, 1), (4, 3, 1), (3, 3, 2), (7, 7, 2), (1, 1, 2), (5, 5, 1),
                          (9, 9, 1)):
            E.update(f"conv_igemm<{t},{kh}x{kw},s{s},MT{mt}>" for mt in (1, 2))
        if h:
            E.add(f"conv_igemm<{t},1x1,s1,MT4>")                       # the up-sampler's pixel-pair form
        E.add(f"dgrad_s2k4<{t},4 parities>")
        E.add(f"deconv_k3s2<{t},4 parities>")
        for kh, kw, s in ((3, 3, 1), (2, 2, 2), (2, 2, 1), (4, 4, 2), (4, 4, 1), (3, 3, 2), (1, 1, 2), (1, 1, 1), (5, 5, 1)):
            E.update(f"conv_wgrad<{t},{kh}x{kw},s{s},MT{mt}>" for mt in (1, 2))
        E.update((f"conv_wgrad<{t},9x9,s1,MT1>", f"conv_wgrad<{t},7x7,s2,MT1>"))
        if h:
            E.update((f"conv_wgrad<{t},3x3,s1,c3>", f"conv_wgrad<{t},4x4,s1,c1>"))
        # dense block: MT = row tiles (1..4), NT = 2, or 3 / 4 in 16 bits with MT <= 2; `fast` (whole tiles) where its table fits
        for mt, nt in [(m, 2) for m in (1, 2, 3, 4)] + ([(m, n) for m in (1, 2) for n in (3, 4)] if h else []):
            E.add(f"wgrad_dense<{t},MT{mt},NT{nt}>")
            if h and (mt, nt) in ((3, 2), (4, 2), (2, 3), (2, 4)):
                E.add(f"wgrad_dense<{t},MT{mt},NT{nt},fast>")
    return E


EXPECTED_CLASSES = _expected_classes()
# reachable, and not run by a case here (DESIGN section 3.5 would give the reasons): none
NOT_COVERED = set()

SEEN = {}            # class -> the first case that ran it
RAN = set()


# --------------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _guarded_slabs(ops):
    """Every srcgan_conv_wgrad / srcgan_wgrad_dense call of this file gets a NaN-filled split-K slab between guards, checked after the
    call (tests/ws_guard.py): the slab's contents on entry are unspecified, like those of the networks' scratch."""
    with guarded_slabs(NAN, "cuda") as g:
        yield g


@pytest.fixture(scope="module")
def ncu(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count


_BUILT = collections.OrderedDict()


def built(c, dt, ncu=256):
    """References are computed once per case -- exact operands are the same numbers in every storage type, and the types of a case
    run back to back -- and only the most recent ones are kept."""
    key = (c["name"], dt if c["real"] else None, ncu if c.get("B") == CE.PERSISTENT else None)
    if key in _BUILT:
        _BUILT.move_to_end(key)
    else:
        fn = {"conv": CE.build_conv, "wgrad": CE.build_wgrad, "dense": CE.build_dense}.get(c["form"], CE.build_par)
        _BUILT[key] = fn(c, dt, ncu) if c["form"] == "conv" else fn(c, dt)
        while len(_BUILT) > 8:
            _BUILT.popitem(last=False)
    return _BUILT[key]


class Prof:
    """records the kernel classes launched inside the block"""
    def __init__(self, name, dt):
        self.key = f"{name}-{dt}"

    def __enter__(self):
        from srcgan_amd import _native as N
        N.prof_enable(True)
        N.prof_collect()
        return self

    def __exit__(self, et, ev, tb):
        from srcgan_amd import _native as N
        self.classes = [r["cls"] for r in N.prof_collect()]
        N.prof_enable(False)
        for k in self.classes:
            SEEN.setdefault(k, self.key)
        if et is None:
            RAN.add(self.key)
        print(f"[class] {self.key}: {', '.join(self.classes)}")
        return False


def put(ops, buf, T, blocked=False):
    t = buf.to(T).cuda()
    return ops.make_blocked(t) if blocked else (t, 0)


def back(ops, t, blocked, cs):
    return (ops.from_blocked(t, cs) if blocked else t).cpu()


def same(got, want64, what):
    """value equality of the whole tensor against the reference cast once (so +0 == -0)"""
    want = want64.to(got.dtype)
    if torch.equal(got, want):
        return
    d = got.double() != want.double()
    idx = d.nonzero()
    raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} elements differ; first at {idx[0].tolist()}: got {float(got[tuple(idx[0])])}, "
                         f"want {float(want[tuple(idx[0])])}; last at {idx[-1].tolist()}; max |diff| {float((got.double() - want.double())[d].abs().max())}")


def within(got, ref, N, K, dt, what, f32_out=False):
    """per-element bound against float64; prints the largest |got - ref| / N and the largest |got - ref| / bound before it asserts"""
    bound = CE.bound64(ref, N, K, dt, f32_out)
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    rel = float((err / N.clamp_min(1e-300)).max())
    print(f"[f64] {what}: K = {K}, max |out - ref| / N = {rel:.3g}, max |out - ref| / bound = {ratio:.3g}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements over the bound, worst ratio {ratio:.3g}"


# ------------------------------------------------------------------------------------------------------------------- the runners
def run_conv(ops, c, dt, b, exact=True):
    T = TDT[dt]
    B, H, W = b["B"], b["H"], b["W"]
    x, xpl = put(ops, b["x"], T, c["blocked"])
    if c["y_in_x"]:
        y, ypl, yblk = x, xpl, c["blocked"]
    else:
        yblk = c["y_blocked"]
        y, ypl = put(ops, b["y0"], T, yblk)
    wp = ops.pack_conv2d_fwd(b["w"].float().cuda(), T)
    kw = dict(kh=c["k"][0], kw=c["k"][1], stride=c["s"], Cin=c["cin"], x_coff=c["x_coff"], Cout=c["cout"], y_coff=c["y_coff"], OH=b["OH"], OW=b["OW"], pad=c["pad"],
              bias=b["bias"].float().cuda() if b["bias"] is not None else None, alpha=c["alpha"], act=c["act"], slope=c["slope"], mslope=c["mslope"],
              os=c["os"], oa=c["oa"], ob=c["ob"], x_plane=xpl, y_plane=ypl, rev_batch=c["rev"])
    if c["blocked"]:
        kw["shape"] = (B, H, W)
    keep = {}
    if c["r1"]:
        if c["r1"] == "y":
            r1, r1pl = y, ypl
        elif c["r1"] == "x":
            r1, r1pl = x, xpl
        else:
            r1, r1pl = put(ops, b["r1"], T, c["ep_blocked"])
            keep["r1"] = (r1, c["ep_blocked"], b["r1"])
        kw.update(r1=r1, r1_coff=b["r1_coff"], r1_cend=b["r1_cend"], beta1=c["beta1"], r1_plane=r1pl)
    if c["r2"]:
        r2, r2pl = put(ops, b["r2"], T, c["ep_blocked"])
        keep["r2"] = (r2, c["ep_blocked"], b["r2"])
        kw.update(r2=r2, r2_cend=b["r2_cend"], beta2=c["beta2"], r2_plane=r2pl)
    sign = None
    if c["sign_in"]:
        bits = b["ep"]["mz"] > 0
        sign = (CE.pack_sign32(bits) if c["cout"] == 32 else CE.pack_sign8(bits)).cuda()
        kw.update(sign_in=sign)
        keep_sign = sign.clone()
    elif c["mz"]:
        mz, mzpl = put(ops, b["mz"], T, c["ep_blocked"])
        keep["mz"] = (mz, c["ep_blocked"], b["mz"])
        kw.update(mz=mz, mz_coff=c["mz_coff"], mz_c0=c["mz_c0"], mz_plane=mzpl)
    if c["sign_out"]:
        sign = torch.zeros(B, b["OH"], b["OW"], dtype=torch.int32, device="cuda")
        kw.update(sign_out=sign)
    y_mz = None
    with Prof(c["name"], dt) as pr:
        ops.conv_igemm(x, wp, y, **kw)
        if c["sign_in"]:                 # the same operands through the mz form: the two outputs must have the same bits
            y_mz, _ = put(ops, b["y0"], T, yblk)
            mz, mzpl = put(ops, b["mz"], T, c["ep_blocked"])
            keep["mz"] = (mz, c["ep_blocked"], b["mz"])
            ops.conv_igemm(x, wp, y_mz, **dict(kw, sign_in=None, mz=mz, mz_coff=c["mz_coff"], mz_c0=0, mz_plane=mzpl))
        torch.cuda.synchronize()
    if y_mz is not None:
        iv = torch.int32 if T == torch.float32 else torch.int16
        assert torch.equal(y.view(iv), y_mz.view(iv)), "sign_in run != mz run of the same data"
    got = back(ops, y, yblk, b["y_cs"])
    if exact:
        same(got, b["want"], "y")
    if not c["y_in_x"]:
        same(back(ops, x, c["blocked"], b["x_cs"]), b["x"], "x after the call")
    for name, (t, blk, ref) in keep.items():
        same(back(ops, t, blk, ref.shape[-1]), ref, name + " after the call")
    if c["sign_out"]:
        assert torch.equal(CE.unpack_sign32(sign.cpu()), b["v"] > 0), "sign_out"
    if c["sign_in"]:
        assert torch.equal(sign, keep_sign), "sign_in after the call"
    return got


def _par_packs(ops, c, b, T):
    w = b["w"].float().cuda()
    cin, cout = c["cin"], c["cout"]
    if c["form"] == "up1x1":
        packs = [ops.pack_weight(w, cout, cin, 1, 1, 4, cout * 4, 0, 0, q, T) for q in range(4)]
    else:
        packs = [ops.pack_weight(w, cin, cout, 2, 2, 16, cin * 16, -8, -2, (2 if a else 3) * 4 + (2 if bb else 3), T) for a in (0, 1) for bb in (0, 1)]
    step = packs[0].numel() * packs[0].element_size()
    return torch.cat([p.reshape(-1).view(torch.uint8) for p in packs]), step


def run_par(ops, c, dt, b, exact=True):
    T = TDT[dt]
    B, (H, W) = c["B"], c["hw"]
    x, _ = put(ops, b["x"], T)
    y, _ = put(ops, b["y0"], T)
    bias = b["bias"].float().cuda() if b["bias"] is not None else None
    keep = {"x": (x, b["x"])}
    sign = None
    with Prof(c["name"], dt) as pr:
        if c["form"] == "deconv3":
            ops.deconv3x3s2(x, b["w"].float().cuda(), bias, relu=c["act"], y=y)
        else:
            wall, step = _par_packs(ops, c, b, T)
            kw = dict(alpha=c["alpha"], act=c["act"], slope=c["slope"], mslope=c["mslope"], os=2, npar=4, wpar_stride=step, bias=bias)
            if c["r1"]:
                r1, _ = put(ops, b["r1"], T)
                keep["r1"] = (r1, b["r1"])
                kw.update(r1=r1, r1_cend=b["Cy"], beta1=c["beta1"])
            if c["mz"]:
                mz, _ = put(ops, b["mz"], T)
                keep["mz"] = (mz, b["mz"])
                kw.update(mz=mz, mz_c0=0)
            if c["sign_out"]:
                sign = torch.zeros(B, b["YH"], b["YW"], 8, dtype=torch.uint8, device="cuda")
                kw.update(sign_out=sign)
            if c["form"] == "up1x1":
                ops.conv_igemm(x, wall, y, kh=1, kw=1, Cout=c["cout"], OH=H, OW=W, **kw)
            else:
                ops.conv_igemm(x, wall, y, kh=2, kw=2, Cout=c["cin"], OH=(H + 1) // 2, OW=(W + 1) // 2, **kw)
        torch.cuda.synchronize()
    got = y.cpu()
    if exact:
        same(got, b["want"], "y")
    if exact and c["form"] == "deconv3" and c["slope"] == 0.0:
        # a negative value times the zero slope is -0.0 by the header's formula: the sign of zero is part of the result
        want = b["want"].to(T)
        iv = torch.int32 if T == torch.float32 else torch.int16
        assert torch.equal(got.view(iv), want.view(iv)), "sign of zero behind ReLU"
    for name, (t, ref) in keep.items():
        same(t.cpu(), ref, name + " after the call")
    if c["sign_out"]:
        assert torch.equal(CE.unpack_sign8(sign.cpu()), b["v"] > 0), "sign_out"
    return got


def run_wgrad(ops, c, dt, b):
    T = TDT[dt]
    x, _ = put(ops, b["x"], T)
    dy, _ = put(ops, b["dy"], T)
    grad = b["grad0"].float().cuda()
    gb = b["bias0"].float().cuda() if c["bias_grad"] else None
    with Prof(c["name"], dt) as pr:
        ops.conv_wgrad(dy, x, grad, kh=c["k"][0], kw=c["k"][1], stride=c["s"], Cout=c["cout"], Cin=c["cin"], dy_coff=c["dy_coff"], x_coff=c["x_coff"], pad=c["pad"],
                       layout=b["layout"], alpha=c["alpha"], nsplit=c["nsplit"], accumulate=c["accumulate"], bias_grad=gb)
        torch.cuda.synchronize()
    same(x.cpu(), b["x"], "x after the call")
    same(dy.cpu(), b["dy"], "dy after the call")
    return pr.classes, grad.cpu(), (gb.cpu() if gb is not None else None)


def _wgrad_dense(dy, x, segs, G, Cc, dy_plane, x_plane, shape, accumulate):
    """ops.wgrad_dense with the descriptor's `accumulate` (the wrapper does not pass it)"""
    import ctypes as C
    from srcgan_amd import _native as N
    lib, d = N.lib(), N.WgradDenseDesc()
    B, H, W = shape
    dt = N.dtype_id(x.dtype)
    slab = torch.empty(lib.srcgan_wgrad_dense_slab_bytes(G, Cc, dt, B, H, W), dtype=torch.uint8, device=x.device)
    d.dy, d.x, d.slab, d.dtype = dy.data_ptr(), x.data_ptr(), slab.data_ptr(), dt
    d.B, d.H, d.W, d.G, d.dy_cs, d.dy_coff, d.C, d.x_cs, d.x_coff = B, H, W, G, dy.shape[-1], 0, Cc, x.shape[-1], 0
    d.dy_plane, d.x_plane, d.accumulate = dy_plane, x_plane, int(accumulate)
    d.nseg = len(segs)
    for i, (g0, g1, grad, bias, cin, alpha) in enumerate(segs):
        d.seg[i].g0, d.seg[i].g1, d.seg[i].Cin, d.seg[i].alpha = g0, g1, cin, alpha
        d.seg[i].grad = grad.data_ptr() if grad is not None else None
        d.seg[i].bias = bias.data_ptr() if bias is not None else None
    N.check(lib.srcgan_wgrad_dense(C.byref(d), N.stream_ptr(x.device)), "srcgan_wgrad_dense")


def run_dense(ops, c, dt, b):
    T = TDT[dt]
    A, apl = put(ops, b["A"], T, c["blocked"])
    Gd, gpl = put(ops, b["Gd"], T, c["blocked"])
    segs, outs = [], []
    for s in b["segs"]:
        gw = s["w0"].float().cuda() if s["w0"] is not None else None
        gb = s["b0"].float().cuda() if s["b0"] is not None else None
        segs.append((s["g0"], s["g1"], gw, gb, s["cin"], s["alpha"]))
        outs.append((gw, gb))
    with Prof(c["name"], dt) as pr:
        _wgrad_dense(Gd, A, segs, b["G"], b["C"], gpl, apl, (c["B"],) + tuple(c["hw"]), c["accumulate"])
        torch.cuda.synchronize()
    same(back(ops, A, c["blocked"], b["C"]), b["A"], "x after the call")
    same(back(ops, Gd, c["blocked"], b["G"]), b["Gd"], "dy after the call")
    return pr.classes, [(w.cpu() if w is not None else None, g.cpu() if g is not None else None) for w, g in outs]


def exact_conditions(c, dt, b):
    """the generator's conditions for one case and type (also run for the whole table on the CPU by the teeth file)"""
    if c["form"] in ("conv", "up1x1", "par4", "deconv3"):
        CE.check_exact(c["name"], dt, b["bound"], b["pre"], b["v"], b["ep"]["alpha"])
    elif c["form"] == "wgrad":
        CE.check_exact(c["name"], dt, b["bound"] + 8, b["val"], b["want"], CE.F32(c["alpha"]), f32_out=True)
    else:
        for s in b["segs"]:
            for want, n in ((s["w_want"], s["w_N"]), (s["b_want"], s["b_N"])):
                if want is not None:
                    CE.check_exact(c["name"], dt, n / s["alpha"] + 8, want, want, s["alpha"], f32_out=True)


# ----------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("c,dt", _params(CONV_CASES))
def test_conv_exact(ops, ncu, c, dt):
    b = built(c, dt, ncu)
    exact_conditions(c, dt, b)
    run_conv(ops, c, dt, b)


@pytest.mark.parametrize("c,dt", _params(PAR_CASES))
def test_four_parities_exact(ops, c, dt):
    b = built(c, dt)
    exact_conditions(c, dt, b)
    run_par(ops, c, dt, b)


@pytest.mark.parametrize("c,dt", _params(WGRAD_CASES))
def test_wgrad_exact(ops, c, dt, _guarded_slabs):
    b = built(c, dt)
    exact_conditions(c, dt, b)
    _, grad, gb = run_wgrad(ops, c, dt, b)
    assert _guarded_slabs.calls >= 1          # the call above ran on the guarded slab
    same(grad, b["want"], "grad")
    if gb is not None:
        same(gb, b["bias_want"], "bias_grad")


@pytest.mark.parametrize("c,dt", _params(DENSE_CASES))
def test_wgrad_dense_exact(ops, c, dt, _guarded_slabs):
    b = built(c, dt)
    exact_conditions(c, dt, b)
    _, outs = run_dense(ops, c, dt, b)
    assert _guarded_slabs.calls >= 1
    for s, (gw, gb) in zip(b["segs"], outs):
        if gw is not None:
            same(gw, s["w_want"], f"grad of rows [{s['g0']}, {s['g1']})")
        if gb is not None:
            same(gb, s["b_want"], f"bias gradient of rows [{s['g0']}, {s['g1']})")


@pytest.mark.parametrize("c,dt", _params(REAL_CASES))
def test_float64_bound(ops, c, dt):
    """Random reals, production constants: |out - ref64| <= eps_T |ref64| + (K + 8) 2^-23 N per element, no other allowance."""
    b = built(c, dt)
    tag = f"{c['name']}-{dt}"
    if c["form"] == "conv":
        want, got = b["want"], run_conv(ops, c, dt, b, exact=False)
        sl = (slice(None), slice(None), slice(None), slice(c["y_coff"], c["y_coff"] + c["cout"]))
        ref = want[sl].permute(0, 3, 1, 2)
        within(got[sl].permute(0, 3, 1, 2), ref, b["N"], b["K"], dt, tag)
    elif c["form"] == "wgrad":
        _, grad, gb = run_wgrad(ops, c, dt, b)
        ref = b["want"]
        N = torch.zeros_like(ref)
        N[b["off"]:b["off"] + b["N"].numel()] = (b["N"].permute(*b["perm"]) if b["perm"] else b["N"]).reshape(-1)
        within(grad, ref, N, b["K"], dt, tag, f32_out=True)
        if gb is not None:
            within(gb, b["bias_want"], b["bias_N"], b["K"], dt, tag + " bias", f32_out=True)
    elif c["form"] == "dense":
        _, outs = run_dense(ops, c, dt, b)
        for s, (gw, gb) in zip(b["segs"], outs):
            within(gw, s["w_want"], s["w_N"], b["K"], dt, f"{tag} rows {s['g0']}", f32_out=True)
            within(gb, s["b_want"], s["b_N"], b["K"], dt, f"{tag} rows {s['g0']} bias", f32_out=True)
    else:
        got = run_par(ops, c, dt, b, exact=False)
        ref = b["v"]
        within(got[..., :b["Cy"]].permute(0, 3, 1, 2), ref, b["N"], b["K"], dt, tag)


def test_every_reachable_class_ran():
    """Classes seen == EXPECTED_CLASSES minus the documented NOT_COVERED.  A class outside EXPECTED_CLASSES means the dispatch has
    changed: extend the list and give the new instance a case."""
    total = {f"{c['name']}-{dt}" for c in ALL_EXACT + REAL_CASES for dt in c["dts"]}
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert RAN == total, f"{len(total - RAN)} cases did not run (a partial selection, or failures): the coverage of a partial run says nothing"
    seen = set(SEEN)
    for k in sorted(seen):
        print(f"[seen] {k}  <- {SEEN[k]}")
    assert not (seen - EXPECTED_CLASSES), f"classes outside EXPECTED_CLASSES: {sorted(seen - EXPECTED_CLASSES)}"
    assert not (NOT_COVERED - EXPECTED_CLASSES), sorted(NOT_COVERED - EXPECTED_CLASSES)
    missing = EXPECTED_CLASSES - NOT_COVERED - seen
    assert not missing, f"reachable classes no case ran: {sorted(missing)}"
    stale = NOT_COVERED & seen
    assert not stale, f"listed as not covered, but run: {sorted(stale)}"
