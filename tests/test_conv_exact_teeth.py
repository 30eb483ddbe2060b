"""The exact comparisons of tests/test_gpu_conv_exact.py have teeth, and its case table is sound -- both shown on the CPU.

Teeth: each exact reference of tests/conv_exact.py is compared, by the comparison the GPU tests use (the reference cast once to the
storage type, `torch.equal`), with a copy of itself that makes ONE of the mistakes those tests are there to catch.  Every such
comparison must fail, in every storage type.  Table: the generator's conditions (check_exact) hold for every case and type of the
GPU table, so a case that would make bit equality the wrong assertion is caught without a GPU.  No kernel runs here."""
import pytest
import torch

import conv_exact as CE
import test_gpu_conv_exact as G

DTS = CE.DTS


def _differs(a64, b64, dts=DTS):
    """the GPU tests' comparison fails in every storage type"""
    return all(not torch.equal(a64.to(CE.TDT[dt]), b64.to(CE.TDT[dt])) for dt in dts)


def _case(name):
    return next(c for c in G.ALL_EXACT if c["name"] == name)


def _want_from(b, conv=None, **ep_over):
    """the case's expected y buffer, from a (possibly damaged) convolution result and epilogue"""
    c = b["case"]
    ep = dict(b["ep"], **ep_over)
    _, v, _ = CE.epilogue(b["conv"] if conv is None else conv, **ep)
    want = b["y0"].clone()
    want[:, c["oa"]::c["os"], c["ob"]::c["os"]][:, :b["OH"], :b["OW"]][..., c["y_coff"]:c["y_coff"] + c["cout"]] = v.permute(0, 2, 3, 1)
    return want, v


def _nonzero_term(b, bi, oy, ox):
    """(co, ci, ky, kx, value) of a non-zero product x w contributing to output pixel (bi, oy, ox) of a 3x3 s1 p1 case"""
    c = b["case"]
    x = CE.nchw(b["x"], c["x_coff"], c["cin"])
    for co in range(c["cout"]):
        for ci in range(c["cin"]):
            for ky in range(3):
                for kx in range(3):
                    iy, ix = oy + ky - 1, ox + kx - 1
                    if 0 <= iy < b["H"] and 0 <= ix < b["W"] and b["w"][co, ci, ky, kx] != 0 and x[bi, ci, iy, ix] != 0:
                        return co, ci, ky, kx, float(b["w"][co, ci, ky, kx] * x[bi, ci, iy, ix])
    raise AssertionError("no non-zero term at this pixel")


@pytest.mark.parametrize("name", ["c3i_cin64_d16", "c3b_cin128_e7", "c3i_co96_e3", "c3b_cin160_e4"])
def test_one_dropped_term_at_a_tile_seam_is_noticed(name):
    b = G.built(_case(name), "fp32")
    oy, ox = min(15, b["OH"] - 1), min(32, b["OW"] - 1)         # last row of the first tile row, first column of the second tile column
    co, ci, ky, kx, term = _nonzero_term(b, 1, oy, ox)
    conv = b["conv"].clone()
    conv[1, co, oy, ox] -= term
    bad, _ = _want_from(b, conv)
    good, _ = _want_from(b)
    assert torch.equal(good, b["want"])
    assert _differs(b["want"], bad, b["case"]["dts"])
    assert int((b["want"] != bad).sum()) == 1


@pytest.mark.parametrize("name,kce", [("c3dma_cin48", 32), ("c3dma_cin24", 16), ("c3dma_cin48_co96", 32)])
def test_dropped_partial_k_chunk_is_noticed(name, kce):
    b = G.built(_case(name), "fp32")
    c = b["case"]
    whole = (c["cin"] // kce) * kce
    x = CE.nchw(b["x"], c["x_coff"], c["cin"])
    conv = CE.conv_ref(x[:, :whole], b["w"][:, :whole], c["s"], c["pad"], b["OH"], b["OW"])
    assert _differs(b["want"], _want_from(b, conv)[0])


def test_channel_offset_shifted_by_4_is_noticed():
    b = G.built(_case("c3dma_xcoff_in_plane"), "fp32")
    c = b["case"]
    conv = CE.conv_ref(CE.nchw(b["x"], c["x_coff"] + 4, c["cin"]), b["w"], c["s"], c["pad"], b["OH"], b["OW"])        # input slice
    assert _differs(b["want"], _want_from(b, conv)[0])
    b = G.built(_case("c3b_cin96_e4"), "fp32")                                                                          # mask slice
    c = b["case"]
    mz = CE.nchw(b["mz"], c["mz_coff"] - 4, c["cout"])
    assert _differs(b["want"], _want_from(b, mz=mz)[0])
    b = G.built(_case("c3i_cin64_co16"), "fp32")                                                                        # output slice
    c = b["case"]
    bad = b["y0"].clone()
    bad[:, :b["OH"], :b["OW"], c["y_coff"] + 4:c["y_coff"] + 4 + c["cout"]] = b["v"].permute(0, 2, 3, 1)
    assert _differs(b["want"], bad)
    w = G.built(_case("w3x3_sliced"), "fp32")                                                                           # weight gradient operands
    c = w["case"]
    for dx, ddy in ((4, 0), (0, 4)):
        g = c["alpha"] * CE.wgrad_ref(CE.nchw(w["x"], c["x_coff"] + dx, c["cin"]), CE.nchw(w["dy"], c["dy_coff"] + ddy, c["cout"]), c["cout"], c["cin"], c["k"], c["s"], c["pad"])
        assert not torch.equal(g.float(), w["val"].float())


@pytest.mark.parametrize("name", ["par4_16x66", "up_pair_5x7", "up_general_5x7", "deconv3_5x7"])
def test_two_swapped_parities_are_noticed(name):
    b = G.built(_case(name), "fp32")
    for p, q in (((0, 1), (1, 0)), ((0, 0), (1, 1)), ((0, 0), (0, 1))):
        assert _differs(b["want"], CE.swap_parities(b["want"], p, q))


@pytest.mark.parametrize("name", ["c3i_cin128_d16", "c3b_cin96_e16", "g4x4s2_co72", "par4_17x67"])
def test_seam_column_taken_from_its_neighbour_is_noticed(name):
    b = G.built(_case(name), "fp32")
    c = b["case"]
    bad = b["want"].clone()
    col = 64 if c["form"] == "par4" else 32                       # par4: tiles of 32 columns PER PARITY
    assert bad.shape[2] > col
    bad[:, :, col] = b["want"][:, :, col - 1]
    assert _differs(b["want"], bad)


def test_ge_for_gt_is_noticed():
    # LeakyReLU' mask: mz == 0 takes mslope
    for name in ("c3b_cin64_e4", "c3i_co64_e4", "par4_16x66", "c3i_dgrad_accumulate"):
        b = G.built(_case(name), "fp32")
        assert int((b["ep"]["mz"] == 0).sum()) > 0
        bad = _want_from(b, gt_mz=torch.ge)[0] if b["case"]["form"] == "conv" else None
        if bad is None:
            _, v, _ = CE.epilogue(b["conv"], **dict(b["ep"], gt_mz=torch.ge))
            bad = b["want"].clone()
            bad[..., :b["Cy"]] = v.permute(0, 2, 3, 1)
        assert _differs(b["want"], bad)
    # sign bits, written (bit = v > 0) and read (bit = mz > 0): the packed words differ
    for name in ("c3b_cin64_e16", "c3b_cin192_e16", "up_pair_sign_5x7"):
        b = G.built(_case(name), "fp32")
        assert int((b["v"] == 0).sum()) > 0, name
        pack = CE.pack_sign32 if b["v"].shape[1] == 32 else CE.pack_sign8
        assert not torch.equal(pack(b["v"] > 0), pack(b["v"] >= 0))
    b = G.built(_case("c3b_cin64_e8"), "fp32")
    assert not torch.equal(CE.pack_sign32(b["ep"]["mz"] > 0), CE.pack_sign32(b["ep"]["mz"] >= 0))
    # the activation: v == 0 maps to 0 under either comparison, so y cannot tell them apart; the decision is
    # visible in the sign mask written beside y, and the pair (y, mask) differs
    b = G.built(_case("c3b_cin64_e16"), "fp32")
    same_y, v_ge = _want_from(b, gt_act=torch.ge)
    assert torch.equal(same_y, b["want"])
    assert not torch.equal(CE.pack_sign32(v_ge >= 0), CE.pack_sign32(b["v"] > 0))


@pytest.mark.parametrize("name", ["w3x3s1_co32", "w4x4s2_co72", "wc3", "w2x2s2_transposed", "w3x3_accumulate"])
def test_weight_gradient_reference_notices(name):
    b = G.built(_case(name), "fp32")
    c = b["case"]
    x, dy = CE.nchw(b["x"], c["x_coff"], c["cin"]), CE.nchw(b["dy"], c["dy_coff"], c["cout"])
    ref = lambda xx, dd: CE.F32(c["alpha"]) * CE.wgrad_ref(xx, dd, c["cout"], c["cin"], c["k"], c["s"], c["pad"])
    lay = lambda g: g.permute(*b["perm"]) if b["perm"] else g
    full = ref(x, dy)
    assert torch.equal(lay(full), b["val"])
    # one pixel left out of the sum
    oy, ox = b["OH"] - 1, min(32, b["OW"] - 1)
    assert float(dy[1, :, oy, ox].abs().sum()) > 0
    d2 = dy.clone()
    d2[1, :, oy, ox] = 0
    assert not torch.equal(ref(x, d2).float(), full.float())
    # two split-K slabs (the two images), one of them added twice
    slab = [ref(x[i:i + 1], dy[i:i + 1]) for i in range(2)]
    assert torch.equal(slab[0] + slab[1], full)
    assert not torch.equal((slab[0] + 2 * slab[1]).float(), full.float())


def test_dense_block_reference_notices():
    b = G.built(_case("d16_8_i_9x33"), "fp32")
    A, Gd = b["A"], b["Gd"]
    s = b["segs"][1]                          # conv4: rows [16, 24), 40 input channels
    dy, x = CE.nchw(Gd, s["g0"], s["g1"] - s["g0"]), CE.nchw(A, 0, s["cin"])
    full = s["alpha"] * CE.wgrad_ref(x, dy, s["g1"] - s["g0"], s["cin"], (3, 3), 1, (1, 1))
    assert torch.equal(full, s["w_want"])
    d2 = dy.clone()
    d2[0, :, 8, 32] = 0                       # the pixel behind the tile seams
    assert not torch.equal(CE.wgrad_ref(x, d2, 8, s["cin"], (3, 3), 1, (1, 1)).float(), full.float())
    shifted = CE.wgrad_ref(x, CE.nchw(Gd, s["g0"] + 4, 8), 8, s["cin"], (3, 3), 1, (1, 1))
    assert not torch.equal(shifted.float(), full.float())


@pytest.mark.parametrize("c", G.ALL_EXACT, ids=lambda c: c["name"])
def test_case_table_meets_the_generators_conditions(c):
    """for every case and storage type of the GPU table; a case that breaks a condition is an error in the table"""
    b = G.built(c, "fp32")
    for dt in c["dts"]:
        G.exact_conditions(c, dt, b)


def test_thresholds_are_exercised():
    """the share of outputs that are exactly zero, over the convolution cases of the table (small cases are already built)"""
    zeros = total = 0
    for c in G.CONV_CASES + G.PAR_CASES:
        if c.get("B") == CE.PERSISTENT:
            continue
        v = G.built(c, "fp32")["v"]
        zeros += int((v == 0).sum())
        total += v.numel()
    assert zeros > 1000 and zeros / total > 0.01, (zeros, total)


def test_expected_class_list_is_consistent():
    assert G.NOT_COVERED <= G.EXPECTED_CLASSES
    names = [c["name"] for c in G.ALL_EXACT + G.REAL_CASES]
    assert len(names) == len(set(names))
