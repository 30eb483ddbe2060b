"""The case table of tests/test_gpu_large_extent.py is sound and its references have teeth -- shown on the CPU, with the counter-based
generator of tests/large_extent.py evaluated at probe indices only.  For every case:
  * the geometry assertions hold (exactly the claimed multiples of 2^31 bytes, each strictly inside a row, by the smallest extent);
  * every claimed boundary has window pixels on both sides;
  * a kernel model that reads an operand at offset mod 2^32, at offset mod 2^31, or at the sign-extended low 32 bits changes the
    float64 reference of at least one window (for the output: a store that wraps leaves the initial value, which differs);
  * the sparse dy support reaches every image and both sides of every claimed boundary, and the bound stays below 2^24.
These are conditions on the reference alone; a case that breaks one is a mistake in the table.  No kernel runs here."""
import pytest
import torch

import large_extent as LE

CONV = [c for c in LE.CONV_CASES if not c["refuse"]]
IDS = lambda c: c["name"]


def test_generator_is_a_pure_function_of_name_and_index():
    idx = torch.tensor([0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) + 5, (1 << 33) + 7, -3])
    for kind in (LE.TERN, LE.INT4, LE.BYTE):
        a = LE.values("a", kind, idx)
        assert torch.equal(a, torch.cat([LE.values("a", kind, idx[i:i + 1]) for i in range(len(idx))]))       # any list of indices
        assert not torch.equal(a, LE.values("b", kind, idx))
    # whole ranges: the GPU's chunked fill is the same function of a range (checked against the device in the GPU test)
    r = torch.arange(5000, 9000)
    t = LE.values("a", LE.TERN, r)
    assert set(t.tolist()) == {-1, 0, 1} and abs(float((t != 0).double().mean()) - 0.5) < 0.05
    i4 = LE.values("a", LE.INT4, r)
    assert int(i4.min()) == -4 and int(i4.max()) == 4
    # elements 2^31 and 2^32 bytes apart are independent: equal about as often as two draws of the class
    for d in (1 << 30, 1 << 31, 1 << 32):
        eq = float((LE.values("a", LE.INT4, r) == LE.values("a", LE.INT4, r + d)).double().mean())
        assert abs(eq - 1 / 9) < 0.03, (d, eq)


@pytest.mark.parametrize("c", LE.ALL_CASES, ids=IDS)
def test_geometry(c):
    LE.check_geometry(c)


@pytest.mark.parametrize("c", CONV, ids=IDS)
def test_every_boundary_has_window_pixels_on_both_sides(c):
    g = LE.geometry(c)
    wins = LE.windows(c, g)
    assert all(w[3] <= 24 and w[4] <= 80 for w in wins)
    for op in LE.OPERANDS:
        if op not in g:
            continue
        buf = g[op]
        for o in buf.boundaries():
            pl = buf.locate(o)[0]
            hit = False
            for w in wins:
                b, y0, y1, x0, x1 = LE.window_region(c, g, op, w)
                ys, xs = torch.arange(y0, y1).view(-1, 1), torch.arange(x0, x1).view(1, -1)
                off = (buf.elem((b * buf.H + ys) * buf.W + xs, pl * buf.kce if buf.blocked else 0)) * buf.esz
                hit |= bool((off + buf.rec <= o).any()) and bool((off >= o).any())
            assert hit, (c["name"], op, o)


@pytest.mark.parametrize("c", CONV, ids=IDS)
def test_a_wrapped_offset_changes_a_window(c):
    g = LE.geometry(c)
    w, bias = LE.weights(c)
    wins = LE.windows(c, g)
    good = [LE.window_want(c, g, win, LE.HashFetch(), w, bias) for win in wins]
    for op in ("x", "sign", "r1"):
        if op not in g or not g[op].boundaries() or (op == "sign" and not c["sign_in"]):
            continue
        buf = g[op]                 # what the kernel READS of it: a blocked x that holds y too ends behind the input channels' last plane
        top = -(-c["cin"] // buf.kce) * buf.plane if (op == "x" and buf.blocked) else buf.nbytes
        for tag, fn in LE.WRAPS.items():
            if top <= ((1 << 32) if tag == "mod 2^32" else (1 << 31)):
                continue                                            # (offsets below the modulus are their own residue)
            bad = [LE.window_want(c, g, win, LE.HashFetch({g[op].name: fn}), w, bias) for win in wins]
            assert any(not torch.equal(a["y"][1], b["y"][1]) for a, b in zip(good, bad)), (c["name"], op, tag)
    # the outputs: an element whose offset a wrapping store maps elsewhere keeps its initial value
    for op in ("y", "sign"):
        buf = g["x"] if (op == "y" and c["y_in_x"]) else g.get(op)
        if buf is None or not buf.boundaries() or (op == "sign" and not c["sign_out"]):
            continue
        for tag, fn in LE.WRAPS.items():
            if tag == "mod 2^32" and buf.boundaries()[-1] < (1 << 32):
                continue
            changed = False
            for win, a in zip(wins, good):
                (b, y0, y1, x0, x1), want = a[op]
                init = LE.HashFetch()(buf, b, y0, y1, x0, x1)
                ys, xs = torch.arange(y0, y1).view(-1, 1, 1), torch.arange(x0, x1).view(1, -1, 1)
                off = buf.elem((b * buf.H + ys) * buf.W + xs, torch.arange(buf.cs).view(1, 1, -1)) * buf.esz
                got = torch.where(fn(off) == off, want, init)
                changed |= not torch.equal(got, want)
            assert changed, (c["name"], op, tag)


@pytest.mark.parametrize("c", LE.WGRAD_CASES, ids=IDS)
def test_sparse_dy_support_and_bound(c):
    g = LE.geometry(c)
    sup = LE.dy_support(c, g)
    assert sup.numel() <= 1 << 20 and int(sup.min()) >= 0 and int(sup.max()) < g["B"] * g["OH"] * g["OW"]
    img = sup // (g["OH"] * g["OW"])
    assert set(img.tolist()) == set(range(g["B"]))
    D = LE.dy_values(g, sup)
    assert float(D.abs().sum(0).max()) + 8 < 2.0 ** 24
    assert all(bool((D[img == b] != 0).any()) for b in range(g["B"]))
    # both sides of every boundary of dy and of x: support pixels whose dy record / whose 3x3 (2x2) patch lies before and behind it
    pix, valid = LE.support_patches(c, g, sup)
    for op, offs in (("dy", g["dy"].elem(sup, 0) * g["dy"].esz), ("x", g["x"].elem(pix, 0) * g["x"].esz)):
        buf = g[op]
        for o in buf.boundaries():
            pl = buf.locate(o)[0]
            base = offs + (pl * buf.plane if buf.blocked else 0)
            near = (base - o).abs() < 64 * buf.rec
            assert bool((near & (base + buf.rec <= o)).any()) and bool((near & (base >= o)).any()), (c["name"], op, o)


@pytest.mark.parametrize("c", LE.WGRAD_CASES, ids=IDS)
def test_a_wrapped_offset_changes_the_weight_gradient(c):
    """on the clustered part of the support (the pixels within 64 records of a boundary, and the image edges): enough to move the sum"""
    g = LE.geometry(c)
    sup = LE.dy_support(c, g)
    keep = torch.zeros_like(sup, dtype=torch.bool)
    for op in ("x", "dy"):
        for o in g[op].boundaries():
            _, b, y, x, _ = g[op].locate(o)
            p = (b * g["OH"] + min(g["OH"] - 1, y // c["s"] if op == "x" else y)) * g["OW"] + (x // c["s"] if op == "x" else x)
            keep |= (sup - p).abs() <= 2 * LE.EDGE
    sup = sup[keep]
    assert sup.numel() >= 2 * LE.EDGE

    def ref(fetch):
        pix, valid = LE.support_patches(c, g, sup)
        X = fetch.at(g["x"], pix.unsqueeze(-1), torch.arange(g["x"].cs).view(1, 1, -1)) * valid.unsqueeze(-1)
        D = LE.dy_values(g, sup, fetch)
        out = LE.wgrad_want(c, g, X, D)
        return torch.cat([s[4].reshape(-1) for s in out]) if c["form"] == "dense" else out[0].reshape(-1)

    good = ref(LE.HashFetch())
    for op in ("x", "dy"):
        if not g[op].boundaries():
            continue
        for tag, fn in LE.WRAPS.items():
            if g[op].nbytes <= ((1 << 32) if tag == "mod 2^32" else (1 << 31)):
                continue                                            # (offsets below the modulus are their own residue)
            assert not torch.equal(good, ref(LE.HashFetch({g[op].name: fn}))), (c["name"], op, tag)


def test_case_names_are_unique_and_rows_complete():
    names = [c["name"] for c in LE.ALL_CASES]
    assert len(names) == len(set(names))
    for c in LE.ALL_CASES:
        assert c["claims"] is not None and (c["family"] or c["refuse"]), c["name"]
