"""Exact tests of the convolution, weight-gradient and glue kernels on tensors past 2 and 4 GiB, through the C ABI
with the launch profiler on.  Operands, geometry and references: tests/large_extent.py; what they notice: tests/test_large_extent_teeth.py.

Every comparison is `torch.equal`, or an exact refusal.  A forward / input-gradient case is checked three ways:
  * windows -- the corners of the first and last image, one rectangle straddling every multiple of 2^31 bytes inside every operand, one
    hashed rectangle per image -- against float64 arithmetic on patches copied from the device, cast once to the storage type;
  * the WHOLE output, on the GPU, against the same entry point run on pieces whose operands are each below 2^30 bytes (whole images, or
    row bands copied with their halo rows into fresh tensors): what tests/test_gpu_conv_exact.py pins to float64;
  * the inputs against the generator afterwards, the output's other channels and the elements behind every buffer against their sentinel.
The weight gradients and the column reduction run on a dy that is zero outside some 2^14 pixels, so their float64 reference is complete.
Peak device memory per test stays below 16 GiB (asserted); the last test holds the kernel classes seen against each row's family."""
import pytest
import torch

import large_extent as LE
from conv_exact import SENTINEL, TDT
from ws_guard import NAN, guarded_slabs

pytestmark = pytest.mark.gpu

GIB = 1 << 30
CAP = 16 * GIB
TAIL = 4096                        # sentinel elements behind every buffer
SEEN = {}                          # case -> classes
RAN = set()
ALL_IDS = [c["name"] for c in LE.ALL_CASES] + ["upsample2", "sum2x2", "add_inplace", "add_inplace_planes", "mask_inplace", "col_reduce", "nhwc_nchw"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _guarded_slabs(ops):
    with guarded_slabs(NAN, "cuda") as g:
        yield g


@pytest.fixture
def budget(ops, request):
    """skips only below 64 GiB of device memory; asserts the 16 GiB peak; frees everything between tests"""
    if torch.cuda.get_device_properties(0).total_memory < 64 * GIB:
        pytest.skip("needs a device with 64 GiB")
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a device fault is sticky: nothing that follows in this process could run, so end the session here
        pytest.exit(f"device error during {request.node.name}: {e}", returncode=3)
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    print(f"[peak] {request.node.name}: {peak / GIB:.2f} GiB")
    assert peak <= CAP, f"peak device memory {peak / GIB:.2f} GiB"


class Prof:
    def __init__(self, key):
        self.key = key

    def __enter__(self):
        from srcgan_amd import _native as N
        N.prof_enable(True)
        N.prof_collect()
        return self

    def __exit__(self, et, ev, tb):
        from srcgan_amd import _native as N
        self.classes = [r["cls"] for r in N.prof_collect()]
        N.prof_enable(False)
        SEEN.setdefault(self.key, []).extend(self.classes)
        print(f"[class] {self.key}: {', '.join(self.classes)}")
        return False


def sentinel_of(dtype):
    return 0xA5 if dtype == torch.uint8 else SENTINEL


def alloc(buf, fill=True):
    """a contiguous device tensor of buf.shape with TAIL sentinel elements behind it -> (tensor, tail)"""
    flat = torch.empty(buf.numel + TAIL, dtype=buf.tdt, device="cuda")
    flat[buf.numel:] = sentinel_of(buf.tdt)
    t = flat[:buf.numel].view(buf.shape)
    if fill:
        LE.fill(t, buf)
    return t, flat[buf.numel:]


def tail_ok(tail):
    return bool((tail == sentinel_of(tail.dtype)).all())


def unchanged(t, buf, lo=0, hi=None):
    """elements [lo, hi) of t's storage still hold the generator's values"""
    flat = t.view(-1)
    hi = buf.numel if hi is None else hi
    for s in range(lo, hi, LE.CHUNK):
        e = min(hi, s + LE.CHUNK)
        if not torch.equal(flat[s:e], LE.values(buf.name, buf.kind, torch.arange(s, e, device=t.device)).to(t.dtype)):
            return False
    return True


class GpuFetch:
    """large_extent's `fetch` on the device buffers: a patch, copied to the CPU"""

    def __init__(self, tensors):
        self.t = tensors

    def __call__(self, buf, b, y0, y1, x0, x1):
        t = self.t[buf.name]
        p = t[:, b, y0:y1, x0:x1].permute(1, 2, 0, 3).reshape(y1 - y0, x1 - x0, -1)[..., :buf.cs] if buf.blocked else t[b, y0:y1, x0:x1]
        return p.cpu().double()


# ----------------------------------------------------------------------------------------------------- forward and input gradient
def pack(ops, c, w, T):
    """-> (packed weights, extra keyword arguments)"""
    wd = w.float().cuda()
    if c["form"] == "up":
        packs = [ops.pack_weight(wd, c["cout"], c["cin"], 1, 1, 4, c["cout"] * 4, 0, 0, q, T) for q in range(4)]
        return torch.cat([p.reshape(-1).view(torch.uint8) for p in packs]), dict(os=2, npar=4, wpar_stride=packs[0].numel() * packs[0].element_size())
    return ops.pack_conv2d_fwd(wd, T), {}


def launch(ops, c, wp, extra, bias, x, y, sign, r1, B, H, W, OH, OW):
    """one srcgan_conv_igemm call of the case's form on [B, H, W] operands (the large call and the pieces alike); r1: "x", a blocked tensor, or None"""
    kw = dict(kh=c["k"][0], kw=c["k"][1], stride=c["s"], Cin=c["cin"], Cout=c["cout"], y_coff=c["y_coff"], OH=OH, OW=OW, pad=c["pad"], bias=bias, alpha=1.0,
              act=c["act"], slope=LE.SLOPE, mslope=LE.MSLOPE, **extra)
    if c["blocked"]:
        kw.update(shape=(B, H, W), x_plane=B * H * W * 64)
    if c["y_in_x"]:
        y = x
        kw.update(y_plane=kw.get("x_plane", 0))
    if c["sign_in"]:
        kw.update(sign_in=sign)
    if c["sign_out"]:
        kw.update(sign_out=sign)
    if r1 is not None:
        kw.update(r1=x if isinstance(r1, str) else r1, r1_cend=c["cout"], beta1=LE.BETA1, r1_plane=B * H * W * 64)
    ops.conv_igemm(x, wp, y, **kw)


def bands(c, g):
    """[(b, r0, r1)]: output rows (the up-sampler: input rows) whose operands are each below 2^30 bytes, halo rows included"""
    x = g["x"]
    per_row = [c["s"] * x.W * x.rec * x.npl]
    for op in ("y", "sign"):
        if op in g:
            per_row.append(g["os"] * g[op].W * g[op].rec)
    GH = g["H"] if c["form"] == "up" else g["OH"]
    most = (GIB - 1) // max(per_row) - 2
    nb = -(-GH // most)
    step = -(-GH // nb)
    return [(b, r0, min(GH, r0 + step)) for b in range(g["B"]) for r0 in range(0, GH, step)]


def check_piece(ops, c, g, wp, extra, bias, t, b, r0, r1):
    """the band's rows of the large output == the same entry on the band alone (input rows with their halo, fresh tensors)"""
    s, (kh, kw), pad, os_ = c["s"], c["k"], c["pad"], g["os"]
    H, W = g["H"], g["W"]
    i0, i1 = max(0, r0 * s - pad[0]), min(H, (r1 - 1) * s - pad[0] + kh)
    top = 1 if (pad[0] and r0 > 0) else 0                              # halo row of the band's own output, dropped
    X = t["x"]
    xp = (X[:, b:b + 1, i0:i1] if c["blocked"] else X[b:b + 1, i0:i1]).contiguous()
    h = i1 - i0
    oh = (h + 2 * pad[0] - kh) // s + 1
    n = r1 - r0
    assert oh >= top + n and xp.numel() * xp.element_size() < GIB
    yp = sp = None
    if c["y_in_x"]:
        pl = c["y_coff"] // g["x"].kce
        xp[pl:] = SENTINEL
    else:
        Y = t["y"]
        yp = torch.full((1, oh * os_, Y.shape[2], Y.shape[3]), SENTINEL, dtype=Y.dtype, device="cuda")
        assert yp.numel() * yp.element_size() < GIB
    if "sign" in t:
        S = t["sign"]
        if c["sign_in"]:                                               # the mask rows of the band's outputs; its halo outputs read zeros
            sp = torch.zeros((1, oh * os_) + tuple(S.shape[2:]), dtype=S.dtype, device="cuda")
            sp[0, top * os_:(top + n) * os_] = S[b, r0 * os_:r1 * os_]
        else:
            sp = torch.full((1, oh * os_) + tuple(S.shape[2:]), 0xA5, dtype=S.dtype, device="cuda")
    r1p = t["r1"][:, b:b + 1, i0:i1].contiguous() if "r1" in t else None
    launch(ops, c, wp, extra, bias, xp, yp, sp, r1p, 1, h, W, oh, g["OW"])
    rows = slice(top * os_, (top + n) * os_)
    big = slice(r0 * os_, r1 * os_)
    if c["y_in_x"]:
        ok = torch.equal(xp[:, 0, rows], X[:, b, big])
    else:
        ok = torch.equal(yp[0, rows], t["y"][b, big])
    if c["sign_out"]:
        ok = ok and torch.equal(sp[0, rows], t["sign"][b, big])
    assert ok, f"{c['name']}: image {b}, rows [{r0}, {r1}) of the large call differ from the same rows computed on their own"


@pytest.mark.parametrize("c", [c for c in LE.CONV_CASES if not c["refuse"]], ids=lambda c: c["name"])
def test_conv_large(ops, budget, c):
    g = LE.geometry(c)
    LE.check_geometry(c, g)
    T = TDT[c["dt"]]
    w, bias = LE.weights(c)
    wp, extra = pack(ops, c, w, T)
    bias_d = bias.float().cuda() if bias is not None else None
    t, tails = {}, {}
    for op in ("x", "y", "sign", "r1"):
        if op in g:
            t[op], tails[op] = alloc(g[op])
    fetch = GpuFetch({g[op].name: t[op] for op in t})
    wins = LE.windows(c, g)
    wants = [LE.window_want(c, g, win, fetch, w, bias) for win in wins]
    # the generator is the same function on both devices: the first boundary window, from the hash on the CPU
    probe = next((i for i, win in enumerate(wins) if " at " in win[5]), 0)
    assert torch.equal(wants[probe]["y"][1], LE.window_want(c, g, wins[probe], LE.HashFetch(), w, bias)["y"][1]), "device fill != CPU generator"
    with Prof(c["name"]):
        launch(ops, c, wp, extra, bias_d, t["x"], t.get("y"), t.get("sign"), t.get("r1"), g["B"], g["H"], g["W"], g["OH"], g["OW"])
        torch.cuda.synchronize()
    out = {"y": (g["x"], t["x"]) if c["y_in_x"] else (g["y"], t["y"])}
    if c["sign_out"]:
        out["sign"] = (g["sign"], t["sign"])
    got = GpuFetch({buf.name: ten for buf, ten in out.values()})
    for win, want in zip(wins, wants):
        for op, (region, ref) in want.items():
            have = got(out[op][0], *region)
            ref = ref.to(out[op][1].dtype).double()
            if not torch.equal(have, ref):
                d = (have != ref).nonzero()
                raise AssertionError(f"{c['name']} window {win}: {op} differs at {d.shape[0]} of {ref.numel()} elements, first (row, col, channel) {d[0].tolist()}: "
                                     f"got {float(have[tuple(d[0])])}, want {float(ref[tuple(d[0])])}; last {d[-1].tolist()}")
    for b, r0, r1 in bands(c, g):
        check_piece(ops, c, g, wp, extra, bias_d, t, b, r0, r1)
    # inputs, sentinel channels, and the elements behind every buffer
    xin = g["x"]
    assert unchanged(t["x"], xin, 0, (c["y_coff"] // xin.kce) * xin.npix * xin.kce if c["y_in_x"] else None), "x after the call"
    if c["sign_in"]:
        assert unchanged(t["sign"], g["sign"]), "sign_in after the call"
    if "r1" in t:
        assert unchanged(t["r1"], g["r1"]), "r1 after the call"
    if "y" in t and g["y"].cs > c["y_coff"] + c["cout"]:
        assert bool((t["y"][..., c["y_coff"] + c["cout"]:] == SENTINEL).all()), "channels behind the output slice"
    assert all(tail_ok(v) for v in tails.values()), "elements behind a buffer"
    RAN.add(c["name"])


def test_blocked_residual_plane_of_2_gib_is_refused(ops, budget):
    """the 64-channel tile with r1 in planes of 2^31 bytes or more: the entry returns its error and launches nothing"""
    c = LE.case("le_c3b_co64_r1_refused")
    g = LE.geometry(c)
    LE.check_geometry(c, g)
    assert g["x"].plane >= (1 << 31) - (1 << 20)
    w, bias = LE.weights(c)
    wp, extra = pack(ops, c, w, torch.bfloat16)
    x, xtail = alloc(g["x"], fill=False)
    y, ytail = alloc(g["y"])
    with Prof(c["name"]) as pr:
        with pytest.raises(RuntimeError, match=c["refuse"]):
            launch(ops, c, wp, extra, bias.float().cuda(), x, y, None, "x", g["B"], g["H"], g["W"], g["OH"], g["OW"])
        torch.cuda.synchronize()
    assert pr.classes == [], pr.classes
    assert bool((y == SENTINEL).all()) and tail_ok(ytail) and tail_ok(xtail)
    RAN.add(c["name"])


# ------------------------------------------------------------------------------------------------------------------ weight gradients
def sparse_dy(c, g):
    """-> (dy tensor, its tail, support on the device, D float64 [n, cs] on the CPU): dy is zero outside the support"""
    buf = g["dy"]
    flat = torch.zeros(buf.numel + TAIL, dtype=buf.tdt, device="cuda")
    flat[buf.numel:] = SENTINEL
    sup = LE.dy_support(c, g).cuda()
    ch = torch.arange(buf.cs, device="cuda")
    idx = buf.elem(sup.view(-1, 1), ch.view(1, -1))
    D = LE.values(buf.name, buf.kind, idx)
    if c["form"] == "wgrad":
        D = D * (ch < c["cout"])                                       # the padding behind Cout is the tensor's own, and zero
    flat[idx] = D.to(buf.tdt)
    Dc = D.cpu().double()
    probe = torch.arange(0, sup.numel(), 97)
    ref = LE.dy_values(g, sup.cpu()[probe])
    if c["form"] == "wgrad":
        ref = ref * (torch.arange(buf.cs) < c["cout"])
    assert torch.equal(Dc[probe], ref), "device values != CPU generator"
    return flat[:buf.numel].view(buf.shape), flat[buf.numel:], sup, Dc


def dy_intact(dy, g, sup, D):
    """dy still holds D on its support and zeros elsewhere (counted in pieces: no temporary of the tensor's size)"""
    buf, flat = g["dy"], dy.view(-1)
    idx = buf.elem(sup.view(-1, 1), torch.arange(buf.cs, device="cuda").view(1, -1))
    nz = sum(int(torch.count_nonzero(flat[s:s + (1 << 28)])) for s in range(0, buf.numel, 1 << 28))
    return torch.equal(flat[idx].cpu().double(), D) and nz == int((D != 0).sum())


def gather_x(c, g, x, sup):
    pix, valid = LE.support_patches(c, g, sup)
    idx = g["x"].elem(pix.unsqueeze(-1), torch.arange(g["x"].cs, device="cuda").view(1, 1, -1))
    return (x.view(-1)[idx] * valid.unsqueeze(-1)).cpu().double()


def same(got, want64, what):
    want = want64.to(got.dtype)
    if not torch.equal(got, want):
        d = (got != want).nonzero()
        raise AssertionError(f"{what}: {d.shape[0]} of {want.numel()} elements differ; first at {d[0].tolist()}: got {float(got[tuple(d[0])])}, want {float(want[tuple(d[0])])}")


@pytest.mark.parametrize("c", LE.WGRAD_CASES, ids=lambda c: c["name"])
def test_wgrad_large(ops, budget, _guarded_slabs, c):
    g = LE.geometry(c)
    LE.check_geometry(c, g)
    x, xtail = alloc(g["x"])
    dy, dytail, sup, D = sparse_dy(c, g)
    want = LE.wgrad_want(c, g, gather_x(c, g, x, sup), D)
    B, H, W = g["B"], g["H"], g["W"]
    if c["form"] == "dense":
        import test_gpu_conv_exact as G
        segs, outs = [], []
        for g0, g1, cin, alpha, dW, db in want:
            gw, gb = torch.full((g1 - g0, cin, 3, 3), SENTINEL, device="cuda"), torch.full((g1 - g0 + 8,), SENTINEL, device="cuda")
            segs.append((g0, g1, gw, gb, cin, alpha))
            outs.append((gw, gb, dW, db))
        with Prof(c["name"]):
            G._wgrad_dense(dy, x, segs, 192, 192, g["dy"].plane, g["x"].plane, (B, H, W), False)
            torch.cuda.synchronize()
        for (g0, g1, *_), (gw, gb, dW, db) in zip(segs, outs):
            same(gw.cpu(), dW, f"grad of rows [{g0}, {g1})")
            same(gb[:g1 - g0].cpu(), db, f"bias gradient of rows [{g0}, {g1})")
            assert bool((gb[g1 - g0:] == SENTINEL).all())
    else:
        dW, db, _ = want
        (kh, kw), cin, cout = c["k"], c["cin"], c["cout"]
        n = kh * kw
        if c["layout"] == "canonical":
            lay, val = (cin * n, n, kw, 1, 0), dW
        else:
            lay, val = (n, cout * n, kw, 1, 5), dW.permute(1, 0, 2, 3)
        grad = torch.full((cout * cin * n + lay[4] + TAIL,), SENTINEL, device="cuda")
        gb = torch.full((cout + 8,), SENTINEL, device="cuda") if c["bias_grad"] else None
        with Prof(c["name"]):
            ops.conv_wgrad(dy, x, grad, kh=kh, kw=kw, stride=c["s"], Cout=cout, Cin=cin, pad=c["pad"], layout=lay, bias_grad=gb)
            torch.cuda.synchronize()
        expect = torch.full((grad.numel(),), SENTINEL, dtype=torch.float64)
        expect[lay[4]:lay[4] + cout * cin * n] = val.reshape(-1)
        same(grad.cpu(), expect, "grad")
        if gb is not None:
            same(gb[:cout].cpu(), db, "bias_grad")
            assert bool((gb[cout:] == SENTINEL).all())
    assert _guarded_slabs.calls >= 1
    assert unchanged(x, g["x"]), "x after the call"
    assert dy_intact(dy, g, sup, D) and tail_ok(xtail) and tail_ok(dytail), "dy after the call"
    RAN.add(c["name"])


# ---------------------------------------------------------------------------------------------------------------------- glue kernels
@pytest.fixture(scope="module")
def L(ops):
    import test_gpu_glue_kernels as GK
    return GK.Lib()


BF = torch.bfloat16
H2, W2 = 1022, 1028                # the low-resolution side of the x2 kernels: 8 images, 64 channels, 1,075,830,784 B; the other side 4 times that


def _past(buf, k):
    assert buf.nbytes > k * LE.G31, (buf.name, buf.nbytes)
    return buf


def test_upsample2_destination_past_4_gib(L, budget):
    src_b = LE.Buf("glue/up/src", LE.INT4, 8, H2, W2, 64, BF)
    dst_b = _past(LE.Buf("glue/up/dst", LE.SENT, 8, 2 * H2, 2 * W2, 64, BF), 2)
    (src, stail), (dst, dtail) = alloc(src_b), alloc(dst_b)
    L.upsample2(src, 64, 0, 0, dst, 64, 8, H2, W2, 64)
    torch.cuda.synchronize()
    for b in range(8):
        assert torch.equal(dst[b], src[b].repeat_interleave(2, 0).repeat_interleave(2, 1)), b
    assert unchanged(src, src_b) and tail_ok(stail) and tail_ok(dtail)
    RAN.add("upsample2")


def test_sum2x2_source_past_4_gib(L, budget):
    src_b = _past(LE.Buf("glue/sum/src", LE.INT4, 8, 2 * H2, 2 * W2, 64, BF), 2)
    dst_b = LE.Buf("glue/sum/dst", LE.SENT, 8, H2, W2, 64, BF)
    (src, stail), (dst, dtail) = alloc(src_b), alloc(dst_b)
    L.sum2x2(src, 64, dst, 64, None, 0, 0.0, 8, H2, W2, 64)
    torch.cuda.synchronize()
    for b in range(8):                 # sums of four integers in [-4, 4]: exact in every type
        assert torch.equal(dst[b], src[b].view(H2, 2, W2, 2, 64).float().sum((1, 3)).to(BF)), b
    assert unchanged(src, src_b) and tail_ok(stail) and tail_ok(dtail)
    RAN.add("sum2x2")


def _sum_matches(y, y_b, x_b, factor=None):
    flat = y.view(-1)
    for s in range(0, y_b.numel, LE.CHUNK):
        e = min(y_b.numel, s + LE.CHUNK)
        idx = torch.arange(s, e, device="cuda")
        want = (LE.values(y_b.name, y_b.kind, idx) + LE.values(x_b.name, x_b.kind, idx)).float()
        if not torch.equal(flat[s:e], want.to(y.dtype)):
            return False
    return True


def test_add_inplace_past_4_gib(L, budget):
    B, (H, W) = 8, LE.IMG
    y_b, x_b = _past(LE.Buf("glue/add/y", LE.INT4, B, H, W, 64, BF), 2), LE.Buf("glue/add/x", LE.INT4, B, H, W, 64, BF)
    (y, ytail), (x, xtail) = alloc(y_b), alloc(x_b)
    L.add_inplace(y, (64, 0, 0), x, (64, 0, 0), None, None, 0.0, B * H * W, 64)
    torch.cuda.synchronize()
    assert _sum_matches(y, y_b, x_b) and unchanged(x, x_b) and tail_ok(ytail) and tail_ok(xtail)
    RAN.add("add_inplace")


def test_add_inplace_planes_past_4_gib(L, budget):
    """both operands blocked, six planes of 806,873,088 B each, all 192 channels: the sum is element-wise in storage order too"""
    B, (H, W) = 3, LE.IMG
    y_b, x_b = _past(LE.Buf("glue/addp/y", LE.INT4, B, H, W, 192, BF, True), 2), LE.Buf("glue/addp/x", LE.INT4, B, H, W, 192, BF, True)
    (y, ytail), (x, xtail) = alloc(y_b), alloc(x_b)
    L.add_inplace(y, (32, 0, y_b.plane), x, (32, 0, x_b.plane), None, None, 0.0, B * H * W, 192)
    torch.cuda.synchronize()
    assert _sum_matches(y, y_b, x_b) and unchanged(x, x_b) and tail_ok(ytail) and tail_ok(xtail)
    RAN.add("add_inplace_planes")


def test_mask_inplace_past_4_gib(L, budget):
    """g *= act > 0 ? 1 : 1/2 on 2^31 + 4,177,920 elements: integers times 1 or 1/2, exact"""
    B, (H, W) = 8, LE.IMG
    g_b, a_b = _past(LE.Buf("glue/mask/g", LE.INT4, B, H, W, 64, BF), 2), LE.Buf("glue/mask/act", ("int", -2, 2), B, H, W, 64, BF)
    (gt, gtail), (act, atail) = alloc(g_b), alloc(a_b)
    L.mask(gt, act, 0.5, g_b.numel)
    torch.cuda.synchronize()
    flat = gt.view(-1)
    for s in range(0, g_b.numel, LE.CHUNK):
        idx = torch.arange(s, min(g_b.numel, s + LE.CHUNK), device="cuda")
        gv, av = LE.values(g_b.name, g_b.kind, idx).float(), LE.values(a_b.name, a_b.kind, idx)
        assert torch.equal(flat[s:s + idx.numel()], torch.where(av > 0, gv, gv * 0.5).to(BF)), s
    assert unchanged(act, a_b) and tail_ok(gtail) and tail_ok(atail)
    RAN.add("mask_inplace")


def test_col_reduce_past_4_gib(ops, budget):
    """mode 0 over 33,619,712 pixels of 64 channels with the sparse integer operand of the weight-gradient case: the float64 column sums"""
    c = LE.case("le_w3_64_64_bias")
    g = LE.geometry(c)
    _past(g["dy"], 2)
    dy, tail, sup, D = sparse_dy(c, g)
    assert float(D.abs().sum(0).max()) < 2.0 ** 24
    for scale in (1.0, 0.5):
        same(ops.col_sum(dy, 64, 0, scale).cpu(), D.sum(0) * scale, "col_reduce mode 0")
    assert tail_ok(tail)
    RAN.add("col_reduce")


def test_nhwc_nchw_past_2_31_elements(ops, budget):
    B, (H, W), C = 8, LE.IMG, 64
    x_b = LE.Buf("glue/nchw/x", LE.INT4, B, H, W, C, BF)
    assert x_b.numel > 1 << 31
    x, xtail = alloc(x_b)
    n = ops.to_nchw(x)
    torch.cuda.synchronize()
    for b in range(B):
        assert torch.equal(n[b], x[b].permute(2, 0, 1).float()), b
    assert unchanged(x, x_b) and tail_ok(xtail)
    del x, xtail
    torch.cuda.empty_cache()
    back = ops.to_nhwc(n, dtype=BF)
    torch.cuda.synchronize()
    assert unchanged(back, x_b)
    RAN.add("nhwc_nchw")


# ---------------------------------------------------------------------------------------------------------------------- the classes
def test_every_case_ran_on_its_kernel_family():
    """every case ran (none skipped on a device that has the memory), every class seen is one test_gpu_conv_exact expects, and each case was
    served by the family its row names: a large case rerouted, say to the self-loading kernel, fails here"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import test_gpu_conv_exact as G
    assert RAN == set(ALL_IDS), f"did not run (a partial selection, failures, or skips): {sorted(set(ALL_IDS) - RAN)}"
    for c in LE.ALL_CASES:
        classes = SEEN.get(c["name"], [])
        if c.get("refuse"):
            assert classes == [], (c["name"], classes)
            continue
        assert classes, c["name"]
        assert not (set(classes) - G.EXPECTED_CLASSES), (c["name"], sorted(set(classes) - G.EXPECTED_CLASSES))
        first = classes[0]                                              # the large call; the pieces follow
        assert c["family"] in first, f"{c['name']}: served by {first}, its row names {c['family']}"
        if c["form"] == "dense":                                        # both launches of a dense block: whole tiles `fast`, ragged ones not
            assert all(("fast" in k) == ("fast" in c["family"]) for k in classes), (c["name"], classes)
