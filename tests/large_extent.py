"""Operands, geometry and float64 references for the exact tests of the convolution and glue kernels on tensors past 2 and 4 GiB
(tests/test_gpu_large_extent.py on the GPU, tests/test_large_extent_teeth.py on the CPU).  No kernel runs here.

Counter-based operands.  Element i of the STORAGE of operand `name` (i = its offset in elements, so the blocked layout counts plane by
plane) has the value value(kind, hash64(seed(name), i)): a 64-bit multiply-xorshift hash in plain int64 torch arithmetic, which wraps, on
the GPU over an index range (fill, in chunks of 2^25 elements) and on the CPU for any list of indices (HashFetch).  Nothing large is ever
materialised on the host, and two elements whose byte offsets differ by 2^31 or 2^32 are independent, so a kernel that wraps an offset
reads other numbers (tests/test_large_extent_teeth.py shows that every case's reference notices).  The value classes are those of
tests/conv_exact.py: ternary x and w (density 1/2 and min(1/2, 864 / K)), integers in [-4, 4] for bias and gradients, SENTINEL where a
buffer must stay untouched, and hashed bytes for a sign mask.

Geometry.  `boundaries(buf)` = every multiple of 2^31 bytes strictly inside an operand's storage, as (plane, b, y, x, byte in the pixel
record); `check_geometry(case)` asserts that a case crosses exactly the boundaries its row claims, each strictly inside a row, and that
one image (row) less would not reach the last of them.

References.  `windows(case)` lists small output rectangles -- the corners of the first and last image, one straddling every boundary of
every operand, one per image at a hashed place -- and `window_want` evaluates one with conv_exact.conv-style float64 arithmetic and
conv_exact.epilogue from patches a `fetch` supplies (HashFetch here, the GPU buffers in the GPU test).  The weight gradients sum over all
pixels, so their dy is zero outside `dy_support(case)` (some 2^14 pixels: the first and last rows of every image, both sides of every
boundary of x and of dy, and one hashed pixel in each of 2^14 equal strata of the batch); `wgrad_want` is then a complete float64
reference from the support's patches alone."""
import zlib

import torch
import torch.nn.functional as F

import conv_exact as CE
from conv_exact import SENTINEL, TDT

M64 = 1 << 64
G31 = 1 << 31
CHUNK = 1 << 25
WIN_H, WIN_W = 20, 72                     # a window (at most 24 x 80): wider than a 32-column tile, taller than a 16-row one
SLOPE, MSLOPE, BETA1 = 0.25, 0.5, 0.5


def _s64(c):
    c %= M64
    return c - M64 if c >= 1 << 63 else c


K0, K1, K2 = _s64(0x9E3779B97F4A7C15), _s64(0xBF58476D1CE4E5B9), _s64(0x94D049BB133111EB)


def _lsr(z, k):
    return (z >> k) & ((1 << (64 - k)) - 1)


def seed(name):
    return _s64((zlib.crc32(name.encode()) + 1) * 0x2545F4914F6CDD1D)


def hash64(sd, idx):
    """splitmix64's finaliser of sd + idx * golden ratio; int64 arithmetic wraps on the CPU and on the GPU alike"""
    z = idx * K0 + sd
    z = (z ^ _lsr(z, 30)) * K1
    z = (z ^ _lsr(z, 27)) * K2
    return z ^ _lsr(z, 31)


def values(name, kind, idx):
    """int64 index tensor (any device) -> the operand's values there, as an int64 tensor (every value class is integral)"""
    if kind[0] == "const":
        return torch.full_like(idx, int(kind[1]))
    h = hash64(seed(name), idx)
    if kind[0] == "tern":                  # {-1, 0, 1}, non-zero with probability kind[1]
        nz = _lsr(h, 40) < int(kind[1] * (1 << 24))
        return nz.to(torch.int64) * ((h & 1) * 2 - 1)
    lo, hi = kind[1], kind[2]              # "int": uniform integers in [lo, hi]
    return lo + _lsr(h, 33) % (hi - lo + 1)


TERN, INT4, SENT, BYTE = ("tern", 0.5), ("int", -4, 4), ("const", SENTINEL), ("int", 0, 255)


class Buf:
    """One operand: logical NHWC [B, H, W, cs] of `tdt`, stored interleaved or blocked ([plane][B*H*W][64 bytes], ops.make_blocked)."""

    def __init__(self, name, kind, B, H, W, cs, tdt, blocked=False):
        self.name, self.kind, self.B, self.H, self.W, self.cs, self.tdt, self.blocked = name, kind, B, H, W, cs, tdt, blocked
        self.esz = torch.empty((), dtype=tdt).element_size()
        self.kce = 64 // self.esz
        self.npl = -(-cs // self.kce) if blocked else 1
        self.npix = B * H * W
        self.rec = 64 if blocked else cs * self.esz                   # bytes of one pixel record
        self.plane = self.npix * 64 if blocked else 0                 # plane stride in bytes, as the C ABI takes it
        self.numel = self.npl * self.npix * self.kce if blocked else self.npix * cs
        self.nbytes = self.numel * self.esz
        self.shape = (self.npl, B, H, W, self.kce) if blocked else (B, H, W, cs)

    def elem(self, pix, c):
        """storage offsets in elements of channel(s) c of the pixel(s) with flat index pix = (b H + y) W + x"""
        if not self.blocked:
            return pix * self.cs + c
        return (c // self.kce) * (self.npix * self.kce) + pix * self.kce + c % self.kce

    def locate(self, off):
        """byte offset -> (plane, b, y, x, byte inside the pixel record)"""
        pl, r = divmod(off, self.plane) if self.blocked else (0, off)
        pix, byte = divmod(r, self.rec)
        b, r2 = divmod(pix, self.H * self.W)
        y, x = divmod(r2, self.W)
        return pl, b, y, x, byte

    def boundaries(self):
        return [k * G31 for k in range(1, (self.nbytes - 1) // G31 + 1)]


def fill(t, buf):
    """the GPU side of the generator: t (buf.shape, contiguous) <- values, in chunks"""
    flat = t.view(-1)
    assert flat.numel() == buf.numel
    if buf.kind[0] == "const":
        flat.fill_(buf.kind[1])
        return t
    for s in range(0, buf.numel, CHUNK):
        e = min(buf.numel, s + CHUNK)
        flat[s:e] = values(buf.name, buf.kind, torch.arange(s, e, device=t.device)).to(t.dtype)
    return t


class HashFetch:
    """fetch(buf, b, y0, y1, x0, x1) -> float64 [y1 - y0, x1 - x0, cs] from the generator, on the CPU.  `remap` = {operand name: function
    of a byte-offset tensor}: the operand is read at remap(offset) instead -- the teeth tests' model of a kernel that wraps."""

    def __init__(self, remap=None):
        self.remap = remap or {}

    def at(self, buf, pix, c):
        idx = buf.elem(pix, c)
        if buf.name in self.remap:
            idx = self.remap[buf.name](idx * buf.esz) // buf.esz
        return values(buf.name, buf.kind, idx).double()

    def __call__(self, buf, b, y0, y1, x0, x1):
        ys, xs = torch.arange(y0, y1).view(-1, 1, 1), torch.arange(x0, x1).view(1, -1, 1)
        return self.at(buf, (b * buf.H + ys) * buf.W + xs, torch.arange(buf.cs).view(1, 1, -1))


WRAPS = {"mod 2^32": lambda o: o % (1 << 32),
         "mod 2^31": lambda o: o % G31,
         "sign-extended low 32 bits": lambda o: ((o + G31) % (1 << 32)) - G31}


# ------------------------------------------------------------------------------------------------------------------- the case table
IMG = (2044, 2056)           # 64 tiles of 32 columns and 8 columns more; 537,915,392 B at 64 16-bit channels
CONV_DEFAULTS = dict(form="conv", dt="bf16", k=(3, 3), s=1, pad=(1, 1), cin=64, cout=64, B=8, hw=IMG, x_cs=None, blocked=False, y_in_x=False, y_coff=0,
                     y_cs=None, act=False, bias=True, sign_in=False, sign_out=False, r1=False, claims=None, tight=None, family=None, refuse=None)


def conv_case(name, **kw):
    bad = set(kw) - set(CONV_DEFAULTS)
    assert not bad, bad
    return dict(CONV_DEFAULTS, name=name, **kw)


# claims: operand -> the multiples of 2^31 bytes its storage crosses; tight: the operand whose last boundary sets the extent;
# family: what the launch profiler must report
CONV_CASES = [
    conv_case("le_c3_64_64_act", act=True, claims=dict(x=[1, 2], y=[1, 2]), tight="x", family="conv3x3_ls<bf16,MT2,"),
    conv_case("le_c3_64_64_act_fp32", dt="fp32", B=4, act=True, claims=dict(x=[1, 2], y=[1, 2]), tight="x", family="conv3x3_ls<f32,MT2,"),
    conv_case("le_c3_64_32_single", cout=32, B=1, hw=(8185, 4100), act=True, claims=dict(x=[1, 2], y=[1]), tight="x", family="conv3x3_ls<bf16,MT1,"),
    conv_case("le_c3_conv_last", cout=3, y_cs=8, claims=dict(x=[1, 2], y=[]), tight="x", family="conv3x3_ls<bf16,MT1,"),
    # conv_last's input gradient.  The mask (8 B per pixel) would need 2^28 pixels, a 32 GiB y, to reach 2^31.  Twenty images are what the
    # 16 GiB cap permits (y 10.0, x 1.3, mask 0.6 GiB): y crosses five multiples of 2^31, the mask of 672,394,240 B crosses nothing
    conv_case("le_c3_8_64_sign_in", cin=8, B=20, bias=False, sign_in=True, claims=dict(x=[], y=[1, 2, 3, 4, 5], sign=[]), tight="y",
              family="conv3x3_ls<bf16,MT2,W8+4,e8>"),
    conv_case("le_up_pair", form="up", k=(1, 1), pad=(0, 0), B=8, hw=(1022, 1028), bias=False, act=True, sign_out=True,
              claims=dict(x=[], y=[1, 2], sign=[]), tight="y", family="conv_igemm<bf16,1x1,s1,MT4>"),
    conv_case("le_g2x2s2", k=(2, 2), s=2, pad=(0, 0), cout=32, claims=dict(x=[1, 2], y=[]), tight="x", family="conv_igemm<bf16,2x2,s2,MT1>"),
    # rows so wide that (18 W + 34) * 384 B reaches 2^31: dispatch_dma leaves the loader-specialised kernel for the self-loading one, whose
    # offsets inside an image are 32-bit.  17 rows are the tallest image below 2^31 bytes (2,028,249,600; the 18th row is refused); the
    # extent is set by that threshold, and nothing crosses a multiple of 2^31
    conv_case("le_c3_wide_rows", cin=192, cout=32, B=1, hw=(17, 310700), act=True, claims=dict(x=[], y=[]), family="conv3x3_dma<bf16,MT1,"),
    # dense-block forward, six planes of 806,873,088 B
    conv_case("le_c3b_160_32", cin=160, cout=32, B=3, x_cs=192, blocked=True, y_in_x=True, y_coff=160, act=True, claims=dict(x=[1, 2]), tight="x",
              family="conv3x3_ls<bf16,MT1,W8+8,e0"),
    # the same form on planes of 2,151,661,568 B >= 2^31: the epilogue without 32-bit buffer offsets (buf16 off), streamed weights ...
    conv_case("le_c3b_bigplane", cin=160, cout=32, B=8, x_cs=192, blocked=True, y_in_x=True, y_coff=160, act=True, claims=dict(x=[1, 2, 3, 4, 5, 6]), tight="x",
              family="conv3x3_ls<bf16,MT1,W8+8,e0"),
    # ... and resident weights, three stages (Cin 64)
    conv_case("le_c3b_bigplane_64", cin=64, cout=32, B=8, x_cs=96, blocked=True, y_in_x=True, y_coff=64, act=True, claims=dict(x=[1, 2, 3]), tight="x",
              family="conv3x3_ls<bf16,MT1,W8+8,wres,s3,e0"),
    # the same with a residual operand of that plane size: Cout <= 32 reads it through 64-bit pointers and must compute ...
    conv_case("le_c3b_bigplane_r1", cin=64, cout=32, B=8, x_cs=96, blocked=True, y_in_x=True, y_coff=64, r1="own", claims=dict(x=[1, 2, 3], r1=[1]), tight="x",
              family="conv3x3_ls<bf16,MT1,W8+8,wres,e7>"),
    # ... while the 64-channel tile requests it with 32-bit per-lane offsets across two planes (conv_lds_rows_request): refused before launch
    conv_case("le_c3b_co64_r1_refused", cin=64, cout=64, B=8, blocked=True, r1="x", claims=dict(x=[1, 2], y=[1, 2]), tight="x",
              refuse="a residual operand's channel plane must be below 2 GiB"),
]

WGRAD_DEFAULTS = dict(form="wgrad", dt="bf16", k=(3, 3), s=1, pad=(1, 1), cin=64, cout=64, B=8, hw=IMG, bias_grad=False, layout="canonical", blocked=False,
                      claims=None, tight="x", family=None)


def wgrad_case(name, **kw):
    bad = set(kw) - set(WGRAD_DEFAULTS)
    assert not bad, bad
    return dict(WGRAD_DEFAULTS, name=name, **kw)


WGRAD_CASES = [
    wgrad_case("le_w3_64_64_bias", bias_grad=True, claims=dict(x=[1, 2], dy=[1, 2]), family="conv_wgrad<bf16,3x3,s1,MT2>"),
    wgrad_case("le_w3_c3", cout=3, claims=dict(x=[1, 2], dy=[]), family="conv_wgrad<bf16,3x3,s1,c3>"),
    wgrad_case("le_w2x2s2_transposed", k=(2, 2), s=2, pad=(0, 0), layout="transposed", claims=dict(x=[1, 2], dy=[]), family="conv_wgrad<bf16,2x2,s2,MT2>"),
    # one image whose own span crosses 2^32 (x) and 2^31 (dy): offsets inside an image, not only image bases
    wgrad_case("le_w3_single", cout=32, B=1, hw=(8185, 4100), bias_grad=True, claims=dict(x=[1, 2], dy=[1]), family="conv_wgrad<bf16,3x3,s1,MT1>"),
    # srcgan_wgrad_dense, nf 64, gc 32: activations [192] and gradients [192] in six planes each; whole tiles (8 x 32) and ragged ones
    wgrad_case("le_dense_fast", form="dense", B=3, hw=(2040, 2080), blocked=True, claims=dict(x=[1, 2], dy=[1, 2]), family="wgrad_dense<bf16,MT2,NT3,fast>"),
    wgrad_case("le_dense_single", form="dense", B=1, hw=(2729, 4100), blocked=True, claims=dict(x=[1, 2], dy=[1, 2]), family="wgrad_dense<bf16,MT2,NT3>"),
    wgrad_case("le_dense_ragged", form="dense", B=3, blocked=True, claims=dict(x=[1, 2], dy=[1, 2]), family="wgrad_dense<bf16,MT2,NT3>"),
]
ALL_CASES = CONV_CASES + WGRAD_CASES


def case(name):
    return next(c for c in ALL_CASES if c["name"] == name)


def geometry(c):
    """-> dict: the operands' Bufs (x, y unless y_in_x, sign; dy for the weight gradients) and the extents"""
    T = TDT[c["dt"]]
    B, (H, W) = c["B"], c["hw"]
    (kh, kw), s, pad = c["k"], c["s"], c["pad"]
    n = c["name"]
    if c["form"] == "dense":
        return dict(B=B, H=H, W=W, OH=H, OW=W, x=Buf(n + "/x", TERN, B, H, W, 192, T, True), dy=Buf(n + "/dy", INT4, B, H, W, 192, T, True))
    OH, OW = (H + 2 * pad[0] - kh) // s + 1, (W + 2 * pad[1] - kw) // s + 1
    if c["form"] == "wgrad":
        cr = -(-c["cout"] // 8) * 8
        return dict(B=B, H=H, W=W, OH=OH, OW=OW, x=Buf(n + "/x", TERN, B, H, W, c["cin"], T), dy=Buf(n + "/dy", INT4, B, OH, OW, cr, T))
    os_ = 2 if c["form"] == "up" else 1
    g = dict(B=B, H=H, W=W, OH=OH, OW=OW, os=os_, YH=OH * os_, YW=OW * os_)
    g["x"] = Buf(n + "/x", TERN, B, H, W, c["x_cs"] or c["cin"], T, c["blocked"])
    if not c["y_in_x"]:
        g["y"] = Buf(n + "/y", SENT, B, g["YH"], g["YW"], c["y_cs"] or c["y_coff"] + c["cout"], T)
    if c["sign_in"] or c["sign_out"]:
        g["sign"] = Buf(n + "/sign", BYTE if c["sign_in"] else ("const", 0), B, g["YH"], g["YW"], c["cout"] // 8, torch.uint8)
    if c["r1"] == "own":
        g["r1"] = Buf(n + "/r1", INT4, B, g["YH"], g["YW"], c["cout"], T, True)
    return g


OPERANDS = ("x", "y", "sign", "r1", "dy")


def check_geometry(c, g=None):
    """on the geometry alone: the case crosses exactly what its row claims, every boundary strictly inside a row, by the smallest extent"""
    g = g or geometry(c)
    for op in OPERANDS:
        if op not in g:
            assert op not in c["claims"], (c["name"], op)
            continue
        buf = g[op]
        got = [o // G31 for o in buf.boundaries()]
        assert got == c["claims"][op], (c["name"], op, "crosses", got, "claims", c["claims"][op], buf.nbytes)
        for o in buf.boundaries():
            pl, b, y, x, byte = buf.locate(o)
            assert 0 < x < buf.W - 1, (c["name"], op, o, "lies at a row's (or an image's) start or end", (pl, b, y, x, byte))
    if c["tight"] is None:
        return
    buf = g[c["tight"]]
    last = buf.boundaries()[-1]
    per = buf.nbytes // (buf.B if buf.B > 1 else buf.H)                 # one image (a single image: one row) less
    assert buf.nbytes - per <= last, (c["name"], "a smaller extent crosses the same boundaries", buf.nbytes, per, last)


def _to_out(c, g, op, y, x):
    """pixel (y, x) of operand op -> the window coordinate it belongs to (the up-sampler's windows live on the input grid)"""
    if op == "x" and c["form"] != "up":
        return min(g["OH"] - 1, y // c["s"]), min(g["OW"] - 1, x // c["s"])
    if op != "x" and c["form"] == "up":
        return y // 2, x // 2
    return y, x


def windows(c, g=None):
    """[(b, oy0, ox0, h, w, why)]: rectangles of WIN_H x WIN_W on the output grid (the up-sampler: on the input grid, each pixel four outputs)"""
    g = g or geometry(c)
    GH, GW = (g["H"], g["W"]) if c["form"] == "up" else (g["OH"], g["OW"])
    h, w = min(WIN_H, GH), min(WIN_W, GW)
    clip = lambda oy, ox: (max(0, min(GH - h, oy)), max(0, min(GW - w, ox)))
    L = []
    for b in sorted({0, g["B"] - 1}):
        for oy in (0, GH - h):
            for ox in (0, GW - w):
                L.append((b, oy, ox, h, w, "corner"))
    for op in OPERANDS:
        if op in g:
            for o in g[op].boundaries():
                pl, b, y, x, _ = g[op].locate(o)
                oy, ox = _to_out(c, g, op, y, x)
                L.append((b,) + clip(oy - h // 2, ox - w // 2) + (h, w, f"{op} at {o // G31} x 2^31"))
    hs = hash64(seed(c["name"] + "/windows"), torch.arange(2 * g["B"]))
    for b in range(g["B"]):
        L.append((b,) + clip(int(_lsr(hs[2 * b], 1)) % GH, int(_lsr(hs[2 * b + 1], 1)) % GW) + (h, w, "hashed"))
    return L


def window_region(c, g, op, win):
    """the pixels (b, y0, y1, x0, x1) of operand op that a window reads or writes"""
    b, oy, ox, h, w, _ = win
    if op == "x":
        if c["form"] == "up":
            return b, oy, oy + h, ox, ox + w
        s, (kh, kw), pad = c["s"], c["k"], c["pad"]
        return (b, max(0, oy * s - pad[0]), min(g["H"], (oy + h - 1) * s - pad[0] + kh), max(0, ox * s - pad[1]), min(g["W"], (ox + w - 1) * s - pad[1] + kw))
    os_ = g["os"]
    return b, oy * os_, (oy + h) * os_, ox * os_, (ox + w) * os_


def weights(c):
    """the small operands, from conv_exact's generators: w (canonical; the up-sampler: [cin, cout, 2, 2]) and the bias"""
    gn = CE.gen(c["name"])
    (kh, kw) = c["k"]
    if c["form"] == "up":
        w = CE.ternary((c["cin"], c["cout"], 2, 2), CE.w_density(c["cin"]), gn)
    else:
        w = CE.ternary((c["cout"], c["cin"], kh, kw), CE.w_density(c["cin"] * kh * kw), gn)
    return w, (CE.ints((c["cout"],), -4, 4, gn) if c["bias"] else None)


def window_want(c, g, win, fetch, w, bias):
    """-> dict(y=(region, float64 [h', w', y_cs]), sign=(region, uint8-valued [h', w', cout / 8]) when a mask is written): what the
    window's part of the output buffer must hold after the call, from float64 arithmetic on fetched patches"""
    b, oy, ox, h, wd, _ = win
    cin, cout = c["cin"], c["cout"]
    xr = window_region(c, g, "x", win)
    xp = fetch(g["x"], *xr)[..., :cin]
    if c["form"] == "up":
        xin = xp.permute(2, 0, 1).unsqueeze(0)
        conv, absconv = F.conv_transpose2d(xin, w, None, 2), F.conv_transpose2d(xin.abs(), w.abs(), None, 2)
    else:
        s, (kh, kw), pad = c["s"], c["k"], c["pad"]
        ph, pw = (h - 1) * s + kh, (wd - 1) * s + kw
        full = torch.zeros(ph, pw, cin, dtype=torch.float64)
        ty, tx = xr[1] - (oy * s - pad[0]), xr[3] - (ox * s - pad[1])
        full[ty:ty + xp.shape[0], tx:tx + xp.shape[1]] = xp
        xin = full.permute(2, 0, 1).unsqueeze(0)
        conv, absconv = F.conv2d(xin, w, None, s), F.conv2d(xin.abs(), w.abs(), None, s)
    ep = dict(bias=bias, alpha=1.0, act=c["act"], slope=SLOPE, mslope=MSLOPE)
    yr = window_region(c, g, "y", win)
    if c["sign_in"]:
        bits = CE.unpack_sign8(fetch(g["sign"], *yr).to(torch.uint8).unsqueeze(0))
        ep["mz"] = torch.where(bits, 1.0, -1.0).double()
    if c["r1"]:
        ep.update(r1=fetch(g["r1"], *yr)[..., :cout].permute(2, 0, 1).unsqueeze(0), beta1=BETA1, r1_cend=cout)
    pre, v, _ = CE.epilogue(conv, **ep)
    CE.check_exact(c["name"], c["dt"], absconv + (bias.abs().view(1, -1, 1, 1) if bias is not None else 0.0), pre, v, 1.0)
    ybuf = g["x"] if c["y_in_x"] else g["y"]
    want = fetch(ybuf, *yr).clone()
    want[..., c["y_coff"]:c["y_coff"] + cout] = v[0].permute(1, 2, 0)
    out = dict(y=(yr, want))
    if c["sign_out"]:
        out["sign"] = (yr, CE.pack_sign8(v > 0)[0].double())
    return out


# ------------------------------------------------------------------------------------------------------ sparse dy, weight gradients
N_SCATTER = 1 << 14
EDGE = 16


def dy_support(c, g=None):
    """sorted flat pixel indices (b OH + oy) OW + ox at which dy is non-zero (well below the 2^20 the exactness allows):
    EDGE pixels at both ends of the first and last row of every image, 2 EDGE pixels around every boundary of x and dy, and one hashed
    pixel in each of N_SCATTER equal strata of the batch -- so every image and every split-K slice of more than 1 / 2^14 holds some."""
    g = g or geometry(c)
    B, OH, OW = g["B"], g["OH"], g["OW"]
    P = []
    e = torch.arange(EDGE)
    for b in range(B):
        for oy in (0, OH - 1):
            P += [(b * OH + oy) * OW + e, (b * OH + oy) * OW + OW - 1 - e]
    s = c["s"]
    for op in ("x", "dy"):
        for o in g[op].boundaries():
            _, b, y, x, _ = g[op].locate(o)
            oy, ox = (min(OH - 1, y // s), x // s) if op == "x" else (y, x)
            P.append((b * OH + oy) * OW + torch.arange(max(0, ox - EDGE), min(OW, ox + EDGE)))
    npix = B * OH * OW
    per = npix // N_SCATTER
    j = torch.arange(N_SCATTER)
    P.append(j * per + _lsr(hash64(seed(c["name"] + "/support"), j), 1) % per)
    return torch.unique(torch.cat(P))


def support_patches(c, g, sup):
    """-> (pix [n, kh kw] flat x pixel indices of every tap, clamped into the image; valid [n, kh kw])"""
    OH, OW, H, W = g["OH"], g["OW"], g["H"], g["W"]
    (kh, kw), s, pad = c["k"], c["s"], c["pad"]
    b, r = sup // (OH * OW), sup % (OH * OW)
    oy, ox = r // OW, r % OW
    ky, kx = torch.arange(kh, device=sup.device).repeat_interleave(kw), torch.arange(kw, device=sup.device).repeat(kh)
    iy, ix = oy.unsqueeze(1) * s + ky - pad[0], ox.unsqueeze(1) * s + kx - pad[1]
    valid = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    return (b.unsqueeze(1) * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1), valid


def dy_values(g, sup, fetch=None):
    """float64 [n, cs] of dy on its support (the padding channels behind Cout are zero: set by the caller)"""
    fetch = fetch or HashFetch()
    return fetch.at(g["dy"], sup.view(-1, 1), torch.arange(g["dy"].cs).view(1, -1))


def wgrad_want(c, g, X, D):
    """X float64 [n, taps, Cx] (zero where a tap is outside the image), D float64 [n, Cdy] -> the float64 gradients and their bound.
    wgrad: (dW [cout, cin, kh, kw], bias gradient [cout], bound); dense: [(g0, g1, cin, alpha, dW, db)] for conv5 .. conv1."""
    n, taps, _ = X.shape
    bound = float((D.abs().sum(0).max()) * 1.0)
    assert bound + 8 < 2.0 ** 24, (c["name"], "a partial sum may leave the exact integers", bound)
    if c["form"] == "dense":
        out = []
        for g0, co, cin, alpha in CE.dense_segments(64, 32):
            dW = alpha * (D[:, g0:g0 + co].t() @ X[:, :, :cin].reshape(n, -1)).view(co, 3, 3, cin).permute(0, 3, 1, 2)
            out.append((g0, g0 + co, cin, alpha, dW.contiguous(), alpha * D[:, g0:g0 + co].sum(0)))
        return out
    (kh, kw), cin, cout = c["k"], c["cin"], c["cout"]
    dW = (D[:, :cout].t() @ X[:, :, :cin].reshape(n, -1)).view(cout, kh, kw, cin).permute(0, 3, 1, 2).contiguous()
    return dW, D[:, :cout].sum(0), bound
