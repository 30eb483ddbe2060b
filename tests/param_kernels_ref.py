"""CPU references (numpy / torch, no GPU import) of the kernels that hold the weights: the fused Adam step, the parameter
fingerprint, the weight pack and the NCHW <-> NHWC layout changes.  tests/test_gpu_param_kernels.py and
tests/test_gpu_layout_kernels.py compare the kernels with them; tests/test_param_kernels_teeth.py shows on the CPU, on the same
inputs, that each reference and bound tells the planted mistakes (the ``mistake=`` arguments below) from the right answer.

Adam is compared with a float64 evaluation under a per-element bound (the device code contracts multiply-adds, torch's does
not, so neither is the other's bit pattern); everything else is data movement or integer arithmetic and is compared in bits."""
import math

import numpy as np
import torch

U = 2.0 ** -24            # unit round-off of f32
SENT = 1000.0             # sentinel around every slice: exact in all three types, far from any datum
DTS = ["fp32", "bf16", "fp16"]
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
KCE = {"fp32": 16, "bf16": 32, "fp16": 32}      # elements of one 64-byte K chunk


def same_bits(a, b):
    """torch tensors of one shape and type with the same bits (so -0.0 != +0.0 and a NaN equals itself)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# =========================================================================== fused Adam
ADAM_SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097, 8195, 12288)
ADAM_BETAS = ((0.9, 0.999), (0.5, 0.999), (0.0, 0.999))
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_LRS = (1e-3, 0.0)
ADAM_EPS = 1e-8
ADAM_CHUNK = 4096
SCALAR_MISTAKES = ("no_bc2", "no_bc1", "beta1_as_weight", "beta2_on_g2")
ELEMENT_MISTAKES = ("skip_last", "skip_chunk_last", "one_past")


def adam_scalars(lr, b1, b2, eps, k, mistake=None):
    """The f32-rounded scalars adam_multi_k receives, formed as srcgan_adam_step forms them (bias corrections in double, one
    rounding each), as float64 values -> dict.  ``omw1`` is the kernel's own ``1.f - w1``, an f32 subtraction."""
    f = np.float32
    bc1, bc2 = 1.0 - math.pow(b1, float(k)), 1.0 - math.pow(b2, float(k))
    w1 = f(1.0 - b1)
    s, c, omb2 = f(lr / bc1), f(1.0 / math.sqrt(bc2)), f(1.0 - b2)
    if mistake == "no_bc2":
        c = f(1.0)
    elif mistake == "no_bc1":
        s = f(lr)
    elif mistake == "beta1_as_weight":
        w1 = f(b1)
    elif mistake == "beta2_on_g2":
        omb2 = f(b2)
    return {k_: float(v) for k_, v in dict(w1=w1, omw1=f(1.0) - w1, b2=f(b2), omb2=omb2, s=s, c=c, eps=f(eps)).items()}


def adam_ref(p, g, m0, v0, sc, mistake=None):
    """One Adam step in float64 from f32 inputs (any float arrays) -> (p*, m*, v*).  The lerp takes the kernel's branch."""
    p, g, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (p, g, m0, v0))
    d = g - m0
    m = m0 + sc["w1"] * d if sc["w1"] < 0.5 else g - d * sc["omw1"]
    v = v0 * sc["b2"] + sc["omb2"] * g * g
    D = np.sqrt(v * sc["c"] ** 2 + sc["eps"]) if mistake == "eps_in_sqrt" else np.sqrt(v) * sc["c"] + sc["eps"]
    return p - sc["s"] * (m / D), m, v


def adam_bound(ps, ms, vs, g, m0, sc):
    """Per-element bounds (E_p, E_m, E_v) of an f32 evaluation, in any rounding order and with or without contraction, against
    the float64 one (starred arguments).  Counting roundings: m takes a subtraction, a multiply and an add with |g - m0| <=
    2 max(|g|, |m0|); v three multiplies and an add of non-negative terms; D = sqrt(v) c + eps half of v's error plus sqrt, mul
    and add; the quotient and the product by s add 2U; the final subtraction rounds at half an ulp of p, which reaches U |p*|
    where the update is far below an ulp, hence the factor 2."""
    g, m0 = np.abs(np.asarray(g, dtype=np.float64)), np.abs(np.asarray(m0, dtype=np.float64))
    e_m = U * (np.abs(ms) + 4.0 * np.maximum(g, m0))
    e_v = 4.0 * U * vs
    D = np.sqrt(vs) * sc["c"] + sc["eps"]
    e_p = 2.0 * U * np.abs(ps) + sc["s"] * (e_m / D + 8.0 * U * np.abs(ms) / D)
    return e_p, e_m, e_v


def adam_f32(p, g, m0, v0, sc, order):
    """The kernel's formulas in numpy float32 -> (p, m, v).  order 'plain': every operation rounded; 'fma' / 'fma2': each
    multiply-add rounded once, the two ways v's expression can contract."""
    f = np.float32
    p, g, m0, v0 = (np.asarray(a, dtype=f) for a in (p, g, m0, v0))
    w1, omw1, b2, omb2, s, c, eps = (f(sc[k]) for k in ("w1", "omw1", "b2", "omb2", "s", "c", "eps"))
    if order == "plain":
        fma = lambda a, b, cc: (a * b).astype(f) + cc
    else:
        fma = lambda a, b, cc: (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(cc, dtype=np.float64)).astype(f)
    d = g - m0
    m = fma(w1, d, m0) if w1 < f(0.5) else fma(-d, omw1, g)
    og = omb2 * g
    v = fma(og, g, v0 * b2) if order != "fma2" else fma(v0, b2, og * g)
    D = fma(np.sqrt(v), c, eps)
    return fma(-s, m / D, p), m, v


def adam_values(rng, n):
    """n elements (p, g, m0, v0) as f32: magnitudes 1e-9 .. 1e2 with random signs (v0 the square of such a magnitude, p 1e-4 .. 10)
    and, by position, the special elements: m0 == g, zero g / m0 / v0, zero gradient on zero state, sqrt(v) below and near eps,
    p == 0.  Non-zero |g| >= 1e-9 >> 1e-15, v0 >= 1e-18: no f32 intermediate is subnormal."""
    f = np.float32
    mag = lambda lo, hi: 10.0 ** rng.uniform(lo, hi, n)
    sign = lambda: rng.choice([-1.0, 1.0], n)
    p, g, m0, v0 = (sign() * mag(-4, 1)).astype(f), (sign() * mag(-9, 2)).astype(f), (sign() * mag(-9, 2)).astype(f), (mag(-9, 2) ** 2).astype(f)
    kind = (np.arange(n) + rng.randint(0, 16)) % 16
    tiny = (sign() * 1e-9 * rng.uniform(1, 5, n)).astype(f)
    m0 = np.where(kind == 0, g, m0)
    g = np.where((kind == 1) | (kind == 4), f(0), g)
    m0 = np.where((kind == 2) | (kind == 4), f(0), m0)
    v0 = np.where((kind == 3) | (kind == 4), f(0), v0)
    g = np.where((kind == 5) | (kind == 6), tiny, g)                                               # sqrt(v) near eps = 1e-8 ...
    v0 = np.where(kind == 5, ((1e-8 * rng.uniform(0.5, 2, n)) ** 2).astype(f), v0)
    v0 = np.where(kind == 6, ((1e-9 * rng.uniform(1, 5, n)) ** 2).astype(f), v0)                   # ... and below it
    p = np.where(kind == 7, f(0), p)
    return p.astype(f), g.astype(f), m0.astype(f), v0.astype(f)


def adam_inputs(seed, sizes=ADAM_SIZES, grad_shift=0):
    """One parameter group as the GPU test lays it out -> dict.  'P', 'M', 'V': f32 buffers filled with SENT, tensor i at
    [offs[i], offs[i] + sizes[i]), every offset a multiple of 4 (16-byte aligned) with at least 4 sentinels on either side.
    'G': one flat gradient buffer, tensor i at the running offset goffs[i] (no gaps, as model._GradArena places them, so most are
    only 4-byte aligned), grad_shift elements before the first and 4 after the last."""
    rng = np.random.RandomState(seed)
    offs, a = [], 4
    for n in sizes:
        offs.append(a)
        a = (a + n + 4 + 3) // 4 * 4
    goffs = [grad_shift + int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    k = dict(sizes=tuple(sizes), offs=offs, goffs=goffs, P=np.full(a, SENT, np.float32), M=np.full(a, SENT, np.float32),
             V=np.full(a, SENT, np.float32), G=np.full(grad_shift + sum(sizes) + 4, SENT, np.float32))
    for n, o, go in zip(sizes, offs, goffs):
        k["P"][o:o + n], k["G"][go:go + n], k["M"][o:o + n], k["V"][o:o + n] = adam_values(rng, n)
    return k


def adam_expected(k, sc, mistake=None):
    """What one step must leave in the three buffers -> ({'P','M','V'} float64 references, {'P','M','V'} bounds); the bound is 0 on
    every sentinel, where equality is required.  The element mistakes: 'skip_last' leaves the last element of every tensor at
    its old values, 'skip_chunk_last' the last element of every full 4096-chunk, 'one_past' also updates element n."""
    ref = {q: k[q].astype(np.float64) for q in "PMV"}
    bound = {q: np.zeros(len(k[q])) for q in "PMV"}
    for n, o, go in zip(k["sizes"], k["offs"], k["goffs"]):
        n = n + 1 if mistake == "one_past" else n
        args = (k["P"][o:o + n], k["G"][go:go + n], k["M"][o:o + n], k["V"][o:o + n])
        new = adam_ref(*args, sc, mistake)
        bnd = adam_bound(*new, args[1], args[2], sc)
        keep = np.zeros(n, bool)
        if mistake == "skip_last":
            keep[n - 1] = True
        elif mistake == "skip_chunk_last":
            keep[ADAM_CHUNK - 1::ADAM_CHUNK] = True
        for q, old, val, b in zip("PMV", (args[0], args[2], args[3]), new, bnd):
            ref[q][o:o + n] = np.where(keep, old.astype(np.float64), val)
            bound[q][o:o + n] = b
    return ref, bound


def adam_check(got, ref, bound):
    """-> (every element within its bound -- equal where the bound is 0 --, worst error / bound over the elements with a bound)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    pos = bound > 0
    with np.errstate(invalid="ignore"):
        ratio = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    return bool(np.all(err <= bound)), ratio


# =========================================================================== parameter fingerprint
FP_SLICE = 16384          # elements a block hashes
FP_SINGLE_SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 16383, 16384, 16385, 3 * 16384 + 5)
FP_TABLE_SIZES = (1, 3, 64, 576, 16384, 16385, 36864)
FP_SPECIALS = (0x00000000, 0x80000000, 0x7FC12345, 0xFFA00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x3F800000)
_M32 = np.uint64(0xFFFFFFFF)


def _fmix32(h):
    """murmur3's finaliser on uint64 arrays holding 32-bit words"""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def fp_tensor(bits, t, drop_tail=False):
    """Tensor t's share of the fingerprint, as a Python int modulo 2^64.  Element i with bits x gives the two 32-bit words
    a = fmix32((x ^ salt_a) + i * 0x9E3779B1) and b = fmix32((x + salt_b) ^ (i * 0x85EBCA77 + 0x165667B1)); a thread of a block
    sums the a's and b's of elements i0 + tid + 256 j of its 16 Ki-element slice as 64-bit integers A, B and contributes
    (B << 32) + A + (B >> 32); everything else is wrapping 64-bit addition."""
    x = np.asarray(bits, dtype=np.uint32).astype(np.uint64)
    n = len(x)
    i = np.arange(n, dtype=np.uint64)             # the kernel's (unsigned)i: indices stay below 2^32 here
    salt_a = _fmix32(np.uint64((0x9E3779B9 * (t + 1)) & 0xFFFFFFFF))
    salt_b = _fmix32(np.uint64((0x7F4A7C15 + t) & 0xFFFFFFFF))
    a = _fmix32(((x ^ salt_a) + ((i * np.uint64(0x9E3779B1)) & _M32)) & _M32)
    b = _fmix32(((x + salt_b) & _M32) ^ ((i * np.uint64(0x85EBCA77) + np.uint64(0x165667B1)) & _M32))
    if drop_tail:
        a[-1] = b[-1] = 0
    pad = -n % FP_SLICE
    A = np.concatenate([a, np.zeros(pad, np.uint64)]).reshape(-1, FP_SLICE // 256, 256).sum(axis=1, dtype=np.uint64)
    B = np.concatenate([b, np.zeros(pad, np.uint64)]).reshape(-1, FP_SLICE // 256, 256).sum(axis=1, dtype=np.uint64)
    h = (B << np.uint64(32)) + A + (B >> np.uint64(32))          # uint64 array arithmetic wraps
    return sum(int(v) for v in h.reshape(-1)) & 0xFFFFFFFFFFFFFFFF


def fp_ref(tensors):
    """The 64-bit fingerprint of a list of uint32 bit arrays"""
    return sum(fp_tensor(b, t) for t, b in enumerate(tensors)) & 0xFFFFFFFFFFFFFFFF


def fp_bits(rng, n):
    """n random 32-bit patterns with the special ones (+-0, NaNs with payloads, infinities, subnormals) planted, the first and
    the last element included; a one-element tensor holds one of the special patterns."""
    x = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    where = np.unique(np.concatenate([[0, n - 1], rng.randint(0, n, min(n, 2 * len(FP_SPECIALS)))]))
    x[where] = np.array(FP_SPECIALS, dtype=np.uint32)[rng.randint(0, len(FP_SPECIALS), len(where))]
    return x


def fp_table_sizes(rng, ntens=700):
    """Sizes of the many-tensor table: two in five are one-element tensors, so that runs of consecutive blocks belong to
    different tensors; a one-element tensor sits in the middle."""
    sizes = rng.choice(FP_TABLE_SIZES, ntens, p=[0.4] + [0.1] * 6).tolist()
    sizes[ntens // 2] = 1
    return sizes


def fp_table_rows(ptrs, sizes):
    """The table rows (pointer, elements, first block) and the block count, as model._PackState.opts builds them"""
    rows, blk = [], 0
    for ptr, n in zip(ptrs, sizes):
        rows.append((ptr, n, blk))
        blk += (n + FP_SLICE - 1) // FP_SLICE
    return rows, blk


# =========================================================================== weight pack
PACK_ROWS = (1, 3, 31, 32, 33, 64, 65, 96)
PACK_TAPS = (1, 2, 3, 4)
PACK_SENT_BYTE = 0xFE          # 0xFEFE... is about -1e38 in f32 and bf16 and a NaN in fp16: no weight has these bits
PACK_FORMS = ("fwd", "dgrad_s1", "deconv_k2s2", "par4x4")


def pack_kdims(dt):
    return (1, 3, KCE[dt] - 1, KCE[dt], KCE[dt] + 1, 160)


def pack_values(shape, seed):
    """f32 weights in the normal range of all three types (2^-10 <= |w| < 4), one in eight an exact tie of bf16 or fp16 rounding
    (1 + 2^-8 and 1 + 3 2^-8 lie half way between bf16 neighbours, 1 + 2^-11 and 1 + 3 2^-11 between fp16 ones)."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(shape, generator=g) * 0.5).clamp(-3.9, 3.9)
    w = torch.where(w.abs() < 2.0 ** -10, torch.full_like(w, 2.0 ** -10), w)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -11)])
    pick = torch.randint(0, 8 * len(ties), w.shape, generator=g)
    return torch.where(pick < len(ties), ties[pick % len(ties)], w).float()


def pack_form(form, rows, kdim, k, q=0):
    """The stride sets the project's callers use -> (canonical weight shape, (rows, kdim, tys, txs, sr, sk, sty, stx, off)).
    'fwd': ops.pack_conv2d_fwd of a [rows, kdim, k, k] weight; 'dgrad_s1': ops.pack_conv2d_dgrad_s1 of [kdim, rows, k, k] (taps
    reversed through negative strides); 'deconv_k2s2': quadrant q of a ConvTranspose2d weight [kdim, rows, 2, 2]; 'par4x4': the
    2x2 taps that output parity q = 2a + b of a 4x4 stride-2 convolution's input gradient reads from [kdim, rows, 4, 4]."""
    if form == "fwd":
        return (rows, kdim, k, k), (rows, kdim, k, k, kdim * k * k, k * k, k, 1, 0)
    if form == "dgrad_s1":
        return (kdim, rows, k, k), (rows, kdim, k, k, k * k, rows * k * k, -k, -1, k * k - 1)
    if form == "deconv_k2s2":
        return (kdim, rows, 2, 2), (rows, kdim, 1, 1, 4, rows * 4, 0, 0, q)
    if form == "par4x4":
        a, b = q >> 1, q & 1
        return (kdim, rows, 4, 4), (rows, kdim, 2, 2, 16, rows * 16, -8, -2, (2 if a else 3) * 4 + (2 if b else 3))
    raise ValueError(form)


def pack_cases(form, dt):
    """Every (rows, kdim, taps or quadrant) of a form -> [(weight shape, pack arguments)]"""
    out = []
    for rows in PACK_ROWS:
        for kdim in pack_kdims(dt):
            for v in (PACK_TAPS if form in ("fwd", "dgrad_s1") else range(4)):
                out.append(pack_form(form, rows, kdim, v, v))
    return out


def pack_elems(rows, k_total, ntaps, dt):
    cot = 32 if rows <= 32 else 64
    return -(-rows // cot) * -(-k_total // KCE[dt]) * ntaps * cot * KCE[dt]


def pack_ref(w, rows, kdim, tys, txs, sr, sk, sty, stx, off, dt, k_off=0, k_total=None, scale=1.0, init=None, mistake=None):
    """Wp[row tile][chunk][tap][row (cot)][k (KCE)] as a flat tensor of the type: element (row, k) of tap (ty, tx) is
    f32(scale * w[off + row sr + (k - k_off) sk + ty sty + tx stx]) cast once (round to nearest even) for row < rows and
    k_off <= k < k_off + kdim.  A whole pack (k_off == 0, kdim == k_total) is zero everywhere else; a part pack leaves every other
    element as ``init`` has it.  Built from index arrays over the five axes, not from a flat-index decomposition."""
    k_total = kdim if k_total is None else k_total
    tdt, kce = TDT[dt], KCE[dt]
    cot = 64 if mistake == "cot64" else (32 if rows <= 32 else 64)
    nrt, nch, ntap = -(-rows // cot), -(-k_total // kce), tys * txs
    rt, ch, tap, rl, kl = torch.meshgrid(torch.arange(nrt), torch.arange(nch), torch.arange(ntap), torch.arange(cot), torch.arange(kce), indexing="ij")
    row, kk = rt * cot + rl, ch * kce + kl - (0 if mistake == "k_off_ignored" else k_off)
    ty, tx = (tap % tys, tap // tys) if mistake == "taps_transposed" else (tap // txs, tap % txs)
    inside = (row < rows) & (kk >= 0) & (kk < kdim)
    idx = off + row * sr + kk * sk + ty * sty + tx * stx
    flat = w.reshape(-1)
    assert int(idx[inside].min()) >= 0 and int(idx[inside].max()) < flat.numel(), "the pack would read outside the weight"
    src = flat[idx.clamp(0, flat.numel() - 1)]
    if mistake == "scale_after_cast":
        val = (src.to(tdt).float() * torch.tensor(scale, dtype=torch.float32)).to(tdt)
    else:
        val = (src * torch.tensor(scale, dtype=torch.float32)).to(tdt)
    if k_off == 0 and kdim == k_total:
        rest = torch.zeros(inside.shape, dtype=tdt)
    else:
        rest = init.reshape(inside.shape)
    return torch.where(inside, val, rest).reshape(-1)


def pack_sentinel(nelem, dt):
    return torch.full((nelem * TDT[dt].itemsize,), PACK_SENT_BYTE, dtype=torch.uint8).view(TDT[dt])


# the dense-block backward's composite matrix (nets.hip, the k_off loop): three calls fill [k_off, k_off + kdim) x [0, rows) of one
# matrix with k_total = 75 (no multiple of 16 or 32) from three weights [kdim, cin, 3, 3], rows = input channels [ss, ss + rows);
# the second call lands between two ranges written before it
PART_KTOTAL = 75
PART_CALLS = ((43, 32, 1.0, 80), (0, 30, -1.0, 96), (30, 13, 0.2, 112))       # (k_off, kdim, scale, cin of the source weight)
PART_ROWS = (70, 20)                                                           # two row tiles of 64 with a ragged second; cot = 32


def part_args(rows, k_off, kdim, cin, ss=5):
    """-> (weight shape, (rows, kdim, tys, txs, sr, sk, sty, stx, off)) of one part call, strides as in nets.hip"""
    return (kdim, cin, 3, 3), (rows, kdim, 3, 3, 9, cin * 9, -3, -1, ss * 9 + 8)


# =========================================================================== layout
LAYOUT_C = (1, 3, 8, 31, 32, 33, 70)
LAYOUT_HW = ((1, 1), (7, 9), (8, 8), (5, 13), (13, 37), (16, 32))              # H W = 1, 63, 64, 65, 481, 512
LAYOUT_B = (1, 3)


def layout_cs(C):
    return sorted({C, (C + 7) // 8 * 8, C + 5})


def layout_cases():
    return [(B, C, H, W, cs) for C in LAYOUT_C for cs in layout_cs(C) for (H, W) in LAYOUT_HW for B in LAYOUT_B]


def layout_coff(C, cs):
    """Where to_nchw's slice starts in a record of cs channels: 2 when there is room for NaN channels on both sides"""
    return 2 if cs >= C + 3 and cs != (C + 7) // 8 * 8 else 0


def layout_values(shape, seed):
    """f32 data in the normal range of all three types with rounding ties planted (pack_values), and a few +-0"""
    x = pack_values(shape, seed)
    g = torch.Generator().manual_seed(seed + 1)
    z = torch.randint(0, 32, shape, generator=g)
    return torch.where(z == 0, torch.zeros_like(x), torch.where(z == 1, -torch.zeros_like(x), x))


def nhwc_ref(x, cs, dt, mistake=None, sentinel=None):
    """NCHW f32 -> NHWC [B, H, W, cs] of the type: permute + one cast, channels [C, cs) +0"""
    B, C, H, W = x.shape
    v = x
    if mistake == "hw_exchanged":
        v = x.reshape(B, C, W, H).transpose(2, 3)
    elif mistake == "channels_rotated":
        v = x.roll(1, dims=1)
    out = torch.zeros(B, H, W, cs, dtype=TDT[dt])
    out[..., :C] = v.permute(0, 2, 3, 1).to(TDT[dt])
    if mistake == "last_pixel_left":
        out[-1, -1, -1, :] = sentinel
    elif mistake == "pad_nonzero":
        out[0, 0, 0, cs - 1] = -0.0 if cs > C else out[0, 0, 0, cs - 1]
    return out


def nchw_ref(buf, C, coff, mistake=None, sentinel=None):
    """NHWC [B, H, W, cs] of the type -> NCHW f32 of channels [coff, coff + C): a slice, a permute and an exact widening"""
    B, H, W, _ = buf.shape
    out = buf[..., coff:coff + C].permute(0, 3, 1, 2).float().clone(memory_format=torch.contiguous_format)
    if mistake == "hw_exchanged":
        out = out.transpose(2, 3).reshape(B, C, H, W).contiguous()
    elif mistake == "channels_rotated":
        out = buf[..., coff + 1:coff + 1 + C].permute(0, 3, 1, 2).float().contiguous() if buf.shape[-1] > coff + C else out.roll(1, dims=1)
    elif mistake == "last_pixel_left":
        out[-1, :, -1, -1] = sentinel
    return out
