"""float64 numpy restatement of the shift search behind NearestSelector / NearestL1Loss, the test data that goes with it, and the
single-mistake variants (``defect=``) that tests/test_nearest_teeth.py feeds to the GPU tests' comparisons.

    sd = shift*stride, ch = H - 2 sd, cw = W - 2 sd, n = 2*shift
    diff[b, i*n + j] = sum_{c, y < ch, x < cw} | target[b, c, i*stride + y, j*stride + x] - output[b, c, sd + y, sd + x] |
    k*[b] = FIRST index of the minimum of diff[b, :];  (r, c) = (k* // n, k* % n)
    output_ = output[:, :, sd : sd+ch, sd : sd+cw];  target_[b] = target[b, :, r*stride : r*stride+ch, c*stride : c*stride+cw]

This is the reference's NearestSelector (src/losses.py:199-255) with integer division in ``unravel_index`` and ``cw`` as the target
window's column extent.  No kernel runs here."""
import numpy as np
import torch

DEFECTS = ("rc_swapped", "candidate_off_by_one", "last_minimum", "stride_ignored", "edge_row_dropped", "apron_short", "crop_row_for_columns")

# (B, C, H, W, shift, stride) of the GPU tests.  The search tiles a crop plane 32 rows x 64 columns: 37 x 71 gives a 33 x 67 crop (one row
# past a tile, three columns past one), 36 x 68 exactly one tile.
TILE_H, TILE_W = 32, 64
SHAPES = {
    "tiny": (1, 1, 5, 5, 1, 1),              # a 3 x 3 crop, smaller than any tile; 4 candidates
    "golden": (3, 2, 12, 12, 2, 1),
    "nonsquare": (2, 3, 37, 71, 2, 1),       # crop 33 x 67: non-square and crossing a tile edge in both directions
    "one_tile": (1, 2, 36, 68, 2, 1),        # crop 32 x 64
    "stride2": (2, 1, 40, 40, 2, 2),
    "shift3": (2, 2, 30, 30, 3, 1),          # 36 candidates
    "tiles": (4, 3, 100, 100, 2, 1),         # 4 x 2 tiles per plane, a second stage over 24 partials in 4 blocks
}


def geometry(H, W, shift, stride):
    sd = shift * stride
    return sd, H - 2 * sd, W - 2 * sd, 2 * shift


def shift_diff(output, target, shift, stride, crop_h=None, crop_w=None, defect=None):
    """-> [B, n*n] float64"""
    o, t = np.asarray(output, np.float64), np.asarray(target, np.float64)
    H, W = o.shape[2:]
    sd, ch, cw, n = geometry(H, W, shift, stride)
    ch, cw = (ch if crop_h is None else crop_h), (cw if crop_w is None else crop_w)
    d = 1 if defect == "stride_ignored" else stride
    rows = ch - 1 if defect == "edge_row_dropped" else ch
    oc = o[:, :, sd:sd + rows, sd:sd + cw]
    out = np.zeros((o.shape[0], n * n))
    for i in range(n):
        for j in range(n):
            ii, jj = (i + 1, j) if defect == "candidate_off_by_one" else (i, j)
            win = t[:, :, ii * d:ii * d + rows, jj * d:jj * d + cw]
            if defect == "apron_short" and j == n - 1:       # the window's last column was never staged: the kernel would read what the
                win = win.copy()                             # column before it left there
                win[..., -1] = t[:, :, ii * d:ii * d + rows, jj * d + cw - 2]
            if win.shape != oc.shape:                        # candidate_off_by_one runs off the image for the last i
                out[:, i * n + j] = np.inf
                continue
            out[:, i * n + j] = np.abs(win - oc).sum(axis=(1, 2, 3))
    return out


def select(diff, n, defect=None):
    """-> [B, 2] int64 (r, c) of the first minimum"""
    diff = np.asarray(diff, np.float64)
    k = diff.shape[1] - 1 - np.argmin(diff[:, ::-1], axis=1) if defect == "last_minimum" else np.argmin(diff, axis=1)
    r, c = k // n, k % n
    return np.stack([c, r] if defect == "rc_swapped" else [r, c], axis=1).astype(np.int64)


def crops(output, target, shift, stride, sel=None, defect=None):
    """-> (output_, target_, sel); the crops keep the inputs' dtype (they are copies of input values)"""
    o, t = np.asarray(output), np.asarray(target)
    H, W = o.shape[2:]
    sd, ch, cw, n = geometry(H, W, shift, stride)
    if sel is None:
        sel = select(shift_diff(o, t, shift, stride, defect=defect), n, defect)
    d = 1 if defect == "stride_ignored" else stride
    wcols = ch if defect == "crop_row_for_columns" else cw
    out_ = o[:, :, sd:sd + ch, sd:sd + cw].copy()
    tgt_ = np.zeros((o.shape[0], o.shape[1], ch, wcols), t.dtype)
    for b, (r, c) in enumerate(sel):
        w = t[b, :, r * d:r * d + ch, c * d:c * d + wcols]
        tgt_[b, :, :w.shape[1], :w.shape[2]] = w
    return out_, tgt_, sel


def l1(output, target, shift, stride, gout=1.0, defect=None):
    """-> dict(loss, dout, dtgt, sel, diff): mean |output_ - target_| in float64, its full-size gradients (f64) times gout"""
    o, t = np.asarray(output, np.float64), np.asarray(target, np.float64)
    H, W = o.shape[2:]
    sd, ch, cw, n = geometry(H, W, shift, stride)
    diff = shift_diff(o, t, shift, stride, defect=defect)
    out_, tgt_, sel = crops(o, t, shift, stride, select(diff, n, defect), defect if defect != "crop_row_for_columns" else None)
    N = out_.size
    s = np.sign(out_ - tgt_) * (gout / N)
    dout, dtgt = np.zeros_like(o), np.zeros_like(t)
    dout[:, :, sd:sd + ch, sd:sd + cw] = s
    d = 1 if defect == "stride_ignored" else stride
    for b, (r, c) in enumerate(sel):
        dtgt[b, :, r * d:r * d + ch, c * d:c * d + cw] = -s[b]
    return {"loss": np.abs(out_ - tgt_).sum() / N, "dout": dout, "dtgt": dtgt, "sel": sel, "diff": diff}


# --------------------------------------------------------------------------- data
def int_case(name, seed):
    """operands in {0..15}: every partial sum is an exact integer below 2^24 in any order -> (output, target) float32 torch"""
    B, C, H, W, _, _ = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 16, (B, C, H, W), generator=g).float(), torch.randint(0, 16, (B, C, H, W), generator=g).float())


def float_case(name, seed, noise=0.05):
    """float16-representable reals: target uniform in [0, 1), the centre crop of output = a per-sample shifted window of target plus
    noise (a misregistered pair), the border of output uniform -> (output, target, planted [B,2]) float32 torch"""
    B, C, H, W, shift, stride = SHAPES[name]
    sd, ch, cw, n = geometry(H, W, shift, stride)
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(B, C, H, W, generator=g).half().float()
    o = torch.rand(B, C, H, W, generator=g)
    planted = torch.randint(0, n, (B, 2), generator=g)
    for b in range(B):
        r, c = (int(v) * stride for v in planted[b])
        o[b, :, sd:sd + ch, sd:sd + cw] = t[b, :, r:r + ch, c:c + cw] + noise * torch.randn(C, ch, cw, generator=g)
    return o.half().float(), t, planted


FLOAT_SEEDS = {"tiny": 11, "golden": 12, "nonsquare": 13, "one_tile": 14, "stride2": 15, "shift3": 16, "tiles": 17}
MARGIN = 1e-3


def margin(diff):
    """per sample (second best - best) / best of a float64 diff: above MARGIN an f32 rounding of the sums (the tests allow 1e-3 of
    the largest) cannot turn into another selection"""
    s = np.sort(np.asarray(diff, np.float64), axis=1)
    return (s[:, 1] - s[:, 0]) / np.maximum(s[:, 0], 1e-300)
