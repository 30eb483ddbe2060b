"""The D4 views of the geometric self-ensemble, restated in numpy straight from the index mapping of include/srcgan_amd.h, and the
sequential f32 average ``srcgan_d4_accumulate`` builds.  op = 0..7: t = op & 1 (transpose), fy = (op >> 1) & 1 (mirror the view's
rows), fx = (op >> 2) & 1 (mirror its columns);  view[y][x] = win[a][b],  y' = fy ? Hv - 1 - y : y,  x' = fx ? Wv - 1 - x : x,
(a, b) = (x', y') if t else (y', x').  The tests compare this with numpy's / torch's named transforms and the kernels with those."""
import numpy as np

OPS = {1: (0,), 2: (0, 4), 4: (0, 2, 4, 6), 8: tuple(range(8))}


def view_shape(op, th, tw):
    return (tw, th) if op & 1 else (th, tw)


def _index(op, th, tw):
    """(a, b): for every position (y, x) of the view, the window position it shows."""
    t, fy, fx = op & 1, (op >> 1) & 1, (op >> 2) & 1
    Hv, Wv = view_shape(op, th, tw)
    y, x = np.mgrid[0:Hv, 0:Wv]
    yp = Hv - 1 - y if fy else y
    xp = Wv - 1 - x if fx else x
    return (xp, yp) if t else (yp, xp)


def view(win, op):
    """The ``op`` view of ``win`` [..., th, tw]."""
    a, b = _index(op, *win.shape[-2:])
    return np.ascontiguousarray(win[..., a, b])


def fold(v, op, ah, aw):
    """The inverse: ``v`` [..., Hv, Wv] back to the identity orientation [..., ah, aw] (the mapping read in the other direction)."""
    if tuple(v.shape[-2:]) != view_shape(op, ah, aw):
        raise ValueError(f"a view of shape {tuple(v.shape[-2:])} under op {op} does not fold into {ah}x{aw}")
    a, b = _index(op, ah, aw)
    out = np.empty((*v.shape[:-2], ah, aw), v.dtype)
    out[..., a, b] = v
    return out


def average(folded):
    """acc = v0; acc = acc + v1; ...; the last addition is multiplied by 1 / V -- every step one f32 rounding, in the order given."""
    acc = np.asarray(folded[0], np.float32)
    for v in folded[1:]:
        acc = acc + np.asarray(v, np.float32)
    return acc * np.float32(1.0 / len(folded))


# the same view / fold with torch's named transforms, for tensors on any device (tests/test_d4_host.py ties them to the above)
def torch_view(win, op):
    import torch
    base = win.transpose(-1, -2) if op & 1 else win
    dims = [d for d, f in ((-2, op & 2), (-1, op & 4)) if f]
    return (torch.flip(base, dims) if dims else base).contiguous()


def torch_fold(v, op):
    import torch
    dims = [d for d, f in ((-2, op & 2), (-1, op & 4)) if f]
    base = torch.flip(v, dims) if dims else v
    return (base.transpose(-1, -2) if op & 1 else base).contiguous()


def torch_average(folded):
    acc = folded[0].clone()
    for v in folded[1:]:
        acc = acc + v
    return acc * (1.0 / len(folded))
