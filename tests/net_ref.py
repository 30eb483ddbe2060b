"""What the float64 restatements of the network families (tests/*_ref.py) share, in one place: the fixtures' count sketch, the storage
rounding, PixelShuffle, the relative L2 measure, the one runner (forward, L1 loss, backward -> gradients), the tile stitcher behind the
receptive-halo tests and the parts of the fixture comparison that are the same for every family.  CPU only, torch and numpy; the
fixture generators (tests/golden/make_golden_*.py) import the restatements outside pytest, so nothing here needs the package."""
import numpy as np
import torch

BIG = 2048          # a gradient of more elements is kept as sketch + first slice


def sketch(t):
    """The fixtures' 64-bucket count sketch of a flattened tensor, in float64 (tests/golden/make_golden_srdense.py): element i goes to
    bucket i mod 64 with the sign of a fixed integer hash of i.  Equal tensors have equal sketches, bit for bit; the relative error of two
    sketches estimates the relative L2 error of the tensors."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    v = np.asarray(t, dtype=np.float64).reshape(-1)
    i = np.arange(v.size, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    sign = 1.0 - 2.0 * ((h >> np.uint64(15)) & np.uint64(1)).astype(np.float64)
    out = np.zeros(64, dtype=np.float64)
    np.add.at(out, (i % np.uint64(64)).astype(np.int64), sign * v)
    return out


def first_slice(g):
    """what a fixture keeps of a gradient of more than BIG elements beside its sketch: its first 64 elements"""
    return g.reshape(-1)[:64]


def q(t, store):
    """The storage emulation: ``t`` rounded to the 16-bit torch dtype ``store`` (None: as it is), straight through -- the backward is
    the exact one of the rounded forward."""
    if store is None:
        return t
    return t + (t.to(store).to(t.dtype) - t).detach()


def pixel_shuffle(x, r):
    """y[c, r h + a, r w + b] = x[c r^2 + a r + b, h, w]"""
    B, Cr, H, W = x.shape
    C = Cr // (r * r)
    return x.reshape(B, C, r, r, H, W).permute(0, 1, 4, 2, 5, 3).reshape(B, C, r * H, r * W)


def rel_l2(a, b):
    a, b = torch.as_tensor(np.asarray(a), dtype=torch.float64), torch.as_tensor(np.asarray(b), dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def worst(errors):
    k = max(errors, key=errors.get)
    return k, errors[k]


def run_l1(forward, sd, x, target, *, frozen=(), loss_scale=1.0, missing="zero", dtype=torch.float64):
    """``forward(sd, x)``, mean L1 loss against ``target`` times ``loss_scale`` and backward, in ``dtype`` on the CPU ->
    (y, loss, dx, {name: gradient}).  ``frozen``: names, or a predicate on names, that take no gradient and have no entry.  A parameter
    the forward does not use reports a zero gradient (missing="zero") or has no entry (missing="absent", the reference's ``.grad`` of None)."""
    assert missing in ("zero", "absent")
    is_frozen = frozen if callable(frozen) else (lambda k: k in frozen)
    p = {k: v.detach().to(dtype).cpu().clone().requires_grad_(not is_frozen(k)) for k, v in sd.items()}
    xx = torch.as_tensor(x).detach().to(dtype).cpu().clone().requires_grad_(True)
    y = forward(p, xx)
    loss = (y - torch.as_tensor(target).detach().to(dtype).cpu()).abs().mean() * loss_scale
    loss.backward()
    live = {k: v for k, v in p.items() if not is_frozen(k)}
    if missing == "zero":
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in live.items()}
    else:
        grads = {k: v.grad for k, v in live.items() if v.grad is not None}
    return y.detach(), loss.detach(), xx.grad, grads


def stitch(forward, x, up, tile, halo):
    """Apply the tile plan with torch slicing: run ``forward`` on every tile and keep its core.  The plan is the package's; it is
    imported here, so the module itself needs no package."""
    from srcgan_amd import plan_tiles
    H, W = x.shape[2:]
    out = None
    for t in plan_tiles(H, W, tile, halo).tiles:
        y = forward(x[:, :, t.y0:t.y0 + t.th, t.x0:t.x0 + t.tw])
        if out is None:
            out = torch.full((1, y.shape[1], H * up, W * up), float("nan"), dtype=y.dtype)
        cy0, cy1, cx0, cx1 = t.core
        out[:, :, cy0 * up:cy1 * up, cx0 * up:cx1 * up] = y[:, :, (cy0 - t.y0) * up:(cy1 - t.y0) * up, (cx0 - t.x0) * up:(cx1 - t.x0) * up]
    return out


def fixture_head(z, y, loss, dx, suffix="", measure=None):
    """{"y", "loss", "dx": relative error} of a run against a fixture's float32 (suffix "") or float64 ("64") values: the part of every
    family's fixture comparison that does not depend on how the fixture lays out its gradients."""
    m = measure or rel_l2
    ref = float(z["loss" + suffix])
    return {"y": m(y, z["y" + suffix]), "loss": abs(float(loss) - ref) / abs(ref), "dx": m(dx, z["dx" + suffix])}


def keyed_grad_error(z, k, g, suffix="", measure=None):
    """The relative error of gradient ``g`` of parameter ``k`` against a fixture with one entry per parameter (MDSR, VDSR,
    ResnetGenerator): ``grad/k`` whole where the fixture holds it, else through ``gsketch/k`` and the first output-channel slice ``gslice/k``."""
    m = measure or rel_l2
    g = g.detach().double().cpu()
    if "grad" + suffix + "/" + k in z:
        return m(g, z["grad" + suffix + "/" + k])
    return max(m(sketch(g.numpy()), z["gsketch" + suffix + "/" + k]), m(g[0], z["gslice" + suffix + "/" + k]))
