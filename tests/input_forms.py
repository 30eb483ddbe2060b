"""The forms a user tensor arrives in, and the table of public front ends that take one (tests/test_gpu_input_forms.py).

A form builds, from contiguous values ``x``, a leaf ``base`` and a view of it that holds ``x``:

    phase4      flat[1:].view(shape): contiguous, data_ptr() % 16 == 4 (one element past a 16-byte boundary for u8)
    batch       big[1:], one sample more in front
    wslice      big[..., 1:-1], one column more on each side (not contiguous)
    chlast      a permute of an allocation with the channels last (not contiguous)
    expand      a stride-0 expand of one channel to three
    bf16, fp16  16-bit tensors; the values are multiples of 1/16 below 2, representable in both
    nonleaf     (base * 1.0)[1:] of a base that requires grad

The rule for every subject and form: the result has the bits of the same call on a fresh contiguous f32 clone; the gradient that reaches
``base`` is the clone's gradient placed into the base through the view (zeros elsewhere; summed over the expanded channel; cast once for
16-bit), in the base's shape and dtype; the base is unchanged.

Exemption.  The flat reductions (csrc/elementwise.hip srcgan_loss_fwd, csrc/class_losses.hip) read a scalar head up to the first 16-byte
boundary, 16-byte groups and a scalar tail, so the ORDER of their f32 summation depends on the pointer phase: a view at phase 4 sums in
another order than its clone at phase 0.  Their values are held to equality on operands of the 1/16 grid where every partial sum is
exact (not FLoss / CELoss: logarithms), and on reals to the family's float64 bound (mean_loss_ref / class_losses_ref).  Their gradients
are element-wise and stay under the rule."""
import math

import numpy as np
import torch

import class_losses_ref as CR
import mean_loss_ref as MR

DEV = "cuda"
FORMS = ("phase4", "batch", "wslice", "chlast", "expand", "bf16", "fp16", "nonleaf")
PHASE_FORMS = ("phase4", "batch", "nonleaf")            # the view's own storage reaches the kernel: its phase decides the summation order
FILL = 0.5                                               # what the base holds outside the view


class Form:
    def __init__(self, name, x, cdim=1):
        """x: contiguous values on the device (f32, or u8 for the 8-bit subjects)."""
        self.name, self.cdim, S = name, cdim, tuple(x.shape)
        dt = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(name, x.dtype)
        new = lambda *shape: torch.full(shape, FILL if x.dtype != torch.uint8 else 7, dtype=dt, device=x.device)
        if name == "phase4":
            self.base, self.place = new(x.numel() + 1), (lambda b: b[1:].view(S))
        elif name in ("batch", "nonleaf"):
            self.base, self.place = new(S[0] + 1, *S[1:]), (lambda b: b[1:])
        elif name == "wslice":
            self.base, self.place = new(*S[:-1], S[-1] + 2), (lambda b: b[..., 1:-1])
        elif name == "chlast":
            c = cdim % len(S)
            self.base, self.place = new(*S[:c], *S[c + 1:], S[c]), (lambda b: b.movedim(-1, c))
        elif name == "expand":
            one = list(S)
            one[cdim] = 1
            self.base, self.place = new(*one), (lambda b: b.expand(S))
        else:
            self.base, self.place = new(*S), (lambda b: b)
        with torch.no_grad():
            if name == "expand":
                self.base.copy_(x.narrow(cdim, 0, 1))
            else:
                self.place(self.base).copy_(x)
        self.before = self.base.clone()

    def view(self, requires_grad):
        """The tensor the user passes: a view of the base (through ``* 1.0`` for the non-leaf form)."""
        if not (requires_grad and self.base.dtype.is_floating_point):
            return self.place(self.base)
        self.base.requires_grad_(True)
        return self.place(self.base * 1.0 if self.name == "nonleaf" else self.base)

    def clone(self):
        """The baseline's input: a fresh contiguous clone, f32 for the float forms."""
        v = self.place(self.before).detach()
        return (v.float() if v.dtype.is_floating_point else v).contiguous().clone()

    def expected_grad(self, g):
        """The clone's gradient ``g`` as it must arrive in the base."""
        if self.name == "expand":
            return g.sum(dim=self.cdim, keepdim=True).to(self.base.dtype)
        e = torch.zeros_like(self.base)
        self.place(e).copy_(g.to(self.base.dtype))
        return e

    def unchanged(self):
        return torch.equal(self.base.detach(), self.before)


def values(shape, seed, grid, lo=0, hi=31, u8=False):
    """f32 values in [lo / 16, hi / 16]: uniform reals, or multiples of 1/16 (``grid``); u8: bytes."""
    g = torch.Generator().manual_seed(1000 + seed)
    if u8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(DEV)
    if grid:
        return (torch.randint(lo, hi + 1, shape, generator=g).float() / 16).to(DEV)
    return (lo / 16 + torch.rand(shape, generator=g) * ((hi - lo) / 16)).to(DEV)


class Subject:
    """One public front end.  ``make()`` -> a callable of the user tensors returning a tensor, a tuple or a dict of tensors;
    ``shapes``: one per user tensor; ``grad``: the arguments whose gradient is checked; ``cdim``: the channel dimension; ``three``:
    takes three channels (the expand form applies); ``lo, hi``: value range in sixteenths; ``exempt``: why bit equality of the VALUE
    does not hold across pointer phases (None: it holds), with ``exact_on_grid`` and ``bound(arrays, phases)`` -> (float64 value,
    allowed error); ``refuse16``: (exception, words of the message) where 16-bit input is a documented refusal; ``u8``: 8-bit input."""

    def __init__(self, name, make, shapes, grad=(), cdim=1, three=False, lo=0, hi=31, exempt=None, exact_on_grid=True, bound=None,
                 refuse16=None, u8=False, skip_forms=()):
        self.name, self.make, self.shapes, self.grad, self.cdim, self.three = name, make, shapes, grad, cdim, three
        self.lo, self.hi, self.exempt, self.exact_on_grid, self.bound = lo, hi, exempt, exact_on_grid, bound
        self.refuse16, self.u8, self.skip_forms = refuse16, u8, skip_forms

    def forms(self):
        out = []
        for f in FORMS:
            if f in self.skip_forms or (f == "expand" and not self.three) or (f in ("bf16", "fp16") and self.u8):
                continue
            if f == "chlast" and any(len(s) < 3 for s in self.shapes):
                continue
            out.append(f)
        return out


# ------------------------------------------------------------------------------------------------ float64 bounds of the exempt subjects
PHASE_REASON = "flat reduction: scalar head / 16-byte groups / tail, so the f32 summation order follows the pointer phase"


def _mean_bound(kind, label=0.0):
    def bound(arrays, phases):
        a = arrays[0].reshape(-1)
        b = arrays[1].reshape(-1) if kind < 2 else None
        ref = MR.forward(kind, a, b, label)
        pa, pb = phases[0], (phases[1] if kind < 2 else None)
        return ref["loss"], MR.value_bound(kind, len(a), ref, pa, pb)
    return bound


def _psnr_bound(arrays, phases):
    mse, allowed = _mean_bound(1)(arrays, phases)
    return float(MR.psnr(np.float32(mse))), 10.0 / math.log(10.0) * (allowed + 2.0 ** -24 * mse) / mse + MR.psnr_bound(mse)


def _class_bound(fn, q, **kw):
    def bound(arrays, phases):
        r = fn(*arrays, **kw)
        return r["loss"], float(CR.tolerance(q + "_loss", r["Nloss"]))
    return bound


# ------------------------------------------------------------------------------------------------ the table
IMG = (2, 3, 11, 13)            # 3 * 11 * 13 = 429 floats a sample: big[1:] lies at byte phase 4; 11 x 13 is the smallest the SSIM windows take
GRAY = (2, 1, 11, 13)
VOL = (2, 1, 3, 11, 13)


def _losses():
    from srcgan_amd import losses as L
    return L


def _gan(mode, real):
    def make():
        crit = _losses().GANLoss(mode, device=DEV)
        return lambda x: crit(x, real)
    return make


def _vgg(cls, kind, **kw):
    def make():
        import vgg_ref
        m = getattr(_losses(), cls)(weights=vgg_ref.seeded_state(kind), dtype="fp32", **kw)
        return m.to(DEV)
    return make


def _metric(name, **kw):
    def make():
        from srcgan_amd import metrics
        m = getattr(metrics, name)()
        return lambda p, t: m(p, t, **kw)
    return make


def _score_scene():
    from srcgan_amd import metrics
    return lambda p, t: metrics.score_scene(p, t, full=True)


def _op(name, *args):
    def make():
        from srcgan_amd import ops
        return lambda x: getattr(ops, name)(x, *args)
    return make


def _data(name):
    def make():
        from srcgan_amd import data
        return getattr(data, name)
    return make


def _net(build):
    def make():
        import srcgan_amd
        torch.manual_seed(5)
        return build(srcgan_amd).to(DEV)
    return make


def _upscale():
    import srcgan_amd
    from srcgan_amd import infer
    torch.manual_seed(6)
    net = srcgan_amd.ESPCN(1, 1, 2).to(DEV).eval()
    return lambda scene: infer.upscale_scene(net, scene, up=2, tile=16)


def _nearest_crop():
    ns = _losses().NearestSelector(2, 1)
    return lambda o, t: ns.crop(o, t)


SCENE16 = (ValueError, "must be")
SUBJECTS = [
    # ---- losses.__all__
    Subject("L1Loss", lambda: _losses().L1Loss(), (IMG, IMG), grad=(0, 1), three=True, exempt=PHASE_REASON, bound=_mean_bound(0)),
    Subject("MSELoss", lambda: _losses().MSELoss(), (IMG, IMG), grad=(0, 1), three=True, exempt=PHASE_REASON, bound=_mean_bound(1)),
    Subject("PSNRLoss", lambda: _losses().PSNRLoss(), (IMG, IMG), three=True, exempt=PHASE_REASON, bound=_psnr_bound),
    Subject("GANLoss-lsgan-real", _gan("lsgan", True), (IMG,), grad=(0,), three=True, exempt=PHASE_REASON, bound=_mean_bound(2, 1.0)),
    Subject("GANLoss-lsgan-fake", _gan("lsgan", False), (IMG,), grad=(0,), three=True, exempt=PHASE_REASON, bound=_mean_bound(2, 0.0)),
    Subject("GANLoss-vanilla-real", _gan("vanilla", True), (IMG,), grad=(0,), three=True, exempt=PHASE_REASON, exact_on_grid=False,
            bound=_mean_bound(3, 1.0)),
    Subject("GANLoss-wgangp-fake", _gan("wgangp", False), (IMG,), grad=(0,), three=True, exempt=PHASE_REASON, bound=_mean_bound(4, 1.0)),
    Subject("DSSIMLoss", lambda: _losses().DSSIMLoss(), (IMG, IMG), grad=(0, 1), three=True),
    Subject("VGG16Loss", _vgg("VGG16Loss", 0), ((1, 3, 16, 16), (1, 3, 16, 16)), grad=(0,), three=True),
    Subject("PerceptionLoss", _vgg("PerceptionLoss", 1), ((1, 3, 16, 16), (1, 3, 16, 16)), grad=(0,), three=True),
    Subject("NearestSelector.crop", lambda: _nearest_crop(), (IMG, IMG), three=True),
    Subject("NearestL1Loss", lambda: _losses().NearestL1Loss(2, 1), (IMG, IMG), grad=(0, 1), three=True),
    Subject("L1Loss3D", lambda: _losses().L1Loss3D(), (VOL, VOL), grad=(0, 1), exempt=PHASE_REASON, bound=_mean_bound(0)),
    Subject("DSSIMLoss3D", lambda: _losses().DSSIMLoss3D(), (VOL, VOL), grad=(0, 1)),
    Subject("VGG16Loss3D", _vgg("VGG16Loss3D", 0, frames_per_pass=1), ((1, 3, 2, 16, 16), (1, 3, 2, 16, 16)), grad=(0,), three=True),
    Subject("FLoss", lambda: _losses().FLoss(), ((3, 1, 5, 7), (3, 1, 5, 7)), grad=(0,), lo=1, hi=15, exempt=PHASE_REASON, exact_on_grid=False,
            bound=_class_bound(CR.focal, "focal")),
    Subject("CELoss-binary", lambda: _losses().CELoss(), ((3, 1, 5, 7), (3, 1, 5, 7)), grad=(0,), lo=1, hi=15, exempt=PHASE_REASON,
            exact_on_grid=False, bound=_class_bound(CR.bce, "bce")),
    Subject("CELoss-classes", lambda: _losses().CELoss(), ((3, 4, 5, 7), (3, 4, 5, 7)), grad=(0,), lo=1, hi=15, exempt=PHASE_REASON,
            exact_on_grid=False, bound=_class_bound(CR.nll, "nll")),
    Subject("ConLoss", lambda: _losses().ConLoss(), ((3, 3, 5, 7),), grad=(0,), three=True, exempt=PHASE_REASON,
            bound=_class_bound(CR.batch_range, "range")),
    Subject("CrossLoss", lambda: _losses().CrossLoss(), ((3, 3, 5, 7), (3, 3, 5, 7)), grad=(0,), three=True, exempt=PHASE_REASON,
            bound=_class_bound(CR.cross, "cross")),
    # ---- metrics
    Subject("metrics.AE", _metric("AE"), (IMG, IMG), three=True),
    Subject("metrics.MSE", _metric("MSE"), (IMG, IMG), three=True, exempt=PHASE_REASON, bound=_mean_bound(1)),
    Subject("metrics.PSNR", _metric("PSNR"), (IMG, IMG), three=True, exempt=PHASE_REASON, bound=_psnr_bound),
    Subject("metrics.SSIM", _metric("SSIM", full=True), (IMG, IMG), three=True),
    Subject("metrics.score_scene", _score_scene, ((1, 3, 11, 13), (1, 3, 11, 13)), three=True, refuse16=SCENE16),
    # ---- ops
    Subject("ops.rgb_to_gray", _op("rgb_to_gray"), ((2, 3, 5, 7),), three=True),
    Subject("ops.bilinear_down", _op("bilinear_down", 2), ((2, 1, 6, 10),)),
    Subject("ops.bilinear_up", _op("bilinear_up", 2), ((2, 1, 5, 7),)),
    Subject("ops.nearest_resize", _op("nearest_resize", 2), ((2, 3, 5, 7),), three=True),
    Subject("ops.to_nhwc", _op("to_nhwc", 8), ((2, 3, 5, 7),), three=True),
    Subject("ops.to_nchw", _op("to_nchw"), ((2, 5, 7, 8),), cdim=3),
    # ---- data
    Subject("data.arr2gray", _data("arr2gray"), ((2, 5, 7, 3),), cdim=3, three=True, u8=True),
    Subject("data.arr2rgb", _data("arr2rgb"), ((2, 5, 7, 3),), cdim=3, three=True, u8=True),
    Subject("data.arr2lab", _data("arr2lab"), ((2, 5, 7, 3),), cdim=3, three=True, u8=True),
    Subject("data.arr2ab", _data("arr2ab"), ((2, 5, 7, 3),), cdim=3, three=True, u8=True),
    Subject("data.lab2img", _data("lab2img"), ((2, 3, 5, 7),), three=True, hi=16, refuse16=(ValueError, "expected float32")),
    # ---- infer
    Subject("infer.upscale_scene", _upscale, ((1, 1, 20, 24),), refuse16=(ValueError, "the scene must be")),
    # ---- one network per autograd Function class of model.py
    Subject("RDDBNet", _net(lambda m: m.RDDBNet(3, 3, 2, nf=16, nb=1, gc=8)), ((2, 3, 6, 7),), grad=(0,), three=True),
    Subject("NLayerDiscriminator", _net(lambda m: m.NLayerDiscriminator(3, 16, 2)), ((2, 3, 16, 18),), grad=(0,), three=True),
    Subject("ESPCN", _net(lambda m: m.ESPCN(1, 1, 2)), ((2, 1, 6, 7),), grad=(0,)),
    Subject("EDSR", _net(lambda m: m.EDSR(1, 1, 2, base_channel=32, num_residuals=1)), ((2, 1, 6, 7),), grad=(0,)),
]
BY_NAME = {s.name: s for s in SUBJECTS}
CASES = [(s.name, f) for s in SUBJECTS for f in s.forms()]
