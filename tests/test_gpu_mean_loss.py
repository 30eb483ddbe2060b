"""GPU: srcgan_loss_fwd, srcgan_loss_bwd and srcgan_psnr_from_mse (csrc/elementwise.hip: loss_fwd_k<0..4>, loss_final_k, loss_bwd_k<0..4>,
psnr_k) straight through the C ABI, on the case tables of tests/mean_loss_ref.py:

  exact      small-integer operands, every length of LENGTHS, a at byte phase 0 / 4 / 8 / 12, b at the same and at another phase: the value
             has the bits of f32(S) * f32(1.0 / n); the gradients of kinds 0 and 4 have the bits of sign * g and label * g for gout 1, 3,
             -0.5 (a device scalar) and gscale +1 / -1, da at phase 0 and 4; sign(0) = 0.
  float64    reals (label 0.9, logits of scale 6 with +-100 planted): the value within (D + 4) 2^-24 mean|e|, the gradients of kinds 1 and 2
             within 5 * 2^-24 |ref64|, kind 3 within K 2^-24 N both ways; psnr within its bound, +inf at mse = 0.
  always     scratch is NaN on entry with a sentinel behind it, out lies between two sentinels, da between sentinels, a and b are compared
             with their copies afterwards, and a second call gives the same bits.
  refusals   a null pointer, n = 0, a kind outside 0..4, kinds 0 / 1 without b: an error, nothing launched, every sentinel intact.

Observed maxima are printed by the last test."""
import itertools

import numpy as np
import pytest
import torch

import mean_loss_ref as R

pytestmark = pytest.mark.gpu
SENT = -7777.0
PAD = 8
OBSERVED = {"value_over_D_plus_4": 0.0, "square_grad_of_5": 0.0, "bce_value_of_3": 0.0, "bce_grad_of_12": 0.0, "psnr_of_3": 0.0}
PHASE_PAIRS = ((0, 0), (4, 4), (0, 4), (4, 0))          # (byte phase of a, of da) of the backward calls
_REF = {}


def _N():
    from srcgan_amd import _native as N
    return N


class Placed:
    """A device copy of ``a`` at byte phase ``phase`` of a 16-byte aligned buffer, sentinels in front of and behind it."""

    def __init__(self, a, phase, fill=None):
        off = PAD + phase // 4
        n = len(a) if fill is None else a
        self.buf = torch.full((off + n + PAD,), SENT, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[off:off + n]
        if fill is None:
            self.host = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
            self.view.copy_(self.host)
        else:
            self.view.fill_(fill)
        self.off, self.n = off, n
        assert self.view.data_ptr() % 16 == phase

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.off] == SENT).all() and (self.buf[self.off + self.n:] == SENT).all())

    def unchanged(self):
        return torch.equal(self.view.cpu(), self.host)


class Buffers:
    """scratch (NaN, a sentinel behind it) and out (a scalar between two sentinels)."""

    def __init__(self):
        self.ns = _N().lib().srcgan_loss_scratch_floats()
        self.scratch = Placed(self.ns, 0, fill=float("nan"))
        self.out = Placed(1, 4, fill=float("nan"))

    def reset(self):
        self.scratch.view.fill_(float("nan"))
        self.out.view.fill_(float("nan"))

    def intact(self):
        return self.scratch.guards_intact() and self.out.guards_intact()


def _fwd(kind, a, b, label, n, bufs):
    N = _N()
    N.check(N.lib().srcgan_loss_fwd(kind, a.ptr(), None if b is None else b.ptr(), float(label), n, bufs.out.ptr(), bufs.scratch.ptr(),
                                    N.stream_ptr()), "srcgan_loss_fwd")
    return bufs.out.view.cpu().numpy().copy()


def _bwd(kind, a, b, label, n, gout, gscale, pda):
    N = _N()
    da = Placed(n, pda, fill=float("nan"))
    g = torch.full((), gout, dtype=torch.float32, device="cuda")
    N.check(N.lib().srcgan_loss_bwd(kind, a.ptr(), None if b is None else b.ptr(), float(label), n, g.data_ptr(), float(gscale), da.ptr(),
                                    N.stream_ptr()), "srcgan_loss_bwd")
    assert da.guards_intact(), "srcgan_loss_bwd wrote outside da"
    assert float(g) == gout
    return da.view.cpu().numpy()


def _placements(kind, a, b):
    """Every (pa, pb, placed a, placed b) of the forward table: a at the four phases, b (kinds 0, 1) at the same and at the next phase."""
    pa_bufs = {p: Placed(a, p) for p in R.A_PHASES}
    pb_bufs = {p: Placed(b, p) for p in R.A_PHASES} if kind < 2 else {}
    for pa in R.A_PHASES:
        if kind < 2:
            for pb in (pa, (pa + 4) % 16):
                yield pa, pb, pa_bufs[pa], pb_bufs[pb]
        else:
            yield pa, None, pa_bufs[pa], None


def _bwd_grid(n):
    """(gout, gscale, pa, pda): the full cross at the small lengths, every (gout, gscale) once over rotating phases at the large ones."""
    combos = list(itertools.product(R.GOUTS, R.GSCALES))
    if n <= 1027:
        return [(go, gs, pa, pda) for go, gs in combos for pa, pda in PHASE_PAIRS]
    return [(go, gs) + PHASE_PAIRS[i % len(PHASE_PAIRS)] for i, (go, gs) in enumerate(combos)]


def _ids(kinds):
    return [pytest.param(k, n, id=f"{R.KIND_NAMES[k]}-{n}") for k in kinds for n in R.LENGTHS]


@pytest.mark.parametrize("kind,n", _ids(R.EXACT_KINDS))
def test_exact_on_small_integers(kind, n):
    a, b = R.exact_inputs(kind, n)
    bufs = Buffers()
    for label in R.EXACT_RANGE[kind][1]:
        ref = R.forward(kind, a, b, label)
        for pa, pb, pa_buf, pb_buf in _placements(kind, a, b):
            bufs.reset()
            got = _fwd(kind, pa_buf, pb_buf, label, n, bufs)
            assert R.exact_forward_ok(kind, n, got, ref), (kind, n, label, pa, pb, got, R.exact_value(ref["sum"], n))
            assert bufs.intact(), (kind, n, pa, pb)
            bufs.reset()
            assert _fwd(kind, pa_buf, pb_buf, label, n, bufs).tobytes() == got.tobytes()
            assert pa_buf.unchanged() and pa_buf.guards_intact() and (pb_buf is None or (pb_buf.unchanged() and pb_buf.guards_intact()))
        if kind not in (0, 4):
            continue
        at = {p: (Placed(a, p), Placed(b, p) if kind < 2 else None) for p in (0, 4)}
        want = {}
        for gout, gscale, pa, pda in _bwd_grid(n):
            if (gout, gscale) not in want:
                want[gout, gscale] = R.backward(kind, a, b, label, gout, gscale, dt=np.float32)["grad"]
            pa_buf, pb_buf = at[pa]
            got = _bwd(kind, pa_buf, pb_buf, label, n, gout, gscale, pda)
            assert R.exact_backward_ok(got, want[gout, gscale]), (kind, n, label, gout, gscale, pa, pda)
            if kind == 0:
                assert np.all(got[a == b] == 0), "sign(0) must be 0"
        for pa_buf, pb_buf in at.values():
            assert pa_buf.unchanged() and (pb_buf is None or pb_buf.unchanged())


@pytest.mark.parametrize("kind,n", _ids(R.KINDS))
def test_reals_against_float64(kind, n):
    a, b = R.real_inputs(kind, n)
    bufs = Buffers()
    for real in ((True, False) if kind == 4 else (True,)):       # kinds 2 and 3: the label 0.9; kind 4: -1 and +1
        label = R.real_label(kind, real)
        ref = R.forward(kind, a, b, label)
        for pa, pb, pa_buf, pb_buf in _placements(kind, a, b):
            bufs.reset()
            got = _fwd(kind, pa_buf, pb_buf, label, n, bufs)
            u, allowed, un = R.value_units(kind, n, got[0], ref, pa, pb)
            print(f"[mean_loss] value {R.KIND_NAMES[kind]} n={n} label={label} phases a={pa} b={pb}: {u:.2f} of D + 4 = {allowed}"
                  + (f", {un:.2f} of K = {R.K_BCE_VALUE:.0f}" if kind == 3 else ""))
            OBSERVED["value_over_D_plus_4"] = max(OBSERVED["value_over_D_plus_4"], u / allowed)
            if kind == 3:
                OBSERVED["bce_value_of_3"] = max(OBSERVED["bce_value_of_3"], un)
            assert R.value_ok(kind, n, got, ref, pa, pb), (kind, n, label, pa, pb, got, ref["loss"])
            assert bufs.intact() and pa_buf.unchanged() and (pb_buf is None or pb_buf.unchanged())
            bufs.reset()
            assert _fwd(kind, pa_buf, pb_buf, label, n, bufs).tobytes() == got.tobytes()
        at = {p: (Placed(a, p), Placed(b, p) if kind < 2 else None) for p in (0, 4)}
        refs = {}
        for gout, gscale, pa, pda in _bwd_grid(n):
            pa_buf, pb_buf = at[pa]
            got = _bwd(kind, pa_buf, pb_buf, label, n, gout, gscale, pda)
            if kind in (0, 4):                               # sign * g and label * g: exact on any operands
                if (gout, gscale) not in refs:
                    refs[gout, gscale] = R.backward(kind, a, b, label, gout, gscale, dt=np.float32)["grad"]
                assert R.exact_backward_ok(got, refs[gout, gscale]), (kind, n, gout, gscale, pa, pda)
                continue
            if (gout, gscale) not in refs:
                refs[gout, gscale] = R.backward(kind, a, b, label, gout, gscale)
            r = refs[gout, gscale]
            u = R.grad_units(kind, got, r)
            key = "bce_grad_of_12" if kind == 3 else "square_grad_of_5"
            OBSERVED[key] = max(OBSERVED[key], u)
            print(f"[mean_loss] gradient {R.KIND_NAMES[kind]} n={n} label={label} gout={gout} gscale={gscale} phases a={pa} da={pda}: "
                  f"{u:.2f} of K = {R.K_BCE_GRAD if kind == 3 else R.K_SQUARE_GRAD:.0f}")
            assert R.grad_ok(kind, got, r), (kind, n, label, gout, gscale, pa, pda, u)
        for pa_buf, pb_buf in at.values():
            assert pa_buf.unchanged() and (pb_buf is None or pb_buf.unchanged())


def test_psnr_from_mse():
    N = _N()
    for mse in R.PSNR_MSE + (0.0,):
        m = Placed(np.array([mse], np.float32), 4)
        out = Placed(1, 8, fill=float("nan"))
        N.check(N.lib().srcgan_psnr_from_mse(m.ptr(), out.ptr(), N.stream_ptr()), "srcgan_psnr_from_mse")
        got = out.view.cpu().numpy()[0]
        assert out.guards_intact() and m.unchanged() and m.guards_intact()
        if mse == 0.0:
            assert got == np.inf
            continue
        u = abs(np.float64(got) - R.psnr(mse)) / (R.psnr_bound(mse) / R.K_PSNR)
        print(f"[mean_loss] psnr mse={mse}: {got!r} against {R.psnr(mse)!r}, {u:.2f} of K = {R.K_PSNR:.0f}")
        OBSERVED["psnr_of_3"] = max(OBSERVED["psnr_of_3"], u)
        assert R.psnr_ok(mse, got), (mse, got)
    assert N.lib().srcgan_psnr_from_mse(None, out.ptr(), N.stream_ptr()) != 0 and b"null pointer" in N.lib().srcgan_last_error()
    assert N.lib().srcgan_psnr_from_mse(m.ptr(), None, N.stream_ptr()) != 0


def test_refusals_launch_nothing():
    N = _N()
    lib, st = N.lib(), N.stream_ptr()
    n = 1027
    a, b = R.real_inputs(0, n)
    pa, pb = Placed(a, 0), Placed(b, 0)
    bufs = Buffers()
    da = Placed(n, 0, fill=float("nan"))
    g = torch.full((), 1.0, device="cuda")
    o, s = bufs.out.ptr(), bufs.scratch.ptr()
    fwd_bad = [((0, None, pb.ptr(), 0.0, n, o, s, st), b"bad arguments"), ((0, pa.ptr(), pb.ptr(), 0.0, n, None, s, st), b"bad arguments"),
               ((0, pa.ptr(), pb.ptr(), 0.0, n, o, None, st), b"bad arguments"), ((0, pa.ptr(), pb.ptr(), 0.0, 0, o, s, st), b"bad arguments"),
               ((-1, pa.ptr(), pb.ptr(), 0.0, n, o, s, st), b"bad arguments"), ((5, pa.ptr(), pb.ptr(), 0.0, n, o, s, st), b"bad arguments"),
               ((0, pa.ptr(), None, 0.0, n, o, s, st), b"needs b"), ((1, pa.ptr(), None, 0.0, n, o, s, st), b"needs b")]
    for args, msg in fwd_bad:
        assert lib.srcgan_loss_fwd(*args) != 0, args
        assert b"srcgan_loss_fwd" in lib.srcgan_last_error() and msg in lib.srcgan_last_error(), (args, lib.srcgan_last_error())
    d = da.ptr()
    bwd_bad = [((0, None, pb.ptr(), 0.0, n, g.data_ptr(), 1.0, d, st), b"bad arguments"), ((0, pa.ptr(), pb.ptr(), 0.0, n, None, 1.0, d, st), b"bad arguments"),
               ((0, pa.ptr(), pb.ptr(), 0.0, n, g.data_ptr(), 1.0, None, st), b"bad arguments"), ((0, pa.ptr(), pb.ptr(), 0.0, 0, g.data_ptr(), 1.0, d, st), b"bad arguments"),
               ((-1, pa.ptr(), pb.ptr(), 0.0, n, g.data_ptr(), 1.0, d, st), b"bad arguments"), ((5, pa.ptr(), pb.ptr(), 0.0, n, g.data_ptr(), 1.0, d, st), b"bad arguments"),
               ((0, pa.ptr(), None, 0.0, n, g.data_ptr(), 1.0, d, st), b"needs b"), ((1, pa.ptr(), None, 0.0, n, g.data_ptr(), 1.0, d, st), b"needs b")]
    for args, msg in bwd_bad:
        assert lib.srcgan_loss_bwd(*args) != 0, args
        assert b"srcgan_loss_bwd" in lib.srcgan_last_error() and msg in lib.srcgan_last_error(), (args, lib.srcgan_last_error())
    torch.cuda.synchronize()
    assert bufs.intact() and da.guards_intact() and pa.unchanged() and pb.unchanged()
    assert torch.isnan(bufs.out.view).all() and torch.isnan(bufs.scratch.view).all() and torch.isnan(da.view).all()      # nothing ran
    for kind in (2, 3, 4):                                   # the label kinds take no b
        assert lib.srcgan_loss_fwd(kind, pa.ptr(), None, 0.5, n, o, s, st) == 0


def test_zz_report_observed_maxima():
    print("[mean_loss] observed maxima (fraction of D + 4 for the value, units of 2^-24 N otherwise):", {k: round(v, 3) for k, v in OBSERVED.items()})
    assert OBSERVED["value_over_D_plus_4"] <= 1 and OBSERVED["square_grad_of_5"] <= R.K_SQUARE_GRAD
    assert OBSERVED["bce_value_of_3"] <= R.K_BCE_VALUE and OBSERVED["bce_grad_of_12"] <= R.K_BCE_GRAD and OBSERVED["psnr_of_3"] <= R.K_PSNR
