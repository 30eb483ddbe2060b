"""The comparisons of tests/test_gpu_param_kernels.py and tests/test_gpu_layout_kernels.py have teeth: on the CPU, on the very
inputs the GPU tests use, each reference (tests/param_kernels_ref.py) is compared, by the same check, with a copy of itself that
makes one of the mistakes those tests are there to catch.  Every such comparison must fail.  For Adam the bound is also shown
to be one the kernel's own formulas meet: numpy float32 evaluations, with every operation rounded and with each multiply-add
rounded once, stay under it on the same inputs.  No kernel runs here."""
import numpy as np
import pytest
import torch

import param_kernels_ref as R


# =========================================================================== fused Adam
def _adam_inputs(step):
    """Both groups the GPU test steps: the first step's, and the second step's layout (shifted gradients)"""
    return [R.adam_inputs(1000 + step % 997), R.adam_inputs(2000 + step % 997, grad_shift=3)]


def _breaks(k, sc_right, sc=None, mistake=None):
    """Does the mistaken reference leave the right one's bound somewhere, in p, m or v?"""
    ref, bound = R.adam_expected(k, sc_right)
    bad, _ = R.adam_expected(k, sc or sc_right, mistake)
    return {q: not R.adam_check(bad[q], ref[q], bound[q])[0] for q in "PMV"}


@pytest.mark.parametrize("lr", R.ADAM_LRS)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("betas", R.ADAM_BETAS)
def test_adam_float32_evaluations_meet_the_bound(betas, step, lr):
    """The kernel's formulas in float32, in three rounding orders, against the float64 reference on the GPU test's inputs"""
    worst = {q: 0.0 for q in "PMV"}
    for k, kk in zip(_adam_inputs(step), (step, step + 1)):
        sc = R.adam_scalars(lr, *betas, R.ADAM_EPS, kk)
        ref, bound = R.adam_expected(k, sc)
        for order in ("plain", "fma", "fma2"):
            got = {q: k[q].copy() for q in "PMV"}
            for n, o, go in zip(k["sizes"], k["offs"], k["goffs"]):
                got["P"][o:o + n], got["M"][o:o + n], got["V"][o:o + n] = R.adam_f32(k["P"][o:o + n], k["G"][go:go + n], k["M"][o:o + n], k["V"][o:o + n], sc, order)
            for q in "PMV":
                assert np.all(np.isfinite(got[q]))
                ok, ratio = R.adam_check(got[q], ref[q], bound[q])
                worst[q] = max(worst[q], ratio)
                assert ok, f"{q} {order}: worst error / bound {ratio}"
    print(f"[param] adam float32 b1={betas[0]} k={step} lr={lr}: worst error/bound p {worst['P']:.3f} m {worst['M']:.3f} v {worst['V']:.3f}")


def test_adam_inputs_cover_the_edges():
    k = R.adam_inputs(1001)
    assert {go % 4 for go in k["goffs"]} == {0, 1, 2, 3} and all(o % 4 == 0 for o in k["offs"])
    cat = lambda q, at: np.concatenate([k[q][a:a + n] for n, a in zip(k["sizes"], k[at])])
    P, G, M, V = cat("P", "offs"), cat("G", "goffs"), cat("M", "offs"), cat("V", "offs")
    sc = R.adam_scalars(1e-3, 0.9, 0.999, R.ADAM_EPS, 1000)
    _, _, v = R.adam_ref(P, G, M, V, sc)
    r = np.sqrt(v) / R.ADAM_EPS
    assert (r < 0.5).sum() > 100 and ((r > 0.5) & (r < 2)).sum() > 100 and (r > 100).sum() > 100      # sqrt(v) below, near, above eps
    assert ((G == 0) & (M == 0) & (V == 0)).sum() > 100 and ((G == M) & (G != 0)).sum() > 100
    assert (G == 0).sum() > 100 and (M == 0).sum() > 100 and (V == 0).sum() > 100 and (P == 0).sum() > 100
    nz = G[G != 0]
    assert np.abs(nz).min() >= 1e-15 and V[V != 0].min() >= 1e-30
    for q in "PMV":                                                       # sentinels on both sides of every tensor
        for n, o in zip(k["sizes"], k["offs"]):
            assert np.all(k[q][o - 4:o] == R.SENT) and np.all(k[q][o + n:o + n + 4] == R.SENT)


@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("betas", R.ADAM_BETAS)
def test_adam_bound_notices_wrong_arithmetic(betas, step):
    """Where a mistake changes a scalar at all, the reference evaluated with it leaves the bound.  eps inside the root, a missing
    bias correction: p, at lr > 0 (bias correction 2 at k = 1 in particular; the corrections are 1 to f32 at k = 100000, and
    bias correction 1 is 1 for beta1 = 0).  beta1 for 1 - beta1 (the same number for beta1 = 0.5): m.  b2 on g^2: v."""
    lr = 1e-3
    k = _adam_inputs(step)[0]
    sc = R.adam_scalars(lr, *betas, R.ADAM_EPS, step)
    assert not any(_breaks(k, sc).values())
    assert _breaks(k, sc, mistake="eps_in_sqrt")["P"]
    wrong = lambda m: R.adam_scalars(lr, *betas, R.ADAM_EPS, step, m)
    if step <= 1000:
        assert wrong("no_bc2")["c"] != sc["c"] and _breaks(k, sc, wrong("no_bc2"))["P"]
    if wrong("no_bc1")["s"] != sc["s"]:
        assert step <= 1000 and betas[0] > 0 and _breaks(k, sc, wrong("no_bc1"))["P"]
    else:
        assert betas[0] == 0 or step >= 1000
    if betas[0] != 0.5:
        assert _breaks(k, sc, wrong("beta1_as_weight"))["M"]
    assert _breaks(k, sc, wrong("beta2_on_g2"))["V"]
    # at lr = 0 the parameters must not move at all: any update leaves the bound 2U |p|
    sc0 = R.adam_scalars(0.0, *betas, R.ADAM_EPS, step)
    assert _breaks(k, sc0, sc)["P"]


@pytest.mark.parametrize("lr", R.ADAM_LRS)
def test_adam_check_notices_misplaced_elements(lr):
    """The last element of a tensor or of a 4096-chunk left at its old values, and element n (the first sentinel) updated"""
    for betas in R.ADAM_BETAS:
        for k in _adam_inputs(10):
            sc = R.adam_scalars(lr, *betas, R.ADAM_EPS, 10)
            for mistake in R.ELEMENT_MISTAKES:
                b = _breaks(k, sc, mistake=mistake)
                assert b["M"] and b["V"] and (b["P"] or lr == 0), (betas, mistake)     # at lr = 0 an old p is the right p
    # every tensor on its own: skipping the last element of ANY tensor shows (in v wherever g != 0 or v0 != 0)
    k = R.adam_inputs(1010)
    sc = R.adam_scalars(lr, 0.9, 0.999, R.ADAM_EPS, 10)
    ref, bound = R.adam_expected(k, sc)
    bad, _ = R.adam_expected(k, sc, "skip_last")
    past, _ = R.adam_expected(k, sc, "one_past")
    for n, o in zip(k["sizes"], k["offs"]):
        e = o + n - 1
        moved = any(abs(bad[q][e] - ref[q][e]) > bound[q][e] for q in "MV")
        assert moved or (k["G"][k["goffs"][k["sizes"].index(n)] + n - 1] == 0), n
        assert any(past[q][e + 1] != ref[q][e + 1] for q in "MV"), n


def test_adam_one_past_at_lr_zero_is_seen_through_the_state():
    """At lr = 0 a stray update of element n leaves p's sentinel in place; exp_avg and exp_avg_sq still give it away"""
    k = R.adam_inputs(1010)
    sc = R.adam_scalars(0.0, 0.9, 0.999, R.ADAM_EPS, 10)
    b = _breaks(k, sc, mistake="one_past")
    assert b["M"] and b["V"]


# =========================================================================== parameter fingerprint
def test_fingerprint_reference_notices():
    rng = np.random.RandomState(7)
    sizes = R.fp_table_sizes(rng)[:60] + [16385, 576, 576, 1]
    tensors = [R.fp_bits(rng, n) for n in sizes]
    base = R.fp_ref(tensors)
    assert base == R.fp_ref([t.copy() for t in tensors]) and 0 <= base < 2 ** 64
    # a changed element: the first, the last, the slice boundary, one bit at a time
    t16 = sizes.index(16385)
    for i, mask in ((0, 1), (16383, 0x80000000), (16384, 1), (16384, 0x00400000), (255, 2), (256, 4)):
        other = [t.copy() for t in tensors]
        other[t16][i] ^= np.uint32(mask)
        assert R.fp_ref(other) != base, (i, mask)
    # two unequal elements of one tensor swapped
    other = [t.copy() for t in tensors]
    a = other[t16]
    assert a[5] != a[6] and a[3] != a[16384]
    a[5], a[6] = a[6], a[5]
    assert R.fp_ref(other) != base
    a[5], a[6] = a[6], a[5]
    a[3], a[16384] = a[16384], a[3]
    assert R.fp_ref(other) != base
    # two unequal tensors of equal size swapped in the table
    i, j = [t for t, n in enumerate(sizes) if n == 576][-2:]
    assert not np.array_equal(tensors[i], tensors[j])
    other = list(tensors)
    other[i], other[j] = other[j], other[i]
    assert R.fp_ref(other) != base
    ones = [t for t, n in enumerate(sizes) if n == 1 and tensors[t][0] != tensors[-1][0]]
    other = list(tensors)
    other[ones[0]], other[-1] = other[-1], other[ones[0]]
    assert R.fp_ref(other) != base
    # a tail element dropped from the sum
    for t in (t16, len(sizes) - 1, sizes.index(576)):
        assert R.fp_tensor(tensors[t], t, drop_tail=True) != R.fp_tensor(tensors[t], t)


def test_fingerprint_reference_is_the_documented_sum():
    """The vectorised reference against a scalar restatement of the kernel's loop on a small tensor: element by element, thread
    by thread, with Python integers"""
    M = 0xFFFFFFFF

    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & M
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & M
        return h ^ (h >> 16)

    rng = np.random.RandomState(3)
    for t, n in ((0, 1), (5, 700), (699, 16384 + 300)):
        x = R.fp_bits(rng, n)
        sa, sb = fmix((0x9E3779B9 * (t + 1)) & M), fmix((0x7F4A7C15 + t) & M)
        total = 0
        for i0 in range(0, n, R.FP_SLICE):
            for tid in range(256):
                ha = hb = 0
                for i in range(i0 + tid, min(i0 + R.FP_SLICE, n), 256):
                    v = int(x[i])
                    ha += fmix(((v ^ sa) + i * 0x9E3779B1) & M)
                    hb += fmix(((v + sb) & M) ^ ((i * 0x85EBCA77 + 0x165667B1) & M))
                total += (hb << 32) + ha + (hb >> 32)
        assert R.fp_tensor(x, t) == total & 0xFFFFFFFFFFFFFFFF
    rows, nblk = R.fp_table_rows([1000, 2000, 3000], [1, 16385, 16384])
    assert rows == [(1000, 1, 0), (2000, 16385, 1), (3000, 16384, 3)] and nblk == 4


# =========================================================================== weight packs
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("form", R.PACK_FORMS)
def test_pack_reference_notices(form, dt):
    """Over the GPU test's whole-pack cases: taps transposed (wherever there is more than one tap), cot fixed at 64 (wherever
    rows <= 32), one padding element left as the sentinel (wherever there is padding)"""
    seen = {"taps": 0, "cot": 0, "pad": 0}
    for n, (shape, args) in enumerate(R.pack_cases(form, dt)):
        if n % 3 and form in ("fwd", "dgrad_s1"):        # a third of the two largest families keeps this test quick
            continue
        w = R.pack_values(shape, 31 * n + 1)
        rows, kdim, tys, txs = args[:4]
        want = R.pack_ref(w, *args, dt)
        assert want.numel() == R.pack_elems(rows, kdim, tys * txs, dt) and R.same_bits(want, R.pack_ref(w, *args, dt))
        if tys * txs > 1:
            seen["taps"] += 1
            assert not R.same_bits(want, R.pack_ref(w, *args, dt, mistake="taps_transposed")), (shape, args)
        if rows <= 32:
            seen["cot"] += 1
            assert not R.same_bits(want, R.pack_ref(w, *args, dt, mistake="cot64")), (shape, args)
        cot = 32 if rows <= 32 else 64
        if rows % cot or kdim % R.KCE[dt]:
            seen["pad"] += 1
            v = want.view(-1, tys * txs, cot, R.KCE[dt])
            padded = torch.nonzero((v.view(torch.int32 if dt == "fp32" else torch.int16) == 0).reshape(-1))
            left = want.clone()
            left[padded[-1]] = R.pack_sentinel(1, dt)
            assert not R.same_bits(want, left)
    assert seen["cot"] and seen["pad"] and (seen["taps"] or form == "deconv_k2s2")


def test_pack_ties_round_to_even():
    w = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11])
    b = R.pack_ref(w.view(1, 4), 1, 4, 1, 1, 4, 1, 0, 0, 0, "bf16")[:4].float()
    h = R.pack_ref(w.view(1, 4), 1, 4, 1, 1, 4, 1, 0, 0, 0, "fp16")[:4].float()
    assert b[0] == 1 and b[1] == 1 + 2.0 ** -6 and h[2] == 1 and h[3] == 1 + 2.0 ** -9
    vals = R.pack_values((64, 160, 3, 3), 1)
    assert float(vals.abs().min()) >= 2.0 ** -10 and float(vals.abs().max()) < 4
    assert int((vals == 1 + 2.0 ** -8).sum()) > 100 and int((vals == 1 + 3 * 2.0 ** -11).sum()) > 100


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("rows", R.PART_ROWS)
def test_part_pack_reference_notices(rows, dt):
    """The three part calls of the GPU test: k_off ignored, the scale applied after the cast (16-bit types: in fp32 there is no
    cast to be on the wrong side of), and a call that writes outside its range"""
    assert R.PART_KTOTAL % R.KCE[dt] and rows % (32 if rows <= 32 else 64)
    assert sorted((o, o + n) for o, n, _, _ in R.PART_CALLS) == [(0, 30), (30, 43), (43, 75)]
    state = R.pack_sentinel(R.pack_elems(rows, R.PART_KTOTAL, 9, dt), dt)
    for n, (k_off, kdim, scale, cin) in enumerate(R.PART_CALLS):
        shape, args = R.part_args(rows, k_off, kdim, cin)
        w = R.pack_values(shape, 500 + n)
        kw = dict(k_off=k_off, k_total=R.PART_KTOTAL, scale=scale, init=state)
        want = R.pack_ref(w, *args, dt, **kw)
        assert not R.same_bits(want, state)
        if k_off:
            assert not R.same_bits(want, R.pack_ref(w, *args, dt, mistake="k_off_ignored", **kw))
        if scale not in (1.0, -1.0) and dt != "fp32":
            assert not R.same_bits(want, R.pack_ref(w, *args, dt, mistake="scale_after_cast", **kw))
        # a call that zeroes what is not its own (the whole-pack behaviour) differs: padding and earlier ranges must stay
        whole = R.pack_ref(w, *args, dt, k_off=k_off, k_total=R.PART_KTOTAL, scale=scale, init=torch.zeros_like(state))
        assert not R.same_bits(want, whole)
        state = want


# =========================================================================== layout
@pytest.mark.parametrize("dt", R.DTS)
def test_layout_references_notice(dt):
    """Over the sweep of the GPU test: H and W exchanged (wherever both exceed 1), channels rotated by one (C > 1), the last pixel
    left as the sentinel, a pad channel that is not +0 (-0.0: the comparison is one of bits)"""
    sent = torch.tensor(R.SENT)
    seen = {"hw": 0, "rot": 0, "pad": 0}
    for n, (B, C, H, W, cs) in enumerate(R.layout_cases()):
        x = R.layout_values((B, C, H, W), 11 * n + 3)
        want = R.nhwc_ref(x, cs, dt)
        assert R.same_bits(want, R.nhwc_ref(x, cs, dt)) and R.same_bits(want[..., :C], x.permute(0, 2, 3, 1).to(R.TDT[dt]))
        coff = R.layout_coff(C, cs)
        buf = torch.full((B, H, W, cs), float("nan"), dtype=R.TDT[dt])
        buf[..., coff:coff + C] = R.layout_values((B, H, W, C), 13 * n + 5).to(R.TDT[dt])
        back = R.nchw_ref(buf, C, coff)
        if H > 1 and W > 1:
            seen["hw"] += 1
            assert not R.same_bits(want, R.nhwc_ref(x, cs, dt, "hw_exchanged"))
            assert not R.same_bits(back, R.nchw_ref(buf, C, coff, "hw_exchanged"))
        if C > 1:
            seen["rot"] += 1
            assert not R.same_bits(want, R.nhwc_ref(x, cs, dt, "channels_rotated"))
            assert not R.same_bits(back, R.nchw_ref(buf, C, coff, "channels_rotated"))
        assert not R.same_bits(want, R.nhwc_ref(x, cs, dt, "last_pixel_left", sent))
        assert not R.same_bits(back, R.nchw_ref(buf, C, coff, "last_pixel_left", sent))
        if cs > C:
            seen["pad"] += 1
            assert not R.same_bits(want, R.nhwc_ref(x, cs, dt, "pad_nonzero"))
            assert float(want[..., C:].float().abs().max()) == 0 and not bool(torch.signbit(want[..., C:].float()).any())
    assert all(seen.values())
    assert {H * W for (_, _, H, W, _) in R.layout_cases()} == {1, 63, 64, 65, 481, 512}
