"""Direct tests, through the C ABI, of srcgan_ca_forward / srcgan_ca_backward (csrc/chan_attn.hip) on the grid of
tests/chan_attn_ref.py (grid_cases): hw = 1, 63, one below / at / above the kernel's pixel chunk, two chunks and a ragged tail; C = 16, 64,
96; Cr = 1, 4, C; B = 1, 3; fp32, bf16, fp16; res null and non-null; dres null, stored and accumulated; single parameter-gradient pointers
null.

Every element of saved (p, h, s), y, dt, dres and the four parameter gradients is held to float64 of the stored inputs within
K * 2^-24 * N (+ one rounding of the storage type for y, dt, dres); K and N are those of chan_attn_ref (K = 4 x the float32 restatement's
own error on these inputs, tests/test_chan_attn_teeth.py).  The maxima are printed ("[ca] ..." lines, pytest -s)."""
import numpy as np
import pytest
import torch

import chan_attn_ref as R

pytestmark = pytest.mark.gpu
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENT = 1000.0


class Lib:
    def __init__(self):
        from srcgan_amd import _native as N
        self.N, self.lib = N, N.lib()

    def st(self):
        return self.N.stream_ptr(torch.device("cuda"))

    def scratch(self, B, hw, C):
        """NaN-filled: a slot read before it is written cannot pass for a number"""
        return torch.full((self.lib.srcgan_ca_scratch_floats(B, hw, C) + 8,), float("nan"), device="cuda")


@pytest.fixture(scope="module")
def L():
    return Lib()


def dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(TDT[dtype]).contiguous()


def run_case(L, case, dtype, inp, fwd_only=False):
    """One forward + backward through the C ABI -> dict of QUANTITIES as float64 numpy arrays (None for a null gradient pointer)."""
    B, hw, C, Cr, with_res, acc, null_grad = case
    p = lambda t: None if t is None else t.data_ptr()
    did = L.N.dtype_id(dtype)
    t, res, g = dev(inp["t"], dtype), dev(inp["res"], dtype), dev(inp["g"], dtype)
    w1, b1, w2, b2 = (torch.from_numpy(inp[k]).cuda() for k in ("w1", "b1", "w2", "b2"))
    y = torch.full((B, hw, C), SENT, device="cuda", dtype=TDT[dtype])
    nsv = B * (2 * C + Cr)
    saved = torch.full((nsv + 8,), SENT, device="cuda")
    scr = L.scratch(B, hw, C)
    L.N.check(L.lib.srcgan_ca_forward(p(t), C, p(res), C if res is not None else 0, p(y), C, p(w1), p(b1), p(w2), p(b2), p(saved), B, hw, C, Cr, did,
                                      p(scr), L.st()), "srcgan_ca_forward")
    assert bool((saved[nsv:] == SENT).all()), "wrote past saved"
    sv = saved[:nsv].view(B, 2 * C + Cr).double().cpu().numpy()
    out = {"p": sv[:, :C], "h": sv[:, C:C + Cr], "s": sv[:, C + Cr:], "y": y.double().cpu().numpy()}
    if fwd_only:
        return out, saved
    dt = torch.full((B, hw, C), SENT, device="cuda", dtype=TDT[dtype])
    no_dres = null_grad == 4 and not acc and (hw + C) % 2 == 1         # some cases pass no dres at all
    dres = dev(inp["old"], dtype) if acc else torch.full((B, hw, C), SENT, device="cuda", dtype=TDT[dtype])
    grads = [torch.full((n + 8,), SENT, device="cuda") for n in (Cr * C, Cr, C * Cr, C)]
    gp = [None if i == null_grad else p(v) for i, v in enumerate(grads)]
    scr = L.scratch(B, hw, C)
    L.N.check(L.lib.srcgan_ca_backward(p(g), C, p(t), C, p(w1), p(w2), p(saved), p(dt), C, None if no_dres else p(dres), 0 if no_dres else C, int(acc), *gp, B, hw, C, Cr, did,
                                       p(scr), L.st()), "srcgan_ca_backward")
    assert not no_dres or bool((dres == SENT).all())
    out["dt"], out["dres"] = dt.double().cpu().numpy(), None if no_dres else dres.double().cpu().numpy()
    for i, (name, shape) in enumerate((("dw1", (Cr, C)), ("db1", (Cr,)), ("dw2", (C, Cr)), ("db2", (C,)))):
        v = grads[i]
        n = int(np.prod(shape))
        if i == null_grad:
            assert bool((v == SENT).all()), f"{name}: written through a null pointer's neighbour"
            out[name] = None
        else:
            assert bool((v[n:] == SENT).all()), f"wrote past {name}"
            out[name] = v[:n].view(*shape).double().cpu().numpy()
    return out, saved


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_grid_per_element_against_float64(L, dtype):
    """Forward and backward against the float64 evaluation of the stored inputs (the backward's float64 uses the float64 p, h, s: the
    bounds carry the earlier stages' errors along, chan_attn_ref.scales)."""
    mx = {q: 0.0 for q in R.QUANTITIES}
    seen, no_dres = set(), 0
    for case in R.grid_cases():
        inp = R.make_inputs(case, dtype)
        ref = R.reference(inp)
        N = R.scales(inp["t"], inp["res"], inp["g"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], inp["old"])
        got, _ = run_case(L, case, dtype, inp)
        seen.add((case[4], case[5], case[6]))
        for q in R.QUANTITIES:
            if got[q] is None:
                no_dres += q == "dres"
                continue
            assert np.isfinite(got[q]).all(), (q, case)
            w = R.worst(q, got[q], ref[q], N[q], dtype)
            mx[q] = max(mx[q], R.units(got[q], ref[q], N[q]))
            assert w <= 1.0, f"{q} {dtype} case {case}: {w:.3f} x the bound"
    assert {a for a, _, _ in seen} == {0, 1} and {b for _, b, _ in seen} == {0, 1} and {c for _, _, c in seen} == {0, 1, 2, 3, 4} and no_dres > 0
    print(f"[ca] grid {dtype}: largest error in units of 2^-24 N (16-bit y / dt / dres: storage rounding included): " +
          ", ".join(f"{q} {v:.2f}" for q, v in mx.items()) + f"; K = {R.K_RECORDED}")


def test_pooled_mean_is_exact_on_integer_data(L):
    """hw a power of two, t small integers: every partial sum and the division are exact in any order."""
    rng = np.random.default_rng(5)
    for dtype in ("fp32", "bf16", "fp16"):
        for B, hw, C, Cr in ((2, 512, 64, 4), (1, 256, 16, 1), (3, 1024, 96, 96)):
            case = (B, hw, C, Cr, 0, 0, 4)
            inp = R.make_inputs(case, dtype)
            inp["t"] = rng.integers(-8, 9, size=(B, hw, C)).astype(np.float32)
            got, _ = run_case(L, case, dtype, inp, fwd_only=True)
            assert np.array_equal(got["p"], inp["t"].astype(np.float64).mean(axis=1)), (dtype, B, hw, C)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_calls_give_the_same_bits(L, dtype):
    for case in ((3, 2 * R.CHUNK + 1, 96, 4, 1, 1, 4), (3, 63, 64, 64, 1, 0, 4)):
        inp = R.make_inputs(case, dtype)
        a, sa = run_case(L, case, dtype, inp)
        b, sb = run_case(L, case, dtype, inp)
        assert torch.equal(sa, sb)
        for q in R.QUANTITIES:
            assert np.array_equal(a[q], b[q]), q


@pytest.mark.parametrize("what", ["C=12", "Cr=0", "Cr>C", "dtype"])
def test_refused_shapes_name_the_entry_point_and_write_nothing(L, what):
    B, hw, C, Cr, did = 2, 10, 16, 4, L.N.dtype_id("fp32")
    if what == "C=12":
        C = 12
    elif what == "Cr=0":
        Cr = 0
    elif what == "Cr>C":
        Cr = 17
    else:
        did = 77
    p = lambda t: t.data_ptr()
    big = lambda: torch.full((B * hw * 16 + 64,), SENT, device="cuda")
    t, y, saved, scr, g, dt, dres = big(), big(), big(), big(), big(), big(), big()
    w = [torch.full((16 * 17 + 8,), SENT, device="cuda") for _ in range(4)]
    dw = [torch.full((16 * 17 + 8,), SENT, device="cuda") for _ in range(4)]
    rc = L.lib.srcgan_ca_forward(p(t), 16, None, 0, p(y), 16, p(w[0]), p(w[1]), p(w[2]), p(w[3]), p(saved), B, hw, C, Cr, did, p(scr), L.st())
    assert rc != 0 and b"srcgan_ca_forward" in L.lib.srcgan_last_error()
    rc = L.lib.srcgan_ca_backward(p(g), 16, p(t), 16, p(w[0]), p(w[2]), p(saved), p(dt), 16, p(dres), 16, 0, p(dw[0]), p(dw[1]), p(dw[2]), p(dw[3]),
                                  B, hw, C, Cr, did, p(scr), L.st())
    assert rc != 0 and b"srcgan_ca_backward" in L.lib.srcgan_last_error()
    torch.cuda.synchronize()
    for v in (y, saved, scr, dt, dres, *dw):
        assert bool((v == SENT).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_every_operand_has_its_own_channel_stride(L, dtype):
    """Records wider than C, a different width for every operand: the result has the bits of the dense call, and nothing outside
    [0, C) of an output record is written (the padding keeps its sentinel; the padding of the inputs is NaN and reaches nothing)."""
    p = lambda v: v.data_ptr()
    did = L.N.dtype_id(dtype)
    for case in ((3, R.CHUNK + 1, 96, 4, 1, 1, 4), (2, 62, 16, 16, 1, 0, 4)):
        B, hw, C, Cr, _, acc, _ = case
        inp = R.make_inputs(case, dtype)
        dense, _ = run_case(L, case, dtype, inp)

        def wide(a, pad, fill):
            buf = torch.full((B, hw, C + pad), fill, device="cuda", dtype=TDT[dtype])
            if a is not None:
                buf[..., :C] = dev(a, dtype)
            return buf
        nan = float("nan")
        t, res, g = wide(inp["t"], 8, nan), wide(inp["res"], 16, nan), wide(inp["g"], 24, nan)
        y, dt, dres = wide(None, 32, SENT), wide(None, 8, SENT), wide(inp["old"] if acc else None, 40, SENT)
        w1, b1, w2, b2 = (torch.from_numpy(inp[k]).cuda() for k in ("w1", "b1", "w2", "b2"))
        saved = torch.full((B * (2 * C + Cr),), SENT, device="cuda")
        grads = [torch.full((n,), SENT, device="cuda") for n in (Cr * C, Cr, C * Cr, C)]
        L.N.check(L.lib.srcgan_ca_forward(p(t), C + 8, p(res), C + 16, p(y), C + 32, p(w1), p(b1), p(w2), p(b2), p(saved), B, hw, C, Cr, did,
                                          p(L.scratch(B, hw, C)), L.st()), "srcgan_ca_forward")
        L.N.check(L.lib.srcgan_ca_backward(p(g), C + 24, p(t), C + 8, p(w1), p(w2), p(saved), p(dt), C + 8, p(dres), C + 40, int(acc),
                                           *[p(v) for v in grads], B, hw, C, Cr, did, p(L.scratch(B, hw, C)), L.st()), "srcgan_ca_backward")
        for name, buf in (("y", y), ("dt", dt), ("dres", dres)):
            assert bool((buf[..., C:] == SENT).all()), f"{name}: wrote outside [0, C)"
            assert np.array_equal(buf[..., :C].double().cpu().numpy(), dense[name]), name
        sv = saved.view(B, 2 * C + Cr).double().cpu().numpy()
        assert np.array_equal(sv[:, :C], dense["p"]) and np.array_equal(sv[:, C + Cr:], dense["s"])
        for name, v, shape in zip(("dw1", "db1", "dw2", "db2"), grads, ((Cr, C), (Cr,), (C, Cr), (C,))):
            assert np.array_equal(v.view(*shape).double().cpu().numpy(), dense[name]), name
