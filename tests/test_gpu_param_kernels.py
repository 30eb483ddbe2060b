"""Direct tests of the kernels that hold the weights (csrc/elementwise.hip): adam_multi_k through srcgan_amd.optim.Adam,
params_fingerprint_k through srcgan_params_fingerprint, pack_weight_k through srcgan_pack_weight and srcgan_pack_weight_part.
The references and the cases live in tests/param_kernels_ref.py; tests/test_param_kernels_teeth.py shows on the CPU that they
notice the mistakes these tests are there to catch.

  * Adam: ONE step from a given state against a float64 evaluation, every element of p, exp_avg and exp_avg_sq under its own
    bound (param_kernels_ref.adam_bound), the sentinels around all three and the gradients bit-unchanged.  Each case prints
    its worst error / bound per quantity ("[param] adam ..." lines, pytest -s).
  * fingerprint and packs: integer arithmetic and data movement, compared in bits.

pack_multi_k and fill_zero_guarded_k have no entry point of their own and none is added for them: they stay covered by the
poisoned-workspace suite (tests/test_gpu_workspace_hygiene.py and the per-family hygiene files) and by the network goldens."""
import numpy as np
import pytest
import torch

import param_kernels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from srcgan_amd import _native as N
    return N.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# =========================================================================== fused Adam
class _Group:
    """A parameter group on the device, laid out by param_kernels_ref.adam_inputs: parameters and state are slices of three
    sentinel-filled buffers, the gradients views of one flat buffer at running offsets."""

    def __init__(self, k, lr, betas, step):
        from srcgan_amd.optim import Adam
        self.k = k
        self.buf = {q: torch.from_numpy(k[q]).cuda() for q in "PMV"}
        self.params = [self.buf["P"][o:o + n].detach().requires_grad_() for n, o in zip(k["sizes"], k["offs"])]
        self.opt = Adam(self.params, lr=lr, betas=betas, eps=R.ADAM_EPS)
        for p, n, o in zip(self.params, k["sizes"], k["offs"]):
            assert p.data_ptr() % 16 == 0 and p.data_ptr() == self.buf["P"].data_ptr() + 4 * o
            self.opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": self.buf["M"][o:o + n], "exp_avg_sq": self.buf["V"][o:o + n]}
        self.set_grads(k["G"], k["goffs"])

    def set_grads(self, G, goffs):
        self.G = torch.from_numpy(G).cuda()
        self.G0 = self.G.clone()
        for p, n, go in zip(self.params, self.k["sizes"], goffs):
            p.grad = self.G[go:go + n]
            assert p.grad.data_ptr() == self.G.data_ptr() + 4 * go

    def step_and_check(self, sc, tag):
        ref, bound = R.adam_expected(self.k, sc)
        self.opt.step()
        torch.cuda.synchronize()
        assert R.same_bits(self.G, self.G0), "the step wrote to a gradient"
        got = {q: self.buf[q].cpu().numpy() for q in "PMV"}
        res = {q: R.adam_check(got[q], ref[q], bound[q]) for q in "PMV"}
        print(f"[param] adam {tag}: worst error/bound p {res['P'][1]:.3f} m {res['M'][1]:.3f} v {res['V'][1]:.3f}")
        sent = np.ones(len(got["P"]), bool)
        for n, o in zip(self.k["sizes"], self.k["offs"]):
            sent[o:o + n] = False
        for q in "PMV":
            bad = np.flatnonzero(np.abs(got[q].astype(np.float64) - ref[q]) > bound[q])
            assert res[q][0], f"{q}: {len(bad)} elements outside their bound, first at buffer index {bad[:5]} (tensor offsets {self.k['offs']})"
            assert np.array_equal(got[q][sent].view(np.uint32), self.k[q][sent].view(np.uint32)), f"{q}: a sentinel changed"
        return got


@pytest.mark.parametrize("lr", R.ADAM_LRS)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("betas", R.ADAM_BETAS)
def test_adam_one_step_against_float64(lib, betas, step, lr):
    """Fourteen tensors (1 ... 12288 elements: every tail length, one to three 4096-chunks) in one launch, gradients at element
    offsets = 0, 1, 2, 3 (mod 4) of a flat buffer; then a second step on fresh gradient addresses (the pointer table is uploaded
    again), checked against the reference applied to the DEVICE's state after the first, so the bound stays a one-step bound."""
    k = R.adam_inputs(1000 + step % 997)
    assert {go % 4 for go in k["goffs"]} == {0, 1, 2, 3}
    g = _Group(k, lr, betas, step)
    tag = f"b1={betas[0]} k={step} lr={lr}"
    got = g.step_and_check(R.adam_scalars(lr, *betas, R.ADAM_EPS, step), tag)
    assert all(int(g.opt.state[p]["step"]) == step for p in g.params)
    old = g.G
    k2 = R.adam_inputs(2000 + step % 997, grad_shift=3)
    k2.update(P=got["P"], M=got["M"], V=got["V"])
    g.k = k2
    g.set_grads(k2["G"], k2["goffs"])
    assert g.G.data_ptr() != old.data_ptr() and {go % 4 for go in k2["goffs"]} == {0, 1, 2, 3}
    g.step_and_check(R.adam_scalars(lr, *betas, R.ADAM_EPS, step + 1), tag + " second step")


def test_adam_unaligned_parameter_takes_torch_path(lib):
    """The kernel moves p, exp_avg and exp_avg_sq with 16-byte accesses: a parameter at a one-element storage offset goes through
    torch's own step and ends bit-identical to torch.optim.Adam on a clone, state included."""
    from srcgan_amd.optim import Adam
    torch.manual_seed(5)
    base = torch.randn(4 + 1031, device="cuda")
    base0 = base.clone()
    pa = [base[1:1 + 1030].detach().requires_grad_(), torch.randn(64, 3, device="cuda").requires_grad_()]
    assert pa[0].data_ptr() % 16 == 4
    pb = [p.detach().clone().requires_grad_() for p in pa]
    oa, ob = Adam(pa, lr=1e-3, betas=(0.5, 0.999)), torch.optim.Adam(pb, lr=1e-3, betas=(0.5, 0.999))
    for _ in range(3):
        for a, b in zip(pa, pb):
            a.grad = torch.randn_like(a)
            b.grad = a.grad.clone()
        oa.step()
        ob.step()
    for a, b in zip(pa, pb):
        assert R.same_bits(a.detach(), b.detach())
        for key in ("exp_avg", "exp_avg_sq"):
            assert R.same_bits(oa.state[a][key], ob.state[b][key])
    assert R.same_bits(base[:1], base0[:1]) and R.same_bits(base[1031:], base0[1031:]) and not R.same_bits(base, base0)
    # aligned parameters whose STATE is not (a loaded state_dict may alias anything) take torch's path too
    p = torch.randn(1030, device="cuda").requires_grad_()
    q = p.detach().clone().requires_grad_()
    sbuf = torch.zeros(2, 1032, device="cuda")
    oa, ob = Adam([p], lr=1e-3), torch.optim.Adam([q], lr=1e-3)
    oa.state[p] = {"step": torch.tensor(0.0), "exp_avg": sbuf[0, 1:1031], "exp_avg_sq": sbuf[1, 1:1031]}
    p.grad = torch.randn_like(p)
    q.grad = p.grad.clone()
    oa.step()
    ob.step()
    assert R.same_bits(p.detach(), q.detach()) and R.same_bits(sbuf[0, 1:1031], ob.state[q]["exp_avg"])
    assert float(sbuf[:, 0].abs().max()) == 0.0 and float(sbuf[:, 1031].abs().max()) == 0.0


# =========================================================================== parameter fingerprint
class _Table:
    """Tensors as slices of one flat device buffer of raw bits, the pointer table as model._PackState.opts builds it, and the
    reference's per-tensor shares, so that a changed element costs one tensor's re-hash on the CPU."""

    def __init__(self, lib, bits_list):
        self.lib = lib
        self.sizes = [len(b) for b in bits_list]
        self.starts = np.concatenate([[0], np.cumsum(self.sizes)[:-1]]).tolist()
        self.host = np.concatenate(bits_list).astype(np.uint32)
        self.flat = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
        self.tensors = [self.flat[s:s + n] for s, n in zip(self.starts, self.sizes)]          # kept alive for the calls
        rows, self.nblocks = R.fp_table_rows([t.data_ptr() for t in self.tensors], self.sizes)
        self.table = torch.tensor(rows, dtype=torch.int64).cuda()
        self.out = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")    # the word between two guards
        self.shares = [R.fp_tensor(self.host[s:s + n], t) for t, (s, n) in enumerate(zip(self.starts, self.sizes))]

    def device(self):
        from srcgan_amd import _native as N
        N.check(self.lib.srcgan_params_fingerprint(self.table.data_ptr(), len(self.sizes), self.nblocks, self.out.data_ptr() + 8, _stream()),
                "srcgan_params_fingerprint")
        o = self.out.cpu()
        assert int(o[0]) == 0x5A5A5A5A5A5A5A5A and int(o[2]) == 0x5A5A5A5A5A5A5A5A
        return int(o[1]) & 0xFFFFFFFFFFFFFFFF

    def ref(self):
        return sum(self.shares) & 0xFFFFFFFFFFFFFFFF

    def flip(self, t, i, mask):
        """xor the bits of element i of tensor t on the device and in the reference"""
        s, n = self.starts[t], self.sizes[t]
        self.host[s + i] ^= np.uint32(mask)
        self.tensors[t][i:i + 1].bitwise_xor_(mask - (1 << 32) if mask >= 1 << 31 else mask)
        self.shares[t] = R.fp_tensor(self.host[s:s + n], t)


def _flips_change_the_word(tb, flips):
    before = tb.device()
    assert before == tb.ref() and tb.device() == before             # the word is cleared by every call, not accumulated
    for t, i, mask in flips:
        tb.flip(t, i, mask)
        now = tb.device()
        assert now == tb.ref(), f"tensor {t} ({tb.sizes[t]} elements), element {i}, mask {mask:#x}"
        assert now != before, f"a change of tensor {t}, element {i} (mask {mask:#x}) went unnoticed"
        before = now


@pytest.mark.parametrize("n", R.FP_SINGLE_SIZES)
def test_fingerprint_one_tensor(lib, n):
    rng = np.random.RandomState(n)
    tb = _Table(lib, [R.fp_bits(rng, n)])
    pos = sorted({p for p in (0, n - 1, 255, 256, 16383, 16384) if p < n})
    _flips_change_the_word(tb, [(0, p, 1 << int(rng.randint(0, 32))) for p in pos])


def test_fingerprint_many_tensors(lib):
    """700 tensors, two in five of one element: runs of consecutive blocks belong to different tensors (the binary search), the
    larger ones span one to three slices.  One element changes at a time."""
    rng = np.random.RandomState(7)
    sizes = R.fp_table_sizes(rng)
    tb = _Table(lib, [R.fp_bits(rng, n) for n in sizes])
    assert tb.nblocks > len(sizes) and sizes[350] == 1
    big = max(range(len(sizes)), key=lambda t: (sizes[t], t))
    assert sizes[big] == 36864
    # only the sign of a zero, only the lowest mantissa bit
    t16 = sizes.index(16385)
    tb.flip(t16, 16384, int(tb.host[tb.starts[t16] + 16384]))      # make the tail element +0.0 first
    assert tb.host[tb.starts[t16] + 16384] == 0
    flips = [(t16, 16384, 0x80000000), (t16, 16383, 0x00000001), (big, 36863, 0x00000001)]
    flips += [(big, p, 0x00400000) for p in (0, 255, 256, 16383, 16384, sizes[big] - 1)]
    flips += [(len(sizes) - 1, sizes[-1] - 1, 0x80000000), (350, 0, 0x00000100)]
    for _ in range(64):
        t = int(rng.randint(0, len(sizes)))
        flips.append((t, int(rng.randint(0, sizes[t])), 1 << int(rng.randint(0, 32))))
    _flips_change_the_word(tb, flips)


# =========================================================================== weight packs
def _pack(lib, w, args, dt, init=None, part=None):
    """srcgan_pack_weight (part None) or srcgan_pack_weight_part (part = (k_off, k_total, scale)) into a sentinel-filled buffer of
    the library's own size with a guard of 64 sentinel elements behind it -> the whole buffer on the CPU"""
    from srcgan_amd import _native as N
    rows, kdim, tys, txs = args[:4]
    k_total = part[1] if part else kdim
    nbytes = lib.srcgan_packed_weight_bytes(rows, k_total, tys * txs, N.dtype_id(dt))
    nel = R.pack_elems(rows, k_total, tys * txs, dt)
    assert nbytes == nel * R.TDT[dt].itemsize
    buf = (R.pack_sentinel(nel + 64, dt) if init is None else init).cuda()
    if part:
        rc = lib.srcgan_pack_weight_part(w.data_ptr(), buf.data_ptr(), *args, part[0], k_total, part[2], N.dtype_id(dt), _stream())
    else:
        rc = lib.srcgan_pack_weight(w.data_ptr(), buf.data_ptr(), *args, N.dtype_id(dt), _stream())
    N.check(rc, "srcgan_pack_weight")
    return buf.cpu()


def _guarded(ref, dt):
    return torch.cat([ref, R.pack_sentinel(64, dt)])


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("form", R.PACK_FORMS)
def test_pack_weight_whole(lib, form, dt):
    """Every rows x kdim of the issue's lists with every tap shape (or quadrant / parity) of the form.  Bit equality with the
    reference over the whole buffer: every sentinel byte overwritten, the padding exactly +0, nothing behind the end."""
    for n, (shape, args) in enumerate(R.pack_cases(form, dt)):
        w = R.pack_values(shape, 31 * n + 1)
        want = _guarded(R.pack_ref(w, *args, dt), dt)            # the reference first: it asserts that the pack reads inside w
        assert R.same_bits(_pack(lib, w.cuda(), args, dt), want), f"{form} {dt}: weight {shape}, arguments {args}"


def test_pack_weight_second_grid_stride_trip(lib):
    """512 x 512 x 3x3 in fp32: 2 359 296 elements, above the 4096 x 256 a grid covers in one trip"""
    shape, args = R.pack_form("fwd", 512, 512, 3)
    w = R.pack_values(shape, 77)
    assert R.pack_elems(512, 512, 9, "fp32") > 4096 * 256
    want = _guarded(R.pack_ref(w, *args, "fp32"), "fp32")
    assert R.same_bits(_pack(lib, w.cuda(), args, "fp32"), want)


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("rows", R.PART_ROWS)
def test_pack_weight_part(lib, rows, dt):
    """The dense-block backward's composite matrix from three calls: each writes exactly its [k_off, k_off + kdim) x [0, rows)
    as f32(scale w) cast once and leaves every other byte as it was -- the padding (never written: no call is a whole pack), the
    guard, and the ranges the calls before it wrote."""
    state = R.pack_sentinel(R.pack_elems(rows, R.PART_KTOTAL, 9, dt) + 64, dt)
    for n, (k_off, kdim, scale, cin) in enumerate(R.PART_CALLS):
        shape, args = R.part_args(rows, k_off, kdim, cin)
        w = R.pack_values(shape, 500 + n)
        want = _guarded(R.pack_ref(w, *args, dt, k_off=k_off, k_total=R.PART_KTOTAL, scale=scale, init=state[:-64]), dt)
        assert not R.same_bits(want, state)
        state = _pack(lib, w.cuda(), args, dt, init=state, part=(k_off, R.PART_KTOTAL, scale))
        assert R.same_bits(state, want), f"call {n}: k_off {k_off}, kdim {kdim}, scale {scale}"
    # all three together are the composite: the padding is still the sentinel, everything else is written
    view = state[:-64].reshape(-1, 9, 32 if rows <= 32 else 64, R.KCE[dt])
    sent = R.pack_sentinel(1, dt)
    nch = view.shape[0] // (-(-rows // view.shape[2]))
    k_of = (torch.arange(view.shape[0]) % nch).view(-1, 1, 1, 1) * R.KCE[dt] + torch.arange(R.KCE[dt]).view(1, 1, 1, -1)
    row_of = (torch.arange(view.shape[0]) // nch).view(-1, 1, 1, 1) * view.shape[2] + torch.arange(view.shape[2]).view(1, 1, -1, 1)
    pad = ((k_of >= R.PART_KTOTAL) | (row_of >= rows)).expand(view.shape)
    it = torch.int32 if dt == "fp32" else torch.int16
    assert bool(((view.view(it) == sent.view(it)) == pad).all())


def test_pack_weight_refusals(lib):
    """k_off + kdim > k_total, a null pointer and zero sizes are errors, and nothing is launched: the buffer keeps its bytes"""
    from srcgan_amd import _native as N
    w = torch.randn(32, 16, 3, 3, device="cuda")
    buf = R.pack_sentinel(4096 * 9, "fp32").cuda()
    keep = buf.clone()
    a = (32, 16, 3, 3, 144, 9, 3, 1, 0)
    part = lambda w_, b_, args, k_off, k_total: lib.srcgan_pack_weight_part(w_, b_, *args, k_off, k_total, 1.0, N.F32, _stream())
    assert part(w.data_ptr(), buf.data_ptr(), a, 8, 16) != 0                  # [8, 24) of 16
    assert b"k range" in lib.srcgan_last_error()
    assert part(w.data_ptr(), buf.data_ptr(), a, -1, 16) != 0
    assert part(None, buf.data_ptr(), a, 0, 16) != 0
    assert part(w.data_ptr(), None, a, 0, 16) != 0
    for i in range(4):                                                        # rows, kdim, tys, txs = 0
        z = list(a)
        z[i] = 0
        assert part(w.data_ptr(), buf.data_ptr(), tuple(z), 0, 16) != 0
        assert lib.srcgan_pack_weight(w.data_ptr(), buf.data_ptr(), *z, N.F32, _stream()) != 0
    torch.cuda.synchronize()
    assert R.same_bits(buf, keep)
    assert part(w.data_ptr(), buf.data_ptr(), a, 0, 16) == 0                  # the same call, well-formed, is accepted and writes
    torch.cuda.synchronize()
    assert not R.same_bits(buf, keep)
