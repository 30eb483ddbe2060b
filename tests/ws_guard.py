"""Poisoned, guarded workspaces for the whole-network drivers (a plain helper module, like tests/conv_exact.py).

The drivers of csrc/nets.hip and csrc/oplist.hip carve every tensor out of caller-supplied buffers whose contents on entry are
unspecified ("Workspace contract").  Nothing in the project uses float atomics, so two runs on the same inputs give the same
bits; hence a driver's results may not depend, not even in one bit, on what its buffers held before the call.  ``guarded(fill, device)``
makes that testable: for its duration

  * ``srcgan_amd._native.workspace`` hands out the interior of a buffer of ``nbytes + 2 G`` bytes (G = 65536, a multiple of 4096, so the
    interior keeps the alignment of a direct ``torch.empty``), the interior filled with the fill byte and both guards with the guard byte;
  * ``srcgan_amd.model._GradArena`` is a subclass whose ``flat`` is carved from such a buffer (whole floats);
  * ``srcgan_amd.model._PackState.opts`` fills a freshly allocated ``buf`` with the fill byte, queued on the current stream ahead of
    the native call that packs.

All three are replaced by attribute assignment and restored on exit.  Fills: ``ZERO`` (interior 0x00, guards 0xA5), ``NAN`` (interior and
guards 0xFF: a NaN in f32, bf16 and fp16, -1 as an integer; a NaN guard makes an over-read visible as well as an over-write) and
``STALE`` (``guarded(STALE, device, previous=g)`` hands out the buffers of the earlier block ``g`` as that block's run left them).

``guarded_slabs(fill, device)`` does the same for the split-K slab of the kernel-level ``srcgan_conv_wgrad`` / ``srcgan_wgrad_dense`` calls.

The checks the GPU test applies (tests/test_gpu_workspace_hygiene.py) live here too, so that tests/test_ws_guard_teeth.py can show on
the CPU what they notice: ``Guard.check``, ``assert_finite``, ``assert_bit_equal``, ``assert_allocations`` and ``run_fills``."""
import contextlib
from collections import namedtuple

import torch

G = 65536                                   # guard bytes on each side of an allocation

Fill = namedtuple("Fill", "name interior guard")
ZERO = Fill("ZERO", 0x00, 0xA5)
NAN = Fill("NAN", 0xFF, 0xFF)
STALE = Fill("STALE", None, None)


class Alloc:
    """One recorded allocation: ``view`` is what the product code got, ``parent`` the buffer it lies in (guards on both sides when
    ``guard`` is a byte; ``None``: the weight pack, which the product allocates itself and this module only fills)."""

    def __init__(self, tag, kind, nbytes, parent, view, guard):
        self.tag, self.kind, self.nbytes, self.parent, self.view, self.guard = tag, kind, nbytes, parent, view, guard


def _caller(depth=2):
    import sys
    f = sys._getframe(depth)
    return f"{f.f_globals.get('__name__', '?').rsplit('.', 1)[-1]}.{f.f_code.co_name}"


class Guard:
    """The record of one ``guarded`` block."""

    def __init__(self, fill, device, previous=None):
        self.fill, self.device, self.allocs = fill, torch.device(device), []
        self._stale = list(previous.allocs) if previous is not None else None
        if fill is STALE:
            assert previous is not None, "guarded(STALE, ...) needs previous=<the Guard of an earlier block>"

    # ---- allocation
    def _take_stale(self, tag, kind, nbytes):
        for i, a in enumerate(self._stale):
            if a.kind == kind and a.nbytes == nbytes:
                return self._stale.pop(i)
        raise AssertionError(f"STALE: {tag} asks for {nbytes} bytes of kind {kind!r}, which the previous block never allocated "
                             f"(left: {[(a.kind, a.nbytes) for a in self._stale]})")

    def carve(self, tag, kind, nbytes):
        """-> uint8 view of ``nbytes`` bytes between two guards, recorded."""
        if self.fill is STALE:
            old = self._take_stale(tag, kind, nbytes)
            a = Alloc(tag, kind, nbytes, old.parent, old.view, old.guard)
        else:
            parent = torch.empty(nbytes + 2 * G, dtype=torch.uint8, device=self.device)
            parent[:G].fill_(self.fill.guard)
            parent[G + nbytes:].fill_(self.fill.guard)
            view = parent[G:G + nbytes]
            view.fill_(self.fill.interior)
            a = Alloc(tag, kind, nbytes, parent, view, self.fill.guard)
        self.allocs.append(a)
        return a.view

    def poison_pack(self, buf):
        """A weight pack the product has just allocated: fill it (STALE: with the bytes the previous block's pack of that size held)."""
        if self.fill is STALE:
            buf.copy_(self._take_stale("wpack", "wpack", buf.numel()).view)
        else:
            buf.fill_(self.fill.interior)
        self.allocs.append(Alloc("wpack", "wpack", buf.numel(), None, buf, None))

    # ---- checks
    def check(self):
        """Synchronise, then assert that every guard still holds its pattern."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for a in self.allocs:
            if a.guard is None:
                continue
            for name, region, base in (("before", a.parent[:G], -G), ("past", a.parent[G + a.nbytes:], a.nbytes)):
                bad = (region != a.guard).nonzero()
                if bad.numel():
                    off = base + int(bad[0, 0])
                    raise AssertionError(f"guard {name} allocation {a.tag!r} ({a.kind}, {a.nbytes} bytes) corrupted: first at offset {off} "
                                         f"from the region's start ({int(bad.shape[0])} guard bytes changed)")

    def sizes(self):
        """sorted [(kind, bytes)] of everything recorded"""
        return sorted((a.kind, a.nbytes) for a in self.allocs)


@contextlib.contextmanager
def guarded(fill, device, previous=None):
    from srcgan_amd import _native as N
    from srcgan_amd import model as M
    g = Guard(fill, device, previous)
    stock_ws, stock_arena, stock_opts = N.workspace, M._GradArena, M._PackState.opts

    def workspace(nbytes, device):
        if nbytes <= 0:
            return stock_ws(nbytes, device)                  # the planner-rejection error of the original
        assert torch.device(device).type == g.device.type, (device, g.device)
        return g.carve(_caller(), "workspace", int(nbytes))

    class GuardedArena(stock_arena):
        def __init__(self, params, needs):
            super().__init__(params, needs)
            n = self.flat.numel()
            flat = g.carve(_caller(), "grad_arena", 4 * n).view(torch.float32)
            assert flat.numel() == n and flat.device == self.flat.device
            self.flat = flat
            self.views = [None if v is None else flat[o:o + v.numel()].view(v.shape) for v, o in zip(self.views, self.offsets)]

    def opts(self, *a, **k):
        before = self.buf
        ret = stock_opts(self, *a, **k)
        if self.buf is not before:
            g.poison_pack(self.buf)
        return ret

    N.workspace, M._GradArena, M._PackState.opts = workspace, GuardedArena, opts
    try:
        yield g
    finally:
        N.workspace, M._GradArena, M._PackState.opts = stock_ws, stock_arena, stock_opts


@contextlib.contextmanager
def guarded_slabs(fill, device):
    """The kernel-level weight-gradient calls: for the block's duration ``srcgan_conv_wgrad`` and ``srcgan_wgrad_dense`` get their split-K
    slab from a guarded, filled buffer of exactly ``*_slab_bytes`` (the descriptor's ``slab`` is redirected to it, whatever the caller
    allocated), and the guards are checked after every call.  Yields the Guard; ``guard.calls`` counts the redirected calls."""
    from srcgan_amd import _native as N
    lib = N.lib()
    g = Guard(fill, device)
    g.calls = 0
    sizes = {"srcgan_conv_wgrad": lambda d: lib.srcgan_conv_wgrad_slab_bytes(d.Cout, d.Cin, d.kh, d.kw, d.nsplit),
             "srcgan_wgrad_dense": lambda d: lib.srcgan_wgrad_dense_slab_bytes(d.G, d.C, d.dtype, d.B, d.H, d.W)}
    stock = {name: getattr(lib, name) for name in sizes}

    def redirect(name):
        def call(dref, stream):
            d = dref._obj                                   # the descriptor behind ctypes.byref
            n = int(sizes[name](d))
            if n > 0:                                       # (0: a shape the planner refuses; the call reports it)
                d.slab = g.carve(name + " slab", "slab", n).data_ptr()
                g.calls += 1
            rc = stock[name](dref, stream)
            g.check()
            g.allocs.clear()
            return rc
        return call

    for name in sizes:
        setattr(lib, name, redirect(name))
    try:
        yield g
    finally:
        for name, fn in stock.items():
            setattr(lib, name, fn)


# ------------------------------------------------------------------------------------------------ the checks of the GPU test
def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def assert_finite(results, what=""):
    """every tensor of {name: tensor or None} is finite"""
    for k, v in results.items():
        if v is not None and v.is_floating_point():
            bad = ~torch.isfinite(v)
            assert not bool(bad.any()), f"{what}: {k} has {int(bad.sum())} non-finite of {v.numel()} elements, first at flat index " \
                                        f"{int(bad.reshape(-1).nonzero()[0, 0])}"


def assert_bit_equal(runs):
    """{run name: {name: tensor or None}}: the same names, None in the same places, and the same bits, in every run."""
    names = list(runs)
    base = runs[names[0]]
    for r in names[1:]:
        other = runs[r]
        assert set(other) == set(base), (names[0], r, set(other) ^ set(base))
        for k, v in base.items():
            w = other[k]
            assert (v is None) == (w is None), f"{k}: None in one of {names[0]} / {r} only"
            if v is None:
                continue
            assert v.shape == w.shape and v.dtype == w.dtype, (k, v.shape, w.shape, v.dtype, w.dtype)
            a, b = _bits(v), _bits(w)
            if not torch.equal(a, b):
                i = int((a != b).nonzero()[0, 0]) // v.element_size()
                raise AssertionError(f"{k} differs between {names[0]} and {r}: {int((a != b).sum())} bytes, first at flat element {i} "
                                     f"({v.reshape(-1)[i].item()!r} vs {w.reshape(-1)[i].item()!r})")


def assert_allocations(guard, expected):
    """What the block recorded is what the planners answer: ``expected`` = [(kind, bytes)], kinds 'workspace', 'grad_arena', 'wpack'."""
    want = sorted((k, int(n)) for k, n in expected)
    assert guard.sizes() == want, f"{guard.fill.name}: recorded {[(a.tag, a.kind, a.nbytes) for a in guard.allocs]}, planners answer {want}"


def run_fills(compute, device, expected=None, stock=True):
    """``compute(guard, scale)`` -> {name: tensor or None}: one whole computation on ``scale`` times its input, calling ``guard.check()``
    (``guard`` is None in the stock run) after each native stage.  Runs it on stock allocation, ZERO, NAN and STALE (whose buffers are those
    of a ZERO block that ran the computation on -3 x its input), and applies every check -> {run name: results}."""
    runs = {}
    if stock:
        runs["stock"] = compute(None, 1.0)
    if callable(expected):                  # sizes that are known only after a run (which parameters got a gradient)
        expected = expected()
    for fill in (ZERO, NAN):
        with guarded(fill, device) as g:
            runs[fill.name] = compute(g, 1.0)
            g.check()
        if expected is not None:
            assert_allocations(g, expected)
    with guarded(ZERO, device) as prev:
        compute(prev, -3.0)
        prev.check()
    with guarded(STALE, device, previous=prev) as g:
        runs["STALE"] = compute(g, 1.0)
        g.check()
    if expected is not None:
        assert_allocations(g, expected)
    for name, res in runs.items():
        assert_finite(res, name)
    assert_bit_equal(runs)
    return runs
