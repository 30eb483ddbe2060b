"""The GPU side of the network families' tests (tests/test_gpu_<family>.py), in one place: the native training step, the fp32 gate
and the 16-bit gate against the float64 restatement, the no_grad path and the two whole-scene checks.  A test builds its case and
calls the check; the lines the checks print (pytest -s) are the ones DESIGN.md's figures were read from."""
import pytest
import torch

from conftest import rel_err, rel_l2

F32_TOL = 1e-3
STORE = {"bf16": torch.bfloat16, "fp16": torch.float16}


def bound16(e):
    """The project's 16-bit yardstick: against float64, the native relative L2 error may not exceed 1.5 x the error ``e`` of the float64
    restatement with 16-bit STORAGE (+ 5e-3), on y, dx and the worst parameter gradient.

    The networks' tests run it with a static loss scale of 1024, as 16-bit training does: the native backward stores its gradient
    tensors in the 16-bit type, the emulation rounds the forward only.  The mean-reduced L1 loss hands 1 / N = 2.2e-4 (DDBPN x4:
    N = 4608) to every output element; two layers of weights around 0.02 further in, the gradients lie below float16's smallest normal
    number 2^-14 = 6.1e-5, where only a few bits are left.  Without the scale the DDBPN x4 float16 case measured 0.040 on
    downmodules.4.conv_2.0.weight against a bound of 0.037 on an MI355X (the emulation with its gradients rounded to float16 too gives
    0.138 for that tensor on the CPU); with it, that emulation returns to the forward-only figures, so the rule compares like with like."""
    return 1.5 * e + 5e-3


def step(m, x, t, loss_scale=1.0):
    """native forward, L1 loss (times loss_scale), backward -> (y, loss, dx, {name: grad}) on the CPU; a parameter whose .grad is None has no entry"""
    for p in m.parameters():
        p.grad = None
    x = x.detach().cuda().requires_grad_(True)
    y = m(x)
    loss = torch.nn.functional.l1_loss(y, t.cuda()) * loss_scale
    loss.backward()
    return y.detach().cpu(), float(loss.detach()), x.grad.cpu(), {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None}


def _same_names(g, gr, names):
    assert names in ("set", "list")
    return set(g) == set(gr) if names == "set" else list(g) == list(gr)


def check_fp32(tag, who, got, ref, *, names, skip=(), tail=""):
    """The fp32 gate: ``got`` = step(...) against ``ref`` = the float64 restatement's run, in ``rel_err``, at F32_TOL on y, the relative
    loss difference, dx and the worst parameter gradient; the gradients' names must be the restatement's, as a set or as a list.
    ``skip``: gradients left out of the relative measure (the caller holds them to another one and reports it in ``tail``)."""
    (y, loss, dx, g), (yr, lr, dxr, gr) = got, ref
    assert _same_names(g, gr, names), (list(g), list(gr))
    errs = sorted(((rel_err(g[k], gr[k]), k) for k in gr if k not in skip), reverse=True)
    print(f"[{tag}] {who} fp32 vs float64: y {rel_err(y, yr):.2e} loss {abs(loss - float(lr)) / float(lr):.2e} dx {rel_err(dx, dxr):.2e} "
          f"worst {'live ' if skip else ''}grads {[(f'{e:.2e}', k) for e, k in errs[:3]]}{tail}")
    assert rel_err(y, yr) < F32_TOL and abs(loss - float(lr)) < F32_TOL * float(lr) and rel_err(dx, dxr) < F32_TOL and errs[0][0] < F32_TOL


def check_fixture(tag, who, e):
    """The fp32 gate on a family's ``fixture_errors`` (measured in ``rel_err``): y, loss, dx and the worst gradient at F32_TOL"""
    worst = sorted(((v, k) for k, v in e.items() if k.startswith("grad ")), reverse=True)
    print(f"[{tag}] {who}: y {e['y']:.2e} loss {e['loss']:.2e} dx {e['dx']:.2e} worst grads {[(f'{v:.2e}', k[5:]) for v, k in worst[:3]]}")
    assert e["y"] < F32_TOL and e["loss"] < F32_TOL and e["dx"] < F32_TOL
    assert worst[0][0] < F32_TOL, worst[:3]


def check_16bit(tag, who, dtype, got, ref, emu, *, names, skip=(), tails=("", "")):
    """The 16-bit gate: ``bound16`` in ``rel_l2`` on y, dx and the worst parameter gradient of ``got`` = step(...) against ``ref``, the
    float64 restatement's run, with ``emu``, its run under storage emulation, as the yardstick; every native gradient finite; names
    and ``skip`` as in check_fp32 (``tails``: one for the native line, one for the emulation's)."""
    (y, _, dx, g), (yr, _, dxr, gr), (ye, _, dxe, ge) = got, ref, emu
    assert _same_names(g, gr, names), (list(g), list(gr))
    nat = sorted(((rel_l2(g[k], gr[k]), k) for k in gr if k not in skip), reverse=True)
    emv = sorted(((rel_l2(ge[k], gr[k]), k) for k in gr if k not in skip), reverse=True)
    head, grads = f"[{tag}] {who + ' ' if who else ''}{dtype}", f"worst {'live ' if skip else ''}grads"
    print(f"{head} native vs float64: y {rel_l2(y, yr):.4f} dx {rel_l2(dx, dxr):.4f} {grads} {nat[:2]}{tails[0]}")
    print(f"{head} storage emulation vs float64: y {rel_l2(ye, yr):.4f} dx {rel_l2(dxe, dxr):.4f} {grads} {emv[:2]}{tails[1]}")
    assert all(torch.isfinite(v).all() for v in g.values())
    assert rel_l2(y, yr) < bound16(rel_l2(ye, yr))
    assert rel_l2(dx, dxr) < bound16(rel_l2(dxe, dxr))
    assert nat[0][0] < bound16(emv[0][0])


def check_no_grad_bits(m, x):
    """With grad mode on the output is on the graph; under no_grad it has the same bits and is off it; a second backward through the
    same output raises (the activations were released).  -> the grad-mode output"""
    x = x.cuda()
    y = m(x)
    assert y.grad_fn is not None
    with torch.no_grad():
        yi = m(x)
    assert yi.grad_fn is None and not yi.requires_grad and torch.equal(yi, y.detach())
    y.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="twice"):
        y.sum().backward()
    return y


def check_one_tile_scene(m, scene, up, out_shape, **kw):
    """``upscale_scene`` on a plan of one 32-pixel tile has the bits of the module's no_grad forward (``kw``: further arguments of
    upscale_scene)"""
    from srcgan_amd import infer
    assert len(infer.plan_tiles(scene.shape[2], scene.shape[3], 32, 8, 1).tiles) == 1
    with torch.no_grad():
        whole = m(scene)
    got = infer.upscale_scene(m, scene, up=up, tile=32, halo=8, blend="feather", **kw)
    assert tuple(got.shape) == tuple(out_shape) and torch.equal(got, whole)


def check_exact_tiles(tag, m, scene, up, tile, n_tiles, out_shape, halo=None):
    """``upscale_scene`` with halo = receptive_halo (crop) against the same module's whole-image no_grad forward; gate: the exact-mode
    tests' fp32 gate, rel_err < 1e-3 (tests/test_gpu_infer_scene.py).  The tiles' convolutions see other tile shapes than the whole
    image's, so the bits may differ; the value is printed.  ``halo``: what receptive_halo must say, where the caller knows."""
    from srcgan_amd import infer
    h = infer.receptive_halo(m)
    assert halo is None or h == halo
    assert len(infer.plan_tiles(scene.shape[2], scene.shape[3], tile, h, 1).tiles) == n_tiles
    with torch.no_grad():
        whole = m(scene)
    got = infer.upscale_scene(m, scene, up=up, tile=tile)
    err = rel_err(got, whole)
    print(f"[{tag}] {f'x{up} ' if up > 1 else ''}exact mode, 2 x 2 tiles, halo {h}: tiled vs whole-image rel_err {err:.3e}")
    assert tuple(got.shape) == tuple(out_shape) and err < 1e-3
