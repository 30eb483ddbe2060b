"""CPU: pins tests/rdn_ref.py (our float64 restatement of RDN) to the three reference fixtures, so the GPU tests never need the
reference, and shows on it that ``receptive_halo`` = D C + 5 is sufficient and tight."""
import pytest
import torch

import rdn_ref
from conftest import load_golden
from net_ref import stitch

FIXTURES = ("rdn_a_x2", "rdn_b_x3", "rdn_a_x4_gray")
_RUNS = {}


def fixture_run(tag):
    """(fixture, the restatement's float64 run on the seeded weights of the native class), computed once per fixture"""
    if tag not in _RUNS:
        import srcgan_amd
        z = load_golden(tag)
        torch.manual_seed(int(z["seed"]))
        m = srcgan_amd.RDN(scale=int(z["scale"]), G0=int(z["G0"]), RDNconfig=str(z["config"]), n_colors=int(z["n_colors"]))
        _RUNS[tag] = (z, rdn_ref.run(m.state_dict(), torch.from_numpy(z["x"]), torch.from_numpy(z["t"]), str(z["config"]), int(z["scale"])))
    return _RUNS[tag]


@pytest.mark.parametrize("tag", FIXTURES)
def test_rdn_ref_reproduces_the_fixture(tag):
    z, (y, loss, dx, g) = fixture_run(tag)
    assert tuple(rdn_ref.config(str(z["config"]))) == tuple(int(v) for v in z["dcg"])
    assert list(g) == [str(n) for n in z["names"]]
    k64, e64 = rdn_ref.worst(rdn_ref.fixture_errors(z, y, loss, dx, g, "64"))
    k32, e32 = rdn_ref.worst(rdn_ref.fixture_errors(z, y, loss, dx, g, ""))
    print(f"[rdn_ref] {tag}: worst against the float64 values {e64:.2e} ({k64}), against the float32 values {e32:.2e} ({k32})")
    assert e64 < 1e-10, k64
    assert e32 < 1e-4, k32


def test_storage_emulation_and_slice_order_are_the_same_function_in_float64():
    """store=float64 takes the native route through GFF.0 (one K slice per block, summed in order) and rounds nothing."""
    cfg, scale = (3, 2, 32), 3
    sd = rdn_ref.random_state_dict(cfg, scale, G0=32, seed=1)
    g = torch.Generator().manual_seed(2)
    x, t = torch.rand(2, 3, 5, 4, generator=g, dtype=torch.float64), torch.rand(2, 3, 15, 12, generator=g, dtype=torch.float64)
    a, b = rdn_ref.run(sd, x, t, cfg, scale), rdn_ref.run(sd, x, t, cfg, scale, store=torch.float64)
    assert rdn_ref.rel_l2(b[0], a[0]) < 1e-13 and rdn_ref.rel_l2(b[2], a[2]) < 1e-12
    assert max(rdn_ref.rel_l2(b[3][k], a[3][k]) for k in a[3]) < 1e-12
    c = rdn_ref.run(sd, x, t, cfg, scale, store=torch.bfloat16)
    assert 1e-4 < rdn_ref.rel_l2(c[0], a[0]) < 5e-2


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_receptive_halo_is_sufficient_and_tight_in_float64(scale):
    """Crop-stitched tiles with halo = receptive_halo == the whole-scene forward to 1e-10 in float64; one pixel less is NOT enough."""
    import srcgan_amd
    cfg = (2, 3, 32)
    halo = srcgan_amd.receptive_halo(srcgan_amd.RDN(scale=scale, G0=32, RDNconfig=cfg))
    assert halo == 2 * 3 + 5
    sd = rdn_ref.random_state_dict(cfg, scale, G0=32, seed=3, gain=1.5)
    forward = lambda x: rdn_ref.forward(sd, x, cfg, scale)
    x = torch.rand(1, 3, 40, 56, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    with torch.no_grad():
        whole = forward(x)
        tiled = stitch(forward, x, scale, 16, halo)
        short = stitch(forward, x, scale, 16, halo - 1)
    assert tuple(whole.shape[2:]) == (40 * scale, 56 * scale)
    rel = float((tiled - whole).abs().max() / whole.abs().max())
    rel_short = float((short - whole).abs().max() / whole.abs().max())
    print(f"[rdn_ref] x{scale}: halo {halo}: rel {rel:.3e}; halo {halo - 1}: rel {rel_short:.3e}")
    assert rel <= 1e-10
    assert rel_short > 1e-10
