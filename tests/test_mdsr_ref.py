"""CPU: pins tests/mdsr_ref.py (our float64 restatement of MDSR and VDSR) to the four reference fixtures, so the GPU tests never need
the reference, and shows on it that ``receptive_halo`` = 2 n_resblocks + 12 (MDSR) / n_resblocks (VDSR) is sufficient and tight."""
import pytest
import torch

import mdsr_ref
from conftest import load_golden
from net_ref import stitch

MDSR_FIXTURES = ("mdsr_s234_idx0", "mdsr_s234_idx1", "mdsr_s234_idx2")
FIXTURES = MDSR_FIXTURES + ("vdsr",)
_RUNS = {}


def native(z, tag, **kw):
    """the native class with the fixture's seeded weights"""
    import srcgan_amd
    torch.manual_seed(int(z["seed"]))
    if tag == "vdsr":
        return srcgan_amd.VDSR(n_resblocks=int(z["cfg"][0]), n_feats=int(z["cfg"][1]), rgb_range=int(z["cfg"][2]), **kw)
    m = srcgan_amd.MDSR(n_resblocks=int(z["cfg"][0]), n_feats=int(z["cfg"][1]), scale=[int(s) for s in z["scales"]], rgb_range=int(z["cfg"][2]), **kw)
    m.set_scale(int(z["cfg"][3]))
    return m


def ref_run(z, tag, sd, **kw):
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    if tag == "vdsr":
        return mdsr_ref.vdsr_run(sd, x, t, int(z["cfg"][0]), **kw)
    return mdsr_ref.mdsr_run(sd, x, t, int(z["cfg"][0]), [int(s) for s in z["scales"]], int(z["cfg"][3]), **kw)


def fixture_run(tag):
    """(fixture, the restatement's float64 run on the seeded weights of the native class), computed once per fixture"""
    if tag not in _RUNS:
        z = load_golden(tag)
        _RUNS[tag] = (z, ref_run(z, tag, native(z, tag).state_dict()))
    return _RUNS[tag]


@pytest.mark.parametrize("tag", FIXTURES)
def test_mdsr_ref_reproduces_the_fixture(tag):
    z, (y, loss, dx, g) = fixture_run(tag)
    names = [str(n) for n in z["names"]]
    assert names == (mdsr_ref.vdsr_names(int(z["cfg"][0])) if tag == "vdsr" else mdsr_ref.mdsr_names(int(z["cfg"][0]), [int(s) for s in z["scales"]]))
    assert set(names) == set(g) | {str(k) for k in z["nograd"]} | {str(k) for k in z["frozen"]}
    if tag != "vdsr":
        assert list(g) == mdsr_ref.mdsr_branch(int(z["cfg"][0]), [int(s) for s in z["scales"]], int(z["cfg"][3]))
    k64, e64 = mdsr_ref.worst(mdsr_ref.fixture_errors(z, y, loss, dx, g, "64"))
    k32, e32 = mdsr_ref.worst(mdsr_ref.fixture_errors(z, y, loss, dx, g, ""))
    print(f"[mdsr_ref] {tag}: worst against the float64 values {e64:.2e} ({k64}), against the float32 values {e32:.2e} ({k32})")
    assert e64 < 1e-10, k64
    assert e32 < 1e-4, k32


def test_the_three_fixtures_are_one_instance():
    a, b, c = (load_golden(t) for t in MDSR_FIXTURES)
    assert int(a["seed"]) == int(b["seed"]) == int(c["seed"]) and [int(v["cfg"][3]) for v in (a, b, c)] == [0, 1, 2]
    for k in a:
        if k.startswith("wsketch/"):
            assert (a[k] == b[k]).all() and (a[k] == c[k]).all()
    assert len(a["names"]) == 50 and len(a["nograd"]) == 22 and len(c["nograd"]) == 20 and len(a["frozen"]) == 4


def test_storage_emulation_in_float64_rounds_nothing():
    z, (y, _, dx, g) = fixture_run("mdsr_s234_idx2")
    sd = native(z, "mdsr_s234_idx2").state_dict()
    b = ref_run(z, "mdsr_s234_idx2", sd, store=torch.float64)
    assert mdsr_ref.rel_l2(b[0], y) < 1e-13 and mdsr_ref.rel_l2(b[2], dx) < 1e-12 and max(mdsr_ref.rel_l2(b[3][k], g[k]) for k in g) < 1e-12
    c = ref_run(z, "mdsr_s234_idx2", sd, store=torch.bfloat16)
    assert 1e-4 < mdsr_ref.rel_l2(c[0], y) < 5e-2


def _sufficient_and_tight(forward, x, up, halo, who):
    with torch.no_grad():
        whole = forward(x)
        tiled = stitch(forward, x, up, 16, halo)
        short = stitch(forward, x, up, 16, halo - 1)
    assert tuple(whole.shape[2:]) == (x.shape[2] * up, x.shape[3] * up)
    rel = float((tiled - whole).abs().max() / whole.abs().max())
    rel_short = float((short - whole).abs().max() / whole.abs().max())
    print(f"[mdsr_ref] {who}: halo {halo}: rel {rel:.3e}; halo {halo - 1}: rel {rel_short:.3e}")
    assert rel <= 1e-10
    assert rel_short > 1e-10


def _gained(m, gain):
    return {k: (v.double() * gain if k.endswith("weight") and "mean" not in k else v.double()) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("idx, scale", [(0, 2), (1, 3), (2, 4), (3, 8)])
def test_mdsr_receptive_halo_is_sufficient_and_tight_in_float64(idx, scale):
    """Crop-stitched tiles with halo = receptive_halo == the whole-scene forward to 1e-10 in float64; one pixel less is NOT enough."""
    import srcgan_amd
    torch.manual_seed(3)
    m = srcgan_amd.MDSR(n_resblocks=1, n_feats=16, scale=(2, 3, 4, 8), rgb_range=1)
    m.set_scale(idx)
    halo = srcgan_amd.receptive_halo(m)
    assert halo == 2 * 1 + 12
    sd = _gained(m, 2.0)
    x = torch.rand(1, 3, 40, 56, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    _sufficient_and_tight(lambda v: mdsr_ref.mdsr_forward(sd, v, 1, [2, 3, 4, 8], idx), x, scale, halo, f"MDSR x{scale}")


def test_vdsr_receptive_halo_is_sufficient_and_tight_in_float64():
    import srcgan_amd
    torch.manual_seed(4)
    m = srcgan_amd.VDSR(n_resblocks=5, n_feats=16, rgb_range=1)
    halo = srcgan_amd.receptive_halo(m)
    assert halo == 5
    sd = _gained(m, 2.0)
    x = torch.rand(1, 3, 40, 56, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    _sufficient_and_tight(lambda v: mdsr_ref.vdsr_forward(sd, v, 5), x, 1, halo, "VDSR")
