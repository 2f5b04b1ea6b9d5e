"""Occlusion blobs of the pair generator, host side (bihome_amd/synth.py blob_field / blob_mask / apply_blobs / draw_other; no GPU):
the reference's CollatorWithBlobs (src/data/transforms.py:746-799).  The blur against scipy, the fixture that
tools/make_golden_blobs.py recorded from the reference's own collator (tests/golden/collator_blobs_b4.npz), the flat field, the argument
rules, the configuration mapping, and the distribution of the source index."""
import ctypes

import numpy as np
import pytest

from bihome_amd import configs, synth
from bihome_amd.synth_gpu import batch_spec

EXISTING = ("zeng-bihome", "zeng-bihome-pds", "detone-bihome", "detone-bihome-pds", "zeng-orig", "detone-orig", "nguyen-orig",
            "nguyen-orig-pds", "zhang-orig", "zhang-bihome", "zeng-ihome", "detone-ihome", "zeng-ihome-cos", "detone-ihome-cos",
            "zeng-bihome-aware", "detone-bihome-aware", "zeng-multihead", "detone-multihead", "zeng-ihome-proj", "zeng-ihome-cos-proj",
            "detone-bihome-proj", "zeng-bihome-rgb256")


@pytest.mark.parametrize("P,blobiness", [(32, 0.1), (32, 0.5), (48, 0.2), (128, 0.2), (64, 1.0)])
def test_blur_equals_scipy(P, blobiness):
    from scipy.ndimage import gaussian_filter
    noise = np.random.RandomState(0).rand(P, P)
    sigma = synth.blob_sigma(P, blobiness)
    if (P, blobiness) == (32, 0.1):
        assert int(4 * sigma + 0.5) == P                       # the largest radius one reflection serves: every tap row reflects
    got = synth.gaussian_blur_reflect(noise, sigma)
    want = gaussian_filter(noise, sigma)
    err = np.abs(got - want).max()
    print("P %d blobiness %g: max |restatement - scipy| = %.2e" % (P, blobiness, err))
    assert err <= 1e-12


def test_blob_field_steps_against_scipy():
    """The whole field, step by step with scipy's own filter and erfc (the arithmetic of the fixture tool's stand-in)."""
    from scipy.ndimage import gaussian_filter
    from scipy.special import erfc
    noise = np.random.RandomState(3).rand(64, 64)
    g = gaussian_filter(noise, 64 / (40 * 0.4))
    u = 0.5 * erfc(-((g - g.mean()) / g.std()) / np.sqrt(2))
    u = (u - u.min()) / (u.max() - u.min())
    got = synth.blob_field(noise, 0.4)
    assert got.dtype == np.float64 and got.min() == 0.0 and got.max() == 1.0
    np.testing.assert_allclose(got, u, rtol=0, atol=1e-12)


@pytest.mark.parametrize("C", [1, 3])
def test_fixture_is_reproduced(golden, C):
    g = golden("collator_blobs_b4")
    t = "c%d_" % C
    por, bl = float(g["porosity"]), float(g["blobiness"])
    assert g[t + "noise"].dtype == np.float32 and g[t + "patch_1"].shape == (4, C, 32, 32)
    mask = synth.blob_mask(g[t + "noise"].astype(np.float64), por, bl)
    assert mask.dtype == bool and np.array_equal(mask, g[t + "mask"].astype(bool))
    share = mask.reshape(4, -1).mean(1)
    assert (share > 0.15).all() and (share < 0.45).all(), share            # blobs of about the porosity, in every sample
    out = synth.apply_blobs(g[t + "patch_1"], g[t + "patch_2"], mask, g[t + "other"])
    assert out.dtype == np.float32 and np.array_equal(out, g[t + "out"])
    assert not np.array_equal(out, g[t + "patch_2"])
    # what the composite is: the other sample's patch_1 under the mask, the old patch_2 elsewhere, in every channel
    for b in range(4):
        for c in range(C):
            assert np.array_equal(out[b, c][mask[b]], g[t + "patch_1"][g[t + "other"][b], c][mask[b]])
            assert np.array_equal(out[b, c][~mask[b]], g[t + "patch_2"][b, c][~mask[b]])


def test_constant_noise_is_no_blob():
    for value in (0.0, 0.25, 0.7314):
        noise = np.full((2, 32, 32), value)
        u = synth.blob_field(noise[0], 0.5)
        assert np.isfinite(u).all() and (u == 1.0).all()
        for por in (0.0, 0.5, 1.0):
            assert not synth.blob_mask(noise, por, 0.5).any()
    rs = np.random.RandomState(1)
    p1, p2 = rs.randn(2, 3, 32, 32).astype(np.float32), rs.randn(2, 3, 32, 32).astype(np.float32)
    out = synth.apply_blobs(p1, p2, synth.blob_mask(noise, 0.5, 0.5), np.array([1, 0]))
    assert np.array_equal(out, p2)


def test_porosity_edges():
    noise = np.random.RandomState(2).rand(32, 32)
    u = synth.blob_field(noise, 0.5)
    assert not synth.blob_mask(noise, 0.0, 0.5).any()
    assert np.array_equal(synth.blob_mask(noise, 1.0, 0.5), u < 1.0) and (u < 1.0).sum() == 32 * 32 - (u == u.max()).sum()


def test_argument_rules():
    with pytest.raises(ValueError):
        synth.make_pairs(1, patch=32, blob_porosity=0.3, blobiness=0.5)            # B = 1: no other sample
    with pytest.raises(ValueError):
        synth.draw_other(np.random.default_rng(0), 1)
    with pytest.raises(ValueError):
        synth.apply_blobs(np.zeros((1, 1, 16, 16)), np.zeros((1, 1, 16, 16)), np.zeros((1, 16, 16), bool), np.array([0]))
    for kw in (dict(blob_porosity=0.3, blobiness=0.05), dict(blob_porosity=1.5, blobiness=0.5), dict(blob_porosity=-0.1, blobiness=0.5),
               dict(blob_porosity=0.3), dict(blobiness=0.5)):
        with pytest.raises(ValueError):
            synth.make_pairs(2, patch=32, **kw)
        with pytest.raises(ValueError):
            synth.check_blob_options(kw.get("blob_porosity"), kw.get("blobiness"))
    assert synth.check_blob_options(None, None) is False and synth.check_blob_options(0.1, 0.2) is True
    with pytest.raises(ValueError):
        synth.gaussian_blur_reflect(np.zeros((32, 32)), synth.blob_sigma(32, 0.05))       # radius 64 > 32


def test_generator_options_need_no_gpu_to_be_refused():
    from bihome_amd.synth_gpu import GpuPairGenerator
    for kw in (dict(blob_porosity=0.3), dict(blobiness=0.5), dict(blob_porosity=0.3, blobiness=0.05),
               dict(blob_porosity=1.5, blobiness=0.5)):
        with pytest.raises(ValueError):
            GpuPairGenerator(n_images=1, device="cpu", **kw)


def test_c_entry_point_argument_rules():
    """Checked before any launch (so without a GPU): pointers are never dereferenced here."""
    from bihome_amd import _lib
    f, p = _lib.lib.bh_synth_blobs, ctypes.c_void_p(64)

    def call(noise=p, mask=p, field=None, scratch=None, B=2, C=1, P=32, sigma=1.6, porosity=0.3):
        return f(noise, p, p, p, mask, field, scratch, B, C, P, sigma, porosity, None)
    for bad in (dict(noise=None), dict(mask=None), dict(B=1), dict(B=0), dict(C=2), dict(C=4), dict(sigma=0.0), dict(sigma=-1.0),
                dict(sigma=float("nan")), dict(porosity=1.5), dict(porosity=-0.01), dict(porosity=float("nan")),
                dict(P=256, sigma=6.4)):                               # (P = 256 needs its scratch)
        assert call(**bad) == -1, bad                                  # BH_E_BADARG
    for bad in (dict(P=24), dict(P=0), dict(P=272, scratch=p), dict(P=32, sigma=synth.blob_sigma(32, 0.05)),
                dict(P=128, sigma=synth.blob_sigma(128, 0.09))):
        assert call(**bad) == -2, bad                                  # BH_E_UNSUPPORTED
    assert _lib.lib.bh_synth_blobs_scratch_floats(4, 128) == 0 and _lib.lib.bh_synth_blobs_scratch_floats(4, 32) == 0
    assert _lib.lib.bh_synth_blobs_scratch_floats(3, 256) == 2 * 3 * 256 * 256


def test_batch_spec_and_config():
    cfg = configs.get("zeng-bihome-pds-blobs")
    base = configs.get("zeng-bihome-pds")
    assert cfg["DATA"]["AUGMENT_BLOB_POROSITY"] == 0.1 and cfg["DATA"]["AUGMENT_BLOBINESS"] == 0.2
    del cfg["DATA"]["AUGMENT_BLOB_POROSITY"], cfg["DATA"]["AUGMENT_BLOBINESS"]
    assert cfg == base
    spec = batch_spec(configs.get("zeng-bihome-pds-blobs"))
    assert spec == dict(batch_spec(base), blob_porosity=0.1, blobiness=0.2)
    for name in EXISTING:
        s = batch_spec(configs.get(name))
        assert "blob_porosity" not in s and "blobiness" not in s, name
        assert not any(k.startswith("AUGMENT_BLOB") for k in configs.get(name)["DATA"]), name
    only_one = configs.get("zeng-bihome")
    only_one["DATA"]["AUGMENT_BLOBINESS"] = 0.2                    # train.py:130-131: the collator is built only when both are set
    assert "blobiness" not in batch_spec(only_one)


def test_host_generator_with_blobs_changes_patch_2_only():
    kw = dict(patch=32, seed=5, channels=3)
    plain = synth.make_pairs(3, **kw)
    d = synth.make_pairs(3, blob_porosity=0.3, blobiness=0.5, **kw)
    assert set(d) == set(plain) | {"blob_mask", "blob_other"}
    for k in plain:
        if k != "patch_2":
            assert np.array_equal(d[k], plain[k]), k
    m = d["blob_mask"].astype(bool)
    assert d["blob_mask"].shape == (3, 1, 32, 32) and d["blob_mask"].dtype == np.float32 and m.any() and not m.all()
    m3 = np.broadcast_to(m, d["patch_2"].shape)
    assert np.array_equal(d["patch_2"][~m3], plain["patch_2"][~m3])
    assert np.array_equal(d["patch_2"][m3], plain["patch_1"][d["blob_other"]][m3])
    assert (d["blob_other"] != np.arange(3)).all()


def test_other_index_is_uniform_over_the_others():
    B, n = 4, 6000
    rng = np.random.default_rng(0)
    draws = np.stack([synth.draw_other(rng, B) for _ in range(n)])
    assert (draws != np.arange(B)).all() and draws.min() >= 0 and draws.max() < B
    # per sample b: three cells of expectation n / 3; chi-square with 2 degrees of freedom has mean 2 and sigma 2, so the 5-sigma band
    # ends at 12
    for b in range(B):
        counts = np.array([(draws[:, b] == o).sum() for o in range(B) if o != b])
        chi2 = ((counts - n / 3) ** 2 / (n / 3)).sum()
        print("sample %d: counts %s chi-square %.2f" % (b, counts.tolist(), chi2))
        assert chi2 <= 12.0, (b, counts)
