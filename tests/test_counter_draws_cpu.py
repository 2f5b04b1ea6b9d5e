"""Counter-based draws on the CPU: the stream's definition (bihome_amd/synth.py philox4x64_10 against numpy's Philox), the numpy oracle
`synth.counter_draws` (split invariance, ranges, coverage, degenerate ranges, records), the generator's refusals and the C surface."""
import numpy as np
import pytest
import torch

from bihome_amd import synth

KEYS = ("img_idx", "origin", "delta", "photo", "noise", "other")
GEOM = dict(n_images=7, h=240, w=320, patch=32, rho=8)


def same(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("seed,purpose,n", [(42, 0, 0), (7, 1, 2 ** 32 - 1), (2 ** 64 - 1, 0, 2 ** 32), (123456789, 1, 2 ** 63 + 5)])
def test_stated_philox_is_numpys(seed, purpose, n):
    """word k of sample n = element k % 4 of philox4x64_10((k // 4 + 1, n, 0, 0), (seed, purpose)) = Philox(...).random_raw(K)[k]"""
    K = 13
    raw = np.random.Philox(key=np.array([seed, purpose], np.uint64), counter=np.array([0, n, 0, 0], np.uint64)).random_raw(K)
    assert raw.dtype == np.uint64
    for k in range(K):
        assert synth.philox4x64_10((k // 4 + 1, n, 0, 0), (seed, purpose))[k % 4] == int(raw[k]), k
    assert np.array_equal(synth.counter_words(seed, purpose, n, K), raw)
    # the double uniform is Generator.random() of the same bit generator
    g = np.random.Generator(np.random.Philox(key=np.array([seed, purpose], np.uint64), counter=np.array([0, n, 0, 0], np.uint64)))
    assert np.array_equal((raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -53, g.random(K))


def test_dtypes_and_shapes():
    d = synth.counter_draws(42, 0, 3, max_delta=32, blobs=True, **GEOM)
    assert [(k, d[k].dtype, d[k].shape) for k in KEYS] == [
        ("img_idx", np.int32, (3,)), ("origin", np.float32, (3, 2)), ("delta", np.float32, (3, 4, 2)), ("photo", np.float32, (3, 2, 6)),
        ("noise", np.float32, (3, 32, 32)), ("other", np.int32, (3,))]
    assert set(synth.counter_draws(42, 0, 3, **GEOM)) == set(KEYS[:4])
    assert d["noise"].min() >= 0 and d["noise"].max() < 1 and len(np.unique(d["noise"])) > 3000
    assert synth.counter_draws(42, 0, 0, blobs=True, **GEOM)["noise"].shape == (0, 32, 32)


def test_split_invariance():
    """Sample n does not depend on the call it is made in - except `other`, which is a position within the batch."""
    kw = dict(max_delta=32, blobs=True, **GEOM)
    whole = synth.counter_draws(42, 0, 8, **kw)
    a, b = synth.counter_draws(42, 0, 3, **kw), synth.counter_draws(42, 3, 5, **kw)
    same(whole, {k: np.concatenate([a[k], b[k]]) for k in KEYS[:5]}, KEYS[:5])
    first = 2 ** 32 - 3                                                      # the sample index crosses 2^32
    whole = synth.counter_draws(42, first, 8, max_delta=32, **GEOM)
    singles = [synth.counter_draws(42, first + b, 1, max_delta=32, **GEOM) for b in range(8)]
    same(whole, {k: np.concatenate([s[k] for s in singles]) for k in KEYS[:4]}, KEYS[:4])
    assert len({s["delta"].tobytes() for s in singles}) == 8                 # (eight different samples)
    # another seed is another stream
    assert synth.counter_draws(43, 0, 8, **kw)["delta"].tobytes() != synth.counter_draws(42, 0, 8, **kw)["delta"].tobytes()


def test_ranges_and_coverage():
    """Seed 42, samples 0..4095, n_images 7, rho 8: 4096 * 8 delta values over 16 bins would be 2048 per bin; per WORD (one of the eight
    delta entries) it is 256 +- 78 (5 sigma of a binomial with p = 1/16: sqrt(4096 / 16 * 15 / 16) = 15.5), per image index
    585 +- 110 (p = 1/7: sigma 22.4)."""
    d = synth.counter_draws(42, 0, 4096, max_delta=32, **GEOM)
    delta = d["delta"].reshape(4096, 8)
    assert np.array_equal(delta, np.round(delta)) and delta.min() == -8 and delta.max() == 7
    for word in range(8):
        counts = np.bincount((delta[:, word] + 8).astype(np.int64), minlength=16)
        assert counts.shape == (16,) and (np.abs(counts - 256) <= 78).all(), (word, counts)
    counts = np.bincount(d["img_idx"], minlength=7)
    assert counts.shape == (7,) and (np.abs(counts - 585) <= 110).all(), counts
    # origin: rho <= x <= w - rho - P, every value an integer, both ends of the short axis reached
    ox, oy = d["origin"][:, 0], d["origin"][:, 1]
    assert ox.min() >= 8 and ox.max() <= 320 - 8 - 32 and oy.min() == 8 and oy.max() == 240 - 8 - 32
    assert np.array_equal(d["origin"], np.round(d["origin"]))
    # records: each coin near one half, the two contrasts never both on, values inside their ranges
    rec = d["photo"].reshape(-1, 6)
    for col, off in ((0, 0.0), (2, 1.0), (3, 0.0)):
        assert abs((rec[:, col] != off).mean() - 0.5) < 0.03, col
    assert not ((rec[:, 1] != 1) & (rec[:, 4] != 1)).any() and abs(((rec[:, 1] != 1) | (rec[:, 4] != 1)).mean() - 0.5) < 0.03
    assert np.abs(rec[:, 0]).max() <= 32 and np.abs(rec[:, 3]).max() <= 16 and rec[:, 2].min() >= 0.5 and rec[:, 2].max() <= 1.5
    assert set(np.unique(rec[:, 5])) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    # the two records of a sample are different draws
    assert (d["photo"][:, 0] != d["photo"][:, 1]).any(axis=1).mean() > 0.9


@pytest.mark.parametrize("B", [2, 3, 64])
def test_other_is_another_sample(B):
    other = synth.counter_draws(42, 0, B, blobs=True, n_images=3, h=24, w=24, patch=16, rho=4)["other"]
    assert ((other >= 0) & (other < B) & (other != np.arange(B))).all()
    if B == 64:
        assert len(np.unique(other)) > 20


def test_degenerate_ranges():
    d = synth.counter_draws(42, 0, 64, n_images=1, h=32 + 16, w=32 + 16, patch=32, rho=8, max_delta=0)
    assert (d["origin"] == 8).all()                                         # an image of exactly P + 2 rho: one position
    assert (d["img_idx"] == 0).all()
    identity = np.array([0, 1, 1, 0, 1, 0], np.float32)
    assert (d["photo"] == identity).all() and not np.signbit(d["photo"]).any()
    d = synth.counter_draws(42, 0, 64, n_images=2 ** 31 - 1, h=19, w=23, patch=17, rho=1)       # odd patch, minimal height
    assert set(np.unique(d["origin"][:, 1])) == {1.0, 2.0} and d["origin"][:, 0].min() == 1 and d["origin"][:, 0].max() == 6
    assert set(np.unique(d["delta"])) == {-1.0, 0.0}
    assert d["img_idx"].min() >= 0 and d["img_idx"].max() > 2 ** 29
    for bad in (dict(h=47), dict(w=47), dict(rho=0), dict(n_images=0), dict(patch=0)):
        with pytest.raises(ValueError):
            synth.counter_draws(42, 0, 1, **dict(dict(n_images=1, h=48, w=48, patch=32, rho=8), **bad))
    with pytest.raises(ValueError):
        synth.counter_draws(42, 0, 1, blobs=True, **GEOM)


@pytest.mark.parametrize("md", [0, 32, 7.5])
def test_records_are_photometric_records_bitwise(md):
    """The oracle's records against synth_gpu.photometric_records (torch, double) on the same uniforms: the stream's own words of
    samples 0..255, and uniforms at the edges of every formula (0, just below and exactly 0.5, the largest double below 1)."""
    from bihome_amd.synth_gpu import photometric_records
    d = synth.counter_draws(42, 0, 256, max_delta=md, **GEOM)
    u = np.stack([(synth.counter_words(42, 0, n, 36) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 for n in range(256)])
    u = np.stack([u[:, 12:23], u[:, 24:35]], 1)
    want = photometric_records(torch.tensor(u), md).numpy()
    assert want.dtype == np.float32 and d["photo"].tobytes() == want.tobytes()
    edges = np.array([0.0, np.nextafter(0.5, 0), 0.5, np.nextafter(1.0, 0), 5 / 6, np.nextafter(5 / 6, 0)])
    grid = edges[np.random.Generator(np.random.PCG64(3)).integers(0, len(edges), (512, 11))]
    assert synth.counter_photometric_records(grid, md).tobytes() == photometric_records(torch.tensor(grid), md).numpy().tobytes()


def test_generator_refusals():
    from bihome_amd.synth_gpu import GpuPairGenerator
    with pytest.raises(ValueError, match="draws"):
        GpuPairGenerator(n_images=1, device="cpu", draws="philox")
    with pytest.raises(ValueError, match="rank"):
        GpuPairGenerator(n_images=1, device="cpu", draws="counter", rank=2, world=2)
    with pytest.raises(ValueError, match="rank"):
        GpuPairGenerator(n_images=1, device="cpu", rank=-1, world=2)
    counter = GpuPairGenerator(n_images=1, patch=32, rho=8, seed=5, device="cpu", draws="counter", rank=1, world=2)
    default = GpuPairGenerator(n_images=1, patch=32, rho=8, seed=5, device="cpu")
    assert default.draws == "torch" and (default.rank, default.world) == (0, 1)
    assert counter.state_dict() == {"draws": "counter", "seed": 5, "position": 0}
    assert {"draws", "seed", "position", "torch_generator", "random_state"} == set(default.state_dict())
    with pytest.raises(ValueError, match="draws"):
        counter.load_state_dict(default.state_dict())
    with pytest.raises(ValueError, match="draws"):
        default.load_state_dict(counter.state_dict())
    with pytest.raises(ValueError, match="counter"):
        default.draw(2, first=0)
    counter.load_state_dict({"draws": "counter", "seed": 6, "position": 2 ** 40})
    assert counter.state_dict() == {"draws": "counter", "seed": 6, "position": 2 ** 40}
    # torch mode: the saved state continues both host-side streams
    state = default.state_dict()
    a = (torch.rand(3, generator=default.gen), default._rs.randint(1000, size=3))
    default.load_state_dict(state)
    b = (torch.rand(3, generator=default.gen), default._rs.randint(1000, size=3))
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_from_config_passes_the_mode_through(monkeypatch):
    from bihome_amd import configs, synth_gpu
    seen = {}
    monkeypatch.setattr(synth_gpu.GpuPairGenerator, "__init__", lambda self, **kw: seen.update(kw))
    synth_gpu.GpuPairGenerator.from_config(configs.get("zeng-bihome-pds"), seed=3, draws="counter", rank=1, world=4)
    assert (seen["draws"], seen["rank"], seen["world"], seen["seed"]) == ("counter", 1, 4, 3)
    seen.clear()
    synth_gpu.GpuPairGenerator.from_config(configs.get("zeng-bihome-pds"))
    assert (seen["draws"], seen["rank"], seen["world"]) == ("torch", 0, 1)


def test_entry_point_is_exported_and_bound():
    import ctypes
    from bihome_amd import _lib, kernels as K
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bh_synth_draw") and "bh_synth_draw" in _lib.SIGNATURES
    sig = _lib.SIGNATURES["bh_synth_draw"]
    assert sig[:2] == [ctypes.c_size_t] * 2 and ctypes.sizeof(ctypes.c_size_t) == 8 and sig[2:8] == [ctypes.c_int] * 6 and sig[8] is ctypes.c_float and len(sig) == 16
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.synth_draw(0, 0, 1, 48, 48, 32, 8, 0, torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2), torch.zeros(2, 4, 2))
    # refusals need no device: they return before any launch
    null = ctypes.c_void_p(None)
    assert _lib.lib.bh_synth_draw(0, 0, 2, 1, 48, 48, 32, 8, 0.0, null, null, null, null, null, null, null) == -1
    assert _lib.lib.bh_synth_draw(0, 0, 0, 1, 48, 48, 32, 8, 0.0, null, null, null, null, null, null, null) == 0
    assert _lib.lib.bh_synth_draw(0, 0, 0, 0, 48, 48, 32, 8, 0.0, null, null, null, null, null, null, null) == -1
