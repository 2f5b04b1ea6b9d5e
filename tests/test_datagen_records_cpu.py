"""Host side of the device pair generator (bihome_amd/synth_gpu.py), checked without a GPU: `photometric_records` - the tensor
function that turns uniforms into PhotometricDistortSimple records for photometric_draws='device' - against
`synth.draw_photometric` (which tests/test_datagen_cpu.py pins against the reference's own classes) driven by a replay of the same
uniforms, its distribution over 65 536 records, and `batch_spec`, the mapping from a configuration to generator arguments."""
import ctypes
import itertools
import os
import re

import numpy as np
import torch

from bihome_amd import configs, synth
from bihome_amd.synth_gpu import batch_spec, photometric_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COINS = (0, 2, 3, 5, 7, 9)             # columns of u: brightness, contrast before/after, contrast, saturation, hue, permutation


class Replay:
    """RandomState stand-in that answers draw_photometric's calls from one row of uniforms: the k-th randint(2) reads the coin
    column of the decision draw_photometric takes k-th (the contrast decision comes before saturation and hue if the
    before/after coin fell on 'before', after them otherwise), a uniform reads the column after the coin that switched it on,
    randint(6) the last column.  randint(n) = floor(n u), uniform(lo, hi) = lo + (hi - lo) u."""

    def __init__(self, u):
        self.u = [float(x) for x in u]
        self.order, self.k, self.last = [0, 2], 0, None

    def randint(self, n):
        if n == 6:
            return int(6 * self.u[10])
        col = self.order[self.k]
        self.k += 1
        self.last = col
        bit = int(2 * self.u[col])
        if col == 2:
            self.order += [3, 5, 7, 9] if bit else [5, 7, 3, 9]
        return bit

    def uniform(self, lo, hi):
        return lo + (hi - lo) * self.u[self.last + 1]


def constructed_uniforms():
    """Every on/off combination of the six coins (64 rows) with seeded values in the other columns, then the edges of a coin:
    exactly 0.5 (on), the float32 below it (off), 0 and the largest float32 below 1 in every column."""
    g = torch.Generator().manual_seed(5)
    rows = []
    for bits in itertools.product((0, 1), repeat=6):
        u = torch.rand(11, generator=g)
        for col, bit in zip(COINS, bits):
            u[col] = 0.5 + 0.5 * u[col] if bit else 0.5 * u[col]
        rows.append(u)
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    top = float(np.nextafter(np.float32(1), np.float32(0)))
    rows += [torch.full((11,), v) for v in (0.5, below, 0.0, top)]
    return torch.stack(rows).to(torch.float32)


def test_records_equal_draw_photometric_on_the_same_uniforms():
    u = constructed_uniforms()
    assert len({tuple((u[i, list(COINS)] >= 0.5).tolist()) for i in range(64)}) == 64
    for md in (32, 18):
        got = photometric_records(u, md)
        assert got.dtype == torch.float32 and got.shape == (len(u), 6)
        want = np.stack([synth.draw_photometric(Replay(row), md) for row in u.double().numpy()])
        # float32 uniforms, arithmetic in double on both sides, one rounding to float32 on ours
        np.testing.assert_allclose(got.double().numpy(), want, rtol=1e-6, atol=0)
    # both images of a pair at once, as GpuPairGenerator.draw() calls it
    pair = photometric_records(u[:64].reshape(32, 2, 11), 32)
    assert torch.equal(pair.reshape(64, 6), photometric_records(u[:64], 32))


def test_record_distribution():
    n = 65536
    u = torch.rand((n, 11), generator=torch.Generator().manual_seed(0))
    r = photometric_records(u, 32).double().numpy()
    br, c1, sat, hue, c2, perm = r.T
    # every decision is a fair coin: 0.5 +- 0.01 is about 5 sigma of the binomial at n = 65536 (sigma = 0.00195).  Contrast lands
    # in c1 or c2 by a second fair coin (0.25 each) and an 'on' permutation is the identity one time in six (5/12 visible).
    freq = {"brightness": (br != 0).mean(), "contrast": ((c1 != 1) | (c2 != 1)).mean(), "saturation": (sat != 1).mean(),
            "hue": (hue != 0).mean(), "permutation": (perm != 0).mean() * 6 / 5,
            "contrast before": (c1 != 1).mean() * 2, "contrast after": (c2 != 1).mean() * 2}
    print("MEASURED on/off frequencies over %d records: %s" % (n, {k: round(float(v), 4) for k, v in freq.items()}))
    for k, v in freq.items():
        assert abs(v - 0.5) <= 0.01, (k, v)
    assert not ((c1 != 1) & (c2 != 1)).any()                       # contrast before OR after the HSV part, never both
    assert sorted(np.unique(perm)) == [0, 1, 2, 3, 4, 5]
    # the values are uniform over the reference's intervals (:152-155, :301-302, :206-210)
    for v, lo, hi in ((br[br != 0], -32, 32), (c1[c1 != 1], 0.5, 1.5), (c2[c2 != 1], 0.5, 1.5), (sat[sat != 1], 0.5, 1.5),
                      (hue[hue != 0], -16, 16)):
        assert lo <= v.min() and v.max() <= hi
        # mean of m uniforms: sigma = (hi - lo) / sqrt(12 m); 5 sigma
        assert abs(v.mean() - (lo + hi) / 2) <= 5 * (hi - lo) / np.sqrt(12 * len(v))
    ident = photometric_records(u[:256], 0)
    assert torch.equal(ident, torch.tensor([0., 1., 1., 0., 1., 0.]).expand(256, 6))


def test_batch_spec():
    want = {
        "zeng-bihome": dict(patch=128, rho=32, channels=1, photometric_max_delta=0, target_gen=None, image=False, corners=False),
        "zeng-bihome-pds": dict(patch=128, rho=32, channels=1, photometric_max_delta=32, target_gen=None, image=False,
                                corners=False),
        "zeng-orig": dict(patch=128, rho=32, channels=1, photometric_max_delta=0, target_gen="all_points", image=False,
                          corners=True),
        "detone-orig": dict(patch=128, rho=32, channels=1, photometric_max_delta=0, target_gen="4_points", image=False,
                            corners=True),
        "nguyen-orig": dict(patch=128, rho=32, channels=1, photometric_max_delta=0, target_gen="4_points", image=True,
                            corners=True),
        "zeng-bihome-rgb256": dict(patch=256, rho=64, channels=3, photometric_max_delta=0, target_gen=None, image=False,
                                   corners=False),
    }
    for name, spec in want.items():
        assert batch_spec(configs.get(name)) == spec, name


def test_header_declares_bh_synth_batch_as_bound():
    from bihome_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bihome.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bh_synth_batch\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/bihome.h does not declare bh_synth_batch"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    want = [ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "float": ctypes.c_float}[a.split()[0]] for a in args]
    assert _lib.SIGNATURES["bh_synth_batch"] == want and len(want) == 17
    assert [a.split()[-1].lstrip("*") for a in args] == ["images", "img_idx", "origin", "Hpatch", "photo", "B", "n_images", "Hs", "Ws",
                                                        "P", "C", "mean", "std", "patch1", "patch2", "target", "stream"]
    assert args[3].startswith("const double*") and args[15].startswith("float*")


def test_bh_synth_batch_argument_rules():
    """bh_synth_pairs' rules, checked before any launch (so without a GPU): pointers are never dereferenced here."""
    from bihome_amd import _lib
    f, p = _lib.lib.bh_synth_batch, ctypes.c_void_p(64)

    def call(images=p, photo=None, B=2, P=32, C=1, std=0.129, patch1=p, target=None):
        return f(images, p, p, p, photo, B, 1, 48, 64, P, C, 0.443, std, patch1, p, target, None)
    assert call(B=0) == 0 and call(B=0, C=3, target=p, photo=p) == 0
    for bad in (dict(images=None), dict(patch1=None), dict(std=0.0), dict(C=2), dict(C=0), dict(C=4), dict(B=-1)):
        assert call(**bad) == -1, bad                              # BH_E_BADARG
    assert call(P=24) == -2 and call(P=24, C=3, target=p) == -2    # BH_E_UNSUPPORTED
    assert call(P=24, C=2) == -1                                   # a bad argument is reported first, as bh_synth_pairs does
