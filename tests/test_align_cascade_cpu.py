"""Cascaded re-prediction, host side (bihome_amd/align.py sample_host / grid_map / prep_warp_host / patch_ncc_host / cascade_compose; the
C entry points bh_align_prep_warp_u8 / bh_patch_ncc as far as they go without a device): the numpy definitions against independent
statements written here, the float32 restatement the GPU test's bound rests on, the host run of the cascade the GPU test replays, and
the argument rules of the entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import align_cascade_cases as Cc
from bihome_amd import align, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH_OK, BH_E_BADARG, BH_E_UNSUPPORTED = 0, -1, -2
MEAN, STD = Cc.MEAN, Cc.STD


# ------------------------------------------------------------------------------------------------
# the warped preparation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
def test_identity_at_an_integer_ratio_is_the_area_average(C):
    """32 x 48, P = 16, the whole image (sx = 3, sy = 2), 3 x 2 sub-samples and H = identity: the sub-samples sit on the pixel centres
    of each cell, so their mean is the exact area average."""
    img = Cc.pixels(2, 32, 48, seed=5)
    want, geom = align.prep_host(img, None, 16, C, MEAN, STD)
    assert geom.tolist() == [[3.0, 2.0, 1.0, 0.5]] * 2
    Hg = np.eye(3)[None] @ align.grid_map(geom, 3, 2)
    got, cover = align.prep_warp_host(img, Hg, 16, C, 3, 2, MEAN, STD)
    err = np.abs(got - want).max()
    print("identity, integer ratio, C = %d: max |prep_warp_host - prep_host| = %.3e" % (C, err))
    assert got.shape == (2, C, 16, 16) and cover.shape == (2, 16, 16) and err <= 1e-12
    assert np.all(cover == 1.0)


def sample_brute(image, h, X, Y):
    """One bilinear sample, written out: -> (rgb [3], valid, guard)."""
    Hs, Ws = image.shape[:2]
    qx, qy, qz = (h[r, 0] * X + h[r, 1] * Y + h[r, 2] for r in range(3))
    guard = not abs(qz) > 1e-8
    if guard:
        return np.zeros(3), False, True
    u, v = qx / qz, qy / qz
    x0, y0 = int(np.floor(u)), int(np.floor(v))
    fx, fy = u - x0, v - y0
    acc = np.zeros(3)
    for yi, wy in ((y0, 1 - fy), (y0 + 1, fy)):
        for xi, wx in ((x0, 1 - fx), (x0 + 1, fx)):
            if 0 <= xi < Ws and 0 <= yi < Hs:
                acc += wy * wx * image[yi, xi].astype(np.float64)
    return acc, 0 <= u <= Ws - 1 and 0 <= v <= Hs - 1, False


def prep_warp_brute(image, h, P, C, nx, ny):
    """The definition, sub-sample by sub-sample."""
    patch, cover = np.zeros((C, P, P)), np.zeros((P, P))
    for y in range(P):
        for x in range(P):
            acc, n = np.zeros(3), 0
            for j in range(ny):
                for i in range(nx):
                    rgb, valid, _ = sample_brute(image, h, x * nx + i, y * ny + j)
                    acc += rgb
                    n += valid
            m = acc / (nx * ny)
            v = np.array([0.299 * m[0] + 0.587 * m[1] + 0.114 * m[2]]) if C == 1 else m
            patch[:, y, x] = (v / 255.0 - MEAN) / STD
            cover[y, x] = n / (nx * ny)
    return patch, cover


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("case", [Cc.WARP_CASES[1], Cc.WARP_CASES[3]], ids=[Cc.WARP_IDS[1], Cc.WARP_IDS[3]])
def test_prep_warp_host_equals_the_sub_sample_loop(case, C):
    bank, Hg = Cc.warp_case(*case)
    (Ha, Wa, _, _, P, nx, ny), b = case, 1
    got, cover = Cc.warp_reference(case, C)
    want, want_cover = prep_warp_brute(bank[Cc.IDX_CLAMPED[b]], Hg[b], P, C, nx, ny)
    assert np.abs(got[b] - want).max() <= 1e-11          # (values up to 1 / std = 7.75, sums of at most 64 x 4 float64 products)
    assert np.array_equal(cover[b], want_cover)
    assert 0.2 < cover.mean() < 1.0 and (cover == 1.0).any() and (cover < 1.0).any()


def test_sample_host_is_the_warp_without_its_rounding():
    img = Cc.pixels(2, 17, 23, seed=3)
    H = np.stack([Cc.corner_homography(7 + b, 17, 23, 19, 21) for b in range(2)])
    values, valid = align.sample_host(img, H, 19, 21)
    out, want_valid = align.warp_u8_host(img, H, 19, 21)
    assert values.dtype == np.float64 and valid.dtype == np.uint8 and np.array_equal(valid, want_valid)
    assert np.array_equal(np.floor(np.clip(values, 0.0, 255.0) + 0.5).astype(np.uint8), out)
    assert np.abs(values - np.round(values)).max() > 0.2          # (not rounded)


def test_a_sample_under_the_guard_contributes_zero_and_is_not_valid():
    img = np.full((1, 12, 20, 3), 200, np.uint8)
    Hg = np.array([[[1.0, 0, 0], [0, 1, 0], [-0.125, 0, 1]]])          # qz = 1 - X / 8: exactly 0 on grid column 8, which patch pixel x = 4 owns
    patch, cover = align.prep_warp_host(img, Hg, 16, 1, 2, 1, MEAN, STD)
    assert np.all(cover[0, :, 4] == 0.0)                                 # column 8 guarded, column 9 projects to u = -72
    assert np.allclose(patch[0, 0, :, 4], (0.0 - MEAN) / STD, atol=1e-12)
    assert np.all(cover[0, :10, 0] == 1.0)                               # X = 0, 1: v = Y and Y / 0.875, inside the 12 rows up to Y = 9


# ------------------------------------------------------------------------------------------------
# the float32 restatement: what the GPU test's bound on the patch rests on
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("case", Cc.WARP_CASES, ids=Cc.WARP_IDS)
def test_f32_restatement_of_the_kernel_stays_inside_the_bound(case, C):
    """Measured here: the float32 restatement of the kernel's arithmetic deviates from the float64 statement by at most 5.1e-5 on the
    inputs the GPU test uses (1.2e-4 on random bytes at 480 x 640, P = 128, 5 x 4, measured once with this function).  Four times that
    is below PREP_BOUND = 7.75e-4, so the GPU test holds the kernel to PREP_BOUND.  cover agrees bit for bit off the border lines, and
    at most 6.6e-3 of the patch pixels (bound: 1e-2) have a sub-sample on one."""
    bank, Hg = Cc.warp_case(*case)
    Ha, Wa, _, _, P, nx, ny = case
    want, want_cover = Cc.warp_reference(case, C)
    got, cover = Cc.prep_warp_f32(bank[list(Cc.IDX_CLAMPED)], Hg, P, C, nx, ny)
    err = np.abs(got.astype(np.float64) - want).max()
    near = Cc.near_border(Hg, P, nx, ny, Ha, Wa)
    print("%s, C = %d: max |float32 restatement - float64| = %.3e (PREP_BOUND %.3e); %.2e of the patch pixels near a border line"
          % (case, C, err, Cc.PREP_BOUND, near.mean()))
    assert 4 * err <= Cc.PREP_BOUND
    assert near.mean() <= 1e-2
    assert np.array_equal(cover[~near], want_cover.astype(np.float32)[~near])


# ------------------------------------------------------------------------------------------------
# composition
# ------------------------------------------------------------------------------------------------
def test_compose_recovers_the_true_map_from_the_residual():
    rs = np.random.RandomState(0)
    P, B = 128, 5
    gb = np.stack([np.array([3.7, 2.9, 11.25, 4.5]), np.array([1.0, 1.0, 0.0, 0.0]), np.array([5.0, 3.75, 2.0, 1.375]),
                   np.array([0.5, 0.25, -0.25, -0.375]), np.array([2.0, 2.0, 0.5, 0.5])])
    c = align.patch_corners(P)
    H_true = np.stack([Cc.corner_homography(b, 300, 400, 300, 400, frac=0.1) for b in range(B)])
    delta = rs.uniform(-0.2 * P, 0.2 * P, (B, 4, 2))
    Ab = align._affine(gb)
    H_prev = np.stack([H_true[b] @ np.linalg.inv(Ab[b] @ synth.four_point_homography(c, c + delta[b]) @ np.linalg.inv(Ab[b])) for b in range(B)])
    H = align.cascade_compose(H_prev, delta, P, gb)
    assert H.shape == (B, 3, 3) and np.all(H[:, 2, 2] == 1.0)
    for b in range(B):
        want = H_true[b] / H_true[b, 2, 2]
        assert np.abs(H[b] - want).max() <= 1e-10 * np.abs(want).max(), b
    # a zero delta changes nothing
    same = align.cascade_compose(H_prev, np.zeros((B, 4, 2)), P, gb)
    for b in range(B):
        want = H_prev[b] / H_prev[b, 2, 2]
        assert np.abs(same[b] - want).max() <= 1e-12 * np.abs(want).max(), b


def test_compose_with_the_identity_before_it_is_the_lift_of_one_geometry():
    gb = np.array([[5.0, 3.75, 2.0, 1.375]])
    d = np.random.RandomState(1).uniform(-20, 20, (1, 4, 2))
    assert np.abs(align.cascade_compose(np.eye(3)[None], d, 128, gb) - align.lift(d, 128, gb, gb)).max() <= 1e-12


# ------------------------------------------------------------------------------------------------
# the score
# ------------------------------------------------------------------------------------------------
def test_ncc_rules():
    rs = np.random.RandomState(2)
    w, t = rs.normal(0.3, 1.0, (3, 3, 16, 16)), rs.normal(-0.2, 2.0, (3, 3, 16, 16))
    t[1] = 0.6 * w[1] + 0.4 * t[1]
    o = align.patch_ncc_host(w, t, None)
    assert o.shape == (3, 8) and np.all(o[:, 0] == 768) and np.all(o[:, 7] == 0) and np.all(np.abs(o[:, 6]) < 1) and o[1, 6] > 0.5
    for b in range(3):                                       # against numpy's own correlation coefficient
        assert abs(o[b, 6] - np.corrcoef(w[b].ravel(), t[b].ravel())[0, 1]) <= 1e-12
        assert np.allclose(o[b, 1:6], [w[b].sum(), t[b].sum(), (w[b] ** 2).sum(), (t[b] ** 2).sum(), (w[b] * t[b]).sum()], rtol=1e-13)
    # blind to a gain and a bias on either input
    for gw, bw, gt, bt in ((2.5, 0.0, 1.0, 0.0), (1.0, -3.0, 1.0, 0.0), (1.0, 0.0, 0.25, 7.0), (3.0, 1.5, 0.5, -2.0)):
        assert np.abs(align.patch_ncc_host(gw * w + bw, gt * t + bt, None)[:, 6] - o[:, 6]).max() <= 1e-12
    assert np.abs(align.patch_ncc_host(w, w, None)[:, 6] - 1.0).max() <= 1e-12
    # only the pixels with cover == 1 count, on all channels
    cover = np.where(rs.uniform(size=(3, 16, 16)) < 0.2, 0.75, 1.0)
    oc = align.patch_ncc_host(w, t, cover)
    for b in range(3):
        keep = cover[b] == 1.0
        assert oc[b, 0] == 3 * keep.sum() < 768
        assert abs(oc[b, 6] - np.corrcoef(w[b][:, keep].ravel(), t[b][:, keep].ravel())[0, 1]) <= 1e-12
    # fewer than 16 counting elements, and a constant input: no score
    few = np.zeros((3, 16, 16))
    few[0].flat[:5] = 1.0                                    # 15 elements
    few[1].flat[:6] = 1.0                                    # 18
    few[2, 3, :] = 1.0
    of = align.patch_ncc_host(w, t, few)
    assert of[:, 0].tolist() == [15.0, 18.0, 48.0] and of[0, 6] == -np.inf and np.isfinite(of[1:, 6]).all()
    const = w.copy()
    const[2] = 1.25
    assert align.patch_ncc_host(const, t, None)[2, 6] == -np.inf and align.patch_ncc_host(t, const, None)[2, 6] == -np.inf
    assert np.isfinite(align.patch_ncc_host(const, t, None)[:2, 6]).all()


# ------------------------------------------------------------------------------------------------
# the cascade on the host (what tests/test_align_cascade_gpu.py replays on the device)
# ------------------------------------------------------------------------------------------------
def test_host_cascade_converges_rejects_and_respects_the_cover():
    s = Cc.cascade_sample(4, 3)
    assert s.accepted == [1, 1, 1, 1] and np.diff(s.score).min() >= 0.02, s.score
    e = [Cc.corner_error(h[0], s.H_true[0], 120, 160) for h in s.H]
    assert e[3] < e[2] < e[1] < e[0] and e[3] < 0.2 * e[0], e
    for d in s.deltas:                                       # what the stub returns is a float32 number
        assert np.array_equal(d, d.astype(np.float32).astype(np.float64))
    g = Cc.cascade_sample(3, 2, garbage=1)
    assert g.accepted == [1, 0, 1] and g.score[1] <= g.score[0] - 0.02 and g.score[2] >= g.score[0] + 0.02, g.score
    assert np.array_equal(g.seen[0], g.seen[1])              # stage 2 starts again from H_0
    c = Cc.cascade_sample(4, 1, min_cover=1.0)
    assert c.accepted == [1, 0] and c.score[1] > c.score[0] and c.count[1] < 32 * 32 and np.array_equal(c.best, c.H[0])


# ------------------------------------------------------------------------------------------------
# the C entry points
# ------------------------------------------------------------------------------------------------
PREP_WARP_ARGS = ["const uint8_t* images", "const int* idx", "int n_images", "int Hs", "int Ws", "const double* Hg", "int B", "int P", "int C",
                  "int nx", "int ny", "float mean", "float std", "float* patch", "float* cover", "void* stream"]
NCC_ARGS = ["const float* w", "const float* t", "const float* cover", "int B", "int C", "int P", "double* out", "void* stream"]


def test_header_declares_what_ctypes_binds():
    from bihome_amd import _lib
    raw = open(os.path.join(ROOT, "include", "bihome.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    for name, args, sig in (("bh_align_prep_warp_u8", PREP_WARP_ARGS, [P, P, I, I, I, P, I, I, I, I, I, F, F, P, P, P]),
                            ("bh_patch_ncc", NCC_ARGS, [P, P, P, I, I, I, P, P])):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/bihome.h does not declare %s" % name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args
        assert _lib.SIGNATURES[name] == sig
        assert list(getattr(_lib.lib, name).argtypes) == sig and getattr(_lib.lib, name).restype is I
    flat = " ".join(raw.split())
    assert flat.index("int bh_ecc_refine(") < flat.index("int bh_align_prep_warp_u8(") < flat.index("int bh_patch_ncc(")
    doc = flat[:flat.index("int bh_align_prep_warp_u8(")].rsplit("/*", 1)[1]
    assert "eval.py:249-255" in doc and "src/data/utils.py:54-67" in doc and "PerceptualHead.py:371" in doc and "CLAMPED" in doc
    assert _lib.lib.bh_version() == 2


def test_prep_warp_entry_point_argument_rules():
    """Checked before any launch (so without a GPU): pointers are never dereferenced here."""
    from bihome_amd import _lib
    f, p = _lib.lib.bh_align_prep_warp_u8, ctypes.c_void_p(64)

    def call(images=p, idx=p, n_images=5, Hs=24, Ws=32, Hg=p, B=2, P=16, C=1, nx=3, ny=2, mean=MEAN, std=STD, patch=p, cover=p):
        return f(images, idx, n_images, Hs, Ws, Hg, B, P, C, nx, ny, mean, std, patch, cover, None)
    for bad in (dict(images=None), dict(Hg=None), dict(patch=None), dict(B=-1), dict(n_images=0), dict(n_images=-2), dict(Hs=0), dict(Hs=-1),
                dict(Ws=0), dict(Ws=-7), dict(P=0), dict(P=-16), dict(std=0.0), dict(std=float("nan")), dict(B=0, patch=None),
                dict(B=0, Ws=0), dict(C=2, Hg=None), dict(P=17, Hs=0), dict(nx=0, images=None)):
        assert call(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(C=0), dict(C=2), dict(C=4), dict(P=8), dict(P=17), dict(P=100), dict(P=272), dict(P=512), dict(nx=0), dict(nx=9),
                        dict(nx=-1), dict(ny=0), dict(ny=9), dict(ny=-3), dict(B=0, C=2), dict(B=0, P=40), dict(B=0, nx=9),
                        dict(Hs=1 << 15, Ws=(1 << 14) + 1)):
        assert call(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(B=0), dict(B=0, idx=None, cover=None), dict(B=0, P=256, C=3, nx=8, ny=8), dict(B=0, Hs=1, Ws=1, n_images=1, nx=1, ny=1),
               dict(B=0, Hs=1 << 15, Ws=1 << 14)):
        assert call(**ok) == BH_OK, ok                                     # an empty batch: nothing launched
    if not torch.cuda.is_available():
        assert call() > 0 and call(idx=None, cover=None, C=3, P=256) > 0   # (an accepted call does launch: the launch's own error)


def test_ncc_entry_point_argument_rules():
    from bihome_amd import _lib
    f, p = _lib.lib.bh_patch_ncc, ctypes.c_void_p(64)

    def call(w=p, t=p, cover=p, B=2, C=1, P=16, out=p):
        return f(w, t, cover, B, C, P, out, None)
    for bad in (dict(w=None), dict(t=None), dict(out=None), dict(B=-1), dict(P=0), dict(P=-16), dict(B=0, out=None), dict(C=2, w=None)):
        assert call(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(C=0), dict(C=2), dict(C=4), dict(P=8), dict(P=17), dict(P=272), dict(B=0, C=2), dict(B=0, P=40)):
        assert call(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(B=0), dict(B=0, cover=None), dict(B=0, P=256, C=3)):
        assert call(**ok) == BH_OK, ok
    if not torch.cuda.is_available():
        assert call() > 0 and call(cover=None, C=3, P=48) > 0


def test_wrappers_and_aligner_refuse_before_any_launch():
    from bihome_amd import kernels as K
    img, eye = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.align_prep_warp_u8(img, eye, torch.zeros(2, 1, 16, 16), torch.zeros(2, 16, 16), 1, 1, MEAN, STD)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.patch_ncc(torch.zeros(2, 1, 16, 16), torch.zeros(2, 1, 16, 16), None, torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        align.prepare_warped(img, eye, 2, 16, 1, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        align.patch_ncc(torch.zeros(2, 1, 16, 16), torch.zeros(2, 1, 16, 16))
    aligner = align.Aligner(torch.nn.Sequential(), patch=16)
    for kw in (dict(cascade=-1), dict(cascade=1.5), dict(cascade="2"), dict(cascade=None), dict(cascade=1, cascade_samples=(0, 1)),
               dict(cascade=1, cascade_samples=(1, 9)), dict(cascade=1, cascade_samples=(2.5, 2)), dict(cascade=1, cascade_samples=3),
               dict(cascade=1, cascade_min_cover=-0.1), dict(cascade=1, cascade_min_cover=1.5), dict(cascade=1, cascade_min_cover=float("nan"))):
        with pytest.raises(ValueError, match="cascade"):
            aligner(img, img, **kw)                            # (CPU tensors: a call that got past these checks says "no CPU path")
    assert align._cascade_samples(None, None, 480, 640, 128) == (5, 4)
    assert align._cascade_samples(None, [(0, 0, 100, 64), (5, 5, 130, 20)], 480, 640, 128) == (2, 1)
    assert align._cascade_samples(None, None, 4000, 6000, 128) == (8, 8) and align._cascade_samples((3, 2), None, 480, 640, 128) == (3, 2)
