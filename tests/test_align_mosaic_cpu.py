"""The mosaic, host side (bihome_amd/align.py mosaic_frame_host / mosaic_host / exposure_host; the C entry point bh_mosaic_u8 as far as it
goes without a device): the numpy definitions against independent statements written here, exact cases, and the argument rules.

test_float32_restatement_stays_within_the_measured_shares holds the figures the device test's caps come from (see its docstring)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import align_mosaic_cases as Mc
from bihome_amd import align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH_OK, BH_E_BADARG, BH_E_UNSUPPORTED = 0, -1, -2
I3 = np.eye(3)[None]


# ------------------------------------------------------------------------------------------------
# mosaic_host against a per-pixel loop
# ------------------------------------------------------------------------------------------------
def mosaic_loop(A, B, Ma, Mb, Hc, Wc, feather, mode, gain):
    """The definition pixel by pixel, on sample_host's values: presence and weight from a projection written here."""
    va, vb = align.sample_host(A, Ma[None], Hc, Wc)[0][0], align.sample_host(B, Mb[None], Hc, Wc)[0][0]
    g, o = (1.0, 0.0) if gain is None else gain
    out, cover = np.zeros((Hc, Wc, 3), np.uint8), np.zeros((Hc, Wc), np.uint8)
    for y in range(Hc):
        for x in range(Wc):
            w, present = [], []
            for M, img in ((Ma, A), (Mb, B)):
                Hx, Wx = img.shape[1:3]
                q = M @ np.array([x, y, 1.0])
                if abs(q[2]) > 1e-8:
                    u, v = q[0] * (1.0 / q[2]), q[1] * (1.0 / q[2])
                    present.append(bool(0 <= u <= Wx - 1 and 0 <= v <= Hx - 1))
                    w.append(min(min(u, Wx - 1 - u, v, Hx - 1 - v) + 1.0, feather))
                else:
                    present.append(False)
                    w.append(0.0)
            a, b = g * va[y, x] + o, vb[y, x]
            if mode == "feather":
                if present[0] and present[1]:
                    val = (w[0] * a + w[1] * b) / (w[0] + w[1])
                else:
                    val = (w[0] * a) / w[0] if present[0] else ((w[1] * b) / w[1] if present[1] else np.zeros(3))
            elif mode == "b_over_a":
                val = b if present[1] else (a if present[0] else np.zeros(3))
            else:
                val = a if present[0] else (b if present[1] else np.zeros(3))
            out[y, x] = np.floor(np.clip(val, 0.0, 255.0) + 0.5)
            cover[y, x] = int(present[0]) | int(present[1]) << 1
    return out, cover


@pytest.mark.parametrize("gain", [None, Mc.GAIN], ids=["no-gain", "gain"])
@pytest.mark.parametrize("mode", align.MOSAIC_MODES)
@pytest.mark.parametrize("h,w", [(17, 23), (48, 80)], ids=["17x23", "48x80"])
def test_mosaic_host_equals_the_pixel_loop(h, w, mode, gain):
    A, B = Mc.pixels(1, h, w, seed=1), Mc.pixels(1, h, w, seed=2)
    Ma = Mc.corner_homography(11, h, w, h, w)
    Mb = np.array([[1.0, 0, -2.5], [0, 1, 1.25], [0, 0, 1]])
    out, cover = align.mosaic_host(A, B, Ma[None], Mb[None], h, w, 8.0, mode, None if gain is None else [gain])
    want, want_cover = mosaic_loop(A, B, Ma, Mb, h, w, 8.0, mode, gain)
    assert out.dtype == np.uint8 and cover.dtype == np.uint8 and out.shape == (1, h, w, 3) and cover.shape == (1, h, w)
    assert np.array_equal(cover[0], want_cover) and {0, 1, 2, 3} >= set(np.unique(cover)) and len(np.unique(cover)) >= 3
    # (the two divide in another order: one pixel in thousands may sit on the other side of a rounding boundary, never further)
    d, share = Mc.differing_share(out[0], want)
    assert d <= 1 and share <= 1e-3, (d, share)


def test_mosaic_host_returns_the_recorded_bytes():
    """tests/golden/align_mosaic_host.npz holds mosaic_host's output on this case as it stood before the blend statement was shared with
    pano_host (`_blend_host`): the statement is the reference of every device test, so it moves by no byte."""
    A, B, Ma, Mb, Hc, Wc = Mc.case("48x80-and-40x56-fitted-64x96-vector")
    want = np.load(os.path.join(ROOT, "tests", "golden", "align_mosaic_host.npz"))
    for i, (mode, feather, gain) in enumerate(Mc.COMBOS):
        out, cover = align.mosaic_host(A, B, Ma, Mb, Hc, Wc, feather, mode, Mc.gain_of(gain, len(A)))
        assert np.array_equal(out, want["out%d" % i]) and np.array_equal(cover, want["cover%d" % i]), (mode, feather, gain)
        assert out.dtype == np.uint8 and cover.dtype == np.uint8


def test_mosaic_host_refuses_what_it_does_not_define():
    A = Mc.pixels(1, 17, 23)
    for kw in (dict(mode="over"), dict(feather=0.5), dict(feather=float("nan")), dict(feather=float("inf"))):
        with pytest.raises(ValueError):
            align.mosaic_host(A, A, I3, I3, 17, 23, **kw)


# ------------------------------------------------------------------------------------------------
# exact cases, bitwise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(17, 23), (48, 80)], ids=["17x23", "48x80"])
def test_identity_of_one_image_returns_it(h, w):
    A = Mc.textures(2, h, w, seed=1)
    eye = np.stack([np.eye(3)] * 2)
    for mode in align.MOSAIC_MODES:
        for feather in (1.0, 8.0, 64.0):
            out, cover = align.mosaic_host(A, A, eye, eye, h, w, feather, mode)
            assert np.array_equal(out, A) and np.all(cover == 3), (mode, feather)


def test_integer_translation_values_and_the_four_cover_codes():
    A, B, Ma, Mb, *parts = Mc.translation_case()
    for mode in align.MOSAIC_MODES:
        for feather in (1.0, 4.0):
            out, cover = align.mosaic_host(A, B, Ma, Mb, 17, 23, feather, mode)
            want, want_cover = Mc.translation_want(mode, feather, None, *parts)
            assert np.array_equal(cover[0], want_cover) and set(np.unique(cover)) == {0, 1, 2, 3}
            assert np.array_equal(out[0], want), (mode, feather)
    assert not out[0][cover[0] == 0].any()


def test_a_single_pixel_image_is_present_at_its_one_point():
    A, B = np.array([[[[200, 100, 50]]]], np.uint8), Mc.pixels(1, 5, 7, seed=6)
    Ma = np.array([[[0.5, 0, -1], [0, 0.5, -1], [0, 0, 1]]])       # u = x / 2 - 1, v = y / 2 - 1: (0, 0) at canvas (2, 2) only
    out, cover = align.mosaic_host(A, B, Ma, I3, 5, 7, 8.0, "a_over_b")
    want = np.full((5, 7), 2, np.uint8)
    want[2, 2] = 3
    assert np.array_equal(cover[0], want)
    assert out[0, 2, 2].tolist() == [200, 100, 50] and np.array_equal(out[0][want == 2], B[0][want == 2])
    out, _ = align.mosaic_host(A, B, Ma, I3, 5, 7, 1.0, "feather")          # both weigh 1 there: the mean, half up
    assert np.array_equal(out[0, 2, 2], np.floor((A[0, 0, 0].astype(np.float64) + B[0, 2, 2]) / 2 + 0.5).astype(np.uint8))


def test_a_vanishing_denominator_selects_the_image_out():
    A, B = Mc.textures(1, 48, 80, seed=1), Mc.textures(1, 48, 80, seed=2)
    Ma = np.array([[[1.0, 0, 0], [0, 1, 0], [-0.125, 0, 1]]])      # qz = 1 - x / 8: exactly 0 on the column x = 8
    for mode in align.MOSAIC_MODES:
        out, cover = align.mosaic_host(A, B, Ma, I3, 48, 80, 8.0, mode)
        assert not (cover[0, :, 8] & 1).any() and (cover[0, :, 8] == 2).all() and (cover[0, :, 0] == 3).all()
        assert np.array_equal(out[0, :, 8], B[0, :, 8]), mode


# ------------------------------------------------------------------------------------------------
# mosaic_frame_host
# ------------------------------------------------------------------------------------------------
def project(H, pts):
    q = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ np.asarray(H).T
    return q[:, :2] / q[:, 2:]


HORIZON = np.array([[1.0, 0, 0], [0, 1, 0], [0.02, 0, -1.0]])      # as a map from B to A; its inverse's denominator changes sign across A
GARBAGE = np.array([[1e-3, 0, 0], [0, 1e-3, 0], [0, 0, 1.0]])      # B -> A shrinks a thousandfold: A's corners land a thousand image sizes away


def test_frame_contains_both_and_fits_the_canvas():
    (Ha, Wa), (Hb, Wb), (Hc, Wc) = (48, 80), (40, 56), (64, 96)
    H = np.stack([Mc.corner_homography(11 + b, Ha, Wa, Hb, Wb) for b in range(3)])
    T, bbox, fitted = align.mosaic_frame_host(H, (Ha, Wa), (Hb, Wb), (Hc, Wc))
    assert T.shape == (3, 3, 3) and bbox.shape == (3, 4) and fitted.dtype == np.uint8 and fitted.tolist() == [1, 1, 1]
    ca = np.array([[0, 0], [Wa - 1, 0], [Wa - 1, Ha - 1], [0, Ha - 1]], np.float64)
    for b in range(3):
        x0, y0, x1, y1 = bbox[b]
        assert x0 <= 0 and y0 <= 0 and x1 >= Wb - 1 and y1 >= Hb - 1                     # B's extent
        p = project(np.linalg.inv(H[b]), ca)                                             # A's corners in B's coordinates (nowhere near the clamp)
        assert np.all(p[:, 0] >= x0 - 1e-9) and np.all(p[:, 0] <= x1 + 1e-9) and np.all(p[:, 1] >= y0 - 1e-9) and np.all(p[:, 1] <= y1 + 1e-9)
        assert min(abs(p[:, 0].min() - x0), abs(x0)) <= 1e-9 and min(abs(p[:, 1].max() - y1), abs(y1 - (Hb - 1))) <= 1e-9      # tight
        s = T[b, 0, 0]
        assert T[b, 1, 1] == s and s > 0 and T[b, 2].tolist() == [0, 0, 1] and T[b, 0, 1] == T[b, 1, 0] == 0
        centre = project(T[b], np.array([[(Wc - 1) / 2, (Hc - 1) / 2]]))[0]
        assert np.abs(centre - [(x0 + x1) / 2, (y0 + y1) / 2]).max() <= 1e-9
        c = project(T[b], np.array([[0, 0], [Wc - 1, Hc - 1]], np.float64))              # the canvas covers the box, one axis with equality
        assert c[0, 0] <= x0 + 1e-9 and c[0, 1] <= y0 + 1e-9 and c[1, 0] >= x1 - 1e-9 and c[1, 1] >= y1 - 1e-9
        assert min(abs(c[1, 0] - c[0, 0] - (x1 - x0)), abs(c[1, 1] - c[0, 1] - (y1 - y0))) <= 1e-9


def test_single_frame_with_a_reference_size_is_the_recorded_mosaic_frame():
    """The pair's frame is the sequence's frame rule for the single frame A around a reference of B's size: bitwise what
    mosaic_frame_host returned while it was a statement of its own (tests/golden/align_mosaic_frame_host.npz), on the matrices, sizes and
    canvases of test_align_mosaic_gpu.py's test_frame_device_equals_the_host_statement."""
    sizes = ((48, 80), (40, 56))
    H = np.stack([Mc.corner_homography(11 + b, 48, 80, 40, 56) for b in range(3)]
                 + [HORIZON, GARBAGE, np.zeros((3, 3)), np.full((3, 3), np.nan), np.array([[1.0, 0, 1e6], [0, 1, -1e6], [0, 0, 1]]), np.eye(3)])
    want = np.load(os.path.join(ROOT, "tests", "golden", "align_mosaic_frame_host.npz"))
    for i, (canvas, limit) in enumerate((((64, 96), 2.0), ((37, 53), 0.5), ((2, 2), 2.0))):
        T, bbox, fitted = align.pano_frame_host(H[:, None], sizes[0], canvas, limit, ref_size=sizes[1])
        assert fitted.shape == (9, 1) and fitted.dtype == np.uint8 and fitted[:, 0].tolist() == [1, 1, 1, 0, 1, 0, 0, 1, 1]
        for got, name in ((T, "T"), (bbox, "bbox"), (fitted[:, 0], "fitted")):
            assert got.dtype == want["%s%d" % (name, i)].dtype and got.tobytes() == want["%s%d" % (name, i)].tobytes(), (name, canvas)
        for got, mine in zip(align.mosaic_frame_host(H, *sizes, canvas, limit), (T, bbox, fitted[:, 0])):
            assert got.tobytes() == mine.tobytes()


def test_frame_of_a_horizon_and_of_garbage():
    sizes = ((48, 80), (40, 56), (64, 96))
    bad = [HORIZON, np.zeros((3, 3)), np.full((3, 3), np.nan), np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])]
    T, bbox, fitted = align.mosaic_frame_host(np.stack(bad), *sizes)
    assert fitted.tolist() == [0, 0, 0, 0]
    for b in range(4):
        assert bbox[b].tolist() == [0, 0, 55, 39] and np.isfinite(T[b]).all()
        assert T[b, 0, 0] == max(55 / 95, 39 / 63)
    T, bbox, fitted = align.mosaic_frame_host(GARBAGE[None], *sizes)                     # usable, and clamped to `limit` image sizes
    assert fitted.tolist() == [1] and bbox[0].tolist() == [0, 0, 3 * 56 - 1, 3 * 40 - 1]
    T, bbox, fitted = align.mosaic_frame_host(GARBAGE[None], *sizes, limit=0.5)
    assert bbox[0].tolist() == [0, 0, 1.5 * 56 - 1, 1.5 * 40 - 1]
    far = np.array([[1.0, 0, 1e6], [0, 1, -1e6], [0, 0, 1]])                             # A a million pixels away: the clamp on the other sides
    _, bbox, fitted = align.mosaic_frame_host(far[None], *sizes)
    assert fitted.tolist() == [1] and bbox[0].tolist() == [-2 * 56, 0, 55, 3 * 40 - 1]
    for canvas in ((1, 96), (64, 1)):
        with pytest.raises(ValueError):
            align.mosaic_frame_host(I3, (48, 80), (40, 56), canvas)
    T, bbox, _ = align.mosaic_frame_host(I3, (1, 1), (1, 1), (2, 2))                     # a box without extent: s = 1
    assert T[0, 0, 0] == 1.0 and bbox[0].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------
# exposure_host
# ------------------------------------------------------------------------------------------------
def gray_sums(A, B, H=np.eye(3)):
    return align.ecc_sums_host(align.gray_pyramid_host(A, 1)[0][0], align.gray_pyramid_host(B, 1)[0][0], H)


def test_exposure_recovers_a_known_line():
    A, B = Mc.darkened_pair()
    g, o = align.exposure_host(gray_sums(A, B))
    print("exposure of B = round(0.8 A + 10): g = %.5f, o = %.3f" % (g, o))
    assert abs(g - 0.8) <= 1e-2 and abs(o - 10.0) <= 1.0
    both = align.exposure_host(np.stack([gray_sums(A, B), gray_sums(A, A)]))
    assert both.shape == (2, 2) and both[0].tolist() == [g, o] and abs(both[1, 0] - 1.0) <= 1e-12 and abs(both[1, 1]) <= 1e-9


def test_exposure_fallbacks():
    A, B = Mc.darkened_pair()
    s = gray_sums(A, B)
    S = lambda i, j: align.ecc_index(i, j)
    few = s * (15.0 / s[S(10, 10)])                                 # n = 15: one short of ECC_MIN_N
    flat = gray_sums(np.zeros_like(A), B)                        # A constant: no variance
    negative = gray_sums(A, 255 - A)                                # B falls where A rises: g < 0
    assert few[S(10, 10)] == 15.0 and flat[S(10, 10)] > 1000 and negative[S(10, 10)] > 1000
    for sums in (few, flat, negative, np.zeros(66), np.full(66, np.nan)):
        assert align.exposure_host(sums).tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------
# the float32 restatement of the kernel: the figures behind the device test's caps
# ------------------------------------------------------------------------------------------------
MEASURED = {"17x23-scalar": (1.3e-3, 3.9e-3), "48x80-vector": (1.4e-4, 4.1e-3), "48x80-and-40x56-fitted-64x96-vector": (8.2e-5, 2.7e-3),
            "48x80-and-40x56-fitted-37x53-scalar": (0.0, 3.6e-3), "240x320-fitted-240x320": (7.9e-5, 3.8e-3)}


@pytest.mark.parametrize("name", list(Mc.CASES))
def test_float32_restatement_stays_within_the_measured_shares(name):
    """The share of pixels on which a float32 numpy restatement of the kernel (align_mosaic_cases.mosaic_f32) differs from mosaic_host on
    exactly the device test's inputs, without and with the gain: MEASURED (rounded up), printed; none differs by more than one level and
    no cover code differs away from the border lines."""
    A, B, Ma, Mb, Hc, Wc = Mc.case(name)
    Ha, Wa, Hb, Wb, _, n = Mc.CASES[name]
    worst = [0.0, 0.0]
    na, nb = Mc.near_border(Ma, Hc, Wc, Ha, Wa), Mc.near_border(Mb, Hc, Wc, Hb, Wb)
    for mode, feather, gain in Mc.COMBOS:
        want, want_cover = Mc.reference(name, mode, feather, gain)
        got, cover = Mc.mosaic_f32(A, B, Ma, Mb, Hc, Wc, feather, mode, Mc.gain_of(gain, n))
        d, share = Mc.differing_share(got, want)
        assert d <= 1
        worst[gain is not None] = max(worst[gain is not None], share)
        assert np.array_equal((cover & 1)[~na], (want_cover & 1)[~na]) and np.array_equal((cover & 2)[~nb], (want_cover & 2)[~nb])
    print("%s: float32 restatement differs from float64 on %.2e of the pixels without gain, %.2e with" % (name, worst[0], worst[1]))
    assert worst[0] <= MEASURED[name][0] and worst[1] <= MEASURED[name][1]


# ------------------------------------------------------------------------------------------------
# the C entry point
# ------------------------------------------------------------------------------------------------
MOSAIC_ARGS = ["const uint8_t* images_a", "const int* idx_a", "int n_a", "int Ha", "int Wa", "const uint8_t* images_b", "const int* idx_b", "int n_b",
               "int Hb", "int Wb", "const double* Ma", "const double* Mb", "const double* gain", "int B", "int Hc", "int Wc", "float feather", "int mode",
               "uint8_t* out", "uint8_t* cover", "void* stream"]


def test_header_declares_what_ctypes_binds():
    from bihome_amd import _lib
    from bihome_amd import kernels as K
    raw = open(os.path.join(ROOT, "include", "bihome.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    sig = [P, P, I, I, I, P, P, I, I, I, P, P, P, I, I, I, F, I, P, P, P]
    m = re.search(r"\bint\s+bh_mosaic_u8\s*\(([^)]*)\)\s*;", text)
    assert m, "include/bihome.h does not declare bh_mosaic_u8"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == MOSAIC_ARGS
    assert _lib.SIGNATURES["bh_mosaic_u8"] == sig
    assert list(_lib.lib.bh_mosaic_u8.argtypes) == sig and _lib.lib.bh_mosaic_u8.restype is I
    modes = dict(re.findall(r"#define\s+BH_MOSAIC_(\w+)\s+(\d+)", text))
    assert {k.lower(): int(v) for k, v in modes.items()} == K.MOSAIC_MODES == {m: i for i, m in enumerate(align.MOSAIC_MODES)}


def test_entry_point_argument_rules():
    """Checked before any launch (so without a GPU): pointers are never dereferenced here."""
    from bihome_amd import _lib
    f, p = _lib.lib.bh_mosaic_u8, ctypes.c_void_p(64)

    def call(images_a=p, idx_a=p, n_a=5, Ha=24, Wa=32, images_b=p, idx_b=p, n_b=4, Hb=20, Wb=28, Ma=p, Mb=p, gain=p, B=2, Hc=30, Wc=40,
             feather=32.0, mode=0, out=p, cover=p):
        return f(images_a, idx_a, n_a, Ha, Wa, images_b, idx_b, n_b, Hb, Wb, Ma, Mb, gain, B, Hc, Wc, feather, mode, out, cover, None)
    for bad in (dict(images_a=None), dict(images_b=None), dict(Ma=None), dict(Mb=None), dict(out=None), dict(B=-1), dict(n_a=0), dict(n_b=0),
                dict(Ha=0), dict(Wa=0), dict(Hb=0), dict(Wb=-1), dict(Hc=0), dict(Wc=0), dict(Hc=-3), dict(feather=float("nan")),
                dict(feather=float("inf")), dict(feather=0.999), dict(feather=0.0), dict(feather=-8.0), dict(mode=3), dict(mode=-1),
                dict(B=0, out=None), dict(B=0, mode=7), dict(B=0, feather=0.5), dict(B=0, Hc=0)):
        assert call(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(Ha=1 << 15, Wa=(1 << 14) + 1), dict(Hb=1 << 15, Wb=(1 << 14) + 1), dict(Hc=1 << 16, Wc=1 << 15),
                        dict(B=0, Ha=1 << 15, Wa=(1 << 14) + 1)):
        assert call(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(B=0), dict(B=0, idx_a=None, idx_b=None, gain=None, cover=None), dict(B=0, Ha=1 << 15, Wa=1 << 14, Hb=1 << 15, Wb=1 << 14),
               dict(B=0, Ha=1, Wa=1, Hb=1, Wb=1, Hc=1, Wc=1, feather=1.0, mode=2)):
        assert call(**ok) == BH_OK, ok                                     # an empty batch: nothing launched
    if not torch.cuda.is_available():
        assert call() > 0 and call(idx_a=None, idx_b=None, gain=None, cover=None, Wc=39, mode=1) > 0      # (an accepted call does launch: the launch's own error)


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from bihome_amd import kernels as K
    img, eye = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.mosaic_u8(img, img, eye, eye, torch.zeros(2, 8, 8, 3, dtype=torch.uint8), None, 8.0, "feather")
    with pytest.raises(RuntimeError, match="no CPU path"):
        align.mosaic_u8(img, img, eye, eye, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        align.mosaic(img, img, eye)
