"""Image alignment, host side (bihome_amd/align.py; the C entry points bh_align_prep_u8 / bh_warp_u8 as far as they go without a device):
the three numpy definitions against independent statements written here, and the argument rules of the entry points."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from bihome_amd import align, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH_OK, BH_E_BADARG, BH_E_UNSUPPORTED = 0, -1, -2
MEAN, STD = 0.443, 0.129


def pixels(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (1, h, w, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# preparation
# ------------------------------------------------------------------------------------------------
def prep_brute(image, roi, P, C):
    """The definition, pixel by pixel: every output pixel sums overlap_y * overlap_x * value over the source pixels its interval touches."""
    H, W = image.shape[:2]
    x0, y0, rw, rh = roi
    sx, sy = rw / P, rh / P
    out = np.zeros((C, P, P))
    for y in range(P):
        yl, yh = y0 + y * sy, y0 + (y + 1) * sy
        for x in range(P):
            xl, xh = x0 + x * sx, x0 + (x + 1) * sx
            acc = np.zeros(C)
            for j in range(int(math.floor(yl)), min(int(math.ceil(yh)), H)):
                oy = min(yh, j + 1) - max(yl, j)
                for i in range(int(math.floor(xl)), min(int(math.ceil(xh)), W)):
                    ox = min(xh, i + 1) - max(xl, i)
                    r, g, b = (float(t) for t in image[j, i])
                    acc += oy * ox * (np.array([0.299 * r + 0.587 * g + 0.114 * b]) if C == 1 else np.array([r, g, b]))
            out[:, y, x] = (acc / (sx * sy) / 255.0 - MEAN) / STD
    return out


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("h,w,roi", [(8, 8, None), (16, 16, None), (37, 53, None), (37, 53, (3.25, 2.5, 41.5, 30.25))],
                         ids=["8x8-enlarge", "16x16-same", "37x53-shrink", "37x53-fractional-region"])
def test_prep_host_equals_the_double_loop(h, w, roi, C):
    img = pixels(h, w, seed=h)
    patch, geom = align.prep_host(img, None if roi is None else [roi], 16, C, MEAN, STD)
    full = (0.0, 0.0, float(w), float(h)) if roi is None else roi
    want = prep_brute(img[0], full, 16, C)
    assert patch.shape == (1, C, 16, 16) and patch.dtype == np.float64
    assert np.abs(patch[0] - want).max() <= 1e-11          # (values up to 1 / std = 7.75, sums of a few dozen float64 products)
    x0, y0, rw, rh = full
    assert geom.tolist() == [[rw / 16, rh / 16, x0 + 0.5 * (rw / 16) - 0.5, y0 + 0.5 * (rh / 16) - 0.5]]
    if (h, w) == (16, 16):                                             # sx = sy = 1: the standardised image itself
        v = img[0].astype(np.float64)
        v = (0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])[None] if C == 1 else v.transpose(2, 0, 1)
        assert np.abs(patch[0] - (v / 255.0 - MEAN) / STD).max() <= 1e-12
        assert geom.tolist() == [[1.0, 1.0, 0.0, 0.0]]


@pytest.mark.parametrize("C", [1, 3])
def test_prep_host_constant_image_gives_a_constant_patch(C):
    img = np.full((2, 37, 53, 3), 97, np.uint8)
    patch, _ = align.prep_host(img, [(3.25, 2.5, 41.5, 30.25), (0, 0, 53, 37)], 16, C, MEAN, STD)
    grey = 97.0 if C == 3 else (0.299 + 0.587 + 0.114) * 97.0
    assert np.abs(patch - (grey / 255.0 - MEAN) / STD).max() <= 1e-12


def test_prep_host_refuses_what_it_does_not_define():
    with pytest.raises(ValueError):
        align.prep_host(np.zeros((1, 8, 8, 3), np.float32), None, 16, 1)
    with pytest.raises(ValueError):
        align.prep_host(np.zeros((1, 8, 8, 3), np.uint8), None, 16, 2)


# ------------------------------------------------------------------------------------------------
# lift
# ------------------------------------------------------------------------------------------------
def apply_h(H, pts):
    q = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ H.T
    return q[:, :2] / q[:, 2:]


def apply_geom(g, pts):
    return pts * np.array([g[0], g[1]]) + np.array([g[2], g[3]])


@pytest.mark.parametrize("P", [16, 128])
def test_lift_maps_the_corners_of_b_onto_the_displaced_corners_of_a(P):
    rs = np.random.RandomState(P)
    B = 6
    delta = rs.uniform(-0.25 * P, 0.25 * P, (B, 4, 2))
    geoms = []
    for _ in range(2):
        H, W = rs.randint(P // 2, 8 * P, B), rs.randint(P // 2, 8 * P, B)
        x0, y0 = rs.uniform(0, 0.3, B) * W, rs.uniform(0, 0.3, B) * H
        rw, rh = rs.uniform(0.4, 0.7, B) * W, rs.uniform(0.4, 0.7, B) * H
        sx, sy = rw / P, rh / P
        geoms.append(np.stack([sx, sy, x0 + 0.5 * sx - 0.5, y0 + 0.5 * sy - 0.5], 1))
    Hs = align.lift(delta, P, geoms[0], geoms[1])
    c = align.patch_corners(P)
    assert Hs.shape == (B, 3, 3) and np.all(Hs[:, 2, 2] == 1.0)
    for b in range(B):
        got, want = apply_h(Hs[b], apply_geom(geoms[1][b], c)), apply_geom(geoms[0][b], c + delta[b])
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), b


def test_lift_of_zero_delta_and_one_geometry_is_the_identity():
    g = np.array([[3.7, 2.9, 11.25, 4.5], [1.0, 1.0, 0.0, 0.0]])
    H = align.lift(np.zeros((2, 4, 2)), 128, g, g)
    assert np.abs(H - np.eye(3)).max() <= 1e-12


# ------------------------------------------------------------------------------------------------
# uint8 warp
# ------------------------------------------------------------------------------------------------
def test_warp_identity_returns_the_image():
    img = pixels(17, 23, seed=3)
    out, valid = align.warp_u8_host(img, np.eye(3)[None], 17, 23)
    assert out.dtype == np.uint8 and valid.dtype == np.uint8
    assert np.array_equal(out, img) and np.all(valid == 1)


def test_warp_integer_translation_shifts_and_pads_with_zeros():
    img = pixels(17, 23, seed=4)
    H = np.array([[1.0, 0, 5], [0, 1, -3], [0, 0, 1]])                 # out(x, y) = img(x + 5, y - 3)
    out, valid = align.warp_u8_host(img, H[None], 17, 23)
    want, inside = np.zeros_like(img[0]), np.zeros((17, 23), np.uint8)
    want[3:, :18], inside[3:, :18] = img[0, :14, 5:], 1
    assert np.array_equal(out[0], want) and np.array_equal(valid[0], inside)


def test_warp_half_pixel_shift_rounds_half_up():
    img = np.zeros((1, 4, 6, 3), np.uint8)
    img[0, :, :, 0] = np.array([0, 1, 4, 9, 10, 255])                  # means of neighbours: 0.5, 2.5, 6.5, 9.5, 132.5
    img[0, :, :, 1] = np.array([2, 2, 7, 7, 0, 0])                    # 2, 4.5, 7, 3.5, 0
    H = np.array([[1.0, 0, 0.5], [0, 1, 0], [0, 0, 1]])
    out, valid = align.warp_u8_host(img, H[None], 4, 6)
    assert out[0, :, :5, 0].tolist() == [[1, 3, 7, 10, 133]] * 4       # x.5 goes UP (half to even would give 0, 2, 6, 10, 132)
    assert out[0, :, :5, 1].tolist() == [[2, 5, 7, 4, 0]] * 4
    assert out[0, :, 5, 0].tolist() == [128] * 4                       # the tap outside contributes 0: 255 / 2 = 127.5 -> 128
    assert valid[0].tolist() == [[1, 1, 1, 1, 1, 0]] * 4               # x = 5.5 lies outside [0, 5]


def test_warp_onto_another_size_and_vanishing_denominator():
    img = pixels(12, 20, seed=5)
    out, valid = align.warp_u8_host(img, np.eye(3)[None], 9, 30)
    assert out.shape == (1, 9, 30, 3) and np.array_equal(out[0, :, :20], img[0, :9]) and not out[0, :, 20:].any()
    assert valid[0, :, :20].all() and not valid[0, :, 20:].any()
    H = np.array([[1.0, 0, 0], [0, 1, 0], [-0.125, 0, 1]])             # qz = 1 - x / 8: exactly 0 on the column x = 8
    out, valid = align.warp_u8_host(img, H[None], 12, 20)
    assert not valid[0, :, 8].any() and valid[0, :, 0].all()


# ------------------------------------------------------------------------------------------------
# the C entry points
# ------------------------------------------------------------------------------------------------
PREP_ARGS = ["const uint8_t* images", "const int* idx", "int n_images", "int H", "int W", "const double* roi", "int B", "int P", "int C",
             "float mean", "float std", "float* patch", "double* geom", "void* stream"]
WARP_ARGS = ["const uint8_t* images", "const int* idx", "int n_images", "int Hs", "int Ws", "const double* H64", "int B", "int Ho", "int Wo",
             "uint8_t* out", "uint8_t* valid", "void* stream"]


def test_header_declares_what_ctypes_binds():
    from bihome_amd import _lib
    raw = open(os.path.join(ROOT, "include", "bihome.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    for name, args, sig in (("bh_align_prep_u8", PREP_ARGS, [P, P, I, I, I, P, I, I, I, F, F, P, P, P]),
                            ("bh_warp_u8", WARP_ARGS, [P, P, I, I, I, P, I, I, I, P, P, P])):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/bihome.h does not declare %s" % name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args
        assert _lib.SIGNATURES[name] == sig
        assert list(getattr(_lib.lib, name).argtypes) == sig and getattr(_lib.lib, name).restype is I
    flat = " ".join(raw.split())
    doc = flat[:flat.index("int bh_align_prep_u8(")].rsplit("/*", 1)[1]
    assert "transforms.py:333-354" in doc and "DictStandardize, :369-378" in doc and "CLAMPED" in doc and "eval.py:249-255" in doc
    doc = flat[:flat.index("int bh_warp_u8(")].rsplit("/*", 1)[1]
    assert "src/data/utils.py:54-59" in doc and "PerceptualHead.py:371" in doc and "eval.py:252-254" in doc


def test_prep_entry_point_argument_rules():
    """Checked before any launch (so without a GPU): pointers are never dereferenced here."""
    from bihome_amd import _lib
    f, p = _lib.lib.bh_align_prep_u8, ctypes.c_void_p(64)

    def call(images=p, idx=p, n_images=5, H=24, W=32, roi=p, B=2, P=16, C=1, mean=MEAN, std=STD, patch=p, geom=p):
        return f(images, idx, n_images, H, W, roi, B, P, C, mean, std, patch, geom, None)
    for bad in (dict(images=None), dict(patch=None), dict(geom=None), dict(B=-1), dict(n_images=0), dict(n_images=-2), dict(H=0), dict(H=-1),
                dict(W=0), dict(W=-7), dict(P=0), dict(P=-16), dict(std=0.0), dict(std=float("nan")), dict(B=0, patch=None),
                dict(B=0, W=0), dict(C=2, geom=None), dict(P=17, H=0)):
        assert call(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(C=0), dict(C=2), dict(C=4), dict(P=8), dict(P=17), dict(P=100), dict(P=272), dict(P=512), dict(B=0, C=2),
                        dict(B=0, P=40), dict(H=1 << 16, W=(1 << 14) + 1)):
        assert call(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(B=0), dict(B=0, idx=None, roi=None), dict(B=0, P=256, C=3), dict(B=0, H=1, W=1, n_images=1),
               dict(B=0, H=1 << 16, W=1 << 14)):
        assert call(**ok) == BH_OK, ok                                     # an empty batch: nothing launched
    if not torch.cuda.is_available():
        assert call() > 0 and call(idx=None, roi=None, C=3, P=256) > 0     # (an accepted call does launch: the launch's own error)


def test_warp_entry_point_argument_rules():
    from bihome_amd import _lib
    f, p = _lib.lib.bh_warp_u8, ctypes.c_void_p(64)

    def call(images=p, idx=p, n_images=5, Hs=24, Ws=32, H64=p, B=2, Ho=20, Wo=28, out=p, valid=p):
        return f(images, idx, n_images, Hs, Ws, H64, B, Ho, Wo, out, valid, None)
    for bad in (dict(images=None), dict(H64=None), dict(out=None), dict(B=-1), dict(n_images=0), dict(Hs=0), dict(Hs=-1), dict(Ws=0),
                dict(Ws=-1), dict(Ho=0), dict(Ho=-3), dict(Wo=0), dict(Wo=-1), dict(B=0, out=None), dict(B=0, Ho=0)):
        assert call(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(Hs=1 << 15, Ws=(1 << 14) + 1), dict(Ho=1 << 16, Wo=1 << 15), dict(B=0, Hs=1 << 15, Ws=(1 << 14) + 1)):
        assert call(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(B=0), dict(B=0, idx=None, valid=None), dict(B=0, Hs=1 << 15, Ws=1 << 14), dict(B=0, Hs=1, Ws=1, Ho=1, Wo=1)):
        assert call(**ok) == BH_OK, ok
    if not torch.cuda.is_available():
        assert call() > 0 and call(idx=None, valid=None, Wo=27) > 0


def test_wrappers_and_aligner_refuse_cpu_tensors():
    from bihome_amd import kernels as K
    img, eye = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.align_prep_u8(img, torch.zeros(2, 1, 16, 16), torch.zeros(2, 4, dtype=torch.float64), MEAN, STD)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.warp_u8(img, eye, torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        align.prepare(img, 2, 16, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        align.warp_u8(img, eye, 8, 8)

    class Stub(torch.nn.Sequential):
        pass
    aligner = align.Aligner(Stub(), patch=16)
    assert (aligner.patch, aligner.channels, aligner.patch_keys) == (16, 1, ("patch_1", "patch_2"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        aligner(img, img)
    for kw in (dict(patch=None), dict(patch=24), dict(patch=512), dict(patch=16, channels=2), dict(patch=16, std=0.0)):
        with pytest.raises(ValueError):
            align.Aligner(Stub(), **kw)


def test_aligner_defaults_come_from_the_model():
    from bihome_amd import configs
    from bihome_amd.step import build_model
    aligner = align.Aligner(build_model(configs.get("zeng-bihome"), "cpu"))
    assert (aligner.patch, aligner.channels, aligner.patch_keys) == (128, 1, ("patch_1", "patch_2"))
    assert (aligner.mean, aligner.std) == (0.443, 0.129)
