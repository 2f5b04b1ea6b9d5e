"""Shared by the aligner's tests (test_align_gpu.py, align_cascade_cases.py, align_mosaic_cases.py and the tests built on them): the input
generators, the "near a border line" rule the `valid` / cover comparisons exclude pixels by, and the float32 numpy restatement of the
device's sample of a uint8 image through a homography (csrc/u8_image.h u8_sample)."""
import functools

import numpy as np

from bihome_amd import synth


@functools.lru_cache(maxsize=None)
def pixels(n, h, w, seed=0):
    """uint8 [n,h,w,3] random bytes on the host, made once per shape and shared; callers do not modify it."""
    a = np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def textures(n, h, w, seed=0):
    """uint8 [n,h,w,3]: synth.texture_image clipped and rounded to uint8, made once per shape and shared."""
    rng = np.random.default_rng(seed)
    a = np.stack([np.floor(np.clip(synth.texture_image(rng, h, w), 0, 255) + 0.5).astype(np.uint8) for _ in range(n)])
    a.setflags(write=False)
    return a


def corner_homography(seed, Hs, Ws, Ho, Wo, frac=0.2):
    """The homography that sends the corners of the Ho x Wo output onto the corners of the Hs x Ws source moved by up to `frac` of each side."""
    rs = np.random.RandomState(seed)
    co = np.array([[0, 0], [Wo - 1, 0], [Wo - 1, Ho - 1], [0, Ho - 1]], np.float64)
    cs = np.array([[0, 0], [Ws - 1, 0], [Ws - 1, Hs - 1], [0, Hs - 1]], np.float64)
    return synth.four_point_homography(co, cs + rs.uniform(-frac, frac, (4, 2)) * np.array([Ws, Hs]))


def whole_geom(h, w, P, n=1):
    """[n,4]: the geometry record (sx, sy, tx, ty) of the preparation of a whole h x w image."""
    sx, sy = w / P, h / P
    return np.tile(np.array([[sx, sy, 0.5 * sx - 0.5, 0.5 * sy - 0.5]]), (n, 1))


def near_border_points(M, Ho, Wo, Hs, Ws, near):
    """bool [B,Ho,Wo]: the float64 point of grid pixel (x, y) through M [B,3,3] lies within `near` px of one of the four border lines of
    the Hs x Ws image - where a float32 point may fall on the other side of the line."""
    M = np.asarray(M, np.float64).reshape(-1, 3, 3)
    ys, xs = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    out = np.zeros((M.shape[0], Ho, Wo), bool)
    for b, h in enumerate(M):
        with np.errstate(all="ignore"):
            qz = h[2, 0] * xs + h[2, 1] * ys + h[2, 2]
            u, v = (h[0, 0] * xs + h[0, 1] * ys + h[0, 2]) / qz, (h[1, 0] * xs + h[1, 1] * ys + h[1, 2]) / qz
            out[b] = np.minimum.reduce([np.abs(u), np.abs(u - (Ws - 1)), np.abs(v), np.abs(v - (Hs - 1))]) < near
    return out


def f32_fma(a, b, c):
    """float32 fma: the product of two floats is exact in double, one double addition, one rounding to float."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def sample_f32(image, M, Ho, Wo):
    """csrc/u8_image.h u8_sample in float32 numpy, for every pixel of a Ho x Wo grid: warp_tap.h's tap_project / tap_place / tap_weights /
    tap_blend and the validity test.  (The kernel's reciprocal is within an ulp of the division used here.)
    image uint8 [Hs,Ws,3], M [3,3] -> (value float32 [Ho,Wo,3], u, v float32 [Ho,Wo], guard, valid bool [Ho,Wo])"""
    f = np.float32
    Hs, Ws = image.shape[:2]
    ys, xs = np.mgrid[0:Ho, 0:Wo].astype(f)
    h = np.asarray(M, np.float64).reshape(9).astype(f)
    img = image.astype(f)
    with np.errstate(all="ignore"):
        qx, qy, qz = (f32_fma(np.full_like(xs, h[3 * r]), xs, f32_fma(np.full_like(ys, h[3 * r + 1]), ys, h[3 * r + 2])) for r in range(3))
        guard = ~(np.abs(qz) > f(1e-8))
        iz = (f(1) / np.where(guard, f(1), qz)).astype(f)
        u, v = qx * iz, qy * iz
        x0f, y0f = np.floor(u), np.floor(v)
        fx, fy = u - x0f, v - y0f
        x0 = np.clip(np.nan_to_num(x0f, nan=-2.0), -2, Ws).astype(np.int64)
        y0 = np.clip(np.nan_to_num(y0f, nan=-2.0), -2, Hs).astype(np.int64)
        vx0, vx1, vy0, vy1 = (x0 >= 0) & (x0 < Ws), (x0 + 1 >= 0) & (x0 + 1 < Ws), (y0 >= 0) & (y0 < Hs), (y0 + 1 >= 0) & (y0 + 1 < Hs)
        wx0, wx1 = np.where(vx0, f(1) - fx, f(0)), np.where(vx1, fx, f(0))
        wy0, wy1 = np.where(vy0, f(1) - fy, f(0)), np.where(vy1, fy, f(0))
        valid = ~guard & (u >= 0) & (u <= f(Ws - 1)) & (v >= 0) & (v <= f(Hs - 1))
        px = lambda dy, dx: img[np.clip(y0 + dy, 0, Hs - 1), np.clip(x0 + dx, 0, Ws - 1)]          # (a tap outside weighs 0)
        w00, w01, w10, w11 = (wx0 * wy0)[..., None], (wx1 * wy0)[..., None], (wx0 * wy1)[..., None], (wx1 * wy1)[..., None]
        val = f32_fma(px(1, 1), w11, f32_fma(px(1, 0), w10, f32_fma(px(0, 1), w01, px(0, 0) * w00)))
    assert val.dtype == f and u.dtype == f and v.dtype == f
    return val, u, v, guard, valid
