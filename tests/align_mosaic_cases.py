"""Shared by tests/test_align_mosaic_cpu.py and tests/test_align_mosaic_gpu.py: the inputs of the mosaic cases (the generators of
tests/align_cases.py), their float64 references (computed once), a float32 numpy restatement of the kernel's arithmetic, the
stub model and the 1/16-pixel delta construction of test_align_gpu.py's test_direction_and_lift_end_to_end."""
import functools

import numpy as np
import torch

import align_cases
from align_cases import corner_homography, f32_fma, near_border_points, pixels, textures, whole_geom
from bihome_amd import align

NEAR = 1e-3                      # cover is compared where the float64 point is at least this far (px) from a border line of the image
GAIN = (0.9, 6.0)
# every combination the kernel cases run: the feather matters to the blend only
COMBOS = [("feather", f, g) for f in (1.0, 8.0, 64.0) for g in (None, GAIN)] + [(m, 8.0, g) for m in ("b_over_a", "a_over_b") for g in (None, GAIN)]

# name -> (Ha, Wa, Hb, Wb, canvas or None for B's grid, samples)
CASES = {
    "17x23-scalar": (17, 23, 17, 23, None, 2),
    "48x80-vector": (48, 80, 48, 80, None, 2),
    "48x80-and-40x56-fitted-64x96-vector": (48, 80, 40, 56, (64, 96), 2),
    "48x80-and-40x56-fitted-37x53-scalar": (48, 80, 40, 56, (37, 53), 2),
    "240x320-fitted-240x320": (240, 320, 240, 320, (240, 320), 1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(A uint8 [n,Ha,Wa,3], B uint8 [n,Hb,Wb,3], Ma [n,3,3], Mb [n,3,3], Hc, Wc): textures of seeds 1 and 2, H = corner_homography(11 + b)
    from B's grid to A, T the identity (B's grid) or mosaic_frame_host's."""
    Ha, Wa, Hb, Wb, canvas, n = CASES[name]
    A, B = textures(2, Ha, Wa, seed=1)[:n], textures(2, Hb, Wb, seed=2)[:n]
    H = np.stack([corner_homography(11 + b, Ha, Wa, Hb, Wb) for b in range(n)])
    if canvas is None:
        Hc, Wc, T = Hb, Wb, np.stack([np.eye(3)] * n)
    else:
        (Hc, Wc), T = canvas, align.mosaic_frame_host(H, (Ha, Wa), (Hb, Wb), canvas)[0]
    Ma = H @ T
    for x in (Ma, T):
        x.setflags(write=False)
    return A, B, Ma, T, Hc, Wc


def gain_of(g, n):
    return None if g is None else np.tile(np.array([g], np.float64), (n, 1))


@functools.lru_cache(maxsize=None)
def reference(name, mode, feather, gain):
    """mosaic_host of the case: (out uint8 [n,Hc,Wc,3], cover uint8 [n,Hc,Wc])."""
    A, B, Ma, Mb, Hc, Wc = case(name)
    return align.mosaic_host(A, B, Ma, Mb, Hc, Wc, feather, mode, gain_of(gain, len(A)))


def near_border(M, Ho, Wo, Hs, Ws):
    """bool [B,Ho,Wo]: the float64 point of the canvas pixel lies within NEAR px of one of the four border lines of the Hs x Ws image."""
    return near_border_points(M, Ho, Wo, Hs, Ws, NEAR)


def differing_share(got, want):
    """(largest difference in grey levels, share of the pixels that differ at all)."""
    d = np.abs(np.asarray(got).astype(np.int32) - np.asarray(want).astype(np.int32))
    return int(d.max()), float((d.max(-1) > 0).mean())


# ------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy
# ------------------------------------------------------------------------------------------------
def sample_f32(image, M, Ho, Wo, feather):
    """What csrc/blend.hip mosaic_kernel takes of one image, in float32 numpy: csrc/u8_image.h's u8_sample (align_cases.sample_f32),
    whose `valid` is the presence, and the border weight u8_border_weight.  -> (value float32 [Ho,Wo,3], weight, present)"""
    f = np.float32
    Hs, Ws = image.shape[:2]
    val, u, v, _, present = align_cases.sample_f32(image, M, Ho, Wo)
    with np.errstate(all="ignore"):
        weight = np.minimum(np.minimum(np.minimum(u, f(Ws - 1) - u), np.minimum(v, f(Hs - 1) - v)) + f(1), f(feather))
    assert weight.dtype == f
    return val, weight, present


def mosaic_f32(images_a, images_b, Ma, Mb, Hc, Wc, feather, mode, gain=None):
    """csrc/blend.hip mosaic_kernel in float32 numpy -> (out uint8 [B,Hc,Wc,3], cover uint8 [B,Hc,Wc])."""
    f = np.float32
    B = len(Ma)
    out, cover = np.empty((B, Hc, Wc, 3), np.uint8), np.empty((B, Hc, Wc), np.uint8)
    for b in range(B):
        a, wa, pa = sample_f32(images_a[b], Ma[b], Hc, Wc, feather)
        t, wb, pb = sample_f32(images_b[b], Mb[b], Hc, Wc, feather)
        g, o = (f(1), f(0)) if gain is None else (f(gain[b][0]), f(gain[b][1]))
        with np.errstate(all="ignore"):
            a = f32_fma(np.full_like(a, g), a, o)
            A, T = pa[..., None], pb[..., None]
            if mode == "feather":
                num = np.where(A, wa[..., None] * a, f(0)) + np.where(T, wb[..., None] * t, f(0))
                den = (np.where(pa, wa, f(0)) + np.where(pb, wb, f(0)))[..., None]
                val = np.where(den > 0, num / np.where(den > 0, den, f(1)), f(0))
            elif mode == "b_over_a":
                val = np.where(T, t, np.where(A, a, f(0)))
            else:
                val = np.where(A, a, np.where(T, t, f(0)))
            assert val.dtype == f
            out[b] = (np.minimum(np.maximum(np.nan_to_num(val, nan=0.0), f(0)), f(255)) + f(0.5)).astype(np.uint8)
        cover[b] = pa.astype(np.uint8) | (pb.astype(np.uint8) << 1)
    return out, cover


# ------------------------------------------------------------------------------------------------
# the integer translation: every sample is a pixel, so the comparison is bitwise
# ------------------------------------------------------------------------------------------------
def translation_case(h=17, w=23):
    """A on a canvas shifted by (+5, -3), B by (-4, +6): strips of only A, only B, both and nothing; every sample is a pixel."""
    A, B = pixels(1, h, w, seed=3), pixels(1, h, w, seed=4)
    Ma = np.array([[[1.0, 0, 5], [0, 1, -3], [0, 0, 1]]])          # canvas (x, y) reads A(x + 5, y - 3)
    Mb = np.array([[[1.0, 0, -4], [0, 1, 6], [0, 0, 1]]])          # ... and B(x - 4, y + 6)
    pa, pb = np.zeros((h, w), bool), np.zeros((h, w), bool)
    a, b = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    pa[3:, :w - 5], pb[:h - 6, 4:] = True, True
    a[3:, :w - 5], b[:h - 6, 4:] = A[0, :h - 3, 5:], B[0, 6:, :w - 4]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    da = np.minimum(np.minimum(xs + 5, w - 1 - (xs + 5)), np.minimum(ys - 3, h - 1 - (ys - 3))) + 1
    db = np.minimum(np.minimum(xs - 4, w - 1 - (xs - 4)), np.minimum(ys + 6, h - 1 - (ys + 6))) + 1
    return A, B, Ma, Mb, pa, pb, a, b, da, db


def translation_want(mode, feather, gain, pa, pb, a, b, da, db):
    g, o = (1.0, 0.0) if gain is None else gain
    a = g * a + o
    if mode == "feather":
        wa, wb = np.where(pa, np.minimum(da, feather), 0.0)[..., None], np.where(pb, np.minimum(db, feather), 0.0)[..., None]
        val = (wa * a + wb * b) / np.maximum(wa + wb, 1e-300)
    elif mode == "b_over_a":
        val = np.where(pb[..., None], b, a)
    else:
        val = np.where(pa[..., None], a, b)
    val = np.where((pa | pb)[..., None], val, 0.0)
    return np.floor(np.clip(val, 0, 255) + 0.5).astype(np.uint8), (pa.astype(np.uint8) | (pb.astype(np.uint8) << 1))


# ------------------------------------------------------------------------------------------------
# single-pixel images in a pair: the byte-load instances of the pair kernels on both store paths
# ------------------------------------------------------------------------------------------------
EXACT_FEATHER, EXACT_GAIN = 2.0, (0.5, 4.0)


@functools.lru_cache(maxsize=None)
def single_pixel_pairs():
    """[(A, Ma, B, Mb, Hc, Wc)] with two samples each: a 1 x 1 image as A, as B and as both, next to a 6 x 9 image, on an 8 x 8 canvas (four
    pixels per thread) and a 5 x 7 one (one pixel per thread, odd width).  The single pixel lies on canvas pixel (2, 2) of sample 0 and
    (3, 2) of sample 1, the 6 x 9 image is shifted down by one row, so every sample is a pixel; with EXACT_FEATHER the weights are 1 or 2
    (2 for the 6 x 9 image where it meets the single pixel) and with EXACT_GAIN every value is a multiple of 1/2: sums and quotients are
    exact or thirds, never within rounding of a half, and float32 gives the float64 statement's bits at EVERY pixel."""
    one, big = np.array([[[[200, 100, 50]]], [[[10, 20, 31]]]], np.uint8), pixels(2, 6, 9, seed=7)
    M1 = np.array([[[0.5, 0, -1], [0, 0.5, -1], [0, 0, 1]], [[0.5, 0, -1.5], [0, 0.5, -1], [0, 0, 1]]])
    Mt = np.array([[[1.0, 0, 0], [0, 1, -1], [0, 0, 1]]] * 2)
    for x in (one, M1, Mt):
        x.setflags(write=False)
    return [(A, Ma, B, Mb, Hc, Wc) for Hc, Wc in ((8, 8), (5, 7)) for (A, Ma), (B, Mb) in (((one, M1), (big, Mt)), ((big, Mt), (one, M1)), ((one, M1), (one[::-1], M1)))]


# ------------------------------------------------------------------------------------------------
# the exposure case and the aligner's pair
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def darkened_pair(h=120, w=160, seed=5, g=0.8, o=10.0):
    """(A, B) uint8 [1,h,w,3]: a texture and B = round_half_up(g A + o) per channel."""
    A = textures(1, h, w, seed=seed)
    B = np.floor(g * A.astype(np.float64) + o + 0.5).astype(np.uint8)
    B.setflags(write=False)
    return A, B


class StubHead(torch.nn.Module):
    """tests/test_align_gpu.py's: a 'model' whose prediction is given."""

    def __init__(self, delta):
        super().__init__()
        self.delta, self.seen = delta, None

    def predict_homography(self, data):
        self.seen = data
        return self.delta, None


@functools.lru_cache(maxsize=None)
def aligner_pair(size_a=(120, 160), size_b=(96, 128), P=32, g=1.0, o=0.0):
    """test_direction_and_lift_end_to_end's construction: A a texture, H_true = lift(delta) with delta on the 1/16-pixel grid (so the
    float32 delta the stub returns is exact), B = round_half_up(g warp_u8_host(A, H_true) + o).  -> (A, B, delta [1,4,2], H_true [1,3,3])"""
    (Ha, Wa), (Hb, Wb) = size_a, size_b
    A = textures(1, Ha, Wa, seed=5)
    delta = np.round(np.random.RandomState(3).uniform(-0.12 * P, 0.12 * P, (1, 4, 2)) * 16) / 16
    H_true = align.lift(delta, P, whole_geom(Ha, Wa, P), whole_geom(Hb, Wb, P))
    B, _ = align.warp_u8_host(A, H_true, Hb, Wb)
    B = np.floor(g * B.astype(np.float64) + o + 0.5).astype(np.uint8)
    for x in (B, delta, H_true):
        x.setflags(write=False)
    return A, B, delta, H_true
