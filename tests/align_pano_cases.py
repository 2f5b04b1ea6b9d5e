"""Shared by tests/test_align_pano_cpu.py and tests/test_align_pano_gpu.py: the inputs of the panorama cases (the generators of
tests/align_cases.py), their float64 references (computed once), a float32 numpy restatement of the kernel's arithmetic and the
sequence the aligner test registers."""
import functools

import numpy as np

import align_mosaic_cases as Mc
from align_cases import corner_homography, f32_fma, pixels, textures, whole_geom
from bihome_amd import align

NEAR = Mc.NEAR                   # count is compared where the float64 point is at least this far (px) from a border line of every frame


def gain_of(n, nb):
    """[nb,n,2]: gain[b,k] = (1 - 0.05 (k % 3), 3 (k % 4))."""
    k = np.arange(n)
    return np.tile(np.stack([1 - 0.05 * (k % 3), 3.0 * (k % 4)], 1)[None], (nb, 1, 1))


# every combination the kernel cases run: (mode, feather, with the gain)
COMBOS = [("feather", f, g) for f in (1.0, 8.0, 64.0) for g in (False, True)] + [(m, 8.0, g) for m in ("first", "last") for g in (False, True)]

# name -> (n, Hs, Ws, canvas or "ref", samples, step)
CASES = {
    "n3-17x23-on-24x53": (3, 17, 23, (24, 53), 2, 0.45),
    "n5-40x56-on-48x160": (5, 40, 56, (48, 160), 2, 0.45),
    "n5-40x56-on-37x131": (5, 40, 56, (37, 131), 2, 0.45),
    "n8-120x160-on-160x640": (8, 120, 160, (160, 640), 1, 0.45),
    "burst-n6-40x56-on-ref": (6, 40, 56, "ref", 2, 0.04),
}


@functools.lru_cache(maxsize=None)
def chain_case(n, Hs, Ws, canvas, nb, step=0.45, frac=0.08):
    """(bank uint8 [n nb,Hs,Ws,3], idx [nb,n], G [nb,n,3,3], M [nb,n,3,3], Hc, Wc): a pan - frame k of sample b sits (k - r) step Ws to the
    right of the reference r = n // 2 and (k - r) 0.1 Hs below (b = 0) or above it, with its corners moved by up to `frac` of each side;
    T from pano_frame_host ("ref": the identity), M = G T."""
    bank = textures(n * nb, Hs, Ws, seed=7)
    idx = np.arange(n * nb).reshape(nb, n)
    r = n // 2
    G = np.empty((nb, n, 3, 3))
    for b in range(nb):
        for k in range(n):
            C = np.eye(3) if k == r else corner_homography(31 + 10 * b + k, Hs, Ws, Hs, Ws, frac)
            S = np.array([[1.0, 0, -(k - r) * step * Ws], [0, 1.0, (1 if b == 0 else -1) * (k - r) * 0.1 * Hs], [0, 0, 1.0]])
            g = C @ S
            G[b, k] = g / g[2, 2]
    if canvas == "ref":
        Hc, Wc, M = Hs, Ws, G.copy()
    else:
        (Hc, Wc), T = canvas, align.pano_frame_host(G, (Hs, Ws), canvas)[0]
        M = G @ T[:, None]
    for x in (idx, G, M):
        x.setflags(write=False)
    return bank, idx, G, M, Hc, Wc


def case(name):
    n, Hs, Ws, canvas, nb, step = CASES[name]
    return chain_case(n, Hs, Ws, canvas, nb, step)


@functools.lru_cache(maxsize=None)
def reference(name, mode, feather, gain):
    """pano_host of the case: (out uint8 [nb,Hc,Wc,3], count uint8 [nb,Hc,Wc])."""
    bank, idx, _, M, Hc, Wc = case(name)
    return align.pano_host(bank, idx, M, Hc, Wc, feather, mode, gain_of(*idx.shape[::-1]) if gain else None)


@functools.lru_cache(maxsize=None)
def near_border(name):
    """(bool [n,nb,Hc,Wc]: per frame, the canvas pixels whose float64 point lies within NEAR px of a border line of the frame; their union).
    A frame whose M is the identity has none: its border lies on pixel centres, exactly, in float32 as in float64."""
    bank, idx, _, M, Hc, Wc = case(name)
    Hs, Ws = bank.shape[1:3]
    per = np.stack([np.zeros((len(M), Hc, Wc), bool) if np.array_equal(M[:, k], np.stack([np.eye(3)] * len(M)))
                    else Mc.near_border(M[:, k], Hc, Wc, Hs, Ws) for k in range(M.shape[1])])
    return per, per.any(0)


# ------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy
# ------------------------------------------------------------------------------------------------
def pano_f32(images, idx, M, Hc, Wc, feather, mode, gain=None, use=None):
    """csrc/blend.hip pano_kernel in float32 numpy (align_mosaic_cases.sample_f32 per frame) -> (out uint8 [B,Hc,Wc,3], count uint8 [B,Hc,Wc])."""
    f = np.float32
    B, n = idx.shape
    out, count = np.empty((B, Hc, Wc, 3), np.uint8), np.zeros((B, Hc, Wc), np.uint8)
    for b in range(B):
        num, den = np.zeros((Hc, Wc, 3), f), np.zeros((Hc, Wc), f)
        for k in range(n):
            if use is not None and not use[b][k]:
                continue
            v, w, p = Mc.sample_f32(images[idx[b, k]], M[b, k], Hc, Wc, feather)
            g, o = (f(1), f(0)) if gain is None else (f(gain[b][k][0]), f(gain[b][k][1]))
            with np.errstate(all="ignore"):
                v = f32_fma(np.full_like(v, g), v, o)
                P = p[..., None]
                if mode == "feather":
                    num = np.where(P, num + w[..., None] * v, num)
                    den = np.where(p, den + w, den)
                elif mode == "first":
                    num = np.where(P & (count[b] == 0)[..., None], v, num)
                else:
                    num = np.where(P, v, num)
            count[b] += p.astype(np.uint8)
        with np.errstate(all="ignore"):
            val = np.where((den > 0)[..., None], num / np.where(den > 0, den, f(1))[..., None], f(0)) if mode == "feather" else num
        assert val.dtype == f
        out[b] = (np.minimum(np.maximum(np.nan_to_num(val, nan=0.0), f(0)), f(255)) + f(0.5)).astype(np.uint8)
    return out, count


# ------------------------------------------------------------------------------------------------
# integer translations: every sample is a pixel, so the comparison is bitwise
# ------------------------------------------------------------------------------------------------
def translation_case(h=17, w=23):
    """Three frames of random bytes shifted by whole pixels so that every count 0..3 occurs: (bank [3,h,w,3], idx [1,3], M [1,3,3,3])."""
    bank = pixels(3, h, w, seed=9)
    shifts = ((5, -3), (-4, 6), (-2, -2))                                  # canvas (x, y) reads frame k at (x + dx, y + dy)
    M = np.array([[[[1.0, 0, dx], [0, 1.0, dy], [0, 0, 1.0]] for dx, dy in shifts]])
    return bank, np.arange(3).reshape(1, 3), M


# ------------------------------------------------------------------------------------------------
# the aligner's sequence
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def aligner_sequence(n=4, ref=1, size=(96, 128), P=32):
    """align_mosaic_cases.aligner_pair's construction along a chain: per-pair deltas on the 1/16-pixel grid (the float32 delta the stub
    returns is exact), H_pairs = lift(delta), G_true = chain_host(H_pairs, ref), frame k = warp_u8_host(texture, G_true[k]^-1) - so that
    frame_a(H_pair x) ~ frame_b(x).  -> (frames uint8 [n,Hs,Ws,3], deltas [n-1,4,2], H_pairs [1,n-1,3,3], G_true [1,n,3,3])"""
    Hs, Ws = size
    base = textures(1, 3 * Hs, 3 * Ws, seed=5)
    deltas = np.round(np.random.RandomState(4).uniform(-0.1 * P, 0.1 * P, (n - 1, 4, 2)) * 16) / 16
    geom = whole_geom(Hs, Ws, P, n - 1)
    H_pairs = align.lift(deltas, P, geom, geom)[None]
    G_true = align.chain_host(H_pairs, ref)
    centre = np.array([[1.0, 0, Ws], [0, 1.0, Hs], [0, 0, 1.0]])          # the reference is the middle third of the texture
    frames = np.concatenate([align.warp_u8_host(base, (centre @ np.linalg.inv(G_true[0, k]))[None], Hs, Ws)[0] for k in range(n)])
    for x in (frames, deltas, H_pairs, G_true):
        x.setflags(write=False)
    return frames, deltas, H_pairs, G_true
