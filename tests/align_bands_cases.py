"""Shared by tests/test_align_bands_cpu.py and tests/test_align_bands_gpu.py: the two-band cases - the panorama cases of
tests/align_pano_cases.py with their low banks - their float64 references (computed once), the pixels on which a float32 winner can be
held to the float64 one, a float32 numpy restatement of the kernel's arithmetic and a float64 Gaussian the integer blur is held to."""
import functools

import numpy as np

import align_mosaic_cases as Mc
import align_pano_cases as Pc
from align_cases import f32_fma
from bihome_amd import align

SIGMA = 3.0
TIE = 1e-3                       # two float64 weights nearer than this may be ordered the other way in float32

# name -> the feathers the case runs at.  The burst's reference frame has M = I: its integer weights sit exactly on a cap of 8.0 and tie
# with every other capped frame's over 5.5e-2 of the canvas, so the burst runs at 7.5 and 64
FEATHERS = {name: ((7.5, 64.0) if name.startswith("burst") else (8.0, 64.0)) for name in Pc.CASES}
# every (case, feather, with the gain) at sigma 3, and one case at sigma 1
RUNS = [(name, f, g, SIGMA) for name in Pc.CASES for f in FEATHERS[name] for g in (False, True)]
RUNS += [("n5-40x56-on-48x160", f, g, 1.0) for f in (8.0, 64.0) for g in (False, True)]


@functools.lru_cache(maxsize=None)
def low_of(name, sigma=SIGMA):
    """blur_host of the case's frames in the order the blend reads them: uint8 [nb,n,Hs,Ws,3]."""
    bank, idx, _, _, _, _ = Pc.case(name)
    low = align.blur_host(bank[idx], sigma)
    low.setflags(write=False)
    return low


@functools.lru_cache(maxsize=None)
def reference(name, feather, gain, sigma=SIGMA):
    """bands_host of the case: (out uint8 [nb,Hc,Wc,3], count uint8 [nb,Hc,Wc], winner uint8 [nb,Hc,Wc])."""
    bank, idx, _, M, Hc, Wc = Pc.case(name)
    return align.bands_host(bank, low_of(name, sigma), idx, M, Hc, Wc, feather, Pc.gain_of(*idx.shape[::-1]) if gain else None)


def frame_weights(M, Hs, Ws, Hc, Wc):
    """(uncapped border weight float64 [B,Hc,Wc], present bool [B,Hc,Wc]) of a Hs x Ws frame through M [B,3,3], from a projection written here."""
    M = np.asarray(M, np.float64).reshape(-1, 3, 3)
    ys, xs = np.mgrid[0:Hc, 0:Wc].astype(np.float64)
    w, p = np.zeros((len(M), Hc, Wc)), np.zeros((len(M), Hc, Wc), bool)
    for b, m in enumerate(M):
        with np.errstate(all="ignore"):
            qz = m[2, 0] * xs + m[2, 1] * ys + m[2, 2]
            ok = np.abs(qz) > 1e-8
            iz = 1.0 / np.where(ok, qz, 1.0)
            u, v = (m[0, 0] * xs + m[0, 1] * ys + m[0, 2]) * iz, (m[1, 0] * xs + m[1, 1] * ys + m[1, 2]) * iz
        p[b] = ok & (u >= 0) & (u <= Ws - 1) & (v >= 0) & (v <= Hs - 1)
        w[b] = np.minimum(np.minimum(u, Ws - 1 - u), np.minimum(v, Hs - 1 - v)) + 1.0
    return w, p


def decided_of(w, p, feather):
    """w, p [n,B,Hc,Wc] (`frame_weights` per frame) -> bool [B,Hc,Wc]: the pixels whose winner does not hang on a near-tie, in float64 -
    exactly one present frame has a capped weight within TIE of the largest, or every such frame has an uncapped weight >= feather + TIE
    (an exact tie by the cap: the lowest k wins in either arithmetic).  A pixel with nothing present is decided."""
    capped = np.where(p, np.minimum(w, feather), -np.inf)
    close = p & (capped >= capped.max(0) - TIE)
    return (close.sum(0) <= 1) | np.where(close, w >= feather + TIE, True).all(0)


@functools.lru_cache(maxsize=None)
def decided(name, feather):
    """`decided_of` for a panorama case: bool [nb,Hc,Wc]."""
    bank, idx, _, M, Hc, Wc = Pc.case(name)
    per = [frame_weights(M[:, k], bank.shape[1], bank.shape[2], Hc, Wc) for k in range(idx.shape[1])]
    return decided_of(np.stack([w for w, _ in per]), np.stack([p for _, p in per]), feather)


@functools.lru_cache(maxsize=None)
def compared(name, feather):
    """bool [nb,Hc,Wc]: decided and outside align_pano_cases.near_border."""
    return decided(name, feather) & ~Pc.near_border(name)[1]


# ------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy
# ------------------------------------------------------------------------------------------------
def bands_f32(images, low, idx, M, Hc, Wc, feather, gain=None, use=None):
    """csrc/blend.hip blend_seq_kernel<BandRule> in float32 numpy (align_mosaic_cases.sample_f32 for the frame and, at the same taps, its low band;
    BandRule's add / value) -> (out uint8 [B,Hc,Wc,3], count uint8 [B,Hc,Wc], winner uint8 [B,Hc,Wc])."""
    f = np.float32
    B, n = idx.shape
    low = np.asarray(low).reshape((B, n) + images.shape[1:])
    out, count, winner = np.empty((B, Hc, Wc, 3), np.uint8), np.zeros((B, Hc, Wc), np.uint8), np.full((B, Hc, Wc), 255, np.uint8)
    for b in range(B):
        num, den, w_best = np.zeros((Hc, Wc, 3), f), np.zeros((Hc, Wc), f), np.zeros((Hc, Wc), f)
        v_best, l_best = np.zeros((Hc, Wc, 3), f), np.zeros((Hc, Wc, 3), f)
        for k in range(n):
            if use is not None and not use[b][k]:
                continue
            v, w, p = Mc.sample_f32(images[idx[b, k]], M[b, k], Hc, Wc, feather)
            l, _, _ = Mc.sample_f32(low[b, k], M[b, k], Hc, Wc, feather)
            g, o = (f(1), f(0)) if gain is None else (f(gain[b][k][0]), f(gain[b][k][1]))
            with np.errstate(all="ignore"):
                v, l = f32_fma(np.full_like(v, g), v, o), f32_fma(np.full_like(l, g), l, o)
                take = p & ((count[b] == 0) | (w > w_best))
                num = np.where(p[..., None], num + w[..., None] * l, num)
                den = np.where(p, den + w, den)
            v_best, l_best = np.where(take[..., None], v, v_best), np.where(take[..., None], l, l_best)
            w_best = np.where(take, w, w_best)
            winner[b] = np.where(take, np.uint8(k), winner[b])
            count[b] += p.astype(np.uint8)
        with np.errstate(all="ignore"):
            mixed = v_best + (num / np.where(den > 0, den, f(1))[..., None] - l_best)
        val = np.where((count[b] == 0)[..., None], f(0), np.where((count[b] == 1)[..., None], v_best, mixed))
        assert val.dtype == f and num.dtype == f and den.dtype == f
        out[b] = (np.minimum(np.maximum(np.nan_to_num(val, nan=0.0), f(0)), f(255)) + f(0.5)).astype(np.uint8)
    return out, count, winner


# ------------------------------------------------------------------------------------------------
# a float64 Gaussian with the same real taps, border replicated
# ------------------------------------------------------------------------------------------------
def gaussian64(images, sigma):
    """images uint8 [...,H,W,3] -> float64 of the same shape: the separable Gaussian with g_i = exp(-i^2 / (2 sigma^2)) normalised over
    -r .. r, r = ceil(3 sigma), on edge-padded rows and columns (written apart from align.blur_host: np.pad and slices)."""
    r = int(np.ceil(3 * sigma))
    g = np.exp(-np.arange(-r, r + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    g /= g.sum()
    v = np.asarray(images).astype(np.float64)
    for axis in (v.ndim - 2, v.ndim - 3):
        n = v.shape[axis]
        pad = [(0, 0)] * v.ndim
        pad[axis] = (r, r)
        padded = np.pad(v, pad, mode="edge")
        v = sum(g[d] * np.take(padded, np.arange(d, d + n), axis=axis) for d in range(2 * r + 1))
    return v
