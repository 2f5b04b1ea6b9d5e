"""Shared by tests/test_align_cascade_cpu.py and tests/test_align_cascade_gpu.py: the inputs of the warped-preparation cases, their float64
references (computed once), a float32 numpy restatement of the kernel's per-sub-sample arithmetic, and the host run of a whole cascade."""
import functools

import numpy as np

from bihome_amd import align, synth

MEAN, STD = 0.443, 0.129
PREP_BOUND = 1e-4 / STD          # the project's fp32 bound on a prepared patch: 1e-4 of the output range 1 / std (tests/test_align_gpu.py)
NEAR = 1e-3                      # cover is compared on patch pixels none of whose sub-samples lies this close (px) to a border line

# (Ha, Wa, Hb, Wb, P, nx, ny): image A seen from the grid of a Hb x Wb image B
WARP_CASES = [(37, 53, 29, 41, 16, 1, 1), (37, 53, 29, 41, 16, 3, 2), (37, 53, 29, 41, 16, 8, 8), (48, 80, 40, 56, 32, 2, 2)]
WARP_IDS = ["37x53-from-29x41-1x1", "37x53-from-29x41-3x2", "37x53-from-29x41-8x8", "48x80-from-40x56-P32-2x2"]
IDX, IDX_CLAMPED = (2, 0, 7), (2, 0, 3)          # a permuted index list into a bank of four; 7 lies outside and is clamped to 3


@functools.lru_cache(maxsize=None)
def pixels(n, h, w, seed=0):
    a = np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def textures(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    a = np.stack([np.floor(np.clip(synth.texture_image(rng, h, w), 0, 255) + 0.5).astype(np.uint8) for _ in range(n)])
    a.setflags(write=False)
    return a


def whole_geom(h, w, P, n=1):
    sx, sy = w / P, h / P
    return np.tile(np.array([[sx, sy, 0.5 * sx - 0.5, 0.5 * sy - 0.5]]), (n, 1))


def corner_homography(seed, Hs, Ws, Ho, Wo, frac=0.2):
    """tests/test_align_gpu.py's: the corners of the Ho x Wo output onto the corners of the Hs x Ws source moved by up to frac of each side."""
    rs = np.random.RandomState(seed)
    co = np.array([[0, 0], [Wo - 1, 0], [Wo - 1, Ho - 1], [0, Ho - 1]], np.float64)
    cs = np.array([[0, 0], [Ws - 1, 0], [Ws - 1, Hs - 1], [0, Hs - 1]], np.float64)
    return synth.four_point_homography(co, cs + rs.uniform(-frac, frac, (4, 2)) * np.array([Ws, Hs]))


@functools.lru_cache(maxsize=None)
def warp_case(Ha, Wa, Hb, Wb, P, nx, ny):
    """(bank uint8 [4,Ha,Wa,3], Hg [3,3,3]): three samples, H from corner_homography(seed, ..., frac=0.2) folded with B's grid map."""
    H = np.stack([corner_homography(21 + b, Ha, Wa, Hb, Wb, frac=0.2) for b in range(3)])
    Hg = H @ align.grid_map(whole_geom(Hb, Wb, P, 3), nx, ny)
    Hg.setflags(write=False)
    return pixels(4, Ha, Wa), Hg


@functools.lru_cache(maxsize=None)
def warp_reference(case, C):
    """prep_warp_host of the case's samples (the clamped index list applied): (patch [3,C,P,P], cover [3,P,P]) float64."""
    bank, Hg = warp_case(*case)
    P, nx, ny = case[4:]
    return align.prep_warp_host(bank[list(IDX_CLAMPED)], Hg, P, C, nx, ny, MEAN, STD)


def near_border(Hg, P, nx, ny, Hs, Ws):
    """bool [B,P,P]: a sub-sample of the patch pixel has its float64 point within NEAR px of one of the four border lines."""
    Hg = np.asarray(Hg, np.float64).reshape(-1, 3, 3)
    ys, xs = np.mgrid[0:P * ny, 0:P * nx].astype(np.float64)
    out = np.zeros((Hg.shape[0], P, P), bool)
    for b, h in enumerate(Hg):
        with np.errstate(all="ignore"):
            qz = h[2, 0] * xs + h[2, 1] * ys + h[2, 2]
            u, v = (h[0, 0] * xs + h[0, 1] * ys + h[0, 2]) / qz, (h[1, 0] * xs + h[1, 1] * ys + h[1, 2]) / qz
            near = np.minimum.reduce([np.abs(u), np.abs(u - (Ws - 1)), np.abs(v), np.abs(v - (Hs - 1))]) < NEAR
        out[b] = near.reshape(P, ny, P, nx).any(axis=(1, 3))
    return out


# ------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy
# ------------------------------------------------------------------------------------------------
def f32_fma(a, b, c):
    """float32 fma: the product of two floats is exact in double, one double addition, one rounding to float."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def prep_warp_f32(images, Hg, P, C, nx, ny, mean=MEAN, std=STD):
    """csrc/cascade.hip align_prep_warp_kernel in float32 numpy: warp_tap.h's tap_project / tap_place / tap_weights / tap_blend per
    sub-sample, float32 sums in the order of the walk (rows of the cell, columns inside a row), the kernel's epilogue.  (The kernel's
    reciprocal is within an ulp of the division used here.)  -> (patch float32 [B,C,P,P], cover float32 [B,P,P])"""
    f = np.float32
    images = np.asarray(images)
    B, Hs, Ws = images.shape[:3]
    Hh, Wh = P * ny, P * nx
    ys, xs = np.mgrid[0:Hh, 0:Wh].astype(f)
    patch, cover = np.empty((B, C, P, P), f), np.empty((B, P, P), f)
    for b in range(B):
        h = np.asarray(Hg[b], np.float64).reshape(9).astype(f)
        img = images[b].astype(f)
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
            ok = ~guard & (u >= 0) & (u <= f(Ws - 1)) & (v >= 0) & (v <= f(Hs - 1))
        px = lambda dy, dx: img[np.clip(y0 + dy, 0, Hs - 1), np.clip(x0 + dx, 0, Ws - 1)]          # (a tap outside weighs 0)
        w00, w01, w10, w11 = (wx0 * wy0)[..., None], (wx1 * wy0)[..., None], (wx0 * wy1)[..., None], (wx1 * wy1)[..., None]
        val = f32_fma(px(1, 1), w11, f32_fma(px(1, 0), w10, f32_fma(px(0, 1), w01, px(0, 0) * w00)))
        assert val.dtype == f
        val = np.where(guard[..., None], f(0), val).reshape(P, ny, P, nx, 3)
        acc = np.zeros((P, P, 3), f)
        for sy in range(ny):
            for sx in range(nx):
                acc = acc + val[:, sy, :, sx]
        assert acc.dtype == f
        inv = f(1) / (f(nx * ny) * f(255))
        if C == 1:
            g = f32_fma(f(0.114), acc[..., 2], f32_fma(f(0.587), acc[..., 1], f(0.299) * acc[..., 0]))
            patch[b, 0] = (g * inv - f(mean)) / f(std)
        else:
            patch[b] = ((acc * inv - f(mean)) / f(std)).transpose(2, 0, 1)
        cover[b] = ok.reshape(P, ny, P, nx).sum(axis=(1, 3)).astype(f) / f(nx * ny)
    return patch, cover


# ------------------------------------------------------------------------------------------------
# a whole cascade on the host, float64
# ------------------------------------------------------------------------------------------------
def project(H, pts):
    q = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ np.asarray(H).T
    return q[:, :2] / q[:, 2:]


def corner_error(H, H_true, h, w):
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    return float(np.abs(project(H, c) - project(H_true, c)).max())


CASCADE_SHAPE = dict(Ha=120, Wa=160, Hb=120, Wb=160, P=32, nx=5, ny=4)          # sx = 5, sy = 3.75: the ratios of 480 x 640 at P = 128


class CascadeSample:
    """One pair and the host's whole run on it.  A is a texture, H_true = lift(delta_true) with delta_true on the 1/16 grid and
    B = warp_u8_host(A, H_true).  deltas[0] = delta_true / 2 is the first prediction; deltas[k] is half the corner displacement of the
    residual A_b^-1 H_best^-1 H_true A_b rounded to the 1/16 grid - unless `garbage` names a stage, whose delta is then uniform
    +-0.3 P.  Every candidate is made by cascade_compose and scored by prep_warp_host + patch_ncc_host; a candidate is taken where its
    rho rises and it counts at least min_cover C P P elements."""

    def __init__(self, seed, stages, garbage=None, min_cover=0.25, C=1):
        s = CASCADE_SHAPE
        Ha, Wa, Hb, Wb, P, nx, ny = (s[k] for k in ("Ha", "Wa", "Hb", "Wb", "P", "nx", "ny"))
        rs = np.random.RandomState(seed)
        self.A = textures(1, Ha, Wa, seed=seed)
        self.ga, self.gb = whole_geom(Ha, Wa, P), whole_geom(Hb, Wb, P)
        self.delta_true = np.round(rs.uniform(-0.2 * P, 0.2 * P, (1, 4, 2)) * 16) / 16
        self.H_true = align.lift(self.delta_true, P, self.ga, self.gb)
        self.B, _ = align.warp_u8_host(self.A, self.H_true, Hb, Wb)
        self.patch_2, _ = align.prep_host(self.B, None, P, C, MEAN, STD)
        G, Ab = align.grid_map(self.gb, nx, ny), align._affine(self.gb)[0]
        c = align.patch_corners(P)

        def look(H):
            W, cov = align.prep_warp_host(self.A, H @ G, P, C, nx, ny, MEAN, STD)
            return W, align.patch_ncc_host(W, self.patch_2, cov)[0]
        self.deltas = [self.delta_true / 2]
        self.H = [align.lift(self.deltas[0], P, self.ga, self.gb)]
        best, (W_best, o) = self.H[0], look(self.H[0])
        self.seen, self.score, self.count, self.accepted, s_best = [], [o[6]], [o[0]], [1], o[6]
        for k in range(1, stages + 1):
            self.seen.append(W_best)                                             # what the model is shown at stage k
            if garbage == k:
                d = rs.uniform(-0.3 * P, 0.3 * P, (1, 4, 2)).astype(np.float32).astype(np.float64)
            else:
                R = np.linalg.inv(Ab) @ np.linalg.inv(best[0]) @ self.H_true[0] @ Ab
                d = np.round(0.5 * (project(R, c) - c)[None] * 16) / 16
            cand = align.cascade_compose(best, d, P, self.gb)
            W_c, o = look(cand)
            take = bool(o[6] > s_best and o[0] >= min_cover * C * P * P)
            if take:
                best, W_best, s_best = cand, W_c, o[6]
            self.deltas.append(d); self.H.append(cand); self.score.append(o[6]); self.count.append(o[0]); self.accepted.append(int(take))
        self.best = best
        self.shape = s


@functools.lru_cache(maxsize=None)
def cascade_sample(seed, stages, garbage=None, min_cover=0.25):
    return CascadeSample(seed, stages, garbage, min_cover)
