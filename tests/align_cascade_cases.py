"""Shared by tests/test_align_cascade_cpu.py and tests/test_align_cascade_gpu.py: the inputs of the warped-preparation cases, their float64
references (computed once), a float32 numpy restatement of the kernel's per-sub-sample arithmetic, and the host run of a whole cascade."""
import functools

import numpy as np

from align_cases import corner_homography, f32_fma, near_border_points, pixels, sample_f32, textures, whole_geom
from bihome_amd import align

MEAN, STD = 0.443, 0.129
PREP_BOUND = 1e-4 / STD          # the project's fp32 bound on a prepared patch: 1e-4 of the output range 1 / std (tests/test_align_gpu.py)
NEAR = 1e-3                      # cover is compared on patch pixels none of whose sub-samples lies this close (px) to a border line

# (Ha, Wa, Hb, Wb, P, nx, ny): image A seen from the grid of a Hb x Wb image B
WARP_CASES = [(37, 53, 29, 41, 16, 1, 1), (37, 53, 29, 41, 16, 3, 2), (37, 53, 29, 41, 16, 8, 8), (48, 80, 40, 56, 32, 2, 2)]
WARP_IDS = ["37x53-from-29x41-1x1", "37x53-from-29x41-3x2", "37x53-from-29x41-8x8", "48x80-from-40x56-P32-2x2"]
IDX, IDX_CLAMPED = (2, 0, 7), (2, 0, 3)          # a permuted index list into a bank of four; 7 lies outside and is clamped to 3


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
    near = near_border_points(Hg, P * ny, P * nx, Hs, Ws, NEAR)
    return near.reshape(-1, P, ny, P, nx).any(axis=(2, 4))


# ------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy
# ------------------------------------------------------------------------------------------------
def prep_warp_f32(images, Hg, P, C, nx, ny, mean=MEAN, std=STD):
    """csrc/cascade.hip align_prep_warp_kernel in float32 numpy: csrc/u8_image.h's u8_sample per sub-sample (align_cases.sample_f32),
    float32 sums in the order of the walk (rows of the cell, columns inside a row), the epilogue (u8_store_patch).
    -> (patch float32 [B,C,P,P], cover float32 [B,P,P])"""
    f = np.float32
    images = np.asarray(images)
    B = images.shape[0]
    patch, cover = np.empty((B, C, P, P), f), np.empty((B, P, P), f)
    for b in range(B):
        val, _, _, guard, ok = sample_f32(images[b], Hg[b], P * ny, P * nx)
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
