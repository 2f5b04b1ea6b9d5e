"""Robust homography of a perspective field (bh_ransac_homography / NoOpHead ALL_POINTS_FIT='ransac'): the boundary, the head's
kwargs, and the yardstick the GPU tests (tests/test_ransac_gpu.py) compare against - a float64 numpy restatement of the algorithm
(minimal-sample hypotheses, inlier counts, selection, inlier mask and Hartley-normalised refit), written from the specification in
include/bihome.h and checked here on its own: on a field with 0.3 px noise, a 30 % block of wrong offsets and 5 % scattered outliers
it recovers the true 4-point offsets to a fraction of a pixel where the least-squares fit of the lattice points is off by tens."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from bihome_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_EPSILON = 1.1920928955078125e-07
THR = 10.0
B_TEST, K_TEST, PAIR_SEED, NOISE_SEED, CHOICE_SEED = 6, 128, 5, 1, 7


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def make_inputs(B=B_TEST, K=K_TEST, pair_seed=PAIR_SEED, noise_seed=NOISE_SEED, choice_seed=CHOICE_SEED):
    """-> pf [B,2,h,w] float32, choice [B,K,4] int64, delta [B,4,2] (truth), clean [B,2,h,w] float32 (the exact field)."""
    d = synth.make_pairs(B, seed=pair_seed, target=True)
    clean = np.asarray(d["target"], np.float32)
    _, _, h, w = clean.shape
    pf = _corrupt(clean, np.random.default_rng(noise_seed))
    choice = torch.randint(0, h * w, (B, K, 4), generator=torch.Generator().manual_seed(choice_seed)).numpy()
    return pf.astype(np.float32), choice.astype(np.int64), np.asarray(d["delta"], np.float64), clean


def _corrupt(clean, rng, reach=False):
    """clean [B,2,h,w] float32 -> float64: 0.3 px noise, a contiguous 30 % block at one far-away offset, 5 % scattered outliers.
    reach: the block's offset lies 90 px beyond the farthest true offset inside the block, not 90 px from the one at its centre
    (for a field that varies by tens of pixels across the block)."""
    B, _, h, w = clean.shape
    pf = clean.astype(np.float64) + rng.normal(0.0, 0.3, clean.shape)
    bh = max(h // 2, 1)
    bw = int(np.ceil(0.3 * h * w / bh))                             # a contiguous block of 30 % of the patch
    assert bh * bw >= 0.3 * h * w and bw <= w
    for b in range(B):
        y0, x0 = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
        ang = rng.uniform(0, 2 * np.pi)
        centre = clean[b, :, y0 + bh // 2, x0 + bw // 2].astype(np.float64)
        far = np.sqrt(((clean[b, :, y0:y0 + bh, x0:x0 + bw] - centre[:, None, None]) ** 2).sum(0)).max() if reach else 0.0
        const = centre + (90.0 + far) * np.array([np.cos(ang), np.sin(ang)])
        away = np.sqrt(((clean[b, :, y0:y0 + bh, x0:x0 + bw] - const[:, None, None]) ** 2).sum(0)).min()
        assert away >= 40.0, away                                   # every pixel of the block is >= 40 px from its true offset
        pf[b, :, y0:y0 + bh, x0:x0 + bw] = const[:, None, None]
        idx = rng.choice(h * w, size=int(round(0.05 * h * w)), replace=False)      # a further 5 %: scattered, uniform in +-64 px
        pf[b].reshape(2, -1)[:, idx] = rng.uniform(-64.0, 64.0, (2, idx.size))
    return pf


def _four_point(src, dst):
    """The homography through four correspondences, H22 = 1 (float64)."""
    S = np.zeros((8, 8))
    for i in range(4):
        (x, y), (u, v) = src[i], dst[i]
        S[2 * i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        S[2 * i + 1] = [0, 0, 0, x, y, 1, -x * v, -y * v]
    return np.append(np.linalg.solve(S, np.asarray(dst, np.float64).reshape(8)), 1.0).reshape(3, 3)


def make_field_inputs(B, K, h, w, seed, choice_seed):
    """make_inputs at any field size: per sample a random 4-point homography (corner offsets uniform in +-0.25 min(h, w)) evaluated in
    float64, then make_inputs' noise, block and scattered outliers; the draws from a seeded torch.randint.
    -> pf [B,2,h,w] float32, choice [B,K,4] int64, delta [B,4,2] (truth), clean [B,2,h,w] float32 (the exact field)."""
    rng = np.random.default_rng(seed)
    c = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    delta = rng.uniform(-0.25 * min(h, w), 0.25 * min(h, w), (B, 4, 2))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    clean = np.empty((B, 2, h, w))
    for b in range(B):
        q = np.stack([xs, ys, np.ones_like(xs)], -1) @ _four_point(c, c + delta[b]).T
        assert (q[..., 2] > 0.1).all()
        clean[b] = np.stack([q[..., 0] / q[..., 2] - xs, q[..., 1] / q[..., 2] - ys])
    clean = clean.astype(np.float32)
    pf = _corrupt(clean, rng, reach=True)
    choice = torch.randint(0, h * w, (B, K, 4), generator=torch.Generator().manual_seed(choice_seed)).numpy()
    return pf.astype(np.float32), choice.astype(np.int64), delta, clean


# (B, K, h, w, thr): the smallest shapes at which bh_ransac_homography's kernels take their other paths
FIELD_CASES = [
    (2, 1100, 37, 83, 10.0),     # N = 3071: two count tiles, the second partial; K = 1024 + 76; B*K = 2200 = 34 * 64 + 24; odd w
    (1, 2100, 16, 16, 5.0),      # three passes of the 1024-entry table (1024, 1024, 52); N = 256: one strip of one tile
    (3, 70, 5, 7, 3.0),          # N = 35: less than one wave; K = 64 + 6; many invalid draws
    (2, 200, 9, 300, 10.0),      # wide and short, w no power of two; N = 2700: one full tile and a partial one
    (2, 130, 3, 700, 10.0),      # w > 512, h = 3; N = 2100
]
FIELD_SEEDS = [(101, 201), (102, 202), (103, 203), (104, 204), (125, 225)]      # (field, draws) per case
TIE_CASES = (0, 2)
WILD_H, WILD_W, WILD_THR = 24, 20, 0.05


# ------------------------------------------------------------------------------------------------
# the restatement (float64)
# ------------------------------------------------------------------------------------------------
def _collinear3(pi, pj, pk):
    dx1, dy1, dx2, dy2 = pi[0] - pk[0], pi[1] - pk[1], pj[0] - pk[0], pj[1] - pk[1]
    return abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2))


def _any_collinear(p):
    return any(_collinear3(p[i], p[j], p[k]) for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)))


def _solve8(S):
    """Gaussian elimination with partial pivoting on the 8x9 augmented system; -> (x, smallest |pivot|)."""
    S = S.copy()
    minp = np.inf
    with np.errstate(all="ignore"):
        for k in range(8):
            r = k + int(np.argmax(np.abs(S[k:, k])))
            minp = min(minp, abs(S[r, k])) if np.isfinite(S[r, k]) else np.nan
            if r != k:
                S[[k, r]] = S[[r, k]]
            for i in range(k + 1, 8):
                S[i, k + 1:] -= (S[i, k] / S[k, k]) * S[k, k + 1:]
        x = np.zeros(8)
        for k in range(7, -1, -1):
            x[k] = (S[k, 8] - S[k, k + 1:8] @ x[k + 1:]) / S[k, k]
    return x, minp


def hypotheses(pf, choice):
    """-> hyp [B,K,9] float64 (NaN rows for invalid hypotheses, H22 = 1), valid [B,K] bool."""
    B, _, h, w = pf.shape
    K = choice.shape[1]
    hyp = np.full((B, K, 9), np.nan)
    valid = np.zeros((B, K), bool)
    for b in range(B):
        fx, fy = pf[b, 0].reshape(-1).astype(np.float64), pf[b, 1].reshape(-1).astype(np.float64)
        for k in range(K):
            ids = choice[b, k]
            if (ids < 0).any() or (ids >= h * w).any() or len(set(ids.tolist())) < 4:
                continue
            src = np.stack([(ids % w).astype(np.float64), (ids // w).astype(np.float64)], 1)
            dst = src + np.stack([fx[ids], fy[ids]], 1)
            if _any_collinear(src) or _any_collinear(dst):
                continue
            S = np.zeros((8, 9))
            for i in range(4):
                (x, y), (u, v) = src[i], dst[i]
                S[2 * i] = [x, y, 1, 0, 0, 0, -x * u, -y * u, u]
                S[2 * i + 1] = [0, 0, 0, x, y, 1, -x * v, -y * v, v]
            sol, minp = _solve8(S)
            if not (minp > 1e-12) or not np.isfinite(sol).all():
                continue
            hyp[b, k, :8], hyp[b, k, 8] = sol, 1.0
            valid[b, k] = True
    return hyp, valid


def _coords(pf):
    B, _, h, w = pf.shape
    x = np.tile(np.arange(w, dtype=np.float64), h)
    y = np.repeat(np.arange(h, dtype=np.float64), w)
    return x, y, x[None] + pf[:, 0].reshape(B, -1).astype(np.float64), y[None] + pf[:, 1].reshape(B, -1).astype(np.float64)


def squared_error(pf, H):
    """H [B,K,9] (as stored: rounded to float32) -> e [B,K,N] squared reprojection distance, ok [B,K,N] (qz > 0 and finite)."""
    x, y, u, v = _coords(pf)
    H = H.astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        qx = H[..., 0, None] * x + H[..., 1, None] * y + H[..., 2, None]
        qy = H[..., 3, None] * x + H[..., 4, None] * y + H[..., 5, None]
        qz = H[..., 6, None] * x + H[..., 7, None] * y + H[..., 8, None]
        e = (qx / qz - u[:, None]) ** 2 + (qy / qz - v[:, None]) ** 2
    return e, (qz > 0) & np.isfinite(qz)


def fp32_margins(pf, hyp):
    """What fp32 can do to the inlier test, for inputs the relative 1e-4 of counts()' border does not cover (a threshold far below the
    offsets, a horizon inside the field).  The kernel evaluates q = H (x, y, 1) with two fused multiply-adds per coordinate (error
    <= 2 eps S, S the sum of the absolute terms), a = qx - u qz and b = qy - v qz with one each, and tests a^2 + b^2 <= (thr qz)^2.
    -> d [B,K,N]: the float64 reprojection distance in px; slack [B,K,N]: a bound in px on what the fp32 evaluation moves d, or the
    threshold, by; horizon [B,K,N]: |qz| over the bound 2 eps Sz on its own fp32 error (the sign of qz is safe where this is large); front [B,K,N]: qz > 0
    (a pixel behind is an outlier whatever its d)."""
    x, y, u, v = _coords(pf)
    H = hyp.astype(np.float32).astype(np.float64)[..., None]
    eps = FLT_EPSILON
    with np.errstate(all="ignore"):
        qz = H[..., 6, :] * x + H[..., 7, :] * y + H[..., 8, :]
        sx = np.abs(H[..., 0, :] * x) + np.abs(H[..., 1, :] * y) + np.abs(H[..., 2, :])
        sy = np.abs(H[..., 3, :] * x) + np.abs(H[..., 4, :] * y) + np.abs(H[..., 5, :])
        sz = np.abs(H[..., 6, :] * x) + np.abs(H[..., 7, :] * y) + np.abs(H[..., 8, :])
        au, av = np.abs(u)[:, None], np.abs(v)[:, None]
        d = np.sqrt(squared_error(pf, hyp)[0])
        slack = (2 * eps * (sx + sy + (au + av) * sz) + 2 * eps * sz * d) / np.abs(qz) + eps * (au + av) + 4 * eps * d
        return d, slack, np.abs(qz) / (2 * eps * sz), qz > 0


def counts(pf, hyp, valid, thr=THR):
    """-> count [B,K] (-1 invalid), border [B,K]: pixels whose squared error lies within a relative 1e-4 of thr^2."""
    e, ok = squared_error(pf, hyp)
    with np.errstate(invalid="ignore"):
        inl = ok & (e <= thr * thr)
        brd = np.abs(e - thr * thr) <= 1e-4 * thr * thr
    count = np.where(valid, inl.sum(-1), -1)
    return count.astype(np.int64), np.where(valid, brd.sum(-1), 0).astype(np.int64)


def select(count):
    """-> best [B] (first maximum), n_inl [B] (0: flagged, fewer than 4 inliers or nothing valid)."""
    best = np.argmax(count, 1)
    top = count[np.arange(count.shape[0]), best]
    return best, np.where(top >= 4, top, 0)


def inlier_mask(pf, hyp, best, n_inl, thr=THR):
    """-> mask [B,h,w] uint8 of the winner (all ones for a flagged sample), border [B,h,w] bool."""
    B, _, h, w = pf.shape
    e, ok = squared_error(pf, hyp[np.arange(B), best][:, None])
    with np.errstate(invalid="ignore"):
        m = (ok & (e <= thr * thr))[:, 0]
        brd = (np.abs(e - thr * thr) <= 1e-4 * thr * thr)[:, 0]
    m[n_inl == 0] = True
    return m.reshape(B, h, w).astype(np.uint8), brd.reshape(B, h, w)


def _hartley(p):
    m = p.mean(0)
    s = np.sqrt(2.0) / (np.sqrt(((p - m) ** 2).sum(1)).mean() + 1e-8)
    return np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1.0]])


def dlt(src, dst, h, w, svd=False):
    """Hartley-normalised DLT (smallest eigenvector of A^T A; svd: the last right singular vector of A instead, a second float64
    formulation to measure this one's own sensitivity with), /(H22 + 1e-8); -> (H [3,3], delta_hat [4,2])."""
    T1, T2 = _hartley(src), _hartley(dst)
    a = np.concatenate([src, np.ones((len(src), 1))], 1) @ T1.T
    q = np.concatenate([dst, np.ones((len(dst), 1))], 1) @ T2.T
    z = np.zeros_like(a)
    A = np.concatenate([np.concatenate([a, z, -q[:, :1] * a], 1), np.concatenate([z, a, -q[:, 1:2] * a], 1)], 0)
    vec = np.linalg.svd(A)[2][-1] if svd else np.linalg.eigh(A.T @ A)[1][:, 0]
    H = np.linalg.inv(T2) @ vec.reshape(3, 3) @ T1
    H = H / (H[2, 2] + 1e-8)
    c = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    p = np.concatenate([c, np.ones((4, 1))], 1) @ H.T
    return H, p[:, :2] / p[:, 2:] - c


def refit(pf, mask, svd=False):
    """Least squares over the pixels of mask -> H [B,3,3], delta_hat [B,4,2]."""
    B, _, h, w = pf.shape
    x, y, u, v = _coords(pf)
    Hs, ds = [], []
    for b in range(B):
        m = mask[b].reshape(-1).astype(bool)
        H, dh = dlt(np.stack([x[m], y[m]], 1), np.stack([u[b][m], v[b][m]], 1), h, w, svd)
        Hs.append(H); ds.append(dh)
    return np.stack(Hs), np.stack(ds)


def ransac_reference(pf, choice, thr=THR):
    hyp, valid = hypotheses(pf, choice)
    count, border = counts(pf, hyp, valid, thr)
    best, n_inl = select(count)
    mask, mask_border = inlier_mask(pf, hyp, best, n_inl, thr)
    H, dh = refit(pf, mask)
    return dict(hyp=hyp, valid=valid, count=count, border=border, best=best, n_inl=n_inl, mask=mask, mask_border=mask_border, H=H,
                delta_hat=dh)


def lattice_least_squares(pf):
    """float64 least squares over the 32 x 16 lattice NoOpHead._postprocess sends through bh_dlt_fwd."""
    B, _, h, w = pf.shape
    ny, nx = min(h, 32), min(w, 16)
    ys = ((np.arange(ny) + 0.5) * h / ny).astype(np.int64)
    xs = ((np.arange(nx) + 0.5) * w / nx).astype(np.int64)
    m = np.zeros((B, h, w), np.uint8)
    m[:, ys[:, None], xs[None, :]] = 1
    return refit(pf, m)[1]


def mace(delta_hat, delta):
    return np.sqrt(((delta_hat - delta) ** 2).sum(-1)).mean(-1)


def candidates(count, border, best):
    """C(b) = {k : count[k] + border[k] >= count[best] - border[best]}, and whether every member has border 0 (counts exact)."""
    out = []
    for b in range(count.shape[0]):
        c = np.nonzero(count[b] + border[b] >= count[b, best[b]] - border[b, best[b]])[0]
        out.append((set(c.tolist()), bool((border[b, c] == 0).all())))
    return out


@functools.lru_cache(maxsize=None)
def field_case(i):
    """FIELD_CASES[i]: its inputs and the restatement's results on them.  Computed once per process; nobody writes into it."""
    B, K, h, w, thr = FIELD_CASES[i]
    pf, choice, delta, clean = make_field_inputs(B, K, h, w, *FIELD_SEEDS[i])
    r = ransac_reference(pf, choice, thr)
    r.update(pf=pf, choice=choice, delta=delta, clean=clean, thr=thr)
    return r


@functools.lru_cache(maxsize=None)
def tie_case(i):
    """The exact field of FIELD_CASES[i], where every valid hypothesis counts h*w: the first three draws of every sample are made
    invalid (a repeated index), and a copy of the first valid draw is appended as hypothesis K - so the winner is pinned by the
    lowest-k rule alone, at a k >= 3, against an identical hypothesis in another lane of the selection kernel."""
    B, K, h, w, thr = FIELD_CASES[i]
    _, choice, delta, clean = make_field_inputs(B, K, h, w, *FIELD_SEEDS[i])
    choice = choice.copy()
    choice[:, :3] = [1, 1, 2, h * w - 1]
    _, valid = hypotheses(clean, choice)
    first = np.argmax(valid, 1)
    choice = np.concatenate([choice, choice[np.arange(B), first][:, None]], 1)
    r = ransac_reference(clean, choice, thr)
    r.update(pf=clean, choice=choice, delta=delta, thr=thr, first=first)
    return r


WILD_B, WILD_K, WILD_SEED, WILD_CHOICE_SEED = 4, 6, 32, 33


@functools.lru_cache(maxsize=None)
def wild_case():
    """A field without structure (uniform +-64 px) under a 0.05 px threshold: a valid hypothesis explains its own four points, if
    it keeps them in front (qz > 0), and nothing else - counts of 0 to 4, the boundary of the fallback rule n_inl = count >= 4 ?"""
    pf = np.random.default_rng(WILD_SEED).uniform(-64.0, 64.0, (WILD_B, 2, WILD_H, WILD_W)).astype(np.float32)
    choice = torch.randint(0, WILD_H * WILD_W, (WILD_B, WILD_K, 4), generator=torch.Generator().manual_seed(WILD_CHOICE_SEED)).numpy()
    choice = choice.astype(np.int64)
    r = ransac_reference(pf, choice, WILD_THR)
    r.update(pf=pf, choice=choice, thr=WILD_THR)
    return r


@pytest.fixture(scope="module")
def reference():
    pf, choice, delta, clean = make_inputs()
    r = ransac_reference(pf, choice)
    r.update(pf=pf, choice=choice, delta=delta, clean=clean)
    return r


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
def test_header_and_ctypes_signature_agree():
    from bihome_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bihome.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bh_ransac_homography\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/bihome.h does not declare bh_ransac_homography"
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else {"int": ctypes.c_int, "float": ctypes.c_float}[arg.split()[0]])
    assert _lib.SIGNATURES["bh_ransac_homography"] == want
    assert len(want) == 16 and want[6] is ctypes.c_float           # thr
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bh_ransac_homography")


def test_bad_arguments_are_refused_before_any_launch():
    from bihome_amd import _lib
    f = _lib.lib.bh_ransac_homography
    p = ctypes.c_void_p(64)         # never dereferenced: the argument check comes first
    assert f(p, p, 1, 0, 128, 128, 10.0, p, p, p, p, None, p, p, p, None) == -1          # K < 1
    assert f(p, p, 1, 8, 1, 3, 10.0, p, p, p, p, None, p, p, p, None) == -1              # h*w < 4
    assert f(p, p, 1, 8, 128, 128, 10.0, p, None, p, p, None, p, p, p, None) == -1       # NULL count
    assert f(None, p, 1, 8, 128, 128, 10.0, p, p, p, p, None, p, p, p, None) == -1       # NULL field
    assert f(p, p, 1, 8, 128, 128, float("nan"), p, p, p, p, None, p, p, p, None) == -1
    assert f(p, p, 70000, 8, 128, 128, 10.0, p, p, p, p, None, p, p, p, None) == -2      # more samples than one launch takes
    assert f(p, p, 0, 8, 128, 128, 10.0, p, p, p, p, None, p, p, p, None) == 0           # empty batch: nothing to do


def test_noophead_kwargs():
    from bihome_amd.heads import NoOpHead
    keys = ["target", "pf_hat_12", "delta", "pf_hat_12"]
    m = NoOpHead.Model(None, TARGET_GEN="all_points", LEARNING_KEYS=keys)
    assert m.all_points_fit == "lattice"
    with pytest.raises(ValueError):
        NoOpHead.Model(None, TARGET_GEN="all_points", LEARNING_KEYS=keys, ALL_POINTS_FIT="bogus")
    m = NoOpHead.Model(None, TARGET_GEN="all_points", LEARNING_KEYS=keys, ALL_POINTS_FIT="ransac")
    assert (m.all_points_fit, m.ransac_iters, m.ransac_threshold) == ("ransac", 256, 10.0)
    m = NoOpHead.Model(None, TARGET_GEN="all_points", LEARNING_KEYS=keys, ALL_POINTS_FIT="ransac", RANSAC_ITERS=64, RANSAC_THRESHOLD=3)
    assert (m.ransac_iters, m.ransac_threshold) == (64, 3.0)
    with pytest.raises(ValueError):
        NoOpHead.Model(None, TARGET_GEN="all_points", LEARNING_KEYS=keys, ALL_POINTS_FIT="ransac", RANSAC_ITERS=0)
    import math
    assert math.log(1 - 0.995) / math.log(1 - 0.38 ** 4) <= 256        # the docstring's derivation of the default


def test_wrapper_refuses_cpu_tensors():
    from bihome_amd import kernels as K
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.ransac_homography(torch.zeros(1, 2, 8, 8), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_restatement_is_robust_where_least_squares_is_not(reference):
    r = reference
    robust, plain = mace(r["delta_hat"], r["delta"]), mace(lattice_least_squares(r["pf"]), r["delta"])
    share = r["n_inl"] / float(r["pf"].shape[2] * r["pf"].shape[3])
    print("RANSAC + refit MACE", robust, "lattice least squares MACE", plain, "inlier share", share)
    assert (robust < 0.5).all(), robust
    assert (plain > 10 * robust).all(), (plain, robust)
    assert (share > 0.6).all() and (share < 0.7).all(), share          # 30 % block + 5 % scatter (a few of them inside the block)
    assert r["valid"].mean() > 0.9 and (r["count"][~r["valid"]] == -1).all()
    assert (r["mask"].reshape(len(share), -1).sum(1) == r["n_inl"]).all()


def test_conditions_the_gpu_comparison_rests_on(reference):
    """Properties of the inputs and of the restatement alone: few pixels sit within a relative 1e-4 of the threshold (only there may
    fp32 and float64 decide differently), and for at least 5 of the 6 samples no candidate winner has such a pixel at all, so the
    GPU's winner must equal the restatement's exactly - lowest-k tie rule included."""
    r = reference
    B, K = r["count"].shape
    n = r["pf"].shape[2] * r["pf"].shape[3]
    print("border pixels", int(r["border"].sum()), "of", B * K * n)
    assert r["border"].sum() <= 1e-3 * B * K * n
    cand = candidates(r["count"], r["border"], r["best"])
    for b in range(B):
        top = np.sort(r["count"][b])[::-1][:3]
        print("sample", b, "best", int(r["best"][b]), "top counts", top, "candidates", len(cand[b][0]), "exact", cand[b][1])
    assert sum(exact for _, exact in cand) >= 5


def test_restatement_invalid_and_fallback_cases():
    pf, choice, _, clean = make_inputs(B=2, K=8)
    h, w = pf.shape[2:]
    choice = choice.copy()
    choice[0, 0] = [5, 5, 9, 200]                      # a repeated index
    choice[0, 1] = [0, 1, 2, 700]                      # three collinear source points
    choice[0, 2] = [0, h * w, 3, 900]                  # outside the field
    hyp, valid = hypotheses(pf, choice)
    assert not valid[0, :3].any() and np.isnan(hyp[0, :3]).all() and valid[0, 3:].any()
    # exact field: every valid hypothesis explains every pixel
    hyp, valid = hypotheses(clean, choice)
    count, _ = counts(clean, hyp, valid)
    assert (count[valid] == h * w).all() and (count[~valid] == -1).all()
    # nothing valid: flagged, the refit takes every point
    deg = np.tile(np.array([3, 3, 7, 9], np.int64), (2, 4, 1))
    r = ransac_reference(pf, deg)
    assert (r["n_inl"] == 0).all() and (r["mask"] == 1).all() and np.isfinite(r["H"]).all()


# ------------------------------------------------------------------------------------------------
# the other shapes (FIELD_CASES), the tie and the fallback boundary: conditions of tests/test_ransac_gpu.py, on the restatement alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(FIELD_CASES)))
def test_conditions_at_the_other_shapes(i):
    """Per case: few border pixels (the cap of the 128 x 128 test), EVERY sample's candidate set exact - so the GPU's winner is pinned
    for every sample -, both valid and invalid hypotheses, and on the exact field every valid hypothesis counts h*w with no border
    pixel.  Also printed: what the refit's float64 formulation itself is good for (eigh of A^T A against the SVD of A on the same
    masks) - at most 2.3e-10 px in delta_hat and a relative 2e-8 in H (the sign of H22 + 1e-8) when the test was written, far inside
    the bands the GPU comparison uses (2e-5 px scaled by max(h, w) / 128; rtol 1e-5), which therefore stand as they are."""
    B, K, h, w, thr = FIELD_CASES[i]
    r = field_case(i)
    n = h * w
    assert r["pf"].shape == (B, 2, h, w) and r["pf"].dtype == np.float32 and r["choice"].shape == (B, K, 4)
    cand = candidates(r["count"], r["border"], r["best"])
    share = r["valid"].mean()
    print("case %d %s: border pixels %d (cap %.0f), valid %.0f %%, best %s n_inl %s, candidates %s exact %s" %
          (i, FIELD_CASES[i], r["border"].sum(), 1e-3 * B * K * n, 100 * share, r["best"], r["n_inl"], [len(c) for c, _ in cand],
           [e for _, e in cand]))
    assert r["border"].sum() <= 1e-3 * B * K * n
    assert all(exact for _, exact in cand)
    assert r["valid"].any() and (~r["valid"]).any() and (r["count"][~r["valid"]] == -1).all()
    assert (r["n_inl"] >= 4).all() and (r["mask"].reshape(B, -1).sum(1) == r["n_inl"]).all()
    hyp, valid = hypotheses(r["clean"], r["choice"])
    count, border = counts(r["clean"], hyp, valid, thr)
    assert (count[valid] == n).all() and (count[~valid] == -1).all() and border.sum() == 0
    Hs, ds = refit(r["pf"], r["mask"], svd=True)
    print("case %d: refit, eigh of A^T A against SVD of A: max |delta_hat| difference %.3e px, max relative |H| difference %.3e; "
          "max |delta_hat| %.1f px, MACE %s" % (i, np.abs(ds - r["delta_hat"]).max(), (np.abs(Hs - r["H"]) / np.abs(r["H"])).max(),
                                                np.abs(r["delta_hat"]).max(), mace(r["delta_hat"], r["delta"])))
    assert np.abs(ds - r["delta_hat"]).max() <= 2e-6 * max(1.0, max(h, w) / 128.0)        # a tenth of the band: it needs no widening


def test_some_first_valid_hypothesis_is_not_the_first():
    first = [np.argmax(field_case(i)["valid"], 1) for i in range(len(FIELD_CASES))]
    print("first valid hypothesis per case and sample:", first)
    assert any((f > 0).any() for f in first)


@pytest.mark.parametrize("i", TIE_CASES)
def test_conditions_of_the_tie(i):
    B, K, h, w, thr = FIELD_CASES[i]
    r = tie_case(i)
    first = r["first"]
    print("tie on case %d: first valid hypothesis %s, its copy at k = %d (lane %d)" % (i, first, K, K % 64))
    assert r["choice"].shape == (B, K + 1, 4) and not r["valid"][:, :3].any()
    assert (first >= 3).all() and r["valid"][np.arange(B), first].all() and not any(r["valid"][b, :first[b]].any() for b in range(B))
    assert K >= 64 and (first % 64 != K % 64).all()                          # the copy sits in another lane of the selection
    assert np.array_equal(r["choice"][:, K], r["choice"][np.arange(B), first])
    assert np.array_equal(r["hyp"][:, K], r["hyp"][np.arange(B), first])
    assert (r["count"][r["valid"]] == h * w).all() and r["border"].sum() == 0 and (~r["valid"]).sum() > 3 * B
    assert np.array_equal(r["best"], first) and (r["n_inl"] == h * w).all()


def test_conditions_of_the_fallback_boundary():
    """The field without structure: a pixel is either within 0.1 thr (a draw's own points, off only by the fp32 rounding of the nine
    coefficients) or beyond 2 thr.  Offsets of +-64 px against a threshold of 0.05 px, and hypotheses with a horizon inside the field,
    are beyond what the relative 1e-4 of `border` was made for, so the distance of every decision from the threshold, and of every qz
    from 0, is held here to 10x a bound on the error of the kernel's fp32 evaluation (fp32_margins): fp32 must count what the
    restatement counts.  Some sample's best count is exactly 4, and some sample has valid hypotheses but none with 4 inliers."""
    r = wild_case()
    v = r["valid"]
    d, slack, horizon, front = fp32_margins(r["pf"], r["hyp"])
    d, slack, horizon, front = d[v], slack[v], horizon[v], front[v]
    near = d <= 2 * WILD_THR
    top = r["count"].max(1)
    room = (np.abs(d - WILD_THR) / slack)[front]
    print("wild field: counts of the valid hypotheses %s; best %s with counts %s; largest error below the threshold %.2e px, smallest "
          "above %.3f px; smallest |d - thr| / (fp32 error bound) %.1f, smallest |qz| / (its fp32 error bound) %.1f" %
          (np.bincount(r["count"][v], minlength=5), r["best"], top, d[near].max(), d[~near & np.isfinite(d)].min(),
           room.min(), horizon.min()))
    assert r["border"].sum() == 0 and r["count"][v].max() == 4 and r["count"][v].min() < 4
    assert d[near].max() <= 0.1 * WILD_THR
    assert horizon.min() >= 10.0 and room.min() >= 10.0
    a, b = np.nonzero(top == 4)[0], np.nonzero((top >= 0) & (top < 4))[0]
    assert len(a) and len(b)
    assert (r["n_inl"][a] == 4).all() and (r["n_inl"][b] == 0).all() and (r["mask"][b] == 1).all()
    assert (r["best"][b] > 0).any() and (r["best"][a] > 0).any()
    for s in a:                                                              # the four inliers are the draw's own points
        assert np.array_equal(np.nonzero(r["mask"][s].reshape(-1))[0], np.sort(r["choice"][s, r["best"][s]]))
    assert np.isfinite(r["H"]).all() and np.isfinite(r["delta_hat"]).all()
    Hs, ds = refit(r["pf"], r["mask"], svd=True)
    rel = np.abs(ds - r["delta_hat"]).reshape(WILD_B, -1).max(1) / (np.abs(r["delta_hat"]).reshape(WILD_B, -1).max(1) + max(WILD_H, WILD_W))
    print("wild field: refit, eigh against SVD: |delta_hat| difference relative to the corner coordinate %s; max |delta_hat| %s" %
          (rel, np.abs(r["delta_hat"]).reshape(WILD_B, -1).max(1)))
    assert (rel <= 2e-5 / 128 / 10).all()
