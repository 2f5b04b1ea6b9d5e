"""Robust homography of a perspective field (bh_ransac_homography / NoOpHead ALL_POINTS_FIT='ransac'): the boundary, the head's
kwargs, and the yardstick the GPU tests (tests/test_ransac_gpu.py) compare against - a float64 numpy restatement of the algorithm
(minimal-sample hypotheses, inlier counts, selection, inlier mask and Hartley-normalised refit), written from the specification in
include/bihome.h and checked here on its own: on a field with 0.3 px noise, a 30 % block of wrong offsets and 5 % scattered outliers
it recovers the true 4-point offsets to a fraction of a pixel where the least-squares fit of the lattice points is off by tens."""
import ctypes
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
    rng = np.random.default_rng(noise_seed)
    pf = clean.astype(np.float64) + rng.normal(0.0, 0.3, clean.shape)
    bh, bw = h // 2, int(np.ceil(0.3 * h * w / (h // 2)))          # a contiguous block of 30 % of the patch
    assert bh * bw >= 0.3 * h * w
    for b in range(B):
        y0, x0 = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
        ang = rng.uniform(0, 2 * np.pi)
        centre = clean[b, :, y0 + bh // 2, x0 + bw // 2].astype(np.float64)
        const = centre + 90.0 * np.array([np.cos(ang), np.sin(ang)])
        away = np.sqrt(((clean[b, :, y0:y0 + bh, x0:x0 + bw] - const[:, None, None]) ** 2).sum(0)).min()
        assert away >= 40.0, away                                   # every pixel of the block is >= 40 px from its true offset
        pf[b, :, y0:y0 + bh, x0:x0 + bw] = const[:, None, None]
        idx = rng.choice(h * w, size=int(round(0.05 * h * w)), replace=False)      # a further 5 %: scattered, uniform in +-64 px
        pf[b].reshape(2, -1)[:, idx] = rng.uniform(-64.0, 64.0, (2, idx.size))
    choice = torch.randint(0, h * w, (B, K, 4), generator=torch.Generator().manual_seed(choice_seed)).numpy()
    return pf.astype(np.float32), choice.astype(np.int64), np.asarray(d["delta"], np.float64), clean


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


def dlt(src, dst, h, w):
    """Hartley-normalised DLT (smallest eigenvector of A^T A), /(H22 + 1e-8); -> (H [3,3], delta_hat [4,2])."""
    T1, T2 = _hartley(src), _hartley(dst)
    a = np.concatenate([src, np.ones((len(src), 1))], 1) @ T1.T
    q = np.concatenate([dst, np.ones((len(dst), 1))], 1) @ T2.T
    z = np.zeros_like(a)
    A = np.concatenate([np.concatenate([a, z, -q[:, :1] * a], 1), np.concatenate([z, a, -q[:, 1:2] * a], 1)], 0)
    _, vec = np.linalg.eigh(A.T @ A)
    H = np.linalg.inv(T2) @ vec[:, 0].reshape(3, 3) @ T1
    H = H / (H[2, 2] + 1e-8)
    c = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    p = np.concatenate([c, np.ones((4, 1))], 1) @ H.T
    return H, p[:, :2] / p[:, 2:] - c


def refit(pf, mask):
    """Least squares over the pixels of mask -> H [B,3,3], delta_hat [B,4,2]."""
    B, _, h, w = pf.shape
    x, y, u, v = _coords(pf)
    Hs, ds = [], []
    for b in range(B):
        m = mask[b].reshape(-1).astype(bool)
        H, dh = dlt(np.stack([x[m], y[m]], 1), np.stack([u[b][m], v[b][m]], 1), h, w)
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
