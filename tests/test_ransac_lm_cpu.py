"""Levenberg-Marquardt polish of the RANSAC homography (bh_homography_refine_lm / NoOpHead RANSAC_REFINE='lm'): the boundary, the
head's kwargs, and the yardstick the GPU tests (tests/test_ransac_lm_gpu.py) compare against - a float64 numpy restatement of the
specification in include/bihome.h (written from that text, with the full 2n x 8 Jacobian, not from the kernel), plus a 100-step run of
the same restatement as the converged minimiser.  Its own properties are asserted here: on the inputs of tests/test_ransac_cpu.py and
on the same fields with N(0, 2 px) added the cost never rises, ten steps are converged, and the polish moves the corners by at least
100x the tolerance the GPU comparison uses - so that comparison cannot pass on an implementation that does nothing."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ransac_cpu import FIELD_CASES, _coords, field_case, mace, make_inputs, ransac_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE2_SEED, NOISE2_SIGMA = 3, 2.0
LM_ITERS = 10


def make_noisy_inputs():
    """make_inputs()' fields with N(0, 2 px) added (seed 3): a field as rough as a half-trained network's."""
    pf, choice, delta, clean = make_inputs()
    rng = np.random.default_rng(NOISE2_SEED)
    return (pf.astype(np.float64) + rng.normal(0.0, NOISE2_SIGMA, pf.shape)).astype(np.float32), choice, delta, clean


SHAPES = [(64, 256), (160, 136), (3, 700), (5, 7), (37, 83)]


def make_shape_inputs(h, w, B=2):
    """A field of any size for the polish alone: one mild homography + N(0, 1 px), a random mask of 80 %, and a start that is off by
    a few tenths of a pixel.  -> pf [B,2,h,w] f32, mask [B,h,w] u8, start [B,3,3] f32"""
    g = np.random.default_rng(17)
    Ht = np.array([[1.02, 0.03, 4.0], [-0.02, 0.98, -3.0], [1e-4, -5e-5, 1.0]])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    q = np.stack([xs, ys, np.ones_like(xs)], -1) @ Ht.T
    field = np.stack([q[..., 0] / q[..., 2] - xs, q[..., 1] / q[..., 2] - ys])
    pf = (field[None] + g.normal(0.0, 1.0, (B, 2, h, w))).astype(np.float32)
    mask = (g.uniform(size=(B, h, w)) < 0.8).astype(np.uint8)
    start = np.tile((Ht + np.array([[2e-3, -1e-3, 0.3], [1e-3, 2e-3, -0.2], [2e-6, 1e-6, 0.0]]))[None], (B, 1, 1)).astype(np.float32)
    return pf, mask, start


def dh_atol(h, w):
    """The GPU comparison's band for delta_hat: 2e-5 px is fp32 output rounding at 128-pixel corner coordinates."""
    return 2e-5 * max(1.0, max(h, w) / 128.0)


# ------------------------------------------------------------------------------------------------
# the restatement (float64), from include/bihome.h
# ------------------------------------------------------------------------------------------------
def _solve(A, rhs):
    """Gaussian elimination with partial pivoting -> (d, ok); ok is the pivot rule: every |pivot| > 1e-12, d finite."""
    S = np.concatenate([A, rhs[:, None]], 1).astype(np.float64)
    n = len(rhs)
    ok = True
    with np.errstate(all="ignore"):
        for k in range(n):
            r = k + int(np.argmax(np.abs(S[k:, k])))
            if r != k:
                S[[k, r]] = S[[r, k]]
            if not abs(S[k, k]) > 1e-12:
                ok = False
            for i in range(k + 1, n):
                S[i, k + 1:] -= (S[i, k] / S[k, k]) * S[k, k + 1:]
        d = np.zeros(n)
        for k in range(n - 1, -1, -1):
            d[k] = (S[k, n] - S[k, k + 1:n] @ d[k + 1:]) / S[k, k]
    return d, bool(ok and np.isfinite(d).all())


def _evaluate(p, x, y, u, v):
    """-> cost, J^T J [8,8], J^T r [8], all qz > 0"""
    with np.errstate(all="ignore"):
        qx, qy, qz = p[0] * x + p[1] * y + p[2], p[3] * x + p[4] * y + p[5], p[6] * x + p[7] * y + 1.0
        px, py = qx / qz, qy / qz
        r = np.concatenate([px - u, py - v])
        z = np.zeros_like(x)
        Jx = np.stack([x / qz, y / qz, 1.0 / qz, z, z, z, -x * px / qz, -y * px / qz], 1)
        Jy = np.stack([z, z, z, x / qz, y / qz, 1.0 / qz, -x * py / qz, -y * py / qz], 1)
        J = np.concatenate([Jx, Jy], 0)
        return float(r @ r), J.T @ J, J.T @ r, bool((qz > 0).all())


def _corners(p, h, w):
    c = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    q = np.concatenate([c, np.ones((4, 1))], 1) @ np.append(p, 1.0).reshape(3, 3).T
    with np.errstate(all="ignore"):
        sc = np.where(np.abs(q[:, 2]) > 1e-8, 1.0 / q[:, 2], 1.0)
    return q[:, :2] * sc[:, None] - c


def lm_sample(H, x, y, u, v, h, w, iters):
    """One sample.  -> dict(H [3,3] f64, delta_hat [4,2], info [4], costs: the cost after every step)."""
    H = np.asarray(H, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        start = H[:8] / H[8]
    p, lam, accepted = start.copy(), 1e-3, 0
    cost, A, g, front = _evaluate(p, x, y, u, v)
    cost0, costs = cost, [cost]
    live = len(x) >= 4 and bool(np.isfinite(start).all()) and bool(np.isfinite(cost)) and front
    failed = False
    for _ in range(iters):
        if live:
            d, ok = _solve(A + lam * np.diag(np.diag(A)), -g)
            if not ok:
                live, failed = False, True
            else:
                t = p + d
                ct, At, gt, ft = _evaluate(t, x, y, u, v)
                if np.isfinite(ct) and ft and ct < cost:
                    p, cost, A, g = t, ct, At, gt
                    lam = max(lam / 10.0, 1e-12)
                    accepted += 1
                else:
                    lam = min(lam * 10.0, 1e12)
        costs.append(cost)
    if failed:
        p, cost, accepted = start, cost0, 0
    Hout = np.append(p, 1.0).reshape(3, 3) if accepted else H.reshape(3, 3)
    return dict(H=Hout, delta_hat=_corners(p, h, w), info=np.array([cost0, cost, accepted, lam]), costs=np.array(costs))


def lm_reference(pf, H, mask=None, iters=LM_ITERS):
    """pf [B,2,h,w], H [B,3,3], mask [B,h,w] or None -> dict of stacked lm_sample results."""
    B, _, h, w = pf.shape
    x, y, u, v = _coords(pf)
    out = []
    for b in range(B):
        m = np.ones(h * w, bool) if mask is None else mask[b].reshape(-1) != 0
        out.append(lm_sample(H[b], x[m], y[m], u[b][m], v[b][m], h, w, iters))
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
def test_header_and_ctypes_signature_agree():
    from bihome_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bihome.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bh_homography_refine_lm\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/bihome.h does not declare bh_homography_refine_lm"
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else {"int": ctypes.c_int, "float": ctypes.c_float}[arg.split()[0]])
    assert _lib.SIGNATURES["bh_homography_refine_lm"] == want
    assert len(want) == 10 and want[2:6] == [ctypes.c_int] * 4
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bh_homography_refine_lm")


def test_bad_arguments_are_refused_before_any_launch():
    from bihome_amd import _lib
    f = _lib.lib.bh_homography_refine_lm
    p = ctypes.c_void_p(64)         # never dereferenced: the argument check comes first
    assert f(None, p, 1, 128, 128, 10, p, p, p, None) == -1          # NULL field
    assert f(p, p, 1, 128, 128, 10, None, p, p, None) == -1          # NULL H
    assert f(p, p, 1, 128, 128, 10, p, None, p, None) == -1          # NULL delta_hat
    assert f(p, p, 1, 128, 128, 10, p, p, None, None) == -1          # NULL work
    assert f(p, None, -1, 128, 128, 10, p, p, p, None) == -1         # B < 0
    assert f(p, None, 1, 1, 3, 10, p, p, p, None) == -1              # h*w < 4
    assert f(p, None, 1, 128, 128, -1, p, p, p, None) == -1          # iters < 0
    assert f(p, None, 70000, 128, 128, 10, p, p, p, None) == -2      # more samples than one launch takes
    assert f(p, None, 0, 128, 128, 10, p, p, p, None) == 0           # empty batch: nothing to do (mask NULL is valid)


def test_noophead_kwargs_and_wrapper():
    from bihome_amd import kernels as K
    from bihome_amd.heads import NoOpHead
    kw = dict(TARGET_GEN="all_points", LEARNING_KEYS=["target", "pf_hat_12", "delta", "pf_hat_12"], ALL_POINTS_FIT="ransac")
    m = NoOpHead.Model(None, **kw)
    assert (m.ransac_refine, m.ransac_lm_iters) == ("none", 10)
    m = NoOpHead.Model(None, RANSAC_REFINE="lm", RANSAC_LM_ITERS=4, **kw)
    assert (m.ransac_refine, m.ransac_lm_iters) == ("lm", 4)
    with pytest.raises(ValueError):
        NoOpHead.Model(None, RANSAC_REFINE="bogus", **kw)
    with pytest.raises(ValueError):
        NoOpHead.Model(None, RANSAC_REFINE="lm", RANSAC_LM_ITERS=0, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.homography_refine_lm(torch.zeros(1, 2, 8, 8), torch.eye(3).reshape(1, 3, 3))


@pytest.fixture(scope="module")
def sets():
    out = {}
    for name, (pf, choice, delta, clean) in (("test", make_inputs()), ("noisy", make_noisy_inputs())):
        r = ransac_reference(pf, choice)
        out[name] = dict(pf=pf, delta=delta, clean=clean, choice=choice, mask=r["mask"], H=r["H"], refit=r["delta_hat"],
                         lm10=lm_reference(pf, r["H"], r["mask"], 10), lm100=lm_reference(pf, r["H"], r["mask"], 100))
    return out


@pytest.mark.parametrize("name,least_move", [("test", 2e-3), ("noisy", 0.05)])
def test_conditions_the_gpu_comparison_rests_on(sets, name, least_move):
    """The restatement alone.  Observed when the test was written: corners moved by >= 4.4e-3 px (test inputs) and >= 0.10 px (noisy);
    the bounds asserted are at least 100x the 2e-5 px the GPU comparison allows."""
    s = sets[name]
    a, z = s["lm10"], s["lm100"]
    moved = np.abs(a["delta_hat"] - s["refit"]).reshape(len(a["H"]), -1).max(1)
    gain = (a["info"][:, 0] - a["info"][:, 1]) / a["info"][:, 0]
    print(name, "corners moved by", moved, "relative cost gain", gain, "accepted", a["info"][:, 2], "inliers", s["mask"].reshape(len(moved), -1).sum(1))
    print(name, "10 vs 100 steps:", np.abs(a["delta_hat"] - z["delta_hat"]).max())
    assert (np.diff(a["costs"], axis=1) <= 0).all() and (np.diff(z["costs"], axis=1) <= 0).all()      # the cost never rises
    assert (a["info"][:, 1] <= a["info"][:, 0]).all() and (a["info"][:, 2] >= 1).all()
    assert np.abs(a["delta_hat"] - z["delta_hat"]).max() <= 1e-9
    assert (moved >= least_move).all(), moved
    assert np.isfinite(a["H"]).all() and (a["H"][:, 2, 2] == 1.0).all()


@pytest.mark.parametrize("h,w", SHAPES)
def test_conditions_at_the_other_field_shapes(h, w):
    """The restatement alone, on what tests/test_ransac_lm_gpu.py::test_other_field_shapes runs: the polish moves the corners by at
    least 100x the band of that comparison (dh_atol), the cost never rises and every sample accepts a step."""
    pf, mask, start = make_shape_inputs(h, w)
    a, z = lm_reference(pf, start, mask, LM_ITERS), lm_reference(pf, start, mask, 0)
    moved = np.abs(a["delta_hat"] - z["delta_hat"]).reshape(len(pf), -1).max(1)
    print("%d x %d: corners moved by %s (100x the band: %.3e), accepted %s, cost %s -> %s" %
          (h, w, moved, 100 * dh_atol(h, w), a["info"][:, 2], a["info"][:, 0], a["info"][:, 1]))
    assert (moved >= 100 * dh_atol(h, w)).all()
    assert (np.diff(a["costs"], axis=1) <= 0).all() and (a["info"][:, 2] >= 1).all()
    assert np.isfinite(a["H"]).all() and np.isfinite(a["delta_hat"]).all()


def test_conditions_of_the_chained_run():
    """RANSAC then the polish on FIELD_CASES[0] (37 x 83, K = 1100), on the restatement's own mask and refit."""
    _, _, h, w, _ = FIELD_CASES[0]
    r = field_case(0)
    a = lm_reference(r["pf"], r["H"], r["mask"], LM_ITERS)
    moved = np.abs(a["delta_hat"] - r["delta_hat"]).reshape(len(a["H"]), -1).max(1)
    print("37 x 83 after RANSAC: corners moved by", moved, "accepted", a["info"][:, 2])
    assert (moved >= 100 * dh_atol(h, w)).all() and (a["info"][:, 2] >= 1).all()
    assert (np.diff(a["costs"], axis=1) <= 0).all()


def test_polish_helps_on_the_noisy_field_and_leaves_an_exact_one(sets):
    s = sets["noisy"]
    before, after = mace(s["refit"], s["delta"]), mace(s["lm10"]["delta_hat"], s["delta"])
    print("noisy set: MACE refit", before, "-> polished", after)
    assert after.mean() < before.mean()
    t = sets["test"]
    print("test set: MACE refit", mace(t["refit"], t["delta"]), "-> polished", mace(t["lm10"]["delta_hat"], t["delta"]))
    # the exact field (exact up to its fp32 rounding): nothing to polish
    clean, choice = t["clean"], t["choice"]
    r = ransac_reference(clean, choice)
    assert (r["mask"] == 1).all()
    e = lm_reference(clean, r["H"], r["mask"], 10)
    moved = np.abs(e["delta_hat"] - r["delta_hat"]).max()
    print("exact field: corners moved by", moved, "costs", e["info"][:, :2])
    assert moved <= 1e-5


def test_restatement_keeps_the_start_where_the_header_says():
    pf, choice, _, _ = make_inputs(B=1, K=8)
    h, w = pf.shape[2:]
    H = np.array([[[1.0, 0.01, 3.0], [0.02, 1.0, -2.0], [1e-5, -1e-5, 1.0]]])
    m = np.zeros((1, h, w), np.uint8)
    m[0, 5, 7] = m[0, 60, 90] = m[0, 100, 20] = 1                       # three correspondences: fewer than four
    r = lm_reference(pf, H, m, 10)
    assert r["info"][0, 2] == 0 and r["info"][0, 0] == r["info"][0, 1] and np.array_equal(r["H"], H)
    np.testing.assert_allclose(r["delta_hat"][0], _corners(H[0].reshape(9)[:8], h, w))
    r = lm_reference(pf, H, None, 0)                                     # no step: the start's corners, two equal costs
    assert r["info"][0, 2] == 0 and r["info"][0, 0] == r["info"][0, 1] and np.array_equal(r["H"], H)
    Hn = H.copy(); Hn[0, 0, 0] = np.nan                                  # a non-finite start
    r = lm_reference(pf, Hn, None, 10)
    assert r["info"][0, 2] == 0
    Hb = H.copy(); Hb[0, 2] = [-0.02, 0.0, 1.0]                          # qz <= 0 for x >= 50 at the start
    r = lm_reference(pf, Hb, None, 10)
    assert r["info"][0, 2] == 0 and np.array_equal(r["H"], Hb)
