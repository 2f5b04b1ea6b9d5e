"""The ECC refinement's statement (bihome_amd/align.py: gray_pyramid_host, ecc_sums_host, ecc_step_host, ecc_level_host,
ecc_refine_host) held to independent restatements, and the refusals of the new entry points - all without a GPU.
tests/test_align_refine_gpu.py holds the kernels (csrc/ecc.hip) to the statement and takes its helpers from here.

F32_DEVIATION.  `ecc_sums_f32` restates the per-pixel arithmetic of the kernel in float32 numpy (tap_project's and tap_place's
operations, float32 terms and products, float64 accumulation).  Its largest deviation from the float64 statement over the 66 sums,
relative to sum |term| of each, at the shapes and seeds the GPU test uses (SUMS_SHAPES, seeds 0..3, pixels within 1e-3 px of a cell line
masked out) was measured as 5.9e-7; test_f32_restatement_stays_inside_the_measured_deviation keeps that figure honest."""
import ctypes
import functools

import numpy as np
import pytest

from bihome_amd import align, synth

F32_DEVIATION = 6.0e-7             # measured 5.912e-7 (module docstring), rounded up
SUMS_SHAPES = ((24, 40, 24, 40), (48, 80, 56, 88), (97, 131, 97, 131))          # (Hb, Wb, Ha, Wa)
MARGIN = 8                         # pixels of texture around image A that image B may look into


# ------------------------------------------------------------------------------------------------
# helpers shared with the GPU tests
# ------------------------------------------------------------------------------------------------
def corners(h, w):
    return np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)


def project(H, pts):
    q = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ np.asarray(H, np.float64).reshape(3, 3).T
    return q[:, :2] / q[:, 2:]


def corner_error(H, H_true, h, w):
    """Mean distance between the images of B's four corners under H and under H_true, in pixels of A."""
    c = corners(h, w)
    return float(np.linalg.norm(project(H, c) - project(H_true, c), axis=1).mean())


@functools.lru_cache(maxsize=None)
def make_pair(seed, h, w, move):
    """(A, B uint8 [h,w,3], H_true, H_start): A is the middle of a synth.texture_image MARGIN pixels larger on every side, B that texture
    seen through H_true (B's index coordinates -> A's; corners moved by up to 4 % of the sides), so B has no black border - then a gain
    in [0.8, 1.2] and a bias in [-20, 20], rounded and clipped to uint8.  H_start moves the true corner images by up to `move` pixels."""
    rng = np.random.default_rng(seed)
    tex = synth.texture_image(rng, h + 2 * MARGIN, w + 2 * MARGIN)
    A = np.floor(tex[MARGIN:MARGIN + h, MARGIN:MARGIN + w] + 0.5).astype(np.uint8)
    c = corners(h, w)
    H_true = synth.four_point_homography(c, c + rng.uniform(-0.04, 0.04, (4, 2)) * np.array([w, h]))
    shift = np.array([[1.0, 0, MARGIN], [0, 1, MARGIN], [0, 0, 1]])
    Bf = synth.warp_bilinear(tex, shift @ H_true, h, w)
    gain, bias = rng.uniform(0.8, 1.2), rng.uniform(-20, 20)
    B = np.floor(np.clip(gain * Bf + bias, 0, 255) + 0.5).astype(np.uint8)
    H_start = synth.four_point_homography(c, project(H_true, c) + rng.uniform(-move, move, (4, 2)))
    for a in (A, B, H_true, H_start):
        a.setflags(write=False)
    return A, B, H_true, H_start


@functools.lru_cache(maxsize=None)
def sums_case(seed, Hb, Wb, Ha, Wa):
    """(A [2,Ha,Wa] gray float32-exact planes, T [2,Hb,Wb], H [2,3,3], mask [2,Hb,Wb] uint8) for the one-pass tests: gray level 0 of
    two textures, near-identity corner homographies (B's corners onto A's corners moved by up to 3 px), and the mask that drops every
    pixel whose float64 (u, v) lies within 1e-3 px of an integer line."""
    rng = np.random.default_rng(100 + seed)
    imgs = lambda n, h, w: np.stack([np.floor(synth.texture_image(rng, h, w) + 0.5).astype(np.uint8) for _ in range(n)])
    A, T = f32_pyramid(imgs(2, Ha, Wa), 1)[0], f32_pyramid(imgs(2, Hb, Wb), 1)[0]
    H = np.stack([synth.four_point_homography(corners(Hb, Wb), corners(Ha, Wa) + rng.uniform(-3, 3, (4, 2))) for _ in range(2)])
    ys, xs = np.mgrid[0:Hb, 0:Wb].astype(np.float64)
    mask = np.empty((2, Hb, Wb), np.uint8)
    for b in range(2):
        q = np.stack([xs, ys, np.ones_like(xs)], -1) @ H[b].T
        u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
        mask[b] = (np.abs(u - np.round(u)) >= 1e-3) & (np.abs(v - np.round(v)) >= 1e-3)
    for a in (A, T, H, mask):
        a.setflags(write=False)
    return A, T, H, mask


def abs_term_sums(A, T, H, mask):
    """sum |z_i z_j| of the float64 statement: what the bound on each of the 66 sums is relative to."""
    z, _ = align.ecc_terms_host(A, T, H, mask)
    z = np.abs(z.reshape(align.ECC_NZ, -1))
    return (z @ z.T)[np.triu_indices(align.ECC_NZ)]


def f32_fma(a, b, c):
    """float32 fma: the product of two floats is exact in double, one double addition, one rounding to float."""
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def f32_pyramid(images_u8, levels):
    """The float32 restatement of bh_gray_pyramid_u8: [levels] arrays [B,h_l,w_l] float32, the kernel's operations one by one (the gray
    value's two fused multiply-adds are exact sums in double here: multiples of 2^-27 below 2^9)."""
    v = np.asarray(images_u8).astype(np.float32)
    f = np.float32
    g = f32_fma(np.full_like(v[..., 2], f(0.114)), v[..., 2], f32_fma(np.full_like(v[..., 1], f(0.587)), v[..., 1], f(0.299) * v[..., 0]))
    out = [g]
    for h, w in align.pyramid_sizes(v.shape[1], v.shape[2], levels)[1:]:
        p = out[-1]
        out.append(((p[:, 0:2 * h:2, 0:2 * w:2] + p[:, 0:2 * h:2, 1:2 * w:2]) + (p[:, 1:2 * h:2, 0:2 * w:2] + p[:, 1:2 * h:2, 1:2 * w:2])) * f(0.25))
        assert out[-1].dtype == np.float32
    return out


def ecc_sums_f32(A, T, H, mask=None):
    """The kernel's per-pixel arithmetic in float32 numpy (csrc/warp_tap.h tap_project / tap_place, csrc/ecc.hip ecc_pixel), products
    z_i z_j rounded to float32, accumulated in float64 -> the 66 sums."""
    f = np.float32
    A, T = np.asarray(A, f), np.asarray(T, f)
    h = (np.asarray(H, np.float64).reshape(9) / np.asarray(H, np.float64).reshape(9)[8]).astype(f)
    (Ha, Wa), (Hb, Wb) = A.shape, T.shape
    ys, xs = np.mgrid[0:Hb, 0:Wb].astype(f)
    with np.errstate(all="ignore"):
        qx, qy, qz = (f32_fma(np.full_like(xs, h[3 * r]), xs, f32_fma(np.full_like(ys, h[3 * r + 1]), ys, h[3 * r + 2])) for r in range(3))
        ok = qz > f(1e-8)
        iz = (f(1) / np.where(ok, qz, f(1))).astype(f)
        u, v = qx * iz, qy * iz
        x0f, y0f = np.floor(u), np.floor(v)
        fx, fy = u - x0f, v - y0f
        ok &= (x0f >= 0) & (x0f + 1 <= Wa - 1) & (y0f >= 0) & (y0f + 1 <= Ha - 1)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    x0, y0 = np.where(ok, x0f, 0).astype(np.int64), np.where(ok, y0f, 0).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, Wa - 1), np.minimum(y0 + 1, Ha - 1)
    a00, a01, a10, a11 = A[y0, x0], A[y0, x1], A[y1, x0], A[y1, x1]
    wx0, wx1, wy0, wy1 = f(1) - fx, fx, f(1) - fy, fy
    iw = f32_fma(a11, wx1 * wy1, f32_fma(a10, wx0 * wy1, f32_fma(a01, wx1 * wy0, a00 * (wx0 * wy0))))
    gx = f32_fma(fy, a11 - a10, (f(1) - fy) * (a01 - a00))
    gy = f32_fma(fx, a11 - a01, (f(1) - fx) * (a10 - a00))
    m = -f32_fma(gy, v, gx * u)
    gxz, gyz, mz = gx * iz, gy * iz, m * iz
    z = np.stack([gxz * xs, gxz * ys, gxz, gyz * xs, gyz * ys, gyz, mz * xs, mz * ys, iw, T, np.ones_like(T)])
    assert z.dtype == np.float32
    z = np.where(ok, z, f(0)).reshape(align.ECC_NZ, -1)
    iu = np.triu_indices(align.ECC_NZ)
    return np.array([(z[i] * z[j]).astype(np.float64).sum() for i, j in zip(*iu)])


def masked_share(mask):
    return 1.0 - float(np.asarray(mask, bool).mean())


# ------------------------------------------------------------------------------------------------
# the pyramid and the level change
# ------------------------------------------------------------------------------------------------
def test_pyramid_sizes_of_odd_shapes():
    assert align.pyramid_sizes(37, 53, 3) == [(37, 53), (18, 26), (9, 13)]
    assert align.pyramid_offsets(37, 53, 3).tolist() == [0, 1961, 2429, 2546]
    img = np.random.RandomState(0).randint(0, 256, (2, 37, 53, 3)).astype(np.uint8)
    pyr = align.gray_pyramid_host(img, 3)
    assert [p.shape for p in pyr] == [(2, 37, 53), (2, 18, 26), (2, 9, 13)]
    g = img.astype(np.float64) @ np.array([0.299, 0.587, 0.114])
    assert np.abs(pyr[0] - g).max() < 1e-12
    # level 2, pixel (y, x): the mean of the 4 x 4 block of level 0 at (4 y, 4 x); row 36 and column 52 (and 17 / 25 of level 1) are dropped
    assert abs(pyr[2][1, 8, 12] - g[1, 32:36, 48:52].mean()) < 1e-12
    assert np.abs(np.stack([f.astype(np.float64) for f in f32_pyramid(img, 3)][:1]) - pyr[0]).max() < 1e-4


def test_pyramid_refuses_what_it_does_not_build():
    for h, w, levels in ((37, 53, 4), (16, 15, 2), (64, 64, 0), (640, 640, 7)):
        with pytest.raises(ValueError):
            align.pyramid_sizes(h, w, levels)
    with pytest.raises(ValueError, match="37 x 53.*4 x 6"):
        align.pyramid_sizes(37, 53, 4)
    assert align.pyramid_sizes(8, 8, 1) == [(8, 8)] and align.pyramid_sizes(256, 256, 6)[-1] == (8, 8)


def test_mask_pyramid_needs_all_four_bytes():
    m = np.ones((1, 17, 20), np.uint8) * 7
    m[0, 5, 9] = 0
    p = align.mask_pyramid_host(m, 2)
    assert p[0].max() == 1 and p[0].sum() == 17 * 20 - 1 and p[1].shape == (1, 8, 10)
    want = np.ones((8, 10), np.uint8)
    want[2, 4] = 0
    assert np.array_equal(p[1][0], want)


def test_level_change_follows_the_points():
    """Pixel x of level l sits at 2 x + 0.5 of level l - 1: a point projected at the coarse level and then taken down equals the point
    taken down and projected with C H C^-1."""
    rng = np.random.RandomState(1)
    H = synth.four_point_homography(corners(20, 30), corners(20, 30) + rng.uniform(-2, 2, (4, 2)))
    pts = rng.uniform(0, 20, (7, 2))
    down = lambda p: 2.0 * p + 0.5
    Hd = align.h_level_down(H)
    assert Hd[2, 2] == 1.0 and np.abs(project(Hd, down(pts)) - down(project(H, pts))).max() < 1e-10
    assert np.abs(align.h_level_up(Hd) - H / H[2, 2]).max() < 1e-12


# ------------------------------------------------------------------------------------------------
# one pass
# ------------------------------------------------------------------------------------------------
def small_case(seed=0):
    rng = np.random.RandomState(seed)
    A, T = rng.uniform(0, 255, (12, 16)), rng.uniform(0, 255, (12, 16))
    H = synth.four_point_homography(corners(12, 16), corners(12, 16) + rng.uniform(-2, 2, (4, 2))) * 1.7          # (H[2,2] != 1: used as H / H[2,2])
    mask = (rng.uniform(size=(12, 16)) > 0.3).astype(np.uint8)
    return A, T, H, mask


def iw_at(A, p, x, y):
    """The bilinear value of A at the image of (x, y) under p = H[0..7] (H[8] = 1), or None where the pixel does not count."""
    qz = p[6] * x + p[7] * y + 1.0
    if not qz > 1e-8:
        return None
    u, v = (p[0] * x + p[1] * y + p[2]) / qz, (p[3] * x + p[4] * y + p[5]) / qz
    if not (0 <= u < A.shape[1] - 1 and 0 <= v < A.shape[0] - 1):
        return None
    x0, y0 = int(np.floor(u)), int(np.floor(v))
    fx, fy = u - x0, v - y0
    return (1 - fy) * ((1 - fx) * A[y0, x0] + fx * A[y0, x0 + 1]) + fy * ((1 - fx) * A[y0 + 1, x0] + fx * A[y0 + 1, x0 + 1]), u, v


@pytest.mark.parametrize("with_mask", [False, True], ids=["no-mask", "mask"])
def test_sums_against_a_pixel_loop(with_mask):
    A, T, H, mask = small_case()
    p = (H / H[2, 2]).reshape(9)[:8]
    G, counted = np.zeros((11, 11)), 0
    for y in range(12):
        for x in range(16):
            r = iw_at(A, p, x, y)
            if r is None or (with_mask and not mask[y, x]):
                continue
            iw, u, v = r
            x0, y0 = int(np.floor(u)), int(np.floor(v))
            fx, fy = u - x0, v - y0
            gx = (1 - fy) * (A[y0, x0 + 1] - A[y0, x0]) + fy * (A[y0 + 1, x0 + 1] - A[y0 + 1, x0])
            gy = (1 - fx) * (A[y0 + 1, x0] - A[y0, x0]) + fx * (A[y0 + 1, x0 + 1] - A[y0, x0 + 1])
            m = -(gx * u + gy * v)
            qz = p[6] * x + p[7] * y + 1.0
            z = np.array([gx * x, gx * y, gx, gy * x, gy * y, gy, m * x, m * y, iw * qz, T[y, x] * qz, qz]) / qz
            G += np.outer(z, z)
            counted += 1
    s = align.ecc_sums_host(A, T, H, mask if with_mask else None)
    assert s.shape == (66,) and s[65] == counted and 40 < counted < 192          # (part of T falls outside A)
    for i in range(11):
        for j in range(11):
            assert abs(s[align.ecc_index(i, j)] - G[i, j]) <= 1e-10 * abs(G).max(), (i, j)
    assert [align.ecc_index(i, j) for i in range(11) for j in range(i, 11)] == list(range(66))          # row-major upper triangle
    assert align.ecc_index(10, 10) == 65 and align.ecc_index(10, 8) == align.ecc_index(8, 10)


def test_jacobian_against_central_differences():
    """j = d iw / d p with p = H[0..7] / H[8], on pixels at least 1e-3 px from a cell line (the derivative jumps there)."""
    A, T, H, _ = small_case(2)
    p = (H / H[2, 2]).reshape(9)[:8]
    z, ok = align.ecc_terms_host(A, T, H)
    eps, checked = 1e-6, 0
    for y in range(12):
        for x in range(16):
            r = iw_at(A, p, x, y)
            if r is None:
                assert not ok[y, x]
                continue
            _, u, v = r
            if min(abs(u - round(u)), abs(v - round(v))) < 1e-3:
                continue
            assert ok[y, x] and abs(z[8, y, x] - r[0]) < 1e-10
            for k in range(8):
                e = np.zeros(8)
                e[k] = eps * max(1.0, abs(p[k]))
                num = (iw_at(A, p + e, x, y)[0] - iw_at(A, p - e, x, y)[0]) / (2 * e[k])
                assert abs(z[k, y, x] - num) <= 1e-5 * max(1.0, abs(num)), (x, y, k, z[k, y, x], num)
            checked += 1
    assert checked > 60


# ------------------------------------------------------------------------------------------------
# one step
# ------------------------------------------------------------------------------------------------
def sums_of(z):
    """The 66 sums of hand-made terms z [11, n]."""
    return (z @ z.T)[np.triu_indices(11)]


def hand_made_terms(seed=0, n=200):
    rng = np.random.RandomState(seed)
    j = rng.standard_normal((8, n)) * np.array([30, 30, 3, 30, 30, 3, 900, 900])[:, None]
    iw = 120 + 40 * rng.standard_normal(n)
    t = 1.1 * iw + 9 + 0.02 * (j.T @ rng.standard_normal(8)) + rng.standard_normal(n)
    return np.concatenate([j, iw[None], t[None], np.ones((1, n))])


def test_step_against_numpy_linalg_solve():
    z = hand_made_terms()
    rho, d = align.ecc_step_host(sums_of(z))
    j, iw, t = z[:8], z[8], z[9]
    jc, iwc, tc = j - j.mean(1, keepdims=True), iw - iw.mean(), t - t.mean()
    G = jc @ jc.T
    ya, yc = np.linalg.solve(G, jc @ iwc), np.linalg.solve(G, jc @ tc)
    lam = (iwc @ iwc - (jc @ iwc) @ ya) / (iwc @ tc - (jc @ tc) @ ya)
    want = lam * yc - ya
    assert abs(rho - (iwc @ tc) / np.sqrt((iwc @ iwc) * (tc @ tc))) < 1e-12
    assert np.abs(d - want).max() <= 1e-8 * np.abs(want).max()


def test_step_failure_rules():
    z = hand_made_terms()
    nan = lambda r: r != r
    # n < 16
    rho, d = align.ecc_step_host(sums_of(z[:, :15]))
    assert nan(rho) and d is None
    assert align.ecc_step_host(sums_of(z[:, :16]))[1] is not None
    # a variance that is not positive: a constant image A, a constant image B
    for row in (8, 9):
        c = z.copy()
        c[row] = 64.0
        rho, d = align.ecc_step_host(sums_of(c))
        assert nan(rho) and d is None
    # a zero pivot: a Jacobian column of zeros (no gradient along it)
    c = z.copy()
    c[3] = 0.0
    rho, d = align.ecc_step_host(sums_of(c))
    assert rho == rho and d is None
    # a NaN pivot
    s = sums_of(z)
    s[align.ecc_index(0, 0)] = np.nan
    assert align.ecc_step_host(s)[1] is None
    # lambda's denominator not > 0: B is the negative of A
    c = z.copy()
    c[9] = -c[8]
    rho, d = align.ecc_step_host(sums_of(c))
    assert rho < 0 and d is None
    # a d that is not finite
    s = sums_of(z)
    s[align.ecc_index(2, 9)] = np.inf
    assert align.ecc_step_host(s)[1] is None


# ------------------------------------------------------------------------------------------------
# levels and the whole refinement
# ------------------------------------------------------------------------------------------------
CONVERGENCE = ((48, 64, 2, 1.5), (96, 128, 3, 3.0))          # (h, w, levels, start moved by up to)


@functools.lru_cache(maxsize=None)
def refined_on_the_host(seed, h, w, levels, move):
    A, B, H_true, H_start = make_pair(seed, h, w, move)
    H, stats = align.ecc_refine_host(A[None], B[None], H_start[None], levels, 10)
    return H[0], stats[0]


@pytest.mark.parametrize("h,w,levels,move", CONVERGENCE, ids=["48x64-2-levels", "96x128-3-levels"])
def test_statement_converges_and_rho_never_falls(h, w, levels, move):
    """The condition of the GPU test, on the statement alone: the mean corner error falls to at most 1/4 of the start's for every seed
    0..5 (measured here: 0.001 .. 0.082 of the start), and rho_best >= rho at the level's first pass on every level."""
    for seed in range(6):
        _, _, H_true, H_start = make_pair(seed, h, w, move)
        H, stats = refined_on_the_host(seed, h, w, levels, move)
        e0, e1 = corner_error(H_start, H_true, h, w), corner_error(H, H_true, h, w)
        print("%d x %d seed %d: %.3f -> %.4f px (%.3f of the start), rho %s" % (h, w, seed, e0, e1, e1 / e0, stats[:, :2].round(5).tolist()))
        assert H[2, 2] == 1.0 and e1 <= 0.25 * e0
        assert (stats[:, 1] >= stats[:, 0]).all() and (stats[:, 2] >= 1).all() and (stats[:, 2] <= 10).all()


def test_a_level_keeps_its_start_when_nothing_can_be_measured():
    A, B, _, H_start = make_pair(0, 48, 64, 1.5)
    ga, gb = align.gray_pyramid_host(A[None], 1)[0][0], align.gray_pyramid_host(B[None], 1)[0][0]
    best, rho_first, rho_best, accepted = align.ecc_level_host(ga, gb, H_start, 3, np.zeros((48, 64), np.uint8))
    assert np.array_equal(best, H_start / H_start[2, 2]) and rho_first != rho_first and rho_best == -np.inf and accepted == 0
    # iters = 0: one pass, no step - the start with its rho
    best, rho_first, rho_best, accepted = align.ecc_level_host(ga, gb, H_start, 0)
    assert np.array_equal(best, H_start / H_start[2, 2]) and rho_first == rho_best and accepted == 0
    # a mask restricts what counts
    m = np.zeros((1, 48, 64), np.uint8)
    m[0, 8:40, 8:56] = 1
    H, stats = align.ecc_refine_host(A[None], B[None], H_start[None], 2, 4, mask=m)
    assert (stats[0, :, 1] >= stats[0, :, 0]).all() and not np.array_equal(H[0], refined_on_the_host(0, 48, 64, 2, 1.5)[0])


# ------------------------------------------------------------------------------------------------
# the float32 restatement (what the GPU test's bound on the sums is derived from)
# ------------------------------------------------------------------------------------------------
def f32_deviation(seed, shape):
    A, T, H, mask = sums_case(seed, *shape)
    worst = 0.0
    for b in range(2):
        want, scale = align.ecc_sums_host(A[b], T[b], H[b], mask[b]), abs_term_sums(A[b], T[b], H[b], mask[b])
        got = ecc_sums_f32(A[b], T[b], H[b], mask[b])
        assert got[65] == want[65]                       # n: the same pixels count
        worst = max(worst, float((np.abs(got - want) / scale).max()))
    return worst


def test_f32_restatement_stays_inside_the_measured_deviation():
    worst = 0.0
    for shape in SUMS_SHAPES:
        for seed in range(4):
            share = masked_share(sums_case(seed, *shape)[3])
            assert share <= 0.02, (shape, seed, share)
            worst = max(worst, f32_deviation(seed, shape))
    print("float32 restatement: largest |sum - float64 sum| / sum |term| = %.3e (F32_DEVIATION %.1e)" % (worst, F32_DEVIATION))
    assert worst <= F32_DEVIATION


# ------------------------------------------------------------------------------------------------
# the C entry points without a GPU: every refusal and every empty batch returns before any launch
# ------------------------------------------------------------------------------------------------
OK, BADARG, UNSUPPORTED = 0, -1, -2


class Raw:
    """Host buffers standing in for device memory (a refused call never touches them; they are compared afterwards)."""

    def __init__(self):
        self.bufs = {}

    def ptr(self, name, nbytes=4096):
        b = self.bufs.setdefault(name, np.full(nbytes, 0x5A, np.uint8))
        return b.ctypes.data_as(ctypes.c_void_p)

    def untouched(self):
        return all((b == 0x5A).all() for b in self.bufs.values())


def raw_call(entry, **over):
    """Call `entry` with valid small arguments, `over` replacing some (a pointer name -> None for NULL); -> (rc, Raw)."""
    from bihome_amd import _lib
    r = Raw()
    P = r.ptr
    base = {
        "bh_gray_pyramid_layout": dict(H=37, W=53, levels=3, offsets=P("offsets")),
        "bh_gray_pyramid_u8": dict(images=P("images"), idx=None, n_images=2, H=37, W=53, B=2, levels=3, pyr=P("pyr"), stream=None),
        "bh_ecc_sums_ws_doubles": dict(Hb=24, Wb=40, B=2, doubles=P("doubles")),
        "bh_ecc_sums": dict(a=P("a"), Ha=24, Wa=40, a_stride=960, t=P("t"), Hb=24, Wb=40, t_stride=960, mask=None, H64=P("H64"), B=2,
                            partial=P("partial"), sums=P("sums"), stream=None),
        "bh_ecc_step": dict(sums=P("sums"), state=P("state"), B=2, last=0, stats=None, stats_stride=3, stream=None),
        "bh_ecc_refine_ws_doubles": dict(Hb=24, Wb=40, B=2, doubles=P("doubles")),
        "bh_ecc_refine": dict(pyr_a=P("pyr_a"), Ha=24, Wa=40, pyr_b=P("pyr_b"), Hb=24, Wb=40, mask_pyr=None, B=2, levels=2, iters=3,
                              H64=P("H64"), stats=P("stats"), ws=P("ws"), stream=None),
    }[entry]
    assert set(over) <= set(base), set(over) - set(base)
    args = dict(base, **over)
    return getattr(_lib.lib, entry)(*args.values()), r


REFUSALS = [
    ("bh_gray_pyramid_layout", dict(offsets=None), BADARG), ("bh_gray_pyramid_layout", dict(H=0), BADARG),
    ("bh_gray_pyramid_layout", dict(W=-3), BADARG), ("bh_gray_pyramid_layout", dict(levels=0), UNSUPPORTED),
    ("bh_gray_pyramid_layout", dict(levels=7), UNSUPPORTED), ("bh_gray_pyramid_layout", dict(levels=4), UNSUPPORTED),
    ("bh_gray_pyramid_layout", dict(H=32768, W=32768, levels=1), UNSUPPORTED),
    ("bh_gray_pyramid_u8", dict(images=None), BADARG), ("bh_gray_pyramid_u8", dict(pyr=None), BADARG),
    ("bh_gray_pyramid_u8", dict(B=-1), BADARG), ("bh_gray_pyramid_u8", dict(n_images=0), BADARG), ("bh_gray_pyramid_u8", dict(H=0), BADARG),
    ("bh_gray_pyramid_u8", dict(W=0), BADARG), ("bh_gray_pyramid_u8", dict(levels=0), UNSUPPORTED),
    ("bh_gray_pyramid_u8", dict(levels=7), UNSUPPORTED), ("bh_gray_pyramid_u8", dict(levels=4), UNSUPPORTED),
    ("bh_gray_pyramid_u8", dict(H=15, levels=2), UNSUPPORTED), ("bh_gray_pyramid_u8", dict(B=0), OK),
    ("bh_ecc_sums_ws_doubles", dict(doubles=None), BADARG), ("bh_ecc_sums_ws_doubles", dict(B=-1), BADARG),
    ("bh_ecc_sums_ws_doubles", dict(Hb=0), BADARG), ("bh_ecc_sums_ws_doubles", dict(Hb=32768, Wb=32768), UNSUPPORTED),
    ("bh_ecc_sums", dict(a=None), BADARG), ("bh_ecc_sums", dict(t=None), BADARG), ("bh_ecc_sums", dict(H64=None), BADARG),
    ("bh_ecc_sums", dict(partial=None), BADARG), ("bh_ecc_sums", dict(sums=None), BADARG), ("bh_ecc_sums", dict(B=-1), BADARG),
    ("bh_ecc_sums", dict(Ha=0), BADARG), ("bh_ecc_sums", dict(Wa=0), BADARG), ("bh_ecc_sums", dict(Hb=0), BADARG),
    ("bh_ecc_sums", dict(Wb=-1), BADARG), ("bh_ecc_sums", dict(a_stride=959), BADARG), ("bh_ecc_sums", dict(t_stride=0), BADARG),
    ("bh_ecc_sums", dict(Ha=32768, Wa=32768, a_stride=1 << 30), UNSUPPORTED), ("bh_ecc_sums", dict(B=0), OK),
    ("bh_ecc_step", dict(sums=None), BADARG), ("bh_ecc_step", dict(state=None), BADARG), ("bh_ecc_step", dict(B=-1), BADARG),
    ("bh_ecc_step", dict(last=3), BADARG), ("bh_ecc_step", dict(last=-1), BADARG), ("bh_ecc_step", dict(B=0), OK),
    ("bh_ecc_refine_ws_doubles", dict(doubles=None), BADARG), ("bh_ecc_refine_ws_doubles", dict(B=-1), BADARG),
    ("bh_ecc_refine_ws_doubles", dict(Wb=0), BADARG),
    ("bh_ecc_refine", dict(pyr_a=None), BADARG), ("bh_ecc_refine", dict(pyr_b=None), BADARG), ("bh_ecc_refine", dict(H64=None), BADARG),
    ("bh_ecc_refine", dict(stats=None), BADARG), ("bh_ecc_refine", dict(ws=None), BADARG), ("bh_ecc_refine", dict(B=-1), BADARG),
    ("bh_ecc_refine", dict(Ha=0), BADARG), ("bh_ecc_refine", dict(Wb=0), BADARG), ("bh_ecc_refine", dict(iters=-1), BADARG),
    ("bh_ecc_refine", dict(levels=0), UNSUPPORTED), ("bh_ecc_refine", dict(levels=7), UNSUPPORTED),
    ("bh_ecc_refine", dict(levels=3), UNSUPPORTED), ("bh_ecc_refine", dict(Hb=15), UNSUPPORTED), ("bh_ecc_refine", dict(B=0), OK),
]


@pytest.mark.parametrize("entry,over,code", REFUSALS, ids=["%s-%s" % (e[3:], "-".join("%s=%s" % kv for kv in o.items())) for e, o, _ in REFUSALS])
def test_refusals_and_empty_batches_return_before_any_launch(entry, over, code):
    """Without a GPU a call that got as far as a launch returns a hipError_t (> 0) instead of the documented code."""
    rc, r = raw_call(entry, **over)
    assert rc == code, "%s %s returned %d, the header documents %d" % (entry, over, rc, code)
    assert r.untouched()


def test_size_queries_and_the_python_layout_agree():
    from bihome_amd import _lib, kernels as K
    assert (_lib.ECC_SUMS, _lib.ECC_STATE) == (align.ECC_SUMS, 24)
    for h, w, levels in ((37, 53, 3), (48, 80, 2), (480, 640, 3), (256, 256, 6), (8, 8, 1)):
        assert K.gray_pyramid_layout(h, w, levels) == align.pyramid_offsets(h, w, levels).tolist()
    assert K.ecc_sums_ws_doubles(24, 40, 2) == 2 * 66 and K.ecc_sums_ws_doubles(480, 640, 64) == 64 * 19 * 66
    assert K.ecc_refine_ws_doubles(480, 640, 64) == 64 * 24 + K.ecc_sums_ws_doubles(480, 640, 64)
    assert K.ecc_sums_ws_doubles(24, 40, 0) == 0
    with pytest.raises(_lib.BihomeLibError, match="BH_E_UNSUPPORTED"):
        K.gray_pyramid_layout(37, 53, 4)


def test_python_refuses_before_any_launch():
    import torch
    a = torch.zeros((1, 37, 53, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        align.gray_pyramid(a, 1, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        align.ecc_refine(a, a, torch.eye(3, dtype=torch.float64)[None])
    with pytest.raises(ValueError, match="refine is None or 'ecc'"):
        align.Aligner(torch.nn.Sequential(torch.nn.Identity()), patch=16)(a, a, refine="lk")
