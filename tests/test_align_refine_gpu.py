"""The ECC refinement on the device (csrc/ecc.hip: bh_gray_pyramid_u8, bh_ecc_sums, bh_ecc_step, bh_ecc_refine; bihome_amd/align.py
gray_pyramid / ecc_sums / ecc_step / ecc_refine / Aligner(refine="ecc")) against the numpy float64 statements of bihome_amd/align.py,
which tests/test_align_refine_cpu.py holds to independent restatements (the helpers and the pair generator are taken from there).

Bounds.  Pyramid: bitwise equal to the float32 restatement f32_pyramid.  One pass: n exact; each of the 66 sums within SUMS_BOUND of the
float64 statement relative to sum |term| of that sum, SUMS_BOUND = 4 x F32_DEVIATION = 4 x 6.0e-7 = 2.4e-6: the float32 numpy
restatement of the per-pixel arithmetic deviates by 5.9e-7 at these shapes (measured on the host, test_align_refine_cpu.py), and the
factor 4 is for the reciprocal's Newton step and the different order of the partial sums.  Pixels whose float64 (u, v) lies within 1e-3
px of a cell line are masked out (the bilinear derivative jumps there and a float32 tap may take the neighbouring cell); at most 2 % of
the pixels may be dropped that way (0.2 - 0.5 % are).  Measured on an MI355X: 1.5e-7 .. 4.1e-7 over the three shapes and two seeds.  One step: 1e-9 of max |d| (double against double, the same operations in the same
order; measured: 7e-17 absolute on steps of 0.6 - 0.9).  Convergence: a condition - the mean corner error falls to at most 1/4 of the start's for every sample."""
import numpy as np
import pytest
import torch

import poisoned_alloc
import test_align_refine_cpu as C
from bihome_amd import align, configs

pytestmark = pytest.mark.gpu

SUMS_BOUND = 4 * C.F32_DEVIATION
N_BIG = 9400        # 240 x 320 x 3 bytes per image: image 9,321 is the first that starts past 2^31 bytes (tests/test_align_gpu.py)


def cuda(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to("cuda")          # (a copy: the shared inputs are read-only)
    return t if dtype is None else t.to(dtype)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def level_views(pyr, h, w, levels):
    return [align.pyramid_level(pyr, h, w, levels, l).cpu().numpy() for l in range(levels)]


# ------------------------------------------------------------------------------------------------
# bh_gray_pyramid_u8
# ------------------------------------------------------------------------------------------------
def test_pyramid_of_odd_sizes_with_an_index_list(monkeypatch):
    p = poisoned_alloc.poison(monkeypatch, align)          # the output handed out NaN-filled between red zones
    imgs = np.random.RandomState(3).randint(0, 256, (4, 37, 53, 3)).astype(np.uint8)
    order, clamped = (2, 0, 3, 7, -5), (2, 0, 3, 3, 0)     # 7 and -5 lie outside the bank: its last and first image
    idx = torch.tensor(order, dtype=torch.int32, device="cuda")
    pyr = align.gray_pyramid(cuda(imgs), 5, 3, idx=idx)
    assert pyr.shape == (5, 2546) and pyr.dtype == torch.float32
    want = C.f32_pyramid(imgs[list(clamped)], 3)
    for got, w in zip(level_views(pyr, 37, 53, 3), want):
        assert got.shape == w.shape and np.array_equal(got.view(np.int32), w.view(np.int32))          # bitwise (and no NaN left)
    again = align.gray_pyramid(cuda(imgs), 5, 3, idx=idx)
    assert torch.equal(bits(again), bits(pyr))                                                        # two calls, equal bits
    assert "gray_pyramid" in p.callers() and p.verify() == 2                                          # nothing written outside the output
    assert np.abs(want[0].astype(np.float64) - align.gray_pyramid_host(imgs[list(clamped)], 3)[0]).max() < 1e-4


def test_pyramid_48x80_two_levels():
    imgs = np.random.RandomState(4).randint(0, 256, (2, 48, 80, 3)).astype(np.uint8)
    pyr = align.gray_pyramid(cuda(imgs), 2, 2)
    for got, w in zip(level_views(pyr, 48, 80, 2), C.f32_pyramid(imgs, 2)):
        assert np.array_equal(got.view(np.int32), w.view(np.int32))
    with pytest.raises(ValueError, match="48 x 80"):
        align.gray_pyramid(cuda(imgs), 2, 4)


def test_pyramid_offsets_are_64_bit():
    """The last image of a bank that starts past 2^31 bytes: a 32-bit byte offset reads it from the wrong place."""
    data = torch.randint(0, 256, (N_BIG, 240, 320, 3), dtype=torch.uint8, device="cuda")
    assert (N_BIG - 1) * 230400 >= 2 ** 31
    idx = torch.tensor([N_BIG - 1], dtype=torch.int32, device="cuda")
    pyr = align.gray_pyramid(data, 1, 1, idx=idx)
    want = C.f32_pyramid(data[N_BIG - 1:].cpu().numpy(), 1)[0]
    assert np.array_equal(pyr.cpu().numpy().reshape(1, 240, 320).view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------------
# bh_ecc_sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.SUMS_SHAPES, ids=["24x40-onto-24x40", "48x80-onto-56x88", "97x131-onto-97x131"])
def test_sums_match_the_host_statement(monkeypatch, shape):
    p = poisoned_alloc.poison(monkeypatch, align)          # partial blocks and sums handed out NaN-filled between red zones
    for seed in (0, 1):
        A, T, H, mask = C.sums_case(seed, *shape)
        share = C.masked_share(mask)
        assert share <= 0.02, share
        dev = [cuda(x) for x in (A, T, H, mask)]
        got = align.ecc_sums(*dev).cpu().numpy()
        assert got.shape == (2, 66)
        worst = 0.0
        for b in range(2):
            want, scale = align.ecc_sums_host(A[b], T[b], H[b], mask[b]), C.abs_term_sums(A[b], T[b], H[b], mask[b])
            assert got[b, 65] == want[65] and 0 < want[65] <= T[b].size                  # n is exact
            worst = max(worst, float((np.abs(got[b] - want) / scale).max()))
        print("sums %s seed %d: %.2f %% of the pixels masked, n = %s of %d, max |kernel - float64| / sum |term| = %.3e (bound %.3e)"
              % (shape, seed, 100 * share, got[:, 65].tolist(), T[0].size, worst, SUMS_BOUND))
        assert worst <= SUMS_BOUND
        again = align.ecc_sums(*dev)
        assert np.array_equal(again.cpu().numpy().view(np.int64), got.view(np.int64))    # two calls, equal bits
    assert "ecc_sums" in p.callers() and p.verify() == 8
    if shape[:2] == shape[2:]:
        assert got[:, 65].max() < T[0].size - share * T[0].size                          # (part of B falls outside A)


def test_sums_on_views_of_a_pyramid():
    """Planes that are strided views of packed pyramid rows (what bh_ecc_refine passes), level 1 of 37 x 53 onto level 1 of 48 x 80, random
    bytes (steeper gradients than the textures of SUMS_SHAPES) under a map that also scales.  The bound follows the same rule on these
    very inputs: 4 x the largest deviation of the float32 restatement from the float64 statement, computed here (8.2e-7 for sample 0,
    1.9e-6 for sample 1, so 7.5e-6)."""
    rs = np.random.RandomState(5)
    ia, ib = rs.randint(0, 256, (2, 48, 80, 3)).astype(np.uint8), rs.randint(0, 256, (2, 37, 53, 3)).astype(np.uint8)
    pa, pb = align.gray_pyramid(cuda(ia), 2, 2), align.gray_pyramid(cuda(ib), 2, 2)
    a, t = align.pyramid_level(pa, 48, 80, 2, 1), align.pyramid_level(pb, 37, 53, 2, 1)
    assert not a.is_contiguous() and a.shape == (2, 24, 40) and t.shape == (2, 18, 26)
    H = np.stack([np.array([[1.0, 0.01, 3.3], [-0.02, 1.0, 2.6], [1e-4, 0, 1.0]]), np.array([[1.1, 0, 0.4], [0, 0.9, 1.7], [0, 2e-4, 1.0]])])
    ys, xs = np.mgrid[0:18, 0:26].astype(np.float64)
    q = np.stack([xs, ys, np.ones_like(xs)], -1) @ H.transpose(0, 2, 1)[:, None]
    u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
    mask = ((np.abs(u - np.round(u)) >= 1e-3) & (np.abs(v - np.round(v)) >= 1e-3)).astype(np.uint8)          # off the cell lines, as in sums_case
    assert C.masked_share(mask) <= 0.02
    got = align.ecc_sums(a, t, cuda(H), cuda(mask)).cpu().numpy()
    planes = [(a[b].cpu().numpy(), t[b].cpu().numpy()) for b in range(2)]
    ref = [(align.ecc_sums_host(A, T, H[b], mask[b]), C.abs_term_sums(A, T, H[b], mask[b])) for b, (A, T) in enumerate(planes)]
    bound = 4 * max(float((np.abs(C.ecc_sums_f32(A, T, H[b], mask[b]) - ref[b][0]) / ref[b][1]).max()) for b, (A, T) in enumerate(planes))
    for b, (want, scale) in enumerate(ref):
        assert got[b, 65] == want[65] and want[65] > 100
        worst = float((np.abs(got[b] - want) / scale).max())
        print("sums on pyramid views, sample %d: n = %d, max |kernel - float64| / sum |term| = %.3e (bound %.3e)" % (b, want[65], worst, bound))
        assert worst <= bound


def test_a_mask_of_zeros_counts_nothing_and_the_sample_keeps_its_start():
    A, T, H, mask = C.sums_case(0, *C.SUMS_SHAPES[0])
    Hd = cuda(H)
    sums = align.ecc_sums(cuda(A), cuda(T), Hd, cuda(np.zeros_like(mask)))
    assert (sums == 0).all()
    state, stats = align.ecc_step(sums, align.ecc_state(Hd), last=1)
    s = state.cpu().numpy()
    assert np.array_equal(s[:, 0:9], H.reshape(2, 9)) and np.array_equal(s[:, 9:18], H.reshape(2, 9))          # bitwise (H[2,2] is 1)
    assert (s[:, 19] == 1).all() and (s[:, 21] == 0).all() and np.isnan(stats.cpu().numpy()[:, 0]).all()


# ------------------------------------------------------------------------------------------------
# bh_ecc_step
# ------------------------------------------------------------------------------------------------
def host_sums():
    """(H [2,3,3], sums [2,66]) of the statement itself: full-size gray planes of two related pairs (seeds 0 and 1) at their starts."""
    pairs = [C.make_pair(seed, 48, 64, 1.5) for seed in (0, 1)]
    H = np.stack([q[3] for q in pairs])
    planes = [(align.gray_pyramid_host(q[0][None], 1)[0][0], align.gray_pyramid_host(q[1][None], 1)[0][0]) for q in pairs]
    return H, np.stack([align.ecc_sums_host(a, t, h) for (a, t), h in zip(planes, H)])


def test_step_matches_the_host_statement():
    H, sums = host_sums()
    state, _ = align.ecc_step(cuda(sums), align.ecc_state(cuda(H)), last=0)
    s = state.cpu().numpy()
    for b in range(2):
        rho, d = align.ecc_step_host(sums[b])
        got = s[b, 0:8] - H[b].reshape(9)[:8]
        # cur = H + d: the subtraction above loses what the addition rounded away, at most an ulp of |H| <= 2^-52 * 256
        err = np.abs(got - d).max()
        print("step sample %d: max |d| %.3e, max |kernel - host| %.3e, rho %.6f" % (b, np.abs(d).max(), err, rho))
        assert err <= 1e-9 * np.abs(d).max() + 2.0 ** -44
        assert s[b, 8] == 1.0 and np.array_equal(s[b, 9:18], H[b].reshape(9)) and abs(s[b, 18] - rho) <= 1e-12 and s[b, 19] == 0
        assert s[b, 20] == s[b, 18] and s[b, 21] == 1 and s[b, 22] == 1
    # the same sums once more: rho did not rise, so cur goes back to best and the sample freezes; a third call changes nothing
    state, _ = align.ecc_step(cuda(sums), state, last=0)
    s2 = state.cpu().numpy()
    assert np.array_equal(s2[:, 0:9], H.reshape(2, 9)) and (s2[:, 19] == 1).all() and (s2[:, 21] == 1).all()
    state, stats = align.ecc_step(cuda(sums), state.clone(), last=2)
    s3, st = state.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(st[:, 0], s2[:, 20]) and np.array_equal(st[:, 1], s2[:, 18]) and (st[:, 2] == 1).all()
    for b in range(2):                                     # last = 2: a level down, the books reset
        assert np.abs(s3[b, 0:9] - align.h_level_down(H[b]).reshape(9)).max() <= 1e-12 * np.abs(s3[b, 0:9]).max()
        assert np.array_equal(s3[b, 0:9], s3[b, 9:18]) and s3[b, 18] == -np.inf and (s3[b, 19:23] == 0).all()


def test_a_singular_system_freezes_the_sample():
    """A constant image A: no variance, nothing to solve - the sample freezes and its H is bitwise what was passed in."""
    A, T, H, mask = C.sums_case(1, *C.SUMS_SHAPES[0])
    flat = np.full_like(A, 77.0)
    sums = align.ecc_sums(cuda(flat), cuda(T), cuda(H), cuda(mask))
    assert align.ecc_step_host(sums[0].cpu().numpy())[1] is None
    state, _ = align.ecc_step(sums, align.ecc_state(cuda(H)), last=0)
    s = state.cpu().numpy()
    assert np.array_equal(s[:, 0:9], H.reshape(2, 9)) and (s[:, 19] == 1).all() and (s[:, 21] == 0).all()


# ------------------------------------------------------------------------------------------------
# bh_ecc_refine
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,levels,move", C.CONVERGENCE, ids=["48x64-2-levels", "96x128-3-levels"])
def test_refinement_converges(monkeypatch, h, w, levels, move):
    """Seeds 0..5 as one batch, iters = 10: the mean corner error against the true homography falls to at most 1/4 of the start's for
    EVERY sample (the statement alone reaches 0.001 .. 0.082 of the start), and rho_best >= rho at the first pass on every level."""
    p = poisoned_alloc.poison(monkeypatch, align)
    pairs = [C.make_pair(seed, h, w, move) for seed in range(6)]
    A, B, H_true, H_start = (np.stack([q[i] for q in pairs]) for i in range(4))
    H, stats = align.ecc_refine(cuda(A), cuda(B), cuda(H_start), levels=levels, iters=10)
    assert H.shape == (6, 3, 3) and H.dtype == torch.float64 and stats.shape == (6, levels, 3) and stats.dtype == torch.float64
    again, stats2 = align.ecc_refine(cuda(A), cuda(B), cuda(H_start), levels=levels, iters=10)
    assert torch.equal(bits(again), bits(H)) and torch.equal(bits(stats2), bits(stats))          # two calls, equal bits
    assert p.verify() == 8                                                                        # 2 x (two pyramids, stats, workspace) inside their red zones
    H, stats = H.cpu().numpy(), stats.cpu().numpy()
    for seed in range(6):
        e0, e1 = C.corner_error(H_start[seed], H_true[seed], h, w), C.corner_error(H[seed], H_true[seed], h, w)
        print("%d x %d seed %d: %.3f -> %.4f px (%.3f of the start), rho %s, steps %s"
              % (h, w, seed, e0, e1, e1 / e0, stats[seed, :, :2].round(5).tolist(), stats[seed, :, 2].tolist()))
        assert H[seed, 2, 2] == 1.0 and e1 <= 0.25 * e0
    assert (stats[:, :, 1] >= stats[:, :, 0]).all() and (stats[:, :, 2] >= 0).all() and (stats[:, :, 2] <= 10).all()


def test_refinement_with_a_mask_and_without_steps():
    A, B, H_true, H_start = (x[None] for x in C.make_pair(2, 48, 64, 1.5))
    dev = [cuda(x) for x in (A, B, H_start)]
    H0, stats0 = align.ecc_refine(*dev, levels=2, iters=0)                 # iters = 0: one pass per level, no step - the start comes back
    assert np.abs(H0.cpu().numpy() - H_start).max() <= 1e-12 and (stats0[:, :, 2] == 0).all() and torch.equal(stats0[:, :, 0], stats0[:, :, 1])
    nothing = torch.zeros((1, 48, 64), dtype=torch.uint8, device="cuda")
    Hn, statsn = align.ecc_refine(*dev, levels=2, iters=3, mask=nothing)   # nothing counts: the start comes back
    assert np.abs(Hn.cpu().numpy() - H_start).max() <= 1e-12 and torch.isnan(statsn[:, :, 0]).all()
    m = np.zeros((1, 48, 64), np.uint8)
    m[0, 6:42, 6:58] = 3
    Hm, statsm = align.ecc_refine(*dev, levels=2, iters=10, mask=cuda(m))
    want, _ = align.ecc_refine_host(A, B, H_start, 2, 10, mask=m)
    e0, e1 = C.corner_error(H_start[0], H_true[0], 48, 64), C.corner_error(Hm[0].cpu().numpy(), H_true[0], 48, 64)
    print("masked: %.3f -> %.4f px; the statement: %.4f px" % (e0, e1, C.corner_error(want[0], H_true[0], 48, 64)))
    assert e1 <= 0.25 * e0 and (statsm[:, :, 1] >= statsm[:, :, 0]).all()
    with pytest.raises(ValueError, match="mask"):
        align.ecc_refine(*dev, levels=2, mask=nothing[:, :40])
    with pytest.raises(ValueError, match="48 x 64"):
        align.ecc_refine(*dev, levels=4)


# ------------------------------------------------------------------------------------------------
# Aligner(refine="ecc")
# ------------------------------------------------------------------------------------------------
class StubHead(torch.nn.Module):
    def __init__(self, delta):
        super().__init__()
        self.delta = delta

    def predict_homography(self, data):
        return self.delta, None


TODAY = {"delta_hat", "H", "patch_1", "patch_2", "geom_a", "geom_b", "aligned", "valid"}


def test_aligner_refines_between_the_lift_and_the_warp():
    from bihome_amd import kernels as K
    from bihome_amd.step import build_model
    pairs = [C.make_pair(seed, 48, 80, 1.5) for seed in (0, 1)]
    a, b = cuda(np.stack([q[0] for q in pairs])), cuda(np.stack([q[1] for q in pairs]))
    with K.det_scope(True):
        model = build_model(configs.get("zeng-bihome"), "cuda:0")
        aligner = align.Aligner(model, patch=128)
        torch.manual_seed(7)
        plain = aligner(a, b)
        torch.manual_seed(7)
        r = aligner(a, b, refine="ecc")
    assert set(plain) == TODAY and set(r) == TODAY | {"H_model", "rho", "refine_stats"}
    # without refine: today's keys and bits - H is the lifted matrix, aligned its warp
    H_lift = align.lift_device(plain["delta_hat"], 128, plain["geom_a"], plain["geom_b"])
    assert torch.equal(plain["H"], H_lift) and torch.equal(r["H_model"], plain["H"]) and torch.equal(r["delta_hat"], plain["delta_hat"])
    out, valid = align.warp_u8(a, plain["H"], 48, 80)
    assert torch.equal(plain["aligned"], out) and torch.equal(plain["valid"], valid)
    assert r["H"].shape == (2, 3, 3) and r["H"].dtype == torch.float64 and r["H_model"].dtype == torch.float64
    assert r["rho"].shape == (2, 2) and r["rho"].dtype == torch.float64 and r["refine_stats"].shape == (2, 3, 3)
    assert r["aligned"].shape == (2, 48, 80, 3) and r["aligned"].dtype == torch.uint8 and r["valid"].shape == (2, 48, 80)
    print("rho before / after: %s" % r["rho"].cpu().tolist())
    assert (r["rho"][:, 1] >= r["rho"][:, 0]).all() and torch.equal(r["rho"], r["refine_stats"][:, 0, :2])
    out, valid = align.warp_u8(a, r["H"], 48, 80)
    assert torch.equal(r["aligned"], out) and torch.equal(r["valid"], valid)          # aligned is the warp of the REFINED H
    H, stats = align.ecc_refine(a, b, r["H_model"])
    assert torch.equal(H, r["H"]) and torch.equal(bits(stats), bits(r["refine_stats"]))


def test_aligner_refine_copies_nothing_to_the_host_and_checks_its_arguments(monkeypatch):
    from bihome_amd import kernels as K
    A, B, H_true, H_start = (x[None] for x in C.make_pair(1, 96, 128, 3.0))
    P = 16
    g = np.array([[128 / P, 96 / P, 0.5 * 128 / P - 0.5, 0.5 * 96 / P - 0.5]])
    Hp = np.linalg.inv(align._affine(g)[0]) @ H_start[0] @ align._affine(g)[0]
    c = align.patch_corners(P)
    delta = C.project(Hp, c) - c                            # the delta that `lift` maps to H_start
    aligner = align.Aligner(torch.nn.Sequential(StubHead(cuda(delta[None], torch.float32))), patch=P)
    a, b = cuda(A), cuda(B)
    mask = torch.ones((1, 96, 128), dtype=torch.uint8, device="cuda")
    aligner(a, b, refine="ecc", mask_b=mask)                # (first call: the corner square is made and kept)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                 # a device-to-host copy (or any other synchronising call) raises
    try:
        r = aligner(a, b, refine="ecc", mask_b=mask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    e0, e1 = C.corner_error(r["H_model"][0].cpu().numpy(), H_true[0], 96, 128), C.corner_error(r["H"][0].cpu().numpy(), H_true[0], 96, 128)
    print("Aligner: model %.3f px -> refined %.4f px" % (e0, e1))
    assert e1 <= 0.25 * e0
    launches = []
    pyramid = K.gray_pyramid_u8
    monkeypatch.setattr(K, "gray_pyramid_u8", lambda *x, **k: launches.append(1) or pyramid(*x, **k))
    prep = K.align_prep_u8
    monkeypatch.setattr(K, "align_prep_u8", lambda *x, **k: launches.append(1) or prep(*x, **k))
    with pytest.raises(ValueError, match="refine is None or 'ecc'"):
        aligner(a, b, refine="ECC")
    with pytest.raises(ValueError, match="96 x 128"):
        aligner(a, b, refine="ecc", refine_levels=5)
    for bad in (mask[:, :90], mask.to(torch.float32), mask.cpu()):
        with pytest.raises(ValueError, match="mask"):
            aligner(a, b, refine="ecc", mask_b=bad)
    with pytest.raises(ValueError, match="mask_b"):
        aligner(a, b, mask_b=mask)
    assert not launches                                     # every refusal came before any launch
