"""Parity of the head kernels (through the C ABI) with the CPU oracle on identical seeded inputs.

Tolerances: the kernels do their per-sample algebra in double, the reference does it in float32;
float32 outputs therefore agree with the *float64* oracle to float32 rounding of the result
(rtol 1e-5) and with the float32 oracle to its own conditioning noise (looser, stated per test).
Integer outputs (arg-min index) must be bit-exact.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bihome_amd import synth
from oracle import bihome_oracle as O
from test_conv_kernels_gpu import grad_result, grad_start

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from bihome_amd import kernels
    return kernels


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda().contiguous()


def rand_delta(B, seed, amp=32):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.uniform(-amp, amp, (B, 4, 2)).astype(np.float32)


def check_h4pt_fwd_bwd(K, size):
    """size: the patch extent, or (W, H)."""
    W, H = size if isinstance(size, tuple) else (size, size)
    B = 37
    d = rand_delta(B, 1)
    H64, H32 = K.h4pt_fwd(dev(d), size)
    dt = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    corners = torch.tensor([[0, 0], [W, 0], [W, H], [0, H]], dtype=torch.float64).repeat(B, 1, 1)
    Href = O.four_point_to_homography(corners, dt)
    np.testing.assert_allclose(H64.cpu().numpy().reshape(B, 3, 3), Href.detach().numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(H32.cpu().numpy(), Href.detach().numpy(), rtol=2e-6, atol=1e-7)
    # property: H maps corners -> corners + delta
    mapped = O.transform_points(H64.cpu().reshape(B, 3, 3), corners)
    np.testing.assert_allclose(mapped.numpy(), corners.numpy() + d, atol=1e-9)
    g = np.random.Generator(np.random.PCG64(2)).standard_normal((B, 9))
    g[:, 8] = 0
    (Href.reshape(B, 9) * torch.tensor(g)).sum().backward()
    gd = K.h4pt_bwd(dev(d), H64, dev(g, torch.float64), size)
    print("MEASURED h4pt %s: max |H64 - f64| %.3e, max |gdelta - f64| %.3e of %.3e" % (size, np.abs(H64.cpu().numpy().reshape(B, 3, 3) - Href.detach().numpy()).max(),
          np.abs(gd.cpu().numpy() - dt.grad.numpy()).max(), np.abs(dt.grad.numpy()).max()))
    np.testing.assert_allclose(gd.cpu().numpy(), dt.grad.numpy(), rtol=2e-5, atol=1e-7 * np.abs(dt.grad.numpy()).max())


def test_h4pt_fwd_bwd(K):
    check_h4pt_fwd_bwd(K, 128)


def check_dlt_fwd_bwd(K, n, P, pf, base=None, oracle32=True):
    """pf [B,2,h,w]: the perspective field the hypotheses are fitted to (the corners of delta_hat are those of the field's own extents).
    oracle32 False: without the comparison with the oracle's own float32 run - at P = 4 / 5 its float32 SVD of the (nearly) exactly
    determined system is 43 px / 7.8e-3 px from its float64 run on the 24 x 24 field of tests/shape_edges.py, no yardstick for 5e-3."""
    B, _, h, w = pf.shape
    choice = O.sample_choice(h * w, B * n * P, torch.Generator().manual_seed(5)).reshape(B, n * P)
    Hd, dh, eig = K.dlt_fwd(dev(pf), choice.cuda(), n, P)
    # float64 oracle
    head = O.BiHomEHead(torch.nn.Identity(), PATCH_SIZE=max(h, w), PATCH_KEYS=["patch_1", "patch_2"], DELTA_HAT_KEYS=[],
                        PF_KEYS=["a", "b"], RANSAC_HYPOTHESIS_NO=n, POINTS_PER_HYPOTHESIS=P, TRIPLET_LOSS="double-line",
                        TRIPLET_DISTANCE="l1", TRIPLET_AGGREGATION="channel-agnostic", TRIPLET_MARGIN="inf",
                        MASK_KEYS=[], TRIPLET_MU=0.01).double()
    pft = torch.tensor(pf, dtype=torch.float64, requires_grad=True)
    dref, Href, _ = head._delta_from_pf(pft, choice)
    np.testing.assert_allclose(Hd.cpu().numpy().reshape(B, n, 3, 3), Href.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dh.cpu().numpy().reshape(B, n, 4, 2), dref.detach().numpy(), atol=2e-5)
    # float32 oracle (what the reference computes): conditioning noise of its float32 SVD
    if oracle32:
        d32, H32, _ = head.float()._delta_from_pf(torch.tensor(pf), choice)
        np.testing.assert_allclose(dh.cpu().numpy().reshape(B, n, 4, 2), d32.detach().numpy(), atol=5e-3)
    # adjoint
    head.double()
    gd = np.random.Generator(np.random.PCG64(9)).standard_normal((B * n, 4, 2)).astype(np.float32)
    (dref.reshape(B * n, 4, 2) * torch.tensor(gd, dtype=torch.float64)).sum().backward()
    ref = pft.grad.numpy()
    if base is None:
        gpf = K.dlt_bwd(dev(pf), choice.cuda(), eig, dev(gd), n, P)
    else:
        # g_pf is a `+=` output (the wrapper hands the kernel a zeroed one): from a nonzero start, through the C entry point
        import ctypes
        from bihome_amd._lib import check, lib
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        args, buf = (dev(pf), choice.cuda(), dev(gd)), grad_start(base, ref)
        check(lib.bh_dlt_bwd(ptr(args[0]), ptr(args[1]), ptr(eig), ptr(args[2]), None, B, n, P, h, w, ptr(buf), K._fdet(),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "bh_dlt_bwd")
        gpf = grad_result(base, buf)
    print("MEASURED dlt n%d P%d %dx%d: max |Hdlt - f64| %.3e, |delta_hat - f64| %.3e, |g_pf - f64| %.3e of %.3e"
          % (n, P, h, w, np.abs(Hd.cpu().numpy().reshape(B, n, 3, 3) - Href.detach().numpy()).max(),
             np.abs(dh.cpu().numpy().reshape(B, n, 4, 2) - dref.detach().numpy()).max(), np.abs(gpf.cpu().numpy() - ref).max(), np.abs(ref).max()))
    np.testing.assert_allclose(gpf.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())


@pytest.mark.parametrize("n,P", [(1, 128), (4, 16), (2, 200)])
def test_dlt_fwd_bwd(K, n, P):
    check_dlt_fwd_bwd(K, n, P, synth.make_head_inputs(6, seed=3, noise=0.7)["pf_hat_12"])


def test_dsac_argmin_bit_exact(K, golden):
    g = golden("dsac_n4_f32")
    d = synth.make_head_inputs(8, 11, noise=2.0)
    pf = dev(d["pf_hat_12"])
    choice = torch.tensor(g["choice"]).cuda()
    Hd, dh, _ = K.dlt_fwd(pf, choice, 4, 16)
    err, best = K.dsac_score(pf, Hd.reshape(-1, 9).contiguous(), 4)
    assert np.array_equal(best.cpu().numpy(), g["best"])                       # integer: bit-exact
    np.testing.assert_allclose(err.cpu().numpy(), g["repr_error"], rtol=2e-4)
    sel = dh.reshape(8, 4, 4, 2)[torch.arange(8), best]
    np.testing.assert_allclose(sel.cpu().numpy(), g["delta_hat"], atol=5e-2)   # f32 SVD noise at P=16, noise=2px


# ~twice the largest error measured on the five cases (round 6, `pytest -s`, profiles/r06b_gpu_tests_measured.txt: 8e-6 ... 3.8e-5 of max |dL/dH|
# by build; rounds 1-5 allowed 2e-3): float32 coordinates and per-pixel products, double sums, against the float64 autograd of the oracle.
WARP_ADJOINT_BOUND = 1e-4


def coordinate_ties(H, h, w):
    """Pixels at which the warp has no derivative at float32 resolution.  The bilinear sampler's derivative jumps where a source coordinate
    crosses an integer, and the kernels place their taps from float32 coordinates (csrc/warp_tap.h: two fused multiply-adds per component of
    H.(x, y, 1), a reciprocal good to an ulp, one product) - within 8 * 2^-24 * max(h, w) of the float64 value (the largest difference seen
    is 3 * 2^-24 * 128, on 64 x 128).  A pixel that float64 puts closer than that to an integer can fall on either side in float32: both
    one-sided derivatives are right there, and ONE such pixel moves dL/dH by percents (an entry is a sum of h w terms of either sign).  Met
    on 64 x 128 with the seeded homography of check_warp_fwd_bwd: (x, y) = (126, 32) maps to u = 120.0000027 in float64 and to 119.9999924
    in the kernel's float32 arithmetic - the adjoint was 4.0e-2 of max |dL/dH| from float64, and so is the oracle's own float32 run (its one
    floor flip is that pixel) - while 128 x 64 and every other shape were within 3e-5.  A fraction ~4 * tie of the pixels.
    H [B,3,3] float64 -> (tie [B,h,w] bool, cov_tie [B,h,w] bool: the ties at a kink of the warped all-ones mask, u in {-1, 0, w-1, w} or
    v in {-1, 0, h-1, h})."""
    tie = 8 * 2.0 ** -24 * max(h, w)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    q = torch.einsum("bij,hwj->bhwi", H.detach(), torch.stack([xs, ys, torch.ones_like(xs)], -1))
    u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
    tu, tv = (u - u.round()).abs() < tie, (v - v.round()).abs() < tie
    edge = lambda t, n: sum((t.round() == k) for k in (-1, 0, n - 1, n)) > 0
    return tu | tv, (tu & edge(u, w)) | (tv & edge(v, h))


def check_warp_fwd_bwd(K, B, C, h, w, pool, delta=None, image=None, H64=None, oracle=None, base=None):
    """Forward, coverage and adjoint of one shape (images of h rows and w columns) against the oracle; returns (cov, gH, the arguments of
    warp_bwd) for further checks.  delta [B,4,2]: the corner offsets of the homographies (default: random, up to a quarter of the smaller extent).
    image: a function of the seeded image [B,C,h,w] (numpy) that returns the image to warp instead; H64 [B,9] float64 on the device: the
    homographies themselves, instead of those of `delta`; oracle(image, H): the reference warp in the dtype of `image` (default: O.warp_image)."""
    warp_image = oracle or O.warp_image
    size = h if h == w else 1000 * h + w             # (seeds)
    rng = np.random.Generator(np.random.PCG64(B * 100 + size))
    img = rng.standard_normal((B, C, h, w)).astype(np.float32)
    # smooth the image a little so that bilinear gradients are O(1)
    img = F.avg_pool2d(torch.tensor(img), 3, 1, 1).numpy()
    if image is not None:
        img = np.ascontiguousarray(image(img), dtype=np.float32)
    if H64 is None:
        if delta is None:
            delta = rand_delta(B, size, amp=min(h, w) / 4.0)
        H64, _ = K.h4pt_fwd(dev(delta), (w, h))
    out, cov = K.warp_fwd(dev(img), H64, pool)
    Ht = H64.cpu().reshape(B, 3, 3).clone().requires_grad_(True)
    imt = torch.tensor(img, dtype=torch.float64)
    ref = warp_image(imt, Ht)
    refcov = F.avg_pool2d(warp_image(torch.ones(B, 1, h, w, dtype=torch.float64), Ht), pool).squeeze(1)
    # north_star: "fp32 warp ... within 1e-4 relative".  The kernel evaluates the map in float32 (like grid_sample's float32 grid):
    # coordinate rounding ~ size * 2^-24 * few -> value error ~ 1e-5 * local gradient.  Bound: 1e-4 of the reference's range, or - where the
    # reference's OWN float32 chain (torch.inverse twice, normalise, grid_sample) is further than that from float64 - 1.5 x that spread.
    o, r64 = out.cpu().double().numpy(), ref.detach().numpy()
    ref32 = warp_image(torch.tensor(img), H64.cpu().reshape(B, 3, 3).float()).double().numpy()
    scale = np.abs(r64).max()
    err, spread = np.abs(o - r64).max(), np.abs(ref32 - r64).max()
    cerr = np.abs(cov.cpu().double().numpy() - refcov.detach().numpy()).max()
    print("MEASURED warp B%d C%d %dx%d pool%d: max|hip - f64| %.3e = %.2e of range; f32 oracle's own %.3e; coverage %.3e"
          % (B, C, h, w, pool, err, err / scale, spread, cerr))
    assert err <= max(1e-4 * scale, 1.5 * spread), (err, scale, spread)
    assert np.abs(o - ref32).max() <= 1e-4 * scale + 1.5 * spread
    assert cerr <= 2e-5
    go = rng.standard_normal(out.shape).astype(np.float32)
    gc = rng.standard_normal(cov.shape).astype(np.float32)
    # no output gradient where the derivative is not defined at float32 resolution (coordinate_ties; as the ReLU inputs within rounding of
    # zero in the BatchNorm tests): those pixels of the image, and the pooling windows with such a pixel on a kink of the coverage
    tie, cov_tie = coordinate_ties(Ht, h, w)
    go[np.broadcast_to(tie[:, None].numpy(), go.shape)] = 0
    gc[F.max_pool2d(cov_tie[:, None].float(), pool).squeeze(1).numpy() > 0] = 0
    print("MEASURED warp B%d C%d %dx%d pool%d: %d of %d pixels within float32 rounding of an integer source coordinate (%d on a coverage kink)"
          % (B, C, h, w, pool, int(tie.sum()), tie.numel(), int(cov_tie.sum())))
    ((ref * torch.tensor(go, dtype=torch.float64)).sum() + (refcov * torch.tensor(gc, dtype=torch.float64)).sum()).backward()
    bwd_args = (dev(img), H64, dev(go), dev(gc), pool)
    r = Ht.grad.numpy().reshape(B, 9)
    # (base: gH is a `+=` output - from a nonzero start, the start taken off again in float64)
    gH = K.warp_bwd(*bwd_args) if base is None else grad_result(base, K.warp_bwd(*bwd_args, gH=grad_start(base, r, torch.float64))).cuda()
    gerr = np.abs(gH.cpu().double().numpy() - r).max() / np.abs(r).max()
    print("MEASURED warp adjoint B%d C%d %dx%d pool%d: max error %.3e of max|dL/dH|" % (B, C, h, w, pool, gerr))
    assert gerr <= WARP_ADJOINT_BOUND, gerr
    # coverage-only entry
    cov2 = K.mask_coverage_fwd(H64, h, w, pool)
    if pool > 16 and not K.deterministic():
        # a default pool-32 call adds a window's four quarter sums with float atomics, in arrival order: three roundings of a sum <= 1 per
        # launch, 2^-25 each at the most - two launches differ by 3 * 2^-24 at the most (a deterministic call has one writer: equal)
        assert (cov2 - cov).abs().max().item() <= 3 * 2.0 ** -24
    else:
        assert torch.equal(cov2, cov)
    return cov, gH, bwd_args


# (2, 1, 64, 32): a 2 x 2 grid of pooling windows of four quarter tiles each; (3, 1, 48, 4): pool 4 on the generic kernels (width % 64 != 0)
@pytest.mark.parametrize("B,C,size,pool", [(5, 1, 128, 4), (2, 3, 64, 4), (3, 1, 32, 8), (2, 2, 48, 1), (1, 1, 256, 16),
                                           (2, 1, 64, 32), (2, 2, 32, 2), (3, 1, 48, 4)])
def test_warp_fwd_bwd(K, B, C, size, pool):
    check_warp_fwd_bwd(K, B, C, size, size, pool)


# rectangular images, each as h x w and as w x h.  48 x 64 / pool 4: the pool-4 kernels (w % 64 == 0) with one row per thread; 64 x 48: the generic
# kernels; 64 x 128: the pool-4 kernels with several rows per thread; 64 x 96 / pool 32: 2 x 3 pooling windows of four quarter tiles
RECT_WARP_CASES = [(2, 2, 48, 64, 4), (2, 1, 64, 128, 4), (2, 1, 32, 64, 8), (1, 1, 64, 128, 16), (2, 1, 64, 96, 32), (2, 2, 32, 48, 1), (2, 2, 32, 48, 2)]
RECT_WARP_CASES = RECT_WARP_CASES + [(B, C, w, h, pool) for (B, C, h, w, pool) in RECT_WARP_CASES]


@pytest.mark.parametrize("B,C,h,w,pool", RECT_WARP_CASES)
def test_warp_fwd_bwd_rectangular(K, B, C, h, w, pool):
    check_warp_fwd_bwd(K, B, C, h, w, pool)


def test_warp_fwd_bwd_pool32_deterministic(K):
    """The pool-32 case in deterministic mode: the one-writer coverage kernel and the single-writer adjoint grid meet the same bounds,
    and two calls give the same bits."""
    with K.det_scope(True):
        cov, gH, bwd_args = check_warp_fwd_bwd(K, 2, 1, 64, 64, 32)
        cov_again = K.warp_fwd(bwd_args[0], bwd_args[1], 32)[1]
        gH_again = K.warp_bwd(*bwd_args)
    assert torch.equal(cov_again, cov)
    assert torch.equal(gH_again, gH)


def test_warped_image_does_not_depend_on_the_pooling_size(K):
    """Every warp kernel takes its tap from one function (csrc/warp_tap.h): the pool-4 kernel and the generic kernel of every other pooling
    size write the same image bit for bit, and the coverage-only call the same coverage as the call with an image."""
    B, C, size = 2, 2, 64
    rng = np.random.Generator(np.random.PCG64(64))
    img = dev(rng.standard_normal((B, C, size, size)).astype(np.float32))
    delta = rand_delta(B, 64, amp=16)
    delta[1] += 40.0        # sample 1 is shifted by 24 ... 56 px: part of it samples outside the image
    H64, _ = K.h4pt_fwd(dev(delta), size)
    outs = {p: K.warp_fwd(img, H64, p) for p in (1, 2, 4, 8, 16, 32)}
    cov1 = outs[1][1]
    assert (cov1[0] > 1 - 1e-6).any() and (cov1[1] == 0).any() and ((cov1[1] > 0) & (cov1[1] < 1)).any()     # interior, outside and edge taps
    for p, (out, cov) in outs.items():
        assert torch.equal(out, outs[1][0]), p
    for p in (1, 4, 8):
        assert torch.equal(K.mask_coverage_fwd(H64, size, size, p), outs[p][1]), p


def test_warp_identity_and_consistency(K):
    """SURVEY 4(iii),(iv): identity H is the identity; delta_hat == delta_gt maps patch_1 onto patch_2."""
    d = synth.make_pairs(4, seed=21)
    p1, p2 = dev(d["patch_1"]), dev(d["patch_2"])
    H0, _ = K.h4pt_fwd(torch.zeros(4, 4, 2, device="cuda"), 128)
    out, cov = K.warp_fwd(p1, H0, 4)
    assert torch.equal(out, p1) and torch.all(cov == 1)
    Hg, _ = K.h4pt_fwd(dev(d["delta"]), 128)
    out, cov = K.warp_fwd(p1, Hg, 1)
    inside = cov.reshape(4, 1, 128, 128) == 1
    err = ((out - p2).abs() * inside).sum() / inside.sum()
    assert err.item() < 0.02, err.item()        # same convention => sub-interpolation-noise residual


# hw = 25 with C = 64 / 16: LP = 16 / 4 lanes per pixel, 4 / 16 pixels per wave pass, the last pass partly filled; C = 512: two float4 per lane
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("B,hf,C", [(5, 32, 64), (2, 8, 16), (3, 4, 256), (2, 16, 128), (2, 5, 64), (2, 5, 16), (2, 4, 512)])
def test_triplet_fwd_bwd(K, B, hf, C, masks, wf=None):
    wf = hf if wf is None else wf                    # (maps of hf x wf pixels: tests/shape_edges.py runs a prime pixel count)
    rng = np.random.Generator(np.random.PCG64(B + C))
    f = [rng.standard_normal((B, hf, wf, C)).astype(np.float32) for _ in range(4)]
    m1w = rng.uniform(0, 1, (B, hf, wf)).astype(np.float32)
    m2w = rng.uniform(0, 1, (B, hf, wf)).astype(np.float32)
    m1w[0] *= 1e-4                                   # force the max(den, 1) clamp branch on one sample
    m1, m2 = (rng.uniform(0, 1, (B, hf, wf)).astype(np.float32) for _ in range(2)) if masks else (None, None)      # content masks
    dm1, dm2 = (dev(m) if masks else None for m in (m1, m2))
    dl = rand_delta(B, 5, 8)
    H1, _ = K.h4pt_fwd(dev(dl), 128)
    H2, _ = K.h4pt_fwd(dev(-dl[::-1].copy()), 128)
    mu = 0.01
    M1, M2, nd = K.triplet_l1_fwd(*[dev(a) for a in f], dev(m1w), dev(m2w), dm1, dm2)
    loss4 = K.bihome_loss_fwd(nd, H1, H2, mu)
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    f1, f2, f1w, f2w = [T(a).requires_grad_(True) for a in f]
    a1, a2 = T(m1w).requires_grad_(True), T(m2w).requires_grad_(True)
    h1 = H1.cpu().reshape(B, 3, 3).clone().requires_grad_(True)
    h2 = H2.cpu().reshape(B, 3, 3).clone().requires_grad_(True)
    l1, l2, l3 = (f1w - f2).abs().sum(-1), (f2w - f1).abs().sum(-1), (f1 - f2).abs().sum(-1)
    w1, w2 = (a1 * T(m2), a2 * T(m1)) if masks else (a1, a2)          # line 1 is weighted by m1w * m2, line 2 by m2w * m1
    d1, d2 = w1.sum((-1, -2)), w2.sum((-1, -2))
    ln1 = ((w1 * (l1 - l3)).sum((-1, -2)) / torch.max(d1, torch.ones_like(d1))).sum()
    ln2 = ((w2 * (l2 - l3)).sum((-1, -2)) / torch.max(d2, torch.ones_like(d2))).sum()
    ln3 = ((h1 @ h2 - torch.eye(3, dtype=torch.float64)) ** 2).sum()
    loss = ln1 + ln2 + mu * ln3
    np.testing.assert_allclose(loss4.cpu().numpy(), [loss.item(), ln1.item(), ln2.item(), ln3.item()], rtol=2e-5)
    np.testing.assert_allclose(M1.cpu().numpy(), (l1 - l3).detach().numpy(), rtol=1e-4, atol=1e-4)
    (loss * 0.7).backward()
    g = torch.tensor([0.7], device="cuda")
    gf1w, gf2w, gm1w, gm2w, gH1, gH2 = K.bihome_loss_bwd(g, *[dev(a) for a in f], dev(m1w), dev(m2w), dm1, dm2, M1, M2,
                                                         nd, H1, H2, mu)
    np.testing.assert_allclose(gf1w.cpu().numpy(), f1w.grad.numpy(), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(gf2w.cpu().numpy(), f2w.grad.numpy(), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(gm1w.cpu().numpy(), a1.grad.numpy(), rtol=2e-4, atol=1e-4 * a1.grad.abs().max().item())
    np.testing.assert_allclose(gm2w.cpu().numpy(), a2.grad.numpy(), rtol=2e-4, atol=1e-4 * a2.grad.abs().max().item())
    np.testing.assert_allclose(gH1.cpu().numpy().reshape(B, 3, 3), h1.grad.numpy(), rtol=1e-6, atol=1e-10)   # g and mu are float32 scalars
    np.testing.assert_allclose(gH2.cpu().numpy().reshape(B, 3, 3), h2.grad.numpy(), rtol=1e-6, atol=1e-10)


def test_head_chain_against_golden(K, golden):
    """DLT -> corners -> 4pt -> warp + coverage on the head-only golden scenario (reference outputs)."""
    g = golden("head_b8_f32")
    d = synth.make_head_inputs(8, 7)
    for tag, src in (("12", "patch_1"), ("21", "patch_2")):
        pf = dev(d["pf_hat_" + tag])
        choice = torch.tensor(g["choice_" + tag]).cuda()
        Hd, dh, _ = K.dlt_fwd(pf, choice, 1, 128)
        np.testing.assert_allclose(dh.cpu().numpy(), g["delta_hat_" + tag], atol=2e-3)
        H64, H32 = K.h4pt_fwd(dh, 128)
        np.testing.assert_allclose(H32.cpu().numpy(), g["H_4pt_" + tag], rtol=1e-4, atol=2e-5)
        out, cov = K.warp_fwd(dev(d[src]), H64, 4)
        np.testing.assert_allclose(out.cpu().numpy()[..., ::4, ::4], g["warp_sub_" + tag], atol=2e-3)
        np.testing.assert_allclose(cov.cpu().numpy(), g["mask_pooled_" + tag], atol=2e-4)


def test_gpu_pair_generator_matches_host_generator(K):
    """bh_synth_pairs against the numpy generator (bihome_amd/synth.py) on the same image, position and delta."""
    from bihome_amd.synth_gpu import GpuPairGenerator
    gen = GpuPairGenerator(n_images=3, seed=5)
    idx, origin, delta, _ = gen.draw(6)
    out = gen.make(idx, origin, delta)
    imgs = gen.images.cpu().numpy()
    c = np.array([[0, 0], [128, 0], [128, 128], [0, 128]], np.float64)
    for b in range(6):
        img = imgs[int(idx[b])].transpose(1, 2, 0).astype(np.float64)
        x0, y0 = int(origin[b, 0]), int(origin[b, 1])
        H = synth.four_point_homography(c, c + delta[b].cpu().numpy().astype(np.float64))
        T = np.array([[1, 0, x0], [0, 1, y0], [0, 0, 1.0]])
        crop2 = synth.warp_bilinear(img, T @ H, 128, 128)
        crop1 = img[y0:y0 + 128, x0:x0 + 128]
        for got, crop in ((out["patch_1"][b, 0], crop1), (out["patch_2"][b, 0], crop2)):
            g = crop[..., 0] * 0.299 + crop[..., 1] * 0.587 + crop[..., 2] * 0.114
            ref = (g / 255 - 0.443) / 0.129
            np.testing.assert_allclose(got.cpu().numpy(), ref, atol=2e-3)
    assert delta.min() >= -32 and delta.max() <= 31 and origin[:, 0].min() >= 32
    # pds-coco: the full PhotometricDistortSimple (brightness, contrast before / after, HSV saturation and hue, channel
    # permutation) on the device against synth.apply_photometric - which tests/test_datagen_cpu.py pins against the
    # reference's own transforms.py classes - on the same parameter records, images, positions and offsets
    gen2 = GpuPairGenerator(n_images=2, seed=6, photometric_max_delta=32)
    idx, origin, delta, photo = gen2.draw(12)
    assert photo.shape == (12, 12)
    o2 = gen2.make(idx, origin, delta, photo)
    imgs = gen2.images.cpu().numpy()
    rec = photo.cpu().numpy().astype(np.float64)
    assert (rec[:, 5] > 0).any() and (rec[:, 3] != 0).any() and (rec[:, 2] != 1).any() and (rec[:, [1, 4]] != 1).any()
    for b in range(12):
        img = imgs[int(idx[b])].transpose(1, 2, 0)
        x0, y0 = int(origin[b, 0]), int(origin[b, 1])
        H = synth.four_point_homography(c, c + delta[b].cpu().numpy().astype(np.float64))
        T = np.array([[1, 0, x0], [0, 1, y0], [0, 0, 1.0]])
        im1 = synth.apply_photometric(img, rec[b, :6]).astype(np.float64)
        im2 = synth.apply_photometric(img, rec[b, 6:]).astype(np.float64)
        ref1 = synth.gray_standardize(im1[y0:y0 + 128, x0:x0 + 128])[0]
        ref2 = synth.gray_standardize(synth.warp_bilinear(im2, T @ H, 128, 128))[0]
        np.testing.assert_allclose(o2["patch_1"][b, 0].cpu().numpy(), ref1, atol=3e-3)
        np.testing.assert_allclose(o2["patch_2"][b, 0].cpu().numpy(), ref2, atol=3e-3)


def test_gpu_pair_generator_matches_reference_fixture(K, golden):
    """bh_synth_pairs DIRECTLY against the outputs of the reference's own HomographyNetPrep + PhotometricDistortSimple +
    DictToGrayscale + DictStandardize (tests/golden/datagen_ref.npz: `p1_std` / `p2_std`, every 4th pixel), not through the host
    generator: the image is regenerated from the fixture's seed, position and corner offsets are the fixture's `corners` /
    `delta`, the photometric records are the reference-order draws of the sample's RandomState (round-2 VERDICT weak #4)."""
    import ctypes
    from bihome_amd._lib import check, lib
    g = golden("datagen_ref")
    rng = np.random.Generator(np.random.PCG64(int(g["prep_image_seed"])))
    image = np.clip(synth.texture_image(rng, 240, 320), 0, 255).astype(np.uint8)
    images = torch.tensor(image.transpose(2, 0, 1)[None].astype(np.float32)).cuda().contiguous()
    pv = ctypes.c_void_p
    worst = 0.0
    for md in (0, 32):
        k = "prep_md%d_" % md
        corners, delta = g[k + "corners"], g[k + "delta"]
        B = corners.shape[0]
        recs = []
        for seed in range(B):
            rs = np.random.RandomState(seed)                 # transforms.py:451-454: the distortion draws come first
            recs.append(np.concatenate([synth.draw_photometric(rs, md), synth.draw_photometric(rs, md)]))
        photo = torch.tensor(np.stack(recs), dtype=torch.float32).cuda().contiguous()
        idx = torch.zeros(B, dtype=torch.int32, device="cuda")
        origin = torch.tensor(corners[:, 0, :].astype(np.float32)).cuda().contiguous()
        dl = torch.tensor(delta.astype(np.float32)).cuda().contiguous()
        H64, _ = K.h4pt_fwd(dl, 128)
        p1 = torch.empty(B, 1, 128, 128, device="cuda")
        p2 = torch.empty_like(p1)
        check(lib.bh_synth_pairs(pv(images.data_ptr()), pv(idx.data_ptr()), pv(origin.data_ptr()), pv(H64.data_ptr()),
                                 pv(photo.data_ptr()), B, 1, 240, 320, 128, 0.443, 0.129, pv(p1.data_ptr()), pv(p2.data_ptr()),
                                 pv(torch.cuda.current_stream().cuda_stream)), "bh_synth_pairs")
        a1, a2 = p1[:, 0, ::4, ::4].cpu().numpy(), p2[:, 0, ::4, ::4].cpu().numpy()
        worst = max(worst, np.abs(a1 - g[k + "p1_std"]).max(), np.abs(a2 - g[k + "p2_std"]).max())
        np.testing.assert_allclose(a1, g[k + "p1_std"], atol=3e-3, err_msg="patch_1 md %d" % md)
        np.testing.assert_allclose(a2, g[k + "p2_std"], atol=3e-3, err_msg="patch_2 md %d" % md)
    print("bh_synth_pairs vs reference fixture: max abs difference %.2e (standardised units)" % worst)


ACTIVE_MARGINS = (36.0, 9.0, 290.0)        # chosen per shape so that the hinge is active at 20 - 80 % of the pixels (asserted below)


@pytest.mark.parametrize("B,hf,C,margin", [(3, 32, 64, 1.0), (2, 8, 128, 0.0), (1, 16, 64, 25.0),
                                           (2, 5, 64, 36.0), (2, 5, 16, 9.0), (2, 4, 512, 290.0)])
def test_oneline_hinge_loss_fwd_bwd(B, hf, C, margin, wf=None):
    """bh_oneline_loss_fwd/bwd (iHomE, PerceptualHead.py:474-538) against torch float64 autograd of the same formula.  The first three
    parameter sets leave the hinge (almost) everywhere inactive; the last three have both states and partly filled wave passes."""
    import torch.nn.functional as F
    from bihome_amd import kernels as K
    wf = hf if wf is None else wf                          # (maps of hf x wf pixels: tests/shape_edges.py)
    g = torch.Generator().manual_seed(B * 7 + hf)
    f1, f2 = torch.randn(B, hf, wf, C, generator=g), torch.randn(B, hf, wf, C, generator=g)
    f1w = (f2 + 0.7 * torch.randn(B, hf, wf, C, generator=g))
    m1w = torch.rand(B, hf, wf, generator=g)
    m1w[0, :2] = 0
    if B > 1:
        m1w[1] *= 1e-4                                     # denominator below 1: max(den, 1) branch
    a, b, c, m = (t.double().requires_grad_(rq) for t, rq in ((f1, False), (f2, False), (f1w, True), (m1w, True)))
    t = (c - b).abs().sum(-1) - (a - b).abs().sum(-1) + margin
    den = m.sum((-1, -2))
    ref = ((m * torch.clamp(t, min=0)).sum((-1, -2)) / torch.max(den, torch.ones_like(den))).sum()
    ref.backward()
    if margin in ACTIVE_MARGINS:
        assert 0.2 < (t > 0).double().mean().item() < 0.8
    loss, T, numden, per = K.oneline_loss_fwd(f1.cuda(), f2.cuda(), f1w.cuda(), m1w.cuda(), margin)
    assert abs(loss.item() - ref.item()) <= 2e-5 * abs(ref.item()) + 1e-6
    gf, gm = K.oneline_loss_bwd(torch.ones(1, device="cuda"), f2.cuda(), f1w.cuda(), m1w.cuda(), T, numden)
    assert (gf.cpu().double() - c.grad).abs().max().item() <= 2e-5 * c.grad.abs().max().item() + 1e-7
    assert (gm.cpu().double() - m.grad).abs().max().item() <= 2e-4 * m.grad.abs().max().item() + 1e-6


def test_dsac_scores_fwd_bwd_vs_torch64():
    """bh_dsac_score + bh_dsac_scores_fwd / _bwd (softmax(-reprojection error) and its adjoint w.r.t. the field and the
    hypotheses' homographies) against torch float64 autograd of ransac_utils.py:76-128."""
    from bihome_amd import kernels as K
    B, n, h = 3, 4, 32
    g = torch.Generator().manual_seed(4)
    pf = torch.randn(B, 2, h, h, generator=g) * 2.0
    Hd = torch.eye(3).repeat(B * n, 1, 1) + 0.01 * torch.randn(B * n, 3, 3, generator=g)
    Hd[:, 2, :2] *= 0.01
    gs = torch.randn(B, n, generator=g)
    pf64, H64 = pf.double().requires_grad_(True), Hd.double().requires_grad_(True)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(h, dtype=torch.float64), indexing="ij")
    coord = torch.stack([xs.reshape(-1), ys.reshape(-1)], -1)
    mapf = coord[None] + pf64.reshape(B, 2, -1).permute(0, 2, 1)
    ph = torch.cat([coord, torch.ones_like(coord[:, :1])], -1)
    q = torch.einsum("bnij,pj->bnpi", H64.reshape(B, n, 3, 3), ph)
    t = q[..., :2] / q[..., 2:3]
    err = (t - mapf[:, None]).abs().sum(-1).sum(-1)
    scores = torch.softmax(-err, -1)
    (scores * gs.double()).sum().backward()
    s, e = K.dsac_scores_fwd(pf.cuda(), Hd.reshape(-1, 9).cuda().contiguous(), n)
    assert (e.cpu().double() - err.detach()).abs().max() <= 1e-5 * err.detach().abs().max()
    assert (s.cpu().double() - scores.detach()).abs().max() < 2e-4
    g_pf, g_H = K.dsac_scores_bwd(pf.cuda(), Hd.reshape(-1, 9).cuda().contiguous(), s, gs.cuda().contiguous(), n)
    rp, rh = pf64.grad, H64.grad.reshape(-1, 9)
    assert (g_pf.cpu().double() - rp).abs().max() <= 2e-3 * rp.abs().max() + 1e-9
    assert (g_H.cpu() - rh).abs().max() <= 2e-3 * rh.abs().max() + 1e-9


def test_scale_samples_and_scored_hinge_vs_torch64(hf=8, C=64, margins=(1.0, 36.0)):
    """bh_scale_samples_fwd/bwd (rep = 1 with g_x, rep = 3 without) and the multi-hypothesis form of the one-line loss
    (rep = 3, per-hypothesis scores) against torch float64 autograd.  (hf, C: L = hf hf C floats per sample; margins: of the scored hinge.)"""
    from bihome_amd import kernels as K
    g = torch.Generator().manual_seed(9)
    B, n = 2, 3
    x1 = torch.randn(B * n, hf, hf, C, generator=g)
    x2 = torch.randn(B, hf, hf, C, generator=g)
    s = torch.rand(B * n, generator=g) + 0.1
    gy = torch.randn(B * n, hf, hf, C, generator=g)
    for x, rep in ((x1, 1), (x2, n)):
        xd, sd = x.double().requires_grad_(True), s.double().requires_grad_(True)
        y = xd.repeat_interleave(rep, 0) * sd.view(-1, 1, 1, 1)
        (y * gy.double()).sum().backward()
        yk = K.scale_samples_fwd(x.cuda(), s.cuda(), rep)
        assert (yk.cpu().double() - y.detach()).abs().max() < 1e-6
        gx, gs = K.scale_samples_bwd(gy.cuda(), x.cuda(), s.cuda(), rep, rep == 1)
        assert (gs.cpu().double() - sd.grad).abs().max() <= 1e-5 * sd.grad.abs().max()
        if rep == 1:
            assert (gx.cpu().double() - xd.grad).abs().max() < 1e-6
    # scored hinge
    f1, f2 = torch.randn(B, hf, hf, C, generator=g), torch.randn(B, hf, hf, C, generator=g)
    f1w = f2.repeat_interleave(n, 0) + 0.7 * torch.randn(B * n, hf, hf, C, generator=g)
    m1w = torch.rand(B * n, hf, hf, generator=g)
    for margin in margins:                    # 36: the hinge is active at about half of the pixels (1: almost nowhere)
        a, b, c, m, sc = (t.double().requires_grad_(rq) for t, rq in ((f1, False), (f2, False), (f1w, True), (m1w, True), (s, True)))
        t = (c - b.repeat_interleave(n, 0)).abs().sum(-1) - (a - b).abs().sum(-1).repeat_interleave(n, 0) + margin
        if margin > 1.0:
            assert 0.2 < (t > 0).double().mean().item() < 0.8
        den = m.sum((-1, -2))
        per = (m * torch.clamp(t, min=0)).sum((-1, -2)) / torch.max(den, torch.ones_like(den))
        ref = (per * sc).sum()
        ref.backward()
        loss, T, numden, perk = K.oneline_loss_fwd(f1.cuda(), f2.cuda(), f1w.cuda(), m1w.cuda(), margin, rep=n, sample_w=s.cuda())
        assert abs(loss.item() - ref.item()) <= 2e-5 * abs(ref.item())
        assert (perk.cpu().double() - per.detach()).abs().max() <= 2e-5 * per.detach().abs().max()
        gf, gm = K.oneline_loss_bwd(torch.ones(1, device="cuda"), f2.cuda(), f1w.cuda(), m1w.cuda(), T, numden, rep=n, sample_w=s.cuda())
        assert (gf.cpu().double() - c.grad).abs().max() <= 2e-5 * c.grad.abs().max() + 1e-8
        assert (gm.cpu().double() - m.grad).abs().max() <= 2e-4 * m.grad.abs().max() + 1e-7


def check_stem_dgrad_with_the_warp_adjoint_folded_in(K, B, h, w, pool, with_cov, prec):
    """Round 6 (bh_stem7_dgrad_c1_warp, include/bihome.h): the extractor stem's dgrad that applies the warp's adjoint to the gradient it has
    just made, against the two calls it replaces - bh_stem7_dgrad_c1, then bh_warp_bwd on its output: the gradient image (when asked for)
    bit for bit, dL/dH to float rounding of the per-pixel products (same taps bitwise: warp_tap.h)."""
    import ctypes
    from bihome_amd._lib import lib, check
    size = h if h == w else 1000 * h + w            # (seeds)
    rng = np.random.Generator(np.random.PCG64(B * 7 + size))
    src = F.avg_pool2d(torch.tensor(rng.standard_normal((B, 1, h, w)).astype(np.float32)), 3, 1, 1).cuda().contiguous()
    gy = torch.tensor(rng.standard_normal((B, h // 2, w // 2, 64)).astype(np.float32)).cuda()
    wt = torch.tensor((rng.standard_normal((64, 7, 7, 1)) * 0.05).astype(np.float32)).cuda()
    gcov = torch.tensor(rng.standard_normal((B, h // pool, w // pool)).astype(np.float32)).cuda() if with_cov else None
    H64, _ = K.h4pt_fwd(dev(rand_delta(B, size + 1, amp=min(h, w) / 4.0)), (w, h))
    d = K.conv_desc(B, h, w, 1, 64, 7, 2, 3, precision=prec)     # (4: the window GEMM in fp16 pieces - both entry points, the same tiles)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gx0 = torch.empty(B, h, w, 1, device="cuda")
    check(lib.bh_stem7_dgrad_c1(p(gy), p(wt), p(gx0), ctypes.byref(d), stream), "bh_stem7_dgrad_c1")
    base = torch.tensor(rng.standard_normal((B, 9))).cuda()          # gH accumulates: something is there already (ln3's gradient in the step)
    gH0 = K.warp_bwd(src, H64, gx0.view(B, 1, h, w), gcov, pool, gH=base.clone())
    for want_gx in (True, False):
        gx1 = torch.full((B, h, w, 1), float("nan"), device="cuda") if want_gx else None
        gH1 = base.clone()
        check(lib.bh_stem7_dgrad_c1_warp(p(gy), p(wt), p(gx1), ctypes.byref(d), p(src), p(H64), p(gcov), pool, p(gH1), stream), "bh_stem7_dgrad_c1_warp")
        if want_gx:
            assert torch.equal(gx1, gx0)
        scale = (gH0 - base).abs().max().item()
        err = (gH1 - gH0).abs().max().item()
        print("MEASURED fused stem dgrad + warp adjoint B%d %dx%d pool%d: max |gH - two calls| %.3e of %.3e" % (B, h, w, pool, err, scale))
        # (same taps bit for bit - warp_tap.h spells the coordinates as fused multiply-adds in one order; what differs is the compiler's
        #  contraction of the per-pixel float products and the order of the double sums: ~1e-7 of the sum of |terms|, and the entries are
        #  the near-cancelling sums of 16 k random-sign terms)
        assert err <= 1e-5 * scale, (err, scale)
    # (the two calls are held against the float64 oracle by test_warp_fwd_bwd; a direct comparison on THESE inputs would measure how many
    #  pixels float32 coordinates put on the other side of an integer - the bilinear derivative jumps there - not the kernel)
    # geometries the kernel does not take are refused, not guessed
    d2 = K.conv_desc(B, h, w, 1, 64, 7, 2, 3, precision=prec)
    assert lib.bh_stem7_dgrad_c1_warp(p(gy), p(wt), None, ctypes.byref(d2), p(src), p(H64), p(gcov), 3, p(gH1), stream) == -2


@pytest.mark.parametrize("prec", [0, 4])
@pytest.mark.parametrize("B,size,pool,with_cov", [(6, 128, 4, True), (3, 64, 4, True), (5, 128, 8, True), (4, 32, 4, False), (2, 256, 16, True),
                                                 (16, 128, 4, True), (40, 128, 4, True), (130, 64, 4, True)])     # (the last three: several tiles per workgroup)
def test_stem_dgrad_with_the_warp_adjoint_folded_in(K, B, size, pool, with_cov, prec):
    check_stem_dgrad_with_the_warp_adjoint_folded_in(K, B, size, size, pool, with_cov, prec)


def check_stem_forward_with_the_warp_folded_in(K, B, h, w, groups, with_cov, with_img, det):
    """Round 6 (bh_stem7_fwd_warp, include/bihome.h): the extractor's one-plane stem that makes the warped pixels while it fetches its
    patches, against the two calls it replaces - bh_warp_fwd, then bh_conv_fwd_bnstats on its output.  Same taps, same blend, the same
    pixels into the same arithmetic: the warped image, the pooled coverage and the stem's output bit for bit; the BatchNorm sums to the
    order of the f64 atomics (bitwise in deterministic calls)."""
    import ctypes
    from bihome_amd._lib import lib, check
    size = h if h == w else 1000 * h + w            # (seeds)
    rng = np.random.Generator(np.random.PCG64(B * 11 + size))
    src = F.avg_pool2d(torch.tensor(rng.standard_normal((B, 1, h, w)).astype(np.float32)), 3, 1, 1).cuda().contiguous()
    wt = torch.tensor((rng.standard_normal((64, 7, 7, 1)) * 0.05).astype(np.float32)).cuda()
    H64, _ = K.h4pt_fwd(dev(rand_delta(B, size + 1, amp=min(h, w) / 4.0)), (w, h))
    H64[B // 2] = torch.tensor([1., 0, 3 * w, 0, 1, 0, 0, 0, 1], dtype=torch.float64)      # one image warped entirely out of its source
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    with K.det_scope(det):
        d = K.conv_desc(B, h, w, 1, 64, 7, 2, 3, precision=4)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        warped0, cov0 = K.warp_fwd(src, H64, 4)
        s0 = K.bn_stats_buffer(groups, 64, "cuda")
        y0 = K.conv_fwd(warped0.view(B, h, w, 1), wt, None, d, bn_sums=s0, groups=groups)
        assert K.conv_variant(d, "fwd", bn_groups=groups) == "stem7_fwd_f16_kernel<1>"
        s1 = K.bn_stats_buffer(groups, 64, "cuda")
        y1 = torch.full_like(y0, float("nan"))
        warped1 = torch.full_like(warped0, float("nan")) if with_img else None
        cov1 = torch.full_like(cov0, float("nan")) if with_cov else None
        check(lib.bh_stem7_fwd_warp(p(src), p(H64), 4, p(wt), None, p(y1), ctypes.byref(d), p(warped1), p(cov1), p(s1), groups, stream),
              "bh_stem7_fwd_warp")
        if with_img:
            assert torch.equal(warped1, warped0)
        if with_cov:
            assert torch.equal(cov1, cov0)
        assert torch.equal(y1, y0)
        assert warped0[B // 2].abs().max().item() == 0.0 and (y1[B // 2] == 0).all()
        if det:
            assert torch.equal(s1.view(torch.int64), s0.view(torch.int64))      # (integer limbs: compared as bit patterns)
        else:
            assert (s1 - s0).abs().max().item() <= 1e-9 * s0.abs().max().item()
        # through kernels.conv_fwd (what the Runner calls): the input buffer is filled on the way
        x2 = torch.full((B, h, w, 1), float("nan"), device="cuda")
        cov2 = torch.full_like(cov0, float("nan"))
        source = dict(src=src, H64=H64, pool=4, cov=cov2, done=False, filled=False)
        y2 = K.conv_fwd(x2, wt, None, d, bn_sums=K.bn_stats_buffer(groups, 64, "cuda"), groups=groups, warp_src=source)
        assert source["done"] and source["filled"]
        assert torch.equal(y2, y0) and torch.equal(x2.view_as(warped0), warped0) and torch.equal(cov2, cov0)
        # ... and where the fused kernel does not apply (fp32-input MFMA stem; pool 8) the two calls are made inside
        for prec, pool in ((0, 4), (4, 8)):
            dd = K.conv_desc(B, h, w, 1, 64, 7, 2, 3, precision=prec)
            x3 = torch.full((B, h, w, 1), float("nan"), device="cuda")
            cov3 = torch.full((B, h // pool, w // pool), float("nan"), device="cuda")
            source = dict(src=src, H64=H64, pool=pool, cov=cov3, done=False, filled=False)
            y3 = K.conv_fwd(x3, wt, None, dd, bn_sums=K.bn_stats_buffer(groups, 64, "cuda"), groups=groups, warp_src=source)
            assert source["filled"] and not source["done"]
            wref, cref = K.warp_fwd(src, H64, pool)
            assert torch.equal(x3.view_as(wref), wref) and torch.equal(cov3, cref)
            yref = K.conv_fwd(wref.view(B, h, w, 1), wt, None, dd, bn_sums=K.bn_stats_buffer(groups, 64, "cuda"), groups=groups)
            assert torch.equal(y3, yref)
        assert lib.bh_stem7_fwd_warp(p(src), p(H64), 8, p(wt), None, p(y1), ctypes.byref(d), None, None, None, 1, stream) == -2


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("B,size,groups,with_cov,with_img", [(4, 128, 2, True, True), (16, 64, 1, True, True), (40, 128, 2, True, False),
                                                             (130, 64, 2, False, True), (6, 256, 1, True, True)])
def test_stem_forward_with_the_warp_folded_in(K, B, size, groups, with_cov, with_img, det):
    check_stem_forward_with_the_warp_folded_in(K, B, size, size, groups, with_cov, with_img, det)


def test_extractor_of_warp_keeps_the_image_only_on_request(K):
    """heads/PerceptualHead._extractor_of_warp (round 6): with the warp made inside the extractor stem's forward nobody reads the warped
    patches - they are written only when `AuxiliaryResnet.keep_warped` asks for them; coverage and features are the same either way and
    equal those of the two separate calls (BIHOME_WARP_IN_STEM_FWD=0 at the kernel level: kernels.conv_fwd without warp_src)."""
    from bihome_amd.heads import PerceptualHead as PH
    torch.manual_seed(3)
    aux = PH.AuxiliaryResnet(AUXILIARY_RESNET_OUTPUT_LAYER=1).cuda().train()
    B, size = 8, 128
    src = torch.rand(B, 1, size, size, device="cuda")
    H64, _ = K.h4pt_fwd(dev(rand_delta(B, size + 1, amp=size / 4.0)), size)
    warped0, cov0 = K.warp_fwd(src, H64, aux.stride)
    with torch.no_grad():
        feat0 = aux(warped0, groups=2)
    for keep in (False, True):
        aux.keep_warped = keep
        warped, cov, wl, featw = PH._extractor_of_warp(aux, src, H64, aux.stride, groups=2)
        assert torch.equal(cov, cov0) and torch.equal(featw.detach(), feat0)
        assert featw.requires_grad and wl.requires_grad
        if keep:
            assert torch.equal(warped, warped0)
        else:
            assert warped is None
    # three-channel patches take the two calls
    src3 = torch.rand(4, 3, size, size, device="cuda")
    H3, _ = K.h4pt_fwd(dev(rand_delta(4, size + 1, amp=size / 4.0)), size)
    warped, cov, wl, featw = PH._extractor_of_warp(aux, src3, H3, aux.stride, groups=1)
    w3, c3 = K.warp_fwd(src3, H3, aux.stride)
    assert torch.equal(warped, w3) and torch.equal(cov, c3)
