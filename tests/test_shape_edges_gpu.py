"""Every entry point at the edges of the shapes it accepts (the tables: tests/shape_edges.py; what holds them together without a GPU:
tests/test_shape_edges_cpu.py).

1. Accepted edges: the family's own float64 comparison - the helper of the family's test file, its reference, its tolerance - at the
   smallest / largest shape the accept-condition in csrc/ admits, with bihome_amd/kernels.py (and the helper's module) allocating through
   tests/poisoned_alloc.py: an overrun at an edge shape lands in a red zone.  `pytest -s` prints the largest normalised error of every conv /
   BatchNorm case next to the helper's tolerance (MEASURED lines, from ERRORS of test_conv_kernels_gpu.py).
2. Refusals: one raw call just outside every boundary the entry point checks before any launch - the return code the header documents,
   every buffer (inputs, outputs, scratch: poisoned beforehand) bit-identical afterwards, and through the wrapper of kernels.py a
   BihomeLibError that names the code.  Empty batches: BH_OK and nothing written but what the source says (a zero loss).

FOUND HERE: BatchNorm over TWO rows per group missed the helpers' tolerances on the MI355X - gx 1.6e-4 / 6.6e-4 of max |gx| from float64
against test_batchnorm_fwd_bwd's 5e-5, the two-branch join's output 8.2e-6 against test_two_branch_batchnorm_join's 2e-6.  Over two rows
the exact input gradient is (g1 - g2) / 2 * eps / (var + eps), the 1e-6 residue of a cancellation between terms of order 1, and fp32
holds one rounding of g of it; a few rows also make var << mean^2 - a large scale, whose product with the rounded mean is the forward's
error - an ordinary channel.  Groups of at most four rows now take bh_bn_bwd, bh_bn_join_fwd and bh_bn_join_bwd / _remask in double
(bn.hip BN_SMALL_ROWS): the same cases measure 9.6e-7 (2e-5) and 3.2e-8 (2e-6); rows = 3, 4 and 5 stand on both sides of the switch.

MEASURED at the edges (largest error of every family next to its helper's tolerance, `pytest -s`): generic / halo / persistent convs 1.4e-6
(3e-5), bf16 operands 3.6e-3 (1e-2), 4 x 4 fp16 pieces 9.9e-7 (2e-5), BatchNorm 9.6e-7 (2e-5), one-row BatchNorm 0.12 of
the header's derived bound, BatchNorm from the 1x1 dgrad 1.9e-7 (5e-6), one-channel BatchNorm 2.4e-8 (5e-5), fused tail 1.1e-7 (1e-6),
max pool 7.9e-8 (1e-6), GAP 1.2e-7 (1e-6), DLT at P = 4 ... 512 |delta_hat - f64| 3.4e-6 px (2e-5), warp 4.8e-6 of the range (1e-4), its
adjoint 2.3e-6 (1e-4), photometric warp 1.4e-6 (1e-4), warp adjoint w.r.t. the image 2.0e-6 (1e-4), RGB patches 4.7e-6 (3e-3).

Thresholds with tests of their own (section 3 below): bh_stem7_fwd_warp at 256 / 255 tiles; the packed kernels - the persistent 3x3 among
them - at the halo kernels' grid minimum WITHOUT BH_ROUTE_HALO_SMALL and one sub-tile pair below it; the split-operand weight gradient,
which has no grid minimum (wgrad_x3.hip:420-424), on one tile and on the maps / channel counts next to it that it does not take.
Groups of at most four rows in the fused BatchNorm forms (bh_bn_maxpool_fwd / _bwd, bh_bn_bwd_from_1x1) are REFUSED (narrowed: no config
of configs.py has a BatchNorm group of four rows; the unfused calls evaluate them in double); the sums-ready form of bh_bn_bwd takes the
double evaluation.  Not run: C = 4 and hw = 1 through the cosine, per-channel-hinge and anchor-adjoint helpers (their inputs place zero
vectors and ties at fixed pixels and assert hinge statistics that four channels or one pixel cannot have; triplet, one-line and l2norm run both).

Refusal sites of csrc/ that no case here reaches, and why:
  - the descriptor checks of the conv family (conv_gemm.hip check_desc, conv3x3.hip:822-835, wgrad.hip:805-815, pointwise.hip, stem7.hip
    bh_stem7_try): a shape the dedicated kernel does not take is not refused, it routes to the generic kernel - pinned by
    test_shape_edges_cpu.py through bh_conv_variant; the refusals of packed / BatchNorm-on-load launches (BH_E_UNSUPPORTED where the halo
    kernel does not take them) are held by test_c_abi_error_codes and test_conv3x3_f32x3_layout_and_precision_must_agree;
  - `B > 65535` / `h * w > 2^30` limits of the geometry and warp files beyond the two cases below: they need nothing but the scalar, and are
    of one form;
  - NULL pointers of the descriptor-taking conv entry points: the raw-call tables assemble scalar and plain-pointer arguments only;
    test_c_abi_error_codes and test_workspace_one_byte_short hold the conv family's pre-launch returns;
  - sites behind a launch (hipError_t returns of BH_LAUNCH_CHECK, hipMemsetAsync failures): not argument checks;
  - bn1.hip:195 (flags bit4 with C == 1) and tail.hip use_running without running statistics: internal arms behind the shape check that
    the tables reach with the shape itself."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import poisoned_alloc
import shape_edges as S
import test_conv_kernels_gpu as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from bihome_amd import kernels
    return kernels


@pytest.fixture(autouse=True)
def report_largest_error(request):
    try:                                                 # a fault of an earlier test is sticky: nothing more is started on the device
        torch.cuda.synchronize()
    except Exception as e:
        pytest.exit("the device reports an error left by an earlier test (%s): stopping" % e, returncode=3)
    del C.ERRORS[:]
    yield
    if C.ERRORS:
        err, tol = max(C.ERRORS, key=lambda e: e[0] / e[1])
        print("\nMEASURED %s: largest normalised error of %d comparisons %.3e (bound %.1e)" % (request.node.name, len(C.ERRORS), err, tol))


def run_poisoned(K, monkeypatch, module, fn, args, extra=()):
    """The helper `fn` of `module` on `args` with every torch.empty of kernels.py, of the helper's module and of `extra` poisoned and
    fenced; the red zones are verified afterwards."""
    mod = importlib.import_module(module)
    p = poisoned_alloc.poison(monkeypatch, K, mod, *[importlib.import_module(m) for m in extra if m != module])
    monkeypatch.setattr(K, "_STEM_WGRAD_WS", {})
    call = getattr(mod, fn)
    if call.__code__.co_varnames[:call.__code__.co_argcount][:1] == ("K",):
        call(K, *args)
    else:
        call(*args)
    p.verify()
    return p


# ------------------------------------------------------------------------------------------------
# helpers of this module: the comparisons of the families' own files on inputs those files cannot make
# ------------------------------------------------------------------------------------------------
def check_batchnorm_one_row(K, groups, Cn):
    """bh_bn_fwd / bh_bn_bwd on ONE row per group (Cn = 1: bn1.hip), where torch's training BatchNorm refuses to run.  The float64 statement
    is the two-pass BatchNorm of tests/value_regimes.py (bn_reference): mean = x, variance 0, y = beta (+ residual, ReLU).  Forward: the
    bound the header derives for the kernels' fp32 coefficient chain (value_regimes.bn_forward_bound: 4 * 2^-24 (|x scale| + |mean scale| +
    |beta| + |y64|) - with var = 0 the scale is gamma / sqrt(eps) = 316 gamma, and x scale - mean scale cancels to the rounding of the
    product: MEASURED 4.6e-5 / 3.6e-5 of max |y| at C = 64 / 1024, 0.12 of the bound).  Running statistics: test_value_regimes_gpu.py's derived
    bound, the variance taking the unbiased estimate var n / (n - 1) only for n > 1 and the biased one otherwise (bn.hip:87, bn1.hip:102:
    what oracle/bihome_oracle.py's torch modules compute for every n they accept).  Adjoint: no gradient passes a constant - gx and
    ggamma exactly zero -, gbeta and the residual's gradient are the masked output gradient (test_batchnorm_fwd_bwd's 5e-5 / 1e-6)."""
    import value_regimes as V
    eps, mom = V.BN_EPS, 0.1
    T = torch.tensor
    x = T((C.rnd((groups, 1, 1, Cn), 20) * 2 + 0.5).astype(np.float32))
    r = T(C.rnd((groups, 1, 1, Cn), 21))
    gamma, beta = T((1 + 0.3 * C.rnd((Cn,), 22)).astype(np.float32)), T((0.2 * C.rnd((Cn,), 23)).astype(np.float32))
    rm0, rv0 = T((0.1 * C.rnd((Cn,), 24)).astype(np.float32)), T((1 + 0.2 * np.abs(C.rnd((Cn,), 25))).astype(np.float32))
    ref = V.bn_reference(x, gamma, beta, groups, r, True)
    assert float(ref["var"].abs().max()) == 0.0
    rmd, rvd, gm, bd = rm0.cuda(), rv0.cuda(), gamma.cuda(), beta.cuda()
    y, st = K.bn_fwd(x.cuda(), gm, bd, rmd, rvd, r.cuda(), groups, eps, mom, True, True)
    bound = V.bn_forward_bound(x, ref, r)
    err = (y.cpu().double() - ref["y"]).abs()
    print("\nMEASURED one-row BatchNorm groups %d C %d: max |y - y64| %.3e of max |y| %.3e, %.3f of the derived bound"
          % (groups, Cn, err.max(), ref["y"].abs().max(), (err / bound).max()))
    assert torch.isfinite(y).all() and (err <= bound).all()
    rm64, rv64 = rm0.double(), rv0.double()
    for g in range(groups):
        rm64, rv64 = (1 - mom) * rm64 + mom * ref["mean"][g], (1 - mom) * rv64 + mom * ref["var"][g]      # n == 1: the biased estimate
    assert ((rmd.cpu().double() - rm64).abs() <= groups * 4 * 2.0 ** -24 * (rm0.double().abs() + ref["mean"].abs().amax(0))).all()
    assert ((rvd.cpu().double() - rv64).abs() <= groups * 4 * 2.0 ** -24 * rv0.double().abs()).all()
    gy = T(C.rnd((groups, 1, 1, Cn), 26))
    gy[V.near_relu(ref["pre"])] = 0
    gg, gb = torch.zeros(Cn, device="cuda"), torch.zeros(Cn, device="cuda")
    gx, gres = K.bn_bwd(gy.cuda(), y, x.cuda(), gm, st, rmd, rvd, groups, eps, True, True, True, gg, gb, beta=bd)
    _sums_ready_is_the_same(K, (gy.cuda(), y, x.cuda(), gm, st, rmd, rvd, groups, eps, True, True, True), bd, gx, gres)
    masked = gy.double() * (ref["pre"] > 0)
    assert float(gx.abs().max()) == 0.0 and float(gg.abs().max()) == 0.0
    C.close(gb.cpu(), masked.reshape(-1, Cn).sum(0), 5e-5)
    C.close(gres.cpu(), masked, 1e-6)


def _sums_ready_is_the_same(K, args, beta, gx, gres):
    """bh_bn_bwd with flags bit4 (the gradient sums already in `scratch`, as bh_conv_dgrad_bnreduce leaves them - no 3x3 conv makes a
    group of four rows or fewer, so the buffer is handed over as the entry point takes it): such groups are evaluated from gy itself, in
    double - bit for bit the call without the bit, with its parameter gradients."""
    Cn = args[2].shape[-1]
    if Cn == 1:
        return                                                  # (bn1.hip refuses the bit: no conv epilogue makes one-channel sums)
    gg0, gb0, gg1, gb1 = (torch.zeros(Cn, device="cuda") for _ in range(4))
    a, ra = K.bn_bwd(*args, gg0, gb0, beta=beta)
    sums = K.bn_stats_buffer(args[7], Cn, "cuda")
    b, rb = K.bn_bwd(*args, gg1, gb1, beta=beta, sums_ready=sums)
    assert torch.equal(a, gx) and torch.equal(b, gx) and torch.equal(gg0, gg1) and torch.equal(gb0, gb1)
    if gres is not None:
        assert torch.equal(rb, gres)


def check_batchnorm_two_rows(K, groups, Cn, res):
    """TWO rows per group against the float64 two-pass BatchNorm of tests/value_regimes.py, quantity by quantity and per element (the
    helper of test_conv_kernels_gpu.py normalises by the largest element).  Forward: the header's derived bound
    (value_regimes.bn_forward_bound); running statistics: test_value_regimes_gpu.py's derived bound; ggamma / gbeta: its floor, 3e-5 of the
    sum of the magnitudes they add up, per channel (_param_scales); the residual's gradient: the masked output gradient, bitwise.  gx
    against a bound derived for an fp32 evaluation of gx = A (d - kb - xhat kg), A = gamma invstd, kb = mean d, kg = mean(d xhat): every
    term carries at most four roundings of its own magnitude, a rounded mean moves xhat by 2^-25 |mean| invstd:
        |gx - gx64| <= 4 * 2^-24 |A| (|d| + |kb| + (|xhat| + |mean| invstd) |kg|)
    (MEASURED: the fp32 kernels 0.55 / 0.32 of it at C = 64 / 8; the double evaluation groups of at most four rows now take 1e-4 of it)."""
    import test_value_regimes_gpu as VG
    import value_regimes as V
    T = torch.tensor
    x = T((C.rnd((2 * groups, 1, 1, Cn), 20) * 2 + 0.5).astype(np.float32))
    r = T(C.rnd((2 * groups, 1, 1, Cn), 21)) if res else None
    gamma, beta = T((1 + 0.3 * C.rnd((Cn,), 22)).astype(np.float32)), T((0.2 * C.rnd((Cn,), 23)).astype(np.float32))
    rm0, rv0 = T((0.1 * C.rnd((Cn,), 24)).astype(np.float32)), T((1 + 0.2 * np.abs(C.rnd((Cn,), 25))).astype(np.float32))
    ref = V.bn_reference(x, gamma, beta, groups, r, True)
    rmd, rvd, gm, bd = rm0.cuda(), rv0.cuda(), gamma.cuda(), beta.cuda()
    y, st = K.bn_fwd(x.cuda(), gm, bd, rmd, rvd, r.cuda() if res else None, groups, V.BN_EPS, 0.1, True, True)
    err = (y.cpu().double() - ref["y"]).abs()
    assert torch.isfinite(y).all() and (err <= V.bn_forward_bound(x, ref, r)).all()
    rm64, rv64 = rm0.double(), rv0.double()
    for g in range(groups):
        rm64, rv64 = 0.9 * rm64 + 0.1 * ref["mean"][g], 0.9 * rv64 + 0.1 * ref["var"][g] * 2.0
    assert ((rmd.cpu().double() - rm64).abs() <= groups * 4 * 2.0 ** -24 * (rm0.double().abs() + ref["mean"].abs().amax(0))).all()
    assert ((rvd.cpu().double() - rv64).abs() <= groups * 4 * 2.0 ** -24 * (rv0.double().abs() + 2.0 * ref["var"].amax(0))).all()
    gy = T(C.rnd((2 * groups, 1, 1, Cn), 26))
    gy[V.near_relu(ref["pre"]) | (ref["pre"].detach().abs() <= 2 * V.bn_forward_bound(x, ref, r))] = 0      # (the ReLU decision is the kernel's own y > 0)
    g64 = VG._bn_autograd(x, gamma, beta, groups, r, True, gy, torch.float64)
    gg, gb = torch.zeros(Cn, device="cuda"), torch.zeros(Cn, device="cuda")
    gx, gres = K.bn_bwd(gy.cuda(), y, x.cuda(), gm, st, rmd, rvd, groups, V.BN_EPS, True, True, res, gg, gb, beta=bd)
    _sums_ready_is_the_same(K, (gy.cuda(), y, x.cuda(), gm, st, rmd, rvd, groups, V.BN_EPS, True, True, res), bd, gx, gres)
    d = (gy.double() * (ref["pre"] > 0)).reshape(groups, 2, Cn)
    invstd = 1.0 / torch.sqrt(ref["var"] + V.BN_EPS)                                    # [groups, Cn]
    xhat = (x.double().reshape(groups, 2, Cn) - ref["mean"][:, None]) * invstd[:, None]
    kb, kg = d.mean(1, keepdim=True).abs(), (d * xhat).mean(1, keepdim=True).abs()
    bound = 4 * 2.0 ** -24 * (gamma.double() * invstd).abs()[:, None] * (d.abs() + kb + (xhat.abs() + (ref["mean"].abs() * invstd)[:, None]) * kg)
    errx = (gx.cpu().double() - g64[0]).reshape(groups, 2, Cn).abs()
    print("\nMEASURED two-row BatchNorm groups %d C %d: max |gx - gx64| %.3e where max |gx64| is %.3e: %.3f of the derived bound"
          % (groups, Cn, errx.max(), g64[0].abs().max(), (errx / bound.clamp_min(1e-300)).max()))
    assert torch.isfinite(gx).all() and (errx <= bound).all()
    sg, sb = VG._param_scales(x, ref, gy, groups, ref["pre"])
    assert ((gg.cpu().double() - g64[1]).abs() <= 3e-5 * sg).all() and ((gb.cpu().double() - g64[2]).abs() <= 3e-5 * sb).all()
    if res:
        assert torch.equal(gres.cpu(), gy * (ref["pre"] > 0))


def check_gap(K, N, HW, Cn):
    """check_maxpool_gap_add's GAP comparisons (1e-6) on [N, HW, 1, Cn] maps of any channel count."""
    x = C.rnd((N, HW, 1, Cn), 30)
    xg = torch.tensor(x).cuda()
    g = K.gap_fwd(xg)
    C.close(g.cpu().reshape(N, Cn), x.mean((1, 2)), 1e-6)
    gg = K.gap_bwd(g, tuple(xg.shape))
    C.close(gg.cpu(), np.broadcast_to(g.cpu().numpy() / HW, (N, HW, 1, Cn)), 1e-6)


def check_add(K, n):
    """check_maxpool_gap_add's bh_add comparison (bitwise) on n elements."""
    a, b = torch.tensor(C.rnd((n,), 32)).cuda(), torch.tensor(C.rnd((n,), 33)).cuda()
    s = a + b
    K.add_(a, b)
    assert torch.equal(a, s)


def check_absmax(K, n):
    """bh_absmax (test_value_regimes_gpu.py holds it on large tensors): the record's maximum is max |x| exactly, on n elements whose largest
    magnitude is the LAST one (the scalar tail of the float4 walk)."""
    x = C.rnd((n,), 34)
    x[-1] = -7.5
    rec = K.absmax(torch.tensor(x).cuda())
    assert rec.shape == (K.AMAX_FLOATS,) and float(rec.max()) == 7.5 and float(rec.min()) >= 0.0


def check_dlt(K, n, P):
    """check_dlt_fwd_bwd on the top-left 24 x 24 window (576 pixels: P = 512 distinct draws are possible) of the noisy field of its own test."""
    import test_head_kernels_gpu as HK
    from bihome_amd import synth
    pf = synth.make_head_inputs(6, seed=3, noise=0.7)["pf_hat_12"]
    HK.check_dlt_fwd_bwd(K, n, P, np.ascontiguousarray(pf[:2, :, :24, :24]), oracle32=P > 5)


def check_ransac_exact_field(K, B, Kh, h, w):
    """test_ransac_gpu's chain (counts, winner, mask, refit, repeatability) on the EXACT field of a random homography: every valid
    hypothesis reproduces it, so every count is h w and the winner is the first valid draw - no pixel near the threshold (asserted on the
    float64 restatement: border == 0), nothing for the comparison to rest on but the kernels.  On a 2 x 2 field a draw is valid only when
    it names all four pixels; a sample without a valid draw is flagged and refitted on everything."""
    import test_ransac_cpu as R
    import test_ransac_gpu as RS
    pf, choice, delta, clean = _exact_field(R, B, Kh, h, w)
    ref = R.ransac_reference(pf, choice, 3.0)
    ref.update(pf=pf, choice=choice, delta=delta, clean=clean, thr=3.0)
    assert ref["border"].sum() == 0 and ref["mask_border"].sum() == 0
    out, gpu = RS.call(K, pf, choice, 3.0)
    f = dict(ref=ref, out=out, gpu=gpu)
    RS.test_counts_at_other_shapes(f)
    RS.test_best_at_other_shapes(f)
    RS.test_mask_at_other_shapes(f)
    RS.test_refit_at_other_shapes(f)
    RS.test_two_calls_agree_bit_for_bit_at_other_shapes(K, f)


def _exact_field(R, B, Kh, h, w):
    rng = np.random.default_rng(1000 * h + w)
    c = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    delta = rng.uniform(-0.25 * min(h, w), 0.25 * min(h, w), (B, 4, 2))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    clean = np.empty((B, 2, h, w))
    for b in range(B):
        q = np.stack([xs, ys, np.ones_like(xs)], -1) @ R._four_point(c, c + delta[b]).T
        clean[b] = np.stack([q[..., 0] / q[..., 2] - xs, q[..., 1] / q[..., 2] - ys])
    choice = torch.randint(0, h * w, (B, Kh, 4), generator=torch.Generator().manual_seed(7 + Kh)).numpy().astype(np.int64)
    # the last draw names the four corners of the field: a valid hypothesis in every sample (on a 2 x 2 field the only kind there is) - a
    # sample without one is flagged and refitted on everything, which tests/test_ransac_gpu.py holds on its own (test_fallback_*)
    choice[:, -1] = np.array([0, w - 1, (h - 1) * w, h * w - 1])
    return clean.astype(np.float32), choice, delta, clean.astype(np.float32)


def check_lm(K, h, w, iters):
    """bh_homography_refine_lm against the float64 restatement of tests/test_ransac_lm_cpu.py (test_other_field_shapes' comparison and its
    delta_hat band) on every pixel of a noisy field; iters = 0: the start itself comes back, bit for bit."""
    import test_ransac_cpu as R
    import test_ransac_lm_cpu as L
    import test_ransac_lm_gpu as LG
    B = 2
    rng = np.random.default_rng(h * 100 + w)
    clean, _, delta, _ = _exact_field(R, B, 1, h, w)
    pf = (clean + rng.normal(0.0, 0.05, clean.shape)).astype(np.float32)
    c = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    start = np.stack([R._four_point(c, c + delta[b] * 1.1 + 0.02) for b in range(B)]).astype(np.float32)
    mask = np.ones((B, h, w), np.uint8)
    H0 = LG.dev(start)
    dh, H, info = K.homography_refine_lm(LG.dev(pf), H0, LG.dev(mask, torch.uint8), iters)
    torch.cuda.synchronize()
    ref = L.lm_reference(pf, start, mask, iters)
    got = dict(H=H.cpu().numpy(), delta_hat=dh.cpu().numpy(), info=info.cpu().numpy())
    LG.compare(got, ref, "%d x %d, %d steps" % (h, w, iters), L.dh_atol(h, w))
    if iters == 0:
        assert torch.equal(H, H0) and torch.equal(info[:, 0], info[:, 1]) and (info[:, 2] == 0).all()


# ------------------------------------------------------------------------------------------------
# 1. accepted edges
# ------------------------------------------------------------------------------------------------
ACCEPTED = [c for t in (S.LOSS_EDGES, S.BN_EDGES, S.BN1_EDGES, S.TAIL_EDGES, S.POOL_EDGES, S.GEOMETRY_EDGES, S.RANSAC_EDGES, S.WARP_EDGES, S.SYNTH_EDGES)
            for c in t]
assert len({c.id for c in ACCEPTED}) == len(ACCEPTED)


@pytest.mark.parametrize("case", ACCEPTED, ids=[c.id for c in ACCEPTED])
def test_accepted_edge(K, monkeypatch, case):
    module, fn, args, extra = case.run
    run_poisoned(K, monkeypatch, module, fn, args, extra)


CONV_RUNS = ([(id, helper, args, want) for id, _, helper, args, want in S.CONV_EDGE_CASES]
             + [(id, "conv2d", (N, H, W, Ci, Co, 3, 1, 1), {"fwd": S.HALO["fwd"] if taken else S.GEMM}) for id, N, H, W, Ci, Co, taken in S.HALO_GRID_CASES]
             + [(id, helper, args, {}) for id, helper, args, _, _, _ in S.STEM_CASES]
             + [(id, helper, args, {}) for id, helper, args in S.CENSUS_CASES])
assert len({c[0] for c in CONV_RUNS}) == len(CONV_RUNS)


@pytest.mark.parametrize("id,helper,args,want", CONV_RUNS, ids=[c[0] for c in CONV_RUNS])
def test_conv_edge(K, monkeypatch, id, helper, args, want):
    """The conv tables of shape_edges.py through the helper each names; `want` pins the kernels (bh_conv_variant), and the launches the
    case was written for are the ones the wrappers report making (kernels.TIMING carries the library's own names)."""
    module, fn = S.CONV_HELPERS[helper]
    kw = {}
    if want and helper in ("conv2d", "convT", "first_conv", "last_conv", "gray_stem"):
        kw = dict(variants=want)
    mod = importlib.import_module(module)
    p = poisoned_alloc.poison(monkeypatch, K, mod)
    monkeypatch.setattr(K, "_STEM_WGRAD_WS", {})
    monkeypatch.setattr(K, "TIMING", {})
    getattr(mod, fn)(K, *args, **kw)
    p.verify()
    ran = {part for name in K.TIMING for part in name.split(" ")[0].split("+")}
    L = S.Launches()
    getattr(L, helper)(*args)
    missing = L.names - ran
    assert not missing, "%s: the launch model of shape_edges.py names %s, the wrappers ran %s" % (id, sorted(missing), sorted(ran))


# ------------------------------------------------------------------------------------------------
# 2. refusals and empty batches
# ------------------------------------------------------------------------------------------------
PROTOS = S.header_prototypes()
RawCall = S.RawCall


RAW = S.REFUSALS + S.EMPTY_CASES


@pytest.mark.parametrize("case", RAW, ids=[c.id for c in RAW])
def test_refusal_or_empty_batch(case):
    entry, over, null, code = case.run
    r = RawCall(entry, over, null)
    assert r.rc == code, "%s: returned %d, the header documents %d" % (case.id, r.rc, code)
    written = dict(next(w for e, _, _, _, w in S.EMPTY_BATCH if e == entry)) if case.family == "empty" else {}
    r.untouched(but=written)
    for name, values in written.items():
        got = r.bufs[name].view(torch.float32)
        assert got[:len(values)].tolist() == list(values), (name, got[:len(values)].tolist())
        assert torch.equal(r.bufs[name][len(values):], r.before[name][len(values):])


@pytest.mark.parametrize("entry,fname,line,pointers", S.NULL_CASES, ids=[c[0] for c in S.NULL_CASES])
def test_null_for_each_required_pointer(entry, fname, line, pointers):
    names = [n for c, n in PROTOS[entry][1] if c == "ptr"]
    assert set(pointers) <= set(names), set(pointers) - set(names)
    for ptr in pointers:
        r = RawCall(entry, {}, (ptr,) + (("scratch",) if entry == "bh_synth_blobs" and ptr != "scratch" else ()))
        assert r.rc == S.BH_E_BADARG, "%s with %s = NULL returned %d" % (entry, ptr, r.rc)
        r.untouched()


def _desc_buffers(n=1 << 16):
    t = lambda: torch.full((n,), float("nan"), device="cuda")
    return t, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_workspace_one_byte_short(K):
    """bh_conv_wgrad_det (the stride-1 partial-tile form, wgrad.hip:928, and the split-operand form, wgrad_x3.hip:456) and bh_stem7_wgrad
    (stem7.hip:877) with a workspace one byte short of what their size query asks for: BH_E_BADARG, nothing written."""
    from bihome_amd._lib import lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    t, stream = _desc_buffers()
    for prec in (0, 2):
        d = K.conv_desc(8, 16, 16, 64, 64, 3, 1, 1, precision=prec)
        need = K.wgrad_det_bytes(d)
        assert need > 0
        x, gy, gw, ws = t(), t(), t(), t()
        keep = [b.clone() for b in (x, gy, gw, ws)]
        assert lib.bh_conv_wgrad_det(p(x), p(gy), p(gw), None, ctypes.byref(d), p(ws), need - 1, stream) == S.BH_E_BADARG, prec
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((x, gy, gw, ws), keep))
    d = K.conv_desc(16, 64, 128, 2, 64, 7, 2, 3, in_nchw=True)
    need = lib.bh_stem7_wgrad_ws_bytes(ctypes.byref(d))
    assert need > 0
    x, gy, gw, ws = t(), t(), t(), t()
    keep = [b.clone() for b in (x, gy, gw, ws)]
    assert lib.bh_stem7_wgrad(p(x), p(gy), p(gw), ctypes.byref(d), p(ws), need - 1, stream) == S.BH_E_BADARG
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((x, gy, gw, ws), keep))


def test_wrappers_name_the_code(K):
    """kernels.py turns a refusal into BihomeLibError with the code's name, and hands back nothing."""
    from bihome_amd._lib import BihomeLibError
    z = lambda *s: torch.zeros(*s, device="cuda")
    U, A = "BH_E_UNSUPPORTED", "BH_E_BADARG"
    H1 = torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 9).repeat(2, 1)
    calls = []
    for Cn in (6, 12, 24):
        f = z(2, 2, 2, Cn)
        m = z(2, 2, 2)
        calls += [(U, lambda f=f, m=m: K.triplet_l1_fwd(f, f, f, f, m, m, None, None)), (U, lambda f=f, m=m: K.triplet_hinge_fwd(f, f, f, f, m, m, 0.5)),
                  (U, lambda f=f, m=m: K.oneline_loss_fwd(f, f, f, m, 1.0)), (U, lambda f=f, m=m: K.oneline_cos_loss_fwd(f, f, f, m, 0.1)),
                  (U, lambda f=f: K.l2norm_fwd(f))]
    f3 = z(4, 2, 2, 8)
    calls += [
        (A, lambda: K.oneline_loss_fwd(z(1, 2, 2, 8), z(1, 2, 2, 8), f3, z(4, 2, 2), 1.0, rep=3)),                      # B % rep
        (U, lambda: K.bn_fwd(z(4, 1, 1, 12), None, None, z(12), z(12) + 1, None, 1, 1e-5, 0.1, True, True)),
        (U, lambda: K.bn_fwd(z(4, 1, 1, 2048), None, None, z(2048), z(2048) + 1, None, 1, 1e-5, 0.1, True, True)),
        (A, lambda: K.dlt_fwd(z(2, 2, 4, 4), torch.zeros(2, 3, dtype=torch.int64, device="cuda"), 1, 3)),
        (U, lambda: K.dlt_fwd(z(2, 2, 32, 32), torch.zeros(2, 513, dtype=torch.int64, device="cuda"), 1, 513)),
        (U, lambda: K.warp_fwd(z(2, 1, 24, 16), H1, 4)), (U, lambda: K.warp_fwd(z(2, 1, 48, 48), H1, 3)),
        (U, lambda: K.warp_bwd(z(2, 1, 24, 16), H1, z(2, 1, 24, 16), None, 4)),
        (U, lambda: K.photo_warp_fwd(z(2, 1, 32, 32), H1, z(2, 2), 24)),
        (U, lambda: K.photo_warp_bwd(z(2, 1, 32, 32), H1, z(2, 2), z(2, 1, 24, 24), 24)),
        (A, lambda: K.relu_bwd(z(6), z(6))),
        (A, lambda: K.scale_samples_fwd(z(2, 6), z(2), 1)), (A, lambda: K.scale_samples_bwd(z(2, 6), z(2, 6), z(2), 1, True)),
        (A, lambda: K.absmax(z(12)[1:9])),                                                                                # misaligned x
        (U, lambda: K.bn_bwd_from_1x1(K.GradFrom1x1(z(16, 1, 1, 8), z(8, 1, 1, 32)), z(16, 1, 1, 32), z(32) + 1, z(32), K.bn_stats_buffer(2, 32, "cuda"), 2, 1e-5, True)),   # KC = 8
        (U, lambda: K.bn_bwd_from_1x1(K.GradFrom1x1(z(4, 1, 1, 16), z(16, 1, 1, 32)), z(4, 1, 1, 32), z(32) + 1, z(32), K.bn_stats_buffer(2, 32, "cuda"), 2, 1e-5, True)),   # two rows
        (U, lambda: K.bn_maxpool_fwd(z(2, 1, 2, 8), z(8) + 1, z(8), z(8), z(8) + 1, 1, 1e-5, 0.1, True, True, K.bn_stats_buffer(1, 8, "cuda"), False)),                      # four rows
        (U, lambda: K.synth_blobs(z(2, 24, 24), torch.zeros(2, dtype=torch.int32, device="cuda"), z(2, 1, 24, 24), z(2, 1, 24, 24), z(2, 24, 24), 1.0, 0.3)),              # P = 24
    ]
    for Ci, Cm, Co, hw in ((32, 64, 2, 4), (12, 64, 2, 4), (16, 32, 2, 4), (16, 320, 2, 4), (16, 64, 5, 4), (16, 64, 2, 3)):
        calls.append((U, lambda Ci=Ci, Cm=Cm, Co=Co, hw=hw: K.tail_fwd(z(1, 2, 2, Ci), z(Cm, Ci), z(Cm), z(Cm) + 1, z(Cm), z(Cm), z(Cm) + 1, z(Co, Cm), z(Co), 1, hw, 1e-5, 0.1, True)))
    for code, call in calls:
        with pytest.raises(BihomeLibError, match=code):
            call()
    # the device pair generator refuses P = 24 by name as well (bh_synth_batch)
    from bihome_amd.synth_gpu import GpuPairGenerator
    with pytest.raises((BihomeLibError, ValueError), match="BH_E_UNSUPPORTED|16"):
        gen = GpuPairGenerator(n_images=1, patch=24, rho=4, seed=0)
        gen.make(*gen.draw(2)[:3])
    # a workspace shorter than the deterministic weight gradient needs: a deterministic call says so instead of using it
    with K.det_scope(True):
        d = K.conv_desc(8, 16, 16, 64, 64, 3, 1, 1)
        with pytest.raises(RuntimeError, match="workspace"):
            K.conv_wgrad(z(8, 16, 16, 64), z(8, 16, 16, 64), z(64, 3, 3, 64), None, d, det_ws=torch.empty(K.wgrad_det_bytes(d) // 4 - 1, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 3. thresholds that need more than a table row
# ------------------------------------------------------------------------------------------------
def test_stem_forward_with_the_warp_at_its_smallest_grid(K, monkeypatch):
    """bh_stem7_fwd_warp takes 256 tiles of 8 x 8 outputs (stem7.hip `a.ntiles < 256`): the family's comparison at exactly 256, and
    BH_E_UNSUPPORTED - nothing written - at 255, where kernels.conv_fwd makes the two calls instead."""
    from bihome_amd._lib import lib
    import test_head_kernels_gpu as HK
    B, h, w = S.STEM_WARP_AT[:3]
    assert B * (h // 16) * (w // 16) == 256
    run_poisoned(K, monkeypatch, "test_head_kernels_gpu", "check_stem_forward_with_the_warp_folded_in", S.STEM_WARP_AT)
    B, h, w = S.STEM_WARP_BELOW
    assert B * (h // 16) * (w // 16) == 255
    d = K.conv_desc(B, h, w, 1, 64, 7, 2, 3, precision=4)
    assert K.conv_variant(d, "fwd").startswith("conv_gemm_kernel<")                  # (the plain stem routes to the generic kernel there)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    src, H64, wt = nan(B, 1, h, w), torch.full((B, 9), float("nan"), dtype=torch.float64, device="cuda"), nan(64, 7, 7, 1)
    y, warped, cov = nan(B, h // 2, w // 2, 64), nan(B, 1, h, w), nan(B, h // 4, w // 4)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.bh_stem7_fwd_warp(p(src), p(H64), 4, p(wt), None, p(y), ctypes.byref(d), p(warped), p(cov), None, 1,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == S.BH_E_UNSUPPORTED
    assert all(torch.isnan(t).all() for t in (y, warped, cov))
    # through the wrapper: the warp and the conv as two calls, the flag says so
    g = torch.Generator().manual_seed(3)
    srcv = torch.randn(B, 1, h, w, generator=g).cuda()
    Hid, _ = K.h4pt_fwd(HK.dev(HK.rand_delta(B, 5, amp=8)), (w, h))
    x, cov2 = nan(B, h, w, 1), nan(B, h // 4, w // 4)
    source = dict(src=srcv, H64=Hid, pool=4, cov=cov2, done=False, filled=False)
    wv = (torch.randn(64, 7, 7, 1, generator=g) * 0.05).cuda()
    y2 = K.conv_fwd(x, wv, None, d, warp_src=source)
    assert source["filled"] and not source["done"]
    wref, cref = K.warp_fwd(srcv, Hid, 4)
    assert torch.equal(x.view_as(wref), wref) and torch.equal(cov2, cref) and torch.equal(y2, K.conv_fwd(wref.view(B, h, w, 1), wv, None, d))


@pytest.mark.parametrize("id,N,H,W,Ci,Co,taken", [c for c in S.HALO_GRID_CASES if c[4] == c[5] == 64], ids=lambda v: v if isinstance(v, str) else None)
def test_packed_kernels_at_the_grid_threshold(K, monkeypatch, id, N, H, W, Ci, Co, taken):
    """The packed launches (precisions 0 / 2 / 3 / 4: halo-tiled kernel, persistent kernel for the fp16 pieces) WITHOUT BH_ROUTE_HALO_SMALL:
    at the smallest grid they take the f16x2 helper's float64 comparison, with the persistent kernel pinned; one sub-tile pair below, a packed
    launch is refused (its weights are no operand of the generic kernel) and nothing is written."""
    from bihome_amd._lib import BihomeLibError
    import test_f16x2_gpu as F16
    d4 = K._with_layout(K.conv_desc(N, H, W, Ci, Co, 3, 1, 1, precision=4), 4)
    if taken:
        assert K.conv_variant(d4, "fwd") == "conv3x3_pc_kernel<false,false,0>" and K.conv_variant(d4, "dgrad") == "conv3x3_pc_kernel<true,false,0>"
        p = poisoned_alloc.poison(monkeypatch, K, F16)
        F16.check_conv3x3_f16x2_forward_and_dgrad(K, N, H, W, Ci, Co, False, kernel4="conv3x3_pc_kernel", halo_small=False)
        p.verify()
        return
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, Ci, generator=g).cuda()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) * 0.05).cuda().contiguous(memory_format=torch.channels_last)
    for prec in (0, 2, 3, 4):
        _, pf, pd = F16._packed(K, w, prec)
        d = K.conv_desc(N, H, W, Ci, Co, 3, 1, 1, precision=prec)
        assert not K.packs_3x3(d)
        for call in (lambda: K.conv_fwd(x, w.permute(0, 2, 3, 1), None, d, wpacked=pf), lambda: K.conv_dgrad(x, w.permute(0, 2, 3, 1), d, wpacked=pd)):
            with pytest.raises(BihomeLibError, match="BH_E_UNSUPPORTED"):
                call()


@pytest.mark.parametrize("N,H,W,Ci,Co,taken", S.WGRAD_X3_GRID)
def test_split_operand_weight_gradient_at_its_smallest_grid(K, monkeypatch, N, H, W, Ci, Co, taken):
    """wgrad_x3.hip has no grid minimum: one 8 x 8 tile runs wgrad_x3_kernel in precisions 2 / 3 / 4 with the default route (the f16x2
    helper's float64 comparison).  A map that is no multiple of 8, or 16-channel blocks, routes to the stride-1 / small-channel kernels:
    pinned, and the precision-2 / 4 weight gradient held to float64 with check_conv2d_fwd_dgrad_wgrad's 3e-5."""
    import test_f16x2_gpu as F16
    names = {prec: K.conv_variant(K.conv_desc(N, H, W, Ci, Co, 3, 1, 1, precision=prec), "wgrad") for prec in (2, 3, 4)}
    assert all(v.startswith("wgrad_x3_kernel<") == taken for v in names.values()), names
    p = poisoned_alloc.poison(monkeypatch, K, F16)
    if taken:
        F16.check_wgrad_f16x2_kernel(K, N, H, W, Ci, Co)
    else:
        import torch.nn.functional as F
        x, gy = C.rnd((N, Ci, H, W), 1), C.rnd((N, Co, H, W), 4)
        wt = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(torch.tensor(x, dtype=torch.float64), wt, None, 1, 1).backward(torch.tensor(gy, dtype=torch.float64))
        xg, gyg = (torch.tensor(a).permute(0, 2, 3, 1).contiguous().cuda() for a in (x, gy))
        for prec in (2, 4):
            gw = torch.zeros(Co, 3, 3, Ci, device="cuda")
            K.conv_wgrad(xg, gyg, gw, None, K.conv_desc(N, H, W, Ci, Co, 3, 1, 1, precision=prec))
            C.close(gw.cpu().permute(0, 3, 1, 2), wt.grad)
    p.verify()
