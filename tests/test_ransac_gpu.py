"""bh_ransac_homography on the MI355X against the float64 restatement of tests/test_ransac_cpu.py (same inputs: a field with 0.3 px
noise, a 30 % block of wrong offsets, 5 % scattered outliers; B = 6, K = 128, seeded minimal samples).

Integer results are compared as integers.  fp32 and float64 can only decide a pixel differently where its float64 squared error lies
within a relative 1e-4 of thr^2 ("border" pixels; the fp32 test's own rounding is ~1e-6 of thr^2), so counts may differ by at most the
number of border pixels of that hypothesis, and where no candidate winner has a border pixel the winner is pinned exactly.

The same comparison runs at the shapes of R.FIELD_CASES - fields of 35 to 3071 pixels that are no multiple of any tile, K up to 2100 -
and on two constructed inputs: a tie that only the lowest-k rule decides, and a best count of exactly 4 / below 4."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ransac_cpu as R  # noqa: E402

from bihome_amd import configs, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from bihome_amd import kernels
    return kernels


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda().contiguous()


@pytest.fixture(scope="module")
def case(K):
    pf, choice, delta, clean = R.make_inputs()
    ref = R.ransac_reference(pf, choice)
    dh, H, best, n_inl, count, mask = K.ransac_homography(dev(pf), dev(choice, torch.int64), R.THR, want_mask=True)
    torch.cuda.synchronize()
    gpu = dict(delta_hat=dh.cpu().numpy(), H=H.cpu().numpy(), best=best.cpu().numpy(), n_inl=n_inl.cpu().numpy(),
               count=count.cpu().numpy(), mask=mask.cpu().numpy())
    return dict(pf=pf, choice=choice, delta=delta, clean=clean, ref=ref, gpu=gpu)


def test_counts(case):
    ref, gpu = case["ref"], case["gpu"]
    B, Kn = ref["count"].shape
    n = case["pf"].shape[2] * case["pf"].shape[3]
    diff = np.abs(gpu["count"].astype(np.int64) - ref["count"])
    print("border pixels %d of %d; hypotheses whose count differs: %d, largest difference %d; invalid %d"
          % (ref["border"].sum(), B * Kn * n, (diff > 0).sum(), diff.max(), (~ref["valid"]).sum()))
    assert ref["border"].sum() <= 1e-3 * B * Kn * n
    assert gpu["count"].dtype == np.int32 and gpu["count"].shape == (B, Kn)
    assert np.array_equal(gpu["count"] == -1, ~ref["valid"])            # invalid hypotheses agree exactly
    assert (diff <= ref["border"]).all(), np.argwhere(diff > ref["border"])


def test_best(case):
    ref, gpu = case["ref"], case["gpu"]
    cand = R.candidates(ref["count"], ref["border"], ref["best"])
    exact = 0
    for b, (members, all_exact) in enumerate(cand):
        print("sample %d: best gpu %d ref %d, candidates %d, exact %s" % (b, gpu["best"][b], ref["best"][b], len(members), all_exact))
        assert int(gpu["best"][b]) in members
        if all_exact:
            exact += 1
            assert gpu["best"][b] == ref["best"][b]                     # counts exact: the same winner, lowest-k tie rule included
    assert exact >= 5
    assert gpu["best"].dtype == np.int64


def test_mask_and_integer_identities(case):
    ref, gpu = case["ref"], case["gpu"]
    B = len(gpu["best"])
    sums = gpu["mask"].reshape(B, -1).astype(np.int64).sum(1)
    assert set(np.unique(gpu["mask"]).tolist()) <= {0, 1}
    assert np.array_equal(sums, gpu["n_inl"])                           # the mask kernel and the counting kernel decide identically
    assert np.array_equal(gpu["n_inl"], gpu["count"][np.arange(B), gpu["best"]])
    # against the restatement's mask OF THE SAME HYPOTHESIS: differences only at border pixels
    rmask, rborder = R.inlier_mask(case["pf"], ref["hyp"], gpu["best"], gpu["n_inl"])
    differ = gpu["mask"] != rmask
    print("mask pixels that differ from the restatement: %d (border pixels of the winners: %d)" % (differ.sum(), rborder.sum()))
    assert not (differ & ~rborder).any()


def test_refit_on_the_gpus_own_mask(case):
    """Tolerances of test_dlt_fwd_bwd (tests/test_head_kernels_gpu.py) for bh_dlt_fwd against its float64 oracle."""
    gpu = case["gpu"]
    H, dh = R.refit(case["pf"], gpu["mask"])
    print("refit: max |H - ref| %.3e, max |delta_hat - ref| %.3e" % (np.abs(gpu["H"] - H).max(), np.abs(gpu["delta_hat"] - dh).max()))
    np.testing.assert_allclose(gpu["H"], H, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gpu["delta_hat"], dh, atol=2e-5)
    m = R.mace(gpu["delta_hat"].astype(np.float64), case["delta"])
    print("MACE of the GPU estimate against the true offsets:", m)
    assert (m < 0.5).all()


def test_exact_field_agrees_with_the_lattice_path(K, case):
    from bihome_amd.heads import NoOpHead
    clean, choice = case["clean"], case["choice"]
    B, _, h, w = clean.shape
    dh, H, best, n_inl, count, _ = K.ransac_homography(dev(clean), dev(choice, torch.int64), R.THR)
    dh_lat, _ = NoOpHead.Model._postprocess(dev(clean))
    _, valid = R.hypotheses(clean, choice)
    count = count.cpu().numpy()
    rel = np.abs(dh.cpu().numpy() - dh_lat.cpu().numpy()).max() / np.abs(dh_lat.cpu().numpy()).max()
    print("exact field: relative difference to the lattice path %.3e; valid hypotheses %d of %d" % (rel, valid.sum(), valid.size))
    assert rel < 1e-3
    assert np.array_equal(count == -1, ~valid)
    assert (count[valid] == h * w).all()
    assert (n_inl.cpu().numpy() == h * w).all()
    assert np.array_equal(best.cpu().numpy(), np.argmax(valid, 1))      # every valid hypothesis ties: the first one wins
    assert np.abs(dh.cpu().numpy() - case["delta"]).max() / np.abs(case["delta"]).max() < 1e-3


# ------------------------------------------------------------------------------------------------
# the other shapes: R.FIELD_CASES (what each reaches is said there; their conditions are asserted in tests/test_ransac_cpu.py)
# ------------------------------------------------------------------------------------------------
NAMES = ("delta_hat", "H", "best", "n_inl", "count", "mask")


def call(K, pf, choice, thr):
    """-> (the call's device tensors in NAMES' order, the same as numpy arrays by name)"""
    out = K.ransac_homography(dev(pf), dev(choice, torch.int64), thr, want_mask=True)
    torch.cuda.synchronize()
    return out, {n: t.cpu().numpy() for n, t in zip(NAMES, out)}


def dh_atol(h, w, reach=0.0):
    """2e-5 px is fp32 output rounding at the 128-pixel corner coordinates of the first tests: it grows with the coordinate."""
    return 2e-5 * max(1.0, (max(h, w) + reach) / 128.0)


@pytest.fixture(scope="module", params=range(len(R.FIELD_CASES)), ids=["%dx%dx%dx%d" % c[:4] for c in R.FIELD_CASES])
def field(K, request):
    ref = R.field_case(request.param)
    out, gpu = call(K, ref["pf"], ref["choice"], ref["thr"])
    return dict(ref=ref, out=out, gpu=gpu)


def test_counts_at_other_shapes(field):
    ref, gpu = field["ref"], field["gpu"]
    diff = np.abs(gpu["count"].astype(np.int64) - ref["count"])
    print("border pixels %d; hypotheses whose count differs: %d, largest difference %d; invalid %d of %d"
          % (ref["border"].sum(), (diff > 0).sum(), diff.max(), (~ref["valid"]).sum(), ref["valid"].size))
    assert gpu["count"].dtype == np.int32 and gpu["count"].shape == ref["count"].shape
    assert np.array_equal(gpu["count"] == -1, ~ref["valid"])
    assert (diff <= ref["border"]).all(), np.argwhere(diff > ref["border"])


def test_best_at_other_shapes(field):
    """Every sample's candidate set is exact (tests/test_ransac_cpu.py): the winner is pinned for every sample."""
    ref, gpu = field["ref"], field["gpu"]
    B = len(ref["best"])
    print("best gpu %s ref %s, n_inl gpu %s ref %s" % (gpu["best"], ref["best"], gpu["n_inl"], ref["n_inl"]))
    assert gpu["best"].dtype == np.int64 and gpu["n_inl"].dtype == np.int32
    assert np.array_equal(gpu["best"], ref["best"])
    assert np.array_equal(gpu["n_inl"], gpu["count"][np.arange(B), gpu["best"]])


def test_mask_at_other_shapes(field):
    ref, gpu = field["ref"], field["gpu"]
    B = len(ref["best"])
    assert gpu["mask"].dtype == np.uint8 and gpu["mask"].shape == ref["mask"].shape
    assert set(np.unique(gpu["mask"]).tolist()) <= {0, 1}
    assert np.array_equal(gpu["mask"].reshape(B, -1).astype(np.int64).sum(1), gpu["n_inl"])
    rmask, rborder = R.inlier_mask(ref["pf"], ref["hyp"], gpu["best"], gpu["n_inl"], ref["thr"])
    differ = gpu["mask"] != rmask
    print("mask pixels that differ from the restatement: %d (border pixels of the winners: %d)" % (differ.sum(), rborder.sum()))
    assert not (differ & ~rborder).any()


def test_refit_at_other_shapes(field):
    """test_refit_on_the_gpus_own_mask's bands, delta_hat's scaled with the corner coordinate (dh_atol).  What the float64 yardstick
    itself is good for at these sizes is measured in tests/test_ransac_cpu.py (test_conditions_at_the_other_shapes): 2.3e-10 px."""
    ref, gpu = field["ref"], field["gpu"]
    h, w = ref["pf"].shape[2:]
    H, dh = R.refit(ref["pf"], gpu["mask"])
    print("refit: max |H - ref| %.3e, max |delta_hat - ref| %.3e (allowed %.3e); MACE against the true offsets %s"
          % (np.abs(gpu["H"] - H).max(), np.abs(gpu["delta_hat"] - dh).max(), dh_atol(h, w), R.mace(gpu["delta_hat"].astype(np.float64), ref["delta"])))
    np.testing.assert_allclose(gpu["H"], H, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gpu["delta_hat"], dh, atol=dh_atol(h, w))


def test_two_calls_agree_bit_for_bit_at_other_shapes(K, field):
    again, _ = call(K, field["ref"]["pf"], field["ref"]["choice"], field["ref"]["thr"])
    for name, a, b in zip(NAMES, field["out"], again):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("i", R.TIE_CASES)
def test_lowest_k_wins_a_tie_across_lanes(K, i):
    """Exact field, the first three draws invalid, the first valid draw repeated as the last hypothesis (R.tie_case): every valid
    hypothesis counts h*w, and the selection has to return the first of them."""
    ref = R.tie_case(i)
    h, w = ref["pf"].shape[2:]
    _, gpu = call(K, ref["pf"], ref["choice"], ref["thr"])
    print("first valid hypothesis %s, best %s" % (ref["first"], gpu["best"]))
    assert np.array_equal(gpu["count"] == -1, ~ref["valid"])
    assert (gpu["count"][ref["valid"]] == h * w).all()
    assert np.array_equal(gpu["best"], ref["first"]) and (ref["first"] >= 3).all()
    assert (gpu["n_inl"] == h * w).all() and (gpu["mask"] == 1).all()


def test_fallback_boundary(K):
    """R.wild_case: a best count of exactly 4 is refitted on its four points; a best count below 4, with valid hypotheses there, falls
    back to every point.  delta_hat's band is dh_atol at the corner's own coordinate (these homographies send corners thousands of
    pixels away; tests/test_ransac_cpu.py holds the yardstick's own sensitivity to a tenth of that band)."""
    ref = R.wild_case()
    pf, choice = ref["pf"], ref["choice"]
    B, _, h, w = pf.shape
    _, gpu = call(K, pf, choice, ref["thr"])
    top = ref["count"].max(1)
    a, b = np.nonzero(top == 4)[0], np.nonzero((top >= 0) & (top < 4))[0]
    print("counts gpu %s; best %s, n_inl %s" % (gpu["count"].tolist(), gpu["best"], gpu["n_inl"]))
    assert len(a) and len(b)
    assert np.array_equal(gpu["count"], ref["count"])                   # no border pixel: exact
    assert np.array_equal(gpu["best"], ref["best"])
    assert (gpu["n_inl"][a] == 4).all() and (gpu["n_inl"][b] == 0).all()
    for s in a:
        assert np.array_equal(np.nonzero(gpu["mask"][s].reshape(-1))[0], np.sort(choice[s, gpu["best"][s]]))
    assert (gpu["mask"][b] == 1).all()
    want = np.ones((B, h, w), np.uint8)
    want[a] = gpu["mask"][a]
    H, dh = R.refit(pf, want)
    assert np.isfinite(gpu["H"]).all() and np.isfinite(gpu["delta_hat"]).all()
    np.testing.assert_allclose(gpu["H"], H, rtol=1e-5, atol=1e-6)
    for s in range(B):
        err, tol = np.abs(gpu["delta_hat"][s] - dh[s]).max(), dh_atol(h, w, np.abs(dh[s]).max())
        print("sample %d (%s): max |delta_hat| %.1f, max |delta_hat - ref| %.3e (allowed %.3e)" % (s, "4 inliers" if s in a else "all points", np.abs(dh[s]).max(), err, tol))
        assert err <= tol


def test_fallback_when_every_hypothesis_is_invalid(K):
    g = np.random.default_rng(3)
    pf = g.uniform(-64, 64, (2, 2, 128, 128)).astype(np.float32)
    choice = np.tile(np.array([3, 3, 7, 9], np.int64), (2, 4, 1))       # a repeated index in every draw
    dh, H, best, n_inl, count, mask = K.ransac_homography(dev(pf), dev(choice, torch.int64), R.THR, want_mask=True)
    torch.cuda.synchronize()
    assert (count.cpu().numpy() == -1).all() and (n_inl.cpu().numpy() == 0).all() and (best.cpu().numpy() == 0).all()
    assert (mask.cpu().numpy() == 1).all()
    assert np.isfinite(H.cpu().numpy()).all() and np.isfinite(dh.cpu().numpy()).all()


def test_kernel_treats_an_index_outside_the_field_as_invalid(K):
    """Below the wrapper's host check (which a graph capture skips): the kernel never dereferences such an index."""
    from bihome_amd._lib import check, lib
    pf, choice, _, _ = R.make_inputs(B=1, K=8)
    choice = choice.copy()
    choice[0, 2, 1] = 128 * 128 + 5
    choice[0, 5, 3] = -7
    pfd, ch = dev(pf), dev(choice, torch.int64)
    z = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")      # noqa: E731
    hyp, count, best, n_inl = z(1, 8, 9), z(1, 8, dt=torch.int32), z(1, dt=torch.int64), z(1, dt=torch.int32)
    work, H, dh = z(1, 32, dt=torch.float64), z(1, 9), z(1, 8)
    check(lib.bh_ransac_homography(K._p(pfd), K._p(ch), 1, 8, 128, 128, R.THR, K._p(hyp), K._p(count), K._p(best), K._p(n_inl), None,
                                   K._p(work), K._p(H), K._p(dh), K._stream()), "bh_ransac_homography")
    torch.cuda.synchronize()
    ref = R.ransac_reference(pf, choice)
    assert not ref["valid"][0, 2] and not ref["valid"][0, 5]
    assert np.array_equal(count.cpu().numpy() == -1, ~ref["valid"])
    assert torch.isnan(hyp[0, 2]).all() and torch.isnan(hyp[0, 5]).all()
    assert int(best[0]) == int(ref["best"][0]) or ref["border"].sum() > 0
    assert torch.isfinite(H).all()


def test_wrapper_checks(K):
    pf = dev(np.zeros((1, 2, 16, 16), np.float32))
    choice = torch.tensor([[[0, 5, 40, 256]]], dtype=torch.int64).cuda()      # 256 = h*w: one past the end
    with pytest.raises(ValueError, match="outside"):
        K.ransac_homography(pf, choice)
    with pytest.raises(ValueError, match="outside"):
        K.ransac_homography(pf, torch.tensor([[[0, 5, 40, -1]]], dtype=torch.int64).cuda())
    with pytest.raises(ValueError):
        K.ransac_homography(pf, torch.zeros(1, 4, 3, dtype=torch.int64).cuda())
    with pytest.raises(RuntimeError, match="gradient"):
        K.ransac_homography(pf.clone().requires_grad_(True), torch.tensor([[[0, 5, 40, 77]]], dtype=torch.int64).cuda())


def test_model_level(K):
    """zeng-orig with ALL_POINTS_FIT='ransac': finite [B,4,2], two calls bitwise equal; the default kwargs still give the lattice fit."""
    from bihome_amd.step import build_model, predict
    from bihome_amd.weights import load_synthetic
    B = 4
    d = synth.make_pairs(B, seed=11, target=True)
    data = {k: dev(d[k]) for k in ("patch_1", "patch_2", "delta", "target", "corners")}
    cfg = configs.get("zeng-orig")
    cfg["MODEL"]["HEAD"]["ALL_POINTS_FIT"] = "ransac"
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    with torch.no_grad():
        a = predict(model, dict(data))
        b = predict(model, dict(data))
        assert a.shape == (B, 4, 2) and torch.isfinite(a).all()
        out = model[0].predict_homography(dict(data))
        c = model[1].predict_homography(out)[0]
        e = model[1].predict_homography(out)[0]
        assert torch.equal(c, e)                                        # fixed-seed draws, integer atomics
        assert torch.equal(a, b)
        # supplied draws are used
        choice = torch.randint(0, 128 * 128, (B, 32, 4), generator=torch.Generator().manual_seed(1)).cuda()
        f = model[1].predict_homography(dict(out, ransac_choice=choice))[0]
        g = K.ransac_homography(out["pf_hat_12"].detach().float().contiguous(), choice)[0]
        assert torch.equal(f, g)
        # on an exact field the estimator recovers the offsets
        dh, H = model[1].predict_homography({"pf_hat_12": data["target"]})
        assert H.shape == (B, 3, 3)
        assert np.abs(dh.cpu().numpy() - d["delta"]).max() / np.abs(d["delta"]).max() < 1e-3
        default = build_model(configs.get("zeng-orig"))
        load_synthetic(default[0], 0)
        default.eval()
        out = default[0].predict_homography(dict(data))
        got = default[1].predict_homography(out)
        want = default[1]._postprocess(out["pf_hat_12"])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
