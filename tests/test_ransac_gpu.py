"""bh_ransac_homography on the MI355X against the float64 restatement of tests/test_ransac_cpu.py (same inputs: a field with 0.3 px
noise, a 30 % block of wrong offsets, 5 % scattered outliers; B = 6, K = 128, seeded minimal samples).

Integer results are compared as integers.  fp32 and float64 can only decide a pixel differently where its float64 squared error lies
within a relative 1e-4 of thr^2 ("border" pixels; the fp32 test's own rounding is ~1e-6 of thr^2), so counts may differ by at most the
number of border pixels of that hypothesis, and where no candidate winner has a border pixel the winner is pinned exactly."""
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
    assert np.abs(dh.cpu().numpy() - case["delta"]).max() / np.abs(case["delta"]).max() < 1e-3


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
