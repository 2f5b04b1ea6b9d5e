"""bh_homography_refine_lm on the MI355X against the float64 restatement of tests/test_ransac_lm_cpu.py.  The restatement runs on the
GPU's OWN inlier mask and the GPU's own fp32 start H, so threshold-border pixels and the refit's rounding play no part; tolerances are
the ones tests/test_ransac_gpu.py holds the refit to (fp32 output rounding at |delta| < 64 is 4e-6).  tests/test_ransac_lm_cpu.py
asserts that the polish moves these corners by at least 2e-3 px / 0.05 px: 100x what is allowed here - and the same, with the
band scaled by the corner coordinate, for the field shapes of test_other_field_shapes and the chained run at 37 x 83."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ransac_cpu as R  # noqa: E402
import test_ransac_lm_cpu as L  # noqa: E402

from bihome_amd import configs, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from bihome_amd import kernels
    return kernels


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda().contiguous()


def run(K, pf, choice, iters=L.LM_ITERS, thr=R.THR):
    pfd = dev(pf)
    _, H0, _, _, _, mask = K.ransac_homography(pfd, dev(choice, torch.int64), thr, want_mask=True)
    keep = H0.clone()
    dh, H, info = K.homography_refine_lm(pfd, H0, mask, iters)
    torch.cuda.synchronize()
    assert torch.equal(H0, keep)                                        # the start is not modified
    return dict(pfd=pfd, H0d=H0, maskd=mask, dhd=dh, Hd=H, infod=info, H0=H0.cpu().numpy(), mask=mask.cpu().numpy(),
                delta_hat=dh.cpu().numpy(), H=H.cpu().numpy(), info=info.cpu().numpy())


def compare(g, ref, what, dh_atol=2e-5):
    print("%s: max |H - ref| %.3e, max |delta_hat - ref| %.3e, accepted gpu %s ref %s" %
          (what, np.abs(g["H"] - ref["H"]).max(), np.abs(g["delta_hat"] - ref["delta_hat"]).max(), g["info"][:, 2], ref["info"][:, 2]))
    print("%s: cost before %s after %s (ref after %s), lambda %s" % (what, g["info"][:, 0], g["info"][:, 1], ref["info"][:, 1], g["info"][:, 3]))
    np.testing.assert_allclose(g["H"], ref["H"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g["delta_hat"], ref["delta_hat"], atol=dh_atol)
    assert (g["info"][:, 1] <= g["info"][:, 0]).all()
    np.testing.assert_allclose(g["info"][:, 0], ref["info"][:, 0], rtol=1e-9)
    np.testing.assert_allclose(g["info"][:, 1], ref["info"][:, 1], rtol=1e-9)


@pytest.fixture(scope="module")
def case(K):
    pf, choice, delta, _ = R.make_inputs()
    return dict(pf=pf, choice=choice, delta=delta, gpu=run(K, pf, choice))


def test_polish_on_the_test_inputs(case):
    g = case["gpu"]
    ref = L.lm_reference(case["pf"], g["H0"], g["mask"], L.LM_ITERS)
    start = L.lm_reference(case["pf"], g["H0"], g["mask"], 0)["delta_hat"]
    moved = np.abs(ref["delta_hat"] - start).reshape(len(start), -1).max(1)
    print("corners moved by the polish (restatement, GPU start):", moved)
    assert (moved >= 2e-3).all()
    compare(g, ref, "test inputs")
    assert g["info"].dtype == np.float64 and (g["info"][:, 2] >= 1).all() and (g["H"][:, 2, 2] == 1.0).all()


def test_polish_on_the_noisy_inputs(K):
    pf, choice, delta, _ = L.make_noisy_inputs()
    g = run(K, pf, choice)
    ref = L.lm_reference(pf, g["H0"], g["mask"], L.LM_ITERS)
    start = L.lm_reference(pf, g["H0"], g["mask"], 0)["delta_hat"]
    moved = np.abs(ref["delta_hat"] - start).reshape(len(start), -1).max(1)
    print("corners moved by the polish (restatement, GPU start):", moved)
    assert (moved >= 0.05).all()
    compare(g, ref, "noisy inputs")
    before, after = R.mace(start, delta), R.mace(g["delta_hat"].astype(np.float64), delta)
    print("MACE against the true offsets: refit", before, "-> polished", after)
    assert after.mean() < before.mean()


def test_two_calls_agree_bit_for_bit(K, case):
    g = case["gpu"]
    dh, H, info = K.homography_refine_lm(g["pfd"], g["H0d"], g["maskd"], L.LM_ITERS)
    torch.cuda.synchronize()
    assert torch.equal(dh, g["dhd"]) and torch.equal(H, g["Hd"]) and torch.equal(info, g["infod"])
    assert np.array_equal(g["H0d"].cpu().numpy(), g["H0"])


def test_mask_none_few_points_and_zero_steps(K, case):
    g = case["gpu"]
    pfd, H0 = g["pfd"], g["H0d"]
    B, _, h, w = pfd.shape
    # no mask == a mask of ones, bit for bit (every pixel: the outlier block too - only the identity is looked at)
    a = K.homography_refine_lm(pfd, H0, None, 3)
    b = K.homography_refine_lm(pfd, H0, torch.ones(B, h, w, dtype=torch.uint8, device="cuda"), 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # three correspondences in sample 1: it keeps its start, the others are polished as before
    m = g["maskd"].clone()
    m[1] = 0
    m[1, 5, 7] = m[1, 60, 90] = m[1, 100, 20] = 1
    dh, H, info = K.homography_refine_lm(pfd, H0, m, L.LM_ITERS)
    dh0, Hz, info0 = K.homography_refine_lm(pfd, H0, g["maskd"], 0)
    torch.cuda.synchronize()
    assert torch.equal(H[1], H0[1]) and info[1, 2] == 0 and info[1, 0] == info[1, 1]
    assert torch.equal(H[0], g["Hd"][0]) and torch.equal(dh[2:], g["dhd"][2:])
    # zero steps: the start's corners (what the refit itself reported, up to its fp32 rounding of H) and two equal costs
    assert torch.equal(Hz, H0) and torch.equal(info0[:, 0], info0[:, 1]) and (info0[:, 2] == 0).all()
    assert torch.equal(info0[:, 0], g["infod"][:, 0])
    want = L.lm_reference(case["pf"], g["H0"], g["mask"], 0)["delta_hat"]
    np.testing.assert_allclose(dh0.cpu().numpy(), want, atol=2e-5)
    np.testing.assert_allclose(dh[1].cpu().numpy(), want[1], atol=2e-5)


def test_head_level(K, case):
    from bihome_amd.heads import NoOpHead
    from bihome_amd.step import build_model, evaluate
    from bihome_amd.weights import load_synthetic
    g = case["gpu"]
    kw = dict(TARGET_GEN="all_points", LEARNING_KEYS=["target", "pf_hat_12", "delta", "pf_hat_12"], ALL_POINTS_FIT="ransac")
    data = {"pf_hat_12": g["pfd"], "ransac_choice": dev(case["choice"], torch.int64)}
    dh, H = NoOpHead.Model(None, RANSAC_REFINE="lm", **kw).predict_homography(dict(data))
    assert torch.equal(dh, g["dhd"]) and torch.equal(H, g["Hd"])
    # 'none' (and the default): exactly the RANSAC call's own result
    want = K.ransac_homography(g["pfd"], data["ransac_choice"], R.THR)
    for head in (NoOpHead.Model(None, RANSAC_REFINE="none", **kw), NoOpHead.Model(None, **kw)):
        got = head.predict_homography(dict(data))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(dh, want[0])
    # the polished path inside step.evaluate on a zeng-orig model
    B = 4
    d = synth.make_pairs(B, seed=11, target=True)
    batch = {k: dev(d[k]) for k in ("patch_1", "patch_2", "delta", "target", "corners")}
    cfg = configs.get("zeng-orig")
    cfg["MODEL"]["HEAD"].update(ALL_POINTS_FIT="ransac", RANSAC_REFINE="lm")
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    m, ms = evaluate(model, [dict(batch), dict(batch)])
    print("zeng-orig evaluate with the polish: MACE %.4f, %.3f ms per batch of %d" % (m, ms, B))
    assert np.isfinite(m) and np.isfinite(ms)
    with torch.no_grad():
        dh, H = model[1].predict_homography({"pf_hat_12": batch["target"]})      # an exact field: the offsets themselves
    assert np.abs(dh.cpu().numpy() - d["delta"]).max() / np.abs(d["delta"]).max() < 1e-3


@pytest.mark.parametrize("h,w", L.SHAPES)
def test_other_field_shapes(K, h, w):
    """A non-square field and one above 16 384 pixels with a width that does not divide the workgroup's stride: the header handles
    every size (the field is re-read per pass), so both must match the restatement.  So must a field wider than the workgroup
    (3 x 700: the stride of the running (x, y) stays inside one row), one smaller than a wave (5 x 7: no thread takes a second pixel)
    and 37 x 83; delta_hat's band there is 2e-5 px scaled with the corner coordinate (L.dh_atol), the first two keep their 2e-5."""
    B = 2
    dh_atol = 2e-5 if (h, w) in L.SHAPES[:2] else L.dh_atol(h, w)
    pf, mask, start = L.make_shape_inputs(h, w, B)
    dh, H, info = K.homography_refine_lm(dev(pf), dev(start), dev(mask, torch.uint8), L.LM_ITERS)
    torch.cuda.synchronize()
    got = dict(H=H.cpu().numpy(), delta_hat=dh.cpu().numpy(), info=info.cpu().numpy())
    ref = L.lm_reference(pf, start, mask, L.LM_ITERS)
    moved = np.abs(ref["delta_hat"] - L.lm_reference(pf, start, mask, 0)["delta_hat"]).max()
    print("%d x %d: corners moved by %.3e" % (h, w, moved))
    assert moved > 2e-3
    compare(got, ref, "%d x %d" % (h, w), dh_atol)


def test_polish_after_ransac_at_37x83(K):
    """bh_ransac_homography then the polish on R.FIELD_CASES[0] (K = 1100, a field of 3071 pixels), on the GPU's own mask and H."""
    B, _, h, w, thr = R.FIELD_CASES[0]
    ref0 = R.field_case(0)
    g = run(K, ref0["pf"], ref0["choice"], thr=thr)
    ref = L.lm_reference(ref0["pf"], g["H0"], g["mask"], L.LM_ITERS)
    start = L.lm_reference(ref0["pf"], g["H0"], g["mask"], 0)["delta_hat"]
    moved = np.abs(ref["delta_hat"] - start).reshape(B, -1).max(1)
    print("corners moved by the polish (restatement, GPU start):", moved)
    assert (moved >= 2e-3).all()
    compare(g, ref, "37 x 83 after RANSAC", L.dh_atol(h, w))
    assert (g["info"][:, 2] >= 1).all() and (g["H"][:, 2, 2] == 1.0).all()
