"""bh_dsac_score / bh_dsac_scores_bwd on the MI355X against the float64 restatement of tests/test_dsac_scoring_cpu.py (torch
autograd for the adjoint), and the head with SCORING_METHOD 'soft_inliers_ratio' / 'inliers_ratio' against the fixtures the reference's
own modules wrote (tools/make_golden_dsac_scoring.py).

Tolerances of the kernel tests are those of test_head_kernels_gpu.py::test_dsac_scores_fwd_bwd_vs_torch64, whose arithmetic the new
kernels share (fp32 per point, double sums): raw scores 1e-5 relative, softmax weights 2e-4, gradients 2e-3 of their maximum.  Counts
are compared as integers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_dsac_scoring_cpu as S  # noqa: E402

from bihome_amd import configs, synth  # noqa: E402
from bihome_amd.weights import load_synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

THR, BETA = 2.0, 1.5
SHAPES = [(3, 4, 32, 24), (3, 4, 5, 7), (3, 1, 32, 24), (2, 1, 5, 7), (2, 11, 9, 30)]      # (B, n, h, w); the last: n over one workgroup's 8 / 4


def make_inputs(B, n, h, w, seed=4):
    """pf ~ 2 px noise, H = I + 0.01 noise; hypothesis (0, 0) is the identity with pf = 0 at one point (e == 0 exactly); one hypothesis has
    a third row (-0.5, 0, 1): qz == 0 on the column x = 2 (the guard), in fp32 and in float64 alike."""
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    pf = torch.randn(B, 2, h, w, generator=g) * 2.0
    Hd = torch.eye(3).repeat(B, n, 1, 1) + 0.01 * torch.randn(B, n, 3, 3, generator=g)
    Hd[:, :, 2, :2] *= 0.01
    Hd[0, 0] = torch.eye(3)
    pf[0, :, h // 2, w // 3] = 0.0
    gb, gj = (0, 1) if n > 1 else (1, 0)
    Hd[gb, gj, 2] = torch.tensor([-0.5, 0.0, 1.0])
    gs = torch.randn(B, n, generator=g)
    return pf, Hd, gs


def reference(pf, Hd, method, thr=THR, beta=BETA, gs=None):
    """float64: (e [B,n,N], raw [B,n], weights [B,n], g_pf, g_H) - the gradients of sum(weights * gs) by autograd."""
    B, _, h, w = pf.shape
    pf64, H64 = pf.double().requires_grad_(gs is not None), Hd.double().requires_grad_(gs is not None)
    coord = S.lattice(h, w)
    mapf = coord[None] + pf64.reshape(B, 2, -1).permute(0, 2, 1)
    e = S.point_distances(H64, coord, mapf)
    raw = S.raw_scores(e, method, thr, beta)
    wts = S.weights(raw)
    if gs is None:
        return e.detach(), raw.detach(), wts.detach(), None, None
    (wts * gs.double()).sum().backward()
    return e.detach(), raw.detach(), wts.detach(), pf64.grad, H64.grad.reshape(-1, 9)


def flat(Hd):
    return Hd.reshape(-1, 9).cuda().contiguous()


@pytest.mark.parametrize("B,n,h,w", SHAPES)
def test_soft_scores_fwd_bwd_vs_torch64(B, n, h, w):
    from bihome_amd import kernels as K
    pf, Hd, gs = make_inputs(B, n, h, w)
    e, raw, wts, rp, rh = reference(pf, Hd, "soft_inliers_ratio", gs=gs)
    assert (e[0, 0].reshape(h, w)[h // 2, w // 3] == 0).item()                        # the e == 0 point is there
    s, r = K.dsac_scores_fwd(pf.cuda(), flat(Hd), n, "soft_inliers_ratio", THR, BETA)
    print("raw", (r.cpu().double() - raw).abs().max().item() / raw.abs().max().item(), "weights", (s.cpu().double() - wts).abs().max().item())
    assert (r.cpu().double() - raw).abs().max() <= 1e-5 * raw.abs().max()
    assert (s.cpu().double() - wts).abs().max() < 2e-4
    g_pf, g_H = K.dsac_scores_bwd(pf.cuda(), flat(Hd), s, gs.cuda().contiguous(), n, "soft_inliers_ratio", THR, BETA)
    print("g_pf", (g_pf.cpu().double() - rp).abs().max().item() / (rp.abs().max().item() + 1e-300),
          "g_H", (g_H.cpu() - rh).abs().max().item() / (rh.abs().max().item() + 1e-300))
    assert torch.isfinite(g_pf).all() and torch.isfinite(g_H).all()
    assert (g_pf.cpu().double() - rp).abs().max() <= 2e-3 * rp.abs().max() + 1e-9
    assert (g_H.cpu() - rh).abs().max() <= 2e-3 * rh.abs().max() + 1e-9
    if n > 1:
        assert rp.abs().max() > 0 and rh.abs().max() > 0
    _, best = K.dsac_score(pf.cuda(), flat(Hd), n, "soft_inliers_ratio", THR, BETA)
    gap = torch.sort(raw, -1).values
    sure = torch.ones(B, dtype=torch.bool) if n == 1 else (gap[:, 1] - gap[:, 0]) > 1e-4 * raw.abs().max()
    assert torch.equal(best.cpu()[sure], torch.argmin(raw, -1)[sure])


def _clear_inputs(B, n, h, w):
    """Inputs whose float64 distances keep 1e-3 clear of THR: points that come closer get their field moved by 0.01 px."""
    pf, Hd, _ = make_inputs(B, n, h, w)
    for _ in range(20):
        e = reference(pf, Hd, "inliers_ratio")[0]
        near = ((e - THR).abs() <= 1e-3).any(1).reshape(B, h, w)
        if not near.any():
            return pf, Hd, e
        pf[:, 0][near] += 0.01
    raise AssertionError("could not clear the threshold")


@pytest.mark.parametrize("B,n,h,w", SHAPES)
def test_hard_counts_are_exact(B, n, h, w):
    from bihome_amd import kernels as K
    pf, Hd, e = _clear_inputs(B, n, h, w)
    assert ((e - THR).abs() > 1e-3).all()
    cnt = (e < THR).sum(-1)
    r, best = K.dsac_score(pf.cuda(), flat(Hd), n, "inliers_ratio", THR)
    assert np.array_equal(r.cpu().numpy(), cnt.numpy().astype(np.float32) / np.float32(h * w)), (r.cpu() * h * w, cnt)
    assert torch.equal(best.cpu(), torch.argmin(cnt, -1))                           # first minimum: the FEWEST inliers (upstream's quirk)
    s, r2 = K.dsac_scores_fwd(pf.cuda(), flat(Hd), n, "inliers_ratio", THR)
    assert torch.equal(r2, r)
    assert (s.cpu().double() - S.weights(cnt.double() / (h * w))).abs().max() < 2e-4
    with pytest.raises(Exception, match="BH_E_BADARG"):                              # no adjoint
        K.dsac_scores_bwd(pf.cuda(), flat(Hd), s, s, n, "inliers_ratio", THR)


def test_hard_pick_is_the_first_minimum_on_a_tie():
    from bihome_amd import kernels as K
    pf, Hd, _ = _clear_inputs(3, 4, 32, 24)
    Hd[1, 0, :2, 2] += 50.0                                                          # hypotheses 0 and 2 of samples 1 and 2 miss every point:
    Hd[1, 2, :2, 2] += 50.0                                                          # two equal minima, the first one is the pick
    Hd[2, 0, :2, 2] += 50.0
    Hd[2, 2, :2, 2] += 50.0
    e = reference(pf, Hd, "inliers_ratio")[0]
    assert ((e - THR).abs() > 1e-3).all()
    cnt = (e < THR).sum(-1)
    assert cnt[1, 0] == cnt[1, 2] == cnt[1].min() and cnt[2, 0] == cnt[2, 2] == cnt[2].min()
    r, best = K.dsac_score(pf.cuda(), flat(Hd), 4, "inliers_ratio", THR)
    assert np.array_equal(np.rint(r.cpu().numpy() * 768).astype(np.int64), cnt.numpy())
    assert best.cpu()[1].item() == 0 and best.cpu()[2].item() == 0 and torch.equal(best.cpu(), torch.argmin(cnt, -1))


@pytest.mark.parametrize("det", [0, 1])
def test_method_zero_is_repeatable_bitwise(det):
    """Method 0 ('repr_error') of the one pair of entry points, called twice: the same bits (its agreement with the reference is
    test_head_kernels_gpu.py's and the golden tests')."""
    from bihome_amd import _lib
    from bihome_amd import kernels as K
    B, n, h, w = 3, 4, 32, 24
    pf, Hd, gs = make_inputs(B, n, h, w)
    pf, Hf, gs = pf.cuda(), flat(Hd), gs.cuda().contiguous()
    p, st = K._p, K._stream
    err = [torch.empty(B, n, device="cuda") for _ in range(2)]
    best = [torch.empty(B, dtype=torch.int64, device="cuda") for _ in range(2)]
    for i in range(2):
        assert _lib.lib.bh_dsac_score(p(pf), p(Hf), B, n, h, w, 0, 0.0, 0.0, p(err[i]), p(best[i]), st()) == 0
    assert torch.equal(err[0], err[1]) and torch.equal(best[0], best[1])
    s = torch.empty(B, n, device="cuda")
    assert _lib.lib.bh_dsac_scores_fwd(p(err[0]), B, n, p(s), st()) == 0
    outs = []
    for _ in range(2):
        ge, gH, gp = torch.empty(B, n, device="cuda"), torch.empty(B * n, 9, dtype=torch.float64, device="cuda"), torch.zeros_like(pf)
        assert _lib.lib.bh_dsac_scores_bwd(p(pf), p(Hf), p(s), p(gs), B, n, h, w, 0, 0.0, 0.0, p(ge), p(gH), p(gp), det, st()) == 0
        outs.append((ge, gH, gp))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    if det:                                                 # (the default path's float atomics into g_pf are order-dependent by contract)
        assert torch.equal(outs[0][2], outs[1][2])
    else:
        assert (outs[0][2] - outs[1][2]).abs().max() <= 1e-5 * outs[0][2].abs().max()


@pytest.mark.parametrize("B,n,h,w", [(3, 4, 32, 24), (2, 11, 9, 30)])
def test_soft_adjoint_deterministic_flag(B, n, h, w):
    from bihome_amd import kernels as K
    pf, Hd, gs = make_inputs(B, n, h, w)
    pf, Hf, gs = pf.cuda(), flat(Hd), gs.cuda().contiguous()
    s, _ = K.dsac_scores_fwd(pf, Hf, n, "soft_inliers_ratio", THR, BETA)
    with K.det_scope(True):
        a = K.dsac_scores_bwd(pf, Hf, s, gs, n, "soft_inliers_ratio", THR, BETA)
        b = K.dsac_scores_bwd(pf, Hf, s, gs, n, "soft_inliers_ratio", THR, BETA)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with K.det_scope(False):
        c = K.dsac_scores_bwd(pf, Hf, s, gs, n, "soft_inliers_ratio", THR, BETA)
    assert (c[0] - a[0]).abs().max() <= 1e-5 * a[0].abs().max()
    assert (c[1] - a[1]).abs().max() <= 1e-5 * a[1].abs().max()


# ------------------------------------------------------------------------------------------------
# the head against the reference's fixtures
# ------------------------------------------------------------------------------------------------
def cuda(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda()


def relerr(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30)


def _model(cfg):
    from bihome_amd.step import build_model
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    return model


def _config(base, g, method="soft_inliers_ratio", thr="thr", beta="beta"):
    cfg = configs.get(base)
    cfg["MODEL"]["HEAD"].update(RANSAC_HYPOTHESIS_NO=4, POINTS_PER_HYPOTHESIS=16, SCORING_METHOD=method,
                                SCORING_DISTANCE_THRESHOLD=float(g[thr]), SCORING_DISTANCE_BETA=float(g[beta]))
    return cfg


@pytest.mark.parametrize("base,loss_name", [("zeng-ihome", None), ("zeng-multihead", "L1Loss")])
def test_soft_scored_training_vs_golden(golden, base, loss_name):
    """test_branches_gpu.py::test_score_weighted_multi_hypothesis_training_vs_golden with SCORING_METHOD 'soft_inliers_ratio': the same
    assertions and the same bands (measured there against the reference's own float32 / float64 spread), plus the step-0 weights."""
    from bihome_amd.step import build_loss, build_optimizer, mace, train_step
    name = base.replace("-", "_") + "_soft_n4_b4"
    g32, g64 = golden(name + "_f32"), golden(name + "_f64")
    model = _model(_config(base, g64))
    opt, sched = build_optimizer(model, configs.get(base)["SOLVER"])
    loss_fn = build_loss(configs.get(base)["SOLVER"])
    assert isinstance(loss_fn, torch.nn.Module) == (loss_name is not None)
    d = synth.make_pairs(4, seed=19)
    losses, maces = [], []
    for it in range(2):
        data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
        data["choice_12"] = cuda(g64["choice_12"][it], torch.int64)
        if it == 0:
            model.train()
            opt.zero_grad()
            out = model(data)
            loss = loss_fn(out[0], out[1]) if loss_name else out[0]
            dgt, dh = out[-2], out[-1]
            loss.backward()
            scores = model[1].last_scores.cpu().double().numpy()
            print(base, "scores0 max error", np.abs(scores - g64["scores0"]).max(), "reference f32/f64", np.abs(g32["scores0"] - g64["scores0"]).max())
            assert scores.shape == (4, 4) and np.abs(scores - g64["scores0"]).max() <= 2e-3
            params = dict(model[0].named_parameters())
            for k in ("layer1.0.weight", "layer4.6.upper_branch.0.weight", "layer8.3.weight", "layer8.3.bias"):
                gn, ref, sp = params[k].grad.double().norm().item(), g64["gradnorm/" + k], abs(g64["gradnorm/" + k] - g32["gradnorm/" + k])
                print(k, gn, ref, sp)
                assert abs(gn - ref) <= max(5 * sp, 5e-3 * ref), (k, gn, ref, sp)
            opt.step(); sched.step()
            loss, dh = loss.detach(), dh.detach()
            assert dh.shape == (4, 4, 2)
            assert relerr(dh.cpu(), g64["delta_hat_12"]) < 2e-3
        else:
            loss, dgt, dh = train_step(model, data, opt, sched, loss_fn=loss_fn)
        losses.append(loss.item()); maces.append(mace(dgt, dh))
    print(base, "loss", losses, "mace", maces, "ref", g64["loss"], g64["mace"], g32["loss"])
    assert abs(losses[0] - g64["loss"][0]) <= max(3 * abs(g32["loss"][0] - g64["loss"][0]), 2e-4 * abs(g64["loss"][0]))
    assert abs(maces[0] - g64["mace"][0]) < 2e-3
    assert abs(losses[1] - g64["loss"][1]) <= 0.15 * abs(g64["loss"][1]), (losses, g64["loss"], g32["loss"])
    assert abs(maces[1] - g64["mace"][1]) <= 0.15, (maces, g64["mace"], g32["mace"])


@pytest.mark.parametrize("base", ["zeng-ihome", "zeng-multihead"])
@pytest.mark.parametrize("method", ["soft", "hard"])
def test_eval_pick_vs_golden(golden, base, method):
    from bihome_amd.step import predict
    g = golden(base.replace("-", "_") + "_soft_n4_b4_f64")
    cfg = (_config(base, g, "soft_inliers_ratio", "eval_thr_soft", "eval_beta") if method == "soft"
           else _config(base, g, "inliers_ratio", "eval_thr_hard", "eval_beta"))
    model = _model(cfg)
    d = synth.make_pairs(4, seed=19)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
    data["choice"] = cuda(g["eval_choice"], torch.int64)
    dh = predict(model, data)
    raw, best = model[1].last["repr_error"].cpu().double().numpy(), model[1].last["best"].cpu().numpy()
    print(base, method, "raw", raw, "reference", g["eval_raw_" + method], "best", best, g["eval_best_" + method])
    assert np.array_equal(best, g["eval_best_" + method])
    assert dh.shape == (4, 4, 2) and relerr(dh.cpu(), g["eval_delta_hat_" + method]) < 2e-3


def test_single_hypothesis_runs_no_scoring():
    """n == 1: scores stay None whatever the method, and no scoring kernel is called."""
    from bihome_amd import kernels as K
    cfg = configs.get("zeng-ihome")
    cfg["MODEL"]["HEAD"].update(SCORING_METHOD="soft_inliers_ratio", SCORING_DISTANCE_THRESHOLD=1.0, SCORING_DISTANCE_BETA=1.0)
    head = _model(cfg)[1]
    pf = torch.randn(2, 2, 128, 128, device="cuda")
    called = []
    orig = K.dsac_scores_fwd, K.dsac_score
    K.dsac_scores_fwd = K.dsac_score = lambda *a, **k: called.append(a)
    try:
        delta, scores = head._delta_12({"pf_hat_12": pf}, 2)
        dh, _ = head.predict_homography({"pf_hat_12": pf})
    finally:
        K.dsac_scores_fwd, K.dsac_score = orig
    assert scores is None and delta.shape == (2, 4, 2) and dh.shape == (2, 4, 2) and not called
