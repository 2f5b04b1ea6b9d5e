"""bh_oneline_cos_loss_fwd / _bwd and bh_triplet_hinge_fwd / _bwd against float64 torch autograd of the restatement that
tests/test_loss_variants_cpu.py pins against torch and the reference's fixtures; the head with TRIPLET_DISTANCE 'cosine' (one-line) and
with a numeric margin + 'channel-aware' (double-line) against the fixtures of tools/make_golden_loss_variants.py, and under HIP-graph
capture.  Tolerances are those of the L1 siblings (tests/test_head_kernels_gpu.py), whose arithmetic class the kernels share: loss 2e-5
relative, feature gradients 2e-5 of their maximum, mask gradients 2e-4 of their maximum, dL/dH 1e-6 relative."""
import numpy as np
import pytest
import torch

from bihome_amd import configs, synth
from bihome_amd.weights import load_synthetic
from test_loss_variants_cpu import aware_loss, aware_terms, cosine_loss

pytestmark = pytest.mark.gpu

# (B, hf, C): the L1 test's three shapes; hw = 25 with LP = 64 lanes per pixel (one pixel per wave pass); two float4 per lane; hw = 25
# with LP = 16 (four pixels per pass, the last pass a quarter full) and with LP = 4 (sixteen per pass, the second pass 9 of 16)
SHAPES = [(3, 32, 64), (2, 8, 128), (1, 16, 64), (2, 5, 256), (2, 4, 512), (2, 5, 64), (2, 5, 16)]
COS_MARGIN, AWARE_MARGIN = 0.8, 0.5          # c1w ~ 0.82, c13 ~ 0 / |f1w - f2| ~ 0.56, |f1 - f2| ~ 1.13 on these inputs: both hinge states
FLIP = 1e-5                                  # |t| below this share of its scale: the float32 indicator may differ from the float64 one


def cosine_inputs(B, hf, C, rep):
    """As test_oneline_hinge_loss_fwd_bwd: two zero rows of m1w, one sample scaled by 1e-4 (the max(den, 1) branch); plus one pixel with
    f1w == 0 and one with f2 == 0 (both in the first, unscaled hypothesis / sample, away from the zero rows)."""
    g = torch.Generator().manual_seed(B * 7 + hf + rep)
    f1, f2 = torch.randn(B, hf, hf, C, generator=g), torch.randn(B, hf, hf, C, generator=g)
    f1w = f2.repeat_interleave(rep, 0) + 0.7 * torch.randn(B * rep, hf, hf, C, generator=g)
    m1w = torch.rand(B * rep, hf, hf, generator=g) * 0.9 + 0.1
    m1w[0, :2] = 0
    if B * rep > 1:
        m1w[1] *= 1e-4
    f1w[0, hf - 1, hf - 1] = 0
    f2[0, hf - 2, 1] = 0
    scores = torch.softmax(torch.randn(B, rep, generator=g), -1).reshape(-1) if rep > 1 else None
    return f1, f2, f1w, m1w, scores


def aware_inputs(B, hf, C, masks):
    g = torch.Generator().manual_seed(B * 11 + hf + int(masks))
    f1, f2 = torch.randn(B, hf, hf, C, generator=g), torch.randn(B, hf, hf, C, generator=g)
    f1w, f2w = f2 + 0.7 * torch.randn(B, hf, hf, C, generator=g), f1 + 0.7 * torch.randn(B, hf, hf, C, generator=g)
    m1w, m2w = torch.rand(B, hf, hf, generator=g), torch.rand(B, hf, hf, generator=g)
    m1w[0, :2] = 0
    m2w[-1] *= 1e-4                                        # denominator below 1: the max(den, 1) branch
    m1, m2 = (torch.rand(B, hf, hf, generator=g), torch.rand(B, hf, hf, generator=g)) if masks else (None, None)
    dl = (torch.rand(B, 4, 2, generator=g) - 0.5) * 16
    return f1, f2, f1w, f2w, m1w, m2w, m1, m2, dl


def _cu(t):
    return None if t is None else t.cuda().contiguous()


def _close(got, ref, rel, what):
    err, scale = (got.cpu().double() - ref).abs().max().item(), ref.abs().max().item()
    print("  %s: max |err| %.3e = %.2e of max |ref| %.3e (bound %.0e)" % (what, err, err / max(scale, 1e-300), scale, rel))
    assert err <= rel * scale, (what, err, scale)


@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("B,hf,C", SHAPES)
def test_cosine_pair_vs_float64_autograd(B, hf, C, rep):
    from bihome_amd import kernels as K
    f1, f2, f1w, m1w, scores = cosine_inputs(B, hf, C, rep)
    a, m = f1w.double().requires_grad_(True), m1w.double().requires_grad_(True)
    s = scores.double().requires_grad_(True) if rep > 1 else None
    ref, per, t = cosine_loss(f1.double(), f2.double(), a, m, COS_MARGIN, rep=rep, scores=s)
    (ref * 0.7).backward()
    t = t.detach()
    assert (t > 0).any() and (t < 0).any()                   # both hinge states occur
    loss, T, numden, perk = K.oneline_cos_loss_fwd(_cu(f1), _cu(f2), _cu(f1w), _cu(m1w), COS_MARGIN, rep=rep, sample_w=_cu(scores))
    assert abs(loss.item() - ref.item()) <= 2e-5 * abs(ref.item()), (loss.item(), ref.item())
    _close(T, t, 2e-5, "T")
    _close(perk, per.detach(), 2e-5, "per-hypothesis loss")      # (d loss / d score_b = loss_b: the head's g_scores)
    if rep > 1:
        _close(perk * 0.7, s.grad, 2e-5, "g_scores")
    gf, gm = K.oneline_cos_loss_bwd(torch.tensor([0.7], device="cuda"), _cu(f2), _cu(f1w), _cu(m1w), T, numden, rep=rep,
                                    sample_w=_cu(scores))
    assert torch.isfinite(gf).all() and torch.isfinite(gm).all()
    _close(gm, m.grad, 2e-4, "g_m1w")
    # the pixel with f1w == 0 carries a gradient of order 1 / eps, the pixels with f2 == 0 exactly none: on their own
    z = (0, hf - 1, hf - 1)
    assert a.grad[z].abs().max() > 1e3
    _close(gf[z], a.grad[z], 2e-5, "g_f1w at f1w == 0")
    for h in range(rep):
        assert a.grad[h, hf - 2, 1].abs().max() == 0 and gf[h, hf - 2, 1].abs().max().item() == 0
    # every other pixel relative to the maximum over those; not where the indicator may flip
    keep = t.abs() >= FLIP * t.abs().max()
    assert (~keep).double().mean() < 0.01
    keep[z] = False
    _close(gf.cpu().double() * keep[..., None], a.grad * keep[..., None], 2e-5, "g_f1w")


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("B,hf,C", SHAPES)
def test_channel_aware_pair_vs_float64_autograd(B, hf, C, masks):
    from bihome_amd import kernels as K
    f1, f2, f1w, f2w, m1w, m2w, m1, m2, dl = aware_inputs(B, hf, C, masks)
    H1, _ = K.h4pt_fwd(_cu(dl), 128)
    H2, _ = K.h4pt_fwd(_cu(-dl.flip(0)), 128)
    mu = 0.01
    d = lambda x: None if x is None else x.double()
    a, b, ma, mb = (x.double().requires_grad_(True) for x in (f1w, f2w, m1w, m2w))
    h1, h2 = (H.cpu().reshape(B, 3, 3).clone().requires_grad_(True) for H in (H1, H2))
    ref = aware_loss(d(f1), d(f2), a, b, ma, mb, h1, h2, AWARE_MARGIN, mu, m1=d(m1), m2=d(m2))
    (ref * 0.7).backward()
    t1, t2 = (x.detach() for x in aware_terms(d(f1), d(f2), a, b, AWARE_MARGIN))
    for t in (t1, t2):
        assert 0.1 < (t > 0).double().mean() < 0.9          # both hinge states occur
    dev = [_cu(x) for x in (f1, f2, f1w, f2w, m1w, m2w)]
    M1, M2, nd = K.triplet_hinge_fwd(*dev, AWARE_MARGIN, m1=_cu(m1), m2=_cu(m2))
    loss4 = K.bihome_loss_fwd(nd, H1, H2, mu)
    assert abs(loss4[0].item() - ref.item()) <= 2e-5 * abs(ref.item()), (loss4[0].item(), ref.item())
    _close(M1, t1.clamp_min(0).sum(-1), 2e-5, "M1")
    _close(M2, t2.clamp_min(0).sum(-1), 2e-5, "M2")
    gf1w, gf2w, gm1w, gm2w, gH1, gH2 = K.triplet_hinge_bwd(torch.tensor([0.7], device="cuda"), *dev, _cu(m1), _cu(m2), M1, M2, nd, H1, H2,
                                                           AWARE_MARGIN, mu)
    for got, leaf, t, what in ((gf1w, a, t1, "g_f1w"), (gf2w, b, t2, "g_f2w")):
        keep = t.abs() >= FLIP * t.abs().max()
        assert (~keep).double().mean() < 0.01
        _close(got.cpu().double() * keep, leaf.grad * keep, 2e-5, what)
    _close(gm1w, ma.grad, 2e-4, "g_m1w")
    _close(gm2w, mb.grad, 2e-4, "g_m2w")
    np.testing.assert_allclose(gH1.cpu().numpy().reshape(B, 3, 3), h1.grad.numpy(), rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(gH2.cpu().numpy().reshape(B, 3, 3), h2.grad.numpy(), rtol=1e-6, atol=1e-10)


def test_deterministic_bit_gives_identical_results():
    """Two calls with the per-call deterministic bit: loss, T / M, the sums and every gradient bit for bit, one shape per pair."""
    from bihome_amd import kernels as K
    B, hf, C = SHAPES[0]
    g = torch.tensor([0.7], device="cuda")
    f1, f2, f1w, m1w, scores = (_cu(x) for x in cosine_inputs(B, hf, C, 3))
    f = [_cu(x) for x in aware_inputs(B, hf, C, True)]
    H, _ = K.h4pt_fwd(f[8], 128)
    runs = []
    with K.det_scope(True):
        for _ in range(2):
            loss, T, nd, per = K.oneline_cos_loss_fwd(f1, f2, f1w, m1w, COS_MARGIN, rep=3, sample_w=scores)
            out = [loss, T, nd, per, *K.oneline_cos_loss_bwd(g, f2, f1w, m1w, T, nd, rep=3, sample_w=scores)]
            M1, M2, nd4 = K.triplet_hinge_fwd(*f[:6], AWARE_MARGIN, m1=f[6], m2=f[7])
            out += [M1, M2, nd4, K.bihome_loss_fwd(nd4, H, H, 0.01)]
            out += list(K.triplet_hinge_bwd(g, *f[:8], M1, M2, nd4, H, H, AWARE_MARGIN, 0.01))
            runs.append(out)
    for x, y in zip(*runs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("metric", ["l1", "hinge"])
def test_double_line_pair_is_symmetric_in_its_lines(metric):
    """Swapping the two images - (f2, f1, f2w, f1w, m2w, m1w, m2, m1) - swaps M1 / M2, the halves of numden and the two directions'
    gradients bit for bit: the adjoint's direction select (the hinge's third operand included) and its batch rotation (B = 3: by 2).
    ln3 = ||H1 H2 - I||^2 is not symmetric: gH stays out."""
    from bihome_amd import kernels as K
    B, hf, C = 3, 5, 64
    f1, f2, f1w, f2w, m1w, m2w, m1, m2, dl = (_cu(x) for x in aware_inputs(B, hf, C, True))
    H, _ = K.h4pt_fwd(dl, 128)
    g = torch.tensor([0.7], device="cuda")
    if metric == "l1":
        fwd = K.triplet_l1_fwd
        bwd = lambda *a: K.bihome_loss_bwd(g, *a, H, H, 0.01)
    else:
        fwd = lambda *a: K.triplet_hinge_fwd(*a[:6], AWARE_MARGIN, *a[6:])
        bwd = lambda *a: K.triplet_hinge_bwd(g, *a, H, H, AWARE_MARGIN, 0.01)
    ab, ba = (f1, f2, f1w, f2w, m1w, m2w, m1, m2), (f2, f1, f2w, f1w, m2w, m1w, m2, m1)
    with K.det_scope(True):
        M1, M2, nd = fwd(*ab)
        N1, N2, ns = fwd(*ba)
        gf1w, gf2w, gm1w, gm2w = bwd(*ab, M1, M2, nd)[:4]
        hf1w, hf2w, hm1w, hm2w = bwd(*ba, N1, N2, ns)[:4]
    assert M1.abs().max() > 0 and gf1w.abs().max() > 0 and gm1w.abs().max() > 0
    assert torch.equal(N1, M2) and torch.equal(N2, M1)
    assert torch.equal(ns[:, :2], nd[:, 2:]) and torch.equal(ns[:, 2:], nd[:, :2])
    assert torch.equal(hf1w, gf2w) and torch.equal(hf2w, gf1w)
    assert torch.equal(hm1w, gm2w) and torch.equal(hm2w, gm1w)


def test_one_line_value_is_the_double_line_first_line():
    """T of the one-line L1 loss at margin 0 is M1 of the double-line one on the same three maps: sum |f1w - f2| - sum |f1 - f2|, summed
    in the same order by the same code."""
    from bihome_amd import kernels as K
    f1, f2, f1w, f2w, m1w, m2w = (_cu(x) for x in aware_inputs(2, 5, 64, False)[:6])
    T = K.oneline_loss_fwd(f1, f2, f1w, m1w, 0.0)[1]
    M1 = K.triplet_l1_fwd(f1, f2, f1w, f2w, m1w, m2w)[0]
    assert T.abs().max() > 0 and torch.equal(T, M1)


def _head_only(aggregation):
    from bihome_amd.heads import PerceptualHead
    kw = dict(configs.get("detone-bihome")["MODEL"]["HEAD"], TRIPLET_AGGREGATION=aggregation)
    head = PerceptualHead.Model(None, **kw).cuda()
    load_synthetic(head.auxiliary_resnet, 0)
    return head.train()


def test_string_margin_channel_aware_is_the_channel_agnostic_loss():
    """PerceptualHead.py:617-620: sum(l1 - l3) against sum(l1) - sum(l3) - the same kernels here."""
    from bihome_amd import kernels as K
    d = synth.make_pairs(2, seed=3)
    g = torch.Generator().manual_seed(6)
    dh = [d["delta"] + np.asarray(torch.randn(2, 4, 2, generator=g)) * 2.0, -d["delta"] + np.asarray(torch.randn(2, 4, 2, generator=g)) * 2.0]
    losses = []
    prev = K.set_deterministic(True)
    try:
        for agg in ("channel-aware", "channel-agnostic"):
            head = _head_only(agg)
            data = {k: torch.tensor(d[k]).cuda() for k in ("patch_1", "patch_2", "delta")}
            data["delta_hat_12"], data["delta_hat_21"] = (torch.tensor(x, dtype=torch.float32).cuda() for x in dh)
            losses.append(head(data)[0].item())
    finally:
        K.set_deterministic(prev)
    assert abs(losses[0] - losses[1]) <= 1e-6 * abs(losses[1]), losses


def relerr(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30)


def _model(cfg):
    from bihome_amd.step import build_model
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    return model


@pytest.mark.parametrize("name,base,n", [("zeng_ihome_cos_b4", "zeng-ihome-cos", 1), ("zeng_ihome_cos_n4_b4", "zeng-ihome-cos", 4),
                                         ("detone_bihome_aware_b4", "detone-bihome-aware", 1)])
def test_head_two_steps_vs_golden(golden, name, base, n):
    """Two Adam steps against the reference's own modules (tools/make_golden_loss_variants.py: batch synth.make_pairs(4, seed=23), the
    recorded DSAC draws, the margin the tool chose): step 0 tight, step 1 - after one update, so it sees the gradients - within a multiple
    of the reference's own float32-vs-float64 spread, the bands of the ihome and variant tests of tests/test_branches_gpu.py."""
    from bihome_amd.step import build_optimizer, mace, train_step
    g32, g64 = golden(name + "_f32"), golden(name + "_f64")
    cfg = configs.get(base)
    cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = float(g64["margin"])
    if n > 1:
        cfg["MODEL"]["HEAD"].update(RANSAC_HYPOTHESIS_NO=n, POINTS_PER_HYPOTHESIS=16)
    model = _model(cfg)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    d = synth.make_pairs(4, seed=23)
    losses, maces = [], []
    for it in range(2):
        data = {k: torch.tensor(d[k]).cuda() for k in ("patch_1", "patch_2", "delta")}
        if "choice_12" in g64 and g64["choice_12"].size:
            data["choice_12"] = torch.tensor(g64["choice_12"][it]).cuda()
        loss, dgt, dh = train_step(model, data, opt, sched)
        losses.append(loss.item()); maces.append(mace(dgt, dh))
        if it == 0:
            ref_dh = g64["delta_hat_12"][0] if g64["delta_hat_12"].ndim == 4 else g64["delta_hat_12"]
            assert dh.shape == (4, 4, 2) and relerr(dh.cpu(), ref_dh) < 1e-3
    print(name, "loss", losses, "mace", maces, "ref f64", g64["loss"], g64["mace"], "ref f32", g32["loss"])
    sp = np.abs(g32["loss"] - g64["loss"])
    assert abs(losses[0] - g64["loss"][0]) <= max(3 * sp[0], 1e-4 * abs(g64["loss"][0])), (losses, g64["loss"], g32["loss"])
    assert abs(maces[0] - g64["mace"][0]) < 1e-3, (maces, g64["mace"])
    assert abs(losses[1] - g64["loss"][1]) <= max(20 * sp[1], 2e-3 * abs(g64["loss"][1])), (losses, g64["loss"], g32["loss"])


def test_cosine_step_under_hip_graph_capture():
    """One B = 2 step of zeng-ihome-cos captured and replayed (no host sync in the new entry points): the replay's loss against the eager
    step's from the same state, in the band tests/test_graph_gpu.py holds non-deterministic replays to."""
    from bihome_amd.graph import GraphedStep
    from bihome_amd.step import build_optimizer, train_step
    B = 2
    d = synth.make_pairs(B, seed=21)
    ch = torch.randint(1, 128 * 128, (B, 128), generator=torch.Generator().manual_seed(2)).cuda()

    def batch():
        b = {k: torch.tensor(d[k]).cuda() for k in ("patch_1", "patch_2", "delta")}
        b["choice_12"] = ch
        return b
    cfg = configs.get("zeng-ihome-cos")
    cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = 0.015625       # (the fixtures' order of magnitude: at 1.0 the hinge is active everywhere)
    runs = []
    for capturable in (False, True):
        model = _model(cfg)
        assert model[1].triplet_distance == "cosine"
        opt, sched = build_optimizer(model, cfg["SOLVER"], capturable=capturable)
        if capturable:
            gs = GraphedStep(model, opt, sched, batch(), warmup=3)
            runs.append(gs(batch())[0].item())
        else:
            for _ in range(3):
                train_step(model, batch(), opt, sched)
            runs.append(train_step(model, batch(), opt, sched)[0].item())
    torch.cuda.synchronize()
    eager, graph = runs
    assert np.isfinite(graph) and abs(graph - eager) <= 0.2 * abs(eager) + 0.3, runs
