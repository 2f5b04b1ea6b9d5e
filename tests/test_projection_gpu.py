"""The trainable projection head (WITH_PROJECTION_HEAD) on the GPU: bh_l2norm_fwd / _bwd, the anchor adjoints bh_oneline_anchor_bwd /
bh_bihome_anchor_bwd and the projection's conv stack against float64 torch autograd of the restatement that tests/test_projection_cpu.py
pins against the reference's fixtures; the head's chain from the extractor's features to the projection's parameter gradients; two Adam
steps against the fixtures of tools/make_golden_projection.py; HIP-graph capture; the data-parallel reducers' coverage.
Tolerances: 2e-5 of the maximum for the per-pixel kernels (the bound the L1 siblings hold for feature gradients,
tests/test_head_kernels_gpu.py - the same arithmetic class), rtol 2e-5 of the scale for the fp32 dot products of the projection
(tests/test_conv_kernels_gpu.py), 1e-4 of the maximum for the head's chain of several such kernels."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bihome_amd import configs, synth
from bihome_amd.weights import load_synthetic
from test_loss_variants_cpu import HEAD_KW, aware_loss, aware_terms, cosine_loss
from test_loss_variants_gpu import AWARE_MARGIN, COS_MARGIN, FLIP, SHAPES, _close, _cu, _model, aware_inputs, cosine_inputs, relerr
from test_projection_cpu import WIDTHS, agnostic_loss, l1_loss, l2n, layers_of, project

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 0.7                                       # the incoming loss gradient of the kernel tests


def l1_margin(C):
    """|f1w - f2|_1 ~ 0.56 C and |f1 - f2|_1 ~ 1.13 C on cosine_inputs: both hinge states (the margins of test_oneline_hinge_loss_fwd_bwd)."""
    return 0.5625 * C


# ------------------------------------------------------------------------------------------------
# 1. L2 normalisation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hf,C", SHAPES)
def test_l2norm_pair_vs_float64(B, hf, C):
    from bihome_amd import kernels as K
    g = torch.Generator().manual_seed(B * 5 + hf + C)
    x, gy = torch.randn(B, hf, hf, C, generator=g), torch.randn(B, hf, hf, C, generator=g)
    x[0, 0, 0] *= 1e-3                                        # a short vector: a large 1 / |x|
    a = x.double().requires_grad_(True)
    ref = l2n(a)
    (gref,) = torch.autograd.grad(ref, a, gy.double())
    y, inv = K.l2norm_fwd(_cu(x))
    gx = K.l2norm_bwd(_cu(gy), y, inv)
    _close(y, ref.detach(), 2e-5, "y")
    _close(inv, 1.0 / x.double().norm(dim=-1), 2e-5, "inv")
    _close(gx, gref, 2e-5, "gx")
    y2, inv2 = K.l2norm_fwd(_cu(x))
    assert torch.equal(y, y2) and torch.equal(inv, inv2) and torch.equal(gx, K.l2norm_bwd(_cu(gy), y2, inv2))


def test_relu_bwd_masks_by_the_output(shape=(3, 7, 7, 96)):
    from bihome_amd import kernels as K
    g = torch.Generator().manual_seed(1)
    y, gy = torch.randn(*shape, generator=g).clamp_min(0), torch.randn(*shape, generator=g)
    assert torch.equal(K.relu_bwd(_cu(gy), _cu(y)).cpu(), gy * (y > 0))


# ------------------------------------------------------------------------------------------------
# 2. anchor adjoints
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("metric", ["l1", "cosine"])
@pytest.mark.parametrize("B,hf,C", SHAPES)
def test_oneline_anchor_adjoint_vs_float64_autograd(B, hf, C, metric, rep, masks):
    from bihome_amd import kernels as K
    cosine = metric == "cosine"
    f1, f2, f1w, m1w, scores = cosine_inputs(B, hf, C, rep)
    m2 = torch.rand(B, hf, hf, generator=torch.Generator().manual_seed(hf + C)) if masks else None
    margin = COS_MARGIN if cosine else l1_margin(C)
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    s = scores.double() if rep > 1 else None
    ref, _, t = (cosine_loss if cosine else l1_loss)(a, b, f1w.double(), m1w.double(), margin, rep=rep, scores=s,
                                                     m2=None if m2 is None else m2.double())
    (ref * G).backward()
    t = t.detach()
    assert (t > 0).any() and (t < 0).any()                   # both hinge states occur
    dev = [_cu(x) for x in (f1, f2, f1w, m1w)]
    fwd = K.oneline_cos_loss_fwd if cosine else K.oneline_loss_fwd
    loss, T, numden, _ = fwd(*dev, margin, m2=_cu(m2), rep=rep, sample_w=_cu(scores))
    assert abs(loss.item() - ref.item()) <= 2e-5 * abs(ref.item()), (loss.item(), ref.item())
    gl = torch.tensor([G], device="cuda")
    args = dict(m2=_cu(m2), rep=rep, sample_w=_cu(scores), cosine=cosine)
    g1, g2 = K.oneline_anchor_bwd(gl, *dev, T, numden, **args)
    assert g1.shape == f1.shape and g2.shape == f2.shape and torch.isfinite(g1).all() and torch.isfinite(g2).all()
    # not where the float32 indicator of ANY hypothesis of the sample may differ from the float64 one
    keep_h = t.abs() >= FLIP * t.abs().max()
    assert (~keep_h).double().mean() < 0.01
    keep = keep_h.reshape(B, rep, hf, hf).all(1)
    if cosine:
        # the pixel with f2 == 0 carries a gradient of order 1 / eps (the clamped norm's value): on its own, as the f1w == 0 pixel of
        # tests/test_loss_variants_gpu.py
        z = (0, hf - 2, 1)
        if keep[z] and b.grad[z].abs().max() > 0:
            assert b.grad[z].abs().max() > 1e3
            _close(g2[z], b.grad[z], 2e-5, "g_f2 at f2 == 0")
        keep[z] = False
    _close(g1.cpu().double() * keep[..., None], a.grad * keep[..., None], 2e-5, "g_f1")
    _close(g2.cpu().double() * keep[..., None], b.grad * keep[..., None], 2e-5, "g_f2")
    h1, h2 = K.oneline_anchor_bwd(gl, *dev, T, numden, **args)
    assert torch.equal(g1, h1) and torch.equal(g2, h2)        # no atomics: the same bits
    if rep > 1:
        # the hypotheses are added inside the kernel: the sum of `rep` single-hypothesis calls, each on one hypothesis per sample
        s1, s2 = torch.zeros_like(g1), torch.zeros_like(g2)
        for h in range(rep):
            pick = lambda x: x[h::rep].contiguous()
            p1, p2 = K.oneline_anchor_bwd(gl, dev[0], dev[1], pick(dev[2]), pick(dev[3]), pick(T), pick(numden), m2=_cu(m2), rep=1,
                                          sample_w=pick(_cu(scores)), cosine=cosine)
            s1 += p1
            s2 += p2
        if cosine:
            s2[z], g2 = 0, g2.clone()
            g2[z] = 0
        _close(g1, s1.cpu().double(), 2e-5, "g_f1 against the sum of %d single-hypothesis calls" % rep)
        _close(g2, s2.cpu().double(), 2e-5, "g_f2 against the sum of %d single-hypothesis calls" % rep)


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("metric", ["agnostic", "hinge"])
@pytest.mark.parametrize("B,hf,C", SHAPES)
def test_double_line_anchor_adjoint_vs_float64_autograd(B, hf, C, metric, masks):
    from bihome_amd import kernels as K
    hinge = metric == "hinge"
    f1, f2, f1w, f2w, m1w, m2w, m1, m2, dl = aware_inputs(B, hf, C, masks)
    H1, _ = K.h4pt_fwd(_cu(dl), 128)
    H2, _ = K.h4pt_fwd(_cu(-dl.flip(0)), 128)
    mu = 0.01
    d = lambda x: None if x is None else x.double()
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    h1, h2 = (H.cpu().reshape(B, 3, 3) for H in (H1, H2))
    if hinge:
        ref = aware_loss(a, b, d(f1w), d(f2w), d(m1w), d(m2w), h1, h2, AWARE_MARGIN, mu, m1=d(m1), m2=d(m2))
    else:
        ref = agnostic_loss(a, b, d(f1w), d(f2w), d(m1w), d(m2w), h1, h2, mu, m1=d(m1), m2=d(m2))
    (ref * G).backward()
    dev = [_cu(x) for x in (f1, f2, f1w, f2w, m1w, m2w)]
    if hinge:
        M1, M2, nd = K.triplet_hinge_fwd(*dev, AWARE_MARGIN, m1=_cu(m1), m2=_cu(m2))
    else:
        M1, M2, nd = K.triplet_l1_fwd(*dev, m1=_cu(m1), m2=_cu(m2))
    loss4 = K.bihome_loss_fwd(nd, H1, H2, mu)
    assert abs(loss4[0].item() - ref.item()) <= 2e-5 * abs(ref.item()), (loss4[0].item(), ref.item())
    gl = torch.tensor([G], device="cuda")
    kw = dict(m1=_cu(m1), m2=_cu(m2), margin=AWARE_MARGIN if hinge else None)
    g1, g2 = K.bihome_anchor_bwd(gl, *dev, nd, **kw)
    keep = torch.ones_like(a, dtype=torch.bool)
    if hinge:
        # not the pixel-channel terms whose float32 indicator (of either line) may differ from the float64 one
        for t in aware_terms(d(f1), d(f2), d(f1w), d(f2w), AWARE_MARGIN):
            assert 0.1 < (t > 0).double().mean() < 0.9          # both hinge states occur
            keep &= t.abs() >= FLIP * t.abs().max()
        assert (~keep).double().mean() < 0.01
    _close(g1.cpu().double() * keep, a.grad * keep, 2e-5, "g_f1")
    _close(g2.cpu().double() * keep, b.grad * keep, 2e-5, "g_f2")
    out = torch.empty(2 * B, hf, hf, C, device="cuda")
    K.bihome_anchor_bwd(gl, *dev, nd, out=out, **kw)
    assert torch.equal(out[:B], g1) and torch.equal(out[B:], g2)       # the same bits, into the halves of one tensor


# ------------------------------------------------------------------------------------------------
# 3. the projection's conv stack
# ------------------------------------------------------------------------------------------------
def _projection(widths=WIDTHS):
    from bihome_amd.heads import PerceptualHead
    ph = PerceptualHead._ProjectionHead([tuple(w) for w in widths], "f32")
    load_synthetic(ph, 3)
    return ph.cuda().train()


def _scale_close(got, ref, what, rtol=2e-5):
    err, scale = (got.detach().cpu().double() - ref).abs().max().item(), ref.abs().max().item()
    print("  %s: max |err| %.3e = %.2e of max |ref| %.3e (bound %.0e)" % (what, err, err / max(scale, 1e-300), scale, rtol))
    assert err <= rtol * scale, (what, err, scale)


@pytest.mark.parametrize("shape", [(2, 5, 5, 64), (3, 32, 32, 64)])
def test_projection_runner_vs_float64_linear(shape):
    ph = _projection()
    layers = [(W.cpu().requires_grad_(True), b.cpu().requires_grad_(True)) for W, b in layers_of(ph)]
    g = torch.Generator().manual_seed(shape[1])
    total = 0
    for call in range(3):                                     # three calls per step: the weight gradients accumulate
        x, gy = torch.randn(*shape, generator=g), torch.randn(*shape[:3], WIDTHS[-1][1], generator=g)
        xd = x.cuda().requires_grad_(True)
        out = ph(xd)
        out.backward(gy.cuda())
        a = x.double().requires_grad_(True)
        ref = project(a, layers)
        total = total + (ref * gy.double()).sum()
        (ga,) = torch.autograd.grad((ref * gy.double()).sum(), a, retain_graph=True)
        assert out.shape == ref.shape
        _scale_close(out, ref.detach(), "call %d output" % call)
        _scale_close(xd.grad, ga, "call %d input gradient" % call)
    grads = torch.autograd.grad(total, [t for pair in layers for t in pair])
    params = list(ph.parameters())
    flat = ph._runner.flat
    for p, gref, name in zip(params, grads, ("W0", "b0", "W1", "b1")):
        _scale_close(p.grad, gref, "accumulated gradient of " + name)
        lo = flat.flat.data_ptr()
        assert lo <= p.grad.data_ptr() < lo + 4 * flat.flat.numel()           # the gradients live in the runner's flat buffer
    # the hidden activation is rectified in the first conv's epilogue: both signs occur in front of it
    pre = F.linear(torch.randn(*shape, generator=g).double(), layers[0][0].detach(), layers[0][1].detach())
    assert 0.1 < (pre > 0).double().mean() < 0.9


# ------------------------------------------------------------------------------------------------
# 4. the head's chain: features -> projection -> (normalise) -> loss, and back
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["one-line", "double-line"])
def test_head_chain_vs_float64(branch, monkeypatch):
    from bihome_amd.heads import PerceptualHead
    one = branch == "one-line"
    kw = dict(HEAD_KW, WITH_PROJECTION_HEAD=WIDTHS)
    if one:
        kw.update(TRIPLET_LOSS="one-line", TRIPLET_MARGIN=0.125)
    head = PerceptualHead.Model(None, **kw).cuda()
    load_synthetic(head.auxiliary_resnet, 0)
    head.train()
    B = 2
    d = synth.make_pairs(B, seed=3)
    gen = torch.Generator().manual_seed(6)
    data = {k: torch.tensor(d[k]).cuda() for k in ("patch_1", "patch_2", "delta")}
    for key, sign in (("delta_hat_12", 1.0), ("delta_hat_21", -1.0)):
        dh = torch.tensor(sign * d["delta"], dtype=torch.float32) + torch.randn(B, 4, 2, generator=gen) * 2.0
        data[key] = dh.cuda().requires_grad_(True)
    handed = []
    orig = PerceptualHead._extractor_dgrad_into_warp

    def spy(aux, featw, wl, gfeatw, *rest):
        handed.append(gfeatw.detach().clone())
        return orig(aux, featw, wl, gfeatw, *rest)
    monkeypatch.setattr(PerceptualHead, "_extractor_dgrad_into_warp", spy)
    loss = head(data)[0]
    last = dict(head.last)
    loss.backward()
    torch.cuda.synchronize()
    assert len(handed) == 1
    # float64 torch from the head's own pre-projection features and coverage
    aux = head.auxiliary_resnet
    layers = [(W.cpu().requires_grad_(True), b.cpu().requires_grad_(True)) for W, b in layers_of(aux)]
    feat, cov = last["features"].cpu().double(), last["coverage"].cpu().double()
    fw = last["features_warped"].cpu().double().requires_grad_(True)
    assert feat.shape == (2 * B, 32, 32, 64) and fw.shape == ((B if one else 2 * B), 32, 32, 64)
    pa, pw = project(feat, layers), project(fw, layers)
    if one:
        pa, pw = l2n(pa), l2n(pw)
        assert float(torch.norm(project(feat, layers), dim=-1).min().detach()) > 0
        ref, _, t = l1_loss(pa[:B], pa[B:], pw, cov, 0.125)
        share = float((t > 0)[cov > 0].double().mean())
        print("  active share of the hinge:", share)
        assert 0.05 < share < 0.95
    else:
        H = last["H_4pt"].cpu().double().reshape(2 * B, 3, 3)
        ref = agnostic_loss(pa[:B], pa[B:], pw[:B], pw[B:], cov[:B], cov[B:], H[:B], H[B:], kw["TRIPLET_MU"])
    grads = torch.autograd.grad(ref, [fw] + [t for pair in layers for t in pair], retain_graph=True)
    print("  loss hip %.8f float64 %.8f: relative %.2e (bound 2e-5)" % (loss.item(), ref.item(), abs(loss.item() - ref.item()) / abs(ref.item())))
    assert abs(loss.item() - ref.item()) <= 2e-5 * abs(ref.item())
    _close(handed[0], grads[0], 1e-4, "gradient handed to the extractor's dgrad")
    for p, gref, name in zip(aux.projection_head.parameters(), grads[1:], ("W0", "b0", "W1", "b1")):
        assert p.grad is not None
        if name == "b1" and not one:
            # Every term of the un-normalised double-line loss is a difference of two projected maps: the last bias cancels and its
            # gradient is EXACTLY zero - the float64 value is rounding noise and "of its maximum" bounds nothing.  The kernels add the
            # same cancelling terms in fp32: their sum is held to the 2e-5 class of the per-pixel kernels relative to what is added,
            # the per-channel sums of |d loss / d projected map| over both walks.
            ga, gw = torch.autograd.grad(ref, [pa, pw])
            added = (ga.abs().sum((0, 1, 2)) + gw.abs().sum((0, 1, 2))).max().item()
            err = p.grad.abs().max().item()
            print("  gradient of projection b1 (exactly zero): float64 %.2e, hip %.2e, |addends| %.2e -> %.2e of them (bound 2e-5)"
                  % (gref.abs().max().item(), err, added, err / added))
            assert gref.abs().max().item() <= 1e-12 * added and err <= 2e-5 * added
            continue
        _close(p.grad, gref, 1e-4, "gradient of projection " + name)
    assert all(p.grad is None for p in aux.resnet.parameters())


# ------------------------------------------------------------------------------------------------
# 5. two Adam steps against the reference's modules
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,base,n", [("zeng_ihome_proj_b4", "zeng-ihome", 1), ("zeng_ihome_cos_proj_n4_b4", "zeng-ihome-cos", 4),
                                         ("detone_bihome_proj_b4", "detone-bihome", 1)])
def test_head_two_steps_vs_golden(golden, name, base, n):
    """As tests/test_loss_variants_gpu.py::test_head_two_steps_vs_golden, on the fixtures of tools/make_golden_projection.py (head
    [[64, 96], [96, 32]], batch synth.make_pairs(4, seed=23), the recorded DSAC draws, the margin the tool chose)."""
    from bihome_amd.step import build_optimizer, mace, train_step
    g32, g64 = golden(name + "_f32"), golden(name + "_f64")
    cfg = configs.get(base)
    cfg["MODEL"]["HEAD"]["WITH_PROJECTION_HEAD"] = WIDTHS
    if np.isfinite(g64["margin"]):
        cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = float(g64["margin"])
    if n > 1:
        cfg["MODEL"]["HEAD"].update(RANSAC_HYPOTHESIS_NO=n, POINTS_PER_HYPOTHESIS=16)
    model = _model(cfg)
    ph = model[1].auxiliary_resnet.projection_head
    before = [p.detach().clone() for p in ph.parameters()]
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
            assert all(not torch.equal(p.detach(), b) for p, b in zip(ph.parameters(), before))      # the projection trains
    print(name, "loss", losses, "mace", maces, "ref f64", g64["loss"], g64["mace"], "ref f32", g32["loss"])
    sp = np.abs(g32["loss"] - g64["loss"])
    assert abs(losses[0] - g64["loss"][0]) <= max(3 * sp[0], 1e-4 * abs(g64["loss"][0])), (losses, g64["loss"], g32["loss"])
    assert abs(maces[0] - g64["mace"][0]) < 1e-3, (maces, g64["mace"])
    assert abs(losses[1] - g64["loss"][1]) <= max(20 * sp[1], 2e-3 * abs(g64["loss"][1])), (losses, g64["loss"], g32["loss"])


# ------------------------------------------------------------------------------------------------
# 6. HIP-graph capture
# ------------------------------------------------------------------------------------------------
def test_projection_step_under_hip_graph_capture():
    """One B = 2 step of zeng-ihome-proj captured and replayed (no host sync in the new entry points, the projection's gradients in static
    buffers): the replay's loss against the eager step's from the same state, in the band of test_cosine_step_under_hip_graph_capture."""
    from bihome_amd.graph import GraphedStep
    from bihome_amd.step import build_optimizer, train_step
    B = 2
    d = synth.make_pairs(B, seed=21)
    ch = torch.randint(1, 128 * 128, (B, 128), generator=torch.Generator().manual_seed(2)).cuda()

    def batch():
        b = {k: torch.tensor(d[k]).cuda() for k in ("patch_1", "patch_2", "delta")}
        b["choice_12"] = ch
        return b
    cfg = configs.get("zeng-ihome-proj")
    cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = 0.125           # (the fixtures' order of magnitude: at 1.0 the hinge is active everywhere)
    runs = []
    for capturable in (False, True):
        model = _model(cfg)
        ph = model[1].auxiliary_resnet.projection_head
        w0 = ph[0].weight.detach().clone()
        opt, sched = build_optimizer(model, cfg["SOLVER"], capturable=capturable)
        if capturable:
            gs = GraphedStep(model, opt, sched, batch(), warmup=3)
            w3 = ph[0].weight.detach().clone()
            runs.append(gs(batch())[0].item())
            torch.cuda.synchronize()
            assert not torch.equal(ph[0].weight.detach(), w3)          # the replay updates the projection's weights
        else:
            for _ in range(3):
                train_step(model, batch(), opt, sched)
            runs.append(train_step(model, batch(), opt, sched)[0].item())
        assert not torch.equal(ph[0].weight.detach(), w0)
    torch.cuda.synchronize()
    eager, graph = runs
    assert np.isfinite(graph) and abs(graph - eager) <= 0.2 * abs(eager) + 0.3, runs


# ------------------------------------------------------------------------------------------------
# 7. data-parallel reducers cover the projection's buffer
# ------------------------------------------------------------------------------------------------
def test_attach_reducer_covers_the_projection_gradients(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "cover.npz")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "projection_ddp_worker.py"), out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = np.load(out)
    assert int(res["n_reducers"]) == 2 and list(res["deferred"]) == [False, True]       # the backbone's, and the deferred projection's
    assert int(res["n_proj"]) == 4 and float(res["proj_grad_max"]) > 0
    assert res["outside"].size == 0, "gradients outside every reducer's buffer: %s" % list(res["outside"])
    assert res["changed"].size == 0, "a one-rank all-reduce changed: %s" % list(res["changed"])
    assert np.isfinite(float(res["loss"]))
