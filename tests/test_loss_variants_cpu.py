"""The cosine one-line loss (bh_oneline_cos_loss_fwd / _bwd) and the channel-aware margin double-line loss (bh_triplet_hinge_fwd / _bwd):
the float64 restatement that tests/test_loss_variants_gpu.py measures the kernels against - checked here against torch's own
cosine_similarity / clamp autograd and against the fixtures the reference's modules wrote (tools/make_golden_loss_variants.py) - the
head's constructor over every row of the branch table (INTEGRATION.md "PerceptualHead loss branches"), and the new config names."""
import numpy as np
import pytest
import torch

EPS = 1e-8


# ------------------------------------------------------------------------------------------------
# the restatement (float64; features NHWC [.., C], channel axis last)
# ------------------------------------------------------------------------------------------------
def _clamped_norm(x):
    """max(|x|, eps) as torch.cosine_similarity takes it: the VALUE is clamped, the gradient is the unclamped norm's (ATen clamps in
    place under no_grad) - x / |x| also where |x| < eps, and vector_norm's sub-gradient 0 at the zero vector."""
    n = torch.linalg.vector_norm(x, dim=-1)
    return n + (n.detach().clamp_min(EPS) - n.detach())


def cos(x, y):
    """c(x, y) = x.y / (max(|x|, eps) max(|y|, eps)): each norm clamped on its own."""
    return (x * y).sum(-1) / (_clamped_norm(x) * _clamped_norm(y))


def masked_mean(w, v):
    """sum_p w v / max(sum_p w, 1) per sample over [B,h,w] maps."""
    return (w * v).sum((-1, -2)) / w.sum((-1, -2)).clamp_min(1.0)


def cosine_loss_from_maps(c13, c1w, w, margin, scores=None):
    per = masked_mean(w, (c13 - c1w + margin).clamp_min(0))
    return (per if scores is None else per * scores).sum(), per


def cosine_loss(f1, f2, f1w, m1w, margin, rep=1, scores=None, m2=None):
    """f1 / f2 [B,h,w,C] per sample, f1w [B*rep,h,w,C], m1w [B*rep,h,w] -> (loss, per-hypothesis values, t before the hinge)."""
    r = (lambda a: a.repeat_interleave(rep, 0)) if rep > 1 else (lambda a: a)
    c13, c1w = r(cos(f1, f2)), cos(f1w, r(f2))
    w = m1w if m2 is None else m1w * r(m2)
    loss, per = cosine_loss_from_maps(c13, c1w, w, margin, scores)
    return loss, per, c13 - c1w + margin


def aware_terms(f1, f2, f1w, f2w, margin):
    l3 = (f1 - f2).abs()
    return (f1w - f2).abs() - l3 + margin, (f2w - f1).abs() - l3 + margin


def aware_loss_from_maps(M1, M2, w1, w2, H1, H2, mu):
    eye = torch.eye(3, dtype=H1.dtype)
    return masked_mean(w1, M1).sum() + masked_mean(w2, M2).sum() + mu * ((H1 @ H2 - eye) ** 2).sum()


def aware_loss(f1, f2, f1w, f2w, m1w, m2w, H1, H2, margin, mu, m1=None, m2=None):
    t1, t2 = aware_terms(f1, f2, f1w, f2w, margin)
    w1, w2 = (m1w if m2 is None else m1w * m2), (m2w if m1 is None else m2w * m1)
    return aware_loss_from_maps(t1.clamp_min(0).sum(-1), t2.clamp_min(0).sum(-1), w1, w2, H1, H2, mu)


# ------------------------------------------------------------------------------------------------
# the restatement against torch
# ------------------------------------------------------------------------------------------------
def _vectors():
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(12, 16, generator=g, dtype=torch.float64), torch.randn(12, 16, generator=g, dtype=torch.float64)
    x[2] = 0                      # an all-zero x
    y[5] = 0                      # an all-zero y
    x[7] *= 1e-10                 # a pair whose norms are below eps
    y[7] *= 1e-10
    return x, y


def test_cosine_restatement_is_torch_cosine_similarity():
    x, y = _vectors()
    gout = torch.linspace(-1, 1, 12, dtype=torch.float64)
    grads = []
    for fn in (cos, lambda a, b: torch.cosine_similarity(a, b, dim=-1, eps=EPS)):
        a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        c = fn(a, b)
        (c * gout).sum().backward()
        grads.append((c.detach(), a.grad, b.grad))
    (c0, ga0, gb0), (c1, ga1, gb1) = grads
    assert c1[2] == 0 and c1[5] == 0 and torch.isfinite(ga1).all()
    # the zero vector's gradient is y_hat / eps: huge, and exactly that
    np.testing.assert_allclose(ga1[2].numpy(), (gout[2] * y[2] / y[2].norm() / EPS).numpy(), rtol=1e-12)
    for r, t in ((c0, c1), (ga0, ga1), (gb0, gb1)):
        np.testing.assert_allclose(r.numpy(), t.numpy(), rtol=1e-12, atol=1e-300)


def _features(B, rep, hf, C, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    f1, f2 = rn(B, hf, hf, C), rn(B, hf, hf, C)
    f1w = f2.repeat_interleave(rep, 0) + 0.7 * rn(B * rep, hf, hf, C)
    f2w = f1 + 0.7 * rn(B, hf, hf, C)
    m1w, m2w = torch.rand(B * rep, hf, hf, generator=g, dtype=torch.float64), torch.rand(B, hf, hf, generator=g, dtype=torch.float64)
    return f1, f2, f1w, f2w, m1w, m2w


def test_cosine_loss_restatement_is_the_torch_formulation():
    """PerceptualHead.py:498-499,505-511,523-525,538 written with torch's own functions on NCHW tensors, n-fold repeated as upstream."""
    B, n, margin = 2, 3, 0.05
    f1, f2, f1w, _, m1w, _ = _features(B, n, 6, 8, 1)
    on = (cos(f1[0], f2[0]) > 0.1).nonzero()[0]                 # a zero f1w where the hinge is active: t = c13 + margin there
    f1w[0, on[0], on[1]] = 0
    f2[1, 2, 3] = 0
    scores = torch.softmax(torch.randn(B, n, generator=torch.Generator().manual_seed(2), dtype=torch.float64), -1).reshape(-1)
    out = []
    for restated in (True, False):
        a, m, s = f1w.clone().requires_grad_(True), m1w.clone().requires_grad_(True), scores.clone().requires_grad_(True)
        if restated:
            loss, _, _ = cosine_loss(f1, f2, a, m, margin, rep=n, scores=s)
        else:
            nchw = lambda t: t.permute(0, 3, 1, 2)
            p1, p2 = nchw(f1).repeat_interleave(n, 0), nchw(f2).repeat_interleave(n, 0)
            l1 = 1 - torch.cosine_similarity(nchw(a), p2, dim=1)
            l3 = 1 - torch.cosine_similarity(p1, p2, dim=1)
            mat = torch.max(l1 - l3 + torch.ones_like(l1) * margin, torch.zeros_like(l1)) * s.reshape(-1, 1, 1)
            den = m.sum((-1, -2))
            loss = ((m * mat).sum((-1, -2)) / torch.max(den, torch.ones_like(den))).sum()
        loss.backward()
        out.append((loss.detach(), a.grad, m.grad, s.grad))
    for r, t in zip(*out):
        np.testing.assert_allclose(r.numpy(), t.numpy(), rtol=1e-11, atol=1e-14)
    assert out[0][1][0, on[0], on[1]].abs().max() > 1e4      # the 1 / eps gradient of the zero pixel is there


def test_channel_aware_restatement_is_the_torch_formulation():
    """PerceptualHead.py:559-561,615,624-625,631-635,644-645,652-665 with torch.max / torch.sum on NCHW tensors."""
    B, margin, mu = 3, 0.3, 0.01
    f1, f2, f1w, f2w, m1w, m2w = _features(B, 1, 5, 8, 4)
    g = torch.Generator().manual_seed(5)
    H1 = torch.eye(3, dtype=torch.float64) + 0.01 * torch.randn(B, 3, 3, generator=g, dtype=torch.float64)
    H2 = torch.eye(3, dtype=torch.float64) + 0.01 * torch.randn(B, 3, 3, generator=g, dtype=torch.float64)
    out = []
    for restated in (True, False):
        leaves = [t.clone().requires_grad_(True) for t in (f1w, f2w, m1w, m2w, H1, H2)]
        a, b, ma, mb, h1, h2 = leaves
        if restated:
            loss = aware_loss(f1, f2, a, b, ma, mb, h1, h2, margin, mu)
        else:
            nchw = lambda t: t.permute(0, 3, 1, 2)
            l1, l2, l3 = (nchw(a) - nchw(f2)).abs(), (nchw(b) - nchw(f1)).abs(), (nchw(f1) - nchw(f2)).abs()
            lm1 = torch.sum(torch.max(l1 - l3 + margin, torch.zeros_like(l1)), dim=1)
            lm2 = torch.sum(torch.max(l2 - l3 + margin, torch.zeros_like(l2)), dim=1)
            d1, d2 = ma.sum((-1, -2)), mb.sum((-1, -2))
            ln1 = ((ma * lm1).sum((-1, -2)) / torch.max(d1, torch.ones_like(d1))).sum()
            ln2 = ((mb * lm2).sum((-1, -2)) / torch.max(d2, torch.ones_like(d2))).sum()
            loss = ln1 + ln2 + mu * torch.sum((torch.matmul(h1, h2) - torch.eye(3, dtype=torch.float64)) ** 2)
        loss.backward()
        out.append([loss.detach()] + [t.grad for t in leaves])
    for r, t in zip(*out):
        np.testing.assert_allclose(r.numpy(), t.numpy(), rtol=1e-12, atol=1e-15)
    t1, _ = aware_terms(f1, f2, f1w, f2w, margin)
    assert 0.1 < float((t1 > 0).double().mean()) < 0.9     # both hinge states occur


# ------------------------------------------------------------------------------------------------
# the restatement against the reference's fixtures
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zeng_ihome_cos_b4", "zeng_ihome_cos_n4_b4"])
def test_cosine_fixture_maps_restate_the_reference_loss(golden, name):
    g = golden(name + "_f64")
    c13, c1w, w = (torch.from_numpy(g[k]) for k in ("c13", "c1w", "w"))
    n = 4 if "n4" in name else 1
    assert c13.shape == c1w.shape == w.shape == (4 * n, 32, 32)
    scores = torch.from_numpy(g["scores0"]) if n > 1 else None
    loss, _ = cosine_loss_from_maps(c13, c1w, w, float(g["margin"]), scores)
    assert abs(loss.item() - g["loss"][0]) <= 1e-9 * abs(g["loss"][0])
    share = float(((c13 - c1w + float(g["margin"])) > 0)[w > 0].double().mean())
    assert abs(share - float(g["active_share"])) < 1e-12 and 0.2 <= share <= 0.8
    assert float(golden(name + "_f32")["margin"]) == float(g["margin"]) == float(np.float32(g["margin"]))


def test_channel_aware_fixture_maps_restate_the_reference_loss(golden):
    g = golden("detone_bihome_aware_b4_f64")
    M1, M2, w1, w2, H1, H2 = (torch.from_numpy(g[k]) for k in ("M1", "M2", "w1", "w2", "H1", "H2"))
    assert M1.shape == M2.shape == w1.shape == w2.shape == (4, 32, 32) and H1.shape == (4, 3, 3)
    from bihome_amd import configs
    mu = configs.get("detone-bihome-aware")["MODEL"]["HEAD"]["TRIPLET_MU"]
    loss = aware_loss_from_maps(M1, M2, w1, w2, H1, H2, mu)
    assert abs(loss.item() - g["loss"][0]) <= 1e-9 * abs(g["loss"][0])
    assert 0.2 <= float(g["active_share"]) <= 0.8
    assert float(golden("detone_bihome_aware_b4_f32")["margin"]) == float(g["margin"]) == float(np.float32(g["margin"]))


# ------------------------------------------------------------------------------------------------
# the head's constructor: every row of the branch table
# ------------------------------------------------------------------------------------------------
HEAD_KW = dict(PATCH_SIZE=128, PATCH_KEYS=["patch_1", "patch_2"], DELTA_HAT_KEYS=["delta_hat_12", "delta_hat_21"], PF_KEYS=[],
               RANSAC_HYPOTHESIS_NO=-1, POINTS_PER_HYPOTHESIS=-1, AUXILIARY_RESNET="resnet34", AUXILIARY_RESNET_OUTPUT_LAYER=1,
               TRIPLET_LOSS="double-line", TRIPLET_AGGREGATION="channel-agnostic", TRIPLET_MARGIN="inf", TRIPLET_DISTANCE="l1",
               TRIPLET_MU=0.01, MASK_KEYS=[], SAMPLING_STRATEGY="downsample-mask")


def _head(**kw):
    from bihome_amd.heads import PerceptualHead
    return PerceptualHead.Model(None, **dict(HEAD_KW, **kw))


@pytest.mark.parametrize("layer", [1, 2, 3, 4])
def test_head_accepts_the_one_line_cosine_loss(layer):
    m = _head(TRIPLET_LOSS="one-line", TRIPLET_DISTANCE="cosine", TRIPLET_MARGIN=0.25, AUXILIARY_RESNET_OUTPUT_LAYER=layer)
    assert m.one_line and m.triplet_distance == "cosine" and m.triplet_margin == 0.25 and not m.hinge_per_channel
    assert m.auxiliary_resnet.resnet.out_channels == 64 << (layer - 1)


def test_head_accepts_the_channel_aware_numeric_margin():
    m = _head(TRIPLET_AGGREGATION="channel-aware", TRIPLET_MARGIN=0.5)
    assert m.hinge_per_channel and not m.one_line and m.triplet_margin == 0.5
    assert _head(TRIPLET_AGGREGATION="channel-aware", TRIPLET_MARGIN=2).hinge_per_channel


def test_head_runs_the_string_margin_channel_aware_row_on_the_l1_kernels():
    m = _head(TRIPLET_AGGREGATION="channel-aware")
    assert not m.hinge_per_channel and not m.one_line


def test_head_keeps_what_it_built_before():
    assert not _head().hinge_per_channel
    m = _head(TRIPLET_LOSS="one-line", TRIPLET_MARGIN=1.0)
    assert m.one_line and m.triplet_distance == "l1"
    assert _head(TRIPLET_LOSS="", TRIPLET_DISTANCE="anything").multihead


@pytest.mark.parametrize("kw,exc,match", [
    (dict(TRIPLET_DISTANCE="cosine"), NotImplementedError, r"double-line 'cosine'.*image rows.*PerceptualHead\.py"),
    (dict(TRIPLET_DISTANCE="l2"), NotImplementedError, r"double-line 'l2'.*image rows.*PerceptualHead\.py"),
    (dict(TRIPLET_DISTANCE="cosine", TRIPLET_AGGREGATION="channel-aware", TRIPLET_MARGIN=1.0), NotImplementedError, "image rows"),
    (dict(TRIPLET_MARGIN=1.0), NotImplementedError, r"channel-agnostic.*\[64,64\].*PerceptualHead\.py:627-628,646-649"),
    (dict(TRIPLET_AGGREGATION="bogus"), NotImplementedError, "TRIPLET_AGGREGATION"),
    (dict(TRIPLET_DISTANCE="bogus"), NotImplementedError, "TRIPLET_DISTANCE"),
    (dict(TRIPLET_LOSS="one-line", TRIPLET_MARGIN=1.0, TRIPLET_DISTANCE="l2"), NotImplementedError, "one-line 'l2'"),
    (dict(TRIPLET_LOSS="one-line", TRIPLET_MARGIN=1.0, TRIPLET_DISTANCE="bogus"), ValueError, "TRIPLET_DISTANCE"),
    (dict(TRIPLET_LOSS="one-line", TRIPLET_DISTANCE="cosine"), NotImplementedError, "numeric TRIPLET_MARGIN"),
    (dict(TRIPLET_LOSS="one-line", TRIPLET_MARGIN="inf"), NotImplementedError, "numeric TRIPLET_MARGIN"),
    (dict(TRIPLET_LOSS="one-line-dual", TRIPLET_MARGIN=1.0), NotImplementedError, "dual"),
    (dict(TRIPLET_LOSS="double-line-dual"), NotImplementedError, "dual"),
    (dict(MASK_KEYS=["mask_1", "mask_2"]), NotImplementedError, "MASK_KEYS"),
    (dict(MASK_CRD=True), NotImplementedError, "MASK_CRD"),
    (dict(SAMPLING_STRATEGY="upsample-patch-2x"), NotImplementedError, "upsample"),
    (dict(WITH_PROJECTION_HEAD=128), NotImplementedError, "PROJECTION_HEAD"),
])
def test_head_rejects_the_undefined_rows_with_their_reason(kw, exc, match):
    with pytest.raises(exc, match=match):
        _head(**kw)


# ------------------------------------------------------------------------------------------------
# configs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["zeng", "detone"])
def test_configs_name_the_new_variants(base):
    from bihome_amd import configs
    ih, cosv = configs.get(base + "-ihome"), configs.get(base + "-ihome-cos")
    assert cosv["MODEL"]["HEAD"]["TRIPLET_DISTANCE"] == "cosine" and cosv["MODEL"]["HEAD"]["TRIPLET_LOSS"] == "one-line"
    assert cosv["MODEL"]["HEAD"]["TRIPLET_MARGIN"] == 1.0 and cosv["SOLVER"]["LOSS"] == "iHomE"
    cosv["MODEL"]["HEAD"]["TRIPLET_DISTANCE"] = "l1"
    assert cosv == ih
    bi, aw = configs.get(base + "-bihome"), configs.get(base + "-bihome-aware")
    assert aw["MODEL"]["HEAD"]["TRIPLET_AGGREGATION"] == "channel-aware" and aw["MODEL"]["HEAD"]["TRIPLET_MARGIN"] == 1.0
    aw["MODEL"]["HEAD"].update(TRIPLET_AGGREGATION="channel-agnostic", TRIPLET_MARGIN="inf")
    assert aw == bi
    from bihome_amd.step import build_model
    for name in (base + "-ihome-cos", base + "-bihome-aware"):
        head = build_model(configs.get(name), "cpu")[1]
        assert (head.triplet_distance == "cosine") == name.endswith("cos") and head.hinge_per_channel == name.endswith("aware")
