"""The trainable projection head of the perceptual loss (AuxiliaryResnet WITH_PROJECTION_HEAD, PerceptualHead.py:41-48,69-74): the
constructor and its validation, the state-dict layout against the reference's (tools/make_golden_projection.py), and the float64
restatement that tests/test_projection_gpu.py measures the kernels against - `project`, `l2n` and the three losses with the unwarped
maps f1 / f2 as differentiable leaves - pinned here against the maps the reference's modules wrote."""
import numpy as np
import pytest
import torch

from test_loss_variants_cpu import HEAD_KW, aware_loss_from_maps, cos, cosine_loss, masked_mean

WIDTHS = [[64, 96], [96, 32]]                  # the fixtures' head
FIXTURES = ["zeng_ihome_proj_b4", "zeng_ihome_cos_proj_n4_b4", "detone_bihome_proj_b4"]


# ------------------------------------------------------------------------------------------------
# the restatement (float64; features NHWC [.., C], channel axis last)
# ------------------------------------------------------------------------------------------------
def project(x, layers):
    """layers: [(W[out,in], b[out]), ...] - Linear, ReLU between the layers (PerceptualHead.py:44-48,69-74)."""
    for i, (W, b) in enumerate(layers):
        x = torch.nn.functional.linear(x, W, b)
        if i != len(layers) - 1:
            x = torch.relu(x)
    return x


def l2n(x):
    """x / |x|_2 over channels, no epsilon (PerceptualHead.py:470-479)."""
    return x / torch.norm(x, p=2, dim=-1, keepdim=True)


def l1_loss(f1, f2, f1w, m1w, margin, rep=1, scores=None, m2=None):
    """The one-line L1 hinge loss (PerceptualHead.py:481-482,505-538): f1 / f2 [B,h,w,C] per sample, f1w [B*rep,h,w,C], m1w [B*rep,h,w]
    -> (loss, per-hypothesis values, t before the hinge)."""
    r = (lambda a: a.repeat_interleave(rep, 0)) if rep > 1 else (lambda a: a)
    t = (f1w - r(f2)).abs().sum(-1) - r((f1 - f2).abs().sum(-1)) + margin
    w = m1w if m2 is None else m1w * r(m2)
    per = masked_mean(w, t.clamp_min(0))
    return (per if scores is None else per * scores).sum(), per, t


def agnostic_loss(f1, f2, f1w, f2w, m1w, m2w, H1, H2, mu, m1=None, m2=None):
    """The double-line loss with a string margin (PerceptualHead.py:559-561,617-620,631-665): no hinge."""
    l3 = (f1 - f2).abs().sum(-1)
    w1, w2 = (m1w if m2 is None else m1w * m2), (m2w if m1 is None else m2w * m1)
    return aware_loss_from_maps((f1w - f2).abs().sum(-1) - l3, (f2w - f1).abs().sum(-1) - l3, w1, w2, H1, H2, mu)


def layers_of(aux, dtype=torch.float64):
    """[(W, b), ...] of an AuxiliaryResnet's projection head (or of the head itself), detached, as `dtype`."""
    ph = getattr(aux, "projection_head", aux)
    return [(ph[i].weight.detach().to(dtype), ph[i].bias.detach().to(dtype)) for i in range(0, len(ph), 2)]


# ------------------------------------------------------------------------------------------------
# constructor, validation, state dict
# ------------------------------------------------------------------------------------------------
def _head(**kw):
    from bihome_amd.heads import PerceptualHead
    return PerceptualHead.Model(None, **dict(HEAD_KW, **kw))


ONE_LINE = dict(TRIPLET_LOSS="one-line", TRIPLET_MARGIN=0.125)


@pytest.mark.parametrize("kw", [dict(ONE_LINE), dict(ONE_LINE, TRIPLET_DISTANCE="cosine"), dict(),
                                dict(TRIPLET_AGGREGATION="channel-aware", TRIPLET_MARGIN=0.5)])
def test_head_accepts_the_projection_head(kw):
    m = _head(WITH_PROJECTION_HEAD=WIDTHS, **kw)
    aux = m.auxiliary_resnet
    assert aux.with_projection_head == WIDTHS and isinstance(aux.projection_head, torch.nn.ModuleList)
    kinds = [type(layer) for layer in aux.projection_head]
    assert kinds == [torch.nn.Linear, torch.nn.ReLU, torch.nn.Linear]
    assert all(p.requires_grad for p in aux.projection_head.parameters())          # trainable ...
    assert not any(p.requires_grad for p in aux.resnet.parameters())               # ... on a frozen extractor (:36-39)


def test_head_without_the_kwarg_owns_an_empty_list_as_upstream():
    m = _head()
    assert m.auxiliary_resnet.with_projection_head is None and len(m.auxiliary_resnet.projection_head) == 0
    assert not [k for k in m.state_dict() if "projection_head" in k]


@pytest.mark.parametrize("name,base", [("zeng-ihome-proj", "zeng-ihome"), ("zeng-ihome-cos-proj", "zeng-ihome-cos"),
                                       ("detone-bihome-proj", "detone-bihome")])
def test_configs_name_the_projection_variants(name, base):
    from bihome_amd import configs, net
    from bihome_amd.step import build_model
    cfg, ref = configs.get(name), configs.get(base)
    assert cfg["MODEL"]["HEAD"].pop("WITH_PROJECTION_HEAD") == [[64, 128], [128, 64]]
    assert cfg == ref
    model = build_model(configs.get(name), "cpu")
    ph = model[1].auxiliary_resnet.projection_head
    assert [tuple(p.shape) for p in ph.parameters()] == [(128, 64), (128,), (64, 128), (64,)]
    # the optimizer's flat buffers cover the projection: one more trainable conv stack whose parameters are exactly the head's
    runners = net.trainable_runners(model)
    mine = [r for r in runners if r.module is ph]
    assert len(mine) == 1 and [id(p) for p in mine[0].flat.params] == [id(p) for p in ph.parameters()]
    assert len(runners) == len(net.trainable_runners(build_model(ref, "cpu"))) + 1


@pytest.mark.parametrize("widths,exc,match", [
    ([[128, 96], [96, 32]], ValueError, r"first layer takes 128 channels.*has 64"),
    ([[64, 96], [64, 32]], ValueError, r"do not chain \(96 outputs into 64 inputs\)"),
    ([[64, 96], [96, 96]], NotImplementedError, r"last width 96.*multiple of 4 whose quarter divides 64 or is at least 64"),
    ([[64, 30], [30, 32]], NotImplementedError, r"hidden width 30.*multiples of 4"),
    ([], NotImplementedError, "PROJECTION_HEAD"),
    ("64x32", NotImplementedError, "PROJECTION_HEAD"),
])
def test_projection_widths_are_validated(widths, exc, match):
    with pytest.raises(exc, match=match):
        _head(WITH_PROJECTION_HEAD=widths)


def test_first_width_follows_the_output_layer():
    m = _head(WITH_PROJECTION_HEAD=[[128, 64]], AUXILIARY_RESNET_OUTPUT_LAYER=2)
    assert [type(layer) for layer in m.auxiliary_resnet.projection_head] == [torch.nn.Linear]
    with pytest.raises(ValueError, match="has 128"):
        _head(WITH_PROJECTION_HEAD=WIDTHS, AUXILIARY_RESNET_OUTPUT_LAYER=2)


def test_multihead_with_a_projection_head_still_raises():
    with pytest.raises(NotImplementedError, match=r"WITH_PROJECTION_HEAD with the multihead.*repeated feature map"):
        _head(TRIPLET_LOSS="", WITH_PROJECTION_HEAD=WIDTHS)
    assert _head(TRIPLET_LOSS="").multihead


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_layout_is_the_references(golden, name):
    g = golden(name + "_f64")
    keys = [str(k) for k in g["sd_keys"]]
    shapes = [tuple(int(v) for v in row if v) for row in g["sd_shapes"]]
    assert keys == ["projection_head.0.weight", "projection_head.0.bias", "projection_head.2.weight", "projection_head.2.bias"]
    m = _head(WITH_PROJECTION_HEAD=WIDTHS, **ONE_LINE)
    own = {k: tuple(v.shape) for k, v in m.auxiliary_resnet.state_dict().items() if k.startswith("projection_head.")}
    assert list(own) == keys and [own[k] for k in keys] == shapes
    assert all("auxiliary_resnet." + k in m.state_dict() for k in keys)


def test_a_state_dict_in_the_reference_layout_loads(golden):
    g = golden(FIXTURES[0] + "_f64")
    gen = torch.Generator().manual_seed(1)
    sd = {str(k): torch.randn(*[int(v) for v in row if v], generator=gen) for k, row in zip(g["sd_keys"], g["sd_shapes"])}
    m = _head(WITH_PROJECTION_HEAD=WIDTHS, **ONE_LINE)
    res = m.load_state_dict({"auxiliary_resnet." + k: v for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if "projection_head" in k]
    for k, v in sd.items():
        assert torch.equal(m.auxiliary_resnet.state_dict()[k], v)
    # and what this build saves is what an upstream module with the same kwargs expects: same names, same shapes
    back = {k: v for k, v in m.state_dict().items() if "projection_head" in k}
    assert sorted(back) == sorted("auxiliary_resnet." + k for k in sd)


def test_sequential_takes_linear_relu_pairs_and_leaves_other_programs_alone():
    """A Linear followed by ReLU is ONE conv op with the activation in its epilogue; programs without such a pair are built as before."""
    from bihome_amd import net
    ph = _head(WITH_PROJECTION_HEAD=[[64, 96], [96, 48], [48, 32]], **ONE_LINE).auxiliary_resnet.projection_head
    prog = net.Program()
    out = prog.sequential(0, ph)
    assert [(op.kind, op.relu, op.mod.out_features) for op in prog.ops] == [("conv", True, 96), ("conv", True, 48), ("conv", False, 32)]
    assert out == 3 and [op.src for op in prog.ops] == [0, 1, 2]
    plain = net.Program()
    plain.sequential(0, [torch.nn.Conv2d(4, 8, 3, 1, 1), torch.nn.BatchNorm2d(8), torch.nn.ReLU(), torch.nn.Conv2d(8, 8, 1)])
    assert [(op.kind, op.relu) for op in plain.ops] == [("conv", False), ("bn", True), ("conv", False)]


# ------------------------------------------------------------------------------------------------
# the restatement against torch and against the reference's fixtures
# ------------------------------------------------------------------------------------------------
def test_l2n_adjoint_is_the_closed_form_the_kernel_uses():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 7, 32, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(5, 7, 32, generator=g, dtype=torch.float64)
    y = l2n(x)
    (gx,) = torch.autograd.grad(y, x, gy)
    inv = 1.0 / x.detach().norm(dim=-1, keepdim=True)
    closed = inv * (gy - y.detach() * (y.detach() * gy).sum(-1, keepdim=True))
    np.testing.assert_allclose(gx.numpy(), closed.numpy(), rtol=1e-12, atol=1e-15)


def _synthetic_layers():
    from bihome_amd.weights import load_synthetic
    aux = _head(WITH_PROJECTION_HEAD=WIDTHS, **ONE_LINE).auxiliary_resnet
    load_synthetic(aux, 0)
    return layers_of(aux)


@pytest.mark.parametrize("name", FIXTURES[:2])
def test_one_line_fixture_maps_restate_the_reference_loss(golden, name):
    g = golden(name + "_f64")
    n = 4 if "n4" in name else 1
    l1, l3, w = (torch.from_numpy(g[k]) for k in ("l1", "l3", "w"))
    assert l1.shape == l3.shape == w.shape == (4 * n, 32, 32)
    margin = float(g["margin"])
    scores = torch.from_numpy(g["scores0"]) if n > 1 else None
    per = masked_mean(w, (l1 - l3 + margin).clamp_min(0))
    loss = (per if scores is None else per * scores).sum()
    assert abs(loss.item() - g["loss"][0]) <= 1e-9 * abs(g["loss"][0])
    share = float(((l1 - l3 + margin) > 0)[w > 0].double().mean())
    assert abs(share - float(g["active_share"])) < 1e-12 and 0.2 <= share <= 0.8
    assert float(golden(name + "_f32")["margin"]) == margin == float(np.float32(margin))
    # project + l2n + the distances from the extractor's features at every 8th pixel, with the weights both sides load by key name
    layers = _synthetic_layers()
    f1, f2, f1w = (l2n(project(torch.from_numpy(g["pre_" + k]), layers)) for k in ("f1", "f2", "f1w"))
    assert f1.shape == (4, 4, 4, 32) and f1w.shape == (4 * n, 4, 4, 32)
    rep = lambda a: a.repeat_interleave(n, 0)
    if "cos" in name:
        d1, d3 = 1 - cos(f1w, rep(f2)), rep(1 - cos(f1, f2))
        _, _, t = cosine_loss(f1, f2, f1w, w[:, ::8, ::8], margin, rep=n)
    else:
        d1, d3 = (f1w - rep(f2)).abs().sum(-1), rep((f1 - f2).abs().sum(-1))
        _, _, t = l1_loss(f1, f2, f1w, w[:, ::8, ::8], margin, rep=n)
    for got, ref in ((d1, l1), (d3, l3), (t - margin, l1 - l3)):
        ref = ref[:, ::8, ::8]
        assert (got - ref).abs().max() <= 1e-9 * ref.abs().max()


def test_double_line_fixture_maps_restate_the_reference_loss(golden):
    g = golden("detone_bihome_proj_b4_f64")
    M1, M2, w1, w2, H1, H2 = (torch.from_numpy(g[k]) for k in ("M1", "M2", "w1", "w2", "H1", "H2"))
    assert M1.shape == M2.shape == w1.shape == w2.shape == (4, 32, 32) and H1.shape == (4, 3, 3)
    from bihome_amd import configs
    mu = configs.get("detone-bihome-proj")["MODEL"]["HEAD"]["TRIPLET_MU"]
    loss = aware_loss_from_maps(M1, M2, w1, w2, H1, H2, mu)
    assert abs(loss.item() - g["loss"][0]) <= 1e-9 * abs(g["loss"][0])
    layers = _synthetic_layers()
    f1, f2, f1w, f2w = (project(torch.from_numpy(g["pre_" + k]), layers) for k in ("f1", "f2", "f1w", "f2w"))       # not normalised
    l3 = (f1 - f2).abs().sum(-1)
    for got, ref in (((f1w - f2).abs().sum(-1) - l3, M1), ((f2w - f1).abs().sum(-1) - l3, M2)):
        ref = ref[:, ::8, ::8]
        assert (got - ref).abs().max() <= 1e-9 * ref.abs().max()
    # the whole-loss restatement on the subsampled maps equals the map form on the same pixels
    sub = lambda a: a[:, ::8, ::8]
    a = agnostic_loss(f1, f2, f1w, f2w, sub(w1), sub(w2), H1, H2, mu)
    b = aware_loss_from_maps(sub(M1), sub(M2), sub(w1), sub(w2), H1, H2, mu)
    assert abs(a.item() - b.item()) <= 1e-9 * abs(b.item())


def test_restated_losses_are_differentiable_in_the_unwarped_maps():
    """f1 / f2 as leaves: what the anchor-adjoint kernels are measured against has a gradient there (it had none to give before)."""
    g = torch.Generator().manual_seed(2)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    f1, f2 = rn(2, 3, 3, 8).requires_grad_(True), rn(2, 3, 3, 8).requires_grad_(True)
    f1w, m = rn(4, 3, 3, 8), torch.rand(4, 3, 3, generator=g, dtype=torch.float64)
    for fn in (l1_loss, cosine_loss):
        loss, _, _ = fn(f1, f2, f1w, m, 0.5, rep=2)
        ga, gb = torch.autograd.grad(loss, (f1, f2))
        assert ga.abs().max() > 0 and gb.abs().max() > 0
