"""DSAC inlier-count scoring (bh_dsac_score / bh_dsac_scores_bwd, SCORING_METHOD 'inliers_ratio' / 'soft_inliers_ratio'): the
boundary, the head's kwargs, and the yardstick of tests/test_dsac_scoring_gpu.py - a float64 torch restatement of
DSACSoftmax.__score_hypotheses (ransac_utils.py:76-128), checked here on its own against the fixtures the reference's modules wrote
(tools/make_golden_dsac_scoring.py), together with the conditions that tool promises about them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("zeng_ihome", "zeng_multihead")
HEAD_KW = dict(PATCH_SIZE=128, PATCH_KEYS=["patch_1", "patch_2"], DELTA_HAT_KEYS=[], PF_KEYS=["pf_hat_12"], RANSAC_HYPOTHESIS_NO=4,
               POINTS_PER_HYPOTHESIS=16, AUXILIARY_RESNET="resnet34", AUXILIARY_RESNET_OUTPUT_LAYER=1, TRIPLET_LOSS="one-line",
               TRIPLET_AGGREGATION="channel-agnostic", TRIPLET_MARGIN=1.0, TRIPLET_DISTANCE="l1", TRIPLET_MU=0.01, MASK_KEYS=[],
               SAMPLING_STRATEGY="downsample-mask")


# ------------------------------------------------------------------------------------------------
# the restatement (float64)
# ------------------------------------------------------------------------------------------------
def point_distances(H, coord, mapf):
    """H [B,n,3,3], coord [N,2] or [B,N,2], mapf [B,N,2] -> e [B,n,N]: |transform_points(H, coord) - mapf|_2 with kornia's guard
    (scale 1/z where |z| > 1e-8, else 1)."""
    coord = coord.expand(mapf.shape) if coord.dim() == 2 else coord
    ph = torch.cat([coord, torch.ones_like(coord[..., :1])], -1)
    q = torch.einsum("bnij,bpj->bnpi", H, ph)
    z = q[..., 2:]
    big = z.abs() > 1e-8
    scale = torch.where(big, 1.0 / torch.where(big, z, torch.ones_like(z)), torch.ones_like(z))
    return (q[..., :2] * scale - mapf[:, None]).norm(dim=-1)


def raw_scores(e, method, thr, beta=0.0):
    """:98-111.  'inliers_ratio': the share of points with e < thr; 'soft_inliers_ratio': sum sigmoid(beta (e - thr))."""
    if method == "inliers_ratio":
        return (e < thr).to(e.dtype).mean(-1)
    assert method == "soft_inliers_ratio"
    return torch.sigmoid(beta * (e - thr)).sum(-1)


def weights(raw):
    return torch.softmax(-raw, -1)                  # :126 - the LOWER raw score gets the larger weight, for both methods


def lattice(h, w, dtype=torch.float64):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    return torch.stack([xs.reshape(-1), ys.reshape(-1)], -1)


# ------------------------------------------------------------------------------------------------
# boundary
# ------------------------------------------------------------------------------------------------
def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bihome.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, "include/bihome.h does not declare " + name
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else {"int": ctypes.c_int, "float": ctypes.c_float}[arg.split()[0]])
    return want


@pytest.mark.parametrize("name,nargs", [("bh_dsac_score", 12), ("bh_dsac_scores_bwd", 16)])
def test_header_and_ctypes_signature_agree(name, nargs):
    from bihome_amd import _lib
    want = _prototype(name)
    assert _lib.SIGNATURES[name] == want and len(want) == nargs
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    text = open(os.path.join(ROOT, "include", "bihome.h")).read()
    assert re.search(r"BH_DSAC_REPR_ERROR\s*=\s*0\s*,\s*BH_DSAC_INLIERS\s*=\s*1\s*,\s*BH_DSAC_SOFT_INLIERS\s*=\s*2", text)
    assert _lib.DSAC_METHODS == {"repr_error": 0, "inliers_ratio": 1, "soft_inliers_ratio": 2}


def test_bad_arguments_are_refused_before_any_launch():
    from bihome_amd import _lib
    f, g = _lib.lib.bh_dsac_score, _lib.lib.bh_dsac_scores_bwd
    p = ctypes.c_void_p(64)         # never dereferenced: the argument check comes first
    nan = float("nan")
    for method in (0, 1, 2):
        assert f(p, p, 1, 4, 8, 8, method, nan, 1.0, p, None, None) == -1
        assert f(p, p, 1, 4, 8, 8, method, 1.0, nan, p, None, None) == -1
        assert f(p, p, 1, 4, 8, 8, method, -0.5, 1.0, p, None, None) == -1
        assert f(None, p, 1, 4, 8, 8, method, 1.0, 1.0, p, None, None) == -1
        assert f(p, None, 1, 4, 8, 8, method, 1.0, 1.0, p, None, None) == -1
        assert f(p, p, 1, 4, 8, 8, method, 1.0, 1.0, None, p, None) == -1
        assert f(p, p, 1, 0, 8, 8, method, 1.0, 1.0, p, None, None) == -1                 # n < 1
        assert f(p, p, 0, 4, 8, 8, method, 1.0, 1.0, p, None, None) == 0                  # empty batch: nothing to do
    for method in (-1, 3):
        assert f(p, p, 1, 4, 8, 8, method, 1.0, 1.0, p, None, None) == -1
        assert f(p, p, 0, 4, 8, 8, method, 1.0, 1.0, p, None, None) == -1                 # ... checked before the empty batch returns
        assert g(p, p, p, p, 1, 4, 8, 8, method, 1.0, 1.0, p, p, p, 0, None) == -1
    assert g(p, p, p, p, 1, 4, 8, 8, 1, 1.0, 1.0, p, p, p, 0, None) == -1                 # the hard count has no adjoint
    assert g(p, p, p, p, 0, 4, 8, 8, 1, 1.0, 1.0, p, p, p, 0, None) == -1
    for method in (0, 2):
        assert g(p, p, p, p, 1, 4, 8, 8, method, nan, 1.0, p, p, p, 0, None) == -1
        assert g(p, p, p, p, 1, 4, 8, 8, method, 1.0, nan, p, p, p, 0, None) == -1
        assert g(p, p, p, p, 1, 4, 8, 8, method, -1.0, 1.0, p, p, p, 0, None) == -1
        for k in (0, 1, 2, 3, 11, 12, 13):
            a = [p, p, p, p, 1, 4, 8, 8, method, 1.0, 1.0, p, p, p, 1, None]
            a[k] = None
            assert g(*a) == -1, k
        assert g(p, p, p, p, 0, 4, 8, 8, method, 1.0, 1.0, p, p, p, 1, None) == 0


def test_wrappers_refuse_cpu_tensors_and_unknown_methods():
    from bihome_amd import kernels as K
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.dsac_score(torch.zeros(1, 2, 8, 8), torch.zeros(4, 9), 4, "soft_inliers_ratio", 1.0, 1.0)
    with pytest.raises(ValueError, match="score_cnn"):
        K._dsac_method("score_cnn", 1.0, 1.0)


# ------------------------------------------------------------------------------------------------
# the head's kwargs (these fail on a build without the scorers: every method but 'repr_error' raised NotImplementedError)
# ------------------------------------------------------------------------------------------------
def _head(**kw):
    from bihome_amd.heads import PerceptualHead
    return PerceptualHead.Model(None, **dict(HEAD_KW, **kw))


def test_head_accepts_the_inlier_count_methods():
    m = _head(SCORING_METHOD="inliers_ratio", SCORING_DISTANCE_THRESHOLD=3)
    assert (m.scoring_method, m.scoring_distance_threshold) == ("inliers_ratio", 3.0)
    m = _head(SCORING_METHOD="soft_inliers_ratio", SCORING_DISTANCE_THRESHOLD=2.5, SCORING_DISTANCE_BETA=0.5)
    assert (m.scoring_method, m.scoring_distance_threshold, m.scoring_distance_beta) == ("soft_inliers_ratio", 2.5, 0.5)
    assert _head().scoring_method == "repr_error" and _head(SCORING_METHOD="repr_error").scoring_method == "repr_error"


def test_head_needs_its_threshold_and_beta():
    with pytest.raises(KeyError):
        _head(SCORING_METHOD="inliers_ratio")
    with pytest.raises(KeyError):
        _head(SCORING_METHOD="soft_inliers_ratio", SCORING_DISTANCE_BETA=1.0)
    with pytest.raises(KeyError):
        _head(SCORING_METHOD="soft_inliers_ratio", SCORING_DISTANCE_THRESHOLD=1.0)


def test_head_still_refuses_the_score_cnn_and_double_line_hypotheses():
    with pytest.raises(NotImplementedError, match="score_cnn"):
        _head(SCORING_METHOD="score_cnn", SCORE_CNN_PRETRAINED=False)
    with pytest.raises(ValueError):
        _head(SCORING_METHOD="bogus")


# ------------------------------------------------------------------------------------------------
# the restatement against the reference's fixtures, and what the fixture tool promises
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps(golden):
    return {k: torch.from_numpy(golden("zeng_soft_n4_b4_%s_f64" % k)["map"]) for k in ("map0", "mapeval")}


@pytest.mark.parametrize("base", BASES)
def test_restatement_reproduces_the_reference(golden, maps, base):
    g = golden(base + "_soft_n4_b4_f64")
    coord = lattice(128, 128)
    e0 = point_distances(torch.from_numpy(g["H0"]), coord, maps["map0"])
    w0 = weights(raw_scores(e0, "soft_inliers_ratio", float(g["thr"]), float(g["beta"])))
    assert (w0 - torch.from_numpy(g["scores0"])).abs().max().item() <= 1e-9
    ee = point_distances(torch.from_numpy(g["eval_H"]), coord, maps["mapeval"])
    soft = raw_scores(ee, "soft_inliers_ratio", float(g["eval_thr_soft"]), float(g["eval_beta"]))
    hard = raw_scores(ee, "inliers_ratio", float(g["eval_thr_hard"]))
    assert (weights(soft) - torch.from_numpy(g["eval_scores_soft"])).abs().max().item() <= 1e-9
    assert (soft - torch.from_numpy(g["eval_raw_soft"])).abs().max().item() <= 1e-9 * soft.abs().max().item()
    assert (hard - torch.from_numpy(g["eval_raw_hard"])).abs().max().item() <= 1e-9
    # the pick: argmax of softmax(-score) = the first minimum of the score - for the hard ratio the FEWEST inliers (upstream's quirk)
    assert np.array_equal(torch.argmax(weights(soft), -1).numpy(), g["eval_best_soft"])
    assert np.array_equal(torch.argmax(weights(hard), -1).numpy(), g["eval_best_hard"])
    assert np.array_equal(torch.argmin(hard, -1).numpy(), g["eval_best_hard"])


@pytest.mark.parametrize("base", BASES)
def test_fixture_conditions(golden, maps, base):
    g64, g32 = golden(base + "_soft_n4_b4_f64"), golden(base + "_soft_n4_b4_f32")
    coord = lattice(128, 128)
    for key in ("thr", "beta", "eval_thr_soft", "eval_beta", "eval_thr_hard"):
        assert float(g64[key]) == float(np.float32(g64[key])) == float(g32[key])      # what the device receives is what the reference used
    # the step-0 weights are neither uniform nor one-hot: at least 3 of the 4 samples have their largest in [0.3, 0.97]
    for top in (g64["scores0"].max(-1), g64["eval_scores_soft"].max(-1)):
        assert int(((top >= 0.3) & (top <= 0.97)).sum()) >= 3, top
    e0 = point_distances(torch.from_numpy(g64["H0"]), coord, maps["map0"])
    assert float(g64["thr"]) == float(np.float32(e0.median().item()))
    # the hard pick is well defined for an fp32 device: no distance within 1e-3 of the threshold, every minimal count unique
    ee = point_distances(torch.from_numpy(g64["eval_H"]), coord, maps["mapeval"])
    thr = float(g64["eval_thr_hard"])
    assert (ee - thr).abs().min().item() > 1e-3
    cnt = (ee < thr).sum(-1)
    for b in range(cnt.shape[0]):
        assert int((cnt[b] == cnt[b].min()).sum()) == 1, cnt[b]
    # the soft pick: the two lowest raw scores of every sample are 0.2 apart or more
    raw = torch.sort(torch.from_numpy(g64["eval_raw_soft"]), -1).values
    assert (raw[:, 1] - raw[:, 0]).min().item() >= 0.2
    # and the reference's own float32 run picks the same hypotheses
    for key in ("eval_best_soft", "eval_best_hard", "eval_choice"):
        assert np.array_equal(g32[key], g64[key])
    assert g64["scores0"].shape == (4, 4) and g64["choice_12"].shape == (2, 4, 64) and g64["loss"].shape == (2,)


def test_restatement_guard_and_zero_distance():
    """The two special points of the definition: a vanishing third coordinate (scale 1) and e == 0, whose sub-gradient is 0."""
    H = torch.eye(3, dtype=torch.float64).repeat(1, 2, 1, 1)
    H[0, 1, 2] = torch.tensor([-0.5, 0.0, 1.0], dtype=torch.float64)        # qz = 0 at x = 2
    coord = lattice(2, 4)
    mapf = coord[None].clone().requires_grad_(True)
    e = point_distances(H, coord, mapf)
    assert e[0, 0].abs().max().item() == 0.0                                 # identity on an exact field
    assert e[0, 1, 2].item() == 0.0 and e[0, 1, 3].item() == 9.0             # x = 2: q = (2, 0, 0) kept; x = 3: 3 / -0.5 = -6
    raw_scores(e, "soft_inliers_ratio", 1.0, 2.0).sum().backward()
    assert torch.isfinite(mapf.grad).all() and mapf.grad[0, 0].abs().max().item() == 0.0
