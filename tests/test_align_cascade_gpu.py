"""Cascaded re-prediction on the device (csrc/cascade.hip: bh_align_prep_warp_u8, bh_patch_ncc; bihome_amd/align.py Aligner(cascade=K))
against the numpy float64 statements of bihome_amd/align.py, which tests/test_align_cascade_cpu.py holds to independent restatements.

Bounds.  Warped preparation: PREP_BOUND, 1e-4 of the output range 1 / std, the project's fp32 bound - the float32 numpy restatement of the
kernel's arithmetic (tests/align_cascade_cases.py prep_warp_f32) stays within 5.1e-5 of the float64 statement on these inputs, and four
times that is below PREP_BOUND = 7.75e-4 (test_align_cascade_cpu.py measures and asserts it).  cover: bit for bit on the patch pixels
none of whose sub-samples' float64 points lies within 1e-3 px of a border line; at most 1e-2 of the patch pixels are excluded (6.6e-3
measured).  Score: the six sums within 1e-10 of the sum of their terms' magnitudes (products of floats are exact in double; at most
2e5 additions at 1.1e-16 each), rho within 1e-6 on inputs whose variance is at least 1 % of their mean square."""
import numpy as np
import pytest
import torch

import align_cascade_cases as Cc
import poisoned_alloc
from bihome_amd import align, configs
from test_align_gpu import N_BIG, StubHead

pytestmark = pytest.mark.gpu

MEAN, STD, PREP_BOUND = Cc.MEAN, Cc.STD, Cc.PREP_BOUND


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ------------------------------------------------------------------------------------------------
# bh_align_prep_warp_u8
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("case", Cc.WARP_CASES, ids=Cc.WARP_IDS)
def test_prep_warp_matches_the_host_statement(monkeypatch, case, C):
    p = poisoned_alloc.poison(monkeypatch, align)          # outputs handed out NaN-filled between red zones
    bank, Hg = Cc.warp_case(*case)
    Ha, Wa, _, _, P, nx, ny = case
    idx = torch.tensor(Cc.IDX, dtype=torch.int32, device="cuda")          # permuted, the last one outside the bank (clamped)
    patch, cover = align.prepare_warped(cuda(bank), cuda(Hg), 3, P, C, nx, ny, MEAN, STD, idx=idx)
    want, want_cover = Cc.warp_reference(case, C)
    assert patch.shape == (3, C, P, P) and patch.dtype == torch.float32 and cover.shape == (3, P, P) and cover.dtype == torch.float32
    err = np.abs(host(patch).astype(np.float64) - want).max()
    near = Cc.near_border(Hg, P, nx, ny, Ha, Wa)
    print("prep_warp %s, C = %d: max |kernel - float64| = %.3e (bound %.3e); cover compared on all but %.2e of the patch pixels, mean %.3f"
          % (case, C, err, PREP_BOUND, near.mean(), want_cover.mean()))
    assert err <= PREP_BOUND
    assert 0.2 < want_cover.mean() < 1.0                                   # (the case shows both sides of the border)
    assert near.mean() <= 1e-2
    assert np.array_equal(host(cover)[~near].view(np.int32), want_cover.astype(np.float32)[~near].view(np.int32))
    assert np.array_equal(host(cover)[~near] == 1.0, want_cover[~near] == 1.0)
    # two calls, equal bits; without cover the same patch
    again, cover2 = align.prepare_warped(cuda(bank), cuda(Hg), 3, P, C, nx, ny, MEAN, STD, idx=idx)
    assert torch.equal(bits(again), bits(patch)) and torch.equal(bits(cover2), bits(cover))
    from bihome_amd import kernels as K
    bare = torch.full((3, C, P, P), float("nan"), dtype=torch.float32, device="cuda")
    K.align_prep_warp_u8(cuda(bank), cuda(Hg), bare, None, nx, ny, MEAN, STD, idx=idx)
    assert torch.equal(bits(bare), bits(patch))
    assert "prepare_warped" in p.callers() and p.verify() == 4            # nothing written outside either output, no NaN left inside
    assert torch.isfinite(patch).all() and torch.isfinite(cover).all()


@pytest.mark.parametrize("C", [1, 3])
def test_identity_at_an_integer_ratio_equals_the_area_average(C):
    img = Cc.pixels(2, 32, 48, seed=5)
    ref, geom = align.prepare(cuda(img), 2, 16, C, MEAN, STD)
    Hg = np.eye(3)[None] @ align.grid_map(host(geom), 3, 2)
    patch, cover = align.prepare_warped(cuda(img), cuda(Hg), 2, 16, C, 3, 2, MEAN, STD)
    err = (patch - ref).abs().max().item()
    print("identity, integer ratio, C = %d: max |prepare_warped - prepare| = %.3e" % (C, err))
    assert err <= PREP_BOUND and torch.equal(cover, torch.ones_like(cover))


def test_outside_the_image_and_under_the_guard():
    img = Cc.pixels(1, 48, 80, seed=6)
    away = np.array([[[1.0, 0, 1000], [0, 1, -1000], [0, 0, 1]]])
    patch, cover = align.prepare_warped(cuda(img), cuda(away), 1, 16, 3, 2, 2, MEAN, STD)
    assert not cover.any()
    assert np.array_equal(host(patch), np.full((1, 3, 16, 16), (np.float32(0) - np.float32(MEAN)) / np.float32(STD), np.float32))
    Hg = np.array([[[1.0, 0, 0], [0, 1, 0], [-0.125, 0, 1]]])             # qz = 1 - X / 8: exactly 0 on grid column 8 (patch column 4 at nx = 2)
    patch, cover = align.prepare_warped(cuda(img), cuda(Hg), 1, 16, 1, 2, 1, MEAN, STD)
    want, want_cover = align.prep_warp_host(img, Hg, 16, 1, 2, 1, MEAN, STD)
    assert not want_cover[0, :, 4].any() and want_cover[0, :, 0].all()
    assert np.array_equal(host(cover), want_cover.astype(np.float32))      # (no point of this map lies within 1e-3 px of a border line without lying on it)
    assert np.abs(host(patch) - want).max() <= PREP_BOUND


def test_offsets_are_64_bit():
    """The smallest bank whose last images start past 2^31 bytes (tests/test_align_gpu.py): an integer translation of a 16 x 16 region at
    one sample per patch pixel reads single pixels, so the result is the preparation of the shifted images."""
    data = torch.randint(0, 256, (N_BIG, 240, 320, 3), dtype=torch.uint8, device="cuda")
    assert data.numel() > 2 ** 31 and 9320 * 230400 < 2 ** 31 <= 9321 * 230400
    idx = torch.tensor([0, 9320, 9321, N_BIG - 1], dtype=torch.int32, device="cuda")
    imgs = host(data[idx.long()])
    shift = np.stack([np.array([[1.0, 0, 4], [0, 1, 2], [0, 0, 1]])] * 4)
    roi = np.array([[100.0, 50.0, 16.0, 16.0]] * 4)
    shifted, _ = align.warp_u8_host(imgs, shift, 240, 320)
    want, geom = align.prep_host(shifted, roi, 16, 3, MEAN, STD)
    patch, cover = align.prepare_warped(data, cuda(shift @ align.grid_map(geom, 1, 1)), 4, 16, 3, 1, 1, MEAN, STD, idx=idx)
    err = np.abs(host(patch).astype(np.float64) - want).max()
    print("prep_warp behind a 2^31-byte offset: max |kernel - float64| = %.3e (bound %.3e)" % (err, PREP_BOUND))
    assert err <= PREP_BOUND and cover.min().item() == 1.0
    assert np.abs(want[1] - want[2]).max() > 1.0                           # (random bytes: an offset that wrapped would show)


# ------------------------------------------------------------------------------------------------
# bh_patch_ncc
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,C", [(16, 1), (48, 3)], ids=["P16-C1-one-element-per-thread", "P48-C3"])
def test_ncc_matches_the_host_statement(monkeypatch, P, C):
    p = poisoned_alloc.poison(monkeypatch, align)
    rs = np.random.RandomState(P)
    w = rs.normal(0.3, 1.0, (3, C, P, P)).astype(np.float32)
    t = (0.5 * w + rs.normal(-0.2, 1.0, (3, C, P, P))).astype(np.float32)
    cover = np.where(rs.uniform(size=(3, P, P)) < 0.2, rs.choice([0.0, 0.5, 0.96875], (3, P, P)), 1.0).astype(np.float32)
    got = host(align.patch_ncc(cuda(w), cuda(t), cuda(cover)))
    want = align.patch_ncc_host(w, t, cover)
    keep = np.broadcast_to((cover == 1.0)[:, None], w.shape)
    w64, t64 = w.astype(np.float64), t.astype(np.float64)
    mags = [keep, np.abs(w64) * keep, np.abs(t64) * keep, w64 * w64 * keep, t64 * t64 * keep, np.abs(w64 * t64) * keep]
    for k, m in enumerate(mags):
        assert np.all(np.abs(got[:, k] - want[:, k]) <= 1e-10 * m.reshape(3, -1).sum(1)), k
    assert 0.7 * C * P * P < want[:, 0].min() and want[:, 0].max() < 0.9 * C * P * P
    for b in range(3):                                                     # the condition under which 1e-6 on rho holds
        n = want[b, 0]
        assert n * want[b, 3] - want[b, 1] ** 2 >= 0.01 * n * want[b, 3] and n * want[b, 4] - want[b, 2] ** 2 >= 0.01 * n * want[b, 4]
    print("ncc P = %d, C = %d: max |rho - host| = %.3e" % (P, C, np.abs(got[:, 6] - want[:, 6]).max()))
    assert np.abs(got[:, 6] - want[:, 6]).max() <= 1e-6 and np.all(got[:, 7] == 0.0)
    # without cover every pixel counts; one sample with fewer than 16 elements, one constant: -inf exactly where the host says so
    few = np.ones((3, P, P), np.float32) * 0.5
    few[0].flat[:15 // C] = 1.0                                            # 15 elements: one short
    few[1].flat[:32] = 1.0
    flat = w.copy()
    flat[2] = 1.25
    for a, b_, c in ((w, t, None), (w, t, few), (flat, t, None), (t, flat, cover)):
        g = host(align.patch_ncc(cuda(a), cuda(b_), None if c is None else cuda(c)))
        h = align.patch_ncc_host(a, b_, c)
        assert np.array_equal(np.isneginf(g[:, 6]), np.isneginf(h[:, 6])) and np.array_equal(g[:, 0], h[:, 0])
        fin = np.isfinite(h[:, 6])
        assert np.abs(g[fin, 6] - h[fin, 6]).max(initial=0.0) <= 1e-6
    assert np.isneginf(align.patch_ncc_host(w, t, few)[:, 6]).tolist() == [True, False, True] and np.isneginf(align.patch_ncc_host(flat, t, None)[:, 6]).tolist() == [False, False, True]
    again = align.patch_ncc(cuda(w), cuda(t), cuda(cover))
    assert np.array_equal(host(again).view(np.int64), got.view(np.int64))   # two calls, equal bits
    assert "patch_ncc" in p.callers() and p.verify() == 6


# ------------------------------------------------------------------------------------------------
# Aligner(cascade=K)
# ------------------------------------------------------------------------------------------------
class SequenceHead(torch.nn.Module):
    """StubHead's idea for several calls: call k returns deltas[k] and the batch it was handed is kept."""

    def __init__(self, deltas):
        super().__init__()
        self.deltas, self.seen = deltas, []

    def predict_homography(self, data):
        self.seen.append(data)
        return self.deltas[len(self.seen) - 1], None


def run_cascade(samples, stages, **kw):
    """The aligner on the pairs of the host runs `samples`, the stub returning their deltas stage by stage."""
    s = samples[0].shape
    deltas = [cuda(np.concatenate([x.deltas[k] for x in samples]), torch.float32) for k in range(stages + 1)]
    head = SequenceHead(deltas)
    aligner = align.Aligner(torch.nn.Sequential(head), patch=s["P"])
    A, B_img = np.concatenate([x.A for x in samples]), np.concatenate([x.B for x in samples])
    r = aligner(cuda(A), cuda(B_img), cascade=stages, warp=False, **kw)
    assert len(head.seen) == stages + 1
    return r, head


def check_stages(r, samples, stages):
    for b, x in enumerate(samples):
        for k in range(stages + 1):
            H, want = host(r["H_stages"][b, k]), x.H[k][0]
            assert np.abs(H - want).max() <= 1e-8 * np.abs(want).max(), (b, k)
        assert np.abs(host(r["score"][b]) - np.array(x.score)).max() <= 1e-4, (b, host(r["score"][b]), x.score)
        assert host(r["accepted"][b]).tolist() == x.accepted, b
        assert np.abs(host(r["H"][b]) - x.best[0]).max() <= 1e-8 * np.abs(x.best[0]).max()
    assert r["H_stages"].shape == (len(samples), stages + 1, 3, 3) and r["delta_stages"].shape == (len(samples), stages + 1, 4, 2)
    assert r["score"].dtype == torch.float64 and r["accepted"].dtype == torch.uint8 and r["score"].shape == r["accepted"].shape


def test_cascade_converges_on_the_true_map():
    x = Cc.cascade_sample(4, 3)
    assert x.accepted == [1, 1, 1, 1] and np.diff(x.score).min() >= 0.02          # on the host: every stage raises the score
    r, head = run_cascade([x], 3)
    check_stages(r, [x], 3)
    assert r["accepted"].all()
    for k in range(3):                                                     # what the model was shown at stage k + 1: A through the best so far
        err = np.abs(host(head.seen[k + 1]["patch_1"]) - x.seen[k]).max()
        print("stage %d: max |patch the model saw - prep_warp_host| = %.3e (bound %.3e)" % (k + 1, err, PREP_BOUND))
        assert err <= PREP_BOUND
        assert head.seen[k + 1]["patch_2"] is r["patch_2"] and torch.equal(head.seen[k + 1]["corners"], head.seen[0]["corners"])
    assert head.seen[0]["patch_1"] is r["patch_1"] and torch.equal(r["delta_hat"], r["delta_stages"][:, 0])
    e0, e = (Cc.corner_error(host(h[0]), x.H_true[0], 120, 160) for h in (r["H_stages"][:, 0], r["H"]))
    print("corner error against H_true: %.2f px after the lift, %.2f px after three stages" % (e0, e))
    assert e < e0
    assert np.abs(host(r["patch_1_warped"]) - align.prep_warp_host(x.A, x.best @ align.grid_map(x.gb, 5, 4), 32, 1, 5, 4, MEAN, STD)[0]).max() <= PREP_BOUND


def test_cascade_rejects_per_sample():
    good, bad = Cc.cascade_sample(4, 2), Cc.cascade_sample(3, 2, garbage=1)
    assert bad.score[1] <= bad.score[0] - 0.02 and bad.accepted == [1, 0, 1] and good.accepted == [1, 1, 1]
    r, head = run_cascade([good, bad], 2)
    check_stages(r, [good, bad], 2)
    assert host(r["accepted"]).tolist() == [[1, 1, 1], [1, 0, 1]]
    s1, s2 = head.seen[1]["patch_1"], head.seen[2]["patch_1"]
    assert torch.equal(bits(s1[1]), bits(s2[1]))                           # sample 1 starts stage 2 again from H_0: the same patch, bit for bit
    assert not torch.equal(s1[0], s2[0])                                   # sample 0 moved on


def test_cascade_min_cover_refuses_a_better_score_on_too_few_pixels():
    x = Cc.cascade_sample(4, 1, min_cover=1.0)
    assert x.accepted == [1, 0] and x.score[1] > x.score[0] + 0.02 and x.count[1] < 32 * 32
    r, _ = run_cascade([x], 1, cascade_min_cover=1.0)
    check_stages(r, [x], 1)
    assert host(r["accepted"]).tolist() == [[1, 0]] and torch.equal(r["H"], r["H_stages"][:, 0])
    r, _ = run_cascade([Cc.cascade_sample(4, 1)], 1)                       # the default share: taken
    assert host(r["accepted"]).tolist() == [[1, 1]]


def test_cascade_defaults_and_arguments(monkeypatch):
    from bihome_amd import kernels as K
    calls = []
    for name in ("align_prep_warp_u8", "patch_ncc", "align_prep_u8"):
        fn = getattr(K, name)
        monkeypatch.setattr(K, name, lambda *a, _fn=fn, _name=name, **k: calls.append(_name) or _fn(*a, **k))
    x = Cc.cascade_sample(4, 1)
    head = StubHead(cuda(x.deltas[0], torch.float32))
    aligner = align.Aligner(torch.nn.Sequential(head), patch=32)
    a, b = cuda(x.A), cuda(x.B)
    for kw in (dict(cascade=-1), dict(cascade=1.5), dict(cascade=1, cascade_samples=(0, 1)), dict(cascade=1, cascade_samples=(1, 9)),
               dict(cascade=1, cascade_min_cover=-0.1), dict(cascade=1, cascade_min_cover=1.01)):
        with pytest.raises(ValueError, match="cascade"):
            aligner(a, b, **kw)
    assert not calls                                                       # every refusal came before any launch
    plain, zero = aligner(a, b), aligner(a, b, cascade=0)
    assert calls == ["align_prep_u8"] * 4                                  # no call to the new wrappers
    assert set(zero) == set(plain) == {"delta_hat", "H", "patch_1", "patch_2", "geom_a", "geom_b", "aligned", "valid"}
    for k in plain:
        assert torch.equal(zero[k], plain[k]), k
    one = aligner(a, b, cascade=1)
    assert calls.count("align_prep_warp_u8") == 2 and calls.count("patch_ncc") == 2
    assert set(one) == set(plain) | {"H_stages", "delta_stages", "score", "accepted", "patch_1_warped"}
    both = aligner(a, b, cascade=1, refine="ecc")
    assert torch.equal(both["H_model"], one["H"]) and torch.equal(both["H_stages"], one["H_stages"])
    assert set(both) == set(one) | {"H_model", "refine_stats", "rho"}
    given = aligner(a, b, cascade=1, cascade_samples=(5, 4), warp=False)   # the default of this shape, spelled out
    assert torch.equal(given["H_stages"], one["H_stages"]) and torch.equal(given["score"], one["score"])


def test_cascade_with_a_real_model():
    from bihome_amd import kernels as K
    from bihome_amd.step import build_model
    from test_align_gpu import textures
    with K.det_scope(True):
        model = build_model(configs.get("zeng-bihome"), "cuda:0")
        aligner = align.Aligner(model, patch=128)
        a, b = cuda(textures(2, 240, 320, seed=1)), cuda(textures(2, 120, 200, seed=2))
        torch.manual_seed(7)
        r = aligner(a, b, cascade=2)
    for k in ("H", "H_stages", "delta_stages", "patch_1_warped", "delta_hat"):
        assert torch.isfinite(r[k]).all(), k
    assert r["H_stages"].shape == (2, 3, 3, 3) and r["patch_1_warped"].shape == (2, 1, 128, 128) and r["aligned"].shape == (2, 120, 200, 3)
    score, acc = host(r["score"]), host(r["accepted"])
    assert acc[:, 0].tolist() == [1, 1] and not np.isnan(score).any()
    for bi in range(2):                                                    # the score of accepted stages never falls
        taken = score[bi][acc[bi] == 1]
        assert np.all(np.diff(taken) > 0), (score[bi], acc[bi])
