"""Image alignment on the device (csrc/align.hip: bh_align_prep_u8, bh_warp_u8; bihome_amd/align.py Aligner) against the numpy float64
statements of bihome_amd/align.py, which tests/test_align_cpu.py holds to independent restatements.

Bounds.  Preparation: 1e-4 of the output range 1 / std (the project's fp32 bound, test_warp_fwd_bwd).  uint8 warp: no pixel differs by
more than one grey level and at most 1e-3 of the pixels differ at all - a float32 tap against the float64 statement lands on the other
side of a rounding boundary for about one pixel in 10^4 (measured on the host with a float32 numpy restatement of the tap: at most 9e-5
of the pixels at 48 x 80, 240 x 320 and 480 x 640, none by more than 1, no `valid` flag).  `valid` is compared where the float64 point
is at least 1e-3 px from a border line; at most 1e-3 of the pixels may be excluded that way."""
import functools

import numpy as np
import pytest
import torch

import poisoned_alloc
from align_cases import corner_homography, near_border_points, pixels, textures
from bihome_amd import align, configs

pytestmark = pytest.mark.gpu

MEAN, STD = 0.443, 0.129
PREP_BOUND = 1e-4 / STD
N_BIG = 9400        # 240 x 320 x 3 bytes per image: image 9,321 is the first that starts past 2^31 bytes (tests/test_bank_gpu.py)


@functools.lru_cache(maxsize=None)
def prep_reference(n, h, w, P, C, roi=None, order=None):
    imgs = pixels(n, h, w)
    return align.prep_host(imgs if order is None else imgs[list(order)], None if roi is None else np.array(roi), P, C, MEAN, STD)


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def check_u8(got, want, what):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((d.max(-1) > 0).mean())
    print("%s: max |difference| %d grey levels, %.2e of the pixels differ" % (what, d.max(), share))
    assert d.max() <= 1 and share <= 1e-3, (what, int(d.max()), share)


def check_valid(got, want, H, Hs, Ws, what):
    B, Ho, Wo = want.shape
    near = near_border_points(H, Ho, Wo, Hs, Ws, 1e-3)
    print("%s: valid compared on all but %.2e of the pixels" % (what, near.mean()))
    assert near.mean() <= 1e-3, (what, near.mean())
    assert np.array_equal(got[~near], want[~near]), what


# ------------------------------------------------------------------------------------------------
# bh_align_prep_u8
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("h,w,P", [(16, 16, 16), (8, 8, 16), (37, 53, 16), (480, 640, 128)],
                         ids=["16x16-same", "8x8-enlarge", "37x53-odd-width", "480x640-to-128"])
def test_prep_matches_the_host_statement(h, w, P, C):
    patch, geom = align.prepare(cuda(pixels(2, h, w)), 2, P, C, MEAN, STD)
    want, want_geom = prep_reference(2, h, w, P, C)
    assert patch.shape == (2, C, P, P) and patch.dtype == torch.float32 and geom.dtype == torch.float64
    err = np.abs(patch.cpu().numpy().astype(np.float64) - want).max()
    print("prep %dx%d -> %d, C = %d: max |kernel - float64| = %.3e (bound %.3e)" % (h, w, P, C, err, PREP_BOUND))
    assert err <= PREP_BOUND
    assert np.array_equal(geom.cpu().numpy().view(np.int64), want_geom.view(np.int64))          # bitwise


ROIS = ((3.25, 2.5, 41.5, 30.25), (0.0, 0.0, 53.0, 37.0), (10.125, 7.75, 16.0, 16.5))


@pytest.mark.parametrize("C", [1, 3])
def test_prep_regions_and_a_permuted_index(monkeypatch, C):
    p = poisoned_alloc.poison(monkeypatch, align)          # outputs handed out NaN-filled between red zones
    imgs, order = cuda(pixels(4, 37, 53)), (2, 0, 3)
    idx = torch.tensor(order, dtype=torch.int32, device="cuda")
    roi = cuda(np.array(ROIS))
    patch, geom = align.prepare(imgs, 3, 16, C, MEAN, STD, idx=idx, roi=roi)
    want, want_geom = prep_reference(4, 37, 53, 16, C, roi=ROIS, order=order)
    err = np.abs(patch.cpu().numpy().astype(np.float64) - want).max()
    print("prep regions, C = %d: max |kernel - float64| = %.3e (bound %.3e)" % (C, err, PREP_BOUND))
    assert err <= PREP_BOUND
    assert np.array_equal(geom.cpu().numpy().view(np.int64), want_geom.view(np.int64))
    again, geom2 = align.prepare(imgs, 3, 16, C, MEAN, STD, idx=idx, roi=roi)
    assert torch.equal(again, patch) and torch.equal(geom2, geom)                               # two calls, equal bits
    assert "prepare" in p.callers() and p.verify() == 4                                         # nothing written outside either output


def test_prep_clamps_the_index_and_what_it_derives_from_a_region():
    """An index outside the bank reads its first / last image; a region that leaves the image reads inside it - pixels outside weigh 0,
    which is what the host statement (it does not range-check) gives as well."""
    imgs = cuda(pixels(4, 37, 53))
    wild = torch.tensor([-1, 4, 2, -2147483648], dtype=torch.int32, device="cuda")
    patch, _ = align.prepare(imgs, 4, 16, 3, MEAN, STD, idx=wild)
    want, _ = prep_reference(4, 37, 53, 16, 3, order=(0, 3, 2, 0))
    assert np.abs(patch.cpu().numpy() - want).max() <= PREP_BOUND
    outside = ((-5.5, -3.25, 80.0, 60.0), (40.0, 30.0, 32.0, 16.0))
    patch, _ = align.prepare(imgs, 2, 16, 1, MEAN, STD, roi=cuda(np.array(outside)))
    want, _ = prep_reference(4, 37, 53, 16, 1, roi=outside, order=(0, 1))
    assert np.abs(patch.cpu().numpy() - want).max() <= PREP_BOUND


# ------------------------------------------------------------------------------------------------
# bh_warp_u8
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hs,Ws,Ho,Wo", [(17, 23, 17, 23), (48, 80, 48, 80), (240, 320, 240, 320), (48, 80, 40, 56)],
                         ids=["17x23-scalar", "48x80", "240x320", "48x80-onto-40x56"])
def test_warp_matches_the_host_statement(monkeypatch, Hs, Ws, Ho, Wo):
    p = poisoned_alloc.poison(monkeypatch, align)          # outputs handed out 1-filled between red zones
    imgs = textures(2, Hs, Ws)
    H = np.stack([corner_homography(11 + b, Hs, Ws, Ho, Wo) for b in range(2)])
    out, valid = align.warp_u8(cuda(imgs), cuda(H), Ho, Wo)
    assert out.shape == (2, Ho, Wo, 3) and out.dtype == torch.uint8 and valid.shape == (2, Ho, Wo) and valid.dtype == torch.uint8
    want, want_valid = align.warp_u8_host(imgs, H, Ho, Wo)
    what = "warp %dx%d onto %dx%d" % (Hs, Ws, Ho, Wo)
    check_u8(out.cpu().numpy(), want, what)
    check_valid(valid.cpu().numpy(), want_valid, H, Hs, Ws, what)
    assert 0.2 < want_valid.mean() < 1.0                                  # (the case shows both sides of the border)
    again, valid2 = align.warp_u8(cuda(imgs), cuda(H), Ho, Wo)
    assert torch.equal(again, out) and torch.equal(valid2, valid)          # two calls, equal bits
    only, none = align.warp_u8(cuda(imgs), cuda(H), Ho, Wo, want_valid=False)
    assert none is None and torch.equal(only, out)
    assert "warp_u8" in p.callers() and p.verify() == 5


@pytest.mark.parametrize("h,w", [(17, 23), (48, 80)], ids=["17x23-scalar", "48x80-vector"])
def test_warp_exact_cases_are_bitwise(h, w):
    imgs = textures(2, h, w)
    shift = np.array([[1.0, 0, 5], [0, 1, -3], [0, 0, 1]])
    H = np.stack([np.eye(3), shift])
    out, valid = (t.cpu().numpy() for t in align.warp_u8(cuda(imgs), cuda(H), h, w))
    want, want_valid = align.warp_u8_host(imgs, H, h, w)
    assert np.array_equal(out, want) and np.array_equal(valid, want_valid)
    assert np.array_equal(out[0], imgs[0]) and valid[0].all()
    moved, inside = np.zeros_like(imgs[1]), np.zeros((h, w), np.uint8)
    moved[3:, :w - 5], inside[3:, :w - 5] = imgs[1, :h - 3, 5:], 1
    assert np.array_equal(out[1], moved) and np.array_equal(valid[1], inside)
    # an index list: sample 0 takes image 1, sample 1 image 0 (and an index outside the bank is clamped into it)
    swapped, _ = align.warp_u8(cuda(imgs), cuda(np.stack([np.eye(3)] * 3)), h, w, idx=torch.tensor([1, 0, 7], dtype=torch.int32, device="cuda"))
    assert np.array_equal(swapped.cpu().numpy(), imgs[[1, 0, 1]])


def test_warp_where_the_denominator_vanishes():
    imgs = textures(1, 48, 80)
    H = np.array([[[1.0, 0, 0], [0, 1, 0], [-0.125, 0, 1]]])              # qz = 1 - x / 8: exactly 0 on the column x = 8
    out, valid = (t.cpu().numpy() for t in align.warp_u8(cuda(imgs), cuda(H), 48, 80))
    want, want_valid = align.warp_u8_host(imgs, H, 48, 80)
    assert out.dtype == np.uint8 and not valid[0, :, 8].any() and not want_valid[0, :, 8].any()
    assert valid[0, :, 0].all()                                            # x = 0: the identity
    keep = np.ones((48, 80), bool)
    keep[:, 8] = False                                                     # (under the guard the value is unspecified, the flag is not)
    check_u8(out[0][keep], want[0][keep], "vanishing denominator")
    assert np.array_equal(valid, want_valid)          # (no projected point of this map lies within 1e-3 px of a border line without lying on it)


def test_offsets_are_64_bit():
    """Both kernels on the smallest bank whose last images start past 2^31 bytes: a 32-bit byte offset reads image 9,321 from the wrong
    place.  The warp is an integer translation, so its comparison is bitwise."""
    data = torch.randint(0, 256, (N_BIG, 240, 320, 3), dtype=torch.uint8, device="cuda")
    assert data.numel() > 2 ** 31 and 9320 * 230400 < 2 ** 31 <= 9321 * 230400
    idx = torch.tensor([0, 9320, 9321, N_BIG - 1], dtype=torch.int32, device="cuda")
    host = data[idx.long()].cpu().numpy()
    patch, _ = align.prepare(data, 4, 16, 3, MEAN, STD, idx=idx)
    want, _ = align.prep_host(host, None, 16, 3, MEAN, STD)
    err = np.abs(patch.cpu().numpy().astype(np.float64) - want).max()
    print("prep behind a 2^31-byte offset: max |kernel - float64| = %.3e (bound %.3e)" % (err, PREP_BOUND))
    assert err <= PREP_BOUND
    H = np.stack([np.array([[1.0, 0, 4], [0, 1, 2], [0, 0, 1]])] * 4)
    out, valid = align.warp_u8(data, cuda(H), 240, 320, idx=idx)
    want, want_valid = align.warp_u8_host(host, H, 240, 320)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), want_valid)
    assert not np.array_equal(want[1], want[2])                            # (random bytes: an offset that wrapped would show)


# ------------------------------------------------------------------------------------------------
# Aligner
# ------------------------------------------------------------------------------------------------
class StubHead(torch.nn.Module):
    """A 'model' whose prediction is given: predict_homography returns (delta_hat, None) and keeps the batch it was handed."""

    def __init__(self, delta):
        super().__init__()
        self.delta, self.seen = delta, None

    def predict_homography(self, data):
        self.seen = data
        return self.delta, None


def region_geom(roi, P):
    x0, y0, rw, rh = roi
    sx, sy = rw / P, rh / P
    return np.array([[sx, sy, x0 + 0.5 * sx - 0.5, y0 + 0.5 * sy - 0.5]])


@pytest.mark.parametrize("size_b,roi_a", [((240, 320), None), ((120, 200), (20.5, 10.25, 256.0, 200.0))],
                         ids=["equal-sizes", "240x320-region-and-120x200"])
def test_direction_and_lift_end_to_end(size_b, roi_a):
    """A is a texture and B = warp_u8_host(A, H_true); the stub model returns the delta that `lift` maps to H_true, solved on the host in
    float64.  A model's delta_hat is float32, so H_true is built from a delta on a 1/16-pixel grid: the solved delta then IS a float32
    number to 1e-12 and the 1e-8 below measures the device lift, not the rounding of its input."""
    P, (Ha, Wa), (Hb, Wb) = 128, (240, 320), size_b
    A = textures(1, Ha, Wa, seed=5)
    ga = region_geom((0.0, 0.0, Wa, Ha) if roi_a is None else roi_a, P)
    gb = region_geom((0.0, 0.0, Wb, Hb), P)
    delta0 = np.round(np.random.RandomState(3).uniform(-0.12 * P, 0.12 * P, (1, 4, 2)) * 16) / 16
    H_true = align.lift(delta0, P, ga, gb)
    B_img, B_valid = align.warp_u8_host(A, H_true, Hb, Wb)
    # solve delta from H_true: H_p = A_a^-1 H_true A_b, delta_i = H_p(c_i) - c_i
    Hp = np.linalg.inv(align._affine(ga)[0]) @ H_true[0] @ align._affine(gb)[0]
    c = align.patch_corners(P)
    q = np.concatenate([c, np.ones((4, 1))], 1) @ Hp.T
    delta = q[:, :2] / q[:, 2:] - c
    assert np.abs(delta - delta0[0]).max() < 1e-9
    head = StubHead(cuda(delta[None], torch.float32))
    aligner = align.Aligner(torch.nn.Sequential(head), patch=P)
    r = aligner(cuda(A), cuda(B_img), roi_a=roi_a)
    assert set(head.seen) >= {"patch_1", "patch_2", "corners"} and head.seen["patch_1"].shape == (1, 1, P, P)
    assert head.seen["corners"].cpu().tolist() == [[[0, 0], [P, 0], [P, P], [0, P]]]
    H = r["H"].cpu().numpy()
    rel = np.abs(H - H_true).max() / np.abs(H_true).max()
    print("lift: max |H - H_true| / max |H_true| = %.3e" % rel)
    assert r["H"].dtype == torch.float64 and H[0, 2, 2] == 1.0 and rel <= 1e-8
    assert np.array_equal(r["geom_a"].cpu().numpy(), ga) and np.array_equal(r["geom_b"].cpu().numpy(), gb)
    want_p1, _ = align.prep_host(A, None if roi_a is None else [roi_a], P, 1, MEAN, STD)
    assert np.abs(r["patch_1"].cpu().numpy() - want_p1).max() <= PREP_BOUND
    assert r["aligned"].shape == (1, Hb, Wb, 3) and r["valid"].shape == (1, Hb, Wb)
    check_u8(r["aligned"].cpu().numpy(), B_img, "aligned")
    check_valid(r["valid"].cpu().numpy(), B_valid, H_true, Ha, Wa, "aligned")
    assert 0.2 < B_valid.mean() < 1.0
    bare = aligner(cuda(A), cuda(B_img), roi_a=roi_a, warp=False)
    assert "aligned" not in bare and "valid" not in bare and torch.equal(bare["H"], r["H"])


@pytest.mark.parametrize("name", ["zeng-bihome", "detone-orig"], ids=["zeng-bihome", "detone-orig-NoOpHead-4_points"])
def test_aligner_runs_the_models_own_chain(name):
    """delta_hat is step.predict's on the patches the aligner made, bit for bit (deterministic launches; the head's point draws come from
    the default device generator, seeded alike before both calls).  NoOpHead '4_points' needs the 'corners' the aligner supplies."""
    from bihome_amd import kernels as K
    from bihome_amd.step import build_model, predict
    with K.det_scope(True):
        model = build_model(configs.get(name), "cuda:0")
        aligner = align.Aligner(model, patch=128)
        assert (aligner.patch, aligner.channels) == (128, 1)
        a, b = cuda(textures(2, 240, 320, seed=1)), cuda(textures(2, 120, 200, seed=2))
        torch.manual_seed(7)
        r = aligner(a, b)
        corners = torch.tensor([[0, 0], [128, 0], [128, 128], [0, 128]], dtype=torch.float32, device="cuda").repeat(2, 1, 1)
        torch.manual_seed(7)
        d = predict(model, {"patch_1": r["patch_1"], "patch_2": r["patch_2"], "corners": corners})
    assert r["delta_hat"].shape == (2, 4, 2) and torch.equal(r["delta_hat"], d.reshape(2, 4, 2))
    assert torch.isfinite(r["delta_hat"]).all()
    assert r["H"].shape == (2, 3, 3) and r["aligned"].shape == (2, 120, 200, 3) and r["valid"].shape == (2, 120, 200)
    want, _ = align.prep_host(textures(2, 120, 200, seed=2), None, 128, 1, MEAN, STD)
    assert np.abs(r["patch_2"].cpu().numpy() - want).max() <= PREP_BOUND


def test_aligner_argument_checks(monkeypatch):
    from bihome_amd import kernels as K
    from bihome_amd.bank import ImageBank
    launches = []
    prep = K.align_prep_u8
    monkeypatch.setattr(K, "align_prep_u8", lambda *a, **k: launches.append(1) or prep(*a, **k))
    head = StubHead(torch.zeros(2, 4, 2, device="cuda"))
    aligner = align.Aligner(torch.nn.Sequential(head), patch=16)
    a, b = cuda(pixels(2, 37, 53)), cuda(pixels(2, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        aligner(a.cpu(), b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        aligner(a, b.cpu())
    for kw in (dict(roi_a=(0, 0, 54, 37)), dict(roi_a=[(0, 0, 53, 37), (-0.5, 0, 10, 10)]), dict(roi_b=(0, 8, 16, 8.5)),
               dict(roi_a=(3, 3, 0, 5)), dict(roi_b=(0, 0, float("nan"), 4))):
        with pytest.raises(ValueError, match="sample [01]"):
            aligner(a, b, **kw)
    with pytest.raises(ValueError, match="sample 1"):
        aligner(a, b, idx_a=[0, 2])
    with pytest.raises(ValueError):
        aligner(a, b, idx_a=[0])                                           # one sample of A, two of B
    assert not launches                                                    # every refusal came before any launch
    # banks, host index lists and regions together; zero delta and one geometry: the identity, and the aligned image is the region's copy
    r = aligner(ImageBank(a), ImageBank(a), idx_a=[1, 0], idx_b=[1, 0], roi_a=(2, 3, 32, 32), roi_b=(2, 3, 32, 32))
    assert launches and (r["H"] - torch.eye(3, dtype=torch.float64, device="cuda")).abs().max().item() <= 1e-12
    assert torch.equal(r["aligned"], a[[1, 0]]) and r["valid"][:, 1:, 1:].all()          # (a rounding of the solve may put row / column 0 at -1e-17)
