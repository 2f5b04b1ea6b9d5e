"""The mosaic on the device (csrc/blend.hip: bh_mosaic_u8; bihome_amd/align.py mosaic_frame_device / exposure_device / mosaic /
Aligner(mosaic=)) against the numpy float64 statements of bihome_amd/align.py, which tests/test_align_mosaic_cpu.py holds to independent
restatements.

Bounds.  No pixel differs from mosaic_host by more than one grey level, and the share of pixels that differ at all is capped at three
times what a float32 numpy restatement of the kernel's arithmetic (tests/align_mosaic_cases.py mosaic_f32) shows against the float64
statement on exactly these inputs, rounded up to one significant digit (three times: the kernel's reciprocal and its compiler's
instruction selection are not the restatement's).  Measured on the host (test_align_mosaic_cpu.py asserts the figures), largest share
over the modes and feathers 1, 8, 64, without the gain / with the gain (0.9, 6):
    17 x 23 onto B's grid                 1.28e-3 (one pixel of 782) / 3.84e-3
    48 x 80 onto B's grid                 1.30e-4 / 4.04e-3
    48 x 80 and 40 x 56 fitted, 64 x 96   8.14e-5 / 2.69e-3
    the same fitted onto 37 x 53          0       / 3.57e-3
    240 x 320, fitted onto 240 x 320      7.81e-5 / 3.76e-3
so CAP = 4e-3 without the gain and CAP_GAIN = 2e-2 with it.  The gain's figures are thirty times the others for a reason that is the
inputs', not the kernel's: 1 to 2.5 % of the canvas samples a saturated patch of A (255 on all taps), and 0.9 * 255 + 6 = 235.5 is a
rounding tie - whether the bilinear weights sum to 1 or to 1 - 1 ulp decides the grey level, in float64 as in float32.  (On an MI355X
the kernel showed the restatement's own figures in every row, 0 to 1.28e-3 without the gain and up to 4.04e-3 with it.)
cover is compared bit for bit where the float64 point is at least 1e-3 px from a border line of the image in question (B on its own
grid: everywhere, the border lies on pixel centres); at most 1e-3 of the canvas may be excluded per image (5.1e-4 measured)."""
import numpy as np
import pytest
import torch

import align_mosaic_cases as Mc
import poisoned_alloc
from bihome_amd import align
from bihome_amd import kernels as K

pytestmark = pytest.mark.gpu

CAP, CAP_GAIN = 4e-3, 2e-2
N_BIG = 9400        # 240 x 320 x 3 bytes per image: image 9,321 is the first that starts past 2^31 bytes (tests/test_align_gpu.py)
I3 = np.eye(3)[None]


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def run(A, B, Ma, Mb, Hc, Wc, feather=8.0, mode="feather", gain=None, **kw):
    out, cover = align.mosaic_u8(cuda(A), cuda(B), cuda(Ma), cuda(Mb), Hc, Wc, feather, mode, gain=None if gain is None else cuda(gain), **kw)
    return host(out), None if cover is None else host(cover)


# ------------------------------------------------------------------------------------------------
# the kernel against mosaic_host
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Mc.CASES))
def test_mosaic_matches_the_host_statement(monkeypatch, name):
    p = poisoned_alloc.poison(monkeypatch, align)          # outputs handed out 1-filled between red zones
    A, B, Ma, Mb, Hc, Wc = Mc.case(name)
    Ha, Wa, Hb, Wb, canvas, n = Mc.CASES[name]
    near_a = Mc.near_border(Ma, Hc, Wc, Ha, Wa)
    near_b = np.zeros_like(near_a) if canvas is None else Mc.near_border(Mb, Hc, Wc, Hb, Wb)
    print("%s: cover compared on all but %.2e (A) and %.2e (B) of the canvas" % (name, near_a.mean(), near_b.mean()))
    assert near_a.mean() <= 1e-3 and near_b.mean() <= 1e-3
    dA, dB, dMa, dMb = cuda(A), cuda(B), cuda(Ma), cuda(Mb)
    for mode, feather, gain in Mc.COMBOS:
        want, want_cover = Mc.reference(name, mode, feather, gain)
        dgain = None if gain is None else cuda(Mc.gain_of(gain, n))
        out, cover = align.mosaic_u8(dA, dB, dMa, dMb, Hc, Wc, feather, mode, gain=dgain)
        assert out.shape == (n, Hc, Wc, 3) and out.dtype == torch.uint8 and cover.shape == (n, Hc, Wc) and cover.dtype == torch.uint8
        d, share = Mc.differing_share(host(out), want)
        cap = CAP if gain is None else CAP_GAIN
        print("%s, %s, feather %g, gain %s: max |difference| %d grey levels, %.2e of the pixels differ (cap %.0e)" % (name, mode, feather, gain, d, share, cap))
        assert d <= 1 and share <= cap, (mode, feather, gain, d, share)
        got = host(cover)
        assert np.array_equal((got & 1)[~near_a], (want_cover & 1)[~near_a]) and np.array_equal((got & 2)[~near_b], (want_cover & 2)[~near_b])
        assert got.max() <= 3
    again, cover2 = align.mosaic_u8(dA, dB, dMa, dMb, Hc, Wc, feather, mode, gain=dgain)
    assert torch.equal(again, out) and torch.equal(cover2, cover)          # two calls, equal bits
    only, none = align.mosaic_u8(dA, dB, dMa, dMb, Hc, Wc, feather, mode, gain=dgain, want_cover=False)
    assert none is None and torch.equal(only, out)
    assert "mosaic_u8" in p.callers() and p.verify() == 2 * len(Mc.COMBOS) + 3          # nothing written outside either output
    if name == "48x80-and-40x56-fitted-64x96-vector":                      # every cover code on at least 2 % of a canvas
        codes = [float((want_cover[0] == k).mean()) for k in range(4)]
        print("cover codes of sample 0: %s" % (codes,))
        assert min(codes) >= 0.02


# ------------------------------------------------------------------------------------------------
# exact cases, bitwise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(17, 23), (48, 80)], ids=["17x23-scalar", "48x80-vector"])
def test_exact_cases_are_bitwise(h, w):
    A = Mc.textures(2, h, w, seed=1)
    eye = np.stack([np.eye(3)] * 2)
    for mode in align.MOSAIC_MODES:
        for feather in (1.0, 8.0, 64.0):
            out, cover = run(A, A, eye, eye, h, w, feather, mode)
            assert np.array_equal(out, A) and np.all(cover == 3), (mode, feather)
    A, B, Ma, Mb, *parts = Mc.translation_case(h, w)
    for mode in align.MOSAIC_MODES:
        for feather in (1.0, 4.0):
            out, cover = run(A, B, Ma, Mb, h, w, feather, mode)
            want, want_cover = Mc.translation_want(mode, feather, None, *parts)
            assert np.array_equal(cover[0], want_cover) and set(np.unique(cover)) == {0, 1, 2, 3}
            assert np.array_equal(out[0], want), (mode, feather)
            host_out, host_cover = align.mosaic_host(A, B, Ma, Mb, h, w, feather, mode)
            assert np.array_equal(out, host_out) and np.array_equal(cover, host_cover)


def test_a_single_pixel_image_and_a_vanishing_denominator():
    A, B = np.array([[[[200, 100, 50]]]], np.uint8), Mc.pixels(1, 5, 7, seed=6)
    Ma = np.array([[[0.5, 0, -1], [0, 0.5, -1], [0, 0, 1]]])               # (0, 0) of A at canvas (2, 2) only
    for mode, feather in (("a_over_b", 8.0), ("feather", 1.0), ("b_over_a", 8.0)):
        out, cover = run(A, B, Ma, I3, 5, 7, feather, mode)
        want, want_cover = align.mosaic_host(A, B, Ma, I3, 5, 7, feather, mode)
        assert np.array_equal(out, want) and np.array_equal(cover, want_cover) and cover[0, 2, 2] == 3 and (cover == 3).sum() == 1
    out, cover = run(B, A, I3, Ma, 5, 7, 8.0, "b_over_a")                  # the single pixel as image B
    assert out[0, 2, 2].tolist() == [200, 100, 50] and cover[0, 2, 2] == 3 and (cover == 1).sum() == 34
    out, cover = run(A, A, I3, I3, 4, 4, 8.0, "feather")                   # both single pixels, the vector path
    assert out[0, 0, 0].tolist() == [200, 100, 50] and not out[0].reshape(-1, 3)[1:].any() and cover.reshape(-1).tolist() == [3] + [0] * 15
    for A, Ma, B, Mb, Hc, Wc in Mc.single_pixel_pairs():                   # a single pixel as A, as B and as both on either store path
        for mode in align.MOSAIC_MODES:
            for gain in (None, Mc.gain_of(Mc.EXACT_GAIN, 2)):
                out, cover = run(A, B, Ma, Mb, Hc, Wc, Mc.EXACT_FEATHER, mode, gain=gain)
                want, want_cover = align.mosaic_host(A, B, Ma, Mb, Hc, Wc, Mc.EXACT_FEATHER, mode, gain)
                assert np.array_equal(out, want) and np.array_equal(cover, want_cover) and (cover == 3).sum() == 2, (A.shape, B.shape, Hc, Wc, mode)
    A, B = Mc.textures(1, 48, 80, seed=1), Mc.textures(1, 48, 80, seed=2)
    Ma = np.array([[[1.0, 0, 0], [0, 1, 0], [-0.125, 0, 1]]])              # qz = 1 - x / 8: exactly 0 on the column x = 8
    for mode in align.MOSAIC_MODES:
        out, cover = run(A, B, Ma, I3, 48, 80, 8.0, mode)
        _, want_cover = align.mosaic_host(A, B, Ma, I3, 48, 80, 8.0, mode)
        assert (cover[0, :, 8] == 2).all() and (cover[0, :, 0] == 3).all() and np.array_equal(out[0, :, 8], B[0, :, 8]), mode
        assert np.array_equal(cover, want_cover)          # (no projected point of this map lies within 1e-3 px of a border line without lying on it)


# ------------------------------------------------------------------------------------------------
# buffer contracts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_off,cover_off", [(3, 1), (4, 1), (4, 8), (3, 4)],
                         ids=["out+3-cover+1-scalar", "out+4-cover+1-vector-byte-cover", "out+4-cover+8-vector", "out+3-cover+4-scalar"])
def test_outputs_at_any_byte_offset_leave_their_surroundings_alone(out_off, cover_off):
    A, B, Ma, Mb, Hc, Wc = Mc.case("48x80-and-40x56-fitted-64x96-vector")
    dA, dB, dMa, dMb = cuda(A), cuda(B), cuda(Ma), cuda(Mb)
    want, want_cover = align.mosaic_u8(dA, dB, dMa, dMb, Hc, Wc, 8.0, "feather")
    n_out, n_cover, tail = want.numel(), want_cover.numel(), 16
    big_out = torch.full((out_off + n_out + tail,), 0xAB, dtype=torch.uint8, device="cuda")
    big_cover = torch.full((cover_off + n_cover + tail,), 0xCD, dtype=torch.uint8, device="cuda")
    assert big_out.data_ptr() % 4 == 0 and big_cover.data_ptr() % 4 == 0
    out, cover = big_out[out_off:out_off + n_out].view(want.shape), big_cover[cover_off:cover_off + n_cover].view(want_cover.shape)
    K.mosaic_u8(dA, dB, dMa, dMb, out, cover, 8.0, "feather")
    assert torch.equal(out, want) and torch.equal(cover, want_cover)
    assert (big_out[:out_off] == 0xAB).all() and (big_out[out_off + n_out:] == 0xAB).all()
    assert (big_cover[:cover_off] == 0xCD).all() and (big_cover[cover_off + n_cover:] == 0xCD).all()


def test_offsets_are_64_bit():
    """One bank whose last images start past 2^31 bytes, as image A and as image B: a 32-bit byte offset reads image 9,321 from the wrong
    place.  Integer translations, so the comparison with the host statement on the gathered images is bitwise."""
    data = torch.randint(0, 256, (N_BIG, 240, 320, 3), dtype=torch.uint8, device="cuda")
    assert data.numel() > 2 ** 31 and 9320 * 230400 < 2 ** 31 <= 9321 * 230400
    order = [0, 9320, 9321, N_BIG - 1]
    idx_a = torch.tensor(order, dtype=torch.int32, device="cuda")
    idx_b = torch.tensor(order[::-1], dtype=torch.int32, device="cuda")
    A, B = host(data[idx_a.long()]), host(data[idx_b.long()])
    Ma = np.stack([np.array([[1.0, 0, 4], [0, 1, 2], [0, 0, 1]])] * 4)
    Mb = np.stack([np.array([[1.0, 0, -7], [0, 1, -5], [0, 0, 1]])] * 4)
    out, cover = align.mosaic_u8(data, data, cuda(Ma), cuda(Mb), 240, 320, 8.0, "feather", idx_a=idx_a, idx_b=idx_b)
    want, want_cover = align.mosaic_host(A, B, Ma, Mb, 240, 320, 8.0, "feather")
    assert np.array_equal(host(out), want) and np.array_equal(host(cover), want_cover)
    assert not np.array_equal(want[1], want[2]) and set(np.unique(want_cover)) == {0, 1, 2, 3}      # (random bytes: an offset that wrapped would show)


def test_wild_indices_are_clamped():
    bank_a, bank_b = Mc.pixels(4, 17, 23, seed=7), Mc.pixels(3, 17, 23, seed=8)
    wild_a = torch.tensor([-1, 4, 2, -2147483648], dtype=torch.int32, device="cuda")
    wild_b = torch.tensor([3, -1, 1, 2147483647], dtype=torch.int32, device="cuda")
    Ma = np.stack([Mc.translation_case()[2][0]] * 4)
    Mb = np.stack([Mc.translation_case()[3][0]] * 4)
    out, cover = align.mosaic_u8(cuda(bank_a), cuda(bank_b), cuda(Ma), cuda(Mb), 17, 23, 4.0, "feather", idx_a=wild_a, idx_b=wild_b)
    want, want_cover = align.mosaic_host(bank_a[[0, 3, 2, 0]], bank_b[[2, 0, 1, 2]], Ma, Mb, 17, 23, 4.0, "feather")
    assert np.array_equal(host(out), want) and np.array_equal(host(cover), want_cover)


# ------------------------------------------------------------------------------------------------
# the frame and the exposure, device twins
# ------------------------------------------------------------------------------------------------
def test_frame_device_equals_the_host_statement(monkeypatch):
    from test_align_mosaic_cpu import GARBAGE, HORIZON
    p = poisoned_alloc.poison(monkeypatch, align)
    sizes = ((48, 80), (40, 56))
    H = np.stack([Mc.corner_homography(11 + b, 48, 80, 40, 56) for b in range(3)]
                 + [HORIZON, GARBAGE, np.zeros((3, 3)), np.full((3, 3), np.nan), np.array([[1.0, 0, 1e6], [0, 1, -1e6], [0, 0, 1]]), np.eye(3)])
    for canvas, limit in (((64, 96), 2.0), ((37, 53), 0.5), ((2, 2), 2.0)):
        T, bbox, fitted = align.mosaic_frame_device(cuda(H), *sizes, canvas, limit)
        wT, wbbox, wfitted = align.mosaic_frame_host(H, *sizes, canvas, limit)
        assert T.dtype == torch.float64 and bbox.dtype == torch.float64 and fitted.dtype == torch.uint8
        assert T.shape == (9, 3, 3) and bbox.shape == (9, 4) and fitted.shape == (9,)
        assert host(fitted).tolist() == wfitted.tolist() == [1, 1, 1, 0, 1, 0, 0, 1, 1]
        for got, want in ((host(T), wT), (host(bbox), wbbox)):
            assert np.isfinite(got).all() and np.all(np.abs(got - want) <= 1e-12 * np.abs(want).max(axis=tuple(range(1, want.ndim)), keepdims=True))
    assert p.verify() == 9                                                 # T, bbox and fitted of each of the three launches
    with pytest.raises(ValueError):
        align.mosaic_frame_device(cuda(H), *sizes, (1, 96))


def test_exposure_device_equals_the_host_statement():
    A, B = Mc.darkened_pair()
    h, w = A.shape[1:3]
    flat, negative = np.zeros_like(A), (255 - A).astype(np.uint8)
    few = np.zeros((1, h, w), np.uint8)
    few[0, 50, 40:55] = 1                                                  # 15 pixels may count: one short of ECC_MIN_N
    imgs_a, imgs_b = np.concatenate([A, flat, A, A]), np.concatenate([B, B, negative, B])
    mask = np.concatenate([np.ones((3, h, w), np.uint8), few])
    eye = cuda(np.stack([np.eye(3)] * 4))
    pa, pb = align.gray_pyramid(cuda(imgs_a), 4, 1), align.gray_pyramid(cuda(imgs_b), 4, 1)
    sums = align.ecc_sums(align.pyramid_level(pa, h, w, 1, 0), align.pyramid_level(pb, h, w, 1, 0), eye, mask=cuda(mask))
    got, want = host(align.exposure_device(sums)), align.exposure_host(host(sums))
    print("exposure on the device's sums: %s (host %s), n = %s" % (got.tolist(), want.tolist(), host(sums)[:, 65].tolist()))
    assert got.shape == (4, 2) and np.abs(got - want).max() <= 1e-9
    assert abs(got[0, 0] - 0.8) <= 1e-2 and abs(got[0, 1] - 10.0) <= 1.0
    assert got[1:].tolist() == [[1.0, 0.0]] * 3 and host(sums)[3, 65] == 15.0 and host(sums)[1, 65] > 1000


# ------------------------------------------------------------------------------------------------
# mosaic() and Aligner(mosaic=)
# ------------------------------------------------------------------------------------------------
PLAIN_KEYS = {"delta_hat", "H", "patch_1", "patch_2", "geom_a", "geom_b", "aligned", "valid"}
MOSAIC_KEYS = {"mosaic", "mosaic_cover", "mosaic_T", "mosaic_bbox", "mosaic_fitted", "mosaic_gain"}


def stub_aligner(delta, P=32):
    return align.Aligner(torch.nn.Sequential(Mc.StubHead(cuda(delta, torch.float32))), patch=P)


def test_aligner_without_mosaic_is_what_it_was(monkeypatch):
    calls = []
    fn = K.mosaic_u8
    monkeypatch.setattr(K, "mosaic_u8", lambda *a, **k: calls.append(1) or fn(*a, **k))
    A, B, delta, _ = Mc.aligner_pair()
    aligner, a, b = stub_aligner(delta), cuda(A), cuda(B)
    plain, none = aligner(a, b), aligner(a, b, mosaic=None)
    assert not calls and set(plain) == set(none) == PLAIN_KEYS
    for k in plain:
        assert torch.equal(none[k], plain[k]), k
    # the pieces, called directly: the result is the chain of before
    p1, ga = align.prepare(a, 1, 32, 1)
    p2, gb = align.prepare(b, 1, 32, 1)
    H = align.lift_device(cuda(delta, torch.float32), 32, ga, gb)
    aligned, valid = align.warp_u8(a, H, B.shape[1], B.shape[2])
    for k, want in (("patch_1", p1), ("patch_2", p2), ("geom_a", ga), ("geom_b", gb), ("H", H), ("aligned", aligned), ("valid", valid)):
        assert torch.equal(plain[k], want), k
    with_it = aligner(a, b, mosaic="b")
    assert calls == [1] and set(with_it) == PLAIN_KEYS | MOSAIC_KEYS
    for k in plain:
        assert torch.equal(with_it[k], plain[k]), k


def test_aligner_mosaic_on_b_with_a_on_top_is_the_aligned_image():
    A, B, delta, _ = Mc.aligner_pair()
    r = stub_aligner(delta)(cuda(A), cuda(B), mosaic="b", mosaic_mode="a_over_b")
    valid = r["valid"].bool()
    assert 0.2 < valid.float().mean().item() < 1.0
    assert torch.equal(r["mosaic"][valid], r["aligned"][valid])
    assert torch.equal(r["mosaic"][~valid], cuda(B)[~valid]) and torch.equal(r["mosaic_cover"], r["valid"] | 2)
    assert torch.equal(r["mosaic_T"], torch.eye(3, dtype=torch.float64, device="cuda")[None])
    assert host(r["mosaic_bbox"]).tolist() == [[0, 0, B.shape[2] - 1, B.shape[1] - 1]] and host(r["mosaic_fitted"]).tolist() == [0]
    assert host(r["mosaic_gain"]).tolist() == [[1.0, 0.0]]


def test_aligner_mosaic_on_a_fitted_canvas():
    A, B, delta, H_true = Mc.aligner_pair()
    Hc, Wc = 100, 152
    r = stub_aligner(delta)(cuda(A), cuda(B), mosaic=(Hc, Wc), mosaic_feather=16.0, mosaic_exposure=cuda(np.array([Mc.GAIN])))
    for k, shape, dtype in (("mosaic", (1, Hc, Wc, 3), torch.uint8), ("mosaic_cover", (1, Hc, Wc), torch.uint8), ("mosaic_T", (1, 3, 3), torch.float64),
                            ("mosaic_bbox", (1, 4), torch.float64), ("mosaic_fitted", (1,), torch.uint8), ("mosaic_gain", (1, 2), torch.float64)):
        assert tuple(r[k].shape) == shape and r[k].dtype == dtype and r[k].is_cuda, k
    H, T, gain = host(r["H"]), host(r["mosaic_T"]), host(r["mosaic_gain"])
    assert gain.tolist() == [list(Mc.GAIN)] and host(r["mosaic_fitted"]).tolist() == [1]
    wT, wbbox, _ = align.mosaic_frame_host(H, A.shape[1:3], B.shape[1:3], (Hc, Wc))
    assert np.abs(T - wT).max() <= 1e-12 * np.abs(wT).max() and np.abs(host(r["mosaic_bbox"]) - wbbox).max() <= 1e-12 * np.abs(wbbox).max()
    want, want_cover = align.mosaic_host(A, B, H @ T, T, Hc, Wc, 16.0, "feather", gain)
    d, share = Mc.differing_share(host(r["mosaic"]), want)
    near = Mc.near_border(H @ T, Hc, Wc, *A.shape[1:3]) | Mc.near_border(T, Hc, Wc, *B.shape[1:3])
    print("aligner, fitted %d x %d: max |difference| %d, %.2e of the pixels differ (cap %.0e); cover compared on all but %.2e" % (Hc, Wc, d, share, CAP_GAIN, near.mean()))
    assert d <= 1 and share <= CAP_GAIN and near.mean() <= 1e-3
    assert np.array_equal(host(r["mosaic_cover"])[~near], want_cover[~near]) and len(np.unique(want_cover)) == 4
    # the public function on the same H: the same bits
    m = align.mosaic(cuda(A), cuda(B), r["H"], canvas=(Hc, Wc), feather=16.0, exposure=cuda(np.array([Mc.GAIN])))
    assert set(m) == MOSAIC_KEYS and all(torch.equal(m[k], r[k]) for k in MOSAIC_KEYS)


def test_aligner_mosaic_exposure_gain_recovers_a_known_line():
    A, B, delta, _ = Mc.aligner_pair(g=0.8, o=10.0)
    aligner, a, b = stub_aligner(delta), cuda(A), cuda(B)
    r = aligner(a, b, mosaic="b", mosaic_exposure="gain")
    g, o = host(r["mosaic_gain"])[0]
    print("aligner, exposure 'gain' on B = round(0.8 A(H) + 10): g = %.5f, o = %.3f" % (g, o))
    assert abs(g - 0.8) <= 1e-2 and abs(o - 10.0) <= 1.0
    both = (r["mosaic_cover"] == 3)
    diff = (r["mosaic"].int() - b.int()).abs()[both]                       # A after the gain looks like B: the blend stays close to it
    assert diff.float().mean().item() < 1.0
    plain = aligner(a, b, mosaic="b")
    assert (plain["mosaic"].int() - b.int()).abs()[both].float().mean().item() > 2.0
    masked = aligner(a, b, refine="ecc", refine_levels=2, refine_iters=1, mask_b=torch.ones((1,) + B.shape[1:3], dtype=torch.uint8, device="cuda"),
                     mosaic="b", mosaic_exposure="gain")
    assert abs(host(masked["mosaic_gain"])[0, 0] - 0.8) <= 1e-2


def test_mosaic_arguments_are_refused_before_any_launch(monkeypatch):
    launches = []
    for name in ("align_prep_u8", "mosaic_u8", "gray_pyramid_u8"):
        fn = getattr(K, name)
        monkeypatch.setattr(K, name, lambda *a, _fn=fn, **k: launches.append(1) or _fn(*a, **k))
    A, B, delta, _ = Mc.aligner_pair()
    aligner, a, b = stub_aligner(delta), cuda(A), cuda(B)
    small = cuda(Mc.pixels(1, 7, 40))
    H = torch.eye(3, dtype=torch.float64, device="cuda")[None]
    bad = (dict(mosaic="a"), dict(mosaic=True), dict(mosaic=(64,)), dict(mosaic=(64, 96, 3)), dict(mosaic=(64.5, 96)), dict(mosaic=(1, 96)), dict(mosaic=(64, 0)),
           dict(mosaic="b", mosaic_feather=float("nan")), dict(mosaic="b", mosaic_feather=float("inf")), dict(mosaic="b", mosaic_feather=0.5),
           dict(mosaic="b", mosaic_feather=None), dict(mosaic="b", mosaic_mode="over"), dict(mosaic="b", mosaic_mode=0),
           dict(mosaic="b", mosaic_exposure="auto"), dict(mosaic="b", mosaic_exposure=1.0), dict(mosaic="b", mosaic_exposure=torch.ones(1, 2, dtype=torch.float64)),
           dict(mosaic="b", mosaic_exposure=torch.ones(1, 2, device="cuda")), dict(mosaic="b", mosaic_exposure=torch.ones(2, 2, dtype=torch.float64, device="cuda")),
           dict(mosaic=(64, 96), mosaic_limit=0.0), dict(mosaic=(64, 96), mosaic_limit=-1.0), dict(mosaic=(64, 96), mosaic_limit=float("nan")))
    for kw in bad:
        with pytest.raises(ValueError, match="mosaic"):
            aligner(a, b, **kw)
        names = {"mosaic": "canvas", "mosaic_feather": "feather", "mosaic_mode": "mode", "mosaic_exposure": "exposure", "mosaic_limit": "limit"}
        with pytest.raises(ValueError, match="mosaic"):
            align.mosaic(a, b, H, **{names[k]: v for k, v in kw.items()})
    with pytest.raises(ValueError, match="7 x 40"):
        aligner(small, b, mosaic="b", mosaic_exposure="gain")
    with pytest.raises(ValueError, match="7 x 40"):
        align.mosaic(a, small, H, exposure="gain")
    assert not launches                                                    # every refusal came before any launch
    assert set(aligner(small, b, mosaic="b")) == PLAIN_KEYS | MOSAIC_KEYS and launches          # (without 'gain' a small image is fine)
