"""The two-band blend, host side (bihome_amd/align.py blur_taps / blur_host / bands_host / mosaic_bands_host; the C entry points
bh_blur_u8, bh_pano_bands_u8 and bh_mosaic_bands_u8 as far as they go without a device): the numpy definitions against independent
statements written here, against the feather and 'first' modes where the rule makes them meet, the pixels a float32 winner can be held
to, and the argument rules.

test_float32_restatement_stays_within_the_measured_shares holds the figures the device test's caps come from (see its docstring)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import align_bands_cases as Bc
import align_mosaic_cases as Mc
import align_pano_cases as Pc
from bihome_amd import align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH_OK, BH_E_BADARG, BH_E_UNSUPPORTED = 0, -1, -2
SAME_SIZE = [name for name, (Ha, Wa, Hb, Wb, _, _) in Mc.CASES.items() if (Ha, Wa) == (Hb, Wb)]
SMALL = "n3-17x23-on-24x53"


# ------------------------------------------------------------------------------------------------
# the taps and the low band
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.0, 3.0, 4.0, 10.5])
def test_taps_sum_to_2048_and_fall_off(sigma):
    w = align.blur_taps(sigma)
    assert w.dtype == np.int64 and w.shape == (int(np.ceil(3 * sigma)) + 1,) and len(w) - 1 == {0.5: 2, 1.0: 3, 3.0: 9, 4.0: 12, 10.5: 32}[sigma]
    r = len(w) - 1
    full = np.concatenate([w[:0:-1], w])                                   # i = -r .. r: symmetric by construction
    assert full.sum() == 2048 and np.array_equal(full, full[::-1]) and (w >= 0).all() and (np.diff(w[1:]) <= 0).all() and w[0] > 0
    g = np.exp(-np.arange(len(w)) ** 2 / (2.0 * sigma * sigma))
    g /= g[0] + 2 * g[1:].sum()
    assert np.array_equal(w[1:], np.floor(2048 * g[1:] + 0.5)) and abs(w[0] - 2048 * g[0]) <= r            # w_0 takes the 2 r roundings of the others
    # non-increasing from w_1 on always (the rounding is monotone); from the CENTRE on wherever w_0 stands out by more than the roundings it
    # absorbs, which 2048 (g_0 - g_1) >= r + 0.5 guarantees (sigma 0.5, 1, 3) and sigma 4 still has (206 198 181 ...).  At sigma 10.5 the
    # definition itself, w_0 = 2048 - 2 sum, gives 72 78 77 75 ...: g_0 - g_1 is 0.35 / 2048 there and w_0 carries 64 roundings - a dent
    # of 6 / 2048 in the centre of a low-pass that still sums to 2048
    if sigma <= 4.0:
        assert (np.diff(w) <= 0).all() and (sigma > 3.0 or 2048 * (g[0] - g[1]) >= r + 0.5)
    else:
        assert w[:4].tolist() == [72, 78, 77, 75]


def test_taps_refuse_a_sigma_outside_the_range():
    for sigma in (0.49, 10.51, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            align.blur_taps(sigma)
        with pytest.raises(ValueError):
            align.blur_host(Mc.textures(1, 17, 23, seed=1), sigma)


@pytest.mark.parametrize("h,w,sigma", [(17, 23, 3.0), (40, 56, 3.0), (17, 23, 0.5), (5, 7, 3.0), (1, 1, 0.5)])
def test_blur_host_order_constants_and_the_float64_gaussian(h, w, sigma):
    A = Mc.textures(2, h, w, seed=1)
    L = align.blur_host(A, sigma)
    assert L.dtype == np.uint8 and L.shape == A.shape
    assert np.array_equal(L, align.blur_host(A, sigma, order="cols"))      # rows first = columns first, bitwise
    assert np.array_equal(L[1], align.blur_host(A[1], sigma))              # any leading shape
    # within one grey level of the real-valued Gaussian: half a level is the final rounding; the integer taps are off by at most 0.5 / 2048
    # each and their errors sum to zero, so on a texture the rest stays far below the other half (printed)
    d = np.abs(L.astype(np.float64) - Bc.gaussian64(A, sigma))
    print("blur_host %d x %d sigma %g: max |integer - float64 Gaussian| = %.3f grey levels" % (h, w, sigma, d.max()))
    assert d.max() <= 1.0
    for c in (0, 1, 77, 254, 255):
        flat = np.full((1, h, w, 3), c, np.uint8)
        assert np.array_equal(align.blur_host(flat, sigma), flat)          # a constant comes back unchanged
    if (h, w) == (5, 7):
        assert len(align.blur_taps(sigma)) - 1 == 9 > w                    # narrower than the radius: every tap clamps
        # ... and equals an explicit loop
        wt = align.blur_taps(sigma)
        r = len(wt) - 1
        want = np.zeros((h, w, 3), np.int64)
        for y in range(h):
            for x in range(w):
                for j in range(-r, r + 1):
                    for i in range(-r, r + 1):
                        want[y, x] += int(wt[abs(j)]) * int(wt[abs(i)]) * A[0, min(max(y + j, 0), h - 1), min(max(x + i, 0), w - 1)].astype(np.int64)
        assert np.array_equal(L[0], (want + (1 << 21)) >> 22)


# ------------------------------------------------------------------------------------------------
# bands_host against a per-pixel loop, and the cases where the rule meets the other modes
# ------------------------------------------------------------------------------------------------
def bands_loop(bank, low, idx, M, Hc, Wc, feather, gain, use=None):
    """The definition pixel by pixel for one sample, on sample_host's values: presence and weight from a projection written here."""
    n = len(idx)
    Hs, Ws = bank.shape[1:3]
    vals = [align.sample_host(bank[idx[k]][None], M[k][None], Hc, Wc)[0][0] for k in range(n)]
    lows = [align.sample_host(low[k][None], M[k][None], Hc, Wc)[0][0] for k in range(n)]
    out, count, winner = np.zeros((Hc, Wc, 3), np.uint8), np.zeros((Hc, Wc), np.uint8), np.full((Hc, Wc), 255, np.uint8)
    for y in range(Hc):
        for x in range(Wc):
            seen = []                                                      # (weight, value, low, k) of the frames present, in order
            for k in range(n):
                q = M[k] @ np.array([x, y, 1.0])
                if use is not None and not use[k] or not abs(q[2]) > 1e-8:
                    continue
                u, v = q[0] * (1.0 / q[2]), q[1] * (1.0 / q[2])
                if 0 <= u <= Ws - 1 and 0 <= v <= Hs - 1:
                    g, o = (1.0, 0.0) if gain is None else gain[k]
                    seen.append((min(min(u, Ws - 1 - u, v, Hs - 1 - v) + 1.0, feather), g * vals[k][y, x] + o, g * lows[k][y, x] + o, k))
            count[y, x] = len(seen)
            if not seen:
                continue
            best = seen[0]
            for s in seen[1:]:
                if s[0] > best[0]:
                    best = s
            winner[y, x] = best[3]
            val = best[1] if len(seen) == 1 else best[1] + (sum(w * l for w, _, l, _ in seen) / sum(w for w, _, _, _ in seen) - best[2])
            out[y, x] = np.floor(np.clip(val, 0.0, 255.0) + 0.5)
    return out, count, winner


@pytest.mark.parametrize("gain", [False, True], ids=["no-gain", "gain"])
def test_bands_host_equals_the_pixel_loop(gain):
    bank, idx, _, M, Hc, Wc = Pc.case(SMALL)
    low = Bc.low_of(SMALL)
    g = Pc.gain_of(3, 2) if gain else None
    out, count, winner = Bc.reference(SMALL, 8.0, gain)
    assert out.dtype == count.dtype == winner.dtype == np.uint8 and out.shape == (2, Hc, Wc, 3) and count.shape == winner.shape == (2, Hc, Wc)
    for b in range(2):
        want, want_count, want_winner = bands_loop(bank, low[b], idx[b], M[b], Hc, Wc, 8.0, None if g is None else g[b])
        assert np.array_equal(count[b], want_count) and set(np.unique(count[b])) >= {0, 1, 2} and np.array_equal(winner[b], want_winner)
        assert set(np.unique(winner[b])) == {0, 1, 2, 255} and np.array_equal(winner[b] == 255, count[b] == 0)
        # (the two sum in another order: a pixel may sit on the other side of a rounding boundary, never further)
        d, share = Mc.differing_share(out[b], want)
        assert d <= 1 and share <= 2e-3, (d, share)
        assert not out[b][count[b] == 0].any()


def test_a_zero_low_bank_gives_the_winners_sample():
    bank, idx, _, M, Hc, Wc = Pc.case(SMALL)
    g = Pc.gain_of(3, 2)
    out, count, winner = align.bands_host(bank, np.zeros((2, 3) + bank.shape[1:], np.uint8), idx, M, Hc, Wc, 8.0)
    for k in range(3):
        own, _ = align.warp_u8_host(bank[idx[:, k]], M[:, k], Hc, Wc)
        assert np.array_equal(out[winner == k], own[winner == k]) and (winner == k).any()
    assert not out[winner == 255].any()
    # with a gain the low band is o everywhere, in every frame: still the winner's own (gained) value wherever the o's agree
    flat = g.copy()
    flat[:, :, 1] = 5.0
    out, count, winner = align.bands_host(bank, np.zeros((2, 3) + bank.shape[1:], np.uint8), idx, M, Hc, Wc, 8.0, flat)
    first = align.pano_host(bank, idx, M, Hc, Wc, 8.0, "first", flat)[0]
    assert np.array_equal(out[winner == 0], first[winner == 0])


def test_low_equal_to_the_frames_is_the_feather_within_a_level():
    """l = v: v_best + (sum w v / sum w - v_best) is the feathered mean up to two roundings."""
    bank, idx, _, M, Hc, Wc = Pc.case(SMALL)
    for gain in (False, True):
        g = Pc.gain_of(3, 2) if gain else None
        out, count, _ = align.bands_host(bank, bank[idx], idx, M, Hc, Wc, 8.0, g)
        want, want_count = Pc.reference(SMALL, "feather", 8.0, gain)
        d, share = Mc.differing_share(out, want)
        print("low = frames against 'feather', gain %s: max |difference| %d, %.2e of the pixels differ" % (gain, d, share))
        assert d <= 1 and np.array_equal(count, want_count), (d, share)


@pytest.mark.parametrize("name", [SMALL, "burst-n6-40x56-on-ref"])
def test_one_frame_present_is_mode_first_bitwise(name):
    for feather in Bc.FEATHERS[name]:
        for gain in (False, True):
            out, count, winner = Bc.reference(name, feather, gain)
            first, first_count = Pc.reference(name, "first", 8.0, gain)
            assert np.array_equal(count, first_count) and np.array_equal(out[count == 1], first[count == 1]) and (count == 1).any()


@pytest.mark.parametrize("name", SAME_SIZE)
def test_two_frames_are_the_pair_bit_for_bit(name):
    A, B, Ma, Mb, Hc, Wc = Mc.case(name)
    n = len(A)
    bank, idx = np.concatenate([A, B]), np.stack([np.arange(n), n + np.arange(n)], 1)
    la, lb = align.blur_host(A, Bc.SIGMA), align.blur_host(B, Bc.SIGMA)
    for feather, gain in ((8.0, None), (64.0, Mc.GAIN)):
        want, cover, want_winner = align.mosaic_bands_host(A, la, B, lb, Ma, Mb, Hc, Wc, feather, Mc.gain_of(gain, n))
        g = None if gain is None else np.tile(np.array([gain, (1.0, 0.0)]), (n, 1, 1))
        out, count, winner = align.bands_host(bank, np.stack([la, lb], 1), idx, np.stack([Ma, Mb], 1), Hc, Wc, feather, g)
        assert np.array_equal(out, want) and np.array_equal(winner, want_winner) and np.array_equal(count, (cover & 1) + (cover >> 1))
        assert cover.dtype == np.uint8 and set(np.unique(want_winner)) <= {0, 1, 255}
        assert np.array_equal(cover, Mc.reference(name, "feather", 8.0, None)[1])


def test_the_pair_with_images_of_two_sizes_and_refusals():
    name = "48x80-and-40x56-fitted-37x53-scalar"
    A, B, Ma, Mb, Hc, Wc = Mc.case(name)
    la, lb = align.blur_host(A, Bc.SIGMA), align.blur_host(B, Bc.SIGMA)
    out, cover, winner = align.mosaic_bands_host(A, la, B, lb, Ma, Mb, Hc, Wc, 8.0)
    assert np.array_equal(cover, Mc.reference(name, "feather", 8.0, None)[1]) and set(np.unique(winner)) == {0, 1, 255}
    a_over_b = Mc.reference(name, "a_over_b", 8.0, None)[0]
    single = (cover == 1) | (cover == 2)
    assert np.array_equal(out[single], a_over_b[single]) and np.array_equal(winner[cover == 1], np.zeros((cover == 1).sum(), np.uint8))
    with pytest.raises(ValueError):
        align.mosaic_bands_host(A, lb, B, lb, Ma, Mb, Hc, Wc, 8.0)         # A's low band has B's size
    with pytest.raises(ValueError):
        align.mosaic_bands_host(A, la, B, lb, Ma, Mb, Hc, Wc, 0.5)
    bank, idx, _, M, Hc, Wc = Pc.case(SMALL)
    for kw in (dict(feather=0.5), dict(feather=float("nan")), dict(low=Bc.low_of(SMALL)[:, :2]), dict(low=Bc.low_of(SMALL).astype(np.float64))):
        args = dict(low=Bc.low_of(SMALL), feather=8.0)
        args.update(kw)
        with pytest.raises(ValueError):
            align.bands_host(bank, args["low"], idx, M, Hc, Wc, args["feather"])


def test_use_zero_equals_leaving_the_frame_out():
    name = "n5-40x56-on-48x160"
    bank, idx, _, M, Hc, Wc = Pc.case(name)
    low = Bc.low_of(name)
    use = np.ones((2, 5), np.uint8)
    use[:, 1] = 0
    keep = [0, 2, 3, 4]
    out, count, winner = align.bands_host(bank, low, idx, M, Hc, Wc, 8.0, None, use)
    want, want_count, want_winner = align.bands_host(bank, low[:, keep], idx[:, keep], M[:, keep], Hc, Wc, 8.0)
    assert np.array_equal(out, want) and np.array_equal(count, want_count)
    assert np.array_equal(winner, np.where(want_winner == 255, 255, np.array(keep + [0] * 252, np.uint8)[want_winner]))


# ------------------------------------------------------------------------------------------------
# the pixels compared on the device, and the float32 restatement of the kernel: the figures behind the device test's caps
# ------------------------------------------------------------------------------------------------
UNDECIDED_MAX = 1e-3


@pytest.mark.parametrize("name", list(Pc.CASES))
def test_undecided_pixels_are_rare(name):
    for feather in Bc.FEATHERS[name]:
        share = 1.0 - Bc.decided(name, feather).mean()
        print("%s, feather %g: %.2e of the canvas is undecided (two float64 weights within %g of the largest)" % (name, feather, share, Bc.TIE))
        assert share <= UNDECIDED_MAX
    if name.startswith("burst"):                                           # why the burst does not run at feather 8
        assert 1.0 - Bc.decided(name, 8.0).mean() > 1e-2


# (case) -> the largest share of compared pixels whose colour differs, without the gain / with it, rounded up to two digits
MEASURED = {("n3-17x23-on-24x53", 3.0): (0.0, 1.6e-3), ("n5-40x56-on-48x160", 3.0): (1.4e-4, 3.3e-4), ("n5-40x56-on-37x131", 3.0): (0.0, 3.1e-4),
            ("n8-120x160-on-160x640", 3.0): (1.4e-4, 5.5e-4), ("burst-n6-40x56-on-ref", 3.0): (0.0, 0.0), ("n5-40x56-on-48x160", 1.0): (2.7e-4, 2.7e-4)}


@pytest.mark.parametrize("name,sigma", list(MEASURED), ids=["%s-sigma%g" % k for k in MEASURED])
def test_float32_restatement_stays_within_the_measured_shares(name, sigma):
    """The share of the compared pixels (decided, away from the border lines) on which a float32 numpy restatement of the kernel
    (align_bands_cases.bands_f32) differs from bands_host on exactly the device test's inputs, without and with the gain: MEASURED
    (rounded up to two digits), printed; none differs by more than one level, and winner and count agree on every one."""
    assert {(n, s) for n, _, _, s in Bc.RUNS} == set(MEASURED)
    bank, idx, _, M, Hc, Wc = Pc.case(name)
    nb, n = idx.shape
    low = Bc.low_of(name, sigma)
    worst = [0.0, 0.0]
    for feather in Bc.FEATHERS[name]:
        keep = Bc.compared(name, feather)
        for gain in (False, True):
            want, want_count, want_winner = Bc.reference(name, feather, gain, sigma)
            got, count, winner = Bc.bands_f32(bank, low, idx, M, Hc, Wc, feather, Pc.gain_of(n, nb) if gain else None)
            assert np.array_equal(count[keep], want_count[keep]) and np.array_equal(winner[keep], want_winner[keep])
            d, share = Mc.differing_share(got[keep], want[keep])
            assert d <= 1
            worst[gain] = max(worst[gain], share)
    print("%s, sigma %g: float32 restatement differs from float64 on %.2e of the compared pixels without gain, %.2e with" % (name, sigma, worst[0], worst[1]))
    assert worst[0] <= MEASURED[name, sigma][0] and worst[1] <= MEASURED[name, sigma][1]


# ------------------------------------------------------------------------------------------------
# the C entry points
# ------------------------------------------------------------------------------------------------
ARGS = {
    "bh_blur_u8": ["const uint8_t* images", "const int* idx", "int n_images", "int H", "int W", "int count", "const int* taps", "int radius",
                   "uint8_t* out", "void* stream"],
    "bh_pano_bands_u8": ["const uint8_t* images", "const uint8_t* low", "const int* idx", "int n_images", "int Hs", "int Ws", "const double* M",
                         "const double* gain", "const uint8_t* use", "int B", "int n", "int Hc", "int Wc", "float feather", "uint8_t* out",
                         "uint8_t* count", "uint8_t* winner", "void* stream"],
    "bh_mosaic_bands_u8": ["const uint8_t* images_a", "const uint8_t* low_a", "const int* idx_a", "int n_a", "int Ha", "int Wa",
                           "const uint8_t* images_b", "const uint8_t* low_b", "const int* idx_b", "int n_b", "int Hb", "int Wb",
                           "const double* Ma", "const double* Mb", "const double* gain", "int B", "int Hc", "int Wc", "float feather",
                           "uint8_t* out", "uint8_t* cover", "uint8_t* winner", "void* stream"],
}


def test_header_declares_what_ctypes_binds():
    from bihome_amd import _lib
    from bihome_amd import kernels as K
    raw = open(os.path.join(ROOT, "include", "bihome.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    sigs = {"bh_blur_u8": [P, P, I, I, I, I, P, I, P, P], "bh_pano_bands_u8": [P, P, P, I, I, I, P, P, P, I, I, I, I, F, P, P, P, P],
            "bh_mosaic_bands_u8": [P, P, P, I, I, I, P, P, P, I, I, I, P, P, P, I, I, I, F, P, P, P, P]}
    for name, args in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/bihome.h does not declare %s" % name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args
        fn = getattr(_lib.lib, name)
        assert _lib.SIGNATURES[name] == sigs[name] and list(fn.argtypes) == sigs[name] and fn.restype is I
    # the new mode has no number: the mode tables are what they were
    assert align.BAND_MODES == ("two_band",) and align.PANO_MODES == ("feather", "first", "last") and align.MOSAIC_MODES == ("feather", "b_over_a", "a_over_b")
    assert set(K.PANO_MODES) == set(align.PANO_MODES) and set(K.MOSAIC_MODES) == set(align.MOSAIC_MODES)
    assert not re.search(r"#define\s+BH_(PANO|MOSAIC)_\w*BAND", text)


def taps_of(values):
    return (ctypes.c_int * len(values))(*values)


def test_entry_point_argument_rules():
    """Checked before any launch (so without a GPU): device pointers are never dereferenced here; the taps are host memory and are."""
    from bihome_amd import _lib
    p = ctypes.c_void_p(64)
    good = taps_of(align.blur_taps(3.0).tolist())

    def blur(images=p, idx=p, n_images=5, H=24, W=32, count=2, taps=good, radius=9, out=p):
        return _lib.lib.bh_blur_u8(images, idx, n_images, H, W, count, taps, radius, out, None)

    def pano(images=p, low=p, idx=p, n_images=5, Hs=24, Ws=32, M=p, gain=p, use=p, B=2, n=4, Hc=30, Wc=40, feather=32.0, out=p, count=p, winner=p):
        return _lib.lib.bh_pano_bands_u8(images, low, idx, n_images, Hs, Ws, M, gain, use, B, n, Hc, Wc, feather, out, count, winner, None)

    def mosaic(images_a=p, low_a=p, idx_a=p, n_a=3, Ha=24, Wa=32, images_b=p, low_b=p, idx_b=p, n_b=3, Hb=20, Wb=28, Ma=p, Mb=p, gain=p, B=2, Hc=30,
               Wc=40, feather=32.0, out=p, cover=p, winner=p):
        return _lib.lib.bh_mosaic_bands_u8(images_a, low_a, idx_a, n_a, Ha, Wa, images_b, low_b, idx_b, n_b, Hb, Wb, Ma, Mb, gain, B, Hc, Wc, feather,
                                           out, cover, winner, None)
    w3 = align.blur_taps(3.0).tolist()
    wrong_sum, negative = list(w3), list(w3)
    wrong_sum[0] += 1
    negative[9], negative[0] = -1, w3[0] + 2 * (w3[9] + 1)                 # still sums to 2048
    assert negative[0] + 2 * sum(negative[1:]) == 2048
    w32 = align.blur_taps(10.5).tolist()
    for bad in (dict(images=None), dict(out=None), dict(taps=None), dict(count=-1), dict(n_images=0), dict(H=0), dict(W=-1), dict(taps=taps_of(wrong_sum)),
                dict(taps=taps_of(negative)), dict(radius=0), dict(radius=-1), dict(taps=taps_of(w32 + [0]), radius=33), dict(radius=8),
                dict(count=0, radius=0), dict(count=0, out=None), dict(count=0, taps=taps_of(wrong_sum))):
        assert blur(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(H=1 << 15, W=(1 << 14) + 1), dict(count=0, H=1 << 15, W=(1 << 14) + 1)):
        assert blur(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(count=0), dict(count=0, idx=None), dict(count=0, taps=taps_of(w32), radius=32), dict(count=0, taps=taps_of([1024, 512]), radius=1),
               dict(count=0, H=1 << 15, W=1 << 14), dict(count=0, H=1, W=1, n_images=1)):
        assert blur(**ok) == BH_OK, ok                                     # an empty batch: nothing launched
    for bad in (dict(images=None), dict(low=None), dict(M=None), dict(out=None), dict(B=-1), dict(n=0), dict(n=256), dict(n=-1), dict(n_images=0), dict(Hs=0),
                dict(Ws=-1), dict(Hc=0), dict(Wc=0), dict(Hc=-3), dict(feather=float("nan")), dict(feather=float("inf")), dict(feather=0.999),
                dict(feather=-8.0), dict(B=0, out=None), dict(B=0, low=None), dict(B=0, feather=0.5), dict(B=0, Hc=0), dict(B=0, n=0)):
        assert pano(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(Hs=1 << 15, Ws=(1 << 14) + 1), dict(Hc=1 << 16, Wc=1 << 15), dict(B=0, Hs=1 << 15, Ws=(1 << 14) + 1)):
        assert pano(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(B=0), dict(B=0, idx=None, gain=None, use=None, count=None, winner=None), dict(B=0, Hs=1 << 15, Ws=1 << 14),
               dict(B=0, n=255, Hs=1, Ws=1, Hc=1, Wc=1, feather=1.0)):
        assert pano(**ok) == BH_OK, ok
    for bad in (dict(images_a=None), dict(low_a=None), dict(images_b=None), dict(low_b=None), dict(Ma=None), dict(Mb=None), dict(out=None), dict(B=-1),
                dict(n_a=0), dict(n_b=0), dict(Ha=0), dict(Wa=0), dict(Hb=-1), dict(Wb=0), dict(Hc=0), dict(Wc=0), dict(feather=float("nan")),
                dict(feather=float("inf")), dict(feather=0.5), dict(B=0, out=None), dict(B=0, low_b=None), dict(B=0, feather=0.0)):
        assert mosaic(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(Ha=1 << 15, Wa=(1 << 14) + 1), dict(Hb=1 << 15, Wb=(1 << 14) + 1), dict(Hc=1 << 16, Wc=1 << 15), dict(B=0, Hc=1 << 16, Wc=1 << 15)):
        assert mosaic(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(B=0), dict(B=0, idx_a=None, idx_b=None, gain=None, cover=None, winner=None), dict(B=0, Ha=1, Wa=1, Hb=1, Wb=1, Hc=1, Wc=1, feather=1.0)):
        assert mosaic(**ok) == BH_OK, ok
    if not torch.cuda.is_available():                                      # (an accepted call does launch: the launch's own error)
        assert blur() > 0 and pano() > 0 and mosaic() > 0 and pano(idx=None, gain=None, use=None, count=None, winner=None, Wc=39) > 0


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from bihome_amd import kernels as K
    img = torch.zeros(3, 8, 8, 3, dtype=torch.uint8)
    G = torch.eye(3, dtype=torch.float64).repeat(1, 3, 1, 1)
    canvas = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.blur_u8(img, torch.zeros_like(img), align.blur_taps(1.0).tolist())
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.pano_bands_u8(img, img, None, G, canvas, None, None, 8.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.mosaic_bands_u8(img[:1], img[:1], img[:1], img[:1], G[:, 0], G[:, 0], canvas, None, None, 8.0)
    for call in (lambda: align.blur_u8(img, 3.0), lambda: align.pano_bands_u8(img, img, None, G, 8, 8),
                 lambda: align.mosaic_bands_u8(img[:1], img[:1], img[:1], img[:1], G[:, 0], G[:, 0], 8, 8),
                 lambda: align.panorama(img, G, mode="two_band"), lambda: align.mosaic(img, img, G[0], mode="two_band")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_the_rules_of_the_mode_the_sigma_and_the_low_bank():
    """The checks `mosaic`, `panorama` and the Aligner run before any launch, on their own (they need no device)."""
    for noun, modes in (("mosaic", align.MOSAIC_MODES), ("panorama", align.PANO_MODES)):
        keyword = align._CANVAS_KINDS[noun][0]
        for mode in modes + align.BAND_MODES:
            assert align._canvas_args(noun, keyword, 32.0, mode, 2.0, "test") is None
            assert align._canvas_args(noun, (24, 32), 32.0, mode, 2.0, "test") == (24, 32)
        for mode in ("bands", "two-band", "median", None, 0, ("two_band",)):
            with pytest.raises(ValueError):
                align._canvas_args(noun, keyword, 32.0, mode, 2.0, "test")
        assert align._CANVAS_KINDS[noun][2] == modes                       # the tables the existing tests loop over are what they were
    for sigma in (0.5, 4.0, 10.5, 1):
        align._band_args("two_band", sigma, "panorama", "test")
    for sigma in (0.49, 10.6, 0, -4.0, float("nan"), float("inf"), None, "4", (4.0,)):
        with pytest.raises(ValueError, match="band_sigma"):
            align._band_args("two_band", sigma, "panorama", "test")
        align._band_args("feather", sigma, "panorama", "test")             # the other modes do not look at it
    shape, cpu = (2, 3, 8, 8, 3), torch.device("cpu")
    assert align._low_arg(None, "feather", shape, cpu, "test") is None and align._low_arg(None, "two_band", shape, cpu, "test") is None
    with pytest.raises(ValueError, match="two_band"):
        align._low_arg(torch.zeros(shape, dtype=torch.uint8), "feather", shape, cpu, "test")          # a low bank with another mode
    for low in (torch.zeros(shape, dtype=torch.uint8), torch.zeros(shape), np.zeros(shape, np.uint8), "low"):
        with pytest.raises(ValueError):
            align._low_arg(low, "two_band", shape, cpu, "test")            # not on a device (and more)
