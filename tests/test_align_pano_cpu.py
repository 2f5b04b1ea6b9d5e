"""The panorama, host side (bihome_amd/align.py chain_host / pano_frame_host / pano_host; the C entry points bh_pano_chain, bh_pano_frame
and bh_pano_u8 as far as they go without a device): the numpy definitions against independent statements written here and against the
pair's definitions (mosaic_frame_host / mosaic_host) for n = 2, exact cases, and the argument rules.

test_float32_restatement_stays_within_the_measured_shares holds the figures the device test's caps come from (see its docstring)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import align_mosaic_cases as Mc
import align_pano_cases as Pc
from bihome_amd import align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH_OK, BH_E_BADARG, BH_E_UNSUPPORTED = 0, -1, -2
SAME_SIZE = [name for name, (Ha, Wa, Hb, Wb, _, _) in Mc.CASES.items() if (Ha, Wa) == (Hb, Wb)]
MODE_OF = {"feather": "feather", "a_over_b": "first", "b_over_a": "last"}          # the pair's modes as the sequence's, frames (A, B)
HORIZON = np.array([[1.0, 0, 0], [0, 1, 0], [0.02, 0, -1.0]])      # test_align_mosaic_cpu.py's: the inverse's denominator changes sign across the frame
GARBAGE = np.array([[1e-3, 0, 0], [0, 1e-3, 0], [0, 0, 1.0]])      # ... and the frame's corners land a thousand image sizes away


# ------------------------------------------------------------------------------------------------
# pano_host against a per-pixel loop, and against mosaic_host for n = 2
# ------------------------------------------------------------------------------------------------
def pano_loop(bank, idx, M, Hc, Wc, feather, mode, gain, use=None):
    """The definition pixel by pixel for one sample, on sample_host's values: presence and weight from a projection written here."""
    n = len(idx)
    Hs, Ws = bank.shape[1:3]
    vals = [align.sample_host(bank[idx[k]][None], M[k][None], Hc, Wc)[0][0] for k in range(n)]
    out, count = np.zeros((Hc, Wc, 3), np.uint8), np.zeros((Hc, Wc), np.uint8)
    for y in range(Hc):
        for x in range(Wc):
            seen = []                                                      # (weight, value) of the frames present, in order
            for k in range(n):
                q = M[k] @ np.array([x, y, 1.0])
                if use is not None and not use[k] or not abs(q[2]) > 1e-8:
                    continue
                u, v = q[0] * (1.0 / q[2]), q[1] * (1.0 / q[2])
                if 0 <= u <= Ws - 1 and 0 <= v <= Hs - 1:
                    g, o = (1.0, 0.0) if gain is None else gain[k]
                    seen.append((min(min(u, Ws - 1 - u, v, Hs - 1 - v) + 1.0, feather), g * vals[k][y, x] + o))
            count[y, x] = len(seen)
            if not seen:
                continue
            if mode == "feather":
                val = sum(w * v for w, v in seen) / sum(w for w, _ in seen)
            else:
                val = seen[0][1] if mode == "first" else seen[-1][1]
            out[y, x] = np.floor(np.clip(val, 0.0, 255.0) + 0.5)
    return out, count


@pytest.mark.parametrize("gain", [False, True], ids=["no-gain", "gain"])
@pytest.mark.parametrize("mode", align.PANO_MODES)
def test_pano_host_equals_the_pixel_loop(mode, gain):
    bank, idx, _, M, Hc, Wc = Pc.case("n3-17x23-on-24x53")
    g = Pc.gain_of(3, 2) if gain else None
    out, count = align.pano_host(bank, idx, M, Hc, Wc, 8.0, mode, g)
    assert out.dtype == np.uint8 and count.dtype == np.uint8 and out.shape == (2, Hc, Wc, 3) and count.shape == (2, Hc, Wc)
    for b in range(2):
        want, want_count = pano_loop(bank, idx[b], M[b], Hc, Wc, 8.0, mode, None if g is None else g[b])
        assert np.array_equal(count[b], want_count) and set(np.unique(count[b])) >= {0, 1, 2}
        # (the two sum and divide in another order: a pixel may sit on the other side of a rounding boundary, never further)
        d, share = Mc.differing_share(out[b], want)
        assert d <= 1 and share <= 2e-3, (d, share)
        assert not out[b][count[b] == 0].any()


@pytest.mark.parametrize("name", SAME_SIZE)
def test_two_frames_are_the_mosaic_bit_for_bit(name):
    A, B, Ma, Mb, Hc, Wc = Mc.case(name)
    n = len(A)
    bank, idx = np.concatenate([A, B]), np.stack([np.arange(n), n + np.arange(n)], 1)
    M = np.stack([Ma, Mb], 1)
    for mode, feather, gain in Mc.COMBOS:
        want, cover = Mc.reference(name, mode, feather, gain)
        g = None if gain is None else np.tile(np.array([gain, (1.0, 0.0)]), (n, 1, 1))
        out, count = align.pano_host(bank, idx, M, Hc, Wc, feather, MODE_OF[mode], g)
        assert np.array_equal(out, want), (mode, feather, gain)
        assert np.array_equal(count, (cover & 1) + (cover >> 1))


def test_pano_host_returns_the_recorded_bytes():
    """tests/golden/align_pano_host.npz holds pano_host's output on this case as it stood before the blend statement was shared with
    mosaic_host (`_blend_host`): the statement is the reference of every device test, so it moves by no byte."""
    bank, idx, _, M, Hc, Wc = Pc.case("n5-40x56-on-48x160")
    want = np.load(os.path.join(ROOT, "tests", "golden", "align_pano_host.npz"))
    for i, (mode, feather, gain) in enumerate(Pc.COMBOS):
        out, count = align.pano_host(bank, idx, M, Hc, Wc, feather, mode, Pc.gain_of(*idx.shape[::-1]) if gain else None)
        assert np.array_equal(out, want["out%d" % i]) and np.array_equal(count, want["count%d" % i]), (mode, feather, gain)
        assert out.dtype == np.uint8 and count.dtype == np.uint8


def test_pano_host_refuses_what_it_does_not_define():
    bank, idx, _, M, Hc, Wc = Pc.case("n3-17x23-on-24x53")
    for kw in (dict(mode="b_over_a"), dict(mode="median"), dict(feather=0.5), dict(feather=float("nan")), dict(feather=float("inf"))):
        with pytest.raises(ValueError):
            align.pano_host(bank, idx, M, Hc, Wc, **kw)
    with pytest.raises(ValueError):
        align.pano_host(bank, idx[:, :2], M, Hc, Wc)                       # n of idx and of M differ


def test_use_zero_equals_leaving_the_frame_out():
    bank, idx, _, M, Hc, Wc = Pc.case("n5-40x56-on-48x160")
    use = np.ones((2, 5), np.uint8)
    use[:, 3] = 0
    keep = [0, 1, 2, 4]
    g = Pc.gain_of(5, 2)
    for mode in align.PANO_MODES:
        out, count = align.pano_host(bank, idx, M, Hc, Wc, 8.0, mode, g, use)
        want, want_count = align.pano_host(bank, idx[:, keep], M[:, keep], Hc, Wc, 8.0, mode, g[:, keep])
        assert np.array_equal(out, want) and np.array_equal(count, want_count), mode
    full = align.pano_host(bank, idx, M, Hc, Wc, 8.0, "feather", g)
    assert not np.array_equal(full[1], count)


def test_exact_cases_are_bitwise():
    A = Mc.textures(1, 17, 23, seed=1)
    for mode in align.PANO_MODES:
        out, count = align.pano_host(A, [[0]], np.eye(3)[None, None], 17, 23, 8.0, mode)          # n = 1, M = I: the image
        assert np.array_equal(out, A) and np.all(count == 1)
    bank, idx, M = Pc.translation_case()
    out, count = align.pano_host(bank, idx, M, 17, 23, 1.0, "feather")
    assert set(np.unique(count)) == {0, 1, 2, 3}
    h, w = 17, 23
    total, cnt = np.zeros((h, w, 3)), np.zeros((h, w))
    first, last = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for k in range(3):
        dx, dy = int(M[0, k, 0, 2]), int(M[0, k, 1, 2])
        for y in range(max(0, -dy), min(h, h - dy)):
            for x in range(max(0, -dx), min(w, w - dx)):
                v = bank[k, y + dy, x + dx].astype(np.float64)
                first[y, x] = v if cnt[y, x] == 0 else first[y, x]
                last[y, x] = v
                total[y, x] += v
                cnt[y, x] += 1
    assert np.array_equal(count[0], cnt)
    assert np.array_equal(out[0], np.floor(total / np.maximum(cnt, 1)[..., None] + 0.5).astype(np.uint8))          # feather 1: the plain mean
    assert np.array_equal(align.pano_host(bank, idx, M, h, w, 4.0, "first")[0][0], first.astype(np.uint8))
    assert np.array_equal(align.pano_host(bank, idx, M, h, w, 4.0, "last")[0][0], last.astype(np.uint8))


# ------------------------------------------------------------------------------------------------
# pano_frame_host
# ------------------------------------------------------------------------------------------------
def test_frame_of_two_is_the_mosaic_frame():
    size = (40, 56)
    H = np.stack([Mc.corner_homography(11 + b, 40, 56, 40, 56) for b in range(3)]
                 + [HORIZON, GARBAGE, np.zeros((3, 3)), np.full((3, 3), np.nan), np.array([[1.0, 0, 1e6], [0, 1, -1e6], [0, 0, 1]]), np.eye(3)])
    G = np.stack([H, np.stack([np.eye(3)] * len(H))], 1)
    for canvas, limit in (((64, 96), 2.0), ((37, 53), 0.5), ((2, 2), 2.0)):
        T, bbox, fitted = align.pano_frame_host(G, size, canvas, limit)
        wT, wbbox, wfitted = align.mosaic_frame_host(H, size, size, canvas, limit)
        assert np.array_equal(T, wT) and np.array_equal(bbox, wbbox)
        assert fitted.dtype == np.uint8 and fitted.shape == (9, 2) and fitted[:, 0].tolist() == wfitted.tolist() and fitted[:, 1].tolist() == [1] * 9
    for canvas in ((1, 96), (64, 1)):
        with pytest.raises(ValueError):
            align.pano_frame_host(G, size, canvas)
    with pytest.raises(ValueError):
        align.pano_frame_host(G, size, (64, 96), limit=0.0)


def test_frame_of_a_horizon_garbage_and_use():
    bank, idx, G, _, _, _ = Pc.case("n5-40x56-on-48x160")
    size, canvas = (40, 56), (48, 160)
    T, bbox, fitted = align.pano_frame_host(G, size, canvas)
    assert fitted.tolist() == [[1] * 5] * 2 and np.all(bbox[:, 0] < -40) and np.all(bbox[:, 2] > 55 + 40)
    bad = G.copy()
    bad[:, 4] = HORIZON                                                    # a horizon frame: fitted 0, and the box is the others'
    T2, bbox2, fitted2 = align.pano_frame_host(bad, size, canvas)
    T3, bbox3, fitted3 = align.pano_frame_host(G[:, :4], size, canvas)
    assert fitted2.tolist() == [[1, 1, 1, 1, 0]] * 2 and np.array_equal(bbox2, bbox3) and np.array_equal(T2, T3)
    use = np.ones((2, 5), np.uint8)
    use[:, 4] = 0                                                          # use = 0: the same as leaving the frame out
    T4, bbox4, fitted4 = align.pano_frame_host(G, size, canvas, use=use)
    assert fitted4.tolist() == [[1, 1, 1, 1, 0]] * 2 and np.array_equal(bbox4, bbox3) and np.array_equal(T4, T3)
    junk = G.copy()
    junk[:, 0] = GARBAGE                                                   # usable, and clamped to `limit` image sizes
    _, bbox5, fitted5 = align.pano_frame_host(junk, size, canvas)
    assert fitted5.tolist() == [[1] * 5] * 2 and np.all(bbox5[:, 2] == 3 * 56 - 1) and np.all(bbox5[:, 3] == 3 * 40 - 1)
    only = align.pano_frame_host(np.eye(3)[None, None], size, (40, 56))    # n = 1: the reference's own grid
    assert np.array_equal(only[0][0], np.eye(3)) and only[1].tolist() == [[0, 0, 55, 39]] and only[2].tolist() == [[1]]


# ------------------------------------------------------------------------------------------------
# chain_host
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [0, 2, 4], ids=["ref-first", "ref-middle", "ref-last"])
def test_chain_equals_the_explicit_products(ref):
    n = 5
    Hp = np.stack([[Mc.corner_homography(51 + 7 * b + j, 40, 56, 40, 56, 0.1) for j in range(n - 1)] for b in range(2)])
    gp = np.random.RandomState(2).uniform(0.5, 1.5, (2, n - 1, 2)) * np.array([1.0, 8.0])
    G, gain = align.chain_host(Hp, ref, gp)
    assert G.shape == (2, n, 3, 3) and gain.shape == (2, n, 2) and np.array_equal(align.chain_host(Hp, ref), G)
    pairs = align.pairs_of(n, ref)
    assert pairs == [(j, j + 1) if j < ref else (j + 1, j) for j in range(n - 1)]
    for b in range(2):
        assert np.array_equal(G[b, ref], np.eye(3)) and gain[b, ref].tolist() == [1.0, 0.0]
        for k in range(n):
            # the product of the pair matrices on the way from the reference to frame k, outermost last
            want, line = np.eye(3), (1.0, 0.0)
            steps = range(ref, k) if k > ref else range(ref - 1, k - 1, -1)
            for j in steps:
                want = Hp[b, j] @ want
                line = (line[0] * gp[b, j, 0], line[0] * gp[b, j, 1] + line[1])
            want = want / want[2, 2]
            assert np.abs(G[b, k] - want).max() <= 1e-12 * np.abs(want).max() and G[b, k, 2, 2] == 1.0
            assert np.abs(gain[b, k] - line).max() <= 1e-12 * max(np.abs(line))
    # the lines, directly: frame a's value v becomes the reference's by applying the pairs' lines on the way
    v = 100.0
    for k in range(n):
        w = v
        for j in (range(k - 1, ref - 1, -1) if k > ref else range(k, ref)):
            w = gp[0, j, 0] * w + gp[0, j, 1]
        assert abs(gain[0, k, 0] * v + gain[0, k, 1] - w) <= 1e-9
    with pytest.raises(ValueError):
        align.chain_host(Hp, n)
    with pytest.raises(ValueError):
        align.pairs_of(0, 0)
    assert align.pairs_of(1, 0) == [] and align.chain_host(np.empty((3, 0, 3, 3)), 0).shape == (3, 1, 3, 3)


# ------------------------------------------------------------------------------------------------
# the float32 restatement of the kernel: the figures behind the device test's caps
# ------------------------------------------------------------------------------------------------
MEASURED = {"n3-17x23-on-24x53": (4.0e-4, 2.0e-3), "n5-40x56-on-48x160": (2.0e-4, 9.2e-4), "n5-40x56-on-37x131": (1.1e-4, 4.2e-4),
            "n8-120x160-on-160x640": (1.3e-4, 1.1e-3), "burst-n6-40x56-on-ref": (2.3e-4, 6.3e-3)}


@pytest.mark.parametrize("name", list(Pc.CASES))
def test_float32_restatement_stays_within_the_measured_shares(name):
    """The share of pixels on which a float32 numpy restatement of the kernel (align_pano_cases.pano_f32) differs from pano_host on
    exactly the device test's inputs, without and with the gain: MEASURED (rounded up to two digits), printed; none differs by more than
    one level and no count differs away from the border lines."""
    bank, idx, _, M, Hc, Wc = Pc.case(name)
    nb, n = idx.shape
    _, near = Pc.near_border(name)
    worst = [0.0, 0.0]
    for mode, feather, gain in Pc.COMBOS:
        want, want_count = Pc.reference(name, mode, feather, gain)
        got, count = Pc.pano_f32(bank, idx, M, Hc, Wc, feather, mode, Pc.gain_of(n, nb) if gain else None)
        d, share = Mc.differing_share(got, want)
        assert d <= 1
        worst[gain] = max(worst[gain], share)
        assert np.array_equal(count[~near], want_count[~near])
    shares = [float((want_count == k).mean()) for k in range(4)] + [float((want_count >= 4).mean())]
    print("%s: float32 restatement differs from float64 on %.2e of the pixels without gain, %.2e with; count 0 / 1 / 2 / 3 / 4+ on %s of the "
          "canvas, at most %d; %.2e of it near a border line" % (name, worst[0], worst[1], [round(s, 3) for s in shares], want_count.max(), near.mean()))
    assert worst[0] <= MEASURED[name][0] and worst[1] <= MEASURED[name][1]
    if name.startswith("burst"):
        assert want_count.max() == 6


# ------------------------------------------------------------------------------------------------
# the C entry points
# ------------------------------------------------------------------------------------------------
ARGS = {
    "bh_pano_chain": ["const double* Hpair", "const double* gain_pair", "int B", "int n", "int ref", "double* G", "double* gain", "void* stream"],
    "bh_pano_frame": ["const double* G", "const uint8_t* use", "int B", "int n", "int Hs", "int Ws", "int Hr", "int Wr", "int Hc", "int Wc", "double limit",
                      "double* T", "double* bbox", "uint8_t* fitted", "double* M", "void* stream"],
    "bh_pano_u8": ["const uint8_t* images", "const int* idx", "int n_images", "int Hs", "int Ws", "const double* M", "const double* gain",
                   "const uint8_t* use", "int B", "int n", "int Hc", "int Wc", "float feather", "int mode", "uint8_t* out", "uint8_t* count", "void* stream"],
}


def test_header_declares_what_ctypes_binds():
    from bihome_amd import _lib
    from bihome_amd import kernels as K
    raw = open(os.path.join(ROOT, "include", "bihome.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    P, I, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    sigs = {"bh_pano_chain": [P, P, I, I, I, P, P, P], "bh_pano_frame": [P, P, I, I, I, I, I, I, I, I, D, P, P, P, P, P],
            "bh_pano_u8": [P, P, I, I, I, P, P, P, I, I, I, I, F, I, P, P, P]}
    for name, args in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/bihome.h does not declare %s" % name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args
        fn = getattr(_lib.lib, name)
        assert _lib.SIGNATURES[name] == sigs[name] and list(fn.argtypes) == sigs[name] and fn.restype is I
    modes = dict(re.findall(r"#define\s+BH_PANO_(\w+)\s+(\d+)", text))
    assert {k.lower(): int(v) for k, v in modes.items()} == K.PANO_MODES == {m: i for i, m in enumerate(align.PANO_MODES)}


def test_entry_point_argument_rules():
    """Checked before any launch (so without a GPU): pointers are never dereferenced here."""
    from bihome_amd import _lib
    p = ctypes.c_void_p(64)

    def chain(Hpair=p, gain_pair=p, B=2, n=4, ref=1, G=p, gain=p):
        return _lib.lib.bh_pano_chain(Hpair, gain_pair, B, n, ref, G, gain, None)

    def frame(G=p, use=p, B=2, n=4, Hs=24, Ws=32, Hr=24, Wr=32, Hc=30, Wc=40, limit=2.0, T=p, bbox=p, fitted=p, M=p):
        return _lib.lib.bh_pano_frame(G, use, B, n, Hs, Ws, Hr, Wr, Hc, Wc, limit, T, bbox, fitted, M, None)

    def pano(images=p, idx=p, n_images=5, Hs=24, Ws=32, M=p, gain=p, use=p, B=2, n=4, Hc=30, Wc=40, feather=32.0, mode=0, out=p, count=p):
        return _lib.lib.bh_pano_u8(images, idx, n_images, Hs, Ws, M, gain, use, B, n, Hc, Wc, feather, mode, out, count, None)
    for bad in (dict(G=None), dict(Hpair=None), dict(B=-1), dict(n=0), dict(n=256), dict(n=-2), dict(ref=-1), dict(ref=4), dict(B=0, ref=4), dict(B=0, G=None)):
        assert chain(**bad) == BH_E_BADARG, bad
    for ok in (dict(B=0), dict(B=0, n=1, ref=0, Hpair=None, gain_pair=None, gain=None), dict(B=0, n=255, ref=254)):
        assert chain(**ok) == BH_OK, ok
    for bad in (dict(G=None), dict(T=None), dict(B=-1), dict(n=0), dict(n=256), dict(Hs=0), dict(Ws=0), dict(Hr=0), dict(Wr=0), dict(Wr=-1), dict(Hc=1),
                dict(Wc=1), dict(Wc=-5), dict(limit=0.0), dict(limit=-1.0), dict(limit=float("nan")), dict(B=0, T=None), dict(B=0, n=0)):
        assert frame(**bad) == BH_E_BADARG, bad
    for ok in (dict(B=0), dict(B=0, use=None, bbox=None, fitted=None, M=None, n=255, Hs=1, Ws=1, Hr=1, Wr=1, Hc=2, Wc=2)):
        assert frame(**ok) == BH_OK, ok
    for bad in (dict(images=None), dict(M=None), dict(out=None), dict(B=-1), dict(n=0), dict(n=256), dict(n=-1), dict(n_images=0), dict(Hs=0), dict(Ws=-1),
                dict(Hc=0), dict(Wc=0), dict(Hc=-3), dict(feather=float("nan")), dict(feather=float("inf")), dict(feather=0.999), dict(feather=0.0),
                dict(feather=-8.0), dict(mode=3), dict(mode=-1), dict(B=0, out=None), dict(B=0, mode=7), dict(B=0, feather=0.5), dict(B=0, Hc=0), dict(B=0, n=0)):
        assert pano(**bad) == BH_E_BADARG, bad
    for unsupported in (dict(Hs=1 << 15, Ws=(1 << 14) + 1), dict(Hc=1 << 16, Wc=1 << 15), dict(B=0, Hs=1 << 15, Ws=(1 << 14) + 1)):
        assert pano(**unsupported) == BH_E_UNSUPPORTED, unsupported
    for ok in (dict(B=0), dict(B=0, idx=None, gain=None, use=None, count=None), dict(B=0, Hs=1 << 15, Ws=1 << 14),
               dict(B=0, n=255, Hs=1, Ws=1, Hc=1, Wc=1, feather=1.0, mode=2)):
        assert pano(**ok) == BH_OK, ok                                     # an empty batch: nothing launched
    if not torch.cuda.is_available():                                      # (an accepted call does launch: the launch's own error)
        assert chain() > 0 and frame() > 0 and pano() > 0 and pano(idx=None, gain=None, use=None, count=None, Wc=39, mode=1) > 0


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from bihome_amd import kernels as K
    img = torch.zeros(3, 8, 8, 3, dtype=torch.uint8)
    G = torch.eye(3, dtype=torch.float64).repeat(2, 3, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.pano_u8(img, None, G, torch.zeros(2, 8, 8, 3, dtype=torch.uint8), None, 8.0, "feather")
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.pano_chain(G[:, :2], 1, G)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.pano_frame(G, (8, 8), (8, 8), 2.0, torch.zeros(2, 3, 3, dtype=torch.float64))
    for call in (lambda: align.pano_u8(img, None, G, 8, 8), lambda: align.chain_device(G[:, :2], 1), lambda: align.pano_frame_device(G, (8, 8), (8, 8)),
                 lambda: align.panorama(img, G)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
