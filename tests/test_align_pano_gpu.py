"""The panorama on the device (csrc/pano.hip: bh_pano_chain, bh_pano_frame, bh_pano_u8; bihome_amd/align.py chain_device /
pano_frame_device / pano_u8 / panorama / Aligner.sequence) against the numpy float64 statements of bihome_amd/align.py, which
tests/test_align_pano_cpu.py holds to independent restatements and to the pair's definitions.

Bounds.  No pixel differs from pano_host by more than one grey level, and the share of pixels that differ at all is capped at three
times what a float32 numpy restatement of the kernel's arithmetic (tests/align_pano_cases.py pano_f32) shows against the float64
statement on exactly these inputs, rounded up to one significant digit (three times, as in test_align_mosaic_gpu.py: the kernel's
reciprocal and its compiler's instruction selection are not the restatement's).  Measured on the host (test_align_pano_cpu.py asserts
the figures), largest share over the modes and feathers 1, 8, 64, without the gain / with gain[b,k] = (1 - 0.05 (k % 3), 3 (k % 4)):
    n = 3, 17 x 23 on 24 x 53          3.93e-4 / 1.97e-3
    n = 5, 40 x 56 on 48 x 160         1.95e-4 / 9.11e-4
    n = 5, 40 x 56 on 37 x 131         1.03e-4 / 4.13e-4
    n = 8, 120 x 160 on 160 x 640      1.27e-4 / 1.07e-3
    burst n = 6, 40 x 56 on "ref"      2.23e-4 / 6.25e-3
so CAP = 2e-3 without the gain and CAP_GAIN = 2e-2 with it (the burst's figure is the largest because 79 % of its canvas blends four or
more frames: every frame's rounding takes part).  count is compared bit for bit where the float64 point is at least 1e-3 px from every
border line of every frame (a frame whose M is the identity lies on pixel centres: compared everywhere); at most 1e-3 of the canvas may
be excluded per frame and 5e-3 in all (8.9e-4 in all at most, measured)."""
import numpy as np
import pytest
import torch

import align_mosaic_cases as Mc
import align_pano_cases as Pc
import poisoned_alloc
from bihome_amd import align
from bihome_amd import kernels as K
from test_align_pano_cpu import GARBAGE, HORIZON, MEASURED, MODE_OF, SAME_SIZE

pytestmark = pytest.mark.gpu

CAP, CAP_GAIN = 2e-3, 2e-2
N_BIG = 9400        # 240 x 320 x 3 bytes per image: image 9,321 is the first that starts past 2^31 bytes (tests/test_align_gpu.py)


def test_caps_are_three_times_the_measured_shares():
    def up(x):                                                             # rounded up to one significant digit
        e = 10.0 ** np.floor(np.log10(x))
        return float(np.ceil(x / e - 1e-9) * e)
    assert CAP == up(3 * max(m[0] for m in MEASURED.values())) and CAP_GAIN == up(3 * max(m[1] for m in MEASURED.values()))


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def run(bank, idx, M, Hc, Wc, feather=8.0, mode="feather", gain=None, use=None, **kw):
    out, count = align.pano_u8(cuda(bank), None if idx is None else cuda(idx, torch.int32), cuda(M), Hc, Wc, feather, mode,
                               gain=None if gain is None else cuda(gain), use=None if use is None else cuda(use), **kw)
    return host(out), None if count is None else host(count)


# ------------------------------------------------------------------------------------------------
# the kernel against pano_host
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Pc.CASES))
def test_pano_matches_the_host_statement(monkeypatch, name):
    p = poisoned_alloc.poison(monkeypatch, align)          # outputs handed out 1-filled between red zones
    bank, idx, _, M, Hc, Wc = Pc.case(name)
    nb, n = idx.shape
    per, near = Pc.near_border(name)
    print("%s: count compared on all but %.2e of the canvas (per frame at most %.2e)" % (name, near.mean(), per.mean((1, 2, 3)).max()))
    assert per.mean((1, 2, 3)).max() <= 1e-3 and near.mean() <= 5e-3
    dbank, didx, dM, dgain = cuda(bank), cuda(idx, torch.int32), cuda(M), cuda(Pc.gain_of(n, nb))
    for mode, feather, gain in Pc.COMBOS:
        want, want_count = Pc.reference(name, mode, feather, gain)
        out, count = align.pano_u8(dbank, didx, dM, Hc, Wc, feather, mode, gain=dgain if gain else None)
        assert out.shape == (nb, Hc, Wc, 3) and out.dtype == torch.uint8 and count.shape == (nb, Hc, Wc) and count.dtype == torch.uint8
        d, share = Mc.differing_share(host(out), want)
        cap = CAP_GAIN if gain else CAP
        print("%s, %s, feather %g, gain %s: max |difference| %d grey levels, %.2e of the pixels differ (cap %.0e)" % (name, mode, feather, gain, d, share, cap))
        assert d <= 1 and share <= cap, (mode, feather, gain, d, share)
        assert np.array_equal(host(count)[~near], want_count[~near]) and host(count).max() <= n
    again, count2 = align.pano_u8(dbank, didx, dM, Hc, Wc, feather, mode, gain=dgain if gain else None)
    assert torch.equal(again, out) and torch.equal(count2, count)          # two calls, equal bits
    only, none = align.pano_u8(dbank, didx, dM, Hc, Wc, feather, mode, gain=dgain if gain else None, want_count=False)
    assert none is None and torch.equal(only, out)
    assert "pano_u8" in p.callers() and p.verify() == 2 * len(Pc.COMBOS) + 3          # nothing written outside either output
    if name.startswith("burst"):
        assert want_count.max() == 6


@pytest.mark.parametrize("name", SAME_SIZE)
def test_two_frames_are_bh_mosaic_u8_bit_for_bit(name):
    A, B, Ma, Mb, Hc, Wc = Mc.case(name)
    n = len(A)
    bank = cuda(np.concatenate([A, B]))
    idx = cuda(np.stack([np.arange(n), n + np.arange(n)], 1), torch.int32)
    M, dMa, dMb = cuda(np.stack([Ma, Mb], 1)), cuda(Ma), cuda(Mb)
    ia, ib = idx[:, 0].contiguous(), idx[:, 1].contiguous()
    for mode, feather, gain in Mc.COMBOS:
        want, cover = align.mosaic_u8(bank, bank, dMa, dMb, Hc, Wc, feather, mode, gain=None if gain is None else cuda(Mc.gain_of(gain, n)), idx_a=ia, idx_b=ib)
        g = None if gain is None else cuda(np.tile(np.array([gain, (1.0, 0.0)]), (n, 1, 1)))
        out, count = align.pano_u8(bank, idx, M, Hc, Wc, feather, MODE_OF[mode], gain=g)
        assert torch.equal(out, want), (mode, feather, gain)
        assert torch.equal(count, (cover & 1) + (cover >> 1))


# ------------------------------------------------------------------------------------------------
# exact cases, bitwise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(17, 23), (48, 80)], ids=["17x23-scalar", "48x80-vector"])
def test_exact_cases_are_bitwise(h, w):
    A = Mc.textures(2, h, w, seed=1)
    eye = np.stack([np.eye(3)] * 2)[:, None]
    for mode in align.PANO_MODES:
        for feather in (1.0, 8.0, 64.0):
            out, count = run(A, np.arange(2).reshape(2, 1), eye, h, w, feather, mode)          # n = 1, M = I: the image
            assert np.array_equal(out, A) and np.all(count == 1), (mode, feather)
    out, count = run(A[:1], None, eye[:1], h, w)                          # no index list: frame k is image k
    assert np.array_equal(out, A[:1]) and np.all(count == 1)
    bank, idx, M = Pc.translation_case(h, w)
    use = np.array([[1, 0, 1]], np.uint8)
    for mode in align.PANO_MODES:
        for feather in (1.0, 4.0):
            out, count = run(bank, idx, M, h, w, feather, mode)
            want, want_count = align.pano_host(bank, idx, M, h, w, feather, mode)
            assert np.array_equal(out, want) and np.array_equal(count, want_count) and set(np.unique(count)) == {0, 1, 2, 3}, (mode, feather)
            assert not out[count == 0].any()
            out, count = run(bank, idx, M, h, w, feather, mode, use=use)  # one frame zeroed: the call without it
            want, want_count = run(bank, idx[:, [0, 2]], M[:, [0, 2]], h, w, feather, mode)
            assert np.array_equal(out, want) and np.array_equal(count, want_count) and count.max() == 2


def test_a_single_pixel_frame_and_a_vanishing_denominator():
    A = np.array([[[[200, 100, 50]]], [[[10, 20, 30]]]], np.uint8)        # two frames of one pixel each
    M = np.array([[[[0.5, 0, -1], [0, 0.5, -1], [0, 0, 1]], [[1.0, 0, -3], [0, 1, -2], [0, 0, 1]]]])      # at canvas (2, 2) and (3, 2)
    for Hc, Wc in ((5, 7), (4, 8)):
        out, count = run(A, np.array([[0, 1]]), M, Hc, Wc, 8.0, "feather")
        want, want_count = align.pano_host(A, [[0, 1]], M, Hc, Wc, 8.0, "feather")
        assert np.array_equal(out, want) and np.array_equal(count, want_count) and count.sum() == 2
        assert out[0, 2, 2].tolist() == [200, 100, 50] and out[0, 2, 3].tolist() == [10, 20, 30]
    bank = Mc.textures(2, 48, 80, seed=1)
    M = np.stack([np.array([[1.0, 0, 0], [0, 1, 0], [-0.125, 0, 1]]), np.eye(3)])[None]          # qz = 1 - x / 8: exactly 0 on the column x = 8
    for mode in align.PANO_MODES:
        out, count = run(bank, np.array([[0, 1]]), M, 48, 80, 8.0, mode)
        assert (count[0, :, 8] == 1).all() and (count[0, :, 0] == 2).all() and np.array_equal(out[0, :, 8], bank[1, :, 8]), mode
        assert np.array_equal(count, align.pano_host(bank, [[0, 1]], M, 48, 80, 8.0, mode)[1])


# ------------------------------------------------------------------------------------------------
# buffer contracts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_off,count_off", [(3, 1), (4, 1), (4, 8), (3, 4)],
                         ids=["out+3-count+1-scalar", "out+4-count+1-vector-byte-count", "out+4-count+8-vector", "out+3-count+4-scalar"])
def test_outputs_at_any_byte_offset_leave_their_surroundings_alone(out_off, count_off):
    bank, idx, _, M, Hc, Wc = Pc.case("n5-40x56-on-48x160")
    dbank, didx, dM = cuda(bank), cuda(idx, torch.int32), cuda(M)
    want, want_count = align.pano_u8(dbank, didx, dM, Hc, Wc, 8.0, "feather")
    n_out, n_count, tail = want.numel(), want_count.numel(), 16
    big_out = torch.full((out_off + n_out + tail,), 0xAB, dtype=torch.uint8, device="cuda")
    big_count = torch.full((count_off + n_count + tail,), 0xCD, dtype=torch.uint8, device="cuda")
    assert big_out.data_ptr() % 4 == 0 and big_count.data_ptr() % 4 == 0
    out, count = big_out[out_off:out_off + n_out].view(want.shape), big_count[count_off:count_off + n_count].view(want_count.shape)
    K.pano_u8(dbank, didx, dM, out, count, 8.0, "feather")
    assert torch.equal(out, want) and torch.equal(count, want_count)
    assert (big_out[:out_off] == 0xAB).all() and (big_out[out_off + n_out:] == 0xAB).all()
    assert (big_count[:count_off] == 0xCD).all() and (big_count[count_off + n_count:] == 0xCD).all()


def test_offsets_are_64_bit():
    """One bank whose last images start past 2^31 bytes: a 32-bit byte offset reads image 9,321 from the wrong place.  Integer
    translations, so the comparison with the host statement on the gathered images is bitwise."""
    data = torch.randint(0, 256, (N_BIG, 240, 320, 3), dtype=torch.uint8, device="cuda")
    assert data.numel() > 2 ** 31 and 9320 * 230400 < 2 ** 31 <= 9321 * 230400
    idx = np.array([[0, 9320, 9321], [N_BIG - 1, 9321, 0]])
    frames = host(data[torch.from_numpy(idx.reshape(-1)).cuda()])
    M = np.stack([np.array([[[1.0, 0, 4], [0, 1, 2], [0, 0, 1]], [[1.0, 0, -7], [0, 1, -5], [0, 0, 1]], [[1.0, 0, -100], [0, 1, 60], [0, 0, 1]]])] * 2)
    out, count = align.pano_u8(data, cuda(idx, torch.int32), cuda(M), 240, 320, 8.0, "feather")
    want, want_count = align.pano_host(frames, np.arange(6).reshape(2, 3), M, 240, 320, 8.0, "feather")
    assert np.array_equal(host(out), want) and np.array_equal(host(count), want_count)
    assert not np.array_equal(want[0], want[1]) and set(np.unique(want_count)) == {0, 1, 2, 3}      # (random bytes: an offset that wrapped would show)


def test_wild_indices_are_clamped():
    bank, _, M = Pc.translation_case()
    wild = torch.tensor([[-7, 1, 2 ** 30], [2, -2147483648, 2147483647]], dtype=torch.int32, device="cuda")
    M2 = np.concatenate([M, M])
    out, count = align.pano_u8(cuda(bank), wild, cuda(M2), 17, 23, 4.0, "feather")
    want, want_count = align.pano_host(bank, [[0, 1, 2], [2, 0, 2]], M2, 17, 23, 4.0, "feather")
    assert np.array_equal(host(out), want) and np.array_equal(host(count), want_count)


# ------------------------------------------------------------------------------------------------
# the chain and the frame, device twins
# ------------------------------------------------------------------------------------------------
def close(got, want, what):
    scale = np.abs(want).max(axis=tuple(range(1, want.ndim)), keepdims=True)
    assert np.isfinite(got).all() and np.all(np.abs(got - want) <= 1e-12 * scale), what


@pytest.mark.parametrize("n,ref", [(5, 0), (5, 2), (5, 4), (2, 1), (255, 100)])
def test_chain_device_equals_the_host_statement(n, ref):
    B = 3
    Hp = np.stack([[Mc.corner_homography(51 + 7 * b + (j % 11), 40, 56, 40, 56, 0.02 if n > 5 else 0.1) for j in range(n - 1)] for b in range(B)])
    gp = np.random.RandomState(2).uniform(0.95, 1.05, (B, n - 1, 2)) * np.array([1.0, 2.0])
    G, gain = align.chain_device(cuda(Hp), ref, cuda(gp))
    wG, wgain = align.chain_host(Hp, ref, gp)
    assert G.shape == (B, n, 3, 3) and gain.shape == (B, n, 2) and G.dtype == gain.dtype == torch.float64
    close(host(G).reshape(B * n, 3, 3), wG.reshape(B * n, 3, 3), "G")
    close(host(gain).reshape(B * n, 2), wgain.reshape(B * n, 2), "gain")
    assert torch.equal(G[:, ref], torch.eye(3, dtype=torch.float64, device="cuda").expand(B, 3, 3)) and (host(G)[:, :, 2, 2] == 1.0).all()
    G2, none = align.chain_device(cuda(Hp), ref)
    assert none is None and torch.equal(G2, G)


def test_chain_of_one_frame_is_the_identity():
    G, gain = align.chain_device(torch.empty((2, 0, 3, 3), dtype=torch.float64, device="cuda"), 0, torch.empty((2, 0, 2), dtype=torch.float64, device="cuda"))
    assert host(G).tolist() == [[np.eye(3).tolist()]] * 2 and host(gain).tolist() == [[[1.0, 0.0]]] * 2


def test_frame_device_equals_the_host_statement(monkeypatch):
    p = poisoned_alloc.poison(monkeypatch, align)
    size = (40, 56)
    _, _, G5, _, _, _ = Pc.case("n5-40x56-on-48x160")
    odd = [HORIZON, GARBAGE, np.zeros((3, 3)), np.full((3, 3), np.nan), np.array([[1.0, 0, 1e6], [0, 1, -1e6], [0, 0, 1]])]
    G = np.stack([G5[0], G5[1]] + [np.stack([G5[0, 0], m, np.eye(3), G5[0, 3], G5[0, 4]]) for m in odd])      # [7,5,3,3]
    use = np.ones((7, 5), np.uint8)
    use[1, 4] = use[3, 0] = 0
    for canvas, limit, u in (((48, 160), 2.0, None), ((37, 131), 0.5, use), ((2, 2), 2.0, use)):
        T, bbox, fitted, M = align.pano_frame_device(cuda(G), size, canvas, limit, use=None if u is None else cuda(u))
        wT, wbbox, wfitted = align.pano_frame_host(G, size, canvas, limit, use=u)
        assert T.shape == (7, 3, 3) and bbox.shape == (7, 4) and fitted.shape == (7, 5) and M.shape == (7, 5, 3, 3) and fitted.dtype == torch.uint8
        assert host(fitted).tolist() == wfitted.tolist() and wfitted[2:, 1].tolist() == [0, 1, 0, 0, 1]
        close(host(T), wT, "T")
        close(host(bbox), wbbox, "bbox")
        ok = np.isfinite(G).all((2, 3))                                    # (M of a frame that is not finite is not)
        close(host(M)[ok], (G @ wT[:, None])[ok], "M")
    assert p.verify() == 12
    ref_size = (48, 80)                                                    # a reference of another size than the frames: one launch of seven workgroups
    T, bbox, fitted, M = align.pano_frame_device(cuda(G), size, (48, 160), 2.0, use=cuda(use), ref_size=ref_size)
    wT, wbbox, wfitted = align.pano_frame_host(G, size, (48, 160), 2.0, use=use, ref_size=ref_size)
    assert host(fitted).tolist() == wfitted.tolist() and wfitted[2:, 1].tolist() == [0, 1, 0, 0, 1]
    assert np.all(wbbox[:, 2] >= 79) and np.all(wbbox[:, 3] >= 47) and wbbox[3].tolist()[2:] == [3 * 80 - 1, 3 * 48 - 1]      # the reference's extent and clamp
    close(host(T), wT, "T")
    close(host(bbox), wbbox, "bbox")
    close(host(M)[ok], (G @ wT[:, None])[ok], "M")
    assert p.verify() == 4
    for n in (1, 255):                                                     # the fewest and the most frames a workgroup takes
        Gn = np.stack([np.eye(3) if k == n // 2 else Mc.corner_homography(k, 40, 56, 40, 56, 0.3) for k in range(n)])[None]
        T, bbox, fitted, M = align.pano_frame_device(cuda(Gn), size, (48, 160))
        wT, wbbox, wfitted = align.pano_frame_host(Gn, size, (48, 160))
        assert host(fitted).tolist() == wfitted.tolist() and wfitted[0, n // 2] == 1 and wfitted.sum() >= 0.9 * n      # (some of the 255 are not usable)
        close(host(T), wT, "T")
        close(host(bbox), wbbox, "bbox")
        close(host(M)[0], (Gn @ wT[:, None])[0], "M")
    with pytest.raises(ValueError):
        align.pano_frame_device(cuda(G), size, (1, 96))


# ------------------------------------------------------------------------------------------------
# panorama() and Aligner.sequence
# ------------------------------------------------------------------------------------------------
PANO_KEYS = {"panorama", "panorama_count", "panorama_T", "panorama_bbox", "panorama_fitted", "panorama_M", "panorama_gain"}
SEQ_KEYS = {"G", "H_pairs", "pairs", "pair"}


def stub_aligner(delta, P=32):
    return align.Aligner(torch.nn.Sequential(Mc.StubHead(cuda(delta, torch.float32))), patch=P)


def test_panorama_on_the_reference_grid_and_on_a_fitted_canvas():
    bank, idx, G, M, Hc, Wc = Pc.case("n5-40x56-on-48x160")
    dbank, dG = cuda(bank), cuda(G)
    r = align.panorama(dbank, dG, idx=idx, canvas=(Hc, Wc), feather=8.0)
    assert set(r) == PANO_KEYS
    for k, shape, dtype in (("panorama", (2, Hc, Wc, 3), torch.uint8), ("panorama_count", (2, Hc, Wc), torch.uint8), ("panorama_T", (2, 3, 3), torch.float64),
                            ("panorama_bbox", (2, 4), torch.float64), ("panorama_fitted", (2, 5), torch.uint8), ("panorama_M", (2, 5, 3, 3), torch.float64),
                            ("panorama_gain", (2, 5, 2), torch.float64)):
        assert tuple(r[k].shape) == shape and r[k].dtype == dtype and r[k].is_cuda, k
    close(host(r["panorama_M"]).reshape(10, 3, 3), M.reshape(10, 3, 3), "M")
    assert host(r["panorama_fitted"]).all() and host(r["panorama_gain"]).tolist() == [[[1.0, 0.0]] * 5] * 2
    want, want_count = Pc.reference("n5-40x56-on-48x160", "feather", 8.0, False)
    d, share = Mc.differing_share(host(r["panorama"]), want)
    _, near = Pc.near_border("n5-40x56-on-48x160")
    assert d <= 1 and share <= CAP and np.array_equal(host(r["panorama_count"])[~near], want_count[~near])
    # the reference's grid: T = I, M = G, no frame launch; the reference's pixels where it alone is
    on_ref = align.panorama(dbank, dG, idx=cuda(idx, torch.int32), canvas="ref", mode="first", use=cuda(np.array([[0, 0, 1, 0, 0]] * 2, np.uint8)))
    assert torch.equal(on_ref["panorama_M"], dG) and torch.equal(on_ref["panorama_T"], torch.eye(3, dtype=torch.float64, device="cuda").expand(2, 3, 3))
    assert torch.equal(on_ref["panorama"], dbank[cuda(idx[:, 2])]) and (on_ref["panorama_count"] == 1).all() and not on_ref["panorama_fitted"].any()
    assert host(on_ref["panorama_bbox"]).tolist() == [[0, 0, 55, 39]] * 2


def test_sequence_with_a_stub_model():
    frames, deltas, H_pairs, G_true = Pc.aligner_sequence()
    n, ref, (Hs, Ws) = 4, 1, frames.shape[1:3]
    aligner, bank = stub_aligner(deltas), cuda(frames)
    r = aligner.sequence(bank, ref=ref)
    assert set(r) == SEQ_KEYS and r["pairs"] == align.pairs_of(n, ref) == [(0, 1), (2, 1), (3, 2)]
    assert r["G"].shape == (1, n, 3, 3) and r["H_pairs"].shape == (1, n - 1, 3, 3) and r["G"].dtype == torch.float64
    assert "aligned" not in r["pair"] and torch.equal(r["pair"]["H"].view(1, n - 1, 3, 3), r["H_pairs"])
    Hp, G = host(r["H_pairs"]), host(r["G"])
    rel_h = max(np.abs(Hp[0, j] - H_pairs[0, j]).max() / np.abs(H_pairs[0, j]).max() for j in range(n - 1))
    assert rel_h <= 1e-8                                                   # test_align_gpu.py's bound on the device lift
    close(G[0], align.chain_host(Hp, ref)[0], "G against the chain of the device's own pairs")
    # against the chain of the lifted deltas: m factors, each within 1e-8 of its largest entry, to first order (|A B|max <= 3 |A|max |B|max)
    for k in range(n):
        path = list(range(ref, k)) if k > ref else list(range(k, ref))
        bound = 1e-8 * len(path) * 3.0 ** max(len(path) - 1, 0) * np.prod([np.abs(H_pairs[0, j]).max() for j in path])
        err = np.abs(G[0, k] - G_true[0, k]).max()
        print("sequence: frame %d, max |G - G_true| = %.3e (bound %.3e)" % (k, err, bound))
        assert err <= bound and G[0, k, 2, 2] == 1.0
    # one pair call for all pairs: the pair call on the same index lists gives the same bits
    ia, ib = (torch.tensor(c, dtype=torch.int32, device="cuda") for c in zip(*r["pairs"]))
    pair = aligner(bank, bank, idx_a=ia, idx_b=ib, warp=False)
    assert torch.equal(pair["H"], r["pair"]["H"])
    # with a canvas: the panorama of G, the public function's bits
    Hc, Wc = 120, 320
    s = aligner.sequence(bank, ref=ref, canvas=(Hc, Wc), feather=16.0)
    assert set(s) == SEQ_KEYS | PANO_KEYS and torch.equal(s["G"], r["G"])
    m = align.panorama(bank, r["G"], canvas=(Hc, Wc), feather=16.0)
    assert all(torch.equal(m[k], s[k]) for k in PANO_KEYS)
    T = host(s["panorama_T"])
    want, want_count = align.pano_host(frames, np.arange(n)[None], G @ T[:, None], Hc, Wc, 16.0)
    d, share = Mc.differing_share(host(s["panorama"]), want)
    near = np.any([Mc.near_border((G @ T[:, None])[:, k], Hc, Wc, Hs, Ws) for k in range(n)], 0)
    print("sequence, fitted %d x %d: max |difference| %d, %.2e of the pixels differ (cap %.0e); count compared on all but %.2e; at most %d frames"
          % (Hc, Wc, d, share, CAP, near.mean(), want_count.max()))
    assert d <= 1 and share <= CAP and near.mean() <= 5e-3 and np.array_equal(host(s["panorama_count"])[~near], want_count[~near]) and want_count.max() >= 3
    # the frames come from one texture: where frames overlap they agree, so the blend is close to each of them
    both = s["panorama_count"] >= 2
    ref_only = align.panorama(bank, r["G"], canvas=(Hc, Wc), mode="first")["panorama"]
    assert (s["panorama"].int() - ref_only.int()).abs()[both].float().mean().item() < 3.0
    # n = 1 runs no model
    one = aligner.sequence(bank, idx=[[2]], canvas="ref")
    assert one["pairs"] == [] and one["pair"] == {} and one["H_pairs"].shape == (1, 0, 3, 3) and host(one["G"]).tolist() == [[np.eye(3).tolist()]]
    assert torch.equal(one["panorama"], bank[2:3])


def test_sequence_exposure_gain_composes_the_pair_lines():
    frames, deltas, _, _ = Pc.aligner_sequence()
    lines = [(1.0, 0.0), (1.0, 0.0), (0.9, 8.0), (0.8, 12.0)]             # frame k = round(g_k reference-exposed frame + o_k) ...
    dark = np.stack([np.floor(np.clip(g * frames[k].astype(np.float64) + o, 0, 255) + 0.5).astype(np.uint8) for k, (g, o) in enumerate(lines)])
    aligner = stub_aligner(deltas)
    r = aligner.sequence(cuda(dark), ref=1, canvas="ref", exposure="gain")
    gain = host(r["panorama_gain"])[0]
    print("sequence, exposure 'gain': %s" % (gain.tolist(),))
    for k, (g, o) in enumerate(lines):                                     # ... so its line back to the reference is (1 / g_k, -o_k / g_k)
        assert abs(gain[k, 0] - 1 / g) <= 3e-2 / g and abs(gain[k, 1] + o / g) <= 3.0, k
    assert gain[1].tolist() == [1.0, 0.0]
    given = cuda(np.tile(np.array([[1.0, 0.0], [1.0, 0.0], [1.1, -9.0], [1.2, -15.0]]), (1, 1, 1)))
    g2 = aligner.sequence(cuda(dark), ref=1, canvas="ref", exposure=given)
    assert torch.equal(g2["panorama_gain"], given)
    # a mask of ones counts the pixels no mask counts; with refine='ecc' every pair is refined and the chain is of the refined pairs
    ones = torch.ones((1, 4) + dark.shape[1:3], dtype=torch.uint8, device="cuda")
    masked = aligner.sequence(cuda(dark), ref=1, canvas="ref", exposure="gain", mask=ones)
    assert np.abs(host(masked["panorama_gain"]) - host(r["panorama_gain"])).max() <= 1e-9
    fine = aligner.sequence(cuda(dark), ref=1, refine="ecc", refine_levels=2, refine_iters=2, mask=ones)
    assert {"H_model", "rho", "refine_stats"} <= set(fine["pair"]) and torch.equal(fine["pair"]["H"].view(1, 3, 3, 3), fine["H_pairs"])
    close(host(fine["G"])[0], align.chain_host(host(fine["H_pairs"]), 1)[0], "G of the refined pairs")


def test_arguments_are_refused_before_any_launch(monkeypatch):
    launches = []
    for name in ("align_prep_u8", "pano_u8", "pano_chain", "pano_frame", "gray_pyramid_u8"):
        fn = getattr(K, name)
        monkeypatch.setattr(K, name, lambda *a, _fn=fn, **k: launches.append(1) or _fn(*a, **k))
    frames, deltas, _, _ = Pc.aligner_sequence()
    aligner, bank = stub_aligner(deltas), cuda(frames)
    G = torch.eye(3, dtype=torch.float64, device="cuda").repeat(1, 4, 1, 1)
    small = cuda(Mc.pixels(4, 7, 40))
    shared = (dict(canvas="b"), dict(canvas=True), dict(canvas=(64,)), dict(canvas=(64.5, 96)), dict(canvas=(1, 96)), dict(canvas="ref", feather=float("nan")),
              dict(canvas="ref", feather=0.5), dict(canvas="ref", feather=None), dict(canvas="ref", mode="a_over_b"), dict(canvas="ref", mode=0),
              dict(canvas=(64, 96), limit=0.0), dict(canvas=(64, 96), limit=float("nan")), dict(canvas="ref", use=torch.ones(1, 4, dtype=torch.uint8)),
              dict(canvas="ref", use=torch.ones(1, 3, dtype=torch.uint8, device="cuda")), dict(canvas="ref", idx=[[0, 1, 2, 4]]), dict(canvas="ref", idx=[0, 1, 2, 3]))
    for kw in shared:
        with pytest.raises(ValueError):
            aligner.sequence(bank, **kw)
        with pytest.raises(ValueError):
            align.panorama(bank, G, **kw)
    for kw in (dict(ref=4), dict(ref=-1), dict(ref=1.5), dict(refine="lk"), dict(cascade=-1), dict(cascade_min_cover=2.0), dict(cascade_samples=(0, 1)),
               dict(refine="ecc", refine_levels=9), dict(roi=(0, 0, 200, 50)), dict(roi=np.zeros((2, 4))), dict(exposure="gain"), dict(use=torch.ones(1, 4, dtype=torch.uint8, device="cuda")),
               dict(canvas="ref", exposure="auto"), dict(canvas="ref", exposure=torch.ones(1, 4, 2, device="cuda")), dict(canvas="ref", mask=torch.ones(1, 4, 96, 128, dtype=torch.uint8, device="cuda")),
               dict(idx=torch.zeros(4, dtype=torch.int32, device="cuda")), dict(idx=np.zeros((1, 256), np.int64))):
        with pytest.raises(ValueError):
            aligner.sequence(bank, **kw)
    with pytest.raises(ValueError, match="7 x 40"):
        aligner.sequence(small, canvas="ref", exposure="gain")
    for kw in (dict(gain=torch.ones(1, 4, 2, dtype=torch.float64)), dict(gain=torch.ones(1, 4, 2, device="cuda")), dict(idx=[[0, 1, 2]])):
        with pytest.raises(ValueError):
            align.panorama(bank, G, **kw)
    with pytest.raises(ValueError):
        align.panorama(bank, G[:, :, :2])
    assert not launches                                                    # every refusal came before any launch
    assert set(aligner.sequence(bank, canvas="ref")) == SEQ_KEYS | PANO_KEYS and launches
