"""The global adjustment on the device (csrc/adjust.hip: bh_pano_adjust; bihome_amd/align.py adjust_device / adjust, Aligner(init=),
Aligner.sequence(links=)) against the numpy float64 statement align.adjust_host, which tests/test_align_adjust_cpu.py holds to an
independent restatement.

Bound.  The measure is the corner distance in the reference's pixels (tests/align_adjust_cases.py corner_distance) after three steps,
every one of which the statement accepts by a wide margin (test_align_adjust_cpu.py asserts the margins), and the cap is
max(100 d_cpu, 1e-9) px with d_cpu what the statement itself moves by when its Cholesky is replaced by np.linalg.solve on exactly these
inputs; the factor of 100 covers the other summation order of J^T J and the blocked factorisation.  `work` agrees in the accepted steps
and the final lambda exactly and in both costs to 1e-9 relative, with one exception that is decided from the case's edge list and weights
alone (tests/align_adjust_cases.py counting_edges_form_a_forest; which samples those are is stated per case in FOREST_SAMPLES and asserted):
where the counting edges form no cycle every residual can be driven to zero, the cost at the result tends to the rounding of its own
evaluation, and no two evaluations agree on it to 1e-9 of itself (the statement's own two solvers differ by 1.4e-8 of it at n = 2).
There the two costs agree to an ABSOLUTE figure derived from that rounding and from the corner cap the iterates are held to
(forest_cost_slack: 7e-17 px^2 at n = 2, where 1e-9 of the cost would be 1e-26); everywhere else the bound is 1e-9 of the cost itself."""
import numpy as np
import pytest
import torch

import align_adjust_cases as C
import align_mosaic_cases as Mc
import align_pano_cases as Pc
import poisoned_alloc
from bihome_amd import align
from bihome_amd import kernels as K

pytestmark = pytest.mark.gpu


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def run(G0, edges, H_edges, weight, ref, grid, iters, size=C.SIZE):
    G, work = align.adjust_device(cuda(G0), cuda(np.asarray(edges, np.int32).reshape(-1, 2)), cuda(H_edges), None if weight is None else cuda(weight), ref,
                                  size, grid, iters)
    return host(G), host(work)


# ------------------------------------------------------------------------------------------------
# the kernel against adjust_host
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.DEVICE_CASES))
def test_adjust_matches_the_host_statement(monkeypatch, name):
    p = poisoned_alloc.poison(monkeypatch, align)          # G, work and the workspace handed out NaN-filled between red zones
    G0, edges, H_edges, weight, ref, grid = C.device_case(name)
    want, want_work = C.device_reference(name)
    G, work = run(G0, edges, H_edges, weight, ref, grid, C.DEVICE_ITERS)
    assert p.verify() == 3 and {"adjust_device"} <= p.callers()
    d, cap = C.corner_distance(G, want).max(), C.cap(name)
    print("%s: %.2e px from the statement at the corners (cap %.2e, d_cpu %.2e); work %s" % (name, d, cap, C.d_cpu(name), work.tolist()))
    assert d <= cap
    assert np.array_equal(work[:, 2:], want_work[:, 2:]) and (work[:, 2] == C.DEVICE_ITERS).all()
    assert np.all(np.abs(work[:, 0] - want_work[:, 0]) <= 1e-9 * want_work[:, 0])
    forest = C.forest_samples(name)
    assert forest == C.FOREST_SAMPLES[name]
    for s_, tree in enumerate(forest):
        diff = abs(work[s_, 1] - want_work[s_, 1])
        if tree:
            slack = C.forest_cost_slack(name, s_, work[s_, 1], want_work[s_, 1])
            print("%s, sample %d (a forest): cost at the result %.3e, %.2e px^2 from the statement's (slack %.2e)" % (name, s_, work[s_, 1], diff, slack))
            assert diff <= slack
        else:
            print("%s, sample %d: cost at the result %.6g, %.2e of it from the statement's" % (name, s_, work[s_, 1], diff / want_work[s_, 1]))
            assert diff <= 1e-9 * want_work[s_, 1]
    assert np.array_equal(G[:, ref], np.tile(np.eye(3), (3, 1, 1))) and np.all(G[:, :, 2, 2] == 1.0)


@pytest.mark.parametrize("n", [6, 9])
def test_consistent_edges_reach_the_truth_on_the_device(n):
    worst = 0.0
    for seed in range(3):
        G_true, G0, edges, H_edges = C.consistent(n, seed)
        G, work = run(G0[None], edges, H_edges[None], None, n // 2, 4, 10)
        worst = max(worst, C.corner_distance(G[0], G_true).max())
        assert work[0, 2] >= 3 and work[0, 1] < 1e-20 * work[0, 0]
    print("consistent edges on the device, n = %d: %.2e px from the truth after 10 steps (the statement: %.1e)" % (n, worst, C.REACHED[n]))
    assert worst <= 10 * C.REACHED[n]


# ------------------------------------------------------------------------------------------------
# bit for bit
# ------------------------------------------------------------------------------------------------
def test_bitwise_contracts():
    G0, edges, H_edges, weight, ref, grid = C.device_case("n16-ref0-grid4")
    G, work = run(G0, edges, H_edges, weight, ref, grid, 3)
    again, work2 = run(G0, edges, H_edges, weight, ref, grid, 3)
    assert G.tobytes() == again.tobytes() and work.tobytes() == work2.tobytes()          # two calls
    # iters = 0: the start, and two equal costs
    same, w0 = run(G0, edges, H_edges, weight, ref, grid, 0)
    assert same.tobytes() == G0.tobytes() and np.array_equal(w0[:, 0], w0[:, 1]) and np.array_equal(w0[:, 0], work[:, 0])
    assert (w0[:, 2] == 0).all() and (w0[:, 3] == 1e-3).all()
    # a NaN sample, a singular one and one whose links all have weight 0 next to a healthy one
    alone, alone_work = run(G0[:1], edges, H_edges[:1], weight[:1], ref, grid, 3)
    assert alone.tobytes() == G[:1].tobytes() and alone_work.tobytes() == work[:1].tobytes()
    nan_G, singular = G0[0].copy(), G0[0].copy()
    nan_G[7, 0, 1] = np.nan
    singular[9] = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    nan_H = H_edges[0].copy()
    nan_H[16, 1, 1] = np.nan                                                   # (a link's)
    no_links = np.array([1.0] * 15 + [0.0] * 4)
    batch_G = np.stack([nan_G, G0[0], singular, G0[0], G0[0]])
    batch_H = np.stack([H_edges[0], H_edges[0], H_edges[0], H_edges[0], nan_H])
    batch_w = np.stack([weight[0], weight[0], weight[0], no_links, weight[0]])
    mixed, mixed_work = run(batch_G, edges, batch_H, batch_w, ref, grid, 3)
    assert mixed[1].tobytes() == G[0].tobytes() and mixed_work[1].tobytes() == work[0].tobytes()
    for s in (0, 2, 4):
        assert mixed[s].tobytes() == batch_G[s].tobytes() and np.isnan(mixed_work[s, :2]).all() and mixed_work[s, 2] == 0 and mixed_work[s, 3] == 1e-3, s
    moved = C.corner_distance(mixed[3], G0[0]).max()
    print("links without weight on the device: the chain moves by %.2e px, costs %s" % (moved, mixed_work[3].tolist()))
    # the pushed start goes back to where its own pairs put it, as the statement says: the bound of the kernel cases, on this sample
    want3 = [align.adjust_host(G0[:1], edges, H_edges[:1], no_links[None], ref, C.SIZE, grid, 3, solver=sv) for sv in ("cholesky", "solve")]
    cap3 = max(100.0 * C.corner_distance(want3[0][0], want3[1][0]).max(), 1e-9)
    d3 = C.corner_distance(mixed[3], want3[0][0][0]).max()
    print("links without weight on the device: %.2e px from the statement (cap %.2e)" % (d3, cap3))
    assert d3 <= cap3 and np.array_equal(mixed_work[3, 2:], want3[0][1][0, 2:]) and mixed_work[3, 1] < mixed_work[3, 0]
    # ... and with the NaN link switched off the sample is the healthy one's, to the bit
    batch_w[4, 16] = 0.0
    healthy_w = weight[0].copy()
    healthy_w[16] = 0.0
    off, off_work = run(batch_G, edges, batch_H, batch_w, ref, grid, 3)
    want, want_work = run(G0[:1], edges, H_edges[:1], healthy_w[None], ref, grid, 3)
    assert off[4].tobytes() == want[0].tobytes() and off_work[4].tobytes() == want_work[0].tobytes()
    # an edge with a == b or an index out of range changes nothing
    more = edges + [(3, 3), (16, 0), (-1, 2), (2, 64)]
    H_more = np.concatenate([H_edges, np.full((3, 4, 3, 3), np.nan)], 1)
    w_more = np.concatenate([weight, np.ones((3, 4))], 1)
    G_more, work_more = run(G0, more, H_more, w_more, ref, grid, 3)
    assert G_more.tobytes() == G.tobytes() and work_more.tobytes() == work.tobytes()
    # weight None is all ones
    ones, ones_work = run(G0, edges, H_edges, np.ones_like(weight), ref, grid, 3)
    none, none_work = run(G0, edges, H_edges, None, ref, grid, 3)
    assert ones.tobytes() == none.tobytes() and ones_work.tobytes() == none_work.tobytes()


def test_the_chain_alone_stays_where_it_is_on_the_device():
    G_true, G0, edges, H_edges = C.there_and_back(8, 1)
    weight = np.array([1.0] * 7 + [0.0] * (len(edges) - 7))
    G, work = run(G0[None], edges, H_edges[None], weight[None], 0, 4, 10)
    moved = C.corner_distance(G[0], G0).max()
    print("link weights all 0 on the device: the chain moves by %.2e px (cost at the start %.2e)" % (moved, work[0, 0]))
    assert moved <= 1e-11 and work[0, 0] <= 1e-20


# ------------------------------------------------------------------------------------------------
# the public function
# ------------------------------------------------------------------------------------------------
def test_adjust_is_the_device_path_and_refuses_before_any_launch(monkeypatch):
    G0, edges, H_edges, weight, ref, grid = C.device_case("n16-ref0-grid4")
    dG, dH, dw = cuda(G0), cuda(H_edges), cuda(weight)
    r = align.adjust(dG, edges, dH, C.SIZE, ref, weight=dw, grid=grid, iters=3)
    G, work = run(G0, edges, H_edges, weight, ref, grid, 3)
    assert set(r) == {"G", "adjust_stats"} and host(r["G"]).tobytes() == G.tobytes() and host(r["adjust_stats"]).tobytes() == work.tobytes()
    assert r["G"].shape == (3, 16, 3, 3) and r["adjust_stats"].shape == (3, 4) and r["G"].dtype == r["adjust_stats"].dtype == torch.float64
    launches = []
    fn = K.pano_adjust
    monkeypatch.setattr(K, "pano_adjust", lambda *a, **k: launches.append(1) or fn(*a, **k))
    p = poisoned_alloc.poison(monkeypatch, align)
    for kw in (dict(links=edges + [(3, 3)]), dict(links=edges + [(16, 0)]), dict(links=edges[:-1]), dict(links=[]), dict(grid=1), dict(grid=9), dict(iters=-1),
               dict(ref=16), dict(ref=-1), dict(size=(48,)), dict(size=(1, 64)), dict(weight=dw[:, :5]), dict(weight=weight), dict(weight=dw.float()),
               dict(H_links=dH[:2]), dict(H_links=dH.float()), dict(G=dG.float()), dict(G=dG[:, :, :2])):
        args = dict(G=dG, links=edges, H_links=dH, size=C.SIZE, ref=ref, weight=dw, grid=grid, iters=3)
        args.update(kw)
        with pytest.raises(ValueError):
            align.adjust(**args)
    assert not launches and len(p) == 0                                        # every refusal came before any launch and any allocation
    assert set(align.adjust(dG, edges, dH, C.SIZE, ref)) == {"G", "adjust_stats"} and launches and p.verify() == 3


# ------------------------------------------------------------------------------------------------
# Aligner(init=)
# ------------------------------------------------------------------------------------------------
def stub_aligner(delta, P=32):
    return align.Aligner(torch.nn.Sequential(Mc.StubHead(cuda(delta, torch.float32))), patch=P)


def test_aligner_starts_the_cascade_from_init():
    A, B_img, delta, H_true = Mc.aligner_pair()
    a, b = cuda(A), cuda(B_img[None] if B_img.ndim == 3 else B_img)
    aligner = stub_aligner(delta)
    before = aligner(a, b, cascade=1)                                          # made before the keyword is touched
    none = aligner(a, b, cascade=1, init=None)
    assert set(none) == set(before) and all(torch.equal(none[k], before[k]) for k in before)
    zero = stub_aligner(np.zeros((1, 4, 2)))
    init = cuda(H_true)
    r = zero(a, b, cascade=2, init=init, warp=False)
    assert set(r) == (set(before) - {"geom_a", "aligned", "valid"})
    assert torch.equal(r["H_stages"][:, 0], init) and (r["accepted"][:, 0] == 1).all()
    # H is init: bit for bit where no later stage was taken; a stage that was (its score rose by rounding alone) composed a zero delta,
    # init A_b I A_b^-1 / [2,2] - two 3 x 3 products and a division, each entry a few ulp of the largest, far inside 1e-12 of it
    kept = (r["accepted"][:, 1:] == 0).all(1)
    assert torch.equal(r["H"][kept], init[kept])
    assert (r["H"] - init).abs().max().item() <= 1e-12 * init.abs().max().item()
    assert r["H_stages"].shape == (1, 3, 3, 3) and not r["delta_hat"].any() and not r["delta_stages"][:, 0].any()
    # patch_1 is A seen through init, and the score of stage 0 its correlation with patch_2
    P = 32
    nx, ny = align._cascade_samples(None, None, b.shape[1], b.shape[2], P)
    seen, cover = align.prepare_warped(a, (init @ align._grid_map_device(r["geom_b"], nx, ny)).contiguous(), 1, P, 1, nx, ny)
    assert torch.equal(r["patch_1"], seen) and torch.equal(r["score"][:, 0], align.patch_ncc(seen, r["patch_2"], cover)[:, 6])
    assert r["score"][0, 0].item() > 0.9                                       # (init is the truth)
    assert zero.model[0].seen["patch_1"].shape == (1, 1, P, P)                 # the model saw warped patches only: two calls, both of the cascade
    for kw in (dict(cascade=0), dict(roi_a=(0, 0, 64, 64)), dict(init=H_true), dict(init=init.float()), dict(init=init[0]), dict(init=init.repeat(2, 1, 1))):
        args = dict(cascade=1, init=init)
        args.update(kw)
        with pytest.raises(ValueError):
            zero(a, b, **args)


# ------------------------------------------------------------------------------------------------
# Aligner.sequence(links=)
# ------------------------------------------------------------------------------------------------
SEQ_KEYS = {"G", "H_pairs", "pairs", "pair"}
LINK_KEYS = {"G_chain", "links", "link", "H_links", "link_score", "link_weight", "adjust_stats"}
PANO_KEYS = {"panorama", "panorama_count", "panorama_T", "panorama_bbox", "panorama_fitted", "panorama_M", "panorama_gain"}


class PairsThenZeros(torch.nn.Module):
    """The pair call's deltas for a batch of their size, zeros for any other batch (the link call)."""

    def __init__(self, delta):
        super().__init__()
        self.delta = delta

    def predict_homography(self, data):
        B = data["patch_2"].shape[0]
        return (self.delta if B == self.delta.shape[0] else torch.zeros((B, 4, 2), dtype=torch.float32, device=self.delta.device)), None


def there_and_back_frames(n=6, size=(96, 128), P=32, back=True, stride=0.2):
    """align_pano_cases.aligner_sequence's construction, there and back (back=False: one way): frames cut from one texture along a sweep
    that returns, the stub's pair deltas the true ones plus a known error on the 1/16-pixel grid.  -> (frames uint8 [n,Hs,Ws,3], deltas
    [n-1,4,2], G_true [n,3,3])"""
    Hs, Ws = size
    base = Pc.textures(1, 3 * Hs, 4 * Ws, seed=5)
    rng = np.random.RandomState(11)
    ref, geom = 0, Pc.whole_geom(Hs, Ws, P, n - 1)
    step = np.array([-stride * P, 0.0])                                        # a pair moves the patch by this share of its side
    true = np.stack([np.round((np.tile(step if j < (n - 1) / 2 or not back else -step, (4, 1)) + rng.uniform(-0.03 * P, 0.03 * P, (4, 2))) * 16) / 16
                     for j in range(n - 1)])
    error = np.round(rng.uniform(-0.02 * P, 0.02 * P, (n - 1, 4, 2)) * 16) / 16
    G_true = align.chain_host(align.lift(true, P, geom, geom)[None], ref)[0]
    centre = np.array([[1.0, 0, 0.5 * Ws], [0, 1.0, Hs], [0, 0, 1.0]])
    frames = np.concatenate([align.warp_u8_host(base, (centre @ np.linalg.inv(G_true[k]))[None], Hs, Ws)[0] for k in range(n)])
    return frames, true + error, G_true


def test_sequence_closes_the_loop_with_links(monkeypatch):
    n, ref, P = 6, 0, 32
    frames, deltas, G_true = there_and_back_frames(n)
    Hs, Ws = frames.shape[1:3]
    bank = cuda(frames)
    aligner = align.Aligner(torch.nn.Sequential(PairsThenZeros(cuda(deltas, torch.float32))), patch=P)
    idx = [[0, 1, 2, 3, 4, 5]]
    plain = aligner.sequence(bank, idx=idx, ref=ref)
    none = aligner.sequence(bank, idx=idx, ref=ref, links=None)
    empty = aligner.sequence(bank, idx=idx, ref=ref, links=[])
    for r in (none, empty):
        assert set(r) == SEQ_KEYS == set(plain) and torch.equal(r["G"], plain["G"]) and torch.equal(r["H_pairs"], plain["H_pairs"])
        assert set(r["pair"]) == set(plain["pair"]) and all(torch.equal(r["pair"][k], plain["pair"][k]) for k in plain["pair"])
    links = [(5, 0), (4, 1)]
    s = aligner.sequence(bank, idx=idx, ref=ref, links=links, canvas=(120, 320), feather=16.0)
    assert set(s) == SEQ_KEYS | LINK_KEYS | PANO_KEYS and s["links"] == links
    for k, shape in (("G", (1, n, 3, 3)), ("G_chain", (1, n, 3, 3)), ("H_links", (1, 2, 3, 3)), ("link_score", (1, 2)), ("link_weight", (1, 2)), ("adjust_stats", (1, 4))):
        assert tuple(s[k].shape) == shape and s[k].dtype == torch.float64 and s[k].is_cuda, k
    assert torch.equal(s["G_chain"], plain["G"]) and torch.equal(s["H_pairs"], plain["H_pairs"])
    assert {"H_stages", "score", "accepted"} <= set(s["link"]) and "aligned" not in s["link"] and torch.equal(s["link"]["H"].view(1, 2, 3, 3), s["H_links"])
    print("sequence with links: scores %s, weights %s, adjust_stats %s" % (host(s["link_score"]).tolist(), host(s["link_weight"]).tolist(), host(s["adjust_stats"]).tolist()))
    assert host(s["link_weight"]).tolist() == [[1.0, 1.0]]
    # G is align.adjust of the same inputs, and the panorama align.panorama of G
    edges = s["pairs"] + links
    same = align.adjust(s["G_chain"], edges, torch.cat([s["H_pairs"], s["H_links"]], 1), (Hs, Ws), ref,
                        weight=torch.cat([torch.ones((1, n - 1), dtype=torch.float64, device="cuda"), s["link_weight"]], 1))
    assert torch.equal(same["G"], s["G"]) and torch.equal(same["adjust_stats"], s["adjust_stats"])
    m = align.panorama(bank, s["G"], idx=idx, canvas=(120, 320), feather=16.0)
    assert all(torch.equal(m[k], s[k]) for k in PANO_KEYS)
    # the zero-delta link through the chain's estimate carries the chain's error; the statement on the same inputs agrees with the device
    want, want_work = align.adjust_host(host(s["G_chain"]), edges, host(torch.cat([s["H_pairs"], s["H_links"]], 1)), None, ref, (Hs, Ws))
    assert C.corner_distance(host(s["G"]), want, (Hs, Ws)).max() <= 1e-6 and abs(host(s["adjust_stats"])[0, 0] - want_work[0, 0]) <= 1e-6
    # one way, 5 steps of 0.24 P: frames 0 and 5 lie 1.2 frame widths apart and share no pixel - that link fails the cover test and drops out
    frames1, deltas1, G1 = there_and_back_frames(n, back=False, stride=0.24)
    assert abs(C.project(np.linalg.inv(G1[5]), np.zeros((1, 2)))[0, 0]) > Ws
    one_way = align.Aligner(torch.nn.Sequential(PairsThenZeros(cuda(deltas1, torch.float32))), patch=P)
    t = one_way.sequence(cuda(frames1), ref=ref, links=[(3, 1), (5, 0)])
    weights = host(t["link_weight"]).tolist()
    print("a link between frames that share no pixel: scores %s, weights %s" % (host(t["link_score"]).tolist(), weights))
    assert weights == [[1.0, 0.0]] and host(t["link_score"])[0, 1] == -np.inf


def test_sequence_refuses_links_before_any_launch(monkeypatch):
    frames, deltas, _ = there_and_back_frames(6)
    bank = cuda(frames)
    aligner = align.Aligner(torch.nn.Sequential(PairsThenZeros(cuda(deltas, torch.float32))), patch=32)
    launches = []
    for name in ("align_prep_u8", "pano_chain", "pano_adjust", "align_prep_warp_u8"):
        fn = getattr(K, name)
        monkeypatch.setattr(K, name, lambda *a, _fn=fn, **k: launches.append(1) or _fn(*a, **k))
    p = poisoned_alloc.poison(monkeypatch, align)
    for kw in (dict(links=[(0, 0)]), dict(links=[(0, 6)]), dict(links=[(-1, 3)]), dict(links=[(1, 0)]), dict(links=[(0, 1)]), dict(links=[(3, 4)]), dict(links=[(5,)]),
               dict(links=3), dict(links=[(5, 0)], link_min_score=1.5), dict(links=[(5, 0)], link_min_score=float("nan")), dict(links=[(5, 0)], link_min_score=-1.01),
               dict(links=[(5, 0)], adjust_iters=-1), dict(links=[(5, 0)], adjust_grid=1), dict(links=[(5, 0)], adjust_grid=9), dict(links=[(5, 0)], adjust_grid=4.5)):
        with pytest.raises(ValueError):
            aligner.sequence(bank, ref=0, **kw)
    big = torch.zeros((65, 8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="64"):
        aligner.sequence(big, ref=0, links=[(64, 0)])
    assert not launches and len(p) == 0
