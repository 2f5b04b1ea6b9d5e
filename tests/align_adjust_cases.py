"""Shared by tests/test_align_adjust_cpu.py and tests/test_align_adjust_gpu.py: the inputs of the global adjustment's cases - the
there-and-back sweep, the consistent edges with a perturbed start, the batches the kernel is held to the statement on - the corner
measure, and the figure the device bound comes from (computed once)."""
import functools

import numpy as np

from bihome_amd import align, synth

SIZE = (48, 64)                  # (Hs, Ws) of every frame
STEP = 0.3                       # of the frame's width, per pair


def corners(size=SIZE):
    Hs, Ws = size
    return np.array([[0.0, 0.0], [Ws - 1.0, 0.0], [Ws - 1.0, Hs - 1.0], [0.0, Hs - 1.0]])


def project(M, pts):
    q = pts @ M[:2, :2].T + M[:2, 2]
    return q / (pts @ M[2, :2] + M[2, 2])[:, None]


def corner_distance(G, G_want, size=SIZE):
    """[..., n]: the largest distance, in the reference's pixels, between where G[k]^-1 and G_want[k]^-1 put frame k's four corners."""
    G, G_want = np.asarray(G, np.float64), np.asarray(G_want, np.float64)
    out = np.empty(G.shape[:-2])
    c = corners(size)
    for at in np.ndindex(*G.shape[:-2]):
        out[at] = np.linalg.norm(project(np.linalg.inv(G[at]), c) - project(np.linalg.inv(G_want[at]), c), axis=1).max()
    return out


def sweep_links(n, count):
    """The links (n - 1 - k, k), k = 0 .. count - 1, of a there-and-back sweep, without the chain's own middle pair."""
    return [(n - 1 - k, k) for k in range(count) if n - 1 - k - k > 1]


@functools.lru_cache(maxsize=None)
def there_and_back(n, seed, ref=0, jitter=0.5, noise=0.25, links=4, size=SIZE):
    """A sweep of n frames, `STEP` of the width to one side per pair for the first half and back for the second, so frame n - 1 - k
    overlaps frame k.  Pair j's TRUE homography moves the frame's corners by that shift plus up to `jitter` px each; the MEASURED pair
    adds up to `noise` px of corner noise to it; the links are exact.  -> (G_true [n,3,3], G0 [n,3,3] the chain of the measured pairs,
    edges [(a, b)] the pairs then the links, H_edges [E,3,3])"""
    rng = np.random.RandomState(1000 * n + seed)
    Hs, Ws = size
    c = corners(size)
    pairs = align.pairs_of(n, ref)
    true, meas = np.empty((n - 1, 3, 3)), np.empty((n - 1, 3, 3))
    for j, (a, b) in enumerate(pairs):
        side = 1.0 if j < (n - 1) / 2 else -1.0                               # frame j + 1 lies to the right of frame j, then to the left
        shift = np.array([(side if a > b else -side) * -STEP * Ws, 0.0])      # b's coordinates -> a's
        true[j] = synth.four_point_homography(c, c + shift + rng.uniform(-jitter, jitter, (4, 2)))
        meas[j] = synth.four_point_homography(c, project(true[j], c) + rng.uniform(-noise, noise, (4, 2)))
    G_true, G0 = align.chain_host(true[None], ref)[0], align.chain_host(meas[None], ref)[0]
    extra = sweep_links(n, links)
    H_links = [G_true[a] @ np.linalg.inv(G_true[b]) for a, b in extra]
    H_edges = np.stack(list(meas) + [h / h[2, 2] for h in H_links])
    for x in (G_true, G0, H_edges):
        x.setflags(write=False)
    return G_true, G0, pairs + extra, H_edges


@functools.lru_cache(maxsize=None)
def consistent(n, seed, ref=None, push=1.0, size=SIZE):
    """Edges that agree: every H_e = G*_a G*_b^-1 of a sweep's truth, pairs and links, and a start whose frames are pushed by up to `push`
    px at the corners.  -> (G_true [n,3,3], G0 [n,3,3], edges, H_edges [E,3,3])"""
    ref = n // 2 if ref is None else ref
    G_true, _, edges, _ = there_and_back(n, seed, ref=ref, links=2, size=size)
    rng = np.random.RandomState(77 * n + seed)
    c = corners(size)
    G0 = np.stack([G_true[k] if k == ref else synth.four_point_homography(c, c + rng.uniform(-push, push, (4, 2))) @ G_true[k] for k in range(n)])
    G0 = G0 / G0[:, 2:3, 2:3]
    H_edges = np.stack([G_true[a] @ np.linalg.inv(G_true[b]) for a, b in edges])
    H_edges = H_edges / H_edges[:, 2:3, 2:3]
    for x in (G0, H_edges):
        x.setflags(write=False)
    return G_true, G0, edges, H_edges


# the batches the kernel is held to the statement on: name -> (n, ref, links, grid, jitter, noise)
DEVICE_CASES = {
    "n2-ref0-grid2": (2, 0, 0, 2, 0.5, 0.25),
    "n2-ref1-grid4": (2, 1, 0, 4, 0.5, 0.25),
    "n3-ref1-grid8": (3, 1, 1, 8, 0.5, 0.25),
    "n16-ref0-grid4": (16, 0, 4, 4, 0.5, 0.25),
    "n64-ref0-grid4": (64, 0, 8, 4, 0.1, 0.05),
}
DEVICE_ITERS = 3


@functools.lru_cache(maxsize=None)
def device_case(name):
    """Three samples (seeds 0, 1, 2) of one edge list with weights that differ per sample: all 1; drawn from [0.5, 2]; drawn, and every
    third edge switched off (never the first, so that something counts).  -> (G0 [3,n,3,3], edges, H_edges [3,E,3,3], weight [3,E], ref, grid)"""
    n, ref, links, grid, jitter, noise = DEVICE_CASES[name]
    per = [there_and_back(n, seed, ref=ref, jitter=jitter, noise=noise, links=links) for seed in (0, 1, 2)]
    edges, H_edges = per[0][2], np.stack([p[3] for p in per])
    E = len(edges)
    rng = np.random.RandomState(5)
    weight = np.stack([np.ones(E), rng.uniform(0.5, 2.0, E), rng.uniform(0.5, 2.0, E) * (np.arange(E) % 3 != 2)])
    # every frame of the start is pushed by up to `jitter` px at its corners: a chain agrees with its own pairs exactly, and a start without
    # a residual would leave every accept decision to the rounding
    c = corners()
    G0 = np.stack([[p[1][k] if k == ref else synth.four_point_homography(c, c + rng.uniform(-jitter, jitter, (4, 2))) @ p[1][k] for k in range(n)] for p in per])
    G0 = G0 / G0[:, :, 2:3, 2:3]
    for x in (G0, H_edges, weight):
        x.setflags(write=False)
    return G0, edges, H_edges, weight, ref, grid


@functools.lru_cache(maxsize=None)
def device_reference(name, solver="cholesky", iters=DEVICE_ITERS):
    """adjust_host of the case -> (G, work)."""
    G0, edges, H_edges, weight, ref, grid = device_case(name)
    return align.adjust_host(G0, edges, H_edges, weight, ref, SIZE, grid, iters, solver=solver)


@functools.lru_cache(maxsize=None)
def d_cpu(name):
    """The largest corner distance between the statement with Cholesky and with np.linalg.solve after DEVICE_ITERS steps: what another
    order of the same arithmetic moves the result by on these inputs."""
    return float(corner_distance(device_reference(name)[0], device_reference(name, "solve")[0]).max())


def cap(name):
    """The device bound of the case: 100 d_cpu - the factor covers the other summation order of J^T J and the blocked factorisation - and
    at least 1e-9 px."""
    return max(100.0 * d_cpu(name), 1e-9)


# ------------------------------------------------------------------------------------------------
# the cost at the result, where it is a figure and where it is the rounding of its own evaluation
# ------------------------------------------------------------------------------------------------
def counting_edges_form_a_forest(edges, weight, n):
    """No cycle among the counting edges (a != b, both frames of the sequence, a weight that is finite and > 0): then every residual can be
    driven to zero - each frame hangs on one edge - and the cost at the result tends to the rounding of its own evaluation.  Decided from
    the edge list and the weights alone (union-find), never from a computed number."""
    root = list(range(n))

    def find(k):
        while root[k] != k:
            root[k] = root[root[k]]
            k = root[k]
        return k
    for (a, b), w in zip(edges, weight):
        if a == b or not (0 <= a < n and 0 <= b < n) or not (np.isfinite(w) and w > 0):
            continue
        ra, rb = find(a), find(b)
        if ra == rb:
            return False
        root[ra] = rb
    return True


# per case, which of the three samples have counting edges without a cycle: n = 2 has one edge; the third sample switches every third edge
# off, which cuts the chain into pieces of three frames that the remaining links join without closing a loop
FOREST_SAMPLES = {"n2-ref0-grid2": [True, True, True], "n2-ref1-grid4": [True, True, True], "n3-ref1-grid8": [False, False, True],
                  "n16-ref0-grid4": [False, False, True], "n64-ref0-grid4": [False, False, True]}


def forest_samples(name):
    G0, edges, _, weight, _, _ = device_case(name)
    return [counting_edges_form_a_forest(edges, w, G0.shape[1]) for w in weight]


def forest_cost_slack(name, sample, cost_a, cost_b):
    """What two evaluations of the cost at the result may differ by, ABSOLUTELY (px^2), on a sample whose counting edges form a forest.
    With r and r' the residual components of the two, |sum w (r^2 - r'^2)| <= max |r - r'| sum w (|r| + |r'|) <= e (sqrt(S a) + sqrt(S b))
    by Cauchy-Schwarz, S the sum of the weights over all components (2 g g per counting edge), a and b the two costs.  A component is a
    difference of two projected points, and the two evaluations differ in it by what their iterates differ by - at most the corner cap
    of the case for each point, twice that as a control point of the other frame may lie outside this frame's corners - plus the rounding
    of the projection itself, 16 ulp of the largest coordinate X for each point: e = 2 (2 cap + 16 * 2^-53 X)."""
    G0, edges, H_edges, weight, ref, grid = device_case(name)
    n = G0.shape[1]
    counts = [(a, b, w) for (a, b), w in zip(edges, weight[sample]) if a != b and 0 <= a < n and 0 <= b < n and np.isfinite(w) and w > 0]
    S = 2.0 * grid * grid * sum(w for _, _, w in counts)
    X = max(np.abs(project(np.linalg.inv(G0[sample, k]), corners())).max() for k in range(n)) + max(SIZE)
    e = 2.0 * (2.0 * cap(name) + 16.0 * 2.0 ** -53 * X)
    return e * (np.sqrt(S * cost_a) + np.sqrt(S * cost_b))


# what the statement reaches on consistent edges after 10 steps, the largest corner distance to the truth over seeds 0..2 (px): recorded
# from test_align_adjust_cpu.py's own print; the assertions are one order of magnitude above it
REACHED = {6: 3.6e-14, 9: 7.3e-14}
