"""Time bh_ransac_homography (kernels.ransac_homography) at the evaluation shape of zeng-orig: B = 64 fields of 128 x 128, K = 64 / 256 /
1024 minimal samples, 100 repetitions behind 10 warm-ups with device events around the whole call - next to (a) today's lattice fit
(NoOpHead._postprocess: bh_dlt_fwd on 512 points) and (b) a numpy float64 restatement of the same algorithm on the host for 8 samples,
the shape of upstream's per-sample host loop.  The `ransac+lm` leg is the same call followed by the Levenberg-Marquardt polish
(kernels.homography_refine_lm on the call's own mask and H: NoOpHead RANSAC_REFINE='lm'), on the same fields and with the same event
timing; `lm_polish_ms` is the difference of the two medians at each K.  Prints one JSON line.

    python tools/ransac_bench.py                  # all of it
    rocprofv3 --kernel-trace --stats -- python tools/ransac_bench.py --no-host --reps 20     # per-kernel times

The count kernel's pixel-hypothesis tests per second come from the K = 1024 minus K = 64 difference of the whole-call times (the
other four kernels do not depend on K beyond the 960 extra 8x8 solves per sample), or from the kernel trace directly."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import kernels as K, synth  # noqa: E402
from bihome_amd.heads import NoOpHead  # noqa: E402

THR = 10.0


def make_fields(B, seed=5):
    """Exact homography fields + 0.3 px noise, a 30 % block of wrong offsets and 5 % scattered outliers (the test inputs' recipe)."""
    clean = np.asarray(synth.make_pairs(B, seed=seed, target=True)["target"], np.float64)
    rng = np.random.default_rng(1)
    pf = clean + rng.normal(0.0, 0.3, clean.shape)
    pf[:, :, 32:96, 20:97] = pf[:, :, 64:65, 58:59] + 90.0
    idx = rng.integers(0, 128 * 128, (B, 819))
    for b in range(B):
        pf[b].reshape(2, -1)[:, idx[b]] = rng.uniform(-64, 64, (2, 819))
    return pf.astype(np.float32)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": t[len(t) // 2], "min_ms": t[0]}


def host_restatement(pf, choice):
    """The algorithm in numpy float64, one sample at a time (vectorised over hypotheses and pixels inside a sample)."""
    B, _, h, w = pf.shape
    x = np.tile(np.arange(w, dtype=np.float64), h)
    y = np.repeat(np.arange(h, dtype=np.float64), w)
    out = []
    for b in range(B):
        u, v = x + pf[b, 0].reshape(-1), y + pf[b, 1].reshape(-1)
        ids = choice[b]
        sx, sy, du, dv = x[ids], y[ids], u[ids], v[ids]                      # [K,4]
        zero, one = np.zeros_like(sx), np.ones_like(sx)
        A = np.concatenate([np.stack([sx, sy, one, zero, zero, zero, -sx * du, -sy * du], -1),
                            np.stack([zero, zero, zero, sx, sy, one, -sx * dv, -sy * dv], -1)], 1)      # [K,8,8]
        rhs = np.concatenate([du, dv], 1)
        ok = np.abs(np.linalg.det(A)) > 1e-9
        Hk = np.zeros((len(ids), 9))
        Hk[ok, :8] = np.linalg.solve(A[ok], rhs[ok][..., None])[..., 0]
        Hk[:, 8] = 1.0
        with np.errstate(all="ignore"):
            qz = Hk[:, 6, None] * x + Hk[:, 7, None] * y + 1.0
            e = ((Hk[:, 0, None] * x + Hk[:, 1, None] * y + Hk[:, 2, None]) / qz - u) ** 2 + \
                ((Hk[:, 3, None] * x + Hk[:, 4, None] * y + Hk[:, 5, None]) / qz - v) ** 2
        inl = (qz > 0) & (e <= THR * THR) & ok[:, None]
        m = inl[int(np.argmax(inl.sum(1)))]
        if m.sum() < 4:
            m = np.ones_like(m)
        src, dst = np.stack([x[m], y[m]], 1), np.stack([u[m], v[m]], 1)

        def norm(p):
            c = p.mean(0)
            s = np.sqrt(2.0) / (np.sqrt(((p - c) ** 2).sum(1)).mean() + 1e-8)
            return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
        T1, T2 = norm(src), norm(dst)
        a = np.concatenate([src, np.ones((len(src), 1))], 1) @ T1.T
        q = np.concatenate([dst, np.ones((len(dst), 1))], 1) @ T2.T
        z = np.zeros_like(a)
        M = np.concatenate([np.concatenate([a, z, -q[:, :1] * a], 1), np.concatenate([z, a, -q[:, 1:2] * a], 1)], 0)
        H = np.linalg.inv(T2) @ np.linalg.eigh(M.T @ M)[1][:, 0].reshape(3, 3) @ T1
        out.append(H / (H[2, 2] + 1e-8))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-samples", type=int, default=8)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--lm-iters", type=int, default=10)
    args = ap.parse_args()
    B = args.batch
    pf_np = make_fields(B)
    pf = torch.tensor(pf_np).cuda()
    res = {"tool": "ransac_bench", "batch": B, "field": [128, 128], "reps": args.reps, "device": torch.cuda.get_device_name(0), "ransac": {},
           "ransac+lm": {}, "lm_iters": args.lm_iters}

    def ransac_lm(choice):
        r = K.ransac_homography(pf, choice, THR, want_mask=True, check_range=False)
        return K.homography_refine_lm(pf, r[1], r[5], args.lm_iters)
    with torch.no_grad():
        res["lattice_dlt"] = timed(lambda: NoOpHead.Model._postprocess(pf), args.reps, args.warmup)
        for k in args.iters:
            choice = torch.randint(0, 128 * 128, (B, k, 4), generator=torch.Generator().manual_seed(7)).cuda()
            # (check_range=False: enqueue only, as with the head's own draws - no host sync inside the timing)
            r = timed(lambda: K.ransac_homography(pf, choice, THR, check_range=False), args.reps, args.warmup)
            r["pixel_hypothesis_tests"] = B * k * 128 * 128
            n_inl = K.ransac_homography(pf, choice, THR)[3]
            r["mean_inlier_share"] = float(n_inl.float().mean().item() / (128 * 128))
            res["ransac"][str(k)] = r
            p = timed(lambda: ransac_lm(choice), args.reps, args.warmup)
            p["lm_polish_ms"] = p["median_ms"] - r["median_ms"]
            info = ransac_lm(choice)[2]
            p["mean_accepted_steps"] = float(info[:, 2].mean().item())
            p["mean_relative_cost_gain"] = float(((info[:, 0] - info[:, 1]) / info[:, 0]).mean().item())
            res["ransac+lm"][str(k)] = p
        ks = sorted(args.iters)
        if len(ks) > 1:
            dt = (res["ransac"][str(ks[-1])]["median_ms"] - res["ransac"][str(ks[0])]["median_ms"]) * 1e-3
            res["count_tests_per_s_from_slope"] = B * (ks[-1] - ks[0]) * 128 * 128 / dt if dt > 0 else None
    if not args.no_host:
        n = min(args.host_samples, B)
        choice = torch.randint(0, 128 * 128, (n, 256, 4), generator=torch.Generator().manual_seed(7)).numpy()
        t0 = time.perf_counter()
        host_restatement(pf_np[:n].astype(np.float64), choice)
        res["host_numpy_f64"] = {"samples": n, "iters": 256, "ms": (time.perf_counter() - t0) * 1e3}
        res["host_numpy_f64"]["ms_per_sample"] = res["host_numpy_f64"]["ms"] / n
        res["host_numpy_f64"]["ms_scaled_to_batch"] = res["host_numpy_f64"]["ms_per_sample"] * B
    print(json.dumps(res))


if __name__ == "__main__":
    main()
