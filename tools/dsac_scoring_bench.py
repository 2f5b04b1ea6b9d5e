"""Time the DSAC soft inlier-count score and its adjoint (bh_dsac_score / bh_dsac_scores_bwd, 'soft_inliers_ratio') on one GPU.

    python tools/dsac_scoring_bench.py [--reps 50]

B = 64 fields of 128 x 128, n in {4, 64} hypotheses.  Two baselines on the same device and shapes: the torch formulation of
ransac_utils.py:76-128 (fp32 eager ops + autograd), and the unchanged 'repr_error' kernels (method 0 of the same two calls: one
workgroup per hypothesis, the field re-read n times).  Forward = raw scores + softmax; backward = the adjoint given the weights' gradient.
Medians over --reps timed calls with HIP events after 5 warm-up calls; one JSON line per n.  The only pass / fail: the kernels beat torch."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bihome_amd import kernels as K  # noqa: E402

THR, BETA = 2.0, 1.5


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def torch_weights(pf, Hd, coord):
    B, n = Hd.shape[:2]
    mapf = coord[None] + pf.reshape(B, 2, -1).permute(0, 2, 1)
    ph = torch.cat([coord, torch.ones_like(coord[:, :1])], -1)
    q = torch.einsum("bnij,pj->bnpi", Hd, ph)
    z = q[..., 2:]
    big = z.abs() > 1e-8
    scale = torch.where(big, 1.0 / torch.where(big, z, torch.ones_like(z)), torch.ones_like(z))
    e = torch.norm(q[..., :2] * scale - mapf[:, None], dim=-1)
    return torch.softmax(-torch.sigmoid(BETA * (e - THR)).sum(-1), -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    B, h, w = 64, 128, 128
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    coord = torch.stack([xs.reshape(-1), ys.reshape(-1)], -1).cuda()
    ok = True
    for n in (4, 64):
        g = torch.Generator().manual_seed(n)
        pf = (torch.randn(B, 2, h, w, generator=g) * 2.0).cuda()
        Hd = torch.eye(3).repeat(B, n, 1, 1) + 0.001 * torch.randn(B, n, 3, 3, generator=g)
        Hd[:, :, 2, :2] *= 0.01
        Hd = Hd.cuda()
        Hf = Hd.reshape(-1, 9).contiguous()
        gs = torch.randn(B, n, generator=g).cuda()
        r = {"B": B, "h": h, "w": w, "n": n, "reps": a.reps}
        for tag, method in (("soft", "soft_inliers_ratio"), ("repr_error", "repr_error")):
            s, _ = K.dsac_scores_fwd(pf, Hf, n, method, THR, BETA)
            r[tag + "_fwd_ms"] = timed(lambda: K.dsac_scores_fwd(pf, Hf, n, method, THR, BETA), a.reps)
            r[tag + "_bwd_ms"] = timed(lambda: K.dsac_scores_bwd(pf, Hf, s, gs, n, method, THR, BETA), a.reps)
        with K.det_scope(True):
            r["soft_bwd_det_ms"] = timed(lambda: K.dsac_scores_bwd(pf, Hf, s, gs, n, "soft_inliers_ratio", THR, BETA), a.reps)
        pfr, Hr = pf.clone().requires_grad_(True), Hd.clone().requires_grad_(True)
        with torch.no_grad():
            r["torch_fwd_ms"] = timed(lambda: torch_weights(pf, Hd, coord), a.reps)
        wts = [None]

        def fwd():
            wts[0] = torch_weights(pfr, Hr, coord)

        def fwd_bwd():
            fwd()
            torch.autograd.grad(wts[0], (pfr, Hr), gs)
        t_f, t_fb = timed(fwd, a.reps), timed(fwd_bwd, a.reps)
        r["torch_bwd_ms"] = t_fb - t_f                       # (autograd needs its own forward: the difference of two medians)
        r["beats_torch"] = bool(r["soft_fwd_ms"] < r["torch_fwd_ms"] and r["soft_bwd_ms"] < r["torch_bwd_ms"])
        ok = ok and r["beats_torch"]
        print(json.dumps(r))
    if not ok:
        sys.exit("the soft-score kernels do not beat the torch formulation")


if __name__ == "__main__":
    main()
