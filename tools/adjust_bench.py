"""Device time of the global adjustment (bihome_amd/align.py adjust_device; csrc/adjust.hip), B there-and-back sweeps of 48 x 64 frames.

    python tools/adjust_bench.py [--batch 8] [--iters 10] [--grid 4] [--rounds 7] [--reps 5] [--skip-model]

One JSON line per row and case (n = 16 with 4 links, n = 64 with 8 links):
    check    both results - bh_pano_adjust's and the torch formulation's - against align.adjust_host, before and after the timing, in this
             process; a formulation that does not agree gets its step-by-step trace printed
    adjust   bh_pano_adjust alone on resident buffers against the torch formulation of the same steps - the batched dense J, J^T W J,
             torch.linalg.cholesky_ex, torch.cholesky_solve, the accept rule by torch.where - measured in the same run; the ratio is
             printed only when both results agreed with the statement both times
    drift    the sweep's drift before and after: the last frame's and the mean corner distance to the truth, in the reference's pixels
    pairs    the pair call of the same sequences (Aligner on the B (n - 1) neighbouring pairs, zeng-bihome at random initialisation): what
             registering the sequence costs before the adjustment

The method is tools/datagen_bench.py's: the callables of a row alternate in this one process, `--rounds` rounds of `--reps` launches
behind `--warmup` launches each, every round between two device events; median and spread."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import align, configs, kernels as K  # noqa: E402
from bihome_amd.step import build_model  # noqa: E402
from align_bench import raw_call  # noqa: E402
from datagen_bench import device_rounds  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import align_adjust_cases as C  # noqa: E402  (the sweep and the corner measure are the tests')

SIZE = C.SIZE
AGREE_PX = 1e-3       # two results "agree" below this corner distance: accept decisions near convergence may differ, results may not


def out(case, **kw):
    print(json.dumps({"tool": "adjust_bench", "case": case, "device": torch.cuda.get_device_name(0), **kw}), flush=True)


def torch_adjust(G0, edges, Hl, ref, size, grid, iters):
    """`adjust_host`'s steps as batched torch operations on the device, weights all 1, every frame touched; nothing is read back.
    -> (G [B,n,3,3], accepted [B], trace: per step (info [B], take [B], cost of the trial [B]), device tensors)"""
    B, n = G0.shape[:2]
    dev, E, P, N = G0.device, len(edges), grid * grid, 8 * (n - 1)
    f64 = dict(dtype=torch.float64, device=dev)
    j, i = np.divmod(np.arange(P), grid)
    y = torch.tensor(np.stack([(i * (size[1] - 1)) / (grid - 1.0), (j * (size[0] - 1)) / (grid - 1.0), np.ones(P)], 1), **f64)          # [P,3]
    ia, ib = (torch.tensor(v, device=dev) for v in zip(*edges))
    slots = torch.eye(n, **f64)[:, [k for k in range(n) if k != ref]]                                                                  # [n,n-1]: frame -> its columns
    Sa, Sb = slots[ia], slots[ib]                                                                                                      # [E,n-1]
    zh = torch.einsum("beij,pj->bepi", Hl / Hl[..., 2:3, 2:3], y)
    z = torch.cat([zh[..., :2] / zh[..., 2:3], torch.ones_like(zh[..., 2:3])], -1)                                                     # [B,E,P,3]
    yb = y.expand(B, E, P, 3)
    W = align._inverse_device(G0)
    W = W / W[..., 2:3, 2:3]
    W = torch.where(torch.eye(n, **f64)[ref][None, :, None, None] > 0, torch.eye(3, **f64).expand(B, n, 3, 3), W)

    def terms(W):
        qa, qb = torch.einsum("beij,bepj->bepi", W[:, ia], z), torch.einsum("beij,bepj->bepi", W[:, ib], yb)
        ua, ub = qa[..., :2] / qa[..., 2:3], qb[..., :2] / qb[..., 2:3]
        ok = ((qa[..., 2] > 0) & (qb[..., 2] > 0)).reshape(B, -1).all(1)
        return ua - ub, (qa, ua), (qb, ub), ok

    def jac(pts, q, u):
        x, yy, iz = pts[..., 0] / q[..., 2], pts[..., 1] / q[..., 2], 1.0 / q[..., 2]
        J = torch.zeros((B, E, P, 2, 8), **f64)
        J[..., 0, 0], J[..., 0, 1], J[..., 0, 2], J[..., 0, 6], J[..., 0, 7] = x, yy, iz, -x * u[..., 0], -yy * u[..., 0]
        J[..., 1, 3], J[..., 1, 4], J[..., 1, 5], J[..., 1, 6], J[..., 1, 7] = x, yy, iz, -x * u[..., 1], -yy * u[..., 1]
        return J
    r, a, b, _ = terms(W)
    cost = (r * r).reshape(B, -1).sum(1)
    lam = torch.full((B,), 1e-3, **f64)
    accepted, trace = torch.zeros((B,), **f64), []
    for _ in range(iters):
        r, a, b, _ = terms(W)
        # (the frames' columns by one-hot products, not by indexed writes)
        full = torch.einsum("ek,bepij->bepikj", Sa, jac(z, *a)) - torch.einsum("ek,bepij->bepikj", Sb, jac(yb, *b))
        J = full.reshape(B, E * P * 2, N)
        A, g = J.transpose(1, 2) @ J, (J.transpose(1, 2) @ r.reshape(B, -1, 1))
        A = A + torch.diag_embed(lam[:, None] * A.diagonal(dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(A)
        d = torch.cholesky_solve(-g, L)[..., 0].reshape(B, n - 1, 8)
        d9 = torch.cat([d, torch.zeros((B, n - 1, 1), **f64)], 2)
        trial = W + torch.cat([d9[:, :ref], torch.zeros((B, 1, 9), **f64), d9[:, ref:]], 1).reshape(B, n, 3, 3)
        rt, _, _, ok = terms(trial)
        ct = (rt * rt).reshape(B, -1).sum(1)
        take = torch.isfinite(ct) & ok & (ct < cost) & (info == 0)
        W = torch.where(take[:, None, None, None], trial, W)
        cost = torch.where(take, ct, cost)
        lam = torch.where(take, (lam / 10).clamp(min=1e-12), (lam * 10).clamp(max=1e12))
        accepted = accepted + take
        trace.append((info, take, ct))
    G = align._inverse_device(W)
    return G / G[..., 2:3, 2:3], accepted, trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-model", action="store_true", help="kernel rows only")
    a = ap.parse_args()
    B = a.batch
    aligner = None if a.skip_model else align.Aligner(build_model(configs.get("zeng-bihome"), "cuda:0"))
    for n, links in ((16, 4), (64, 8)):
        shape = dict(batch=B, n=n, links=links, frame=list(SIZE), grid=a.grid, iters=a.iters, rounds=a.rounds, reps=a.reps)
        cases = [C.there_and_back(n, seed, links=links) for seed in range(B)]
        edges = cases[0][2]
        E = len(edges)
        G_true, G0h, Hlh = (np.stack([c[k] for c in cases]) for k in (0, 1, 3))
        G0, Hl = torch.from_numpy(G0h).cuda(), torch.from_numpy(Hlh).cuda()
        link = torch.tensor(edges, dtype=torch.int32).cuda()
        G, work = torch.empty_like(G0), torch.empty((B, 4), dtype=torch.float64, device="cuda")
        ws = torch.empty((K.pano_adjust_ws_doubles(n, E, B),), dtype=torch.float64, device="cuda")
        ours = raw_call("bh_pano_adjust", G0, link, Hl, None, B, n, E, 0, SIZE[0], SIZE[1], a.grid, a.iters, G, work, ws)
        want, want_work = align.adjust_host(G0h, edges, Hlh, None, 0, SIZE, a.grid, a.iters)

        def check(when):
            """Both results against the statement, in this process: a time is only worth printing for a result that is right."""
            ours()
            Gt, accepted, trace = torch_adjust(G0, edges, Hl, 0, SIZE, a.grid, a.iters)
            dk, dt = float(C.corner_distance(G.cpu().numpy(), want).max()), float(C.corner_distance(Gt.cpu().numpy(), want).max())
            row = dict(when=when, kernel_from_statement_px=dk, torch_from_statement_px=dt, kernel_agrees=dk <= AGREE_PX, torch_agrees=dt <= AGREE_PX,
                       accepted_steps=work[:, 2].cpu().tolist(), statement_accepted_steps=want_work[:, 2].tolist(), torch_accepted_steps=accepted.cpu().tolist())
            if not row["torch_agrees"]:                                        # what the formulation did, step by step
                row["torch_trace"] = [dict(info=i.cpu().tolist(), take=t.cpu().tolist(), trial_cost=c.cpu().tolist()) for i, t, c in trace]
            out("both results against adjust_host", **row, **shape)
            return row["kernel_agrees"], row["torch_agrees"]
        ok_before = check("before timing")
        r = device_rounds({"adjust": ours, "torch": lambda: torch_adjust(G0, edges, Hl, 0, SIZE, a.grid, a.iters)}, a.reps, a.rounds, a.warmup)
        ok_after = check("after timing")
        kernel_ok, torch_ok = ok_before[0] and ok_after[0], ok_before[1] and ok_after[1]
        out("bh_pano_adjust against the torch formulation", adjust=r["adjust"] if kernel_ok else None, torch_formulation=r["torch"],
            torch_result_verified=torch_ok, kernel_result_verified=kernel_ok,
            torch_over_adjust=round(r["torch"]["median_us"] / r["adjust"]["median_us"], 2) if kernel_ok and torch_ok else None,
            note=None if kernel_ok and torch_ok else "no ratio: a result did not agree with adjust_host to %g px in this process" % AGREE_PX,
            unknowns=8 * (n - 1), edges=E, **shape)
        Gd = G.cpu().numpy()
        before, after = C.corner_distance(G0h, G_true), C.corner_distance(Gd, G_true)
        out("there-and-back drift before and after", last_frame_px_before=[round(v, 3) for v in before[:, -1]], last_frame_px_after=[round(v, 3) for v in after[:, -1]],
            mean_px_before=[round(v, 3) for v in before.mean(1)], mean_px_after=[round(v, 3) for v in after.mean(1)],
            cost_before=[round(v, 4) for v in work[:, 0].cpu().tolist()], cost_after=[round(v, 4) for v in work[:, 1].cpu().tolist()], **shape)
        if aligner is not None:
            frames = torch.randint(0, 256, (B * n, SIZE[0], SIZE[1], 3), dtype=torch.uint8, device="cuda")
            idx = torch.arange(B * n, dtype=torch.int32, device="cuda").reshape(B, n)
            ia, ib = idx[:, 1:].reshape(-1).contiguous(), idx[:, :-1].reshape(-1).contiguous()
            rp = device_rounds({"pairs": lambda: aligner(frames, frames, idx_a=ia, idx_b=ib, warp=False), "adjust": ours}, 1, a.rounds, 1)
            out("the pair call of the same sequences", model="zeng-bihome", pairs=B * (n - 1), pair_call=rp["pairs"], adjust=rp["adjust"],
                adjust_share_of_pair_call=round(rp["adjust"]["median_us"] / rp["pairs"]["median_us"], 3), **dict(shape, reps=1))


if __name__ == "__main__":
    main()
