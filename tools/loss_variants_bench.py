"""Time the cosine one-line loss pair (bh_oneline_cos_loss_fwd / _bwd) and the channel-aware margin pair (bh_triplet_hinge_fwd / _bwd)
on one GPU, next to their L1 siblings and the torch formulation, and the training step of the configs that use them.

    python tools/loss_variants_bench.py [--reps 50] [--steps 30] [--no-steps]

Kernels: B = 64 samples of 32 x 32 x 64 features (the shipped configs' extractor output), rep in {1, 4} hypotheses for the one-line pair.
Medians over --reps timed calls with HIP events after 5 warm-up calls.  `*_gbs` = the bytes the pass has to move (feature maps read +
gradients written, from the shapes; the per-pixel maps are < 2 %) over the median time; `*_hbm_share` = that rate over the 8.0 TB/s HBM3E
peak.  At these sizes (50 - 200 MB per pass) the operands of a repeated call partly stay in the 256 MiB last-level cache, so the rate is an
upper estimate of what the pass sees inside a training step.
Steps: zeng-ihome-cos / detone-bihome-aware next to zeng-ihome / detone-bihome, B = 64 synthetic pairs, median wall time per step over
--steps steps (host clock around a device synchronise) after 5 warm-up steps.  One JSON line per measurement group.
Reported, not asserted: each pass against its L1 sibling (expected within a small factor, in proportion to the bytes it moves)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bihome_amd import configs, kernels as K, synth  # noqa: E402

HBM_PEAK = 8.0e12
EPS = 1e-8


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


def rates(r, tag, nbytes):
    r[tag + "_gbs"] = round(nbytes / (r[tag + "_ms"] * 1e-3) / 1e9, 1)
    r[tag + "_hbm_share"] = round(nbytes / (r[tag + "_ms"] * 1e-3) / HBM_PEAK, 3)


def torch_cosine(f1, f2, f1w, m1w, margin, rep, s):
    """PerceptualHead.py:498-511,523-538 on NHWC tensors (fp32 eager ops)."""
    rp = (lambda x: x.repeat_interleave(rep, 0)) if rep > 1 else (lambda x: x)
    l1 = 1 - torch.cosine_similarity(f1w, rp(f2), dim=-1, eps=EPS)
    l3 = rp(1 - torch.cosine_similarity(f1, f2, dim=-1, eps=EPS))
    mat = torch.clamp(l1 - l3 + margin, min=0)
    if s is not None:
        mat = mat * s.view(-1, 1, 1)
    den = m1w.sum((-1, -2))
    return ((m1w * mat).sum((-1, -2)) / torch.clamp(den, min=1.0)).sum()


def torch_aware(f1, f2, f1w, f2w, m1w, m2w, margin):
    """PerceptualHead.py:559-561,615,624-625,631-635,644-645,652-657 (without the mu term)."""
    l3 = (f1 - f2).abs()
    M1 = torch.clamp((f1w - f2).abs() - l3 + margin, min=0).sum(-1)
    M2 = torch.clamp((f2w - f1).abs() - l3 + margin, min=0).sum(-1)
    d1, d2 = m1w.sum((-1, -2)), m2w.sum((-1, -2))
    return ((m1w * M1).sum((-1, -2)) / torch.clamp(d1, min=1.0)).sum() + ((m2w * M2).sum((-1, -2)) / torch.clamp(d2, min=1.0)).sum()


def torch_pair(r, loss_fn, leaves, reps):
    with torch.no_grad():
        r["torch_fwd_ms"] = timed(loss_fn, reps)
    out = [None]

    def fwd():
        out[0] = loss_fn()

    def fwd_bwd():
        fwd()
        torch.autograd.grad(out[0], leaves)
    t_f, t_fb = timed(fwd, reps), timed(fwd_bwd, reps)
    r["torch_bwd_ms"] = t_fb - t_f                           # (autograd needs its own forward: the difference of two medians)


def bench_oneline(B, hf, C, rep, reps):
    g = torch.Generator().manual_seed(rep)
    f1, f2 = (torch.randn(B, hf, hf, C, generator=g).cuda() for _ in range(2))
    f1w = (f2.repeat_interleave(rep, 0) + 0.7 * torch.randn(B * rep, hf, hf, C, generator=g).cuda()).contiguous()
    m1w = torch.rand(B * rep, hf, hf, generator=g).cuda()
    s = torch.softmax(torch.randn(B, rep, generator=g), -1).reshape(-1).cuda() if rep > 1 else None
    gl = torch.ones(1, device="cuda")
    fmap = 4.0 * f1w.numel()
    r = {"pair": "oneline", "B": B, "hf": hf, "C": C, "rep": rep, "reps": reps}
    for tag, fwd, bwd, margin in (("cos", K.oneline_cos_loss_fwd, K.oneline_cos_loss_bwd, 0.8), ("l1", K.oneline_loss_fwd, K.oneline_loss_bwd, 1.0)):
        loss, T, nd, per = fwd(f1, f2, f1w, m1w, margin, rep=rep, sample_w=s)
        r[tag + "_fwd_ms"] = timed(lambda: fwd(f1, f2, f1w, m1w, margin, rep=rep, sample_w=s), reps)
        r[tag + "_bwd_ms"] = timed(lambda: bwd(gl, f2, f1w, m1w, T, nd, rep=rep, sample_w=s), reps)
        rates(r, tag + "_fwd", fmap + 2 * fmap / rep)         # f1w once per hypothesis; f1, f2 once per sample (re-reads hit the cache)
        rates(r, tag + "_bwd", 2 * fmap + fmap / rep)         # f1w in, g_f1w out, f2 once per sample
    a = f1w.clone().requires_grad_(True)
    torch_pair(r, lambda: torch_cosine(f1, f2, a, m1w, 0.8, rep, s), (a,), reps)
    for p in ("fwd", "bwd"):
        r["cos_over_l1_" + p] = round(r["cos_%s_ms" % p] / r["l1_%s_ms" % p], 2)
        r["torch_over_cos_" + p] = round(r["torch_%s_ms" % p] / r["cos_%s_ms" % p], 1)
    return r


def bench_double(B, hf, C, reps):
    g = torch.Generator().manual_seed(7)
    f1, f2 = (torch.randn(B, hf, hf, C, generator=g).cuda() for _ in range(2))
    f1w, f2w = f2 + 0.7 * torch.randn(B, hf, hf, C, generator=g).cuda(), f1 + 0.7 * torch.randn(B, hf, hf, C, generator=g).cuda()
    m1w, m2w = (torch.rand(B, hf, hf, generator=g).cuda() for _ in range(2))
    H, _ = K.h4pt_fwd(torch.zeros(B, 4, 2, device="cuda"), 128)
    gl = torch.ones(1, device="cuda")
    fmap = 4.0 * f1.numel()
    r = {"pair": "double-line", "B": B, "hf": hf, "C": C, "reps": reps}
    M1, M2, nd = K.triplet_hinge_fwd(f1, f2, f1w, f2w, m1w, m2w, 0.5)
    r["aware_fwd_ms"] = timed(lambda: K.triplet_hinge_fwd(f1, f2, f1w, f2w, m1w, m2w, 0.5), reps)
    r["aware_bwd_ms"] = timed(lambda: K.triplet_hinge_bwd(gl, f1, f2, f1w, f2w, m1w, m2w, None, None, M1, M2, nd, H, H, 0.5, 0.01), reps)
    L1, L2, nl = K.triplet_l1_fwd(f1, f2, f1w, f2w, m1w, m2w)
    r["l1_fwd_ms"] = timed(lambda: K.triplet_l1_fwd(f1, f2, f1w, f2w, m1w, m2w), reps)
    r["l1_bwd_ms"] = timed(lambda: K.bihome_loss_bwd(gl, f1, f2, f1w, f2w, m1w, m2w, None, None, L1, L2, nl, H, H, 0.01), reps)
    rates(r, "aware_fwd", 4 * fmap)
    rates(r, "l1_fwd", 4 * fmap)
    rates(r, "aware_bwd", 6 * fmap)                           # 4 maps read (each direction: three, two of them shared), 2 gradients written
    rates(r, "l1_bwd", 6 * fmap)
    a, b = f1w.clone().requires_grad_(True), f2w.clone().requires_grad_(True)
    torch_pair(r, lambda: torch_aware(f1, f2, a, b, m1w, m2w, 0.5), (a, b), reps)
    for p in ("fwd", "bwd"):
        r["aware_over_l1_" + p] = round(r["aware_%s_ms" % p] / r["l1_%s_ms" % p], 2)
        r["torch_over_aware_" + p] = round(r["torch_%s_ms" % p] / r["aware_%s_ms" % p], 1)
    return r


def bench_step(name, steps):
    from bihome_amd.step import build_model, build_optimizer, train_step
    from bihome_amd.weights import load_synthetic
    cfg = configs.get(name)
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    B = cfg["DATA"]["BATCH_SIZE"]
    d = synth.make_pairs(B, seed=1)
    data = {k: torch.tensor(d[k]).cuda() for k in ("patch_1", "patch_2", "delta")}
    for _ in range(5):
        train_step(model, dict(data), opt, sched)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        train_step(model, dict(data), opt, sched)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-steps", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is a CPU measurement"
    B, hf, C = 64, 32, 64
    for rep in (1, 4):
        print(json.dumps(bench_oneline(B, hf, C, rep, a.reps)), flush=True)
    print(json.dumps(bench_double(B, hf, C, a.reps)), flush=True)
    if not a.no_steps:
        r = {"steps": a.steps, "B": 64}
        for name in ("zeng-ihome", "zeng-ihome-cos", "detone-bihome", "detone-bihome-aware"):
            r[name + "_step_ms"] = round(bench_step(name, a.steps), 3)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
