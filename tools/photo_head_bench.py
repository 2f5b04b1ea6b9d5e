"""Timing of the photometric head (nguyen-orig, config/s-coco/nguyen-orig-lr-5e-3.yaml) on one GPU; prints one JSON line.

  head_fwd_bwd_us       the HIP head at B = 64: PhotometricHead's autograd Function (h4pt solve + warp-and-crop gather) forward, L1
                        against patch_2, backward (warp adjoint + h4pt adjoint) - device events over 100 repetitions after warm-up
  torch_reference_us    the reference's formulation of the same on the same GPU (PhotometricHead.py:26-42 as kornia runs it):
                        4-point solve, inverse, full-image grid_sample warp of image_1, per-sample crop, L1, autograd backward
  step_ms               one full nguyen-orig train_step at B = 64 (mean over the timed steps; PRECISION 'f32' as bench.py runs)
  detone_orig_step_ms   the same for detone-orig (the same ResNet-34 regressor under NoOpHead + MSELoss)

    python tools/photo_head_bench.py [--batch 64] [--reps 100] [--steps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps          # ms


def torch_reference(image, corners, delta_hat, patch_2):
    """PhotometricHead.py:26-42 in plain torch: kornia.get_perspective_transform (8x8 solve), warp_image = warp_perspective(image,
    inverse(H)) over the whole image (normalise, inverse, grid, grid_sample bilinear / zeros / align_corners), crop, L1Loss."""
    B, _, h, w = image.shape
    dst = corners + delta_hat
    x, y, u, v = corners[..., 0], corners[..., 1], dst[..., 0], dst[..., 1]
    o, z = torch.ones_like(x), torch.zeros_like(x)
    A = torch.stack([torch.stack([x, y, o, z, z, z, -x * u, -y * u], -1), torch.stack([z, z, z, x, y, o, -x * v, -y * v], -1)], 2).reshape(B, 8, 8)
    hv = torch.linalg.solve(A, torch.stack([u, v], 2).reshape(B, 8, 1)).squeeze(-1)
    H = torch.cat([hv, torch.ones_like(hv[:, :1])], 1).reshape(B, 3, 3)
    M = torch.inverse(H)
    N = torch.tensor([[2.0 / (w - 1), 0, -1], [0, 2.0 / (h - 1), -1], [0, 0, 1]], device=image.device)
    G = torch.inverse(N @ (M @ torch.inverse(N)))
    ys, xs = torch.linspace(-1, 1, h, device=image.device), torch.linspace(-1, 1, w, device=image.device)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    base = torch.stack([gx, gy, torch.ones_like(gx)], -1).reshape(1, h * w, 3)
    q = torch.einsum("bij,bnj->bni", G, base.expand(B, -1, -1))
    zq = q[..., 2:3]
    grid = (q[..., :2] / torch.where(zq.abs() > 1e-8, zq, torch.ones_like(zq))).reshape(B, h, w, 2)
    warped = F.grid_sample(image, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    c = corners.int().cpu()
    patch_hat = torch.stack([warped[i, :, c[i, 0, 1]:c[i, 3, 1], c[i, 0, 0]:c[i, 1, 0]] for i in range(B)])
    return F.l1_loss(patch_2, patch_hat)


def step_ms(name, d, steps):
    from bihome_amd import configs
    from bihome_amd.step import build_loss, build_model, build_optimizer, train_step
    from bihome_amd.weights import load_synthetic
    cfg = configs.get(name)
    cfg["MODEL"]["BACKBONE"]["PRECISION"] = "f32"          # bench.py's headline arithmetic (its --precision default)
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    loss_fn = build_loss(cfg["SOLVER"])
    keys = ("patch_1", "patch_2", "delta", "corners") + (("image_1",) if cfg["MODEL"]["HEAD"]["NAME"] == "PhotometricHead" else ("target",))
    data = {k: torch.tensor(d[k]).cuda() for k in keys}
    return timed(lambda: train_step(model, dict(data), opt, sched, loss_fn=loss_fn), steps, warmup=5)      # (a fresh dict per step, as bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from bihome_amd import synth
    from bihome_amd.heads.PhotometricHead import _PatchHat
    B = a.batch
    d = synth.make_pairs(B, seed=5, image=True, target=True)
    image, patch_2 = torch.tensor(d["image_1"]).cuda(), torch.tensor(d["patch_2"]).cuda()
    corners = torch.tensor(d["corners"]).cuda()
    origin = corners[:, 0].contiguous()
    rng = np.random.Generator(np.random.PCG64(1))
    delta_hat = torch.tensor(d["delta"] + rng.uniform(-4, 4, d["delta"].shape).astype(np.float32)).cuda().requires_grad_(True)

    def hip():
        F.l1_loss(patch_2, _PatchHat.apply(delta_hat, image, origin, 128)).backward()

    def ref():
        torch_reference(image, corners, delta_hat, patch_2).backward()
    from bihome_amd._lib import BihomeLibError
    res = {"batch": B}
    for key, name in (("detone_orig_step_ms", "detone-orig"), ("step_ms", "nguyen-orig")):
        try:
            res[key] = round(step_ms(name, d, a.steps), 3)
        except BihomeLibError as e:                       # (reported, not fatal: the head legs below are independent of it)
            res[key], res[key + "_error"] = None, str(e)
    res["head_fwd_bwd_us"] = round(1e3 * timed(hip, a.reps), 1)
    res["torch_reference_us"] = round(1e3 * timed(ref, a.reps), 1)
    if res["step_ms"] and res["detone_orig_step_ms"]:
        res["head_share_of_step"] = round(res["head_fwd_bwd_us"] / (1e3 * res["step_ms"]), 4)
        res["step_vs_detone"] = round(res["step_ms"] / res["detone_orig_step_ms"], 4)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
