"""Time the occlusion-blob stage of the pair generator (bh_synth_blobs, csrc/blobs.hip; CollatorWithBlobs, transforms.py:746-799) at
B = 64, P = 128, C = 1, blobiness 0.2 (blur radius 64), porosity 0.1 - one JSON line per case:

    stage              synth_gpu.apply_blobs alone (K.synth_blobs and its two allocations) against the same stage written with torch operators on the
                       same GPU: the separable blur as two conv2d calls over a 'reflect'-padded plane (F.pad mode 'symmetric' does
                       not exist: the pad is a flip-and-concatenate), torch.special.erfc, amin / amax, torch.where.  The two alternate
                       round by round in this one process; the masks are compared.
    batch              GpuPairGenerator.next(64) of zeng-bihome-pds with and without blobs, alternating the same way.

    python tools/blob_bench.py

`--warmup` calls, then `--rounds` rounds of `--reps` calls per variant, each round between two device events with one synchronise at
its end; median, min and max over the rounds."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import configs, synth  # noqa: E402
from bihome_amd.synth_gpu import GpuPairGenerator, apply_blobs, batch_spec  # noqa: E402
from tools.datagen_bench import device_rounds  # noqa: E402


def torch_blobs(noise, other, p1, p2, sigma, porosity):
    """The stage with torch operators (float32 throughout, the blur on centred noise like the kernel's): (mask, composite)."""
    B, P, _ = noise.shape
    r = int(4.0 * sigma + 0.5)
    k = torch.arange(-r, r + 1, dtype=torch.float64, device=noise.device)
    w = torch.exp(-0.5 * (k / sigma) ** 2)
    w = (w / w.sum()).float()
    x = (noise - 0.5)[:, None]
    x = torch.cat([x[..., :r].flip(-1), x, x[..., P - r:].flip(-1)], -1)                 # scipy 'reflect': d c b a | a b c d | d c b a
    x = F.conv2d(x, w.view(1, 1, 1, -1))
    x = torch.cat([x[..., :r, :].flip(-2), x, x[..., P - r:, :].flip(-2)], -2)
    g = F.conv2d(x, w.view(1, 1, -1, 1))[:, 0]
    z = (g - g.mean((1, 2), keepdim=True)) / g.std((1, 2), unbiased=False, keepdim=True)
    u = 0.5 * torch.special.erfc(-z * 0.7071067811865476)
    lo, hi = u.amin((1, 2), keepdim=True), u.amax((1, 2), keepdim=True)
    mask = (u - lo) / (hi - lo) < porosity
    return mask, torch.where(mask[:, None], p1[other.long()], p2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    B, P, C, blobiness, porosity = args.batch, 128, 1, 0.2, 0.1
    sigma = synth.blob_sigma(P, blobiness)
    g = torch.Generator(device="cuda").manual_seed(0)
    noise = torch.rand((B, P, P), generator=g, device="cuda")
    r = torch.randint(0, B - 1, (B,), generator=g, device="cuda")
    other = (r + (r >= torch.arange(B, device="cuda"))).to(torch.int32)
    p1 = torch.randn((B, C, P, P), generator=g, device="cuda")
    p2 = torch.randn((B, C, P, P), generator=g, device="cuda")
    work = p2.clone()
    res = device_rounds({"hip": lambda: apply_blobs(noise, other, p1, work, sigma, porosity),
                         "torch": lambda: torch_blobs(noise, other, p1, p2, sigma, porosity)}, args.reps, args.rounds, args.warmup)
    work.copy_(p2)
    mask, _ = apply_blobs(noise, other, p1, work, sigma, porosity)
    tmask, tout = torch_blobs(noise, other, p1, p2, sigma, porosity)
    differ = int(((mask != 0) != tmask).sum().item())
    print(json.dumps({"tool": "blob_bench", "case": "stage", "batch": B, "patch": P, "channels": C, "blobiness": blobiness,
                      "porosity": porosity, "device": dev, "reps": args.reps, "rounds": args.rounds, "hip": res["hip"],
                      "torch": res["torch"], "torch_over_hip_median": round(res["torch"]["median_us"] / res["hip"]["median_us"], 2),
                      "mask_pixels_that_differ": differ, "mask_pixels": B * P * P, "blob_share": round(float(mask.mean().item()), 4)}),
          flush=True)
    spec = batch_spec(configs.get("zeng-bihome-pds"))
    plain = GpuPairGenerator(photometric_draws="device", **spec)
    occluded = GpuPairGenerator(photometric_draws="device", blob_porosity=porosity, blobiness=blobiness, **spec)
    res = device_rounds({"plain": lambda: plain.next(B), "blobs": lambda: occluded.next(B)}, args.reps, args.rounds, args.warmup)
    print(json.dumps({"tool": "blob_bench", "case": "batch", "config": "zeng-bihome-pds", "batch": B, "device": dev, "reps": args.reps,
                      "rounds": args.rounds, "next_without_blobs": res["plain"], "next_with_blobs": res["blobs"],
                      "blobs_minus_plain_median_us": round(res["blobs"]["median_us"] - res["plain"]["median_us"], 2)}), flush=True)


if __name__ == "__main__":
    main()
