"""Device time of the mosaic (bihome_amd/align.py mosaic / Aligner(mosaic=); csrc/blend.hip, the pair walk), B pairs of 480 x 640 uint8 images on a
fitted 640 x 960 canvas.

    python tools/mosaic_bench.py [--batch 64] [--height 480] [--width 640] [--canvas-height 640] [--canvas-width 960] [--rounds 21] [--reps 10]
                                 [--warmup 5] [--other-lib LABEL=PATH ...] [--skip-model]

One JSON line per row:
    mosaic    bh_mosaic_u8 (one launch: eight taps, weights, blend, rounding, cover) against the two-call route - bh_warp_u8 of A and of B
              onto the canvas with their validity masks, then the weights (from the projected coordinates), products, sum, division and
              rounding as torch tensor operations - and against a Tensor.copy_ of the same bytes (A + B read, the canvas written);
              `fused_not_above_two_call` is the condition the fused kernel is kept on (its median over the rounds is not above the
              two-call route's in this run); the share of pixels on which the two results differ and the largest difference are reported
              next to it (the two-call route rounds both warped images to uint8 before it blends them).  --other-lib LABEL=PATH times
              the same entry point of another build of the library in the same rounds (tools/pano_bench.py's other_call) and reports
              whether its output is the same bits
    exposure  the gain / bias measurement alone: two one-level gray pyramids, bh_ecc_sums, exposure_device
    aligner   Aligner end to end without and with mosaic=(Hc, Wc), zeng-bihome at random initialisation: the cost of the stage

The method is tools/align_cascade_bench.py's: the callables of a row alternate in this one process, `--rounds` rounds (at least 20) of
`--reps` launches behind `--warmup` launches each, every round between two device events; median and spread over the rounds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import align, configs, synth  # noqa: E402
from bihome_amd.step import build_model  # noqa: E402
from align_bench import copy_pair, raw_call  # noqa: E402
from datagen_bench import device_rounds  # noqa: E402


def out(case, **kw):
    print(json.dumps({"tool": "mosaic_bench", "case": case, "device": torch.cuda.get_device_name(0), **kw}), flush=True)


def border_weight(M, xs, ys, w, h, feather):
    """min(distance of M (x, y, 1) to the border of a w x h image + 1, feather) as float32 tensor operations: [B,Hc,Wc]."""
    m = M.to(torch.float32).reshape(-1, 9, 1, 1)
    qz = m[:, 6] * xs + m[:, 7] * ys + m[:, 8]
    u, v = (m[:, 0] * xs + m[:, 1] * ys + m[:, 2]) / qz, (m[:, 3] * xs + m[:, 4] * ys + m[:, 5]) / qz
    return torch.clamp(torch.minimum(torch.minimum(u, (w - 1) - u), torch.minimum(v, (h - 1) - v)) + 1.0, max=feather)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--canvas-height", type=int, default=640)
    ap.add_argument("--canvas-width", type=int, default=960)
    ap.add_argument("--feather", type=float, default=32.0)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--other-lib", action="append", default=[], metavar="LABEL=PATH", help="another build of libbihome_hip.so whose bh_mosaic_u8 is timed too")
    ap.add_argument("--skip-model", action="store_true", help="kernel rows only")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds is at least 20: the medians compared come from that many alternating repetitions")
    B, h, w, Hc, Wc, feather = a.batch, a.height, a.width, a.canvas_height, a.canvas_width, a.feather
    shape = dict(batch=B, height=h, width=w, canvas_height=Hc, canvas_width=Wc, feather=feather, rounds=a.rounds, reps=a.reps)
    rng = np.random.default_rng(0)
    few = np.stack([np.floor(np.clip(synth.texture_image(rng, h, w), 0, 255) + 0.5).astype(np.uint8) for _ in range(4)])
    images_a = torch.from_numpy(few).cuda().repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    images_b = images_a.flip(0).contiguous()
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    H_host = np.stack([synth.four_point_homography(c, c + rng.uniform(-0.2, 0.2, (4, 2)) * np.array([w, h])) for _ in range(B)])
    H = torch.from_numpy(H_host).cuda()
    T, _, fitted = align.mosaic_frame_device(H, (h, w), (h, w), (Hc, Wc))
    Ma, Mb = (H @ T).contiguous(), T.contiguous()

    # the mosaic: one launch against two warps and the torch formulation of the blend
    res = torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device="cuda")
    cover = torch.empty((B, Hc, Wc), dtype=torch.uint8, device="cuda")
    args = (images_a, None, B, h, w, images_b, None, B, h, w, Ma, Mb, None, B, Hc, Wc, feather, 0)
    fused = raw_call("bh_mosaic_u8", *args, res, cover)
    other_out, others = {}, {}
    if a.other_lib:
        from pano_bench import other_call                                 # (not at the top: pano_bench imports this module's border_weight)
    for spec in a.other_lib:
        label, path = spec.split("=", 1)
        other_out[label] = (torch.empty_like(res), torch.empty_like(cover))
        others[label] = other_call(path, "bh_mosaic_u8", *args, *other_out[label])
    wa_img, wb_img = torch.empty_like(res), torch.empty_like(res)
    va, vb = torch.empty_like(cover), torch.empty_like(cover)
    warp_a = raw_call("bh_warp_u8", images_a, None, B, h, w, Ma, B, Hc, Wc, wa_img, va)
    warp_b = raw_call("bh_warp_u8", images_b, None, B, h, w, Mb, B, Hc, Wc, wb_img, vb)
    ys, xs = torch.meshgrid(torch.arange(Hc, dtype=torch.float32, device="cuda"), torch.arange(Wc, dtype=torch.float32, device="cuda"), indexing="ij")
    two = {}

    def two_call():
        warp_a()
        warp_b()
        wa = border_weight(Ma, xs, ys, w, h, feather) * va
        wb = border_weight(Mb, xs, ys, w, h, feather) * vb
        den = wa + wb
        num = wa_img * wa[..., None] + wb_img * wb[..., None]
        two["out"] = torch.floor(num / den.clamp(min=1.0)[..., None] + 0.5).to(torch.uint8)
        two["cover"] = va | (vb << 1)
    moved = 2 * B * h * w * 3 + B * Hc * Wc * 4
    src, dst = copy_pair(moved)
    r = device_rounds({"fused": fused, **others, "two_call": two_call, "copy": lambda: dst.copy_(src)}, a.reps, a.rounds, a.warmup)
    for fn in (fused, two_call, *others.values()):
        fn()
    differ = float((res != two["out"]).any(-1).float().mean().item())
    largest = int((res.to(torch.int16) - two["out"].to(torch.int16)).abs().max().item())
    out("bh_mosaic_u8 against two bh_warp_u8 + the torch formulation of weights and blend", fused=r["fused"], two_call=r["two_call"],
        device_copy_same_bytes=r["copy"], bytes_moved=moved, **{k: r[k] for k in others},
        fused_over_other={k: round(r["fused"]["median_us"] / r[k]["median_us"], 3) for k in others},
        other_same_bits={k: bool(torch.equal(o, res) and torch.equal(c, cover)) for k, (o, c) in other_out.items()},
        fused_GBps=round(moved / (r["fused"]["median_us"] * 1e-6) / 1e9, 1), copy_GBps=round(moved / (r["copy"]["median_us"] * 1e-6) / 1e9, 1),
        share_of_copy_rate=round(r["copy"]["median_us"] / r["fused"]["median_us"], 3),
        fused_over_two_call=round(r["fused"]["median_us"] / r["two_call"]["median_us"], 3),
        fused_not_above_two_call=bool(r["fused"]["median_us"] <= r["two_call"]["median_us"]),
        share_of_pixels_that_differ=differ, largest_difference_grey_levels=largest, cover_differs=float((cover != two["cover"]).float().mean().item()),
        fitted=int(fitted.sum().item()), cover_shares=[round(float((cover == k).float().mean().item()), 3) for k in range(4)], **shape)
    two.clear()
    del wa_img, wb_img, va, vb, src, dst, other_out, others

    # the exposure measurement alone
    r = device_rounds({"exposure": lambda: align.measure_exposure(images_a, images_b, H)}, a.reps, a.rounds, a.warmup)
    out("exposure: two gray pyramids of one level, bh_ecc_sums, exposure_device", exposure=r["exposure"], **shape)

    if a.skip_model:
        return
    model = build_model(configs.get("zeng-bihome"), "cuda:0")
    aligner = align.Aligner(model)
    reps = max(1, a.reps // 4)
    fns = {"plain": lambda: aligner(images_a, images_b), "mosaic": lambda: aligner(images_a, images_b, mosaic=(Hc, Wc), mosaic_feather=feather),
           "mosaic_gain": lambda: aligner(images_a, images_b, mosaic=(Hc, Wc), mosaic_feather=feather, mosaic_exposure="gain")}
    r = device_rounds(fns, reps, a.rounds, a.warmup)
    out("Aligner end to end without and with mosaic=(Hc, Wc)", model="zeng-bihome", plain=r["plain"], mosaic=r["mosaic"], mosaic_gain=r["mosaic_gain"],
        mosaic_stage_median_us=round(r["mosaic"]["median_us"] - r["plain"]["median_us"], 2),
        exposure_stage_median_us=round(r["mosaic_gain"]["median_us"] - r["mosaic"]["median_us"], 2), **dict(shape, reps=reps))


if __name__ == "__main__":
    main()
