"""Device time of the ECC refinement (bihome_amd/align.py ecc_refine; csrc/ecc.hip), B pairs of 480 x 640 uint8 images.

    python tools/align_refine_bench.py [--batch 64] [--height 480] [--width 640] [--levels 3] [--iters 10] [--rounds 9] [--reps 20]

One JSON line per row:
    pyramid  bh_gray_pyramid_u8 alone (one image set, `levels` levels) against a Tensor.copy_ that moves the bytes it reads and writes
    pass     one level-0 bh_ecc_sums pass (both gray planes read once: 2 x B x H x W x 4 bytes) against a copy that moves the same bytes
    refine   bh_ecc_refine alone on resident pyramids, levels x (iters + 1) passes, and its share that a level-0 pass accounts for
    aligner  Aligner end to end with refine="ecc" against refine=None, zeng-bihome at random initialisation

The method is tools/datagen_bench.py --bank's (see tools/align_bench.py): the two callables of a row alternate in this one process,
`--rounds` rounds of `--reps` launches behind `--warmup` launches each, every round between two device events; median and spread."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import align, configs, kernels as K, synth  # noqa: E402
from bihome_amd.step import build_model  # noqa: E402
from align_bench import copy_pair, raw_call  # noqa: E402
from datagen_bench import device_rounds  # noqa: E402


def out(case, **kw):
    print(json.dumps({"tool": "align_refine_bench", "case": case, "device": torch.cuda.get_device_name(0), **kw}), flush=True)


def gbps(moved, r, k):
    return round(moved / (r[k]["median_us"] * 1e-6) / 1e9, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true", help="kernel rows only")
    a = ap.parse_args()
    B, h, w, L = a.batch, a.height, a.width, a.levels
    shape = dict(batch=B, height=h, width=w, levels=L, iters=a.iters, rounds=a.rounds, reps=a.reps)
    rng = np.random.default_rng(0)
    few = np.stack([np.floor(synth.texture_image(rng, h, w) + 0.5).astype(np.uint8) for _ in range(4)])
    images_a = torch.from_numpy(few).cuda().repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    images_b = images_a.clone()
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    H = torch.from_numpy(np.stack([synth.four_point_homography(c, c + rng.uniform(-3, 3, (4, 2))) for _ in range(B)])).cuda()

    total = K.gray_pyramid_layout(h, w, L)[-1]
    pyr_a = torch.empty((B, total), dtype=torch.float32, device="cuda")
    moved = B * h * w * 3 + B * total * 4 + B * (total - h * w) * 4          # the image, every level written, every level but the last read
    src, dst = copy_pair(moved)
    pyramid = raw_call("bh_gray_pyramid_u8", images_a, None, B, h, w, B, L, pyr_a)
    r = device_rounds({"pyramid": pyramid, "copy": lambda: dst.copy_(src)}, a.reps, a.rounds, a.warmup)
    out("bh_gray_pyramid_u8 alone", bytes_moved=moved, pyramid=r["pyramid"], pyramid_GBps=gbps(moved, r, "pyramid"), device_copy_same_bytes=r["copy"],
        copy_GBps=gbps(moved, r, "copy"), **shape)

    pyr_b = align.gray_pyramid(images_b, B, L)
    partial = torch.empty((K.ecc_sums_ws_doubles(h, w, B),), dtype=torch.float64, device="cuda")
    sums = torch.empty((B, 66), dtype=torch.float64, device="cuda")
    moved = 2 * B * h * w * 4
    src, dst = copy_pair(moved)
    one = raw_call("bh_ecc_sums", pyr_a, h, w, total, pyr_b, h, w, total, None, H, B, partial, sums)
    r = device_rounds({"pass": one, "copy": lambda: dst.copy_(src)}, a.reps, a.rounds, a.warmup)
    out("one level-0 bh_ecc_sums pass", bytes_moved=moved, **{"pass": r["pass"]}, pass_GBps=gbps(moved, r, "pass"), device_copy_same_bytes=r["copy"],
        copy_GBps=gbps(moved, r, "copy"), share_of_copy_rate=round(gbps(moved, r, "pass") / gbps(moved, r, "copy"), 3), **shape)
    pass_us = r["pass"]["median_us"]

    Hw = H.clone()
    stats = torch.empty((B, L, 3), dtype=torch.float64, device="cuda")
    ws = torch.empty((K.ecc_refine_ws_doubles(h, w, B),), dtype=torch.float64, device="cuda")
    refine = raw_call("bh_ecc_refine", pyr_a, h, w, pyr_b, h, w, None, B, L, a.iters, Hw, stats, ws)

    def refine_from_start():
        Hw.copy_(H)
        refine()
    reps = max(1, a.reps // 4)
    r = device_rounds({"refine": refine_from_start, "copy": lambda: dst.copy_(src)}, reps, a.rounds, a.warmup)
    out("bh_ecc_refine on resident pyramids", refine=r["refine"], level0_passes=a.iters + 1,
        level0_passes_share=round((a.iters + 1) * pass_us / r["refine"]["median_us"], 3), launches=1 + 2 * L * (a.iters + 1),
        **dict(shape, reps=reps))

    if a.skip_model:
        return
    model = build_model(configs.get("zeng-bihome"), "cuda:0")
    aligner = align.Aligner(model)
    r = device_rounds({"refined": lambda: aligner(images_a, images_b, refine="ecc", refine_levels=L, refine_iters=a.iters),
                       "plain": lambda: aligner(images_a, images_b)}, reps, a.rounds, a.warmup)
    out("Aligner end to end with and without refine='ecc'", model="zeng-bihome", aligner_refine=r["refined"], aligner_plain=r["plain"],
        refine_adds_median_us=round(r["refined"]["median_us"] - r["plain"]["median_us"], 2), **dict(shape, reps=reps))


if __name__ == "__main__":
    main()
