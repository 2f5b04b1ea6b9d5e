"""Device time of the image-alignment path (bihome_amd/align.py; csrc/align.hip), B pairs of 480 x 640 uint8 images.

    python tools/align_bench.py [--batch 64] [--height 480] [--width 640] [--rounds 9] [--reps 20] [--warmup 5]

One JSON line per row:
    prep    bh_align_prep_u8 alone (whole images -> 128 x 128 gray patches) against a Tensor.copy_ that moves the bytes it reads and writes
    warp    bh_warp_u8 alone (homographies whose corners move by up to 10 % of each side) against a copy of the bytes it reads and
            writes; the bytes read are counted as the whole source once (the taps of a smooth map touch each source pixel about once)
    aligner Aligner end to end (prepare both, predict, lift, warp) against step.predict alone on resident patches, zeng-bihome at
            random initialisation

The method is tools/datagen_bench.py --bank's: the two callables of a row alternate in this one process, `--rounds` rounds of `--reps`
launches behind `--warmup` launches each, every round between two device events; median and max - min spread over the rounds."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import _lib, align, configs, synth  # noqa: E402
from bihome_amd.step import build_model, predict  # noqa: E402
from datagen_bench import device_rounds  # noqa: E402


def raw_call(name, *args):
    """The entry point itself on preallocated buffers (the tensor-level wrapper allocates its outputs, which costs the host more than
    a short kernel costs the device): a callable that launches once."""
    fn = getattr(_lib.lib, name)
    pv = ctypes.c_void_p
    args = tuple(pv(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args) + (pv(torch.cuda.current_stream().cuda_stream),)
    return lambda: _lib.check(fn(*args), name)


def copy_pair(nbytes):
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    return src, torch.empty_like(src)


def row(case, r, ours, moved, **extra):
    gbs = {k: round(moved / (r[k]["median_us"] * 1e-6) / 1e9, 1) for k in (ours, "copy")}
    print(json.dumps({"tool": "align_bench", "case": case, "device": torch.cuda.get_device_name(0), "bytes_moved": moved, ours: r[ours],
                      ours + "_GBps": gbs[ours], "device_copy_same_bytes": r["copy"], "copy_GBps": gbs["copy"],
                      "share_of_copy_rate": round(gbs[ours] / gbs["copy"], 3), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true", help="kernel rows only")
    a = ap.parse_args()
    B, h, w, P = a.batch, a.height, a.width, 128
    shape = dict(batch=B, height=h, width=w, rounds=a.rounds, reps=a.reps)
    images_a = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, device="cuda")
    images_b = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, device="cuda")

    moved = B * h * w * 3 + B * P * P * 4
    src, dst = copy_pair(moved)
    patch = torch.empty((B, 1, P, P), dtype=torch.float32, device="cuda")
    geom = torch.empty((B, 4), dtype=torch.float64, device="cuda")
    prep = raw_call("bh_align_prep_u8", images_a, None, B, h, w, None, B, P, 1, 0.443, 0.129, patch, geom)
    r = device_rounds({"prep": prep, "copy": lambda: dst.copy_(src)}, a.reps, a.rounds, a.warmup)
    row("bh_align_prep_u8 alone", r, "prep", moved, patch=P, channels=1, **shape)

    rs = np.random.RandomState(0)
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    H = np.stack([synth.four_point_homography(c, c + rs.uniform(-0.1, 0.1, (4, 2)) * np.array([w, h])) for _ in range(B)])
    H = torch.from_numpy(H).cuda()
    moved = B * h * w * (3 + 3 + 1)
    src, dst = copy_pair(moved)
    out = torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda")
    valid = torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
    warp = raw_call("bh_warp_u8", images_a, None, B, h, w, H, B, h, w, out, valid)
    r = device_rounds({"warp": warp, "copy": lambda: dst.copy_(src)}, a.reps, a.rounds, a.warmup)
    row("bh_warp_u8 alone", r, "warp", moved, **shape)

    if a.skip_model:
        return
    model = build_model(configs.get("zeng-bihome"), "cuda:0")
    aligner = align.Aligner(model)
    first = aligner(images_a, images_b)
    batch = {"patch_1": first["patch_1"], "patch_2": first["patch_2"]}
    reps = max(1, a.reps // 4)
    r = device_rounds({"aligner": lambda: aligner(images_a, images_b), "predict": lambda: predict(model, dict(batch))}, reps, a.rounds, a.warmup)
    print(json.dumps({"tool": "align_bench", "case": "Aligner end to end against step.predict on resident patches",
                      "device": torch.cuda.get_device_name(0), "model": "zeng-bihome", **dict(shape, reps=reps), "aligner": r["aligner"],
                      "predict_alone": r["predict"],
                      "aligner_minus_predict_median_us": round(r["aligner"]["median_us"] - r["predict"]["median_us"], 2)}), flush=True)


if __name__ == "__main__":
    main()
