"""Device time of the two-band blend (bihome_amd/align.py blur_u8 / pano_bands_u8 / panorama(mode="two_band"); csrc/blur.hip,
csrc/blend.hip's band rule) on tools/pano_bench.py's workload: B samples of n frames of 480 x 640 uint8, a pan of 0.45 frame widths per step, on a
fitted 720 x 2560 canvas with feather 32.

    python tools/bands_bench.py [--batch 8] [--frames 8] [--height 480] [--width 640] [--canvas-height 720] [--canvas-width 2560] [--step 0.45]
                                [--feather 32] [--rounds 21] [--reps 10] [--warmup 5] [--other-lib LABEL=PATH ...]

One JSON line per row:
    blur      bh_blur_u8 of the B n frames at sigma 4 (radius 12) and 10.5 (radius 32) against (a) a Tensor.copy_ of the bytes read and
              written and (b) the torch formulation: the frames as a float NCHW copy, replicate padding and two conv2d calls with the
              real-valued taps (its conversion from and to uint8 is timed apart)
    bands     bh_pano_bands_u8 against bh_pano_u8 in feather mode, alternating in this one process, and the share of canvas pixels with
              0, 1, 2, 3+ frames.  --other-lib LABEL=PATH times bh_pano_bands_u8 of another build of the library in the same rounds
              (tools/pano_bench.py's other_call) and reports whether its outputs are the same bits
    pair      bh_mosaic_bands_u8 against bh_mosaic_u8 in feather mode on tools/mosaic_bench.py's workload (64 pairs on a fitted
              640 x 960 canvas), and with --other-lib the same of the other build
    panorama  panorama(mode="two_band") end to end with and without a precomputed low bank, and panorama(mode="feather")

The method is tools/pano_bench.py's: the callables of a row alternate in this one process, `--rounds` rounds (at least 20) of `--reps`
launches behind `--warmup` launches each, every round between two device events; median and spread over the rounds."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import align, synth  # noqa: E402
from align_bench import copy_pair, raw_call  # noqa: E402
from datagen_bench import device_rounds  # noqa: E402
from pano_bench import other_call, pan  # noqa: E402


def out(case, **kw):
    print(json.dumps({"tool": "bands_bench", "case": case, "device": torch.cuda.get_device_name(0), **kw}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--canvas-height", type=int, default=720)
    ap.add_argument("--canvas-width", type=int, default=2560)
    ap.add_argument("--step", type=float, default=0.45)
    ap.add_argument("--feather", type=float, default=32.0)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--other-lib", action="append", default=[], metavar="LABEL=PATH", help="another build of libbihome_hip.so whose two-band blends are timed too")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds is at least 20: the medians compared come from that many alternating repetitions")
    B, n, h, w, Hc, Wc, feather = a.batch, a.frames, a.height, a.width, a.canvas_height, a.canvas_width, a.feather
    shape = dict(batch=B, frames=n, height=h, width=w, canvas_height=Hc, canvas_width=Wc, step=a.step, feather=feather, rounds=a.rounds, reps=a.reps)
    rng = np.random.default_rng(0)
    few = np.stack([np.floor(np.clip(synth.texture_image(rng, h, w), 0, 255) + 0.5).astype(np.uint8) for _ in range(4)])
    bank = torch.from_numpy(few).cuda().repeat((B * n + 3) // 4, 1, 1, 1)[:B * n].contiguous()
    idx = torch.arange(B * n, dtype=torch.int32, device="cuda").reshape(B, n)
    G = torch.from_numpy(pan(rng, B, n, h, w, a.step)).cuda()
    T, bbox, fitted, M = align.pano_frame_device(G, (h, w), (Hc, Wc))

    # the low band
    low = torch.empty((B * n, h, w, 3), dtype=torch.uint8, device="cuda")
    moved = 2 * low.numel()
    src, dst = copy_pair(moved)
    as_float = bank.permute(0, 3, 1, 2).float().contiguous()
    for sigma in (4.0, 10.5):
        taps = align.blur_taps(sigma)
        r_ = len(taps) - 1
        host_taps = (ctypes.c_int * len(taps))(*taps.tolist())
        g = torch.from_numpy(np.concatenate([taps[:0:-1], taps]).astype(np.float32) / 2048.0).cuda()
        kx, ky = g.view(1, 1, 1, -1).repeat(3, 1, 1, 1), g.view(1, 1, -1, 1).repeat(3, 1, 1, 1)
        keep = {}

        def torch_blur():
            x = torch.nn.functional.pad(as_float, (r_, r_, r_, r_), mode="replicate")
            keep["f"] = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, kx, groups=3), ky, groups=3)

        def torch_blur_u8():
            x = torch.nn.functional.pad(bank.permute(0, 3, 1, 2).float(), (r_, r_, r_, r_), mode="replicate")
            y = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, kx, groups=3), ky, groups=3)
            keep["u8"] = torch.floor(y + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        fns = {"blur": raw_call("bh_blur_u8", bank, idx, B * n, h, w, B * n, host_taps, r_, low), "torch_conv2d": torch_blur,
               "torch_conv2d_from_and_to_uint8": torch_blur_u8, "copy": lambda: dst.copy_(src)}
        r = device_rounds(fns, a.reps, a.rounds, a.warmup)
        for fn in fns.values():
            fn()
        diff = (low.to(torch.int16) - keep["u8"].to(torch.int16)).abs()
        out("bh_blur_u8 against two torch conv2d calls on a float copy, and a copy of the same bytes", sigma=sigma, radius=r_,
            **{k: v for k, v in r.items() if k != "copy"}, device_copy_same_bytes=r["copy"], bytes_moved=moved,
            blur_GBps=round(moved / (r["blur"]["median_us"] * 1e-6) / 1e9, 1), copy_GBps=round(moved / (r["copy"]["median_us"] * 1e-6) / 1e9, 1),
            share_of_copy_rate=round(r["copy"]["median_us"] / r["blur"]["median_us"], 3),
            blur_over_torch_conv2d=round(r["blur"]["median_us"] / r["torch_conv2d"]["median_us"], 3),
            largest_difference_from_torch_grey_levels=int(diff.max().item()), share_of_bytes_that_differ_from_torch=float((diff > 0).float().mean().item()), **shape)
        keep.clear()
    del src, dst, as_float

    # the blend: eight taps per present frame against four
    low = align.blur_u8(bank, 4.0, idx).view(B * n, h, w, 3)               # (what the blend reads: sigma 4)
    res, res_f = (torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    count, count_f, winner = (torch.empty((B, Hc, Wc), dtype=torch.uint8, device="cuda") for _ in range(3))
    args = (bank, low, idx, B * n, h, w, M, None, None, B, n, Hc, Wc, feather)
    fns = {"bands": raw_call("bh_pano_bands_u8", *args, res, count, winner),
           "pano_feather": raw_call("bh_pano_u8", bank, idx, B * n, h, w, M, None, None, B, n, Hc, Wc, feather, 0, res_f, count_f)}
    other_libs = dict(spec.split("=", 1) for spec in a.other_lib)
    other_out = {label: (torch.empty_like(res), torch.empty_like(count), torch.empty_like(winner)) for label in other_libs}
    fns.update({label: other_call(path, "bh_pano_bands_u8", *args, *other_out[label]) for label, path in other_libs.items()})
    r = device_rounds(fns, a.reps, a.rounds, a.warmup)
    for fn in fns.values():
        fn()
    diff = (res.to(torch.int16) - res_f.to(torch.int16)).abs()
    out("bh_pano_bands_u8 against bh_pano_u8 in feather mode", **r, bands_over_other={k: round(r["bands"]["median_us"] / r[k]["median_us"], 3) for k in other_libs},
        other_same_bits={k: all(torch.equal(x, y) for x, y in zip(o, (res, count, winner))) for k, o in other_out.items()},
        bands_over_pano_feather=round(r["bands"]["median_us"] / r["pano_feather"]["median_us"], 3), same_count=bool(torch.equal(count, count_f)),
        mean_difference_from_feather_grey_levels=round(float(diff.float().mean().item()), 3), largest_difference_from_feather_grey_levels=int(diff.max().item()),
        count_shares=[round(float((count == k).float().mean().item()), 3) for k in range(3)] + [round(float((count >= 3).float().mean().item()), 3)], **shape)

    # the pair, on tools/mosaic_bench.py's workload
    B2, Hc2, Wc2 = 64, 640, 960
    images = torch.from_numpy(few).cuda().repeat(B2 // 4, 1, 1, 1).contiguous()
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    H = torch.from_numpy(np.stack([synth.four_point_homography(c, c + rng.uniform(-0.2, 0.2, (4, 2)) * np.array([w, h])) for _ in range(B2)])).cuda()
    T2 = align.mosaic_frame_device(H, (h, w), (h, w), (Hc2, Wc2))[0]
    Ma, Mb = (H @ T2).contiguous(), T2.contiguous()
    ia = torch.arange(B2, dtype=torch.int32, device="cuda")
    ib = ia.flip(0).contiguous()
    low_a, low_b = align.blur_u8(images, 4.0, ia), align.blur_u8(images, 4.0, ib)
    res2, res2_f = (torch.empty((B2, Hc2, Wc2, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    cover2, cover2_f, winner2 = (torch.empty((B2, Hc2, Wc2), dtype=torch.uint8, device="cuda") for _ in range(3))
    args = (images, low_a, ia, B2, h, w, images, low_b, ib, B2, h, w, Ma, Mb, None, B2, Hc2, Wc2, feather)
    fns = {"mosaic_bands": raw_call("bh_mosaic_bands_u8", *args, res2, cover2, winner2),
           "mosaic_feather": raw_call("bh_mosaic_u8", images, ia, B2, h, w, images, ib, B2, h, w, Ma, Mb, None, B2, Hc2, Wc2, feather, 0, res2_f, cover2_f)}
    other_out = {label: (torch.empty_like(res2), torch.empty_like(cover2), torch.empty_like(winner2)) for label in other_libs}
    fns.update({label: other_call(path, "bh_mosaic_bands_u8", *args, *other_out[label]) for label, path in other_libs.items()})
    r = device_rounds(fns, a.reps, a.rounds, a.warmup)
    for fn in fns.values():
        fn()
    out("bh_mosaic_bands_u8 against bh_mosaic_u8 in feather mode, tools/mosaic_bench.py's workload", **r,
        bands_over_mosaic_feather=round(r["mosaic_bands"]["median_us"] / r["mosaic_feather"]["median_us"], 3), same_cover=bool(torch.equal(cover2, cover2_f)),
        bands_over_other={k: round(r["mosaic_bands"]["median_us"] / r[k]["median_us"], 3) for k in other_libs},
        other_same_bits={k: all(torch.equal(x, y) for x, y in zip(o, (res2, cover2, winner2))) for k, o in other_out.items()},
        **dict(shape, batch=B2, frames=2, canvas_height=Hc2, canvas_width=Wc2))
    del res2, res2_f, cover2, cover2_f, winner2, other_out, images, low_a, low_b

    # the public function
    low5 = low.view(B, n, h, w, 3)
    fns = {"two_band": lambda: align.panorama(bank, G, idx=idx, canvas=(Hc, Wc), feather=feather, mode="two_band"),
           "two_band_with_low": lambda: align.panorama(bank, G, idx=idx, canvas=(Hc, Wc), feather=feather, mode="two_band", low=low5),
           "feather_mode": lambda: align.panorama(bank, G, idx=idx, canvas=(Hc, Wc), feather=feather)}
    r = device_rounds(fns, a.reps, a.rounds, a.warmup)
    out("panorama(mode='two_band') end to end without and with a precomputed low bank, and mode='feather'", **r,
        low_bank_median_us=round(r["two_band"]["median_us"] - r["two_band_with_low"]["median_us"], 2), **shape)


if __name__ == "__main__":
    main()
