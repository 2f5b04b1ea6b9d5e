"""Device time of the panorama (bihome_amd/align.py panorama / Aligner.sequence; csrc/pano.hip, csrc/blend.hip): B samples of n frames of 480 x 640 uint8,
a pan of 0.45 frame widths per step, on a fitted 720 x 2560 canvas.

    python tools/pano_bench.py [--batch 8] [--frames 8] [--height 480] [--width 640] [--canvas-height 720] [--canvas-width 2560] [--step 0.45]
                               [--rounds 21] [--reps 10] [--warmup 5] [--other-lib LABEL=PATH ...] [--skip-model]

One JSON line per row:
    pano      bh_pano_u8 against (a) the same entry point of other builds of the library, --other-lib LABEL=PATH, e.g. the skip compiled out
              (`make -C bihome_amd/csrc ab ABFLAGS=-DPANO_SKIP=0`, then LABEL=bihome_amd/libbihome_hip_ab.so) or the row mapping
              (ABFLAGS=-DPANO_TILE=0; copy the first A/B library aside before building the second), and whether their outputs are the same
              bits; (b) the route without the kernel: n bh_warp_u8 calls onto the canvas with their validity masks, then the weights,
              products, sums, division and rounding as torch tensor operations; (c) a Tensor.copy_ of the bytes read and written.  The
              share of canvas pixels with 0, 1, 2, 3+ frames is printed with it.
    frame     bh_pano_frame, one launch for the n frames, against n - 1 launches of it for a single frame each (`mosaic_frame_device`, the
              pair's frame, which is the same kernel with n = 1)
    n2        bh_pano_u8 with n = 2 against bh_mosaic_u8 on tools/mosaic_bench.py's workload (64 pairs on a fitted 640 x 960 canvas), and
              whether the two outputs are the same bits
    sequence  Aligner.sequence end to end without and with canvas=(Hc, Wc), zeng-bihome at random initialisation

The method is tools/mosaic_bench.py's: the callables of a row alternate in this one process, `--rounds` rounds (at least 20) of `--reps`
launches behind `--warmup` launches each, every round between two device events; median and spread over the rounds."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import _lib, align, configs, synth  # noqa: E402
from bihome_amd.step import build_model  # noqa: E402
from align_bench import copy_pair, raw_call  # noqa: E402
from datagen_bench import device_rounds  # noqa: E402
from mosaic_bench import border_weight  # noqa: E402


def out(case, **kw):
    print(json.dumps({"tool": "pano_bench", "case": case, "device": torch.cuda.get_device_name(0), **kw}), flush=True)


def other_call(path, name, *args):
    """`raw_call` on another build of the library."""
    fn = getattr(ctypes.CDLL(path), name)
    fn.argtypes, fn.restype = _lib.SIGNATURES[name], ctypes.c_int
    pv = ctypes.c_void_p
    args = tuple(pv(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args) + (pv(torch.cuda.current_stream().cuda_stream),)
    return lambda: _lib.check(fn(*args), name)


def pan(rng, B, n, h, w, step, frac=0.08):
    """G [B,n,3,3]: frame k sits (k - r) step w to the right of the reference r = n // 2, its corners moved by up to `frac` of each side."""
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    r = n // 2
    G = np.empty((B, n, 3, 3))
    for b in range(B):
        for k in range(n):
            C = np.eye(3) if k == r else synth.four_point_homography(c, c + rng.uniform(-frac, frac, (4, 2)) * np.array([w, h]))
            g = C @ np.array([[1.0, 0, -(k - r) * step * w], [0, 1.0, (1 if b % 2 == 0 else -1) * (k - r) * 0.1 * h], [0, 0, 1.0]])
            G[b, k] = g / g[2, 2]
    return G


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
    ap.add_argument("--other-lib", action="append", default=[], metavar="LABEL=PATH", help="another build of libbihome_hip.so whose bh_pano_u8 is timed too")
    ap.add_argument("--skip-model", action="store_true", help="kernel rows only")
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

    # the frame: one launch for n frames against n - 1 single-frame launches
    T, bbox, fitted, M = align.pano_frame_device(G, (h, w), (Hc, Wc))
    frame = raw_call("bh_pano_frame", G, None, B, n, h, w, h, w, Hc, Wc, 2.0, T, bbox, fitted, M)
    others = [G[:, k].contiguous() for k in range(n) if k != n // 2]
    r = device_rounds({"pano_frame": frame, "single_frames": lambda: [align.mosaic_frame_device(H, (h, w), (h, w), (Hc, Wc)) for H in others]},
                      a.reps, a.rounds, a.warmup)
    out("bh_pano_frame for n frames against n - 1 single-frame launches (mosaic_frame_device)", pano_frame=r["pano_frame"], single_frames=r["single_frames"],
        fitted=int(fitted.sum().item()), **shape)

    # the blend
    res = torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device="cuda")
    count = torch.empty((B, Hc, Wc), dtype=torch.uint8, device="cuda")
    args = (bank, idx, B * n, h, w, M, None, None, B, n, Hc, Wc, feather, 0)
    fns = {"pano": raw_call("bh_pano_u8", *args, res, count)}
    other_out = {}
    for spec in a.other_lib:
        label, path = spec.split("=", 1)
        other_out[label] = (torch.empty_like(res), torch.empty_like(count))
        fns[label] = other_call(path, "bh_pano_u8", *args, *other_out[label])
    warped, valid = torch.empty_like(res), torch.empty_like(count)
    Mk, idx_k = [M[:, k].contiguous() for k in range(n)], [idx[:, k].contiguous() for k in range(n)]      # (kept: raw_call holds pointers only)
    warps = [raw_call("bh_warp_u8", bank, idx_k[k], B * n, h, w, Mk[k], B, Hc, Wc, warped, valid) for k in range(n)]
    ys, xs = torch.meshgrid(torch.arange(Hc, dtype=torch.float32, device="cuda"), torch.arange(Wc, dtype=torch.float32, device="cuda"), indexing="ij")
    route = {}

    def warp_route():
        num = torch.zeros((B, Hc, Wc, 3), dtype=torch.float32, device="cuda")
        den = torch.zeros((B, Hc, Wc), dtype=torch.float32, device="cuda")
        cnt = torch.zeros((B, Hc, Wc), dtype=torch.uint8, device="cuda")
        for k in range(n):
            warps[k]()
            wk = border_weight(Mk[k], xs, ys, w, h, feather) * valid
            num += warped * wk[..., None]
            den += wk
            cnt += valid
        route["out"] = torch.floor(num / den.clamp(min=1.0)[..., None] + 0.5).to(torch.uint8)
        route["count"] = cnt
    fns["warp_route"] = warp_route
    moved = B * n * h * w * 3 + B * Hc * Wc * 4
    src, dst = copy_pair(moved)
    fns["copy"] = lambda: dst.copy_(src)
    r = device_rounds(fns, a.reps, a.rounds, a.warmup)
    for fn in fns.values():
        fn()
    differ = float((res != route["out"]).any(-1).float().mean().item())
    largest = int((res.to(torch.int16) - route["out"].to(torch.int16)).abs().max().item())
    out("bh_pano_u8 against other builds, n bh_warp_u8 + the torch formulation of weights and blend, and a copy",
        **{k: v for k, v in r.items() if k != "copy"}, device_copy_same_bytes=r["copy"], bytes_moved=moved,
        pano_GBps=round(moved / (r["pano"]["median_us"] * 1e-6) / 1e9, 1), copy_GBps=round(moved / (r["copy"]["median_us"] * 1e-6) / 1e9, 1),
        share_of_copy_rate=round(r["copy"]["median_us"] / r["pano"]["median_us"], 3),
        pano_over_warp_route=round(r["pano"]["median_us"] / r["warp_route"]["median_us"], 3),
        pano_not_above_warp_route=bool(r["pano"]["median_us"] <= r["warp_route"]["median_us"]),
        pano_over_other={k: round(r["pano"]["median_us"] / r[k]["median_us"], 3) for k in other_out},
        other_same_bits={k: bool(torch.equal(o, res) and torch.equal(c, count)) for k, (o, c) in other_out.items()},
        share_of_pixels_that_differ_from_warp_route=differ, largest_difference_grey_levels=largest,
        count_differs_from_warp_route=float((count != route["count"]).float().mean().item()),
        count_shares=[round(float((count == k).float().mean().item()), 3) for k in range(3)] + [round(float((count >= 3).float().mean().item()), 3)], **shape)
    route.clear()
    del warped, valid, src, dst, other_out, fns

    # n = 2 on tools/mosaic_bench.py's workload, against bh_mosaic_u8
    B2, Hc2, Wc2 = 64, 640, 960
    images = torch.from_numpy(few).cuda().repeat(B2 // 4, 1, 1, 1).contiguous()
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    H = torch.from_numpy(np.stack([synth.four_point_homography(c, c + rng.uniform(-0.2, 0.2, (4, 2)) * np.array([w, h])) for _ in range(B2)])).cuda()
    T2 = align.mosaic_frame_device(H, (h, w), (h, w), (Hc2, Wc2))[0]
    Ma, Mb = (H @ T2).contiguous(), T2.contiguous()
    ia = torch.arange(B2, dtype=torch.int32, device="cuda")
    ib = ia.flip(0).contiguous()
    o1, c1 = torch.empty((B2, Hc2, Wc2, 3), dtype=torch.uint8, device="cuda"), torch.empty((B2, Hc2, Wc2), dtype=torch.uint8, device="cuda")
    o2, c2 = torch.empty_like(o1), torch.empty_like(c1)
    mosaic = raw_call("bh_mosaic_u8", images, ia, B2, h, w, images, ib, B2, h, w, Ma, Mb, None, B2, Hc2, Wc2, feather, 0, o1, c1)
    idx2, M2 = torch.stack([ia, ib], 1).contiguous(), torch.stack([Ma, Mb], 1).contiguous()
    pano2 = raw_call("bh_pano_u8", images, idx2, B2, h, w, M2, None, None, B2, 2, Hc2, Wc2, feather, 0, o2, c2)
    r = device_rounds({"mosaic": mosaic, "pano_n2": pano2}, a.reps, a.rounds, a.warmup)
    out("bh_pano_u8 with n = 2 against bh_mosaic_u8, tools/mosaic_bench.py's workload", mosaic=r["mosaic"], pano_n2=r["pano_n2"],
        pano_over_mosaic=round(r["pano_n2"]["median_us"] / r["mosaic"]["median_us"], 3), same_bits=bool(torch.equal(o1, o2)),
        count_is_popcount_of_cover=bool(torch.equal(c2, (c1 & 1) + (c1 >> 1))), **dict(shape, batch=B2, frames=2, canvas_height=Hc2, canvas_width=Wc2))
    del o1, o2, c1, c2, images

    if a.skip_model:
        return
    aligner = align.Aligner(build_model(configs.get("zeng-bihome"), "cuda:0"))
    reps = max(1, a.reps // 4)
    fns = {"register": lambda: aligner.sequence(bank, idx=idx), "panorama": lambda: aligner.sequence(bank, idx=idx, canvas=(Hc, Wc), feather=feather)}
    r = device_rounds(fns, reps, a.rounds, a.warmup)
    out("Aligner.sequence end to end without and with canvas=(Hc, Wc)", model="zeng-bihome", register=r["register"], panorama=r["panorama"],
        panorama_stage_median_us=round(r["panorama"]["median_us"] - r["register"]["median_us"], 2), **dict(shape, reps=reps))


if __name__ == "__main__":
    main()
