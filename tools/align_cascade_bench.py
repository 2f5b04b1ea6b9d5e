"""Device time of the cascaded re-prediction (bihome_amd/align.py Aligner(cascade=K); csrc/cascade.hip), B pairs of 480 x 640 uint8
images, P = 128, 5 x 4 sub-samples per patch pixel.

    python tools/align_cascade_bench.py [--batch 64] [--height 480] [--width 640] [--nx 5] [--ny 4] [--rounds 21] [--reps 10] [--warmup 5]

One JSON line per row:
    prep_warp  bh_align_prep_warp_u8 (A through H as the model's patch, one launch) against the two-call route - bh_warp_u8 of A onto
               B's grid, then bh_align_prep_u8 of the result - and against a Tensor.copy_ of A's bytes; `fused_not_above_two_call` is
               the condition the fused kernel is kept on (its median over the rounds is not above the two-call route's in this run),
               and the largest difference of the two patches is reported next to it (the two-call route rounds its intermediate to uint8)
    ncc        bh_patch_ncc against the same sums in torch (double, masked by cover == 1)
    aligner    Aligner end to end with cascade = 0, 1, 2 next to step.predict alone on resident patches, zeng-bihome at random
               initialisation: the cost of a stage

The method is tools/datagen_bench.py --bank's (see tools/align_bench.py): the callables of a row alternate in this one process,
`--rounds` rounds (at least 20) of `--reps` launches behind `--warmup` launches each, every round between two device events; median and
spread over the rounds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import align, configs, synth  # noqa: E402
from bihome_amd.step import build_model, predict  # noqa: E402
from align_bench import copy_pair, raw_call  # noqa: E402
from datagen_bench import device_rounds  # noqa: E402

MEAN, STD = 0.443, 0.129


def out(case, **kw):
    print(json.dumps({"tool": "align_cascade_bench", "case": case, "device": torch.cuda.get_device_name(0), **kw}), flush=True)


def ncc_torch(w, t, cover):
    """bh_patch_ncc's sums and rho in torch: double, all channels of the pixels with cover == 1."""
    m = (cover == 1.0)[:, None].to(torch.float64)
    wd, td = w.double() * m, t.double() * m
    n = m.sum((1, 2, 3)) * w.shape[1]
    sw, st, sww, stt, swt = wd.sum((1, 2, 3)), td.sum((1, 2, 3)), (wd * wd).sum((1, 2, 3)), (td * td).sum((1, 2, 3)), (wd * td).sum((1, 2, 3))
    return (n * swt - sw * st) / torch.sqrt((n * sww - sw * sw) * (n * stt - st * st))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--nx", type=int, default=5)
    ap.add_argument("--ny", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true", help="kernel rows only")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds is at least 20: the medians compared come from that many alternating repetitions")
    B, h, w, P, nx, ny = a.batch, a.height, a.width, 128, a.nx, a.ny
    shape = dict(batch=B, height=h, width=w, patch=P, nx=nx, ny=ny, rounds=a.rounds, reps=a.reps)
    rng = np.random.default_rng(0)
    few = np.stack([np.floor(np.clip(synth.texture_image(rng, h, w), 0, 255) + 0.5).astype(np.uint8) for _ in range(4)])
    images_a = torch.from_numpy(few).cuda().repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    images_b = images_a.flip(0).contiguous()
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    H_host = np.stack([synth.four_point_homography(c, c + rng.uniform(-0.1, 0.1, (4, 2)) * np.array([w, h])) for _ in range(B)])
    H = torch.from_numpy(H_host).cuda()
    geom_b = np.tile(np.array([[w / P, h / P, 0.5 * w / P - 0.5, 0.5 * h / P - 0.5]]), (B, 1))
    Hg = torch.from_numpy(H_host @ align.grid_map(geom_b, nx, ny)).cuda().contiguous()

    # the warped preparation: one launch against warp + prepare
    patch = torch.empty((B, 1, P, P), dtype=torch.float32, device="cuda")
    cover = torch.empty((B, P, P), dtype=torch.float32, device="cuda")
    fused = raw_call("bh_align_prep_warp_u8", images_a, None, B, h, w, Hg, B, P, 1, nx, ny, MEAN, STD, patch, cover)
    mid = torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda")
    patch2 = torch.empty_like(patch)
    geom = torch.empty((B, 4), dtype=torch.float64, device="cuda")
    warp = raw_call("bh_warp_u8", images_a, None, B, h, w, H, B, h, w, mid, None)
    prep = raw_call("bh_align_prep_u8", mid, None, B, h, w, None, B, P, 1, MEAN, STD, patch2, geom)

    def two_call():
        warp()
        prep()
    src, dst = copy_pair(2 * B * h * w * 3)
    r = device_rounds({"fused": fused, "two_call": two_call, "copy": lambda: dst.copy_(src)}, a.reps, a.rounds, a.warmup)
    inside = (cover == 1.0)[:, None]
    diff = float(((patch - patch2).abs() * inside).max().item())
    mean_diff = float((((patch - patch2).abs() * inside).sum() / inside.sum()).item())
    out("bh_align_prep_warp_u8 against bh_warp_u8 + bh_align_prep_u8", fused=r["fused"], two_call=r["two_call"],
        device_copy_of_a=r["copy"], bytes_of_a=B * h * w * 3, intermediate_bytes_not_moved=2 * B * h * w * 3,
        fused_over_two_call=round(r["fused"]["median_us"] / r["two_call"]["median_us"], 3),
        fused_not_above_two_call=bool(r["fused"]["median_us"] <= r["two_call"]["median_us"]),
        max_patch_difference_where_covered=diff, mean_patch_difference_where_covered=mean_diff, covered_share=round(float(inside.float().mean().item()), 3), **shape)

    # the score
    t = align.prepare(images_b, B, P, 1, MEAN, STD)[0]
    res = torch.empty((B, 8), dtype=torch.float64, device="cuda")
    ncc = raw_call("bh_patch_ncc", patch, t, cover, B, 1, P, res)
    r = device_rounds({"ncc": ncc, "torch": lambda: ncc_torch(patch, t, cover)}, a.reps, a.rounds, a.warmup)
    ncc()
    out("bh_patch_ncc against the same sums in torch", ncc=r["ncc"], torch_formulation=r["torch"],
        max_rho_difference=float((res[:, 6] - ncc_torch(patch, t, cover)).abs().max().item()), **shape)

    if a.skip_model:
        return
    model = build_model(configs.get("zeng-bihome"), "cuda:0")
    aligner = align.Aligner(model)
    first = aligner(images_a, images_b, warp=False)
    batch = {"patch_1": first["patch_1"], "patch_2": first["patch_2"]}
    reps = max(1, a.reps // 4)
    fns = {"cascade_%d" % k: (lambda k=k: aligner(images_a, images_b, cascade=k, cascade_samples=(nx, ny))) for k in (0, 1, 2)}
    fns["predict"] = lambda: predict(model, dict(batch))
    r = device_rounds(fns, reps, a.rounds, a.warmup)
    out("Aligner end to end with cascade = 0, 1, 2 against step.predict alone", model="zeng-bihome", cascade_0=r["cascade_0"],
        cascade_1=r["cascade_1"], cascade_2=r["cascade_2"], predict_alone=r["predict"],
        stage_median_us=round((r["cascade_2"]["median_us"] - r["cascade_0"]["median_us"]) / 2, 2),
        stage_minus_predict_median_us=round((r["cascade_2"]["median_us"] - r["cascade_0"]["median_us"]) / 2 - r["predict"]["median_us"], 2),
        first_look_median_us=round(2 * r["cascade_1"]["median_us"] - r["cascade_0"]["median_us"] - r["cascade_2"]["median_us"], 2),
        **dict(shape, reps=reps))


if __name__ == "__main__":
    main()
