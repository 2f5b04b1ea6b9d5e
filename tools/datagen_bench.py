"""Time a batch from the two pair generators: the host generator (synth.make_pairs, one numpy loop over the samples) and the device
generator (synth_gpu.GpuPairGenerator.next: the draws, the 8x8 solves and bh_synth_batch), microseconds per batch, one JSON line per
case:

    gray               zeng-bihome's batch: 1-channel 128 x 128 patches, B = 64
    gray+all_points    zeng-orig's batch: the same plus the perspective-field target
    rgb256             zeng-bihome-rgb256's batch: 3-channel 256 x 256 patches, rho 64, B = 32
    pds host draws     zeng-bihome-pds' batch with the photometric records drawn in Python and copied to the device every step
    pds device draws   the same with photometric_draws='device'
    kernel A/B         --other-lib PATH: bh_synth_pairs of another build of the library (e.g. the parent commit's, built in a git
                       worktree with `make -C bihome_amd/csrc`) against this build's, on the same inputs, launches only, the two
                       alternating round by round in this one process, and whether the two outputs are the same bits

    bank               --bank (these rows only): zeng-bihome-pds' and nguyen-orig's batch from a uint8 240 x 320 ImageBank against the
                       float layout over the same pixels, alternating in this one process; bh_bank_gather_u8 alone, its GB/s (bytes
                       read + written) and those of a device copy that moves the same bytes

    ingest             --ingest (these rows only): bh_bank_ingest_u8 alone (Rescale + CenterCrop of raw-size images into 240 x 320 bank
                       slots, tables already on the device), 64 images per launch: 480 x 640 (the exact-halving path), 427 x 640 (the
                       fixed-point path with a crop) and a mixed batch; its GB/s (source bytes inside the crop window + bank bytes
                       written) and those of a device copy that moves the same bytes

    draws              --draws counter (these rows only): `next(64)` with counter-based draws (draws='counter': one bh_synth_draw launch
                       makes every parameter) against device draws (draws='torch', photometric_draws='device'), the two alternating
                       in this one process, for zeng-bihome-pds, zeng-bihome-pds-blobs and zeng-bihome (gray s-coco); then
                       bh_synth_draw alone with and without the blob noise

    python tools/datagen_bench.py [--other-lib ../parent/bihome_amd/libbihome_hip.so]
    python tools/datagen_bench.py --draws counter
    python tools/datagen_bench.py --bank [--bank-images 512]
    python tools/datagen_bench.py --ingest

Device cases: `--warmup` batches, then `--rounds` rounds of `--reps` batches, each round between two device events with one synchronise
at its end (so a round's time is the device's, host gaps included: what a training loop that waits for the batch sees); median, min and
max over the rounds are reported - the spread is max - min.  The host generator is timed with the host clock over --host-reps calls
(each call also makes its four base images, as the function does for every batch)."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bihome_amd import _lib, kernels as K, synth  # noqa: E402
from bihome_amd.synth_gpu import GpuPairGenerator  # noqa: E402


def stats(us):
    s = sorted(us)
    return {"median_us": round(s[len(s) // 2], 2), "min_us": round(s[0], 2), "max_us": round(s[-1], 2), "spread_us": round(s[-1] - s[0], 2)}


def device_rounds(fns, reps, rounds, warmup):
    """fns: {name: callable}.  Per round every callable gets its own timed window of `reps` calls, in turn (interleaved)."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / reps)
    return {k: stats(v) for k, v in us.items()}


def host_time(reps, **kw):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        synth.make_pairs(**kw)
        t.append((time.perf_counter() - t0) * 1e6)
    return stats(t)


def kernel_ab(other_path, B, reps, rounds, warmup):
    """bh_synth_pairs of two builds on one set of inputs (gray, no records, no target), launches only."""
    other = ctypes.CDLL(other_path)
    other.bh_synth_pairs.argtypes = _lib.SIGNATURES["bh_synth_pairs"]
    other.bh_synth_pairs.restype = ctypes.c_int
    gen = GpuPairGenerator(seed=7)
    idx, origin, delta, _ = gen.draw(B)
    H64, _ = K.h4pt_fwd(delta, gen.patch)
    pv = ctypes.c_void_p
    stream = pv(torch.cuda.current_stream().cuda_stream)
    outs, fns = {}, {}
    for name, fn in (("other", other.bh_synth_pairs), ("this", _lib.lib.bh_synth_pairs)):
        p1 = torch.empty(B, 1, gen.patch, gen.patch, device="cuda")
        p2 = torch.empty_like(p1)
        args = (pv(gen.images.data_ptr()), pv(idx.data_ptr()), pv(origin.data_ptr()), pv(H64.data_ptr()), None, B, gen.images.shape[0],
                gen.h, gen.w, gen.patch, 0.443, 0.129, pv(p1.data_ptr()), pv(p2.data_ptr()), stream)
        outs[name] = (p1, p2)
        fns[name] = (lambda fn=fn, args=args: _lib.check(fn(*args), "bh_synth_pairs"))
    res = device_rounds(fns, reps, rounds, warmup)
    res["same_bits"] = bool(torch.equal(outs["other"][0], outs["this"][0]) and torch.equal(outs["other"][1], outs["this"][1]))
    res["this_minus_other_median_us"] = round(res["this"]["median_us"] - res["other"]["median_us"], 2)
    return res


def bank_rows(n_images, B, reps, rounds, warmup, kernel_reps):
    """--bank: `next(B)` of a generator on a uint8 240 x 320 ImageBank against a generator of the float layout over the same pixel values
    (the two alternating round by round in this process), for zeng-bihome-pds (gray 128 x 128) and nguyen-orig (plus image_1); then
    the gather kernel alone against a device copy that moves the same number of bytes (read + written)."""
    from bihome_amd import configs
    from bihome_amd.bank import ImageBank
    dev = torch.cuda.get_device_name(0)
    bank = ImageBank(torch.randint(0, 256, (n_images, 240, 320, 3), dtype=torch.uint8, device="cuda"))
    planes = bank.data.permute(0, 3, 1, 2).float().contiguous()
    for name in ("zeng-bihome-pds", "nguyen-orig"):
        cfg = configs.get(name)
        on_bank = GpuPairGenerator.from_config(cfg, seed=7, bank=bank)
        on_float = GpuPairGenerator.from_config(cfg, seed=7, n_images=1)
        on_float.images, on_float.h, on_float.w = planes, bank.h, bank.w
        a, b = on_bank.next(B), on_float.next(B)
        same = all(torch.equal(a[k], b[k]) for k in a)
        r = device_rounds({"bank": lambda: on_bank.next(B), "float": lambda: on_float.next(B)}, reps, rounds, warmup)
        print(json.dumps({"tool": "datagen_bench", "case": "bank: " + name, "batch": B, "device": dev, "reps": reps, "rounds": rounds,
                          "bank_images": n_images, "bank_bytes": bank.nbytes, "float_layout_bytes": planes.numel() * 4,
                          "uint8_bank": r["bank"], "float_layout": r["float"], "same_bits": bool(same),
                          "bank_minus_float_median_us": round(r["bank"]["median_us"] - r["float"]["median_us"], 2)}), flush=True)
    idx = torch.randint(0, n_images, (B,), dtype=torch.int32, device="cuda")
    out = torch.empty(B, 3, bank.h, bank.w, device="cuda")
    moved = B * bank.h * bank.w * 3 * (1 + 4)                            # bytes read from the bank + bytes written as floats
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    r = device_rounds({"gather": lambda: bank.gather(idx, out), "copy": lambda: dst.copy_(src)}, kernel_reps, rounds, warmup)
    gbs = {k: round(moved / (r[k]["median_us"] * 1e-6) / 1e9, 1) for k in r}
    print(json.dumps({"tool": "datagen_bench", "case": "bank: bh_bank_gather_u8 alone", "batch": B, "device": dev, "reps": kernel_reps,
                      "rounds": rounds, "bytes_moved": moved, "gather": r["gather"], "gather_GBps": gbs["gather"],
                      "device_copy_same_bytes": r["copy"], "copy_GBps": gbs["copy"],
                      "gather_over_copy_bandwidth": round(gbs["gather"] / gbs["copy"], 3)}), flush=True)


def ingest_rows(B, rounds, warmup, kernel_reps):
    """--ingest: one bh_bank_ingest_u8 launch of B raw-size images into a [B,240,320,3] bank against a device copy that moves the same
    number of bytes (read + written).  Bytes read: of every source image the part inside the crop window, h w 3 (H W) / (nh nw)."""
    import numpy as np
    from bihome_amd.bank import rescale_size
    dev = torch.cuda.get_device_name(0)
    W, H = 320, 240
    cases = [("480x640 (exact halving)", [(480, 640)]), ("427x640 (fixed point, crop in x)", [(427, 640)]),
             ("mixed", [(480, 640), (427, 640), (640, 480), (375, 500), (240, 320), (612, 612), (333, 500), (480, 360)])]
    for name, sizes in cases:
        hw = np.asarray([sizes[k % len(sizes)] for k in range(B)], np.int32)
        nbytes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
        off = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        src = torch.randint(0, 256, (int(nbytes.sum()),), dtype=torch.uint8, device="cuda")
        read = 0.0
        for h, w in hw.tolist():
            nh, nw, _, _ = rescale_size(h, w, (W, H))
            read += h * w * 3 * (H * W) / (nh * nw)
        moved = int(read) + B * H * W * 3
        bank = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
        off_d, hw_d = torch.from_numpy(off).cuda(), torch.from_numpy(hw).cuda()
        a, b = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        r = device_rounds({"ingest": lambda: K.bank_ingest_u8(src, off_d, hw_d, bank), "copy": lambda: b.copy_(a)}, kernel_reps, rounds, warmup)
        gbs = {k: round(moved / (r[k]["median_us"] * 1e-6) / 1e9, 1) for k in r}
        print(json.dumps({"tool": "datagen_bench", "case": "ingest: " + name, "batch": B, "device": dev, "reps": kernel_reps, "rounds": rounds,
                          "source_bytes": int(nbytes.sum()), "bytes_moved": moved, "ingest": r["ingest"], "ingest_GBps": gbs["ingest"],
                          "device_copy_same_bytes": r["copy"], "copy_GBps": gbs["copy"],
                          "ingest_over_copy_bandwidth": round(gbs["ingest"] / gbs["copy"], 3)}), flush=True)


def draws_rows(B, reps, rounds, warmup, kernel_reps):
    """--draws counter: `next(B)` of a generator with counter-based draws against one with device draws (the two alternating round by
    round in this process), then the draw entry point alone (its outputs allocated once)."""
    from bihome_amd import configs
    dev = torch.cuda.get_device_name(0)
    for name in ("zeng-bihome-pds", "zeng-bihome-pds-blobs", "zeng-bihome"):
        cfg = configs.get(name)
        counter = GpuPairGenerator.from_config(cfg, seed=7, draws="counter")
        device = GpuPairGenerator.from_config(cfg, seed=7, draws="torch", photometric_draws="device")
        r = device_rounds({"counter": lambda: counter.next(B), "device": lambda: device.next(B)}, reps, rounds, warmup)
        diff = round(r["counter"]["median_us"] - r["device"]["median_us"], 2)
        spread = max(r["counter"]["spread_us"], r["device"]["spread_us"])
        print(json.dumps({"tool": "datagen_bench", "case": "draws: " + name, "batch": B, "device": dev, "reps": reps, "rounds": rounds,
                          "counter_draws": r["counter"], "device_draws": r["device"], "counter_minus_device_median_us": diff,
                          "counter_not_slower_than_spread": bool(diff <= spread)}), flush=True)
    gen = GpuPairGenerator.from_config(configs.get("zeng-bihome-pds-blobs"), seed=7, draws="counter")
    P = gen.patch
    idx = torch.empty(B, dtype=torch.int32, device="cuda")
    origin, delta, photo = torch.empty(B, 2, device="cuda"), torch.empty(B, 4, 2, device="cuda"), torch.empty(B, 2, 6, device="cuda")
    noise, other = torch.empty(B, P, P, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    geom = (gen.n_images, gen.h, gen.w, P, gen.rho, gen.pmd)
    r = device_rounds({"params": lambda: K.synth_draw(7, 0, *geom, idx, origin, delta, photo),
                       "params+noise": lambda: K.synth_draw(7, 0, *geom, idx, origin, delta, photo, noise, other)},
                      kernel_reps, rounds, warmup)
    print(json.dumps({"tool": "datagen_bench", "case": "draws: bh_synth_draw alone", "batch": B, "patch": P, "device": dev,
                      "reps": kernel_reps, "rounds": rounds, "parameters_and_records": r["params"], "with_blob_noise": r["params+noise"],
                      "noise_bytes": B * P * P * 4}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", choices=["counter"], default=None,
                    help="only the draw rows: counter-based draws against device draws, and bh_synth_draw alone")
    ap.add_argument("--bank", action="store_true", help="only the image-bank rows: uint8 bank against the float layout, and the gather kernel")
    ap.add_argument("--bank-images", type=int, default=512)
    ap.add_argument("--ingest", action="store_true", help="only the ingest rows: bh_bank_ingest_u8 (Rescale + CenterCrop into bank slots) against a device copy")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--other-lib", default=None, help="another build of libbihome_hip.so for the kernel A/B case")
    ap.add_argument("--kernel-reps", type=int, default=2000)
    args = ap.parse_args()
    if args.draws:
        draws_rows(64, args.reps, args.rounds, args.warmup, args.kernel_reps)
        return
    if args.ingest:
        ingest_rows(64, args.rounds, args.warmup, args.kernel_reps)
        return
    if args.bank:
        bank_rows(args.bank_images, 64, args.reps, args.rounds, args.warmup, args.kernel_reps)
        return
    dev = torch.cuda.get_device_name(0)
    cases = [
        ("gray", 64, dict(), dict()),
        ("gray+all_points", 64, dict(target_gen="all_points"), dict(target=True)),
        ("rgb256", 32, dict(patch=256, rho=64, channels=3), dict(patch=256, rho=64, channels=3)),
        ("pds host draws", 64, dict(photometric_max_delta=32, photometric_draws="host"), dict(photometric_max_delta=32)),
        ("pds device draws", 64, dict(photometric_max_delta=32, photometric_draws="device"), None),
    ]
    for name, B, gkw, hkw in cases:
        gen = GpuPairGenerator(**gkw)
        res = {"tool": "datagen_bench", "case": name, "batch": B, "device": dev, "reps": args.reps, "rounds": args.rounds,
               "device_generator": device_rounds({"next": lambda: gen.next(B)}, args.reps, args.rounds, args.warmup)["next"]}
        if hkw is not None and not args.no_host:
            res["host_generator"] = dict(host_time(args.host_reps, batch=B, **hkw), reps=args.host_reps)
        print(json.dumps(res), flush=True)
    res = {"tool": "datagen_bench", "case": "kernel A/B (gray, no target)", "batch": 64, "device": dev, "reps": args.kernel_reps,
           "rounds": args.rounds}
    if args.other_lib:
        res.update(kernel_ab(args.other_lib, 64, args.kernel_reps, args.rounds, args.warmup))
    else:
        res["not_measured"] = "no --other-lib given"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
