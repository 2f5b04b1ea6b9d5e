#!/usr/bin/env python3
"""Benchmark of the biHomE training hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one full training iteration of BASELINE.json configs[1]: s-coco Zeng backbone + biHomE head,
batch 64 per GPU, 128x128 grayscale synthetic COCO-style pairs, fp32: model.train(), zero_grad, forward,
backward, (N>1: RCCL all-reduce SUM of the flat gradient), Adam step, MultiStepLR step
(train.py:296-387).  Inputs are resident in HBM before the timed region.  The timed region starts from the seeded
initial weights with a fresh optimizer state, and the last timed step starts from them again (seeded_state), so that
what that step computes depends on the arguments alone.  Rank 0 prints ONE JSON line with the whole-job
image-pairs/s and ms_per_step.  A plain run does nothing else: set-up, W warm-up steps, K timed steps, the outputs
of the last timed step (--dump-outputs), the line.  --full adds the secondary legs after the timed steps: the eval
leg, the roofline of the dominant kernel (per-launch HIP-event timing inside this process) with the measured peaks,
the exact-arithmetic (f32x3) step time, at N>1 the exchange diagnostics and, at N=1, the CPU baseline (the oracle =
PyTorch-CPU restatement, timed on the host cores).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16, dense (~2.5 PF)
X3_PRODUCTS = {3: 6, 2: 3}        # bf16 MFMA products per fp32 product by pieces per operand: f32x3 (common.h bh_split8), f32x2 (bh_split8_2)


def x3_pieces(kernel):
    """Split-operand kernels: bf16 pieces per operand (3 = f32x3, 2 = f32x2; the algorithmic flops of a launch are executed as
    X3_PRODUCTS[pieces] bf16 MFMA flops each), 0 for every other kernel."""
    if kernel.startswith("wgrad_x3_kernel<"):                     # template arguments: CB, BNI, NP
        args = kernel[len("wgrad_x3_kernel<"):].split(">")[0].split(",")
        return int(args[2]) if len(args) >= 3 else 3
    if kernel.startswith("conv3x3_pc_kernel<"):                   # template arguments: DGRAD, BNI - fp16 pieces only (csrc/conv3x3_pc.hip)
        return 2
    if kernel.startswith("conv3x3_halo_kernel<"):                 # template arguments: FLIP, BN, BF16, SUBT, PACKED, X3, BNI, NP
        args = kernel[len("conv3x3_halo_kernel<"):].split(">")[0].split(",")
        if len(args) >= 6 and args[5] == "true":
            return int(args[7]) if len(args) >= 8 else 3
    return 0
F16X2_TEXT = ("fp32 tensors, fp32 accumulate; 3x3 / stride-1 convs (fwd, dgrad, wgrad): each fp32 operand times a power-of-two scale per "
              "tensor as two FP16 pieces (22 significand bits and a sign), 3 partial products per product on v_mfma_f32_32x32x16_f16 "
              "(~2^-22 per product; error vs float64 <= the fp32-input MFMA form: tests/test_f16x2_gpu.py), results rescaled exactly; all "
              "other convs: v_mfma_f32_32x32x2_f32")
def x3_is_f16(kernel):
    """fp16 pieces with per-tensor scales (the last template argument of both split-operand kernels; v_mfma_f32_32x32x16_f16)."""
    if kernel.startswith("conv3x3_pc_kernel<"):
        return True
    args = kernel.split(">")[0].split(",")
    if kernel.startswith("wgrad_x3_kernel<"):                     # CB, BNI, NP, F16[, PC, MAP4]
        return len(args) >= 4 and args[3] == "true"
    return bool(x3_pieces(kernel)) and len(args) == 10 and args[-1] == "true"


PEAK_HBM_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)     # (round 4: 1.4 s of timed region by default - round-3 VERDICT: ">= 100 next time")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=None, help="image pairs per GPU (default: the config's DATA.BATCH_SIZE)")
    ap.add_argument("--config", default="zeng-bihome")
    ap.add_argument("--precision", default="f32", choices=["f32", "f32x3", "f32-mfma", "bf16", "f32x2", "f16x2"],
                    help="conv operand precision; the headline config (BASELINE.json configs[1]) is f32")
    ap.add_argument("--gpu-datagen", action="store_true",
                    help="draw a fresh batch every step with the device-side pair generator (bh_synth_pairs) inside the "
                         "timed region, instead of reusing one resident batch")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-alt", action="store_true", help="skip the exact-arithmetic (f32x3) timing leg that rides along with the f32 headline")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--autograd-single-thread", action="store_true",
                    help="experiments: run autograd's backward on the calling thread (torch.autograd.set_multithreading_enabled(False)) - "
                         "with --host-profile cProfile then sees the backward functions")
    ap.add_argument("--overlap", action="store_true", help="(default since round 4; kept for old command lines)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="one HIP stream: no weight-gradient side stream, no extractor prefetch under the backbone (the roofline leg "
                         "always runs this way, so that per-kernel durations are those of each kernel alone)")
    ap.add_argument("--host-profile", action="store_true", help="print the host-side enqueue time per step and a cProfile of five steps to stderr")
    ap.add_argument("--graph", action="store_true",
                    help="capture the whole training step in a HIP graph (bihome_amd.graph.GraphedStep) and time replays")
    ap.add_argument("--hook", action="append", default=[], metavar="A,B",
                    help="tuning experiments: call bh_debug_force_tile(A, B) before the run (see csrc/conv_gemm.hip)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the secondary legs: eval, roofline + measured peaks (--no-roofline), the f32x3 "
                         "step time (--no-alt), the CPU baseline (--no-cpu-baseline) and, at N>1, the exchange diagnostics")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (rank 0): loss, delta_gt, delta_hat, and a fixed "
                         "seeded sample of the updated parameters and of the floating-point buffers (BatchNorm running statistics)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def seeded_state(model, opt):
    """Returns restore(): puts the weights and the BatchNorm running statistics back to what they are now (the seeded initial state) and
    the optimizer to a fresh state (Adam moments and step count zero, as before its first step).  A step taken from there computes (on
    the resident batch, with the DSAC indices of the seeded generator) a function of the arguments alone, up to rounding.  Chained steps do
    not: the fp32 atomics sum in a different order from run to run, and training amplifies those last-bit differences to percents of the
    loss within a few steps.  main() restores before the timed steps and before the last of them, whose outputs --dump-outputs writes;
    a restore before every step would add its copy of the weights and moments (~0.07 ms, 0.6 % of a step) to each."""
    params = list(model.parameters())
    bufs = [b for b in model.buffers() if b.is_floating_point()]
    saved = [t.detach().clone() for t in params + bufs]

    def restore():
        with torch.no_grad():
            torch._foreach_copy_([p.data for p in params] + bufs, saved)
            state = [v for st in opt.state.values() for v in st.values() if torch.is_tensor(v)]
            if state:
                torch._foreach_zero_(state)
    return restore


DUMP_SAMPLE = 1 << 22          # elements kept of a larger parameter / buffer vector (16 MB each as float32)


def dump_outputs(outdir, model, loss, delta_gt, delta_hat):
    """The arrays a caller of the timed step receives - its return values and the model state it updated - as float32 .npy files.
    Parameters and buffers are concatenated in name order; above DUMP_SAMPLE elements, a fixed sample (seed 0, sorted indices) is kept."""
    os.makedirs(outdir, exist_ok=True)

    def flat(named):
        ts = [t.detach().reshape(-1).float() for _, t in sorted(named, key=lambda kv: kv[0]) if t.is_floating_point()]
        v = torch.cat(ts) if ts else torch.zeros(0, device=loss.device)
        if v.numel() > DUMP_SAMPLE:
            idx = torch.randperm(v.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_SAMPLE].sort().values
            v = v[idx.to(v.device)]
        return v

    arrays = {"loss": loss, "delta_gt": delta_gt, "delta_hat": delta_hat,
              "params_sample": flat(model.named_parameters()), "buffers_sample": flat(model.named_buffers())}
    for name, t in arrays.items():
        np.save(os.path.join(outdir, name + ".npy"), t.detach().float().cpu().numpy())


def cpu_baseline(cfg, seed=42, batch=8, steps=20, warmup=1):
    """The oracle (plain PyTorch-CPU restatement of the same modules, oracle/bihome_oracle.py) timed on this
    box's host cores: a bounded sample (bs=8, `steps` full train steps, ~10 s of CPU work, capped at 40 s) of the same
    workload."""
    from bihome_amd import synth
    from bihome_amd.weights import load_synthetic
    from oracle import bihome_oracle as O
    # threads actually used: PyTorch-CPU conv/BN stop scaling (and collapse under OpenMP oversubscription) well
    # before the 100+ hardware threads of a GPU host, so the baseline runs on a bounded pool and says so
    cores = min(os.cpu_count() or 1, int(os.environ.get("BIHOME_CPU_THREADS", "16")))
    torch.set_num_threads(cores)
    bb, head = O.build(cfg)
    load_synthetic(bb, 0)
    if hasattr(head, "auxiliary_resnet"):
        load_synthetic(head.auxiliary_resnet, 0)
    opt, sched = O.make_optimizer(torch.nn.Sequential(bb, head), cfg["SOLVER"])
    d = synth.make_pairs(batch, seed=seed, target=True)
    name = cfg["SOLVER"]["LOSS"]
    loss_fn = getattr(torch.nn, name)() if hasattr(torch.nn, name) else None     # supervised "-orig" configs
    times, budget_s, t_begin = [], 40.0, time.perf_counter()
    for it in range(warmup + steps):
        data = {k: torch.tensor(d[k]) for k in ("patch_1", "patch_2", "delta", "target")}
        t0 = time.perf_counter()
        O.train_step(bb, head, opt, sched, data, loss_fn=loss_fn)
        times.append(time.perf_counter() - t0)
        if time.perf_counter() - t_begin > budget_s and len(times) > warmup:      # bounded sample
            break
    steps = len(times) - warmup
    t = float(np.median(times[warmup:]))
    return {"value": batch / t, "unit": "image-pairs/s", "cores": cores, "kind": "port",
            "sample": "oracle (PyTorch-CPU restatement) full train step, bs=%d, median of %d steps after %d warm-up, "
                      "%.2f s/step" % (batch, steps, warmup, t)}


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the newest committed PMC summary (profiles/*pmc_traffic.json, made by
    tools/pmc_summary.py from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command, with the
    gfx950 FETCH_SIZE x2 correction).  PMC counters cannot be read from inside the process, so this is the recorded
    value of the profiled build, or None when no summary matches."""
    import glob
    key = kernel.replace(" ", "")
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_traffic.json")), reverse=True):
        try:
            ks = json.load(open(path))["kernels"]
        except Exception:
            continue
        if "+" in key and all(p in ks for p in key.split("+")):        # an entry of several launches (e.g. kernel + its reduce pass)
            return sum(ks[p]["traffic_bytes_per_launch"] for p in key.split("+")), os.path.relpath(path, ROOT)
        if key in ks:
            return ks[key]["traffic_bytes_per_launch"], os.path.relpath(path, ROOT)
    return None, None


def warp_adjoint_fold_cost(B2, size, pool=4, rounds=4, n=40):
    """Per-launch time of bh_stem7_dgrad_c1 and of bh_stem7_dgrad_c1_warp (the same dgrad with the warp's adjoint applied to the gradient
    it makes) on B2 images of size x size, buffer sets rotating beyond the Infinity Cache; returns the best round of each and the difference."""
    import ctypes
    from bihome_amd import kernels as K
    from bihome_amd._lib import check, lib
    nset = 6
    H64, _ = K.h4pt_fwd((torch.rand(B2, 4, 2, device="cuda") - 0.5) * (size / 4.0), size)
    src = [torch.randn(B2, 1, size, size, device="cuda") for _ in range(nset)]
    gy = [torch.randn(B2, size // 2, size // 2, 64, device="cuda") for _ in range(nset)]
    gcov = [torch.randn(B2, size // pool, size // pool, device="cuda") for _ in range(nset)]
    w = torch.randn(64, 7, 7, 1, device="cuda") * 0.05
    gx = torch.empty(B2, size, size, 1, device="cuda")
    gH = torch.zeros(B2, 9, dtype=torch.float64, device="cuda")
    d = K.conv_desc(B2, size, size, 1, 64, 7, 2, 3, precision=4)      # (the step's arithmetic: the fp16-piece window GEMM)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def plain(i):
        check(lib.bh_stem7_dgrad_c1(p(gy[i]), p(w), p(gx), ctypes.byref(d), st), "bh_stem7_dgrad_c1")

    def fused(i):
        check(lib.bh_stem7_dgrad_c1_warp(p(gy[i]), p(w), None, ctypes.byref(d), p(src[i]), p(H64), p(gcov[i]), pool, p(gH), st), "bh_stem7_dgrad_c1_warp")

    def run(fn):
        for i in range(nset):
            fn(i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            fn(i % nset)
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / n
    tp, tf = [], []
    for _ in range(rounds):
        tp.append(run(plain)); tf.append(run(fused))
    return {"plain_stem_dgrad_us": round(min(tp), 2), "with_warp_adjoint_us": round(min(tf), 2), "added_us": round(max(min(tf) - min(tp), 0.0), 2),
            "rounds": rounds, "launches_per_round": n}


def warp_forward_fold_cost(B2, size, rounds=4, n=40):
    """Per-launch time of the one-plane fp16-piece stem forward on a resident image (bh_conv_fwd_bnstats) and of bh_stem7_fwd_warp (the same
    stem making the warped pixels and the pooled coverage on the way, as the step calls it: the warped image is not written) on B2 images of size x size, buffer sets rotating
    beyond the Infinity Cache; returns the best round of each and the difference."""
    import ctypes
    from bihome_amd import kernels as K
    from bihome_amd._lib import check, lib
    nset = 6
    H64, _ = K.h4pt_fwd((torch.rand(B2, 4, 2, device="cuda") - 0.5) * (size / 4.0), size)
    src = [torch.randn(B2, 1, size, size, device="cuda") for _ in range(nset)]
    y = [torch.empty(B2, size // 2, size // 2, 64, device="cuda") for _ in range(nset)]
    cov = torch.empty(B2, size // 4, size // 4, device="cuda")
    sums = K.bn_stats_buffer(2, 64, "cuda")
    w = torch.randn(64, 7, 7, 1, device="cuda") * 0.05
    d = K.conv_desc(B2, size, size, 1, 64, 7, 2, 3, precision=4)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def plain(i):
        check(lib.bh_conv_fwd_bnstats(p(src[i]), p(w), None, p(y[i]), ctypes.byref(d), p(sums), 2, st), "bh_conv_fwd_bnstats")

    def fused(i):
        check(lib.bh_stem7_fwd_warp(p(src[i]), p(H64), 4, p(w), None, p(y[i]), ctypes.byref(d), None, p(cov), p(sums), 2, st), "bh_stem7_fwd_warp")

    def run(fn):
        for i in range(nset):
            fn(i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            fn(i % nset)
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / n
    tp, tf = [], []
    for _ in range(rounds):
        tp.append(run(plain)); tf.append(run(fused))
    return {"plain_stem_fwd_us": round(min(tp), 2), "with_warp_us": round(min(tf), 2), "added_us": round(max(min(tf) - min(tp), 0.0), 2),
            "rounds": rounds, "launches_per_round": n}


def roofline_leg(model, data, opt, sched, reducer, nsteps=2):
    """Per-launch HIP-event timing (events recorded on the launch stream) of every conv/BN launch for a few
    extra steps; returns the roofline object of the kernel with the largest total time plus a breakdown."""
    from bihome_amd import kernels as K, net
    from bihome_amd.step import train_step
    # per-kernel timing wants each kernel alone on the GPU: the side stream (weight gradients, feature prefetch) is off for this leg
    net.set_stream_overlap(False, model)
    # one untimed pass in timing mode first: the first event pairs / variant queries of a process stall the host for
    # milliseconds, and an event pair also measures the time the GPU waits for the host between its two markers
    K.TIMING = {}
    train_step(model, dict(data), opt, sched, reducer=reducer, loss_fn=LOSS_FN[0])
    torch.cuda.synchronize()
    K.TIMING = {}
    # an event pair also measures the time the GPU waits for the HOST between its two markers, and the instrumented pass (two event records
    # per launch) is host-bound on boxes with a slow host: ~20 ms of device work is queued in front of every instrumented step, so that the
    # host runs ahead of the GPU and the pairs measure the device (round 4: hbm_path_frac.raw moved 0.31 -> 0.21 between two boxes without it)
    lead = torch.empty(1 << 28, dtype=torch.float32, device=next(model.parameters()).device)
    for _ in range(nsteps):
        for _ in range(50):
            lead.add_(1.0)
        train_step(model, dict(data), opt, sched, reducer=reducer, loss_fn=LOSS_FN[0])
    torch.cuda.synchronize()
    del lead
    rows = []
    for name, r in K.TIMING.items():
        ms = sum(a.elapsed_time(b) for a, b in r["events"])
        rows.append({"kernel": name, "launches_per_step": r["n"] // nsteps, "ms_per_step": ms / nsteps,
                     "avg_us": 1e3 * ms / max(r["n"], 1), "tflops": r["flops"] / (ms * 1e-3) / 1e12 if ms > 0 else 0.0,
                     "gbs": r["bytes"] / (ms * 1e-3) / 1e9 if ms > 0 else 0.0,
                     "flops_per_launch": r["flops"] / max(r["n"], 1), "bytes_per_launch": r["bytes"] / max(r["n"], 1)})
    K.TIMING = None
    net.set_stream_overlap(os.environ.get("BIHOME_OVERLAP", "1") != "0", model)
    rows.sort(key=lambda r: -r["ms_per_step"])
    # the roofline object describes ONE kernel instantiation: rows that time a C-ABI call of several launches ("bn_bwd(3 kernels)",
    # "tail_bwd(5 kernels)": reduce + finalize + apply of different shapes under one key) stay in the breakdown but are not `top`
    single = [r for r in rows if "kernels)" not in r["kernel"] or "(1 kernels)" in r["kernel"]]
    top = single[0] if single else rows[0]
    traffic, traffic_src = pmc_traffic(top["kernel"])
    # BASELINE.json's HBM-bound part: homography warp + perceptual-feature L1 / triplet reduction (SURVEY.md 8(d) bytes)
    hp = [r for r in rows if r["kernel"] in ("warp_fwd_kernel", "warp_bwd_kernel", "triplet_fwd_kernel", "triplet_bwd_kernel")]
    hbm_path = None
    fold = ffold = None
    names = {r["kernel"] for r in rows}
    B2_, size_ = data["patch_1"].shape[0] * 2, data["patch_1"].shape[-1]
    warp_bytes = 4.0 * (2 * B2_ * size_ * size_ + B2_ * (size_ // 4) ** 2)      # 8 B / pixel + the pooled coverage, each direction
    if hp and "stem7_fwd_f16_kernel<1,true>" in names and "warp_fwd_kernel" not in names:
        # round 6: the warp runs INSIDE the extractor stem's forward (bh_stem7_fwd_warp) - there is no warp_fwd launch to time.  Its cost is
        # what it adds to that launch: the fused and the plain stem forward timed back to back on buffers of the step's shape
        ffold = warp_forward_fold_cost(B2_, size_)
        hp = hp + [{"kernel": "warp_fwd (folded into stem7_fwd_f16_kernel<1,true>: its launch time over the plain stem forward's)",
                    "launches_per_step": 0, "ms_per_step": 1e-3 * ffold["added_us"], "avg_us": ffold["added_us"],
                    "gbs": warp_bytes / (max(ffold["added_us"], 1e-3) * 1e-6) / 1e9, "bytes_per_launch": warp_bytes, "bytes_total": warp_bytes}]
    if hp and "stem7_dgrad_c1_kernel<true>" in names and "warp_bwd_kernel" not in names:
        # round 6: the warp's adjoint runs INSIDE the extractor stem's dgrad (bh_stem7_dgrad_c1_warp) - there is no warp_bwd launch to time.
        # Its cost is what it adds to that launch: the fused and the plain stem dgrad timed back to back on buffers of the step's shape
        # (alternating rounds, per-launch time from one event pair around each round); its bytes stay SURVEY 8(d)'s (image + gradient read).
        fold = warp_adjoint_fold_cost(B2_, size_)
        hp = hp + [{"kernel": "warp_bwd (folded into stem7_dgrad_c1_kernel<true>: its launch time over the plain stem dgrad's)",
                    "launches_per_step": 0, "ms_per_step": 1e-3 * fold["added_us"], "avg_us": fold["added_us"],
                    "gbs": warp_bytes / (max(fold["added_us"], 1e-3) * 1e-6) / 1e9, "bytes_per_launch": warp_bytes, "bytes_total": warp_bytes}]
    if hp:
        # these launches take 12-20 us, so the cost of the event pair itself matters: time empty pairs on the same stream
        # (median) and report the path both as recorded and net of that; profiles/*kernel_stats.csv holds rocprofv3's
        # per-kernel durations of the same launches for comparison
        pairs = []
        for _ in range(65):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); b.record(); pairs.append((a, b))
        torch.cuda.synchronize()
        ovh_us = sorted(1e3 * a.elapsed_time(b) for a, b in pairs[1:])[32]
        ms_ = sum(r["ms_per_step"] for r in hp)
        nl_ = sum(r["launches_per_step"] for r in hp)
        net_ = max(ms_ - 1e-3 * ovh_us * nl_, 1e-6)
        by_ = sum(r.get("bytes_total", r["bytes_per_launch"] * r["launches_per_step"]) for r in hp)
        hbm_path = {"kernels": {r["kernel"]: {"us": round(r["avg_us"], 1), "GB/s": round(r["gbs"], 1)} for r in hp},
                    "algorithmic_bytes_per_step": by_, "ms_per_step": round(ms_, 4), "achieved_GBs": round(by_ / (ms_ * 1e-3) / 1e9, 1),
                    "frac_of_hbm_peak": round(by_ / (ms_ * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                    "warp_adjoint_fold": fold, "warp_forward_fold": ffold,
                    "empty_event_pair_us": round(ovh_us, 2), "ms_per_step_net_of_event_pairs": round(net_, 4),
                    "frac_of_hbm_peak_net_of_event_pairs": round(by_ / (net_ * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
    # the same launches grouped by kernel template (all instantiations of one __global__ function)
    fam = {}
    for r in rows:
        f = fam.setdefault(r["kernel"].split("<")[0].split("(")[0], {"ms_per_step": 0.0, "flops": 0.0, "launches_per_step": 0})
        f["ms_per_step"] += r["ms_per_step"]
        f["flops"] += r["flops_per_launch"] * r["launches_per_step"]
        f["launches_per_step"] += r["launches_per_step"]
    families = [{"kernel": k, "launches_per_step": v["launches_per_step"], "ms_per_step": round(v["ms_per_step"], 3),
                 "tflops": round(v["flops"] / (v["ms_per_step"] * 1e-3) / 1e12, 2) if v["ms_per_step"] > 0 else 0.0,
                 "frac_of_f32_mfma_peak": round(v["flops"] / (v["ms_per_step"] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
                 if v["ms_per_step"] > 0 else 0.0}
                for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms_per_step"])[:4]]
    if top["tflops"] > 0 and x3_pieces(top["kernel"]):
        # fp32 products evaluated as six (f32x2: three) bf16 MFMA products: the roofline is the bf16 matrix pipe, `achieved` counts
        # the MFMA flops the launch executes (6 x algorithmic); fp32_equivalent_* relate the algorithmic flops to the fp32-input MFMA
        nprod = X3_PRODUCTS[x3_pieces(top["kernel"])]
        ex = nprod * top["tflops"]
        roof = {"kernel": top["kernel"], "bound": "mfma", "achieved": ex, "peak": PEAK_BF16_MFMA_TFLOPS,
                "unit": "TFLOP/s", "frac": ex / PEAK_BF16_MFMA_TFLOPS, "traffic": traffic,
                "mfma": ("v_mfma_f32_32x32x16_f16, %d products per fp32 product (operands times a power-of-two scale per tensor as %d fp16 pieces)"
                         if x3_is_f16(top["kernel"]) else
                         "v_mfma_f32_32x32x16_bf16, %d products per fp32 product (operands cut into %d bf16 pieces)")
                        % (nprod, x3_pieces(top["kernel"])),
                "algorithmic_tflops": top["tflops"], "fp32_equivalent_frac_of_f32_mfma_peak": top["tflops"] / PEAK_F32_MFMA_TFLOPS,
                "traffic_source": traffic_src, "algorithmic_bytes_per_launch": top["bytes_per_launch"],
                "avg_launch_us": top["avg_us"], "flops_per_launch": top["flops_per_launch"],
                "launches_per_step": top["launches_per_step"], "by_kernel_template": families,
                "warp_perceptual_path": hbm_path}
        # a launch with epilogue operands (dgrad + BatchNorm-backward sums + accumulate: five tensor passes) can sit closer to the HBM roof than
        # to the matrix pipe's: the object names the roof that bounds it and keeps the other fraction next to it
        hbm_frac = top["gbs"] / PEAK_HBM_GBS
        roof["mfma_frac"] = ex / PEAK_BF16_MFMA_TFLOPS
        roof["hbm_frac"] = hbm_frac
        if hbm_frac > roof["mfma_frac"]:
            roof.update({"bound": "hbm", "achieved": top["gbs"], "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": hbm_frac,
                         "mfma_executed_tflops": ex})
        # round-5 VERDICT: a kernel whose two fractions are both below 0.5 and within 5 % of each other is bound by NEITHER roof (latency,
        # and the matrix pipe's power-limited clock on toggling operands: DESIGN.md 5.0); `achieved` / `peak` / `frac` stay those of the nearer one
        if max(hbm_frac, roof["mfma_frac"]) < 0.5 and abs(hbm_frac - roof["mfma_frac"]) <= 0.05 * max(hbm_frac, roof["mfma_frac"]):
            roof["nearest_roof"] = roof["bound"]
            roof["bound"] = "neither"
    elif top["tflops"] > 0:
        roof = {"kernel": top["kernel"], "bound": "mfma", "achieved": top["tflops"], "peak": PEAK_F32_MFMA_TFLOPS,
                "unit": "TFLOP/s", "frac": top["tflops"] / PEAK_F32_MFMA_TFLOPS, "traffic": traffic,
                "traffic_source": traffic_src, "algorithmic_bytes_per_launch": top["bytes_per_launch"],
                "avg_launch_us": top["avg_us"], "flops_per_launch": top["flops_per_launch"],
                "launches_per_step": top["launches_per_step"], "by_kernel_template": families,
                "warp_perceptual_path": hbm_path}
    else:
        roof = {"kernel": top["kernel"], "bound": "hbm", "achieved": top["gbs"], "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": top["gbs"] / PEAK_HBM_GBS, "traffic": traffic, "traffic_source": traffic_src, "avg_launch_us": top["avg_us"],
                "bytes_per_launch": top["bytes_per_launch"], "launches_per_step": top["launches_per_step"]}
    return roof, rows


def measured_peaks():
    """the peaks this chip SUSTAINS, measured in the same run - a bare bf16 MFMA stream with constant and with random-bit
    operands (bh_probe_mfma_bf16: real tensors toggle the operand lines; the pipe is power-limited then) and a device-to-device copy."""
    import ctypes
    from bihome_amd._lib import check, lib
    sink = torch.zeros(1, device="cuda")
    out = {}
    for name, rnd in (("bf16_mfma_constant_operands_TFLOPs", 0), ("bf16_mfma_random_operands_TFLOPs", 1)):
        v = ctypes.c_double(0.0)
        check(lib.bh_probe_mfma_bf16(rnd, ctypes.c_void_p(sink.data_ptr()), ctypes.byref(v),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "bh_probe_mfma_bf16")
        out[name] = round(v.value, 1)
    for name, rnd in (("f32_mfma_constant_operands_TFLOPs", 0), ("f32_mfma_random_operands_TFLOPs", 1)):      # (the generic / stem kernels' instruction)
        v = ctypes.c_double(0.0)
        check(lib.bh_probe_mfma_f32(rnd, ctypes.c_void_p(sink.data_ptr()), ctypes.byref(v),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "bh_probe_mfma_f32")
        out[name] = round(v.value, 1)
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")          # 1 GiB read + 1 GiB written: beyond the Infinity Cache
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    out["hbm_copy_GBs"] = round(4 * 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
    return out


LOSS_FN = ["biHomE"]           # the loss of the running config (roofline_leg re-runs train steps)

WORKLOADS = {
    "zeng-orig": "config/s-coco/zeng-orig (supervised SmoothL1 on the perspective field, OneLine Zeng backbone)",
    "detone-orig": "config/s-coco/detone-orig (supervised MSE on the 4-point offsets, ResNet-34 regressor)",
    "zeng-bihome": "BASELINE.json configs[1]: s-coco Zeng (Rethinking/ResNet34 blocks)",
    "zeng-bihome-pds": "BASELINE.json configs[2]: pds-coco Zeng (photometric-distorted)",
    "detone-bihome": "BASELINE.json configs[3]: s-coco ResNet-34 regressor",
    "zeng-bihome-rgb256": "BASELINE.json configs[4]: 256x256 RGB Zeng (build-side extension)",
    "zhang-orig": "config/s-coco/zhang-orig (Zhang content-aware baseline: ContentAware backbone + TripletHead)",
    "zhang-bihome": "config/s-coco/zhang-bihome (ContentAware backbone under the biHomE PerceptualHead)",
}


def spawn_ranks(args):
    """`python bench.py --gpus N` (N > 1) without a launcher: start `python -m torch.distributed.run --nproc-per-node N
    bench.py <same flags>` as a CHILD process - this process has made no GPU call yet (a process that has initialised the GPU
    is never replaced or re-executed) - relay its output (rank 0's JSON line) and exit with its code.  A box with fewer than
    N GPUs fails here, loudly, instead of reporting a one-rank number as an N-GPU one."""
    import socket
    import subprocess
    ndev = torch.cuda.device_count()                   # (counting devices does not initialise the GPU on this image)
    gloo_dev = os.environ.get("BIHOME_DIST_BACKEND", "nccl") != "nccl"      # dev only: ranks may share a GPU over gloo
    if ndev < args.gpus and not gloo_dev:
        raise SystemExit("bench.py: --gpus %d but this node exposes %d GPU(s): refusing to report fewer ranks as %d "
                         "(RCCL needs one device per rank)" % (args.gpus, ndev, args.gpus))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: --gpus %d without a launcher: spawning %s" % (args.gpus, " ".join(cmd[1:9])), file=sys.stderr, flush=True)
    r = subprocess.run(cmd, env=env)
    raise SystemExit(r.returncode)


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)                              # never returns
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with --nproc-per-node %d, or without a launcher)"
                         % (args.gpus, world, args.gpus))
    ndev = torch.cuda.device_count()
    backend = os.environ.get("BIHOME_DIST_BACKEND", "nccl")           # "nccl" IS RCCL on ROCm
    if world > 1 and backend == "nccl" and ndev < world:
        raise SystemExit("bench.py: %d ranks but %d GPU(s) visible: RCCL needs one device per rank" % (world, ndev))
    local = local % max(ndev, 1)          # (dev only: several ranks may share one GPU with BIHOME_DIST_BACKEND=gloo)
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # CU budget of the exchange: 42.3 MB per 12 ms step is ~6 GB/s per GPU on a ring - a fraction of ONE xGMI link - while every RCCL
        # channel is a persistent workgroup that holds a CU which the step's 256-workgroup persistent conv kernels (one per CU, 158.5 KB
        # of LDS: nothing co-resides) then have to queue for.  Eight channels are plenty and cost eight CUs (a guess without a node to measure on); the caller's setting wins.
        os.environ.setdefault("NCCL_MAX_NCHANNELS", "8")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        if dist.get_world_size() != args.gpus:
            raise SystemExit("bench.py: process group has %d ranks, --gpus %d" % (dist.get_world_size(), args.gpus))
        # every rank proves it is there: one all-reduce of ones over the data-path backend must count N
        ones = torch.ones(1, device="cuda")
        dist.all_reduce(ones)
        torch.cuda.synchronize()
        if int(ones.item()) != world:
            raise SystemExit("bench.py: all-reduce counted %d ranks, expected %d" % (int(ones.item()), world))
        if rank == 0:
            ver = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else "-"
            print("bench.py: process group up: backend=%s (RCCL %s) world_size=%d, all-reduce counted %d ranks, devices/node=%d"
                  % (backend, ver, world, int(ones.item()), ndev), file=sys.stderr, flush=True)

    from bihome_amd import configs, synth
    from bihome_amd.step import attach_reducer, build_model, build_optimizer, mace, train_step
    from bihome_amd.weights import load_synthetic

    if args.no_overlap:
        os.environ["BIHOME_OVERLAP"] = "0"
    if args.hook:
        from bihome_amd._lib import TUNING, lib
        if not TUNING:
            raise SystemExit("--hook needs the -DBH_TUNING library: `make -C bihome_amd/csrc tuning` and BIHOME_TUNING=1 "
                             "(the product library has no process-global tuning state)")
        for h in args.hook:
            a_, b_ = (int(v) for v in h.split(","))
            lib.bh_debug_force_tile(a_, b_)
    if args.autograd_single_thread:
        torch.autograd.set_multithreading_enabled(False)
    cfg = configs.get(args.config)
    cfg["MODEL"]["BACKBONE"]["PRECISION"] = args.precision
    cfg["MODEL"]["HEAD"]["PRECISION"] = args.precision
    model = build_model(cfg, "cuda")
    load_synthetic(model[0], 0)                       # identical replicas on every rank
    if hasattr(model[1], "auxiliary_resnet"):
        load_synthetic(model[1].auxiliary_resnet, 0)
    use_graph = args.graph and world == 1 and not args.gpu_datagen
    opt, sched = build_optimizer(model, cfg["SOLVER"], capturable=use_graph)
    reducer = attach_reducer(model) if world > 1 else None
    restore = seeded_state(model, opt)

    B = args.batch or cfg["DATA"]["BATCH_SIZE"]
    # each rank owns its contiguous shard of the global batch; synthetic data generated on the host
    # from seeds, then resident in HBM for the whole run
    D = cfg["DATA"]
    P, CH = D["PATCH_SIZE"], D.get("PATCH_CHANNELS", 1)
    KEYS = ("patch_1", "patch_2", "delta", "target", "corners")
    d = synth.make_pairs(B, patch=P, rho=D["RHO"], seed=42 + rank, photometric_max_delta=D["PHOTOMETRIC_MAX_DELTA"],
                         channels=CH, target=CH == 1)
    data = {k: torch.tensor(d[k]).cuda() for k in KEYS if k in d}
    from bihome_amd.step import build_loss
    loss_fn = build_loss(cfg["SOLVER"])
    LOSS_FN[0] = loss_fn
    torch.manual_seed(1234 + rank)                    # DSAC sample indices: per-rank stream

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    gen = None
    if args.gpu_datagen:
        from bihome_amd.synth_gpu import GpuPairGenerator
        gen = GpuPairGenerator(n_images=16, seed=42 + rank, photometric_max_delta=cfg["DATA"]["PHOTOMETRIC_MAX_DELTA"])

    def batch():
        return gen.next(B) if gen is not None else dict(data)

    if use_graph:
        from bihome_amd.graph import GraphedStep
        gs = GraphedStep(model, opt, sched, dict(data), loss_fn=loss_fn, warmup=3)

        def one_step():
            return gs(batch())
    else:
        def one_step():
            return train_step(model, batch(), opt, sched, reducer=reducer, loss_fn=loss_fn)
    # (BIHOME_MAIN_PRIORITY: experiments - run the steps on a stream of this priority instead of the default stream; -1 = high)
    _prio = os.environ.get("BIHOME_MAIN_PRIORITY")
    if _prio:
        sync()
        _main = torch.cuda.Stream(priority=int(_prio))
        torch.cuda.set_stream(_main)
    for _ in range(args.warmup):
        loss, dgt, dh = one_step()
    restore()                                         # (outside the timed region: its first launches load their kernels)
    sync()
    # (one event per step on the launch stream: no host synchronisation inside the timed region; the gaps between consecutive
    #  events are the per-step times the percentiles below come from)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        if i == args.steps - 1:
            restore()                                 # the step whose outputs --dump-outputs writes: from the seeded state
        loss, dgt, dh = one_step()
        marks[i + 1].record()
    sync()
    dt = time.perf_counter() - t0
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    pct = lambda q: round(step_ms[min(len(step_ms) - 1, int(q * len(step_ms)))], 4)
    if dist is not None:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    ms = 1e3 * dt / args.steps
    value = world * B * args.steps / dt
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, loss, dgt, dh)
    if args.host_profile and rank == 0:
        # host side of the step (tools/: where does Python spend the launch time?): enqueue time per step against the device time, then cProfile
        import cProfile, pstats
        sync()
        th = []
        for _ in range(10):
            t1 = time.perf_counter(); one_step(); th.append(time.perf_counter() - t1)
        sync()
        print("host enqueue ms per step: %s (device: %.2f)" % (" ".join("%.2f" % (1e3 * v) for v in th), ms), file=sys.stderr)
        pr = cProfile.Profile()
        pr.enable()
        for _ in range(5):
            one_step()
        pr.disable()
        sync()
        pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(45)
    final_loss, final_mace = float(loss.item()), mace(dgt, dh)

    # inference leg (eval.py:80-112): eval-mode forward + DLT on fresh batches, BatchNorms folded into the convs
    eval_info = None
    if args.full:
        from bihome_amd.step import evaluate
        ev = [{k: torch.tensor(v).cuda() for k, v in synth.make_pairs(B, patch=P, rho=D["RHO"], seed=1000 + rank + 7 * i,
                                                                       channels=CH, target=CH == 1).items() if k in KEYS}
              for i in range(2)]
        eval_mace, eval_ms = evaluate(model, [ev[i % 2] for i in range(6)])
        eval_info = {"mace": eval_mace, "ms_per_batch": eval_ms, "pairs_per_s_per_gpu": 1e3 * B / eval_ms,
                     "note": "predict_homography in eval mode (BatchNorm folded), held-out synthetic pairs, random-init "
                             "weights after the timed steps"}

    roof, rows = (None, None)
    if args.full and not args.no_roofline:
        roof, rows = roofline_leg(model, data, opt, sched, reducer)
        if dist is not None:
            dist.barrier()                 # the probe below (2 GiB, synchronising) runs on rank 0 only: keep the ranks together around it
        if rank == 0:
            mp = measured_peaks()
            roof["measured_peaks"] = mp
            # `frac` is against the vendor peak (the contract); this is the same `achieved` against what the chip sustains
            sustained = mp["bf16_mfma_random_operands_TFLOPs"] if (roof.get("unit") == "TFLOP/s" and roof.get("peak") == PEAK_BF16_MFMA_TFLOPS) \
                else (mp["hbm_copy_GBs"] if roof.get("unit") == "GB/s" else None)
            # (None for rooflines bound by the fp32-input MFMA pipe - `--precision f32-mfma`, the zhang / detone tops: only the bf16 / fp16 pipe
            #  and an HBM copy are probed)
            roof["frac_of_measured_peak"] = (roof["achieved"] / sustained) if sustained else None
        if dist is not None:
            dist.barrier()
    dist_info = None
    if args.full and dist is not None:
        # The N-GPU line proves itself (round-4 VERDICT item 8): backend and RCCL version, ranks counted by an all-reduce, the buckets, the
        # exchange alone (event-timed around the bucket sequence: launch -> Work.wait() puts the RCCL stream's completion on the timed
        # stream) and the SAME ranks stepping WITHOUT the exchange in the same run - what each replica costs alone, warm, on this node.
        reds = reducer.reducers if hasattr(reducer, "reducers") else [reducer]
        nref = max(5, min(args.steps, 20))
        for r in reds:
            r.enabled = False
        for _ in range(3):
            one_step()
        sync()
        t1 = time.perf_counter()
        for _ in range(nref):
            one_step()
        sync()
        tref = torch.tensor([time.perf_counter() - t1], device="cuda", dtype=torch.float64)
        dist.all_reduce(tref, op=dist.ReduceOp.MAX)
        ms_alone = 1e3 * tref.item() / nref
        for r in reds:
            r.enabled = True
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        payload = sum((hi - lo) * 4 for r in reds for (lo, hi) in r.buckets)
        nrep = 5
        sync()
        e0.record()
        for _ in range(nrep):
            works = [dist.all_reduce(r.fg.flat[lo:hi], async_op=True) for r in reds for (lo, hi) in r.buckets]
            for w in works:
                w.wait()
        e1.record()
        torch.cuda.synchronize()
        tar = torch.tensor([e0.elapsed_time(e1) / nrep], device="cuda", dtype=torch.float64)
        dist.all_reduce(tar, op=dist.ReduceOp.MAX)
        dist_info = {"backend": backend, "rccl_version": (".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None),
                     "world_size": world, "ranks_counted": int(ones.item()), "devices_per_node": ndev,
                     "buckets": sum(len(r.buckets) for r in reds), "payload_bytes_per_step": payload, "reduce_op": "SUM",
                     "rccl_max_nchannels": os.environ.get("NCCL_MAX_NCHANNELS"),
                     "exchange_launch": "each bucket behind the weight-gradient stream (event from the main stream, no wait on it); one join "
                                        "in front of the optimizer",
                     "allreduce_ms_per_step": tar.item(),
                     "allreduce_note": "the step's bucket sequence alone (nothing to overlap with), max over ranks; inside a step the buckets "
                                       "leave from the backward hooks and run under the remaining backward kernels",
                     "same_run_ms_per_step_without_exchange": ms_alone, "same_run_reference_steps": nref,
                     "exchange_overhead_ms_per_step": ms - ms_alone,
                     "scaling_efficiency": ms_alone / ms,
                     "scaling_efficiency_note": "ms/step of these ranks stepping WITHOUT the exchange (each replica alone, warm, same run) / "
                                                "ms/step with it; weak scaling, so value = n_gpus x pairs per GPU / ms"}
    # The headline's 'f32' is the fp16-piece arithmetic (22-bit operands, fp32 accumulate): the SAME run also times the exact form - three
    # bf16 pieces per operand, six products, bit-exact operand cut ('f32x3', the default of rounds 2-3) - on a second model of the same
    # config, so that the --full line carries the exact-arithmetic number next to the headline (round-4 VERDICT item 7).
    alt = None
    if args.full and rank == 0 and world == 1 and args.precision in ("f32", "f16x2") and not args.no_alt and not use_graph:
        import copy
        cfg2 = copy.deepcopy(cfg)
        cfg2["MODEL"]["BACKBONE"]["PRECISION"] = "f32x3"
        cfg2["MODEL"]["HEAD"]["PRECISION"] = "f32x3"
        m2 = build_model(cfg2, "cuda")
        load_synthetic(m2[0], 0)
        if hasattr(m2[1], "auxiliary_resnet"):
            load_synthetic(m2[1].auxiliary_resnet, 0)
        o2, s2 = build_optimizer(m2, cfg2["SOLVER"])
        for _ in range(5):
            l2, _, _ = train_step(m2, dict(data), o2, s2, loss_fn=loss_fn)
        torch.cuda.synchronize()
        n2 = max(10, min(args.steps, 30))
        t2 = time.perf_counter()
        for _ in range(n2):
            l2, _, _ = train_step(m2, dict(data), o2, s2, loss_fn=loss_fn)
        torch.cuda.synchronize()
        ms2 = 1e3 * (time.perf_counter() - t2) / n2
        alt = {"arithmetic": "f32x3 (exact cut of every fp32 operand into three bf16 pieces, six products per product on v_mfma_f32_32x32x16_bf16)",
               "ms_per_step": ms2, "value": B * 1e3 / ms2, "unit": "image-pairs/s", "steps": n2,
               "note": "same config, same resident batch, same run; a second model instance (the timed model is not touched)"}
        del m2, o2, s2
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and CH == 1:    # the reference (and so the oracle) has no RGB path
        cpu = cpu_baseline(cfg)
    if dist is not None:
        dist.barrier()
    if rank == 0:
        out = {
            "metric": "training image-pairs/s (%dx%d patch, bs=%d per GPU, full step: fwd+bwd+Adam)" % (P, P, B),
            "value": value, "unit": "image-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"f32": "f32", "f32x3": "f32", "f16x2": "f32", "f32-mfma": "f32", "bf16": "bf16", "f32x2": "f32x2"}[args.precision],
            "data": "synthetic (seeded COCO-style texture pairs, random-init weights%s)" % (
                "; fresh batch per step from the device-side generator" if args.gpu_datagen else "; one resident batch"),
            "config": {"workload": "%s: %s backbone + %s head, %d pairs/GPU, %dx%d %s, %s MFMA conv + HIP "
                                   "warp/DLT/triplet kernels" % (
                                       WORKLOADS.get(args.config, args.config), cfg["MODEL"]["BACKBONE"]["NAME"],
                                       cfg["MODEL"]["HEAD"]["NAME"], B, P, P,
                                       "RGB" if CH == 3 else "grayscale", args.precision),
                       "arithmetic": {"f32": F16X2_TEXT,
                                      "f32x3": "fp32 tensors, fp32 accumulate; 3x3 / stride-1 convs (fwd, dgrad, wgrad): each fp32 operand cut "
                                               "exactly into 3 bf16 pieces, 6 partial products per product on v_mfma_f32_32x32x16_bf16; all "
                                               "other convs: v_mfma_f32_32x32x2_f32 (the default arithmetic of rounds 2-3)",
                                      "f32-mfma": "fp32 tensors, v_mfma_f32_32x32x2_f32 everywhere",
                                      "bf16": "REDUCED precision (not the headline): fp32 tensors in HBM, conv operands rounded to bf16 on their "
                                              "way to v_mfma_f32_32x32x16_bf16, fp32 accumulate",
                                      "f16x2": F16X2_TEXT,
                                      "f32x2": "REDUCED precision (not the headline): fp32 tensors, fp32 accumulate; 3x3 / stride-1 convs: each "
                                               "operand as two bf16 pieces rounded to nearest (x = hi + mid + e, |e| <= 2^-18 |x|), 3 partial "
                                               "products per product on v_mfma_f32_32x32x16_bf16 (~4e-6 per product); all other convs: "
                                               "v_mfma_f32_32x32x2_f32"}[args.precision],
                       "arithmetic_mode": {"f32": "f16x2"}.get(args.precision, args.precision),
                       "stream_overlap": os.environ.get("BIHOME_OVERLAP", "1") != "0",
                       "hip_graph": bool(use_graph),
                       "global_batch": world * B, "parallelism": "dp%d" % world, "optimizer": "Adam lr 1e-3"},
            "final_loss": final_loss, "final_mace": final_mace,
            "eval": eval_info,
            "step_ms_percentiles": {"p10": pct(0.10), "p50": pct(0.50), "p90": pct(0.90), "min": round(step_ms[0], 4), "max": round(step_ms[-1], 4),
                                    "note": "rank 0, gaps between per-step events on the launch stream"},
            "roofline": roof, "cpu_baseline": cpu, "distributed": dist_info, "alt_arithmetic": alt,
            # (compact copy of roofline.warp_perceptual_path: BASELINE.json's HBM-bound part - homography warp + perceptual L1 / triplet -
            #  as a fraction of the 8 TB/s HBM peak, by raw event pairs and net of the cost of an empty event pair)
            "hbm_path_frac": ({"raw": roof["warp_perceptual_path"]["frac_of_hbm_peak"],
                               "net_of_event_pairs": roof["warp_perceptual_path"]["frac_of_hbm_peak_net_of_event_pairs"]}
                              if roof and roof.get("warp_perceptual_path") else None),
        }
        if rows:
            out["kernel_breakdown"] = [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()
                                        if k in ("kernel", "launches_per_step", "ms_per_step", "avg_us", "tflops", "gbs")}
                                       for r in rows[:12]]
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
