"""The memory axis: what a kernel does with memory it was given but did not fill, and whether it stays inside what it was given.

include/bihome.h states a contract per pointer - "overwritten", "+=", "caller zeroes", "scratch of bh_*_scratch_doubles() / *_ws_bytes()".
The other test files hold every kernel family to a float64 reference; in a fresh process the caching allocator mostly hands those tests
zero pages, so a scratch entry read before it is written, a "caller zeroes" buffer the wrapper made with torch.empty, a partly written
"overwritten" output or a store past a hand-written size formula all pass there.  Here the same cases run again with
tests/poisoned_alloc.py installed as the `torch` of bihome_amd/kernels.py and of the test module that owns the case: every torch.empty is
NaN (floats) / 1 (integers) throughout, every buffer - the helpers' own det_ws, gw, gH and statistics buffers included - has exactly its
requested size with 4096 fill bytes in front and behind.

1. Kernel level (CASES): one case per kernel family, the smallest its own file lists (a smaller one that takes the same kernel, asserted
   through bh_conv_variant by the helper, where the listed ones are full-size), through the family's own helper - same reference, same
   bound -, then verify() (red zones intact), then the wrappers the case claims in COVERED_BY must have allocated under the shim.  Both in
   the default mode and inside K.det_scope(True), except where the helper pins the mode itself, calls conv_wgrad without a workspace
   (which a deterministic call refuses by design) or reads BatchNorm sums in the default layout (the `det` column says which).
2. Step level: two deterministic training steps, plain and poisoned, must agree bit for bit - deterministic sums are order-independent,
   so the only thing that can differ is memory the step read without owning; the second step meets what the first left in the
   long-lived workspaces (Runner._det_ws, kernels._STEM_WGRAD_WS, the pack tables).
3. `+=` outputs: every gradient output the header documents as accumulated starts from a base b ~ U(-max|ref|, max|ref|) and (out - b),
   formed in float64, is held to the float64 reference under the bound of the family's own test (rounding b into the sum costs 2^-23 of
   the result's scale per addition: far inside those bounds).

tests/test_buffer_contracts_cpu.py holds COVERED_BY + EXEMPT against the census of allocating wrappers in kernels.py, and tests the
shim itself."""
import importlib

import numpy as np
import pytest
import torch

import poisoned_alloc

pytestmark = pytest.mark.gpu

CONV = ("conv_fwd", "conv_dgrad")


def _field_chain(RS, K, i):
    """test_ransac_gpu's `field` fixture and the four tests that read it, for R.FIELD_CASES[i]."""
    ref = RS.R.field_case(i)
    out, gpu = RS.call(K, ref["pf"], ref["choice"], ref["thr"])
    f = dict(ref=ref, out=out, gpu=gpu)
    RS.test_counts_at_other_shapes(f)
    RS.test_best_at_other_shapes(f)
    RS.test_mask_at_other_shapes(f)
    RS.test_refit_at_other_shapes(f)


def _dlt(HK, K, n, P):
    from bihome_amd import synth
    HK.check_dlt_fwd_bwd(K, n, P, np.ascontiguousarray(synth.make_head_inputs(6, seed=3, noise=0.7)["pf_hat_12"][:, :, :48, :80]))


def _backbone_64x96(R, K):
    """test_rectangular_gpu.test_backbone_forward_backward_vs_oracle with a model of its own (the module fixture of test_model_gpu is not
    ours to build under the shim: its buffers would outlive the test)."""
    M = R.M
    from bihome_amd.step import build_model
    from bihome_amd.weights import load_synthetic
    cfg = M.configs.get("zeng-bihome")
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    R.test_backbone_forward_backward_vs_oracle(K, (cfg, model))


def _det_default(K, fn, *args):
    """test_determinism_gpu's `det` fixture around one of its tests."""
    prev = K.set_deterministic(True)
    try:
        fn(K, *args)
    finally:
        K.set_deterministic(prev)


# the `det` column of CASES: True - the case runs in the default mode and again inside K.det_scope(True); otherwise once, because
OWN = None        # the helper sets the mode itself through the process default (no scope of ours around it),
PINNED = False    # the helper opens its own scope / the fused kernel under test exists in the default mode only / the model was built with its mode,
NO_WS = False     # the helper calls conv_wgrad without a workspace, which a deterministic call refuses by design, or
STATS = False     # the helper reads the BatchNorm sums in the default layout (entry word 0): a deterministic call leaves integer limbs there


# (id, module, function or callable(module, K), arguments after K, wrappers claimed, det: also inside det_scope(True), extra modules to poison).
# A function named test_* / check_* of `module` gets (K, *args) when its first parameter is K, else (*args).
CASES = [
    # generic implicit GEMM: forward, dgrad, accumulating dgrad, bh_conv_dgrad_s2, the four weight-gradient kernels of _generic_wgrad
    ("generic-3x3-s1-wgrad_s1+wgrad_kernel", "test_rectangular_gpu", "test_generic_conv", (2, 16, 32, 64, 64, 3, 1, 1), CONV, NO_WS, ("test_conv_kernels_gpu",)),
    ("generic-3x3-s1-small_taps", "test_rectangular_gpu", "test_generic_conv", (1, 20, 28, 24, 40, 3, 1, 1), CONV, NO_WS, ("test_conv_kernels_gpu",)),
    ("generic-3x3-s2-dgrad_s2", "test_rectangular_gpu", "test_generic_conv", (2, 16, 32, 64, 128, 3, 2, 1), CONV, NO_WS, ("test_conv_kernels_gpu",)),
    ("generic-1x1-s2-dgrad_s2", "test_rectangular_gpu", "test_generic_conv", (2, 16, 24, 64, 128, 1, 2, 0), CONV, NO_WS, ("test_conv_kernels_gpu",)),
    ("generic-1x1-wgrad_small", "test_rectangular_gpu", "test_generic_conv", (1, 32, 64, 32, 16, 1, 1, 0), CONV, NO_WS, ("test_conv_kernels_gpu",)),
    ("first-conv-nchw-in", "test_rectangular_gpu", "test_first_conv_nchw_input", (3, 32, 48, 2, 64), ("conv_fwd",), NO_WS, ("test_conv_kernels_gpu",)),
    ("last-conv-nchw-out", "test_rectangular_gpu", "test_last_conv_nchw_output", (2, 16, 40), CONV, NO_WS, ("test_conv_kernels_gpu",)),
    ("convT-2x2", "test_rectangular_gpu", "test_conv_transpose_2x2", (2, 8, 12, 64, 32, "wgrad_small_taps_kernel<2>"), CONV, NO_WS, ("test_conv_kernels_gpu",)),
    # halo-tiled 3x3 in precisions 0, 2, 3, 4 (16 x 24: tiles_x = 3, odd sub-tile count with N = 3)
    ("halo-fp32", "test_rectangular_gpu", "test_halo_kernel_fp32", (3, 16, 24, 64, 64), CONV, NO_WS, ("test_conv_kernels_gpu",)),
    ("halo-f32x3", "test_rectangular_gpu", "test_halo_kernel_f32x3", (3, 16, 24, 64, 64), CONV + ("get",), STATS, ("test_conv_kernels_gpu",)),
    ("halo-f32x2", "test_rectangular_gpu", "test_halo_kernel_f32x2", (3, 16, 24, 64, 64), CONV + ("get",), STATS, ("test_conv_kernels_gpu",)),
    ("halo-f16x2", "test_rectangular_gpu", "test_halo_kernel_f16x2", (3, 16, 24, 64, 64), CONV + ("get",), True, ("test_f16x2_gpu",)),
    ("halo-4x4-maps", "test_conv_kernels_gpu", "test_conv3x3_halo_kernel_on_4x4_maps", (16, 64, 128, 2, 1), CONV + ("get",), STATS, ()),
    # persistent 3x3
    ("pc-f16x2-vs-f64", "test_rectangular_gpu", "test_persistent_kernel_f16x2", (4, 16, 32, 64, 64), CONV + ("get",), True, ("test_f16x2_gpu",)),
    ("pc-forward", "test_conv_pc_gpu", "test_forward_bit_identical", (8, 16, 16, 64, 64), ("conv_fwd", "get"), STATS, ()),
    ("pc-forward-bn-on-load", "test_conv_pc_gpu", "test_forward_batchnorm_on_load_bit_identical", (8, 16, 16, 64, 64, True), ("conv_fwd", "bn_fwd_coeffs"), STATS, ()),
    ("pc-dgrad", "test_conv_pc_gpu", "test_dgrad_bit_identical", (8, 16, 16, 64, 64), ("conv_dgrad", "get"), STATS, ()),
    ("pc-dgrad-bnreduce", "test_conv_pc_gpu", "test_dgrad_batchnorm_reduce_bit_identical", (8, 16, 16, 64, 64, True, False, False), ("conv_dgrad",), STATS, ()),
    # streaming 1x1 / 2x2
    ("pointwise-convT", "test_pointwise_gpu", "test_pointwise_forward_against_float64", ("convT", 16, 64, 64, 32, 16, 2), ("conv_fwd",), STATS, ()),
    ("pointwise-1x1", "test_pointwise_gpu", "test_pointwise_forward_against_float64", ("1x1", 16, 64, 64, 32, 16, 2), ("conv_fwd",), STATS, ()),
    ("pointwise-1x1-bn-on-load", "test_pointwise_gpu", "test_pointwise_batchnorm_on_load", (16, 64, 64, 32, 16, True), ("conv_fwd", "bn_fwd_coeffs"), STATS, ()),
    # 7x7 stems
    ("stem7-forward-1", "test_conv_kernels_gpu", "check_stem7_forward_kernel", (4, 128, 128, 1, False), ("conv_fwd",), True, ()),
    ("stem7-forward-2", "test_conv_kernels_gpu", "check_stem7_forward_kernel", (4, 128, 128, 2, False), ("conv_fwd",), True, ()),
    ("stem7-forward-f16-1", "test_conv_kernels_gpu", "check_stem7_forward_in_fp16_pieces", (4, 128, 128, 1, False, 1.0), ("conv_fwd",), STATS, ()),
    ("stem7-forward-f16-2", "test_conv_kernels_gpu", "check_stem7_forward_in_fp16_pieces", (4, 128, 128, 2, True, 1.0), ("conv_fwd",), True, ()),
    ("stem7-wgrad-ws", "test_rectangular_gpu", "test_stem7_wgrad_two_planes", (16, 64, 128), ("conv_fwd", "conv_wgrad"), True, ("test_conv_kernels_gpu",)),
    ("stem7-dgrad", "test_rectangular_gpu", "test_stem7_dgrad_one_plane", (4, 64, 128), CONV, True, ("test_conv_kernels_gpu",)),
    ("stem7-dgrad-two-step", "test_conv_kernels_gpu", "check_gray_stem_conv_and_its_dgrad", (8, 64, 64, True), CONV, PINNED, ()),
    ("stem7-dgrad-small", "test_conv_kernels_gpu", "check_gray_stem_conv_and_its_dgrad", (2, 32, 32, False), CONV, True, ()),
    ("stem7-dgrad-rgb", "test_rgb_gpu", "test_rgb_stem_dgrad_vs_torch", (4, 128), ("_stem_dgrad_two_step",), True, ()),
    ("stem7-dgrad-f16", "test_conv_kernels_gpu", "test_gray_stem_dgrad_in_fp16_pieces", (8, 64, 1.0), ("conv_dgrad",), PINNED, ()),
    ("stem7-dgrad-warp-fp32", "test_head_kernels_gpu", "check_stem_dgrad_with_the_warp_adjoint_folded_in", (4, 64, 128, 4, True, 0), ("h4pt_fwd",), PINNED, ()),
    ("stem7-dgrad-warp-f16", "test_head_kernels_gpu", "check_stem_dgrad_with_the_warp_adjoint_folded_in", (4, 64, 128, 4, True, 4), ("h4pt_fwd",), PINNED, ()),
    ("stem7-forward-warp", "test_head_kernels_gpu", "check_stem_forward_with_the_warp_folded_in", (8, 128, 64, 2, True, True, False), ("conv_fwd",), PINNED, ()),
    ("stem7-forward-warp-det", "test_head_kernels_gpu", "check_stem_forward_with_the_warp_folded_in", (8, 128, 64, 2, True, True, True), ("conv_fwd",), PINNED, ()),
    # bh_conv_wgrad_det: s1 partial tiles, f32x3 / fp16 pieces; (the shadow path: test_wgrad_det_accumulates below)
    ("wgrad-det-s1", "test_rectangular_gpu", "test_wgrad_deterministic_mode", (16, 16, 32, 64, 64), (), NO_WS, ("test_conv_kernels_gpu",)),
    ("wgrad-f32x3", "test_conv_kernels_gpu", "check_wgrad_f32x3_kernel", (2, 8, 8, 64, 64), (), NO_WS, ()),
    ("wgrad-f32x3-32ch", "test_conv_kernels_gpu", "check_wgrad_f32x3_kernel", (2, 16, 16, 64, 32), (), NO_WS, ()),
    ("wgrad-f16x2", "test_f16x2_gpu", "check_wgrad_f16x2_kernel", (2, 8, 8, 64, 64), (), NO_WS, ()),
    ("wgrad-f16x2-4x4", "test_f16x2_gpu", "test_wgrad_f16x2_on_4x4_maps", (12, 64, 128), (), NO_WS, ()),
    # BatchNorm
    ("bn-fwd-bwd", "test_conv_kernels_gpu", "test_batchnorm_fwd_bwd", (2, 3, 8, 64, True, True, True), ("bn_fwd", "bn_bwd"), True, ()),
    ("bn-fwd-bwd-mask-from-x", "test_conv_kernels_gpu", "test_batchnorm_fwd_bwd", (1, 2, 16, 128, True, False, True), ("bn_fwd", "bn_bwd"), True, ()),
    ("bn-fwd-bwd-eval", "test_conv_kernels_gpu", "test_batchnorm_fwd_bwd", (2, 2, 8, 64, True, True, False), ("bn_fwd", "bn_bwd"), True, ()),
    ("bn-one-channel", "test_zhang_gpu", "test_one_channel_batchnorm", (1, 3, 17, False, True, True), ("bn_fwd", "bn_bwd"), True, ()),
    ("bn-join", "test_conv_kernels_gpu", "test_two_branch_batchnorm_join", (2, 2, 16, 16, True), ("bn_join_fwd", "bn_join_bwd"), True, ()),
    ("bn-from-1x1", "test_conv_kernels_gpu", "test_batchnorm_adjoint_rebuilds_the_1x1_dgrad", (4, 32, 32, True), ("bn_bwd_from_1x1",), True, ()),
    ("bn-maxpool", "test_conv_kernels_gpu", "check_batchnorm_relu_maxpool_in_one_pass", (1, 3, 10, 14, 32, True), ("bn_maxpool_fwd", "bn_maxpool_bwd"), True, ()),
    ("bn-on-load-3x3", "test_conv_kernels_gpu", "check_batchnorm_on_load_matches_materialised_batchnorm", (6, 24, 16, 64, 96, True), ("bn_fwd_coeffs", "conv_fwd", "get"), STATS, ()),
    ("bn-on-load-3x3-f16x2", "test_f16x2_gpu", "test_f16x2_batchnorm_on_load_and_records", (4, 32, 32, 32, False), ("bn_fwd_coeffs", "conv_fwd", "get"), True, ()),
    ("bn-on-load-1x1", "test_conv_kernels_gpu", "test_batchnorm_on_load_1x1_matches_materialised_batchnorm", (4, 32, 32, 16, True), ("bn_fwd_coeffs", "conv_fwd"), True, ()),
    ("conv-fwd-bnstats-3x3", "test_conv_kernels_gpu", "check_conv_fwd_with_batchnorm_sums", (2, 8, 8, 32, 64, 3, 2), ("conv_fwd", "bn_fwd"), STATS, ()),
    ("conv-fwd-bnstats-1x1", "test_conv_kernels_gpu", "check_conv_fwd_with_batchnorm_sums", (2, 4, 4, 16, 32, 1, 2), ("conv_fwd", "bn_fwd"), STATS, ()),
    ("convT-fwd-bnstats", "test_conv_kernels_gpu", "test_conv_transpose_fwd_with_batchnorm_sums", (4, 8, 32, 32, 2), ("conv_fwd",), STATS, ()),
    ("dgrad-bnreduce", "test_conv_kernels_gpu", "check_dgrad_epilogue_accumulates_batchnorm_backward_sums", (4, 8, 8, 32, 64, 2, False, False, False), ("conv_dgrad", "bn_bwd"), True, ()),
    ("dgrad-bnreduce-acc", "test_conv_kernels_gpu", "check_dgrad_epilogue_accumulates_batchnorm_backward_sums", (8, 16, 16, 64, 32, 2, True, True, True), ("bn_fwd", "bn_bwd"), True, ()),
    # fused tail
    ("tail-dense", "test_conv_kernels_gpu", "test_fused_tail_fwd_bwd", (1, 3, 8, 16, 128, 2, True, 0), ("tail_fwd", "tail_bwd"), True, ()),
    ("tail-sparse-1", "test_conv_kernels_gpu", "test_fused_tail_fwd_bwd", (1, 3, 8, 16, 128, 2, True, 1), ("tail_fwd", "tail_bwd"), True, ()),
    ("tail-sparse-2", "test_conv_kernels_gpu", "test_fused_tail_fwd_bwd", (2, 2, 16, 16, 128, 2, True, 2), ("tail_fwd", "tail_bwd"), True, ()),
    ("tail-eval", "test_conv_kernels_gpu", "test_fused_tail_fwd_bwd", (2, 2, 16, 16, 128, 2, False, 0), ("tail_fwd", "tail_bwd"), True, ()),
    # pool / GAP / add
    ("maxpool-gap-add", "test_conv_kernels_gpu", "check_maxpool_gap_add", (1, 17, 9, 8), ("maxpool_fwd", "maxpool_bwd", "gap_fwd", "gap_bwd"), True, ()),
    # geometry
    ("h4pt", "test_head_kernels_gpu", "check_h4pt_fwd_bwd", ((96, 64),), ("h4pt_fwd", "h4pt_bwd"), True, ()),
    ("dlt-n4-P16", "test_head_kernels_gpu", lambda HK, K: _dlt(HK, K, 4, 16), (), ("dlt_fwd",), True, ()),
    ("dlt-n1-P128", "test_head_kernels_gpu", lambda HK, K: _dlt(HK, K, 1, 128), (), ("dlt_fwd",), True, ()),
    # warp
    ("warp-pool8", "test_head_kernels_gpu", "check_warp_fwd_bwd", (3, 1, 32, 32, 8), ("warp_fwd", "mask_coverage_fwd", "h4pt_fwd"), True, ()),
    ("warp-pool4-fast", "test_head_kernels_gpu", "check_warp_fwd_bwd", (2, 3, 64, 64, 4), ("warp_fwd", "mask_coverage_fwd"), True, ()),
    ("warp-pool4-generic", "test_head_kernels_gpu", "check_warp_fwd_bwd", (2, 2, 48, 64, 4), ("warp_fwd", "mask_coverage_fwd"), True, ()),
    ("warp-pool1", "test_head_kernels_gpu", "check_warp_fwd_bwd", (2, 2, 32, 48, 1), ("warp_fwd", "mask_coverage_fwd"), True, ()),
    ("warp-pool32", "test_head_kernels_gpu", "check_warp_fwd_bwd", (2, 1, 64, 96, 32), ("warp_fwd", "mask_coverage_fwd"), True, ()),
    ("warp-bwd-img", "test_zhang_gpu", "check_warp_adjoint_with_respect_to_the_image", (False, 48, 80), ("warp_bwd_img", "warp_fwd"), PINNED, ()),
    ("warp-bwd-img-det", "test_zhang_gpu", "check_warp_adjoint_with_respect_to_the_image", (True, 48, 80), ("warp_bwd_img", "warp_fwd"), PINNED, ()),
    ("photo-warp", "test_photometric_gpu", "test_photo_warp_fwd_and_adjoint_vs_float64", (1,), ("photo_warp_fwd", "h4pt_fwd"), True, ()),
    ("photo-warp-rgb", "test_photometric_gpu", "test_photo_warp_fwd_and_adjoint_vs_float64", (3,), ("photo_warp_fwd", "h4pt_fwd"), True, ()),
    # losses, their adjoints and anchor adjoints
    ("triplet", "test_head_kernels_gpu", "test_triplet_fwd_bwd", (2, 8, 16, False), ("_triplet_fwd", "bihome_loss_fwd", "_bihome_bwd"), True, ()),
    ("triplet-masks", "test_head_kernels_gpu", "test_triplet_fwd_bwd", (2, 5, 64, True), ("_triplet_fwd", "bihome_loss_fwd", "_bihome_bwd"), True, ()),
    ("hinge", "test_loss_variants_gpu", "test_channel_aware_pair_vs_float64_autograd", (2, 5, 16, True), ("_triplet_fwd", "bihome_loss_fwd", "_bihome_bwd"), True, ()),
    ("one-line", "test_head_kernels_gpu", "test_oneline_hinge_loss_fwd_bwd", (2, 5, 16, 9.0), ("_oneline_fwd", "_oneline_bwd"), True, ()),
    ("cosine", "test_loss_variants_gpu", "test_cosine_pair_vs_float64_autograd", (2, 5, 16, 3), ("_oneline_fwd", "_oneline_bwd"), True, ()),
    ("one-line-anchor", "test_projection_gpu", "test_oneline_anchor_adjoint_vs_float64_autograd", (2, 5, 16, "l1", 3, True), ("oneline_anchor_bwd", "_oneline_fwd"), True, ()),
    ("cosine-anchor", "test_projection_gpu", "test_oneline_anchor_adjoint_vs_float64_autograd", (2, 5, 16, "cosine", 1, False), ("oneline_anchor_bwd", "_oneline_fwd"), True, ()),
    ("double-line-anchor", "test_projection_gpu", "test_double_line_anchor_adjoint_vs_float64_autograd", (2, 5, 16, "agnostic", True), ("bihome_anchor_bwd", "_triplet_fwd"), True, ()),
    ("hinge-anchor", "test_projection_gpu", "test_double_line_anchor_adjoint_vs_float64_autograd", (2, 5, 16, "hinge", False), ("bihome_anchor_bwd", "_triplet_fwd"), True, ()),
    ("zhang-double", "test_zhang_gpu", "test_zhang_triplet_kernels", (2, 16, "inf", True), ("zhang_triplet_fwd", "zhang_triplet_bwd", "bihome_loss_fwd"), True, ()),
    ("zhang-one-line", "test_zhang_gpu", "test_zhang_triplet_kernels", (2, 32, 0.5, False), ("zhang_triplet_fwd", "zhang_triplet_bwd", "bihome_loss_fwd"), True, ()),
    # mask, scale_samples, l2norm, projection
    ("mask-gate", "test_zhang_gpu", "test_mask_gate_kernels", (0.5,), ("mask_fwd", "mask_bwd"), True, ()),
    ("mask-gate-no-normalisation", "test_zhang_gpu", "test_mask_gate_kernels", (-1.0,), ("mask_fwd", "mask_bwd"), True, ()),
    ("scale-samples", "test_head_kernels_gpu", "test_scale_samples_and_scored_hinge_vs_torch64", (), ("scale_samples_fwd", "scale_samples_bwd", "_oneline_fwd", "_oneline_bwd"), True, ()),
    ("l2norm", "test_projection_gpu", "test_l2norm_pair_vs_float64", (2, 5, 16), ("l2norm_fwd", "l2norm_bwd"), True, ()),
    ("relu-bwd", "test_projection_gpu", "test_relu_bwd_masks_by_the_output", (), ("relu_bwd",), True, ()),
    ("projection", "test_projection_gpu", "test_projection_runner_vs_float64_linear", ((2, 5, 5, 64),), ("conv_fwd",), True, ("bihome_amd.net", "bihome_amd.heads.PerceptualHead")),
    # DSAC scoring
    ("dsac-soft", "test_dsac_scoring_gpu", "test_soft_scores_fwd_bwd_vs_torch64", (3, 4, 5, 7), ("dsac_scores_fwd", "dsac_scores_bwd"), True, ()),
    ("dsac-soft-n11", "test_dsac_scoring_gpu", "test_soft_scores_fwd_bwd_vs_torch64", (2, 11, 9, 30), ("dsac_scores_fwd", "dsac_scores_bwd"), True, ()),
    ("dsac-hard", "test_dsac_scoring_gpu", "test_hard_counts_are_exact", (3, 4, 5, 7), ("dsac_score",), True, ()),
    ("dsac-repr-error", "test_head_kernels_gpu", "test_dsac_scores_fwd_bwd_vs_torch64", (), ("dsac_scores_fwd", "dsac_scores_bwd"), True, ()),
    # RANSAC and its LM polish
    ("ransac-5x7", "test_ransac_gpu", lambda RS, K: _field_chain(RS, K, 2), (), ("ransac_homography",), True, ()),
    ("ransac-16x16-K2100", "test_ransac_gpu", lambda RS, K: _field_chain(RS, K, 1), (), ("ransac_homography",), True, ()),
    ("ransac-tie", "test_ransac_gpu", "test_lowest_k_wins_a_tie_across_lanes", (2,), ("ransac_homography",), True, ()),
    ("ransac-fallback", "test_ransac_gpu", "test_fallback_boundary", (), ("ransac_homography",), True, ()),
    ("lm-5x7", "test_ransac_lm_gpu", "test_other_field_shapes", (5, 7), ("homography_refine_lm",), True, ()),
    ("lm-after-ransac-37x83", "test_ransac_lm_gpu", "test_polish_after_ransac_at_37x83", (), ("ransac_homography", "homography_refine_lm"), True, ()),
    # the device pair generator
    ("pairs-gray", "test_head_kernels_gpu", "test_gpu_pair_generator_matches_host_generator", (), (), True, ("bihome_amd.synth_gpu",)),
    ("pairs-rgb", "test_datagen_gpu", "test_rgb_patches_match_host_arithmetic", (32, 8, 4, 32), (), True, ("bihome_amd.synth_gpu",)),
    ("pairs-all-points", "test_datagen_gpu", "test_all_points_target", (32, 8, 5), (), True, ("bihome_amd.synth_gpu",)),
    # deterministic calls whose helpers need the deterministic default: limb statistics from the conv epilogue, the weight gradients without
    # a partial-tile form (limb shadow, zeroed by the callee), the one-writer pool-32 coverage
    ("det-bnstats-limbs", "test_determinism_gpu", lambda D, K: _det_default(K, D.test_limb_accumulation_of_batchnorm_sums_is_exact_and_repeatable), (),
     ("conv_fwd", "bn_fwd"), OWN, ()),
    ("det-wgrad-shadow-small", "test_determinism_gpu", lambda D, K: _det_default(K, D.test_weight_gradient_every_shape_has_a_deterministic_form, 4, 64, 32, 16, 1, 1, 0, False), (),
     (), OWN, ()),
    ("det-wgrad-shadow-convT", "test_determinism_gpu", lambda D, K: _det_default(K, D.test_weight_gradient_every_shape_has_a_deterministic_form, 4, 32, 32, 32, 2, 2, 0, True), (),
     (), OWN, ()),
    ("det-pool32-coverage", "test_determinism_gpu", lambda D, K: _det_default(K, D.test_pool32_coverage_has_a_one_writer_form), (), ("warp_fwd",), OWN, ()),
    # the backbone through the planner's fusions, 64 x 96 patches (its Runner is built in the default mode)
    ("backbone-64x96", "test_rectangular_gpu", lambda R, K: _backbone_64x96(R, K), (), CONV + ("bn_fwd_coeffs", "bn_join_fwd", "bn_join_bwd", "tail_fwd", "tail_bwd", "bn_maxpool_fwd", "bn_maxpool_bwd", "bn_bwd_from_1x1", "get"), False,
     ("test_model_gpu", "bihome_amd.net", "bihome_amd.backbones.Rethinking")),
]
SYNTH_CLAIMS = {"pairs-gray": ("make",), "pairs-rgb": ("make",), "pairs-all-points": ("make",)}      # allocating functions of synth_gpu.py

# wrapper of bihome_amd/kernels.py that calls torch.empty / torch.empty_like -> a case above that runs it under the shim (asserted there)
COVERED_BY = {}
for _c in CASES:
    for _w in _c[4]:
        COVERED_BY.setdefault(_w, _c[0])
# allocating wrappers no case reaches, each with its reason (at most 5: test_buffer_contracts_cpu.py)
EXEMPT = {}


def _ids():
    out = []
    for c in CASES:
        out.append(pytest.param(c, False, id=c[0]))
        if c[5]:
            out.append(pytest.param(c, True, id=c[0] + "-det"))
    return out


def _kernels():
    from bihome_amd import kernels
    return kernels


def run_case(case, det, monkeypatch):
    name, modname, fn, args, claims, _, extra = case
    K = _kernels()
    mod = importlib.import_module(modname)
    p = poisoned_alloc.poison(monkeypatch, K, mod, *[importlib.import_module(m) for m in extra])
    monkeypatch.setattr(K, "_STEM_WGRAD_WS", {})          # (the stem weight gradient's cached workspace is born under the shim)
    call = fn if callable(fn) else getattr(mod, fn)
    takes_K = callable(fn) or call.__code__.co_varnames[:call.__code__.co_argcount][:1] == ("K",)
    import contextlib
    with (contextlib.nullcontext() if case[5] is OWN else K.det_scope(det)):
        if callable(fn):
            call(mod, K)
        elif takes_K:
            call(K, *args)
        else:
            call(*args)
    n = p.verify()
    assert n > 0
    print("\nALLOCATED %s%s: %d buffers, from %s" % (name, "-det" if det else "", n, sorted(p.callers())))
    missing = [w for w in claims if "bihome_amd.kernels" not in p.modules_of(w)]
    missing += [w for w in SYNTH_CLAIMS.get(name, ()) if "bihome_amd.synth_gpu" not in p.modules_of(w)]
    assert not missing, "%s claims %s, which did not allocate under the shim (allocated: %s)" % (name, sorted(missing), sorted(p.callers()))
    return p


@pytest.mark.parametrize("case,det", _ids())
def test_kernel_family_in_poisoned_exact_size_buffers(case, det, monkeypatch):
    run_case(case, det, monkeypatch)


def test_the_shim_on_device_tensors():
    """What test_buffer_contracts_cpu.py holds on CPU tensors, on the device: the fill, the address (512-byte multiple: what vector and buffer
    loads of a torch.empty block see), and that a store next to the interior - made through the block itself, inside the allocation - is
    reported with its side."""
    p = poisoned_alloc.Poisoned()
    f, i, z = p.empty(3, 5, device="cuda"), p.empty(7, dtype=torch.int32, device="cuda"), p.zeros(2, 9, dtype=torch.float64, device="cuda")
    like = p.empty_like(f, dtype=torch.uint8)
    assert torch.isnan(f).all() and (i == 1).all() and (z == 0).all() and (like == 1).all() and like.is_cuda and like.shape == f.shape
    assert all(t.data_ptr() % poisoned_alloc.ALIGN_BYTES == 0 and t.is_contiguous() for t in (f, i, z, like))
    assert p.callers() == {"test_the_shim_on_device_tensors"} and p.verify() == 4
    for side, at in (("front", -1), ("behind", 15)):
        t = p.empty(3, 5, device="cuda")
        rec = p._records[-1]
        rec.block[rec.front + at] = 0.0
        with pytest.raises(AssertionError, match="red zone %s" % side):
            p.verify()


# ------------------------------------------------------------------------------------------------
# 2. step level
# ------------------------------------------------------------------------------------------------
STEP_MODULES = ("bihome_amd.kernels", "bihome_amd.net", "bihome_amd.step", "bihome_amd.synth_gpu", "bihome_amd.backbones.ContentAware",
                "bihome_amd.heads.NoOpHead", "bihome_amd.heads.PerceptualHead", "bihome_amd.heads.PhotometricHead", "bihome_amd.heads.TripletHead")


@pytest.mark.parametrize("cfg_name", ["zeng-bihome", "detone-bihome", "zhang-orig", "zeng-ihome-proj"])
def test_two_deterministic_steps_do_not_depend_on_memory_they_do_not_own(cfg_name, monkeypatch):
    import test_determinism_gpu as D
    K = _kernels()
    prev = K.set_deterministic(True)
    try:
        l0, p0 = D._three_steps(cfg_name, B=4, steps=2)
        with monkeypatch.context() as m:
            p = poisoned_alloc.poison(m, *[importlib.import_module(n) for n in STEP_MODULES])
            m.setattr(K, "_STEM_WGRAD_WS", {})
            l1, p1 = D._three_steps(cfg_name, B=4, steps=2)
            checked = p.verify()
    finally:
        K.set_deterministic(prev)
    print("\n%s: %d allocations under the shim, from %s" % (cfg_name, checked, sorted(p.callers())))
    assert checked > 0 and "conv_fwd" in p.callers()
    assert l0 == l1, (l0, l1)
    assert set(p0) == set(p1)
    bad = [k for k in p0 if not torch.equal(p0[k], p1[k])]
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------
# 3. `+=` outputs from a nonzero start
# ------------------------------------------------------------------------------------------------
# The census of include/bihome.h (gradient outputs documented as accumulated; statistics / sums buffers are "zero on entry" and not in it):
#   g_pf of bh_dlt_bwd; gH of bh_warp_bwd, bh_photo_warp_bwd, bh_stem7_dgrad_c1_warp; gw / gbias of bh_conv_wgrad, bh_conv_wgrad_det,
#   bh_conv_wgrad_bnin; ggamma / gbeta of bh_bn_bwd, bh_bn_maxpool_bwd, bh_bn_bwd_from_1x1, both branches of bh_bn_join_bwd; gw1, ggamma,
#   gbeta, gw2, gb2 of bh_tail_bwd; gx of bh_conv_dgrad with `accumulate`.
# Held from a nonzero start elsewhere already: gx (check_conv2d_fwd_dgrad_wgrad, base 1), gH of bh_stem7_dgrad_c1_warp
# (check_stem_dgrad_with_the_warp_adjoint_folded_in, random base), gw of bh_stem7_wgrad and of the s1 form of bh_conv_wgrad_det (twice the
# gradient).  The others: the family's own helper with `base` - its reference, its bound, (out - b) in float64.
def _routes(*names):
    from bihome_amd import _lib
    r = 0
    for n in names:
        r |= getattr(_lib, n)
    return r


def _generic(C, K, base, case, wgrad, *route):
    C.check_conv2d_fwd_dgrad_wgrad(K, *case, route=_routes("ROUTE_GENERIC_CONV", *route), variants={"wgrad": wgrad}, base=base)


def _dlt_base(HK, K, base, n, P):
    from bihome_amd import synth
    HK.check_dlt_fwd_bwd(K, n, P, np.ascontiguousarray(synth.make_head_inputs(6, seed=3, noise=0.7)["pf_hat_12"][:, :, :48, :80]), base=base)


# (id, module, callable(module, K, base), det: also inside det_scope(True))
ACCUMULATED = [
    ("conv_wgrad-wgrad_s1", "test_conv_kernels_gpu", lambda C, K, b: _generic(C, K, b, (2, 16, 32, 64, 64, 3, 1, 1), "wgrad_s1_kernel<1"), False),
    ("conv_wgrad-wgrad_kernel", "test_conv_kernels_gpu", lambda C, K, b: _generic(C, K, b, (2, 16, 32, 64, 64, 3, 1, 1), "wgrad_kernel<true", "ROUTE_WGRAD_GENERIC"), False),
    ("conv_wgrad-small_taps3", "test_conv_kernels_gpu", lambda C, K, b: _generic(C, K, b, (1, 20, 28, 24, 40, 3, 1, 1), "wgrad_small_taps_kernel<3>"), False),
    ("conv_wgrad-stride2", "test_conv_kernels_gpu", lambda C, K, b: _generic(C, K, b, (2, 16, 32, 64, 128, 3, 2, 1), "wgrad_kernel<true"), False),
    ("conv_wgrad-wgrad_small", "test_conv_kernels_gpu", lambda C, K, b: _generic(C, K, b, (1, 32, 64, 32, 16, 1, 1, 0), "wgrad_small_kernel<"), False),
    ("conv_wgrad-convT-small_taps2", "test_conv_kernels_gpu", lambda C, K, b: C.check_conv_transpose_2x2(K, 2, 8, 12, 64, 32, variants={"wgrad": "wgrad_small_taps_kernel<2>"}, base=b), False),
    ("conv_wgrad-convT-wgrad_kernel", "test_conv_kernels_gpu", lambda C, K, b: C.check_conv_transpose_2x2(K, 2, 8, 16, 256, 128, variants={"wgrad": "wgrad_kernel<true"}, base=b), False),
    ("conv_wgrad-nchw-out", "test_conv_kernels_gpu", lambda C, K, b: C.check_last_conv_nchw_output(K, 2, 16, 40, variants={"wgrad": "wgrad_small_kernel<"}, base=b), False),
    ("conv_wgrad_bnin-3x3", "test_conv_kernels_gpu", lambda C, K, b: C.check_batchnorm_on_load_matches_materialised_batchnorm(K, 6, 24, 16, 64, 96, True, base=b), False),
    ("conv_wgrad_bnin-1x1", "test_conv_kernels_gpu", lambda C, K, b: C.test_batchnorm_on_load_1x1_matches_materialised_batchnorm(K, 4, 32, 32, 16, True, base=b), False),
    ("bn_bwd", "test_conv_kernels_gpu", lambda C, K, b: C.test_batchnorm_fwd_bwd(K, 2, 3, 8, 64, True, True, True, base=b), True),
    ("bn_bwd-mask-from-x", "test_conv_kernels_gpu", lambda C, K, b: C.test_batchnorm_fwd_bwd(K, 1, 2, 16, 128, True, False, True, base=b), True),
    ("bn_bwd-eval", "test_conv_kernels_gpu", lambda C, K, b: C.test_batchnorm_fwd_bwd(K, 2, 2, 8, 64, True, True, False, base=b), True),
    ("bn_bwd-one-channel", "test_zhang_gpu", lambda Z, K, b: Z.test_one_channel_batchnorm(2, 2, 16, True, True, True, base=b), True),
    ("bn_maxpool_bwd", "test_conv_kernels_gpu", lambda C, K, b: C.check_batchnorm_relu_maxpool_in_one_pass(K, 1, 3, 10, 14, 32, True, base=b), True),
    ("bn_bwd_from_1x1", "test_conv_kernels_gpu", lambda C, K, b: C.test_batchnorm_adjoint_rebuilds_the_1x1_dgrad(K, 4, 32, 32, True, base=b), True),
    ("bn_join_bwd", "test_conv_kernels_gpu", lambda C, K, b: C.test_two_branch_batchnorm_join(K, 2, 2, 16, 16, True, base=b), True),
    ("bn_join_bwd-64", "test_conv_kernels_gpu", lambda C, K, b: C.test_two_branch_batchnorm_join(K, 1, 3, 8, 64, True, base=b), True),
    ("tail_bwd-dense", "test_conv_kernels_gpu", lambda C, K, b: C.test_fused_tail_fwd_bwd(K, 1, 3, 8, 16, 128, 2, True, 0, base=b), True),
    ("tail_bwd-sparse-1", "test_conv_kernels_gpu", lambda C, K, b: C.test_fused_tail_fwd_bwd(K, 1, 3, 8, 16, 128, 2, True, 1, base=b), True),
    ("tail_bwd-sparse-2", "test_conv_kernels_gpu", lambda C, K, b: C.test_fused_tail_fwd_bwd(K, 2, 2, 16, 16, 128, 2, True, 2, base=b), True),
    ("tail_bwd-eval", "test_conv_kernels_gpu", lambda C, K, b: C.test_fused_tail_fwd_bwd(K, 2, 2, 16, 16, 128, 2, False, 0, base=b), True),
    ("dlt_bwd-n4-P16", "test_head_kernels_gpu", lambda HK, K, b: _dlt_base(HK, K, b, 4, 16), True),
    ("dlt_bwd-n1-P128", "test_head_kernels_gpu", lambda HK, K, b: _dlt_base(HK, K, b, 1, 128), True),
    ("warp_bwd-pool8", "test_head_kernels_gpu", lambda HK, K, b: HK.check_warp_fwd_bwd(K, 3, 1, 32, 32, 8, base=b), True),
    ("warp_bwd-pool4", "test_head_kernels_gpu", lambda HK, K, b: HK.check_warp_fwd_bwd(K, 2, 3, 64, 64, 4, base=b), True),
    ("warp_bwd-pool4-generic", "test_head_kernels_gpu", lambda HK, K, b: HK.check_warp_fwd_bwd(K, 2, 2, 48, 64, 4, base=b), True),
    ("photo_warp_bwd", "test_photometric_gpu", lambda PH, K, b: PH.test_photo_warp_fwd_and_adjoint_vs_float64(K, 1, base=b), True),
    ("photo_warp_bwd-rgb", "test_photometric_gpu", lambda PH, K, b: PH.test_photo_warp_fwd_and_adjoint_vs_float64(K, 3, base=b), True),
]


def _acc_ids():
    out = []
    for c in ACCUMULATED:
        out.append(pytest.param(c, False, id=c[0]))
        if c[3]:
            out.append(pytest.param(c, True, id=c[0] + "-det"))
    return out


@pytest.mark.parametrize("case,det", _acc_ids())
def test_accumulated_outputs_from_a_nonzero_start(case, det):
    import test_conv_kernels_gpu as C
    name, modname, fn, _ = case
    K = _kernels()
    base = C.FromBase(seed=len(name))
    del C.ERRORS[:]
    with K.det_scope(det):
        fn(importlib.import_module(modname), K, base)
    assert base.checked > 0 and base.checked == len(base.bases), (base.checked, len(base.bases))
    if C.ERRORS:
        err, tol = max(C.ERRORS, key=lambda e: e[0] / e[1])
        print("\nMEASURED %s%s: %d outputs from a nonzero start; largest normalised error of %d comparisons %.3e (bound %.1e)"
              % (name, "-det" if det else "", base.checked, len(C.ERRORS), err, tol))


# bh_conv_wgrad_det, gw AND gbias, in a workspace of exactly bh_conv_wgrad_det_bytes() with red zones (this module's torch.empty below is the
# shim's): (N, H, Ci, Co, k, s, p, transposed, precision, the kernel bh_conv_variant must name)
WGRAD_DET = [
    (4, 16, 64, 64, 3, 1, 1, False, 0, "wgrad_s1_kernel<1,false>+wgrad_s1_reduce_kernel"),      # partial tiles, stride-1 fast path
    (4, 16, 96, 96, 3, 1, 1, False, 0, "wgrad_kernel<true"),                                                     # channels % 64 != 0
    (2, 8, 64, 64, 3, 1, 1, False, 2, "wgrad_x3_kernel<"),                                        # f32x3 partial blocks
    (2, 16, 64, 32, 3, 1, 1, False, 2, "wgrad_x3_kernel<"),                                       # 32-channel blocks
    (2, 8, 64, 64, 3, 1, 1, False, 4, "wgrad_x3_kernel<"),                                        # fp16 pieces
    (2, 16, 64, 128, 3, 2, 1, False, 0, "wgrad_kernel<true"),                                                    # generic split-K kernel: limb shadow
    (2, 32, 32, 16, 1, 1, 0, False, 0, "wgrad_small_kernel<true>"),                                                     # small-channel kernel
    (2, 16, 32, 32, 2, 2, 0, True, 0, "wgrad_small_taps_kernel<2>"),                                                      # ConvTranspose 2x2
]


@pytest.mark.parametrize("N,H,Ci,Co,k,s,p,tr,prec,kernel", WGRAD_DET)
def test_wgrad_det_accumulates_in_a_workspace_of_exactly_its_size(N, H, Ci, Co, k, s, p, tr, prec, kernel, monkeypatch):
    import sys
    import torch.nn.functional as F
    import test_conv_kernels_gpu as C
    K = _kernels()
    shim = poisoned_alloc.poison(monkeypatch, K, sys.modules[__name__])
    g = torch.Generator().manual_seed(N + H + Ci + Co)
    base = C.FromBase(seed=k + s)
    with K.det_scope(True):
        d = K.conv_desc(N, H, H, Ci, Co, k, s, p, transposed=tr, precision=prec)
        x = torch.randn(N, H, H, Ci, generator=g)
        gy = torch.randn(N, d.Ho, d.Wo, Co, generator=g)
        w = torch.zeros((Ci, Co, k, k) if tr else (Co, Ci, k, k), dtype=torch.float64, requires_grad=True)
        b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
        xd = x.double().permute(0, 3, 1, 2)
        y = F.conv_transpose2d(xd, w, b, stride=s) if tr else F.conv2d(xd, w, b, stride=s, padding=p)
        y.backward(gy.double().permute(0, 3, 1, 2))
        name = K.conv_variant(d, "wgrad_det")
        assert name.startswith(kernel), name
        need = K.wgrad_det_bytes(d)
        assert need > 0 and need % 4 == 0
        ws = torch.empty(need // 4, dtype=torch.float32, device="cuda")
        gw, gb = base.start(w.grad.permute(0, 2, 3, 1), torch.float32), base.start(b.grad, torch.float32)
        K.conv_wgrad(x.cuda(), gy.cuda(), gw, gb, d, det_ws=ws)
        del C.ERRORS[:]
        try:
            # (the bound of check_conv2d_fwd_dgrad_wgrad for gw and gbias against float64)
            C.close(base.result(gw).permute(0, 3, 1, 2), w.grad)
            C.close(base.result(gb), b.grad)
        finally:
            print("\nMEASURED %s, %d workspace bytes: (gw - b, gbias - b) against float64 %s (bound 3.0e-05)" % (name, need, ["%.3e" % e for e, _ in C.ERRORS]))
    assert shim.verify() > 0 and "test_wgrad_det_accumulates_in_a_workspace_of_exactly_its_size" in shim.callers()
