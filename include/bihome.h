/*
 * bihome.h - C ABI of libbihome_hip.so: the MI355X (gfx950) kernels behind the biHomE training hot path.
 *
 * Boundary contract: plain device pointers + sizes + a hipStream_t passed as void*,
 * int status return (0 = ok, >0 = hipError_t, <0 = BH_E_*), no allocation, no global mutable state (kernel routing is
 * a pure function of the arguments; the only process state is the per-device "dynamic LDS attribute set" flags),
 * re-entrant per stream.  Builds with -DBH_TUNING (tools/ only, `make tuning`) add the bh_debug_force_tile ablation
 * hook, which IS global state; the default library does not contain it.  The reference has no FFI of its own (it is pure Python over ATen); each entry point
 * below names the reference call site (path:line under the upstream repository) whose arithmetic it
 * replaces.  The host-side mirror of the reference's plugin API (src/backbones/<Name>.Model,
 * src/heads/<Name>.Model) lives in bihome_amd/ and calls these through ctypes.
 *
 * Layouts: images/patches/perspective fields are NCHW float32 exactly as the reference hands them
 * over; *internal* feature maps of the conv stacks are NHWC float32 ("pixels x channels"), conv
 * weights are [Cout][kh][kw][Cin] (= a torch channels_last OIHW tensor), transposed-conv weights
 * [Cin][kh][kw][Cout] (= channels_last IOHW).  Homographies are row-major 3x3.
 *
 * One operation, one entry point: it has the plain name and takes ALL its arguments; the optional ones are NULL / 0.  ABI version 2
 * (bh_version) removed the _f / _m / _amax / _route twins of version 1: each full-signature call took the plain name of the short form
 * that forwarded to it.
 */
#ifndef BIHOME_H
#define BIHOME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BH_OK 0
#define BH_E_BADARG (-1)
#define BH_E_UNSUPPORTED (-2)

/* library / device probe: returns ABI version (>0); writes gcnArchName of device 0 if buf != NULL */
int bh_version(void);
int bh_device_arch(char* buf, int buflen);

/* Deterministic calls (round 3: a process-wide switch; round 4: a PER-CALL bit - the library holds no mode and no other mutable
 * state).  What torch.use_deterministic_algorithms is to the reference's ATen path (train.py:379-387).
 * By default cross-workgroup sums use hardware floating-point atomics, whose rounding depends on arrival order: two runs of the
 * same step differ in the last bits.  With the bit set a launch is order-independent:
 *   - conv family (bh_conv_desc.route & BH_ROUTE_DETERMINISTIC): BatchNorm statistics / backward sums / bias column sums accumulated
 *     in conv epilogues go through exact integer limbs inside the padded sums entries (csrc/common.h bh_det_add); weight and bias
 *     gradients: bh_conv_wgrad_det with a workspace of bh_conv_wgrad_det_bytes(d) - partial tiles added in split order (split-operand /
 *     stride-1 kernels) or integer-limb shadow entries (every other shape).  bh_conv_wgrad / bh_conv_bias_grad have no workspace
 *     and stay atomic;
 *   - BatchNorm (flags & BH_BN_DETERMINISTIC in bh_bn_fwd / bh_bn_bwd and their fused forms): the statistics pass writes, and every pass reads, the limb
 *     encoding.  A sums table must be written and read in ONE mode (the forward that leaves sums for its backward, a conv epilogue and
 *     the BatchNorm that consumes its statistics); bh_bn_fwd_coeffs looks at both encodings;
 *   - bh_warp_bwd, bh_photo_warp_bwd, bh_triplet_l1_fwd, bh_triplet_hinge_fwd, bh_oneline_loss_fwd, bh_oneline_cos_loss_fwd,
 *     bh_scale_samples_bwd, bh_dsac_scores_bwd, bh_tail_bwd
 *     (flags & BH_F_DETERMINISTIC): one workgroup per sample / channel is the only writer of its sums;
 *   - bh_dlt_bwd: duplicates of a sample's indices are added in point order inside the wave, hypotheses in launch order;
 *   - bh_warp_fwd with pool = 32: the pooled coverage by a one-writer kernel (the default adds four quarter-window sums with atomics);
 *   - bh_warp_bwd_img: integer-limb entries in the caller's scratch instead of float atomics.
 * flags = 0 is the default (atomic) form of each.  Same arithmetic otherwise: results differ from the default only by the order of
 * additions.  A HIP graph replays whatever bits its captured launches carried. */
#define BH_F_DETERMINISTIC 1          /* flags argument of the entry points listed above */
#define BH_BN_DETERMINISTIC 32        /* flags argument of the BatchNorm entry points (bh_bn_fwd, bh_bn_bwd, bh_bn_stats, ...) */
/* Measured matrix-pipe peak for the roofline: sustained TFLOP/s of a bare v_mfma_f32_32x32x16_bf16 stream on the whole
 * chip (two workgroups of four waves per CU, ~5 ms), with constant operands (random_operands = 0) or random-bit operands (1: the data
 * toggling of real tensors - on MI355X the power-limited rate, 25-35 % below the first).  Synchronises the stream.  sink_dev: 4 bytes of
 * device memory (never written). */
int bh_probe_mfma_bf16(int random_operands, float* sink_dev, double* tflops, void* stream);
/* the same stream of v_mfma_f32_32x32x2_f32 (the fp32-input instruction of the generic, stem and small-channel kernels) */
int bh_probe_mfma_f32(int random_operands, float* sink_dev, double* tflops, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Geometry (per-sample small dense algebra, double precision inside)
 * ------------------------------------------------------------------------------------------- */

/* four_point_to_homography, src/data/utils.py:7-33 (torch branch -> kornia.get_perspective_transform):
 * corners [[0,0],[W,0],[W,H],[0,H]] (image_shape_to_corners, src/data/utils.py:36-51) + delta[B,4,2]
 * -> H[B,9] with H22 = 1, 8x8 solve with partial pivoting.  H64 feeds the warp kernels, H32 is the
 * float copy handed back to the host module. */
int bh_h4pt_fwd(const float* delta, int B, float W, float H, double* H64, float* H32, void* stream);
/* adjoint of the above: gH[B,9] (double; entry 8 ignored) -> gdelta[B,8] (overwritten) */
int bh_h4pt_bwd(const float* delta, const double* H64, const double* gH, int B, float W, float H,
                float* gdelta, void* stream);

/* DSACSoftmax.__sample_hypotheses, src/heads/ransac_utils.py:47-74, fused with forward_map_field
 * (src/heads/PerceptualHead.py:125-146) and the corner transform (PerceptualHead.py:175-178):
 * pf[B,2,h,w] perspective field, choice[B, n*P] int64 sampled indices (row-major idx = y*w + x)
 * -> Hdlt[B*n,9] (kornia.find_homography_dlt: Hartley normalisation, A^T A, smallest eigenvector,
 * denormalise, /(H22+1e-8)) and delta_hat[B*n,4,2] = H.corners - corners.
 * eig[B*n,96] doubles: eigenvectors (81, column i = vector i), eigenvalues (9), index of the
 * smallest (1), spare - saved for the adjoint. */
int bh_dlt_fwd(const float* pf, const int64_t* choice, int B, int n, int P, int h, int w,
               float* Hdlt, float* delta_hat, double* eig, void* stream);
/* adjoint: g_delta[B*n,4,2] -> g_pf[B,2,h,w] += (scatter-add at the sampled indices; caller zeroes) */
/* g_Hdlt[B*n,9] (double, NULL ok): gradient that reaches the normalised homography itself (from the hypothesis scores,
 * bh_dsac_scores_bwd), added to the one that arrives through delta_hat.  flags: BH_F_DETERMINISTIC */
int bh_dlt_bwd(const float* pf, const int64_t* choice, const double* eig, const float* g_delta, const double* g_Hdlt,
               int B, int n, int P, int h, int w, float* g_pf, int flags, void* stream);

/* Hypothesis scoring of DSACSoftmax.__score_hypotheses, src/heads/ransac_utils.py:76-128, all its methods behind one pair of calls, and the
 * softmax over the hypotheses between them.  Per point (x, y) of the field (all h*w of them) and hypothesis j: t = H_j.(x, y) (scale
 * s = |qz| > 1e-8 ? 1/qz : 1), m = (x + pf[b,0,y,x], y + pf[b,1,y,x]), e = sqrt((tx - mx)^2 + (ty - my)^2), all fp32.
 *   BH_DSAC_REPR_ERROR     'repr_error': score[B,n] = sum over the points of |t - m|_1; thr and beta are checked and otherwise unused
 *   BH_DSAC_INLIERS        'inliers_ratio' (:98-103): score = #{points with e < thr} / (h*w); the comparison strict, the count an integer
 *                          (independent of the order of execution).  No adjoint: upstream's comparison cuts the graph
 *   BH_DSAC_SOFT_INLIERS   'soft_inliers_ratio' (:105-111): score = sum over the points of sigmoid(beta (e - thr)), accumulated in double
 * SIGN CONVENTION, upstream's and kept: the weights are softmax(-score) (:126, bh_dsac_scores_fwd) and the evaluation pick
 * (src/heads/PerceptualHead.py:755-757) is their arg-max = the FIRST MINIMUM of score (best[B] int64, NULL ok).  The soft score thus
 * counts soft OUTLIERS and the lower one wins.  The hard ratio counts INLIERS and is negated too: upstream prefers the hypothesis with
 * the FEWEST inliers.  That is an upstream quirk; it is reproduced, not repaired.
 * bh_dsac_scores_fwd: scores[B,n] = softmax(-err) over the hypotheses (ransac_utils.py:126): the weights of the score-weighted
 * multi-hypothesis losses (PerceptualHead.py:276-280,505-511,708-710).
 * bh_dsac_scores_bwd: adjoint of scoring + softmax for BH_DSAC_REPR_ERROR and BH_DSAC_SOFT_INLIERS.  scores[B,n] the softmax weights,
 * g_scores[B,n] -> g_err[B,n] (scratch, overwritten: the gradient w.r.t. the raw scores), g_Hdlt[B*n,9] (double, overwritten; feed to
 * bh_dlt_bwd) and g_pf[B,2,h,w] += (atomics; every point of the field is seen).  'repr_error': sign(t - m) per point.  Soft method:
 * d score / d e = beta sg (1 - sg) with sg = sigmoid(beta (e - thr)); d e / d t = (t - m) / e and exactly 0 where e == 0 (torch's
 * sub-gradient of norm).  Both go through the quotient t = q / qz.  flags & BH_F_DETERMINISTIC: one workgroup per sample adds the
 * hypotheses in order - bit-identical from call to call.
 * BH_E_BADARG, checked before any launch: an unknown method, BH_DSAC_INLIERS passed to the adjoint, thr or beta NaN, thr < 0, n < 1,
 * h or w < 1, a NULL pointer other than best.  BH_E_UNSUPPORTED: h*w > 2^30 (the two inlier-count methods).  B == 0: BH_OK, nothing
 * launched. */
enum { BH_DSAC_REPR_ERROR = 0, BH_DSAC_INLIERS = 1, BH_DSAC_SOFT_INLIERS = 2 };
int bh_dsac_score(const float* pf, const float* Hdlt, int B, int n, int h, int w, int method, float thr, float beta,
                  float* score, int64_t* best, void* stream);
int bh_dsac_scores_fwd(const float* err, int B, int n, float* scores, void* stream);
int bh_dsac_scores_bwd(const float* pf, const float* Hdlt, const float* scores, const float* g_scores, int B, int n, int h, int w,
                       int method, float thr, float beta, float* g_err, double* g_Hdlt, float* g_pf, int flags, void* stream);

/* Robust homography of a perspective field: RANSAC over K minimal samples + least-squares refit on the inliers of the winner - the
 * estimator of upstream's NoOpHead._postprocess, cv2.findHomography(src, dst, cv2.RANSAC, 10) over all h*w correspondences
 * (src/heads/NoOpHead.py:75-109), batched on the device (csrc/ransac.hip).  cv2's Levenberg-Marquardt polish after the refit is a call
 * of its own (bh_homography_refine_lm, below); not included: cv2's sampler - the minimal samples are an input.  Forward only.
 *   pf[B,2,h,w]      the field; pixel (x, y) corresponds to (x + pf[b,0,y,x], y + pf[b,1,y,x]) as in bh_dsac_score
 *   choice[B,K,4]    int64 pixel indices y*w + x of the K minimal samples of every field
 *   thr              inlier threshold in pixels (upstream: 10)
 *   hyp[B,K,9]       out: the hypotheses, H22 = 1 (8x8 solve with partial pivoting in double, stored fp32); all NaN when INVALID:
 *                      - an index outside [0, h*w) (never dereferenced), or two equal indices;
 *                      - three collinear points among the four source or among the four destination points: for every triple
 *                        i < j < k, d1 = p_i - p_k, d2 = p_j - p_k: |d2.x d1.y - d2.y d1.x| <= FLT_EPSILON (|d1.x| + |d1.y| + |d2.x| +
 *                        |d2.y|), evaluated in double without contraction (cv2's minimal-sample check);
 *                      - an elimination pivot with |pivot| <= 1e-12 (or NaN), or a non-finite coefficient
 *   count[B,K]       out: inliers of every hypothesis, -1 for an invalid one.  A pixel is an inlier when (qx/qz - x')^2 + (qy/qz - y')^2
 *                    <= thr^2 with q = hyp.(x, y, 1) (cv2's measure), qz > 0 and finite; fp32, evaluated as (qx - x' qz)^2 + (qy - y' qz)^2
 *                    <= (thr qz)^2.  Integer atomics: independent of the order of execution
 *   best[B]          out: the FIRST k with the maximal count (cv2 replaces its model on strictly more inliers only)
 *   n_inl[B]         out: count[b, best[b]], or 0 when that is below 4 (every hypothesis invalid, or nothing to refit on): the sample is
 *                    FLAGGED and its result is the least-squares fit of all h*w points
 *   mask[B,h,w]      out, NULL ok: 1 where the pixel is an inlier of hypothesis best[b] (the same decision, bit for bit, that was
 *                    counted: sum(mask[b]) == n_inl[b]); all ones for a flagged sample
 *   work[B,32]       scratch (doubles)
 *   H[B,9], delta_hat[B,4,2]   out: the Hartley-normalised DLT over all inliers, /(H22 + 1e-8), and H.corners - corners - the
 *                    arithmetic and the corner convention of bh_dlt_fwd
 * BH_E_BADARG: K < 1, h*w < 4, thr negative or NaN, a NULL pointer other than mask.  BH_E_UNSUPPORTED: B > 65535 or h*w, B*K > 2^30. */
int bh_ransac_homography(const float* pf, const int64_t* choice, int B, int K, int h, int w, float thr, float* hyp, int32_t* count,
                         int64_t* best, int32_t* n_inl, uint8_t* mask, double* work, float* H, float* delta_hat, void* stream);

/* Levenberg-Marquardt polish of a homography on the REPROJECTION error of a perspective field's correspondences - the step
 * cv2.findHomography(src, dst, cv2.RANSAC, 10) (src/heads/NoOpHead.py:75-109) runs after its inlier refit, which minimises the algebraic
 * error only.  Chained after bh_ransac_homography with its mask, H and delta_hat.  The specification below is this project's own: cv2's
 * solver source is not available to this project, so its constants are RECALLED, not copied - 8 free parameters with H22 fixed to 1, at
 * most 10 iterations, lambda starting at 1e-3 and moved by factors of 10 - and cv2 may stop before its tenth iteration where this call
 * never does.  Forward only; all arithmetic in double.
 *   pf[B,2,h,w]      the field, as in bh_ransac_homography
 *   mask[B,h,w]      NULL ok (every pixel).  The correspondences of sample b: every pixel i with mask[b,i] != 0, (x, y) = (i % w, i / w),
 *                    (u, v) = (x + pf[b,0,i], y + pf[b,1,i])
 *   iters            number of steps; every sample runs all of them (fixed work, no early exit, nothing read back by the host).  0 is
 *                    valid: delta_hat of the start and two equal costs
 *   H[B,9]           in: the start; out: the refined homography, fp32 of the double parameters with H[8] = 1 - written only for a sample
 *                    with at least one accepted step, otherwise left as passed in
 *   delta_hat[B,4,2] out: p.corners - corners for corners [[0,0],[w,0],[w,h],[0,h]] from the double parameters p (the corner
 *                    transform of bh_dlt_fwd: the quotient is skipped where |qz| <= 1e-8)
 *   work[B,4]        out (doubles): cost at the start, cost at the result, number of accepted steps, final lambda
 * Parameters p[0..7] = H[0..7] / H[8].  With q = (p0 x + p1 y + p2, p3 x + p4 y + p5, p6 x + p7 y + 1): residuals r = (qx/qz - u,
 * qy/qz - v), cost = sum over the correspondences of rx^2 + ry^2, and the analytic Jacobian J: d rx / d p0..2 = (x, y, 1) / qz,
 * d rx / d p6,7 = -(x, y) (qx/qz) / qz, zero for p3..5; d ry likewise with p3..5 and qy.
 * One step: solve (J^T J + lambda diag(J^T J)) d = -J^T r (8x8, Gaussian elimination with partial pivoting), trial = p + d.  The trial
 * is ACCEPTED iff its cost is finite, every correspondence has qz > 0 at the trial, and cost(trial) < cost(p) - then p = trial and
 * lambda = max(lambda / 10, 1e-12); otherwise p stays and lambda = min(lambda * 10, 1e12).  lambda starts at 1e-3.
 * A sample KEEPS ITS START (H untouched, delta_hat of the start, both costs the start's, zero accepted steps) when it has fewer than
 * 4 correspondences, when a start parameter or the start's cost is not finite, when a correspondence has qz <= 0 at the start, or when
 * the solve of ANY of its steps fails: an elimination pivot with |pivot| <= 1e-12 (or NaN) or a non-finite component of d - the pivot
 * rule of bh_ransac_homography's hypotheses.
 * J^T J, J^T r and the cost are accumulated in double and reduced in a fixed order without floating-point atomics (the 36 unique
 * entries of J^T J are formed from the 19 distinct sums they consist of): two calls agree bit for bit.
 * A field of any size is handled: it is re-read from memory in each of the iters + 1 passes (one launch, one workgroup per sample).
 * BH_E_BADARG: NULL pf / H / delta_hat / work, B < 0, h*w < 4, iters < 0.  BH_E_UNSUPPORTED: B > 65535 or h*w > 2^30.  B == 0: BH_OK,
 * nothing launched.  All checks come before any launch. */
int bh_homography_refine_lm(const float* pf, const uint8_t* mask, int B, int h, int w, int iters, float* H, float* delta_hat,
                            double* work, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Homography warp (warp_image, src/data/utils.py:54-59 -> kornia.warp_perspective(bilinear, zeros,
 * align_corners=True); net map out(x,y) = bilinear img(H.(x,y,1)))  and the warped all-ones mask
 * + AvgPool2d(k) (src/heads/PerceptualHead.py:380-382,401,447-459) fused into the same pass.
 * ------------------------------------------------------------------------------------------- */
/* img[B,C,h,w] (NULL => only the coverage is produced), H64[B,9]; out[B,C,h,w] (may be NULL when
 * img is NULL); cov[B,h/pool,w/pool] (NULL => skipped). h,w positive multiples of 16 and of pool; pool in {1,2,4,8,16,32}
 * (else BH_E_UNSUPPORTED, for all three warp entry points; B == 0: BH_OK, nothing launched).
 * flags: BH_F_DETERMINISTIC (matters for pool = 32) */
int bh_warp_fwd(const float* img, const double* H64, int B, int C, int h, int w, int pool,
                float* out, float* cov, int flags, void* stream);
/* adjoint w.r.t. H only (the image is data): g_out[B,C,h,w] (NULL ok), g_cov[B,h/pool,w/pool]
 * (NULL ok) -> gH[B,9] += (double, atomics; caller zeroes).  flags: BH_F_DETERMINISTIC */
int bh_warp_bwd(const float* img, const double* H64, const float* g_out, const float* g_cov,
                int B, int C, int h, int w, int pool, double* gH, int flags, void* stream);
/* Photometric head (src/heads/PhotometricHead.py:29-41, Nguyen et al.'s unsupervised baseline): H_hat = four_point_to_homography(corners,
 * delta_hat, crop=False) (:29-30, src/data/utils.py:7-33), image_warped = warp_image(image_1, H_hat) (:33-35, utils.py:54-59) and the
 * per-sample crop image_warped[b, :, c[0,1]:c[3,1], c[0,0]:c[1,0]] (:38-42) in ONE gather over the crop window only.  Written in patch
 * coordinates: Hp64[B,9] = bh_h4pt_fwd(delta_hat) for the corners [[0,0],[P,0],[P,P],[0,P]], origin[B,2] float = the integer top-left
 * corner (x, y) of each patch; then H_hat.(o + u) = o + Hp.u and out[b,c,j,i] = bilinear img[b,c](origin_b + Hp_b.(i, j, 1)), zero padding
 * outside the Hi x Wi image (kornia.warp_perspective, align_corners=True).  img[B,C,Hi,Wi], out[B,C,P,P]; P a multiple of 16. */
int bh_photo_warp_fwd(const float* img, const double* Hp64, const float* origin, int B, int C, int Hi, int Wi, int P, float* out,
                      int flags, void* stream);
/* adjoint w.r.t. Hp only (image_1 is data): g_out[B,C,P,P] -> gH[B,9] double += (the caller zeroes it; feed to bh_h4pt_bwd).
 * flags & BH_F_DETERMINISTIC: one workgroup per sample is the only writer of gH[b]; otherwise workgroup sums are added with atomics. */
int bh_photo_warp_bwd(const float* img, const double* Hp64, const float* origin, const float* g_out, int B, int C, int Hi, int Wi,
                      int P, double* gH, int flags, void* stream);
/* adjoint w.r.t. the IMAGE (the trained masks of the Zhang baseline are warped, src/heads/TripletHead.py:60,69, and their gradient must
 * reach the mask predictor): g_out[B,C,h,w] -> g_img[B,C,h,w] (overwritten) = transpose of the bilinear gather with the same taps and
 * zero padding.  flags & BH_F_DETERMINISTIC: scratch = bh_warp_bwd_img_scratch_doubles(...) doubles (integer-limb entries); else NULL. */
size_t bh_warp_bwd_img_scratch_doubles(int B, int C, int h, int w, int flags);
int bh_warp_bwd_img(const double* H64, const float* g_out, int B, int C, int h, int w, float* g_img, double* scratch, int flags,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * biHomE triplet L1 reduction (triplet_resnet_loss, double-line / l1 / channel-agnostic / str margin:
 * src/heads/PerceptualHead.py:559-561, 609-665).  Features are NHWC [B,hw,C].
 * Every entry point of the loss family on [B,hw,C] features (bh_triplet_l1_fwd, bh_bihome_loss_bwd, bh_oneline_loss_*, bh_oneline_cos_loss_*,
 * bh_triplet_hinge_*): BH_E_BADARG for a NULL operand, B < 0, hw < 1, rep < 1 or B % rep; BH_E_UNSUPPORTED unless C is a multiple of 4
 * with C / 4 a divisor of 64 or at least 64, and for B > 65535; B == 0 is BH_OK.
 * ------------------------------------------------------------------------------------------- */
/* M1[B,hw] = sum_c |f1w-f2| - sum_c |f1-f2| ; M2[B,hw] = sum_c |f2w-f1| - sum_c |f1-f2| ;
 * numden[B,4] (double) = { sum m1w*m2*M1, sum m1w*m2, sum m2w*m1*M2, sum m2w*m1 } ; m1,m2 NULL => ones.  flags: BH_F_DETERMINISTIC */
int bh_triplet_l1_fwd(const float* f1, const float* f2, const float* f1w, const float* f2w,
                      const float* m1w, const float* m2w, const float* m1, const float* m2,
                      int B, int hw, int C, float* M1, float* M2, double* numden, int flags, void* stream);
/* loss4[4] = { loss, ln1, ln2, ln3 }: ln_k = sum_b num/max(den,1); ln3 = sum_b ||H1 H2 - I||_F^2;
 * loss = ln1 + ln2 + mu*ln3 (PerceptualHead.py:656-665).  B == 0: the sums of nothing, loss4 = { 0, 0, 0, 0 } (B < 0: BH_E_BADARG) */
int bh_bihome_loss_fwd(const double* numden, const double* H1, const double* H2, int B, float mu,
                       float* loss4, void* stream);
/* adjoint of both: g_loss[1] (device scalar) -> g_f1w,g_f2w [B,hw,C] (overwritten), g_m1w,g_m2w
 * [B,hw] (overwritten), gH1,gH2 [B,9] double (overwritten) */
int bh_bihome_loss_bwd(const float* g_loss, const float* f1, const float* f2, const float* f1w,
                       const float* f2w, const float* m1w, const float* m2w, const float* m1,
                       const float* m2, const float* M1, const float* M2, const double* numden,
                       const double* H1, const double* H2, int B, int hw, int C, float mu,
                       float* g_f1w, float* g_f2w, float* g_m1w, float* g_m2w,
                       double* gH1, double* gH2, void* stream);

/* One-line variant (iHomE; triplet_resnet_loss 'one-line' / l1 / numeric margin: PerceptualHead.py:465-538):
 *   loss = sum_b [ sum_p w max(|f1w-f2|_1 - |f1-f2|_1 + margin, 0) / max(sum_p w, 1) ],  w = m1w * m2 (m2 NULL => ones)
 * T[B,hw] = pre-hinge value (kept for the adjoint), numden[B,2] double, loss[1]. */
/* Multi-hypothesis form (RANSAC_HYPOTHESIS_NO = rep > 1, PerceptualHead.py:352-361,505-511): B counts hypotheses
 * (samples * rep); f1, f2, m2 hold one entry per SAMPLE (row b / rep), f1w / m1w / T one per hypothesis; sample_w[B]
 * (NULL = 1) = DSAC score of the hypothesis, loss = sum_b sample_w[b] * loss_b; per_sample[B] (NULL ok) = loss_b.
 * flags: BH_F_DETERMINISTIC */
int bh_oneline_loss_fwd(const float* f1, const float* f2, const float* f1w, const float* m1w, const float* m2, int B, int hw,
                        int C, float margin, int rep, const float* sample_w, float* T, double* numden, float* per_sample,
                        float* loss, int flags, void* stream);
/* adjoint: g_loss[1] -> g_f1w[B,hw,C], g_m1w[B,hw] (overwritten); d loss / d sample_w[b] = g_loss * per_sample[b] */
int bh_oneline_loss_bwd(const float* g_loss, const float* f2, const float* f1w, const float* m1w, const float* m2,
                        const float* T, const double* numden, int B, int hw, int C, int rep, const float* sample_w,
                        float* g_f1w, float* g_m1w, void* stream);
/* One-line variant with TRIPLET_DISTANCE 'cosine' (src/heads/PerceptualHead.py:485-499, the hinge :505, the scores :508-511):
 *   c(x, y) = sum_c x_c y_c / (max(|x|_2, eps) max(|y|_2, eps)), eps = 1e-8 (torch.cosine_similarity: each norm is clamped on its own;
 *   a zero vector gives c = 0 and receives the gradient y_hat / eps)
 *   t = c(f1, f2) - c(f1w, f2) + margin  ( = (1 - c1w) - (1 - c13) + margin );  loss as bh_oneline_loss_fwd with this t.
 * Arguments, outputs (T = t before the hinge), the multi-hypothesis form, flags and the batch sum are those of bh_oneline_loss_fwd / _bwd.
 * fp32 per pixel (sqrtf and division), double across pixels.  The adjoint recomputes f1w.f2, |f1w|^2 and |f2|^2 from the two maps it
 * reads anyway; as in torch only the VALUE of a norm is clamped - its gradient f1w / |f1w| is taken wherever |f1w| > 0. */
int bh_oneline_cos_loss_fwd(const float* f1, const float* f2, const float* f1w, const float* m1w, const float* m2, int B, int hw,
                            int C, float margin, int rep, const float* sample_w, float* T, double* numden, float* per_sample,
                            float* loss, int flags, void* stream);
int bh_oneline_cos_loss_bwd(const float* g_loss, const float* f2, const float* f1w, const float* m1w, const float* m2,
                            const float* T, const double* numden, int B, int hw, int C, int rep, const float* sample_w,
                            float* g_f1w, float* g_m1w, void* stream);
/* biHomE with a numeric margin and TRIPLET_AGGREGATION 'channel-aware' (double-line / l1: src/heads/PerceptualHead.py:624-625, 644-645) -
 * the hinge inside the channel sum, the same margin in both directions:
 *   M1[B,hw] = sum_c max(|f1w_c - f2_c| - |f1_c - f2_c| + margin, 0) ; M2[B,hw] = sum_c max(|f2w_c - f1_c| - |f1_c - f2_c| + margin, 0)
 * numden[B,4] as bh_triplet_l1_fwd (flags: BH_F_DETERMINISTIC); bh_bihome_loss_fwd turns it into the loss.  The adjoint is
 * bh_bihome_loss_bwd's with g_f1w_c = k [t1_c > 0] sgn(f1w_c - f2_c): the per-channel indicator is recomputed (each direction reads
 * three maps), nothing of size [B,hw,C] is stored. */
int bh_triplet_hinge_fwd(const float* f1, const float* f2, const float* f1w, const float* f2w, const float* m1w,
                         const float* m2w, const float* m1, const float* m2, int B, int hw, int C, float margin, float* M1,
                         float* M2, double* numden, int flags, void* stream);
int bh_triplet_hinge_bwd(const float* g_loss, const float* f1, const float* f2, const float* f1w, const float* f2w,
                         const float* m1w, const float* m2w, const float* m1, const float* m2, const float* M1,
                         const float* M2, const double* numden, const double* H1, const double* H2, int B, int hw, int C,
                         float margin, float mu, float* g_f1w, float* g_f2w, float* g_m1w, float* g_m2w, double* gH1,
                         double* gH2, void* stream);
/* Zhang et al. content-aware triplet loss (TripletHead.forward, src/heads/TripletHead.py:75-152) on ONE-channel full-resolution feature
 * maps f*[B,hw] (the ContentAware feature extractor, src/backbones/ContentAware.py:57-81) and masks m*[B,hw] (m1 / m2 NULL = ones: FIX_MASK):
 *   num1 = sum_p m1w m2 h(|f1w - f2| - |f1 - f2| + margin), den1 = sum_p m1w m2; num2 / den2 with (f2w, f1, m2w m1); f2w NULL: one line.
 * hinge != 0: h = max(., 0) (numeric margin, :98-107); hinge == 0: h = identity and margin is ignored (string margin, :92-97).
 * T1 / T2[B,hw] = pre-hinge values (for the adjoint), numden[B,4] double (overwritten) -> bh_bihome_loss_fwd gives ln1 + ln2 + mu ln3
 * (:150-152; one line: pass identity homographies and mu = 0).  The adjoint writes the gradients of ALL FOUR feature maps (the extractor
 * is trainable here) and of the two warped masks (overwritten), and on request those of the UNWARPED masks (trained masks, FIX_MASK False:
 * m2 weights line 1, m1 line 2): g_m1 / g_m2[B,hw] overwritten, NULL = not wanted (the masks are constants). */
int bh_zhang_triplet_fwd(const float* f1, const float* f2, const float* f1w, const float* f2w, const float* m1w, const float* m2w,
                         const float* m1, const float* m2, int B, int hw, float margin, int hinge, float* T1, float* T2, double* numden,
                         void* stream);
int bh_zhang_triplet_bwd(const float* g_loss, const float* f1, const float* f2, const float* f1w, const float* f2w, const float* m1w,
                         const float* m2w, const float* m1, const float* m2, const float* T1, const float* T2, const double* numden, int B,
                         int hw, int hinge, float* g_f1, float* g_f2, float* g_f1w, float* g_f2w, float* g_m1w, float* g_m2w,
                         float* g_m1, float* g_m2, void* stream);
/* Trained content masks (src/backbones/ContentAware.py:24-26,28-35,47-50,128-134) after the mask predictor's last BatchNorm y[N,P]
 * (P = h w pixels of a one-channel map): s = sigmoid(y); strength > 0: m = clamp(s / (max_p s * strength), 0, 1) (per-sample maximum),
 * else m = s; g = m * f (f, g NULL: the mask only).  smax[N] / imax[N]: the maximum of s and its first pixel (kept for the adjoint).
 * Adjoint: g_m (gradient of the mask from the head, NULL = none) and g_g (gradient of g from the resnet, NULL = none) -> g_y and g_f
 * (NULL = not wanted); the maximum's gradient goes to pixel imax (torch: max(1)[0] backward).  One workgroup per sample, no atomics. */
int bh_mask_fwd(const float* y, const float* f, int N, int P, float strength, float* m, float* g, float* smax, int* imax, void* stream);
int bh_mask_bwd(const float* y, const float* f, const float* m, const float* smax, const int* imax, const float* g_m, const float* g_g,
                int N, int P, float strength, float* g_y, float* g_f, void* stream);
/* y[b,:] = x[b / rep,:] * s[b] over Bn hypotheses of L floats (the score weighting of multihead_resnet_loss,
 * PerceptualHead.py:276-280) and its adjoint (g_x only for rep = 1, may be NULL; g_s[Bn] overwritten; flags: BH_F_DETERMINISTIC). */
int bh_scale_samples_fwd(const float* x, const float* s, int Bn, long long L, int rep, float* y, void* stream);
int bh_scale_samples_bwd(const float* g_y, const float* x, const float* s, int Bn, long long L, int rep, float* g_x, float* g_s,
                         int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Trainable projection head on the perceptual features (AuxiliaryResnet WITH_PROJECTION_HEAD, src/heads/PerceptualHead.py:41-48,
 * 69-74; csrc/proj.hip).  Its Linear layers run as 1x1 convs (bh_conv_fwd_act / bh_conv_dgrad / bh_conv_wgrad); below is the rest.
 * C of every map: the loss kernels' set (a multiple of 4 with C / 4 a divisor of 64 or at least 64, else BH_E_UNSUPPORTED).  No atomics:
 * every output element has one writer and a fixed summation order (bitwise repeatable in every mode).
 * --------------------------------------------------------------------------------------------- */
/* The L2 normalisation over channels of the one-line loss (src/heads/PerceptualHead.py:470-479, 487-496: x / torch.norm(x, p=2, dim=1)):
 *   y[M,C] = x / |x|_2 per pixel, inv[M] = 1 / |x|_2.  No epsilon, as upstream: a zero vector gives NaN in y and in the gradients.
 * adjoint: gx = inv (g - y (y . g)). */
int bh_l2norm_fwd(const float* x, int M, int C, float* y, float* inv, void* stream);
int bh_l2norm_bwd(const float* g, const float* y, const float* inv, int M, int C, float* gx, void* stream);
/* The adjoint of the nn.ReLU between two projection layers (src/heads/PerceptualHead.py:46-47): gx[n] = gy [y > 0], y the ReLU's
 * OUTPUT; n a multiple of 4. */
int bh_relu_bwd(const float* gy, const float* y, long long n, float* gx, void* stream);
/* The gradient of the one-line loss (bh_oneline_loss_fwd, cosine = 0: src/heads/PerceptualHead.py:481-482; bh_oneline_cos_loss_fwd,
 * cosine = 1: :498-499; hinge, scores and masks :505-538) w.r.t. the UNWARPED maps - what bh_oneline_loss_bwd / _cos_loss_bwd leave out
 * because a frozen extractor has no use for it.  Arguments as the forward's (B hypotheses = samples * rep, T and numden its outputs);
 *   k_q = [T_q > 0] g_loss sample_w_q m1w_q m2 / max(den_q, 1)      (the existing adjoint's k), q = b rep + h
 *   l1:      g_f1[b] = - sum_h k_q sgn(f1 - f2)           g_f2[b] = sum_h k_q (sgn(f1 - f2) - sgn(f1w_q - f2))
 *   cosine:  g_f1[b] = sum_h k_q dc(f1, f2)/df1           g_f2[b] = sum_h k_q (dc(f1, f2)/df2 - dc(f1w_q, f2)/df2)
 * g_f1, g_f2 [B / rep, hw, C] (overwritten): per SAMPLE, the hypotheses added in the order h = 0 .. rep - 1 by one thread.  The cosine
 * form keeps bh_oneline_cos_loss_bwd's convention: the value of a norm is clamped at 1e-8, its gradient is not and is 0 at the zero
 * vector. */
int bh_oneline_anchor_bwd(const float* g_loss, const float* f1, const float* f2, const float* f1w, const float* m1w, const float* m2,
                          const float* T, const double* numden, int B, int hw, int C, int rep, const float* sample_w, int cosine,
                          float* g_f1, float* g_f2, void* stream);
/* The same for the double-line loss (bh_triplet_l1_fwd, hinge = 0: src/heads/PerceptualHead.py:559-561, 617-620; bh_triplet_hinge_fwd,
 * hinge = 1: :624-625, 644-645; masks and sums :631-657): ka = g_loss m1w m2 / max(den1, 1), kb = g_loss m2w m1 / max(den2, 1),
 *   g_f1 = - ka I1 sgn(f1 - f2) - kb I2 (sgn(f2w - f1) + sgn(f1 - f2))      g_f2 = ka I1 (sgn(f1 - f2) - sgn(f1w - f2)) + kb I2 sgn(f1 - f2)
 * with I1 = I2 = 1, or per channel the forward's indicators [|f1w - f2| - |f1 - f2| + margin > 0], [|f2w - f1| - |f1 - f2| + margin > 0].
 * numden[B,4] the forward's; m1 / m2 may be NULL (= 1); g_f1, g_f2 [B,hw,C] overwritten.  Elementwise. */
int bh_bihome_anchor_bwd(const float* g_loss, const float* f1, const float* f2, const float* f1w, const float* f2w, const float* m1w,
                         const float* m2w, const float* m1, const float* m2, const double* numden, int B, int hw, int C, float margin,
                         int hinge, float* g_f1, float* g_f2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Conv stacks (Rethinking._forward src/backbones/Rethinking.py:284-294 with blocks
 * src/backbones/utils.py:60-131; ResNet34 src/backbones/ResNet34.py:15-28; AuxiliaryResnet.forward
 * src/heads/PerceptualHead.py:50-76).  Replace ATen conv2d / conv_transpose2d / batch_norm / relu /
 * max_pool2d / adaptive_avg_pool2d / linear and their autograd adjoints.  Implicit GEMM on the
 * f32-input MFMA (v_mfma_f32_32x32x2_f32): exact fp32 products, fp32 accumulate.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int N, Hi, Wi, Ci;      /* input  NHWC */
    int Ho, Wo, Co;         /* output NHWC */
    int kh, kw, stride, pad;
    int transposed;         /* 0: Conv2d ; 1: ConvTranspose2d with kernel == stride, pad 0 */
    int in_nchw;            /* 1: x is NCHW (only for the network inputs, Ci <= 4) */
    int out_nchw;           /* 1: y is NCHW (only for the network output, Co <= 4) */
    int precision;          /* 0: exact fp32 MFMA (v_mfma_f32_32x32x2_f32); 1: operands rounded to bf16 while staging,
                             * fp32 accumulate (v_mfma_f32_32x32x16_bf16), tensors stay fp32 in HBM; 2 ("f32x3"): fp32
                             * accuracy on the bf16 matrix pipe - every fp32 operand is cut EXACTLY into three bf16 pieces
                             * and the six partial products of order <= 2 are accumulated in fp32 (what is dropped is
                             * below 2^-23 of a product, one fp32 rounding); taken by the halo-tiled 3x3 kernel with
                             * w_layout 2, every other kernel computes precision 2 as precision 0;
                             * 3 ("f32x2", REDUCED precision, reported separately): two bf16 pieces per operand, both rounded to
                             * nearest (x = hi + mid + e, |e| <= 2^-18 |x|), products hi*hi + hi*mid + mid*hi (~4e-6 per
                             * product: 13x the fp32 rounding, 500x below precision 1); same kernels as 2 with w_layout 3;
                             * 4 ("f16x2", round 4: fp32 accuracy at three products): two FP16 pieces per operand of the operand times
                             * a power-of-two scale per tensor (x 2^k = hi + lo + e, 11 + 11 significand bits and a sign: |e| <= 2^-23
                             * of the element down to 2^-18 of the tensor's largest magnitude, an absolute 2^-40 of it below), products
                             * hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 (~2^-22 per product: 16x below precision 3, one or two
                             * fp32 roundings), results rescaled exactly.  The scales come from MAGNITUDE RECORDS (a_bound / b_bound
                             * below); same kernels as 3 with w_layout 4; the weight gradient without both records runs as precision 2 */
    int w_layout;           /* 0: w is [Co][kh][kw][Ci].  2: as 1, made with bh_pack3x3_job.split = 1 (three bf16 pieces, 6 bytes
                             * per weight; requires precision 2).  3: as 1, made with split = 2 (two rounded bf16 pieces, 4 bytes
                             * per weight; requires precision 3).  4: as 1, made with split = 3 by bh_conv3x3_pack_f16 (two fp16 pieces
                             * and the weights' maxima; requires precision 4 and a_bound).  1 (3x3 / stride 1 / pad 1 only): w is the fragment-ordered copy made
                             * by bh_conv3x3_pack - its `pf` buffer for bh_conv_fwd*, its `pd` buffer for bh_conv_dgrad* -
                             * which the halo-tiled 3x3 kernel streams straight into registers; BH_E_UNSUPPORTED when
                             * that kernel does not take the launch (ask bh_conv_variant first) */
    int route;              /* 0: automatic kernel choice (production).  BH_ROUTE_* bits: explicit per-call routing for
                             * tests and benchmarks (e.g. drive the halo-tiled 3x3 kernel on a grid it would decline) */
    /* precision 4 only (NULL otherwise; the only per-call members of the descriptor): magnitude records (BH_AMAX_FLOATS floats each,
     * device memory) of the operand tensors - a_bound: the tensor the launch convolves (x for forward / weight gradient - of the
     * BatchNorm OUTPUT for the *_bnin forms -, gy for dgrad); b_bound: gy of the weight gradient.  A record holds an upper bound
     * of max |element| as the maximum over its 16 slots (one per 128-byte line; non-negative floats): written by bh_absmax, by the
     * amax outputs of the BatchNorm entry points (measured) or by bh_bn_fwd_coeffs (|gamma| sqrt(rows) + |beta|).  A bound
     * that is too small overflows fp16 (inf / NaN in the result, never a silently wrong value); one that is too large by 2^j
     * costs j of the 18 binades of full precision.
     * Error per product a b of the two-piece form (csrc/common.h F16X2; held by tests/test_value_regimes_gpu.py on a gradient that is
     * nonzero in one pixel, where every entry of the weight gradient is a single product):
     *   |err| <= 1.25 * 2^-21 |a b| + 2^-39 (|a| bound_b + |b| bound_a)
     * (2^-23 per operand's cut, 2^-22 for the dropped lo x lo, one fp32 rounding; the second term is the absolute floor of elements below
     * 2^-18 of their tensor's record).  The fp32-input MFMA rounds a single product once, 2^-24: "no worse than 1.5 x the fp32-input
     * MFMA kernel's error" is a statement about sums of 64 or more products, whose fp32 accumulation rounding dominates both forms. */
    const float* a_bound;
    const float* b_bound;
} bh_conv_desc;
#define BH_AMAX_FLOATS 512        /* 16 slots x 32 floats (csrc/common.h BH_AMAX_*) */
/* record[slot] = max(record[slot], max |x[i]|) over n floats: the record must be zeroed (or hold an earlier bound to be combined with).
 * One streaming pass: the fallback where no producer kernel left a record. */
int bh_absmax(const float* x, long long n, float* record, void* stream);
#define BH_ROUTE_GENERIC_CONV 1   /* fwd / dgrad: never the halo-tiled 3x3 kernel (generic implicit GEMM) */
#define BH_ROUTE_HALO_SMALL 2     /* fwd / dgrad: let the halo-tiled 3x3 kernel take grids below its workgroup minimum */
#define BH_ROUTE_NO_STEM7 4       /* fwd: never the dedicated 7x7/2 stem kernel */
#define BH_ROUTE_WGRAD_GENERIC 8  /* wgrad: generic split-K kernel instead of the stride-1 fast path */
#define BH_ROUTE_WGRAD_3TAP 16    /* wgrad: three taps per workgroup in the stride-1 fast path */
#define BH_ROUTE_C3_ONE_SUBTILE 32  /* fwd / dgrad: halo-tiled 3x3 kernel with one 8x8 sub-tile per workgroup (64-channel tile) */
#define BH_ROUTE_C3_ONE_POSITION 64 /* fwd / dgrad: halo-tiled 3x3 kernel never walks two tile positions per workgroup */
#define BH_ROUTE_DETERMINISTIC 128  /* every launch of this call is order-independent (see "Deterministic calls" above) */
#define BH_ROUTE_C3_PC 512          /* fwd / dgrad, precision 4, 64-channel tile: the persistent producer / consumer kernel for every launch it supports
                                     * (default: only where it is the faster one) */
#define BH_ROUTE_C3_TILE_WG 256     /* fwd / dgrad, precision 4: the one-workgroup-per-tile halo kernel instead of the persistent producer /
                                     * consumer kernel (round 5) - same convolution results bit for bit */
#define BH_ROUTE_WX3_PC 1024        /* wgrad, precision 4, 64-channel blocks: the EIGHT-wave producer / consumer form of wgrad_x3_kernel (bitwise the
                                     * four-wave result).  Faster alone (-2 us per launch); the default four-wave form leaves 200 registers per
                                     * SIMD lane to co-resident kernels of a second stream, which is worth more in a two-stream step (round 5) */
#define BH_ROUTE_WX3_SHARED 2048    /* wgrad, split-operand 3x3 kernels: the launch shares the GPU with another stream - 160 workgroups instead of one
                                     * per CU (fewer, longer workgroups: the other stream's launches start at once on the free CUs, and the split-K
                                     * partial blocks shrink with the workgroup count).  Same-box in-step A/B, round 5: -0.19 ms per two-stream step */
#define BH_ROUTE_GEMM_X3 4096       /* fwd / dgrad, precision 2 / 4, round 6: layers that run on the generic implicit-GEMM kernel (strided and 1x1 convs,
                                     * 128- / 256-channel transposed convs, their dgrads) cut their operands exactly into three bf16 pieces and make six
                                     * products per product (the arithmetic of the f32x3 3x3 kernels) instead of running the fp32-input MFMA: error against
                                     * float64 <= the fp32-input MFMA's (tests/test_conv_kernels_gpu.py), those launches ~10 % shorter, the step 0.05 ms.
                                     * Opt-in: without it these layers are bit-identical to precision 0. */

/* One 3x3 layer's weights for bh_conv3x3_pack: w[Co][3][3][Ci] (Co, Ci multiples of 32) -> pf (forward operand order) and
 * pd (dgrad operand order: transposed, taps flipped), Co*9*Ci floats each (split: 1.5x that); either may be NULL. */
typedef struct {
    const float* w;
    float* pf;
    float* pd;
    int Co, Ci;
    int split;              /* 0: fp32 fragments (w_layout 1).  1: three bf16 pieces per weight (w_layout 2): pf / pd then hold
                             * Co*9*Ci*6 bytes each.  2: two rounded bf16 pieces (w_layout 3): Co*9*Ci*4 bytes each.  3: two fp16
                             * pieces of w 2^k (w_layout 4; bh_conv3x3_pack_f16): Co*9*Ci*4 + 64 bytes each - the last 64 bytes hold
                             * sixteen partial maxima of |w|, from which the pack and every consumer derive k */
    int reserved;
} bh_pack3x3_job;
/* Packs the weights of njobs layers in one launch (jobs_dev: device array).  Call after every optimizer step (the
 * parameters changed) before the next forward; frozen layers need it once. */
int bh_conv3x3_pack(const bh_pack3x3_job* jobs_dev, int njobs, void* stream);
/* the same for tables with split = 3 jobs: one more launch in front that takes the layers' max |w| */
int bh_conv3x3_pack_f16(const bh_pack3x3_job* jobs_dev, int njobs, void* stream);

/* Which kernel a launch described by d would run: which = 0 forward, 1 dgrad, 2 wgrad, 3 wgrad through a workspace (bh_conv_wgrad_det),
 * 4 / 5 bh_conv_dgrad_bnreduce with the ReLU mask from z / from y (bn_groups = its groups), 6 bh_conv_dgrad_colsum.  Writes the kernel template
 * instantiation (the symbol rocprofv3 lists, e.g. "conv3x3_halo_kernel<false,64,false,2>"; several launches joined by
 * '+') into buf[n].  Runs the real dispatch code with the launches replaced by a name record, so it cannot drift from it.
 * accumulate / bn_groups (0: plain bh_conv_fwd, > 0: bh_conv_fwd_bnstats with that many groups) mirror the arguments of
 * the call being described (they influence routing). */
int bh_conv_variant(const bh_conv_desc* d, int which, int accumulate, int bn_groups, char* buf, int n);

#ifdef BH_TUNING
/* ablation / tuning hook of the -DBH_TUNING build (tools/ only; process-global state) */
int bh_debug_force_tile(int bm, int bn);
#endif
/* y = conv(x, w) (+ bias[Co] if bias != NULL) */
int bh_conv_fwd(const float* x, const float* w, const float* bias, float* y, const bh_conv_desc* d, void* stream);
/* bh_conv_fwd on the generic implicit-GEMM kernel (Conv2d of any geometry, ConvTranspose2d with k == s) that also leaves the magnitude
 * record of its output: amax_y (BH_AMAX_FLOATS floats, zeroed by the caller) receives max |y| - what the fp16-piece 3x3 kernels (precision 4)
 * need of their source tensor; round 4: the transposed convs in front of the decoder units' 3x3 convs (their outputs were measured by a
 * separate bh_absmax pass, 4 launches of 25-55 us per step). */
int bh_conv_fwd_amax(const float* x, const float* w, const float* bias, float* y, const bh_conv_desc* d, float* amax_y, void* stream);

/* y = act(conv(x, w) + bias + res): res (NULL ok) has the layout of y, relu != 0 applies max(.,0).  The inference path:
 * an eval-mode BatchNorm is folded into (w, bias) by the host and its ReLU / residual add ride in the conv epilogue. */
int bh_conv_fwd_act(const float* x, const float* w, const float* bias, const float* res, float* y, const bh_conv_desc* d,
                    int relu, void* stream);
/* BatchNorm-on-load (f32x3 3x3 layers, round 2): x is the INPUT of a training-mode BatchNorm(+ReLU) whose output this convolution
 * is the only consumer of; the kernels apply y = max(x * scale + shift, relu ? 0 : -inf) per channel while staging their operand
 * (zero padding stays zero), so the BatchNorm's output tensor is never written or read.  table[groups][C] x (scale, shift) comes from
 * bh_bn_fwd_coeffs (which also makes the running-statistics update); the images of x are `groups` equal stacks along N.
 * bh_conv_fwd_bnin: packed f32x3 forward (w_layout 2), optional BatchNorm sums of ITS output as in bh_conv_fwd_bnstats (sums NULL: none);
 * bh_conv_wgrad_bnin: the f32x3 weight gradient (workspace form) with the same transform on x.  BH_E_UNSUPPORTED when the launch is
 * not taken by those kernels (ask bh_conv_variant; table > 4 KB). */
typedef struct {
    const float* table;
    int groups;
    int relu;
} bh_bn_in;
/* amax_y (NULL ok): the magnitude record of the BatchNorm's OUTPUT (what the *_bnin consumers convolve): the a-priori bound
 * max_c 2 (|gamma_c| sqrt(rows) + |beta_c|) - a normalised sample is at most sqrt(rows - 1) standard deviations from its mean. */
int bh_bn_fwd_coeffs(const double* stats, const float* gamma, const float* beta, float* running_mean, float* running_var, int groups,
                     int rows, int C, float eps, float momentum, float* table, float* amax_y, void* stream);
int bh_conv_fwd_bnin(const float* x, const float* w, const float* bias, float* y, const bh_conv_desc* d, double* sums, int groups,
                     const bh_bn_in* bni, void* stream);
int bh_conv_wgrad_bnin(const float* x, const float* gy, float* gw, float* gbias, const bh_conv_desc* d, float* ws, long long ws_bytes,
                       const bh_bn_in* bni, void* stream);
/* y = conv(x, w) + bias, and sums (bh_bn_stats_doubles(groups, Co) doubles, caller-zeroed) += per-channel (sum y, sum y^2) of each of the
 * `groups` sub-batches stacked along N: the batch statistics of the BatchNorm that follows, accumulated in the conv
 * epilogue (halo-tiled 3x3 kernel; generic implicit GEMM incl. ConvTranspose2d when the pixels of a group are a
 * multiple of 128; one extra statistics launch otherwise).  Pass the buffer to bh_bn_fwd with flags bit3.  NHWC output. */
int bh_conv_fwd_bnstats(const float* x, const float* w, const float* bias, float* y, const bh_conv_desc* d, double* sums,
                        int groups, void* stream);
/* gx = conv^T(gy, w)  (overwritten; accumulate != 0: gx += ..., used where gradient branches join).
 * d->in_nchw: gx is written NCHW (gradient w.r.t. an NCHW network input; no accumulate, not transposed). */
int bh_conv_dgrad(const float* gy, const float* w, float* gx, const bh_conv_desc* d, int accumulate, void* stream);
/* dgrad of a stride-2 conv (3x3 pad 1 or 1x1 pad 0, even Hi/Wi, NHWC) by output parity class: four dense stride-1
 * launches on class-packed weights instead of one adjoint gather that multiplies 3/4 zeros.  wpack: scratch of
 * Co*kh*kw*Ci floats (rewritten by every call).  BH_E_UNSUPPORTED for any other geometry (use bh_conv_dgrad). */
int bh_conv_dgrad_s2(const float* gy, const float* w, float* gx, const bh_conv_desc* d, int accumulate, float* wpack,
                     void* stream);
/* The BatchNorm (+ReLU) whose OUTPUT gradient a dgrad produces: z = its input, y = its output (needed for the ReLU mask
 * only when a residual was added; NULL: the mask is recomputed from z), stats = its forward sums (bh_bn_fwd). */
typedef struct bh_bn_reduce {
    const float* z;
    const float* y;
    const double* stats;
    const float* gamma;
    const float* beta;
    float eps;
    int relu;
} bh_bn_reduce;
/* bh_conv_dgrad that also accumulates, in its epilogue, the backward sums of that BatchNorm (sum g*mask, sum g*mask*xhat
 * per group and channel) into `sums` (bh_bn_stats_doubles(groups, Ci) doubles, caller-zeroed): pass them to bh_bn_bwd
 * with flags bit4 and its reduce pass is skipped.  gx must be the FINAL gradient (accumulate = 1 adds to the partial
 * sum already in gx).  Only for shapes the halo-tiled 3x3 kernel takes (3x3, stride 1, pad 1, H, W multiples of 8,
 * Co % 32 == 0, Ci % 32 == 0, fp32 or bf16 operands); BH_E_UNSUPPORTED otherwise and nothing is written. */
int bh_conv_dgrad_bnreduce(const float* gy, const float* w, float* gx, const bh_conv_desc* d, int accumulate,
                           const bh_bn_reduce* bnr, double* sums, int groups, void* stream);
/* bh_conv_dgrad (no accumulate) that also adds, in its epilogue, the per-channel sums of the gradient it writes into
 * `sums` (bh_bn_stats_doubles(1, Ci) doubles, caller-zeroed; entry (0, c, 0) = column sum).  The column sums of a conv's
 * input gradient ARE the bias gradient of the layer that produced that input (ConvTranspose2d + bias in the decoder
 * units, src/backbones/utils.py:60-82): bh_bias_grad_from_sums adds them to gbias[C] and the separate streaming pass of
 * bh_conv_bias_grad over that gradient disappears.  Only where the halo-tiled 3x3 kernel applies (else BH_E_UNSUPPORTED). */
int bh_conv_dgrad_colsum(const float* gy, const float* w, float* gx, const bh_conv_desc* d, double* sums, void* stream);
int bh_bias_grad_from_sums(const double* sums, float* gbias, int groups, int C, void* stream);
/* Second half of the two-step dgrad of the extractor's 7x7/2 stem on a grayscale (Ci = 1) or RGB (Ci = 3, in_nchw) patch:
 * Tm[N*Ho*Wo][ldT] = gy x w^T (one 1x1 bh_conv_fwd launch; column = tap*Ci + c, ldT >= 49*Ci padded)
 * -> gx[N,Ci,Hi,Wi] = col2im(Tm). */
int bh_col2im_c1(const float* Tm, float* gx, const bh_conv_desc* d, int ldT, void* stream);
/* The same dgrad for ONE input channel in one kernel (round 4: no tap table in HBM): gy[N,Ho,Wo,64] NHWC, w[64][7][7][1] -> gx[N,1,2Ho,2Wo]
 * (overwritten).  The frozen extractor's conv1 on a warped patch (src/heads/PerceptualHead.py:52-55,377,398).  BH_E_UNSUPPORTED for other
 * geometries: the caller keeps the two-pass form for those.  No atomics: every image tile has one writer. */
int bh_stem7_dgrad_c1(const float* gy, const float* w, float* gx, const bh_conv_desc* d, void* stream);
/* Round 6: that dgrad WITH the adjoint of the homography warp that produced the extractor's input (src/data/utils.py:54-59 `warp_image`
 * as called by src/heads/PerceptualHead.py:371,392 `_warp`, followed by `auxiliary_resnet` :377,398): the gradient of the warped patch
 * has one consumer - dL/dH - so the thread that sums a pixel's gradient applies the warp's adjoint on the spot (the pixel's bilinear tap,
 * four gathered pixels of the SOURCE patch src[N,1,Hi,Wi], the coverage term of the pool-averaged all-ones mask when g_cov[N,Hi/pool,
 * Wi/pool] is given: PerceptualHead.py:380-382,401,447-459) and gH[N,9] += the nine sums.  Equal to bh_stem7_dgrad_c1 followed by
 * bh_warp_bwd(src, H64, gx, g_cov, N, 1, Hi, Wi, pool, gH) up to the order of the double sums; the 4 Hi Wi-byte gradient image is not
 * written (gx = NULL) or written as before (gx != NULL).  gH accumulates through f64 atomics: deterministic callers
 * (BH_F_DETERMINISTIC) use the two separate calls.  BH_E_UNSUPPORTED as bh_stem7_dgrad_c1, or when pool is not a power of two <= 32. */
int bh_stem7_dgrad_c1_warp(const float* gy, const float* w, float* gx, const bh_conv_desc* d, const float* src, const double* H64,
                           const float* g_cov, int pool, double* gH, void* stream);
/* Round 6: the one-plane 7x7 / 2 stem ON the homography warp of a source patch - `auxiliary_resnet(_warp(patch, H))` of
 * src/heads/PerceptualHead.py:371-377,392-398 (warp_image: src/data/utils.py:54-59) in one launch: y[N,Ho,Wo,64] = conv(warp(src[N,1,Hi,Wi],
 * H64[N,9])) with the fp16-piece stem kernel (d->precision = 4) making the warped pixels while it fetches its patches; warped[N,1,Hi,Wi]
 * (the image, as bh_warp_fwd writes it - bitwise) and cov[N,Hi/4,Wi/4] (the pool-averaged warped all-ones mask, :380-382,447-459 - bitwise
 * bh_warp_fwd's) are written on the way, either may be NULL; bn_sums / groups as bh_conv_fwd_bnstats (NULL: no statistics).  Equal to
 * bh_warp_fwd(src, H64, N, 1, Hi, Wi, 4, warped, cov) followed by bh_conv_fwd_bnstats(warped, ...) - bitwise in y as well (the same
 * pixels into the same arithmetic).  BH_E_UNSUPPORTED where the fp16-piece stem does not apply, or pool != 4: the caller makes the two calls. */
int bh_stem7_fwd_warp(const float* src, const double* H64, int pool, const float* w, const float* bias, float* y, const bh_conv_desc* d,
                      float* warped, float* cov, double* bn_sums, int groups, void* stream);
/* Weight gradient of the backbone's 7x7 / 2 stem on TWO stacked image planes (Rethinking.py:31, ResNet34.py:17) in a dedicated kernel
 * (round 4): x[N,2,Hi,Wi] NCHW, gy[N,Ho,Wo,64] NHWC, gw[64][7][7][2] +=.  Partial sums of the persistent workgroups go through the
 * caller's workspace (bh_stem7_wgrad_ws_bytes(d) bytes, 0 = geometry not taken) and are added in workgroup order: no atomics, bitwise
 * repeatable.  bh_conv_wgrad computes the same gradient for every geometry. */
size_t bh_stem7_wgrad_ws_bytes(const bh_conv_desc* d);
int bh_stem7_wgrad(const float* x, const float* gy, float* gw, const bh_conv_desc* d, float* ws, size_t ws_bytes, void* stream);
/* gw += x^T * gy ; gbias += sum gy  (accumulated: caller zeroes; gbias NULL ok) */
int bh_conv_wgrad(const float* x, const float* gy, float* gw, float* gbias, const bh_conv_desc* d, void* stream);
/* Deterministic form of bh_conv_wgrad for the stride-1 "same" 3x3 / 5x5 / 7x7 layers its fast path takes (Co, Ci multiples
 * of 64, power-of-two maps): the split-K workgroups store their partial tiles into ws (bh_conv_wgrad_det_bytes(d) bytes, 0 =
 * shape not supported) and a second launch adds them in a fixed order - bitwise repeatable gw, no fp32 atomics.
 * With precision 2 (f32x3: 3x3 layers, H and W multiples of 8, channels multiples of 64) this is the FAST form - the kernel
 * keeps one 64 x 9 x 64 block per workgroup and storing + reducing <= 256 of them costs less than the atomics tail.
 * BH_E_UNSUPPORTED for other shapes (use bh_conv_wgrad). */
/* In a deterministic call (BH_ROUTE_DETERMINISTIC) every shape has a workspace form (bh_conv_wgrad_det_bytes > 0) and gbias, when given,
 * is accumulated deterministically as well (its entries are the last Co * 32 bytes of the workspace). */
long long bh_conv_wgrad_det_bytes(const bh_conv_desc* d);
int bh_conv_wgrad_det(const float* x, const float* gy, float* gw, float* gbias, const bh_conv_desc* d, float* ws, long long ws_bytes,
                      void* stream);
/* the bias part alone: gbias[Co] += sum of gy over all output pixels (what bh_conv_wgrad does when gbias != NULL) */
int bh_conv_bias_grad(const float* gy, float* gbias, const bh_conv_desc* d, void* stream);

/* Training-mode BatchNorm2d over `groups` independent sub-batches stacked along N (the reference
 * runs the backbone once per direction and the extractor once per patch, each call with its own
 * batch statistics - Rethinking.py:296-313, PerceptualHead.py:358-398 - this build stacks those
 * calls into one launch and keeps the statistics separate per group).  x,y: [groups*rows, C].
 *   stats[groups, C, 2] double = {mean, biased var}; running stats are updated group after group
 *   with `momentum`, unbiased variance, exactly like consecutive nn.BatchNorm2d calls.
 *   flags: bit0 relu, bit1 residual add (y = act(bn(x) + res)), BH_BN_DETERMINISTIC. eval mode: use_running = 1. */
/* stats (forward): bh_bn_stats_doubles() doubles = [groups,C,2] per-channel sums (sum x, sum x^2), each entry on its
 * own 128-byte line (same-line f64 atomics serialise; layout in csrc/common.h).  Accumulated with f64 atomics: MUST BE
 * ZERO on entry unless eval mode; flags bit3 = the sums were already accumulated by bh_conv_fwd_bnstats.  Kept for the
 * adjoint.  scratch (backward): bh_bn_scratch_doubles() doubles, need not be initialised (coefficient table +
 * per-chunk partial sums, reduced deterministically). */
int bh_bn_stats_doubles(int groups, int C);
int bh_bn_scratch_doubles(int groups, int C);
/* groups >= 1, rows >= 1 (else BH_E_UNSUPPORTED, as every shape the BatchNorm entry points do not take).
 * C: a multiple of 4 (4 <= C <= 1024, C/4 dividing 256), or 1 (round 3: the one-channel BatchNorms of the Zhang feature extractor /
 * mask predictor, ContentAware.py:24-26,68-70 - csrc/bn1.hip, same contract; BH_E_UNSUPPORTED with a magnitude record).
 * amax_y (NULL ok; BH_AMAX_FLOATS floats, zeroed by the caller) receives the measured max |y| (precision 4 consumers).
 * Arithmetic of every BatchNorm apply (this entry point, the (scale, shift) table of bh_bn_fwd_coeffs, bh_bn_maxpool_fwd, bh_bn_join_fwd and
 * the masks the adjoints recompute): the sums are float64; mean and 1 / sqrt(var + eps) are rounded to fp32, scale = gamma invstd and
 * shift = beta - mean scale are fp32 operations, y = fma(x, scale, shift).  Against the float64 BatchNorm, per element,
 *   |y - y64| <= 4 * 2^-24 (|x scale| + |mean scale| + |beta| + |y64|)
 * (tests/test_value_regimes_gpu.py, tests/value_regimes.py bn_forward_bound): relative to |mean scale|, not to |shift| - where beta and
 * mean scale cancel the shift carries the rounding of its two terms, as torch's float32 BatchNorm does; on a channel with
 * |mean| / sigma = 2^10 that is 6e-5 absolute on outputs of order 1, which a consumer that applies the table on load (bh_conv_fwd_bnin)
 * sees on every input: |out - out64| <= conv(that bound, |w|) + the conv's own rounding. */
int bh_bn_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
              const float* res, float* y, double* stats, int groups, int rows, int C, float eps, float momentum,
              int flags, int use_running, float* amax_y, void* stream);
/* adjoint. gy: grad w.r.t. y; y: the forward output (for the relu mask); x: forward input.
 * -> gx (overwritten), gres (written when non-NULL: = masked gy), ggamma/gbeta += (NULL ok => frozen).
 * flags bit2 (only without residual): recompute the ReLU mask from x (y is not read, may be NULL).
 * flags bit4: `scratch` already holds the gradient sums (bh_bn_stats_doubles() layout) accumulated by
 * bh_conv_dgrad_bnreduce - one launch instead of three.
 * amax_gx (NULL ok; BH_AMAX_FLOATS floats, zeroed by the caller) receives the measured max |gx|.
 * Groups of at most 4 rows (training mode, with or without flags bit4; bh_bn_join_fwd / _bwd / _remask likewise): evaluated in double
 * from the rows themselves - over two rows the input gradient is the residue eps / (var + eps) of a cancellation that fp32 cannot hold.
 * The fused forms bh_bn_maxpool_fwd / _bwd and bh_bn_bwd_from_1x1 have no such evaluation: groups of at most 4 rows are
 * BH_E_UNSUPPORTED there (the unfused calls take them). */
int bh_bn_bwd(const float* gy, const float* y, const float* x, const float* gamma, const float* beta, const double* stats,
              float* gx, float* gres, float* ggamma, float* gbeta, double* scratch,
              int groups, int rows, int C, float eps, int flags, int use_running,
              const float* running_mean, const float* running_var, float* amax_gx, void* stream);

/* BatchNorm (+ReLU) + MaxPool2d(3, 2, 1) in one pass (round 4: conv1-bn1-relu-maxpool of the backbone stem, Rethinking.py:31-36, and of the
 * perceptual extractor): x[N,Hi,Wi,C] -> y[N,Ho,Wo,C], idx (one byte per element: window position 0..8 of the first maximum, as
 * bh_maxpool3s2_fwd; NULL ok).  stats / flags / use_running / momentum / amax_y as in bh_bn_fwd (flags: bit0 relu, bit3 sums ready,
 * BH_BN_DETERMINISTIC).  The activation between BatchNorm and pooling is never stored: the adjoint is bh_maxpool3s2_bwd followed by bh_bn_bwd
 * with the mask recomputed from x (flags bit2). */
int bh_bn_maxpool_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y,
                      unsigned char* idx, double* stats, int groups, int N, int Hi, int Wi, int C, float eps, float momentum, int flags,
                      int use_running, float* amax_y, void* stream);
/* Adjoint of bh_bn_maxpool_fwd in one call (round 5): gy[N,Ho,Wo,C] and idx as written by the forward, x the BatchNorm input -> gx[N,Hi,Wi,C]
 * (and ggamma / gbeta +=, NULL ok).  The full-resolution gradient between pooling and BatchNorm is never stored (bh_maxpool3s2_bwd + bh_bn_bwd
 * wrote and re-read it: 850 -> 490 MB on the extractor stem, /root/reference/src/heads/PerceptualHead.py:50-60).  scratch: bh_bn_scratch_doubles
 * doubles; flags: bit0 relu (mask recomputed from x), BH_BN_DETERMINISTIC; use_running / running_* / amax_gx as in bh_bn_bwd.  The sums are
 * chunk partials added in fixed order: bitwise reproducible in either mode. */
int bh_bn_maxpool_bwd(const float* gy, const unsigned char* idx, const float* x, const float* gamma, const float* beta, const double* stats,
                      float* gx, float* ggamma, float* gbeta, double* scratch, int groups, int N, int Hi, int Wi, int C, float eps, int flags,
                      int use_running, const float* running_mean, const float* running_var, float* amax_gx, void* stream);
/* BatchNorm (+ReLU, no residual) adjoint whose output gradient is the dgrad of a 1x1 / stride-1 convolution with KC = 16 or 32 output channels
 * (round 5): gs[groups*rows][KC] is the gradient of THAT CONVOLUTION's output, w[KC][C] its kernel-layout weight ([Co][1][1][Ci]); the
 * BatchNorm's output gradient g = gs w is rebuilt per element in both passes and never stored (the decoder units' BatchNorm + ReLU + 1x1
 * conv, /root/reference/src/backbones/utils.py:60-82).  Equivalent to bh_conv_dgrad (1x1) followed by bh_bn_bwd with flags bit0 | bit2
 * (training mode), up to the summation order of the KC products.  scratch: bh_bn_scratch_doubles; flags: bit0 relu, BH_BN_DETERMINISTIC. */
int bh_bn_bwd_from_1x1(const float* gs, const float* w, int KC, const float* x, const float* gamma, const float* beta, const double* stats,
                       float* gx, float* ggamma, float* gbeta, double* scratch, int groups, int rows, int C, float eps, int flags,
                       float* amax_gx, void* stream);
/* Two-branch join (round 4): y = act(bn_a(xa) + bn_b(xb)), both BatchNorms in training mode with their own statistics tables (already
 * accumulated: by the producers' epilogues or bh_bn_stats-style passes) - the end of ResNet50DeconvBlock / the strided ResNet34ConvBlock
 * (src/backbones/utils.py:60-82, 85-112) without writing the normalised lower branch.  flags: bit0 relu, BH_BN_DETERMINISTIC.  Running
 * statistics of both are updated (NULL: skipped).  amax_y as in bh_bn_fwd.
 * Adjoint: gy, y (ReLU mask), xa, xb -> gxa, gxb (overwritten), ggamma / gbeta of both += (NULL ok); scratch: bh_bn_join_scratch_doubles()
 * doubles; amax_gxa / amax_gxb (NULL ok) receive max |gxa| / max |gxb|.  One reduce pass for the three sums (sum d, sum d xhat_a,
 * sum d xhat_b with d = gy [y > 0]) and one apply pass. */
/* the statistics pass alone: stats (zeroed, bh_bn_stats_doubles() doubles) += per-channel (sum x, sum x^2); flags: BH_BN_DETERMINISTIC */
int bh_bn_stats(const float* x, double* stats, int groups, int rows, int C, int flags, void* stream);
int bh_bn_join_scratch_doubles(int groups, int C);
int bh_bn_join_fwd(const float* xa, const float* xb, const float* gamma_a, const float* beta_a, float* rmean_a, float* rvar_a,
                   const float* gamma_b, const float* beta_b, float* rmean_b, float* rvar_b, const double* stats_a, const double* stats_b,
                   float* y, int groups, int rows, int C, float eps_a, float eps_b, float momentum_a, float momentum_b, int flags,
                   float* amax_y, void* stream);
int bh_bn_join_bwd(const float* gy, const float* y, const float* xa, const float* xb, const float* gamma_a, const float* gamma_b,
                   const double* stats_a, const double* stats_b, float* gxa, float* gxb, float* ggamma_a, float* gbeta_a, float* ggamma_b,
                   float* gbeta_b, double* scratch, int groups, int rows, int C, float eps_a, float eps_b, int flags, float* amax_gxa,
                   float* amax_gxb, void* stream);
/* The same adjoint with the ReLU mask RECOMPUTED from xa, xb (round 5): y is not read - the kernels evaluate the forward kernel's own
 * expression y = fma(xa, sc_a, fma(xb, sc_b, sh_a + sh_b)) with the same coefficient arithmetic, so the mask is bitwise the forward's
 * decision and the result bitwise bh_bn_join_bwd's; one of four input streams less in both passes (1.34 -> 1.07 GB at the full-resolution
 * join of ResNet50DeconvBlock, /root/reference/src/backbones/utils.py:60-82).  beta_a / beta_b: the BatchNorms' shifts (NULL: 0). */
int bh_bn_join_bwd_remask(const float* gy, const float* xa, const float* xb, const float* gamma_a, const float* beta_a, const float* gamma_b,
                          const float* beta_b, const double* stats_a, const double* stats_b, float* gxa, float* gxb, float* ggamma_a,
                          float* gbeta_a, float* ggamma_b, float* gbeta_b, double* scratch, int groups, int rows, int C, float eps_a, float eps_b,
                          int flags, float* amax_gxa, float* amax_gxb, void* stream);

/* Fused tail of the Zeng backbone, `layer8` (src/backbones/Rethinking.py:145-147):
 *   Conv2d(Ci,Cm,1,bias) -> BatchNorm2d(Cm) -> ReLU -> Conv2d(Cm,Co,1,bias), NHWC x[groups*rows,Ci] -> NCHW out[N,Co,h,w]
 * (hw = h*w pixels per image, rows = pixels per group).  The Cm-channel intermediate is never materialised: its batch
 * statistics are derived from the first/second moments of x (a 1x1 conv is linear).  Ci in {8,16}, Cm a multiple of 64 (64 <= Cm <= 256),
 * 1 <= Co <= 4, groups >= 1, hw >= 1 and rows a positive multiple of hw (else BH_E_UNSUPPORTED).  ws: bh_tail_ws_doubles() doubles (kept for the adjoint); scratch: bh_tail_scratch_floats().
 * route, per call (no process state): 0 = the library's choice - round 4: for Ci = 16, Co <= 2, rows % 32 == 0 and
 * hw % 32 == 0 the Ci -> Cm product runs on the matrix pipe in the exact three-bf16-piece arithmetic (tail_fwd_mfma_kernel);
 * bit 0 (BH_TAIL_ROUTE_VALU_FWD) keeps the per-pixel VALU kernel (tests compare the two, tools time them). */
int bh_tail_ws_doubles(int groups, int Ci, int Cm);
int bh_tail_scratch_floats(int groups, int Ci, int Cm);
#define BH_TAIL_ROUTE_VALU_FWD 1
#define BH_TAIL_ROUTE_LDS_MOMENTS 2      /* bit 1: the input moments by the LDS-slab kernel instead of the matrix-pipe one (Ci = 16) */
int bh_tail_fwd(const float* x, const float* w1, const float* b1, const float* gamma, const float* beta,
                float* running_mean, float* running_var, const float* w2, const float* b2, float* out, double* ws,
                int groups, int rows, int hw, int Ci, int Cm, int Co, float eps, float momentum, int use_running,
                int route, void* stream);
/* adjoint: gout[N,Co,h,w] -> gx[groups*rows,Ci] (overwritten, NULL ok); gw1[Cm][Ci], ggamma, gbeta, gw2[Co][Cm], gb2 +=
 * Round 4: pixels whose output gradient is exactly zero are skipped by the reduction (they add exactly zero: on the biHomE path only
 * the DSAC-sampled points of the field carry a gradient), and gx = c0 - M x (the BatchNorm mean terms, an affine map of x made once
 * per group) + the Cm-channel term where the gradient is non-zero.  Dense gradients take the per-lane channel loop as before.
 * flags: BH_F_DETERMINISTIC (the bias gradient gb2) */
int bh_tail_bwd(const float* gout, const float* x, const float* w1, const float* b1, const float* gamma,
                const float* beta, const float* w2, const double* ws, const float* running_mean,
                const float* running_var, float* gx, float* gw1, float* ggamma, float* gbeta, float* gw2, float* gb2,
                float* scratch, int groups, int rows, int hw, int Ci, int Cm, int Co, float eps, int use_running,
                int flags, void* stream);

/* Synthetic pair generator (next-row f1): HomographyNetPrep + PhotometricDistortSimple + DictToGrayscale +
 * DictStandardize of src/data/transforms.py:296-330,344-378,441-725 for B samples in one launch.
 * images[n_images,3,Hs,Ws] float RGB 0..255 (resident); img_idx[B]; origin[B,2] = top-left corner (x0,y0) of the
 * patch; Hpatch[B,9] double = bh_h4pt_fwd(delta) in patch coordinates; photo[B,2,6] = per image of the pair
 * {brightness delta, contrast factor applied before the HSV part, saturation factor, hue delta (degrees), contrast factor
 * applied after the HSV part, channel-permutation index 0..5 into ((0,1,2),(0,2,1),(1,0,2),(1,2,0),(2,0,1),(2,1,0))}
 * (transforms.py:141-245; OpenCV float HSV), or NULL for no distortion.  The distortion is applied to the image before
 * it is warped, as upstream.  patch1 = crop, patch2(x) = image(origin + Hpatch.x) bilinear; both standardised
 * ((gray/255 - mean)/std), [B,1,P,P].  This is bh_synth_batch with C = 1 and no target: the same kernel, the same bits. */
int bh_synth_pairs(const float* images, const int* img_idx, const float* origin, const double* Hpatch, const float* photo,
                   int B, int n_images, int Hs, int Ws, int P, float mean, float std, float* patch1, float* patch2,
                   void* stream);

/* The generator in its general form (same inputs and argument rules as bh_synth_pairs).  C = 1: grayscale patches [B,1,P,P].  C = 3
 * (BASELINE.json configs[4]): patch1 / patch2 are [B,3,P,P], channel c = the permuted, distorted channel c itself, standardised
 * ((v/255 - mean)/std) - no grayscale step; sampling as for C = 1 (bilinear, each tap zero outside the base image, the photometric
 * record applied to the image before the warp).  target: NULL, or [B,2,P,P] = HomographyNetPrep's 'all_points' perspective field
 * (transforms.py:635-685): channel 0 / 1 = x / y of Hpatch.(x,y,1) dehomogenised minus (x,y), evaluated in double from the Hpatch
 * the warp uses and stored as float.  BH_E_BADARG: a NULL required pointer, std == 0, C not 1 or 3; BH_E_UNSUPPORTED: P % 16 != 0. */
int bh_synth_batch(const float* images, const int* img_idx, const float* origin, const double* Hpatch, const float* photo,
                   int B, int n_images, int Hs, int Ws, int P, int C, float mean, float std, float* patch1, float* patch2,
                   float* target, void* stream);

/* image_1 for the photometric head (config/s-coco/nguyen-orig-lr-5e-3.yaml: HomographyNetPrep's image_1 after DictToGrayscale and
 * DictStandardize, transforms.py:344-378): image1[B,1,Hs,Ws] = the whole base image images[img_idx[b]] under image 1's photometric record
 * (photo[b,0,:] of bh_synth_pairs' layout, NULL = none), grayscale, standardised - the same per-pixel arithmetic as bh_synth_pairs'
 * patch1, whose crop at origin it equals bitwise. */
int bh_synth_image(const float* images, const int* img_idx, const float* photo, int B, int n_images, int Hs, int Ws, float mean,
                   float std, float* image1, void* stream);

/* Occlusion blobs of the pair generator: CollatorWithBlobs (src/data/transforms.py:746-799; DATA.AUGMENT_BLOB_POROSITY /
 * AUGMENT_BLOBINESS, train.py:130-136,575-577) for B samples.  noise[B,P,P] uniform in [0,1) and other[B] (int32, the sample whose
 * patch_1 is pasted, 0 <= other[b] < B; an index outside that range is read as b) are inputs: nothing is drawn here.  Per sample:
 * g = Gaussian blur of noise (separable, radius int(4 sigma + 0.5), scipy's 'reflect' border), z = (g - mean) / std (population),
 * u = 0.5 erfc(-z / sqrt 2) min-max normalised to [0,1], blob = u < porosity (what porespy's generators.blobs computes with
 * sigma = P / (40 blobiness); bihome_amd/synth.py blob_field is the float64 restatement).  Outputs, all fully overwritten:
 * mask[B,P,P] = 1.0 / 0.0; field[B,P,P] = u (NULL ok); patch2[B,C,P,P] in place: patch2[b,c] = patch1[other[b],c] where blob, every
 * other element keeps its bits (patch1 is only read).  A flat plane (std == 0 or max == min, where upstream's arithmetic is NaN and
 * selects nothing) gives field 1, mask 0, patch2 untouched.  scratch: bh_synth_blobs_scratch_floats(B, P) floats (0 for P <= 128),
 * need not be initialised.  No atomics: two calls on the same inputs are bitwise equal.
 * BH_E_BADARG: a NULL required pointer, B < 2, C not 1 or 3, sigma not positive and finite, porosity outside [0,1];
 * BH_E_UNSUPPORTED: P % 16 != 0, P > 256, radius > P (blobiness < 0.1: more than one reflection). */
size_t bh_synth_blobs_scratch_floats(int B, int P);
int bh_synth_blobs(const float* noise, const int* other, const float* patch1, float* patch2, float* mask, float* field,
                   float* scratch, int B, int C, int P, double sigma, double porosity, void* stream);

/* Counter-based draws of the pair generator: every random quantity of sample n of a seed is a pure function of (seed, n), whatever the
 * batch size, the rank count or the calls made before.  Sample b of a call is sample first + b of the stream (64-bit, wrapping).
 *
 * The stream.  philox4x64_10(counter[4], key[2]) is the standard 10-round Philox function on 64-bit words (Salmon et al., SC'11):
 * multipliers 0xD2E7470EE14C6C93 on counter[0] and 0xCA5A826395121157 on counter[2]; one round gives {hi1 ^ c1 ^ k0, lo1,
 * hi0 ^ c3 ^ k1, lo0} (hi / lo: the halves of the 128-bit products); between rounds the key grows by (0x9E3779B97F4A7C15,
 * 0xBB67AE8584CAA73B).  Word k (k = 0, 1, ...) of sample n for purpose p is element k % 4 of
 *     philox4x64_10(counter = (k / 4 + 1, n, 0, 0), key = (seed, p)),
 * which is np.random.Philox(key=[seed, p], counter=[0, n, 0, 0]).random_raw(K)[k] (numpy advances its counter before its first block).
 * Maps of a word: an integer in [0, r), r < 2^31, is (word * r) >> 64; a double uniform is (word >> 11) * 2^-53 (numpy's
 * Generator.random()); a float noise value is (word >> 40) * 2^-24.
 *
 * Purpose 0, the sample's parameters:
 *   word 0       img_idx = int(n_images)
 *   words 1, 2   patch centre px = rho + P/2 + int(Ws - 2 rho - 2 (P/2) + 1), py likewise with Hs (transforms.py:505-506);
 *                origin = (px - P/2, py - P/2)
 *   word 3       blob source: r = int(B - 1), other = r + (r >= b) - the only quantity that depends on the batch (B, and the position b)
 *   words 4..11  delta[4,2] row-major: -rho + int(2 rho) (transforms.py:538)
 *   words 12..22 the 11 uniforms of image 1's photometric record, in the column order of bihome_amd.synth_gpu.photometric_records
 *   words 24..34 the same for image 2 (words 23 and 35 are unused)
 * A record is {brightness, contrast-first, saturation, hue, contrast-last, permutation index} (bh_synth_pairs' layout) by
 * photometric_records' formulas - coins u >= 0.5, values lo + (hi - lo) u, the index floor(6 u) clamped to 5, permutation 0 at
 * max_delta == 0 - evaluated in double without contraction and rounded once to float.
 * Purpose 1, blob noise: noise[y, x] = the float map of word y * P + x.
 *
 * Outputs: img_idx[B], origin[B,2] and delta[B,4,2] always; photo[B,2,6] or NULL; noise[B,P,P] and other[B] both or neither.  Every
 * element of every given output is written exactly once and nothing else is touched; no atomics, no scratch: two calls are bitwise
 * equal.  At most two launches (parameters; noise), no allocation, no host synchronisation.  bihome_amd.synth.counter_draws is the
 * same function in numpy, and every output equals it bit for bit.
 * BH_E_BADARG: B < 0, n_images < 1, rho < 1, P < 1, Hs < P + 2 rho, Ws < P + 2 rho, only one of noise / other given; then B == 0:
 * BH_OK, nothing launched; then BH_E_BADARG for a NULL img_idx / origin / delta, and for noise given with B < 2.  Refusals return
 * before any launch. */
int bh_synth_draw(size_t seed, size_t first, int B, int n_images, int Hs, int Ws, int P, int rho,
                  float max_delta, int* img_idx, float* origin, float* delta, float* photo, float* noise, int* other, void* stream);

/* Resident image bank of the pair generator: Dataset.load_image (src/data/coco/dataset.py:95-103: one np.load of a uint8 [H,W,3] RGB
 * array per sample, written by preprocess_offline.py:22) as a gather on the device.  bank[n_images,Hs,Ws,3] uint8, interleaved RGB - the
 * .npy layout, all images of one split in one tensor (82,783 x 240 x 320 x 3 = 19 GB for COCO train2014); img_idx[count] int32;
 * out[count,3,Hs,Ws] float planar, values 0..255: out[b,c,y,x] = (float)bank[img_idx[b],y,x,c] - what bh_synth_batch / bh_synth_image
 * take as `images` (with n_images = count and img_idx = 0..count-1).  Every element of out is overwritten and nothing outside it is
 * touched; no atomics: two calls on the same inputs are bitwise equal.  Every offset is 64-bit (the bank may be far larger than 2^31
 * bytes).  An index outside [0, n_images) is CLAMPED into that range in the kernel (a negative one reads image 0, one >= n_images the
 * last image): nothing outside the bank is ever read.  Hs*Ws % 4 == 0 (every Ws % 4 == 0) with bank on a 4-byte and out on a 16-byte
 * boundary takes the vector path (12-byte loads, float4 stores per plane), anything else a scalar path with the same results.
 * BH_E_BADARG: a NULL pointer, count < 0, n_images < 1, Hs < 1, Ws < 1; count == 0: BH_OK, nothing launched;
 * BH_E_UNSUPPORTED: more than 2^39 pixels per image.  Refusals return before any launch. */
int bh_bank_gather_u8(const unsigned char* bank, const int* img_idx, int count, int n_images, int Hs, int Ws, float* out, void* stream);

/* Filling the bank from raw-size images: Rescale((W, H)) then CenterCrop((W, H)) (src/data/transforms.py:24-46 and :103-122, which
 * preprocess_offline.py runs through cv2.resize one image at a time on the host) for `count` images of DIFFERENT sizes in one launch.
 * src: one packed device buffer of interleaved RGB uint8 images; src_off[count] int64: the byte offset of each image in src;
 * src_hw[count,2] int32: its height and width; bank[n_slots,H,W,3] uint8: image b is written to slot first + b.  Every byte of slots
 * first .. first+count-1 is written exactly once and nothing outside them is touched; no atomics, no scratch: two calls on the same
 * inputs are bitwise equal.  Every byte offset is 64-bit, on the source and on the bank side.  Per image, in double: r = h / w; if
 * r < H / W then (nw, nh) = (round(H / r), H) else (W, round(W r)), round half to even as numpy's; top = (nh - H) / 2,
 * left = (nw - W) / 2; bank pixel (y, x) = resized pixel (y + top, x + left) - the resized image itself is never stored.  The resize is
 * cv2.resize's default, INTER_LINEAR on 8-bit data, AS RECALLED (not read from OpenCV's source, and not compared with cv2):
 * w == 2 nw and h == 2 nh: (s00 + s01 + s10 + s11 + 2) >> 2 over the 2x2 block; (nh, nw) == (h, w): a copy; otherwise two taps per
 * axis at f = (float)((d + 0.5) (n / n_new) - 0.5), s = floor(f), f -= s, both clamped at the borders with f = 0, 11-bit coefficients
 * rint((1 - f) 2048), rint(f 2048), rows S = s[sx] a0 + s[sx+1] a1 in int32, out = (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2.
 * bihome_amd.bank.rescale_center_crop_host is the same arithmetic in numpy, and the kernel equals it bit for bit.
 * src_hw is device memory, so this function cannot see it: an image with h < 1 or w < 1 (or whose resized size does not fit an int)
 * leaves its slot UNTOUCHED, and an offset or size that points outside src is the caller's to exclude (bihome_amd.kernels.bank_ingest_u8
 * checks both on the host before it uploads them).  W % 4 == 0 with bank on a 4-byte boundary takes dword stores, anything else byte
 * stores with the same results.
 * BH_E_BADARG: a NULL pointer, count < 0, n_slots < 1, H < 1, W < 1, first < 0, first + count > n_slots; count == 0: BH_OK, nothing
 * launched; BH_E_UNSUPPORTED: H * W > 2^31 - 1 pixels per bank image.  Refusals return before any launch. */
int bh_bank_ingest_u8(const unsigned char* src, const int64_t* src_off, const int* src_hw, int count, unsigned char* bank, int n_slots,
                      int first, int H, int W, void* stream);

/* Image alignment: a trained model applied to two full-size uint8 images.  Upstream has this only at patch level and on the host
 * (eval.py:249-255 builds four_point_to_homography(corners, delta_hat) and warps with kornia / cv2; src/data/utils.py:54-67 warp_image);
 * the three steps around the model are stated here and, in numpy float64, in bihome_amd/align.py (prep_host, lift, warp_u8_host).
 * INDEX coordinates: pixel j of an image sits at coordinate j and occupies [j - 0.5, j + 0.5) - the convention of csrc/warp_tap.h and of
 * four_point_to_homography.  EDGE coordinates (regions only): pixel i spans [i, i + 1).
 *
 * Preparation (ToGrayscale / DictToGrayscale, src/data/transforms.py:333-354; DictStandardize, :369-378; the resize is new).
 * images[n_images,H,W,3] uint8 interleaved RGB (a bank); idx[B] int32 picks each sample's image (NULL: sample b is image b; CLAMPED into
 * [0, n_images) in the kernel); roi[B,4] double = (x0, y0, rw, rh) in edge coordinates (NULL: the whole image, (0, 0, W, H)).  With
 * sx = rw / P, sy = rh / P, output pixel (y, x) is the exact area average of the source over
 * [x0 + x sx, x0 + (x+1) sx) x [y0 + y sy, y0 + (y+1) sy):
 *     patch[b,c,y,x] = ((1 / (sx sy)) sum_j sum_i ov_y(y,j) ov_x(x,i) v_c(j,i) / 255 - mean) / std,
 * ov the length of the overlap of the output interval with pixel i's unit interval, v = 0.299 R + 0.587 G + 0.114 B for C = 1 and
 * channel c for C = 3: one formula for shrinking, sx = 1 (the standardised image itself) and enlarging.  patch[B,C,P,P] float;
 * geom[b] = (sx, sy, tx, ty) double with tx = x0 + 0.5 sx - 0.5, ty = y0 + 0.5 sy - 0.5: the affine map A from patch index coordinates
 * to image index coordinates (evaluated in double without contraction: the bits of the numpy statement).  Interval ends are double, the
 * overlaps and sums float.  roi is device memory, so this function cannot see it: every source index derived from it is clamped to the
 * image - a wrong region gives wrong pixels, never a read outside the bank (bihome_amd.align.Aligner range-checks regions on the host).
 * The offset of an image in the bank is 64-bit (the bank may be far larger than 2^31 bytes), offsets inside an image 32-bit.  One writer
 * per output element, no atomics: two calls are bitwise equal.
 * BH_E_BADARG: NULL images / patch / geom, B < 0, n_images < 1, H < 1, W < 1, P < 1, std zero or NaN; then BH_E_UNSUPPORTED: C not 1 or
 * 3, P % 16 != 0, P > 256, H * W > 2^30 pixels; then B == 0: BH_OK, nothing launched.  Refusals return before any launch. */
int bh_align_prep_u8(const uint8_t* images, const int* idx, int n_images, int H, int W, const double* roi,
                     int B, int P, int C, float mean, float std, float* patch, double* geom, void* stream);

/* The uint8 warp: out[b,y,x,:] = round_half_up(clamp(bilinear images[idx[b]](H64[b] (x, y, 1)), 0, 255)), taps outside the image
 * contribute 0 - warp_image's net map with zero padding (src/data/utils.py:54-59) on interleaved uint8 RGB.  images[n_images,Hs,Ws,3],
 * idx as above; H64[B,9] double maps index coordinates of the OUTPUT (Ho x Wo) to index coordinates of the source - for the lifted
 * H_img = A_a H_p A_b^-1 (H_p = bh_h4pt_fwd(delta_hat, P), eval.py:252-254; the loss trains patch_1(H_p x) ~ patch_2(x),
 * PerceptualHead.py:371) the source is image A and the output has image B's size.  out[B,Ho,Wo,3] uint8; valid[B,Ho,Wo] uint8 (NULL
 * ok) = 1 where the projected point lies in [0, Ws - 1] x [0, Hs - 1] and the projection guard (|qz| <= 1e-8) did not fire, else 0.
 * The projection and the placement of the taps are csrc/warp_tap.h's (tap_project / tap_place, float), as in every other warp here; the
 * sample of the uint8 image and its valid are csrc/u8_image.h's u8_sample, the one bh_align_prep_warp_u8 and bh_mosaic_u8 call too.
 * Wo % 4 == 0 with out on a 4-byte boundary: four pixels and three dword stores per thread; anything else one pixel and byte stores,
 * same results.  The offset of an image in the bank and every offset into out are 64-bit, offsets inside a source image 32-bit.  One writer per output element, no atomics: two calls are bitwise
 * equal.  BH_E_BADARG: NULL images / H64 / out, B < 0, n_images < 1, Hs < 1, Ws < 1, Ho < 1, Wo < 1; then BH_E_UNSUPPORTED: Hs * Ws
 * > 2^29 or Ho * Wo > 2^31 - 1 pixels; then B == 0: BH_OK, nothing launched.  Refusals return before any launch. */
int bh_warp_u8(const uint8_t* images, const int* idx, int n_images, int Hs, int Ws, const double* H64,
               int B, int Ho, int Wo, uint8_t* out, uint8_t* valid, void* stream);

/* ECC refinement: a photometric polish of the lifted homography on the two images themselves, coarse to fine - the forward-additive
 * enhanced-correlation-coefficient iteration (Evangelidis & Psarakis 2008; what cv2.findTransformECC does on the host), which does not
 * see a gain or a bias between the images.  Fixed work, no early exit, no atomics: two calls give equal bits.  The numpy float64
 * statements are bihome_amd/align.py's gray_pyramid_host, ecc_sums_host, ecc_step_host, ecc_refine_host.  Index coordinates throughout.
 *
 * Pyramid.  Level 0 is g = fmaf(0.114, B, fmaf(0.587, G, 0.299 R)) of the uint8 image (float, 0..255); level l is the 2 x 2 box mean
 * ((a + b) + (c + d)) * 0.25 of level l - 1 and has (h >> 1, w >> 1) pixels (an odd last row / column is dropped); pixel x of level l
 * sits at 2 x + 0.5 of level l - 1, so with C = [[2,0,.5],[0,2,.5],[0,0,1]] a homography moves a level down (finer) as C H C^-1 and up
 * as C^-1 H C, rescaled to H[8] = 1.  pyr[B, total] float holds a sample's levels one after another: bh_gray_pyramid_layout writes
 * offsets[levels + 1] (HOST memory, in floats; offsets[levels] = total).  images / idx / n_images as in bh_align_prep_u8 (idx clamped,
 * 64-bit image offsets).  One writer per element; bitwise a float32 restatement.
 * BH_E_BADARG: a NULL images / pyr / offsets, B < 0, n_images < 1, H < 1, W < 1; then BH_E_UNSUPPORTED: levels outside 1..6, a coarsest
 * level under 8 pixels on a side, H * W > 2^29; then B == 0: BH_OK, nothing launched.  Refusals return before any launch. */
#define BH_ECC_SUMS 66
#define BH_ECC_STATE 24
int bh_gray_pyramid_layout(int H, int W, int levels, int64_t* offsets);
int bh_gray_pyramid_u8(const uint8_t* images, const int* idx, int n_images, int H, int W, int B, int levels, float* pyr, void* stream);

/* One pass at one level.  a: B gray planes Ha x Wa of image A, a_stride floats apart; t: B planes Hb x Wb of image B, t_stride floats
 * apart; mask[B,Hb,Wb] uint8 (NULL ok); H64[B,9] double maps t's index coordinates to a's and is used as H / H[8].  For every pixel
 * (x, y) of t: q = H (x, y, 1), (u, v) = (qx, qy) / qz by csrc/warp_tap.h's tap_project / tap_place - the taps bh_warp_u8 takes.  The
 * pixel COUNTS iff qz > 1e-8, 0 <= u < Wa - 1, 0 <= v < Ha - 1 (all four taps a00 a01 a10 a11 inside a) and its mask byte is non-zero.
 * With the fractions fx, fy: iw = the bilinear value, gx = (1-fy)(a01-a00) + fy(a11-a10), gy = (1-fx)(a10-a00) + fx(a11-a01) (the
 * exact derivative of the interpolant), m = -(gx u + gy v), j = (gx x, gx y, gx, gy x, gy y, gy, m x, m y) / qz = d iw / d H[0..7].
 * sums[B,66] double = the upper triangle, row-major (entry (i, j), i <= j, at 11 i - i (i - 1) / 2 + j - i), of sum z z^T over the
 * counting pixels, z = (j0..j7, iw, t, 1): entry 65 is n, (8,10) sum iw, (9,10) sum t, (8,8) (9,9) (8,9) the second moments, (i,10)
 * sum j_i, (i,8) sum j_i iw, (i,9) sum j_i t.  Per-pixel terms are float and no float accumulator carries more than 16 pixels; beyond
 * that the sums are double.  partial: scratch of bh_ecc_sums_ws_doubles() doubles (written to HOST memory by that query), one block of
 * 66 per workgroup, overwritten, then added in block-index order.
 * BH_E_BADARG: a NULL a / t / H64 / partial / sums (doubles for the query), B < 0, Ha, Wa, Hb, Wb < 1, a stride shorter than its plane;
 * then BH_E_UNSUPPORTED: Ha * Wa or Hb * Wb > 2^29; then B == 0: BH_OK, nothing launched. */
int bh_ecc_sums_ws_doubles(int Hb, int Wb, int B, int64_t* doubles);
int bh_ecc_sums(const float* a, int Ha, int Wa, int64_t a_stride, const float* t, int Hb, int Wb, int64_t t_stride, const uint8_t* mask,
                const double* H64, int B, double* partial, double* sums, void* stream);

/* One step and the books of a level, all double.  With n, the means m_iw = sum iw / n, m_t = sum t / n, |iw'|^2 = sum iw^2 - n m_iw^2,
 * |t'|^2 likewise, <iw',t'> = sum iw t - n m_iw m_t: rho = <iw',t'> / sqrt(|iw'|^2 |t'|^2); G = sum j j^T - (sum j)(sum j)^T / n,
 * a = sum j iw - m_iw sum j, c = sum j t - m_t sum j; G (ya, yc) = (a, c) by 8 x 8 Gaussian elimination with partial pivoting;
 * lambda = (|iw'|^2 - a.ya) / (<iw',t'> - c.ya); d = lambda yc - ya.  The step FAILS for n < 16, a variance not positive, a zero or NaN
 * pivot, a denominator of lambda not > 0, or a d that is not finite.
 * state[B, BH_ECC_STATE] double: 0..8 cur, 9..17 best, 18 rho_best (-inf at the start of a level), 19 frozen (0 / 1), 20 rho at the
 * level's first pass, 21 accepted steps, 22 passes done, 23 unused.  A sample that is not frozen and whose rho rose above rho_best
 * takes best = cur, rho_best = rho and then, if last == 0 and the step did not fail, cur[0..7] += d, cur[8] = 1 - else it freezes; one
 * whose rho did not rise (or is NaN) takes cur = best and freezes; a frozen sample changes nothing.  last = 1, the level's final pass:
 * cur = best, and stats (NULL ok; sample b at stats + b * stats_stride) = (rho first, rho_best, accepted steps).  last = 2: as 1, then
 * cur = best = C cur C^-1 (a level down) with the books reset.
 * BH_E_BADARG: a NULL sums / state, B < 0, last outside 0..2, stats with stats_stride < 3; B == 0: BH_OK, nothing launched. */
int bh_ecc_step(const double* sums, double* state, int B, int last, double* stats, int stats_stride, void* stream);

/* The whole refinement on one stream, without allocation or host synchronisation (capturable): H64[B,9] (in: the start at level 0, out:
 * the result, H[8] = 1) is taken to level levels - 1; every level runs iters + 1 passes (iters steps at most) and hands its best to
 * the next finer one.  pyr_a / pyr_b: pyramids of bh_gray_pyramid_u8 for Ha x Wa and Hb x Wb with the same `levels`; mask_pyr (NULL ok)
 * uint8 [B, total of B's pyramid] in the same layout, non-zero = the pixel of B may count.  stats[B, levels, 3] = (rho at the level's
 * first pass, rho_best, accepted steps), index 0 the FINEST level.  ws: bh_ecc_refine_ws_doubles() doubles (HOST memory query).
 * BH_E_BADARG: a NULL pyr_a / pyr_b / H64 / stats / ws (doubles for the query), B < 0, a size < 1, iters < 0; then BH_E_UNSUPPORTED:
 * levels outside 1..6 or a coarsest level of either image under 8 pixels on a side, more than 2^29 pixels; then B == 0: BH_OK, nothing
 * launched.  Refusals return before any launch. */
int bh_ecc_refine_ws_doubles(int Hb, int Wb, int B, int64_t* doubles);
int bh_ecc_refine(const float* pyr_a, int Ha, int Wa, const float* pyr_b, int Hb, int Wb, const uint8_t* mask_pyr, int B, int levels, int iters,
                  double* H64, double* stats, double* ws, void* stream);

/* Cascaded re-prediction: the model is run again on image A seen through the current homography, so that a stage only predicts the
 * residual, and the stages are composed.  Upstream makes one prediction (eval.py:249-255) and warps whole images on the host
 * (src/data/utils.py:54-67); the direction is the loss's, patch_1(H_p x) ~ patch_2(x) (PerceptualHead.py:371).  Two passes are stated
 * here and, in numpy float64, in bihome_amd/align.py (prep_warp_host, patch_ncc_host; grid_map and cascade_compose hold the algebra).
 *
 * The warped preparation.  The sub-sample grid is a virtual integer grid of P ny rows and P nx columns: patch pixel (y, x) owns columns
 * x nx .. x nx + nx - 1 and rows y ny .. y ny + ny - 1.  Hg[B,9] double maps the grid's index coordinates to index coordinates of
 * images[idx[b]] (the caller folds everything into it: Hg = H A_b S with A_b the affine map of B's preparation and
 * S = [[1/nx, 0, 0.5/nx - 0.5], [0, 1/ny, 0.5/ny - 0.5], [0, 0, 1]]).  Every sub-sample (X, Y) is bh_warp_u8's bilinear sample at
 * Hg (X, Y, 1) - csrc/u8_image.h's u8_sample, the function bh_warp_u8 calls; taps outside the image contribute 0 - and a
 * sub-sample under the projection guard (|qz| <= 1e-8) contributes 0.  With m_c the sum over the nx ny sub-samples divided by nx ny:
 *     patch[b,c,y,x] = (v / 255 - mean) / std,  v = 0.299 m_R + 0.587 m_G + 0.114 m_B for C = 1, m_c for C = 3,
 * without a full-size intermediate image and without its rounding to uint8.  cover[B,P,P] float (NULL ok) = (number of VALID
 * sub-samples) / (nx ny), valid by bh_warp_u8's rule (no guard, 0 <= u <= Ws - 1, 0 <= v <= Hs - 1): exactly 1.0f if and only if every
 * sub-sample is valid.  images / idx / n_images as in bh_align_prep_u8 (idx CLAMPED, 64-bit image offsets, 32-bit offsets inside an
 * image).  One thread per patch pixel, one writer per element, no atomics, no scratch: two calls are bitwise equal.
 * BH_E_BADARG: NULL images / Hg / patch, a negative B, n_images < 1, Hs < 1, Ws < 1, P < 1, std zero or NaN; then BH_E_UNSUPPORTED: C
 * not 1 or 3, P % 16 != 0, P > 256, nx or ny outside 1..8, Hs * Ws > 2^29 pixels; then B == 0: BH_OK, nothing launched.  Refusals
 * return before any launch. */
int bh_align_prep_warp_u8(const uint8_t* images, const int* idx, int n_images, int Hs, int Ws, const double* Hg,
                          int B, int P, int C, int nx, int ny, float mean, float std,
                          float* patch, float* cover, void* stream);

/* The score of a stage: the zero-mean normalised correlation of the warped patch w[B,C,P,P] and B's patch t[B,C,P,P] over all C
 * channels of the pixels with cover[b,y,x] == 1.0f (cover[B,P,P]; NULL: every pixel counts).  out[B,8] double = (n, sum w, sum t,
 * sum w w, sum t t, sum w t, rho, 0) with num = n sum wt - sum w sum t, va = n sum ww - (sum w)^2, vt = n sum tt - (sum t)^2 and
 * rho = num / sqrt(va vt) when n >= 16, va > 0 and vt > 0, else rho = -inf.  One workgroup of 256 threads per sample; products and
 * accumulators are double, reduced inside a wavefront by shuffles and across the four wavefronts through LDS in a fixed order: no
 * atomics, no workspace, two calls are bitwise equal.
 * BH_E_BADARG: NULL w / t / out, a negative B, P < 1; then BH_E_UNSUPPORTED: C not 1 or 3, P % 16 != 0, P > 256; then B == 0: BH_OK,
 * nothing launched.  Refusals return before any launch. */
int bh_patch_ncc(const float* w, const float* t, const float* cover, int B, int C, int P, double* out, void* stream);

/* Mosaic: both images of an aligned pair on one canvas, combined in one pass - what an inter-image homography is usually computed for
 * (panoramas, frame stacks, before / after composites).  The numpy float64 statement is bihome_amd/align.py's mosaic_host
 * (mosaic_frame_host places the canvas - bh_pano_frame with n = 1 - and exposure_host gives the gain / bias).  Index coordinates throughout.
 *
 * images_a[n_a,Ha,Wa,3], images_b[n_b,Hb,Wb,3] uint8 interleaved RGB banks, idx_a / idx_b[B] int32 as in bh_align_prep_u8 (NULL: sample b
 * is image b; CLAMPED into the bank in the kernel).  Ma[B,9], Mb[B,9] double map index coordinates of the CANVAS (Hc x Wc) to index
 * coordinates of A and of B: with H from B to A and T from the canvas to B, Ma = H T and Mb = T.  For image X in {A, B} at canvas pixel
 * (x, y): (u, v) and the bilinear value (taps outside the image contribute 0) are bh_warp_u8's, by the function it calls
 * (csrc/u8_image.h's u8_sample, float); X is PRESENT where bh_warp_u8's valid holds (no projection guard, 0 <= u <= Wx - 1,
 * 0 <= v <= Hx - 1); its weight is w = min(min(u, Wx - 1 - u, v, Hx - 1 - v) + 1, feather) where present: the distance to the border
 * of the image in its own pixels, plus 1, capped - feather = 1 is the plain average.  gain[B,2] double = (g, o) (NULL: (1, 0)) turns
 * A's value a into a' = fmaf(g, a, o) per channel, in grey levels, before the blend.  Then, by mode,
 *     BH_MOSAIC_FEATHER   v = (wa a' + wb b) / (wa + wb) over the images present,
 *     BH_MOSAIC_B_OVER_A  v = b where B is present, else a' where A is present,
 *     BH_MOSAIC_A_OVER_B  the reverse,
 * v = 0 where neither is, and out[b,y,x,:] = round_half_up(clamp(v, 0, 255)) as in bh_warp_u8.  An image that is not present is
 * selected out, not multiplied by 0 (its sample is unspecified under the guard).  out[B,Hc,Wc,3] uint8; cover[B,Hc,Wc] uint8 (NULL ok)
 * = (A present) | (B present) << 1: 0 empty, 1 only A, 2 only B, 3 both.  Floating point is float apart from reading the matrices.
 * Wc % 4 == 0 with out on a 4-byte boundary: four pixels and three dword stores per thread (cover: one dword when it is on a 4-byte
 * boundary, else four bytes); anything else one pixel and byte stores, same results.  64-bit image offsets and offsets into out, 32-bit
 * offsets inside an image.  One pass, one writer per output element, no atomics, no scratch: two calls are bitwise equal.
 * BH_E_BADARG: NULL images_a / images_b / Ma / Mb / out, B < 0, n_a, n_b, Ha, Wa, Hb, Wb, Hc or Wc < 1, a feather that is NaN, infinite
 * or below 1, an unknown mode; then BH_E_UNSUPPORTED: Ha * Wa or Hb * Wb > 2^29 or Hc * Wc > 2^31 - 1 pixels; then B == 0: BH_OK,
 * nothing launched.  Refusals return before any launch. */
#define BH_MOSAIC_FEATHER 0
#define BH_MOSAIC_B_OVER_A 1
#define BH_MOSAIC_A_OVER_B 2
int bh_mosaic_u8(const uint8_t* images_a, const int* idx_a, int n_a, int Ha, int Wa,
                 const uint8_t* images_b, const int* idx_b, int n_b, int Hb, int Wb,
                 const double* Ma, const double* Mb, const double* gain,
                 int B, int Hc, int Wc, float feather, int mode,
                 uint8_t* out, uint8_t* cover, void* stream);

/* Panorama: the n frames of a registered SEQUENCE (a pan, a burst, an aerial strip) on one canvas - the mosaic beyond a pair.  Upstream has
 * nothing like it.  The numpy float64 statements are bihome_amd/align.py's chain_host, pano_frame_host and pano_host.  Index coordinates
 * throughout.  A sample is n frames (1 <= n <= 255) of ONE uint8 bank images[n_images,Hs,Ws,3], all of one size; frame r is the reference,
 * and G[b,k] maps index coordinates of the reference to index coordinates of frame k (the pair convention "B's -> A's" with B = the
 * reference): G[b,r] = I, every G scaled to G[2,2] = 1.
 *
 * bh_pano_chain: Hpair[B,n-1,9] double, pair j connects frames j and j + 1: for j >= ref it is (a, b) = (j + 1, j) and G[j+1] = Hpair[j] G[j],
 * for j < ref it is (a, b) = (j, j + 1) and G[j] = Hpair[j] G[j+1] - Hpair[j] maps b's coordinates to a's; each product is divided by its
 * [2,2] entry, unguarded.  With gain_pair[B,n-1,2] and gain[B,n,2] both given (either NULL: no gains; n = 1 has no pair and needs gain alone), a pair's (g, o) matches a to b,
 * v_b ~ g v_a + o, and frame a's line to the reference is (g_b g, g_b o + o_b), the reference's (1, 0).  G[B,n,9] double.  One thread per
 * sample, plain double arithmetic without contraction.
 * BH_E_BADARG: NULL G, NULL Hpair with n > 1, a negative B, n outside 1..255, ref outside [0, n); then B == 0: BH_OK, nothing launched.
 *
 * bh_pano_frame: the canvas, the ONE frame rule of the mosaic and the panorama (pano_frame_host) for all n frames in one launch.  Hs x Ws is
 * the size of every frame, whose corners (0, 0), (Ws-1, 0), (Ws-1, Hs-1), (0, Hs-1) are projected; Hr x Wr is the size of the reference -
 * the frames' own in a sequence, image B's for a pair, where n = 1, G = H and the frame is image A.  It starts from the reference's extent
 * [0, Wr-1] x [0, Hr-1]; frame k takes part where it is usable - det G finite and not 0, the denominators of its four corners through G^-1
 * (adjugate / determinant) finite, of one sign and above 1e-8 in magnitude, the projected corners finite - and use[b,k] != 0 (use[B,n]
 * uint8, NULL: all): its corners, clamped to [-limit Wr, (1 + limit) Wr - 1] x [-limit Hr, (1 + limit) Hr - 1], are united into the box.
 * s = max((x1 - x0) / (Wc - 1), (y1 - y0) / (Hc - 1)), 1 where that is 0; T[B,9] = (s 0 tx; 0 s ty; 0 0 1) maps canvas index coordinates to
 * the reference's with the box centred; bbox[B,4] = (x0, y0, x1, y1) (NULL ok); fitted[B,n] uint8 (NULL ok): frame k took part;
 * M[B,n,9] = G[b,k] T (NULL ok), what bh_pano_u8 takes.  One workgroup of 256 threads per sample, thread k is frame k, a min / max reduction;
 * all double, no contraction.
 * BH_E_BADARG: NULL G / T, a negative B, n outside 1..255, Hs, Ws, Hr or Wr < 1, Hc or Wc < 2, a limit that is not > 0; then B == 0: BH_OK.
 *
 * bh_pano_u8: idx[B,n] int32: frame k of sample b is image idx[b n + k], CLAMPED into the bank in the kernel (NULL: frame k is image k, for
 * every sample).  M[B,n,9] double maps index coordinates of the canvas (Hc x Wc) to frame k's.  At canvas pixel (x, y) frame k's (u, v) and
 * bilinear value are bh_warp_u8's (csrc/u8_image.h, float); the frame is PRESENT where bh_warp_u8's valid holds and use[b n + k] != 0 (use
 * NULL: all); its value is fmaf(g_k, v, o_k) per channel with gain[B,n,2] double (NULL: (1, 0)), its weight bh_mosaic_u8's
 * w = min(min(u, Ws - 1 - u, v, Hs - 1 - v) + 1, feather).  By mode, over the frames present in the order k = 0 .. n - 1,
 *     BH_PANO_FEATHER  (sum_k w_k v_k) / (sum_k w_k), every product rounded before it is added,
 *     BH_PANO_FIRST    the value of the lowest k present,
 *     BH_PANO_LAST     the value of the highest k present,
 * 0 where none is, and out[b,y,x,:] = round_half_up(clamp(., 0, 255)).  A frame that is not present is selected out, not multiplied by 0 -
 * so a wavefront none of whose pixels has frame k present passes on to frame k + 1 without loading anything of it, and in a pan, where a
 * canvas pixel sees a few of the n frames, that is most (wavefront, frame) pairs.  count[B,Hc,Wc] uint8 (NULL ok): the number of frames
 * present.  For n = 2 with frames (A, B), gain ((g, o), (1, 0)) the result is bit for bit bh_mosaic_u8's: FEATHER = BH_MOSAIC_FEATHER,
 * FIRST = BH_MOSAIC_A_OVER_B, LAST = BH_MOSAIC_B_OVER_A, count = the number of bits set in cover.  Stores, offsets and the two paths
 * (Wc % 4 == 0 with out on a 4-byte boundary: four pixels per thread) are bh_mosaic_u8's; one pass, one writer per output element, no
 * atomics, no scratch, no LDS: two calls are bitwise equal.
 * BH_E_BADARG: NULL images / M / out, a negative B, n outside 1..255, n_images, Hs, Ws, Hc or Wc < 1, a feather that is NaN, infinite or
 * below 1, an unknown mode; then BH_E_UNSUPPORTED: Hs * Ws > 2^29 or Hc * Wc > 2^31 - 1 pixels; then B == 0: BH_OK, nothing launched.
 * Refusals return before any launch. */
#define BH_PANO_FEATHER 0
#define BH_PANO_FIRST 1
#define BH_PANO_LAST 2
int bh_pano_chain(const double* Hpair, const double* gain_pair, int B, int n, int ref, double* G, double* gain, void* stream);
int bh_pano_frame(const double* G, const uint8_t* use, int B, int n, int Hs, int Ws, int Hr, int Wr, int Hc, int Wc, double limit,
                  double* T, double* bbox, uint8_t* fitted, double* M, void* stream);
int bh_pano_u8(const uint8_t* images, const int* idx, int n_images, int Hs, int Ws, const double* M, const double* gain,
               const uint8_t* use, int B, int n, int Hc, int Wc, float feather, int mode, uint8_t* out, uint8_t* count, void* stream);

/* Two-band blend: the mosaic and the panorama without the feather's doubled edges.  Every frame is split into a LOW band, a Gaussian
 * low-pass of the frame in its own pixels, and a HIGH band, frame minus low (Burt & Adelson; two bands as in Brown & Lowe).  The low bands
 * are blended with the wide feather, so exposure and vignetting fade over the whole overlap; the high band is taken from ONE frame per
 * pixel, so frames that disagree by a pixel or two double nothing.  The numpy statements are bihome_amd/align.py's blur_taps, blur_host,
 * bands_host and mosaic_bands_host.
 *
 * bh_blur_u8: out[count,H,W,3] uint8, sample s the low band of image idx[s] of images[n_images,H,W,3] (NULL: image s; CLAMPED into the
 * bank in the kernel).  taps is a HOST pointer to radius + 1 ints w_0 .. w_radius, 1 <= radius <= 32, every w >= 0 and
 * w_0 + 2 sum_{i >= 1} w_i = 2048 (align.blur_taps(sigma): radius = ceil(3 sigma), w_i = floor(2048 g_i + 0.5) of the normalised Gaussian
 * for i >= 1, w_0 the rest); they are read before the call returns and go to the kernel by value.
 *     L[y,x,c] = (sum_j sum_i w_|j| w_|i| I[clamp(y + j, 0, H - 1), clamp(x + i, 0, W - 1), c] + 2^21) >> 22,  -radius <= i, j <= radius,
 * the border replicated.  The sum is exact in 32-bit unsigned integers (255 * 2048 * 2048 < 2^31): its order does not show, the kernel
 * equals the statement bit for bit, and a constant image comes back unchanged.  One launch for all samples; a workgroup stages a 32 x 24
 * tile with its halo in LDS, sums along the rows into 32-bit LDS words, then along the columns, and stores; no atomics, one writer per
 * output byte: two calls are bitwise equal.
 * BH_E_BADARG: NULL images / taps / out, count < 0, n_images, H or W < 1, a radius outside 1..32, a negative tap, taps that do not sum to
 * 2048; then BH_E_UNSUPPORTED: H * W > 2^29 pixels; then count == 0: BH_OK, nothing launched.
 *
 * bh_pano_bands_u8: bh_pano_u8's arguments without a mode, plus low[B n,Hs,Ws,3] uint8: low image b n + k is the low band of frame k of
 * sample b (what bh_blur_u8 writes for idx[B,n] flattened).  Frame k is PRESENT exactly where bh_pano_u8 has it present.  Over the frames
 * present, in the order k = 0 .. n - 1, all in float without contraction, with I_k(p) bh_warp_u8's bilinear value and L_k(p) the same
 * bilinear sample of the low image at the SAME taps (one projection, eight loads):
 *     v = fmaf(g_k, I_k(p), o_k),  l = fmaf(g_k, L_k(p), o_k),  w = bh_mosaic_u8's weight min(border distance + 1, feather),
 *     num_c += w l_c (the product rounded before it is added),  den += w,
 *     the frame becomes the WINNER if it is the first present or w > w_best, strictly (ties: the lowest k): w_best, v_best, l_best, winner = k.
 * Before rounding the value is 0 where nothing is present, v_best where exactly one frame is, else v_best + (num / den - l_best); then
 * out[b,y,x,:] = round_half_up(clamp(., 0, 255)).  So where one frame is present the result is BH_PANO_FIRST's bit for bit, and with an
 * all-zero low bank it is the winner's own sample bit for bit.  count[B,Hc,Wc] uint8 (NULL ok): the number of frames present;
 * winner[B,Hc,Wc] uint8 (NULL ok): the winner's k, 255 where nothing is present.  The wavefront skip, the 32 x 8 tile, the two store paths
 * and their alignment rules are bh_pano_u8's; no LDS, no atomics, no scratch, one writer per output element.
 * Refusals: bh_pano_u8's (and a NULL low), without the mode.
 *
 * bh_mosaic_bands_u8: bh_mosaic_u8's arguments without a mode, plus low_a[B,Ha,Wa,3] and low_b[B,Hb,Wb,3] uint8, the low bands of the
 * B samples' images in sample order.  The frames are (A, B), the gain applies to A (both bands), and the rule is bh_pano_bands_u8's - one
 * device function: for same-size frames bh_pano_bands_u8 with n = 2 and gain ((g, o), (1, 0)) gives out and winner bit for bit, and count
 * equals the number of bits set in cover.  cover as in bh_mosaic_u8; winner[B,Hc,Wc] uint8 (NULL ok): 0 for A, 1 for B, 255 for none.
 * Refusals: bh_mosaic_u8's (and a NULL low_a / low_b), without the mode. */
int bh_blur_u8(const uint8_t* images, const int* idx, int n_images, int H, int W, int count, const int* taps, int radius, uint8_t* out,
               void* stream);
int bh_pano_bands_u8(const uint8_t* images, const uint8_t* low, const int* idx, int n_images, int Hs, int Ws, const double* M, const double* gain,
                     const uint8_t* use, int B, int n, int Hc, int Wc, float feather, uint8_t* out, uint8_t* count, uint8_t* winner, void* stream);
int bh_mosaic_bands_u8(const uint8_t* images_a, const uint8_t* low_a, const int* idx_a, int n_a, int Ha, int Wa,
                       const uint8_t* images_b, const uint8_t* low_b, const int* idx_b, int n_b, int Hb, int Wb,
                       const double* Ma, const double* Mb, const double* gain,
                       int B, int Hc, int Wc, float feather,
                       uint8_t* out, uint8_t* cover, uint8_t* winner, void* stream);

/* Global adjustment: bh_pano_chain composes neighbouring pairs, so its error grows along the chain and a sequence that comes back to where it
 * started does not close.  bh_pano_adjust solves all frames' homographies JOINTLY from a list of EDGES - the chain's pairs and any further
 * links between frames that overlap - by Levenberg-Marquardt on the disagreement of the edges in the reference's pixels (the "global
 * alignment" / "bundle adjustment of the homographies" step of stitching pipelines).  The numpy float64 statement is bihome_amd/align.py's
 * adjust_host.  All arithmetic is double; one workgroup of 256 threads per sample, one launch, nothing read back by the host, no atomics.
 *   G0[B,n,9]      the start: the reference's index coordinates -> frame k's, as bh_pano_chain makes it (2 <= n <= BH_ADJUST_MAX_FRAMES)
 *   link[E,2]      int32 in DEVICE memory, the edges (a, b), one list for all samples (1 <= E <= BH_ADJUST_MAX_EDGES); an edge with
 *                  a == b or an index outside [0, n) counts for nothing
 *   Hlink[B,E,9]   b's index coordinates -> a's, used as H / H[8] (the pair convention)
 *   weight[B,E]    NULL: all 1.  An edge COUNTS iff its weight is finite and > 0 (and its indices are two distinct frames)
 *   Hs, Ws         the frame size (2 .. 2^24 each); grid: g in 2..8; iters >= 0 steps, every sample that starts runs all of them
 *   G[B,n,9]       out; work[B,4] out: cost at the start, cost at the result, accepted steps, final lambda
 *   ws             scratch of bh_pano_adjust_ws_doubles() doubles (written to HOST memory by that query): B (N + 1) N, the normal matrix
 *                  with the right-hand side as its last row
 * Unknowns: W_k = G_k^-1 (frame k -> reference) scaled to W[2,2] = 1; the 8 leading entries of every k != ref are free, W_ref = I is fixed:
 * N = 8 (n - 1), frame k's columns at 8 (k < ref ? k : k - 1).  W_k of the start is adj(G0_k) / adj(G0_k)[2,2] with the adjugate written
 * out.  Control points: y_p, p = j g + i, the g x g lattice x = (i (Ws - 1)) / (g - 1), y = (j (Hs - 1)) / (g - 1); for edge e,
 * z_p = proj(H_e y_p).  Residual of edge e at point p: r = proj(W_a z_p) - proj(W_b y_p), where the two frames put one scene point in the
 * reference; cost = sum_e w_e sum_p |r|^2.  With q = W (x, y, 1), (u, v) = (qx, qy) / qz the Jacobian of proj(W (x, y)) with respect to
 * W[0..7] is bh_homography_refine_lm's: d u / d W0..2 = (x, y, 1) / qz, d u / d W6,7 = -(x, y) u / qz, zero for W3..5; d v likewise with
 * W3..5 and v - taken at z_p for W_a and, negated, at y_p for W_b.  Columns of the reference do not exist.
 * One step (bh_homography_refine_lm's rules and constants): solve (J^T W J + lambda diag(J^T W J)) d = -J^T W r, a dense N x N system, by
 * Cholesky; a frame that no counting edge touches has a zero diagonal and gets unit rows (diagonal 1, right-hand side 0), so it does not
 * move; trial = W + d.  The trial is ACCEPTED iff its cost is finite, every point of every counting edge has qz > 0 under the link and
 * under both of its matrices at the trial, and cost(trial) < cost - then W = trial and lambda = max(lambda / 10, 1e-12); otherwise W stays
 * and lambda = min(10 lambda, 1e12).  lambda starts at 1e-3.
 * A sample KEEPS ITS START - G = G0 copied bit for bit, both costs the start's, zero accepted steps - when
 *   - an entry of G0 or of a counting Hlink is not finite; a G0_k, k != ref, is singular: the determinant by the adjugate's first column,
 *     (a adj00 + b adj10) + c adj20, is 0 or not finite, or an entry of adj / adj[2,2] is not finite (then both costs are NaN and no step is
 *     tried);
 *   - a counting point has qz <= 0 at the start, or the start's cost is not finite (both costs are that sum, and no step is tried);
 *   - a Cholesky pivot of any of its steps is not > 0, or a component of d is not finite (the steps end there);
 *   - no step is accepted, or an entry of the result is not finite.
 * Otherwise G_k = adj(W_k) / adj(W_k)[2,2] and G_ref = I exactly.
 * Orders of summation.  A matrix entry: over the counting edges in index order, each edge's term w_e t, t = sum over p ascending of
 * (jx_r jx_c + jy_r jy_c), products rounded before they are added; the right-hand side likewise with (jx_r rx + jy_r ry).  The cost: thread
 * t sums w_e s_e over its edges e = t, t + 256, .. with s_e = sum over p ascending of (rx^2 + ry^2), and the 256 partial sums are added
 * pairwise, [i] += [i + h] for h = 128, 64, .. 1.  The factorisation is a right-looking Cholesky in blocks of 8 with the right-hand side as row
 * N (the forward substitution), then L^T d = y backwards in blocks of 8; an entry takes its subtractions as fused multiply-adds, the
 * columns of a block ascending, block after block.  One workgroup per sample, no atomics: two calls agree bit for bit, and a sample's
 * result does not depend on its neighbours.
 * BH_E_BADARG: NULL G0 / link / Hlink / G / work / ws (doubles for the query), a negative B, n outside 2..64, E outside 1..1024, ref outside
 * [0, n), Hs or Ws outside 2..2^24, grid outside 2..8, iters < 0; then B == 0: BH_OK, nothing launched.  Refusals come before any launch. */
#define BH_ADJUST_MAX_FRAMES 64
#define BH_ADJUST_MAX_EDGES 1024
int bh_pano_adjust_ws_doubles(int n, int E, int B, int64_t* doubles);
int bh_pano_adjust(const double* G0, const int* link, const double* Hlink, const double* weight, int B, int n, int E, int ref, int Hs, int Ws,
                   int grid, int iters, double* G, double* work, double* ws, void* stream);

/* MaxPool2d(3, 2, 1) NHWC. argmax[N,Ho,Wo,C] (uint8, NULL ok in inference): window position 0..8 of the first
 * maximum (ATen's tie rule); the adjoint gathers through it (no atomics, no recomputation).
 * BH_E_BADARG: a NULL x / y (gy / gx / argmax in the adjoint), N < 0, Hi < 1, Wi < 1, C < 4; BH_E_UNSUPPORTED: C % 4; N == 0: BH_OK, nothing launched. */
int bh_maxpool3s2_fwd(const float* x, float* y, unsigned char* argmax, int N, int Hi, int Wi, int C, void* stream);
int bh_maxpool3s2_bwd(const unsigned char* argmax, const float* gy, float* gx, int N, int Hi, int Wi, int C, void* stream);
/* AdaptiveAvgPool2d(1) NHWC -> [N,C], and adjoint.  BH_E_BADARG: a NULL pointer, N < 0, HW < 1, C < 1; N == 0: BH_OK, nothing launched. */
int bh_gap_fwd(const float* x, float* y, int N, int HW, int C, void* stream);
int bh_gap_bwd(const float* gy, float* gx, int N, int HW, int C, void* stream);
/* out = a + b (elementwise, used to join gradient branches) */
int bh_add(const float* a, const float* b, float* out, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
