"""Aligning two full-size uint8 images with a trained model, on the device.

A model here predicts `delta_hat`, the displacement of the four corners of a P x P patch, from two standardised patches.  Upstream lifts
that to a homography and warps only at patch level, on the host, for visualisation (eval.py:249-255, src/data/utils.py:54-67, through
cv2 / kornia).  `Aligner` does it for whole images of any size without a host round trip:

    aligner = Aligner(model)                                  # model: step.build_model(cfg, "cuda:0") with trained weights
    r = aligner(images_a, images_b)                           # uint8 [N,H,W,3] device tensors or ImageBanks; sizes may differ
    r["H"], r["aligned"], r["valid"]                          # image B index coordinates -> image A; A resampled onto B's grid

Three steps surround the model; their definitions are stated below in numpy float64 (`prep_host`, `lift`, `warp_u8_host`) and in
include/bihome.h, and the kernels (csrc/align.hip: bh_align_prep_u8, bh_warp_u8) are tested against these statements.

INDEX coordinates: pixel j sits at coordinate j and occupies [j - 0.5, j + 0.5) (csrc/warp_tap.h, four_point_to_homography).
EDGE coordinates, used for regions only: pixel i spans [i, i + 1).

Preparation (ToGrayscale / DictToGrayscale, src/data/transforms.py:333-354; DictStandardize, :369-378; the resize is new): a region
(x0, y0, rw, rh) of the image in edge coordinates (default: the whole image) becomes the P x P patch whose pixel (y, x) is the exact area
average of the source over [x0 + x sx, x0 + (x+1) sx) x [y0 + y sy, y0 + (y+1) sy), sx = rw / P, sy = rh / P, of
v = 0.299 R + 0.587 G + 0.114 B (C = 1) or of each channel (C = 3), then (v / 255 - mean) / std.  geom = (sx, sy, tx, ty), tx = x0 + 0.5
sx - 0.5, ty = y0 + 0.5 sy - 0.5, is the affine map A from patch index coordinates to image index coordinates.  Unlike cv2.resize
(INTER_LINEAR two-tap, INTER_AREA with its own rounding) this is one formula for shrinking, copying and enlarging.

Lift: H_p = four_point_to_homography of the corners (0,0), (P,0), (P,P), (0,P) and delta_hat (K.h4pt_fwd; eval.py:252-254), and
H_img = A_a H_p A_b^-1 scaled to H[2,2] = 1.  The loss trains patch_1(H_p x) ~ patch_2(x) (PerceptualHead.py:371), so H_img maps index
coordinates of image B to index coordinates of image A.

uint8 warp: aligned[y,x,:] = round_half_up(clamp(bilinear A(H_img (x, y, 1)), 0, 255)) on B's grid, taps outside A contribute 0
(warp_image's net map with zero padding, src/data/utils.py:54-59); valid = 1 where the projected point lies in [0, Wa-1] x [0, Ha-1].
cv2.warpPerspective rounds half to even in fixed point with 1/32-pixel coordinates; this rounds half up in float.

Refinement (optional, `Aligner(..., refine="ecc")` / `ecc_refine`; csrc/ecc.hip): the lift multiplies the model's patch-level error by
sx, sy, so H_img is polished on the two images themselves before the warp - the forward-additive enhanced-correlation-coefficient
iteration (Evangelidis & Psarakis; what cv2.findTransformECC does on the host) on gray 2 x 2 box pyramids, coarse to fine, blind to a gain
and a bias between the images, with the exact derivative of the bilinear interpolant at warp_tap.h's taps, a fixed number of passes per
level and the best H so far kept.  Stated below as gray_pyramid_host / ecc_sums_host / ecc_step_host / ecc_level_host / ecc_refine_host.

Cascade (optional, `aligner(..., cascade=K)`; csrc/cascade.hip): the models are trained on corner displacements of at most P / 4 patch
pixels and their error grows with the displacement, so the model is run again on A SEEN THROUGH the current H - stage k reads
patch_1 = A through H_prev on B's patch grid (bh_align_prep_warp_u8: the mean of nx x ny bilinear samples per patch pixel, no full-size
intermediate image) and patch_2 = B's patch, predicts only the residual delta_k, and the stages compose: patch coordinate q of that
patch_1 is A's coordinate H_prev A_b q, hence H_k = H_prev A_b H_p(delta_k) A_b^-1, still B's index coordinates -> A's.  A stage is kept
only where it raises the zero-mean normalised correlation of the two patches over the fully covered pixels (bh_patch_ncc), decided per
sample on the device.  Stated below as sample_host / grid_map / prep_warp_host / patch_ncc_host / cascade_compose.

Mosaic (optional, `aligner(..., mosaic="b")` / `mosaic=(Hc, Wc)` / `mosaic`; csrc/blend.hip): the warp alone gives "A on B's grid" - what
of A falls outside B's frame is lost and inside it the two are never combined.  bh_mosaic_u8 puts both on one canvas in one pass: with T
from canvas index coordinates to B's (the identity for canvas "b"; else `mosaic_frame_host`: the bounding box of B's extent and of A's
corners projected through H^-1 - clamped to `limit` image sizes around B, so that a garbage H cannot shrink B to a dot - scaled and centred
onto the Hc x Wc canvas with the aspect ratio kept; it is the panorama's frame rule for the single frame A) each canvas pixel takes
warp_u8_host's sample of A through H T and of B through T, and an image is PRESENT where warp_u8_host's `valid` holds.  Its weight
is min(distance of the projected point to the border of the image, in its own pixels, + 1, feather); mode "feather" gives (wa a' + wb b) / (wa + wb) over the images present, "b_over_a" / "a_over_b" put one
image on top, nothing present gives 0, then round half up; cover = (A present) | (B present) << 1.  a' = g a + o is A after the optional
gain / bias match: the ECC step is blind to both by design, so the blend handles them - `exposure_host` is the least-squares line of B's
gray on A's through H from the sums ecc_sums_host already makes.  Stated below as mosaic_frame_host / mosaic_host / exposure_host.

Panorama (`aligner.sequence(images, idx, ..., canvas=...)` / `panorama`; csrc/pano.hip): a SEQUENCE of n frames (1..255) of one size and
one bank, chosen by idx [B,n].  Frame r is the reference and G[b,k] maps the reference's index coordinates to frame k's (the pair
convention with B = the reference; G[b,r] = I).  The n - 1 neighbouring pairs (`pairs_of`: pair j connects frames j and j + 1, b the
one nearer to the reference) go through the aligner in ONE call, `chain_host` composes them outwards from the reference - G[a] = H_pair
G[b], divided by its [2,2] entry; the exposure lines compose alongside - `pano_frame_host` is the frame rule (the reference's extent
united with the clamped corners of every usable frame; `_corner_box` / `_fit_canvas`), and `pano_host` the blend over the frames present
(`_blend_host`, the one statement `mosaic_host` is made of too): 'feather' sum w v / sum w in frame order, 'first' / 'last' the lowest /
highest frame present, count = the number present.  For n = 2 both equal the pair's results bit for bit.  bh_pano_u8 makes the canvas
in one pass, and a wavefront none of whose pixels has a frame present takes no tap of it.

Two-band blend (mode "two_band" of `mosaic`, `panorama`, the aligner's mosaic and `Aligner.sequence`; csrc/blur.hip, csrc/blend.hip):
wherever two frames disagree by a pixel or two a feather doubles edges over the whole overlap, and a narrow feather shows the exposure
step instead.  So every frame is split into a LOW band - `blur_host`, a Gaussian of `band_sigma` frame pixels in integer arithmetic
with the taps of `blur_taps`, bit for bit what bh_blur_u8 makes - and a HIGH band, frame minus low (Burt & Adelson; two bands as in Brown
& Lowe).  The low bands are blended with the feather; the high band comes from ONE frame per pixel, the one with the largest weight
(ties: the lowest k): value = v_winner + (sum w l / sum w - l_winner), the frame's own value where one frame is present, `winner` the
frame chosen.  Stated below as blur_taps / blur_host / bands_host / mosaic_bands_host; bh_pano_bands_u8 and bh_mosaic_bands_u8 gather the
frame and its low band at the same taps, eight loads per present frame.

Global adjustment (`aligner.sequence(..., links=[(a, b), ...])` / `adjust`; csrc/adjust.hip): the chain composes neighbouring pairs, so
its error grows with n and a pan that comes back, an out-and-back sweep or a raster scan does not close.  With further EDGES between
frames that overlap - each link predicted through the chain's own estimate, `Aligner(..., init=)`, and kept only where the two frames
correlate through it - all frames are solved jointly: the unknowns are W_k = G_k^-1 (frame k -> reference, W[2,2] = 1, the reference
fixed), the residual of an edge (a, b) with H (b's index coordinates -> a's) at a control point y of a g x g lattice over the frame is
proj(W_a proj(H y)) - proj(W_b y), where the two frames put one scene point in the reference's pixels, and Levenberg-Marquardt with
bh_homography_refine_lm's rules (lambda from 1e-3 by factors of 10, a step accepted iff the cost falls with every denominator positive)
solves the dense 8 (n - 1) system by Cholesky, one workgroup per sample, a fixed number of steps.  A sample that cannot be evaluated
or solved keeps its start bit for bit.  Stated below as adjust_points / adjust_system_host / adjust_host."""
import operator

import numpy as np
import torch

from . import kernels as K
from . import synth

QZ_GUARD = 1e-8          # csrc/warp_tap.h tap_project: |qz| <= 1e-8 is not divided by


# ------------------------------------------------------------------------------------------------
# the definitions, numpy float64
# ------------------------------------------------------------------------------------------------
def _overlaps(origin, s, P, n):
    """[P, n]: the length of the overlap of output interval k, [origin + k s, origin + (k+1) s), with pixel i's [i, i+1)."""
    k = np.arange(P, dtype=np.float64)
    lo, hi = origin + k * s, origin + (k + 1) * s
    i = np.arange(n, dtype=np.float64)
    return np.maximum(np.minimum(hi[:, None], i[None, :] + 1) - np.maximum(lo[:, None], i[None, :]), 0.0)


def prep_host(images, roi=None, P=128, C=1, mean=0.443, std=0.129):
    """images uint8 [B,H,W,3], roi [B,4] (x0, y0, rw, rh) in edge coordinates or None (whole images) -> (patch [B,C,P,P] float64,
    geom [B,4] float64 (sx, sy, tx, ty)): the Preparation of the module docstring."""
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError("prep_host: images uint8 [B,H,W,3], got %s %s" % (images.dtype, images.shape))
    if C not in (1, 3):
        raise ValueError("prep_host: C is 1 (grayscale) or 3 (RGB), got %r" % (C,))
    B, H, W = images.shape[:3]
    roi = np.tile(np.array([0.0, 0.0, W, H]), (B, 1)) if roi is None else np.asarray(roi, np.float64).reshape(B, 4)
    patch, geom = np.empty((B, C, P, P)), np.empty((B, 4))
    for b in range(B):
        x0, y0, rw, rh = roi[b]
        sx, sy = rw / P, rh / P
        geom[b] = sx, sy, x0 + 0.5 * sx - 0.5, y0 + 0.5 * sy - 0.5
        v = images[b].astype(np.float64)
        v = (0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])[None] if C == 1 else v.transpose(2, 0, 1)
        oy, ox = _overlaps(y0, sy, P, H), _overlaps(x0, sx, P, W)
        area = np.matmul(np.matmul(oy[None], v), ox.T[None]) / (sx * sy)          # [C,P,P]: sum_j sum_i ov_y(y,j) v(j,i) ov_x(x,i)
        patch[b] = (area / 255.0 - mean) / std
    return patch, geom


def _affine(geom):
    """geom [B,4] -> A [B,3,3]: patch index coordinates -> image index coordinates."""
    g = np.asarray(geom, np.float64).reshape(-1, 4)
    A = np.zeros((g.shape[0], 3, 3))
    A[:, 0, 0], A[:, 1, 1], A[:, 0, 2], A[:, 1, 2], A[:, 2, 2] = g[:, 0], g[:, 1], g[:, 2], g[:, 3], 1.0
    return A


def patch_corners(P):
    """[4,2] float64: (0,0), (P,0), (P,P), (0,P)."""
    return np.array([[0, 0], [P, 0], [P, P], [0, P]], np.float64)


def _compose(left, delta, P, geom_b):
    """left [B,3,3], delta [B,4,2] (patch pixels), geom_b [B,4] -> left H_p(delta) A_b^-1 [B,3,3] float64 scaled to H[2,2] = 1, H_p =
    four_point_to_homography of the patch square: what `lift` (left = A_a) and `cascade_compose` (left = H_prev A_b) share."""
    d = np.asarray(delta, np.float64).reshape(-1, 4, 2)
    Ab = _affine(geom_b)
    c = patch_corners(P)
    H = np.empty((d.shape[0], 3, 3))
    for b in range(d.shape[0]):
        Hb = left[b] @ synth.four_point_homography(c, c + d[b]) @ np.linalg.inv(Ab[b])
        H[b] = Hb / Hb[2, 2]
    return H


def lift(delta_hat, P, geom_a, geom_b):
    """delta_hat [B,4,2] (patch pixels), the geometry records of both preparations -> H [B,3,3] float64 with H[2,2] = 1: index
    coordinates of image B -> index coordinates of image A (the Lift of the module docstring)."""
    return _compose(_affine(geom_a), delta_hat, P, geom_b)


def _project_host(M, Ho, Wo):
    """(u, v float64 [Ho,Wo], guard bool [Ho,Wo]) of the output grid through M [3,3]; 1 / qz is 1 under the guard."""
    ys, xs = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    qz = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
    guard = ~(np.abs(qz) > QZ_GUARD)
    iz = 1.0 / np.where(guard, 1.0, qz)
    return (M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) * iz, (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) * iz, guard


def _sample_host(images, H, Ho, Wo):
    """(values float64 [B,Ho,Wo,3], valid bool [B,Ho,Wo], guard bool [B,Ho,Wo]): the uint8 warp of the module docstring up to its
    rounding."""
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError("sample_host: images uint8 [B,Hs,Ws,3], got %s %s" % (images.dtype, images.shape))
    H = np.asarray(H, np.float64).reshape(-1, 3, 3)
    B, Hs, Ws = images.shape[:3]
    out, valid, guards = np.empty((B, Ho, Wo, 3)), np.empty((B, Ho, Wo), bool), np.empty((B, Ho, Wo), bool)
    for b in range(B):
        img = images[b].astype(np.float64)
        u, v, guard = _project_host(H[b], Ho, Wo)
        with np.errstate(invalid="ignore"):
            x0f, y0f = np.floor(u), np.floor(v)
            fx, fy = u - x0f, v - y0f
            x0 = np.clip(np.nan_to_num(x0f, nan=-2.0), -2, Ws).astype(np.int64)
            y0 = np.clip(np.nan_to_num(y0f, nan=-2.0), -2, Hs).astype(np.int64)
            acc = np.zeros((Ho, Wo, 3))
            for dy, wy in ((0, 1 - fy), (1, fy)):
                for dx, wx in ((0, 1 - fx), (1, fx)):
                    xi, yi = x0 + dx, y0 + dy
                    ok = (xi >= 0) & (xi < Ws) & (yi >= 0) & (yi < Hs)
                    w = np.where(ok, wy * wx, 0.0)
                    acc += img[np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)] * np.nan_to_num(w)[..., None]
            valid[b] = ~guard & (u >= 0) & (u <= Ws - 1) & (v >= 0) & (v <= Hs - 1)
        out[b], guards[b] = acc, guard
    return out, valid, guards


def warp_u8_host(images, H, Ho, Wo):
    """images uint8 [B,Hs,Ws,3], H [B,3,3] (output index coordinates -> source index coordinates) -> (out uint8 [B,Ho,Wo,3],
    valid uint8 [B,Ho,Wo]): the uint8 warp of the module docstring."""
    values, valid, _ = _sample_host(images, H, Ho, Wo)
    return _round_u8(values), valid.astype(np.uint8)


def _round_u8(values):
    """round_half_up(clamp(values, 0, 255)) as uint8."""
    return np.floor(np.clip(values, 0.0, 255.0) + 0.5).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# mosaic, the definitions (numpy float64; include/bihome.h "Mosaic" states the same in C terms)
# ------------------------------------------------------------------------------------------------
MOSAIC_MODES = tuple(K.MOSAIC_MODES)          # ("feather", "b_over_a", "a_over_b"): kernels.py has the BH_MOSAIC_* numbers


def _corner_box(H, size_a, size_b, limit):
    """H [K,3,3] (B's index coordinates -> A's) -> (x0, x1, y0, y1 [K] float64, usable [K] bool): B's extent united with A's four corners
    through H^-1 (adjugate / determinant, written out) clamped to `limit` image sizes around B; B's extent alone where H is not usable.
    `pano_frame_host`'s half of the frame rule per frame (A the frame, B the reference)."""
    (Ha, Wa), (Hb, Wb) = size_a, size_b
    a, b, c, d, e, f, g, h, i = (H[:, r, k] for r in range(3) for k in range(3))
    with np.errstate(all="ignore"):
        adj = ((e * i - f * h, c * h - b * i, b * f - c * e), (f * g - d * i, a * i - c * g, c * d - a * f), (d * h - e * g, b * g - a * h, a * e - b * d))
        det = a * adj[0][0] + b * adj[1][0] + c * adj[2][0]
        inv = [[adj[r][k] / det for k in range(3)] for r in range(3)]
        corners = ((0.0, 0.0), (Wa - 1.0, 0.0), (Wa - 1.0, Ha - 1.0), (0.0, Ha - 1.0))
        qx, qy, qz = (np.stack([inv[r][0] * x + inv[r][1] * y + inv[r][2] for x, y in corners], 1) for r in range(3))          # [K,4]
        px, py = qx / qz, qy / qz
        usable = np.isfinite(det) & (det != 0) & np.isfinite(qz).all(1) & ((qz > 0).all(1) | (qz < 0).all(1)) & (np.abs(qz) > QZ_GUARD).all(1)
        usable &= np.isfinite(px).all(1) & np.isfinite(py).all(1)
        x0 = np.minimum(np.clip(px.min(1), -limit * Wb, (1 + limit) * Wb - 1), 0.0)
        x1 = np.maximum(np.clip(px.max(1), -limit * Wb, (1 + limit) * Wb - 1), Wb - 1.0)
        y0 = np.minimum(np.clip(py.min(1), -limit * Hb, (1 + limit) * Hb - 1), 0.0)
        y1 = np.maximum(np.clip(py.max(1), -limit * Hb, (1 + limit) * Hb - 1), Hb - 1.0)
    return np.where(usable, x0, 0.0), np.where(usable, x1, Wb - 1.0), np.where(usable, y0, 0.0), np.where(usable, y1, Hb - 1.0), usable


def _fit_canvas(x0, x1, y0, y1, canvas):
    """The box [x0, x1] x [y0, y1] ([K] each) -> T [K,3,3]: canvas index coordinates -> the box's, one scale (the aspect ratio kept; 1 for
    a box without extent) and the box centred."""
    Hc, Wc = canvas
    s = np.maximum((x1 - x0) / (Wc - 1), (y1 - y0) / (Hc - 1))
    s = np.where(s == 0, 1.0, s)
    T = np.zeros((x0.shape[0], 3, 3))
    T[:, 0, 0], T[:, 1, 1], T[:, 2, 2] = s, s, 1.0
    T[:, 0, 2], T[:, 1, 2] = (x0 + x1) * 0.5 - s * (0.5 * (Wc - 1)), (y0 + y1) * 0.5 - s * (0.5 * (Hc - 1))
    return T


def _frame_args(canvas, limit, who):
    if min(canvas) < 2:
        raise ValueError("%s: a canvas has at least 2 pixels on each side, got %d x %d (H x W)" % (who, canvas[0], canvas[1]))
    if not limit > 0:
        raise ValueError("%s: limit > 0, got %r" % (who, limit))


def mosaic_frame_host(H, size_a, size_b, canvas, limit=2.0):
    """H [B,3,3] (B's index coordinates -> A's), size_a = (Ha, Wa), size_b = (Hb, Wb), canvas = (Hc, Wc) -> (T [B,3,3] float64: canvas
    index coordinates -> B's, a scale and a translation; bbox [B,4] = (xmin, ymin, xmax, ymax) in B's index coordinates; fitted [B]
    uint8): the Mosaic frame of the module docstring - `pano_frame_host` for the single frame A around the reference B."""
    _frame_args(canvas, limit, "mosaic_frame")
    T, bbox, fitted = pano_frame_host(np.asarray(H, np.float64).reshape(-1, 1, 3, 3), size_a, canvas, limit, ref_size=size_b)
    return T, bbox, fitted[:, 0]


def _border_weight_host(M, size, present, feather, Hc, Wc):
    """The weight of a frame of size = (Hs, Ws) on a canvas it is projected to through M [B,3,3]: min(distance of the projected point to
    the border of the frame + 1, feather) where present [B,Hc,Wc] holds, else 0 -> [B,Hc,Wc] float64."""
    Hs, Ws = size
    with np.errstate(all="ignore"):
        points = [_project_host(M[b], Hc, Wc) for b in range(present.shape[0])]
        w = np.stack([np.minimum(np.minimum(np.minimum(pu, Ws - 1 - pu), np.minimum(pv, Hs - 1 - pv)) + 1.0, feather) for pu, pv, _ in points])
    return np.where(present, w, 0.0)


def _blend_host(frames, feather, mode):
    """The blend statement of the mosaic and the panorama.  frames yields, in order, (values float64 [B,Hc,Wc,3] (`_sample_host`), present
    bool [B,Hc,Wc], M [B,3,3], (Hs, Ws), gain [B,2] = (g, o) or None) per frame; mode is 'feather', 'first' or 'last' -> (the values before
    rounding [B,Hc,Wc,3], the list of the `present` planes).  A frame's value is g v + o and its weight min(distance of its projected point
    to the border of the frame + 1, feather); 'feather' is sum w v / sum w over the frames present, accumulated in the order given, 'first'
    / 'last' the value of the first / last frame present, nothing present 0.  A frame that is not present is selected out, never
    multiplied by 0: under the projection guard its sample is unspecified."""
    num = den = val = 0.0
    seen, planes = False, []
    for v, present, M, size, gain in frames:
        P = present[..., None]
        if gain is not None:
            v = gain[:, 0, None, None, None] * v + gain[:, 1, None, None, None]
        if mode == "feather":
            w = _border_weight_host(M, size, present, feather, *present.shape[1:])[..., None]
            num = num + np.where(P, w * np.where(P, v, 0.0), 0.0)
            den = den + w
        elif mode == "first":
            val = np.where(P & np.logical_not(seen), v, val)
        else:
            val = np.where(P, v, val)
        seen = seen | P
        planes.append(present)
    if mode == "feather":
        val = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    return np.where(seen, val, 0.0), planes


def _blend_args(feather, mode, modes, who):
    if mode not in modes:
        raise ValueError("%s: mode is one of %s, got %r" % (who, modes, mode))
    if not (feather >= 1 and np.isfinite(feather)):
        raise ValueError("%s: feather is finite and at least 1, got %r" % (who, feather))


def mosaic_host(images_a, images_b, Ma, Mb, Hc, Wc, feather=32.0, mode="feather", gain=None):
    """images_a uint8 [B,Ha,Wa,3], images_b uint8 [B,Hb,Wb,3], Ma / Mb [B,3,3] (canvas index coordinates -> A's / B's; the caller passes
    Ma = H T, Mb = T), gain [B,2] = (g, o) or None -> (out uint8 [B,Hc,Wc,3], cover uint8 [B,Hc,Wc] = (A present) | (B present) << 1):
    the Mosaic of the module docstring - `_blend_host` on the frames (A, B), 'b_over_a' the last present and 'a_over_b' the first."""
    _blend_args(feather, mode, MOSAIC_MODES, "mosaic_host")
    Ma, Mb = np.asarray(Ma, np.float64).reshape(-1, 3, 3), np.asarray(Mb, np.float64).reshape(-1, 3, 3)
    B = Ma.shape[0]
    gain = np.tile(np.array([[1.0, 0.0]]), (B, 1)) if gain is None else np.asarray(gain, np.float64).reshape(B, 2)
    frames = []
    for images, M, g in ((images_a, Ma, gain), (images_b, Mb, None)):
        v, present, _ = _sample_host(images, M, Hc, Wc)
        frames.append((v, present, M, np.asarray(images).shape[1:3], g))
    val, (pa, pb) = _blend_host(frames, feather, {"feather": "feather", "b_over_a": "last", "a_over_b": "first"}[mode])
    return _round_u8(val), (pa.astype(np.uint8) | (pb.astype(np.uint8) << 1)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# panorama, the definitions (numpy float64; include/bihome.h "Panorama" states the same in C terms)
# ------------------------------------------------------------------------------------------------
PANO_MODES = tuple(K.PANO_MODES)              # ("feather", "first", "last"): kernels.py has the BH_PANO_* numbers
PANO_MAX_FRAMES = K.PANO_MAX_FRAMES           # 255: count is a byte


def pairs_of(n, ref):
    """The n - 1 pairs (a, b) of a chain of n frames around the reference `ref`: pair j connects frames j and j + 1, and b is the one
    nearer to the reference - (j + 1, j) for j >= ref, (j, j + 1) for j < ref."""
    if not (1 <= n <= PANO_MAX_FRAMES and 0 <= ref < n):
        raise ValueError("pairs_of: 1 <= n <= %d and 0 <= ref < n, got n = %r, ref = %r" % (PANO_MAX_FRAMES, n, ref))
    return [(j, j + 1) if j < ref else (j + 1, j) for j in range(n - 1)]


def chain_host(H_pairs, ref, gain_pairs=None):
    """H_pairs [B,n-1,3,3] (pair j of `pairs_of`: b's index coordinates -> a's), gain_pairs [B,n-1,2] = (g, o) with v_b ~ g v_a + o, or
    None -> G [B,n,3,3] float64 (the reference's index coordinates -> frame k's, G[ref] = I, every G scaled to G[2,2] = 1 by an unguarded
    division), and with gains also gain [B,n,2] (frame k's line to the reference, (1, 0) for the reference): the Panorama chain."""
    Hp = np.asarray(H_pairs, np.float64)
    if Hp.ndim != 4 or Hp.shape[2:] != (3, 3):
        raise ValueError("chain_host: H_pairs [B,n-1,3,3], got %s" % (Hp.shape,))
    B, n = Hp.shape[0], Hp.shape[1] + 1
    order = pairs_of(n, ref)
    G = np.empty((B, n, 3, 3))
    G[:, ref] = np.eye(3)
    gp = None if gain_pairs is None else np.asarray(gain_pairs, np.float64).reshape(B, n - 1, 2)
    gain = np.empty((B, n, 2))
    gain[:, ref] = 1.0, 0.0
    with np.errstate(all="ignore"):
        for j in list(range(ref, n - 1)) + list(range(ref - 1, -1, -1)):
            a, b = order[j]
            P = Hp[:, j] @ G[:, b]
            G[:, a] = P / P[:, 2:3, 2:3]
            if gp is not None:
                gain[:, a, 0] = gain[:, b, 0] * gp[:, j, 0]
                gain[:, a, 1] = gain[:, b, 0] * gp[:, j, 1] + gain[:, b, 1]
    return G if gp is None else (G, gain)


def pano_frame_host(G, size, canvas, limit=2.0, use=None, ref_size=None):
    """G [B,n,3,3] (the reference's index coordinates -> frame k's), size = (Hs, Ws) of every frame, canvas = (Hc, Wc), use [B,n] or None,
    ref_size = (Hr, Wr) of the reference (None: size) -> (T [B,3,3] float64: canvas index coordinates -> the reference's; bbox [B,4] =
    (xmin, ymin, xmax, ymax) in the reference's index coordinates; fitted [B,n] uint8): the frame rule - the reference's extent united
    with the corners of every frame that is usable and in use, clamped to `limit` reference sizes around it (`_corner_box`), then fitted to
    the canvas (`_fit_canvas`)."""
    G = np.asarray(G, np.float64)
    if G.ndim != 4 or G.shape[2:] != (3, 3) or not 1 <= G.shape[1] <= PANO_MAX_FRAMES:
        raise ValueError("pano_frame: G [B,n,3,3] with 1 <= n <= %d, got %s" % (PANO_MAX_FRAMES, G.shape))
    _frame_args(canvas, limit, "pano_frame")
    B, n = G.shape[:2]
    Hr, Wr = ref_size = size if ref_size is None else ref_size
    x0, x1, y0, y1, usable = (v.reshape(B, n) for v in _corner_box(G.reshape(B * n, 3, 3), size, ref_size, limit))
    fitted = usable if use is None else usable & (np.asarray(use).reshape(B, n) != 0)
    x0, x1 = np.where(fitted, x0, 0.0).min(1), np.where(fitted, x1, Wr - 1.0).max(1)
    y0, y1 = np.where(fitted, y0, 0.0).min(1), np.where(fitted, y1, Hr - 1.0).max(1)
    return _fit_canvas(x0, x1, y0, y1, canvas), np.stack([x0, y0, x1, y1], 1), fitted.astype(np.uint8)


def pano_host(images, idx, M, Hc, Wc, feather=32.0, mode="feather", gain=None, use=None):
    """images uint8 [N,Hs,Ws,3], idx [B,n] (frame k of sample b is images[idx[b,k]]), M [B,n,3,3] (canvas index coordinates -> frame
    k's; the caller passes G T), gain [B,n,2] = (g, o) or None, use [B,n] or None -> (out uint8 [B,Hc,Wc,3], count uint8 [B,Hc,Wc]): frame
    k is PRESENT at a canvas pixel where warp_u8_host's `valid` holds and use[b,k] != 0; `_blend_host` on the n frames in the order
    k = 0..n-1 ('first' / 'last': the value of the lowest / highest k present), then round half up.  count is the number of frames
    present."""
    _blend_args(feather, mode, PANO_MODES, "pano_host")
    images, idx = np.asarray(images), np.asarray(idx)
    M = np.asarray(M, np.float64)
    if idx.ndim != 2 or not 1 <= idx.shape[1] <= PANO_MAX_FRAMES or M.shape != idx.shape + (3, 3):
        raise ValueError("pano_host: idx [B,n] with 1 <= n <= %d and M [B,n,3,3], got %s and %s" % (PANO_MAX_FRAMES, idx.shape, M.shape))
    B, n = idx.shape
    gain = np.tile(np.array([1.0, 0.0]), (B, n, 1)) if gain is None else np.asarray(gain, np.float64).reshape(B, n, 2)
    use = np.ones((B, n), bool) if use is None else np.asarray(use).reshape(B, n) != 0

    def frames():
        for k in range(n):
            v, present, _ = _sample_host(images[idx[:, k]], M[:, k], Hc, Wc)
            yield v, present & use[:, k, None, None], M[:, k], images.shape[1:3], gain[:, k]
    val, planes = _blend_host(frames(), feather, mode)
    return _round_u8(val), np.sum(planes, axis=0, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------
# global adjustment, the definitions (numpy float64; include/bihome.h "Global adjustment" states the same in C terms)
# ------------------------------------------------------------------------------------------------
ADJUST_MAX_FRAMES, ADJUST_MAX_EDGES = K.ADJUST_MAX_FRAMES, K.ADJUST_MAX_EDGES          # 64 frames (N = 504 unknowns), 1024 edges
ADJUST_LAMBDA = (1e-3, 1e-12, 1e12)                                                    # the start, the floor, the ceiling


def _adjugate(M):
    """M [...,3,3] -> (adj [...,3,3], det [...]): the adjugate written out and the determinant by its first column."""
    a, b, c, d, e, f, g, h, i = (M[..., r, k] for r in range(3) for k in range(3))
    adj = np.stack([np.stack([e * i - f * h, c * h - b * i, b * f - c * e], -1), np.stack([f * g - d * i, a * i - c * g, c * d - a * f], -1),
                    np.stack([d * h - e * g, b * g - a * h, a * e - b * d], -1)], -2)
    return adj, (a * adj[..., 0, 0] + b * adj[..., 1, 0]) + c * adj[..., 2, 0]


def adjust_points(size, grid):
    """[g g,2] float64: the control points, the g x g lattice over a frame of size = (Hs, Ws), p = j g + i at
    ((i (Ws - 1)) / (g - 1), (j (Hs - 1)) / (g - 1))."""
    Hs, Ws = size
    j, i = np.divmod(np.arange(grid * grid), grid)
    return np.stack([(i * (Ws - 1)) / (grid - 1.0), (j * (Hs - 1)) / (grid - 1.0)], 1)


def _proj(M, pts):
    """M [3,3], pts [P,2] -> ((u, v) [P,2], qz [P])."""
    q = pts @ M[:, :2].T + M[:, 2]
    return q[:, :2] / q[:, 2:3], q[:, 2]


def _adjust_jacobian(W, pts):
    """d proj(W pts) / d W[0..7] -> [P,2,8]: (x, y, 1) / qz for the row of the coordinate, -(x, y) (u or v) / qz in columns 6, 7."""
    uv, qz = _proj(W, pts)
    x, y, iz = pts[:, 0] / qz, pts[:, 1] / qz, 1.0 / qz
    J = np.zeros((len(pts), 2, 8))
    J[:, 0, 0], J[:, 0, 1], J[:, 0, 2], J[:, 0, 6], J[:, 0, 7] = x, y, iz, -x * uv[:, 0], -y * uv[:, 0]
    J[:, 1, 3], J[:, 1, 4], J[:, 1, 5], J[:, 1, 6], J[:, 1, 7] = x, y, iz, -x * uv[:, 1], -y * uv[:, 1]
    return J


def adjust_system_host(W, edges, ref, want_J=True):
    """W [n,3,3] (frame k -> reference), edges = [(a, b, w, y [P,2], z [P,2])] of the counting edges -> (r [2 P E'], sw [2 P E'] the
    weight of each residual, J [2 P E', N] dense or None, ok: every qz > 0): the residuals proj(W_a z_p) - proj(W_b y_p), edge after edge,
    point after point, x before y, and their Jacobian with respect to the 8 (n - 1) unknowns (frame k's at 8 (k < ref ? k : k - 1))."""
    n = W.shape[0]
    N, rows = 8 * (n - 1), sum(2 * len(e[3]) for e in edges)
    r, sw, J, ok, at = np.empty(rows), np.empty(rows), np.zeros((rows, N)) if want_J else None, True, 0
    for a, b, w, y, z in edges:
        m = 2 * len(y)
        (pa, qa), (pb, qb) = _proj(W[a], z), _proj(W[b], y)
        ok = ok and bool((qa > 0).all() and (qb > 0).all())
        r[at:at + m], sw[at:at + m] = (pa - pb).reshape(m), w
        if want_J:
            for k, pts, sign in ((a, z, 1.0), (b, y, -1.0)):
                if k != ref:
                    c = 8 * (k if k < ref else k - 1)
                    J[at:at + m, c:c + 8] = sign * _adjust_jacobian(W[k], pts).reshape(m, 8)
        at += m
    return r, sw, J, ok


def adjust_host(G0, links, H_links, weight, ref, size, grid=4, iters=10, solver="cholesky"):
    """The global adjustment: G0 [B,n,3,3] (the reference's index coordinates -> frame k's, `chain_host`'s), links [E,2] the edges (a, b),
    H_links [B,E,3,3] (b's index coordinates -> a's, used as H / H[2,2]), weight [B,E] or None (all 1), size = (Hs, Ws) of the frames ->
    (G [B,n,3,3] float64, work [B,4] = (cost at the start, cost at the result, accepted steps, final lambda)).
    An edge COUNTS iff a != b, both are frames of the sequence and its weight is finite and > 0.  The unknowns are W_k = G_k^-1 =
    adj(G_k) / adj(G_k)[2,2] for k != ref (8 entries each, W[2,2] = 1), W_ref = I; with y_p `adjust_points` and z_p = proj(H_e y_p) the
    residual of edge e at p is proj(W_a z_p) - proj(W_b y_p) and cost = sum_e w_e sum_p |r|^2.  One Levenberg-Marquardt step solves
    (J^T w J + lambda diag(J^T w J)) d = -J^T w r with the dense J of `adjust_system_host` (a frame no counting edge touches gets unit
    rows) by Cholesky (solver="solve": np.linalg.solve, what the device bound is measured with) and is accepted iff the cost of W + d is
    finite, every qz is > 0 and the cost fell; lambda starts at 1e-3 and moves by factors of 10 inside [1e-12, 1e12].  The sample keeps its
    start bit for bit (both costs the start's - NaN where it cannot be evaluated -, zero accepted steps) for an entry of G0 or of a
    counting H that is not finite, a singular G0, a qz <= 0 or a cost that is not finite at the start, a failed factorisation or a d that
    is not finite in any step, no accepted step, or a result that is not finite.  Otherwise G_k = adj(W_k) / adj(W_k)[2,2], G_ref = I."""
    G0 = np.asarray(G0, np.float64)
    links = np.asarray(links, np.int64).reshape(-1, 2)
    B, n, E = G0.shape[0], G0.shape[1], links.shape[0]
    if G0.ndim != 4 or G0.shape[2:] != (3, 3) or not 2 <= n <= ADJUST_MAX_FRAMES or not 1 <= E <= ADJUST_MAX_EDGES or not 0 <= ref < n:
        raise ValueError("adjust_host: G0 [B,n,3,3] with 2 <= n <= %d, 1 <= E <= %d edges and 0 <= ref < n, got %s, E = %d, ref = %r"
                         % (ADJUST_MAX_FRAMES, ADJUST_MAX_EDGES, G0.shape, E, ref))
    if not 2 <= grid <= 8 or iters < 0 or min(size) < 2 or solver not in ("cholesky", "solve"):
        raise ValueError("adjust_host: grid in 2..8, iters >= 0, a frame of at least 2 x 2 and solver 'cholesky' or 'solve', got %r, %r, %r, %r" % (grid, iters, size, solver))
    Hl = np.asarray(H_links, np.float64).reshape(B, E, 3, 3)
    weight = np.ones((B, E)) if weight is None else np.asarray(weight, np.float64).reshape(B, E)
    y = adjust_points(size, grid)
    N, lam0, lam_min, lam_max = 8 * (n - 1), *ADJUST_LAMBDA
    G, work = G0.copy(), np.empty((B, 4))
    for s in range(B):
        with np.errstate(all="ignore"):
            work[s] = np.nan, np.nan, 0.0, lam0
            counts = [e for e, (a, b) in enumerate(links.tolist()) if a != b and 0 <= a < n and 0 <= b < n and np.isfinite(weight[s, e]) and weight[s, e] > 0]
            adj, det = _adjugate(G0[s])
            W = adj / adj[:, 2:3, 2:3]
            W[ref] = np.eye(3)
            others = np.arange(n) != ref
            if not (np.isfinite(G0[s]).all() and np.isfinite(Hl[s, counts]).all() and np.isfinite(det[others]).all() and (det[others] != 0).all() and np.isfinite(W).all()):
                continue
            edges, ok = [], True
            for e in counts:
                z, qz = _proj(Hl[s, e] / Hl[s, e, 2, 2], y)
                ok = ok and bool((qz > 0).all())
                edges.append((int(links[e, 0]), int(links[e, 1]), weight[s, e], y, z))
            r, sw, _, ok_w = adjust_system_host(W, edges, ref, want_J=False)
            cost = float((sw * r * r).sum())
            work[s, :2] = cost
            if not (ok and ok_w and np.isfinite(cost)):
                continue
            touched = np.zeros(n, bool)
            for a, b, *_ in edges:
                touched[a] = touched[b] = True
            free = np.repeat(touched[others], 8)
            lam, accepted, failed = lam0, 0, False
            for _ in range(iters):
                r, sw, J, _ = adjust_system_host(W, edges, ref)
                A, g = J.T @ (sw[:, None] * J), J.T @ (sw * r)
                A[np.diag_indices(N)] = np.where(free, np.diag(A) + lam * np.diag(A), 1.0)
                try:
                    if solver == "cholesky":
                        L = np.linalg.cholesky(A)
                        d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
                    else:
                        d = np.linalg.solve(A, -g)
                except np.linalg.LinAlgError:
                    failed = True
                    break
                if not np.isfinite(d).all():
                    failed = True
                    break
                trial = W.copy()
                trial[others] = (W[others].reshape(-1, 9) + np.concatenate([d.reshape(n - 1, 8), np.zeros((n - 1, 1))], 1)).reshape(-1, 3, 3)
                rt, _, _, ok_t = adjust_system_host(trial, edges, ref, want_J=False)
                cost_t = float((sw * rt * rt).sum())
                if np.isfinite(cost_t) and ok_t and cost_t < cost:
                    W, cost, accepted, lam = trial, cost_t, accepted + 1, max(lam / 10.0, lam_min)
                else:
                    lam = min(lam * 10.0, lam_max)
            work[s, 3] = lam
            if failed or accepted == 0:
                continue
            adj, _ = _adjugate(W)
            out = adj / adj[:, 2:3, 2:3]
            out[ref] = np.eye(3)
            if np.isfinite(out).all():
                G[s], work[s, 1], work[s, 2] = out, cost, accepted
    return G, work


# ------------------------------------------------------------------------------------------------
# two-band blend, the definitions (numpy; include/bihome.h "Two-band blend" states the same in C terms)
# ------------------------------------------------------------------------------------------------
BAND_MODES = ("two_band",)         # the mode of `mosaic` / `panorama` that has no BH_MOSAIC_* / BH_PANO_* number: entry points of its own
BAND_SIGMA_MIN, BAND_SIGMA_MAX = 0.5, 10.5
BAND_NONE = 255                    # winner where nothing is present


def blur_taps(sigma):
    """The integer taps of the low band: int64 [r + 1] = (w_0 .. w_r), r = ceil(3 sigma) (0.5 <= sigma <= 10.5, so 1 <= r <= 32).
    g_i = exp(-i^2 / (2 sigma^2)) normalised over i = -r .. r, w_i = floor(2048 g_i + 0.5) for i >= 1 and w_0 = 2048 - 2 sum_{i>=1} w_i: the
    taps sum to 2048 exactly, whatever the rounding did.  Pure numpy float64."""
    sigma = float(sigma)
    if not BAND_SIGMA_MIN <= sigma <= BAND_SIGMA_MAX:                          # (False for a NaN too)
        raise ValueError("blur_taps: %g <= sigma <= %g, got %r" % (BAND_SIGMA_MIN, BAND_SIGMA_MAX, sigma))
    r = int(np.ceil(3.0 * sigma))
    i = np.arange(r + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    g = g / (g[0] + 2.0 * g[1:].sum())
    w = np.floor(2048.0 * g + 0.5).astype(np.int64)
    w[0] = 2048 - 2 * int(w[1:].sum())
    return w


def blur_host(images, sigma, order="rows"):
    """images uint8 [...,H,W,3] -> the low band, uint8 of the same shape:
    L[y,x,c] = (sum_j sum_i w|j| w|i| I[clamp(y + j), clamp(x + i), c] + 2^21) >> 22 with `blur_taps(sigma)`, the border replicated.
    Integer arithmetic (the sum stays below 2^31), so order = 'rows' (rows first) and 'cols' give the same bits, and bh_blur_u8 too."""
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim < 3 or images.shape[-1] != 3:
        raise ValueError("blur_host: images uint8 [...,H,W,3], got %s %s" % (images.dtype, images.shape))
    if order not in ("rows", "cols"):
        raise ValueError("blur_host: order is 'rows' or 'cols', got %r" % (order,))
    w = blur_taps(sigma)
    r = len(w) - 1

    def along(v, axis):
        n = v.shape[axis]
        at = np.clip(np.arange(-r, n + r), 0, n - 1)
        acc = np.zeros(v.shape, np.int64)
        for d in range(-r, r + 1):
            acc += int(w[abs(d)]) * np.take(v, at[r + d:r + d + n], axis=axis)
        return acc
    v = images.astype(np.int64)
    H_axis, W_axis = images.ndim - 3, images.ndim - 2
    v = along(along(v, W_axis), H_axis) if order == "rows" else along(along(v, H_axis), W_axis)
    return ((v + (1 << 21)) >> 22).astype(np.uint8)


def _bands_blend_host(frames, feather):
    """The two-band statement of the mosaic and the panorama.  frames yields, in order, (v, l float64 [B,Hc,Wc,3]: `_sample_host` of the
    frame and of its low band, present bool [B,Hc,Wc], M [B,3,3], (Hs, Ws), gain [B,2] or None) per frame -> (the values before rounding
    [B,Hc,Wc,3], the list of the `present` planes, winner uint8 [B,Hc,Wc]).  Both bands take the gain, the weight is `_blend_host`'s;
    num += w l and den += w over the frames present, and the frame becomes the winner if it is the first present or its weight is
    strictly larger than the winner's (ties: the lowest k).  Nothing present: 0; one frame present: its value; else
    v_winner + (num / den - l_winner)."""
    num = den = 0.0
    v_best = l_best = w_best = cnt = winner = None
    planes = []
    for k, (v, l, present, M, size, gain) in enumerate(frames):
        B, Hc, Wc = present.shape
        if cnt is None:
            v_best, l_best = np.zeros((B, Hc, Wc, 3)), np.zeros((B, Hc, Wc, 3))
            w_best, cnt, winner = np.zeros((B, Hc, Wc)), np.zeros((B, Hc, Wc), np.int64), np.full((B, Hc, Wc), BAND_NONE, np.uint8)
        P = present[..., None]
        if gain is not None:
            g, o = gain[:, 0, None, None, None], gain[:, 1, None, None, None]
            v, l = g * v + o, g * l + o
        w = _border_weight_host(M, size, present, feather, Hc, Wc)
        num = num + np.where(P, w[..., None] * np.where(P, l, 0.0), 0.0)
        den = den + w
        take = present & ((cnt == 0) | (w > w_best))
        v_best, l_best = np.where(take[..., None], v, v_best), np.where(take[..., None], l, l_best)
        w_best, winner = np.where(take, w, w_best), np.where(take, np.uint8(k), winner).astype(np.uint8)
        cnt = cnt + present
        planes.append(present)
    mixed = v_best + (num / np.where(den > 0, den, 1.0)[..., None] - l_best)
    val = np.where((cnt == 0)[..., None], 0.0, np.where((cnt == 1)[..., None], v_best, mixed))
    return val, planes, winner


def bands_host(images, low, idx, M, Hc, Wc, feather=32.0, gain=None, use=None):
    """`pano_host`'s arguments without a mode, plus low uint8 [B,n,Hs,Ws,3] (or [B n,Hs,Ws,3]): the low band of frame k of sample b
    (`blur_host(images[idx])`) -> (out uint8 [B,Hc,Wc,3], count uint8 [B,Hc,Wc], winner uint8 [B,Hc,Wc]: the frame whose high band the
    pixel takes, 255 for none): the two-band blend, `_bands_blend_host` on the n frames in the order k = 0..n-1, presence as in
    `pano_host`, then round half up."""
    _blend_args(feather, "feather", PANO_MODES, "bands_host")
    images, idx = np.asarray(images), np.asarray(idx)
    M = np.asarray(M, np.float64)
    if idx.ndim != 2 or not 1 <= idx.shape[1] <= PANO_MAX_FRAMES or M.shape != idx.shape + (3, 3):
        raise ValueError("bands_host: idx [B,n] with 1 <= n <= %d and M [B,n,3,3], got %s and %s" % (PANO_MAX_FRAMES, idx.shape, M.shape))
    B, n = idx.shape
    low = np.asarray(low)
    if low.dtype != np.uint8 or low.size != B * n * images[0].size or low.shape[-3:] != images.shape[1:]:
        raise ValueError("bands_host: low uint8 [B,n,Hs,Ws,3] with B = %d, n = %d, got %s %s" % (B, n, low.dtype, low.shape))
    low = low.reshape((B, n) + images.shape[1:])
    gain = np.tile(np.array([1.0, 0.0]), (B, n, 1)) if gain is None else np.asarray(gain, np.float64).reshape(B, n, 2)
    use = np.ones((B, n), bool) if use is None else np.asarray(use).reshape(B, n) != 0

    def frames():
        for k in range(n):
            v, present, _ = _sample_host(images[idx[:, k]], M[:, k], Hc, Wc)
            l, _, _ = _sample_host(low[:, k], M[:, k], Hc, Wc)
            yield v, l, present & use[:, k, None, None], M[:, k], images.shape[1:3], gain[:, k]
    val, planes, winner = _bands_blend_host(frames(), feather)
    return _round_u8(val), np.sum(planes, axis=0, dtype=np.uint8), winner


def mosaic_bands_host(images_a, low_a, images_b, low_b, Ma, Mb, Hc, Wc, feather=32.0, gain=None):
    """`mosaic_host`'s arguments without a mode, plus the low bands low_a uint8 [B,Ha,Wa,3] and low_b uint8 [B,Hb,Wb,3] -> (out uint8
    [B,Hc,Wc,3], cover uint8 [B,Hc,Wc] as `mosaic_host`'s, winner uint8 [B,Hc,Wc]: 0 for A, 1 for B, 255 for none):
    `_bands_blend_host` on the frames (A, B); the gain applies to A."""
    _blend_args(feather, "feather", MOSAIC_MODES, "mosaic_bands_host")
    Ma, Mb = np.asarray(Ma, np.float64).reshape(-1, 3, 3), np.asarray(Mb, np.float64).reshape(-1, 3, 3)
    B = Ma.shape[0]
    gain = np.tile(np.array([[1.0, 0.0]]), (B, 1)) if gain is None else np.asarray(gain, np.float64).reshape(B, 2)
    frames = []
    for images, low, M, g in ((images_a, low_a, Ma, gain), (images_b, low_b, Mb, None)):
        if np.asarray(low).shape != np.asarray(images).shape or np.asarray(low).dtype != np.uint8:
            raise ValueError("mosaic_bands_host: a low band is uint8 of its images' shape %s, got %s" % (np.asarray(images).shape, np.asarray(low).shape))
        v, present, _ = _sample_host(images, M, Hc, Wc)
        l, _, _ = _sample_host(low, M, Hc, Wc)
        frames.append((v, l, present, M, np.asarray(images).shape[1:3], g))
    val, (pa, pb), winner = _bands_blend_host(frames, feather)
    return _round_u8(val), (pa.astype(np.uint8) | (pb.astype(np.uint8) << 1)).astype(np.uint8), winner


def exposure_host(sums):
    """The 66 sums of `ecc_sums_host` at level 0 ([66], or [B,66]) -> (g, o) ([2], or [B,2]) float64: the least-squares line of B's gray
    on A's gray seen through H over the counting pixels, t ~ g iw + o; (1, 0) for n < ECC_MIN_N, a variance of iw that is not > 0, or a
    g that is not finite and positive."""
    s = np.asarray(sums, np.float64)
    rows = s.reshape(-1, ECC_SUMS)
    out = np.empty((rows.shape[0], 2))
    for k, r in enumerate(rows):
        S = lambda i, j: float(r[ecc_index(i, j)])
        g, o, n = 1.0, 0.0, S(10, 10)
        if n >= ECC_MIN_N:
            m_iw, m_t = S(8, 10) / n, S(9, 10) / n
            v_iw, c_it = S(8, 8) - (n * m_iw) * m_iw, S(8, 9) - (n * m_iw) * m_t
            if v_iw > 0:
                gg = c_it / v_iw
                if np.isfinite(gg) and gg > 0:
                    g, o = gg, m_t - gg * m_iw
        out[k] = g, o
    return out[0] if s.ndim == 1 else out


# ------------------------------------------------------------------------------------------------
# cascaded re-prediction, the definitions (numpy float64; include/bihome.h "Cascaded re-prediction" states the same in C terms)
# ------------------------------------------------------------------------------------------------
def sample_host(images, H, Ho, Wo):
    """images uint8 [B,Hs,Ws,3], H [B,3,3] (output index coordinates -> source index coordinates) -> (values float64 [B,Ho,Wo,3], the
    bilinear samples with zero padding, NOT rounded or clamped; valid uint8 [B,Ho,Wo]): `warp_u8_host` without its rounding."""
    values, valid, _ = _sample_host(images, H, Ho, Wo)
    return values, valid.astype(np.uint8)


def grid_map(geom, nx, ny):
    """geom [B,4], the sub-samples per patch pixel -> A S [B,3,3]: index coordinates of the P ny x P nx sub-sample grid -> image index
    coordinates.  Grid column X = x nx + i is the sub-sample at patch coordinate x + (i + 0.5) / nx - 0.5: S = [[1/nx, 0, 0.5/nx - 0.5],
    [0, 1/ny, 0.5/ny - 0.5], [0, 0, 1]]."""
    S = np.array([[1.0 / nx, 0.0, 0.5 / nx - 0.5], [0.0, 1.0 / ny, 0.5 / ny - 0.5], [0.0, 0.0, 1.0]])
    return _affine(geom) @ S


def prep_warp_host(images, Hg, P=128, C=1, nx=1, ny=1, mean=0.443, std=0.129):
    """images uint8 [B,Hs,Ws,3], Hg [B,3,3] (index coordinates of the P ny x P nx sub-sample grid -> image index coordinates) ->
    (patch [B,C,P,P] float64, cover [B,P,P] float64): patch pixel (y, x) is the mean over grid rows y ny .. y ny + ny - 1 and columns
    x nx .. x nx + nx - 1 of the bilinear sample (taps outside the image 0; a sample under the guard |qz| <= 1e-8 is 0), as gray
    0.299 R + 0.587 G + 0.114 B (C = 1) or per channel (C = 3), then (v / 255 - mean) / std; cover is the share of its sub-samples that
    are valid by warp_u8_host's rule - 1.0 exactly where all are."""
    if C not in (1, 3):
        raise ValueError("prep_warp_host: C is 1 (grayscale) or 3 (RGB), got %r" % (C,))
    values, valid, guard = _sample_host(images, Hg, P * ny, P * nx)
    B = values.shape[0]
    values = np.where(guard[..., None], 0.0, values)
    m = values.reshape(B, P, ny, P, nx, 3).sum(axis=(2, 4)) / (nx * ny)                     # [B,P,P,3]
    v = (0.299 * m[..., 0] + 0.587 * m[..., 1] + 0.114 * m[..., 2])[:, None] if C == 1 else m.transpose(0, 3, 1, 2)
    cover = valid.reshape(B, P, ny, P, nx).sum(axis=(2, 4)) / float(nx * ny)
    return (v / 255.0 - mean) / std, cover


def patch_ncc_host(w, t, cover=None):
    """w, t [B,C,P,P], cover [B,P,P] or None -> [B,8] float64 (n, sum w, sum t, sum ww, sum tt, sum wt, rho, 0) over all channels of the
    pixels with cover == 1 (None: all): rho = (n sum wt - sum w sum t) / sqrt((n sum ww - (sum w)^2)(n sum tt - (sum t)^2)) for
    n >= ECC_MIN_N and both variances positive, else -inf."""
    w, t = np.asarray(w, np.float64), np.asarray(t, np.float64)
    B, C = w.shape[:2]
    out = np.zeros((B, 8))
    for b in range(B):
        keep = np.ones(w.shape[2:], bool) if cover is None else np.asarray(cover[b]) == 1.0
        a, c = w[b][:, keep].ravel(), t[b][:, keep].ravel()
        n, sw, st, sww, stt, swt = float(a.size), a.sum(), c.sum(), (a * a).sum(), (c * c).sum(), (a * c).sum()
        num, va, vt = n * swt - sw * st, n * sww - sw * sw, n * stt - st * st
        rho = num / np.sqrt(va * vt) if (n >= ECC_MIN_N and va > 0 and vt > 0) else -np.inf
        out[b] = n, sw, st, sww, stt, swt, rho, 0.0
    return out


def cascade_compose(H_prev, delta, P, geom_b):
    """H_prev [B,3,3] (B's index coordinates -> A's), delta [B,4,2] predicted on (A seen through H_prev on B's patch grid, B's patch),
    geom_b [B,4] -> H_prev A_b H_p(delta) A_b^-1 [B,3,3] scaled to H[2,2] = 1, H_p = four_point_to_homography of the patch square as in
    `lift`: patch coordinate q of the warped patch is A's coordinate H_prev A_b q, so the product still maps B's coordinates to A's."""
    Hp = np.asarray(H_prev, np.float64).reshape(-1, 3, 3)
    return _compose([h @ a for h, a in zip(Hp, _affine(geom_b))], delta, P, geom_b)


# ------------------------------------------------------------------------------------------------
# ECC refinement, the definitions (numpy float64; include/bihome.h "ECC refinement" states the same in C terms)
# ------------------------------------------------------------------------------------------------
ECC_NZ, ECC_SUMS = 11, 66          # z = (j0..j7, iw, t, 1); the upper triangle of z z^T, row-major
ECC_MIN_N = 16                     # fewer counting pixels than this: no step
ECC_MAX_LEVELS, ECC_MIN_SIDE = 6, 8
PYR_C = np.array([[2.0, 0.0, 0.5], [0.0, 2.0, 0.5], [0.0, 0.0, 1.0]])          # index coordinates of level l -> level l - 1
_ECC_IU = np.triu_indices(ECC_NZ)


def ecc_index(i, j):
    """Where entry (i, j) of the 11 x 11 Gram matrix sits among the 66 sums (either order of i, j)."""
    i, j = min(i, j), max(i, j)
    return i * ECC_NZ - i * (i - 1) // 2 + (j - i)


def pyramid_sizes(h, w, levels):
    """[(h_l, w_l)] for l = 0 .. levels - 1; ValueError (naming the sizes) for a pyramid that is not built."""
    if not 1 <= levels <= ECC_MAX_LEVELS:
        raise ValueError("pyramid: levels is 1..%d, got %r" % (ECC_MAX_LEVELS, levels))
    sizes = [(h >> l, w >> l) for l in range(levels)]
    if min(sizes[-1]) < ECC_MIN_SIDE:
        raise ValueError("pyramid: %d levels of a %d x %d (H x W) image end at %d x %d; the coarsest level has at least %d pixels on each "
                         "side" % (levels, h, w, sizes[-1][0], sizes[-1][1], ECC_MIN_SIDE))
    return sizes


def pyramid_offsets(h, w, levels):
    """offsets [levels + 1] of the levels inside a sample's packed row (bh_gray_pyramid_layout); the last is the row's length."""
    return np.concatenate([[0], np.cumsum([a * b for a, b in pyramid_sizes(h, w, levels)])]).astype(np.int64)


def gray_pyramid_host(images_u8, levels):
    """uint8 [B,H,W,3] -> [levels] arrays [B,h_l,w_l] float64: level 0 the gray image 0.299 R + 0.587 G + 0.114 B, level l the 2 x 2 box
    mean of level l - 1 (an odd last row / column dropped)."""
    images = np.asarray(images_u8)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError("gray_pyramid_host: images uint8 [B,H,W,3], got %s %s" % (images.dtype, images.shape))
    sizes = pyramid_sizes(images.shape[1], images.shape[2], levels)
    v = images.astype(np.float64)
    out = [0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2]]
    for h, w in sizes[1:]:
        p = out[-1]
        out.append(((p[:, 0:2 * h:2, 0:2 * w:2] + p[:, 0:2 * h:2, 1:2 * w:2]) + (p[:, 1:2 * h:2, 0:2 * w:2] + p[:, 1:2 * h:2, 1:2 * w:2])) * 0.25)
    return out


def mask_pyramid_host(mask, levels):
    """uint8 [B,H,W] -> [levels] uint8 arrays: level l is 1 where all four bytes of the 2 x 2 block below are non-zero."""
    m = (np.asarray(mask) != 0).astype(np.uint8)
    out = [m]
    for h, w in pyramid_sizes(m.shape[1], m.shape[2], levels)[1:]:
        p = out[-1]
        out.append(p[:, 0:2 * h:2, 0:2 * w:2] & p[:, 0:2 * h:2, 1:2 * w:2] & p[:, 1:2 * h:2, 0:2 * w:2] & p[:, 1:2 * h:2, 1:2 * w:2])
    return out


def h_level_down(H):
    """H at level l -> level l - 1 (the finer one): C H C^-1, H[2,2] = 1."""
    R = PYR_C @ np.asarray(H, np.float64).reshape(3, 3) @ np.linalg.inv(PYR_C)
    return R / R[2, 2]


def h_level_up(H):
    """H at level l - 1 -> level l (the coarser one): C^-1 H C, H[2,2] = 1."""
    R = np.linalg.inv(PYR_C) @ np.asarray(H, np.float64).reshape(3, 3) @ PYR_C
    return R / R[2, 2]


def ecc_terms_host(A_l, T_l, H, mask_l=None):
    """The per-pixel terms of one pass: (z [11,Hb,Wb] float64 with z = (j0..j7, iw, t, 1), counts [Hb,Wb] bool).  H is used as H / H[2,2]."""
    A, T = np.asarray(A_l, np.float64), np.asarray(T_l, np.float64)
    h = np.asarray(H, np.float64).reshape(3, 3)
    h = h / h[2, 2]
    (Ha, Wa), (Hb, Wb) = A.shape, T.shape
    ys, xs = np.mgrid[0:Hb, 0:Wb].astype(np.float64)
    qz = h[2, 0] * xs + h[2, 1] * ys + h[2, 2]
    with np.errstate(all="ignore"):
        ok = qz > QZ_GUARD
        iz = 1.0 / np.where(ok, qz, 1.0)
        u, v = (h[0, 0] * xs + h[0, 1] * ys + h[0, 2]) * iz, (h[1, 0] * xs + h[1, 1] * ys + h[1, 2]) * iz
        ok &= (u >= 0) & (u < Wa - 1) & (v >= 0) & (v < Ha - 1)
    if mask_l is not None:
        ok &= np.asarray(mask_l) != 0
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = u - x0, v - y0
    x1, y1 = np.minimum(x0 + 1, Wa - 1), np.minimum(y0 + 1, Ha - 1)          # (only where the pixel does not count)
    a00, a01, a10, a11 = A[y0, x0], A[y0, x1], A[y1, x0], A[y1, x1]
    iw = (1 - fy) * ((1 - fx) * a00 + fx * a01) + fy * ((1 - fx) * a10 + fx * a11)
    gx = (1 - fy) * (a01 - a00) + fy * (a11 - a10)
    gy = (1 - fx) * (a10 - a00) + fx * (a11 - a01)
    m = -(gx * u + gy * v)
    z = np.stack([gx * xs * iz, gx * ys * iz, gx * iz, gy * xs * iz, gy * ys * iz, gy * iz, m * xs * iz, m * ys * iz, iw, T, np.ones_like(T)])
    return z * ok, ok


def ecc_sums_host(A_l, T_l, H, mask_l=None):
    """One pass: the 66 sums (upper triangle of sum z z^T over the counting pixels, row-major; `ecc_index`) of the gray planes A_l
    (image A) and T_l (image B) at one level under H (B's index coordinates -> A's)."""
    z, _ = ecc_terms_host(A_l, T_l, H, mask_l)
    z = z.reshape(ECC_NZ, -1)
    return (z @ z.T)[_ECC_IU]


def ecc_step_host(sums):
    """One step from the 66 sums: (rho, d).  rho is NaN where it cannot be measured (n < 16, a variance not positive); d [8] is None where
    the step FAILS (that, a zero or NaN pivot, lambda's denominator not > 0, a d that is not finite).  Plain double operations in the
    order the kernel performs them (csrc/ecc.hip ecc_step_kernel)."""
    s = np.asarray(sums, np.float64).reshape(ECC_SUMS)
    S = lambda i, j: float(s[ecc_index(i, j)])
    n = S(10, 10)
    if not n >= ECC_MIN_N:
        return float("nan"), None
    m_iw, m_t = S(8, 10) / n, S(9, 10) / n
    v_iw, v_t, c_it = S(8, 8) - (n * m_iw) * m_iw, S(9, 9) - (n * m_t) * m_t, S(8, 9) - (n * m_iw) * m_t
    if not (v_iw > 0 and v_t > 0):
        return float("nan"), None
    rho = c_it / float(np.sqrt(v_iw * v_t))
    M = np.empty((8, 10))
    for r in range(8):
        for c in range(8):
            M[r, c] = S(r, c) - (S(r, 10) * S(c, 10)) / n
        M[r, 8], M[r, 9] = S(r, 8) - m_iw * S(r, 10), S(r, 9) - m_t * S(r, 10)
    a, cc = M[:, 8].copy(), M[:, 9].copy()
    with np.errstate(all="ignore"):
        for k in range(8):
            p, big = k, abs(M[k, k])
            for q in range(k + 1, 8):
                if abs(M[q, k]) > big:
                    p, big = q, abs(M[q, k])
            if not big > 0:
                return rho, None
            if p != k:
                M[[k, p]] = M[[p, k]]
            for r in range(k + 1, 8):
                f = M[r, k] / M[k, k]
                for c in range(k + 1, 10):
                    M[r, c] = M[r, c] - f * M[k, c]
        ya, yc = np.zeros(8), np.zeros(8)
        for i in range(7, -1, -1):
            sa, sc = M[i, 8], M[i, 9]
            for j in range(i + 1, 8):
                sa, sc = sa - M[i, j] * ya[j], sc - M[i, j] * yc[j]
            ya[i], yc[i] = sa / M[i, i], sc / M[i, i]
        da = dc = 0.0
        for i in range(8):
            da, dc = da + a[i] * ya[i], dc + cc[i] * ya[i]
        lambda_n, lambda_d = v_iw - da, c_it - dc
        if not lambda_d > 0:
            return rho, None
        d = (lambda_n / lambda_d) * yc - ya
    return (rho, d) if np.isfinite(d).all() else (rho, None)


def ecc_level_host(A_l, T_l, H, iters, mask_l=None):
    """One level: iters + 1 passes from H -> (best [3,3], rho at the first pass, rho_best, accepted steps)."""
    cur = np.asarray(H, np.float64).reshape(3, 3)
    cur = cur / cur[2, 2]
    best, rho_best, rho_first, frozen, accepted = cur.copy(), -np.inf, None, False, 0
    for k in range(iters + 1):
        rho, d = ecc_step_host(ecc_sums_host(A_l, T_l, cur, mask_l))          # (a frozen sample runs its passes too: fixed work)
        rho_first = rho if k == 0 else rho_first
        if frozen:
            continue
        if rho > rho_best:
            best, rho_best = cur.copy(), rho
            if k < iters and d is not None:
                cur = (cur.reshape(9) + np.append(d, 0.0)).reshape(3, 3)
                cur[2, 2] = 1.0
                accepted += 1
            else:
                frozen = True
        else:
            cur, frozen = best.copy(), True
    return best, rho_first, rho_best, accepted


def ecc_refine_host(images_a, images_b, H, levels=3, iters=10, mask=None):
    """images_* uint8 [B,H*,W*,3], H [B,3,3] (B's index coordinates -> A's), mask uint8 [B,Hb,Wb] or None -> (H [B,3,3] float64 with
    H[2,2] = 1, stats [B,levels,3] = (rho at the level's first pass, rho_best, accepted steps), index 0 the FINEST level)."""
    pa, pb = gray_pyramid_host(images_a, levels), gray_pyramid_host(images_b, levels)
    pm = None if mask is None else mask_pyramid_host(mask, levels)
    H = np.asarray(H, np.float64).reshape(-1, 3, 3)
    out, stats = np.empty_like(H), np.empty((H.shape[0], levels, 3))
    for b in range(H.shape[0]):
        cur = H[b] / H[b, 2, 2]
        for _ in range(levels - 1):
            cur = h_level_up(cur)
        for l in range(levels - 1, -1, -1):
            cur, stats[b, l, 0], stats[b, l, 1], stats[b, l, 2] = ecc_level_host(pa[l][b], pb[l][b], cur, iters, None if pm is None else pm[l][b])
            if l > 0:
                cur = h_level_down(cur)
        out[b] = cur
    return out, stats


# ------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------
def _model_attr(model, name):
    for m in model.modules():
        v = getattr(m, name, None)
        if isinstance(v, int) and not isinstance(v, bool):
            return v
    return None


def _images(x, what):
    """The uint8 [N,H,W,3] device tensor of an ImageBank or a tensor."""
    data = getattr(x, "data", None) if not isinstance(x, torch.Tensor) else x
    if not isinstance(data, torch.Tensor):
        raise TypeError("Aligner: %s is a uint8 [N,H,W,3] device tensor or an ImageBank, got %s" % (what, type(x).__name__))
    if not data.is_cuda:
        raise RuntimeError("Aligner: %s is on %s; bihome_amd kernels need device tensors, there is no CPU path" % (what, data.device))
    if data.dtype != torch.uint8 or data.dim() != 4 or data.shape[3] != 3 or min(data.shape) < 1:
        raise ValueError("Aligner: %s is uint8 [N,H,W,3] with N, H, W >= 1, got %s %s" % (what, data.dtype, tuple(data.shape)))
    return data.contiguous()


def _index(idx, n_images, device, what):
    """idx -> (int32 device tensor or None, B or None).  Host values are range-checked here; a device tensor is the kernel's to clamp."""
    if idx is None:
        return None, None
    if isinstance(idx, torch.Tensor) and idx.is_cuda:
        if idx.dim() != 1 or idx.dtype != torch.int32:
            raise ValueError("Aligner: %s on the device is an int32 [B] tensor, got %s %s" % (what, idx.dtype, tuple(idx.shape)))
        return idx.contiguous(), idx.shape[0]
    host = np.asarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx)
    if host.ndim != 1 or not np.issubdtype(host.dtype, np.integer):
        raise ValueError("Aligner: %s is a list of image indices, got %s %s" % (what, host.dtype, host.shape))
    for b, i in enumerate(host.tolist()):
        if not 0 <= i < n_images:
            raise ValueError("Aligner: %s of sample %d is %d, outside [0, %d)" % (what, b, i, n_images))
    return torch.from_numpy(host.astype(np.int32)).to(device), host.shape[0]


def _regions(roi, B, H, W, device, what):
    """roi (host values: one (x0, y0, rw, rh) for every sample, or [B,4]) -> float64 [B,4] device tensor, or None for whole images.
    Range-checked here, before any launch: 0 <= x0, rw > 0, x0 + rw <= W and the same for y; a ValueError names the sample."""
    if roi is None:
        return None
    if isinstance(roi, torch.Tensor):
        if roi.is_cuda:
            raise ValueError("Aligner: %s is given as host values (they are range-checked before any launch), got a device tensor" % what)
        roi = roi.numpy()
    r = np.asarray(roi, np.float64)
    if r.shape == (4,):
        r = np.tile(r, (B, 1))
    if r.shape != (B, 4):
        raise ValueError("Aligner: %s is (x0, y0, rw, rh) or [B,4] of them with B = %d, got shape %s" % (what, B, r.shape))
    for b, (x0, y0, rw, rh) in enumerate(r.tolist()):
        if not (0 <= x0 and rw > 0 and x0 + rw <= W and 0 <= y0 and rh > 0 and y0 + rh <= H):      # (False for a NaN too)
            raise ValueError("Aligner: %s of sample %d, (x0, y0, rw, rh) = (%g, %g, %g, %g), does not lie inside its %d x %d (H x W) "
                             "image with a positive extent" % (what, b, x0, y0, rw, rh, H, W))
    return torch.from_numpy(np.ascontiguousarray(r)).to(device)


def _need_device(*tensors, name=True):
    """RuntimeError unless every argument is a device tensor (name: the message says where they are)."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        got = " (got %s)" % " and ".join(str(t.device) for t in tensors) if name else ""
        raise RuntimeError("bihome_amd kernels need device tensors%s; there is no CPU path" % got)


def _need_h(H, who):
    """ValueError unless H is [B,3,3] (or [B,9]) float64."""
    if H.dtype != torch.float64 or H.dim() < 2 or H.numel() != 9 * H.shape[0]:
        raise ValueError("%s: H [B,3,3] float64, got %s %s" % (who, H.dtype, tuple(H.shape)))


def _affine_dev(geom, inverse=False):
    """geom [B,4] float64 device tensor -> A [B,3,3] (or A^-1), batched tensor arithmetic only."""
    A = torch.zeros((geom.shape[0], 3, 3), dtype=torch.float64, device=geom.device)
    sx, sy, tx, ty = geom.unbind(1)
    if inverse:
        A[:, 0, 0], A[:, 1, 1], A[:, 0, 2], A[:, 1, 2] = 1.0 / sx, 1.0 / sy, -tx / sx, -ty / sy
    else:
        A[:, 0, 0], A[:, 1, 1], A[:, 0, 2], A[:, 1, 2] = sx, sy, tx, ty
    A[:, 2, 2] = 1.0
    return A


def _inverse_device(M):
    """M [...,3,3] float64 device tensor -> M^-1, the adjugate written out over the determinant, unguarded (torch.linalg.inv would
    synchronise with the host)."""
    a, b, c, d, e, f, g, h, i = (M[..., r, k] for r in range(3) for k in range(3))
    adj = torch.stack([e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d], -1)
    det = (a * adj[..., 0] + b * adj[..., 3]) + c * adj[..., 6]
    return (adj / det[..., None]).reshape(M.shape)


def _compose_device(left, delta, P, geom_b):
    """`_compose` on the device: left [B,3,3] float64, delta [B,4,2] float32, geom_b [B,4] float64 -> H [B,3,3] float64.  The 8 x 8 solve
    is bh_h4pt_fwd's (double), the rest batched [B,3,3] double arithmetic; nothing is copied to the host."""
    B = delta.shape[0]
    Hp = K.h4pt_fwd(delta.reshape(B, 4, 2).to(torch.float32).contiguous(), P)[0].view(B, 3, 3)
    H = left @ Hp @ _affine_dev(geom_b, inverse=True)
    return (H / H[:, 2:3, 2:3]).contiguous()


def lift_device(delta_hat, P, geom_a, geom_b):
    """`lift` on the device: delta_hat [B,4,2] float32, geom_* [B,4] float64 -> H [B,3,3] float64 (`_compose_device`, left = A_a)."""
    return _compose_device(_affine_dev(geom_a), delta_hat, P, geom_b)


def prepare(images, B, patch, channels, mean=0.443, std=0.129, idx=None, roi=None):
    """bh_align_prep_u8 on outputs allocated here: (patch [B,C,P,P] float32, geom [B,4] float64) of B samples of the uint8 bank
    images [N,H,W,3]; idx [B] int32 and roi [B,4] float64 are DEVICE tensors or None (kernels.align_prep_u8)."""
    _need_device(images)
    out = torch.empty((B, channels, patch, patch), dtype=torch.float32, device=images.device)
    geom = torch.empty((B, 4), dtype=torch.float64, device=images.device)
    return K.align_prep_u8(images, out, geom, mean, std, idx=idx, roi=roi)


def warp_u8(images, H64, Ho, Wo, idx=None, want_valid=True):
    """bh_warp_u8 on outputs allocated here: (out [B,Ho,Wo,3] uint8, valid [B,Ho,Wo] uint8 or None) (kernels.warp_u8)."""
    _need_device(images)
    B = H64.shape[0]
    out = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=images.device)
    valid = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=images.device) if want_valid else None
    return K.warp_u8(images, H64, out, valid, idx=idx)


def prepare_warped(images, Hg, B, patch, channels, nx, ny, mean=0.443, std=0.129, idx=None):
    """bh_align_prep_warp_u8 on outputs allocated here: (patch [B,C,P,P] float32, cover [B,P,P] float32) of B samples of the uint8 bank
    images [N,Hs,Ws,3] seen through Hg [B,3,3] float64 (`prep_warp_host`; Hg = H @ grid_map(geom_b, nx, ny)); idx [B] int32 DEVICE tensor
    or None (kernels.align_prep_warp_u8)."""
    _need_device(images)
    out = torch.empty((B, channels, patch, patch), dtype=torch.float32, device=images.device)
    cover = torch.empty((B, patch, patch), dtype=torch.float32, device=images.device)
    return K.align_prep_warp_u8(images, Hg, out, cover, nx, ny, mean, std, idx=idx)


def patch_ncc(w, t, cover=None):
    """bh_patch_ncc on an output allocated here: w, t [B,C,P,P] float32, cover [B,P,P] float32 or None -> [B,8] float64
    (n, sum w, sum t, sum ww, sum tt, sum wt, rho, 0) (`patch_ncc_host`)."""
    _need_device(w)
    out = torch.empty((w.shape[0], 8), dtype=torch.float64, device=w.device)
    return K.patch_ncc(w, t, cover, out)


def cascade_compose_device(H_prev, delta, P, geom_b):
    """`cascade_compose` on the device: H_prev [B,3,3] float64, delta [B,4,2] float32, geom_b [B,4] float64 -> H [B,3,3] float64
    (`_compose_device`, left = H_prev A_b)."""
    return _compose_device(H_prev @ _affine_dev(geom_b), delta, P, geom_b)


def _grid_map_device(gb, nx, ny):
    """`grid_map` on the device, A_b S written out (no upload): geom_b [B,4] float64 -> [B,3,3], the sub-sample grid -> B's index
    coordinates."""
    G = _affine_dev(gb)
    G[:, 0, 2] += G[:, 0, 0] * (0.5 / nx - 0.5)
    G[:, 1, 2] += G[:, 1, 1] * (0.5 / ny - 0.5)
    G[:, 0, 0] *= 1.0 / nx
    G[:, 1, 1] *= 1.0 / ny
    return G


def _cascade_samples(samples, roi_b, Hb, Wb, P):
    """(nx, ny): given, or min(8, max(1, ceil(s))) per axis with s the largest rw_b / P (rh_b / P) of the batch - host values only."""
    if samples is not None:
        try:
            nx, ny = (operator.index(v) for v in samples)
        except (TypeError, ValueError):
            raise ValueError("Aligner: cascade_samples is (nx, ny), two integers in 1..8, got %r" % (samples,)) from None
        if not (1 <= nx <= 8 and 1 <= ny <= 8):
            raise ValueError("Aligner: cascade_samples is (nx, ny), two integers in 1..8, got %r" % (samples,))
        return nx, ny
    if roi_b is None:
        rw, rh = float(Wb), float(Hb)
    else:
        r = np.asarray(roi_b.numpy() if isinstance(roi_b, torch.Tensor) else roi_b, np.float64).reshape(-1, 4)
        rw, rh = float(r[:, 2].max()), float(r[:, 3].max())
    return tuple(min(8, max(1, int(np.ceil(s / P)))) for s in (rw, rh))


def gray_pyramid(images, B, levels, idx=None):
    """bh_gray_pyramid_u8 on an output allocated here: pyr [B,total] float32, the gray box pyramids of B samples of the uint8 bank
    images [N,H,W,3] with the levels packed one after another (`pyramid_offsets`; `pyramid_level` views one).  idx [B] int32 DEVICE
    tensor or None.  ValueError, before any launch, for levels the images are too small for."""
    _need_device(images)
    total = int(pyramid_offsets(images.shape[1], images.shape[2], levels)[-1])
    pyr = torch.empty((B, total), dtype=torch.float32, device=images.device)
    return K.gray_pyramid_u8(images, pyr, levels, idx=idx)


def pyramid_level(pyr, h, w, levels, l):
    """The [B,h_l,w_l] view of level l inside a packed pyramid [B,total] of h x w images (float planes or mask bytes)."""
    off, (hl, wl) = pyramid_offsets(h, w, levels), pyramid_sizes(h, w, levels)[l]
    return pyr[:, int(off[l]):int(off[l + 1])].view(pyr.shape[0], hl, wl)


def mask_pyramid(mask, levels):
    """mask [B,H,W] uint8 device tensor -> uint8 [B,total] in the pyramid's layout: level 0 is mask != 0, level l is 1 where all four
    bytes of the 2 x 2 block below are (tensor slicing and & on the device)."""
    B, h, w = mask.shape
    sizes = pyramid_sizes(h, w, levels)
    cur, parts = (mask != 0).to(torch.uint8), []
    for l in range(levels):
        if l:
            hl, wl = sizes[l]
            cur = cur[:, 0:2 * hl:2, 0:2 * wl:2] & cur[:, 0:2 * hl:2, 1:2 * wl:2] & cur[:, 1:2 * hl:2, 0:2 * wl:2] & cur[:, 1:2 * hl:2, 1:2 * wl:2]
        parts.append(cur.reshape(B, -1))
    return torch.cat(parts, 1).contiguous()


def ecc_sums(a, t, H64, mask=None):
    """bh_ecc_sums on buffers allocated here: a [B,Ha,Wa], t [B,Hb,Wb] float32 gray planes of one level (`pyramid_level` views),
    H64 [B,3,3] float64, mask [B,Hb,Wb] uint8 or None -> sums [B,66] float64 (`ecc_sums_host`)."""
    _need_device(a)
    B = H64.shape[0]
    partial = torch.empty((K.ecc_sums_ws_doubles(t.shape[1], t.shape[2], B),), dtype=torch.float64, device=a.device)
    sums = torch.empty((B, ECC_SUMS), dtype=torch.float64, device=a.device)
    return K.ecc_sums(a, t, H64, partial, sums, mask=mask)


def ecc_state(H64):
    """The state [B,24] float64 of a level that starts at H64 [B,3,3] (include/bihome.h bh_ecc_step): cur = best = H / H[2,2],
    rho_best = -inf, nothing frozen, counters 0."""
    B = H64.shape[0]
    state = torch.zeros((B, K.ECC_STATE), dtype=torch.float64, device=H64.device)
    h = H64.reshape(B, 9) / H64.reshape(B, 9)[:, 8:9]
    state[:, 0:9], state[:, 9:18], state[:, 18] = h, h, float("-inf")
    return state


def ecc_step(sums, state, last=0):
    """bh_ecc_step in place on `state`; -> (state, stats [B,3] float64 (written when last != 0))."""
    stats = torch.zeros((state.shape[0], 3), dtype=torch.float64, device=state.device)
    K.ecc_step(sums, state, last=last, stats=stats)
    return state, stats


def ecc_refine_pyramids(pyr_a, size_a, pyr_b, size_b, H64, levels, iters, mask_pyr=None):
    """bh_ecc_refine on pyramids already built: -> (H [B,3,3] float64, stats [B,levels,3] float64); H64 itself is left as it is."""
    B = H64.shape[0]
    H = H64.reshape(B, 3, 3).clone()
    stats = torch.empty((B, levels, 3), dtype=torch.float64, device=H64.device)
    ws = torch.empty((K.ecc_refine_ws_doubles(size_b[0], size_b[1], B),), dtype=torch.float64, device=H64.device)
    return K.ecc_refine(pyr_a, size_a, pyr_b, size_b, H, stats, ws, levels, iters, mask_pyr=mask_pyr)


def _check_mask(mask, B, Hb, Wb, device):
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.device != device:
        raise ValueError("ecc_refine: mask is a uint8 [B,Hb,Wb] tensor on the images' device")
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (B, Hb, Wb):
        raise ValueError("ecc_refine: mask is uint8 [B,Hb,Wb] = [%d,%d,%d], got %s %s" % (B, Hb, Wb, mask.dtype, tuple(mask.shape)))
    return mask.contiguous()


def _refine_args(levels, iters, sizes, iters_label):
    """The refinement's argument rules, checked before any launch: `pyramid_sizes` of every (label, (h, w)) of `sizes`, and iters >= 0; the
    labels open the messages with the caller's name for the argument."""
    for label, (h, w) in sizes:
        try:
            pyramid_sizes(h, w, levels)
        except ValueError as e:
            raise ValueError("%s: %s" % (label, e)) from None
    if not iters >= 0:
        raise ValueError("%s >= 0, got %r" % (iters_label, iters))


def ecc_refine(images_a, images_b, H, levels=3, iters=10, idx_a=None, idx_b=None, mask=None):
    """Coarse-to-fine ECC refinement on the device (`ecc_refine_host`): images_* uint8 [N,H*,W*,3] device tensors, H [B,3,3] float64 (B's
    index coordinates -> A's), idx_* [B] int32 DEVICE tensors or None, mask [B,Hb,Wb] uint8 or None (non-zero: the pixel of B may count)
    -> (H [B,3,3] float64 with H[2,2] = 1, stats [B,levels,3] = (rho at the level's first pass, rho_best, accepted steps), index 0 the
    finest level).  ValueError, before any launch, for levels too deep for the images.  Nothing is copied to the host."""
    _need_device(images_a, images_b, H, name=False)
    _need_h(H, "ecc_refine")
    B, (Ha, Wa), (Hb, Wb) = H.shape[0], images_a.shape[1:3], images_b.shape[1:3]
    _refine_args(levels, iters, (("ecc_refine: images_a", (Ha, Wa)), ("ecc_refine: images_b", (Hb, Wb))), "ecc_refine: iters")
    mask = _check_mask(mask, B, Hb, Wb, images_b.device)
    pa, pb = gray_pyramid(images_a, B, levels, idx=idx_a), gray_pyramid(images_b, B, levels, idx=idx_b)
    return ecc_refine_pyramids(pa, (Ha, Wa), pb, (Hb, Wb), H.contiguous(), levels, iters, mask_pyr=None if mask is None else mask_pyramid(mask, levels))


# ------------------------------------------------------------------------------------------------
# mosaic, the device path
# ------------------------------------------------------------------------------------------------
def mosaic_frame_device(H, size_a, size_b, canvas, limit=2.0):
    """`mosaic_frame_host` on the device: H [B,3,3] float64 -> (T [B,3,3] float64, bbox [B,4] float64, fitted [B] uint8) - bh_pano_frame
    for the single frame A around the reference B (`pano_frame_device`): one launch, nothing copied to the host."""
    _frame_args(canvas, limit, "mosaic_frame")
    T, bbox, fitted, _ = pano_frame_device(H.reshape(-1, 1, 3, 3), size_a, canvas, limit, ref_size=size_b, want_M=False)
    return T, bbox, fitted[:, 0].contiguous()


def exposure_device(sums):
    """`exposure_host` on the device: sums [B,66] float64 (`ecc_sums` at level 0) -> [B,2] float64 (g, o), the fallbacks by torch.where."""
    S = lambda i, j: sums[:, ecc_index(i, j)]
    n = S(10, 10)
    m_iw, m_t = S(8, 10) / n, S(9, 10) / n
    v_iw, c_it = S(8, 8) - (n * m_iw) * m_iw, S(8, 9) - (n * m_iw) * m_t
    g = c_it / v_iw
    ok = (n >= ECC_MIN_N) & (v_iw > 0) & torch.isfinite(g) & (g > 0)
    return torch.stack([torch.where(ok, g, torch.ones_like(g)), torch.where(ok, m_t - g * m_iw, torch.zeros_like(g))], 1)


def measure_exposure(a, b, H, ia=None, ib=None, mask=None):
    """The exposure 'gain' of B samples on the device: a, b uint8 banks, H [B,3,3] float64 (b's index coordinates -> a's), ia / ib [B]
    int32 device tensors or None, mask uint8 [B,Hb,Wb] or None (non-zero: the pixel of b may count) -> [B,2] float64 (g, o), the
    least-squares line of b's gray on a's through H - a one-level `gray_pyramid` of both, `ecc_sums`, `exposure_device`."""
    B, (Ha, Wa), (Hb, Wb) = H.shape[0], a.shape[1:3], b.shape[1:3]
    pa, pb = gray_pyramid(a, B, 1, idx=ia), gray_pyramid(b, B, 1, idx=ib)
    return exposure_device(ecc_sums(pyramid_level(pa, Ha, Wa, 1, 0), pyramid_level(pb, Hb, Wb, 1, 0), H, mask=mask))


def mosaic_u8(images_a, images_b, Ma, Mb, Hc, Wc, feather=32.0, mode="feather", gain=None, idx_a=None, idx_b=None, want_cover=True):
    """bh_mosaic_u8 on outputs allocated here: (out [B,Hc,Wc,3] uint8, cover [B,Hc,Wc] uint8 or None) (kernels.mosaic_u8; `mosaic_host`)."""
    _need_device(images_a, images_b)
    B = Ma.shape[0]
    out = torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device=images_a.device)
    cover = torch.empty((B, Hc, Wc), dtype=torch.uint8, device=images_a.device) if want_cover else None
    return K.mosaic_u8(images_a, images_b, Ma, Mb, out, cover, feather, mode, gain=gain, idx_a=idx_a, idx_b=idx_b)


# noun -> (the canvas keyword, what it names, the modes, what `limit` counts image sizes around)
_CANVAS_KINDS = {"mosaic": ("b", "image B's grid", MOSAIC_MODES, "B"), "panorama": ("ref", "the reference frame's grid", PANO_MODES, "the reference")}


def _canvas_args(noun, canvas, feather, mode, limit, who):
    """The host-side rules of the canvas, feather, mode and limit of a mosaic (`mosaic`, Aligner(mosaic=)) or a panorama (`panorama`,
    Aligner.sequence(canvas=)), checked before any launch -> (Hc, Wc), or None for the canvas keyword ('b' / 'ref')."""
    keyword, grid, modes, around = _CANVAS_KINDS[noun]
    size = None
    if not (isinstance(canvas, str) and canvas == keyword):
        try:
            size = tuple(operator.index(v) for v in canvas)
        except (TypeError, ValueError):
            size = ()
        if len(size) != 2:
            raise ValueError("%s: the %s canvas is %r (%s) or (Hc, Wc), got %r" % (who, noun, keyword, grid, canvas))
        if min(size) < 2:
            raise ValueError("%s: a %s canvas has at least 2 pixels on each side, got %d x %d (H x W)" % (who, noun, size[0], size[1]))
    try:
        feather_ok = bool(1.0 <= float(feather) < float("inf"))                # (False for a NaN too)
    except (TypeError, ValueError):
        feather_ok = False
    if not feather_ok:
        raise ValueError("%s: the %s feather is finite and at least 1 (pixels), got %r" % (who, noun, feather))
    if not (isinstance(mode, str) and mode in modes + BAND_MODES):
        raise ValueError("%s: the %s mode is one of %s, got %r" % (who, noun, ", ".join(modes + BAND_MODES), mode))
    try:
        limit_ok = bool(float(limit) > 0)
    except (TypeError, ValueError):
        limit_ok = False
    if not limit_ok:
        raise ValueError("%s: the %s limit (image sizes around %s that the frame may reach) is > 0, got %r" % (who, noun, around, limit))
    return size


def _mosaic_exposure_args(exposure, B, size_a, size_b, who, name):
    """The rules of the mosaic's exposure (`name`: what the caller calls the argument), checked before any launch."""
    if isinstance(exposure, torch.Tensor):
        if not exposure.is_cuda or exposure.dtype != torch.float64 or exposure.dim() != 2 or exposure.shape[1] != 2:
            raise ValueError("%s: the mosaic exposure as a tensor is [B,2] float64 (g, o) on the device, got %s %s on %s"
                             % (who, exposure.dtype, tuple(exposure.shape), exposure.device))
        if exposure.shape[0] != B:
            raise ValueError("%s: %s [B,2] with B = %d, got %s" % (who, name, B, tuple(exposure.shape)))
    elif exposure == "gain":
        for (h, w), what in ((size_a, "images_a"), (size_b, "images_b")):
            if min(h, w) < ECC_MIN_SIDE:
                raise ValueError("%s: the mosaic exposure 'gain' measures on the gray images, which need at least %d pixels on each side; "
                                 "%s is %d x %d (H x W)" % (who, ECC_MIN_SIDE, what, h, w))
    elif exposure is not None:
        raise ValueError("%s: the mosaic exposure is None, 'gain' or a [B,2] float64 device tensor (g, o), got %r" % (who, exposure))


def _identity_canvas(B, H, W, fitted_shape, device):
    """The canvas that is the reference's own H x W grid: (T = I [B,3,3], bbox = (0, 0, W - 1, H - 1) [B,4], fitted = 0 of fitted_shape)."""
    T = torch.zeros((B, 3, 3), dtype=torch.float64, device=device)
    T[:, 0, 0] = T[:, 1, 1] = T[:, 2, 2] = 1.0
    bbox = torch.zeros((B, 4), dtype=torch.float64, device=device)
    bbox[:, 2], bbox[:, 3] = W - 1.0, H - 1.0
    return T, bbox, torch.zeros(fitted_shape, dtype=torch.uint8, device=device)


def _mosaic(a, b, H, size, feather, mode, exposure, limit, ia, ib, mask_b, band_sigma=None):
    """The mosaic stage on checked arguments (a, b: uint8 banks on the device, ia / ib: int32 device tensors or None) -> its six keys (in
    the two-band mode, whose low bands of sigma band_sigma are made here with one launch per image: seven, with 'mosaic_winner')."""
    B, dev, (Ha, Wa), (Hb, Wb) = H.shape[0], H.device, a.shape[1:3], b.shape[1:3]
    H = H.reshape(B, 3, 3).contiguous()
    if size is None:
        Hc, Wc, Ma = Hb, Wb, H
        T, bbox, fitted = _identity_canvas(B, Hb, Wb, (B,), dev)
    else:
        Hc, Wc = size
        T, bbox, fitted = mosaic_frame_device(H, (Ha, Wa), (Hb, Wb), (Hc, Wc), limit)
        Ma = (H @ T).contiguous()                                              # (torch's product, not the frame kernel's M: other roundings)
    if isinstance(exposure, torch.Tensor):
        gain = exposure.contiguous()
    elif exposure == "gain":
        gain = measure_exposure(a, b, H, ia, ib, mask_b).contiguous()
    else:
        gain = None
    extra = {}
    if mode in BAND_MODES:
        out, cover, extra["mosaic_winner"] = mosaic_bands_u8(a, blur_u8(a, band_sigma, ia), b, blur_u8(b, band_sigma, ib), Ma, T, Hc, Wc, feather,
                                                             gain=gain, idx_a=ia, idx_b=ib)
    else:
        out, cover = mosaic_u8(a, b, Ma, T, Hc, Wc, feather, mode, gain=gain, idx_a=ia, idx_b=ib)
    if gain is None:
        gain = torch.zeros((B, 2), dtype=torch.float64, device=dev)
        gain[:, 0] = 1.0
    return {"mosaic": out, "mosaic_cover": cover, "mosaic_T": T, "mosaic_bbox": bbox, "mosaic_fitted": fitted, "mosaic_gain": gain, **extra}


def mosaic(images_a, images_b, H, canvas="b", feather=32.0, mode="feather", exposure=None, limit=2.0, idx_a=None, idx_b=None, mask_b=None,
           band_sigma=4.0):
    """Both images on one canvas, for a caller who has H [B,3,3] float64 (B's index coordinates -> A's) from anywhere: images_* uint8
    [N,H*,W*,3] device tensors or ImageBanks, idx_* as in `Aligner`.  canvas="b": the canvas is B's grid (T the identity);
    canvas=(Hc, Wc): the frame `mosaic_frame_device` fits around B and A's projected corners, `limit` image sizes around B at most.
    feather / mode: `mosaic_host`.  exposure: None, "gain" (A's gray is matched to B's by the least-squares line through H over the
    pixels the ECC pass counts - one-level `gray_pyramid` of both, `ecc_sums` (mask_b uint8 [B,Hb,Wb]: non-zero, the pixel of B may
    count), `exposure_device`) or a [B,2] float64 device tensor (g, o).  -> dict: 'mosaic' [B,Hc,Wc,3] uint8, 'mosaic_cover'
    [B,Hc,Wc] uint8 (0 empty, 1 only A, 2 only B, 3 both), 'mosaic_T' [B,3,3] float64 (canvas -> B), 'mosaic_bbox' [B,4] float64
    (xmin, ymin, xmax, ymax in B's coordinates), 'mosaic_fitted' [B] uint8 (A's corners took part in the frame), 'mosaic_gain' [B,2]
    float64.  mode="two_band" (`mosaic_bands_host`; band_sigma in [0.5, 10.5], a default and not a tuned value, in each image's own
    pixels; the other modes do not look at it): each image is split by `blur_u8` into a low band, blended with the feather, and a high
    band, taken per pixel from the image with the larger weight - and 'mosaic_winner' [B,Hc,Wc] uint8 (0: A, 1: B, 255: neither) is
    added; the exposure applies to both bands.  ValueError before any launch for arguments outside these; nothing is copied to the host."""
    a, b = _images(images_a, "images_a"), _images(images_b, "images_b")
    _need_device(H, name=False)
    if a.device != b.device or H.device != a.device:
        raise ValueError("mosaic: images_a is on %s, images_b on %s, H on %s" % (a.device, b.device, H.device))
    _need_h(H, "mosaic")
    B = H.shape[0]
    size = _canvas_args("mosaic", canvas, feather, mode, limit, "mosaic")
    _band_args(mode, band_sigma, "mosaic", "mosaic")
    _mosaic_exposure_args(exposure, B, a.shape[1:3], b.shape[1:3], "mosaic", "exposure")
    ia, na = _index(idx_a, a.shape[0], a.device, "idx_a")
    ib, nb = _index(idx_b, b.shape[0], b.device, "idx_b")
    for n, what in ((a.shape[0] if na is None else na, "images_a"), (b.shape[0] if nb is None else nb, "images_b")):
        if n != B:
            raise ValueError("mosaic: %d samples of %s, H has %d" % (n, what, B))
    if mask_b is not None and not (isinstance(exposure, str) and exposure == "gain"):
        raise ValueError("mosaic: mask_b restricts the pixels the exposure measurement counts; pass exposure='gain' with it")
    mask_b = _check_mask(mask_b, B, b.shape[1], b.shape[2], b.device)
    with torch.cuda.device(a.device):
        return _mosaic(a, b, H, size, feather, mode, exposure, limit, ia, ib, mask_b, band_sigma)


# ------------------------------------------------------------------------------------------------
# panorama, the device path
# ------------------------------------------------------------------------------------------------
def chain_device(H_pairs, ref, gain_pairs=None):
    """bh_pano_chain on outputs allocated here (`chain_host`): H_pairs [B,n-1,3,3] float64, gain_pairs [B,n-1,2] float64 or None ->
    (G [B,n,3,3] float64, gain [B,n,2] float64 or None)."""
    _need_device(H_pairs)
    if H_pairs.dim() != 4 or tuple(H_pairs.shape[2:]) != (3, 3):
        raise ValueError("chain_device: H_pairs [B,n-1,3,3] float64, got %s" % (tuple(H_pairs.shape),))
    B, n = H_pairs.shape[0], H_pairs.shape[1] + 1
    G = torch.empty((B, n, 3, 3), dtype=torch.float64, device=H_pairs.device)
    gain = None if gain_pairs is None else torch.empty((B, n, 2), dtype=torch.float64, device=H_pairs.device)
    return K.pano_chain(H_pairs.contiguous(), ref, G, None if gain_pairs is None else gain_pairs.contiguous(), gain)


def pano_frame_device(G, size, canvas, limit=2.0, use=None, ref_size=None, want_M=True):
    """bh_pano_frame on outputs allocated here (`pano_frame_host`): G [B,n,3,3] float64, use [B,n] uint8 or None, ref_size = (Hr, Wr) of
    the reference (None: size) -> (T [B,3,3] float64, bbox [B,4] float64, fitted [B,n] uint8, M [B,n,3,3] float64 = G T or None): one
    launch."""
    _need_device(G)
    _frame_args(canvas, limit, "pano_frame")
    if G.dim() != 4:
        raise ValueError("pano_frame: G [B,n,3,3] float64, got %s" % (tuple(G.shape),))
    B, n = G.shape[:2]
    T = torch.empty((B, 3, 3), dtype=torch.float64, device=G.device)
    bbox = torch.empty((B, 4), dtype=torch.float64, device=G.device)
    fitted = torch.empty((B, n), dtype=torch.uint8, device=G.device)
    M = torch.empty((B, n, 3, 3), dtype=torch.float64, device=G.device) if want_M else None
    return K.pano_frame(G.contiguous(), size, canvas, limit, T, bbox, fitted, M, use=use, ref_size=ref_size)


def pano_u8(images, idx, M, Hc, Wc, feather=32.0, mode="feather", gain=None, use=None, want_count=True):
    """bh_pano_u8 on outputs allocated here: (out [B,Hc,Wc,3] uint8, count [B,Hc,Wc] uint8 or None) (kernels.pano_u8; `pano_host`)."""
    _need_device(images)
    B = M.shape[0]
    out = torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device=images.device)
    count = torch.empty((B, Hc, Wc), dtype=torch.uint8, device=images.device) if want_count else None
    return K.pano_u8(images, idx, M, out, count, feather, mode, gain=gain, use=use)


# ------------------------------------------------------------------------------------------------
# global adjustment, the device path
# ------------------------------------------------------------------------------------------------
def adjust_device(G0, links, H_links, weight, ref, size, grid=4, iters=10):
    """bh_pano_adjust on G, work and a workspace allocated here (`adjust_host`): G0 [B,n,3,3] float64, links [E,2] int32 ON THE DEVICE,
    H_links [B,E,3,3] float64, weight [B,E] float64 or None -> (G [B,n,3,3] float64, work [B,4] float64): one launch."""
    _need_device(G0, links, H_links)
    if G0.dim() != 4 or links.dim() != 2:
        raise ValueError("adjust_device: G0 [B,n,3,3] float64 and links [E,2] int32, got %s and %s" % (tuple(G0.shape), tuple(links.shape)))
    B, n, E = G0.shape[0], G0.shape[1], links.shape[0]
    G = torch.empty((B, n, 3, 3), dtype=torch.float64, device=G0.device)
    work = torch.empty((B, 4), dtype=torch.float64, device=G0.device)
    ws = torch.empty((K.pano_adjust_ws_doubles(n, E, B),), dtype=torch.float64, device=G0.device)
    return K.pano_adjust(G0.contiguous(), links.contiguous(), H_links.contiguous(), None if weight is None else weight.contiguous(), ref, size, grid, iters,
                         G, work, ws)


def _adjust_args(links, n, ref, grid, iters, who, pairs=()):
    """The host-side rules of the adjustment, checked before any launch -> the links as a list of (a, b): every link is two distinct
    frames of the sequence and none repeats one of `pairs` (in either order); 2 <= n <= 64, at most 1024 edges with the pairs, the grid in
    2..8, iters >= 0."""
    try:
        out = [(operator.index(a), operator.index(b)) for a, b in links]
    except (TypeError, ValueError):
        raise ValueError("%s: links is a host list of (a, b) frame pairs, got %r" % (who, links)) from None
    if not 2 <= n <= ADJUST_MAX_FRAMES:
        raise ValueError("%s: the adjustment takes 2 <= n <= %d frames, got %d" % (who, ADJUST_MAX_FRAMES, n))
    if not 1 <= len(out) + len(pairs) <= ADJUST_MAX_EDGES:
        raise ValueError("%s: the adjustment takes 1..%d edges, got %d" % (who, ADJUST_MAX_EDGES, len(out) + len(pairs)))
    taken = {frozenset(p) for p in pairs}
    for a, b in out:
        if not (0 <= a < n and 0 <= b < n and a != b):
            raise ValueError("%s: a link is two distinct frames of the sequence, indices in [0, %d), got (%d, %d)" % (who, n, a, b))
        if frozenset((a, b)) in taken:
            raise ValueError("%s: the link (%d, %d) repeats a pair of the chain" % (who, a, b))
    try:
        ok = 2 <= operator.index(grid) <= 8 and operator.index(iters) >= 0 and 0 <= operator.index(ref) < n
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("%s: the adjustment's grid is an integer in 2..8, its iters an integer >= 0 and ref a frame in [0, %d), got %r, %r and %r"
                         % (who, n, grid, iters, ref))
    return out


def adjust(G, links, H_links, size, ref, weight=None, grid=4, iters=10):
    """The global adjustment for a caller who has the chain and the links from anywhere: G [B,n,3,3] float64 device tensor (the reference's
    index coordinates -> frame k's, 2 <= n <= 64), links a HOST list of 1..1024 edges (a, b), two distinct frames each (range-checked here
    and uploaded), H_links [B,E,3,3] float64 device tensor (b's index coordinates -> a's), size = (Hs, Ws) of the frames, ref the
    reference frame, weight [B,E] float64 device tensor or None (an edge counts iff its weight is finite and > 0), grid the side of the
    control lattice, iters the Levenberg-Marquardt steps (`adjust_host`) -> dict: 'G' [B,n,3,3] float64, 'adjust_stats' [B,4] float64
    (cost at the start, cost at the result, accepted steps, final lambda).  ValueError before any launch for arguments outside these;
    nothing is copied to the host."""
    _need_device(G, H_links, name=False)
    if G.dtype != torch.float64 or G.dim() != 4 or tuple(G.shape[2:]) != (3, 3):
        raise ValueError("adjust: G [B,n,3,3] float64, got %s %s" % (G.dtype, tuple(G.shape)))
    B, n = G.shape[:2]
    edges = _adjust_args(links, n, ref, grid, iters, "adjust")
    E = len(edges)
    if H_links.dtype != torch.float64 or H_links.device != G.device or H_links.dim() < 3 or tuple(H_links.shape[:2]) != (B, E) or H_links.numel() != 9 * B * E:
        raise ValueError("adjust: H_links [B,E,3,3] float64 on G's device with B = %d, E = %d, got %s %s" % (B, E, H_links.dtype, tuple(H_links.shape)))
    if weight is not None and not (isinstance(weight, torch.Tensor) and weight.is_cuda and weight.dtype == torch.float64 and tuple(weight.shape) == (B, E)):
        raise ValueError("adjust: weight is a [B,E] = [%d,%d] float64 device tensor or None" % (B, E))
    try:
        size_ok = len(size) == 2 and min(operator.index(v) for v in size) >= 2
    except TypeError:
        size_ok = False
    if not size_ok:
        raise ValueError("adjust: size is (Hs, Ws), at least 2 pixels on each side, got %r" % (size,))
    with torch.cuda.device(G.device):
        link = torch.tensor(edges, dtype=torch.int32).to(G.device)
        out, work = adjust_device(G, link, H_links, weight, operator.index(ref), (int(size[0]), int(size[1])), operator.index(grid), operator.index(iters))
    return {"G": out, "adjust_stats": work}


# ------------------------------------------------------------------------------------------------
# two-band blend, the device path
# ------------------------------------------------------------------------------------------------
def blur_u8(images, sigma, idx=None):
    """bh_blur_u8 on an output allocated here (`blur_host`): images a uint8 [N,H,W,3] device tensor, idx an int32 device tensor of any
    shape S (clamped by the kernel) or None (S = [N]) -> the low bands, uint8 [*S,H,W,3]: one launch."""
    _need_device(images)
    shape = (images.shape[0],) if idx is None else tuple(idx.shape)
    out = torch.empty((int(np.prod(shape)),) + tuple(images.shape[1:]), dtype=torch.uint8, device=images.device)
    return K.blur_u8(images, out, blur_taps(sigma).tolist(), idx=idx).view(shape + tuple(images.shape[1:]))


def pano_bands_u8(images, low, idx, M, Hc, Wc, feather=32.0, gain=None, use=None, want_count=True, want_winner=True):
    """bh_pano_bands_u8 on outputs allocated here: (out [B,Hc,Wc,3], count [B,Hc,Wc] or None, winner [B,Hc,Wc] or None), uint8
    (kernels.pano_bands_u8; `bands_host`)."""
    _need_device(images, low)
    B = M.shape[0]
    out = torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device=images.device)
    count = torch.empty((B, Hc, Wc), dtype=torch.uint8, device=images.device) if want_count else None
    winner = torch.empty((B, Hc, Wc), dtype=torch.uint8, device=images.device) if want_winner else None
    return K.pano_bands_u8(images, low, idx, M, out, count, winner, feather, gain=gain, use=use)


def mosaic_bands_u8(images_a, low_a, images_b, low_b, Ma, Mb, Hc, Wc, feather=32.0, gain=None, idx_a=None, idx_b=None, want_cover=True,
                    want_winner=True):
    """bh_mosaic_bands_u8 on outputs allocated here: (out [B,Hc,Wc,3], cover [B,Hc,Wc] or None, winner [B,Hc,Wc] or None), uint8
    (kernels.mosaic_bands_u8; `mosaic_bands_host`)."""
    _need_device(images_a, low_a, images_b, low_b)
    B = Ma.shape[0]
    out = torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device=images_a.device)
    cover = torch.empty((B, Hc, Wc), dtype=torch.uint8, device=images_a.device) if want_cover else None
    winner = torch.empty((B, Hc, Wc), dtype=torch.uint8, device=images_a.device) if want_winner else None
    return K.mosaic_bands_u8(images_a, low_a, images_b, low_b, Ma, Mb, out, cover, winner, feather, gain=gain, idx_a=idx_a, idx_b=idx_b)


def _band_args(mode, band_sigma, noun, who, name="band_sigma"):
    """The rule of the low band's sigma in the two-band mode, checked before any launch (the other modes do not look at it)."""
    if not (isinstance(mode, str) and mode in BAND_MODES):
        return
    try:
        ok = not isinstance(band_sigma, (str, bytes)) and bool(BAND_SIGMA_MIN <= float(band_sigma) <= BAND_SIGMA_MAX)      # (False for a NaN too)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: the %s %s (the low band's Gaussian, in the frame's own pixels) is in [%g, %g], got %r"
                         % (who, noun, name, BAND_SIGMA_MIN, BAND_SIGMA_MAX, band_sigma))


def _frames_index(idx, n_images, device, who):
    """idx -> int32 [B,n] device tensor.  None: one sample of all the bank's images in order; host values are range-checked here, a
    device tensor is the kernel's to clamp."""
    if idx is None:
        if n_images > PANO_MAX_FRAMES:
            raise ValueError("%s: idx=None takes the whole bank as one sequence, at most %d frames; the bank has %d" % (who, PANO_MAX_FRAMES, n_images))
        return torch.arange(n_images, dtype=torch.int32, device=device).reshape(1, n_images)
    if isinstance(idx, torch.Tensor) and idx.is_cuda:
        if idx.dim() != 2 or idx.dtype != torch.int32 or not 1 <= idx.shape[1] <= PANO_MAX_FRAMES:
            raise ValueError("%s: idx on the device is an int32 [B,n] tensor with 1 <= n <= %d, got %s %s" % (who, PANO_MAX_FRAMES, idx.dtype, tuple(idx.shape)))
        return idx.contiguous()
    host = np.asarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx)
    if host.ndim != 2 or not np.issubdtype(host.dtype, np.integer) or not 1 <= host.shape[1] <= PANO_MAX_FRAMES:
        raise ValueError("%s: idx is [B,n] image indices with 1 <= n <= %d, got %s %s" % (who, PANO_MAX_FRAMES, host.dtype, host.shape))
    for b, row in enumerate(host.tolist()):
        for k, i in enumerate(row):
            if not 0 <= i < n_images:
                raise ValueError("%s: idx of sample %d, frame %d is %d, outside [0, %d)" % (who, b, k, i, n_images))
    return torch.from_numpy(host.astype(np.int32)).to(device)


def _pano_tensor(t, shape, dtype, what, who):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != shape:
        got = "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else repr(t)
        raise ValueError("%s: the panorama %s is a %s %s device tensor, got %s" % (who, what, dtype, list(shape), got))
    return t.contiguous()


def _low_arg(low, mode, shape, device, who):
    """The rules of a precomputed low bank, checked before any launch: it belongs to the two-band mode and is a uint8 device tensor of
    `shape` on the images' device."""
    if low is None:
        return None
    if not (isinstance(mode, str) and mode in BAND_MODES):
        raise ValueError("%s: low is the two-band mode's low bank; pass mode='two_band' with it (got mode %r)" % (who, mode))
    if not isinstance(low, torch.Tensor) or not low.is_cuda or low.device != device or low.dtype != torch.uint8 or tuple(low.shape) != shape:
        got = "%s %s on %s" % (low.dtype, tuple(low.shape), low.device) if isinstance(low, torch.Tensor) else repr(low)
        raise ValueError("%s: low is a uint8 %s tensor on %s (`blur_u8(images, band_sigma, idx)`), got %s" % (who, list(shape), device, got))
    return low.contiguous()


def _panorama(images, idx, G, size, feather, mode, gain, use, limit, band_sigma=None, low=None):
    """The panorama stage on checked arguments -> its seven keys (in the two-band mode, whose low bank is `low` or made here with one
    launch: eight, with 'panorama_winner')."""
    B, n = G.shape[:2]
    dev, (Hs, Ws) = G.device, images.shape[1:3]
    if size is None:
        Hc, Wc, M = Hs, Ws, G
        T, bbox, fitted = _identity_canvas(B, Hs, Ws, (B, n), dev)
    else:
        Hc, Wc = size
        T, bbox, fitted, M = pano_frame_device(G, (Hs, Ws), (Hc, Wc), limit, use=use)
    extra = {}
    if mode in BAND_MODES:
        low = blur_u8(images, band_sigma, idx) if low is None else low
        out, count, extra["panorama_winner"] = pano_bands_u8(images, low, idx, M, Hc, Wc, feather, gain=gain, use=use)
    else:
        out, count = pano_u8(images, idx, M, Hc, Wc, feather, mode, gain=gain, use=use)
    if gain is None:
        gain = torch.zeros((B, n, 2), dtype=torch.float64, device=dev)
        gain[:, :, 0] = 1.0
    return {"panorama": out, "panorama_count": count, "panorama_T": T, "panorama_bbox": bbox, "panorama_fitted": fitted, "panorama_M": M,
            "panorama_gain": gain, **extra}


def panorama(images, G, idx=None, canvas="ref", feather=32.0, mode="feather", gain=None, use=None, limit=2.0, band_sigma=4.0, low=None):
    """The n frames of a sequence on one canvas, for a caller who has G [B,n,3,3] float64 (the reference's index coordinates -> frame
    k's, the identity for the reference) from anywhere: images a uint8 [N,Hs,Ws,3] device tensor or an ImageBank, idx [B,n] (host values:
    range-checked; int32 device tensor: clamped by the kernel; None: one sample of all N images in order).  canvas="ref": the canvas is
    the reference's grid (T the identity, M = G, no frame launch); canvas=(Hc, Wc): the frame `pano_frame_device` fits around the
    reference and every usable frame's projected corners, `limit` image sizes around the reference at most.  feather / mode: `pano_host`.
    gain [B,n,2] float64 device tensor (g, o) per frame, use [B,n] uint8 device tensor (0: the frame is left out), or None.  -> dict:
    'panorama' [B,Hc,Wc,3] uint8, 'panorama_count' [B,Hc,Wc] uint8 (frames present), 'panorama_T' [B,3,3] float64 (canvas -> reference),
    'panorama_bbox' [B,4] float64, 'panorama_fitted' [B,n] uint8, 'panorama_M' [B,n,3,3] float64 (canvas -> frame k), 'panorama_gain'
    [B,n,2] float64.  mode="two_band" (`bands_host`; band_sigma in [0.5, 10.5], a default and not a tuned value, in the frames' own
    pixels; the other modes do not look at it): every frame is split into a low band, blended with the feather, and a high band, taken
    per pixel from the frame with the largest weight - and 'panorama_winner' [B,Hc,Wc] uint8 (that frame's k, 255 for none) is added;
    the gain applies to both bands.  low: the low bank, a uint8 [B,n,Hs,Ws,3] device tensor from an earlier `blur_u8(images, band_sigma,
    idx)`, or None: made here with one launch.  ValueError before any launch for arguments outside these (a low bank with another mode
    among them); nothing is copied to the host."""
    data = _images(images, "images")
    _need_device(G, name=False)
    if G.device != data.device:
        raise ValueError("panorama: images is on %s, G on %s" % (data.device, G.device))
    if G.dtype != torch.float64 or G.dim() != 4 or tuple(G.shape[2:]) != (3, 3) or not 1 <= G.shape[1] <= PANO_MAX_FRAMES:
        raise ValueError("panorama: G [B,n,3,3] float64 with 1 <= n <= %d, got %s %s" % (PANO_MAX_FRAMES, G.dtype, tuple(G.shape)))
    B, n = G.shape[:2]
    size = _canvas_args("panorama", canvas, feather, mode, limit, "panorama")
    _band_args(mode, band_sigma, "panorama", "panorama")
    low = _low_arg(low, mode, (B, n) + tuple(data.shape[1:]), data.device, "panorama")
    ix = _frames_index(idx, data.shape[0], data.device, "panorama")
    if tuple(ix.shape) != (B, n):
        raise ValueError("panorama: idx names %d samples of %d frames, G has %d of %d" % (ix.shape[0], ix.shape[1], B, n))
    gain = _pano_tensor(gain, (B, n, 2), torch.float64, "gain", "panorama")
    use = _pano_tensor(use, (B, n), torch.uint8, "use", "panorama")
    with torch.cuda.device(data.device):
        return _panorama(data, ix, G.contiguous(), size, feather, mode, gain, use, limit, band_sigma, low)


def _stage_args(refine, cascade, cascade_min_cover, cascade_samples):
    """The rules of Aligner's refine / cascade arguments that need no image, checked before any launch -> (stages, (nx, ny) or None)."""
    if refine not in (None, "ecc"):
        raise ValueError("Aligner: refine is None or 'ecc', got %r" % (refine,))
    try:
        stages = operator.index(cascade)
    except TypeError:
        stages = -1
    if stages < 0:
        raise ValueError("Aligner: cascade is the number of re-prediction stages, an integer >= 0, got %r" % (cascade,))
    if not 0.0 <= cascade_min_cover <= 1.0:                                # (False for a NaN too)
        raise ValueError("Aligner: cascade_min_cover is a share in [0, 1], got %r" % (cascade_min_cover,))
    return stages, None if cascade_samples is None else _cascade_samples(cascade_samples, None, 0, 0, 1)


class Aligner:
    """Aligner(model, patch=None, channels=None, mean=0.443, std=0.129): `model` is the Sequential(backbone, head) of step.build_model
    on the device.  patch / channels default to the model's PATCH_SIZE / PATCH_CHANNELS (channels to 1, upstream's grayscale pair,
    where the model does not say); mean / std are DictStandardize's (transforms.py:369-378).

    aligner(images_a, images_b, idx_a=None, idx_b=None, roi_a=None, roi_b=None, warp=True, refine=None, refine_levels=3,
            refine_iters=10, mask_b=None, cascade=0, cascade_samples=None, cascade_min_cover=0.25, mosaic=None, mosaic_feather=32.0,
            mosaic_mode="feather", mosaic_exposure=None, mosaic_limit=2.0, mosaic_band_sigma=4.0, init=None) -> dict
        images_*: uint8 [N,H,W,3] device tensors or ImageBanks; the two may differ in size.
        idx_*: which image each of the B samples uses (host list: range-checked; int32 device tensor: clamped by the kernel;
               None: sample b is image b, so B = N).
        roi_*: the region of each image the model looks at, host values (x0, y0, rw, rh) in edge coordinates, one for all samples or
               [B,4]; None: the whole image.
        'delta_hat' [B,4,2]            the model's prediction, in patch pixels
        'H' [B,3,3] float64            index coordinates of image B -> index coordinates of image A, H[2,2] = 1
        'patch_1', 'patch_2'           what the model saw: [B,C,P,P] float32 of image A and of image B
        'geom_a', 'geom_b' [B,4]       the geometry records (sx, sy, tx, ty) of the two preparations
        'aligned' [B,Hb,Wb,3] uint8    image A resampled onto image B's grid; 'valid' [B,Hb,Wb] uint8 (both absent with warp=False)
    refine="ecc" (default None: nothing below happens, the result is key for key the one above): between the lift and the warp the
        homography is polished on the two images themselves by `ecc_refine` - refine_levels pyramid levels, refine_iters steps per level,
        mask_b uint8 [B,Hb,Wb] on the device (non-zero: the pixel of B may count; moving objects, overlays) - and then
        'H' is the refined matrix, 'H_model' the lifted one, 'rho' [B,2] the correlation coefficient at full size before and after,
        'refine_stats' [B,levels,3] the whole table; 'aligned' / 'valid' come from the refined 'H'.  Levels too deep for the images
        raise a ValueError that names the sizes, before any launch.
    cascade=K (default 0: nothing below happens, no further launch, the result is key for key and bit for bit the one above),
        cascade_samples=None, cascade_min_cover=0.25: after the lift the model predicts K more times, each time on A seen through the best
        H so far (`prepare_warped`, nx x ny bilinear samples per patch pixel: cascade_samples=(nx, ny), or min(8, max(1, ceil(s))) per
        axis with s the largest rw_b / P, rh_b / P of the batch) against patch_2, and the candidate `cascade_compose_device` makes of it
        replaces the best where its score - the correlation of the two patches over the fully covered pixels, `patch_ncc` - is higher
        and counts at least cascade_min_cover C P P elements.  Every sample runs every stage; the choice is torch.where on the device.
        'H' is then the best candidate, 'H_stages' [B,K+1,3,3] all of them (index 0 the lift), 'delta_stages' [B,K+1,4,2] the prediction
        of each stage, 'score' [B,K+1] float64 their correlations, 'accepted' [B,K+1] uint8 (index 0 always 1), 'patch_1_warped' A
        through 'H' as the model last saw it; 'delta_hat', 'patch_1', 'geom_*' stay stage 0's.  With refine="ecc" the refinement starts
        from the cascade's 'H', and 'H_model' is that matrix.  A cascade that is no integer >= 0, samples outside 1..8 and a
        cascade_min_cover outside [0, 1] raise a ValueError before any launch.
    init=None (nothing below happens, the result is key for key and bit for bit the one above) or a [B,3,3] float64 device tensor, B's
        index coordinates -> A's: the cascade (cascade >= 1 is required) starts from init instead of from the lift, and the model is not
        run on the unwarped patches - for two images too far apart for the model (it is trained on displacements up to P / 4), whose
        homography is known roughly from elsewhere, as a sequence's link between distant frames is from its chain.  Stage 0 of
        'H_stages', 'score' and 'accepted' is init itself, 'delta_stages'[:, 0] and 'delta_hat' are zero, 'patch_1' is A seen through
        init, and 'geom_a' is absent: A is not prepared on its own, so roi_a is refused.
    mosaic="b" or (Hc, Wc) (default None: nothing below happens, no further launch, the result is key for key and bit for bit the one
        above), mosaic_feather=32.0, mosaic_mode="feather", mosaic_exposure=None, mosaic_limit=2.0: from the final 'H' - after the cascade
        and the refinement - both images are put on one canvas by `mosaic` (bh_mosaic_u8, one pass): "b" is image B's grid, (Hc, Wc) the
        frame fitted around B and A's projected corners (`mosaic_frame_device`, at most mosaic_limit image sizes around B).
        mosaic_mode "feather" blends by the distance to each image's border capped at mosaic_feather pixels, "b_over_a" / "a_over_b" put
        one image on top; mosaic_exposure "gain" matches A's gray to B's by a least-squares gain and bias first (`exposure_device`;
        mask_b, where refine="ecc" was given one, restricts the pixels it counts), a [B,2] float64 device tensor gives (g, o).  Added:
        'mosaic' [B,Hc,Wc,3] uint8, 'mosaic_cover' [B,Hc,Wc] uint8 (0 empty, 1 only A, 2 only B, 3 both), 'mosaic_T' [B,3,3] float64
        (canvas index coordinates -> B's), 'mosaic_bbox' [B,4] float64, 'mosaic_fitted' [B] uint8, 'mosaic_gain' [B,2] float64.  A
        mosaic that is neither of the two, a canvas side below 2, a feather that is NaN, infinite or below 1, an unknown mode or
        exposure, 'gain' on an image side below 8 and a limit that is not > 0 raise a ValueError before any launch.
        mosaic_mode "two_band" with mosaic_band_sigma=4.0 (in [0.5, 10.5], in each image's own pixels; a default, not a tuned value) is
        `mosaic`'s two-band blend - the low bands blended with the feather, the high band from the image with the larger weight - and
        adds 'mosaic_winner' [B,Hc,Wc] uint8 (0: A, 1: B, 255: neither); the other modes do not look at mosaic_band_sigma.
    aligner.sequence(images, idx=None, ref=None, ..., canvas=None) registers n frames of one bank to a reference frame through this
        call and blends them on one canvas (`chain_device`, `pano_frame_device`, `pano_u8`): see its docstring.
    The aligner copies nothing from the device to the host (host-given idx / roi values are uploaded).  What a model's own
    predict_homography does is the model's: NoOpHead '4_points' and PhotometricHead read the patch extent off 'corners' with .item()."""

    def __init__(self, model, patch=None, channels=None, mean=0.443, std=0.129):
        self.model = model
        self.patch = int(patch) if patch is not None else _model_attr(model, "patch_size")
        if self.patch is None:
            raise ValueError("Aligner: the model does not carry a PATCH_SIZE; pass patch=")
        c = int(channels) if channels is not None else _model_attr(model, "patch_channels")
        self.channels = 1 if c is None else c
        if self.channels not in (1, 3):
            raise ValueError("Aligner: channels is 1 (grayscale) or 3 (RGB), got %r" % (self.channels,))
        if self.patch < 16 or self.patch % 16 or self.patch > 256:
            raise ValueError("Aligner: patch is a multiple of 16 up to 256, got %r" % (self.patch,))
        if not std > 0:
            raise ValueError("Aligner: std must be positive, got %r" % (std,))
        self.mean, self.std = float(mean), float(std)
        backbone = next(iter(model.children()), None)
        keys = getattr(backbone, "patch_keys", None) or ("patch_1", "patch_2")
        self.patch_keys = (keys[0], keys[1])
        self._square = None

    def _corners(self, B, device):
        """[B,4,2] float32 on the device: (0,0), (P,0), (P,P), (0,P) per sample, filled there (no upload) and kept between calls."""
        c = self._square
        if c is None or c.shape[0] != B or c.device != device:
            c = torch.zeros((B, 4, 2), dtype=torch.float32, device=device)
            c[:, 1:3, 0] = float(self.patch)
            c[:, 2:4, 1] = float(self.patch)
            self._square = c
        return c

    def _cascade(self, predict, a, ia, p2, gb, H0, delta0, stages, nx, ny, min_cover):
        """The stages after the lift, all on the device: every sample runs every stage, a candidate replaces the best so far where its
        score is higher on enough elements (torch.where; False for a NaN or -inf score).  -> (the keys the cascade adds or replaces, A
        through H0 as the model's patch)."""
        B, P, dev = H0.shape[0], self.patch, H0.device
        G = _grid_map_device(gb, nx, ny)
        need = float(min_cover) * self.channels * P * P

        def seen(Hc):                                                          # A through Hc as the model's patch, and its score
            W, cov = prepare_warped(a, (Hc @ G).contiguous(), B, P, self.channels, nx, ny, self.mean, self.std, idx=ia)
            return W, patch_ncc(W, p2, cov)
        H_best = H0
        W_best, o = seen(H_best)
        W0 = W_best                                                            # (A through H0: `init=`'s patch_1)
        s_best = o[:, 6]
        Hs, deltas, scores, accepted = [H0], [delta0], [s_best], [torch.ones(B, dtype=torch.uint8, device=dev)]
        for _ in range(stages):
            d = predict(self.model, {self.patch_keys[0]: W_best, self.patch_keys[1]: p2, "corners": self._corners(B, dev)})
            d = d.detach().reshape(B, 4, 2)
            H_c = cascade_compose_device(H_best, d, P, gb)
            W_c, o = seen(H_c)
            take = (o[:, 6] > s_best) & (o[:, 0] >= need)
            H_best = torch.where(take[:, None, None], H_c, H_best)
            W_best = torch.where(take[:, None, None, None], W_c, W_best)
            s_best = torch.where(take, o[:, 6], s_best)
            Hs.append(H_c); deltas.append(d); scores.append(o[:, 6]); accepted.append(take.to(torch.uint8))
        return {"H": H_best, "H_stages": torch.stack(Hs, 1), "delta_stages": torch.stack(deltas, 1), "score": torch.stack(scores, 1),
                "accepted": torch.stack(accepted, 1), "patch_1_warped": W_best}, W0

    def __call__(self, images_a, images_b, idx_a=None, idx_b=None, roi_a=None, roi_b=None, warp=True, refine=None, refine_levels=3,
                 refine_iters=10, mask_b=None, cascade=0, cascade_samples=None, cascade_min_cover=0.25, mosaic=None, mosaic_feather=32.0,
                 mosaic_mode="feather", mosaic_exposure=None, mosaic_limit=2.0, mosaic_band_sigma=4.0, init=None):
        from .step import predict
        stages, samples = _stage_args(refine, cascade, cascade_min_cover, cascade_samples)
        if init is not None:
            if stages < 1:
                raise ValueError("Aligner: init is where the cascade starts; pass cascade >= 1 with it")
            if roi_a is not None:
                raise ValueError("Aligner: with init image A is only seen through the homography; roi_a does not apply")
        a, b = _images(images_a, "images_a"), _images(images_b, "images_b")
        if a.device != b.device:
            raise ValueError("Aligner: images_a is on %s, images_b on %s" % (a.device, b.device))
        ia, na = _index(idx_a, a.shape[0], a.device, "idx_a")
        ib, nb = _index(idx_b, b.shape[0], b.device, "idx_b")
        na, nb = a.shape[0] if na is None else na, b.shape[0] if nb is None else nb
        if na != nb:
            raise ValueError("Aligner: %d samples of images_a, %d of images_b" % (na, nb))
        B, P = na, self.patch
        ra = _regions(roi_a, B, a.shape[1], a.shape[2], a.device, "roi_a")
        rb = _regions(roi_b, B, b.shape[1], b.shape[2], b.device, "roi_b")
        if refine is not None:
            _refine_args(refine_levels, refine_iters, (("Aligner: refine_levels, images_a", a.shape[1:3]), ("Aligner: refine_levels, images_b", b.shape[1:3])),
                         "Aligner: refine_iters")
            mask_b = _check_mask(mask_b, B, b.shape[1], b.shape[2], b.device)
        elif mask_b is not None:
            raise ValueError("Aligner: mask_b restricts the pixels the refinement counts; pass refine='ecc' with it")
        nx, ny = samples or _cascade_samples(None, roi_b, b.shape[1], b.shape[2], P)
        if mosaic is not None:
            canvas = _canvas_args("mosaic", mosaic, mosaic_feather, mosaic_mode, mosaic_limit, "Aligner")
            _band_args(mosaic_mode, mosaic_band_sigma, "mosaic", "Aligner", "mosaic_band_sigma")
            _mosaic_exposure_args(mosaic_exposure, B, a.shape[1:3], b.shape[1:3], "Aligner", "mosaic_exposure")
        if init is not None and not (isinstance(init, torch.Tensor) and init.is_cuda and init.device == a.device and init.dtype == torch.float64
                                     and tuple(init.shape) == (B, 3, 3)):
            got = "%s %s on %s" % (init.dtype, tuple(init.shape), init.device) if isinstance(init, torch.Tensor) else repr(init)
            raise ValueError("Aligner: init is a [B,3,3] = [%d,3,3] float64 tensor on the images' device (B's index coordinates -> A's), got %s" % (B, got))
        with torch.cuda.device(a.device):
            if init is None:
                p1, ga = prepare(a, B, P, self.channels, self.mean, self.std, idx=ia, roi=ra)
            p2, gb = prepare(b, B, P, self.channels, self.mean, self.std, idx=ib, roi=rb)
            if init is None:
                # the patch square, for the heads that ask for it (NoOpHead '4_points', PhotometricHead.predict_homography)
                delta_hat = predict(self.model, {self.patch_keys[0]: p1, self.patch_keys[1]: p2, "corners": self._corners(B, a.device)})
                delta_hat = delta_hat.detach().reshape(B, 4, 2)
                H = lift_device(delta_hat, P, ga, gb)
                out = {"delta_hat": delta_hat, "H": H, "patch_1": p1, "patch_2": p2, "geom_a": ga, "geom_b": gb}
            else:                                                              # the cascade starts from init: no prediction on the unwarped patches
                delta_hat = torch.zeros((B, 4, 2), dtype=torch.float32, device=a.device)
                H = init.contiguous()
                out = {"delta_hat": delta_hat, "H": H, "patch_2": p2, "geom_b": gb}
            if stages:
                added, seen_0 = self._cascade(predict, a, ia, p2, gb, H, delta_hat, stages, nx, ny, cascade_min_cover)
                out.update(added)
                if init is not None:
                    out["patch_1"] = seen_0
                H = out["H"]
            if refine is not None:
                H, stats = ecc_refine(a, b, H, refine_levels, refine_iters, idx_a=ia, idx_b=ib, mask=mask_b)
                out.update({"H_model": out["H"], "H": H, "refine_stats": stats, "rho": stats[:, 0, :2]})
            if warp:
                out["aligned"], out["valid"] = warp_u8(a, H, b.shape[1], b.shape[2], idx=ia)
            if mosaic is not None:
                out.update(_mosaic(a, b, H, canvas, mosaic_feather, mosaic_mode, mosaic_exposure, mosaic_limit, ia, ib, mask_b, mosaic_band_sigma))
        return out

    def sequence(self, images, idx=None, ref=None, roi=None, refine=None, refine_levels=3, refine_iters=10, mask=None, cascade=0,
                 cascade_samples=None, cascade_min_cover=0.25, canvas=None, feather=32.0, mode="feather", exposure=None, limit=2.0, use=None,
                 band_sigma=4.0, links=None, link_min_score=0.5, adjust_iters=10, adjust_grid=4):
        """Register a sequence of n frames (1 <= n <= 255) to one of them and, with a canvas, blend them all on it.
            images: one uint8 [N,Hs,Ws,3] device tensor or ImageBank; every frame has this size.
            idx: [B,n], frame k of sample b (host values: range-checked; int32 device tensor: clamped by the kernels; None: one sample
                 of all N images in order).  ref: the reference frame, default n // 2.
            roi: the region the model looks at, host values (x0, y0, rw, rh) for every frame or [B,4] per sample; None: whole frames.
        The B (n - 1) neighbouring pairs `pairs_of(n, ref)` - (a, b) with b the frame nearer to the reference - go through the aligner
        ONCE (`self(images, images, idx_a=, idx_b=, warp=False, ...)`, sample b (n - 1) + j is pair j of sample b; refine, refine_levels,
        refine_iters, cascade, cascade_samples and cascade_min_cover are that call's and apply per pair; mask uint8 [B,n,Hs,Ws] on the
        device gives the pixels of each frame that may count where the frame is a pair's b), and `chain_device` composes them outwards
        from the reference.  -> dict: 'G' [B,n,3,3] float64 (the reference's index coordinates -> frame k's, G[ref] = I), 'H_pairs'
        [B,n-1,3,3] float64, 'pairs' (the host list of (a, b)), 'pair' (the pair call's dict; empty for n = 1, which runs no model).
        canvas="ref" or (Hc, Wc) (default None: no further launch) adds `panorama`'s keys with feather, mode, limit and use [B,n] uint8 on
        the device (0: the frame is left out of the blend and of the frame fit); exposure=None, "gain" (each pair's least-squares line of
        b's gray on a's through its H - one-level `gray_pyramid`, `ecc_sums`, `exposure_device`, counting the pixels `mask` allows -
        composed along the chain) or a [B,n,2] float64 device tensor (g, o) per frame.  mode="two_band" with band_sigma=4.0 is
        `panorama`'s two-band blend (the low bank is made here, one launch) and adds 'panorama_winner'.
        links=None, link_min_score=0.5, adjust_iters=10, adjust_grid=4: the chain accumulates every pair's error and drifts with n, so a
        pan that comes back, an out-and-back sweep or a raster scan does not close.  links is a HOST list of further frame pairs (a, b)
        that overlap (None or empty: nothing below happens, no further launch, the result is key for key and bit for bit the one above;
        2 <= n <= 64 with links).  After the chain each link is predicted THROUGH the chain's own estimate - all B L links go through the
        aligner in ONE call with init = G_a G_b^-1 (the 3 x 3 inverse written out as an adjugate), cascade=max(1, cascade), the same
        refine arguments and warp=False - and a link COUNTS (weight 1) iff the correlation of A seen through its final H against
        patch_2 (`prepare_warped` + `patch_ncc`) is at least link_min_score on at least cascade_min_cover C P P elements, decided on the
        device by torch.where: two frames that do not overlap fail the cover test and simply drop out.  0.5 is a default, not a tuned
        value.  Then `adjust_device` solves all frames jointly (`adjust_host`: adjust_iters Levenberg-Marquardt steps on an adjust_grid x
        adjust_grid lattice of control points) from the edges - the chain's pairs with weight 1 followed by the links.  'G' is then the
        adjusted one and the canvas and panorama keys follow from it; added: 'G_chain' (the chain's G), 'links' (the host list),
        'link' (the link call's dict), 'H_links' [B,L,3,3] float64, 'link_score' [B,L] float64, 'link_weight' [B,L] float64,
        'adjust_stats' [B,4] float64 (cost at the start, cost at the result, accepted steps, final lambda).  The exposure lines stay the
        chain's: adjusting the gains over the links is out of scope.  Refused: links with n > 64, a link that is not two distinct
        frames of the sequence or that repeats a pair of the chain, a link_min_score outside [-1, 1], adjust_iters < 0, a grid outside 2..8.
        Arguments outside these rules raise a ValueError before any launch; nothing is copied to the host."""
        who = "Aligner.sequence"
        stages, _ = _stage_args(refine, cascade, cascade_min_cover, cascade_samples)
        data = _images(images, "images")
        dev, (Hs, Ws) = data.device, data.shape[1:3]
        ix = _frames_index(idx, data.shape[0], dev, who)
        B, n = ix.shape
        if ref is None:
            ref = n // 2
        try:
            ref = operator.index(ref)
        except TypeError:
            ref = -1
        if not 0 <= ref < n:
            raise ValueError("%s: ref is a frame of the sequence, an integer in [0, %d), got %r" % (who, n, ref))
        pairs = pairs_of(n, ref)
        try:
            links = [] if links is None else list(links)
        except TypeError:
            raise ValueError("%s: links is a host list of (a, b) frame pairs, got %r" % (who, links)) from None
        if links:
            links = _adjust_args(links, n, ref, adjust_grid, adjust_iters, who, pairs=pairs)
            try:
                score_ok = bool(-1.0 <= float(link_min_score) <= 1.0)          # (False for a NaN too)
            except (TypeError, ValueError):
                score_ok = False
            if not score_ok:
                raise ValueError("%s: link_min_score is a correlation in [-1, 1], got %r" % (who, link_min_score))
        roi_links = roi
        if roi is not None:
            if not (isinstance(roi, torch.Tensor) and roi.is_cuda):           # (a device tensor is `_regions`' to refuse)
                roi = np.asarray(roi.numpy() if isinstance(roi, torch.Tensor) else roi, np.float64)
                if roi.shape not in ((4,), (B, 4)):
                    raise ValueError("%s: roi is (x0, y0, rw, rh) or [B,4] of them with B = %d, got shape %s" % (who, B, roi.shape))
                roi_links = np.repeat(roi, len(links), axis=0) if roi.ndim == 2 else roi
                if roi.ndim == 2:
                    roi = np.repeat(roi, n - 1, axis=0)                        # one region per sample -> one per pair
            _regions(roi, B * (n - 1), Hs, Ws, torch.device("cpu"), "roi")
        if refine is not None:
            _refine_args(refine_levels, refine_iters, (("%s: refine_levels" % who, (Hs, Ws)),), "%s: refine_iters" % who)
        if canvas is None:
            if exposure is not None or use is not None:
                raise ValueError("%s: exposure and use belong to the panorama; pass canvas='ref' or (Hc, Wc) with them" % who)
            size = None
        else:
            size = _canvas_args("panorama", canvas, feather, mode, limit, who)
            _band_args(mode, band_sigma, "panorama", who)
        measure = isinstance(exposure, str) and exposure == "gain"
        if measure:
            if min(Hs, Ws) < ECC_MIN_SIDE:
                raise ValueError("%s: the panorama exposure 'gain' measures on the gray frames, which need at least %d pixels on each side; "
                                 "the frames are %d x %d (H x W)" % (who, ECC_MIN_SIDE, Hs, Ws))
        elif isinstance(exposure, torch.Tensor):
            exposure = _pano_tensor(exposure, (B, n, 2), torch.float64, "exposure", who)
        elif exposure is not None:
            raise ValueError("%s: the panorama exposure is None, 'gain' or a [B,n,2] float64 device tensor (g, o), got %r" % (who, exposure))
        use = _pano_tensor(use, (B, n), torch.uint8, "use", who)
        if mask is not None:
            if refine is None and not measure:
                raise ValueError("%s: mask restricts the pixels the refinement and the exposure measurement count; pass refine='ecc' or "
                                 "exposure='gain' with it" % who)
            mask = _pano_tensor(mask, (B, n, Hs, Ws), torch.uint8, "mask", who)
        with torch.cuda.device(dev):
            out = {"pairs": pairs, "pair": {}}
            gain_pairs = None
            if n > 1:
                ia = ix[:, [a for a, _ in pairs]].reshape(-1).contiguous()
                ib = ix[:, [b for _, b in pairs]].reshape(-1).contiguous()
                mask_b = None if mask is None else mask[:, [b for _, b in pairs]].reshape(B * (n - 1), Hs, Ws).contiguous()
                r = self(data, data, idx_a=ia, idx_b=ib, roi_a=roi, roi_b=roi, warp=False, refine=refine, refine_levels=refine_levels,
                         refine_iters=refine_iters, mask_b=mask_b if refine is not None else None, cascade=cascade,
                         cascade_samples=cascade_samples, cascade_min_cover=cascade_min_cover)
                out["pair"] = r
                H_pairs = r["H"].reshape(B, n - 1, 3, 3).contiguous()
                if measure:
                    gain_pairs = measure_exposure(data, data, r["H"], ia, ib, mask_b).reshape(B, n - 1, 2).contiguous()
            else:
                H_pairs = torch.empty((B, 0, 3, 3), dtype=torch.float64, device=dev)
                if measure:
                    gain_pairs = torch.empty((B, 0, 2), dtype=torch.float64, device=dev)
            G, gain = chain_device(H_pairs, ref, gain_pairs)
            out.update({"G": G, "H_pairs": H_pairs})
            if links:
                L, la, lb = len(links), [a for a, _ in links], [b for _, b in links]
                init = (G[:, la] @ _inverse_device(G[:, lb])).reshape(B * L, 3, 3)          # b's index coordinates -> a's, through the chain
                init = (init / init[:, 2:3, 2:3]).contiguous()
                ia, ib = ix[:, la].reshape(-1).contiguous(), ix[:, lb].reshape(-1).contiguous()
                mask_b = None if mask is None or refine is None else mask[:, lb].reshape(B * L, Hs, Ws).contiguous()
                r = self(data, data, idx_a=ia, idx_b=ib, roi_b=roi_links, warp=False, refine=refine, refine_levels=refine_levels,
                         refine_iters=refine_iters, mask_b=mask_b, cascade=max(1, stages), cascade_samples=cascade_samples,
                         cascade_min_cover=cascade_min_cover, init=init)
                H_links = r["H"].reshape(B, L, 3, 3).contiguous()
                # the link's score: A through its final H against patch_2, on the grid the cascade samples
                nx, ny = _cascade_samples(cascade_samples, roi_links, Hs, Ws, self.patch)
                seen, cover = prepare_warped(data, (r["H"] @ _grid_map_device(r["geom_b"], nx, ny)).contiguous(), B * L, self.patch, self.channels, nx, ny,
                                             self.mean, self.std, idx=ia)
                o = patch_ncc(seen, r["patch_2"], cover)
                counts = (o[:, 6] >= float(link_min_score)) & (o[:, 0] >= float(cascade_min_cover) * self.channels * self.patch * self.patch)
                link_weight = torch.where(counts, torch.ones_like(o[:, 6]), torch.zeros_like(o[:, 6])).reshape(B, L)
                edges = torch.tensor(pairs + links, dtype=torch.int32).to(dev)
                weight = torch.cat([torch.ones((B, n - 1), dtype=torch.float64, device=dev), link_weight], 1).contiguous()
                G_adj, stats = adjust_device(G, edges, torch.cat([H_pairs, H_links], 1).contiguous(), weight, ref, (Hs, Ws), adjust_grid, adjust_iters)
                out.update({"G_chain": G, "G": G_adj, "links": links, "link": r, "H_links": H_links, "link_score": o[:, 6].reshape(B, L).contiguous(),
                            "link_weight": link_weight, "adjust_stats": stats})
                G = G_adj
            if canvas is not None:
                out.update(_panorama(data, ix, G, size, feather, mode, exposure if isinstance(exposure, torch.Tensor) else gain, use, limit, band_sigma))
        return out
