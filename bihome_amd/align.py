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
cv2.warpPerspective rounds half to even in fixed point with 1/32-pixel coordinates; this rounds half up in float."""
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


def lift(delta_hat, P, geom_a, geom_b):
    """delta_hat [B,4,2] (patch pixels), the geometry records of both preparations -> H [B,3,3] float64 with H[2,2] = 1: index
    coordinates of image B -> index coordinates of image A (the Lift of the module docstring)."""
    d = np.asarray(delta_hat, np.float64).reshape(-1, 4, 2)
    Aa, Ab = _affine(geom_a), _affine(geom_b)
    c = patch_corners(P)
    H = np.empty((d.shape[0], 3, 3))
    for b in range(d.shape[0]):
        Hb = Aa[b] @ synth.four_point_homography(c, c + d[b]) @ np.linalg.inv(Ab[b])
        H[b] = Hb / Hb[2, 2]
    return H


def warp_u8_host(images, H, Ho, Wo):
    """images uint8 [B,Hs,Ws,3], H [B,3,3] (output index coordinates -> source index coordinates) -> (out uint8 [B,Ho,Wo,3],
    valid uint8 [B,Ho,Wo]): the uint8 warp of the module docstring."""
    images = np.asarray(images)
    H = np.asarray(H, np.float64).reshape(-1, 3, 3)
    B, Hs, Ws = images.shape[:3]
    out, valid = np.empty((B, Ho, Wo, 3), np.uint8), np.empty((B, Ho, Wo), np.uint8)
    ys, xs = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    for b in range(B):
        h, img = H[b], images[b].astype(np.float64)
        qz = h[2, 0] * xs + h[2, 1] * ys + h[2, 2]
        guard = ~(np.abs(qz) > QZ_GUARD)
        iz = 1.0 / np.where(guard, 1.0, qz)
        u, v = (h[0, 0] * xs + h[0, 1] * ys + h[0, 2]) * iz, (h[1, 0] * xs + h[1, 1] * ys + h[1, 2]) * iz
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
        out[b] = np.floor(np.clip(acc, 0.0, 255.0) + 0.5).astype(np.uint8)
    return out, valid


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


def lift_device(delta_hat, P, geom_a, geom_b):
    """`lift` on the device: delta_hat [B,4,2] float32, geom_* [B,4] float64 -> H [B,3,3] float64.  The 8 x 8 solve is bh_h4pt_fwd's
    (double), the conjugation batched [B,3,3] double arithmetic; nothing is copied to the host."""
    B = delta_hat.shape[0]
    Hp = K.h4pt_fwd(delta_hat.reshape(B, 4, 2).to(torch.float32).contiguous(), P)[0].view(B, 3, 3)
    H = _affine_dev(geom_a) @ Hp @ _affine_dev(geom_b, inverse=True)
    return (H / H[:, 2:3, 2:3]).contiguous()


def prepare(images, B, patch, channels, mean=0.443, std=0.129, idx=None, roi=None):
    """bh_align_prep_u8 on outputs allocated here: (patch [B,C,P,P] float32, geom [B,4] float64) of B samples of the uint8 bank
    images [N,H,W,3]; idx [B] int32 and roi [B,4] float64 are DEVICE tensors or None (kernels.align_prep_u8)."""
    if not images.is_cuda:
        raise RuntimeError("bihome_amd kernels need device tensors (got %s); there is no CPU path" % images.device)
    out = torch.empty((B, channels, patch, patch), dtype=torch.float32, device=images.device)
    geom = torch.empty((B, 4), dtype=torch.float64, device=images.device)
    return K.align_prep_u8(images, out, geom, mean, std, idx=idx, roi=roi)


def warp_u8(images, H64, Ho, Wo, idx=None, want_valid=True):
    """bh_warp_u8 on outputs allocated here: (out [B,Ho,Wo,3] uint8, valid [B,Ho,Wo] uint8 or None) (kernels.warp_u8)."""
    if not images.is_cuda:
        raise RuntimeError("bihome_amd kernels need device tensors (got %s); there is no CPU path" % images.device)
    B = H64.shape[0]
    out = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=images.device)
    valid = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=images.device) if want_valid else None
    return K.warp_u8(images, H64, out, valid, idx=idx)


class Aligner:
    """Aligner(model, patch=None, channels=None, mean=0.443, std=0.129): `model` is the Sequential(backbone, head) of step.build_model
    on the device.  patch / channels default to the model's PATCH_SIZE / PATCH_CHANNELS (channels to 1, upstream's grayscale pair,
    where the model does not say); mean / std are DictStandardize's (transforms.py:369-378).

    aligner(images_a, images_b, idx_a=None, idx_b=None, roi_a=None, roi_b=None, warp=True) -> dict
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

    def __call__(self, images_a, images_b, idx_a=None, idx_b=None, roi_a=None, roi_b=None, warp=True):
        from .step import predict
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
        with torch.cuda.device(a.device):
            p1, ga = prepare(a, B, P, self.channels, self.mean, self.std, idx=ia, roi=ra)
            p2, gb = prepare(b, B, P, self.channels, self.mean, self.std, idx=ib, roi=rb)
            # the patch square, for the heads that ask for it (NoOpHead '4_points', PhotometricHead.predict_homography)
            delta_hat = predict(self.model, {self.patch_keys[0]: p1, self.patch_keys[1]: p2, "corners": self._corners(B, a.device)})
            delta_hat = delta_hat.detach().reshape(B, 4, 2)
            H = lift_device(delta_hat, P, ga, gb)
            out = {"delta_hat": delta_hat, "H": H, "patch_1": p1, "patch_2": p2, "geom_a": ga, "geom_b": gb}
            if warp:
                out["aligned"], out["valid"] = warp_u8(a, H, b.shape[1], b.shape[2], idx=ia)
        return out
