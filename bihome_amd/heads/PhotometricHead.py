"""Drop-in for `src/heads/PhotometricHead.py` (Nguyen et al.'s unsupervised photometric baseline:
config/s-coco/nguyen-orig-lr-5e-3.yaml).  LEARNING_KEYS = (patch_2, image_1, delta, delta_hat_12).

`forward` (PhotometricHead.py:17-47) returns (patch_2, patch_hat, delta, delta_hat) for the torch loss of train.py:318-322
(L1Loss).  Upstream builds H_hat = four_point_to_homography(corners, delta_hat, crop=False) in full-image coordinates, warps the
whole image_1 with it (warp_image: kornia.warp_perspective, bilinear, zeros, align_corners=True) and crops every sample at its
corners.  Here only the crop window is sampled: with Hp the 4-point homography of the patch corners [[0,0],[P,0],[P,P],[0,P]]
and o the integer top-left corner, H_hat.(o + u) = o + Hp.u, so patch_hat = bh_photo_warp_fwd(image_1, Hp, o) after the
existing 4-point solve (bh_h4pt_fwd); the backward runs the adjoint w.r.t. Hp (bh_photo_warp_bwd) and then bh_h4pt_bwd.
image_1 is data and gets no gradient.

The corners must be integer-valued axis-aligned squares of one size across the batch (what HomographyNetPrep produces,
transforms.py:505-521; upstream's torch.stack of the crops needs one size anyway); anything else raises ValueError.

`predict_homography` (:49-61) returns (delta_hat, H_hat) with H_hat in full-image coordinates (NoOpHead's corner conjugation).
"""
import weakref

import torch
import torch.nn as nn

from .. import kernels as K
from .NoOpHead import Model as _NoOpHead


@K.scoped_function
class _PatchHat(torch.autograd.Function):
    """delta_hat [B,4,2] (or [B,8]) -> patch_hat [B,C,P,P] = crop at `origin` of warp_image(image, H_hat)."""

    @staticmethod
    def forward(ctx, delta_hat, image, origin, P):
        B = image.shape[0]
        delta = delta_hat.detach().reshape(B, 4, 2).to(torch.float32).contiguous()
        img = image.detach().to(torch.float32).contiguous()
        Hp64, _ = K.h4pt_fwd(delta, P)                                      # :29-30 in patch coordinates
        out = K.photo_warp_fwd(img, Hp64, origin, P)                        # :33-42 (warp + crop, crop window only)
        ctx.saved = (delta, Hp64, img, origin)
        ctx.P, ctx.shape = P, delta_hat.shape
        return out

    @staticmethod
    def backward(ctx, g_out):
        delta, Hp64, img, origin = ctx.saved
        ctx.saved = None
        gH = K.photo_warp_bwd(img, Hp64, origin, g_out.to(torch.float32).contiguous(), ctx.P)
        g_delta = K.h4pt_bwd(delta, Hp64, gH, ctx.P)
        return g_delta.reshape(ctx.shape), None, None, None


@K.scoped_module
class Model(nn.Module):

    def __init__(self, backbone, **kwargs):
        super().__init__()
        self.learning_keys = kwargs['LEARNING_KEYS']             # ground_truth, original_non_patched_image, delta_gt, delta_hat

    _checked = None               # (weak reference to the last device corners tensor validated, its version, P)

    @classmethod
    def _window(cls, corners, patch_size, device):
        """(P, origin [B,2] float32 on `device`) of integer axis-aligned square corners of one size.  Validating device corners reads
        them back (a stream synchronisation): done once per tensor (the same tensor object at the same version is not read again), and not
        inside a HIP-graph capture, where nothing can be read back - P is then the ground-truth patch's size (the eager warm-up steps
        validated the corners)."""
        c = corners.reshape(-1, 4, 2)
        seen = cls._checked
        if c.is_cuda and torch.cuda.is_current_stream_capturing():
            P = int(patch_size)
        elif c.is_cuda and seen is not None and seen[0]() is corners and seen[1] == corners._version:
            P = seen[2]
        else:
            h = c.detach().to("cpu", torch.float64)
            x0, y0 = h[:, 0, 0], h[:, 0, 1]
            size = h[:, 1, 0] - x0
            square = torch.stack([x0, y0, x0 + size, y0, x0 + size, y0 + size, x0, y0 + size], 1).reshape(-1, 4, 2)
            if (h.shape[0] == 0 or not torch.equal(h, h.round()) or not torch.equal(h, square) or not bool((size > 0).all())
                    or not bool((size == size[0]).all())):
                raise ValueError("PhotometricHead: corners must be integer-valued axis-aligned squares of one size across the batch "
                                 "(HomographyNetPrep, transforms.py:505-521)")
            P = int(size[0].item())
            if P % 16:
                raise ValueError("PhotometricHead: patch size %d is not a multiple of 16 (bh_photo_warp_fwd)" % P)
            if c.is_cuda:
                cls._checked = (weakref.ref(corners), corners._version, P)
        return P, c[:, 0, :].to(device, torch.float32).contiguous()

    def forward(self, data):
        if 'corners' not in data:
            raise KeyError("PhotometricHead needs data['corners'] (PhotometricHead.py:20-24 asserts without them)")
        k_gt, k_img, k_dgt, k_dhat = self.learning_keys
        image, delta_hat = data[k_img], data[k_dhat]
        if not image.is_cuda:
            raise RuntimeError("bihome_amd heads run on the MI355X only; no CPU fallback (use oracle/ for CPU checks)")
        P, origin = self._window(data['corners'], data[k_gt].shape[-1], image.device)
        patch_hat = _PatchHat.apply(delta_hat, image, origin, P)
        return data[k_gt], patch_hat, data[k_dgt], delta_hat

    def predict_homography(self, data):
        if 'corners' not in data:
            raise KeyError("PhotometricHead.predict_homography needs data['corners'] (PhotometricHead.py:51-55)")
        delta_hat = data[self.learning_keys[3]]
        return delta_hat, _NoOpHead._h_from_corners(data['corners'], delta_hat)
