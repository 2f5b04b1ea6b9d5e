"""Generators of the value regimes of test_value_regimes_gpu.py (host tensors only: test_value_regimes_cpu.py checks here, without a GPU,
that they produce what the GPU tests claim of them)."""
import numpy as np
import torch

# bh_absmax (csrc/pool.hip): n & 3 elements in a scalar tail, one float4, 256 lanes x eight float4 per workgroup and pass (2048 * 4 floats:
# one side and the other of the second workgroup), one eight-deep pass of all 512 workgroups plus one float4 and a tail
ABSMAX_LENGTHS = (1, 3, 4, 5, 255, 2048 * 4 - 1, 2048 * 4, 2048 * 4 * 8 + 7, 512 * 256 * 8 * 4 + 4)


# ------------------------------------------------------------------------------------------------
# post-ReLU feature maps for the loss kernels (section 5)
# ------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(2, 5, 16), (2, 5, 64), (2, 8, 16), (2, 8, 64)]          # (B, hf, C)
AWARE_MARGIN, COS_MARGIN = 0.1, 0.05                                    # both hinge states occur on these maps (test_value_regimes_cpu.py)
FLIP = 1e-5                                  # |t| below this share of its scale: the float32 indicator may differ from the float64 one


def post_relu_features(B, hf, C, rep=1, seed=0):
    """What the extractor hands the loss kernels: relu(randn - 0.5) maps (more than half exact zeros), with the warped maps EQUAL to their
    targets in every channel on a quarter of the pixels (flat pixel index % 4 == 0) and in single channels (one in eight) elsewhere, two
    all-zero pixel vectors in f2 and two in f1w (at pixels without the all-channel tie), warped masks with two zero rows and one sample
    whose mask sum is below 1.  f1, f2, f2w, m2w, m1, m2: one entry per sample; f1w, m1w: one per hypothesis (B * rep).
    -> dict of float32 host tensors, plus 'tie' [hf,hf] bool and 'zero_f1', 'zero_f2', 'zero_f1w': EVERY all-zero vector of those maps as
    (b, i, j) - with 16 channels a vector is all zeros by chance now and then."""
    g = torch.Generator().manual_seed(977 * seed + B * 7 + hf * 31 + C + rep)
    relu = lambda *s: (torch.randn(*s, generator=g) - 0.5).clamp_min(0)
    r = lambda a: a.repeat_interleave(rep, 0)
    f1, f2, f1w, f2w = relu(B, hf, hf, C), relu(B, hf, hf, C), relu(B * rep, hf, hf, C), relu(B, hf, hf, C)
    tie = (torch.arange(hf * hf).reshape(hf, hf) % 4) == 0
    f1w = torch.where(tie[None, :, :, None] | (torch.rand(B * rep, hf, hf, C, generator=g) < 0.125), r(f2), f1w)
    f2w = torch.where(tie[None, :, :, None] | (torch.rand(B, hf, hf, C, generator=g) < 0.125), f1, f2w)
    free = [tuple(int(v) for v in p) for p in (~tie).nonzero()]
    for z in ((0,) + free[0], (B - 1,) + free[1]):
        f2[z] = 0
    for z in ((0,) + free[-1], (B * rep - 1,) + free[-2]):
        f1w[z] = 0
    m1w, m2w = torch.rand(B * rep, hf, hf, generator=g) * 0.9 + 0.1, torch.rand(B, hf, hf, generator=g) * 0.9 + 0.1
    m1w[0, :2] = 0
    m2w[-1] *= 1e-4                                          # denominator below 1: the max(den, 1) branch
    m1, m2 = torch.rand(B, hf, hf, generator=g), torch.rand(B, hf, hf, generator=g)
    dl = (torch.rand(B, 4, 2, generator=g) - 0.5) * 16
    scores = torch.softmax(torch.randn(B, rep, generator=g), -1).reshape(-1) if rep > 1 else None
    return with_zero_vectors(dict(f1=f1, f2=f2, f1w=f1w, f2w=f2w, m1w=m1w, m2w=m2w, m1=m1, m2=m2, dl=dl, scores=scores, tie=tie))


def with_zero_vectors(d):
    for k in ("f1", "f2", "f1w"):
        d["zero_" + k] = [tuple(p) for p in (d[k].abs().sum(-1) == 0).nonzero().tolist()]
    return d


def l1_margin(d, rep=1):
    """A margin at which the one-line L1 hinge is active at half of the pixels of these maps: halfway between the two middle values of
    sum |f1 - f2| - sum |f1w - f2| (an input of the loss like any other; no pixel sits on the hinge)."""
    f1, f2, f1w = (d[k].double() for k in ("f1", "f2", "f1w"))
    r = lambda a: a.repeat_interleave(rep, 0)
    v = (r((f1 - f2).abs().sum(-1)) - (f1w - r(f2)).abs().sum(-1)).flatten().sort().values
    return float(v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2


# ------------------------------------------------------------------------------------------------
# BatchNorm on channels that are not N(0.1, 1.2^2) (section 4)
# ------------------------------------------------------------------------------------------------
BN_C, BN_EPS = 32, 1e-5
BN_SHAPES = [(2, 4, 16, 16), (1, 3, 10, 14)]            # (groups, N, H, W): shift-decoded rows; three images of 140 pixels - divisions
BN_CONSTANT, BN_ZERO, BN_PLUS, BN_MINUS, BN_ONE_HOT, BN_DEAD = 0, 1, 2, 3, 4, 5
NEAR = 1e-5                                             # ReLU inputs closer to 0 than this get no output gradient (test_two_branch_batchnorm_join)


def bn_channels(groups, N, H, W, seed=0):
    """x [N,H,W,32] NHWC, gamma, beta (float32 host tensors).  Channel 0: constant 3 (var = 0 exactly); 1: constant 0; 2 / 3: mean +-1000,
    sigma 1 (|mean| / sigma ~ 2^10); 4: a single 1 among zeros in every group; 5: gamma 0.5, beta -5 - every output below 0, dead under
    ReLU; beta = 0.25 on the constant channels and the one-hot channel, so that their ReLU decision is not at a rounding; the rest
    N(0.1, 1.2^2) with gamma = 1 + 0.3 randn, beta = 0.2 randn."""
    g = torch.Generator().manual_seed(131 * seed + 7 * H + W)
    x = torch.randn(N, H, W, BN_C, generator=g) * 1.2 + 0.1
    x[..., BN_CONSTANT], x[..., BN_ZERO], x[..., BN_ONE_HOT] = 3.0, 0.0, 0.0
    x[..., BN_PLUS] = 1000.0 + torch.randn(N, H, W, generator=g)
    x[..., BN_MINUS] = -1000.0 + torch.randn(N, H, W, generator=g)
    for grp in range(groups):
        x[grp * (N // groups), H // 2, W // 3 + grp, BN_ONE_HOT] = 1.0
    gamma, beta = 1 + 0.3 * torch.randn(BN_C, generator=g), 0.2 * torch.randn(BN_C, generator=g)
    gamma[BN_DEAD], beta[BN_DEAD] = 0.5, -5.0
    beta[[BN_CONSTANT, BN_ZERO, BN_ONE_HOT]] = 0.25
    return x, gamma, beta


def bn_reference(x, gamma, beta, groups, res=None, relu=False, dtype=torch.float64):
    """Two-pass training-mode BatchNorm per group in `dtype` on torch ops (autograd-able): x [N,H,W,C] (a leaf or not) ->
    dict(y, pre: before the ReLU, scale, shift [groups,1,C], mean, var [groups,C])."""
    C = x.shape[-1]
    xg = x.to(dtype).reshape(groups, -1, C)
    mean = xg.mean(1, keepdim=True)
    var = ((xg - mean) ** 2).mean(1, keepdim=True)
    scale = gamma.to(dtype) / torch.sqrt(var + BN_EPS)
    shift = beta.to(dtype) - mean * scale
    pre = ((xg - mean) * scale + beta.to(dtype)).reshape(x.shape)
    if res is not None:
        pre = pre + res.to(dtype)
    return dict(y=pre.clamp_min(0) if relu else pre, pre=pre, scale=scale, shift=shift, mean=mean[:, 0], var=var[:, 0])


def bn_forward_bound(x, ref, res=None, shift_rounded_once=False):
    """derived.  |y - y64| <= 4 * 2^-24 (|x scale| + |mean scale| + |beta| + |y64|) per element, for the documented fp32 coefficient chain
    of the kernels (include/bihome.h, bh_bn_fwd): mean and 1 / sqrt(var + eps) are rounded to fp32, scale = gamma invstd and
    shift = beta - mean scale are fp32 operations, y = fma(x, scale, shift).  In units u = 2^-24: the rounded mean 0.5 |mean scale|, the
    product mean scale 0.5 |mean scale|, the subtraction 0.5 |shift| <= 0.5 (|beta| + |mean scale|), the relative error of scale (var to
    fp32, + eps, sqrt, reciprocal, times gamma: <= 2.5) on (x - mean) scale = y - beta, the fused multiply-add 0.5 |y|:
    <= 1.5 |mean scale| + 3 |beta| + 3 |y|.  (A residual: one more addend, one more term.)
    shift_rounded_once: |shift| in place of |mean scale| + |beta| - what a shift rounded ONCE from float64 would meet; smaller only where beta and
    mean scale cancel, and there neither the kernels nor torch's float32 BatchNorm meet it (printed as context, not asserted)."""
    C = x.shape[-1]
    groups = ref["scale"].shape[0]
    ms = (ref["mean"][:, None] * ref["scale"]).abs()
    b = (x.double().reshape(groups, -1, C) * ref["scale"]).abs() + (ref["shift"].abs() if shift_rounded_once else ms + (ref["shift"] + ref["mean"][:, None] * ref["scale"]).abs())
    b = b.reshape(x.shape) + ref["y"].detach().abs() + (res.double().abs() if res is not None else 0)
    return 4 * 2.0 ** -24 * b.detach()


def near_relu(pre):
    return pre.detach().abs() < NEAR


# ------------------------------------------------------------------------------------------------
# warp (section 6)
# ------------------------------------------------------------------------------------------------
def warp_delta(B, size):
    """Corner offsets [B,4,2] of the homographies of the degenerate-image cases: up to a quarter of the extent, sample 1 pushed 0.4 extents
    to the right - part of it samples outside its source."""
    rng = np.random.Generator(np.random.PCG64(7000 + size))
    delta = ((rng.random((B, 4, 2)) - 0.5) * size / 2).astype(np.float32)
    delta[1, :, 0] += 0.4 * size
    return delta


HORIZON = [[1, .013, .3], [.007, 1, .2], [-1 / 8, 0, 1]]      # qz = 1 - x / 8: exactly 0 on column x = 8 - the guard of csrc/warp_tap.h:33
QZ_GUARD = 1e-8


def _project_guarded(H, h, w, dtype):
    """(u, v, guard) [B,h,w] of H.(x, y, 1) as the kernels take it: (qx, qy) / qz, or (qx, qy) themselves where |qz| <= 1e-8."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    p = torch.stack([xs, ys, torch.ones_like(xs)], -1)
    q = (H.to(dtype)[:, None, None, :, :] * p[None, :, :, None, :]).sum(-1)
    qz = q[..., 2]
    guard = ~(qz.abs() > QZ_GUARD)
    one = torch.ones_like(qz)
    iz = torch.where(guard, one, 1.0 / torch.where(guard, one, qz))
    return q[..., 0] * iz, q[..., 1] * iz, guard


def warp_pixel_guard(image, H, out_hw=None, origin=None):
    """The oracle's stand-in with the kernels' guard: out(x, y) = bilinear image(origin + H.(x, y, 1)) with zero padding, written in PIXEL
    coordinates in the dtype of `image` (float64: the reference; float32: its own spread) on torch ops, differentiable in H and in the
    image.  oracle.warp_image is the same map wherever |qz| > 1e-8 (to 1e-12 in float64); it takes kornia's guard in NORMALISED
    coordinates, which under the guard samples (w - 1) / 2, (h - 1) / 2 pixels away from where the kernels do.  image [B,C,hi,wi], H [B,3,3];
    out_hw: the output grid (default: the image's), origin [B,2]: the photometric head's patch corner."""
    B, C, hi, wi = image.shape
    h, w = out_hw or (hi, wi)
    u, v, _ = _project_guarded(H, h, w, image.dtype)
    if origin is not None:
        u, v = u + origin.to(image.dtype)[:, 0, None, None], v + origin.to(image.dtype)[:, 1, None, None]
    x0, y0 = u.detach().floor(), v.detach().floor()
    fx, fy = u - x0, v - y0
    flat = image.reshape(B, C, hi * wi)
    out = 0
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx <= wi - 1) & (yy >= 0) & (yy <= hi - 1)
            idx = (yy.clamp(0, hi - 1) * wi + xx.clamp(0, wi - 1)).long().reshape(B, 1, h * w).expand(B, C, h * w)
            out = out + flat.gather(2, idx).reshape(B, C, h, w) * (wx * wy * ok)[:, None]
    return out


def guarded_coordinate_ties(H, h, w, origin=None, extent=None):
    """test_head_kernels_gpu.coordinate_ties with the guard: [B,h,w] bool, the pixels whose float64 source coordinate is within
    8 * 2^-24 * extent of an integer (extent: the largest coordinate in play, default max(h, w))."""
    u, v, _ = _project_guarded(H, h, w, torch.float64)
    if origin is not None:
        u, v = u + origin.double()[:, 0, None, None], v + origin.double()[:, 1, None, None]
    tie = 8 * 2.0 ** -24 * (extent or max(h, w))
    return ((u - u.round()).abs() < tie) | ((v - v.round()).abs() < tie)


def qz_float32(H, h, w):
    """qz [h,w] in float32 in the order of csrc/warp_tap.h: fmaf(h6, x, fmaf(h7, y, h8)), each fused multiply-add rounded once (the float64
    product of two float32 numbers is exact)."""
    h6, h7, h8 = (np.float32(v) for v in H[2])
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    inner = (np.float64(h7) * ys.astype(np.float64) + np.float64(h8)).astype(np.float32)
    return (np.float64(h6) * xs.astype(np.float64) + inner.astype(np.float64)).astype(np.float32)
