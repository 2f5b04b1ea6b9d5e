"""Thin tensor-level wrappers over the C ABI (include/bihome.h): argument checking, raw device
pointers and the current HIP stream.  No arithmetic happens here."""
import ctypes
import os

import torch

from ._lib import (AMAX_FLOATS, BN_DETERMINISTIC, DSAC_METHODS, F_DETERMINISTIC, GEOMETRY_FIELDS, ROUTE_DETERMINISTIC, ROUTE_WX3_PC, ROUTE_WX3_SHARED, BhBnIn, BhBnReduce, BhConvDesc,
                   BhPack3x3Job, ECC_STATE, ECC_SUMS, check, lib)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# Deterministic calls (include/bihome.h "Deterministic calls"): the C library has NO mode - every launch carries its own bit.  What is
# kept here is host-side convenience: a default for newly built models (BIHOME_DETERMINISTIC=1 / set_deterministic) and a scope that the
# models' forward / backward passes open around their launches with THEIR mode (net.Runner.det, the heads' .det), so two models of one
# process can run in different modes.
_DET_DEFAULT = os.environ.get("BIHOME_DETERMINISTIC", "0") == "1"
_DET_SCOPE = []


def set_deterministic(on=True):
    """The mode of calls made OUTSIDE a model's scope and the default of models built from now on: every cross-workgroup sum
    order-independent - bit-identical training steps from run to run, HIP-graph replays identical to eager steps.  Returns the
    previous default.  A model keeps the mode it was built with (net.Runner.det, head.det)."""
    global _DET_DEFAULT
    prev, _DET_DEFAULT = _DET_DEFAULT, bool(on)
    return prev


def deterministic():
    """The mode of the calls being made right now (innermost det_scope, else the default)."""
    return _DET_SCOPE[-1] if _DET_SCOPE else _DET_DEFAULT


class det_scope:
    """with det_scope(on): ... - the wrappers below set the per-call bit of every launch inside from `on`."""

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        _DET_SCOPE.append(self.on)
        return self

    def __exit__(self, *exc):
        _DET_SCOPE.pop()


def scoped_function(cls):
    """Class decorator for torch.autograd.Function subclasses that launch kernels: forward records the mode in force (ctx.det),
    backward re-opens it - a backward pass runs wherever autograd calls it, long after the model's own scope was closed."""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *a, **k):
        ctx.det = deterministic()
        return fwd(ctx, *a, **k)

    def backward(ctx, *g):
        with det_scope(ctx.det):
            return bwd(ctx, *g)
    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


def scoped_module(cls):
    """Class decorator for the head modules: the mode is fixed when the module is built (self.det) and forward /
    predict_homography open a scope with it."""
    init = cls.__init__

    def __init__(self, *a, **k):
        init(self, *a, **k)
        if not hasattr(self, "det"):
            self.det = deterministic()
    cls.__init__ = __init__
    for name in ("forward", "predict_homography"):
        fn = cls.__dict__.get(name)
        if fn is None:
            continue

        def wrap(fn):
            def method(self, *a, **k):
                with det_scope(self.det):
                    return fn(self, *a, **k)
            method.__name__, method.__doc__ = fn.__name__, fn.__doc__
            return method
        setattr(cls, name, wrap(fn))
    return cls


def _mark(d):
    _route_det(d)
    dp = getattr(d, "bh_packed", None)
    if dp is not None:
        _route_det(dp)
    return d


def _fdet():
    return F_DETERMINISTIC if deterministic() else 0


def _route_det(d):
    """The descriptor with its BH_ROUTE_DETERMINISTIC bit set from the current scope (in place: descriptors are per-call host objects)."""
    d.route = (d.route | ROUTE_DETERMINISTIC) if deterministic() else (d.route & ~ROUTE_DETERMINISTIC)
    return d


_raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice


def _stream():
    # (the raw handle of torch's current stream: two C calls - torch.cuda.current_stream() builds a Stream object through four Python
    #  frames, ~140 times per training step)
    return ctypes.c_void_p(_raw_stream(_cur_device()))


# ------------------------------------------------------------------------------------------------
# optional per-launch timing (bench.py's roofline leg): HIP events on the launch stream around each call
# ------------------------------------------------------------------------------------------------
TIMING_DETAIL = False   # True: key by launch geometry as well (per-layer tables)
TIMING = None       # None, or dict name -> {"events": [(start, end)], "flops": float, "bytes": float, "n": int}


class _Timed:
    __slots__ = ("name", "flops", "bytes", "ev")

    def __init__(self, name, flops=0.0, nbytes=0.0):
        self.name, self.flops, self.bytes = name, flops, nbytes

    def __enter__(self):
        if TIMING is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if TIMING is not None:
            self.ev[1].record()
            r = TIMING.setdefault(self.name, {"events": [], "flops": 0.0, "bytes": 0.0, "n": 0})
            r["events"].append(self.ev)
            r["flops"] += self.flops
            r["bytes"] += self.bytes
            r["n"] += 1


_VARIANT_CACHE = {}


def conv_variant(d, which, accumulate=False, bn_groups=0):
    """Kernel symbol(s) a launch described by `d` runs, as the LIBRARY reports it (bh_conv_variant executes the real
    dispatch code with the launches replaced by a name record): 'fwd' / 'dgrad' / 'wgrad'.  Used for the roofline
    attribution in bench.py and the per-launch timing tables; several launches are joined by '+'."""
    key = (tuple(getattr(d, f) for f in GEOMETRY_FIELDS), which, bool(accumulate), int(bn_groups))
    v = _VARIANT_CACHE.get(key)
    if v is None:
        buf = ctypes.create_string_buffer(256)
        if d.precision == 4 and not d.a_bound:
            # (routing does not depend on the magnitude records, but a precision-4 launch without one is refused: describe it with a dummy)
            d = _with_layout(d, d.w_layout)
            d.a_bound = d.b_bound = 256
        check(lib.bh_conv_variant(ctypes.byref(d), {"fwd": 0, "dgrad": 1, "wgrad": 2, "wgrad_det": 3, "dgrad_bnr_z": 4, "dgrad_bnr_y": 5, "dgrad_colsum": 6}[which], int(bool(accumulate)), int(bn_groups),
                                  buf, 256), "bh_conv_variant")
        v = _VARIANT_CACHE[key] = buf.value.decode()
    return v


def _conv_variant(d, which, accumulate=False, bn_groups=0):
    if TIMING is None:
        return ""
    v = conv_variant(d, which, accumulate, bn_groups)
    if TIMING_DETAIL:
        v += " %s N%d %dx%d C%d->%d k%d s%d%s" % (which.split("_")[0], d.N, d.Hi, d.Wi, d.Ci, d.Co, d.kh, d.stride, " T" if d.transposed else "")
    return v


def _bni_name(v):
    """The library's name of a plain launch with the BatchNorm-on-load template argument (second to last) switched on."""
    import re
    if v.startswith("conv3x3_pc_kernel<"):                 # conv3x3_pc_kernel<DGRAD,BNI,EM>
        return re.sub(r"<(false|true),false,", r"<\1,true,", v, count=1)
    # conv3x3_halo_kernel<..,BNI,NP,MAP4> / wgrad_x3_kernel<CB,BNI,NP>
    return re.sub(r",false,(\d)((?:,(?:false|true))*)>", r",true,\1\2>", v, count=1)


def conv_flops(d):
    """Algorithmic flops of one conv launch: 2 * MACs (same count for fwd, dgrad and wgrad)."""
    if d.transposed:
        return 2.0 * d.N * d.Hi * d.Wi * d.Ci * d.Co * d.kh * d.kw
    return 2.0 * d.N * d.Ho * d.Wo * d.Co * d.Ci * d.kh * d.kw


def _chk(t, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError("bihome_amd kernels need device tensors (got %s); there is no CPU path" % t.device)
    if t.dtype != dtype:
        raise TypeError("expected %s, got %s" % (dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
def _extents(size):
    """size: one number for a square patch, or a (W, H) pair -> (W, H) floats."""
    W, H = size if isinstance(size, (tuple, list)) else (size, size)
    return float(W), float(H)


def h4pt_fwd(delta, size):
    """delta [B,4,2] f32 -> (H64 [B,9] f64, H32 [B,3,3] f32); size: the patch extent, or (W, H) for the corners
    [[0,0],[W,0],[W,H],[0,H]]."""
    _chk(delta)
    W, H = _extents(size)
    B = delta.shape[0]
    H64 = torch.empty(B, 9, dtype=torch.float64, device=delta.device)
    H32 = torch.empty(B, 3, 3, dtype=torch.float32, device=delta.device)
    check(lib.bh_h4pt_fwd(_p(delta), B, W, H, _p(H64), _p(H32), _stream()), "bh_h4pt_fwd")
    return H64, H32


def h4pt_bwd(delta, H64, gH, size):
    _chk(delta); _chk(H64, torch.float64); _chk(gH, torch.float64)
    W, H = _extents(size)
    B = delta.shape[0]
    gd = torch.empty(B, 4, 2, dtype=torch.float32, device=delta.device)
    check(lib.bh_h4pt_bwd(_p(delta), _p(H64), _p(gH), B, W, H, _p(gd), _stream()), "bh_h4pt_bwd")
    return gd


def dlt_fwd(pf, choice, n, P):
    """pf [B,2,h,w] f32, choice [B,n*P] i64 -> Hdlt [B*n,3,3], delta_hat [B*n,4,2], eig [B*n,96] f64."""
    _chk(pf); _chk(choice, torch.int64)
    B, _, h, w = pf.shape
    assert choice.shape == (B, n * P), (choice.shape, B, n, P)
    Hd = torch.empty(B * n, 3, 3, dtype=torch.float32, device=pf.device)
    dh = torch.empty(B * n, 4, 2, dtype=torch.float32, device=pf.device)
    eig = torch.empty(B * n, 96, dtype=torch.float64, device=pf.device)
    check(lib.bh_dlt_fwd(_p(pf), _p(choice), B, n, P, h, w, _p(Hd), _p(dh), _p(eig), _stream()), "bh_dlt_fwd")
    return Hd, dh, eig


def dlt_bwd(pf, choice, eig, g_delta, n, P, g_H=None):
    """g_H [B*n,9] float64 (optional): gradient reaching the homography itself (hypothesis scoring)."""
    _chk(pf); _chk(choice, torch.int64); _chk(eig, torch.float64); _chk(g_delta); _chk(g_H, torch.float64)
    B, _, h, w = pf.shape
    g_pf = torch.zeros_like(pf)
    check(lib.bh_dlt_bwd(_p(pf), _p(choice), _p(eig), _p(g_delta), _p(g_H), B, n, P, h, w, _p(g_pf), _fdet(), _stream()), "bh_dlt_bwd")
    return g_pf


def _dsac_method(method, thr, beta):
    """-> (BH_DSAC_* code, thr, beta) of a DSACSoftmax scoring method; 'repr_error' takes neither parameter."""
    if method not in DSAC_METHODS:
        raise ValueError("unknown DSAC scoring method %r (built: %s)" % (method, ", ".join(DSAC_METHODS)))
    return DSAC_METHODS[method], float(thr), float(beta)


def dsac_scores_fwd(pf, Hd, n, method="repr_error", thr=0.0, beta=0.0):
    """scores[B,n] = softmax(-raw score) (ransac_utils.py:76-128); returns (scores, raw).  raw: the reprojection error ('repr_error'),
    the inlier ratio ('inliers_ratio', e < thr) or the soft outlier count ('soft_inliers_ratio', sum sigmoid(beta (e - thr)))."""
    _chk(pf); _chk(Hd)
    B, _, h, w = pf.shape
    err = torch.empty(B, n, dtype=torch.float32, device=pf.device)
    scores = torch.empty_like(err)
    m, thr, beta = _dsac_method(method, thr, beta)
    check(lib.bh_dsac_score(_p(pf), _p(Hd), B, n, h, w, m, thr, beta, _p(err), None, _stream()), "bh_dsac_score")
    check(lib.bh_dsac_scores_fwd(_p(err), B, n, _p(scores), _stream()), "bh_dsac_scores_fwd")
    return scores, err


def dsac_scores_bwd(pf, Hd, scores, g_scores, n, method="repr_error", thr=0.0, beta=0.0):
    """-> (g_pf [B,2,h,w], g_Hd [B*n,9] float64).  'inliers_ratio' has no adjoint (BH_E_BADARG)."""
    _chk(pf); _chk(Hd); _chk(scores); _chk(g_scores)
    B, _, h, w = pf.shape
    g_err = torch.empty_like(scores)
    g_Hd = torch.empty(B * n, 9, dtype=torch.float64, device=pf.device)
    g_pf = torch.zeros_like(pf)
    m, thr, beta = _dsac_method(method, thr, beta)
    check(lib.bh_dsac_scores_bwd(_p(pf), _p(Hd), _p(scores), _p(g_scores), B, n, h, w, m, thr, beta, _p(g_err), _p(g_Hd), _p(g_pf),
                                 _fdet(), _stream()), "bh_dsac_scores_bwd")
    return g_pf, g_Hd


def scale_samples_fwd(x, s, rep):
    """y[b] = x[b // rep] * s[b]: x [Bx, ...] (one row per sample), s [Bx * rep] -> y [Bx * rep, ...]."""
    _chk(x); _chk(s)
    Bn = s.numel()
    L = x.numel() // x.shape[0]
    y = torch.empty((Bn,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    check(lib.bh_scale_samples_fwd(_p(x), _p(s), Bn, L, rep, _p(y), _stream()), "bh_scale_samples_fwd")
    return y


def scale_samples_bwd(g_y, x, s, rep, want_gx):
    _chk(g_y); _chk(x); _chk(s)
    Bn = s.numel()
    L = x.numel() // x.shape[0]
    g_x = torch.empty_like(g_y) if want_gx else None
    g_s = torch.empty(Bn, dtype=torch.float32, device=x.device)
    check(lib.bh_scale_samples_bwd(_p(g_y), _p(x), _p(s), Bn, L, rep, _p(g_x), _p(g_s), _fdet(), _stream()), "bh_scale_samples_bwd")
    return g_x, g_s


def dsac_score(pf, Hd, n, method="repr_error", thr=0.0, beta=0.0):
    """-> (raw score [B,n], best [B] int64: its first minimum = argmax softmax(-score))."""
    _chk(pf); _chk(Hd)
    B, _, h, w = pf.shape
    err = torch.empty(B, n, dtype=torch.float32, device=pf.device)
    best = torch.empty(B, dtype=torch.int64, device=pf.device)
    m, thr, beta = _dsac_method(method, thr, beta)
    check(lib.bh_dsac_score(_p(pf), _p(Hd), B, n, h, w, m, thr, beta, _p(err), _p(best), _stream()), "bh_dsac_score")
    return err, best


def ransac_homography(pf, choice, thr=10.0, want_mask=False, check_range=True):
    """RANSAC + inlier refit of one homography per perspective field (bh_ransac_homography: upstream's
    cv2.findHomography(src, dst, cv2.RANSAC, 10) of NoOpHead.py:75-109; its LM polish is homography_refine_lm; evaluation only).
    pf [B,2,h,w] f32, choice [B,K,4] i64 (pixel indices y*w + x of the K minimal samples)
    -> (delta_hat [B,4,2], H [B,3,3], best [B] i64, n_inl [B] i32, count [B,K] i32, mask [B,h,w] u8 or None).
    count is -1 for an invalid hypothesis; n_inl = 0 flags a sample that fell back to the least-squares fit of all points.
    check_range: the indices are range-checked on the host (one device sync, skipped inside a graph capture) - for caller-supplied
    indices; a caller that drew them in range itself passes False and the call only enqueues five launches.  (The kernel treats an
    index outside the field as an invalid hypothesis and never dereferences it.)"""
    _chk(pf); _chk(choice, torch.int64)
    if pf.requires_grad:
        raise RuntimeError("ransac_homography is an evaluation path without a gradient: call it under torch.no_grad() on a detached field")
    if pf.dim() != 4 or pf.shape[1] != 2:
        raise ValueError("pf must be [B,2,h,w], got %s" % (tuple(pf.shape),))
    B, _, h, w = pf.shape
    if choice.dim() != 3 or choice.shape[0] != B or choice.shape[2] != 4 or choice.shape[1] < 1:
        raise ValueError("choice must be [B,K,4] with K >= 1, got %s for B = %d" % (tuple(choice.shape), B))
    K = choice.shape[1]
    if check_range and choice.numel() and not torch.cuda.is_current_stream_capturing() and not bool(((choice >= 0) & (choice < h * w)).all()):
        raise ValueError("bihome_amd: ransac_homography choice holds indices outside [0, %d)" % (h * w))
    dev = pf.device
    hyp = torch.empty(B, K, 9, dtype=torch.float32, device=dev)
    count = torch.empty(B, K, dtype=torch.int32, device=dev)
    best = torch.empty(B, dtype=torch.int64, device=dev)
    n_inl = torch.empty(B, dtype=torch.int32, device=dev)
    mask = torch.empty(B, h, w, dtype=torch.uint8, device=dev) if want_mask else None
    work = torch.empty(B, 32, dtype=torch.float64, device=dev)
    Hd = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
    dh = torch.empty(B, 4, 2, dtype=torch.float32, device=dev)
    check(lib.bh_ransac_homography(_p(pf), _p(choice), B, K, h, w, float(thr), _p(hyp), _p(count), _p(best), _p(n_inl), _p(mask),
                                   _p(work), _p(Hd), _p(dh), _stream()), "bh_ransac_homography")
    return dh, Hd, best, n_inl, count, mask


def homography_refine_lm(pf, H, mask=None, iters=10):
    """Levenberg-Marquardt polish of H on the reprojection error of the field's correspondences (bh_homography_refine_lm: the step
    cv2.findHomography runs after its inlier refit; evaluation only).
    pf [B,2,h,w] f32, H [B,3,3] f32 (the start, e.g. ransac_homography's; not modified), mask [B,h,w] u8 or None (every pixel)
    -> (delta_hat [B,4,2], H [B,3,3], info [B,4] f64: cost at the start, cost at the result, accepted steps, final lambda).
    One launch, no sync."""
    _chk(pf); _chk(H); _chk(mask, torch.uint8)
    if pf.requires_grad or H.requires_grad:
        raise RuntimeError("homography_refine_lm is an evaluation path without a gradient: call it under torch.no_grad() on a detached field")
    if pf.dim() != 4 or pf.shape[1] != 2:
        raise ValueError("pf must be [B,2,h,w], got %s" % (tuple(pf.shape),))
    B, _, h, w = pf.shape
    if H.numel() != B * 9 or H.shape[0] != B:
        raise ValueError("H must be [B,3,3], got %s for B = %d" % (tuple(H.shape), B))
    if mask is not None and tuple(mask.shape) != (B, h, w):
        raise ValueError("mask must be [B,h,w] = %s, got %s" % ((B, h, w), tuple(mask.shape)))
    iters = int(iters)
    if iters < 0:
        raise ValueError("iters must be >= 0")
    Hd = H.clone().view(B, 3, 3)
    dh = torch.empty(B, 4, 2, dtype=torch.float32, device=pf.device)
    info = torch.empty(B, 4, dtype=torch.float64, device=pf.device)
    check(lib.bh_homography_refine_lm(_p(pf), _p(mask), B, h, w, iters, _p(Hd), _p(dh), _p(info), _stream()), "bh_homography_refine_lm")
    return dh, Hd, info


# ------------------------------------------------------------------------------------------------
# warp
# ------------------------------------------------------------------------------------------------
def warp_fwd(img, H64, pool=4, want_cov=True):
    """img [B,C,h,w], H64 [B,9] -> (out [B,C,h,w], cov [B,h/pool,w/pool] or None)."""
    _chk(img); _chk(H64, torch.float64)
    B, C, h, w = img.shape
    out = torch.empty_like(img)
    cov = torch.empty(B, h // pool, w // pool, dtype=torch.float32, device=img.device) if want_cov else None
    with _Timed("warp_fwd_kernel", 0.0, 4.0 * (img.numel() + out.numel() + (cov.numel() if want_cov else 0))):     # 8 B/px/channel
        check(lib.bh_warp_fwd(_p(img), _p(H64), B, C, h, w, pool, _p(out), _p(cov), _fdet(), _stream()), "bh_warp_fwd")
    return out, cov


def mask_coverage_fwd(H64, h, w, pool=4):
    _chk(H64, torch.float64)
    B = H64.shape[0]
    cov = torch.empty(B, h // pool, w // pool, dtype=torch.float32, device=H64.device)
    check(lib.bh_warp_fwd(None, _p(H64), B, 1, h, w, pool, None, _p(cov), _fdet(), _stream()), "bh_warp_fwd(cov)")
    return cov


def warp_bwd(img, H64, g_out, g_cov, pool=4, gH=None):
    _chk(img); _chk(H64, torch.float64); _chk(g_out); _chk(g_cov)
    B, C, h, w = img.shape
    if gH is None:
        gH = torch.zeros(B, 9, dtype=torch.float64, device=img.device)
    with _Timed("warp_bwd_kernel", 0.0, 4.0 * (img.numel() + g_out.numel() + (g_cov.numel() if g_cov is not None else 0))):
        check(lib.bh_warp_bwd(_p(img), _p(H64), _p(g_out), _p(g_cov), B, C, h, w, pool, _p(gH), _fdet(), _stream()), "bh_warp_bwd")
    return gH


def _photo_shapes(B, Hp64, origin):
    if Hp64.numel() != B * 9 or tuple(origin.shape) != (B, 2):
        raise ValueError("photo warp: Hp64 must hold [%d,9] and origin be [%d,2] (got %s, %s)" % (B, B, tuple(Hp64.shape), tuple(origin.shape)))


def photo_warp_fwd(img, Hp64, origin, P):
    """Photometric head (PhotometricHead.py:29-42): img [B,C,Hi,Wi], Hp64 [B,9] (bh_h4pt_fwd in patch coordinates), origin [B,2] float
    (integer top-left patch corners) -> out [B,C,P,P] = bilinear img(origin + Hp.(x, y, 1)), the crop of the full-image warp."""
    _chk(img); _chk(Hp64, torch.float64); _chk(origin)
    B, C, Hi, Wi = img.shape
    _photo_shapes(B, Hp64, origin)
    out = torch.empty(B, C, P, P, dtype=torch.float32, device=img.device)
    with _Timed("photo_warp_fwd_kernel", 0.0, 4.0 * 5 * out.numel()):        # four gathered taps + one write per output pixel
        check(lib.bh_photo_warp_fwd(_p(img), _p(Hp64), _p(origin), B, C, Hi, Wi, int(P), _p(out), _fdet(), _stream()), "bh_photo_warp_fwd")
    return out


def photo_warp_bwd(img, Hp64, origin, g_out, P, gH=None):
    """Adjoint of photo_warp_fwd w.r.t. Hp: g_out [B,C,P,P] -> gH [B,9] float64 (added into gH when given, else a zeroed one)."""
    _chk(img); _chk(Hp64, torch.float64); _chk(origin); _chk(g_out); _chk(gH, torch.float64)
    B, C, Hi, Wi = img.shape
    _photo_shapes(B, Hp64, origin)
    if tuple(g_out.shape) != (B, C, P, P) or (gH is not None and tuple(gH.shape) != (B, 9)):
        raise ValueError("photo_warp_bwd: g_out must be [%d,%d,%d,%d] and gH [%d,9]" % (B, C, P, P, B))
    if gH is None:
        gH = torch.zeros(B, 9, dtype=torch.float64, device=img.device)
    with _Timed("photo_warp_bwd_kernel", 0.0, 4.0 * 5 * g_out.numel()):
        check(lib.bh_photo_warp_bwd(_p(img), _p(Hp64), _p(origin), _p(g_out), B, C, Hi, Wi, int(P), _p(gH), _fdet(), _stream()),
              "bh_photo_warp_bwd")
    return gH


def warp_bwd_img(H64, g_out):
    """Adjoint of warp_fwd w.r.t. the image (the trained masks of the Zhang baseline, TripletHead.py:60,69): g_out[B,C,h,w] -> g_img."""
    _chk(H64, torch.float64); _chk(g_out)
    B, C, h, w = g_out.shape
    g_img = torch.empty_like(g_out)
    flags = _fdet()
    n = lib.bh_warp_bwd_img_scratch_doubles(B, C, h, w, flags)
    scratch = torch.empty(n, dtype=torch.float64, device=g_out.device) if n else None
    check(lib.bh_warp_bwd_img(_p(H64), _p(g_out), B, C, h, w, _p(g_img), _p(scratch), flags, _stream()), "bh_warp_bwd_img")
    return g_img


# ------------------------------------------------------------------------------------------------
# trained content masks (Zhang baseline, FIX_MASK False)
# ------------------------------------------------------------------------------------------------
def mask_fwd(y, f, strength):
    """y[N,1,h,w] = the mask predictor's last BatchNorm output, f = the features (None: mask only) -> (m, g | None, smax[N], imax[N])
    (ContentAware.py:24-26,28-35,128-134: Sigmoid, per-sample max normalisation when strength > 0, G = m * f)."""
    _chk(y); _chk(f)
    N, P = y.shape[0], y.numel() // y.shape[0]
    m = torch.empty_like(y)
    g = torch.empty_like(y) if f is not None else None
    smax = torch.empty(N, dtype=torch.float32, device=y.device)
    imax = torch.empty(N, dtype=torch.int32, device=y.device)
    check(lib.bh_mask_fwd(_p(y), _p(f), N, P, float(strength), _p(m), _p(g), _p(smax), _p(imax), _stream()), "bh_mask_fwd")
    return m, g, smax, imax


def mask_bwd(y, f, m, smax, imax, g_m, g_g, strength, want_gf=True):
    """-> (g_y, g_f | None); g_m / g_g None = no gradient from that consumer."""
    for t in (y, f, m, g_m, g_g):
        _chk(t)
    N, P = y.shape[0], y.numel() // y.shape[0]
    g_y = torch.empty_like(y)
    g_f = torch.empty_like(y) if (want_gf and g_g is not None) else None
    check(lib.bh_mask_bwd(_p(y), _p(f), _p(m), _p(smax), _p(imax), _p(g_m), _p(g_g), N, P, float(strength), _p(g_y), _p(g_f), _stream()),
          "bh_mask_bwd")
    return g_y, g_f


# ------------------------------------------------------------------------------------------------
# triplet
# ------------------------------------------------------------------------------------------------
def _triplet_fwd(entry, kernel, margin, f1, f2, f1w, f2w, m1w, m2w, m1, m2):
    for t in (f1, f2, f1w, f2w, m1w, m2w, m1, m2):
        _chk(t)
    B, hf, wf, C = f1.shape
    M1 = torch.empty(B, hf, wf, dtype=torch.float32, device=f1.device)
    M2 = torch.empty_like(M1)
    numden = torch.empty(B, 4, dtype=torch.float64, device=f1.device)
    with _Timed(kernel, 0.0, 4.0 * (4 * f1.numel() + 4 * M1.numel())):      # 4 feature maps in, masks in, M1 / M2 out
        check(getattr(lib, entry)(_p(f1), _p(f2), _p(f1w), _p(f2w), _p(m1w), _p(m2w), _p(m1), _p(m2), B, hf * wf, C, *margin,
                                  _p(M1), _p(M2), _p(numden), _fdet(), _stream()), entry)
    return M1, M2, numden


def triplet_l1_fwd(f1, f2, f1w, f2w, m1w, m2w, m1=None, m2=None):
    """features NHWC [B,hf,wf,C]; masks [B,hf,wf]."""
    return _triplet_fwd("bh_triplet_l1_fwd", "triplet_fwd_kernel", (), f1, f2, f1w, f2w, m1w, m2w, m1, m2)


def triplet_hinge_fwd(f1, f2, f1w, f2w, m1w, m2w, margin, m1=None, m2=None):
    """biHomE with the hinge inside the channel sum ('channel-aware', numeric margin: PerceptualHead.py:624-625,644-645); shapes and
    returns as triplet_l1_fwd."""
    return _triplet_fwd("bh_triplet_hinge_fwd", "triplet_fwd_kernel<L1ChannelHinge, 2>", (float(margin),), f1, f2, f1w, f2w, m1w, m2w, m1, m2)


def _oneline_fwd(entry, f1, f2, f1w, m1w, margin, m2, rep, sample_w):
    for t in (f1, f2, f1w, m1w, m2, sample_w):
        _chk(t)
    B, hf, wf, C = f1w.shape
    T = torch.empty(B, hf, wf, dtype=torch.float32, device=f1.device)
    numden = torch.empty(B, 2, dtype=torch.float64, device=f1.device)
    per = torch.empty(B, dtype=torch.float32, device=f1.device)
    loss = torch.empty(1, dtype=torch.float32, device=f1.device)
    check(getattr(lib, entry)(_p(f1), _p(f2), _p(f1w), _p(m1w), _p(m2), B, hf * wf, C, float(margin), rep, _p(sample_w), _p(T),
                              _p(numden), _p(per), _p(loss), _fdet(), _stream()), entry)
    return loss, T, numden, per


def _oneline_bwd(entry, g_loss, f2, f1w, m1w, T, numden, m2, rep, sample_w):
    _chk(g_loss); _chk(sample_w)
    B, hf, wf, C = f1w.shape
    g_f1w = torch.empty_like(f1w)
    g_m1w = torch.empty(B, hf, wf, dtype=torch.float32, device=f1w.device)
    check(getattr(lib, entry)(_p(g_loss), _p(f2), _p(f1w), _p(m1w), _p(m2), _p(T), _p(numden), B, hf * wf, C, rep, _p(sample_w),
                              _p(g_f1w), _p(g_m1w), _stream()), entry)
    return g_f1w, g_m1w


def oneline_loss_fwd(f1, f2, f1w, m1w, margin, m2=None, rep=1, sample_w=None):
    """iHomE one-line hinge loss (PerceptualHead.py:465-538): returns (loss[1], T[B,hf,wf], numden[B,2], per_sample[B]).
    rep > 1: B = samples * rep hypotheses; f1 / f2 / m2 hold one entry per sample; sample_w[B] = DSAC scores."""
    return _oneline_fwd("bh_oneline_loss_fwd", f1, f2, f1w, m1w, margin, m2, rep, sample_w)


def oneline_loss_bwd(g_loss, f2, f1w, m1w, T, numden, m2=None, rep=1, sample_w=None):
    return _oneline_bwd("bh_oneline_loss_bwd", g_loss, f2, f1w, m1w, T, numden, m2, rep, sample_w)


def oneline_cos_loss_fwd(f1, f2, f1w, m1w, margin, m2=None, rep=1, sample_w=None):
    """The one-line hinge loss on cosine distances (TRIPLET_DISTANCE 'cosine', PerceptualHead.py:485-499): arguments and returns as
    oneline_loss_fwd, T = c(f1, f2) - c(f1w, f2) + margin."""
    return _oneline_fwd("bh_oneline_cos_loss_fwd", f1, f2, f1w, m1w, margin, m2, rep, sample_w)


def oneline_cos_loss_bwd(g_loss, f2, f1w, m1w, T, numden, m2=None, rep=1, sample_w=None):
    return _oneline_bwd("bh_oneline_cos_loss_bwd", g_loss, f2, f1w, m1w, T, numden, m2, rep, sample_w)


def zhang_triplet_fwd(f1, f2, f1w, f2w, m1w, m2w, margin, hinge, m1=None, m2=None):
    """Zhang content-aware triplet loss on one-channel full-resolution features [B,1,h,w] / masks [B,h,w] (TripletHead.py:75-152):
    returns (T1, T2 | None, numden[B,4]).  f2w / m2w None: one line."""
    for t in (f1, f2, f1w, f2w, m1w, m2w, m1, m2):
        _chk(t)
    B, hw = f1.shape[0], f1.numel() // f1.shape[0]
    T1 = torch.empty(B, hw, dtype=torch.float32, device=f1.device)
    T2 = torch.empty_like(T1) if f2w is not None else None
    numden = torch.empty(B, 4, dtype=torch.float64, device=f1.device)
    check(lib.bh_zhang_triplet_fwd(_p(f1), _p(f2), _p(f1w), _p(f2w), _p(m1w), _p(m2w), _p(m1), _p(m2), B, hw, float(margin), int(bool(hinge)),
                                   _p(T1), _p(T2), _p(numden), _stream()), "bh_zhang_triplet_fwd")
    return T1, T2, numden


def zhang_triplet_bwd(g_loss, f1, f2, f1w, f2w, m1w, m2w, T1, T2, numden, hinge, m1=None, m2=None, mask_grads=False):
    """-> (g_f1, g_f2, g_f1w, g_f2w | None, g_m1w, g_m2w | None), shaped like their tensors; mask_grads (trained masks): two more,
    (g_m1, g_m2) - the gradients of the unwarped masks."""
    _chk(g_loss)
    B, hw = f1.shape[0], f1.numel() // f1.shape[0]
    g_f1, g_f2, g_f1w = torch.empty_like(f1), torch.empty_like(f2), torch.empty_like(f1w)
    g_m1w = torch.empty_like(m1w)
    g_f2w = torch.empty_like(f2w) if f2w is not None else None
    g_m2w = torch.empty_like(m2w) if f2w is not None else None
    g_m1 = torch.empty_like(m1w) if mask_grads else None
    g_m2 = torch.empty_like(m1w) if mask_grads else None
    check(lib.bh_zhang_triplet_bwd(_p(g_loss), _p(f1), _p(f2), _p(f1w), _p(f2w), _p(m1w), _p(m2w), _p(m1), _p(m2), _p(T1), _p(T2), _p(numden),
                                   B, hw, int(bool(hinge)), _p(g_f1), _p(g_f2), _p(g_f1w), _p(g_f2w), _p(g_m1w), _p(g_m2w), _p(g_m1), _p(g_m2),
                                   _stream()), "bh_zhang_triplet_bwd")
    if mask_grads:
        return g_f1, g_f2, g_f1w, g_f2w, g_m1w, g_m2w, g_m1, g_m2
    return g_f1, g_f2, g_f1w, g_f2w, g_m1w, g_m2w


def bihome_loss_fwd(numden, H1, H2, mu):
    _chk(numden, torch.float64); _chk(H1, torch.float64); _chk(H2, torch.float64)
    loss4 = torch.empty(4, dtype=torch.float32, device=numden.device)
    check(lib.bh_bihome_loss_fwd(_p(numden), _p(H1), _p(H2), numden.shape[0], float(mu), _p(loss4), _stream()),
          "bh_bihome_loss_fwd")
    return loss4


def _bihome_bwd(entry, kernel, maps, margin, g_loss, f1, f2, f1w, f2w, m1w, m2w, m1, m2, M1, M2, numden, H1, H2, mu, joined):
    _chk(g_loss)
    B, hf, wf, C = f1.shape
    g_fw = torch.empty((2 * B,) + tuple(f1w.shape[1:]), dtype=torch.float32, device=f1.device)
    g_mw = torch.empty((2 * B,) + tuple(m1w.shape[1:]), dtype=torch.float32, device=f1.device)
    gH = torch.empty(2 * B, 9, dtype=torch.float64, device=f1.device)
    g_f1w, g_f2w, g_m1w, g_m2w, gH1, gH2 = g_fw[:B], g_fw[B:], g_mw[:B], g_mw[B:], gH[:B], gH[B:]
    with _Timed(kernel, 0.0, 4.0 * (maps * f1.numel() + 6 * M1.numel())):      # feature maps read + the 2 gradients written
        check(getattr(lib, entry)(_p(g_loss), _p(f1), _p(f2), _p(f1w), _p(f2w), _p(m1w), _p(m2w), _p(m1), _p(m2), _p(M1),
                                  _p(M2), _p(numden), _p(H1), _p(H2), B, hf * wf, C, *margin, float(mu), _p(g_f1w), _p(g_f2w),
                                  _p(g_m1w), _p(g_m2w), _p(gH1), _p(gH2), _stream()), entry)
    if joined:
        return g_fw, g_mw, gH
    return g_f1w, g_f2w, g_m1w, g_m2w, gH1, gH2


def bihome_loss_bwd(g_loss, f1, f2, f1w, f2w, m1w, m2w, m1, m2, M1, M2, numden, H1, H2, mu, joined=False):
    """joined: the two directions' outputs are the halves of ONE [2B, ...] tensor each and (g_fw, g_mw, gH) are returned whole (the
    caller's extractor / warp adjoints take both directions in one call: no torch.cat of 33 MB)."""
    return _bihome_bwd("bh_bihome_loss_bwd", "triplet_bwd_kernel", 6, (), g_loss, f1, f2, f1w, f2w, m1w, m2w, m1, m2, M1, M2, numden,
                       H1, H2, mu, joined)


def triplet_hinge_bwd(g_loss, f1, f2, f1w, f2w, m1w, m2w, m1, m2, M1, M2, numden, H1, H2, margin, mu, joined=False):
    """The adjoint of triplet_hinge_fwd + bihome_loss_fwd; arguments (plus the margin) and returns as bihome_loss_bwd."""
    return _bihome_bwd("bh_triplet_hinge_bwd", "triplet_bwd_kernel<L1ChannelHinge, 2>", 8, (float(margin),), g_loss, f1, f2, f1w, f2w, m1w, m2w, m1, m2,
                       M1, M2, numden, H1, H2, mu, joined)


# ------------------------------------------------------------------------------------------------
# trainable projection head (csrc/proj.hip)
# ------------------------------------------------------------------------------------------------
def l2norm_fwd(x):
    """x [..., C] -> (y = x / |x|_2 over the last axis, inv[...] = 1 / |x|_2): PerceptualHead.py:470-479 (no epsilon, as upstream)."""
    _chk(x)
    C = x.shape[-1]
    y, inv = torch.empty_like(x), torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    with _Timed("l2norm_fwd_kernel", 0.0, 8.0 * x.numel()):
        check(lib.bh_l2norm_fwd(_p(x), x.numel() // C, C, _p(y), _p(inv), _stream()), "bh_l2norm_fwd")
    return y, inv


def l2norm_bwd(g, y, inv):
    """gx = inv (g - y (y . g)): the adjoint of l2norm_fwd from its outputs."""
    _chk(g); _chk(y); _chk(inv)
    C = y.shape[-1]
    gx = torch.empty_like(y)
    with _Timed("l2norm_bwd_kernel", 0.0, 12.0 * y.numel()):
        check(lib.bh_l2norm_bwd(_p(g), _p(y), _p(inv), y.numel() // C, C, _p(gx), _stream()), "bh_l2norm_bwd")
    return gx


def relu_bwd(gy, y):
    """gx = gy [y > 0] (y: the ReLU's output)."""
    _chk(gy); _chk(y)
    gx = torch.empty_like(gy)
    with _Timed("relu_bwd_kernel", 0.0, 12.0 * y.numel()):
        check(lib.bh_relu_bwd(_p(gy), _p(y), y.numel(), _p(gx), _stream()), "bh_relu_bwd")
    return gx


def oneline_anchor_bwd(g_loss, f1, f2, f1w, m1w, T, numden, m2=None, rep=1, sample_w=None, cosine=False, out=None):
    """(g_f1, g_f2) [samples,hf,wf,C]: the gradient of oneline_loss_fwd / oneline_cos_loss_fwd w.r.t. the unwarped maps, the `rep`
    hypotheses of a sample added in order (include/bihome.h bh_oneline_anchor_bwd).  out: a [2 samples,hf,wf,C] tensor whose halves take
    the two gradients."""
    for t in (g_loss, f1, f2, f1w, m1w, T, m2, sample_w):
        _chk(t)
    _chk(numden, torch.float64)
    B, hf, wf, C = f1w.shape
    if out is None:
        out = torch.empty((2 * f1.shape[0],) + tuple(f1.shape[1:]), dtype=torch.float32, device=f1.device)
    _chk(out)
    g_f1, g_f2 = out[:f1.shape[0]], out[f1.shape[0]:]
    with _Timed("oneline_anchor_bwd_kernel", 0.0, 4.0 * (4 * f1.numel() + f1w.numel())):
        check(lib.bh_oneline_anchor_bwd(_p(g_loss), _p(f1), _p(f2), _p(f1w), _p(m1w), _p(m2), _p(T), _p(numden), B, hf * wf, C, rep,
                                        _p(sample_w), int(bool(cosine)), _p(g_f1), _p(g_f2), _stream()), "bh_oneline_anchor_bwd")
    return g_f1, g_f2


def bihome_anchor_bwd(g_loss, f1, f2, f1w, f2w, m1w, m2w, numden, m1=None, m2=None, margin=None, out=None):
    """(g_f1, g_f2) [B,hf,wf,C]: the gradient of triplet_l1_fwd (margin None) / triplet_hinge_fwd (numeric margin) + bihome_loss_fwd
    w.r.t. the unwarped maps (include/bihome.h bh_bihome_anchor_bwd).  out: a [2B,hf,wf,C] tensor whose halves take the two gradients."""
    for t in (g_loss, f1, f2, f1w, f2w, m1w, m2w, m1, m2):
        _chk(t)
    _chk(numden, torch.float64)
    B, hf, wf, C = f1.shape
    if out is None:
        out = torch.empty((2 * B, hf, wf, C), dtype=torch.float32, device=f1.device)
    _chk(out)
    g_f1, g_f2 = out[:B], out[B:]
    with _Timed("bihome_anchor_bwd_kernel", 0.0, 4.0 * 6 * f1.numel()):
        check(lib.bh_bihome_anchor_bwd(_p(g_loss), _p(f1), _p(f2), _p(f1w), _p(f2w), _p(m1w), _p(m2w), _p(m1), _p(m2), _p(numden), B, hf * wf,
                                       C, float(margin or 0.0), int(margin is not None), _p(g_f1), _p(g_f2), _stream()),
              "bh_bihome_anchor_bwd")
    return g_f1, g_f2


# ------------------------------------------------------------------------------------------------
# conv stacks
# ------------------------------------------------------------------------------------------------
# conv arithmetic (bh_conv_desc.precision).  'f32' (default) asks for fp32 ACCURACY and lets the library pick the evaluation.
# Round 4: the packed 3x3 kernels (forward, dgrad, weight gradient: 80 % of the step's flops) evaluate every product from TWO FP16
# pieces per operand of the operand times a power-of-two scale per tensor - 22 significand bits and a sign, three partial products
# on v_mfma_f32_32x32x16_f16 with fp32 accumulate, results rescaled exactly (precision 4, "f16x2": ~2^-22 per product; against
# float64 the kernels measure at or BELOW the error of the fp32-input MFMA kernels on every shape tested, tests/test_f16x2_gpu.py,
# because sixteen products enter one fp32 accumulate rounding instead of two).  Everything else runs v_mfma_f32_32x32x2_f32.
# 'f32x3' (precision 2, the default of rounds 2-3): the exact cut into three bf16 pieces, six partial products per product.
# 'f32-mfma' forces the fp32-input MFMA everywhere (precision 0); 'bf16' rounds the operands to bf16 (precision 1).
# 'f32x2' (precision 3): two bf16 pieces per operand, both rounded to nearest, three products - ~4e-6 per product (13x the fp32
# rounding, 500x below 'bf16'); a separately reported reduced-precision arithmetic.
PRECISION = {"f32": 4, "fp32": 4, "f16x2": 4, "f32x3": 2, "f32-mfma": 0, "bf16": 1, "f32x2": 3}
SPLIT_PIECES = {2: 3, 3: 2, 4: 2}   # precision -> pieces per operand of the split-operand kernels
SPLIT_LAYOUT = {2: 2, 3: 3, 4: 4}   # precision -> bh_conv_desc.w_layout of the packed split weights
F16X2 = 4


def amax_record(device):
    """A zeroed magnitude record (include/bihome.h BH_AMAX_FLOATS); net.run_forward / run_backward cut theirs from one arena."""
    return torch.zeros(AMAX_FLOATS, dtype=torch.float32, device=device)


def absmax(x, rec=None):
    """Magnitude record of a tensor by a streaming pass (the fallback where no producer kernel left one)."""
    _chk(x)
    if rec is None:
        rec = amax_record(x.device)
    with _Timed("absmax_kernel", 0.0, 4.0 * x.numel()):
        check(lib.bh_absmax(_p(x), x.numel(), _p(rec), _stream()), "bh_absmax")
    return rec


def amax_of(x, make=True):
    """The magnitude record attached to a tensor (or BnOnLoad) by its producer; make: measure it when there is none."""
    rec = x.amax if isinstance(x, BnOnLoad) else getattr(x, "_bh_amax", None)
    if rec is None and make:
        if isinstance(x, BnOnLoad):
            raise RuntimeError("BatchNorm-on-load operand without a magnitude record (bn_fwd_coeffs(..., amax=...))")
        rec = x._bh_amax = absmax(x)
    return rec


def packed_layout(precision):
    """bh_conv_desc.w_layout of WeightPacker copies for this precision (1: fp32 fragments, 2 / 3: three / two bf16 pieces)."""
    return SPLIT_LAYOUT.get(int(precision), 1)
_ENV_ROUTE = int(os.environ.get("BIHOME_ROUTE", "0"))     # benchmarks: OR these BH_ROUTE_* bits into every conv descriptor


def conv_desc(N, Hi, Wi, Ci, Co, k, stride, pad, transposed=False, in_nchw=False, out_nchw=False, precision=0, route=0):
    d = BhConvDesc()
    d.precision = int(precision)
    d.route = int(route) | _ENV_ROUTE | (ROUTE_DETERMINISTIC if deterministic() else 0)
    d.N, d.Hi, d.Wi, d.Ci, d.Co = N, Hi, Wi, Ci, Co
    d.kh = d.kw = k
    d.stride, d.pad = stride, pad
    d.transposed, d.in_nchw, d.out_nchw = int(transposed), int(in_nchw), int(out_nchw)
    if transposed:
        d.Ho, d.Wo = Hi * stride, Wi * stride
    else:
        d.Ho, d.Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    return d


def conv_out_shape(d):
    return (d.N, d.Co, d.Ho, d.Wo) if d.out_nchw else (d.N, d.Ho, d.Wo, d.Co)


def _with_layout(d, w_layout):
    d2 = BhConvDesc()
    ctypes.memmove(ctypes.byref(d2), ctypes.byref(d), ctypes.sizeof(BhConvDesc))
    d2.w_layout = w_layout
    return d2


# the halo-tiled 3x3 kernels: one workgroup per tile position (csrc/conv3x3.hip) / persistent producer-consumer workgroups (csrc/conv3x3_pc.hip)
_C3_KERNELS = ("conv3x3_halo_kernel", "conv3x3_pc_kernel")


def packs_3x3(d):
    """True when the halo-tiled 3x3 kernel takes both the forward and the dgrad of this conv (then the fragment-ordered
    weight copies of bh_conv3x3_pack can be used for it)."""
    # (asked with the layout the packed copies would have: the 4 x 4 map form of the halo kernel exists for split operands only)
    q = _with_layout(d, packed_layout(d.precision)) if (d.w_layout == 0 and int(d.precision) in SPLIT_PIECES) else d
    try:
        return conv_variant(q, "fwd").startswith(_C3_KERNELS) and conv_variant(q, "dgrad").startswith(_C3_KERNELS)
    except Exception:
        return False


class WeightPacker:
    """Fragment-ordered copies (forward and dgrad operand order) of the 3x3 conv weights of one module tree, refreshed by
    ONE bh_conv3x3_pack launch whenever a parameter version changed (every optimizer step in training, once for frozen
    weights).  Buffers and the device job table are allocated once (addresses stay fixed: HIP-graph safe)."""
    _serials = 0

    def __init__(self, split=False, f16=False):
        # split: False / 0 = fp32 fragments (w_layout 1); True / 3 = three exact bf16 pieces (w_layout 2, precision 2);
        # 2 = two rounded bf16 pieces (w_layout 3, precision 3 "f32x2"); 2 with f16: two fp16 pieces of w 2^k (w_layout 4, precision 4)
        self.pieces = 0 if not split else (2 if (split == 2 and split is not True) else 3)
        self.split = self.pieces > 0
        self.f16 = bool(f16)
        if self.f16 and self.pieces != 2:
            raise ValueError("fp16 pieces: two per weight")
        self.layout = 4 if self.f16 else {0: 1, 3: 2, 2: 3}[self.pieces]
        self.job_split = 3 if self.f16 else {0: 0, 3: 1, 2: 2}[self.pieces]
        self.entries = {}          # id(weight) -> (weight, pf, pd)
        WeightPacker._serials += 1
        self.serial = WeightPacker._serials       # names this packer in cache keys (net.run_forward's plan cache)
        self.table = None
        self.versions = None
        self.dirty = False         # a training forward ran since the last pack: the optimizer has (probably) moved the weights

    def get(self, weight, need_dgrad=True):
        e = self.entries.get(id(weight))
        if e is None:
            Co, Ci = weight.shape[0], weight.shape[1]
            n = weight.numel() * self.pieces // 2 if self.split else weight.numel()
            if self.f16:
                n += 16                       # the layer's sixteen partial maxima of |w| (bh_conv3x3_pack_f16)
            pf = torch.empty(n, dtype=torch.float32, device=weight.device)
            pd = torch.empty(n, dtype=torch.float32, device=weight.device) if need_dgrad else None
            e = self.entries[id(weight)] = (weight, pf, pd)
            self.table = None
        return e[1], e[2]

    def invalidate(self):
        """The weights changed behind the version counters (graph replay, broadcast into .data): repack at the next refresh."""
        self.versions = None
        self.dirty = True

    def refresh(self, training=False):
        """Repack when a parameter changed.  Version counters catch load_state_dict / copy_ / the default optimizers, but
        torch's FUSED optimizers update parameters without bumping them - so trainable weights are repacked on every
        training forward, and on the first inference forward after one."""
        if not self.entries:
            return
        vers = tuple((w._version, w.data_ptr()) for w, _, _ in self.entries.values())
        trainable = any(w.requires_grad for w, _, _ in self.entries.values())
        force = trainable and (training or self.dirty)
        self.dirty = bool(training and trainable)
        if self.table is not None and vers == self.versions and not force:
            return
        if self.table is None or any(p != q[1] for p, q in zip(self._ptrs, vers)):
            jobs = (BhPack3x3Job * len(self.entries))()
            for j, (w, pf, pd) in zip(jobs, self.entries.values()):
                if not w.permute(0, 2, 3, 1).is_contiguous():
                    raise RuntimeError("conv weight is not in kernel (channels_last) layout")
                j.w, j.pf, j.pd = w.data_ptr(), pf.data_ptr(), (pd.data_ptr() if pd is not None else None)
                j.Co, j.Ci, j.split = w.shape[0], w.shape[1], self.job_split
            raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8)
            dev = next(iter(self.entries.values()))[0].device
            self.table = raw.to(dev)
            self._ptrs = [v[1] for v in vers]
        if self.f16:
            check(lib.bh_conv3x3_pack_f16(_p(self.table), len(self.entries), _stream()), "bh_conv3x3_pack_f16")
        else:
            check(lib.bh_conv3x3_pack(_p(self.table), len(self.entries), _stream()), "bh_conv3x3_pack")
        self.versions = vers


def packer_for_precision(precision):
    """A WeightPacker whose copies are what the packed kernels of this precision read."""
    p = int(precision)
    return WeightPacker(split=SPLIT_PIECES.get(p, 0), f16=p == F16X2)


class BnOnLoad:
    """A training-mode BatchNorm(+ReLU) whose APPLY rides in its consumer: `z` is the BatchNorm's input, `table` the
    [groups][C] x (scale, shift) coefficients made by bn_fwd_coeffs.  The f32x3 3x3 forward and weight-gradient kernels take
    it as their input operand and transform it while staging (zero padding stays zero): the BatchNorm's output is never stored."""
    __slots__ = ("z", "table", "groups", "relu", "amax")

    def __init__(self, z, table, groups, relu, amax=None):
        self.z, self.table, self.groups, self.relu = z, table, groups, relu
        self.amax = amax            # magnitude record of the (never stored) BatchNorm output: precision 4 consumers

    @property
    def shape(self):
        return self.z.shape

    def struct(self):
        b = BhBnIn()
        b.table, b.groups, b.relu = self.table.data_ptr(), int(self.groups), int(bool(self.relu))
        return b


def bn_fwd_coeffs(stats, gamma, beta, rmean, rvar, groups, rows, C, eps, momentum, amax=None):
    """(scale, shift) table of a training-mode BatchNorm from its forward sums (+ the running-statistics update).
    amax: zeroed magnitude record - receives the a-priori bound of the BatchNorm's output."""
    table = torch.empty((groups, C, 2), dtype=torch.float32, device=stats.device)
    check(lib.bh_bn_fwd_coeffs(_p(stats), _p(gamma), _p(beta), _p(rmean), _p(rvar), groups, rows, C, float(eps), float(momentum),
                               _p(table), _p(amax), _stream()), "bh_bn_fwd_coeffs")
    return table


def conv_fwd(x, w, bias, d, bn_sums=None, groups=1, res=None, relu=False, wpacked=None, amax=None, warp_src=None):
    """wpacked: the forward buffer of WeightPacker for this conv (then `w` is only used for the byte count).
    bn_sums: zeroed float64 sums buffer - the conv also accumulates the batch statistics of its output for the
    BatchNorm that follows (bn_fwd(..., stats=bn_sums, stats_ready=True)).  res / relu: inference epilogue
    y = act(conv + bias + res) (BatchNorm folded into w, bias by the caller).
    warp_src (round 6; the extractor's one-plane stem only): dict(src, H64, pool, cov[, want_image]) - x is an UNFILLED buffer for the
    homography warp of `src`; where the fused kernel applies, the stem makes the warped pixels itself (bh_stem7_fwd_warp: warp_src["cov"]
    and - unless want_image is False - x are written on the way; warp_src["done"] is set), else bh_warp_fwd fills them here and the conv
    runs as always."""
    _mark(d)
    if warp_src is not None:
        ws_ = warp_src
        _chk(ws_["src"]); _chk(ws_["H64"], torch.float64); _chk(ws_["cov"]); _chk(x); _chk(w); _chk(bias); _chk(bn_sums, torch.float64)
        B_, h_, w_ = ws_["src"].shape[0], ws_["src"].shape[-2], ws_["src"].shape[-1]
        if (res is None and not relu and wpacked is None and amax is None and d.Ci == 1 and d.precision == F16X2 and ws_["pool"] == 4
                and not d.transposed and d.kh == 7 and d.kw == 7 and d.stride == 2 and d.pad == 3 and d.Co == 64 and not d.out_nchw
                and d.Ho % 8 == 0 and d.Wo % 8 == 0 and d.Ho * 2 == d.Hi and d.Wo * 2 == d.Wi and d.N * (d.Ho // 8) * (d.Wo // 8) >= 256
                and w.is_contiguous() and os.environ.get("BIHOME_WARP_IN_STEM_FWD", "1") != "0"):
            y = torch.empty(conv_out_shape(d), dtype=torch.float32, device=x.device)
            with _Timed("stem7_fwd_f16_kernel<1,true>", conv_flops(d), 4.0 * (2 * x.numel() + y.numel() + w.numel())):
                # (want_image False: nobody reads the warped image - the kernel keeps it to itself, x stays unfilled)
                rc = lib.bh_stem7_fwd_warp(_p(ws_["src"]), _p(ws_["H64"]), 4, _p(w), _p(bias), _p(y), ctypes.byref(d),
                                           _p(x) if ws_.get("want_image", True) else None, _p(ws_["cov"]), _p(bn_sums), groups, _stream())
            if rc != -2:                                 # (BH_E_UNSUPPORTED: the geometry is not the fp16-piece stem's - the two calls)
                check(rc, "bh_stem7_fwd_warp")
                ws_["done"] = ws_["filled"] = True
                return y
        with _Timed("warp_fwd_kernel", 0.0, 4.0 * (2 * x.numel() + (ws_["cov"].numel() if ws_["cov"] is not None else 0))):
            check(lib.bh_warp_fwd(_p(ws_["src"]), _p(ws_["H64"]), B_, 1, h_, w_, int(ws_["pool"]), _p(x), _p(ws_["cov"]), _fdet(), _stream()),
                  "bh_warp_fwd")
        ws_["filled"] = True
    if isinstance(x, BnOnLoad):
        # the BatchNorm in front of this conv is applied on load (packed f32x3 forward only)
        bol, x = x, x.z
        _chk(x); _chk(bias); _chk(bn_sums, torch.float64)
        if d.kh == 1 and wpacked is None and res is None and not relu:
            # round 4: a 1x1 conv behind BatchNorm + ReLU (decoder units) - the generic kernel transforms its A operand while staging
            _chk(w)
            y = torch.empty(conv_out_shape(d), dtype=torch.float32, device=x.device)
            bs = bol.struct()
            with _Timed((conv_variant(d, "fwd") + " bnin" + (" fwd N%d %dx%d C%d->%d k1" % (d.N, d.Hi, d.Wi, d.Ci, d.Co) if TIMING_DETAIL else "")) if TIMING is not None else "",
                        conv_flops(d), 4.0 * (x.numel() + y.numel() + w.numel())):
                check(lib.bh_conv_fwd_bnin(_p(x), _p(w), _p(bias), _p(y), ctypes.byref(d), _p(bn_sums), groups, ctypes.byref(bs), _stream()),
                      "bh_conv_fwd_bnin(1x1)")
            return y
        if wpacked is None or res is not None or relu:
            raise RuntimeError("BatchNorm-on-load needs the packed f32x3 3x3 forward")
        y = torch.empty(conv_out_shape(d), dtype=torch.float32, device=x.device)
        dp = getattr(d, "bh_packed", None) or _with_layout(d, packed_layout(d.precision))
        _route_det(dp)
        if dp.precision == F16X2:
            dp.a_bound = amax_of(bol).data_ptr()
        bs = bol.struct()
        # (the library's name of the plain launch with the last template argument - BatchNorm-on-load - switched on)
        with _Timed(_bni_name(_conv_variant(dp, "fwd", bn_groups=groups if bn_sums is not None else 0)) if TIMING is not None else "",
                    conv_flops(d), 4.0 * (x.numel() + y.numel() + w.numel())):
            check(lib.bh_conv_fwd_bnin(_p(x), _p(wpacked), _p(bias), _p(y), ctypes.byref(dp), _p(bn_sums), groups, ctypes.byref(bs),
                                       _stream()), "bh_conv_fwd_bnin")
        return y
    _chk(x); _chk(w); _chk(bias); _chk(res)
    y = torch.empty(conv_out_shape(d), dtype=torch.float32, device=x.device)
    if wpacked is not None:
        d, w = _route_det(getattr(d, "bh_packed", None) or _with_layout(d, packed_layout(d.precision))), wpacked
        if d.precision == F16X2:
            d.a_bound = amax_of(x).data_ptr()
    with _Timed(_conv_variant(d, "fwd", bn_groups=groups if bn_sums is not None else 0), conv_flops(d),
                4.0 * (x.numel() + y.numel() + w.numel())):
        if res is not None or relu:
            check(lib.bh_conv_fwd_act(_p(x), _p(w), _p(bias), _p(res), _p(y), ctypes.byref(d), int(bool(relu)), _stream()),
                  "bh_conv_fwd_act")
        elif amax is not None and bn_sums is None and wpacked is None:
            # (amax: zeroed magnitude record - the generic kernel measures max |y| in its epilogue; precision-4 consumers of y)
            check(lib.bh_conv_fwd_amax(_p(x), _p(w), _p(bias), _p(y), ctypes.byref(d), _p(amax), _stream()), "bh_conv_fwd_amax")
            y._bh_amax = amax
        elif bn_sums is None:
            check(lib.bh_conv_fwd(_p(x), _p(w), _p(bias), _p(y), ctypes.byref(d), _stream()), "bh_conv_fwd")
        else:
            _chk(bn_sums, torch.float64)
            check(lib.bh_conv_fwd_bnstats(_p(x), _p(w), _p(bias), _p(y), ctypes.byref(d), _p(bn_sums), groups, _stream()),
                  "bh_conv_fwd_bnstats")
    return y


_STEM_WT = {}          # (id(param), device, Ci) -> [version, table]: one table per stem parameter, NEVER freed or replaced - a
                       # captured HIP graph holds its address; a changed weight is written into the same storage
_STEM_WT_DIRTY = set()


def invalidate_stem_tables():
    """The weights may have changed behind the version counters (graph replay, broadcast): rebuild every table IN PLACE at its next use."""
    _STEM_WT_DIRTY.update(_STEM_WT.keys())


def _stem_dgrad_two_step(gy, w, d, wkey=None):
    """dgrad of the 1- or 3-input-channel 7x7/2 stem as (1x1 MFMA GEMM gy x w^T -> per-source-pixel tap table) + col2im.
    w is the kernel-layout weight [Co][7][7][Ci]; the result is NCHW [N,Ci,Hi,Wi] (== NHWC for Ci = 1).
    wkey: the SOURCE parameter and its version, (param, param._version) - `w` itself may be a per-forward temporary (the
    extractor's channel-summed stem weight) whose address and version repeat although the parameter changed; without a
    key the transposed table is rebuilt on every call (64 x 52 floats)."""
    cols = 49 * d.Ci
    ld = (cols + 3) // 4 * 4                                                          # 52 / 148
    import weakref
    key = None if wkey is None else (id(wkey[0]), str(w.device), d.Ci)
    ent = _STEM_WT.get(key) if key is not None else None
    if ent is not None and (ent[2]() is not wkey[0] or ent[1].shape != (ld, 1, 1, d.Co)):
        ent = None                                                                    # (the id of a dead parameter was reused)
    if ent is None:
        wt = torch.zeros(ld, 1, 1, d.Co, dtype=torch.float32, device=w.device)        # [tap*Ci + c, padded][Co]
        wt[:cols, 0, 0, :] = w.reshape(d.Co, cols).t()
        if key is not None:
            _STEM_WT[key] = [wkey[1], wt, weakref.ref(wkey[0])]
            _STEM_WT_DIRTY.discard(key)
    else:
        wt = ent[1]
        if ent[0] != wkey[1] or key in _STEM_WT_DIRTY:
            wt[:cols, 0, 0, :] = w.reshape(d.Co, cols).t()                            # same storage: graph-safe
            ent[0] = wkey[1]
            _STEM_WT_DIRTY.discard(key)
    d1 = conv_desc(d.N, d.Ho, d.Wo, d.Co, ld, 1, 1, 0, precision=d.precision)
    tm = conv_fwd(gy, wt, None, d1)                                                   # [N,Ho,Wo,ld]
    shape = (d.N, d.Hi, d.Wi, 1) if d.Ci == 1 else (d.N, d.Ci, d.Hi, d.Wi)
    gx = torch.empty(shape, dtype=torch.float32, device=gy.device)
    with _Timed("col2im_c1_kernel", 0.0, 4.0 * (tm.numel() + gx.numel())):
        check(lib.bh_col2im_c1(_p(tm), _p(gx), ctypes.byref(d), ld, _stream()), "bh_col2im_c1")
    return gx


def dgrad_bn_reduce_ok(d):
    """True when conv_dgrad(..., bn_reduce=...) is available for this conv (the halo-tiled 3x3 kernel takes its dgrad)."""
    return conv_variant(d, "dgrad").startswith(_C3_KERNELS)


def bias_grad_from_sums(sums, gbias, groups, C):
    """gbias[C] += column sums accumulated by conv_dgrad(..., colsum=sums)."""
    _chk(sums, torch.float64); _chk(gbias)
    check(lib.bh_bias_grad_from_sums(_p(sums), _p(gbias), groups, C, _stream()), "bh_bias_grad_from_sums")


def conv_dgrad(gy, w, d, out=None, bn_reduce=None, wkey=None, wpacked=None, colsum=None, warp_sink=None):
    """warp_sink (round 6; the extractor stem's dgrad on a one-channel image only): dict(src, H64, g_cov, pool, gH) - the image is the
    homography warp of `src`; where the fused kernel applies, the warp's adjoint is accumulated into gH, warp_sink["done"] is set and
    None is returned instead of the gradient image.
    colsum (only when dgrad_bn_reduce_ok(d), no `out`, no bn_reduce): zeroed bn_stats_buffer(1, Ci) - the per-channel sums
    of the gradient written are accumulated in the epilogue (bias gradient of the producer of this conv's input).
    wpacked: the dgrad buffer of WeightPacker for this conv.
    wkey: (param, param._version) of the parameter `w` was derived from (cache key of derived weight tables).
    bn_reduce (only when dgrad_bn_reduce_ok(d)): dict(z, y, stats, gamma, beta, eps, relu, sums, groups) of the
    BatchNorm whose output gradient this call completes - its backward sums are accumulated into `sums` (zeroed
    bn_stats_buffer) in the conv epilogue; pass them to bn_bwd(..., sums_ready=sums)."""
    _chk(gy); _chk(w)
    _mark(d)
    if wpacked is not None:
        d, w = _route_det(getattr(d, "bh_packed", None) or _with_layout(d, packed_layout(d.precision))), wpacked
        if d.precision == F16X2:
            d.a_bound = amax_of(gy).data_ptr()
    if colsum is not None:
        assert out is None and bn_reduce is None
        _chk(colsum, torch.float64)
        out = torch.empty((d.N, d.Hi, d.Wi, d.Ci), dtype=torch.float32, device=gy.device)
        with _Timed(_conv_variant(d, "dgrad_colsum"), conv_flops(d), 4.0 * (gy.numel() + out.numel() + w.numel())):
            check(lib.bh_conv_dgrad_colsum(_p(gy), _p(w), _p(out), ctypes.byref(d), _p(colsum), _stream()), "bh_conv_dgrad_colsum")
        return out
    if bn_reduce is not None:
        acc = out is not None
        if out is None:
            out = torch.empty((d.N, d.Hi, d.Wi, d.Ci), dtype=torch.float32, device=gy.device)
        b = bn_reduce
        _chk(b["z"]); _chk(b["y"]); _chk(b["stats"], torch.float64); _chk(b["sums"], torch.float64)
        st = BhBnReduce(_p(b["z"]), _p(b["y"]), _p(b["stats"]), _p(b["gamma"]), _p(b["beta"]), float(b["eps"]), int(bool(b["relu"])))
        with _Timed(_conv_variant(d, "dgrad_bnr_y" if b["y"] is not None else "dgrad_bnr_z", acc, int(b["groups"])), conv_flops(d),
                    4.0 * (gy.numel() + out.numel() * ((3 if acc else 2) + (1 if b["y"] is not None else 0)) + w.numel())):
            check(lib.bh_conv_dgrad_bnreduce(_p(gy), _p(w), _p(out), ctypes.byref(d), int(acc), ctypes.byref(st), _p(b["sums"]),
                                             int(b["groups"]), _stream()), "bh_conv_dgrad_bnreduce")
        if acc:
            out._bh_amax = None              # (a record left by an earlier producer no longer bounds the sum: as add_ does)
        return out
    if (out is None and not d.transposed and d.kh == 7 and d.stride == 2 and not d.out_nchw
            and (d.Ci == 1 or (d.Ci == 3 and d.in_nchw)) and d.Co % 4 == 0 and d.N * d.Ho * d.Wo >= 4096):
        if (d.Ci == 1 and d.Co == 64 and d.pad == 3 and d.Ho % 8 == 0 and d.Wo % 8 == 0 and d.Ho * 2 == d.Hi and d.Wo * 2 == d.Wi
                and w.is_contiguous() and os.environ.get("BIHOME_STEM_DGRAD_FUSED", "1") != "0"):
            # one kernel (round 4): a workgroup owns a 16 x 16 image tile - window GEMM into a tap table in LDS + gather; no tap table in HBM
            if warp_sink is not None and not deterministic() and os.environ.get("BIHOME_WARP_IN_STEM_DGRAD", "1") != "0":
                # round 6: the image is the homography warp of warp_sink["src"] and its gradient has one consumer, the warp's adjoint: the
                # kernel applies it to every pixel it has just summed (bh_stem7_dgrad_c1_warp) - no gradient image, no warp_bwd launch
                ws_ = warp_sink
                _chk(ws_["src"]); _chk(ws_["H64"], torch.float64); _chk(ws_["gH"], torch.float64); _chk(ws_["g_cov"])
                # (the name keeps the plain kernel's: rocprofv3 prints the template argument, bh_conv_variant-style)
                with _Timed("stem7_dgrad_c1_kernel<true>", conv_flops(d), 4.0 * (gy.numel() + ws_["src"].numel())):
                    check(lib.bh_stem7_dgrad_c1_warp(_p(gy), _p(w), None, ctypes.byref(d), _p(ws_["src"]), _p(ws_["H64"]), _p(ws_["g_cov"]),
                                                     int(ws_["pool"]), _p(ws_["gH"]), _stream()), "bh_stem7_dgrad_c1_warp")
                ws_["done"] = True
                return None
            gx = torch.empty((d.N, d.Hi, d.Wi, 1), dtype=torch.float32, device=gy.device)
            with _Timed("stem7_dgrad_c1_kernel", conv_flops(d), 4.0 * (gy.numel() + gx.numel())):
                check(lib.bh_stem7_dgrad_c1(_p(gy), _p(w), _p(gx), ctypes.byref(d), _stream()), "bh_stem7_dgrad_c1")
            return gx
        return _stem_dgrad_two_step(gy, w, d, wkey)
    acc = out is not None
    if (not d.transposed and d.stride == 2 and not d.in_nchw and not d.out_nchw and d.Co % 4 == 0 and d.Ci % 4 == 0
            and d.Hi % 2 == 0 and d.Wi % 2 == 0 and d.Ho * 2 == d.Hi and d.Wo * 2 == d.Wi
            and ((d.kh == 3 and d.kw == 3 and d.pad == 1) or (d.kh == 1 and d.kw == 1 and d.pad == 0))):
        # stride-2 dgrad by output parity class (csrc/conv_gemm.hip bh_conv_dgrad_s2)
        if out is None:
            out = torch.empty((d.N, d.Hi, d.Wi, d.Ci), dtype=torch.float32, device=gy.device)
        wpack = torch.empty(w.numel(), dtype=torch.float32, device=gy.device)
        nlaunch = 2 if d.kh == 3 else (2 + (0 if acc else 1))         # (weight pack + ONE launch for the parity classes: round 6)
        with _Timed("conv_dgrad_s2(%d kernels)" % nlaunch + (" N%d %dx%d C%d->%d k%d" % (d.N, d.Hi, d.Wi, d.Ci, d.Co, d.kh) if TIMING_DETAIL else ""),
                    conv_flops(d) / 4.0 * (1.0 if d.kh == 1 else 1.0), 4.0 * (gy.numel() + out.numel() * (2 if acc else 1) + 2 * w.numel())):
            check(lib.bh_conv_dgrad_s2(_p(gy), _p(w), _p(out), ctypes.byref(d), int(acc), _p(wpack), _stream()), "bh_conv_dgrad_s2")
        if acc:
            out._bh_amax = None
        return out
    if out is None:
        shape = (d.N, d.Ci, d.Hi, d.Wi) if d.in_nchw else (d.N, d.Hi, d.Wi, d.Ci)
        out = torch.empty(shape, dtype=torch.float32, device=gy.device)
    with _Timed(_conv_variant(d, "dgrad", acc), conv_flops(d), 4.0 * (gy.numel() + out.numel() * (2 if acc else 1) + w.numel())):
        check(lib.bh_conv_dgrad(_p(gy), _p(w), _p(out), ctypes.byref(d), int(acc), _stream()), "bh_conv_dgrad")
    if acc:
        out._bh_amax = None
    return out


def wgrad_det_bytes(d):
    """Workspace bytes of the deterministic weight-gradient form for this conv (0: not available for the shape)."""
    _route_det(d)
    if d.precision == 4 and not d.a_bound:
        # (a precision-4 launch is described WITH magnitude records - conv_wgrad attaches them -, and the fp16-piece forms size their
        #  workspace differently from what a description without them falls back to: ask with placeholders, as conv_variant does)
        d = _with_layout(d, d.w_layout)
        d.a_bound = d.b_bound = 256
    return int(lib.bh_conv_wgrad_det_bytes(ctypes.byref(d)))


_STEM_WGRAD_WS = {}      # (device, bytes, stream) -> the stem weight gradient's partial-sum workspace: launches of ONE stream serialise on it;
                         # another stream (a second model's side stream) gets its own.  Allocated by a step's first eager run - GraphedStep
                         # warms up eagerly before it captures, so the buffer is never born inside a graph's private pool


def conv_wgrad(x, gy, gw, gbias, d, det_ws=None):
    """gw += x^T gy (split-K MFMA kernel, fp32 atomics); gbias += column sums of gy (separate launch, own timing entry so
    that the wgrad entry is the kernel rocprofv3 lists under the same name).
    det_ws: float32 workspace of >= wgrad_det_bytes(d) bytes - the split-K partial tiles are stored there and added in a
    fixed order by a second launch (bitwise repeatable, no atomics); ignored where the shape has no deterministic form."""
    _route_det(d)
    if d.precision == F16X2 and getattr(d, "bh_wx3", True):
        # both records -> the fp16-piece kernel; (a description without them runs the exact three-piece form)
        d.a_bound, d.b_bound = amax_of(x).data_ptr(), amax_of(gy).data_ptr()
    if isinstance(x, BnOnLoad):
        bol, x = x, x.z
        _chk(x); _chk(gy); _chk(gw); _chk(gbias)
        if d.kh == 1:
            # round 4: 1x1 conv behind BatchNorm + ReLU - the small-channel kernel transforms x while staging (no workspace outside
            # deterministic calls)
            bs = bol.struct()
            ws_ = det_ws if deterministic() else None
            with _Timed((conv_variant(d, "wgrad") + " bnin") if TIMING is not None else "", conv_flops(d), 4.0 * (x.numel() + gy.numel() + gw.numel())):
                check(lib.bh_conv_wgrad_bnin(_p(x), _p(gy), _p(gw), _p(gbias), ctypes.byref(d), _p(ws_), ws_.numel() * 4 if ws_ is not None else 0,
                                             ctypes.byref(bs), _stream()), "bh_conv_wgrad_bnin(1x1)")
            return
        need = wgrad_det_bytes(d)
        if det_ws is None or not (0 < need <= det_ws.numel() * 4):
            raise RuntimeError("BatchNorm-on-load needs the f32x3 weight gradient and its workspace")
        bs = bol.struct()
        with _Timed((_bni_name(conv_variant(d, "wgrad_det")) if TIMING is not None else ""), conv_flops(d),
                    4.0 * (x.numel() + gy.numel() + gw.numel())):
            check(lib.bh_conv_wgrad_bnin(_p(x), _p(gy), _p(gw), _p(gbias), ctypes.byref(d), _p(det_ws), det_ws.numel() * 4,
                                         ctypes.byref(bs), _stream()), "bh_conv_wgrad_bnin")
        return
    _chk(x); _chk(gy); _chk(gw); _chk(gbias)
    if d.kh == 7 and d.stride == 2 and d.Ci == 2 and d.in_nchw and gbias is None and gw.is_contiguous():
        # the backbone's stem (round 4): dedicated kernel + ordered reduction through a private workspace (no atomics: every mode)
        need = lib.bh_stem7_wgrad_ws_bytes(ctypes.byref(d))
        if need:
            if torch.cuda.is_current_stream_capturing():
                # under a graph capture the workspace is born in THAT graph's private pool: it must not outlive the capture in a module-level
                # cache (a second graph capturing on the same stream handle would be handed a buffer the first graph's pool owns - round-5
                # ADVICE); stream order inside the capture keeps a freed block safe for later allocations of the same stream
                ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
            else:
                key = (str(x.device), int(need), int(torch.cuda.current_stream(x.device).cuda_stream))
                ws = _STEM_WGRAD_WS.get(key)
                if ws is None:
                    if len(_STEM_WGRAD_WS) >= 8:           # (streams come and go: the cache stays bounded)
                        _STEM_WGRAD_WS.clear()
                    ws = _STEM_WGRAD_WS[key] = torch.empty(need // 4, dtype=torch.float32, device=x.device)
            with _Timed("stem7_wgrad_kernel<2>+stem7_wgrad_reduce_kernel<2>", conv_flops(d), 4.0 * (x.numel() + gy.numel() + gw.numel())):
                check(lib.bh_stem7_wgrad(_p(x), _p(gy), _p(gw), ctypes.byref(d), _p(ws), need, _stream()), "bh_stem7_wgrad")
            return
    det = deterministic()
    if det and det_ws is None:
        raise RuntimeError("deterministic mode: conv_wgrad needs a workspace (det_ws) - bh_conv_wgrad has only the atomic form")
    if det_ws is not None:
        need = wgrad_det_bytes(d)
        if det and not (0 < need <= det_ws.numel() * 4):
            raise RuntimeError("deterministic mode: workspace of %d bytes, %d needed" % (det_ws.numel() * 4, need))
        if 0 < need <= det_ws.numel() * 4:
            with _Timed((conv_variant(d, "wgrad_det") if TIMING is not None else ""), conv_flops(d), 4.0 * (x.numel() + gy.numel() + gw.numel())):
                # (deterministic mode: the bias gradient rides in the same call - its limb entries are the tail of the workspace)
                check(lib.bh_conv_wgrad_det(_p(x), _p(gy), _p(gw), _p(gbias) if det else None, ctypes.byref(d), _p(det_ws),
                                            det_ws.numel() * 4, _stream()), "bh_conv_wgrad_det")
            if gbias is not None and not det:
                check(lib.bh_conv_bias_grad(_p(gy), _p(gbias), ctypes.byref(d), _stream()), "bh_conv_bias_grad")
            return
    with _Timed((conv_variant(d, "wgrad") if TIMING is not None else "") + (" N%d %dx%d C%d->%d k%d s%d%s" % (d.N, d.Hi, d.Wi, d.Ci, d.Co, d.kh, d.stride, " T" if d.transposed else "") if TIMING_DETAIL else ""), conv_flops(d), 4.0 * (x.numel() + gy.numel() + gw.numel())):
        check(lib.bh_conv_wgrad(_p(x), _p(gy), _p(gw), None, ctypes.byref(d), _stream()), "bh_conv_wgrad")
    if gbias is not None:
        with _Timed("bias_grad(colsum)", 0.0, 4.0 * gy.numel()):
            check(lib.bh_conv_bias_grad(_p(gy), _p(gbias), ctypes.byref(d), _stream()), "bh_conv_bias_grad")


BN_SUM_STRIDE = 16                                     # doubles between entries (one 128-byte line each; csrc/common.h)
BN_SUM_SLOTS = 1


def bn_stats_doubles(groups, C):
    return BN_SUM_SLOTS * groups * C * 2 * BN_SUM_STRIDE    # == lib.bh_bn_stats_doubles(groups, C)


def bn_stats_buffer(groups, C, device):
    """Zeroed [BN_SUM_SLOTS,groups,C,2,BN_SUM_STRIDE] float64 sums buffer (entry at [...,0], total = sum over slots; the
    kernels accumulate with f64 atomics)."""
    return torch.zeros(lib.bh_bn_stats_doubles(groups, C), dtype=torch.float64, device=device)


def bn_fwd(x, gamma, beta, rmean, rvar, res, groups, eps, momentum, relu, training, stats=None, stats_ready=False, amax=None):
    """x [groups*rows..., C] NHWC (any leading shape); returns (y, stats).  stats: optional zeroed sums buffer (a slice of
    the caller's arena); stats_ready: the producing conv already accumulated the sums (conv_fwd(..., bn_sums=stats))."""
    _chk(x); _chk(res)
    # channels: the affine parameter's length (a one-channel NCHW tensor [N,1,h,w] IS its NHWC form: the Zhang extractor's last layer)
    C = gamma.numel() if gamma is not None else x.shape[-1]
    rows = x.numel() // C // groups
    y = torch.empty_like(x)
    if stats is None:
        stats = bn_stats_buffer(groups, C, x.device)
        stats_ready = False
    flags = (1 if relu else 0) | (2 if res is not None else 0) | (8 if stats_ready else 0) | (BN_DETERMINISTIC if deterministic() else 0)
    nb = 4.0 * x.numel() * ((2 if (training and not stats_ready) else 1) + 1 + (1 if res is not None else 0))
    with _Timed("bn_fwd(%d kernels)" % (2 if (training and not stats_ready) else 1) + (" g%d rows%d C%d" % (groups, rows, C) if TIMING_DETAIL else ""), 0.0, nb):
        check(lib.bh_bn_fwd(_p(x), _p(gamma), _p(beta), _p(rmean), _p(rvar), _p(res), _p(y), _p(stats), groups, rows, C,
                            float(eps), float(momentum), flags, 0 if training else 1, _p(amax), _stream()), "bh_bn_fwd")
    if amax is not None:
        y._bh_amax = amax           # zeroed magnitude record, now max |y| (measured by the apply kernel)
    return y, stats


def bn_bwd(gy, y, x, gamma, stats, rmean, rvar, groups, eps, relu, training, want_gres, ggamma=None, gbeta=None, beta=None,
           had_res=None, scratch=None, sums_ready=None, amax=None):
    """sums_ready: the gradient sums buffer filled by conv_dgrad(..., bn_reduce=...) - reduce / finalize are skipped."""
    _chk(gy); _chk(x)
    C = gamma.numel() if gamma is not None else x.shape[-1]
    rows = x.numel() // C // groups
    gx = torch.empty_like(x)
    gres = torch.empty_like(x) if want_gres else None
    if sums_ready is not None:
        scratch = sums_ready
    elif scratch is None:
        scratch = torch.empty(lib.bh_bn_scratch_doubles(groups, C), dtype=torch.float64, device=x.device)
    had_res = want_gres if had_res is None else had_res
    mask_from_x = relu and not had_res          # y = relu(x*scale+shift): the mask is recomputed, y is not read
    flags = ((1 if relu else 0) | (2 if want_gres else 0) | (4 if mask_from_x else 0) | (16 if sums_ready is not None else 0)
             | (BN_DETERMINISTIC if deterministic() else 0))
    passes = 1 if sums_ready is not None else 2
    nb = 4.0 * x.numel() * (passes * (2 + (1 if (relu and not mask_from_x) else 0)) + 1 + (1 if want_gres else 0))
    with _Timed("bn_bwd(%d kernels)" % (1 if sums_ready is not None else 3) + (" g%d rows%d C%d" % (groups, rows, C) if TIMING_DETAIL else ""), 0.0, nb):
        check(lib.bh_bn_bwd(_p(gy), _p(y), _p(x), _p(gamma), _p(beta), _p(stats), _p(gx), _p(gres), _p(ggamma), _p(gbeta),
                            _p(scratch), groups, rows, C, float(eps), flags, 0 if training else 1, _p(rmean), _p(rvar),
                            _p(amax), _stream()), "bh_bn_bwd")
    if amax is not None:
        gx._bh_amax = amax          # zeroed magnitude record, now max |gx|
    return gx, gres


def bn_stats(x, stats, groups, C):
    """stats (zeroed slice of the caller's arena) += per-channel (sum, sum of squares) of x: the statistics pass alone."""
    _chk(x); _chk(stats, torch.float64)
    rows = x.numel() // C // groups
    with _Timed("bn_stats_kernel", 0.0, 4.0 * x.numel()):
        check(lib.bh_bn_stats(_p(x), _p(stats), groups, rows, C, BN_DETERMINISTIC if deterministic() else 0, _stream()), "bh_bn_stats")
    return stats


class BnPooled:
    """A BatchNorm(+ReLU) whose only consumer is MaxPool2d(3, 2, 1), both done by bn_maxpool_fwd: the BatchNorm's output does not exist;
    `pooled` / `idx` are what the pooling op returns, `shape` the shape the BatchNorm output would have had (for the adjoint)."""
    __slots__ = ("pooled", "idx", "shape")

    def __init__(self, pooled, idx, shape):
        self.pooled, self.idx, self.shape = pooled, idx, tuple(shape)


def bn_maxpool_fwd(x, gamma, beta, rmean, rvar, groups, eps, momentum, relu, training, stats, stats_ready, want_index=True, amax=None):
    """x NHWC -> BnPooled(maxpool3s2(act(bn(x))), idx, x.shape) in one pass; stats as in bn_fwd."""
    _chk(x)
    N, Hi, Wi, C = x.shape
    y = torch.empty((N, (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1, C), dtype=torch.float32, device=x.device)
    idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device) if want_index else None
    flags = (1 if relu else 0) | (8 if stats_ready else 0) | (BN_DETERMINISTIC if deterministic() else 0)
    with _Timed("bn_maxpool_fwd" + (" N%d %dx%d C%d" % (N, Hi, Wi, C) if TIMING_DETAIL else ""), 0.0, 4.0 * (x.numel() + y.numel()) + y.numel()):
        check(lib.bh_bn_maxpool_fwd(_p(x), _p(gamma), _p(beta), _p(rmean), _p(rvar), _p(y), _p(idx), _p(stats), groups, N, Hi, Wi, C,
                                    float(eps), float(momentum), flags, 0 if training else 1, _p(amax), _stream()), "bh_bn_maxpool_fwd")
    if amax is not None:
        y._bh_amax = amax
    return BnPooled(y, idx, x.shape)


class BnJoinPending:
    """The lower-branch BatchNorm of a residual unit whose apply rides in the join (bn_join_fwd): `x` is its INPUT, `stats` its sums."""
    __slots__ = ("x", "stats", "mod")

    def __init__(self, x, stats, mod):
        self.x, self.stats, self.mod = x, stats, mod

    @property
    def shape(self):
        return self.x.shape


def bn_join_fwd(xa, xb, ma, mb, stats_a, stats_b, groups, relu, mom_a, mom_b, amax=None):
    """y = act(bn_a(xa) + bn_b(xb)) (training mode, both statistics tables already accumulated); ma / mb: the BatchNorm2d modules."""
    _chk(xa); _chk(xb); _chk(stats_a, torch.float64); _chk(stats_b, torch.float64)
    C = ma.num_features
    rows = xa.numel() // C // groups
    y = torch.empty_like(xa)
    flags = (1 if relu else 0) | (BN_DETERMINISTIC if deterministic() else 0)
    with _Timed("bn_join_fwd" + (" g%d rows%d C%d" % (groups, rows, C) if TIMING_DETAIL else ""), 0.0, 12.0 * xa.numel()):
        check(lib.bh_bn_join_fwd(_p(xa), _p(xb), _p(ma.weight), _p(ma.bias), _p(ma.running_mean), _p(ma.running_var), _p(mb.weight), _p(mb.bias),
                                 _p(mb.running_mean), _p(mb.running_var), _p(stats_a), _p(stats_b), _p(y), groups, rows, C, float(ma.eps),
                                 float(mb.eps), float(mom_a), float(mom_b), flags, _p(amax), _stream()), "bh_bn_join_fwd")
    if amax is not None:
        y._bh_amax = amax
    return y


def bn_join_bwd(gy, y, xa, xb, ma, mb, stats_a, stats_b, groups, relu, train_a, train_b, amax_a=None, amax_b=None):
    """-> (gxa, gxb); the affine parameters' gradients are added to .grad when train_a / train_b."""
    _chk(gy); _chk(xa); _chk(xb)
    C = ma.num_features
    rows = xa.numel() // C // groups
    gxa, gxb = torch.empty_like(xa), torch.empty_like(xb)
    scratch = torch.empty(lib.bh_bn_join_scratch_doubles(groups, C), dtype=torch.float64, device=xa.device)
    flags = (1 if relu else 0) | (BN_DETERMINISTIC if deterministic() else 0)
    # (round 5: the ReLU mask is recomputed from xa, xb - `y` is not read; BIHOME_JOIN_REMASK=0: the form that reads it)
    if os.environ.get("BIHOME_JOIN_REMASK", "1") != "0":
        with _Timed("bn_join_bwd(3 kernels)" + (" g%d rows%d C%d" % (groups, rows, C) if TIMING_DETAIL else ""), 0.0, 32.0 * xa.numel()):
            check(lib.bh_bn_join_bwd_remask(_p(gy), _p(xa), _p(xb), _p(ma.weight), _p(ma.bias), _p(mb.weight), _p(mb.bias), _p(stats_a),
                                            _p(stats_b), _p(gxa), _p(gxb),
                                            _p(ma.weight.grad) if train_a else None, _p(ma.bias.grad) if train_a else None,
                                            _p(mb.weight.grad) if train_b else None, _p(mb.bias.grad) if train_b else None, _p(scratch), groups,
                                            rows, C, float(ma.eps), float(mb.eps), flags, _p(amax_a), _p(amax_b), _stream()),
                  "bh_bn_join_bwd_remask")
    else:
      with _Timed("bn_join_bwd(3 kernels)" + (" g%d rows%d C%d" % (groups, rows, C) if TIMING_DETAIL else ""), 0.0, 40.0 * xa.numel()):
        check(lib.bh_bn_join_bwd(_p(gy), _p(y), _p(xa), _p(xb), _p(ma.weight), _p(mb.weight), _p(stats_a), _p(stats_b), _p(gxa), _p(gxb),
                                 _p(ma.weight.grad) if train_a else None, _p(ma.bias.grad) if train_a else None,
                                 _p(mb.weight.grad) if train_b else None, _p(mb.bias.grad) if train_b else None, _p(scratch), groups, rows, C,
                                 float(ma.eps), float(mb.eps), flags, _p(amax_a), _p(amax_b), _stream()), "bh_bn_join_bwd")
    if amax_a is not None:
        gxa._bh_amax = amax_a
    if amax_b is not None:
        gxb._bh_amax = amax_b
    return gxa, gxb


TAIL_ROUTE_VALU_FWD = 1     # include/bihome.h BH_TAIL_ROUTE_VALU_FWD
TAIL_ROUTE_LDS_MOMENTS = 2  # include/bihome.h BH_TAIL_ROUTE_LDS_MOMENTS


def tail_fwd(x, w1, b1, gamma, beta, rmean, rvar, w2, b2, groups, hw, eps, momentum, training, route=0):
    """x NHWC [N,h,w,Ci] -> out NCHW [N,Co,h,w] through conv1x1+BN+ReLU+conv1x1 (fused); returns (out, ws).
    route: per-call bits of bh_tail_fwd (TAIL_ROUTE_VALU_FWD keeps the per-pixel VALU kernel)."""
    _chk(x)
    N, h, w, Ci = x.shape
    Cm, Co = w1.shape[0], w2.shape[0]
    rows = N * h * w // groups
    out = torch.empty((N, Co, h, w), dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.bh_tail_ws_doubles(groups, Ci, Cm), dtype=torch.float64, device=x.device)
    fl = 2.0 * N * h * w * Cm * (Ci + Co)
    with _Timed("tail_fwd(4 kernels)", fl, 4.0 * (x.numel() * (2 if training else 1) + out.numel())):
        check(lib.bh_tail_fwd(_p(x), _p(w1), _p(b1), _p(gamma), _p(beta), _p(rmean), _p(rvar), _p(w2), _p(b2), _p(out),
                              _p(ws), groups, rows, hw, Ci, Cm, Co, float(eps), float(momentum), 0 if training else 1,
                              int(route), _stream()), "bh_tail_fwd")
    return out, ws


def tail_bwd(gout, x, w1, b1, gamma, beta, w2, ws, rmean, rvar, groups, hw, eps, training, want_gx, gw1, ggamma, gbeta,
             gw2, gb2):
    _chk(gout); _chk(x)
    N, h, w, Ci = x.shape
    Cm, Co = w1.shape[0], w2.shape[0]
    rows = N * h * w // groups
    gx = torch.empty_like(x) if want_gx else None
    scratch = torch.empty(lib.bh_tail_scratch_floats(groups, Ci, Cm), dtype=torch.float32, device=x.device)
    fl = 2.0 * N * h * w * Cm * (3 * Ci + 2 * Co + Ci)
    with _Timed("tail_bwd(5 kernels)", fl, 4.0 * (x.numel() * 3 + gout.numel() * 3)):
        check(lib.bh_tail_bwd(_p(gout), _p(x), _p(w1), _p(b1), _p(gamma), _p(beta), _p(w2), _p(ws), _p(rmean), _p(rvar),
                              _p(gx), _p(gw1), _p(ggamma), _p(gbeta), _p(gw2), _p(gb2), _p(scratch), groups, rows, hw, Ci,
                              Cm, Co, float(eps), 0 if training else 1, _fdet(), _stream()), "bh_tail_bwd")
    return gx


def maxpool_fwd(x, want_index=True):
    _chk(x)
    N, Hi, Wi, C = x.shape
    y = torch.empty((N, (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1, C), dtype=torch.float32, device=x.device)
    idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device) if want_index else None
    check(lib.bh_maxpool3s2_fwd(_p(x), _p(y), _p(idx), N, Hi, Wi, C, _stream()), "bh_maxpool3s2_fwd")
    rec = getattr(x, "_bh_amax", None)
    if rec is not None:
        y._bh_amax = rec            # a window maximum is bounded by the bound of its input
    return y, idx


class GradFrom1x1:
    """Gradient of a BatchNorm output that IS the dgrad of a 1x1 conv with few output channels: the conv's output gradient and its weight,
    handed to the BatchNorm's adjoint (bn_bwd_from_1x1) - the dgrad's result is never formed."""
    __slots__ = ("gs", "w")

    def __init__(self, gs, w):
        self.gs, self.w = gs, w


def bn_bwd_from_1x1(gf, x, gamma, beta, stats, groups, eps, relu, ggamma=None, gbeta=None, amax=None):
    """Adjoint of a training-mode BatchNorm (+ReLU, no residual) whose output feeds only a 1x1 conv: GradFrom1x1 + the BatchNorm input ->
    gx (bh_bn_bwd_from_1x1: conv_dgrad + bn_bwd without the tensor in between)."""
    gs, w = gf.gs, gf.w
    _chk(gs); _chk(w); _chk(x)
    C = x.shape[-1]
    KC = gs.shape[-1]
    rows = x.numel() // C // groups
    gx = torch.empty_like(x)
    scratch = torch.empty(lib.bh_bn_scratch_doubles(groups, C), dtype=torch.float64, device=x.device)
    flags = (1 if relu else 0) | (BN_DETERMINISTIC if deterministic() else 0)
    with _Timed("bn_bwd_from_1x1(3 kernels)" + (" g%d rows%d C%d<-%d" % (groups, rows, C, KC) if TIMING_DETAIL else ""), 4.0 * gs.numel() * C,
                4.0 * (3 * x.numel() + 2 * gs.numel())):
        check(lib.bh_bn_bwd_from_1x1(_p(gs), _p(w), KC, _p(x), _p(gamma), _p(beta), _p(stats), _p(gx), _p(ggamma), _p(gbeta), _p(scratch), groups,
                                     rows, C, float(eps), flags, _p(amax), _stream()), "bh_bn_bwd_from_1x1")
    if amax is not None:
        gx._bh_amax = amax
    return gx


class PooledGrad:
    """Gradient of a BnPooled slot: the pooled gradient and the arg-max positions, handed from the pooling op's adjoint to the BatchNorm's
    (bn_maxpool_bwd) - the full-resolution gradient in between is never formed."""
    __slots__ = ("gy", "idx")

    def __init__(self, gy, idx):
        self.gy, self.idx = gy, idx


def bn_maxpool_bwd(pg, x, gamma, beta, stats, rmean, rvar, groups, eps, relu, training, ggamma=None, gbeta=None, amax=None):
    """Adjoint of bn_maxpool_fwd: PooledGrad + the BatchNorm input -> gx (bh_bn_maxpool_bwd; bitwise what maxpool_bwd + bn_bwd give)."""
    gy, idx = pg.gy, pg.idx
    _chk(gy); _chk(idx, torch.uint8); _chk(x)
    N, Hi, Wi, C = x.shape
    gx = torch.empty_like(x)
    scratch = torch.empty(lib.bh_bn_scratch_doubles(groups, C), dtype=torch.float64, device=x.device)
    flags = (1 if relu else 0) | (BN_DETERMINISTIC if deterministic() else 0)
    with _Timed("bn_maxpool_bwd(3 kernels)" + (" g%d N%d %dx%d C%d" % (groups, N, Hi, Wi, C) if TIMING_DETAIL else ""), 0.0,
                4.0 * (3 * x.numel() + 2 * gy.numel()) + 2.0 * idx.numel()):
        check(lib.bh_bn_maxpool_bwd(_p(gy), _p(idx), _p(x), _p(gamma), _p(beta), _p(stats), _p(gx), _p(ggamma), _p(gbeta), _p(scratch), groups,
                                    N, Hi, Wi, C, float(eps), flags, 0 if training else 1, _p(rmean), _p(rvar), _p(amax), _stream()),
              "bh_bn_maxpool_bwd")
    if amax is not None:
        gx._bh_amax = amax
    return gx


def maxpool_bwd(idx, gy, in_shape):
    _chk(idx, torch.uint8); _chk(gy)
    N, Hi, Wi, C = in_shape
    gx = torch.empty(in_shape, dtype=torch.float32, device=gy.device)
    check(lib.bh_maxpool3s2_bwd(_p(idx), _p(gy), _p(gx), N, Hi, Wi, C, _stream()), "bh_maxpool3s2_bwd")
    return gx


def gap_fwd(x):
    _chk(x)
    N, H, W, C = x.shape
    y = torch.empty((N, 1, 1, C), dtype=torch.float32, device=x.device)
    check(lib.bh_gap_fwd(_p(x), _p(y), N, H * W, C, _stream()), "bh_gap_fwd")
    return y


def gap_bwd(gy, shape):
    _chk(gy)
    N, H, W, C = shape
    gx = torch.empty(shape, dtype=torch.float32, device=gy.device)
    check(lib.bh_gap_bwd(_p(gy), _p(gx), N, H * W, C, _stream()), "bh_gap_bwd")
    return gx


def add_(a, b):
    """a += b (same shape, contiguous)."""
    _chk(a); _chk(b)
    check(lib.bh_add(_p(a), _p(b), _p(a), a.numel(), _stream()), "bh_add")
    if getattr(a, "_bh_amax", None) is not None:
        a._bh_amax = None           # the magnitude record described the old contents
    return a


# ------------------------------------------------------------------------------------------------
# pair generator: occlusion blobs
# ------------------------------------------------------------------------------------------------
def synth_blobs_scratch_floats(B, P):
    return int(lib.bh_synth_blobs_scratch_floats(int(B), int(P)))


def synth_blobs(noise, other, patch1, patch2, mask, sigma, porosity, field=None, scratch=None):
    """CollatorWithBlobs on the device (include/bihome.h bh_synth_blobs): noise [B,P,P] in [0,1), other [B] int32, patch1 / patch2
    [B,C,P,P]; patch2 is composited IN PLACE (patch1[other[b]] where the blob field of noise[b] lies below `porosity`).
    Outputs are the caller's: mask [B,P,P] (1.0 / 0.0), field [B,P,P] or None, scratch of synth_blobs_scratch_floats(B, P) floats
    (None where that is 0); bihome_amd.synth_gpu.apply_blobs allocates them."""
    _chk(noise); _chk(other, torch.int32); _chk(patch1); _chk(patch2); _chk(mask); _chk(field); _chk(scratch)
    if noise.dim() != 3 or patch1.dim() != 4 or patch1.shape != patch2.shape or noise.shape[1] != noise.shape[2] or \
            tuple(noise.shape) != (patch1.shape[0],) + tuple(patch1.shape[2:]) or other.shape != (noise.shape[0],) or \
            mask.shape != noise.shape or (field is not None and field.shape != noise.shape):
        raise ValueError("synth_blobs: noise, mask and field [B,P,P], other [B], patch1 and patch2 [B,C,P,P]")
    B, C, P = patch1.shape[0], patch1.shape[1], patch1.shape[2]
    if (scratch.numel() if scratch is not None else 0) < synth_blobs_scratch_floats(B, P):
        raise ValueError("synth_blobs: scratch needs synth_blobs_scratch_floats(B, P) = %d floats" % synth_blobs_scratch_floats(B, P))
    check(lib.bh_synth_blobs(_p(noise), _p(other), _p(patch1), _p(patch2), _p(mask), _p(field), _p(scratch), B, C, P, float(sigma),
                             float(porosity), _stream()), "bh_synth_blobs")
    return mask, field


def synth_draw(seed, first, n_images, h, w, patch, rho, max_delta, img_idx, origin, delta, photo=None, noise=None, other=None):
    """Counter-based draws (include/bihome.h bh_synth_draw): the parameters of samples first .. first + B - 1 of the stream of `seed`,
    one launch (two with blob noise).  Outputs are the caller's: img_idx [B] int32, origin [B,2], delta [B,4,2]; photo [B,2,6] (or
    [B,12]) or None; noise [B,P,P] and other [B] int32, both or neither.  seed and first are taken modulo 2^64."""
    _chk(img_idx, torch.int32); _chk(origin); _chk(delta); _chk(photo); _chk(noise); _chk(other, torch.int32)
    B = img_idx.shape[0]
    if img_idx.dim() != 1 or tuple(origin.shape) != (B, 2) or tuple(delta.shape) != (B, 4, 2) or \
            (photo is not None and photo.numel() != 12 * B) or (noise is not None and tuple(noise.shape) != (B, patch, patch)) or \
            (other is not None and tuple(other.shape) != (B,)):
        raise ValueError("synth_draw: img_idx [B] int32, origin [B,2], delta [B,4,2], photo [B,2,6], noise [B,P,P], other [B] int32")
    if (noise is None) != (other is None):
        raise ValueError("synth_draw: noise and other are given together (or neither)")
    m64 = (1 << 64) - 1
    check(lib.bh_synth_draw(int(seed) & m64, int(first) & m64, B, int(n_images), int(h), int(w), int(patch), int(rho), float(max_delta),
                            _p(img_idx), _p(origin), _p(delta), _p(photo), _p(noise), _p(other), _stream()), "bh_synth_draw")
    return img_idx, origin, delta, photo, noise, other


# ------------------------------------------------------------------------------------------------
# pair generator: resident uint8 image bank
# ------------------------------------------------------------------------------------------------
def bank_gather_u8(bank, idx, out):
    """Images idx [count] (int32) of a uint8 bank [N,H,W,3] as the float planes out [count,3,H,W], values 0..255 (include/bihome.h
    bh_bank_gather_u8; an index outside [0, N) is clamped by the kernel).  `out` is the caller's: bihome_amd.bank.ImageBank.gather
    allocates or reuses it."""
    _chk(bank, torch.uint8); _chk(idx, torch.int32); _chk(out)
    if bank.dim() != 4 or bank.shape[3] != 3 or idx.dim() != 1 or tuple(out.shape) != (idx.shape[0], 3, bank.shape[1], bank.shape[2]):
        raise ValueError("bank_gather_u8: bank [N,H,W,3] uint8, idx [count] int32, out [count,3,H,W] float32")
    check(lib.bh_bank_gather_u8(_p(bank), _p(idx), idx.shape[0], bank.shape[0], bank.shape[1], bank.shape[2], _p(out), _stream()),
          "bh_bank_gather_u8")
    return out


def bank_ingest_u8(src, src_off, src_hw, bank, first=0):
    """Rescale + CenterCrop of n raw-size images into slots first .. first+n-1 of a uint8 bank [N,H,W,3], one launch (include/bihome.h
    bh_bank_ingest_u8).  src: uint8 [bytes] on the device, the images packed as interleaved RGB; src_off [n] int64: the byte offset of
    each; src_hw [n,2] int32: its height and width.  src_off / src_hw on the HOST (numpy arrays or CPU tensors) are checked here - h, w
    >= 1, every image inside src, a resized size that fits an int: ValueError - and then uploaded.  Device tensors are taken as they are
    (nothing is copied: a captured launch), and what the kernel does with a bad entry is the header's: h < 1 or w < 1 leaves the slot
    untouched, an offset outside src is read."""
    _chk(src, torch.uint8); _chk(bank, torch.uint8)
    off, hw = torch.as_tensor(src_off), torch.as_tensor(src_hw)
    if src.dim() != 1 or bank.dim() != 4 or bank.shape[3] != 3 or off.dim() != 1 or tuple(hw.shape) != (off.shape[0], 2) or \
            off.dtype != torch.int64 or hw.dtype != torch.int32 or off.is_cuda != hw.is_cuda:
        raise ValueError("bank_ingest_u8: src [bytes] uint8, src_off [n] int64, src_hw [n,2] int32 (both on the host or both on the "
                         "device), bank [N,H,W,3] uint8")
    n, (N, H, W) = off.shape[0], bank.shape[:3]
    if first < 0 or first + n > N:
        raise ValueError("bank_ingest_u8: slots %d .. %d of a bank of %d" % (first, first + n - 1, N))
    if n == 0:
        return bank
    if not off.is_cuda:
        for k, (o, (h, w)) in enumerate(zip(off.tolist(), hw.tolist())):
            if h < 1 or w < 1:
                raise ValueError("bank_ingest_u8: image %d is %d x %d, an image has at least one pixel" % (k, h, w))
            if o < 0 or o + h * w * 3 > src.numel():
                raise ValueError("bank_ingest_u8: image %d (%d x %d at byte %d) does not lie inside src (%d bytes)" % (k, h, w, o, src.numel()))
            if H * w >= h << 31 or W * h >= w << 31:
                raise ValueError("bank_ingest_u8: image %d (%d x %d) rescaled to %d x %d does not fit an int" % (k, h, w, H, W))
        off, hw = off.contiguous().to(bank.device), hw.contiguous().to(bank.device)
    _chk(off, torch.int64); _chk(hw, torch.int32)
    check(lib.bh_bank_ingest_u8(_p(src), _p(off), _p(hw), n, _p(bank), N, first, H, W, _stream()), "bh_bank_ingest_u8")
    return bank


# ------------------------------------------------------------------------------------------------
# image alignment: uint8 images -> standardised patches, and the uint8 warp (bihome_amd/align.py)
# ------------------------------------------------------------------------------------------------
def _is_h(M):
    """M is [B,3,3] or [B,9]: the shape of a batch of homographies (the dtype is _chk's)."""
    return M.dim() >= 2 and M.numel() == 9 * M.shape[0]


def _chk_images_u8(images, idx, idx_shape, what):
    """A uint8 bank and its index list idx (None: the images in order) of shape idx_shape: (B,), or (B, n) for sequences."""
    _chk(images, torch.uint8); _chk(idx, torch.int32)
    if images.dim() != 4 or images.shape[3] != 3 or min(images.shape) < 1:
        raise ValueError("%s: images [N,H,W,3] uint8 with N, H, W >= 1, got %s" % (what, tuple(images.shape)))
    if idx is not None and tuple(idx.shape) != tuple(idx_shape):
        names = "Bn"[:len(idx_shape)]
        raise ValueError("%s: idx [%s] int32, got %s for %s" % (what, ",".join(names), tuple(idx.shape), ", ".join("%s = %d" % p for p in zip(names, idx_shape))))


def _chk_u8(out, planes):
    """An output image and its flag planes are uint8 device tensors."""
    for t in [out] + [plane for _, plane in planes]:
        _chk(t, torch.uint8)


def _chk_canvas_u8(out, planes, B, what, hw):
    """The shapes of an output image out [B,H,W,3] and its uint8 flag planes [B,H,W]: planes = [(name, plane or None), ...]; hw = "H,W" as
    the message spells them.  Device and dtype are `_chk_u8`'s, which the callers run before any shape check."""
    for name, plane in planes or [("the flag plane", None)]:
        if out.dim() != 4 or out.shape[0] != B or out.shape[3] != 3 or (plane is not None and tuple(plane.shape) != tuple(out.shape[:3])):
            raise ValueError("%s: out [B,%s,3] uint8 and %s [B,%s] uint8 with B = %d, got %s and %s"
                             % (what, hw, name, hw, B, tuple(out.shape), None if plane is None else tuple(plane.shape)))


def _mode_number(mode, modes, what):
    """A blend mode by name, or already its number in include/bihome.h."""
    if isinstance(mode, str):
        if mode not in modes:
            raise ValueError("%s: mode is one of %s, got %r" % (what, sorted(modes), mode))
        mode = modes[mode]
    return int(mode)


def align_prep_u8(images, patch, geom, mean, std, idx=None, roi=None):
    """B samples of a uint8 bank [N,H,W,3] as the standardised patches patch [B,C,P,P] float32 by exact area averaging, and their
    geometry records geom [B,4] float64 (sx, sy, tx, ty) (include/bihome.h bh_align_prep_u8).  Both outputs are the caller's
    (bihome_amd.align.prepare allocates them).  idx [B] int32: each sample's image (None: sample b is image b; clamped by the kernel);
    roi [B,4] float64 DEVICE tensor (x0, y0, rw, rh) in edge coordinates (None: whole images) - the kernel clamps what it derives from
    it, range checks belong to the caller (bihome_amd.align.Aligner)."""
    _chk(patch); _chk(geom, torch.float64); _chk(roi, torch.float64)
    if patch.dim() != 4 or patch.shape[2] != patch.shape[3] or tuple(geom.shape) != (patch.shape[0], 4):
        raise ValueError("align_prep_u8: patch [B,C,P,P] float32 and geom [B,4] float64, got %s and %s" % (tuple(patch.shape), tuple(geom.shape)))
    B, C, P = patch.shape[:3]
    _chk_images_u8(images, idx, (B,), "align_prep_u8")
    if roi is not None and tuple(roi.shape) != (B, 4):
        raise ValueError("align_prep_u8: roi [B,4] float64, got %s" % (tuple(roi.shape),))
    check(lib.bh_align_prep_u8(_p(images), _p(idx), images.shape[0], images.shape[1], images.shape[2], _p(roi), B, P, C,
                               float(mean), float(std), _p(patch), _p(geom), _stream()), "bh_align_prep_u8")
    return patch, geom


def warp_u8(images, H64, out, valid=None, idx=None):
    """out [B,Ho,Wo,3] uint8 = round_half_up(bilinear images[idx[b]](H64[b] (x, y, 1))) with zero padding, and valid [B,Ho,Wo] uint8
    (may be None) (include/bihome.h bh_warp_u8).  Both outputs are the caller's (bihome_amd.align.warp_u8 allocates them).  H64 [B,3,3]
    or [B,9] float64: output index coordinates -> source index coordinates."""
    _chk(H64, torch.float64); _chk_u8(out, [("valid", valid)])
    if not _is_h(H64):
        raise ValueError("warp_u8: H64 [B,3,3] float64, got %s" % (tuple(H64.shape),))
    B = H64.shape[0]
    _chk_canvas_u8(out, [("valid", valid)], B, "warp_u8", "Ho,Wo")
    _chk_images_u8(images, idx, (B,), "warp_u8")
    check(lib.bh_warp_u8(_p(images), _p(idx), images.shape[0], images.shape[1], images.shape[2], _p(H64), B, out.shape[1], out.shape[2],
                         _p(out), _p(valid), _stream()), "bh_warp_u8")
    return out, valid


# ------------------------------------------------------------------------------------------------
# ECC refinement of the lifted homography (bihome_amd/align.py; csrc/ecc.hip).  Every buffer is the caller's.
# ------------------------------------------------------------------------------------------------
def _size_query(fn, name, *args):
    out = ctypes.c_int64(0)
    check(fn(*args, ctypes.byref(out)), name)
    return int(out.value)


def gray_pyramid_layout(H, W, levels):
    """offsets [levels + 1] (floats) of the levels inside a sample's packed pyramid row; the last is the row's length (host only)."""
    off = (ctypes.c_int64 * 8)()                         # (at most 6 levels; a refused call writes nothing)
    check(lib.bh_gray_pyramid_layout(int(H), int(W), int(levels), off), "bh_gray_pyramid_layout")
    return [int(v) for v in off[:levels + 1]]


def ecc_sums_ws_doubles(Hb, Wb, B):
    return _size_query(lib.bh_ecc_sums_ws_doubles, "bh_ecc_sums_ws_doubles", int(Hb), int(Wb), int(B))


def ecc_refine_ws_doubles(Hb, Wb, B):
    return _size_query(lib.bh_ecc_refine_ws_doubles, "bh_ecc_refine_ws_doubles", int(Hb), int(Wb), int(B))


def gray_pyramid_u8(images, pyr, levels, idx=None):
    """pyr [B,total] float32 = the gray box pyramids of B samples of the uint8 bank images [N,H,W,3], levels packed one after another
    (include/bihome.h bh_gray_pyramid_u8; total = gray_pyramid_layout(H, W, levels)[-1]).  pyr is the caller's."""
    _chk(pyr)
    if pyr.dim() != 2:
        raise ValueError("gray_pyramid_u8: pyr [B,total] float32, got %s" % (tuple(pyr.shape),))
    B = pyr.shape[0]
    _chk_images_u8(images, idx, (B,), "gray_pyramid_u8")
    total = gray_pyramid_layout(images.shape[1], images.shape[2], levels)[-1]
    if pyr.shape[1] != total:
        raise ValueError("gray_pyramid_u8: %d levels of %d x %d take %d floats per sample, pyr has %d" % (levels, images.shape[1], images.shape[2], total, pyr.shape[1]))
    check(lib.bh_gray_pyramid_u8(_p(images), _p(idx), images.shape[0], images.shape[1], images.shape[2], B, int(levels), _p(pyr), _stream()),
          "bh_gray_pyramid_u8")
    return pyr


def ecc_sums(a, t, H64, partial, sums, mask=None):
    """One ECC pass at one level (include/bihome.h bh_ecc_sums): a [B,Ha,Wa], t [B,Hb,Wb] float32 gray planes (views of pyramid rows are
    fine: the last two dimensions dense), H64 [B,3,3] float64, mask [B,Hb,Wb] uint8 or None -> sums [B,66] float64.  partial (float64,
    ecc_sums_ws_doubles(Hb, Wb, B) elements) and sums are the caller's."""
    _chk(H64, torch.float64); _chk(partial, torch.float64); _chk(sums, torch.float64); _chk(mask, torch.uint8)
    for x in (a, t):                                     # (views: device and dtype here, the layout below)
        if not x.is_cuda:
            raise RuntimeError("bihome_amd kernels need device tensors (got %s); there is no CPU path" % x.device)
        if x.dtype != torch.float32:
            raise TypeError("expected %s, got %s" % (torch.float32, x.dtype))
    B = H64.shape[0]
    for x, what in ((a, "a"), (t, "t")):
        if x.dim() != 3 or x.shape[0] != B or x.stride(2) != 1 or x.stride(1) != x.shape[2] or (B > 1 and x.stride(0) < x.shape[1] * x.shape[2]):
            raise ValueError("ecc_sums: %s [B,H,W] float32 with dense planes and B = %d, got %s strides %s" % (what, B, tuple(x.shape), x.stride()))
    if H64.numel() != 9 * B or tuple(sums.shape) != (B, ECC_SUMS) or (mask is not None and tuple(mask.shape) != tuple(t.shape)):
        raise ValueError("ecc_sums: H64 [B,3,3], sums [B,66], mask [B,Hb,Wb]")
    (Ha, Wa), (Hb, Wb) = a.shape[1:], t.shape[1:]
    if partial.numel() < ecc_sums_ws_doubles(Hb, Wb, B):
        raise ValueError("ecc_sums: partial has %d doubles, %d are needed" % (partial.numel(), ecc_sums_ws_doubles(Hb, Wb, B)))
    sa, st = (a.stride(0), t.stride(0)) if B > 1 else (Ha * Wa, Hb * Wb)
    check(lib.bh_ecc_sums(a.data_ptr(), Ha, Wa, sa, t.data_ptr(), Hb, Wb, st, _p(mask), _p(H64), B, _p(partial), _p(sums), _stream()), "bh_ecc_sums")
    return sums


def ecc_step(sums, state, last=0, stats=None):
    """One ECC step and the books of its level on state [B,24] float64, in place (include/bihome.h bh_ecc_step); stats [B,3] float64 or
    None receives (rho first, rho_best, accepted) when last != 0."""
    _chk(sums, torch.float64); _chk(state, torch.float64); _chk(stats, torch.float64)
    B = state.shape[0]
    if tuple(state.shape) != (B, ECC_STATE) or tuple(sums.shape) != (B, ECC_SUMS) or (stats is not None and tuple(stats.shape) != (B, 3)):
        raise ValueError("ecc_step: sums [B,66], state [B,24], stats [B,3] float64")
    check(lib.bh_ecc_step(_p(sums), _p(state), B, int(last), _p(stats), 3, _stream()), "bh_ecc_step")
    return state


def ecc_refine(pyr_a, size_a, pyr_b, size_b, H64, stats, ws, levels, iters, mask_pyr=None):
    """The whole coarse-to-fine refinement, enqueued on the current stream (include/bihome.h bh_ecc_refine): H64 [B,3,3] float64 is the
    start and becomes the result; stats [B,levels,3] float64; ws float64 with ecc_refine_ws_doubles(Hb, Wb, B) elements.  All the caller's."""
    _chk(pyr_a); _chk(pyr_b); _chk(H64, torch.float64); _chk(stats, torch.float64); _chk(ws, torch.float64); _chk(mask_pyr, torch.uint8)
    B, (Ha, Wa), (Hb, Wb) = H64.shape[0], size_a, size_b
    ta, tb = gray_pyramid_layout(Ha, Wa, levels)[-1], gray_pyramid_layout(Hb, Wb, levels)[-1]
    if tuple(pyr_a.shape) != (B, ta) or tuple(pyr_b.shape) != (B, tb) or (mask_pyr is not None and tuple(mask_pyr.shape) != (B, tb)):
        raise ValueError("ecc_refine: pyr_a [B,%d], pyr_b [B,%d] (and mask_pyr like pyr_b) with B = %d, got %s, %s" % (ta, tb, B, tuple(pyr_a.shape), tuple(pyr_b.shape)))
    if H64.numel() != 9 * B or tuple(stats.shape) != (B, levels, 3) or ws.numel() < ecc_refine_ws_doubles(Hb, Wb, B):
        raise ValueError("ecc_refine: H64 [B,3,3], stats [B,levels,3], ws of ecc_refine_ws_doubles() float64")
    check(lib.bh_ecc_refine(_p(pyr_a), Ha, Wa, _p(pyr_b), Hb, Wb, _p(mask_pyr), B, int(levels), int(iters), _p(H64), _p(stats), _p(ws), _stream()),
          "bh_ecc_refine")
    return H64, stats


# ------------------------------------------------------------------------------------------------
# cascaded re-prediction: image A through a homography as the model's patch, and the score of a stage (bihome_amd/align.py; csrc/cascade.hip)
# ------------------------------------------------------------------------------------------------
def align_prep_warp_u8(images, Hg, patch, cover, nx, ny, mean, std, idx=None):
    """B samples of a uint8 bank [N,Hs,Ws,3] seen through Hg [B,3,3] / [B,9] float64 (index coordinates of the P ny x P nx sub-sample
    grid -> index coordinates of the image) as the standardised patches patch [B,C,P,P] float32: the mean of nx x ny bilinear samples per
    patch pixel; cover [B,P,P] float32 (may be None) the share of them that is valid (include/bihome.h bh_align_prep_warp_u8).  Both
    outputs are the caller's (bihome_amd.align.prepare_warped allocates them).  idx [B] int32 as in align_prep_u8."""
    _chk(Hg, torch.float64); _chk(patch); _chk(cover)
    if patch.dim() != 4 or patch.shape[2] != patch.shape[3] or not _is_h(Hg) or Hg.shape[0] != patch.shape[0]:
        raise ValueError("align_prep_warp_u8: patch [B,C,P,P] float32 and Hg [B,3,3] float64, got %s and %s" % (tuple(patch.shape), tuple(Hg.shape)))
    B, C, P = patch.shape[:3]
    if cover is not None and tuple(cover.shape) != (B, P, P):
        raise ValueError("align_prep_warp_u8: cover [B,P,P] float32 = [%d,%d,%d], got %s" % (B, P, P, tuple(cover.shape)))
    _chk_images_u8(images, idx, (B,), "align_prep_warp_u8")
    check(lib.bh_align_prep_warp_u8(_p(images), _p(idx), images.shape[0], images.shape[1], images.shape[2], _p(Hg), B, P, C, int(nx), int(ny),
                                    float(mean), float(std), _p(patch), _p(cover), _stream()), "bh_align_prep_warp_u8")
    return patch, cover


def patch_ncc(w, t, cover, out):
    """out [B,8] float64 = (n, sum w, sum t, sum ww, sum tt, sum wt, rho, 0) of the patches w, t [B,C,P,P] float32 over all channels of the
    pixels with cover [B,P,P] float32 == 1 (None: all pixels) (include/bihome.h bh_patch_ncc).  out is the caller's."""
    _chk(w); _chk(t); _chk(cover); _chk(out, torch.float64)
    if w.dim() != 4 or w.shape[2] != w.shape[3] or t.shape != w.shape:
        raise ValueError("patch_ncc: w and t [B,C,P,P] float32 of one shape, got %s and %s" % (tuple(w.shape), tuple(t.shape)))
    B, C, P = w.shape[:3]
    if tuple(out.shape) != (B, 8) or (cover is not None and tuple(cover.shape) != (B, P, P)):
        raise ValueError("patch_ncc: out [B,8] float64 and cover [B,P,P] float32 with B = %d, P = %d, got %s and %s"
                         % (B, P, tuple(out.shape), None if cover is None else tuple(cover.shape)))
    check(lib.bh_patch_ncc(_p(w), _p(t), _p(cover), B, C, P, _p(out), _stream()), "bh_patch_ncc")
    return out


# ------------------------------------------------------------------------------------------------
# mosaic: both images of an aligned pair on one canvas, feathered, in one pass (bihome_amd/align.py; csrc/blend.hip, the pair walk)
# ------------------------------------------------------------------------------------------------
MOSAIC_MODES = {"feather": 0, "b_over_a": 1, "a_over_b": 2}          # include/bihome.h BH_MOSAIC_*


def _chk_pair_blend(what, images_a, images_b, Ma, Mb, gain, out, planes, idx_a, idx_b):
    """What mosaic_u8 and mosaic_bands_u8 check in common -> B."""
    _chk(Ma, torch.float64); _chk(Mb, torch.float64); _chk(gain, torch.float64); _chk_u8(out, planes)
    for M, name in ((Ma, "Ma"), (Mb, "Mb")):
        if not _is_h(M):
            raise ValueError("%s: %s [B,3,3] float64, got %s" % (what, name, tuple(M.shape)))
    B = Ma.shape[0]
    if Mb.shape[0] != B or (gain is not None and tuple(gain.shape) != (B, 2)):
        raise ValueError("%s: Ma and Mb [B,3,3] and gain [B,2] float64 with one B, got %s, %s and %s"
                         % (what, tuple(Ma.shape), tuple(Mb.shape), None if gain is None else tuple(gain.shape)))
    _chk_canvas_u8(out, planes, B, what, "Hc,Wc")
    _chk_images_u8(images_a, idx_a, (B,), what)
    _chk_images_u8(images_b, idx_b, (B,), what)
    return B


def mosaic_u8(images_a, images_b, Ma, Mb, out, cover, feather, mode, gain=None, idx_a=None, idx_b=None):
    """out [B,Hc,Wc,3] uint8 = the mosaic of images_a[idx_a[b]] and images_b[idx_b[b]] (uint8 banks [N,H,W,3]) on a canvas whose index
    coordinates Ma / Mb [B,3,3] or [B,9] float64 map to A's / B's, cover [B,Hc,Wc] uint8 (may be None) = (A present) | (B present) << 1
    (include/bihome.h bh_mosaic_u8).  feather >= 1 caps the border-distance weights; mode is 'feather', 'b_over_a' or 'a_over_b' (or
    its BH_MOSAIC_* number); gain [B,2] float64 (g, o) turns A's value into g a + o (None: unchanged).  Both outputs are the caller's
    (bihome_amd.align.mosaic_u8 allocates them)."""
    B = _chk_pair_blend("mosaic_u8", images_a, images_b, Ma, Mb, gain, out, [("cover", cover)], idx_a, idx_b)
    mode = _mode_number(mode, MOSAIC_MODES, "mosaic_u8")
    check(lib.bh_mosaic_u8(_p(images_a), _p(idx_a), images_a.shape[0], images_a.shape[1], images_a.shape[2],
                           _p(images_b), _p(idx_b), images_b.shape[0], images_b.shape[1], images_b.shape[2],
                           _p(Ma), _p(Mb), _p(gain), B, out.shape[1], out.shape[2], float(feather), mode, _p(out), _p(cover), _stream()),
          "bh_mosaic_u8")
    return out, cover


# ------------------------------------------------------------------------------------------------
# panorama: the n frames of a registered sequence on one canvas (bihome_amd/align.py; csrc/pano.hip, and csrc/blend.hip's sequence walk).
# Every buffer is the caller's.
# ------------------------------------------------------------------------------------------------
PANO_MODES = {"feather": 0, "first": 1, "last": 2}                    # include/bihome.h BH_PANO_*
PANO_MAX_FRAMES = 255


def _is_hn(M):
    """M is [B,n,3,3] or [B,n,9] with 1 <= n <= 255: the homographies of a batch of sequences."""
    return M.dim() >= 3 and 1 <= M.shape[1] <= PANO_MAX_FRAMES and M.numel() == 9 * M.shape[0] * M.shape[1]


def pano_chain(H_pairs, ref, G, gain_pairs=None, gain=None):
    """G [B,n,3,3] float64 = the chain of H_pairs [B,n-1,3,3] float64 around frame `ref` (include/bihome.h bh_pano_chain;
    bihome_amd.align.chain_host), and with gain_pairs [B,n-1,2] and gain [B,n,2] float64 both given the exposure lines along it.  The
    outputs are the caller's (bihome_amd.align.chain_device allocates them)."""
    _chk(H_pairs, torch.float64); _chk(G, torch.float64); _chk(gain_pairs, torch.float64); _chk(gain, torch.float64)
    if not _is_hn(G):
        raise ValueError("pano_chain: G [B,n,3,3] float64 with 1 <= n <= %d, got %s" % (PANO_MAX_FRAMES, tuple(G.shape)))
    B, n = G.shape[:2]
    if H_pairs.dim() < 3 or tuple(H_pairs.shape[:2]) != (B, n - 1) or H_pairs.numel() != 9 * B * (n - 1):
        raise ValueError("pano_chain: H_pairs [B,n-1,3,3] float64 with B = %d, n = %d, got %s" % (B, n, tuple(H_pairs.shape)))
    if (gain_pairs is None) != (gain is None) or (gain is not None and (tuple(gain_pairs.shape) != (B, n - 1, 2) or tuple(gain.shape) != (B, n, 2))):
        raise ValueError("pano_chain: gain_pairs [B,n-1,2] and gain [B,n,2] float64 come together, got %s and %s"
                         % (None if gain_pairs is None else tuple(gain_pairs.shape), None if gain is None else tuple(gain.shape)))
    if not 0 <= ref < n:
        raise ValueError("pano_chain: ref in [0, %d), got %r" % (n, ref))
    check(lib.bh_pano_chain(_p(H_pairs), _p(gain_pairs), B, n, int(ref), _p(G), _p(gain), _stream()), "bh_pano_chain")
    return G, gain


def pano_frame(G, size, canvas, limit, T, bbox=None, fitted=None, M=None, use=None, ref_size=None):
    """The canvas of a sequence (include/bihome.h bh_pano_frame; bihome_amd.align.pano_frame_host): G [B,n,3,3] float64, size = (Hs, Ws)
    of the frames, ref_size = (Hr, Wr) of the reference (None: size), canvas = (Hc, Wc), use [B,n] uint8 or None -> T [B,3,3], bbox [B,4],
    M [B,n,3,3] float64 and fitted [B,n] uint8, the caller's (bihome_amd.align.pano_frame_device allocates them; all but T may be None)."""
    _chk(G, torch.float64); _chk(T, torch.float64); _chk(bbox, torch.float64); _chk(M, torch.float64); _chk(fitted, torch.uint8); _chk(use, torch.uint8)
    if not _is_hn(G):
        raise ValueError("pano_frame: G [B,n,3,3] float64 with 1 <= n <= %d, got %s" % (PANO_MAX_FRAMES, tuple(G.shape)))
    B, n = G.shape[:2]
    if not _is_h(T) or T.shape[0] != B or (bbox is not None and tuple(bbox.shape) != (B, 4)) or (M is not None and tuple(M.shape) != tuple(G.shape)):
        raise ValueError("pano_frame: T [B,3,3], bbox [B,4] and M like G, float64, with B = %d, got %s, %s and %s"
                         % (B, tuple(T.shape), None if bbox is None else tuple(bbox.shape), None if M is None else tuple(M.shape)))
    for t, what in ((fitted, "fitted"), (use, "use")):
        if t is not None and tuple(t.shape) != (B, n):
            raise ValueError("pano_frame: %s [B,n] uint8 with B = %d, n = %d, got %s" % (what, B, n, tuple(t.shape)))
    (Hs, Ws), (Hr, Wr), (Hc, Wc) = size, size if ref_size is None else ref_size, canvas
    check(lib.bh_pano_frame(_p(G), _p(use), B, n, int(Hs), int(Ws), int(Hr), int(Wr), int(Hc), int(Wc), float(limit), _p(T), _p(bbox), _p(fitted),
                            _p(M), _stream()), "bh_pano_frame")
    return T, bbox, fitted, M


def _chk_seq_blend(what, images, idx, M, gain, use, out, planes):
    """What pano_u8 and pano_bands_u8 check in common -> (B, n)."""
    _chk(M, torch.float64); _chk(gain, torch.float64); _chk(use, torch.uint8); _chk_u8(out, planes)
    if not _is_hn(M):
        raise ValueError("%s: M [B,n,3,3] float64 with 1 <= n <= %d, got %s" % (what, PANO_MAX_FRAMES, tuple(M.shape)))
    B, n = M.shape[:2]
    if (gain is not None and tuple(gain.shape) != (B, n, 2)) or (use is not None and tuple(use.shape) != (B, n)):
        raise ValueError("%s: gain [B,n,2] float64 and use [B,n] uint8 with B = %d, n = %d, got %s and %s"
                         % (what, B, n, None if gain is None else tuple(gain.shape), None if use is None else tuple(use.shape)))
    _chk_canvas_u8(out, planes, B, what, "Hc,Wc")
    _chk_images_u8(images, idx, (B, n), what)
    return B, n


def pano_u8(images, idx, M, out, count, feather, mode, gain=None, use=None):
    """out [B,Hc,Wc,3] uint8 = the n frames images[idx[b,k]] (one uint8 bank [N,Hs,Ws,3], idx [B,n] int32 or None: frame k is image k)
    on a canvas whose index coordinates M [B,n,3,3] float64 map to frame k's, count [B,Hc,Wc] uint8 (may be None) the number of frames
    present (include/bihome.h bh_pano_u8; bihome_amd.align.pano_host).  mode is 'feather', 'first' or 'last' (or its BH_PANO_* number);
    gain [B,n,2] float64 (g, o) per frame and use [B,n] uint8 (0: the frame is left out) may be None.  Both outputs are the caller's
    (bihome_amd.align.pano_u8 allocates them)."""
    B, n = _chk_seq_blend("pano_u8", images, idx, M, gain, use, out, [("count", count)])
    mode = _mode_number(mode, PANO_MODES, "pano_u8")
    check(lib.bh_pano_u8(_p(images), _p(idx), images.shape[0], images.shape[1], images.shape[2], _p(M), _p(gain), _p(use), B, n,
                         out.shape[1], out.shape[2], float(feather), mode, _p(out), _p(count), _stream()), "bh_pano_u8")
    return out, count


# ------------------------------------------------------------------------------------------------
# global adjustment: all frames of a sequence solved jointly from its edges (bihome_amd/align.py; csrc/adjust.hip).  Every buffer is the
# caller's.
# ------------------------------------------------------------------------------------------------
ADJUST_MAX_FRAMES = 64                                                # include/bihome.h BH_ADJUST_MAX_FRAMES
ADJUST_MAX_EDGES = 1024                                               # include/bihome.h BH_ADJUST_MAX_EDGES


def pano_adjust_ws_doubles(n, E, B):
    return _size_query(lib.bh_pano_adjust_ws_doubles, "bh_pano_adjust_ws_doubles", int(n), int(E), int(B))


def pano_adjust(G0, link, H_links, weight, ref, size, grid, iters, G, work, ws):
    """G [B,n,3,3] float64 = G0 [B,n,3,3] float64 after `iters` Levenberg-Marquardt steps on the edges link [E,2] int32 (a, b) with
    H_links [B,E,3,3] float64 (b's index coordinates -> a's) and weight [B,E] float64 or None; size = (Hs, Ws) of the frames, grid the
    control lattice's side; work [B,4] float64 = (cost at the start, cost at the result, accepted steps, final lambda); ws float64 with
    pano_adjust_ws_doubles(n, E, B) elements (include/bihome.h bh_pano_adjust; bihome_amd.align.adjust_host).  G, work and ws are the
    caller's (bihome_amd.align.adjust_device allocates them)."""
    _chk(G0, torch.float64); _chk(H_links, torch.float64); _chk(weight, torch.float64); _chk(G, torch.float64); _chk(work, torch.float64)
    _chk(ws, torch.float64); _chk(link, torch.int32)
    if G0.dim() < 3 or not 2 <= G0.shape[1] <= ADJUST_MAX_FRAMES or G0.numel() != 9 * G0.shape[0] * G0.shape[1] or tuple(G.shape) != tuple(G0.shape):
        raise ValueError("pano_adjust: G0 and G [B,n,3,3] float64 with 2 <= n <= %d, got %s and %s" % (ADJUST_MAX_FRAMES, tuple(G0.shape), tuple(G.shape)))
    B, n = G0.shape[:2]
    if link.dim() != 2 or link.shape[1] != 2 or not 1 <= link.shape[0] <= ADJUST_MAX_EDGES:
        raise ValueError("pano_adjust: link [E,2] int32 with 1 <= E <= %d, got %s" % (ADJUST_MAX_EDGES, tuple(link.shape)))
    E = link.shape[0]
    if H_links.dim() < 3 or tuple(H_links.shape[:2]) != (B, E) or H_links.numel() != 9 * B * E or (weight is not None and tuple(weight.shape) != (B, E)):
        raise ValueError("pano_adjust: H_links [B,E,3,3] and weight [B,E] float64 with B = %d, E = %d, got %s and %s"
                         % (B, E, tuple(H_links.shape), None if weight is None else tuple(weight.shape)))
    if tuple(work.shape) != (B, 4) or ws.numel() < pano_adjust_ws_doubles(n, E, B):
        raise ValueError("pano_adjust: work [B,4] and ws of pano_adjust_ws_doubles() float64, got %s and %d elements" % (tuple(work.shape), ws.numel()))
    if not 0 <= ref < n:
        raise ValueError("pano_adjust: ref in [0, %d), got %r" % (n, ref))
    check(lib.bh_pano_adjust(_p(G0), _p(link), _p(H_links), _p(weight), B, n, E, int(ref), int(size[0]), int(size[1]), int(grid), int(iters), _p(G),
                             _p(work), _p(ws), _stream()), "bh_pano_adjust")
    return G, work


# ------------------------------------------------------------------------------------------------
# two-band blend: the low band of uint8 frames, and the mosaic / panorama that blends it with the feather and takes the high band from one
# frame per pixel (bihome_amd/align.py; csrc/blur.hip, and csrc/blend.hip's two walks with its band rule).  Every buffer is the caller's.
# ------------------------------------------------------------------------------------------------
BLUR_MAX_RADIUS = 32


def blur_u8(images, out, taps, idx=None):
    """out [count,H,W,3] uint8 = the integer Gaussian low-pass of images[idx[s]] (one uint8 bank [N,H,W,3]; idx int32 of count elements in
    any shape, or None: sample s is image s and count <= N is out's) with the HOST taps w_0 .. w_r (bihome_amd.align.blur_taps), border
    replicated (include/bihome.h bh_blur_u8; bihome_amd.align.blur_host).  out is the caller's (bihome_amd.align.blur_u8 allocates it)."""
    _chk(out, torch.uint8)
    if out.dim() != 4 or out.shape[3] != 3:
        raise ValueError("blur_u8: out [count,H,W,3] uint8, got %s" % (tuple(out.shape),))
    count = out.shape[0]
    _chk_images_u8(images, None if idx is None else idx.reshape(-1), (count,), "blur_u8")
    if tuple(out.shape[1:]) != tuple(images.shape[1:]):
        raise ValueError("blur_u8: out [count,H,W,3] of the images' size %s, got %s" % (tuple(images.shape[1:3]), tuple(out.shape)))
    w = [int(t) for t in taps]
    if not 2 <= len(w) <= BLUR_MAX_RADIUS + 1 or min(w) < 0 or w[0] + 2 * sum(w[1:]) != 2048:
        raise ValueError("blur_u8: taps are w_0 .. w_r, 1 <= r <= %d, none negative, w_0 + 2 sum w_i = 2048, got %r" % (BLUR_MAX_RADIUS, w))
    check(lib.bh_blur_u8(_p(images), _p(idx), images.shape[0], images.shape[1], images.shape[2], count, (ctypes.c_int * len(w))(*w), len(w) - 1,
                         _p(out), _stream()), "bh_blur_u8")
    return out


def pano_bands_u8(images, low, idx, M, out, count, winner, feather, gain=None, use=None):
    """out [B,Hc,Wc,3] uint8 = the two-band blend of the n frames images[idx[b,k]] with their low bands low [B,n,Hs,Ws,3] (or [B n,Hs,Ws,3])
    uint8 on a canvas whose index coordinates M [B,n,3,3] float64 map to frame k's; count [B,Hc,Wc] uint8 the number of frames present and
    winner [B,Hc,Wc] uint8 the frame the high band comes from, 255 for none (either may be None) (include/bihome.h bh_pano_bands_u8;
    bihome_amd.align.bands_host).  gain and use as in pano_u8.  The outputs are the caller's (bihome_amd.align.pano_bands_u8 allocates)."""
    _chk(low, torch.uint8)
    B, n = _chk_seq_blend("pano_bands_u8", images, idx, M, gain, use, out, [("count", count), ("winner", winner)])
    if low.numel() != B * n * images[0].numel() or tuple(low.shape[-3:]) != tuple(images.shape[1:]) or tuple(low.shape[:-3]) not in ((B, n), (B * n,)):
        raise ValueError("pano_bands_u8: low [B,n,Hs,Ws,3] uint8 with B = %d, n = %d and the frames' size %s, got %s"
                         % (B, n, tuple(images.shape[1:3]), tuple(low.shape)))
    check(lib.bh_pano_bands_u8(_p(images), _p(low), _p(idx), images.shape[0], images.shape[1], images.shape[2], _p(M), _p(gain), _p(use), B, n,
                               out.shape[1], out.shape[2], float(feather), _p(out), _p(count), _p(winner), _stream()), "bh_pano_bands_u8")
    return out, count, winner


def mosaic_bands_u8(images_a, low_a, images_b, low_b, Ma, Mb, out, cover, winner, feather, gain=None, idx_a=None, idx_b=None):
    """out [B,Hc,Wc,3] uint8 = the two-band blend of images_a[idx_a[b]] and images_b[idx_b[b]] with their low bands low_a [B,Ha,Wa,3] and
    low_b [B,Hb,Wb,3] uint8 (in sample order); cover as in mosaic_u8, winner [B,Hc,Wc] uint8 = 0 for A, 1 for B, 255 for none (either may be
    None) (include/bihome.h bh_mosaic_bands_u8; bihome_amd.align.mosaic_bands_host).  The outputs are the caller's."""
    _chk(low_a, torch.uint8); _chk(low_b, torch.uint8)
    B = _chk_pair_blend("mosaic_bands_u8", images_a, images_b, Ma, Mb, gain, out, [("cover", cover), ("winner", winner)], idx_a, idx_b)
    for low, images, what in ((low_a, images_a, "low_a"), (low_b, images_b, "low_b")):
        if tuple(low.shape) != (B,) + tuple(images.shape[1:]):
            raise ValueError("mosaic_bands_u8: %s [B,H,W,3] uint8 with B = %d and its images' size %s, got %s" % (what, B, tuple(images.shape[1:3]), tuple(low.shape)))
    check(lib.bh_mosaic_bands_u8(_p(images_a), _p(low_a), _p(idx_a), images_a.shape[0], images_a.shape[1], images_a.shape[2],
                                 _p(images_b), _p(low_b), _p(idx_b), images_b.shape[0], images_b.shape[1], images_b.shape[2],
                                 _p(Ma), _p(Mb), _p(gain), B, out.shape[1], out.shape[2], float(feather), _p(out), _p(cover), _p(winner), _stream()),
          "bh_mosaic_bands_u8")
    return out, cover, winner
