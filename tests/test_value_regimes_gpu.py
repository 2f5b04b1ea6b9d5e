"""Every kernel family on the VALUES training feeds it, not on randn: exact zeros, ties, constants and extreme magnitudes.

The shape sweeps (test_rectangular_gpu.py and the square tests) draw every operand from randn times a constant.  The extractor's maps are
post-ReLU (more than half exact zeros, f1w - f2 == 0 exactly at many positions), a hinge that is inactive everywhere sends an exactly-zero
gradient through the whole network, masks can be all zero, patches constant, and the fp16-piece arithmetic (precision 4) takes its scales
from the data.  Each case here pins its kernel with bh_conv_variant / route bits and uses the smallest shape that kernel takes.

Every bound in this file is of one of three kinds, named where it is used:
  exact     bitwise equality (power-of-two equivariance, an accumulating call that must leave its target alone) or exactly 0;
  derived   from the float64 quantities and the roundings the documented arithmetic makes (BatchNorm forward, section 4);
  measured  against the float64 / float32 reference with the stated margin - the bounds of the square tests, through their helpers.
No bound is taken from the output of the kernel under test.

Sections: 1 power-of-two scaling (conv stack, stems, warp image) and the ends of the fp16 scale exponent; 2 exact zeros, one-hot
gradients, wide and non-finite operands in the conv stack; 3 bh_absmax; 4 BatchNorm on hand-set channels; 5 loss kernels on post-ReLU
features; 6 the warp family - plain, fused into the stem, its image adjoint, the photometric head's - on degenerate images and
homographies, the horizon inside the patch included.  The generators and the float64 stand-ins live in tests/value_regimes.py and are
checked without a GPU by tests/test_value_regimes_cpu.py.

`pytest -s` prints a MEASURED line per comparison next to its bound."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_conv_kernels_gpu as C
import test_f16x2_gpu as F16
import test_head_kernels_gpu as HK
import value_regimes as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from bihome_amd import kernels
    return kernels


MEASURED = []         # (what, measured, bound as text) of the comparisons a test made outside C.close


@pytest.fixture(autouse=True)
def report_measured(request):
    del C.ERRORS[:]
    del MEASURED[:]
    yield
    for what, got, bound in MEASURED:
        print("\nMEASURED %s: %s: %s (bound: %s)" % (request.node.name, what, got, bound))
    if C.ERRORS:
        err, tol = max(C.ERRORS, key=lambda e: e[0] / e[1])
        print("\nMEASURED %s: largest normalised error of %d comparisons %.3e (bound %.1e)" % (request.node.name, len(C.ERRORS), err, tol))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_bits(a, b):
    """Number of elements of a whose bit pattern is not b's (+0 and -0 count as equal: an exactly-zero sum has either sign)."""
    return int(((a != b) & ~(torch.isnan(a) & torch.isnan(b))).sum().item())


def exact(what, a, b):
    """exact bound: a == b bit for bit."""
    n = _same_bits(a, b)
    MEASURED.append((what, "%d of %d elements differ" % (n, a.numel()), "exact, 0 differ"))
    assert n == 0, "%s: %d of %d elements differ, largest |a - b| %.3e of max |b| %.3e" % (
        what, n, a.numel(), (a.double() - b.double()).abs().max().item(), b.abs().max().item())


def rel_l2(a, ref):
    return ((a.detach().cpu().double() - ref).norm() / ref.norm()).item()


# ------------------------------------------------------------------------------------------------
# the operations of sections 1 and 2: each is a dict of closures over ONE pinned launch geometry
# ------------------------------------------------------------------------------------------------
POW2 = (-40, -13, 13, 40)


class Conv3x3:
    """A 3x3 / stride-1 layer on packed weights (halo or persistent kernel, precision 0 / 2 / 4) and its workspace-form weight gradient."""

    def __init__(self, K, N, H, W, Ci, Co, prec, route, fwd_kernel):
        from bihome_amd._lib import ROUTE_HALO_SMALL
        self.K, self.shape, self.prec = K, (N, H, W, Ci, Co), prec
        self.d = K.conv_desc(N, H, W, Ci, Co, 3, 1, 1, precision=prec, route=ROUTE_HALO_SMALL | route)
        dp = K._with_layout(self.d, K.packed_layout(prec))
        for which, acc in (("fwd", False), ("dgrad", False), ("dgrad", True)):
            assert K.conv_variant(dp, which, accumulate=acc).startswith(fwd_kernel + ("<false," if which == "fwd" else "<true,")), K.conv_variant(dp, which)
        if prec == 4:
            assert K.conv_variant(dp, "fwd").endswith(("true>", "conv3x3_pc_kernel<false,false,0>"))          # (the fp16-piece form)

    def data(self, seed=0):
        N, H, W, Ci, Co = self.shape
        g = torch.Generator().manual_seed(1000 + seed + N * 7 + H)
        x = torch.randn(N, H, W, Ci, generator=g).cuda()
        gy = (torch.randn(N, H, W, Co, generator=g) * 1e-4).cuda()
        w = (torch.randn(Co, Ci, 3, 3, generator=g) * 0.05).cuda().contiguous(memory_format=torch.channels_last)
        b = torch.randn(Co, generator=g).cuda()
        return x, gy, w, b

    def fwd(self, x, w, b=None):
        _, pf, _ = F16._packed(self.K, w, self.prec)
        return self.K.conv_fwd(x, w.permute(0, 2, 3, 1), b, self.d, wpacked=pf)

    def dgrad(self, gy, w, out=None):
        _, _, pd = F16._packed(self.K, w, self.prec)
        return self.K.conv_dgrad(gy, w.permute(0, 2, 3, 1), self.d, out=out, wpacked=pd)


def wgrad_x3(K, x, gy, prec, gw=None, kernel="wgrad_x3_kernel<"):
    """gw (+)= the workspace-form weight gradient of a 3x3 / stride-1 layer, on wgrad_x3_kernel."""
    N, H, W, Ci = x.shape
    Co = gy.shape[-1]
    d = K.conv_desc(N, H, W, Ci, Co, 3, 1, 1, precision=prec)
    assert K.conv_variant(d, "wgrad_det").startswith(kernel), K.conv_variant(d, "wgrad_det")
    need = K.wgrad_det_bytes(d)
    assert need > 0
    ws = torch.empty(need // 4, dtype=torch.float32, device="cuda")
    gw = torch.zeros(Co, 3, 3, Ci, device="cuda") if gw is None else gw.clone()
    K.conv_wgrad(x, gy, gw, None, d, det_ws=ws)
    return gw


def pow2_sweep(what, op, a, b, acc=None):
    """exact bound.  op(a 2^s, b) == op(a, b) 2^s == op(a, b 2^s) and op(a 2^s, b 2^-s) == op(a, b), bit for bit, for s in POW2 (acc: a
    third operand the operation accumulates onto - it is scaled with the result)."""
    base = op(a, b) if acc is None else op(a, b, acc)
    assert torch.isfinite(base).all() and base.abs().max().item() > 0
    for s in POW2:
        f, r = 2.0 ** s, 2.0 ** -s
        for fa, fb, fo, name in ((f, 1.0, f, "first operand"), (1.0, f, f, "second operand"), (f, r, 1.0, "both operands, s and -s")):
            y = op(a * fa, b * fb) if acc is None else op(a * fa, b * fb, acc * fo)
            exact("%s, 2^%d on the %s" % (what, s, name), y, base * fo)


# ------------------------------------------------------------------------------------------------
# 1. power-of-two scaling is exact (conv stack, warp image)
# ------------------------------------------------------------------------------------------------
def _halo(K, N, H, W, Ci, Co, prec):
    from bihome_amd._lib import ROUTE_C3_TILE_WG
    return Conv3x3(K, N, H, W, Ci, Co, prec, ROUTE_C3_TILE_WG, "conv3x3_halo_kernel")


def _persistent(K, N=4, H=16, W=32, Ci=64, Co=64):
    return Conv3x3(K, N, H, W, Ci, Co, 4, 0, "conv3x3_pc_kernel")


def _sweep_3x3(layer):
    x, gy, w, b = layer.data()
    pow2_sweep("forward", lambda x_, w_: layer.fwd(x_, w_), x, w)
    pow2_sweep("dgrad", lambda g_, w_: layer.dgrad(g_, w_), gy, w)
    pow2_sweep("accumulating dgrad", lambda g_, w_, o_: layer.dgrad(g_, w_, out=o_.clone()), gy, w, acc=x * 1e-4)
    # a bias scaled with the operand
    base = layer.fwd(x, w, b)
    for s in POW2:
        exact("forward with bias, 2^%d on x and the bias" % s, layer.fwd(x * 2.0 ** s, w, b * 2.0 ** s), base * 2.0 ** s)


@pytest.mark.parametrize("N,H,W,Ci,Co,prec", [(2, 8, 8, 64, 64, 4), (2, 8, 8, 32, 32, 4), (2, 8, 8, 64, 64, 2), (2, 8, 8, 64, 64, 0)])
def test_pow2_halo_kernel(K, N, H, W, Ci, Co, prec):
    """exact.  conv3x3_halo_kernel, forward / dgrad / accumulating dgrad: fp16 pieces of x 2^k with k from the magnitude record (precision 4),
    three exact bf16 pieces (2), fp32-input MFMA (0) - a power-of-two factor on an operand changes no significand anywhere."""
    _sweep_3x3(_halo(K, N, H, W, Ci, Co, prec))


def test_pow2_persistent_kernel(K):
    """exact.  conv3x3_pc_kernel at the smallest shape test_persistent_kernel_f16x2 uses."""
    _sweep_3x3(_persistent(K))


@pytest.mark.parametrize("N,H,Ci,Co,prec", [(2, 8, 64, 64, 4), (2, 8, 64, 64, 2), (12, 4, 64, 128, 4)])
def test_pow2_wgrad_x3(K, N, H, Ci, Co, prec):
    """exact.  wgrad_x3_kernel, workspace form (fixed-order split-K reduction); 4 x 4 maps: its four-images-per-tile form, which exists in
    fp16 pieces only."""
    kernel = "wgrad_x3_kernel<64,false,2,true,false,true>" if H == 4 else "wgrad_x3_kernel<64,false,%d,%s,false,false>" % ((2, "true") if prec == 4 else (3, "false"))
    g = torch.Generator().manual_seed(N + H + Ci)
    x = torch.randn(N, H, H, Ci, generator=g).cuda()
    gy = (torch.randn(N, H, H, Co, generator=g) * 3e-5).cuda()
    pow2_sweep("weight gradient", lambda x_, g_: wgrad_x3(K, x_, g_, prec, kernel=kernel), x, gy)
    gw0 = (torch.randn(Co, 3, 3, Ci, generator=g) * 1e-3).cuda()
    pow2_sweep("accumulating weight gradient", lambda x_, g_, o_: wgrad_x3(K, x_, g_, prec, gw=o_, kernel=kernel), x, gy, acc=gw0)


@pytest.mark.parametrize("prec,route_x3", [(0, False), (4, True)])
@pytest.mark.parametrize("N,Hi,Wi,Ci,Co,k,s,p", [c for c in C.RECT_CONV_CASES if c in ((2, 16, 24, 64, 128, 1, 2, 0), (2, 16, 32, 64, 128, 3, 2, 1))])
def test_pow2_generic_kernel(K, N, Hi, Wi, Ci, Co, k, s, p, prec, route_x3):
    """exact.  conv_gemm_kernel: fp32-input MFMA, and three exact bf16 pieces (BH_ROUTE_GEMM_X3 at precision 4), on the 1x1 and the 3x3
    stride-2 layer of RECT_CONV_CASES; forward, dgrad (the output-parity-class form: even extents) and weight gradient."""
    from bihome_amd._lib import ROUTE_GENERIC_CONV, ROUTE_GEMM_X3
    d = K.conv_desc(N, Hi, Wi, Ci, Co, k, s, p, precision=prec, route=ROUTE_GENERIC_CONV | (ROUTE_GEMM_X3 if route_x3 else 0))
    for which in ("fwd", "dgrad"):
        v = K.conv_variant(d, which)
        assert v.startswith("conv_gemm_kernel<") and (len(v.split(",")) == 7 and v.endswith(",true>")) == route_x3, v
    x = torch.tensor(C.rnd((N, Hi, Wi, Ci), 1)).cuda()
    w = torch.tensor((C.rnd((Co, k, k, Ci), 2) / np.sqrt(Ci * k * k)).astype(np.float32)).cuda()
    gy = torch.tensor(C.rnd((N, d.Ho, d.Wo, Co), 4)).cuda()
    pow2_sweep("forward", lambda x_, w_: K.conv_fwd(x_, w_, None, d), x, w)
    pow2_sweep("dgrad", lambda g_, w_: K.conv_dgrad(g_, w_, d), gy, w)
    pow2_sweep("accumulating dgrad", lambda g_, w_, o_: K.conv_dgrad(g_, w_, d, out=o_.clone()), gy, w, acc=x)

    # measured (check_conv2d_fwd_dgrad_wgrad's bound, 3e-5 of the largest entry of the float64 gradient).  The generic weight gradient adds its
    # split-K partial blocks with float atomics in arrival order (csrc/wgrad.hip): two launches need not agree bitwise, so it is held to its
    # square test's bound at every s instead of to the sweep.
    assert K.conv_variant(d, "wgrad").startswith("wgrad_kernel<true")
    wt = w.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), wt, None, stride=s, padding=p)
    ref = torch.autograd.grad(y, wt, gy.double().cpu().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    for e in POW2:
        for fx, fg in ((2.0 ** e, 1.0), (1.0, 2.0 ** e)):
            gw = torch.zeros_like(w)
            K.conv_wgrad(x * fx, gy * fg, gw, None, d)
            C.close(gw.cpu().double() * 2.0 ** -e, ref)


def _stem_fwd(K, N, Ci, prec=4):
    d = K.conv_desc(N, 64, 64, Ci, 64, 7, 2, 3, in_nchw=Ci != 1, precision=prec)
    assert K.conv_variant(d, "fwd") == "stem7_fwd_f16_kernel<%d>" % Ci
    return d


@pytest.mark.parametrize("Ci", [1, 2])
def test_pow2_stem_forward(K, Ci):
    """exact.  stem7_fwd_f16_kernel<1> / <2> at its minimum of 256 tiles: the patch's scale is taken per tile from the tile's own maximum and
    the filter bank's per launch - both follow a power-of-two factor."""
    N = 16
    d = _stem_fwd(K, N, Ci)
    g = torch.Generator().manual_seed(7 + Ci)
    x = torch.randn(N, Ci, 64, 64, generator=g).cuda()
    x[0, :, :32] *= 1e-4                                     # dark tiles keep their own scale
    if Ci == 1:
        x = x.view(N, 64, 64, 1)
    w = (torch.randn(64, 7, 7, Ci, generator=g) * 0.1).cuda()
    pow2_sweep("stem forward", lambda x_, w_: K.conv_fwd(x_, w_, None, d), x, w)


def _stem_dgrad(K, gy, w, prec, N):
    from bihome_amd._lib import check, lib
    d = K.conv_desc(N, 64, 64, 1, 64, 7, 2, 3, precision=prec)
    assert d.N * d.Ho * d.Wo >= 4096
    gx = torch.full((N, 64, 64, 1), float("nan"), device="cuda")
    check(lib.bh_stem7_dgrad_c1(_p(gy), _p(w), _p(gx), ctypes.byref(d), _stream()), "bh_stem7_dgrad_c1")
    return gx


@pytest.mark.parametrize("prec", [4, 0])
def test_pow2_stem_dgrad(K, prec):
    """exact.  bh_stem7_dgrad_c1 (the C entry point: no doubt about the kernel), window GEMM in fp16 pieces with a scale per tile (4) and on
    the fp32-input MFMA (0).  The kernel has no atomics - every image pixel sums its <= 16 taps itself (csrc/stem7.hip) - so two launches
    agree bit for bit, which is asserted first."""
    N = 4
    g = torch.Generator().manual_seed(21)
    gy = torch.randn(N, 32, 32, 64, generator=g).cuda()
    w = (torch.randn(64, 7, 7, 1, generator=g) / 7).cuda()
    op = lambda g_, w_: _stem_dgrad(K, g_, w_, prec, N)
    exact("two launches on the same data", op(gy, w), op(gy, w))
    pow2_sweep("stem dgrad", op, gy, w)


@pytest.mark.parametrize("size", [64, 48])
def test_pow2_warp_image(K, size):
    """exact.  The warped image of bh_warp_fwd (pool 4: the fast kernel on 64 x 64, the generic one on 48 x 48): a blend of four taps with
    weights that do not depend on the image."""
    B = 2
    rng = np.random.Generator(np.random.PCG64(size))
    img = HK.dev(rng.standard_normal((B, 2, size, size)).astype(np.float32))
    H64, _ = K.h4pt_fwd(HK.dev(HK.rand_delta(B, size, amp=size / 4.0)), (size, size))
    base, cov = K.warp_fwd(img, H64, 4)
    assert base.abs().max().item() > 0
    for s in POW2:
        out, cov_s = K.warp_fwd(img * 2.0 ** s, H64, 4)
        exact("warped image, 2^%d on the image" % s, out, base * 2.0 ** s)
        exact("coverage, 2^%d on the image" % s, cov_s, cov)


def _stem_fwd_warp(K, src, H64, wt, d):
    from bihome_amd._lib import check, lib
    B, _, h, w = src.shape
    y = torch.full((B, h // 2, w // 2, 64), float("nan"), device="cuda")
    warped = torch.full((B, 1, h, w), float("nan"), device="cuda")
    cov = torch.full((B, h // 4, w // 4), float("nan"), device="cuda")
    check(lib.bh_stem7_fwd_warp(_p(src), _p(H64), 4, _p(wt), None, _p(y), ctypes.byref(d), _p(warped), _p(cov), None, 1, _stream()), "bh_stem7_fwd_warp")
    return y, warped, cov


def test_pow2_stem_forward_with_the_warp_folded_in(K):
    """exact.  bh_stem7_fwd_warp: y and the warped image follow a power-of-two factor on the source image (and y one on the filter bank)."""
    B, size = 16, 64
    rng = np.random.Generator(np.random.PCG64(B * 11 + size))
    src = F.avg_pool2d(torch.tensor(rng.standard_normal((B, 1, size, size)).astype(np.float32)), 3, 1, 1).cuda().contiguous()
    wt = torch.tensor((rng.standard_normal((64, 7, 7, 1)) * 0.05).astype(np.float32)).cuda()
    H64, _ = K.h4pt_fwd(HK.dev(HK.rand_delta(B, size + 1, amp=size / 4.0)), (size, size))
    d = _stem_fwd(K, B, 1)
    y0, warped0, cov0 = _stem_fwd_warp(K, src, H64, wt, d)
    for s in POW2:
        f = 2.0 ** s
        y, warped, cov = _stem_fwd_warp(K, src * f, H64, wt, d)
        exact("y, 2^%d on the source image" % s, y, y0 * f)
        exact("warped image, 2^%d on the source image" % s, warped, warped0 * f)
        exact("coverage, 2^%d on the source image" % s, cov, cov0)
        y, warped, _ = _stem_fwd_warp(K, src, H64, wt * f, d)
        exact("y, 2^%d on the filter bank" % s, y, y0 * f)
        exact("warped image, 2^%d on the filter bank" % s, warped, warped0)
        y, _, _ = _stem_fwd_warp(K, src * f, H64, wt * 2.0 ** -s, d)
        exact("y, 2^%d on the source image and 2^%d on the filter bank" % (s, -s), y, y0)


# 1 (continued): beyond the exponent clamp of bh_f16_scale_exp: loud or graceful
@pytest.mark.parametrize("op", ["forward", "wgrad"])
def test_f16x2_beyond_the_exponent_clamp(K, op):
    """The scale exponent k = 14 - floor(log2 record) is clamped to [-100, 127] (csrc/common.h bh_f16_scale_exp).  The contract at the ends is
    "loud or graceful", never a plausible wrong finite number:
      x 2^110 (max |x| ~ 2^112, k = -98: inside the clamp) - exact, the power-of-two sweep continues to hold;
      x 2^116 (record exponent 118, k = -104 clamped to -100: the scaled operand passes 65504) - the result has an inf or a NaN;
      x 2^-110 (k = 122) - measured: finite and within the square test's bound of float64 (err[4] <= 1.5 err[0], the fp32-input MFMA
      kernel's error on the same data; + 1e-8 for the weight gradient), or exactly 0.
    With the upper clamp at 100, as it was, this last case came out finite and wrong: rel-L2 against float64 1.77e-5 (forward) / 1.78e-5
    (weight gradient) on the MI355X where the fp32-input MFMA kernel has 4.1e-7 / 1.9e-7 - x 2^100 peaks at 2^-8 and the fp16 pieces keep
    16 bits of it.  The scale is a float built from its exponent field, so k may be 127: the clamp moved, the case stays."""
    if op == "forward":
        layer, base = _halo(K, 2, 8, 8, 64, 64, 4), _halo(K, 2, 8, 8, 64, 64, 0)
        x, _, w, _ = layer.data()
        run4, run0 = (lambda a: layer.fwd(a, w)), (lambda a: base.fwd(a, w))
        ref = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), w.double().cpu(), None, 1, 1).permute(0, 2, 3, 1)
        slack = 0.0
    else:
        g = torch.Generator().manual_seed(2 + 8 + 64)
        x = torch.randn(2, 8, 8, 64, generator=g).cuda()
        gy = (torch.randn(2, 8, 8, 64, generator=g) * 3e-5).cuda()
        run4, run0 = (lambda a: wgrad_x3(K, a, gy, 4)), (lambda a: wgrad_x3(K, a, gy, 0, kernel="wgrad_s1_kernel<"))
        wz = torch.zeros(64, 64, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), wz, None, 1, 1)
        ref = torch.autograd.grad(y, wz, gy.double().cpu().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
        slack = 1e-8
    y1 = run4(x)
    exact("2^110 on x (inside the clamp)", run4(x * 2.0 ** 110), y1 * 2.0 ** 110)
    up = run4(x * 2.0 ** 116)
    MEASURED.append(("2^116 on x", "%d of %d results non-finite" % (int((~torch.isfinite(up)).sum()), up.numel()), "at least one: loud"))
    assert not torch.isfinite(up).all()
    xs = x * 2.0 ** -110
    down = run4(xs)
    assert torch.isfinite(down).all()
    e4, e0 = rel_l2(down.double() * 2.0 ** 110, ref), rel_l2(run0(xs).double() * 2.0 ** 110, ref)
    MEASURED.append(("2^-110 on x: rel-L2 vs f64", "%.2e" % e4, "1.5 x fp32-input MFMA's %.2e + %g, or exactly 0" % (e0, slack)))
    assert (down == 0).all() or e4 <= 1.5 * e0 + slack, (e4, e0)


# ------------------------------------------------------------------------------------------------
# 2. exact zeros in the conv stack
# ------------------------------------------------------------------------------------------------
def _layers(K):
    return [("halo f16x2 64", lambda: _halo(K, 2, 8, 8, 64, 64, 4)), ("halo f16x2 32", lambda: _halo(K, 2, 8, 8, 32, 32, 4)),
            ("halo f32x3", lambda: _halo(K, 2, 8, 8, 64, 64, 2)), ("halo fp32", lambda: _halo(K, 2, 8, 8, 64, 64, 0)),
            ("persistent f16x2", lambda: _persistent(K))]


@pytest.mark.parametrize("which", range(5))
def test_zero_operand_3x3(K, which):
    """exact.  x == 0: y is the bias, bit for bit; gy == 0: gx is 0 and an accumulating call leaves `out` as it was; w == 0 (through
    bh_conv3x3_pack_f16 at precision 4: its maxima slots are 0): the same; the magnitude record measured for a zero operand is exactly 0;
    nothing is non-finite."""
    name, make = _layers(K)[which]
    layer = make()
    x, gy, w, b = layer.data()
    N, H, W, Ci, Co = layer.shape
    for zx, zw in ((True, False), (False, True)):
        xx, ww = (torch.zeros_like(x) if zx else x), (torch.zeros_like(w) if zw else w)
        gg = torch.zeros_like(gy) if zx else gy
        y = layer.fwd(xx, ww, b)
        exact("%s: forward of %s == 0" % (name, "x" if zx else "w"), y, b.expand(N, H, W, Co))
        exact("%s: forward without bias" % name, layer.fwd(xx, ww), torch.zeros(N, H, W, Co, device="cuda"))
        exact("%s: dgrad of %s == 0" % (name, "gy" if zx else "w"), layer.dgrad(gg, ww), torch.zeros_like(x))
        exact("%s: accumulating dgrad" % name, layer.dgrad(gg, ww, out=x.clone()), x)
        if layer.prec == 4 and zx:
            assert xx._bh_amax.max().item() == 0.0 and gg._bh_amax.max().item() == 0.0 and (xx._bh_amax >= 0).all()
        if layer.prec == 4 and zw:
            _, pf, pd = F16._packed(K, ww, 4)
            n = Co * 9 * Ci
            assert pf[n:].abs().max().item() == 0.0 and pd[n:].abs().max().item() == 0.0 and (pf[:n].view(torch.int32) == 0).all()


@pytest.mark.parametrize("N,H,Ci,Co,prec", [(2, 8, 64, 64, 4), (2, 8, 64, 64, 2), (12, 4, 64, 128, 4)])
def test_zero_operand_wgrad_x3(K, N, H, Ci, Co, prec):
    """exact.  x == 0, then gy == 0: gw is 0, an accumulating call leaves gw as it was, the measured record of the zero operand is 0."""
    kernel = "wgrad_x3_kernel<64,false,2,true,false,true>" if H == 4 else "wgrad_x3_kernel<64,"
    g = torch.Generator().manual_seed(N + H + Ci)
    x = torch.randn(N, H, H, Ci, generator=g).cuda()
    gy = (torch.randn(N, H, H, Co, generator=g) * 3e-5).cuda()
    gw0 = (torch.randn(Co, 3, 3, Ci, generator=g) * 1e-3).cuda()
    for xx, gg, what in ((torch.zeros_like(x), gy, "x"), (x, torch.zeros_like(gy), "gy"), (torch.zeros_like(x), torch.zeros_like(gy), "x and gy")):
        exact("weight gradient of %s == 0" % what, wgrad_x3(K, xx, gg, prec, kernel=kernel), torch.zeros_like(gw0))
        exact("accumulating weight gradient of %s == 0" % what, wgrad_x3(K, xx, gg, prec, gw=gw0, kernel=kernel), gw0)
        if prec == 4:
            for t in (xx, gg):
                assert t._bh_amax.max().item() == t.abs().max().item() and (t._bh_amax >= 0).all()


@pytest.mark.parametrize("prec,route_x3", [(0, False), (4, True)])
@pytest.mark.parametrize("N,Hi,Wi,Ci,Co,k,s,p", [(2, 16, 24, 64, 128, 1, 2, 0), (2, 16, 32, 64, 128, 3, 2, 1)])
def test_zero_operand_generic_kernel(K, N, Hi, Wi, Ci, Co, k, s, p, prec, route_x3):
    """exact.  conv_gemm_kernel (fp32-input MFMA; three bf16 pieces) and the generic weight gradient on all-zero operands."""
    from bihome_amd._lib import ROUTE_GENERIC_CONV, ROUTE_GEMM_X3
    d = K.conv_desc(N, Hi, Wi, Ci, Co, k, s, p, precision=prec, route=ROUTE_GENERIC_CONV | (ROUTE_GEMM_X3 if route_x3 else 0))
    for which in ("fwd", "dgrad"):
        v = K.conv_variant(d, which)
        assert v.startswith("conv_gemm_kernel<") and (len(v.split(",")) == 7 and v.endswith(",true>")) == route_x3, v
    x = torch.tensor(C.rnd((N, Hi, Wi, Ci), 1)).cuda()
    w = torch.tensor((C.rnd((Co, k, k, Ci), 2) / np.sqrt(Ci * k * k)).astype(np.float32)).cuda()
    b = torch.tensor(C.rnd((Co,), 3)).cuda()
    gy = torch.tensor(C.rnd((N, d.Ho, d.Wo, Co), 4)).cuda()
    zx, zg, zw = torch.zeros_like(x), torch.zeros_like(gy), torch.zeros_like(w)
    for xx, ww, what in ((zx, w, "x"), (x, zw, "w")):
        exact("forward of %s == 0" % what, K.conv_fwd(xx, ww, b, d), b.expand(N, d.Ho, d.Wo, Co))
    for gg, ww, what in ((zg, w, "gy"), (gy, zw, "w")):
        exact("dgrad of %s == 0" % what, K.conv_dgrad(gg, ww, d), zx)
        exact("accumulating dgrad of %s == 0" % what, K.conv_dgrad(gg, ww, d, out=x.clone()), x)
    for xx, gg, what in ((zx, gy, "x"), (x, zg, "gy")):
        gw, gb = w.clone(), b.clone()
        K.conv_wgrad(xx, gg, gw, gb, d)
        exact("accumulating weight gradient of %s == 0" % what, gw, w)
        if gg is zg:
            exact("accumulating bias gradient of gy == 0", gb, b)


@pytest.mark.parametrize("Ci", [1, 2])
def test_zero_operand_stem_forward(K, Ci):
    """exact.  stem7_fwd_f16_kernel on an all-zero image (every tile's scale comes from a maximum of 0) and on an all-zero filter bank."""
    N = 16
    d = _stem_fwd(K, N, Ci)
    g = torch.Generator().manual_seed(7 + Ci)
    x = torch.randn(N, 64, 64, 1, generator=g).cuda() if Ci == 1 else torch.randn(N, Ci, 64, 64, generator=g).cuda()
    w = (torch.randn(64, 7, 7, Ci, generator=g) * 0.1).cuda()
    b = torch.randn(64, generator=g).cuda()
    for xx, ww, what in ((torch.zeros_like(x), w, "x"), (x, torch.zeros_like(w), "w")):
        exact("stem forward of %s == 0" % what, K.conv_fwd(xx, ww, b, d), b.expand(N, 32, 32, 64))


@pytest.mark.parametrize("prec", [4, 0])
def test_zero_operand_stem_dgrad(K, prec):
    """exact.  bh_stem7_dgrad_c1 on gy == 0 and on w == 0: the gradient image is 0 everywhere (it is overwritten: NaN before the call)."""
    N = 4
    g = torch.Generator().manual_seed(21)
    gy = torch.randn(N, 32, 32, 64, generator=g).cuda()
    w = (torch.randn(64, 7, 7, 1, generator=g) / 7).cuda()
    zero = torch.zeros(N, 64, 64, 1, device="cuda")
    exact("stem dgrad of gy == 0", _stem_dgrad(K, torch.zeros_like(gy), w, prec, N), zero)
    exact("stem dgrad of w == 0", _stem_dgrad(K, gy, torch.zeros_like(w), prec, N), zero)


def _one_hot_cases(N, H, W):
    # (image, row, column): a tile corner of the first image (8 x 8 output tiles: (7, 7) | (8, 8) where the map has more than one tile),
    # and the last pixel of the last image
    return [(0, min(8, H - 1), min(8, W - 1)), (N - 1, H - 1, W - 1)]


@pytest.mark.parametrize("which", [0, 1, 4])
def test_one_hot_gradient_dgrad(K, which):
    """measured (the square test's bound: err[4] <= 1.5 err[0] against float64, test_f16x2_gpu.py - here against the fp32-input MFMA halo
    kernel on the same data).  gy is nonzero in ONE pixel of one image - a hinge active in one place: the record is that pixel's maximum,
    every other tile multiplies zeros."""
    name, make = _layers(K)[which]
    layer = make()
    N, H, W, Ci, Co = layer.shape
    base = _halo(K, N, H, W, Ci, Co, 0)
    x, gy, w, b = layer.data()
    for n, i, j in _one_hot_cases(N, H, W):
        g1 = torch.zeros_like(gy)
        g1[n, i, j] = gy[n, i, j]
        ref = F.conv_transpose2d(g1.double().cpu().permute(0, 3, 1, 2), w.double().cpu(), None, 1, 1).permute(0, 2, 3, 1)
        gx, gx0 = layer.dgrad(g1, w), base.dgrad(g1, w)
        e4, e0 = rel_l2(gx, ref), rel_l2(gx0, ref)
        MEASURED.append(("%s dgrad, one-hot gy at %s: rel-L2 vs f64" % (name, (n, i, j)), "%.2e" % e4, "1.5 x fp32-input MFMA's %.2e" % e0))
        assert e4 <= 1.5 * e0, (e4, e0)
        exact("%s dgrad outside the pixel's 3 x 3 neighbourhood" % name, gx * (ref == 0).cuda(), torch.zeros_like(gx))


@pytest.mark.parametrize("N,H,Ci,Co", [(2, 8, 64, 64), (4, 16, 64, 64)])
def test_one_hot_gradient_wgrad_x3(K, N, H, Ci, Co):
    """derived.  With gy nonzero in one pixel every entry of gw is ONE product x[n, i + kh - 1, j + kw - 1, ci] gy[n, i, j, co]: there is no
    sum whose fp32 accumulation rounding would cover the pieces' own error, and check_wgrad_f16x2_kernel's comparison with the fp32-input
    MFMA kernel (err[4] <= 1.5 err[0] + 1e-8; that kernel rounds an exact product once) does not apply - measured on the MI355X, rel-L2
    against float64: fp16 pieces 9.0e-8 / 7.7e-8 on the two shapes, fp32-input MFMA 2.5e-8.  That is the documented arithmetic
    (csrc/common.h F16X2, include/bihome.h bh_conv_desc.a_bound), and the bound held here is the one it states, per product a b:
      each operand is cut into 11 + 11 bits, |e| <= 2^-23 of the element (2 x 2^-23), or - for elements below 2^-18 of the tensor's record -
      2^-25 in scaled units, i.e. 2^-39 of the record; the dropped lo x lo is <= 2^-22 |a b|; one fp32 rounding of the sum of the three
      piece products, 2^-24:  |err| <= (2^-22 + 2^-22 + 2^-24) |a b| + 2^-39 (|a| max |gy| + |b| max |x|), with 1.25 x 2^-21 for the first
      factor (second-order terms)."""
    g = torch.Generator().manual_seed(N + H + Ci)
    x = torch.randn(N, H, H, Ci, generator=g).cuda()
    gy = (torch.randn(N, H, H, Co, generator=g) * 3e-5).cuda()
    xd = x.double().cpu().permute(0, 3, 1, 2)
    for n, i, j in _one_hot_cases(N, H, H):
        g1 = torch.zeros_like(gy)
        g1[n, i, j] = gy[n, i, j]
        wz = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xd, wz, None, 1, 1)
        ref = torch.autograd.grad(y, wz, g1.double().cpu().permute(0, 3, 1, 2), retain_graph=True)[0].permute(0, 2, 3, 1)
        xa = torch.autograd.grad(y, wz, (g1 != 0).double().cpu().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1).abs()      # the x of each entry
        ga = g1[n, i, j].double().cpu().abs().reshape(Co, 1, 1, 1)
        bound = 1.25 * 2.0 ** -21 * ref.abs() + 2.0 ** -39 * (xa * ga.max() + ga * xd.abs().max()) * (xa != 0)
        gw = wgrad_x3(K, x, g1, 4).cpu().double()
        err = (gw - ref).abs()
        MEASURED.append(("wgrad_x3 f16x2, one-hot gy at %s: largest |err| / derived bound over the entries" % ((n, i, j),),
                         "%.3f (rel-L2 vs f64 %.2e)" % ((err / bound.clamp_min(1e-300)).max().item(), rel_l2(gw, ref)), "1, derived"))
        assert (err <= bound).all()
        assert (gw[ref == 0] == 0).all()                                  # taps outside the image: exactly 0


def test_one_hot_gradient_stem_dgrad(K):
    """measured (test_gray_stem_dgrad_in_fp16_pieces' bound: err[4] <= 1.5 err[0] + 1e-8 against float64), and bh_stem7_dgrad_c1_warp
    against the two calls it replaces (its square test's bound: 1e-5 of the largest entry; the gradient image bit for bit)."""
    from bihome_amd._lib import check, lib
    N, size = 4, 64
    g = torch.Generator().manual_seed(21)
    gy = torch.randn(N, 32, 32, 64, generator=g)
    w = torch.randn(64, 1, 7, 7, generator=g) / 7
    wk = w.permute(0, 2, 3, 1).contiguous().cuda()
    rng = np.random.Generator(np.random.PCG64(N * 7 + size))
    src = F.avg_pool2d(torch.tensor(rng.standard_normal((N, 1, size, size)).astype(np.float32)), 3, 1, 1).cuda().contiguous()
    H64, _ = K.h4pt_fwd(HK.dev(HK.rand_delta(N, size + 1, amp=size / 4.0)), (size, size))
    for n, i, j in [(0, 8, 8), (N - 1, 31, 31)]:
        g1 = torch.zeros_like(gy)
        g1[n, i, j] = gy[n, i, j]
        xt = torch.zeros(N, 1, size, size, dtype=torch.float64, requires_grad=True)
        F.conv2d(xt, w.double(), None, stride=2, padding=3).backward(g1.double().permute(0, 3, 1, 2))
        gx = {prec: _stem_dgrad(K, g1.cuda(), wk, prec, N) for prec in (0, 4)}
        e = {prec: rel_l2(gx[prec].reshape(N, 1, size, size), xt.grad) for prec in (0, 4)}
        MEASURED.append(("stem dgrad in fp16 pieces, one-hot gy at %s: rel-L2 vs f64" % ((n, i, j),), "%.2e" % e[4], "1.5 x fp32-input MFMA's %.2e + 1e-8" % e[0]))
        assert e[4] <= 1.5 * e[0] + 1e-8, e
        exact("stem dgrad outside the pixel's 7 x 7 footprint", gx[4].reshape(N, 1, size, size) * (xt.grad == 0).cuda(), torch.zeros(N, 1, size, size, device="cuda"))
        # the fused form against the two calls
        d = K.conv_desc(N, size, size, 1, 64, 7, 2, 3, precision=4)
        base = torch.tensor(rng.standard_normal((N, 9))).cuda()
        gH0 = K.warp_bwd(src, H64, gx[4].view(N, 1, size, size), None, 4, gH=base.clone())
        gx1 = torch.full((N, size, size, 1), float("nan"), device="cuda")
        gH1 = base.clone()
        check(lib.bh_stem7_dgrad_c1_warp(_p(g1.cuda()), _p(wk), _p(gx1), ctypes.byref(d), _p(src), _p(H64), None, 4, _p(gH1), _stream()), "bh_stem7_dgrad_c1_warp")
        exact("fused stem dgrad + warp adjoint: the gradient image", gx1, gx[4])
        scale, err = (gH0 - base).abs().max().item(), (gH1 - gH0).abs().max().item()
        MEASURED.append(("fused stem dgrad + warp adjoint, one-hot gy at %s: max |gH - two calls|" % ((n, i, j),), "%.3e" % err, "1e-5 of %.3e" % scale))
        assert err <= 1e-5 * scale, (err, scale)
        exact("samples without a gradient keep their dL/dH", (gH1 - base)[[b for b in range(N) if b != n]], torch.zeros(N - 1, 9, dtype=torch.float64, device="cuda"))


def test_wide_operands_wgrad_f16x2(K):
    """measured (check_wgrad_f16x2_kernel's own bound, err[4] <= 1.5 err[0] + 1e-8 and < 0.25 err[3], through that helper).  x and gy
    spread over 24 binades, as check_conv3x3_f16x2_forward_and_dgrad(wide=True) spreads them for forward and dgrad."""
    def wide(x, gy, g):
        return (x * torch.exp2(torch.randint(-12, 12, x.shape, generator=g).float()),
                gy * torch.exp2(torch.randint(-12, 12, gy.shape, generator=g).float()))
    F16.check_wgrad_f16x2_kernel(K, 8, 16, 16, 64, 64, values=wide)


def _field(H, W, n, i, j, k=3):
    """[H][W] bool: the outputs of a k x k / stride-1 / same-padding layer whose receptive field holds pixel (i, j)."""
    m = torch.zeros(H, W, dtype=torch.bool)
    r = k // 2
    m[max(i - r, 0):i + r + 1, max(j - r, 0):j + r + 1] = True
    return m


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_element_is_loud_3x3(K, bad):
    """exact (a property, no tolerance).  A NaN or +inf in ONE element of x (then of gy): the fp16-piece forward (halo and persistent kernel)
    and the weight gradient are non-finite at every output whose receptive field holds the element.  The magnitude pass keeps an inf (k = 0,
    the inf reaches the products) and drops a NaN (the scale comes from the finite rest; NaN 2^k is NaN): both routes end loud.  Nothing is
    claimed about the other outputs."""
    for layer in (_halo(K, 2, 8, 8, 64, 64, 4), _persistent(K)):
        N, H, W, Ci, Co = layer.shape
        x, gy, w, b = layer.data()
        n, i, j, c = N - 1, 3, H - 1, 5
        xb = x.clone()
        xb[n, i, j, c] = bad
        y = layer.fwd(xb, w, b)
        assert not torch.isfinite(y[n][_field(H, W, n, i, j)]).any()
        gb_ = gy.clone()
        gb_[n, i, j, c] = bad
        gx = layer.dgrad(gb_, w)
        assert not torch.isfinite(gx[n][_field(H, W, n, i, j)]).any()
    N, H, Ci, Co = 2, 8, 64, 64
    g = torch.Generator().manual_seed(N + H + Ci)
    x = torch.randn(N, H, H, Ci, generator=g).cuda()
    gy = (torch.randn(N, H, H, Co, generator=g) * 3e-5).cuda()
    xb = x.clone()
    xb[1, 3, 4, 5] = bad                                        # interior pixel: all nine taps see it
    assert not torch.isfinite(wgrad_x3(K, xb, gy, 4)[:, :, :, 5]).any()
    gb_ = gy.clone()
    gb_[1, 3, 4, 5] = bad
    assert not torch.isfinite(wgrad_x3(K, x, gb_, 4)[5]).any()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_element_is_loud_stem(K, bad):
    """exact (a property).  The fp16-piece stem: every output whose 7 x 7 / stride-2 window holds the element is non-finite."""
    N = 16
    d = _stem_fwd(K, N, 1)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(N, 64, 64, 1, generator=g).cuda()
    w = (torch.randn(64, 7, 7, 1, generator=g) * 0.1).cuda()
    i, j = 33, 16                                                # (a tile border column)
    x[N - 1, i, j, 0] = bad
    y = K.conv_fwd(x, w, None, d)
    # output (a, b) reads rows 2a - 3 ... 2a + 3
    rows = [a for a in range(32) if 2 * a - 3 <= i <= 2 * a + 3]
    cols = [c for c in range(32) if 2 * c - 3 <= j <= 2 * c + 3]
    assert not torch.isfinite(y[N - 1][rows][:, cols]).any()


# ------------------------------------------------------------------------------------------------
# 3. bh_absmax, directly
# ------------------------------------------------------------------------------------------------
def _absmax(x, n=None, rec=None):
    from bihome_amd._lib import AMAX_FLOATS, lib
    rec = torch.zeros(AMAX_FLOATS, device="cuda") if rec is None else rec
    rc = lib.bh_absmax(_p(x), ctypes.c_longlong(x.numel() if n is None else n), _p(rec), _stream())
    return rc, rec


@pytest.mark.parametrize("n", V.ABSMAX_LENGTHS)
def test_absmax(K, n):
    """exact.  record.max() == max |x| and all 512 floats are non-negative, for the maximum in the first element, in the last element
    of the float4 part, in the last element (of the scalar tail, where n & 3), negative, and subnormal; all zeros including -0.0 leave +0."""
    from bihome_amd._lib import AMAX_FLOATS
    g = torch.Generator().manual_seed(n % 1000)
    base = torch.randn(n, generator=g).clamp_(-3, 3)
    for pos in sorted({0, max(n // 4 * 4 - 1, 0), n - 1}):
        for peak in (7.5, -7.5):
            x = base.clone()
            x[pos] = peak
            rc, rec = _absmax(x.cuda())
            assert rc == 0 and rec.numel() == AMAX_FLOATS
            assert rec.max().item() == 7.5 and (rec.view(torch.int32) >= 0).all(), (n, pos, peak, rec.max().item())
        x = torch.zeros(n)
        x[pos] = -1e-40                                         # subnormal: |x| has to arrive, not 0
        rc, rec = _absmax(x.cuda())
        assert rc == 0 and rec.max().item() == float(np.float32(1e-40)) and (rec.view(torch.int32) >= 0).all(), (n, pos, rec.max().item())
    x = torch.zeros(n)
    x[::2] = -0.0
    rc, rec = _absmax(x.cuda())
    assert rc == 0 and (rec.view(torch.int32) == 0).all()       # +0, bit for bit
    rc, rec = _absmax(base.cuda())
    assert rc == 0 and rec.max().item() == base.abs().max().item()
    MEASURED.append(("n = %d" % n, "record == max |x| at %d positions of the maximum" % len({0, max(n // 4 * 4 - 1, 0), n - 1}), "exact"))


def test_absmax_combines_with_an_earlier_bound(K):
    """exact.  "the record must be zeroed (or hold an earlier bound to be combined with)", include/bihome.h: a second call on a smaller
    tensor leaves the record as it is, one on a larger tensor raises it."""
    g = torch.Generator().manual_seed(5)
    a = torch.randn(2048 * 4 * 8 + 7, generator=g).cuda()
    rc, rec = _absmax(a)
    before = rec.clone()
    rc2, _ = _absmax(a[:1024] * 0.5, rec=rec)
    assert rc == 0 and rc2 == 0 and torch.equal(rec, before)
    rc3, _ = _absmax((a * 4.0)[:1027].contiguous(), rec=rec)
    assert rc3 == 0 and rec.max().item() == max(before.max().item(), (a[:1027] * 4.0).abs().max().item()) and (rec >= before).all()
    MEASURED.append(("combined record", "%.6g after %.6g" % (rec.max().item(), before.max().item()), "exact"))


def test_absmax_bad_arguments(K):
    """exact.  n < 0 and a pointer off 16 bytes are BH_E_BADARG (-1) without a launch: the record stays as it was."""
    x = torch.ones(64, device="cuda")
    rc, rec = _absmax(x, n=-1)
    assert rc == -1 and (rec == 0).all()
    rc, rec = _absmax(x[1:], n=8)
    assert x[1:].data_ptr() % 16 == 4 and rc == -1 and (rec == 0).all()
    rc, rec = _absmax(x, n=0)
    assert rc == 0 and (rec == 0).all()


# ------------------------------------------------------------------------------------------------
# 4. BatchNorm on channels that are not N(0.1, 1.2^2)
# ------------------------------------------------------------------------------------------------
# Forward: derived (V.bn_forward_bound).  Backward: measured - per channel, against float64 autograd of the two-pass BatchNorm, within
# max(3 x the distance of torch's float32 BatchNorm autograd from float64 on the same data, 3e-5 of the channel's largest gradient): the
# margin of test_backbone_forward_backward_vs_oracle for the same kind of yardstick, the floor of the square tests.
# MEASURED on the MI355X, worst channel of every case (`pytest -s`): forward 0.29 ... 0.37 of the derived bound (torch's float32 BatchNorm on
# the same data: 0.28 ... 0.51); gx 1.9e-7 ... 1.2e-6 of the channel's largest gradient where torch float32 is 2.0e-7 ... 1.2e-6 from float64
# - the worst channel is always one of the two with mean +-1000 -, the sums_ready form 2.5e-6 (float32: 1.4e-6; the sums pass through the
# conv epilogue's own rounding of the gradient); BatchNorm-on-load convs 0.012 ... 0.014 of their bound.  Every case sits at the 3e-5 floor.
C32 = V.BN_C


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _bn_autograd(x, gamma, beta, groups, res, relu, gy, dtype, xb=None, gamma_b=None, beta_b=None):
    """(gx, ggamma, gbeta, gres | gxb ...) of act(bn(x) [+ res | + bn_b(xb)]) for the output gradient gy.  float64: the two-pass reference
    (V.bn_reference); float32: torch's own BatchNorm (F.batch_norm per group) - the yardstick."""
    leaves = [t.to(dtype).clone().requires_grad_(True) if t is not None else None for t in (x, gamma, beta, res, xb, gamma_b, beta_b)]
    xt, gt, bt, rt, xbt, gbt, bbt = leaves

    def bn(a, g_, b_):
        if dtype == torch.float64:
            return V.bn_reference(a, g_, b_, groups)["pre"]
        n = a.shape[0] // groups
        return torch.cat([F.batch_norm(_nchw(a[i * n:(i + 1) * n]), None, None, g_, b_, True, 0.1, V.BN_EPS).permute(0, 2, 3, 1)
                          for i in range(groups)], 0)
    pre = bn(xt, gt, bt)
    if rt is not None:
        pre = pre + rt
    if xbt is not None:
        pre = pre + bn(xbt, gbt, bbt)
    (pre.clamp_min(0) if relu else pre).backward(gy.to(dtype))
    return [t.grad if t is not None else None for t in leaves]


def _per_channel(what, got, r64, r32, floor_scale=None):
    """measured: per channel, |got - float64| <= max(3 |float32 - float64|, 3e-5 of the channel's largest float64 gradient)."""
    Cn = r64.shape[-1]
    g, a, b = (t.detach().cpu().double().reshape(-1, Cn) for t in (got, r64, r32))
    scale = a.abs().amax(0) if floor_scale is None else floor_scale.detach().double().reshape(Cn)
    err, spread = (g - a).abs().amax(0), (b - a).abs().amax(0)
    bound = torch.maximum(3 * spread, 3e-5 * scale)
    c = int((err / bound.clamp_min(1e-300)).argmax())
    MEASURED.append((what, "worst channel %d: |err| %.3e = %.2e of its largest gradient %.3e (torch float32: %.2e of it); channels 2 / 3 (mean +-1000): %.2e / %.2e"
                     % (c, err[c], err[c] / max(scale[c].item(), 1e-300), scale[c], spread[c] / max(scale[c].item(), 1e-300),
                        err[2] / max(scale[2].item(), 1e-300), err[3] / max(scale[3].item(), 1e-300)),
                     "max(3 x torch float32's distance from float64, 3e-5 of the largest gradient), per channel"))
    assert torch.isfinite(got).all() and (err <= bound).all(), (what, c, err[c].item(), bound[c].item())


def _param_scales(x, ref, gy, groups, pre=None):
    """Per channel, the size of the terms the parameter gradients add up: (sum |d xhat|, sum |d|) with d = gy [pre > 0] (pre: the ReLU's
    input, None without a ReLU) - the floor of ggamma / gbeta is 3e-5 of THESE, channel by channel, so that a channel cannot hide
    behind the others (a dead channel and the xhat = 0 of a constant channel have scale 0: exact)."""
    Cn = x.shape[-1]
    d = gy.double() * (pre.detach() > 0) if pre is not None else gy.double()
    xg = x.double().reshape(groups, -1, Cn)
    xhat = ((xg - ref["mean"][:, None]) / torch.sqrt(ref["var"][:, None] + V.BN_EPS)).reshape(x.shape)
    return (d * xhat).abs().reshape(-1, Cn).sum(0), d.abs().reshape(-1, Cn).sum(0)


def _derived(what, got, ref, bound, f32=None):
    err = (got.detach().cpu().double() - ref.detach()).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    ctx = "" if f32 is None else "; torch float32 BatchNorm on the same data: %.3f" % ((f32.double() - ref.detach()).abs() / bound.clamp_min(1e-300)).max().item()
    MEASURED.append((what, "largest |err| / bound %.3f%s" % (ratio, ctx), "1, derived"))
    assert torch.isfinite(got).all() and (err <= bound).all(), (what, ratio)


def _record_is(rec, t):
    assert rec.max().item() == t.abs().max().item() and (rec.view(torch.int32) >= 0).all(), (rec.max().item(), t.abs().max().item())


def _gy_for(ref, relu, seed):
    """A random output gradient, zero where the float64 ReLU input is within NEAR of 0 (at most 1 % of the elements)."""
    gy = torch.randn(ref["pre"].shape, generator=torch.Generator().manual_seed(seed))
    if relu:
        near = V.near_relu(ref["pre"])
        assert near.double().mean().item() <= 0.01
        gy[near] = 0
    return gy


def _dead_and_constant(relu, y, gx, gg, gb, beta):
    """exact expectations.  Dead channel (under ReLU): output, gx, ggamma, gbeta exactly 0; constant channels: finite everywhere."""
    if relu:
        assert (y[..., V.BN_DEAD] == 0).all() and (gx[..., V.BN_DEAD] == 0).all() and gg[V.BN_DEAD].item() == 0 and gb[V.BN_DEAD].item() == 0
    for t in (y, gx, gg, gb):
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("groups,N,H,W", V.BN_SHAPES)
def test_batchnorm_fwd_bwd_on_hand_set_channels(K, groups, N, H, W, relu, res):
    """bh_bn_fwd (training) and bh_bn_bwd: the plain form that reads y (ReLU + residual), the mask-from-z form (ReLU, no residual), and -
    on 16 x 16 - the sums_ready form fed by bh_conv_dgrad_bnreduce; running statistics; the measured records."""
    x, gamma, beta = V.bn_channels(groups, N, H, W)
    r = torch.randn(N, H, W, C32, generator=torch.Generator().manual_seed(3)) if res else None
    ref = V.bn_reference(x, gamma, beta, groups, r, relu)
    xg, gm, bt, rg = _cu(x), _cu(gamma), _cu(beta), _cu(r)
    rm0 = 0.1 * torch.randn(C32, generator=torch.Generator().manual_seed(4))
    rv0 = 1 + 0.2 * torch.rand(C32, generator=torch.Generator().manual_seed(5))
    rm, rv = _cu(rm0), _cu(rv0)
    rec = K.amax_record("cuda")
    y, st = K.bn_fwd(xg, gm, bt, rm, rv, rg, groups, V.BN_EPS, 0.1, relu, True, amax=rec)
    n = N // groups
    y32 = torch.cat([F.batch_norm(_nchw(x[i * n:(i + 1) * n]), None, None, gamma, beta, True, 0.1, V.BN_EPS).permute(0, 2, 3, 1) for i in range(groups)], 0)
    y32 = y32 + r if res else y32
    y32 = y32.clamp_min(0) if relu else y32
    _derived("bn_fwd", y, ref["y"], V.bn_forward_bound(x, ref, r), y32)
    tight = V.bn_forward_bound(x, ref, r, shift_rounded_once=True)
    MEASURED.append(("bn_fwd against the bound of a shift rounded once from float64 (context)", "largest |err| / bound %.3f; torch float32: %.3f" % (
        ((y.cpu().double() - ref["y"]).abs() / tight).max().item(), ((y32.double() - ref["y"]).abs() / tight).max().item()), "not asserted"))
    _record_is(rec, y)
    # running statistics.  derived: one fp32 update rm = (1 - m) rm + m (float) mean per group, three roundings of terms no larger than
    # |rm| + |mean| each: 4 * 2^-24 (|rm0| + max |statistic|) per group
    rows = N * H * W // groups
    rm64, rv64 = rm0.double(), rv0.double()
    for i in range(groups):
        rm64, rv64 = 0.9 * rm64 + 0.1 * ref["mean"][i], 0.9 * rv64 + 0.1 * ref["var"][i] * rows / (rows - 1)
    _derived("running_mean", rm, rm64, groups * 4 * 2.0 ** -24 * (rm0.double().abs() + ref["mean"].abs().amax(0)))
    _derived("running_var", rv, rv64, groups * 4 * 2.0 ** -24 * (rv0.double().abs() + ref["var"].amax(0) * rows / (rows - 1)) + 1e-300)
    # adjoint
    gy = _gy_for(ref, relu, 6)
    g64 = _bn_autograd(x, gamma, beta, groups, r, relu, gy, torch.float64)
    g32 = _bn_autograd(x, gamma, beta, groups, r, relu, gy, torch.float32)
    gg, gb = torch.zeros(C32, device="cuda"), torch.zeros(C32, device="cuda")
    recb = K.amax_record("cuda")
    gx, gres = K.bn_bwd(_cu(gy), y, xg, gm, st, rm, rv, groups, V.BN_EPS, relu, True, res, gg, gb, beta=bt, amax=recb)
    sg, sb_ = _param_scales(x, ref, gy, groups, ref["pre"] if relu else None)
    _per_channel("gx", gx, g64[0], g32[0])
    _per_channel("ggamma", gg, g64[1], g32[1], floor_scale=sg)
    _per_channel("gbeta", gb, g64[2], g32[2], floor_scale=sb_)
    _record_is(recb, gx)
    if res:
        exact("gres is the masked gy", gres, _cu(gy * (ref["pre"] > 0)) if relu else _cu(gy))
    _dead_and_constant(relu, y, gx, gg, gb, bt)
    if not res:                                                  # constant channels: y = beta, within the derived bound (checked above) of it
        for c in (V.BN_CONSTANT, V.BN_ZERO):
            assert (ref["y"][..., c] == float(beta[c])).all()
    if H == 16 and relu:
        # the sums_ready form: the BatchNorm's output gradient is the dgrad of a 3x3 conv, whose epilogue accumulates the backward sums
        from bihome_amd._lib import ROUTE_HALO_SMALL
        assert not V.near_relu(ref["pre"]).any()
        d = K.conv_desc(N, H, W, C32, 32, 3, 1, 1, route=ROUTE_HALO_SMALL)
        assert K.dgrad_bn_reduce_ok(d) and K.conv_variant(d, "dgrad_bnr_y" if res else "dgrad_bnr_z", bn_groups=groups).startswith("conv3x3_halo_kernel<true,")
        gen = torch.Generator().manual_seed(8)
        w, go = _cu(torch.randn(32, 3, 3, C32, generator=gen) * 0.1), _cu(torch.randn(N, H, W, 32, generator=gen))
        sums = K.bn_stats_buffer(groups, C32, "cuda")
        red = dict(z=xg, y=y if res else None, stats=st, gamma=gm, beta=bt, eps=V.BN_EPS, relu=relu, sums=sums, groups=groups)
        g_f = K.conv_dgrad(go, w, d, bn_reduce=red)
        exact("the dgrad with the sums in its epilogue", g_f, K.conv_dgrad(go, w, d))
        g64 = _bn_autograd(x, gamma, beta, groups, r, relu, g_f.cpu(), torch.float64)
        g32 = _bn_autograd(x, gamma, beta, groups, r, relu, g_f.cpu(), torch.float32)
        gg1, gb1 = torch.zeros(C32, device="cuda"), torch.zeros(C32, device="cuda")
        gx1, _ = K.bn_bwd(g_f, y, xg, gm, st, rm, rv, groups, V.BN_EPS, relu, True, res, gg1, gb1, beta=bt, sums_ready=sums)
        _per_channel("gx (sums_ready)", gx1, g64[0], g32[0])
        sg, sb_ = _param_scales(x, ref, g_f.cpu(), groups, ref["pre"])
        _per_channel("ggamma (sums_ready)", gg1, g64[1], g32[1], floor_scale=sg)
        _per_channel("gbeta (sums_ready)", gb1, g64[2], g32[2], floor_scale=sb_)
        _dead_and_constant(relu, y, gx1, gg1, gb1, bt)


@pytest.mark.parametrize("groups,N,H,W", V.BN_SHAPES)
def test_batchnorm_on_load_on_hand_set_channels(K, groups, N, H, W):
    """bh_bn_fwd_coeffs + bh_conv_fwd_bnin: the 1x1 layer on the generic kernel and - on 16 x 16 - the packed 3x3 layer at precision 2 and 4.
    derived: every input of the conv carries the BatchNorm's forward error e (V.bn_forward_bound: the table form's, 6e-5 absolute on the
    mean +-1000 channels), the conv adds its own rounding - |out - out64| <= conv(e, |w|) + 3e-5 max |out64| (the square tests' 3e-5)."""
    from bihome_amd._lib import ROUTE_HALO_SMALL
    x, gamma, beta = V.bn_channels(groups, N, H, W)
    ref = V.bn_reference(x, gamma, beta, groups, None, True)
    e_in = V.bn_forward_bound(x, ref)
    xg, gm, bt = _cu(x), _cu(gamma), _cu(beta)
    st = K.bn_stats(xg, K.bn_stats_buffer(groups, C32, "cuda"), groups, C32)
    rec = K.amax_record("cuda")
    table = K.bn_fwd_coeffs(st, gm, bt, torch.zeros(C32, device="cuda"), torch.ones(C32, device="cuda"), groups, N * H * W // groups, C32, V.BN_EPS, 0.1, amax=rec)
    assert rec.max().item() >= ref["y"].abs().max().item() and torch.isfinite(table).all()
    bol = K.BnOnLoad(xg, table, groups, True, amax=rec)
    gen = torch.Generator().manual_seed(9)
    if H != 16:
        # 140 rows per image: the on-load 1x1 form takes groups of a multiple of 128 rows, the 3x3 kernel maps of 8 x 8 tiles - refused, not guessed
        d = K.conv_desc(N, H, W, C32, 16, 1, 1, 0)
        with pytest.raises(Exception, match="BH_E_UNSUPPORTED"):
            K.conv_fwd(bol, torch.zeros(16, 1, 1, C32, device="cuda"), None, d)
        return
    cases = [(1, 16, 0, None), (3, 32, 2, "conv3x3_halo_kernel<false,"), (3, 32, 4, "conv3x3_halo_kernel<false,")]
    for k, Co, prec, kernel in cases:
        w = (torch.randn(Co, C32, k, k, generator=gen) * 0.1).contiguous(memory_format=torch.channels_last)
        out64 = F.conv2d(_nchw(ref["y"]), w.double(), None, 1, k // 2).permute(0, 2, 3, 1)
        bound = F.conv2d(_nchw(e_in), w.double().abs(), None, 1, k // 2).permute(0, 2, 3, 1) + 3e-5 * out64.abs().max()
        d = K.conv_desc(N, H, W, C32, Co, k, 1, k // 2, precision=prec, route=ROUTE_HALO_SMALL)
        wg = w.cuda()
        if kernel:
            assert K.conv_variant(K._with_layout(d, K.packed_layout(prec)), "fwd").startswith(kernel)
            _, pf, _ = F16._packed(K, wg, prec)
            out = K.conv_fwd(bol, wg.permute(0, 2, 3, 1), None, d, wpacked=pf)
        else:
            assert K.conv_variant(d, "fwd").startswith("conv_gemm_kernel<")
            out = K.conv_fwd(bol, wg.permute(0, 2, 3, 1), None, d)
        _derived("conv %dx%d behind BatchNorm-on-load, precision %d" % (k, k, prec), out, out64, bound)


@pytest.mark.parametrize("groups,N,H,W", V.BN_SHAPES)
def test_batchnorm_maxpool_on_hand_set_channels(K, groups, N, H, W):
    """bh_bn_maxpool_fwd / bh_bn_maxpool_bwd.  Forward derived: a window maximum moves by no more than its largest input does -
    maxpool(V.bn_forward_bound); adjoint measured per channel, the pooled gradient scattered through the kernel's own arg-max positions
    (the constant channels are nothing but ties)."""
    x, gamma, beta = V.bn_channels(groups, N, H, W)
    ref = V.bn_reference(x, gamma, beta, groups, None, True)
    assert not V.near_relu(ref["pre"]).any()
    xg, gm, bt = _cu(x), _cu(gamma), _cu(beta)
    rm, rv = torch.zeros(C32, device="cuda"), torch.ones(C32, device="cuda")
    rec, recb = K.amax_record("cuda"), K.amax_record("cuda")
    st = K.bn_stats_buffer(groups, C32, "cuda")
    fused = K.bn_maxpool_fwd(xg, gm, bt, rm, rv, groups, V.BN_EPS, 0.1, True, True, st, False, amax=rec)
    p64 = F.max_pool2d(_nchw(ref["y"]), 3, 2, 1).permute(0, 2, 3, 1)
    _derived("pooled", fused.pooled, p64, F.max_pool2d(_nchw(V.bn_forward_bound(x, ref)), 3, 2, 1).permute(0, 2, 3, 1))
    _record_is(rec, fused.pooled)
    assert (fused.pooled[..., V.BN_DEAD] == 0).all()
    gp = torch.randn(p64.shape, generator=torch.Generator().manual_seed(10))
    gy = K.maxpool_bwd(fused.idx, _cu(gp), fused.shape).cpu()
    g64 = _bn_autograd(x, gamma, beta, groups, None, True, gy, torch.float64)
    g32 = _bn_autograd(x, gamma, beta, groups, None, True, gy, torch.float32)
    gg, gb = torch.zeros(C32, device="cuda"), torch.zeros(C32, device="cuda")
    gx = K.bn_maxpool_bwd(K.PooledGrad(_cu(gp), fused.idx), xg, gm, bt, st, rm, rv, groups, V.BN_EPS, True, True, gg, gb, amax=recb)
    sg, sb_ = _param_scales(x, ref, gy, groups, ref["pre"])
    _per_channel("gx", gx, g64[0], g32[0])
    _per_channel("ggamma", gg, g64[1], g32[1], floor_scale=sg)
    _per_channel("gbeta", gb, g64[2], g32[2], floor_scale=sb_)
    _record_is(recb, gx)
    _dead_and_constant(True, fused.pooled, gx, gg, gb, bt)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("groups,N,H,W", V.BN_SHAPES)
def test_batchnorm_join_on_hand_set_channels(K, groups, N, H, W, relu):
    """bh_bn_join_fwd / bh_bn_join_bwd, both branches with the hand-set channels.  Forward derived: y = fma(xa, sc_a, fma(xb, sc_b, sh_a + sh_b))
    - the two tables' roundings, the sum of the shifts, two fused multiply-adds: 4 * 2^-24 (|xa sc_a| + |sh_a| + |xb sc_b| + |sh_b| + |y64|)."""
    (xa, ga, ba), (xb, gb_, bb) = V.bn_channels(groups, N, H, W, seed=0), V.bn_channels(groups, N, H, W, seed=1)
    ra, rb = V.bn_reference(xa, ga, ba, groups), V.bn_reference(xb, gb_, bb, groups)
    pre = ra["pre"] + rb["pre"]
    y64 = pre.clamp_min(0) if relu else pre
    zero = dict(y=torch.zeros_like(pre))
    bound = V.bn_forward_bound(xa, dict(ra, **zero)) + V.bn_forward_bound(xb, dict(rb, **zero)) + 4 * 2.0 ** -24 * y64.abs()
    ma, mb = torch.nn.BatchNorm2d(C32).cuda(), torch.nn.BatchNorm2d(C32).cuda()
    for m, g_, b_ in ((ma, ga, ba), (mb, gb_, bb)):
        m.weight.data, m.bias.data = _cu(g_), _cu(b_)
        m.weight.grad, m.bias.grad = torch.zeros(C32, device="cuda"), torch.zeros(C32, device="cuda")
    xag, xbg = _cu(xa), _cu(xb)
    sa, sb = K.bn_stats(xag, K.bn_stats_buffer(groups, C32, "cuda"), groups, C32), K.bn_stats(xbg, K.bn_stats_buffer(groups, C32, "cuda"), groups, C32)
    rec, reca, recb = (K.amax_record("cuda") for _ in range(3))
    y = K.bn_join_fwd(xag, xbg, ma, mb, sa, sb, groups, relu, 0.1, 0.1, amax=rec)
    _derived("y", y, y64, bound)
    _record_is(rec, y)
    gy = torch.randn(pre.shape, generator=torch.Generator().manual_seed(11))
    if relu:
        near = V.near_relu(pre)
        assert near.double().mean().item() <= 0.01
        gy[near] = 0
    g64 = _bn_autograd(xa, ga, ba, groups, None, relu, gy, torch.float64, xb, gb_, bb)
    g32 = _bn_autograd(xa, ga, ba, groups, None, relu, gy, torch.float32, xb, gb_, bb)
    gxa, gxb = K.bn_join_bwd(_cu(gy), y, xag, xbg, ma, mb, sa, sb, groups, relu, True, True, amax_a=reca, amax_b=recb)
    _per_channel("gxa", gxa, g64[0], g32[0])
    _per_channel("gxb", gxb, g64[4], g32[4])
    sga, sba = _param_scales(xa, ra, gy, groups, pre if relu else None)
    sgb, sbb = _param_scales(xb, rb, gy, groups, pre if relu else None)
    for what, got, i, fs in (("ggamma_a", ma.weight.grad, 1, sga), ("gbeta_a", ma.bias.grad, 2, sba), ("ggamma_b", mb.weight.grad, 5, sgb),
                             ("gbeta_b", mb.bias.grad, 6, sbb)):
        _per_channel(what, got, g64[i], g32[i], floor_scale=fs)
    _record_is(reca, gxa)
    _record_is(recb, gxb)
    _dead_and_constant(relu, y, gxa, ma.weight.grad, ma.bias.grad, None)
    _dead_and_constant(relu, y, gxb, mb.weight.grad, mb.bias.grad, None)


@pytest.mark.parametrize("groups,N,H,W", V.BN_SHAPES)
def test_batchnorm_adjoint_from_1x1_on_hand_set_channels(K, groups, N, H, W):
    """bh_bn_bwd_from_1x1 (BatchNorm + ReLU in front of a 1x1 conv with 16 output channels): the BatchNorm's output gradient gs w is rebuilt
    per element.  measured per channel; the float32 yardstick forms gs w in float32 too."""
    x, gamma, beta = V.bn_channels(groups, N, H, W)
    ref = V.bn_reference(x, gamma, beta, groups, None, True)
    assert not V.near_relu(ref["pre"]).any()
    gen = torch.Generator().manual_seed(12)
    w, gs = torch.randn(16, 1, 1, C32, generator=gen) * 0.2, torch.randn(N, H, W, 16, generator=gen)
    g64 = _bn_autograd(x, gamma, beta, groups, None, True, gs.double() @ w.double().reshape(16, C32), torch.float64)
    g32 = _bn_autograd(x, gamma, beta, groups, None, True, gs @ w.reshape(16, C32), torch.float32)
    xg, gm, bt = _cu(x), _cu(gamma), _cu(beta)
    st = K.bn_stats(xg, K.bn_stats_buffer(groups, C32, "cuda"), groups, C32)
    gg, gb = torch.zeros(C32, device="cuda"), torch.zeros(C32, device="cuda")
    rec = K.amax_record("cuda")
    gx = K.bn_bwd_from_1x1(K.GradFrom1x1(_cu(gs), _cu(w)), xg, gm, bt, st, groups, V.BN_EPS, True, gg, gb, amax=rec)
    sg, sb_ = _param_scales(x, ref, gs.double() @ w.double().reshape(16, C32), groups, ref["pre"])
    _per_channel("gx", gx, g64[0], g32[0])
    _per_channel("ggamma", gg, g64[1], g32[1], floor_scale=sg)
    _per_channel("gbeta", gb, g64[2], g32[2], floor_scale=sb_)
    _record_is(rec, gx)
    _dead_and_constant(True, ref["y"].float().cuda(), gx, gg, gb, bt)


# ------------------------------------------------------------------------------------------------
# 5. loss kernels on post-ReLU features
# ------------------------------------------------------------------------------------------------
# measured: float64 torch autograd of the restatements of test_loss_variants_cpu.py / test_projection_cpu.py, at the tolerances of the
# existing tests of each kernel (loss 2e-5 relative, feature gradients 2e-5 of their maximum - 1e-5 per element for the L1 double line -,
# mask gradients 2e-4 of their maximum, dL/dH 1e-6 relative).  Both sides take |.|' = 0 at 0.
G = 0.7
REGIMES = ("ties", "masks_zero", "all_equal")


def _cu(t):
    return None if t is None else t.cuda().contiguous()


def _dbl(t):
    return None if t is None else t.double()


def _close(got, ref, rel, what, scale=None):
    """scale: what the error is relative to (default: max |ref|)."""
    err, scale = (got.detach().cpu().double() - ref).abs().max().item(), ref.abs().max().item() if scale is None else scale
    MEASURED.append((what, "max |err| %.3e = %.2e of the scale %.3e" % (err, err / max(scale, 1e-300), scale), "%.0e of max |ref|" % rel))
    assert torch.isfinite(got).all() and err <= rel * scale, (what, err, scale)


def _close_split(got, ref, special, keep, rel, what, scale=None):
    """The pixels `special` (all-zero vectors: gradients of order 1 / eps under the cosine) each on their own, the rest - where `keep` -
    relative to the maximum over the rest."""
    got, keep = got.detach().cpu().double(), keep.clone()
    for z in special:
        _close(got[z], ref[z], rel, "%s at the all-zero vector %s" % (what, z))
        keep[z] = False
    _close(got * keep[..., None], ref * keep[..., None], rel, what, scale)


def _regime(d, regime, rep=1):
    if regime == "masks_zero":
        for k in ("m1w", "m2w"):
            d[k] = torch.zeros_like(d[k])
    if regime == "all_equal":
        d["f2"], d["f2w"], d["f1w"] = d["f1"].clone(), d["f1"].clone(), d["f1"].repeat_interleave(rep, 0)
    return V.with_zero_vectors(d)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("metric", ["l1", "hinge"])
@pytest.mark.parametrize("B,hf,C", V.LOSS_SHAPES)
def test_loss_double_line(K, B, hf, C, metric, masks, regime):
    """bh_triplet_l1_fwd / bh_triplet_hinge_fwd + bh_bihome_loss_fwd, their adjoints and bh_bihome_anchor_bwd."""
    from test_loss_variants_cpu import aware_loss, aware_terms
    from test_projection_cpu import agnostic_loss
    hinge = metric == "hinge"
    d = _regime(V.post_relu_features(B, hf, C), regime)
    m1, m2 = (d["m1"], d["m2"]) if masks else (None, None)
    H1, _ = K.h4pt_fwd(_cu(d["dl"]), 128)
    H2, _ = K.h4pt_fwd(_cu(-d["dl"].flip(0)), 128)
    mu = 0.01
    f1, f2, a, b, ma, mb = (d[k].double().requires_grad_(True) for k in ("f1", "f2", "f1w", "f2w", "m1w", "m2w"))
    h1, h2 = (H.cpu().reshape(B, 3, 3).clone().requires_grad_(True) for H in (H1, H2))
    if hinge:
        ref = aware_loss(f1, f2, a, b, ma, mb, h1, h2, V.AWARE_MARGIN, mu, m1=_dbl(m1), m2=_dbl(m2))
        t1, t2 = (t.detach() for t in aware_terms(f1, f2, a, b, V.AWARE_MARGIN))
        M1r, M2r = t1.clamp_min(0).sum(-1), t2.clamp_min(0).sum(-1)
        keep = (t1.abs() >= V.FLIP * t1.abs().max()) & (t2.abs() >= V.FLIP * t2.abs().max())
        assert (~keep).double().mean() < 0.01
    else:
        ref = agnostic_loss(f1, f2, a, b, ma, mb, h1, h2, mu, m1=_dbl(m1), m2=_dbl(m2))
        l3 = (f1 - f2).abs().sum(-1).detach()
        M1r, M2r = (a - f2).abs().sum(-1).detach() - l3, (b - f1).abs().sum(-1).detach() - l3
        keep = torch.ones(B, hf, hf, C, dtype=torch.bool)
    (ref * G).backward()
    dev = [_cu(d[k]) for k in ("f1", "f2", "f1w", "f2w", "m1w", "m2w")]
    if hinge:
        M1, M2, nd = K.triplet_hinge_fwd(*dev, V.AWARE_MARGIN, m1=_cu(m1), m2=_cu(m2))
    else:
        M1, M2, nd = K.triplet_l1_fwd(*dev, m1=_cu(m1), m2=_cu(m2))
    loss4 = K.bihome_loss_fwd(nd, H1, H2, mu)
    MEASURED.append(("loss", "%.9g against %.9g" % (loss4[0].item(), ref.item()), "2e-5 relative"))
    assert abs(loss4[0].item() - ref.item()) <= 2e-5 * abs(ref.item()), (loss4[0].item(), ref.item())
    if hinge:
        _close(M1, M1r, 2e-5, "M1")
        _close(M2, M2r, 2e-5, "M2")
    else:
        np.testing.assert_allclose(M1.cpu().numpy(), M1r.numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(M2.cpu().numpy(), M2r.numpy(), rtol=1e-4, atol=1e-4)
    gl = torch.tensor([G], device="cuda")
    if hinge:
        gf1w, gf2w, gm1w, gm2w, gH1, gH2 = K.triplet_hinge_bwd(gl, *dev, _cu(m1), _cu(m2), M1, M2, nd, H1, H2, V.AWARE_MARGIN, mu)
        _close(gf1w.cpu().double() * keep, a.grad * keep, 2e-5, "g_f1w")
        _close(gf2w.cpu().double() * keep, b.grad * keep, 2e-5, "g_f2w")
    else:
        gf1w, gf2w, gm1w, gm2w, gH1, gH2 = K.bihome_loss_bwd(gl, *dev, _cu(m1), _cu(m2), M1, M2, nd, H1, H2, mu)
        np.testing.assert_allclose(gf1w.cpu().numpy(), a.grad.numpy(), rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(gf2w.cpu().numpy(), b.grad.numpy(), rtol=1e-5, atol=1e-9)
        # exact: a tie has no gradient (sgn(0) = 0), also in float32 - the operands are equal bit for bit
        assert (gf1w.cpu()[d["f1w"] == d["f2"]] == 0).all() and (gf2w.cpu()[d["f2w"] == d["f1"]] == 0).all()
    # (equal maps: every pixel has the same value v and the mask gradient G (v - num / den) / max(den, 1) cancels to rounding - 1e-17 in
    #  float64, 1e-8 in float32: the tolerance is held relative to the terms that cancel, G max |v| (max(den, 1) >= 1), not to that noise)
    ms = G * max(M1r.abs().max().item(), M2r.abs().max().item()) if regime == "all_equal" else None
    _close(gm1w, ma.grad, 2e-4, "g_m1w", ms)
    _close(gm2w, mb.grad, 2e-4, "g_m2w", ms)
    np.testing.assert_allclose(gH1.cpu().numpy().reshape(B, 3, 3), h1.grad.numpy(), rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(gH2.cpu().numpy().reshape(B, 3, 3), h2.grad.numpy(), rtol=1e-6, atol=1e-10)
    g1, g2 = K.bihome_anchor_bwd(gl, *dev, nd, m1=_cu(m1), m2=_cu(m2), margin=V.AWARE_MARGIN if hinge else None)
    _close(g1.cpu().double() * keep, f1.grad * keep, 2e-5, "g_f1 (anchor adjoint)")
    _close(g2.cpu().double() * keep, f2.grad * keep, 2e-5, "g_f2 (anchor adjoint)")
    if regime != "ties":
        for t in (gf1w, gf2w, g1, g2):                           # (weights of 0, or sgn(0) = 0 in every channel)
            exact("all-zero masks / equal maps: no feature gradient", t, torch.zeros_like(t))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("metric", ["l1", "cosine"])
@pytest.mark.parametrize("B,hf,C", V.LOSS_SHAPES)
def test_loss_one_line(K, B, hf, C, metric, rep, regime):
    """bh_oneline_loss_fwd / _bwd, bh_oneline_cos_loss_fwd / _bwd (the all-zero vectors take the COS_EPS branch: a gradient of y_hat / eps)
    and bh_oneline_anchor_bwd."""
    from test_loss_variants_cpu import cosine_loss
    from test_projection_cpu import l1_loss
    cosine = metric == "cosine"
    d = _regime(V.post_relu_features(B, hf, C, rep=rep), regime, rep)
    margin = V.COS_MARGIN if cosine else (1.0 if regime == "all_equal" else V.l1_margin(d, rep))
    f1, f2, a, m = (d[k].double().requires_grad_(True) for k in ("f1", "f2", "f1w", "m1w"))
    s = d["scores"].double().requires_grad_(True) if rep > 1 else None
    ref, per, t = (cosine_loss if cosine else l1_loss)(f1, f2, a, m, margin, rep=rep, scores=s)
    (ref * G).backward()
    t = t.detach()
    if regime == "ties":
        assert (t > 0).any() and (t < 0).any()                   # both hinge states occur
    keep_h = t.abs() >= V.FLIP * t.abs().max()
    assert (~keep_h).double().mean() < 0.01
    dev = [_cu(d[k]) for k in ("f1", "f2", "f1w", "m1w")]
    fwd, bwd = (K.oneline_cos_loss_fwd, K.oneline_cos_loss_bwd) if cosine else (K.oneline_loss_fwd, K.oneline_loss_bwd)
    loss, T, numden, perk = fwd(*dev, margin, rep=rep, sample_w=_cu(d["scores"]))
    MEASURED.append(("loss", "%.9g against %.9g" % (loss.item(), ref.item()), "2e-5 relative"))
    assert abs(loss.item() - ref.item()) <= 2e-5 * abs(ref.item()), (loss.item(), ref.item())
    _close(T, t, 2e-5, "T")
    _close(perk, per.detach(), 2e-5, "per-hypothesis loss")
    gl = torch.tensor([G], device="cuda")
    gf, gm = bwd(gl, dev[1], dev[2], dev[3], T, numden, rep=rep, sample_w=_cu(d["scores"]))
    # (equal maps: the mask gradient cancels to rounding, as in test_loss_double_line - relative to the terms that cancel)
    _close(gm, m.grad, 2e-4, "g_m1w", G * t.clamp_min(0).max().item() if regime == "all_equal" else None)
    scale = None
    if cosine and regime == "all_equal":
        # c(x, x) = 1 has no gradient: (y_hat - c x_hat) / |x| cancels to rounding, ~1e-16 of its terms in float64 and ~1e-7 in float32.  The
        # existing tolerance is held relative to the size of the two terms that cancel, G w / (max(den, 1) |x|) at its largest, instead of
        # relative to a reference that is itself rounding noise.
        n = d["f1"].double().norm(dim=-1)
        wgt = d["m1w"].double() / d["m1w"].double().sum((-1, -2), keepdim=True).clamp_min(1.0)
        scale = G * (wgt.reshape(B, rep, hf, hf).amax(1)[n > 0] / n[n > 0]).max().item()
    _close_split(gf, a.grad, d["zero_f1w"], keep_h, 2e-5, "g_f1w", scale)
    for bz, i, j in d["zero_f2"]:
        if cosine:                                               # c(f1w, 0) = 0 whatever f1w is
            for h in range(rep):
                assert a.grad[bz * rep + h, i, j].abs().max() == 0 and gf[bz * rep + h, i, j].abs().max().item() == 0
    if not cosine and regime != "masks_zero":
        tied = (d["f1w"] == d["f2"].repeat_interleave(rep, 0))
        assert tied.double().mean() > 0.25 and (gf.cpu()[tied] == 0).all()       # exact: sgn(0) = 0
    g1, g2 = K.oneline_anchor_bwd(gl, *dev, T, numden, rep=rep, sample_w=_cu(d["scores"]), cosine=cosine)
    keep = keep_h.reshape(B, rep, hf, hf).all(1)
    _close_split(g1, f1.grad, d["zero_f1"] if cosine else [], keep, 2e-5, "g_f1 (anchor adjoint)", None if scale is None else 2 * rep * scale)
    _close_split(g2, f2.grad, d["zero_f2"] if cosine else [], keep, 2e-5, "g_f2 (anchor adjoint)", None if scale is None else 2 * rep * scale)
    if regime == "masks_zero":
        exact("all-zero masks: the loss", loss, torch.zeros_like(loss))
        for x in (gf, g1, g2):
            exact("all-zero masks: no feature gradient", x, torch.zeros_like(x))


@pytest.mark.parametrize("B,hf,C", V.LOSS_SHAPES)
def test_loss_with_every_hinge_inactive(K, B, hf, C):
    """exact.  Margin -1e3: every hinge is inactive - the loss terms are exactly 0 and so is every gradient the kernels write (what then
    flows through the whole extractor and backbone)."""
    d = V.post_relu_features(B, hf, C, rep=3)
    gl = torch.tensor([G], device="cuda")
    dev = [_cu(d[k]) for k in ("f1", "f2", "f1w", "m1w")]
    for cosine in (False, True):
        fwd, bwd = (K.oneline_cos_loss_fwd, K.oneline_cos_loss_bwd) if cosine else (K.oneline_loss_fwd, K.oneline_loss_bwd)
        loss, T, numden, per = fwd(*dev, -1e3, rep=3, sample_w=_cu(d["scores"]))
        outs = [loss, per, *bwd(gl, dev[1], dev[2], dev[3], T, numden, rep=3, sample_w=_cu(d["scores"])),
                *K.oneline_anchor_bwd(gl, *dev, T, numden, rep=3, sample_w=_cu(d["scores"]), cosine=cosine)]
        assert (T < 0).all()
        for x in outs:
            exact("one-line %s, margin -1e3" % ("cosine" if cosine else "L1"), x, torch.zeros_like(x))
    d = V.post_relu_features(B, hf, C)
    dev = [_cu(d[k]) for k in ("f1", "f2", "f1w", "f2w", "m1w", "m2w")]
    H, _ = K.h4pt_fwd(_cu(d["dl"]), 128)
    M1, M2, nd = K.triplet_hinge_fwd(*dev, -1e3, m1=_cu(d["m1"]), m2=_cu(d["m2"]))
    loss4 = K.bihome_loss_fwd(nd, H, H, 0.01)
    gf1w, gf2w, gm1w, gm2w, _, _ = K.triplet_hinge_bwd(gl, *dev, _cu(d["m1"]), _cu(d["m2"]), M1, M2, nd, H, H, -1e3, 0.01)
    g1, g2 = K.bihome_anchor_bwd(gl, *dev, nd, m1=_cu(d["m1"]), m2=_cu(d["m2"]), margin=-1e3)
    for x in (M1, M2, loss4[1:3], gf1w, gf2w, gm1w, gm2w, g1, g2):
        exact("double-line channel hinge, margin -1e3", x, torch.zeros_like(x))


@pytest.mark.parametrize("B,hf,C", V.LOSS_SHAPES)
def test_l2norm_on_post_relu_vectors(K, B, hf, C):
    """bh_l2norm_fwd / _bwd at test_l2norm_pair_vs_float64's 2e-5 of the maximum; the all-zero vectors have no direction - there is no
    epsilon, as upstream: 0 / 0 - and are non-finite on both sides, which is all that is claimed of them."""
    from test_projection_cpu import l2n
    d = V.post_relu_features(B, hf, C)
    x, gy = d["f2"], d["f1w"] - 0.1
    assert (x == 0).double().mean() > 0.5
    a = x.double().requires_grad_(True)
    ref = l2n(a)
    (gref,) = torch.autograd.grad(ref, a, gy.double())
    y, inv = K.l2norm_fwd(_cu(x))
    gx = K.l2norm_bwd(_cu(gy), y, inv)
    ok = torch.ones(B, hf, hf, dtype=torch.bool)
    for z in d["zero_f2"]:
        assert not torch.isfinite(ref[z]).any() and not torch.isfinite(y[z]).any() and not torch.isfinite(gx[z]).any()
        ok[z] = False
    _close(y[ok.cuda()], ref.detach()[ok], 2e-5, "y")
    _close(inv[ok.cuda()], (1.0 / x.double().norm(dim=-1))[ok], 2e-5, "inv")
    _close(gx[ok.cuda()], gref[ok], 2e-5, "gx")
    assert (y.cpu()[ok][x[ok] == 0] == 0).all()                  # exact: a zero entry stays zero


# 5 (continued): the Zhang content-aware triplet loss (one-channel full-resolution features)
@pytest.mark.parametrize("margin,double,regime", [(m, dbl, r) for m, dbl in ((0.5, True), ("inf", True), (0.5, False))
                                                  for r in REGIMES + ("inactive",) if not (m == "inf" and r == "inactive")])
def test_zhang_triplet_on_post_relu_features(K, margin, double, regime):
    """bh_zhang_triplet_fwd / _bwd + bh_bihome_loss_fwd against float64 autograd of test_zhang_triplet_kernels' formula, at its tolerances
    (loss 2e-6 relative + 1e-6, gradients 1e-5 of their maximum): relu(randn - 0.5) maps, the warped map equal to its target on a
    quarter of the pixels; all-zero masks; f1w == f2 == f1; every hinge inactive (margin -1e3: exact zeros)."""
    B, h = 2, 16
    g = torch.Generator().manual_seed(B * h + 1)
    f = [(torch.randn(B, 1, h, h, generator=g) - 0.5).clamp_min(0) for _ in range(4)]      # f1, f2, f1w, f2w
    tie = ((torch.arange(h * h).reshape(h, h) % 4) == 0)[None, None]
    f[2], f[3] = torch.where(tie, f[1], f[2]), torch.where(tie, f[0], f[3])
    m = [torch.rand(B, h, h, generator=g) for _ in range(2)]                                # m1w, m2w
    m[1][-1] *= 1e-4                                                                        # the max(den, 1) branch
    if regime == "masks_zero":
        m = [torch.zeros_like(t) for t in m]
    if regime == "all_equal":
        f = [f[0].clone() for _ in range(4)]
    hinge = not isinstance(margin, str)
    if regime == "inactive":                                                                # (only with a hinge: there is none to switch off otherwise)
        margin = -1e3
    assert all((t == 0).double().mean() > 0.5 for t in f)
    fd, md = [t.double().requires_grad_(True) for t in f], [t.double().requires_grad_(True) for t in m]

    def line(fw, fo, fs, mw):
        t = (fw - fo).abs().sum(1) - (fs - fo).abs().sum(1)
        if hinge:
            t = torch.clamp(t + margin, min=0)
        den = mw.sum((-1, -2))
        return ((mw * t).sum((-1, -2)) / torch.max(den, torch.ones_like(den))).sum()
    ref = line(fd[2], fd[1], fd[0], md[0])
    if double:
        ref = ref + line(fd[3], fd[0], fd[1], md[1])
    ref.backward()
    fc, mc = [_cu(t) for t in f], [_cu(t) for t in m]
    T1, T2, numden = K.zhang_triplet_fwd(fc[0], fc[1], fc[2], fc[3] if double else None, mc[0], mc[1] if double else None, margin if hinge else 0.0, hinge)
    eye = torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 9).expand(B, 9).contiguous()
    loss4 = K.bihome_loss_fwd(numden, eye, eye, 0.0)
    MEASURED.append(("loss", "%.9g against %.9g" % (loss4[0].item(), ref.item()), "2e-6 relative + 1e-6"))
    assert abs(loss4[0].item() - ref.item()) <= 2e-6 * abs(ref.item()) + 1e-6
    grads = K.zhang_triplet_bwd(torch.ones(1, device="cuda"), fc[0], fc[1], fc[2], fc[3] if double else None, mc[0], mc[1] if double else None,
                                T1, T2, numden, hinge)
    refs = (fd[0].grad, fd[1].grad, fd[2].grad, fd[3].grad if double else None, md[0].grad, md[1].grad if double else None)
    # (equal maps under the hinge: every pixel's value is the margin and the mask gradient cancels to rounding - relative to the margin, as in
    #  test_loss_double_line)
    ms = float(margin) if (regime == "all_equal" and hinge) else None
    for name, got, want in zip(("g_f1", "g_f2", "g_f1w", "g_f2w", "g_m1w", "g_m2w"), grads, refs):
        if want is not None:
            _close(got, want.reshape(got.shape), 1e-5, name, ms if name.startswith("g_m") else None)
    if regime in ("inactive", "masks_zero", "all_equal"):
        for name, got in zip(("g_f1", "g_f2", "g_f1w", "g_f2w"), grads[:4]):
            if got is not None:
                exact("%s: no feature gradient" % name, got, torch.zeros_like(got))
    if regime == "inactive":
        exact("the loss", loss4[:3], torch.zeros(3, device="cuda"))
        for got in grads[4:]:
            if got is not None:
                exact("no mask gradient", got, torch.zeros_like(got))
    if regime == "ties":
        tied = (f[2] == f[1])
        assert (grads[2].cpu()[tied] == 0).all()                                            # exact: sgn(0) = 0


# ------------------------------------------------------------------------------------------------
# 6. warp on degenerate images and homographies
# ------------------------------------------------------------------------------------------------
def _tie_cap(H64, B, h, w):
    tie, _ = HK.coordinate_ties(H64.cpu().reshape(B, 3, 3), h, w)
    MEASURED.append(("pixels excluded as coordinate ties", "%d of %d" % (int(tie.sum()), tie.numel()), "at most 1 %"))
    assert tie.double().mean().item() <= 0.01


@pytest.mark.parametrize("size", [64, 48])             # (pool 4: the fast kernels on 64 x 64, the generic ones on 48 x 48)
@pytest.mark.parametrize("image", ["constant", "zero"])
def test_warp_of_a_constant_image(K, size, image):
    """measured: check_warp_fwd_bwd's oracle and bounds (forward 1e-4 of range or 1.5 x the float32 oracle's spread, coverage 2e-5, adjoint
    WARP_ADJOINT_BOUND) with its coordinate_ties exclusion.  A constant image: every interior blend is c (w00 + ... + w11), the gradient
    lives on the border taps only.  An all-zero image - exact: the warped image is 0 and its term of dL/dH is exactly 0, dL/dH is the
    coverage term alone, bit for bit what the call without an image gradient gives."""
    B, pool = 2, 4
    c = 0.75 if image == "constant" else 0.0
    H64, _ = K.h4pt_fwd(HK.dev(V.warp_delta(B, size)), (size, size))
    _tie_cap(H64, B, size, size)
    cov, gH, (img, H64, go, gc, _) = HK.check_warp_fwd_bwd(K, B, 2, size, size, pool, image=lambda a: np.full_like(a, c), H64=H64)
    assert (cov > 0.99).any() and (cov == 0).any()                  # inside and outside parts
    if image == "zero":
        exact("the warped all-zero image", K.warp_fwd(img, H64, pool)[0], torch.zeros_like(img))
        # (in a deterministic call: the default adjoint adds its partial sums with f64 atomics in arrival order - two launches of the SAME
        #  arguments differ in the last bit, 3.6e-15 of 1.7e+03 met on 48 x 48)
        with K.det_scope(True):
            exact("dL/dH of the all-zero image: the coverage term alone", K.warp_bwd(img, H64, go, gc, pool), K.warp_bwd(img, H64, torch.zeros_like(go), gc, pool))
        assert (gH - K.warp_bwd(img, H64, torch.zeros_like(go), gc, pool)).abs().max().item() <= 1e-12 * gH.abs().max().item()


@pytest.mark.parametrize("size", [64, 48])
def test_warp_wholly_outside(K, size):
    """exact.  Every sample is warped wholly outside its source: the image, the coverage and dL/dH (for any output gradient) are exactly 0."""
    B, pool = 2, 4
    rng = np.random.Generator(np.random.PCG64(size))
    img = HK.dev(rng.standard_normal((B, 2, size, size)).astype(np.float32))
    H64 = torch.tensor([[1., 0, 3 * size, 0, 1, 0, 0, 0, 1], [1., 0, 0, 0, 1, -3 * size, 0, 0, 1]], dtype=torch.float64).cuda()
    out, cov = K.warp_fwd(img, H64, pool)
    exact("warped image", out, torch.zeros_like(out))
    exact("coverage", cov, torch.zeros_like(cov))
    exact("coverage-only entry", K.mask_coverage_fwd(H64, size, size, pool), torch.zeros_like(cov))
    go, gc = HK.dev(rng.standard_normal(out.shape).astype(np.float32)), HK.dev(rng.standard_normal(cov.shape).astype(np.float32))
    gH = K.warp_bwd(img, H64, go, gc, pool)
    exact("dL/dH", gH, torch.zeros_like(gH))


# the degenerate cases through the extractor stem's fused forms, held against the two calls each replaces (kernel against kernel: no oracle)
HORIZON = [v for row in V.HORIZON for v in row]          # qz = 1 - x / 8 is exactly 0 on column x = 8 (asserted in float32 by test_value_regimes_cpu.py)
FUSED_CASES = ("constant", "zero", "outside", "horizon")


def _fused_case(K, case, B, size, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    src = F.avg_pool2d(torch.tensor(rng.standard_normal((B, 1, size, size)).astype(np.float32)), 3, 1, 1)
    if case in ("constant", "zero"):
        src = torch.full_like(src, 0.75 if case == "constant" else 0.0)
    H64, _ = K.h4pt_fwd(HK.dev(HK.rand_delta(B, size + 1, amp=size / 4.0)), (size, size))
    if case == "outside":
        H64 = torch.tensor([1., 0, 3 * size, 0, 1, 0, 0, 0, 1], dtype=torch.float64).repeat(B, 1).cuda()
    if case == "horizon":
        H64 = torch.tensor(HORIZON, dtype=torch.float64).repeat(B, 1).cuda()
    return src.cuda().contiguous(), H64.contiguous(), rng


@pytest.mark.parametrize("case", FUSED_CASES)
def test_stem_forward_with_the_warp_folded_in_on_degenerate_inputs(K, case):
    """exact.  bh_stem7_fwd_warp against bh_warp_fwd followed by the fp16-piece stem: y, the warped image and the pooled coverage bit for
    bit (check_stem_forward_with_the_warp_folded_in's criterion); everything finite, also with the horizon inside the patch."""
    B, size = 16, 64
    src, H64, rng = _fused_case(K, case, B, size, 5)
    wt = torch.tensor((rng.standard_normal((64, 7, 7, 1)) * 0.05).astype(np.float32)).cuda()
    d = _stem_fwd(K, B, 1)
    warped0, cov0 = K.warp_fwd(src, H64, 4)
    y0 = K.conv_fwd(warped0.view(B, size, size, 1), wt, None, d)
    y1, warped1, cov1 = _stem_fwd_warp(K, src, H64, wt, d)
    exact("warped image", warped1, warped0)
    exact("coverage", cov1, cov0)
    exact("y", y1, y0)
    assert torch.isfinite(y1).all() and torch.isfinite(warped1).all() and torch.isfinite(cov1).all()
    if case in ("zero", "outside"):
        exact("y of an all-zero warped image", y1, torch.zeros_like(y1))
    if case == "outside":
        exact("coverage outside", cov1, torch.zeros_like(cov1))
    if case == "constant":
        assert (cov1 > 0.99).any() and (warped1 == 0.75).any()


@pytest.mark.parametrize("prec", [4, 0])
@pytest.mark.parametrize("case", FUSED_CASES)
def test_stem_dgrad_with_the_warp_adjoint_folded_in_on_degenerate_inputs(K, case, prec):
    """bh_stem7_dgrad_c1_warp against bh_stem7_dgrad_c1 followed by bh_warp_bwd: the gradient image bit for bit, dL/dH within 1e-5 of the
    largest entry the two calls add (check_stem_dgrad_with_the_warp_adjoint_folded_in's criterion - where they add exactly 0, exactly 0);
    everything finite."""
    from bihome_amd._lib import check, lib
    B, size, pool = 4, 64, 4
    src, H64, rng = _fused_case(K, case, B, size, 6)
    gy = torch.tensor(rng.standard_normal((B, size // 2, size // 2, 64)).astype(np.float32)).cuda()
    wt = torch.tensor((rng.standard_normal((64, 7, 7, 1)) * 0.05).astype(np.float32)).cuda()
    gcov = torch.tensor(rng.standard_normal((B, size // pool, size // pool)).astype(np.float32)).cuda()
    base = torch.tensor(rng.standard_normal((B, 9))).cuda()
    gx0 = _stem_dgrad(K, gy, wt, prec, B)
    gH0 = K.warp_bwd(src, H64, gx0.view(B, 1, size, size), gcov, pool, gH=base.clone())
    d = K.conv_desc(B, size, size, 1, 64, 7, 2, 3, precision=prec)
    gx1, gH1 = torch.full((B, size, size, 1), float("nan"), device="cuda"), base.clone()
    check(lib.bh_stem7_dgrad_c1_warp(_p(gy), _p(wt), _p(gx1), ctypes.byref(d), _p(src), _p(H64), _p(gcov), pool, _p(gH1), _stream()), "bh_stem7_dgrad_c1_warp")
    exact("gradient image", gx1, gx0)
    scale, err = (gH0 - base).abs().max().item(), (gH1 - gH0).abs().max().item()
    MEASURED.append(("max |gH - two calls|", "%.3e" % err, "1e-5 of %.3e" % scale))
    assert torch.isfinite(gH1).all() and err <= 1e-5 * scale, (err, scale)
    if case == "outside":
        exact("dL/dH of samples warped wholly outside: nothing is added", gH1, base)


@pytest.mark.parametrize("size", [64, 48])
def test_warp_adjoint_with_respect_to_the_image_on_degenerate_gradients(K, size):
    """bh_warp_bwd_img.  exact: an all-zero output gradient, and samples warped wholly outside, leave an image gradient of exactly 0.
    measured (check_warp_adjoint_with_respect_to_the_image's bound, 1e-4 of max |g_img| against float64 autograd of the oracle's warp): a
    constant output gradient - the image gradient is then the map of summed bilinear weights, zero where no output pixel looks."""
    from oracle import bihome_oracle as O
    B, C = 2, 2
    H64, _ = K.h4pt_fwd(HK.dev(V.warp_delta(B, size)), (size, size))
    gout = torch.full((B, C, size, size), 0.75, device="cuda")
    exact("all-zero output gradient", K.warp_bwd_img(H64, torch.zeros_like(gout)), torch.zeros_like(gout))
    out_H = torch.tensor([1., 0, 3 * size, 0, 1, 0, 0, 0, 1], dtype=torch.float64).repeat(B, 1).cuda()
    exact("wholly outside", K.warp_bwd_img(out_H, gout), torch.zeros_like(gout))
    gimg = K.warp_bwd_img(H64, gout)
    imt = torch.zeros(B, C, size, size, dtype=torch.float64, requires_grad=True)
    (O.warp_image(imt, H64.cpu().reshape(B, 3, 3)) * gout.double().cpu()).sum().backward()
    _close(gimg, imt.grad, 1e-4, "g_img of a constant output gradient")
    assert (gimg.cpu()[imt.grad == 0] == 0).all() and (imt.grad == 0).any()        # exact: pixels no output pixel samples


# the horizon inside the patch, against an independent float64 reference: V.warp_pixel_guard, the oracle's warp written in pixel
# coordinates with the kernels' guard (oracle.warp_image takes kornia's guard in normalised coordinates and samples elsewhere on that column)
def _horizon(B):
    return torch.tensor(HORIZON, dtype=torch.float64).repeat(B, 1).cuda().contiguous()


@pytest.mark.parametrize("size", [64, 48])             # (pool 4: the fast kernels on 64 x 64, the generic ones on 48 x 48)
def test_warp_with_the_horizon_inside_the_patch(K, size):
    """measured: check_warp_fwd_bwd's bounds (forward 1e-4 of range or 1.5 x the float32 reference's spread, coverage 2e-5, adjoint
    WARP_ADJOINT_BOUND) with its coordinate_ties exclusion (at most 1 % of the pixels, none on the guarded column) - forward, coverage
    and adjoint of bh_warp_fwd / bh_warp_bwd / bh_mask_coverage_fwd with qz == 0 on column 8; everything finite."""
    B = 2
    H64 = _horizon(B)
    tie = V.guarded_coordinate_ties(H64.cpu().reshape(B, 3, 3), size, size)
    MEASURED.append(("pixels excluded as coordinate ties", "%d of %d" % (int(tie.sum()), tie.numel()), "at most 1 %"))
    assert tie.double().mean().item() <= 0.01 and not tie[:, :, 8].any()
    cov, gH, (img, _, go, gc, pool) = HK.check_warp_fwd_bwd(K, B, 2, size, size, 4, H64=H64, oracle=V.warp_pixel_guard)
    out = K.warp_fwd(img, H64, pool)[0]
    assert torch.isfinite(out).all() and torch.isfinite(cov).all() and torch.isfinite(gH).all()
    assert (out[:, :, :, 8] != 0).any() and (cov > 0).any() and (cov == 0).any()      # the guarded column samples inside the image


@pytest.mark.parametrize("size", [64, 48])
def test_warp_adjoint_with_respect_to_the_image_with_the_horizon_inside_the_patch(K, size):
    """measured (check_warp_adjoint_with_respect_to_the_image's bound: 1e-4 of max |g_img| against float64 autograd of the reference warp)."""
    B, C = 2, 2
    H64 = _horizon(B)
    gout = torch.randn(B, C, size, size, generator=torch.Generator().manual_seed(size))
    gimg = K.warp_bwd_img(H64, gout.cuda())
    imt = torch.zeros(B, C, size, size, dtype=torch.float64, requires_grad=True)
    (V.warp_pixel_guard(imt, H64.cpu().reshape(B, 3, 3)) * gout.double()).sum().backward()
    _close(gimg, imt.grad, 1e-4, "g_img")
    assert (imt.grad[:, :, :, 8:10] != 0).any()                                      # the guarded column's taps land in columns 8 and 9


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("case", FUSED_CASES)
def test_photo_warp_on_degenerate_inputs(K, case, C):
    """bh_photo_warp_fwd / bh_photo_warp_bwd (a 128 x 128 patch gathered from a 240 x 320 image at origin + Hp.(x, y, 1)) on a constant
    image, an all-zero image, a patch mapped wholly outside and the horizon inside the patch.  measured: the bars of
    test_photo_warp_fwd_and_adjoint_vs_float64 - forward 1e-4 of the range or 1.5 x the float32 reference's own spread, dL/dHp 1e-4 of its
    largest entry or 1.5 x that spread - against V.warp_pixel_guard in float64, no output gradient at coordinate ties (at most 1 %).
    exact: the all-zero image and the patch outside give an image and a dL/dHp of exactly 0."""
    import test_photometric_gpu as PG
    B, P = 4, 128
    img, corners, delta = PG.inputs(B, C, 300 + C)
    if case in ("constant", "zero"):
        img = np.full_like(img, 0.75 if case == "constant" else 0.0)
    origin = torch.tensor(corners[:, 0])
    Hp64, _ = K.h4pt_fwd(PG.cuda(delta), P)
    if case == "outside":
        Hp64 = torch.tensor([1., 0, 1000.5, 0, 1, 0.25, 0, 0, 1], dtype=torch.float64).repeat(B, 1).cuda()      # (no integer coordinates: no ties)
    if case == "horizon":
        Hp64 = _horizon(B)
    Hp64 = Hp64.contiguous()
    out = K.photo_warp_fwd(PG.cuda(img), Hp64, PG.cuda(origin), P)
    Ht = Hp64.cpu().reshape(B, 3, 3).clone().requires_grad_(True)
    ref = V.warp_pixel_guard(torch.tensor(img, dtype=torch.float64), Ht, (P, P), origin)
    H32 = Hp64.cpu().reshape(B, 3, 3).float().requires_grad_(True)
    ref32 = V.warp_pixel_guard(torch.tensor(img), H32, (P, P), origin)
    o, r64 = out.cpu().double(), ref.detach()
    scale, err, spread = r64.abs().max().item(), (o - r64).abs().max().item(), (ref32.detach().double() - r64).abs().max().item()
    MEASURED.append(("forward: max |hip - f64|", "%.3e of range %.3e (float32 reference: %.3e)" % (err, scale, spread), "max(1e-4 of range, 1.5 x float32's)"))
    assert torch.isfinite(out).all() and err <= max(1e-4 * scale, 1.5 * spread), (err, scale, spread)
    tie = V.guarded_coordinate_ties(Ht.detach(), P, P, origin=origin, extent=320)
    MEASURED.append(("pixels excluded as coordinate ties", "%d of %d" % (int(tie.sum()), tie.numel()), "at most 1 %"))
    assert tie.double().mean().item() <= 0.01
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7 + C))
    go[tie[:, None].expand_as(go)] = 0
    (ref * go.double()).sum().backward()
    (ref32 * go).sum().backward()
    gH = K.photo_warp_bwd(PG.cuda(img), Hp64, PG.cuda(origin), go.cuda(), P)
    r = Ht.grad.reshape(B, 9)
    gscale = r.abs().max().item()
    gerr, gspread = (gH.cpu().double() - r).abs().max().item(), (H32.grad.reshape(B, 9).double() - r).abs().max().item()
    MEASURED.append(("adjoint: max |gH - f64|", "%.3e of max |dL/dHp| %.3e (float32 reference: %.3e)" % (gerr, gscale, gspread), "max(1e-4 of the maximum, 1.5 x float32's)"))
    assert torch.isfinite(gH).all() and gerr <= max(1e-4 * gscale, 1.5 * gspread), (gerr, gscale, gspread)
    if case in ("zero", "outside"):
        exact("the image", out, torch.zeros_like(out))
        exact("dL/dHp", gH, torch.zeros_like(gH))
    if case == "constant":
        assert ((out - 0.75).abs() < 1e-6).any() and ((out - 0.75).abs() > 1e-3).any()      # interior blends, and taps that leave the image
