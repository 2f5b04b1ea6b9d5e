"""Case tables of the support boundary: the smallest and the largest shape every entry point takes, one step on either side, the
empty batch - and the census of the conv dispatch.  tests/test_shape_edges_gpu.py runs the tables on the GPU, tests/test_shape_edges_cpu.py
holds them against the accept-conditions restated below and against the source lines they cite.  Nothing here needs a GPU.

A Case names the family, the shape (`args`, what the accept-condition is a predicate of), whether the entry point takes it, the line of
csrc/ that holds the condition (file, line, a fragment of the condition as written there) and how the GPU module runs it:
  accepted:  run = (test module, function, arguments after K, further modules whose torch.empty is poisoned) - the family's existing
             float64 comparison, unchanged, at the edge shape, inside tests/poisoned_alloc.py;
  refused:   run = (C entry point, {argument: value} laid over BASE[entry point], pointers passed as NULL) - a raw call on poisoned
             buffers: the return code, and every buffer bit-identical afterwards."""
import ctypes
import importlib
import itertools
import os
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH_OK, BH_E_BADARG, BH_E_UNSUPPORTED = 0, -1, -2

Case = namedtuple("Case", "family id accepted cite accept args run")


# ------------------------------------------------------------------------------------------------
# the header's prototypes (with the argument names: the raw calls are assembled from them)
# ------------------------------------------------------------------------------------------------
_SCALARS = {"int": "int", "long long": "i64", "int64_t": "i64", "size_t": "size", "float": "float", "double": "double"}


def header_text():
    text = open(os.path.join(ROOT, "include", "bihome.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"#ifdef BH_TUNING.*?#endif", "", text, flags=re.S)


def c_class(decl):
    """(type class, name) of one C parameter / return type: ptr, int, i64 (long long / int64_t), size (size_t), float, double."""
    decl = " ".join(decl.split())
    if "*" in decl:
        return "ptr", decl.split("*")[-1].strip()
    words = [w for w in decl.split(" ") if w != "const"]
    for n in (2, 1):                                     # "long long L" / "long long" / "int B" / "int"
        t = " ".join(words[:n])
        if t in _SCALARS and len(words) <= n + 1:
            return _SCALARS[t], (words[n] if len(words) > n else "")
    raise AssertionError("unparsed C declaration %r" % decl)


def header_prototypes():
    """name -> (return class, [(argument class, argument name)]) of every bh_* function include/bihome.h declares."""
    protos = {}
    for ret, name, args in re.findall(r"(?:^|[;}\n])\s*((?:unsigned\s+)?(?:long long|\w+))\s+(bh_\w+)\s*\(([^)]*)\)\s*;", header_text()):
        args = args.strip()
        protos[name] = (c_class(ret)[0], [] if args in ("", "void") else [c_class(a) for a in args.split(",")])
    return protos


# ------------------------------------------------------------------------------------------------
# accept-conditions, restated (each next to the line it restates)
# ------------------------------------------------------------------------------------------------
def loss_ok(C, B=2, hw=4, rep=1, **_):
    """triplet.hip:483-484 (triplet_args) / proj.hip:245, 288-289 (the anchor adjoints): the same set."""
    return B >= 0 and hw >= 1 and rep >= 1 and B % rep == 0 and C % 4 == 0 and C >= 4 and (C // 4 >= 64 or 64 % (C // 4) == 0) and B <= 65535


def l2norm_ok(C, M=4, **_):
    """proj.hip:244-245 (proj_args)"""
    return M >= 0 and C % 4 == 0 and C >= 4 and (C // 4 >= 64 or 64 % (C // 4) == 0)


def relu_bwd_ok(n, **_):
    """proj.hip:277"""
    return n >= 0 and n % 4 == 0


def scale_samples_ok(L, Bn=2, rep=1, **_):
    """triplet.hip:642 / :651"""
    return Bn >= 0 and rep >= 1 and L % 4 == 0


def bn_ok(C, groups=1, rows=4, **_):
    """bn.hip:22-24 (bn_geom): C in {4, 8, 16, ..., 1024}, any rows >= 1"""
    return C % 4 == 0 and groups >= 1 and rows >= 1 and C // 4 <= 256 and C >= 4 and 256 % (C // 4) == 0


BN_SMALL_ROWS = 4          # bn.hip: groups of at most this many rows are evaluated in double (bh_bn_bwd, the join) or refused (the fused forms)


def bn_chunks(rows, C):
    """bn.hip:25-30: (chunks, rows per chunk) of the statistics / reduce launches"""
    rpp = 256 // (C // 4)
    n = min(max(rows // (rpp * 4), 1), 256)
    rpc = (rows + n - 1) // n
    return (rows + rpc - 1) // rpc, rpc


def bn_maxpool_ok(C, groups, N, Hi, Wi, **_):
    """bn.hip (bh_bn_maxpool_fwd / _bwd): the geometry, the 32768-byte table, and more than BN_SMALL_ROWS rows per group (the fused forms
    have no double evaluation)"""
    return (N >= 1 and groups >= 1 and N % groups == 0 and bn_ok(C, groups, (N // groups) * Hi * Wi) and groups * C * 8 <= 32768
            and (N // groups) * Hi * Wi > BN_SMALL_ROWS)


def bn_from_1x1_ok(KC, C=8, groups=1, rows=4, **_):
    """bn.hip:1230-1231"""
    return KC in (16, 32) and bn_ok(C, groups, rows) and rows > BN_SMALL_ROWS


def bn1_ok(groups, rows, **_):
    """bn1.hip:16 (bn1_geom)"""
    return groups >= 1 and rows >= 1


def bn1_scalar_branch(groups, rows):
    """bn1.hip:41: a group whose first element is not 16-byte aligned is read one float at a time"""
    return any((g * rows) & 3 for g in range(groups))


def tail_ok(Ci, Cm, Co, groups=1, rows=4, hw=4, **_):
    """tail.hip:34-35 (tail_geom) and :942: Ci * Ci <= 256 leaves 8 and 16 of the entry point's {8, 16, 32}"""
    return (groups >= 1 and rows >= 1 and hw >= 1 and Ci % 4 == 0 and Ci <= 32 and Ci * Ci <= 256 and Cm % 64 == 0 and 0 < Cm <= 256
            and 1 <= Co <= 4 and rows % hw == 0 and Ci in (8, 16, 32))


def maxpool_ok(N, Hi, Wi, C, **_):
    """pool.hip:127-128 (bh_maxpool3s2_fwd / _bwd)"""
    return N >= 0 and Hi >= 1 and Wi >= 1 and C >= 4 and C % 4 == 0


def gap_ok(N, HW, C, **_):
    """pool.hip:149 / :157 (bh_gap_fwd / _bwd)"""
    return N >= 0 and HW >= 1 and C >= 1


def add_ok(n, **_):
    """pool.hip:176"""
    return n >= 0


def absmax_ok(n, misaligned=0, **_):
    """pool.hip:165"""
    return n >= 0 and not misaligned


def dlt_ok(P, n=1, B=2, **_):
    """geometry.hip:591-592: 4 <= P <= 64 * DLT_MAXPTS (8 points per lane)"""
    return B >= 0 and n >= 1 and 4 <= P <= 512


def dsac_ok(n, h, w, B=2, method=2, **_):
    """geometry.hip:629-632"""
    return method in (0, 1, 2) and B >= 0 and n >= 1 and h >= 1 and w >= 1 and (method == 0 or h * w <= 1 << 30)


def ransac_ok(K, h, w, B=2, **_):
    """ransac.hip:489-490"""
    return B >= 0 and K >= 1 and h >= 1 and w >= 1 and h * w >= 4 and h * w <= 1 << 30 and B * K <= 1 << 30 and B <= 65535


def lm_ok(h, w, iters, B=2, **_):
    """ransac.hip:510-511"""
    return B >= 0 and h >= 1 and w >= 1 and h * w >= 4 and iters >= 0 and h * w <= 1 << 30 and B <= 65535


def warp_ok(h, w, pool, **_):
    """warp.hip:326-327 (warp_shape_ok)"""
    return h % 16 == 0 and w % 16 == 0 and pool in (1, 2, 4, 8, 16, 32) and h % pool == 0 and w % pool == 0 and h * w < 1 << 30 and h > 0 and w > 0


def photo_ok(P, Hi, Wi, B=2, C=1, **_):
    """photo.hip:78-79"""
    return B >= 0 and C >= 1 and Hi >= 1 and Wi >= 1 and P >= 1 and P % 16 == 0 and Hi * Wi * 4 < 0xFFFFFFFF


def synth_ok(P, B=2, C=1, **_):
    """synth.hip:193-195"""
    return B >= 0 and C in (1, 3) and P % 16 == 0


def blobs_ok(P, B=2, C=1, blobiness=0.5, **_):
    """blobs.hip:209-216: 16 <= P <= 256 in steps of 16, radius int(4 sigma + 0.5) <= P with sigma = P / (40 blobiness)"""
    sigma = P / (40.0 * blobiness)
    return B >= 2 and C in (1, 3) and 16 <= P <= 256 and P % 16 == 0 and 4.0 * sigma + 0.5 <= P + 1.0 and int(4.0 * sigma + 0.5) <= P


def blobs_needs_scratch(P):
    """blobs.hip:217 / :203 (BLOB_LDS_P = 128)"""
    return P > 128


def stem7_fwd_ok(N, Hi, Wi, Ci, **_):
    """stem7.hip (bh_stem7_try): Ho, Wo multiples of 8, at least 256 tiles of 8 x 8 outputs"""
    return Ci in (1, 2, 3) and Hi % 16 == 0 and Wi % 16 == 0 and N * (Hi // 16) * (Wi // 16) >= 256


def stem7_wgrad_ok(N, Hi, Wi, Ci=2, **_):
    """stem7.hip:862-863 (stem7_wgrad_ok)"""
    return Ci == 2 and Hi % 16 == 0 and Wi % 16 == 0 and N * (Hi // 16) * (Wi // 16) >= 512


def halo_grid_ok(N, H, W, Ci, Co, dgrad=False, **_):
    """conv3x3.hip:833-835, 871-873, 907: the halo-tiled 3x3 kernel without BH_ROUTE_HALO_SMALL takes a launch of at least C3_MIN_BLOCKS
    workgroup slots (sub-tile pairs x output-channel tiles)"""
    if H % 8 or W % 8 or Ci % 32 or Co % 32:
        return False
    nn = Ci if dgrad else Co
    tile = 32 if nn % 64 else 64
    sub = N * (H // 8) * (W // 8)
    return (sub + 1) // 2 * (nn // tile) >= C3_MIN_BLOCKS


def _c3_min_blocks():
    src = open(os.path.join(ROOT, "bihome_amd", "csrc", "conv3x3.hip")).read() + open(os.path.join(ROOT, "bihome_amd", "csrc", "conv3x3_args.h")).read()
    m = re.search(r"C3_MIN_BLOCKS\s*=?\s*(\d+)", src)
    assert m, "C3_MIN_BLOCKS not found"
    return int(m.group(1))


C3_MIN_BLOCKS = _c3_min_blocks()


def pc_pairs_ok(N, H, W, groups, **_):
    """conv3x3_pc.hip:709-710 / :714: both sub-tiles of a tile position in one statistics (BatchNorm-on-load) group"""
    return ((N // groups) * (H // 8) * (W // 8)) % 2 == 0


def conv_desc_ok(Hi, Wi, k, s, p, transposed=False, **_):
    """conv_gemm.hip:1077-1083 (check_desc): a Conv2d of any geometry with at least one output pixel, a ConvTranspose2d with kernel == stride"""
    if transposed:
        return k == s and p == 0
    return Hi + 2 * p >= k and Wi + 2 * p >= k


def wgrad_ws_ok(short, **_):
    """wgrad.hip / stem7.hip:877: the workspace holds at least bh_conv_wgrad_det_bytes / bh_stem7_wgrad_ws_bytes bytes"""
    return short <= 0


def always(**_):
    return True


def never(**_):
    return False


# ------------------------------------------------------------------------------------------------
# 1. accepted edges
# ------------------------------------------------------------------------------------------------
HK, CK, PJ, LV, ZH, DS, PH, BL, DG, F16, PC, PW, SE = ("test_head_kernels_gpu", "test_conv_kernels_gpu", "test_projection_gpu",
                                                       "test_loss_variants_gpu", "test_zhang_gpu", "test_dsac_scoring_gpu",
                                                       "test_photometric_gpu", "test_blobs_gpu", "test_datagen_gpu", "test_f16x2_gpu",
                                                       "test_conv_pc_gpu", "test_pointwise_gpu", "test_shape_edges_gpu")
LOSS_CITE = ("triplet.hip", 484, "(C / 4 < 64 && (64 % (C / 4)))")
PROJ_CITE = ("proj.hip", 245, "(C / 4 < 64 && (64 % (C / 4)))")


def _acc(family, id, cite, accept, args, run):
    return Case(family, id, True, cite, accept, args, run)


def _loss_cases():
    out = []
    # C: the divisor rule's smallest values, its top (C / 4 = 64) and the first two values of the C / 4 >= 64 arm (65 and 80 float4 groups per
    # pixel: the second pass of a lane over the channels is partly filled).  hw = 9 / 25 as the files' own small shapes (partly filled wave passes)
    for C in (4, 8, 256, 260, 320):
        a = dict(C=C, B=2, hw=9)
        out += [
            _acc("loss", "triplet-l1-C%d" % C, LOSS_CITE, loss_ok, a, (HK, "test_triplet_fwd_bwd", (2, 3, C, True), ())),
            _acc("loss", "oneline-l1-C%d" % C, LOSS_CITE, loss_ok, a, (HK, "test_oneline_hinge_loss_fwd_bwd", (2, 3, C, 0.5625 * C), ())),
            _acc("loss", "l2norm-C%d" % C, PROJ_CITE, l2norm_ok, dict(C=C, M=18), (PJ, "test_l2norm_pair_vs_float64", (2, 3, C), (LV,))),
        ]
    for C in (8, 256, 260, 320):
        # (the files' own inputs put single all-zero vectors and ties at fixed pixels: hf = 5 as in their SHAPES.  C = 4 leaves a cosine of four
        #  terms and per-channel hinges of four channels: the statistics those tests assert of their inputs do not hold there)
        a = dict(C=C, B=2, hw=25)
        out += [
            _acc("loss", "cosine-C%d" % C, LOSS_CITE, loss_ok, dict(C=C, B=6, hw=25, rep=3), (LV, "test_cosine_pair_vs_float64_autograd", (2, 5, C, 3), ())),
            _acc("loss", "hinge-C%d" % C, LOSS_CITE, loss_ok, a, (LV, "test_channel_aware_pair_vs_float64_autograd", (2, 5, C, True), ())),
            _acc("loss", "anchor-l1-C%d" % C, PROJ_CITE, loss_ok, dict(C=C, B=6, hw=25, rep=3), (PJ, "test_oneline_anchor_adjoint_vs_float64_autograd", (2, 5, C, "l1", 3, True), (LV,))),
            _acc("loss", "anchor-cos-C%d" % C, PROJ_CITE, loss_ok, a, (PJ, "test_oneline_anchor_adjoint_vs_float64_autograd", (2, 5, C, "cosine", 1, False), (LV,))),
            _acc("loss", "anchor2-l1-C%d" % C, PROJ_CITE, loss_ok, a, (PJ, "test_double_line_anchor_adjoint_vs_float64_autograd", (2, 5, C, "agnostic", True), (LV,))),
            _acc("loss", "anchor2-hinge-C%d" % C, PROJ_CITE, loss_ok, a, (PJ, "test_double_line_anchor_adjoint_vs_float64_autograd", (2, 5, C, "hinge", False), (LV,))),
        ]
    hw_cite = ("triplet.hip", 483, "hw < 1")
    out += [
        # hw = 1: one pixel per sample, every wave pass but the first lane group empty; hw = 7: a prime
        _acc("loss", "triplet-hw1", hw_cite, loss_ok, dict(C=64, B=2, hw=1), (HK, "test_triplet_fwd_bwd", (2, 1, 64, True), ())),
        _acc("loss", "oneline-hw1", hw_cite, loss_ok, dict(C=64, B=2, hw=1), (HK, "test_oneline_hinge_loss_fwd_bwd", (2, 1, 64, 36.25), ())),
        _acc("loss", "l2norm-M1", ("proj.hip", 244, "rows < 0"), l2norm_ok, dict(C=16, M=1), (PJ, "test_l2norm_pair_vs_float64", (1, 1, 16), (LV,))),
        _acc("loss", "triplet-hw7", hw_cite, loss_ok, dict(C=16, B=2, hw=7), (HK, "test_triplet_fwd_bwd", (2, 1, 16, True, 7), ())),
        _acc("loss", "oneline-hw7", hw_cite, loss_ok, dict(C=16, B=2, hw=7), (HK, "test_oneline_hinge_loss_fwd_bwd", (2, 1, 16, 9.25, 7), ())),
        # B = 1; rep > 1 with B = rep (one sample, three hypotheses)
        _acc("loss", "triplet-B1", ("triplet.hip", 483, "B < 0"), loss_ok, dict(C=64, B=1, hw=9), (HK, "test_triplet_fwd_bwd", (1, 3, 64, False), ())),
        _acc("loss", "oneline-B1", ("triplet.hip", 483, "B < 0"), loss_ok, dict(C=64, B=1, hw=9), (HK, "test_oneline_hinge_loss_fwd_bwd", (1, 3, 64, 36.25), ())),
        _acc("loss", "cosine-B3-rep3", ("triplet.hip", 483, "B % rep"), loss_ok, dict(C=64, B=3, hw=25, rep=3), (LV, "test_cosine_pair_vs_float64_autograd", (1, 5, 64, 3), ())),
        _acc("loss", "anchor-B3-rep3", ("proj.hip", 288, "B % rep"), loss_ok, dict(C=64, B=3, hw=25, rep=3),
             (PJ, "test_oneline_anchor_adjoint_vs_float64_autograd", (1, 5, 64, "l1", 3, False), (LV,))),
        _acc("relu_bwd", "relu-bwd-n4", ("proj.hip", 277, "n % 4"), relu_bwd_ok, dict(n=4), (PJ, "test_relu_bwd_masks_by_the_output", ((1, 1, 1, 4),), (LV,))),
        _acc("scale_samples", "scale-samples-L4", ("triplet.hip", 642, "L % 4"), scale_samples_ok, dict(L=4, Bn=6),
             (HK, "test_scale_samples_and_scored_hinge_vs_torch64", (1, 4, ()), ())),
    ]
    return out


LOSS_EDGES = _loss_cases()

BN_CITE = ("bn.hip", 24, "g.C4 > 256 || (256 % g.C4)")
ROWS_CITE = ("bn.hip", 22, "rows < 1")


def _bn_cases():
    out = []
    join = lambda id, groups, N, H, C: _acc("bn", id, BN_CITE, bn_ok, dict(C=C, groups=groups, rows=N * H * H),
                                            (CK, "test_two_branch_batchnorm_join", (groups, N, H, C, True), ()))
    bn = lambda id, groups, N, H, C, relu=True, res=False, cite=BN_CITE: _acc(
        "bn", id, cite, bn_ok, dict(C=C, groups=groups, rows=N * H * H), (CK, "test_batchnorm_fwd_bwd", (groups, N, H, C, relu, res, True), ()))
    out += [
        bn("bn-C4", 2, 2, 3, 4, res=True), bn("bn-C1024", 1, 2, 2, 1024),
        # rows = 1: variance 0, y = beta; the unbiased estimate of the running variance keeps the biased one (bn.hip:87, n > 1 ? ... : var)
        _acc("bn", "bn-rows1", ROWS_CITE, bn_ok, dict(C=64, groups=2, rows=1), (SE, "check_batchnorm_one_row", (2, 64), (CK,))),
        _acc("bn", "bn-rows1-C1024", ROWS_CITE, bn_ok, dict(C=1024, groups=1, rows=1), (SE, "check_batchnorm_one_row", (1, 1024), (CK,))),
        # rows = 2: over two rows xhat = +-1 up to eps and the exact input gradient is (g1 - g2) / 2 * eps / (var + eps), 1e-6 ... 1e-5 for output
        # gradients of order 1 - the residue of a cancellation.  Formed in fp32 it missed the helpers' tolerances (gx 1.6e-4 / 6.6e-4 of
        # max |gx| against 5e-5, the join 8.2e-6 against 2e-6): groups of at most BN_SMALL_ROWS = 4 rows take their adjoint in double
        # (bn.hip bn_bwd_small_kernel, bn_join_bwd_small_kernel).  rows = 3 / 4 / 5: both sides of that switch
        bn("bn-rows2", 2, 2, 1, 64, cite=ROWS_CITE), bn("bn-rows2-res", 1, 2, 1, 8, res=True, cite=ROWS_CITE),
        _acc("bn", "bn-rows2-derived", ROWS_CITE, bn_ok, dict(C=64, groups=2, rows=2), (SE, "check_batchnorm_two_rows", (2, 64, False), (CK,))),
        _acc("bn", "bn-rows2-res-derived", ROWS_CITE, bn_ok, dict(C=8, groups=1, rows=2), (SE, "check_batchnorm_two_rows", (1, 8, True), (CK,))),
        bn("bn-rows3", 1, 3, 1, 64, cite=ROWS_CITE), bn("bn-rows3-2-groups", 2, 3, 1, 8, res=True, cite=ROWS_CITE),
        bn("bn-rows4", 2, 1, 2, 64, res=True, cite=("bn.hip", 988, "rows <= BN_SMALL_ROWS")), bn("bn-rows4-mask-from-x", 1, 4, 1, 16, cite=("bn.hip", 988, "rows <= BN_SMALL_ROWS")),
        bn("bn-rows5", 2, 5, 1, 64, res=True, cite=("bn.hip", 988, "rows <= BN_SMALL_ROWS")),
        join("bn-join-rows4", 2, 1, 2, 16), join("bn-join-rows5", 1, 5, 1, 16),
        # a prime row count below RPP * 4 (C = 64: RPP = 16): one chunk, the last row group of the workgroup partly filled
        bn("bn-rows61", 1, 61, 1, 64, cite=("bn.hip", 26, "rows / (g.RPP * 4)")),
        # the chunk count saturates at BN_MAX_CHUNKS = 256 (C = 1024: RPP = 1, rows >= 1024): rows = 4 * 256 + 1 -> 205 chunks of 5 rows
        bn("bn-rows1025-C1024", 1, 1025, 1, 1024, relu=False, cite=("bn.hip", 28, "n > BN_MAX_CHUNKS")),
        bn("bn-rows2049-C1024", 1, 2049, 1, 1024, cite=("bn.hip", 28, "n > BN_MAX_CHUNKS")),
        # groups = 1, and three groups whose rows (5 x 9 = 45, C = 16: RPP = 64) do not fill a chunk evenly
        bn("bn-groups3", 3, 5, 3, 16, res=True, cite=("bn.hip", 22, "groups < 1")),
    ]
    assert bn_chunks(1025, 1024) == (205, 5) and bn_chunks(2049, 1024) == (228, 9) and bn_chunks(61, 64) == (1, 61)
    mp = ("bn.hip", 1038, "groups * C * 8 > 32768")
    out += [
        join("bn-join-C4", 2, 2, 3, 4), join("bn-join-C1024", 1, 2, 2, 1024), join("bn-join-rows2", 1, 2, 1, 64),
        # bh_bn_maxpool_*: the largest groups * C its 32768-byte coefficient table admits (4 x 1024 x 8 bytes), and C = 4 on a 1 x 1 map
        _acc("bn", "bn-maxpool-4x1024", mp, bn_maxpool_ok, dict(C=1024, groups=4, N=4, Hi=2, Wi=3),
             (CK, "check_batchnorm_relu_maxpool_in_one_pass", (4, 4, 2, 3, 1024, True), ())),
        _acc("bn", "bn-maxpool-C4", mp, bn_maxpool_ok, dict(C=4, groups=1, N=5, Hi=1, Wi=1),
             (CK, "check_batchnorm_relu_maxpool_in_one_pass", (1, 5, 1, 1, 4, True), ())),
        _acc("bn_from_1x1", "bn-from-1x1-rows5", ("bn.hip", 1398, "rows <= BN_SMALL_ROWS) return BH_E_UNSUPPORTED"), bn_from_1x1_ok, dict(KC=16, C=32, rows=5),
             (CK, "test_batchnorm_adjoint_rebuilds_the_1x1_dgrad", (10, 1, 32, True), ())),
        _acc("bn_from_1x1", "bn-from-1x1-KC16-C32", ("bn.hip", 1396, "KC != 16 && KC != 32"), bn_from_1x1_ok, dict(KC=16, C=32, rows=2 * 64),
             (CK, "test_batchnorm_adjoint_rebuilds_the_1x1_dgrad", (2, 8, 32, True), ())),
        _acc("bn_from_1x1", "bn-from-1x1-KC32-C64", ("bn.hip", 1396, "KC != 16 && KC != 32"), bn_from_1x1_ok, dict(KC=32, C=64, rows=2 * 64),
             (CK, "test_batchnorm_adjoint_rebuilds_the_1x1_dgrad", (2, 8, 64, False), ())),
        # bh_bn_fwd_coeffs + BatchNorm-on-load at the smallest vector Ci of the 1x1 form
        _acc("bn", "bn-coeffs-1x1", ("bn.hip", 967, "bn_geom(groups, rows, C, g, -1)"), bn_ok, dict(C=32, groups=2, rows=128),
             (CK, "test_batchnorm_on_load_1x1_matches_materialised_batchnorm", (4, 8, 32, 16, True), ())),
    ]
    return out


BN_EDGES = _bn_cases()

BN1_CITE = ("bn1.hip", 16, "rows < 1")
BN1_EDGES = [
    # (groups, N, H, relu, res, training), N counting the images of all groups: rows = (N / groups) * H * H in {1 (eval: torch's training BatchNorm refuses one value), 3, 5, 4097 = 17 * 241};
    # two groups of an odd row count: the second group starts unaligned - the scalar branch of bn1_stats_kernel
    _acc("bn1", "bn1-rows1-eval", BN1_CITE, bn1_ok, dict(groups=1, rows=1), (ZH, "test_one_channel_batchnorm", (1, 1, 1, True, False, False), ())),
    _acc("bn1", "bn1-rows1", BN1_CITE, bn1_ok, dict(groups=2, rows=1), (SE, "check_batchnorm_one_row", (2, 1), (CK,))),
    _acc("bn1", "bn1-rows3", BN1_CITE, bn1_ok, dict(groups=1, rows=3), (ZH, "test_one_channel_batchnorm", (1, 3, 1, True, False, True), ())),
    _acc("bn1", "bn1-rows5", BN1_CITE, bn1_ok, dict(groups=1, rows=5), (ZH, "test_one_channel_batchnorm", (1, 5, 1, False, True, True), ())),
    _acc("bn1", "bn1-rows4097", ("bn1.hip", 18, "rows / 4096"), bn1_ok, dict(groups=1, rows=4097), (ZH, "test_one_channel_batchnorm", (1, 4097, 1, True, False, True), ())),
    _acc("bn1", "bn1-odd-rows-2-groups", ("bn1.hip", 41, "& 3) == 0"), bn1_ok, dict(groups=2, rows=9), (ZH, "test_one_channel_batchnorm", (2, 2, 3, True, True, True), ())),
    _acc("bn1", "bn1-rows4097-2-groups", ("bn1.hip", 41, "& 3) == 0"), bn1_ok, dict(groups=2, rows=4097), (ZH, "test_one_channel_batchnorm", (2, 8194, 1, True, False, True), ())),
]
assert bn1_scalar_branch(2, 9) and bn1_scalar_branch(2, 4097) and not bn1_scalar_branch(1, 5)

TAIL_CITE = ("tail.hip", 35, "Ci * Ci > 256 || Cm < 64 || Cm % 64 || Cm > 256 || Co < 1 || Co > 4")


def _tail_cases():
    out = []
    # (groups, N, H, Ci, Cm, Co, training, sparse): rows = N H H per group, hw = H H.  One image per group (rows = hw) at 4 x 4
    for Ci, Cm, Co in itertools.product((8, 16), (64, 256), (1, 4)):
        out.append(_acc("tail", "tail-%d-%d-%d" % (Ci, Cm, Co), TAIL_CITE, tail_ok, dict(Ci=Ci, Cm=Cm, Co=Co, groups=2, rows=16, hw=16),
                        (CK, "test_fused_tail_fwd_bwd", (2, 1, 4, Ci, Cm, Co, True, 0), ())))
    out += [
        # the smallest hw the geometry admits: 1 x 1 images (32 of them: batch statistics over a handful of rows are a cancellation, see BN_EDGES)
        _acc("tail", "tail-hw1", ("tail.hip", 36, "rows % hw"), tail_ok, dict(Ci=16, Cm=64, Co=2, groups=1, rows=32, hw=1),
             (CK, "test_fused_tail_fwd_bwd", (1, 32, 1, 16, 64, 2, True, 0), ())),
        _acc("tail", "tail-hw1-eval", ("tail.hip", 36, "rows % hw"), tail_ok, dict(Ci=8, Cm=64, Co=1, groups=1, rows=1, hw=1),
             (CK, "test_fused_tail_fwd_bwd", (1, 1, 1, 8, 64, 1, False, 0), ())),
        # Ci = 16, Co <= 2, rows % 32 == 0 and hw % 32 == 0: the smallest shape of the matrix-pipe forward (tail.hip, header: 32 pixels)
        _acc("tail", "tail-mfma-hw64", TAIL_CITE, tail_ok, dict(Ci=16, Cm=64, Co=2, groups=1, rows=64, hw=64),
             (CK, "test_fused_tail_fwd_bwd", (1, 1, 8, 16, 64, 2, True, 1), ())),
    ]
    return out


TAIL_EDGES = _tail_cases()

POOL_EDGES = (
    # check_maxpool_gap_add(N, H, W, C): MaxPool2d(3, 2, 1) and its adjoint, GAP and its adjoint, bh_add on 1001 elements; GAP and bh_add on
    # channel counts / lengths the max pool does not take: the same comparisons (test_shape_edges_gpu.py check_gap, check_add)
    [_acc("maxpool", "maxpool-%dx%d" % (h, w), ("pool.hip", 127, "Hi < 1 || Wi < 1"), maxpool_ok, dict(N=2, Hi=h, Wi=w, C=4),
          (CK, "check_maxpool_gap_add", (2, h, w, 4), ())) for h, w in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 3), (3, 2))]
    + [_acc("gap", "gap-HW%d-C%d" % (hw, C), ("pool.hip", 149, "HW < 1 || C < 1"), gap_ok, dict(N=2, HW=hw, C=C), (SE, "check_gap", (2, hw, C), (CK,)))
       for hw, C in ((1, 1), (1, 257), (7, 1), (7, 257))]
    + [_acc("add", "add-n%d" % n, ("pool.hip", 176, "n < 0"), add_ok, dict(n=n), (SE, "check_add", (n,), (CK,))) for n in (1, 2, 3, 4, 5)]
    + [_acc("absmax", "absmax-n%d" % n, ("pool.hip", 165, "n < 0"), absmax_ok, dict(n=n), (SE, "check_absmax", (n,), (CK,))) for n in (1, 3, 4, 5, 2049)]
)

DLT_CITE = ("geometry.hip", 591, "P < 4")
DLT_TOP = ("geometry.hip", 592, "P > 64 * DLT_MAXPTS")
GEOMETRY_EDGES = (
    # bh_dlt_fwd / _bwd: eight points per lane - P = 64 / 65: the first lane takes a second point; 511 / 512: the last lane's eighth
    [_acc("dlt", "dlt-P%d" % P, DLT_TOP if P > 64 else DLT_CITE, dlt_ok, dict(P=P, n=1), (SE, "check_dlt", (1, P), (HK,))) for P in (4, 5, 6, 63, 64, 65, 511, 512)]
    # bh_dsac_score / bh_dsac_scores_fwd / _bwd: one hypothesis per sample; a field of one point
    + [_acc("dsac", "dsac-soft-n%d-%dx%d" % (n, h, w), ("geometry.hip", 631, "n < 1 || h < 1 || w < 1"), dsac_ok, dict(n=n, h=h, w=w, method=2),
            (DS, "test_soft_scores_fwd_bwd_vs_torch64", (2, n, h, w), ())) for n, h, w in ((1, 5, 7), (1, 1, 1), (3, 1, 1), (2, 1, 5))]
    + [_acc("dsac", "dsac-hard-n%d-%dx%d" % (n, h, w), ("geometry.hip", 631, "n < 1 || h < 1 || w < 1"), dsac_ok, dict(n=n, h=h, w=w, method=1),
            (DS, "test_hard_counts_are_exact", (2, n, h, w), ())) for n, h, w in ((1, 5, 7), (1, 1, 1), (3, 1, 1))]
)

RANSAC_CITE = ("ransac.hip", 489, "(long long)h * w < 4")
RANSAC_EDGES = (
    # a 2 x 2 field is the smallest the entry accepts (four correspondences); K = 63 / 64 / 65 around one wave of hypotheses
    [_acc("ransac", "ransac-2x2-K%d" % K, ("ransac.hip", 489, "K < 1") if K == 1 else RANSAC_CITE, ransac_ok, dict(K=K, h=2, w=2),
          (SE, "check_ransac_exact_field", (2, K, 2, 2), ("test_ransac_gpu",))) for K in (1, 63, 64, 65)]
    + [_acc("ransac", "ransac-%dx%d-K%d" % (h, w, K), RANSAC_CITE, ransac_ok, dict(K=K, h=h, w=w),
            (SE, "check_ransac_exact_field", (2, K, h, w), ("test_ransac_gpu",))) for K, h, w in ((1, 5, 7), (65, 2, 3), (64, 3, 2))]
    # the polish: iters = 0 leaves the start, on the smallest field and on 5 x 7; ten steps on six correspondences (four fit exactly: cost 0)
    + [_acc("lm", "lm-%dx%d-iters%d" % (h, w, it), ("ransac.hip", 510, "iters < 0"), lm_ok, dict(h=h, w=w, iters=it),
            (SE, "check_lm", (h, w, it), ("test_ransac_lm_gpu",))) for h, w, it in ((2, 2, 0), (5, 7, 0), (2, 3, 10), (3, 2, 10))]
)

WARP_CITE = ("warp.hip", 326, "pool == 1 || pool == 2 || pool == 4 || pool == 8 || pool == 16 || pool == 32")
WARP_EDGES = (
    [_acc("warp", "warp-16x16-pool%d" % pool, WARP_CITE, warp_ok, dict(h=16, w=16, pool=pool), (HK, "check_warp_fwd_bwd", (2, 1, 16, 16, pool), ()))
     for pool in (1, 2, 4, 8, 16)]
    + [_acc("warp", "warp-32x32-pool32", WARP_CITE, warp_ok, dict(h=32, w=32, pool=32), (HK, "check_warp_fwd_bwd", (2, 1, 32, 32, 32), ())),
       _acc("warp", "warp-16x48-pool16", WARP_CITE, warp_ok, dict(h=16, w=48, pool=16), (HK, "check_warp_fwd_bwd", (2, 2, 16, 48, 16), ())),
       _acc("warp", "warp-48x16-pool16", WARP_CITE, warp_ok, dict(h=48, w=16, pool=16), (HK, "check_warp_fwd_bwd", (1, 1, 48, 16, 16), ())),
       _acc("warp", "warp-bwd-img-16x16", ("warp.hip", 390, "warp_shape_ok(h, w, 1)"), warp_ok, dict(h=16, w=16, pool=1),
            (ZH, "check_warp_adjoint_with_respect_to_the_image", (False, 16, 16), ())),
       _acc("warp", "warp-bwd-img-16x16-det", ("warp.hip", 390, "warp_shape_ok(h, w, 1)"), warp_ok, dict(h=16, w=16, pool=1),
            (ZH, "check_warp_adjoint_with_respect_to_the_image", (True, 16, 16), ()))]
    # bh_photo_warp_*: P = 16 on an image smaller than the patch (8 x 12) and on a one-pixel image
    + [_acc("photo_warp", "photo-warp-P16-%dx%d-C%d" % (Hi, Wi, C), ("photo.hip", 79, "(P % 16)"), photo_ok, dict(P=16, Hi=Hi, Wi=Wi, C=C),
            (PH, "test_photo_warp_fwd_and_adjoint_vs_float64", (C, None, 4, Hi, Wi, 16), ())) for Hi, Wi, C in ((8, 12, 1), (1, 1, 1), (1, 1, 3), (40, 56, 3))]
)

SYNTH_CITE = ("synth.hip", 195, "P % 16")
BLOB_CITE = ("blobs.hip", 212, "P < 16 || P % 16 || P > BLOB_MAX_P")
SYNTH_EDGES = (
    [_acc("synth", "pairs-all-points-P%d" % P, SYNTH_CITE, synth_ok, dict(P=P, C=1), (DG, "test_all_points_target", (P, P // 4, 3), ("bihome_amd.synth_gpu",))) for P in (16, 256)]
    + [_acc("synth", "pairs-rgb-P%d" % P, SYNTH_CITE, synth_ok, dict(P=P, C=3), (DG, "test_rgb_patches_match_host_arithmetic", (P, P // 4, 2, 32), ("bihome_amd.synth_gpu",)))
       for P in (16, 144)]
    # blobs: P = 16 (the smallest), 128 / 144 (the two sides of BLOB_LDS_P: 144 needs scratch), 256 (the largest); blobiness 0.1 is radius == P
    + [_acc("blobs", "blobs-field-P%d-b%g" % (P, bl), BLOB_CITE, blobs_ok, dict(P=P, blobiness=bl, B=2, C=C), (BL, "test_field_accuracy", (P, bl, 2, C), ("bihome_amd.synth_gpu",)))
       for P, bl, C in ((16, 0.1, 1), (16, 1.0, 3), (128, 0.1, 1), (144, 0.1, 1), (144, 0.5, 3), (256, 0.1, 1))]
    + [_acc("blobs", "blobs-mask-P%d" % P, BLOB_CITE, blobs_ok, dict(P=P, blobiness=0.5, B=2, C=3), (BL, "test_porosity_edges", (P, 0.5, 2, 3), ("bihome_amd.synth_gpu",)))
       for P in (16, 144)]
)
assert not blobs_needs_scratch(128) and blobs_needs_scratch(144)


# ---- convolutions --------------------------------------------------------------------------------------------------------------------
# Each conv case is (helper, arguments): HELPERS[helper] says how the GPU module runs it and launches_of() which launches of the library
# (descriptor, `which`, accumulate, bn_groups of bh_conv_variant) the helper makes - the census is held against those.
GEMM = "conv_gemm_kernel<"
DISPATCH = ("conv_gemm.hip", 874, "(a.Kc % 4 == 0) && (a.Cs % 4 == 0)")
BUF = ("conv_gemm.hip", 876, "(a.Nn % 4 == 0)")
TILE = ("conv_gemm.hip", 923, "if (a.Nn > 64) return launch<128, 128, 32, false>")
K16 = ("conv_gemm.hip", 930, "(a.Kc % 32) != 0 && a.Kc <= 16")
DESC = ("conv_gemm.hip", 1082, "d->Ho != (d->Hi + 2 * d->pad - d->kh) / d->stride + 1")
TDESC = ("conv_gemm.hip", 1078, "d->kh != d->stride || d->kw != d->stride || d->pad != 0")

# (id, cite, helper, arguments, expected kernel prefixes {which: prefix})
CONV_EDGE_CASES = [
    # scalar arm (!vec: Ci or Co of the operand in K position not a multiple of 4) at its three tile widths (Nn <= 32, <= 64, > 64)
    ("scalar-6-10", TILE, "conv2d", (1, 5, 5, 6, 10, 3, 1, 1), {"fwd": "conv_gemm_kernel<128,32,32,false", "dgrad": "conv_gemm_kernel<128,32,32,false"}),
    ("scalar-5-70", TILE, "conv2d", (1, 4, 6, 5, 70, 3, 1, 1), {"fwd": "conv_gemm_kernel<128,128,32,false", "dgrad": "conv_gemm_kernel<128,32,32,false"}),
    ("scalar-70-5", TILE, "conv2d", (1, 4, 6, 70, 5, 1, 1, 0), {"fwd": "conv_gemm_kernel<128,32,32,false", "dgrad": "conv_gemm_kernel<128,128,32,false"}),
    ("scalar-6-40", TILE, "conv2d", (1, 3, 3, 6, 40, 3, 1, 1), {"fwd": "conv_gemm_kernel<128,64,32,false", "dgrad": "conv_gemm_kernel<128,32,32,true,false,false>"}),
    ("scalar-40-6", TILE, "conv2d", (1, 3, 3, 42, 6, 3, 2, 1), {"fwd": "conv_gemm_kernel<128,32,32,false", "dgrad": "conv_gemm_kernel<128,64,32,false"}),
    # vector arm with Kc % 32 != 0: buffer loads off; Kc <= 16: the BK = 16 tiles at the three widths
    ("vec-12-8", K16, "conv2d", (1, 5, 7, 12, 8, 3, 1, 1), {"fwd": "conv_gemm_kernel<128,32,16,true,false,false>", "dgrad": "conv_gemm_kernel<128,32,16,true,false,false>"}),
    ("vec-12-40", K16, "conv2d", (1, 5, 7, 12, 40, 3, 1, 1), {"fwd": "conv_gemm_kernel<128,64,16,true,false,false>"}),
    ("vec-16-72", K16, "conv2d", (1, 5, 7, 16, 72, 1, 1, 0), {"fwd": "conv_gemm_kernel<128,128,16,true,false,false>"}),
    ("vec-24-40", BUF, "conv2d", (1, 5, 7, 24, 40, 3, 1, 1), {"fwd": "conv_gemm_kernel<64,64,32,true,false,false>", "dgrad": "conv_gemm_kernel<128,32,32,true,false,false>"}),
    ("vec-24-72", BUF, "conv2d", (1, 5, 7, 24, 72, 3, 1, 1), {"fwd": "conv_gemm_kernel<64,64,32,true,false,false>"}),
    # Co % 4 != 0 with a vector Ci: buffer loads switched off by Nn % 4
    ("vec-32-6", BUF, "conv2d", (1, 5, 7, 32, 6, 3, 1, 1), {"fwd": "conv_gemm_kernel<128,32,32,true,false,false>"}),
    ("vec-32-70", BUF, "conv2d", (1, 4, 4, 32, 70, 1, 1, 0), {"fwd": "conv_gemm_kernel<64,64,32,true,false,false>"}),
    ("vec-64-1", BUF, "conv2d", (1, 5, 7, 64, 1, 3, 1, 1), {"fwd": "conv_gemm_kernel<128,32,32,true,false,false>", "dgrad": "conv_gemm_kernel<128,64,32,false"}),
    ("co1-1x1", BUF, "conv2d", (1, 4, 4, 32, 1, 1, 1, 0), {"fwd": "conv_gemm_kernel<128,32,32,true,false,false>"}),
    ("ci1-co1", DISPATCH, "conv2d", (1, 3, 3, 1, 1, 3, 1, 1), {"fwd": "conv_gemm_kernel<128,32,32,false"}),
    # a 1 x 1 map under a 3x3 kernel with pad 1 (eight of nine taps fall outside), N = 1
    ("1x1-map-k3", DESC, "conv2d", (1, 1, 1, 64, 64, 3, 1, 1), {"fwd": GEMM, "dgrad": GEMM}),
    ("1x1-map-k3-s2", DESC, "conv2d", (1, 1, 1, 32, 32, 3, 2, 1), {"fwd": GEMM, "dgrad": GEMM}),
    ("1x1-map-k5", DESC, "conv2d", (1, 1, 1, 8, 12, 5, 1, 2), {"fwd": GEMM}),
    ("1x2-map-k7", DESC, "conv2d", (1, 1, 2, 4, 4, 7, 1, 3), {"fwd": GEMM}),
    ("2x2-map-k2", DESC, "conv2d", (1, 2, 2, 16, 8, 2, 2, 0), {"fwd": GEMM}),
    # long-K tiles of the fp32 vector arm: BK = 64 (Kc % 64 == 0, Kc >= 256) with and without buffer loads, the 64 x 128 tile
    ("k64-256-72", ("conv_gemm.hip", 932, "(a.Kc % 64) == 0 && a.Kc >= 256"), "conv2d", (1, 3, 3, 256, 72, 1, 1, 0), {"fwd": "conv_gemm_kernel<64,64,64,true,false,true>"}),
    ("k64-256-70", ("conv_gemm.hip", 932, "(a.Kc % 64) == 0 && a.Kc >= 256"), "conv2d", (1, 3, 3, 256, 70, 1, 1, 0), {"fwd": "conv_gemm_kernel<64,64,64,true,false,false>"}),
    # stride-2 adjoint on odd maps (no parity-class form): the gather dgrad, buffer loads off (a.adjoint && a.stride > 1)
    ("s2-odd-64-128", ("conv_gemm.hip", 876, "!(a.adjoint && a.stride > 1)"), "conv2d", (2, 5, 7, 64, 128, 3, 2, 1), {"dgrad": "conv_gemm_kernel<64,64,32,true,false,false>"}),
    # transposed conv with kernel == stride == 2 on a 1 x 1 map, N = 1; scalar and k16 forms; kernel == stride == 1
    ("convT-1x1-map", TDESC, "convT", (1, 1, 1, 64, 32), {"fwd": GEMM, "dgrad": GEMM}),
    ("convT-1x1-map-small", TDESC, "convT", (1, 1, 1, 4, 6), {"fwd": "conv_gemm_kernel<128,32,16,true,false,false>"}),
    ("convT-scalar", TDESC, "convT", (1, 2, 3, 6, 5), {"fwd": "conv_gemm_kernel<128,32,32,false"}),
    ("convT-24-24", TDESC, "convT", (1, 2, 3, 24, 24), {"fwd": "conv_gemm_kernel<64,64,32,true,false,false>"}),
    ("convT-12-40", TDESC, "convT", (1, 2, 3, 12, 40), {"fwd": "conv_gemm_kernel<128,128,16,true,false,false>"}),
    ("convT-5-20", TDESC, "convT", (1, 2, 3, 5, 20), {"fwd": "conv_gemm_kernel<128,128,32,false"}),
    ("convT-5-10", TDESC, "convT", (1, 2, 3, 5, 10), {"fwd": "conv_gemm_kernel<128,64,32,false"}),
    ("convT-8-10", TDESC, "convT", (1, 2, 3, 8, 10), {"fwd": "conv_gemm_kernel<128,64,16,true,false,false>"}),
    # the NCHW ends of the network at N = 1 on the smallest maps
    ("first-conv-1x1", DESC, "first_conv", (1, 1, 1, 2, 64), {"fwd": "conv_gemm_kernel<128,64,32,false"}),
    ("first-conv-ci4", DESC, "first_conv", (1, 5, 3, 4, 8), {"fwd": "conv_gemm_kernel<128,32,32,false"}),
    ("last-conv-1x1", DESC, "last_conv", (1, 1, 1, 128, 2), {"fwd": GEMM}),
    ("last-conv-co1", DESC, "last_conv", (1, 2, 3, 32, 1), {"fwd": GEMM}),
    ("last-conv-co3-ci6", DESC, "last_conv", (1, 2, 3, 6, 3), {"fwd": "conv_gemm_kernel<128,32,32,false"}),
    ("gray-stem-2x2", DESC, "gray_stem", (1, 2, 2, False), {"fwd": "conv_gemm_kernel<128,64,32,false", "dgrad": "stem_dgrad_c1_kernel<7,2>"}),
    # bf16 operands: the tiles of conv_gemm.hip:890-891 (Nn <= 32; 64-row tiles while the grid is small; 128-row tiles from 1024 on)
    ("bf16-32-32-1x1", ("conv_gemm.hip", 890, "if (a.Nn <= 32) { bm = 128; bn = 32; }"), "bf16", (1, 4, 32, 32, 1, 1, 0), {"fwd": "conv_gemm_kernel<128,32,32,true,true,true>"}),
    ("bf16-32-32-s2", ("conv_gemm.hip", 890, "if (a.Nn <= 32) { bm = 128; bn = 32; }"), "bf16", (1, 5, 32, 32, 3, 2, 1), {"dgrad": "conv_gemm_kernel<128,32,32,true,true,false>"}),
    ("bf16-64-64-s2", ("conv_gemm.hip", 891, "bn = 64"), "bf16", (1, 5, 64, 64, 3, 2, 1), {"fwd": "conv_gemm_kernel<64,64,32,true,true,true>", "dgrad": "conv_gemm_kernel<64,64,32,true,true,false>"}),
]

HALO = {"fwd": "conv3x3_halo_kernel<false,", "dgrad": "conv3x3_halo_kernel<true,"}
GRID_CITE = ("conv3x3.hip", 907, "BH_ROUTE_HALO_SMALL")
# the smallest grid the halo-tiled kernel takes without BH_ROUTE_HALO_SMALL, and one sub-tile pair below it (-> the generic kernel):
# (id, N, H, W, Ci, Co) with the default route
HALO_GRID_CASES = [
    # (id, N, H, W, Ci, Co, taken): 16 x 16 maps are four sub-tiles each
    ("halo-grid-64-at", 128, 16, 16, 64, 64, True), ("halo-grid-64-below", 127, 16, 16, 64, 64, False),          # 512 / 508 sub-tiles, one 64-channel tile
    ("halo-grid-64-128-at", 64, 16, 16, 64, 128, True), ("halo-grid-64-128-below", 63, 16, 16, 64, 128, False),  # 128 / 126 pairs x two tiles
    ("halo-grid-32-96-at", 43, 16, 16, 32, 96, True), ("halo-grid-32-96-below", 42, 16, 16, 32, 96, False),      # 86 / 84 pairs x three 32-channel tiles
]
assert C3_MIN_BLOCKS == 256 and all(halo_grid_ok(c[1], c[2], c[3], c[4], c[5]) == c[6] for c in HALO_GRID_CASES)
# 7x7 / 2 stems: the dedicated kernels from 256 tiles of 8 x 8 outputs (stem7.hip:437), the two-plane weight gradient from 512 (:863);
# one tile fewer routes to the generic kernels.  (id, helper, arguments, cite, accept, its arguments, taken)
STEM_CASES = [
    ("stem7-fwd-1-at", "stem7", (1, 16, 4096, 1, False), stem7_fwd_ok, dict(N=1, Hi=16, Wi=4096, Ci=1), True),
    ("stem7-fwd-2-at", "stem7", (1, 256, 256, 2, False), stem7_fwd_ok, dict(N=1, Hi=256, Wi=256, Ci=2), True),
    ("stem7-fwd-3-at", "stem7", (2, 128, 256, 3, True), stem7_fwd_ok, dict(N=2, Hi=128, Wi=256, Ci=3), True),
    ("stem7-fwd-f16-1-at", "stem7_f16", (2, 128, 256, 1, False, 1.0), stem7_fwd_ok, dict(N=2, Hi=128, Wi=256, Ci=1), True),
    ("stem7-fwd-f16-2-at", "stem7_f16", (2, 128, 256, 2, True, 1.0), stem7_fwd_ok, dict(N=2, Hi=128, Wi=256, Ci=2), True),
    ("stem7-fwd-1-below", "gray_stem", (1, 16, 4080, False), stem7_fwd_ok, dict(N=1, Hi=16, Wi=4080, Ci=1), False),
    ("stem7-fwd-2-below", "first_conv", (1, 240, 272, 2, 64), stem7_fwd_ok, dict(N=1, Hi=240, Wi=272, Ci=2), False),
    ("stem7-wgrad-at", "first_conv", (2, 256, 256, 2, 64), stem7_wgrad_ok, dict(N=2, Hi=256, Wi=256), True),
    ("stem7-wgrad-below", "first_conv", (1, 368, 352, 2, 64), stem7_wgrad_ok, dict(N=1, Hi=368, Wi=352), False),
]
assert 23 * 22 == 506 and 15 * 17 == 255
# bh_stem7_fwd_warp (stem7.hip `a.ntiles < 256`): accepted at 256 tiles (B, h, w, groups, with_cov, with_img, det), BH_E_UNSUPPORTED at 255
STEM_WARP_AT, STEM_WARP_BELOW = (2, 128, 256, 2, True, True, False), (1, 240, 272)
# split-operand weight gradient (wgrad_x3.hip:420-424): NO grid threshold and no route bit - one 8 x 8 tile of one image is taken; "one tile
# below" is a map that is no multiple of 8 (or 16-channel blocks): the stride-1 / small-channel kernels.  (N, H, W, Ci, Co, taken)
WGRAD_X3_GRID = [(1, 8, 8, 32, 32, True), (1, 8, 8, 64, 64, True), (1, 8, 16, 64, 32, True), (1, 4, 8, 64, 64, False), (1, 8, 12, 64, 64, False),
                 (1, 8, 8, 16, 32, False)]


def _find_line(fname, fragment):
    for i, line in enumerate(open(os.path.join(ROOT, "bihome_amd", "csrc", fname)).read().split("\n"), 1):
        if fragment in line:
            return i
    raise AssertionError("%s: %r not found" % (fname, fragment))


# ------------------------------------------------------------------------------------------------
# 2. refusals and empty batches: raw calls
# ------------------------------------------------------------------------------------------------
# the scalar arguments of a small valid call of every entry point the tables reach (by the header's argument names)
_LOSS = dict(B=2, hw=4, C=8, margin=0.5, mu=0.01, rep=1, flags=0, cosine=0, hinge=0)
_BN = dict(groups=1, rows=4, C=8, eps=1e-5, momentum=0.1, flags=0, use_running=0, eps_a=1e-5, eps_b=1e-5, momentum_a=0.1, momentum_b=0.1)
BASE = {
    "bh_h4pt_fwd": dict(B=2, W=128.0, H=128.0), "bh_h4pt_bwd": dict(B=2, W=128.0, H=128.0),
    "bh_dlt_fwd": dict(B=2, n=1, P=8, h=4, w=4), "bh_dlt_bwd": dict(B=2, n=1, P=8, h=4, w=4, flags=0),
    "bh_dsac_scores_fwd": dict(B=2, n=2), "bh_dsac_score": dict(B=2, n=2, h=4, w=4, method=0, thr=1.0, beta=1.0),
    "bh_dsac_scores_bwd": dict(B=2, n=2, h=4, w=4, method=0, thr=1.0, beta=1.0, flags=0),
    "bh_ransac_homography": dict(B=2, K=4, h=4, w=4, thr=1.0), "bh_homography_refine_lm": dict(B=2, h=4, w=4, iters=1),
    "bh_warp_fwd": dict(B=2, C=1, h=16, w=16, pool=4, flags=0), "bh_warp_bwd": dict(B=2, C=1, h=16, w=16, pool=4, flags=0),
    "bh_warp_bwd_img": dict(B=2, C=1, h=16, w=16, flags=0),
    "bh_photo_warp_fwd": dict(B=2, C=1, Hi=8, Wi=8, P=16, flags=0), "bh_photo_warp_bwd": dict(B=2, C=1, Hi=8, Wi=8, P=16, flags=0),
    "bh_triplet_l1_fwd": _LOSS, "bh_bihome_loss_fwd": dict(B=2, mu=0.01), "bh_bihome_loss_bwd": _LOSS, "bh_oneline_loss_fwd": _LOSS,
    "bh_oneline_loss_bwd": _LOSS, "bh_oneline_cos_loss_fwd": _LOSS, "bh_oneline_cos_loss_bwd": _LOSS, "bh_triplet_hinge_fwd": _LOSS,
    "bh_triplet_hinge_bwd": _LOSS, "bh_oneline_anchor_bwd": _LOSS, "bh_bihome_anchor_bwd": _LOSS,
    "bh_zhang_triplet_fwd": dict(B=2, hw=4, margin=0.5, hinge=1), "bh_zhang_triplet_bwd": dict(B=2, hw=4, hinge=1),
    "bh_mask_fwd": dict(N=2, P=4, strength=0.5), "bh_mask_bwd": dict(N=2, P=4, strength=0.5),
    "bh_scale_samples_fwd": dict(Bn=2, L=4, rep=1), "bh_scale_samples_bwd": dict(Bn=2, L=4, rep=1, flags=0),
    "bh_l2norm_fwd": dict(M=4, C=8), "bh_l2norm_bwd": dict(M=4, C=8), "bh_relu_bwd": dict(n=8), "bh_absmax": dict(n=8), "bh_add": dict(n=8),
    "bh_bn_fwd": _BN, "bh_bn_bwd": _BN, "bh_bn_stats": _BN, "bh_bn_fwd_coeffs": _BN, "bh_bn_join_fwd": _BN, "bh_bn_join_bwd": _BN,
    "bh_bn_join_bwd_remask": _BN, "bh_bn_bwd_from_1x1": dict(_BN, KC=16, rows=8),
    "bh_bn_maxpool_fwd": dict(_BN, N=1, Hi=2, Wi=4), "bh_bn_maxpool_bwd": dict(_BN, N=1, Hi=2, Wi=4),
    "bh_tail_fwd": dict(groups=1, rows=4, hw=4, Ci=8, Cm=64, Co=1, eps=1e-5, momentum=0.1, use_running=0, route=0),
    "bh_tail_bwd": dict(groups=1, rows=4, hw=4, Ci=8, Cm=64, Co=1, eps=1e-5, use_running=0, flags=0),
    "bh_synth_pairs": dict(B=2, n_images=1, Hs=32, Ws=32, P=16, mean=0.4, std=0.1),
    "bh_synth_batch": dict(B=2, n_images=1, Hs=32, Ws=32, P=16, C=1, mean=0.4, std=0.1),
    "bh_synth_image": dict(B=2, n_images=1, Hs=32, Ws=32, mean=0.4, std=0.1),
    "bh_synth_blobs": dict(B=2, C=1, P=16, sigma=1.0, porosity=0.3),
    "bh_maxpool3s2_fwd": dict(N=1, Hi=2, Wi=2, C=4), "bh_maxpool3s2_bwd": dict(N=1, Hi=2, Wi=2, C=4),
    "bh_gap_fwd": dict(N=1, HW=1, C=4), "bh_gap_bwd": dict(N=1, HW=1, C=4),
}

LOSS_ENTRIES = ("bh_triplet_l1_fwd", "bh_bihome_loss_bwd", "bh_oneline_loss_fwd", "bh_oneline_loss_bwd", "bh_oneline_cos_loss_fwd",
                "bh_oneline_cos_loss_bwd", "bh_triplet_hinge_fwd", "bh_triplet_hinge_bwd")
ANCHOR_ENTRIES = ("bh_oneline_anchor_bwd", "bh_bihome_anchor_bwd")
BN_ENTRIES = ("bh_bn_fwd", "bh_bn_bwd", "bh_bn_stats", "bh_bn_fwd_coeffs", "bh_bn_join_fwd", "bh_bn_join_bwd", "bh_bn_join_bwd_remask", "bh_bn_bwd_from_1x1",
              "bh_bn_maxpool_fwd", "bh_bn_maxpool_bwd")
BN_LINES = {"bh_bn_fwd": 949, "bh_bn_bwd": 984, "bh_bn_stats": 925, "bh_bn_fwd_coeffs": 967, "bh_bn_join_fwd": 1423, "bh_bn_join_bwd": 1445,
            "bh_bn_join_bwd_remask": 1445, "bh_bn_bwd_from_1x1": 1397, "bh_bn_maxpool_fwd": 1038, "bh_bn_maxpool_bwd": 1225}


def _ref(family, id, code, cite, accept, args, entry, over, null=()):
    return Case(family, id, False, cite, accept, args, (entry, dict(over), tuple(null), code))


def _refusals():
    out = []
    U, A = BH_E_UNSUPPORTED, BH_E_BADARG
    for e in LOSS_ENTRIES:
        for C in (6, 12, 24):
            out.append(_ref("loss", "%s-C%d" % (e, C), U, LOSS_CITE, loss_ok, dict(C=C), e, dict(C=C)))
        out.append(_ref("loss", "%s-C0" % e, U, LOSS_CITE, loss_ok, dict(C=0), e, dict(C=0)))
        out.append(_ref("loss", "%s-hw0" % e, A, ("triplet.hip", 483, "hw < 1"), loss_ok, dict(C=8, hw=0), e, dict(hw=0)))
        out.append(_ref("loss", "%s-B65536" % e, U, ("triplet.hip", 484, "B > 65535"), loss_ok, dict(C=8, B=65536), e, dict(B=65536)))
    for e in ("bh_oneline_loss_fwd", "bh_oneline_loss_bwd", "bh_oneline_cos_loss_fwd", "bh_oneline_cos_loss_bwd"):
        out.append(_ref("loss", "%s-B-rep" % e, A, ("triplet.hip", 483, "B % rep"), loss_ok, dict(C=8, B=4, rep=3), e, dict(B=4, rep=3)))
        out.append(_ref("loss", "%s-rep0" % e, A, ("triplet.hip", 483, "rep < 1"), loss_ok, dict(C=8, B=4, rep=0), e, dict(B=4, rep=0)))
    for e in ANCHOR_ENTRIES:
        for C in (6, 12, 24):
            out.append(_ref("loss", "%s-C%d" % (e, C), U, PROJ_CITE, loss_ok, dict(C=C), e, dict(C=C)))
        out.append(_ref("loss", "%s-hw0" % e, A, ("proj.hip", 288 if "oneline" in e else 306, "hw < 1"), loss_ok, dict(C=8, hw=0), e, dict(hw=0)))
    out.append(_ref("loss", "bh_oneline_anchor_bwd-B-rep", A, ("proj.hip", 288, "B % rep"), loss_ok, dict(C=8, B=4, rep=3), "bh_oneline_anchor_bwd", dict(B=4, rep=3)))
    for e in ("bh_l2norm_fwd", "bh_l2norm_bwd"):
        for C in (6, 12, 24):
            out.append(_ref("loss", "%s-C%d" % (e, C), U, PROJ_CITE, l2norm_ok, dict(C=C), e, dict(C=C)))
    out.append(_ref("relu_bwd", "relu-bwd-n6", A, ("proj.hip", 277, "n % 4"), relu_bwd_ok, dict(n=6), "bh_relu_bwd", dict(n=6)))
    for e in ("bh_scale_samples_fwd", "bh_scale_samples_bwd"):
        out.append(_ref("scale_samples", "%s-L6" % e, A, ("triplet.hip", 642 if e.endswith("fwd") else 651, "L % 4"), scale_samples_ok, dict(L=6), e, dict(L=6)))
        out.append(_ref("scale_samples", "%s-rep0" % e, A, ("triplet.hip", 642 if e.endswith("fwd") else 651, "rep < 1"), scale_samples_ok, dict(L=4, rep=0), e, dict(rep=0)))
    for e in BN_ENTRIES:
        for C in (12, 2048, 0):
            a = dict(C=C)
            over = dict(C=C)
            out.append(_ref("bn", "%s-C%d" % (e, C), U, ("bn.hip", BN_LINES[e], "bn_geom("), bn_ok, a, e, over))
    for e in ("bh_bn_fwd", "bh_bn_bwd", "bh_bn_stats", "bh_bn_fwd_coeffs", "bh_bn_join_fwd", "bh_bn_join_bwd", "bh_bn_join_bwd_remask", "bh_bn_bwd_from_1x1"):
        out.append(_ref("bn", "%s-rows0" % e, U, ("bn.hip", BN_LINES[e], "bn_geom("), bn_ok, dict(C=8, rows=0), e, dict(rows=0)))
        out.append(_ref("bn", "%s-groups0" % e, U, ("bn.hip", BN_LINES[e], "bn_geom("), bn_ok, dict(C=8, groups=0), e, dict(groups=0)))
    out.append(_ref("bn_from_1x1", "bn-from-1x1-KC8", U, ("bn.hip", 1396, "KC != 16 && KC != 32"), bn_from_1x1_ok, dict(KC=8), "bh_bn_bwd_from_1x1", dict(KC=8)))
    for rows in (1, 2, 4):
        out.append(_ref("bn_from_1x1", "bn-from-1x1-rows%d" % rows, U, ("bn.hip", 1398, "rows <= BN_SMALL_ROWS) return BH_E_UNSUPPORTED"), bn_from_1x1_ok,
                        dict(KC=16, rows=rows), "bh_bn_bwd_from_1x1", dict(rows=rows)))
    out.append(_ref("bn_from_1x1", "bn-from-1x1-KC64", U, ("bn.hip", 1396, "KC != 16 && KC != 32"), bn_from_1x1_ok, dict(KC=64), "bh_bn_bwd_from_1x1", dict(KC=64)))
    for e in ("bh_bn_maxpool_fwd", "bh_bn_maxpool_bwd"):
        line = 1035 if e.endswith("fwd") else 1222
        out.append(_ref("bn", "%s-N-groups" % e, A, ("bn.hip", line, "N % groups"), bn_maxpool_ok, dict(C=8, groups=2, N=3, Hi=2, Wi=4), e, dict(groups=2, N=3)))
        out.append(_ref("bn", "%s-N0" % e, A, ("bn.hip", line, "N < 1"), bn_maxpool_ok, dict(C=8, groups=1, N=0, Hi=2, Wi=4), e, dict(N=0)))
        # one, two and four rows per group: the fused forms have fp32 evaluation only (bn.hip BN_SMALL_ROWS) - refused, the unfused calls take them
        for Hi, Wi in ((1, 1), (1, 2), (2, 2)):
            out.append(_ref("bn", "%s-rows%d" % (e, Hi * Wi), U, ("bn.hip", 1039 if e.endswith("fwd") else 1226, "rows <= BN_SMALL_ROWS) return BH_E_UNSUPPORTED"), bn_maxpool_ok,
                            dict(C=8, groups=1, N=1, Hi=Hi, Wi=Wi), e, dict(Hi=Hi, Wi=Wi)))
    # one channel group more than the 32768-byte coefficient table of the fused BatchNorm + max pool holds
    out.append(_ref("bn", "bn-maxpool-8x1024", U, ("bn.hip", 1038, "groups * C * 8 > 32768"), bn_maxpool_ok, dict(C=1024, groups=8, N=8, Hi=2, Wi=2),
                    "bh_bn_maxpool_fwd", dict(C=1024, groups=8, N=8)))
    for e in ("bh_bn_fwd", "bh_bn_bwd"):
        out.append(_ref("bn1", "%s-C1-rows0" % e, U, ("bn1.hip", 178 if e.endswith("fwd") else 194, "bn1_geom("), bn1_ok, dict(groups=1, rows=0), e, dict(C=1, rows=0)))
    for e in ("bh_tail_fwd", "bh_tail_bwd"):
        line = 943 if e.endswith("fwd") else 989
        tc = ("tail.hip", line, "tail_geom(")
        for over in (dict(Ci=32), dict(Ci=4), dict(Ci=12), dict(Ci=24), dict(Cm=32), dict(Cm=320), dict(Cm=0), dict(Co=0), dict(Co=5), dict(hw=3), dict(hw=0), dict(rows=0)):
            a = dict(Ci=8, Cm=64, Co=1, groups=1, rows=4, hw=4)
            a.update(over)
            out.append(_ref("tail", "%s-%s" % (e, "-".join("%s%d" % kv for kv in over.items())), U, tc, tail_ok, a, e, over))
    for e in ("bh_dlt_fwd", "bh_dlt_bwd"):
        out.append(_ref("dlt", "%s-P3" % e, A, ("geometry.hip", 591 if e.endswith("fwd") else 602, "P < 4"), dlt_ok, dict(P=3), e, dict(P=3)))
        out.append(_ref("dlt", "%s-P513" % e, U, ("geometry.hip", 592 if e.endswith("fwd") else 603, "P > 64 * DLT_MAXPTS"), dlt_ok, dict(P=513), e, dict(P=513)))
        out.append(_ref("dlt", "%s-n0" % e, A, ("geometry.hip", 591 if e.endswith("fwd") else 602, "n < 1"), dlt_ok, dict(P=8, n=0), e, dict(n=0)))
    for e, line in (("bh_dsac_score", 631), ("bh_dsac_scores_bwd", 653)):
        out.append(_ref("dsac", "%s-n0" % e, A, ("geometry.hip", line, "n < 1"), dsac_ok, dict(n=0, h=4, w=4), e, dict(n=0)))
        out.append(_ref("dsac", "%s-h0" % e, A, ("geometry.hip", line, "h < 1"), dsac_ok, dict(n=2, h=0, w=4), e, dict(h=0)))
        out.append(_ref("dsac", "%s-method3" % e, A, ("geometry.hip", line - 2, "method != BH_DSAC_REPR_ERROR"), dsac_ok, dict(n=2, h=4, w=4, method=3), e, dict(method=3)))
        out.append(_ref("dsac", "%s-thr-1" % e, A, ("geometry.hip", line - 1, "thr < 0.f"), never, dict(), e, dict(thr=-1.0)))
    out.append(_ref("dsac", "bh_dsac_scores_bwd-hard", A, ("geometry.hip", 651, "method != BH_DSAC_REPR_ERROR && method != BH_DSAC_SOFT_INLIERS"), never, dict(), "bh_dsac_scores_bwd", dict(method=1)))
    out.append(_ref("dsac", "bh_dsac_scores_fwd-n0", A, ("geometry.hip", 620, "n < 1"), never, dict(), "bh_dsac_scores_fwd", dict(n=0)))
    out += [
        _ref("ransac", "ransac-1x3", A, RANSAC_CITE, ransac_ok, dict(K=4, h=1, w=3), "bh_ransac_homography", dict(h=1, w=3)),
        _ref("ransac", "ransac-K0", A, ("ransac.hip", 489, "K < 1"), ransac_ok, dict(K=0, h=4, w=4), "bh_ransac_homography", dict(K=0)),
        _ref("ransac", "ransac-thr-1", A, ("ransac.hip", 489, "!(thr >= 0.0f)"), never, dict(), "bh_ransac_homography", dict(thr=-1.0)),
        _ref("ransac", "ransac-B65536", U, ("ransac.hip", 490, "B > 65535"), ransac_ok, dict(K=1, h=2, w=2, B=65536), "bh_ransac_homography", dict(B=65536, K=1)),
        _ref("lm", "lm-1x3", A, ("ransac.hip", 510, "(long long)h * w < 4"), lm_ok, dict(h=1, w=3, iters=1), "bh_homography_refine_lm", dict(h=1, w=3)),
        _ref("lm", "lm-iters-1", A, ("ransac.hip", 510, "iters < 0"), lm_ok, dict(h=4, w=4, iters=-1), "bh_homography_refine_lm", dict(iters=-1)),
    ]
    for e, line in (("bh_warp_fwd", 335), ("bh_warp_bwd", 364)):
        c = ("warp.hip", line, "warp_shape_ok(h, w, pool)")
        for over in (dict(h=24), dict(w=24), dict(pool=3), dict(pool=64, h=64, w=64), dict(pool=0), dict(h=0), dict(pool=32)):
            a = dict(h=16, w=16, pool=4)
            a.update(over)
            out.append(_ref("warp", "%s-%s" % (e, "-".join("%s%d" % kv for kv in over.items())), U, c, warp_ok, a, e, over))
    out.append(_ref("warp", "bh_warp_bwd_img-h24", U, ("warp.hip", 390, "warp_shape_ok(h, w, 1)"), warp_ok, dict(h=24, w=16, pool=1), "bh_warp_bwd_img", dict(h=24)))
    out.append(_ref("warp", "bh_warp_bwd_img-C0", A, ("warp.hip", 389, "C < 1"), never, dict(), "bh_warp_bwd_img", dict(C=0)))
    for e, line in (("bh_photo_warp_fwd", 79), ("bh_photo_warp_bwd", 90)):
        out.append(_ref("photo_warp", "%s-P24" % e, U, ("photo.hip", line, "(P % 16)"), photo_ok, dict(P=24, Hi=8, Wi=8), e, dict(P=24)))
        out.append(_ref("photo_warp", "%s-P0" % e, A, ("photo.hip", line - 1, "P < 1"), photo_ok, dict(P=0, Hi=8, Wi=8), e, dict(P=0)))
        out.append(_ref("photo_warp", "%s-Hi0" % e, A, ("photo.hip", line - 1, "Hi < 1"), photo_ok, dict(P=16, Hi=0, Wi=8), e, dict(Hi=0)))
    for e in ("bh_synth_pairs", "bh_synth_batch"):
        out.append(_ref("synth", "%s-P24" % e, U, SYNTH_CITE, synth_ok, dict(P=24), e, dict(P=24)))
        out.append(_ref("synth", "%s-std0" % e, A, ("synth.hip", 193, "std == 0.f"), never, dict(), e, dict(std=0.0)))
    out.append(_ref("synth", "bh_synth_batch-C2", A, ("synth.hip", 193, "(C != 1 && C != 3)"), synth_ok, dict(P=16, C=2), "bh_synth_batch", dict(C=2)))
    out.append(_ref("synth", "bh_synth_image-Hs0", A, ("synth.hip", 182, "Hs < 1"), never, dict(), "bh_synth_image", dict(Hs=0)))
    for over, code, cite in ((dict(P=24), U, BLOB_CITE), (dict(P=0), U, BLOB_CITE), (dict(P=272), U, BLOB_CITE), (dict(B=1), A, ("blobs.hip", 209, "B < 2")),
                             (dict(C=2), A, ("blobs.hip", 209, "(C != 1 && C != 3)")), (dict(sigma=8.0), U, ("blobs.hip", 214, "r4 > (double)P + 1.0"))):
        a = dict(P=16, B=2, C=1, blobiness=16 / (40.0 * over.get("sigma", 0.8)))
        a.update({k: v for k, v in over.items() if k != "sigma"})
        out.append(_ref("blobs", "blobs-%s" % "-".join("%s%g" % kv for kv in over.items()), code, cite, blobs_ok, a, "bh_synth_blobs", over))
    # P = 144 needs scratch (the raw call hands none over: NULL)
    out.append(_ref("blobs", "blobs-P144-no-scratch", A, ("blobs.hip", 217, "P > BLOB_LDS_P && !scratch"), never, dict(), "bh_synth_blobs", dict(P=144, sigma=7.2), ("scratch",)))
    for e in ("bh_maxpool3s2_fwd", "bh_maxpool3s2_bwd"):
        line = 127 if e.endswith("fwd") else 138
        out.append(_ref("maxpool", "%s-C6" % e, U, ("pool.hip", line + 1, "C % 4"), maxpool_ok, dict(N=1, Hi=2, Wi=2, C=6), e, dict(C=6)))
        for over in (dict(Hi=0), dict(Wi=0), dict(C=0), dict(N=-1)):
            a = dict(N=1, Hi=2, Wi=2, C=4)
            a.update(over)
            out.append(_ref("maxpool", "%s-%s" % (e, "-".join("%s%d" % kv for kv in over.items())), A, ("pool.hip", line, "N < 0 || Hi < 1 || Wi < 1 || C < 4"), maxpool_ok, a, e, over))
    for e in ("bh_gap_fwd", "bh_gap_bwd"):
        line = 149 if e.endswith("fwd") else 157
        for over in (dict(HW=0), dict(C=0), dict(N=-1)):
            a = dict(N=1, HW=1, C=4)
            a.update(over)
            out.append(_ref("gap", "%s-%s" % (e, "-".join("%s%d" % kv for kv in over.items())), A, ("pool.hip", line, "N < 0 || HW < 1 || C < 1"), gap_ok, a, e, over))
    for e, line in (("bh_mask_fwd", 89), ("bh_mask_bwd", 98)):
        out.append(_ref("mask", "%s-P0" % e, A, ("mask.hip", line, "P < 1"), never, dict(), e, dict(P=0)))
    out.append(_ref("mask", "bh_mask_fwd-g-without-f", A, ("mask.hip", 89, "(g && !f)"), never, dict(), "bh_mask_fwd", dict(), ("f",)))
    out.append(_ref("loss", "bh_zhang_triplet_fwd-hw0", A, ("triplet.hip", 545, "hw < 1"), never, dict(), "bh_zhang_triplet_fwd", dict(hw=0)))
    out.append(_ref("loss", "bh_zhang_triplet_bwd-hw0", A, ("triplet.hip", 558, "hw < 1"), never, dict(), "bh_zhang_triplet_bwd", dict(hw=0)))
    out.append(_ref("scale_samples", "bh_scale_samples_bwd-g_x-rep3", A, ("triplet.hip", 651, "(g_x && rep != 1)"), never, dict(), "bh_scale_samples_bwd", dict(rep=3)))
    out.append(_ref("warp", "bh_warp_fwd-img-without-out", A, ("warp.hip", 334, "(img && !out)"), never, dict(), "bh_warp_fwd", dict(), ("out",)))
    out.append(_ref("warp", "bh_warp_fwd-nothing-asked", A, ("warp.hip", 334, "(!img && !cov)"), never, dict(), "bh_warp_fwd", dict(), ("img", "cov")))
    out.append(_ref("warp", "bh_warp_bwd-g_out-without-img", A, ("warp.hip", 363, "(g_out && !img)"), never, dict(), "bh_warp_bwd", dict(), ("img",)))
    out.append(_ref("warp", "bh_warp_bwd_img-det-without-scratch", A, ("warp.hip", 389, "((flags & BH_F_DETERMINISTIC) && !scratch)"), never, dict(), "bh_warp_bwd_img", dict(flags=1), ("scratch",)))
    for e, line in (("bh_photo_warp_fwd", 78), ("bh_photo_warp_bwd", 89)):
        out.append(_ref("photo_warp", "%s-C0" % e, A, ("photo.hip", line, "C < 1"), never, dict(), e, dict(C=0)))
        out.append(_ref("photo_warp", "%s-Wi0" % e, A, ("photo.hip", line, "Wi < 1"), photo_ok, dict(P=16, Hi=8, Wi=0), e, dict(Wi=0)))
    out.append(_ref("synth", "bh_synth_image-n_images0", A, ("synth.hip", 182, "n_images < 1"), never, dict(), "bh_synth_image", dict(n_images=0)))
    out.append(_ref("synth", "bh_synth_batch-n_images0", A, ("synth.hip", 193, "n_images < 1"), never, dict(), "bh_synth_batch", dict(n_images=0)))
    out.append(_ref("add", "add-n-1", A, ("pool.hip", 176, "n < 0"), add_ok, dict(n=-1), "bh_add", dict(n=-1)))
    out.append(_ref("absmax", "absmax-n-1", A, ("pool.hip", 165, "n < 0"), absmax_ok, dict(n=-1), "bh_absmax", dict(n=-1)))
    out.append(_ref("absmax", "absmax-misaligned", A, ("pool.hip", 165, "& 15"), absmax_ok, dict(n=8, misaligned=4), "bh_absmax", dict(_misalign=("x", 4))))
    return out


REFUSALS = _refusals()

# a NULL for each required pointer of one entry point per file: (entry point, file, line of the check, required pointers)
NULL_CASES = [
    ("bh_dlt_fwd", "geometry.hip", 591, ("pf", "choice", "Hdlt", "delta_hat", "eig")),
    ("bh_ransac_homography", "ransac.hip", 488, ("pf", "choice", "hyp", "count", "best", "n_inl", "work", "H", "delta_hat")),
    ("bh_warp_bwd", "warp.hip", 363, ("H64", "gH")),
    ("bh_photo_warp_bwd", "photo.hip", 89, ("img", "Hp64", "origin", "g_out", "gH")),
    ("bh_triplet_hinge_bwd", "triplet.hip", 482, ("g_loss", "f1", "f2", "f1w", "f2w", "m1w", "m2w", "M1", "M2", "numden", "H1", "H2", "g_f1w", "g_f2w", "g_m1w",
                                                  "g_m2w", "gH1", "gH2")),
    ("bh_oneline_anchor_bwd", "proj.hip", 243, ("g_loss", "f1", "f2", "f1w", "m1w", "T", "numden", "g_f1", "g_f2")),
    ("bh_bn_bwd", "bn.hip", 980, ("gy", "x", "gx", "stats", "scratch")),
    ("bh_tail_bwd", "tail.hip", 988, ("gout", "x", "w1", "w2", "ws", "scratch")),
    ("bh_mask_fwd", "mask.hip", 89, ("y", "m", "smax", "imax")),
    ("bh_synth_batch", "synth.hip", 193, ("images", "img_idx", "origin", "Hpatch", "patch1", "patch2")),
    ("bh_synth_blobs", "blobs.hip", 209, ("noise", "other", "patch1", "patch2", "mask")),
    ("bh_add", "pool.hip", 176, ("a", "b", "out")),
]

# every entry point whose check is `B < 0` / `N < 0` / `n < 0`: (entry point, the count's name, file, line of the early return,
# outputs still written: name -> (dtype, values))
EMPTY_BATCH = [
    ("bh_h4pt_fwd", "B", "geometry.hip", 573, {}), ("bh_h4pt_bwd", "B", "geometry.hip", 582, {}),
    ("bh_dlt_fwd", "B", "geometry.hip", 593, {}), ("bh_dlt_bwd", "B", "geometry.hip", 604, {}),
    ("bh_dsac_scores_fwd", "B", "geometry.hip", 621, {}), ("bh_dsac_score", "B", "geometry.hip", 633, {}), ("bh_dsac_scores_bwd", "B", "geometry.hip", 655, {}),
    ("bh_ransac_homography", "B", "ransac.hip", 491, {}), ("bh_homography_refine_lm", "B", "ransac.hip", 512, {}),
    ("bh_warp_fwd", "B", "warp.hip", 336, {}), ("bh_warp_bwd", "B", "warp.hip", 365, {}), ("bh_warp_bwd_img", "B", "warp.hip", 391, {}),
    ("bh_photo_warp_fwd", "B", "photo.hip", 80, {}), ("bh_photo_warp_bwd", "B", "photo.hip", 91, {}),
    ("bh_triplet_l1_fwd", "B", "triplet.hip", 493, {}), ("bh_triplet_hinge_fwd", "B", "triplet.hip", 493, {}),
    ("bh_bihome_loss_bwd", "B", "triplet.hip", 509, {}), ("bh_triplet_hinge_bwd", "B", "triplet.hip", 509, {}),
    ("bh_oneline_loss_bwd", "B", "triplet.hip", 509, {}), ("bh_oneline_cos_loss_bwd", "B", "triplet.hip", 509, {}),
    # (the forwards of the losses that END in a sum over the batch write the sum of nothing: a zero loss)
    ("bh_oneline_loss_fwd", "B", "triplet.hip", 493, {"loss": (0.0,)}), ("bh_oneline_cos_loss_fwd", "B", "triplet.hip", 493, {"loss": (0.0,)}),
    ("bh_bihome_loss_fwd", "B", "triplet.hip", 621, {"loss4": (0.0, 0.0, 0.0, 0.0)}),
    ("bh_oneline_anchor_bwd", "B", "proj.hip", 290, {}), ("bh_bihome_anchor_bwd", "B", "proj.hip", 307, {}),
    ("bh_zhang_triplet_fwd", "B", "triplet.hip", 546, {}), ("bh_zhang_triplet_bwd", "B", "triplet.hip", 560, {}),
    ("bh_mask_fwd", "N", "mask.hip", 90, {}), ("bh_mask_bwd", "N", "mask.hip", 99, {}),
    ("bh_scale_samples_fwd", "Bn", "triplet.hip", 643, {}), ("bh_scale_samples_bwd", "Bn", "triplet.hip", 652, {}),
    ("bh_l2norm_fwd", "M", "proj.hip", 260, {}), ("bh_l2norm_bwd", "M", "proj.hip", 269, {}), ("bh_relu_bwd", "n", "proj.hip", 278, {}),
    ("bh_absmax", "n", "pool.hip", 166, {}), ("bh_add", "n", "pool.hip", 177, {}),
    ("bh_maxpool3s2_fwd", "N", "pool.hip", 129, {}), ("bh_maxpool3s2_bwd", "N", "pool.hip", 140, {}),
    ("bh_gap_fwd", "N", "pool.hip", 150, {}), ("bh_gap_bwd", "N", "pool.hip", 158, {}),
    ("bh_synth_pairs", "B", "synth.hip", 196, {}), ("bh_synth_batch", "B", "synth.hip", 196, {}), ("bh_synth_image", "B", "synth.hip", 183, {}),
]
EMPTY_CASES = [Case("empty", "%s-%s0" % (e, n), True, (f, line, "== 0) return BH_OK" if not w or e.startswith("bh_oneline") else "B == 0"), always, {n: 0}, (e, {n: 0}, (), BH_OK))
               for e, n, f, line, w in EMPTY_BATCH]

BUF_BYTES = 1 << 16
NAN_BITS = 0x7FC00000


class RawCall:
    """One call of a C entry point on poisoned 64 KiB buffers (one per pointer argument, every 32-bit word a float NaN), the scalars from
    BASE with the case's values laid over them.  The buffers are device memory where there is a GPU and host memory where there is none:
    a call that is refused (or returns for an empty batch) BEFORE ANY LAUNCH never looks at them - which is what running the tables on a
    machine without a GPU shows (tests/test_shape_edges_cpu.py)."""

    def __init__(self, entry, over, null=()):
        import torch
        from bihome_amd._lib import lib
        self.entry = entry
        self.cuda = torch.cuda.is_available()
        scalars = dict(BASE[entry])
        misalign = over.get("_misalign")
        scalars.update({k: v for k, v in over.items() if not k.startswith("_")})
        self.bufs, cargs = {}, []
        for cls, name in header_prototypes()[entry][1]:
            if cls != "ptr":
                cargs.append(scalars[name])
            elif name == "stream":
                cargs.append(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if self.cuda else None)
            elif name in null:
                cargs.append(None)
            else:
                t = torch.full((BUF_BYTES // 4,), NAN_BITS, dtype=torch.int32, device="cuda" if self.cuda else "cpu")
                self.bufs[name] = t
                cargs.append(ctypes.c_void_p(t.data_ptr() + (misalign[1] if misalign and misalign[0] == name else 0)))
        self.before = {k: t.clone() for k, t in self.bufs.items()}
        if self.cuda:
            torch.cuda.synchronize()
        self.rc = getattr(lib, entry)(*cargs)
        if self.cuda:
            torch.cuda.synchronize()

    def untouched(self, but=()):
        import torch
        bad = [k for k, t in self.bufs.items() if k not in but and not torch.equal(t, self.before[k])]
        assert not bad, "%s wrote into %s" % (self.entry, bad)


ALL_TABLES = [LOSS_EDGES, BN_EDGES, BN1_EDGES, TAIL_EDGES, POOL_EDGES, GEOMETRY_EDGES, RANSAC_EDGES, WARP_EDGES, SYNTH_EDGES, REFUSALS, EMPTY_CASES]


# ------------------------------------------------------------------------------------------------
# 3. the dispatch census
# ------------------------------------------------------------------------------------------------
CHANNELS = (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 40, 64, 70, 96, 128, 256, 512)
EXTENTS = (1, 2, 4, 8, 16, 20, 32, 64, 128)
BATCHES = (1, 2, 3, 128)
ROUTES = (0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
# (k, stride, pad, transposed)
GEOMETRIES = ((1, 1, 0, 0), (1, 2, 0, 0), (2, 2, 0, 1), (3, 1, 1, 0), (3, 2, 1, 0), (7, 2, 3, 0), (5, 1, 2, 0), (7, 1, 3, 0), (2, 1, 0, 0), (2, 2, 0, 0),
              (1, 1, 0, 1), (5, 2, 2, 0))
WHICH = {"fwd": 0, "dgrad": 1, "wgrad": 2, "wgrad_det": 3, "dgrad_bnr_z": 4, "dgrad_bnr_y": 5, "dgrad_colsum": 6}
PACKED_LAYOUT = {0: 1, 1: 1, 2: 2, 3: 3, 4: 4}
FIELDS = ("N", "H", "W", "Ci", "Co", "k", "s", "p", "T", "in_nchw", "out_nchw", "precision", "w_layout", "route", "which", "accumulate", "bn_groups")


def describe(key):
    return " ".join("%s=%s" % kv for kv in zip(FIELDS, key))


class _Query:
    """bh_conv_variant on one reused descriptor (no GPU: the library's dispatch with the launches replaced by a name record)."""

    def __init__(self):
        from bihome_amd._lib import BhConvDesc, lib
        self.lib, self.d = lib, BhConvDesc()
        self.ref = ctypes.byref(self.d)
        self.buf = ctypes.create_string_buffer(256)
        self.calls = 0

    def geometry(self, N, H, W, Ci, Co, k, s, p, T, inn=0, outn=0):
        d = self.d
        d.N, d.Hi, d.Wi, d.Ci, d.Co, d.kh, d.kw, d.stride, d.pad, d.transposed, d.in_nchw, d.out_nchw = N, H, W, Ci, Co, k, k, s, p, T, inn, outn
        if T:
            d.Ho, d.Wo = H * s, W * s
        else:
            d.Ho, d.Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self.geo = (N, H, W, Ci, Co, k, s, p, T, inn, outn)

    def ask(self, prec, lay, route, which, acc, bng):
        d = self.d
        d.precision, d.w_layout, d.route = prec, lay, route
        d.a_bound = d.b_bound = 256 if prec == 4 else None      # (routing does not read the records; a precision-4 launch without one is refused)
        self.calls += 1
        if self.lib.bh_conv_variant(self.ref, which, acc, bng, self.buf, 256) != 0:
            return ()
        return self.buf.value.decode().split("+")


ALL_LAUNCHES = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (1, 0, 0), (1, 1, 0), (2, 0, 0), (3, 0, 0), (4, 0, 1), (4, 1, 2), (5, 0, 1), (5, 1, 2), (6, 0, 0)]
PLAIN_LAUNCHES = [(0, 0, 0), (0, 0, 2), (1, 0, 0), (1, 1, 0), (2, 0, 0), (3, 0, 0)]


def dispatch_census():
    """-> ({kernel name: the first descriptor that reached it}, number of queries).  The full cross product of the grid (batches x extents^2
    x channels^2 x geometries x layouts x precisions x routes x launches) is beyond 10^10 queries; three overlapping sub-grids cover what
    each axis can change:
      A  every channel pair x every geometry x the NCHW ends, fp32, default route: the arms and tiles of conv_gemm.hip dispatch() and of
         the weight-gradient routing (wgrad.hip) - they are decided by channel counts, taps and the pixel count;
      B  every precision x weight layout x route bit x launch kind on the channel counts the matrix-pipe kernels take, 3x3 / stride 1
         (halo-tiled, persistent, split-operand weight gradient); precisions and the routes of the generic kernel on the other geometries;
      C  every H x W of the grid on two channel pairs: the tile-count thresholds."""
    q = _Query()
    names = {}

    def sweep(batches, extents, chans, geoms, precs, routes, launches, layouts):
        for N, (H, W), (Ci, Co), (k, s, p, T) in itertools.product(batches, extents, chans, geoms):
            if not T and (H + 2 * p < k or W + 2 * p < k):
                continue
            for inn, outn in ((0, 0), (1, 0), (0, 1)):
                if (inn and (Ci > 4 or T)) or (outn and (Co > 4 or T)):
                    continue
                q.geometry(N, H, W, Ci, Co, k, s, p, T, inn, outn)
                for prec in precs:
                    for lay in ((0, PACKED_LAYOUT[prec]) if layouts and (k, s, T) == (3, 1, 0) else (0,)):
                        for route in routes:
                            for which, acc, bng in launches:
                                for nm in q.ask(prec, lay, route, which, acc, bng):
                                    if nm not in names:
                                        names[nm] = q.geo + (prec, lay, route, which, acc, bng)

    square = [(e, e) for e in EXTENTS]
    rect = square + [(8, 16), (16, 8), (16, 20), (4, 8), (1, 2), (16, 32), (64, 128), (1, 128), (128, 4)]
    sweep(BATCHES, [(1, 1), (4, 4), (8, 8), (16, 16), (20, 20), (64, 64), (128, 128), (8, 16), (1, 128)], list(itertools.product(CHANNELS, CHANNELS)), GEOMETRIES, (0,), (0,),
          [(0, 0, 0), (1, 0, 0), (2, 0, 0)], False)
    mfma = [(16, 16), (32, 32), (64, 64), (32, 64), (64, 32), (96, 64), (64, 128), (128, 128), (256, 256), (512, 512), (1, 64), (2, 64), (3, 64), (128, 2), (32, 16), (32, 1), (64, 1)]
    sweep((1, 2, 128), rect, mfma, GEOMETRIES[3:4], range(5), ROUTES + (2 | 512, 2 | 256, 2 | 32, 2 | 64), ALL_LAUNCHES, True)
    sweep((1, 2, 128), rect, mfma, GEOMETRIES[:3] + GEOMETRIES[4:6], (0, 1, 2, 4), (0, 128, 4096), PLAIN_LAUNCHES, False)
    sweep(BATCHES, list(itertools.product(EXTENTS, EXTENTS)), [(64, 64), (32, 32), (1, 64), (2, 64)], GEOMETRIES[:4] + GEOMETRIES[5:6], (0, 4), (0, 2),
          [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)], True)
    return names, q.calls


# ---- what the suite's float64-checked conv cases launch ----------------------------------------------------------------------------------
def _parametrized(module, fn):
    """The argument tuples of the parametrize marks of a test function (the product of stacked marks, in the order of the signature)."""
    f = getattr(importlib.import_module(module), fn)
    marks = [m for m in getattr(f, "pytestmark", []) if m.name == "parametrize"]
    names, values = [], []
    for m in marks:
        ns = [n.strip() for n in m.args[0].split(",")]
        names.append(ns)
        values.append([v if isinstance(v, (tuple, list)) and len(ns) > 1 else (v,) for v in m.args[1]])
    out = []
    for combo in itertools.product(*values):
        out.append({n: v for ns, vs in zip(names, combo) for n, v in zip(ns, vs)})
    return out


class Launches:
    """The launches a helper of the test files makes, as (geometry, precision, w_layout, route, which, accumulate, bn_groups) - restated from
    the helper's code and from the routing of bihome_amd/kernels.py (conv_dgrad takes bh_conv_dgrad_s2 / the stem forms for some
    geometries: those launches are not bh_conv_dgrad's, and are left out).  tests/test_shape_edges_gpu.py holds the restatement against
    what the wrappers report to kernels.TIMING when a helper runs - for the cases THAT module runs (test_conv_edge); for the older tables
    the restatement stands on the reading of their helpers.  "float64-checked" is transitive for three helpers: `pc` / `pc_reduce` hold the
    persistent kernel bit for bit against the halo kernel (which the f16x2 helper holds against float64 on the same shapes), `bnreduce`
    holds the dgrad with BatchNorm sums against the three-launch adjoint (held against float64 by test_batchnorm_fwd_bwd)."""
    HALO_SMALL, GENERIC, NO_STEM7, WG_GENERIC, WG_3TAP, TILE_WG, C3_PC, WX3_PC, GEMM_X3 = 2, 1, 4, 8, 16, 256, 512, 1024, 4096

    def __init__(self):
        self.q = _Query()
        self.names = set()

    def add(self, N, H, W, Ci, Co, k, s, p, T=0, inn=0, outn=0, prec=0, lay=0, route=0, which="fwd", acc=0, bng=0):
        self.q.geometry(N, H, W, Ci, Co, k, s, p, T, inn, outn)
        got = self.q.ask(prec, lay, route, WHICH[which], acc, bng)
        self.names.update(got)
        return got

    def det_bytes(self, N, H, W, Ci, Co, k, s, p, prec, route=0):
        self.q.geometry(N, H, W, Ci, Co, k, s, p, 0)
        d = self.q.d
        d.precision, d.w_layout, d.route = prec, 0, route
        d.a_bound = d.b_bound = 256 if prec == 4 else None
        return int(self.q.lib.bh_conv_wgrad_det_bytes(self.q.ref))

    # kernels.conv_dgrad's routing in front of bh_conv_dgrad
    @staticmethod
    def dgrad_is_plain(N, H, W, Ci, Co, k, s, p, T=0, inn=0, outn=0, acc=0):
        Ho, Wo = ((H * s, W * s) if T else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1))
        if not acc and not T and k == 7 and s == 2 and not outn and (Ci == 1 or (Ci == 3 and inn)) and Co % 4 == 0 and N * Ho * Wo >= 4096:
            return False
        if (not T and s == 2 and not inn and not outn and Co % 4 == 0 and Ci % 4 == 0 and H % 2 == 0 and W % 2 == 0 and Ho * 2 == H and Wo * 2 == W
                and ((k == 3 and p == 1) or (k == 1 and p == 0))):
            return False
        return True

    def wgrad(self, g, prec=0, route=0, ws=False, **kw):
        """kernels.conv_wgrad: the workspace form where a workspace is handed over and the shape has one, else bh_conv_wgrad"""
        N, H, W, Ci, Co, k, s, p = g
        if kw.get("inn") and k == 7 and s == 2 and Ci == 2 and stem7_wgrad_ok(N, H, W, Ci):
            return                                                        # (bh_stem7_wgrad: not a launch bh_conv_variant describes)
        if ws and not kw.get("T") and self.det_bytes(N, H, W, Ci, Co, k, s, p, prec, route) > 0:
            self.add(*g, prec=prec, route=route, which="wgrad_det", **kw)
        else:
            self.add(*g, prec=prec, route=route, which="wgrad", **kw)

    # ---- the helpers ----
    def conv2d(self, N, H, W, Ci, Co, k, s, p, route=0, prec=0):
        """check_conv2d_fwd_dgrad_wgrad (precision 0) / test_bf16_operand_mode (precision 1: no accumulating dgrad)"""
        g = (N, H, W, Ci, Co, k, s, p)
        self.add(*g, prec=prec, route=route)
        for acc in ((0, 1) if prec == 0 else (0,)):
            if self.dgrad_is_plain(*g, acc=acc):
                self.add(*g, prec=prec, route=route, which="dgrad", acc=acc)
        self.wgrad(g, prec, route)

    def bf16(self, N, H, Ci, Co, k, s, p):
        self.conv2d(N, H, H, Ci, Co, k, s, p, prec=1)

    def convT(self, N, H, W, Ci, Co):
        g = (N, H, W, Ci, Co, 2, 2, 0)
        self.add(*g, T=1)
        self.add(*g, T=1, which="dgrad")
        self.wgrad(g, T=1)

    def first_conv(self, N, H, W, Ci, Co):
        g = (N, H, W, Ci, Co, 7, 2, 3)
        self.add(*g, inn=1)
        self.wgrad(g, inn=1)

    def last_conv(self, N, H, W, Ci=128, Co=2):
        g = (N, H, W, Ci, Co, 1, 1, 0)
        self.add(*g, outn=1)
        self.add(*g, outn=1, which="dgrad")
        self.wgrad(g, outn=1)

    def gray_stem(self, N, H, W, det=False):
        g = (N, H, W, 1, 64, 7, 2, 3)
        self.add(*g)
        if self.dgrad_is_plain(*g):
            self.add(*g, which="dgrad")
        else:
            Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
            if not (Ho % 8 == 0 and Wo % 8 == 0 and Ho * 2 == H and Wo * 2 == W):
                self.add(N, Ho, Wo, 64, 52, 1, 1, 0)                      # the two-step form: a 1x1 launch into the tap table

    def stem7(self, N, H, W, Ci, relu=False):
        """check_stem7_forward_kernel: the stem kernel and the generic one on the same data (relu: bh_conv_fwd_act routes alike)"""
        g = (N, H, W, Ci, 64, 7, 2, 3)
        self.add(*g, inn=int(Ci != 1))
        self.add(*g, inn=int(Ci != 1), route=self.NO_STEM7)

    def stem7_f16(self, N, H, W, Ci, relu=False, scale=1.0):
        g = (N, H, W, Ci, 64, 7, 2, 3)
        for prec in (0, 4):
            self.add(*g, inn=int(Ci != 1), prec=prec)

    def bnstats(self, N, H, W, Ci, Co, k, groups):
        g = (N, H, W, Ci, Co, k, 1, k // 2)
        self.add(*g, route=self.HALO_SMALL, bng=groups)
        self.add(*g, route=self.HALO_SMALL)

    def convT_bnstats(self, N, H, Ci, Co, groups):
        self.add(N, H, H, Ci, Co, 2, 2, 0, T=1, bng=groups)
        self.add(N, H, H, Ci, Co, 2, 2, 0, T=1)

    def bnreduce(self, N, H, W, C, Co, groups, relu, res, acc):
        """check_dgrad_epilogue_accumulates_batchnorm_backward_sums: held against the three-launch BatchNorm adjoint (itself float64-checked)"""
        g = (N, H, W, C, Co, 3, 1, 1)
        self.add(*g, route=self.HALO_SMALL, which="dgrad", acc=int(acc))
        self.add(*g, route=self.HALO_SMALL, which="dgrad_bnr_y" if (relu and res) else "dgrad_bnr_z", acc=int(acc), bng=groups)

    def packed(self, N, H, Ci, Co, prec):
        """test_conv3x3_packed_weights_match_lds_slab_path"""
        g = (N, H, H, Ci, Co, 3, 1, 1)
        for lay in (0, 1):
            for bng in (0, 1):
                self.add(*g, prec=prec, lay=lay, route=self.HALO_SMALL, bng=bng)
            for acc in (0, 1):
                self.add(*g, prec=prec, lay=lay, route=self.HALO_SMALL, which="dgrad", acc=acc)

    def _split(self, g, prec, route):
        lay = PACKED_LAYOUT[prec]
        for bng in (0, 1):
            self.add(*g, prec=prec, lay=lay, route=route, bng=bng)
        for acc in (0, 1):
            self.add(*g, prec=prec, lay=lay, route=route, which="dgrad", acc=acc)

    def f32x3(self, N, H, W, Ci, Co, wide=False):
        """check_conv3x3_f32x3_is_fp32_accurate"""
        for prec in (0, 2):
            self._split((N, H, W, Ci, Co, 3, 1, 1), prec, self.HALO_SMALL)

    def f32x2(self, N, H, W, Ci, Co):
        """check_conv3x3_f32x2_two_piece_mode"""
        g = (N, H, W, Ci, Co, 3, 1, 1)
        for prec in (3, 2):
            self._split(g, prec, self.HALO_SMALL)
            self.wgrad(g, prec, self.HALO_SMALL, ws=True)
        self.add(*g, prec=1, route=self.HALO_SMALL)
        self.add(*g, prec=1, route=self.HALO_SMALL, which="dgrad")
        self.wgrad(g, 1, self.HALO_SMALL)

    def f16x2(self, N, H, W, Ci, Co, wide=False, route=0, kernel4=None):
        """check_conv3x3_f16x2_forward_and_dgrad"""
        for prec in (0, 2, 3, 4):
            self._split((N, H, W, Ci, Co, 3, 1, 1), prec, self.HALO_SMALL | route)

    def map4(self, N, Ci, Co, prec, groups):
        """test_conv3x3_halo_kernel_on_4x4_maps"""
        g = (N, 4, 4, Ci, Co, 3, 1, 1)
        lay = PACKED_LAYOUT[prec]
        self.add(*g, prec=prec, lay=lay, route=self.HALO_SMALL)
        self.add(*g, prec=prec, lay=lay, route=self.HALO_SMALL, bng=groups)
        for acc in (0, 1):
            self.add(*g, prec=prec, lay=lay, route=self.HALO_SMALL, which="dgrad", acc=acc)
        self.add(*g, route=self.GENERIC)
        self.add(*g, route=self.GENERIC, which="dgrad")

    def wgrad_x3(self, N, H, W, Ci, Co):
        """check_wgrad_f32x3_kernel"""
        g = (N, H, W, Ci, Co, 3, 1, 1)
        for prec in (0, 2):
            self.wgrad(g, prec)
        self.wgrad(g, 2, ws=True)

    def wgrad_f16(self, N, H, W, Ci, Co):
        """check_wgrad_f16x2_kernel / test_wgrad_f16x2_on_4x4_maps"""
        g = (N, H, W, Ci, Co, 3, 1, 1)
        for prec in (0, 2, 3, 4):
            self.wgrad(g, prec, ws=True)
        if Ci % 64 == 0 and Co % 64 == 0:
            self.wgrad(g, 4, self.WX3_PC, ws=True)
        self.wgrad(g, 4)

    def wgrad_s1(self, N, H, Ci, Co, k):
        """test_wgrad_stride1_fast_path_matches_generic_kernel"""
        for route in (self.WG_GENERIC, 0, self.WG_3TAP):
            self.wgrad((N, H, H, Ci, Co, k, 1, k // 2), 0, route)

    def wgrad_det(self, N, H, W, Ci, Co):
        """check_wgrad_deterministic_mode_is_bitwise_repeatable"""
        g = (N, H, W, Ci, Co, 3, 1, 1)
        self.wgrad(g, 0, ws=True)
        self.wgrad(g, 0)

    def gemm_x3(self, N, H, Ci, Co, k, s, p, T, scale, prec):
        """test_generic_kernel_in_three_bf16_pieces"""
        g = (N, H, H, Ci, Co, k, s, p)
        for pr in (0, prec):
            self.add(*g, T=int(T), prec=pr, route=self.GEMM_X3)
            if self.dgrad_is_plain(*g, T=int(T)):
                self.add(*g, T=int(T), prec=pr, route=self.GEMM_X3, which="dgrad")

    def pc(self, N, H, W, Ci, Co):
        """test_conv_pc_gpu.py: the persistent kernel bit for bit against the halo kernel (which the f16x2 helper holds against float64) -
        forward, forward + statistics in 1 and 2 groups, dgrad, accumulating dgrad, dgrad + column sums, dgrad + BatchNorm sums"""
        g = (N, H, W, Ci, Co, 3, 1, 1)
        for route in (self.HALO_SMALL | self.C3_PC, self.HALO_SMALL | self.TILE_WG):
            for bng in (0, 1, 2):
                if bng == 2 and N % 2:
                    continue
                self.add(*g, prec=4, lay=4, route=route, bng=bng)
            for acc in (0, 1):
                self.add(*g, prec=4, lay=4, route=route, which="dgrad", acc=acc)
            self.add(*g, prec=4, lay=4, route=route, which="dgrad_colsum")
            if N % 2 == 0 and 256 % (Ci // 4) == 0:
                for which, acc in (("dgrad_bnr_z", 0), ("dgrad_bnr_y", 1), ("dgrad_bnr_z", 1)):
                    self.add(*g, prec=4, lay=4, route=route, which=which, acc=acc, bng=2)

    def pc_reduce(self, N, H, W, Ci, Co, relu, with_y, acc):
        """test_conv_pc_gpu.test_dgrad_batchnorm_reduce_bit_identical: two statistics groups"""
        for route in (self.HALO_SMALL | self.C3_PC, self.HALO_SMALL | self.TILE_WG):
            self.add(N, H, W, Ci, Co, 3, 1, 1, prec=4, lay=4, route=route, which="dgrad_bnr_y" if (relu and with_y) else "dgrad_bnr_z", acc=int(acc), bng=2)

    def pointwise(self, kind, N, H, W, Ci, Co, groups):
        """test_pointwise_forward_against_float64"""
        g = (N, H, W, Ci, Co, 2, 2, 0) if kind == "convT" else (N, H, W, Ci, Co, 1, 1, 0)
        self.add(*g, T=int(kind == "convT"), prec=4)
        self.add(*g, T=int(kind == "convT"), prec=4, bng=groups)


CONV_HELPERS = {
    # helper -> (test module, function the GPU module calls with (K, *arguments))
    "conv2d": (CK, "check_conv2d_fwd_dgrad_wgrad"), "convT": (CK, "check_conv_transpose_2x2"), "first_conv": (CK, "check_first_conv_nchw_input"),
    "last_conv": (CK, "check_last_conv_nchw_output"), "gray_stem": (CK, "check_gray_stem_conv_and_its_dgrad"), "bf16": (CK, "test_bf16_operand_mode"),
    "stem7": (CK, "check_stem7_forward_kernel"), "stem7_f16": (CK, "check_stem7_forward_in_fp16_pieces"),
    "f32x3": (CK, "check_conv3x3_f32x3_is_fp32_accurate"), "f32x2": (CK, "check_conv3x3_f32x2_two_piece_mode"), "f16x2": (F16, "check_conv3x3_f16x2_forward_and_dgrad"),
    "wgrad_x3": (CK, "check_wgrad_f32x3_kernel"), "wgrad_f16": (F16, "check_wgrad_f16x2_kernel"), "packed": (CK, "test_conv3x3_packed_weights_match_lds_slab_path"),
    "bnstats": (CK, "check_conv_fwd_with_batchnorm_sums"), "bnreduce": (CK, "check_dgrad_epilogue_accumulates_batchnorm_backward_sums"),
    "map4": (CK, "test_conv3x3_halo_kernel_on_4x4_maps"), "gemm_x3": (CK, "test_generic_kernel_in_three_bf16_pieces"),
    "wgrad_s1": (CK, "test_wgrad_stride1_fast_path_matches_generic_kernel"), "pointwise": (PW, "test_pointwise_forward_against_float64"),
    "pc_reduce": (PC, "test_dgrad_batchnorm_reduce_bit_identical"),
}

# census-driven cases (the kernels of the census no case of the older tables reaches), run by test_shape_edges_gpu.py through the helper named:
# (id, helper, arguments of Launches.<helper> = of the helper after K)
CENSUS_CASES = [
    # halo-tiled 3x3, 32-channel tile with bf16 operands, LDS-slab and packed; 64-channel tile, one sub-tile, bf16
    ("halo-bf16-32", "packed", (2, 8, 32, 32, 1)), ("halo-bf16-64-one-subtile", "packed", (1, 8, 64, 64, 1)), ("halo-bf16-64", "packed", (16, 16, 64, 64, 1)),
    ("halo-fp32-32-packed", "packed", (2, 8, 32, 32, 0)), ("halo-fp32-64-one-subtile-packed", "packed", (1, 8, 64, 64, 0)),
    # split operands at the smallest grids: one 8 x 8 tile, N = 1
    ("halo-f16x2-32-one-tile", "f16x2", (1, 8, 8, 32, 32, False)), ("halo-f16x2-64-one-tile", "f16x2", (1, 8, 8, 64, 64, False, 256, "conv3x3_halo_kernel")),
    ("pc-f16x2-one-tile", "f16x2", (1, 8, 8, 64, 64, False)),
    # weight gradients: the small-channel kernels at N = 1 on the smallest maps, 1x1 and taps
    ("wgrad-x3-one-tile-32", "wgrad_f16", (1, 8, 8, 32, 32)), ("wgrad-x3-one-tile-64", "wgrad_f16", (1, 8, 8, 64, 64)),
    ("wgrad-s1-one-tile", "wgrad_s1", (1, 8, 64, 64, 3)), ("wgrad-s1-1x1", "wgrad_s1", (1, 8, 64, 64, 1)),
    ("wgrad-bf16-s1", "bf16", (1, 8, 64, 64, 3, 1, 1)), ("wgrad-bf16-1x1", "bf16", (1, 8, 64, 64, 1, 1, 0)), ("wgrad-bf16-generic", "bf16", (1, 1, 64, 64, 1, 1, 0)),
    # the streaming 1x1 / 2x2 kernel: one output channel, the narrow transposed forms
    ("pw-32-1", "pointwise", ("1x1", 128, 32, 32, 32, 1, 2)), ("pw-64-1", "pointwise", ("1x1", 128, 32, 32, 64, 1, 2)),
    ("pw-32-12-T", "pointwise", ("convT", 128, 32, 32, 32, 12, 2)), ("pw-32-24-T", "pointwise", ("convT", 128, 32, 32, 32, 24, 2)),
    ("pw-64-12-T", "pointwise", ("convT", 128, 32, 32, 64, 12, 2)),
    # the generic kernel in three bf16 pieces (BH_ROUTE_GEMM_X3) at its three tiles
    ("gemm-x3-32-32", "gemm_x3", (1, 4, 32, 32, 1, 1, 0, False, 1.0, 2)), ("gemm-x3-32-32-s2", "gemm_x3", (2, 17, 32, 32, 3, 2, 1, False, 1.0, 4)),
    ("gemm-x3-64-64-s2", "gemm_x3", (1, 5, 64, 64, 3, 2, 1, False, 1.0, 2)), ("gemm-x3-T-32-32", "gemm_x3", (1, 2, 32, 32, 2, 2, 0, True, 1.0, 2)),
    ("gemm-x3-32-256", "gemm_x3", (1, 128, 32, 256, 1, 1, 0, False, 1.0, 2)),            # Nn >= 256 and 512 tiles: the 64 x 128 tile
    ("gemm-fp32-32-256", "conv2d", (1, 128, 128, 32, 256, 1, 1, 0)),                      # the same tile of the fp32 arm
    ("gemm-fp32-24-256", "conv2d", (1, 128, 128, 24, 256, 1, 1, 0)),                      # ... without buffer loads (Kc % 32 != 0)
    ("gemm-x3-256-32-s2-odd", "gemm_x3", (1, 129, 256, 32, 1, 2, 0, False, 1.0, 2)),      # ... of the three-piece form, the stride-2 adjoint gather
    # bf16 operands: 128-row tiles from 1024 tiles on (conv_gemm.hip:891), with buffer loads and (Co % 4 != 0) without
    ("bf16-32-128-1024-tiles", "bf16", (1, 256, 32, 128, 1, 1, 0)), ("bf16-32-126-1024-tiles", "bf16", (1, 256, 32, 126, 1, 1, 0)),
    # bf16 operands, packed fragments, two sub-tiles per workgroup (more than 256 sub-tile pairs)
    ("halo-bf16-64-two-subtiles", "packed", (33, 32, 64, 64, 1)),
    # the 4 x 4 map form in fp16 pieces, forward and dgrad
    ("map4-f16x2", "map4", (4, 64, 64, 4, 1)), ("map4-f16x2-128", "map4", (8, 128, 64, 4, 2)),
    # persistent 3x3 dgrad with the BatchNorm sums and the saved output, not accumulating (epilogue mode 13)
    ("pc-dgrad-bnreduce-y", "pc_reduce", (8, 16, 16, 64, 64, True, True, False)), ("pc-dgrad-bnreduce-y-odd-pairs", "pc_reduce", (2, 8, 8, 64, 64, True, True, False)),
]

# kernels of the census that no float64-checked case runs (at most five, each with the reason the code gives)
CENSUS_EXEMPT = {}


def covered_kernel_names():
    """Every kernel name a float64-checked GPU case of the suite resolves to: the older modules' tables and parametrisations through
    Launches, the rectangular module's tables, and the conv tables of this module."""
    L = Launches()
    C = importlib.import_module(CK)
    R = importlib.import_module("test_rectangular_gpu")
    for c in C.CONV_CASES:
        L.conv2d(c[0], c[1], c[1], *c[2:])
    for c in R.both(C.RECT_CONV_CASES):
        L.conv2d(*c, route=L.GENERIC)
        L.conv2d(*c, route=L.GENERIC | L.WG_GENERIC)
    for c in R.HALO_SHAPES:
        L.conv2d(*c, 3, 1, 1, route=L.HALO_SMALL)
        L.f32x3(*c)
        L.f32x2(*c)
        L.f16x2(*c, route=L.TILE_WG)
    for c in R.WX3_SHAPES:
        L.wgrad_x3(*c)
        L.wgrad_f16(*c)
    for c in R.both([(4, 16, 32, 64, 64), (2, 24, 40, 64, 128)]):
        L.f16x2(*c)
    for p in _parametrized(CK, "test_conv_transpose_2x2"):
        L.convT(p["N"], p["Hi"], p["Hi"], p["Ci"], p["Co"])
    for p in _parametrized(CK, "test_first_conv_nchw_input"):
        L.first_conv(p["N"], p["Hi"], p["Hi"], p["Ci"], p["Co"])
    for p in _parametrized(CK, "test_gray_stem_conv_and_its_dgrad"):
        L.gray_stem(p["N"], p["Hi"], p["Hi"])
    L.last_conv(2, 16, 16)
    for p in _parametrized(CK, "test_bf16_operand_mode"):
        L.bf16(p["N"], p["Hi"], p["Ci"], p["Co"], p["k"], p["s"], p["p"])
    for p in _parametrized(CK, "test_generic_kernel_in_three_bf16_pieces"):
        L.gemm_x3(p["N"], p["Hi"], p["Ci"], p["Co"], p["k"], p["s"], p["p"], p["T"], 1.0, p["prec"])
    for p in _parametrized(CK, "test_conv_fwd_with_batchnorm_sums"):
        L.bnstats(p["N"], p["H"], p["H"], p["Ci"], p["Co"], p["k"], p["groups"])
    for p in _parametrized(CK, "test_conv_transpose_fwd_with_batchnorm_sums"):
        L.convT_bnstats(p["N"], p["H"], p["Ci"], p["Co"], p["groups"])
    for p in _parametrized(CK, "test_dgrad_epilogue_accumulates_batchnorm_backward_sums"):
        L.bnreduce(p["N"], p["H"], p["H"], p["C"], p["Co"], p["groups"], p["relu"], p["res"], p["acc"])
    for p in _parametrized(CK, "test_wgrad_stride1_fast_path_matches_generic_kernel"):
        L.wgrad_s1(p["N"], p["H"], p["Ci"], p["Co"], p["k"])
    for p in _parametrized(CK, "test_stem7_forward_kernel"):
        L.stem7(p["N"], p["H"], p["H"], p["Ci"])
    for p in _parametrized(CK, "test_stem7_forward_in_fp16_pieces"):
        L.stem7_f16(p["N"], p["H"], p["H"], p["Ci"])
    for p in _parametrized(CK, "test_conv3x3_packed_weights_match_lds_slab_path"):
        L.packed(p["N"], p["H"], p["Ci"], p["Co"], p["prec"])
    for p in _parametrized(CK, "test_conv3x3_f32x3_is_fp32_accurate"):
        L.f32x3(p["N"], p["H"], p["H"], p["Ci"], p["Co"])
    for p in _parametrized(CK, "test_conv3x3_f32x2_two_piece_mode"):
        L.f32x2(p["N"], p["H"], p["H"], p["Ci"], p["Co"])
    for p in _parametrized(CK, "test_conv3x3_halo_kernel_on_4x4_maps"):
        L.map4(p["N"], p["Ci"], p["Co"], p["prec"], p["groups"])
    for p in _parametrized(CK, "test_wgrad_f32x3_kernel"):
        L.wgrad_x3(p["N"], p["H"], p["H"], p["Ci"], p["Co"])
    for p in _parametrized(CK, "test_wgrad_deterministic_mode_is_bitwise_repeatable"):
        L.wgrad_det(p["N"], p["H"], p["H"], p["Ci"], p["Co"])
    L.conv2d(65, 32, 32, 64, 64, 3, 1, 1)                          # (test_conv3x3_two_tile_positions_per_workgroup)
    for p in _parametrized(F16, "test_conv3x3_f16x2_forward_and_dgrad"):
        L.f16x2(p["N"], p["H"], p["H"], p["Ci"], p["Co"])
    for p in _parametrized(F16, "test_wgrad_f16x2_kernel"):
        L.wgrad_f16(p["N"], p["H"], p["H"], p["Ci"], p["Co"])
    for p in _parametrized(F16, "test_wgrad_f16x2_on_4x4_maps"):
        L.wgrad_f16(p["N"], 4, 4, p["Ci"], p["Co"])
    for c in importlib.import_module(PC).SHAPES:
        L.pc(*c)
    for c in importlib.import_module(PW).CASES:
        for groups in (1, 2):
            L.pointwise(*c, groups)
    # this module's tables
    for _, _, helper, args, _ in CONV_EDGE_CASES:
        getattr(L, helper)(*args)
    for _, N, H, W, Ci, Co, _ in HALO_GRID_CASES:
        L.conv2d(N, H, W, Ci, Co, 3, 1, 1)
    for _, helper, args, _, _, _ in STEM_CASES:
        getattr(L, helper)(*args)
    for _, helper, args in CENSUS_CASES:
        getattr(L, helper)(*args)
    return L.names
