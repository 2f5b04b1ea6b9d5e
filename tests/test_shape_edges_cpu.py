"""The support boundary, checked without a GPU (tests/shape_edges.py holds the tables, tests/test_shape_edges_gpu.py runs them):

  - the dispatch census: every kernel name bh_conv_variant returns over a grid of descriptors is run by a float64-checked GPU case of the
    suite's conv tables (or is one of at most five exempted names);
  - the ABI mirror: every prototype of include/bihome.h against the ctypes signature bihome_amd/_lib.py sets, argument by argument, and
    the Python copies of the header's constants;
  - table integrity: every accepted-edge case satisfies the accept-condition cited for it, every refusal case violates it, and every
    citation points at a line of csrc/ that holds the condition."""
import ctypes
import os
import re

import pytest

import shape_edges as S
from test_cabi_cpu import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_header, _c_class = S.header_text, lambda decl: S.c_class(decl)[0]


def header_prototypes():
    """name -> (return class, [argument classes])"""
    return {n: (ret, [c for c, _ in args]) for n, (ret, args) in S.header_prototypes().items()}


def _ctypes_class(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    if t is ctypes.c_size_t:                              # (before the width test: c_size_t is an unsigned 64-bit integer)
        return "size"
    if t is ctypes.c_int:
        return "int"
    if t in (ctypes.c_int64, ctypes.c_longlong):
        return "i64"
    if t is ctypes.c_float:
        return "float"
    if t is ctypes.c_double:
        return "double"
    raise AssertionError("ctypes type %r has no C type class here" % (t,))


def test_c_type_classes_of_the_parser():
    assert _c_class("const float* x") == "ptr" and _c_class("void* stream") == "ptr" and _c_class("const bh_conv_desc* d") == "ptr"
    assert _c_class("int B") == "int" and _c_class("long long L") == "i64" and _c_class("int64_t n") == "i64"
    assert _c_class("size_t ws_bytes") == "size" and _c_class("float eps") == "float" and _c_class("double sigma") == "double"
    assert _c_class("long long") == "i64" and _c_class("size_t") == "size"
    with pytest.raises(AssertionError):
        _c_class("short n")
    assert ctypes.sizeof(ctypes.c_int) == 4 and ctypes.sizeof(ctypes.c_int64) == 8 and ctypes.sizeof(ctypes.c_size_t) == 8


def test_every_prototype_agrees_with_its_ctypes_signature():
    """A c_int where the header says long long (or a c_float where it says double) passes garbage in that argument and shifts nothing else:
    no GPU test is bound to notice.  Every declared function - the status-returning ones of _lib.SIGNATURES and the size queries whose
    argtypes / restype _lib._load() sets by hand - is held against its prototype in arity, per argument and in its return type."""
    from bihome_amd import _lib
    protos = header_prototypes()
    assert set(header_symbols()) <= set(protos), set(header_symbols()) - set(protos)
    assert set(_lib.SIGNATURES) <= set(protos)
    sizes = sorted(set(protos) - set(header_symbols()))                    # the functions that do not return a status
    assert sizes == ["bh_conv_wgrad_det_bytes", "bh_stem7_wgrad_ws_bytes", "bh_synth_blobs_scratch_floats", "bh_warp_bwd_img_scratch_doubles"], sizes
    bad = []
    for name, (ret, args) in sorted(protos.items()):
        fn = getattr(_lib.lib, name)
        assert fn.argtypes is not None, "%s: no argtypes set" % name
        if name in _lib.SIGNATURES:
            assert list(fn.argtypes) == list(_lib.SIGNATURES[name]), name
        mirror = [_ctypes_class(t) for t in fn.argtypes]
        if len(mirror) != len(args):
            bad.append("%s: %d arguments in the header, %d in ctypes" % (name, len(args), len(mirror)))
            continue
        for i, (h, c) in enumerate(zip(args, mirror)):
            if h != c:
                bad.append("%s: argument %d is %s in the header, %s in ctypes" % (name, i, h, c))
        if _ctypes_class(fn.restype) != ret:
            bad.append("%s: returns %s in the header, %s in ctypes" % (name, ret, _ctypes_class(fn.restype)))
    assert not bad, "\n".join(bad)
    assert len(protos) == len(header_symbols()) + 4 and len(protos) >= 90


# ------------------------------------------------------------------------------------------------
# 2. constants
# ------------------------------------------------------------------------------------------------
def _defines(text):
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(BH_\w+)\s+\(?(-?\d+)\)?\s*(?://.*)?$", text, flags=re.M)}
    for body in re.findall(r"enum\s*\{([^}]*)\}", text):
        for m in re.finditer(r"(BH_\w+)\s*=\s*(-?\d+)", body):
            out[m.group(1)] = int(m.group(2))
    return out


def test_python_constants_equal_the_header_defines():
    from bihome_amd import _lib, kernels
    H = _defines(_header())
    common = re.sub(r"//.*", "", open(os.path.join(ROOT, "bihome_amd", "csrc", "common.h")).read())
    Cm = _defines(common)
    assert H["BH_OK"] == 0 and H["BH_E_BADARG"] == -1 and H["BH_E_UNSUPPORTED"] == -2
    # the names _lib.check() puts into BihomeLibError
    for code in ("BH_E_BADARG", "BH_E_UNSUPPORTED"):
        with pytest.raises(_lib.BihomeLibError, match=code + "$"):
            _lib.check(H[code], "x")
    _lib.check(H["BH_OK"], "x")
    # every ROUTE_* copy of _lib.py by name, and every BH_ROUTE_* the wrappers use
    routes = {n: getattr(_lib, n) for n in dir(_lib) if n.startswith("ROUTE_")}
    assert len(routes) >= 11
    for n, v in routes.items():
        assert H["BH_" + n] == v, n
    for n in ("ROUTE_DETERMINISTIC", "ROUTE_WX3_PC", "ROUTE_WX3_SHARED"):
        assert getattr(kernels, n) == H["BH_" + n]
    assert _lib.BN_DETERMINISTIC == kernels.BN_DETERMINISTIC == H["BH_BN_DETERMINISTIC"]
    assert _lib.F_DETERMINISTIC == kernels.F_DETERMINISTIC == H["BH_F_DETERMINISTIC"]
    assert _lib.AMAX_FLOATS == kernels.AMAX_FLOATS == H["BH_AMAX_FLOATS"] == Cm["BH_AMAX_SLOTS"] * Cm["BH_AMAX_STRIDE"]
    assert _lib.DSAC_METHODS == kernels.DSAC_METHODS == {"repr_error": H["BH_DSAC_REPR_ERROR"], "inliers_ratio": H["BH_DSAC_INLIERS"],
                                                        "soft_inliers_ratio": H["BH_DSAC_SOFT_INLIERS"]}
    assert kernels.TAIL_ROUTE_VALU_FWD == H["BH_TAIL_ROUTE_VALU_FWD"] and kernels.TAIL_ROUTE_LDS_MOMENTS == H["BH_TAIL_ROUTE_LDS_MOMENTS"]
    assert kernels.BN_SUM_STRIDE == Cm["BH_BN_SUM_STRIDE"] and kernels.BN_SUM_SLOTS == Cm["BH_BN_SUM_SLOTS"]
    # ... and the size the library derives from them (no GPU needed)
    for groups, C in ((1, 4), (2, 64), (3, 1024)):
        assert _lib.lib.bh_bn_stats_doubles(groups, C) == kernels.BN_SUM_SLOTS * groups * C * 2 * kernels.BN_SUM_STRIDE
    # SPLIT_PIECES: the header states the pieces per operand in the descriptions of bh_conv_desc.precision ("three bf16 pieces" for 2, "two
    # bf16 pieces" for 3, "two FP16 pieces" for 4); the library's own statement is the weight-gradient kernel it names: wgrad_x3_kernel<CB,BNI,NP,..>
    assert kernels.SPLIT_PIECES == {2: 3, 3: 2, 4: 2} and kernels.SPLIT_LAYOUT == {2: 2, 3: 3, 4: 4} and kernels.F16X2 == 4
    for prec, pieces in kernels.SPLIT_PIECES.items():
        v = kernels.conv_variant(kernels.conv_desc(8, 16, 16, 64, 64, 3, 1, 1, precision=prec), "wgrad")
        assert v.startswith("wgrad_x3_kernel<64,false,%d," % pieces), (prec, v)
    words = {2: r"three bf16 pieces", 3: r"two bf16 pieces", 4: r"two FP16 pieces"}
    raw = " ".join(open(os.path.join(ROOT, "include", "bihome.h")).read().split())
    for prec, phrase in words.items():
        assert re.search(r"\b%d \(\"f\d+x%d\"[^;]*?%s" % (prec, kernels.SPLIT_PIECES[prec], phrase), raw.replace("* ", "")), prec


# ------------------------------------------------------------------------------------------------
# 3. the dispatch census
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def census():
    return S.dispatch_census()


def test_census_sweeps_what_it_claims(census):
    names, calls = census
    assert calls > 200000 and len(names) >= 40
    fam = {n.split("<")[0] for n in names}
    assert {"conv_gemm_kernel", "conv3x3_halo_kernel", "conv3x3_pc_kernel", "wgrad_kernel", "wgrad_s1_kernel", "wgrad_small_kernel",
            "wgrad_small_taps_kernel", "wgrad_x3_kernel", "stem7_fwd_kernel"} <= fam, fam
    # the arms of conv_gemm.hip dispatch() beyond the vector path: scalar at three tile widths, vector with Kc % 32 != 0, buffer loads off
    for n in ("conv_gemm_kernel<128,128,32,false,false,false>", "conv_gemm_kernel<128,64,32,false,false,false>",
              "conv_gemm_kernel<128,32,32,false,false,false>", "conv_gemm_kernel<128,32,16,true,false,false>",
              "conv_gemm_kernel<64,64,32,true,false,false>"):
        assert n in names, n


def test_every_kernel_of_the_census_has_a_float64_checked_case(census):
    names, _ = census
    covered = S.covered_kernel_names()
    assert len(S.CENSUS_EXEMPT) <= 5
    for n, why in S.CENSUS_EXEMPT.items():
        assert n in names and n not in covered and len(why) > 20, n          # an exemption that is needed, with its reason
    missing = sorted(set(names) - set(covered) - set(S.CENSUS_EXEMPT))
    assert not missing, "%d kernels no float64-checked case runs:\n  %s" % (
        len(missing), "\n  ".join("%s   e.g. %s" % (n, S.describe(names[n])) for n in missing))


# ------------------------------------------------------------------------------------------------
# 4. table integrity
# ------------------------------------------------------------------------------------------------
def test_citations_point_at_the_condition():
    """Every table cites `file:line` with a fragment of the condition: that line holds it."""
    src, bad = {}, set()
    n = 0
    for table in S.ALL_TABLES:
        for case in table:
            f, line, frag = case.cite
            if f not in src:
                src[f] = open(os.path.join(ROOT, "bihome_amd", "csrc", f)).read().split("\n")
            if frag not in src[f][line - 1]:                      # the cited line itself: drift shows
                bad.add("%s:%d does not hold %r" % (f, line, frag))
            n += 1
    assert not bad, "\n".join(sorted(bad))
    assert n >= 60


def test_accepted_cases_satisfy_and_refusals_violate_their_condition():
    n_ok = n_bad = 0
    for table in S.ALL_TABLES:
        for case in table:
            ok = bool(case.accept(**case.args))
            assert ok == case.accepted, "%s %s: the accept-condition gives %s" % (case.family, case.args, ok)
            n_ok += case.accepted
            n_bad += not case.accepted
    assert n_ok >= 40 and n_bad >= 20


def test_listed_edges_are_in_the_tables():
    """The boundaries the tables exist for, by value (a case that drifts into the middle of a range fails here)."""
    val = lambda fam, key: {c.args[key] for t in S.ALL_TABLES for c in t if c.family == fam and c.accepted and key in c.args}
    rej = lambda fam, key: {c.args[key] for t in S.ALL_TABLES for c in t if c.family == fam and not c.accepted and key in c.args}
    assert {4, 8, 256, 260, 320} <= val("loss", "C") and {1} <= val("loss", "hw") and {6, 12, 24} <= rej("loss", "C")
    assert {4, 1024} <= val("bn", "C") and {1, 2} <= val("bn", "rows") and {12, 2048} <= rej("bn", "C")
    assert {4, 5, 63, 64, 65, 511, 512} <= val("dlt", "P") and {3, 513} <= rej("dlt", "P")
    assert {1, 2, 3, 4, 5} <= val("add", "n")
    assert {1, 2, 4, 8, 16, 32} <= val("warp", "pool") and {3} <= rej("warp", "pool") and {24} <= rej("warp", "h")
    assert {24} <= rej("photo_warp", "P") and {24} <= rej("synth", "P") and {24} <= rej("blobs", "P")
    assert {16, 128, 144, 256} <= val("blobs", "P")
    assert {4} <= val("relu_bwd", "n") and {6} <= rej("relu_bwd", "n")
    assert {4} <= val("scale_samples", "L") and {6} <= rej("scale_samples", "L")
    assert {8} <= rej("bn_from_1x1", "KC")
    assert {1, 63, 64, 65} <= val("ransac", "K")


# ------------------------------------------------------------------------------------------------
# 5. the conv tables: every case still takes the arm it was written for
# ------------------------------------------------------------------------------------------------
def _desc_of(K, helper, args):
    if helper == "conv2d":
        return K.conv_desc(*args)
    if helper == "convT":
        return K.conv_desc(*args, 2, 2, 0, transposed=True)
    if helper == "first_conv":
        return K.conv_desc(*args, 7, 2, 3, in_nchw=True)
    if helper == "last_conv":
        return K.conv_desc(*args, 1, 1, 0, out_nchw=True)
    if helper == "gray_stem":
        return K.conv_desc(args[0], args[1], args[2], 1, 64, 7, 2, 3)
    if helper == "bf16":
        return K.conv_desc(args[0], args[1], args[1], *args[2:], precision=1)
    if helper in ("stem7", "stem7_f16"):
        return K.conv_desc(args[0], args[1], args[2], args[3], 64, 7, 2, 3, in_nchw=args[3] != 1)
    raise AssertionError(helper)


def test_conv_edge_cases_take_the_arm_they_cite():
    from bihome_amd import kernels as K
    src = {}
    for id, cite, helper, args, want in S.CONV_EDGE_CASES:
        f, line, frag = cite
        src.setdefault(f, open(os.path.join(ROOT, "bihome_amd", "csrc", f)).read().split("\n"))
        assert frag in src[f][line - 1], "%s: %s:%d does not hold %r" % (id, f, line, frag)
        d = _desc_of(K, helper, args)
        assert want, id
        for which, prefix in want.items():
            assert K.conv_variant(d, which).startswith(prefix), (id, which, K.conv_variant(d, which))
        assert S.conv_desc_ok(d.Hi, d.Wi, d.kh, d.stride, d.pad, bool(d.transposed)), id
    # the three widths of the scalar arm, the BK = 16 tiles, buffer loads off with a vector Ci: all pinned by some case
    pinned = {p for c in S.CONV_EDGE_CASES for p in c[4].values()}
    for p in ("conv_gemm_kernel<128,128,32,false", "conv_gemm_kernel<128,64,32,false", "conv_gemm_kernel<128,32,32,false",
              "conv_gemm_kernel<128,32,16,true,false,false>", "conv_gemm_kernel<128,64,16,true,false,false>",
              "conv_gemm_kernel<128,128,16,true,false,false>", "conv_gemm_kernel<128,32,32,true,false,false>"):
        assert p in pinned, p
    assert all(c[3][0] == 1 for c in S.CONV_EDGE_CASES if c[2] != "conv2d" or c[0] != "s2-odd-64-128")          # N = 1 throughout


def test_thresholds_are_pinned_on_both_sides():
    """The smallest grid each dedicated kernel takes, and one tile below it: the accept-condition restated in shape_edges.py and the
    library's own routing agree on both."""
    from bihome_amd import kernels as K
    from bihome_amd._lib import BihomeLibError, lib
    assert S.C3_MIN_BLOCKS == 256
    for id, N, H, W, Ci, Co, taken in S.HALO_GRID_CASES:
        d = K.conv_desc(N, H, W, Ci, Co, 3, 1, 1)
        assert S.halo_grid_ok(N, H, W, Ci, Co) == taken, id
        assert K.conv_variant(d, "fwd").startswith("conv3x3_halo_kernel<false," if taken else "conv_gemm_kernel<"), (id, K.conv_variant(d, "fwd"))
        if Ci == Co:
            assert K.conv_variant(d, "dgrad").startswith("conv3x3_halo_kernel<true," if taken else "conv_gemm_kernel<"), id
        # the packed fp16-piece launch of the same grid: the persistent kernel at the threshold, refused below it (its weights are no
        # operand of the generic kernel)
        if Co % 64 == 0:
            d4 = K._with_layout(K.conv_desc(N, H, W, Ci, Co, 3, 1, 1, precision=4), 4)
            if taken:
                assert K.conv_variant(d4, "fwd") == "conv3x3_pc_kernel<false,false,0>", id
            else:
                with pytest.raises(BihomeLibError, match="BH_E_UNSUPPORTED"):
                    K.conv_variant(d4, "fwd")
    for id, helper, args, accept, a, taken in S.STEM_CASES:
        assert bool(accept(**a)) == taken, id
        d = K.conv_desc(a["N"], a["Hi"], a["Wi"], a.get("Ci", 2), 64, 7, 2, 3, in_nchw=a.get("Ci", 2) != 1)
        if accept is S.stem7_fwd_ok:
            v = K.conv_variant(d, "fwd")
            assert v.startswith("stem7_fwd_kernel<%d>" % a["Ci"] if taken else "conv_gemm_kernel<"), (id, v)
            if helper == "stem7_f16":
                assert K.conv_variant(K.conv_desc(a["N"], a["Hi"], a["Wi"], a["Ci"], 64, 7, 2, 3, in_nchw=a["Ci"] != 1, precision=4), "fwd") == "stem7_fwd_f16_kernel<%d>" % a["Ci"]
        else:
            assert (lib.bh_stem7_wgrad_ws_bytes(ctypes.byref(d)) > 0) == taken, id
    # conv3x3_pc.hip:709-710: an odd number of sub-tiles per statistics group sends the launch WITH statistics to the halo kernel
    for N, groups, pc in ((1, 1, False), (2, 1, True), (2, 2, False), (4, 2, True)):
        assert S.pc_pairs_ok(N, 8, 8, groups) == pc
        d4 = K._with_layout(K.conv_desc(N, 8, 8, 64, 64, 3, 1, 1, precision=4, route=2), 4)
        assert K.conv_variant(d4, "fwd") == "conv3x3_pc_kernel<false,false,0>"
        assert K.conv_variant(d4, "fwd", bn_groups=groups).startswith("conv3x3_pc_kernel<false,false,1>" if pc else "conv3x3_halo_kernel<false,64,"), (N, groups)


# ------------------------------------------------------------------------------------------------
# 6. the raw-call tables: complete, and refused before any launch
# ------------------------------------------------------------------------------------------------
def test_raw_cases_name_every_scalar_argument():
    protos = S.header_prototypes()
    entries = {c.run[0] for c in S.REFUSALS + S.EMPTY_CASES} | {c[0] for c in S.NULL_CASES}
    assert len(entries) >= 55
    for e in sorted(entries):
        scalars = {n for c, n in protos[e][1] if c != "ptr"}
        assert scalars == set(S.BASE[e]) & scalars and scalars <= set(S.BASE[e]), (e, scalars - set(S.BASE[e]))
    for c in S.REFUSALS + S.EMPTY_CASES:
        names = {n for _, n in protos[c.run[0]][1]}
        assert {k for k in c.run[1] if not k.startswith("_")} <= names and set(c.run[2]) <= names, c.id
        assert c.run[3] == (S.BH_OK if c.family == "empty" else c.run[3]) and c.run[3] in (S.BH_OK, S.BH_E_BADARG, S.BH_E_UNSUPPORTED)
    # every entry point whose check is `B < 0`, `N < 0` or `n < 0` is in the empty-batch table
    src = "\n".join(open(os.path.join(ROOT, "bihome_amd", "csrc", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "bihome_amd", "csrc"))) if f.endswith(".hip"))
    src = re.sub(r"//.*", "", src)
    listed = {e for e, _, _, _, _ in S.EMPTY_BATCH}
    for m in re.finditer(r"\bint (bh_\w+)\(([^)]*)\)\s*\{(.*?)\n\}", src, flags=re.S):
        name, body = m.group(1), m.group(3)
        if re.search(r"\b(B|N|n|Bn) < 0\b", body) or (name in protos and re.search(r"(triplet_args|proj_args)\(", body)):
            assert name in listed, "%s checks a negative count and is not in EMPTY_BATCH" % name


@pytest.mark.parametrize("case", S.REFUSALS + S.EMPTY_CASES, ids=[c.id for c in S.REFUSALS + S.EMPTY_CASES])
def test_refusals_come_before_any_launch(case):
    """The return code and the untouched buffers of every refusal and empty-batch case, here too: without a GPU a call that got as far as
    a launch (or a memset) returns a hipError_t instead.  (The three forwards that still write a zero loss for an empty batch do launch.)"""
    import torch
    entry, over, null, code = case.run
    if case.family == "empty" and dict(next(w for e, _, _, _, w in S.EMPTY_BATCH if e == entry)) and not torch.cuda.is_available():
        # these three DO launch (one workgroup writes the zero loss): without a device the launch's error comes back, not a refusal
        assert S.RawCall(entry, over, null).rc > 0
        return
    r = S.RawCall(entry, over, null)
    assert r.rc == code, "%s: returned %d, the header documents %d" % (case.id, r.rc, code)
    r.untouched(but=dict(next(w for e, _, _, _, w in S.EMPTY_BATCH if e == entry)) if case.family == "empty" else ())


def test_null_pointers_are_refused_before_any_launch():
    protos = S.header_prototypes()
    for entry, fname, line, pointers in S.NULL_CASES:
        names = [n for c, n in protos[entry][1] if c == "ptr"]
        assert set(pointers) <= set(names), (entry, set(pointers) - set(names))
        text = open(os.path.join(ROOT, "bihome_amd", "csrc", fname)).read().split("\n")
        assert "BH_E_BADARG" in " ".join(text[line - 1:line + 2]), (fname, line)              # (the check: its `return` is at most two lines below)
        for ptr in pointers:
            r = S.RawCall(entry, {}, (ptr,) + (("scratch",) if entry == "bh_synth_blobs" else ()))
            assert r.rc == S.BH_E_BADARG, "%s with %s = NULL returned %d" % (entry, ptr, r.rc)
            r.untouched()
