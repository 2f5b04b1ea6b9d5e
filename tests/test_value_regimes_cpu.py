"""What tests/test_value_regimes_gpu.py assumes of its inputs and of its yardsticks, checked without a GPU: the generators of
tests/value_regimes.py produce the value regimes they claim (shares of exact zeros and ties, var = 0 channels, dead channels), the caps on
excluded elements hold for the committed seeds, torch's float32 BatchNorm - the yardstick of the measured bounds - stays inside the bounds
itself, and the header, the ctypes table and the library agree on bh_absmax."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import value_regimes as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# post-ReLU features (section 5)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("B,hf,C", V.LOSS_SHAPES)
def test_post_relu_features_are_what_they_claim(B, hf, C, rep):
    from test_loss_variants_cpu import aware_terms, cosine_loss
    from test_projection_cpu import l1_loss
    d = V.post_relu_features(B, hf, C, rep=rep)
    r = lambda a: a.repeat_interleave(rep, 0)
    for k in ("f1", "f2", "f1w", "f2w"):
        assert (d[k] == 0).double().mean() > 0.5 and (d[k] >= 0).all()            # more than half exact zeros
    assert d["tie"].double().mean() >= 0.25 - 1.0 / (hf * hf)
    tie1, tie2 = d["f1w"] == r(d["f2"]), d["f2w"] == d["f1"]
    for b, i, j in d["zero_f2"] + [(z[0] // rep,) + z[1:] for z in d["zero_f1w"]]:
        tie1[b * rep:(b + 1) * rep, i, j] = True                                   # (the all-zero vectors were set after the ties)
    assert tie1[:, d["tie"]].all() and tie2[:, d["tie"]].all()                    # every channel of a quarter of the pixels
    off = ~d["tie"]
    nz = (d["f1w"] != 0) & (r(d["f2"]) != 0)
    assert (tie1 & nz)[:, off].any() and not tie1[:, off].all()                   # single channels elsewhere, nonzero ones among them
    assert len(d["zero_f2"]) >= 2 and len(d["zero_f1w"]) >= 2
    assert not any(bool(d["tie"][i, j]) for _, i, j in d["zero_f2"][:1] + d["zero_f1w"][:1])
    assert (d["m1w"][0, :2] == 0).all() and d["m2w"][-1].sum() < 1
    # both hinge states occur, and the elements at which the float32 indicator may differ from the float64 one stay below 1 %
    D = lambda k: d[k].double()
    t1, t2 = aware_terms(D("f1"), D("f2"), D("f1w")[::rep], D("f2w"), V.AWARE_MARGIN)
    _, _, tc = cosine_loss(D("f1"), D("f2"), D("f1w"), D("m1w"), V.COS_MARGIN, rep=rep)
    _, _, tl = l1_loss(D("f1"), D("f2"), D("f1w"), D("m1w"), V.l1_margin(d, rep), rep=rep)
    for t in (t1, t2, tc, tl):
        assert 0.1 < (t > 0).double().mean() < 0.9
        assert (t.abs() < V.FLIP * t.abs().max()).double().mean() < 0.01
    assert abs((tl > 0).double().mean().item() - 0.5) <= 1.0 / tl.numel() and (tl != 0).all()      # the L1 margin halves the pixels, none on the hinge
    for margin_t in (aware_terms(D("f1"), D("f2"), D("f1w")[::rep], D("f2w"), -1e3)[0], cosine_loss(D("f1"), D("f2"), D("f1w"), D("m1w"), -1e3, rep=rep)[2]):
        assert (margin_t < 0).all()                                                # margin -1e3: every hinge inactive


# ------------------------------------------------------------------------------------------------
# BatchNorm channels (section 4)
# ------------------------------------------------------------------------------------------------
def _f32_batchnorm(x, gamma, beta, groups):
    n = x.shape[0] // groups
    return torch.cat([F.batch_norm(x[i * n:(i + 1) * n].permute(0, 3, 1, 2), None, None, gamma, beta, True, 0.1, V.BN_EPS).permute(0, 2, 3, 1)
                      for i in range(groups)], 0)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("groups,N,H,W", V.BN_SHAPES)
def test_batchnorm_channels_are_what_they_claim(groups, N, H, W, seed):
    x, gamma, beta = V.bn_channels(groups, N, H, W, seed=seed)
    ref = V.bn_reference(x, gamma, beta, groups, None, True)
    assert (ref["var"][:, [V.BN_CONSTANT, V.BN_ZERO]] == 0).all()                  # exactly
    assert (ref["mean"][:, V.BN_CONSTANT] == 3).all() and (ref["mean"][:, V.BN_ZERO] == 0).all()
    for c, sign in ((V.BN_PLUS, 1), (V.BN_MINUS, -1)):
        ratio = sign * ref["mean"][:, c] / ref["var"][:, c].sqrt()
        assert (ratio > 2 ** 9.75).all() and (ratio < 2 ** 10.25).all()            # |mean| / sigma ~ 2^10
    assert (x[..., V.BN_ONE_HOT].reshape(groups, -1).sum(1) == 1).all() and ((x[..., V.BN_ONE_HOT] == 0) | (x[..., V.BN_ONE_HOT] == 1)).all()
    assert (ref["pre"][..., V.BN_DEAD] < -1).all() and (ref["y"][..., V.BN_DEAD] == 0).all()      # dead under ReLU, far from the decision
    for c in (V.BN_CONSTANT, V.BN_ZERO):
        assert (ref["y"][..., c] == 0.25).all()                                    # y = beta exactly in float64
    assert (ref["pre"][..., V.BN_ONE_HOT].abs() > 0.1).all()                       # the one-hot channel's ReLU decision is not at a rounding
    # the cap of the `near` convention: at most 1 % of the elements within NEAR of the ReLU decision; the GPU tests that cannot zero an
    # output gradient (it is made by a kernel) use seed 0 and assume there is none
    near = V.near_relu(ref["pre"])
    assert near.double().mean() <= 0.01
    if seed == 0:
        assert not near.any()
        res = torch.randn(N, H, W, V.BN_C, generator=torch.Generator().manual_seed(3))
        assert not V.near_relu(V.bn_reference(x, gamma, beta, groups, res, True)["pre"]).any()
        xb, gb, bb = V.bn_channels(groups, N, H, W, seed=1)
        assert V.near_relu(ref["pre"] + V.bn_reference(xb, gb, bb, groups)["pre"]).double().mean() <= 0.01


@pytest.mark.parametrize("groups,N,H,W", V.BN_SHAPES)
def test_float32_batchnorm_is_inside_the_bounds_held_to_the_kernels(groups, N, H, W):
    """The derived forward bound holds for torch's float32 BatchNorm (the same fp32 coefficient chain), which does NOT meet the bound of a
    shift rounded once from float64 - the reason include/bihome.h states the bound with |mean scale| + |beta|; and in the backward pass the
    float32 yardstick alone stays below the 3e-5 floor in every channel, the mean +-1000 ones included."""
    worst_once = 0.0
    for seed in (0, 1):
        x, gamma, beta = V.bn_channels(groups, N, H, W, seed=seed)
        ref = V.bn_reference(x, gamma, beta, groups)
        err = (_f32_batchnorm(x, gamma, beta, groups).double() - ref["y"]).abs()
        assert (err <= V.bn_forward_bound(x, ref)).all()
        worst_once = max(worst_once, (err / V.bn_forward_bound(x, ref, shift_rounded_once=True)).max().item())
    assert worst_once > 1.0                                                  # (2.3 ... 3.6 x on these seeds)
    x, gamma, beta = V.bn_channels(groups, N, H, W)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(6))
    grads = {}
    for dtype in (torch.float64, torch.float32):
        xt, gt, bt = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
        y = V.bn_reference(xt, gt, bt, groups)["pre"] if dtype == torch.float64 else _f32_batchnorm(xt, gt, bt, groups)
        y.clamp_min(0).backward(gy.to(dtype))
        grads[dtype] = xt.grad.double().reshape(-1, V.BN_C)
    scale = grads[torch.float64].abs().amax(0)
    spread = (grads[torch.float32] - grads[torch.float64]).abs().amax(0)
    assert (spread <= 3e-5 * scale).all() and scale[V.BN_DEAD] == 0 and spread[V.BN_DEAD] == 0
    assert (spread[[V.BN_PLUS, V.BN_MINUS]] > 0).all()


# ------------------------------------------------------------------------------------------------
# warp (section 6)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [64, 48])
def test_warp_homographies_exclude_at_most_one_percent_of_the_pixels(size):
    from oracle import bihome_oracle as O
    from test_head_kernels_gpu import coordinate_ties
    B = 2
    corners = torch.tensor([[0, 0], [size, 0], [size, size], [0, size]], dtype=torch.float64).repeat(B, 1, 1)
    H = O.four_point_to_homography(corners, torch.tensor(V.warp_delta(B, size), dtype=torch.float64))
    tie, _ = coordinate_ties(H, size, size)
    assert tie.double().mean() <= 0.01
    # sample 1 samples partly outside its source, sample 0 mostly inside
    ys, xs = torch.meshgrid(torch.arange(size, dtype=torch.float64), torch.arange(size, dtype=torch.float64), indexing="ij")
    q = torch.einsum("bij,hwj->bhwi", H, torch.stack([xs, ys, torch.ones_like(xs)], -1))
    u = q[..., 0] / q[..., 2]
    assert (u[1] > size).double().mean() > 0.2 and (u[0] > size).double().mean() < 0.2


@pytest.mark.parametrize("size", [64, 48, 128])
def test_horizon_homography_puts_qz_on_zero_in_float32(size):
    """The horizon of V.HORIZON is column x = 8: qz is exactly 0 there in the float32 arithmetic of csrc/warp_tap.h (two fused multiply-adds),
    so the kernels take the |qz| <= 1e-8 guard on that column and nowhere else; the float64 stand-in (V.warp_pixel_guard) takes it on the
    same pixels; and the pixels excluded as coordinate ties stay below 1 % (none of them on the guarded column) - on the warp's own grid and
    on the photometric head's 128 x 128 patch inside a 240 x 320 image."""
    qz = V.qz_float32(V.HORIZON, size, size)
    assert (qz[:, 8] == 0).all() and (np.abs(np.delete(qz, 8, axis=1)) >= 0.125).all()
    H = torch.tensor([V.HORIZON] * 2, dtype=torch.float64)
    _, _, guard = V._project_guarded(H, size, size, torch.float64)
    _, _, guard32 = V._project_guarded(H, size, size, torch.float32)
    assert guard[:, :, 8].all() and guard.sum() == 2 * size and torch.equal(guard, guard32)
    origin = torch.tensor([[60., 40.], [100., 70.]]) if size == 128 else None
    tie = V.guarded_coordinate_ties(H, size, size, origin=origin, extent=320 if size == 128 else None)
    assert tie.double().mean() <= 0.01 and not tie[:, :, 8].any()
    if size != 128:
        from test_head_kernels_gpu import coordinate_ties
        assert torch.equal(coordinate_ties(H, size, size)[0], tie)             # the helper's own exclusion sees the same pixels
    # away from the guard the stand-in is the oracle's warp
    from oracle import bihome_oracle as O
    img = torch.randn(2, 1, size, size, dtype=torch.float64, generator=torch.Generator().manual_seed(size))
    d = (V.warp_pixel_guard(img, H) - O.warp_image(img, H)).abs()
    cols = [c for c in range(size) if c != 8]
    assert d[..., cols].max() <= 1e-10 and d[..., 8].max() > 0.1


# ------------------------------------------------------------------------------------------------
# bh_absmax (section 3)
# ------------------------------------------------------------------------------------------------
def test_absmax_lengths_cover_the_kernel_paths():
    per_pass = 256 * 8 * 4                          # floats of one workgroup's eight-deep pass (csrc/pool.hip absmax_kernel)
    n = V.ABSMAX_LENGTHS
    assert any(x < 4 for x in n) and 4 in n and any(x > 4 and x & 3 for x in n)                    # tail only, one float4, float4 + tail
    assert per_pass - 1 in n and per_pass in n                                                        # one side and the other of a full pass
    assert any(x // 4 > 512 * 256 * 8 and x & 3 == 0 for x in n)                                      # all 512 workgroups loop, then a remainder
    assert any(x > per_pass and x & 3 for x in n)


def test_absmax_header_and_ctypes_signature_agree():
    from bihome_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bihome.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bh_absmax\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/bihome.h does not declare bh_absmax"
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_int64}[arg.rsplit(" ", 1)[0]])
    assert _lib.SIGNATURES["bh_absmax"] == want and want == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bh_absmax")
    assert re.search(r"#define\s+BH_AMAX_FLOATS\s+512\b", text) and _lib.AMAX_FLOATS == 512
