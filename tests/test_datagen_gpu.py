"""The device pair generator beyond grayscale patches (bh_synth_batch, bihome_amd/synth_gpu.py): the 'all_points' perspective-field
target, RGB patches, the gray form against bh_synth_pairs bit for bit, taps outside the base image, photometric records drawn on the
device, and whole batches from GpuPairGenerator.from_config through one training step.  The oracle throughout is the host generator's
arithmetic (bihome_amd/synth.py), which tests/test_datagen_cpu.py pins against the reference's own transforms."""
import ctypes

import numpy as np
import pytest
import torch

from bihome_amd import configs, synth
from bihome_amd.weights import load_synthetic

pytestmark = pytest.mark.gpu

MEAN, STD = 0.443, 0.129


def square(P):
    return np.array([[0, 0], [P, 0], [P, P], [0, P]], np.float64)


def standardise(crop, channels):
    """The two arms of make_pairs (bihome_amd/synth.py): DictToGrayscale + DictStandardize, or the per-channel standardisation."""
    if channels == 1:
        return synth.gray_standardize(crop, MEAN, STD)
    return ((crop.astype(np.float32) / 255) - MEAN).transpose(2, 0, 1) / STD


def host_pairs(gen, idx, origin, delta, photo, b):
    """patch_1 / patch_2 of sample b by the host generator's arithmetic on the same (image, origin, delta, records)."""
    P = gen.patch
    img = gen.images[int(idx[b])].cpu().numpy().transpose(1, 2, 0)
    im1 = im2 = img.astype(np.float64)
    if photo is not None:
        rec = photo[b].cpu().numpy().astype(np.float64)
        im1 = synth.apply_photometric(img, rec[:6]).astype(np.float64)
        im2 = synth.apply_photometric(img, rec[6:]).astype(np.float64)
    x0, y0 = int(origin[b, 0]), int(origin[b, 1])
    H = synth.four_point_homography(square(P), square(P) + delta[b].cpu().numpy().astype(np.float64))
    T = np.array([[1, 0, x0], [0, 1, y0], [0, 0, 1.0]])
    return (standardise(im1[y0:y0 + P, x0:x0 + P], gen.channels), standardise(synth.warp_bilinear(im2, T @ H, P, P), gen.channels))


def synth_call(name, images, idx, origin, H64, photo, P, C=1, target=False):
    """bh_synth_batch / bh_synth_pairs through ctypes: (patch_1, patch_2, target or None)."""
    from bihome_amd._lib import check, lib
    pv = ctypes.c_void_p
    B, (n, _, Hs, Ws) = idx.shape[0], images.shape
    p1 = torch.empty(B, C, P, P, device="cuda")
    p2 = torch.empty_like(p1)
    tg = torch.full((B, 2, P, P), float("nan"), device="cuda") if target else None
    head = (pv(images.data_ptr()), pv(idx.data_ptr()), pv(origin.data_ptr()), pv(H64.data_ptr()),
            pv(photo.data_ptr()) if photo is not None else None, B, n, Hs, Ws, P)
    stream = pv(torch.cuda.current_stream().cuda_stream)
    if name == "bh_synth_pairs":
        check(lib.bh_synth_pairs(*head, MEAN, STD, pv(p1.data_ptr()), pv(p2.data_ptr()), stream), name)
    else:
        check(lib.bh_synth_batch(*head, C, MEAN, STD, pv(p1.data_ptr()), pv(p2.data_ptr()),
                                 pv(tg.data_ptr()) if target else None, stream), name)
    return p1, p2, tg


# ---- 1. all-points target -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch,rho,B", [(32, 8, 5), (128, 32, 2)])
def test_all_points_target(patch, rho, B):
    from bihome_amd.synth_gpu import GpuPairGenerator
    out = GpuPairGenerator(n_images=2, patch=patch, rho=rho, seed=3, target_gen="all_points").next(B)
    assert set(out) == {"patch_1", "patch_2", "delta", "target"} and out["target"].shape == (B, 2, patch, patch)
    delta, got = out["delta"].cpu().numpy().astype(np.float64), out["target"].cpu().numpy()
    ref = np.stack([synth.perspective_field(synth.four_point_homography(square(patch), square(patch) + delta[b]), patch)
                    for b in range(B)])
    print("MEASURED all-points target P %d: max|hip - host| %.3e px (max |field| %.1f)" % (patch, np.abs(got - ref).max(), np.abs(ref).max()))
    # the field is evaluated in double and rounded once to float32 (an ulp at these magnitudes is < 1e-5); 1e-4 px is the
    # project's corner-mapping bound
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4)
    np.testing.assert_allclose(got[:, :, 0, 0], delta[:, 0], rtol=0, atol=1e-4)


def test_four_points_target_is_delta():
    from bihome_amd.synth_gpu import GpuPairGenerator
    out = GpuPairGenerator(n_images=2, patch=32, rho=8, seed=3, target_gen="4_points", corners=True).next(5)
    assert set(out) == {"patch_1", "patch_2", "delta", "target", "corners"}
    assert out["target"] is out["delta"]
    c = out["corners"].cpu().numpy()
    assert np.array_equal(c, c[:, :1] + square(32)[None].astype(np.float32))
    with pytest.raises(ValueError):
        GpuPairGenerator(n_images=1, patch=32, rho=8, channels=3, image=True)
    with pytest.raises(ValueError):
        GpuPairGenerator(n_images=1, patch=32, rho=8, channels=3).next(1, image=True)


# ---- 2. RGB patches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch,rho,B,md", [(32, 8, 4, 0), (32, 8, 4, 32), (256, 64, 2, 32)])
def test_rgb_patches_match_host_arithmetic(patch, rho, B, md):
    from bihome_amd.synth_gpu import GpuPairGenerator
    gen = GpuPairGenerator(n_images=2, patch=patch, rho=rho, seed=0, photometric_max_delta=md, channels=3)
    assert (gen.h, gen.w) == {32: (240, 320), 256: (432, 512)}.get(patch, (gen.h, gen.w))      # (other patch sizes: tests/shape_edges.py)
    idx, origin, delta, photo = gen.draw(B)
    out = gen.make(idx, origin, delta, photo)
    assert out["patch_1"].shape == out["patch_2"].shape == (B, 3, patch, patch)
    if md and B == 4:            # the eight records exercise every part of the distortion
        rec = photo.cpu().numpy().reshape(8, 6)
        assert (rec[:, 5] > 0).any() and (rec[:, 3] != 0).any() and (rec[:, 2] != 1).any()
        assert (rec[:, 1] != 1).any() and (rec[:, 4] != 1).any() and (rec[:, 0] != 0).any()
    worst = 0.0
    for b in range(B):
        ref1, ref2 = host_pairs(gen, idx, origin, delta, photo, b)
        got1, got2 = out["patch_1"][b].cpu().numpy(), out["patch_2"][b].cpu().numpy()
        worst = max(worst, np.abs(got1 - ref1).max(), np.abs(got2 - ref2).max())
        # the bars of test_gpu_pair_generator_matches_host_generator (tests/test_head_kernels_gpu.py) for the same per-tap arithmetic
        np.testing.assert_allclose(got1, ref1, rtol=0, atol=3e-3 if md else 2e-3)
        np.testing.assert_allclose(got2, ref2, rtol=0, atol=3e-3 if md else 2e-3)
    print("MEASURED rgb patches P %d md %d: max abs difference %.2e (standardised units)" % (patch, md, worst))
    assert not torch.equal(out["patch_1"][:, 0], out["patch_1"][:, 1])          # (three distinct planes)


# ---- 3. one kernel, same bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("md", [0, 32])
def test_gray_form_is_bh_synth_pairs_bitwise(md):
    from bihome_amd import kernels as K
    from bihome_amd.synth_gpu import GpuPairGenerator
    gen = GpuPairGenerator(n_images=2, patch=32, rho=8, seed=1, photometric_max_delta=md)
    idx, origin, delta, photo = gen.draw(3)
    assert (photo is not None) == bool(md)
    H64, _ = K.h4pt_fwd(delta, 32)
    a1, a2, _ = synth_call("bh_synth_pairs", gen.images, idx, origin, H64, photo, 32)
    b1, b2, _ = synth_call("bh_synth_batch", gen.images, idx, origin, H64, photo, 32)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    # the target is an extra output: the patches next to it are the same bits
    c1, c2, tg = synth_call("bh_synth_batch", gen.images, idx, origin, H64, photo, 32, target=True)
    assert torch.equal(a1, c1) and torch.equal(a2, c2) and torch.isfinite(tg).all()


# ---- 4. taps outside the base image ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
def test_taps_outside_the_base_image(C):
    from bihome_amd import kernels as K
    P, Hs, Ws = 32, 48, 64
    img = np.full((Hs, Ws, 3), 255.0)
    origins = [(0, 0), (32, 16)]
    deltas = np.array([[[-6, -6], [5, -4], [6, 6], [-5, 4]], [[-5, 4], [6, 6], [7, 7], [-6, 5]]], np.float64)
    images = torch.tensor(img.transpose(2, 0, 1)[None], dtype=torch.float32, device="cuda").contiguous()
    idx = torch.zeros(2, dtype=torch.int32, device="cuda")
    origin = torch.tensor(origins, dtype=torch.float32, device="cuda")
    H64, _ = K.h4pt_fwd(torch.tensor(deltas, dtype=torch.float32, device="cuda"), P)
    p1, p2, tg = synth_call("bh_synth_batch", images, idx, origin, H64, None, P, C=C, target=True)
    for b, (x0, y0) in enumerate(origins):
        H = synth.four_point_homography(square(P), square(P) + deltas[b])
        T = np.array([[1, 0, x0], [0, 1, y0], [0, 0, 1.0]])
        raw = synth.warp_bilinear(img, T @ H, P, P)
        outside, partly = (raw[..., 0] == 0).sum(), ((raw[..., 0] > 1e-6) & (raw[..., 0] < 255 - 1e-6)).sum()
        print("oracle sample %d: %d pixels fully outside, %d partly" % (b, outside, partly))
        assert outside > 0 and partly > 0
        np.testing.assert_allclose(p2[b].cpu().numpy(), standardise(raw, C), rtol=0, atol=2e-3)
        np.testing.assert_allclose(p1[b].cpu().numpy(), standardise(img[y0:y0 + P, x0:x0 + P], C), rtol=0, atol=2e-3)
    assert torch.isfinite(tg).all()
    np.testing.assert_allclose(tg[:, :, 0, 0].cpu().numpy(), deltas[:, 0], rtol=0, atol=1e-4)


# ---- 5. device draws ------------------------------------------------------------------------------------------------------------
def test_device_drawn_records():
    from bihome_amd.synth_gpu import GpuPairGenerator
    kw = dict(n_images=2, patch=32, rho=8, seed=9, photometric_max_delta=32, photometric_draws="device")
    gen = GpuPairGenerator(**kw)
    idx, origin, delta, photo = gen.draw(64)
    assert photo.shape == (64, 12) and photo.is_cuda and photo.dtype == torch.float32
    again = GpuPairGenerator(**kw).draw(64)
    for a, b in zip((idx, origin, delta, photo), again):
        assert torch.equal(a, b)
    rec = photo.cpu().numpy().reshape(128, 6)
    assert (rec[:, 5] > 0).any() and (rec[:, 3] != 0).any() and (rec[:, 2] != 1).any() and (rec[:, 0] != 0).any()
    assert not ((rec[:, 1] != 1) & (rec[:, 4] != 1)).any() and (rec[:, 1] != 1).any() and (rec[:, 4] != 1).any()
    out = gen.make(idx, origin, delta, photo)
    for b in (0, 31, 63):
        ref1, ref2 = host_pairs(gen, idx, origin, delta, photo, b)
        np.testing.assert_allclose(out["patch_1"][b].cpu().numpy(), ref1, rtol=0, atol=3e-3)
        np.testing.assert_allclose(out["patch_2"][b].cpu().numpy(), ref2, rtol=0, atol=3e-3)
    b1, b2 = GpuPairGenerator(**kw).next(64), GpuPairGenerator(**kw).next(64)
    assert set(b1) == {"patch_1", "patch_2", "delta"}
    for k in b1:
        assert torch.equal(b1[k], b2[k]), k


@pytest.mark.parametrize("md", [0, 32])
def test_host_draws_are_what_they_were(md):
    """photometric_draws='host' (the default): draw() restated as it was before the generator learned the other modes - the same
    calls on a device generator and a RandomState of the same seed - gives the same bits, call after call."""
    from bihome_amd.synth_gpu import GpuPairGenerator
    seed, B, patch, rho = 12, 6, 128, 32
    gen = GpuPairGenerator(n_images=3, seed=seed, photometric_max_delta=md)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rs = np.random.RandomState(seed)
    half = patch // 2
    for _ in range(2):
        idx = torch.randint(0, 3, (B,), generator=g, device="cuda", dtype=torch.int32)
        px = torch.randint(rho + half, gen.w - rho - half + 1, (B,), generator=g, device="cuda")
        py = torch.randint(rho + half, gen.h - rho - half + 1, (B,), generator=g, device="cuda")
        origin = torch.stack([px - half, py - half], 1).to(torch.float32)
        delta = torch.randint(-rho, rho, (B, 4, 2), generator=g, device="cuda").to(torch.float32)
        photo = None
        if md:
            recs = np.stack([np.concatenate([synth.draw_photometric(rs, md), synth.draw_photometric(rs, md)]) for _ in range(B)])
            photo = torch.tensor(recs, dtype=torch.float32, device="cuda")
        got = gen.draw(B)
        assert torch.equal(got[0], idx) and torch.equal(got[1], origin) and torch.equal(got[2], delta)
        assert (got[3] is None) if photo is None else torch.equal(got[3], photo)
    assert set(gen.make(*got)) == {"patch_1", "patch_2", "delta"}


# ---- 6. whole batches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zeng-orig", "nguyen-orig", "zeng-bihome-pds", "zeng-bihome-rgb256"])
def test_from_config_batch_trains_one_step(name):
    from bihome_amd.step import build_loss, build_model, build_optimizer, train_step
    from bihome_amd.synth_gpu import GpuPairGenerator, batch_spec
    cfg = configs.get(name)
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    if hasattr(model[1], "auxiliary_resnet"):
        load_synthetic(model[1].auxiliary_resnet, 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    gen = GpuPairGenerator.from_config(cfg, n_images=2)
    assert gen.photometric_draws == "device"
    batch = gen.next(2)
    spec = batch_spec(cfg)
    P, C = spec["patch"], spec["channels"]
    assert batch["patch_1"].shape == batch["patch_2"].shape == (2, C, P, P)
    want = {"patch_1", "patch_2", "delta"} | ({"target"} if spec["target_gen"] else set()) | \
        ({"corners"} if spec["corners"] else set()) | ({"image_1"} if spec["image"] else set())
    assert set(batch) == want
    if spec["target_gen"] == "all_points":
        assert batch["target"].shape == (2, 2, P, P)
    loss, dgt, _ = train_step(model, dict(batch), opt, sched, loss_fn=build_loss(cfg["SOLVER"]))
    assert np.isfinite(loss.item())
    assert torch.equal(dgt.reshape(2, 4, 2), batch["delta"])
