"""The photometric baseline on the MI355X (config/s-coco/nguyen-orig-lr-5e-3.yaml): the warp-and-crop gather of PhotometricHead
(bh_photo_warp_fwd) and its adjoint against a float64 restatement from the oracle, the identity map, the whole model against the
reference's own modules (tests/golden/nguyen_orig_b4_*.npz, tools/make_golden_nguyen.py), determinism and HIP-graph capture, the
device data path (bh_synth_image) and the pds-coco sibling (NoOpHead + L1Loss)."""
import numpy as np
import pytest
import torch

from bihome_amd import configs, synth
from bihome_amd.weights import load_synthetic
from oracle import bihome_oracle as O

pytestmark = pytest.mark.gpu

SEED, BATCH = 23, 4                   # tools/make_golden_nguyen.py
KEYS = ("patch_1", "patch_2", "delta", "corners", "image_1")
SQUARE = np.array([[0, 0], [128, 0], [128, 128], [0, 128]], np.float64)


@pytest.fixture(scope="module")
def K():
    from bihome_amd import kernels
    return kernels


def cuda(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to("cuda", dtype).contiguous()


def relerr(a, ref):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def restated(image, corners, delta, dtype=torch.float64):
    """PhotometricHead.py:26-42 from the oracle alone: four_point_to_homography(corners, delta) in full-image coordinates, warp_image
    of the whole image, crop at the corners."""
    c = torch.as_tensor(np.asarray(corners), dtype=dtype)
    H = O.four_point_to_homography(c, delta.to(dtype))
    warped = O.warp_image(torch.as_tensor(np.asarray(image)).to(dtype), H)
    ci = c.int()
    return torch.stack([warped[i, :, ci[i, 0, 1]:ci[i, 3, 1], ci[i, 0, 0]:ci[i, 1, 0]] for i in range(len(ci))])


def wild_deltas(rng, B, amp=80.0, square=SQUARE):
    """delta_hat uniform in +-amp px: many taps leave the 240 x 320 image.  Draws whose quadrilateral folds over (qz of the patch
    homography crossing 0 inside the patch - the map is then singular, in the reference as well) are redrawn."""
    out = []
    while len(out) < B:
        d = rng.uniform(-amp, amp, (4, 2))
        H = synth.four_point_homography(square, square + d)
        qz = H[2, 0] * square[:, 0] + H[2, 1] * square[:, 1] + H[2, 2]
        if qz.min() > 0.2:
            out.append(d)
    return np.stack(out).astype(np.float32)


def inputs(B, C, seed, Hi=240, Wi=320, P=128):
    """Hi x Wi images and P x P patches.  An image that cannot hold the generator's margin of 32 pixels around the patch (tests/shape_edges.py:
    images smaller than the patch) has the patch at its top-left corner and offsets of up to 5 P / 8, as 80 is of 128."""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = torch.nn.functional.avg_pool2d(torch.tensor(rng.standard_normal((B, C, Hi, Wi)), dtype=torch.float32), 3, 1, 1).numpy()
    square = SQUARE * (P / 128.0)
    if Wi - 32 - P >= 32 and Hi - 32 - P >= 32:
        x0 = rng.integers(32, Wi - 32 - P + 1, B)                  # the generator's range of top-left corners (rho 32)
        y0 = rng.integers(32, Hi - 32 - P + 1, B)
    else:
        x0 = y0 = np.zeros(B, np.int64)
    corners = np.stack([x0, y0], 1)[:, None, :].astype(np.float64) + square[None]
    return img, corners.astype(np.float32), wild_deltas(rng, B, 80.0 * P / 128.0, square)


@pytest.mark.parametrize("C", [1, 3])
def test_photo_warp_fwd_and_adjoint_vs_float64(K, C, base=None, B=8, Hi=240, Wi=320, P=128):
    img, corners, delta = inputs(B, C, 100 + C, Hi, Wi, P)
    Hp64, _ = K.h4pt_fwd(cuda(delta), P)
    origin = cuda(corners[:, 0])
    out = K.photo_warp_fwd(cuda(img), Hp64, origin, P)
    dt = torch.tensor(delta, dtype=torch.float64, requires_grad=True)
    # the restatement crops the warp of the WHOLE image: an image smaller than the patch is laid into a canvas of zeros that holds the crop
    # window (zero padding outside the image is what the warp reads there anyway: the same taps, the same values)
    kernel_img = img
    if Hi < P or Wi < P:
        canvas = np.zeros((B, C, max(Hi, P), max(Wi, P)), np.float32)
        canvas[:, :, :Hi, :Wi] = img
        img = canvas
    ref = restated(img, corners, dt)
    ref32 = restated(img, corners, torch.tensor(delta), torch.float32).double().numpy()
    ref_img, img = img, kernel_img
    o, r64 = out.cpu().double().numpy(), ref.detach().numpy()
    inside = (r64 != 0).mean()
    scale = np.abs(r64).max()
    err, spread = np.abs(o - r64).max(), np.abs(ref32 - r64).max()
    print("MEASURED photo warp C%d: max|hip - f64| %.3e = %.2e of range; f32 oracle's own %.3e; %.0f %% of pixels inside"
          % (C, err, err / scale, spread, 100 * inside))
    assert inside < 1.0                                           # (some taps do leave the image)
    # the bar of test_warp_fwd_bwd (tests/test_head_kernels_gpu.py): 1e-4 of the range, or 1.5x the f32 oracle's own spread
    assert err <= max(1e-4 * scale, 1.5 * spread), (err, scale, spread)
    # adjoint: photo_warp_bwd -> h4pt_bwd against float64 autograd of the restatement
    rng = np.random.Generator(np.random.PCG64(7 + C))
    go = rng.standard_normal(o.shape).astype(np.float32)
    (ref * torch.tensor(go, dtype=torch.float64)).sum().backward()
    r = dt.grad.numpy()
    d32 = torch.tensor(delta, requires_grad=True)
    (restated(ref_img, corners, d32, torch.float32) * torch.tensor(go)).sum().backward()
    spread = relerr(d32.grad, r)
    gH = K.photo_warp_bwd(cuda(img), Hp64, origin, cuda(go), P)
    if base is not None:
        # gH is a `+=` output: from a nonzero start (of the scale of the result itself), the start taken off again in float64
        from test_conv_kernels_gpu import grad_result, grad_start
        gH = grad_result(base, K.photo_warp_bwd(cuda(img), Hp64, origin, cuda(go), P, gH=grad_start(base, gH, torch.float64))).cuda()
    gd = K.h4pt_bwd(cuda(delta), Hp64, gH, P)
    gerr = relerr(gd, r)
    print("MEASURED photo warp adjoint C%d: max error %.3e of max|dL/ddelta|; f32 oracle's own %.3e" % (C, gerr, spread))
    # The warp adjoint's contract (1e-4 of the maximum) with the forward's widening: at most 1.5x the reference arithmetic's own float32
    # spread.  The widening is what applies here: the bilinear derivative jumps where a coordinate crosses an integer, and these maps
    # (+-80 px offsets, strong perspective, full-image coordinates up to ~300 px) put a few pixels per sample on the other side of such a
    # kink in float32 than in float64 - with a random g_out each moves an entry by ~1e-3 of the maximum.  The reference's own float32
    # chain is 1.5-2e-2 away from float64 on these draws; the kernel ~5e-3.
    assert gerr <= max(1e-4, 1.5 * spread), (gerr, spread)
    # deterministic mode: bitwise repeatable, and the atomic mode's sums to rounding
    with K.det_scope(True):
        d1 = K.photo_warp_bwd(cuda(img), Hp64, origin, cuda(go), P)
        d2 = K.photo_warp_bwd(cuda(img), Hp64, origin, cuda(go), P)
    assert torch.equal(d1, d2)
    assert relerr(gH, d1.cpu().numpy()) <= 1e-9


def test_identity_reproduces_patch_2(K):
    """delta_hat = delta (the ground truth) maps image_1's crop window onto patch_2 (s-coco: no photometric distortion), on the host
    generator's batch and on the device generator's."""
    from bihome_amd.synth_gpu import GpuPairGenerator
    d = synth.make_pairs(8, seed=31, image=True)
    batches = [{k: cuda(d[k]) for k in KEYS}, GpuPairGenerator(n_images=3, seed=4).next(8, image=True)]
    for data in batches:
        Hp64, _ = K.h4pt_fwd(data["delta"].contiguous(), 128)
        ph = K.photo_warp_fwd(data["image_1"], Hp64, data["corners"][:, 0].contiguous(), 128)
        p2 = data["patch_2"]
        rng_ = (p2.max() - p2.min()).item()
        err = (ph - p2).abs().max().item()
        print("MEASURED identity: max|patch_hat - patch_2| %.3e = %.2e of range" % (err, err / rng_))
        assert err <= 1e-4 * rng_, err


def _model():
    """build_model(nguyen-orig) in the mode in force (a model keeps the mode it was built with), synthetic weights."""
    from bihome_amd.step import build_loss, build_model
    cfg = configs.get("nguyen-orig")
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    return cfg, model, build_loss(cfg["SOLVER"])


def test_model_vs_reference_fixture(golden):
    import importlib
    from bihome_amd.step import build_optimizer, mace, predict, train_step
    g32, g64 = golden("nguyen_orig_b4_f32"), golden("nguyen_orig_b4_f64")
    cfg, model, loss_fn = _model()
    assert importlib.import_module("src.heads.PhotometricHead").Model is type(model[1])
    assert isinstance(loss_fn, torch.nn.L1Loss)
    d = synth.make_pairs(BATCH, seed=SEED, image=True)
    # inference at the initial weights (the fixture records it before training): eval.py:21-28
    data = {k: cuda(d[k]) for k in KEYS}
    dh_eval = predict(model, data)
    with torch.no_grad():
        dh2, H = model[1].predict_homography(model[0].predict_homography(dict(data)))
    assert torch.equal(dh2, dh_eval)
    e_dh = relerr(dh_eval.reshape(BATCH, 4, 2), g64["eval_delta_hat"])
    # H_hat through where it sends the corners (its entries span 1e-2 .. 1e4): within the delta_hat bar of the fixture's map
    c = torch.tensor(d["corners"], dtype=torch.float64)
    Href = torch.tensor(g64["eval_H_hat"])
    moved, moved_ref = O.transform_points(H.cpu().double(), c), O.transform_points(Href, c)
    e_H = (moved - moved_ref).abs().max().item() / np.abs(g64["eval_delta_hat"]).max()
    print("MEASURED nguyen-orig eval: delta_hat %.2e rel, H_hat corner transfer %.2e of max|delta_hat|" % (e_dh, e_H))
    assert e_dh < 2e-3 and e_H < 2e-3
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    losses = []
    for it in range(2):
        data = {k: cuda(d[k]) for k in KEYS}
        loss, dgt, dh = train_step(model, data, opt, sched, loss_fn=loss_fn)
        losses.append(loss.item())
        if it == 0:
            assert relerr(dh, g64["delta_hat0"]) < 2e-3
            assert abs(mace(dgt, dh) - g64["mace"][0]) < 1e-3 * g64["mace"][0]
            # patch_hat of this step: the head on the step's delta_hat (the same launch sequence as inside the step's forward)
            with torch.no_grad():
                ph = model[1](dict(data, delta_hat_12=dh))[1].cpu().double()
            own = restated(d["image_1"], d["corners"], dh.cpu().double()).numpy()
            ref = g64["patch_hat0"]
            scale = np.abs(ref).max()
            # bound: 1e-4 of the range (the kernel's own float32 arithmetic - pinned tightly against its restatement on this
            # delta_hat) plus what the backbone's delta_hat difference moves the taps by: |d patch / d delta| <= max |image
            # gradient| per pixel of displacement, and the map's displacement is at most ~ the largest corner difference (x2 margin
            # for the projective part and the two axes)
            im = d["image_1"].astype(np.float64)
            grad = max(np.abs(np.diff(im, axis=-1)).max(), np.abs(np.diff(im, axis=-2)).max())
            shift = np.abs(dh.cpu().double().numpy() - g64["delta_hat0"]).max()
            e_own = np.abs(ph.numpy() - own).max()
            e_ref = np.abs(ph.numpy()[..., ::8, ::8] - ref).max()
            print("MEASURED nguyen-orig patch_hat0: vs own restatement %.3e, vs fixture %.3e (bound %.3e: shift %.2e px, grad %.3f)"
                  % (e_own, e_ref, 1e-4 * scale + 2 * grad * shift, shift, grad))
            assert e_own <= 1e-4 * scale
            assert e_ref <= 1e-4 * scale + 2 * grad * shift
    print("MEASURED nguyen-orig loss hip %s f64 %s f32 %s" % (losses, g64["loss"], g32["loss"]))
    assert abs(losses[0] - g64["loss"][0]) <= 1e-4 * abs(g64["loss"][0])
    spread = abs(g32["loss"][1] - g64["loss"][1])
    assert abs(losses[1] - g64["loss"][1]) <= max(20 * spread, 2e-3 * abs(g64["loss"][1]))


def _steps(batches, how="eager"):
    """Deterministic mode: three training steps on `batches`, eagerly ('eager'; 'capturable': with the device-resident Adam state a
    graph needs) or as one eager warm-up step inside GraphedStep, capture and two replays ('graph')."""
    from bihome_amd import kernels as K
    from bihome_amd.step import build_optimizer, train_step
    prev = K.set_deterministic(True)
    try:
        cfg, model, loss_fn = _model()
        opt, sched = build_optimizer(model, cfg["SOLVER"], capturable=how != "eager")
        if how == "graph":
            from bihome_amd.graph import GraphedStep
            gs = GraphedStep(model, opt, sched, batches[0], loss_fn=loss_fn, warmup=1)
            losses = [None] + [gs(b)[0].item() for b in batches[1:]]
        else:
            losses = [train_step(model, b, opt, sched, loss_fn=loss_fn)[0].item() for b in batches]
        torch.cuda.synchronize()
        return losses, {k: v.detach().float().cpu().clone() for k, v in model[0].state_dict().items()}
    finally:
        K.set_deterministic(prev)


def test_deterministic_steps_and_graph_replay():
    d = synth.make_pairs(8, seed=33, image=True)
    batches = [{k: cuda(np.roll(d[k], i, axis=0)) for k in KEYS} for i in range(3)]
    l0, p0 = _steps(batches)
    l1, p1 = _steps(batches)
    assert l0 == l1, (l0, l1)
    bad = [k for k in p0 if not torch.equal(p0[k], p1[k])]
    assert not bad, bad[:10]
    le, pe = _steps(batches, "capturable")
    lg, pg = _steps(batches, "graph")
    assert lg[1:] == le[1:], (le, lg)
    bad = [k for k in pe if not torch.equal(pe[k], pg[k])]
    assert not bad, bad[:10]


@pytest.mark.parametrize("md", [0, 32])
def test_gpu_generator_image_1(md):
    from bihome_amd.synth_gpu import GpuPairGenerator
    gen = GpuPairGenerator(n_images=3, seed=12, photometric_max_delta=md)
    idx, origin, delta, photo = gen.draw(8)
    plain = gen.make(idx, origin, delta, photo)
    out = gen.make(idx, origin, delta, photo, image=True)
    assert set(plain) == {"patch_1", "patch_2", "delta"} and set(out) == set(plain) | {"image_1", "corners"}
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    assert out["image_1"].shape == (8, 1, gen.h, gen.w)
    c = out["corners"].cpu().numpy()
    assert np.array_equal(c, c[:, :1] + SQUARE[None].astype(np.float32))
    ci = c.astype(int)
    im = out["image_1"].cpu().numpy()
    p1 = out["patch_1"].cpu().numpy()
    imgs = gen.images.cpu().numpy()
    rec = photo.cpu().numpy().astype(np.float64) if photo is not None else None
    for b in range(8):
        assert np.array_equal(im[b, :, ci[b, 0, 1]:ci[b, 3, 1], ci[b, 0, 0]:ci[b, 1, 0]], p1[b]), b      # bitwise patch_1
        img = imgs[int(idx[b])].transpose(1, 2, 0)
        im1 = synth.apply_photometric(img, rec[b, :6]).astype(np.float64) if rec is not None else img.astype(np.float64)
        # the bar of test_gpu_pair_generator_matches_host_generator (tests/test_head_kernels_gpu.py)
        np.testing.assert_allclose(im[b, 0], synth.gray_standardize(im1)[0], atol=3e-3 if md else 2e-3)


def test_nguyen_orig_pds_one_step():
    from bihome_amd.step import build_loss, build_model, build_optimizer, mace, train_step
    cfg = configs.get("nguyen-orig-pds")
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    loss_fn = build_loss(cfg["SOLVER"])
    assert isinstance(loss_fn, torch.nn.L1Loss)
    d = synth.make_pairs(4, seed=44, photometric_max_delta=cfg["DATA"]["PHOTOMETRIC_MAX_DELTA"], target=True)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta", "target", "corners")}
    loss, dgt, dh = train_step(model, data, opt, sched, loss_fn=loss_fn)
    assert np.isfinite(loss.item()) and np.isfinite(mace(dgt, dh))
