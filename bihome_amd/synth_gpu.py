"""Device-side synthetic COCO-style pair generator.

Same sample distribution as the host generator `bihome_amd.synth.make_pairs` (which mirrors
`HomographyNetPrep`, src/data/transforms.py:441-725), but the crops/warps run in one HIP kernel
(`bh_synth_batch`) over base images that stay resident in HBM, so a training loop never waits for CPU workers.
Grayscale or RGB patches, the 'all_points' perspective-field target of the supervised configurations, and - with
`photometric_draws='device'` - the photometric records drawn on the device as well (`photometric_records`): nothing of a
step's batch is then made on, or copied from, the host.  The base images are synthetic textures, or - `bank=` - a dataset: a
`bihome_amd.bank.ImageBank` of uint8 images resident in HBM, whose batch is staged as float planes for the same kernels, and whose
images a `BankSampler` picks in the reference's order (`epoch`)."""
import ctypes

import numpy as np
import torch

from . import kernels as K
from . import synth
from ._lib import check, lib


def photometric_records(u, max_delta):
    """[..., 11] uniforms in [0, 1) -> [..., 6] PhotometricDistortSimple records in the layout and with the distribution of
    `synth.draw_photometric` (transforms.py:296-330): a pure tensor function (no loop over records, any device).  Columns of `u`:
    0 brightness on, 1 its value; 2 contrast before (on) or after the HSV part; 3 contrast on, 4 its value; 5 saturation on, 6 its
    value; 7 hue on, 8 its value; 9 permutation on, 10 its index.  A coin is `u >= 0.5` (randint(2) = floor(2u)), a value
    lo + (hi - lo) u, the index floor(6u).  Arithmetic in double (lo + (hi - lo) u near zero has no relative accuracy in float32),
    result float32."""
    u = u.double()
    on = u >= 0.5
    md = float(max_delta)
    lower, upper = 1.0 - md / 32 * 0.5, 1.0 + md / 32 * 0.5
    one, zero = torch.ones_like(u[..., 0]), torch.zeros_like(u[..., 0])
    br = torch.where(on[..., 0], -md + 2 * md * u[..., 1], zero)
    first = on[..., 2]
    con = torch.where(on[..., 3], lower + (upper - lower) * u[..., 4], one)
    c1, c2 = torch.where(first, con, one), torch.where(first, one, con)
    sat = torch.where(on[..., 5], lower + (upper - lower) * u[..., 6], one)
    hue = torch.where(on[..., 7], -md / 2 + md * u[..., 8], zero)
    perm = torch.where(on[..., 9], torch.floor(6 * u[..., 10]).clamp(max=5), zero) if md > 0 else zero
    return torch.stack([br, c1, sat, hue, c2, perm], -1).to(torch.float32)


def batch_spec(cfg):
    """GpuPairGenerator keyword arguments for a `configs.get(name)` dictionary (needs no GPU).  The patch geometry, the distortion
    and the target come from DATA; the head decides what else its batch carries: PhotometricHead warps the whole image_1 (and
    its corners), NoOpHead's '4_points' predict_homography reads the corners."""
    data, head = cfg["DATA"], cfg["MODEL"]["HEAD"]["NAME"]
    spec = {"patch": data["PATCH_SIZE"], "rho": data["RHO"], "photometric_max_delta": data.get("PHOTOMETRIC_MAX_DELTA", 0),
            "channels": data.get("PATCH_CHANNELS", 1), "target_gen": data.get("TARGET_GEN"),
            "image": head == "PhotometricHead", "corners": head in ("PhotometricHead", "NoOpHead")}
    if "AUGMENT_BLOB_POROSITY" in data and "AUGMENT_BLOBINESS" in data:            # CollatorWithBlobs (train.py:130-136,575-577)
        spec.update(blob_porosity=data["AUGMENT_BLOB_POROSITY"], blobiness=data["AUGMENT_BLOBINESS"])
    return spec


def apply_blobs(noise, other, patch1, patch2, sigma, porosity, want_field=False):
    """K.synth_blobs with its outputs allocated here: patch2 [B,C,P,P] is composited in place; returns (mask [B,P,P], field [B,P,P] |
    None - the continuous field, for tests)."""
    mask = torch.empty(noise.shape, dtype=torch.float32, device=noise.device)
    field = torch.empty(noise.shape, dtype=torch.float32, device=noise.device) if want_field else None
    n = K.synth_blobs_scratch_floats(noise.shape[0], noise.shape[-1])
    scratch = torch.empty(n, dtype=torch.float32, device=noise.device) if n else None
    return K.synth_blobs(noise, other, patch1, patch2, mask, sigma, porosity, field=field, scratch=scratch)


class GpuPairGenerator:

    def __init__(self, n_images=16, patch=128, rho=32, seed=42, photometric_max_delta=0, device="cuda", channels=1,
                 target_gen=None, corners=False, photometric_draws="host", image=False, blob_porosity=None, blobiness=None, bank=None,
                 draws="torch", rank=0, world=1):
        """bank: a `bihome_amd.bank.ImageBank` - the base images are the bank's (n_images = len(bank), h, w = bank.h, bank.w; the
        `n_images` argument is not used), staged per batch as float planes by bh_bank_gather_u8.  None: synthetic textures.
        draws: 'torch' - every random quantity comes from one torch.Generator, in sequence (the stream depends on the batch size of
        every earlier call); 'counter' - sample n of `seed` gets its parameters as a pure function of (seed, n) from one bh_synth_draw
        launch (`synth.counter_draws` is the definition), so a run can be resumed onto its stream (`state_dict`) and `world` ranks of B
        samples see exactly the samples of one rank of world * B: rank r's call takes samples position + r B .. position + (r + 1) B - 1,
        and every call moves `position` on by world * B.  photometric_draws is not consulted in counter mode."""
        if draws not in ("torch", "counter"):
            raise ValueError("draws must be 'torch' or 'counter', got %r" % (draws,))
        if int(world) < 1 or not 0 <= int(rank) < int(world):
            raise ValueError("rank must lie in [0, world): got rank %r, world %r" % (rank, world))
        self.draws, self.rank, self.world, self.seed, self.position = draws, int(rank), int(world), int(seed), 0
        if channels not in (1, 3):
            raise ValueError("channels must be 1 (grayscale) or 3 (RGB)")
        if target_gen not in (None, "4_points", "all_points"):
            raise ValueError("target_gen must be None, '4_points' or 'all_points'")
        if photometric_draws not in ("host", "device"):
            raise ValueError("photometric_draws must be 'host' or 'device'")
        if image and channels != 1:
            raise ValueError("image=True produces the grayscale image_1 of the photometric head: channels must be 1")
        self.blobs = synth.check_blob_options(blob_porosity, blobiness)
        self.blob_porosity, self.blobiness = blob_porosity, blobiness
        self.bank = bank
        if bank is not None:
            if bank.h < patch + 2 * rho or bank.w < patch + 2 * rho:
                # transforms.py:505-506 would draw the patch position from an empty range
                raise ValueError("the bank's images are %d x %d: patch + 2 rho = %d does not fit" % (bank.h, bank.w, patch + 2 * rho))
            self.h, self.w = bank.h, bank.w
            self.images = None                            # (the batch's images are gathered from the bank in make())
            self._arange = None
        else:
            rng = np.random.Generator(np.random.PCG64(seed))
            self.h = max(240, patch + 2 * rho + 48)
            self.w = max(320, patch + 2 * rho + 128)
            imgs = np.stack([synth.texture_image(rng, self.h, self.w).transpose(2, 0, 1) for _ in range(n_images)])
            self.images = torch.tensor(imgs, dtype=torch.float32, device=device).contiguous()      # [NI,3,H,W] 0..255
        self.patch, self.rho, self.pmd = patch, rho, photometric_max_delta
        self.channels, self.target_gen, self.corners, self.image = channels, target_gen, corners, image
        self.photometric_draws = photometric_draws
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)
        self._rs = np.random.RandomState(seed)            # photometric decisions (host draws, reference order)
        self.device = device

    @classmethod
    def from_config(cls, cfg, seed=42, n_images=16, device="cuda", photometric_draws="device", bank=None, draws="torch", rank=0, world=1):
        """The generator whose `next(B)` is the complete batch of the model `cfg` (a `configs.get(name)` dictionary) builds.
        bank: the dataset (an ImageBank, e.g. of DATA.DATASET_ROOT's .npy files) instead of synthetic textures."""
        return cls(n_images=n_images, seed=seed, device=device, photometric_draws=photometric_draws, bank=bank, draws=draws, rank=rank,
                   world=world, **batch_spec(cfg))

    @property
    def n_images(self):
        return len(self.bank) if self.bank is not None else self.images.shape[0]

    def _given_idx(self, idx, B):
        """A caller's image indices as the int32 [B] device tensor the kernels take.  Host values (a list, a numpy array, a CPU tensor) are
        range-checked here; a device tensor is not read back (with a bank, an index outside it is clamped by the gather)."""
        if isinstance(idx, torch.Tensor) and idx.device.type != "cpu":
            if idx.shape != (B,) or idx.dtype.is_floating_point:
                raise ValueError("idx must hold %d integers, got %s %s" % (B, tuple(idx.shape), idx.dtype))
            return idx.to(device=self.device, dtype=torch.int32).contiguous()
        a = np.asarray(idx)
        if a.shape != (B,) or a.dtype.kind not in "iu":
            raise ValueError("idx must hold %d integers, got %s %s" % (B, a.shape, a.dtype))
        if B and (int(a.min()) < 0 or int(a.max()) >= self.n_images):
            raise ValueError("idx must lie in [0, %d): got %d .. %d" % (self.n_images, a.min(), a.max()))
        return torch.tensor(a.astype(np.int32), dtype=torch.int32, device=self.device)

    def state_dict(self):
        """What `load_state_dict` needs to continue this generator's sample stream, to be saved next to a checkpoint.  Counter mode:
        {"draws", "seed", "position"} is the whole state.  Torch mode: also the torch.Generator's state and the host RandomState's."""
        state = {"draws": self.draws, "seed": self.seed, "position": self.position}
        if self.draws == "torch":
            state["torch_generator"] = self.gen.get_state()
            state["random_state"] = self._rs.get_state()
        return state

    def load_state_dict(self, state):
        """Continue the stream of a `state_dict()` of the same draw mode (another mode: ValueError).  The base images are the
        constructor's: build the generator with the seed (or the bank) it was built with before."""
        if state.get("draws") != self.draws:
            raise ValueError("a state of draws=%r cannot be loaded into a generator with draws=%r" % (state.get("draws"), self.draws))
        if self.draws == "torch":
            self.gen.set_state(state["torch_generator"])
            self._rs.set_state(state["random_state"])
        self.seed, self.position = int(state["seed"]), int(state["position"])

    def _draw_counter(self, B, idx, first):
        """draw() with draws='counter': one K.synth_draw call makes every tensor."""
        dev, P = self.device, self.patch
        given = self._given_idx(idx, B) if idx is not None else None            # (refused before anything is launched)
        if self.blobs and B < 2:
            raise ValueError("blobs paste content of ANOTHER sample of the batch: the batch needs at least 2 samples")
        advance = first is None
        if advance:
            first = self.position + self.rank * B
        own = torch.empty(B, dtype=torch.int32, device=dev)
        origin = torch.empty(B, 2, dtype=torch.float32, device=dev)
        delta = torch.empty(B, 4, 2, dtype=torch.float32, device=dev)
        photo = torch.empty(B, 12, dtype=torch.float32, device=dev) if self.pmd > 0 else None
        noise = torch.empty(B, P, P, dtype=torch.float32, device=dev) if self.blobs else None
        other = torch.empty(B, dtype=torch.int32, device=dev) if self.blobs else None
        K.synth_draw(self.seed, first, self.n_images, self.h, self.w, P, self.rho, self.pmd, own, origin, delta, photo, noise, other)
        if advance:
            self.position += self.world * B
        idx = given if given is not None else own              # (the stream's own index is made and dropped, as in torch mode)
        return (idx, origin, delta, photo) + (((noise, other),) if self.blobs else ())

    def draw(self, B, idx=None, first=None):
        """Random sample parameters exactly as transforms.py:505-506,538 draw them (uniform integer position with a
        rho margin, integer corner offsets in [-rho, rho-1]).  With blobs on, a fifth element (noise [B,P,P], other [B] int32) drawn
        AFTER everything else: a seed yields the same idx / origin / delta / photo with and without blobs.
        idx: the image of every sample ([B] integers, host or device - a sampler's batch) instead of the generator's own index draw,
        which is still made and dropped: a seed yields the same origin / delta / photo / blobs with and without idx.
        first (draws='counter' only): the stream position of the call's first sample; None: position + rank * B, and position then moves
        on by world * B.  An explicit `first` leaves `position` alone."""
        if self.draws == "counter":
            return self._draw_counter(B, idx, first)
        if first is not None:
            raise ValueError("first= names a position of the counter stream: it needs draws='counter'")
        g, dev, half = self.gen, self.device, self.patch // 2
        given = self._given_idx(idx, B) if idx is not None else None            # (refused before anything is drawn or launched)
        self.position += B                                                      # (torch mode: the number of samples drawn so far)
        idx = torch.randint(0, self.n_images, (B,), generator=g, device=dev, dtype=torch.int32)
        if given is not None:
            idx = given
        px = torch.randint(self.rho + half, self.w - self.rho - half + 1, (B,), generator=g, device=dev)
        py = torch.randint(self.rho + half, self.h - self.rho - half + 1, (B,), generator=g, device=dev)
        origin = torch.stack([px - half, py - half], 1).to(torch.float32).contiguous()
        delta = torch.randint(-self.rho, self.rho, (B, 4, 2), generator=g, device=dev).to(torch.float32).contiguous()
        photo = None
        if self.pmd > 0 and self.photometric_draws == "device":
            # the same decisions from one device draw: no Python loop over the batch, no host-to-device copy
            u = torch.rand((B, 2, 11), generator=g, device=dev)
            photo = photometric_records(u, self.pmd).reshape(B, 12).contiguous()
        elif self.pmd > 0:
            # PhotometricDistortSimple's decisions (transforms.py:296-330) for both images of every pair: the same record
            # layout and draw order as the host generator (synth.draw_photometric), drawn on the host - 12 floats per pair
            recs = np.stack([np.concatenate([synth.draw_photometric(self._rs, self.pmd), synth.draw_photometric(self._rs, self.pmd)])
                             for _ in range(B)])
            photo = torch.tensor(recs, dtype=torch.float32, device=dev).contiguous()
        if not self.blobs:
            return idx, origin, delta, photo
        if B < 2:
            raise ValueError("blobs paste content of ANOTHER sample of the batch: the batch needs at least 2 samples")
        # CollatorWithBlobs' draws (transforms.py:782-787): the field's noise, and a source uniform over the other B - 1 samples
        noise = torch.rand((B, self.patch, self.patch), generator=g, device=dev)
        r = torch.randint(0, B - 1, (B,), generator=g, device=dev)
        other = (r + (r >= torch.arange(B, device=dev))).to(torch.int32)
        return idx, origin, delta, photo, (noise, other)

    def make(self, idx, origin, delta, photo=None, blobs=None, image=None):
        """blobs = (noise, other), `draw`'s fifth element: patch_2 becomes CollatorWithBlobs' composite (bh_synth_blobs), and the batch
        gains blob_mask [B,1,P,P] and blob_other [B]; every other entry is what it is without blobs.
        image=True: also image_1 [B,1,h,w] (the whole standardised grayscale image 1 under its photometric record, bh_synth_image:
        its crop at the corners is patch_1 bitwise) and corners [B,4,2] - the batch of the photometric head (nguyen-orig).  Default:
        what the generator was constructed with."""
        image = self.image if image is None else image
        if image and self.channels != 1:
            raise ValueError("image=True produces the grayscale image_1 of the photometric head: channels must be 1")
        B, P, C = delta.shape[0], self.patch, self.channels
        H64, _ = K.h4pt_fwd(delta, P)
        p1 = torch.empty(B, C, P, P, dtype=torch.float32, device=self.device)
        p2 = torch.empty_like(p1)
        field = torch.empty(B, 2, P, P, dtype=torch.float32, device=self.device) if self.target_gen == "all_points" else None
        pv = ctypes.c_void_p
        images = self.images
        if self.bank is not None:
            # the batch's images leave the uint8 bank as the float planes the kernels read: image b of the staged batch is sample b's
            images = self.bank.gather(idx)
            if self._arange is None or self._arange.shape[0] != B:
                self._arange = torch.arange(B, dtype=torch.int32, device=self.device)
            idx = self._arange
        check(lib.bh_synth_batch(pv(images.data_ptr()), pv(idx.data_ptr()), pv(origin.data_ptr()), pv(H64.data_ptr()),
                                 pv(photo.data_ptr()) if photo is not None else None, B, images.shape[0], self.h,
                                 self.w, P, C, 0.443, 0.129, pv(p1.data_ptr()), pv(p2.data_ptr()),
                                 pv(field.data_ptr()) if field is not None else None,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "bh_synth_batch")
        out = {"patch_1": p1, "patch_2": p2, "delta": delta}
        if blobs is not None:
            if not self.blobs:
                raise ValueError("make(blobs=...) needs a generator constructed with blob_porosity and blobiness")
            noise, other = blobs
            mask, _ = apply_blobs(noise, other, p1, p2, synth.blob_sigma(P, self.blobiness), self.blob_porosity)
            out["blob_mask"], out["blob_other"] = mask.view(B, 1, P, P), other
        elif self.blobs:
            raise ValueError("this generator was constructed with blobs: make() needs draw()'s fifth element")
        if self.target_gen is not None:
            out["target"] = delta if self.target_gen == "4_points" else field            # transforms.py:628-633 / :635-685
        if image or self.corners:
            # corners in HomographyNetPrep's order (top-left, top-right, bottom-right, bottom-left; transforms.py:510-513)
            sq = torch.tensor([[0, 0], [P, 0], [P, P], [0, P]], dtype=torch.float32, device=self.device)
            out["corners"] = (origin[:, None, :] + sq).contiguous()
        if image:
            im = torch.empty(B, 1, self.h, self.w, dtype=torch.float32, device=self.device)
            check(lib.bh_synth_image(pv(images.data_ptr()), pv(idx.data_ptr()), pv(photo.data_ptr()) if photo is not None else None,
                                     B, images.shape[0], self.h, self.w, 0.443, 0.129, pv(im.data_ptr()),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "bh_synth_image")
            out["image_1"] = im
        return out

    def next(self, B, idx=None, image=None):
        return self.make(*self.draw(B, idx), image=image)        # (four or five draws: the fifth lands on `blobs`)

    def epoch(self, sampler):
        """One epoch of `sampler` (a `bihome_amd.bank.BankSampler`, or any iterable of index arrays): the batch of each of its index
        batches, in its order."""
        for batch in sampler:
            yield self.next(len(batch), idx=batch)
