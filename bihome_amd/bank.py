"""A dataset of real images for the device pair generator: a uint8 bank resident in HBM, and the reference's epoch sampler.

The reference trains from one uint8 [240,320,3] RGB `.npy` per image (src/data/coco/dataset.py:95-103, written by
preprocess_offline.py:22) that CPU workers load sample by sample.  `ImageBank` keeps the whole split on the device as ONE uint8
[N,H,W,3] tensor (COCO train2014: 82,783 images, 19 GB - as float32 planes it would be 76 GB), and `gather` hands a batch's images to
the generator as the float planes [count,3,H,W] its kernels read (bh_bank_gather_u8).  `BankSampler` is the reference's
`DatasetSampler` (dataset.py:106-157): which image each sample of an epoch uses.

    bank = ImageBank.from_directory(cfg["DATA"]["DATASET_ROOT"])
    gen = GpuPairGenerator.from_config(cfg, bank=bank)
    s = cfg["DATA"]["SAMPLER"]
    for batch in gen.epoch(BankSampler(len(bank), 64, s["TRAIN_SAMPLES_PER_EPOCH"], seed=s["TRAIN_SEED"])): ..."""
import os

import numpy as np
import torch

from . import kernels as K

UPLOAD_CHUNK_BYTES = 64 << 20        # from_directory: host staging per upload (the host never holds a second copy of the bank)


def _check_images(shape, dtype, what):
    """uint8 [N,H,W,3] with N, H, W >= 1, or a ValueError naming `what`."""
    if not (dtype is torch.uint8 if isinstance(dtype, torch.dtype) else dtype == np.uint8):
        raise ValueError("%s: an image bank is uint8 (values 0..255), got %s" % (what, dtype))
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError("%s: an image bank is [N,H,W,3] interleaved RGB, got %s" % (what, tuple(shape)))
    if min(shape) < 1:
        raise ValueError("%s: an image bank needs at least one image of at least one pixel, got %s" % (what, tuple(shape)))


class ImageBank:
    """One contiguous uint8 [N,H,W,3] tensor on `device` (`.data`); `len(bank)`, `.h`, `.w`, `.nbytes`."""

    def __init__(self, images, device="cuda"):
        # (every check before the tensor goes to the device: refusals need no GPU)
        if isinstance(images, torch.Tensor):
            _check_images(images.shape, images.dtype, "ImageBank")
        else:
            images = np.asarray(images)
            _check_images(images.shape, images.dtype, "ImageBank")
            images = torch.from_numpy(np.ascontiguousarray(images))
        self.data = images.to(device).contiguous()
        self._stage = None

    @classmethod
    def from_directory(cls, root, max_images=None, device="cuda"):
        """Every `*.npy` of `root` (uint8 [H,W,3] RGB, one common size: what upstream's preprocess_offline.py writes), the first
        `max_images` of them if given, in SORTED file-name order: image k of the bank is the k-th name.  Upstream indexes its files in
        os.listdir order (dataset.py:32), which depends on the file system and is not reproducible across machines; sorted order is.
        A file of another dtype, rank, channel count or size is refused with a ValueError that names it.  `.jpg` files are refused:
        there is no decoder (nor upstream's Rescale / CenterCrop) here - run upstream's preprocess_offline.py first.  The files are
        uploaded in chunks of UPLOAD_CHUNK_BYTES, so the host never holds a second full copy."""
        names = sorted(os.listdir(root))
        jpg = [f for f in names if f.lower().endswith((".jpg", ".jpeg"))]
        if jpg:
            raise ValueError("%s: there is no JPEG decoder here - convert the dataset with upstream's preprocess_offline.py (uint8 "
                             "[H,W,3] .npy files) first" % os.path.join(root, jpg[0]))
        names = [f for f in names if f.endswith(".npy")]
        if max_images is not None:
            names = names[:max_images]
        if not names:
            raise ValueError("%s: no .npy files" % root)
        data, size, chunk, start = None, None, [], 0
        for k, name in enumerate(names):
            path = os.path.join(root, name)
            a = np.load(path, allow_pickle=False)
            if a.dtype != np.uint8:
                raise ValueError("%s: dtype %s, an image bank takes uint8" % (path, a.dtype))
            if a.ndim != 3:
                raise ValueError("%s: shape %s, an image bank takes [H,W,3]" % (path, a.shape))
            if a.shape[2] != 3:
                raise ValueError("%s: %d channels, an image bank takes 3 (RGB)" % (path, a.shape[2]))
            if a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError("%s: empty image %s" % (path, a.shape))
            if size is None:
                size = a.shape
                data = torch.empty((len(names),) + size, dtype=torch.uint8, device=device)
                per_chunk = max(1, UPLOAD_CHUNK_BYTES // a.nbytes)
            elif a.shape != size:
                raise ValueError("%s: size %s, the images before it are %s (one bank holds one size)" % (path, a.shape[:2], size[:2]))
            chunk.append(a)
            if len(chunk) == per_chunk or k == len(names) - 1:
                data[start:start + len(chunk)].copy_(torch.from_numpy(np.stack(chunk)))
                start, chunk = start + len(chunk), []
        return cls(data, device=device)

    def __len__(self):
        return self.data.shape[0]

    @property
    def h(self):
        return self.data.shape[1]

    @property
    def w(self):
        return self.data.shape[2]

    @property
    def nbytes(self):
        return self.data.numel()

    def gather(self, idx, out=None):
        """Images idx [count] (int32 device tensor) as float planes [count,3,h,w], values 0..255 - the `images` layout of the
        generator's kernels.  out: the buffer to fill; None: the bank's own staging buffer, reused while `count` stays the same (its
        content lasts until the next gather)."""
        shape = (idx.shape[0], 3, self.h, self.w)
        if out is None:
            if self._stage is None or tuple(self._stage.shape) != shape:
                self._stage = torch.empty(shape, dtype=torch.float32, device=self.data.device)
            out = self._stage
        return K.bank_gather_u8(self.data, idx, out)


class BankSampler:
    """The reference's DatasetSampler (dataset.py:106-157).  Every `__iter__` draws a new epoch, `choice(np.arange(n_images),
    samples_per_epoch)` (with replacement), from ONE RandomState(seed) that continues from epoch to epoch (:133-139) - with seed=None
    from the global np.random (:141-142) - and yields consecutive int64 index arrays of `batch_size`; a trailing partial batch is
    dropped (:153-157).  `len()` is the number of batches of an epoch (:145)."""

    def __init__(self, n_images, batch_size, samples_per_epoch, seed=None):
        if n_images < 1 or batch_size < 1 or samples_per_epoch < 0:
            raise ValueError("BankSampler: n_images >= 1, batch_size >= 1, samples_per_epoch >= 0")
        self.n_images, self.batch_size, self.samples_per_epoch, self.seed = n_images, batch_size, samples_per_epoch, seed
        self.random_state = np.random.RandomState(seed) if seed is not None else None

    def __len__(self):
        return self.samples_per_epoch // self.batch_size

    def __iter__(self):
        rs = self.random_state if self.random_state is not None else np.random
        order = rs.choice(np.arange(self.n_images), self.samples_per_epoch)
        for i in range(len(self)):
            yield order[i * self.batch_size:(i + 1) * self.batch_size]
