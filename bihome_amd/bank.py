"""A dataset of real images for the device pair generator: a uint8 bank resident in HBM, and the reference's epoch sampler.

The reference trains from one uint8 [240,320,3] RGB `.npy` per image (src/data/coco/dataset.py:95-103, written by
preprocess_offline.py:22) that CPU workers load sample by sample.  `ImageBank` keeps the whole split on the device as ONE uint8
[N,H,W,3] tensor (COCO train2014: 82,783 images, 19 GB - as float32 planes it would be 76 GB), and `gather` hands a batch's images to
the generator as the float planes [count,3,H,W] its kernels read (bh_bank_gather_u8).  `BankSampler` is the reference's
`DatasetSampler` (dataset.py:106-157): which image each sample of an epoch uses.

    bank = ImageBank.from_directory(cfg["DATA"]["DATASET_ROOT"])                    # preprocess_offline.py's .npy files, or the raw
    bank = ImageBank.from_directory(raw_root, size=(320, 240))                      # dataset: Rescale + CenterCrop on the device
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


# ------------------------------------------------------------------------------------------------
# raw-size images: upstream's Rescale + CenterCrop, stated on the host (the kernel bh_bank_ingest_u8 is held to this bit for bit)
# ------------------------------------------------------------------------------------------------
IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png")       # decoded with PIL where it is importable (from_directory with size=)


def _check_size(size):
    """size = (W, H), upstream's (width, height) order, both integers >= 1."""
    try:
        W, H = size
        ok = int(W) == W and int(H) == H and W >= 1 and H >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("size is (width, height), two integers >= 1, got %r" % (size,))
    return int(W), int(H)


def _check_image(a, what):
    """uint8 [h,w,3] with h, w >= 1, or a ValueError naming `what`."""
    if a.dtype != np.uint8:
        raise ValueError("%s: dtype %s, an image bank takes uint8" % (what, a.dtype))
    if a.ndim != 3:
        raise ValueError("%s: shape %s, an image bank takes [H,W,3]" % (what, a.shape))
    if a.shape[2] != 3:
        raise ValueError("%s: %d channels, an image bank takes 3 (RGB)" % (what, a.shape[2]))
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("%s: empty image %s" % (what, a.shape))


def rescale_size(h, w, size):
    """(nh, nw, top, left): the size upstream's Rescale(size) gives an h x w image (src/data/transforms.py:36-41, tuple target
    size = (W, H), in double, numpy's round half to even) and the window CenterCrop(size) then takes from it (:108-118)."""
    W, H = _check_size(size)
    if h < 1 or w < 1:
        raise ValueError("rescale_size: an image has at least one pixel, got %d x %d" % (h, w))
    r = h / w
    if r < H / W:
        nw, nh = int(np.round(H / r)), H
    else:
        nw, nh = W, int(np.round(W * r))
    top = (nh - H) // 2 if nh != H else 0
    left = (nw - W) // 2 if nw != W else 0
    return nh, nw, top, left


def _taps(d, n, n_new):
    """cv2.resize's INTER_LINEAR taps for positions d (int array) of an axis resized from n to n_new, as recalled: the two source
    indices (the second equal to the first at the far edge, where its coefficient is 0) and the 11-bit coefficients as int32."""
    f = ((d.astype(np.float64) + 0.5) * (n / n_new) - 0.5).astype(np.float32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = f - fl
    low, high = s < 0, s >= n - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = n - 1, 0
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int16).astype(np.int32)
    c1 = np.rint(f * np.float32(2048)).astype(np.int16).astype(np.int32)
    return s, np.minimum(s + 1, n - 1), c0, c1


def rescale_center_crop_host(image, size):
    """Upstream's Rescale(size) then CenterCrop(size) (transforms.py:24-46, 103-122; preprocess_offline.py) of one uint8 [h,w,3] image,
    size = (W, H): uint8 [H,W,3].  Only the cropped window of the resized image is computed.  The resize is cv2.resize's default
    (INTER_LINEAR on 8-bit data) AS RECALLED - there is no cv2 to compare with, and OpenCV's source was not read: exact halving of both
    axes is the rounded mean of each 2x2 block, the same size a copy, anything else two taps per axis with coefficients rounded to 11
    bits and OpenCV's shifts, in integers (include/bihome.h bh_bank_ingest_u8 has the formulas).  This is the arithmetic of a bank built
    on device="cpu" and the reference bh_bank_ingest_u8 equals bit for bit."""
    image = np.asarray(image)
    _check_image(image, "rescale_center_crop_host")
    W, H = _check_size(size)
    h, w = image.shape[:2]
    nh, nw, top, left = rescale_size(h, w, (W, H))
    ys, xs = np.arange(H) + top, np.arange(W) + left
    if (nh, nw) == (h, w):
        return np.ascontiguousarray(image[top:top + H, left:left + W])
    s = image.astype(np.int32)
    if w == 2 * nw and h == 2 * nh:
        r0, r1 = s[2 * ys], s[2 * ys + 1]
        return np.ascontiguousarray(((r0[:, 2 * xs] + r0[:, 2 * xs + 1] + r1[:, 2 * xs] + r1[:, 2 * xs + 1] + 2) >> 2).astype(np.uint8))
    y0, y1, b0, b1 = _taps(ys, h, nh)
    x0, x1, a0, a1 = _taps(xs, w, nw)
    a0, a1, b0, b1 = a0[None, :, None], a1[None, :, None], b0[:, None, None], b1[:, None, None]
    S0 = s[y0][:, x0] * a0 + s[y0][:, x1] * a1
    S1 = s[y1][:, x0] * a0 + s[y1][:, x1] * a1
    return np.ascontiguousarray(((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8))


def _pil():
    """PIL.Image, or None where PIL cannot be imported."""
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


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
    def _ingest(cls, n, items, size, device):
        """The bank of `n` raw-size images, each rescaled and centre-cropped to size = (W, H).  items yields (what, uint8 [h,w,3] array)
        n times, `what` naming the image in a refusal.  The images are packed into one host staging buffer of UPLOAD_CHUNK_BYTES (an
        image larger than that travels alone); a full buffer is uploaded and ingested into its slots with ONE bh_bank_ingest_u8 launch,
        so the host holds one chunk and the device the bank plus one chunk.  On a CPU device rescale_center_crop_host fills the slots."""
        W, H = _check_size(size)
        data = torch.empty((n, H, W, 3), dtype=torch.uint8, device=device)
        on_host = data.device.type == "cpu"
        stage = np.empty(UPLOAD_CHUNK_BYTES, np.uint8)
        state = dict(start=0, fill=0, off=[], hw=[])

        def flush(buf):
            if not state["off"]:
                return
            if on_host:
                for k, (o, (h, w)) in enumerate(zip(state["off"], state["hw"])):
                    data[state["start"] + k] = torch.from_numpy(rescale_center_crop_host(buf[o:o + h * w * 3].reshape(h, w, 3), (W, H)))
            else:
                src = torch.from_numpy(buf[:state["fill"]]).to(data.device)          # (a pageable copy: done when .to returns)
                K.bank_ingest_u8(src, np.asarray(state["off"], np.int64), np.asarray(state["hw"], np.int32).reshape(-1, 2), data,
                                 state["start"])
            state.update(start=state["start"] + len(state["off"]), fill=0, off=[], hw=[])

        for what, a in items:
            _check_image(a, what)
            if state["fill"] + a.nbytes > stage.size:
                flush(stage)
            buf = stage if a.nbytes <= stage.size else np.empty(a.nbytes, np.uint8)      # an image larger than a chunk: one of its own
            at = state["fill"] if buf is stage else 0
            buf[at:at + a.nbytes].reshape(a.shape)[...] = a
            state["off"].append(at)
            state["hw"].append(a.shape[:2])
            state["fill"] += a.nbytes
            if buf is not stage:
                flush(buf)
        flush(stage)
        assert state["start"] == n
        return cls(data, device=device)

    @classmethod
    def from_images(cls, images, size, device="cuda"):
        """A list of uint8 [h,w,3] RGB arrays of ANY sizes as a bank of size = (W, H) images (upstream's (width, height) order): each
        goes through upstream's Rescale(size) and CenterCrop(size) (src/data/transforms.py:24-46, 103-122) on the device
        (bh_bank_ingest_u8, one launch per UPLOAD_CHUNK_BYTES of source pixels), on device="cpu" through rescale_center_crop_host, which
        the kernel equals bit for bit.  Image k of the bank is images[k].  A ValueError names the index of an array of another dtype,
        rank or channel count, or without pixels."""
        _check_size(size)
        images = [np.asarray(a) for a in images]
        if not images:
            raise ValueError("from_images: no images")
        for k, a in enumerate(images):                                               # (every refusal before any device work)
            _check_image(a, "from_images: image %d" % k)
        return cls._ingest(len(images), (("from_images: image %d" % k, a) for k, a in enumerate(images)), size, device)

    @classmethod
    def _from_raw_directory(cls, root, max_images, device, size):
        """from_directory with size=: see there."""
        _check_size(size)
        names = [f for f in sorted(os.listdir(root)) if f.endswith(".npy") or f.lower().endswith(IMAGE_SUFFIXES)]
        if max_images is not None:
            names = names[:max_images]
        if not names:
            raise ValueError("%s: no .npy, .jpg, .jpeg or .png files" % root)
        coded = [f for f in names if not f.endswith(".npy")]
        Image = _pil() if coded else None
        if coded and Image is None:
            raise ValueError("%s: no decoder is available for .jpg / .jpeg / .png files (PIL cannot be imported) - install Pillow, or "
                             "convert the images to uint8 [h,w,3] .npy files" % os.path.join(root, coded[0]))

        def items():
            for name in names:
                path = os.path.join(root, name)
                if name.endswith(".npy"):
                    yield path, np.load(path, allow_pickle=False)
                else:
                    try:
                        with Image.open(path) as im:
                            a = np.asarray(im.convert("RGB"))
                    except (OSError, SyntaxError) as e:
                        raise ValueError("%s: cannot be decoded (%s)" % (path, e)) from e
                    yield path, a
        return cls._ingest(len(names), items(), size, device)

    @classmethod
    def from_directory(cls, root, max_images=None, device="cuda", size=None):
        """size=None: every `*.npy` of `root` (uint8 [H,W,3] RGB, one common size: what upstream's preprocess_offline.py writes), the first
        `max_images` of them if given, in SORTED file-name order: image k of the bank is the k-th name.  Upstream indexes its files in
        os.listdir order (dataset.py:32), which depends on the file system and is not reproducible across machines; sorted order is.
        A file of another dtype, rank, channel count or size is refused with a ValueError that names it.  `.jpg` files are refused:
        without a size there is no Rescale / CenterCrop to bring them to one - pass size=, or run upstream's preprocess_offline.py first.
        The files are uploaded in chunks of UPLOAD_CHUNK_BYTES, so the host never holds a second full copy.

        size=(W, H) (upstream's (width, height) order, e.g. (320, 240) for COCO, (320, 256) for FLIR ADAS, (192, 192) for CIFAR): the
        raw dataset.  `.npy` files of ANY [h,w,3] uint8 size and - where PIL can be imported - `.jpg`, `.jpeg` and `.png` files
        (`Image.open(path).convert("RGB")`), mixed freely and taken in sorted name order, each brought to H x W by upstream's
        Rescale(size) + CenterCrop(size) on the device (see from_images: this is that function plus file reading, one chunk of
        UPLOAD_CHUNK_BYTES on the host at a time).  Without PIL a ValueError names the first such file.  PIL's JPEG decoder need not
        match cv2.imread's byte for byte (they may differ in the inverse DCT and the chroma upsampling), so a bank built from `.jpg`
        files is not promised to equal upstream's `.npy` files; from decoded pixels on, the arithmetic is the one stated in
        rescale_center_crop_host."""
        if size is not None:
            return cls._from_raw_directory(root, max_images, device, size)
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
