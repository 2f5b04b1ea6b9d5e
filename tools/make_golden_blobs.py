"""Write tests/golden/collator_blobs_b4.npz: the REFERENCE's own CollatorWithBlobs (src/data/transforms.py:746-799) on a B = 4 batch of
32x32 patches, once grayscale (C = 1) and once RGB (C = 3).  Runs only where the reference tree exists (never on the GPU box).

    python tools/make_golden_blobs.py

Upstream the collator cannot run: its `import porespy as ps` is commented out (transforms.py:3).  This tool imports the reference's
module unchanged (with the cv2 stand-in of oracle/refshim that the other fixtures use) and sets `transforms.ps` to a stand-in whose
`generators.blobs(shape, porosity, blobiness)` is porespy's algorithm as recalled (bihome_amd/synth.py blob_field states it), written
independently of that restatement with scipy.ndimage.gaussian_filter / scipy.special.erfc, on noise that the tool draws and records
(float32 values, so that the device kernel can be given exactly the same numbers).  The source indices the collator draws are logged
through its `rand_choice_fn`.

Recorded per case c1 / c3 (numeric arrays only): patch_1, patch_2 (the inputs: synth.make_pairs), noise [4,32,32] float32, mask
[4,32,32] uint8 (what the stand-in returned), other [4], out [4,C,32,32] (the collated patch_2), and porosity / blobiness."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import REF, install_standins  # noqa: E402

POROSITY, BLOBINESS = 0.3, 0.5
BATCH, PATCH = 4, 32
SEEDS = {1: (31, 7, 101), 3: (32, 8, 102)}            # C -> (make_pairs seed, collator random_seed, noise seed)


class BlobsStandin:
    """`ps.generators.blobs`: every call draws its noise from `rs` and keeps (noise, mask)."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.calls = []

    def blobs(self, shape, porosity, blobiness):
        from scipy.ndimage import gaussian_filter
        from scipy.special import erfc
        noise = self.rs.rand(*shape).astype(np.float32)
        sigma = np.mean(shape) / (40 * blobiness)
        g = gaussian_filter(noise.astype(np.float64), sigma=sigma)
        z = (g - g.mean()) / g.std()
        u = 0.5 * erfc(-z / np.sqrt(2))
        u = (u - u.min()) / (u.max() - u.min())
        mask = u < porosity
        self.calls.append((noise, mask))
        return mask


def run(transforms, channels):
    from bihome_amd import synth
    seed, collator_seed, noise_seed = SEEDS[channels]
    d = synth.make_pairs(BATCH, patch=PATCH, seed=seed, channels=channels)
    standin = BlobsStandin(noise_seed)
    transforms.ps = types.SimpleNamespace(generators=standin)
    collator = transforms.CollatorWithBlobs("patch_1", "patch_2", POROSITY, BLOBINESS, random_seed=collator_seed)
    drawn, choice = [], collator.rand_choice_fn

    def logged(a, size):
        r = choice(a, size)
        drawn.append(int(r[0]))
        return r
    collator.rand_choice_fn = logged
    batch = [{"patch_1": torch.from_numpy(d["patch_1"][b].copy()), "patch_2": torch.from_numpy(d["patch_2"][b].copy())}
             for b in range(BATCH)]
    out = collator(batch)
    assert len(drawn) == BATCH == len(standin.calls) and all(o != b for b, o in enumerate(drawn))
    assert torch.equal(out["patch_1"], torch.from_numpy(d["patch_1"]))            # upstream changes only the patch_2 key
    tag = "c%d_" % channels
    return {tag + "patch_1": d["patch_1"], tag + "patch_2": d["patch_2"],
            tag + "noise": np.stack([n for n, _ in standin.calls]), tag + "mask": np.stack([m for _, m in standin.calls]).astype(np.uint8),
            tag + "other": np.array(drawn, np.int64), tag + "out": out["patch_2"].numpy().copy()}


def main():
    install_standins()
    import importlib
    transforms = importlib.import_module("src.data.transforms")
    assert os.path.realpath(transforms.__file__).startswith(os.path.realpath(REF)), transforms.__file__
    rec = {"porosity": np.float64(POROSITY), "blobiness": np.float64(BLOBINESS)}
    for channels in (1, 3):
        r = run(transforms, channels)
        rec.update(r)
        tag = "c%d_" % channels
        print("C = %d: other %s, blob share per sample %s" % (channels, r[tag + "other"].tolist(),
                                                               r[tag + "mask"].reshape(BATCH, -1).mean(1).round(3).tolist()))
    path = os.path.join(ROOT, "tests", "golden", "collator_blobs_b4.npz")
    np.savez_compressed(path, **rec)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
