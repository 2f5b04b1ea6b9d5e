"""The kwargs contract of the two shipped biHomE experiments this build covers.

Values (not text) of MODEL.BACKBONE / MODEL.HEAD / SOLVER from the reference's
config/s-coco/zeng-bihome-lr-1e-3.yaml and config/s-coco/detone-bihome-lr-5e-3.yaml; the reference
splats them as **kwargs into `Model.__init__` (train.py:679,690).  pds-coco differs only in the
data transform (photometric max_delta 32 instead of 0).
"""
import copy

ZENG_BIHOME = {
    "MODEL": {
        "BACKBONE": {
            "NAME": "Rethinking", "VARIANT": "DoubleLine", "IMAGE_SIZE": 128, "RESNET_BLOCK": "ResNet34",
            "PRETRAINED_RESNET": False,      # reference: True (ImageNet URL); no network here
            "IMAGE_KEY": ["image"], "PATCH_KEYS": ["patch_1", "patch_2"],
            "TARGET_KEYS": ["pf_hat_12", "pf_hat_21"],
        },
        "HEAD": {
            "NAME": "PerceptualHead", "PATCH_SIZE": 128, "PATCH_KEYS": ["patch_1", "patch_2"],
            "DELTA_HAT_KEYS": [], "PF_KEYS": ["pf_hat_12", "pf_hat_21"],
            "RANSAC_HYPOTHESIS_NO": 1, "POINTS_PER_HYPOTHESIS": 128,
            "AUXILIARY_RESNET": "resnet34", "AUXILIARY_RESNET_OUTPUT_LAYER": 1,
            "TRIPLET_LOSS": "double-line", "TRIPLET_AGGREGATION": "channel-agnostic",
            "TRIPLET_MARGIN": "inf", "TRIPLET_DISTANCE": "l1", "TRIPLET_MU": 0.01,
            "MASK_KEYS": [], "SAMPLING_STRATEGY": "downsample-mask",
        },
    },
    "SOLVER": {"OPTIMIZER": "Adam", "MOMENTUM_1": 0.9, "MOMENTUM_2": 0.999, "LR": 0.001,
               "MILESTONES": [30000, 60000, 90000], "LR_DECAY": 0.1, "LOSS": "biHomE"},
    "DATA": {"BATCH_SIZE": 64, "RHO": 32, "PATCH_SIZE": 128, "PHOTOMETRIC_MAX_DELTA": 0},
}

DETONE_BIHOME = {
    "MODEL": {
        "BACKBONE": {
            "NAME": "ResNet34", "VARIANT": "DoubleLine", "PRETRAINED_RESNET": False,
            "IMAGE_KEY": ["image"], "PATCH_KEYS": ["patch_1", "patch_2"],
            "TARGET_KEYS": ["delta_hat_12", "delta_hat_21"],
        },
        "HEAD": {
            "NAME": "PerceptualHead", "PATCH_SIZE": 128, "PATCH_KEYS": ["patch_1", "patch_2"],
            "DELTA_HAT_KEYS": ["delta_hat_12", "delta_hat_21"], "PF_KEYS": [],
            "RANSAC_HYPOTHESIS_NO": -1, "POINTS_PER_HYPOTHESIS": -1,
            "AUXILIARY_RESNET": "resnet34", "AUXILIARY_RESNET_OUTPUT_LAYER": 1,
            "TRIPLET_LOSS": "double-line", "TRIPLET_AGGREGATION": "channel-agnostic",
            "TRIPLET_MARGIN": "inf", "TRIPLET_DISTANCE": "l1", "TRIPLET_MU": 0.01,
            "MASK_KEYS": [], "SAMPLING_STRATEGY": "downsample-mask",
        },
    },
    "SOLVER": {"OPTIMIZER": "Adam", "MOMENTUM_1": 0.9, "MOMENTUM_2": 0.999, "LR": 0.005,
               "MILESTONES": [30000, 60000, 90000], "LR_DECAY": 0.1, "LOSS": "biHomE"},
    "DATA": {"BATCH_SIZE": 64, "RHO": 32, "PATCH_SIZE": 128, "PHOTOMETRIC_MAX_DELTA": 0},
}


# the supervised baselines of the same two backbones (config/s-coco/zeng-orig-lr-1e-3.yaml, detone-orig-lr-5e-3.yaml):
# one direction only (VARIANT OneLine), NoOpHead, a torch loss on (target, output) - train.py:318-322
ZENG_ORIG = {
    "MODEL": {
        "BACKBONE": {
            "NAME": "Rethinking", "VARIANT": "OneLine", "IMAGE_SIZE": 128, "RESNET_BLOCK": "ResNet34",
            "PRETRAINED_RESNET": False, "IMAGE_KEY": ["image"], "PATCH_KEYS": ["patch_1", "patch_2"],
            "TARGET_KEYS": ["pf_hat_12"],
        },
        "HEAD": {"NAME": "NoOpHead", "TARGET_GEN": "all_points",
                 "LEARNING_KEYS": ["target", "pf_hat_12", "delta", "pf_hat_12"]},
    },
    "SOLVER": {"OPTIMIZER": "Adam", "MOMENTUM_1": 0.9, "MOMENTUM_2": 0.999, "LR": 0.001,
               "MILESTONES": [30000, 60000, 90000], "LR_DECAY": 0.1, "LOSS": "SmoothL1Loss"},
    "DATA": {"BATCH_SIZE": 64, "RHO": 32, "PATCH_SIZE": 128, "PHOTOMETRIC_MAX_DELTA": 0, "TARGET_GEN": "all_points"},
}

DETONE_ORIG = {
    "MODEL": {
        "BACKBONE": {
            "NAME": "ResNet34", "VARIANT": "OneLine", "PRETRAINED_RESNET": False,
            "IMAGE_KEY": ["image"], "PATCH_KEYS": ["patch_1", "patch_2"], "TARGET_KEYS": ["delta_hat_12"],
        },
        "HEAD": {"NAME": "NoOpHead", "TARGET_GEN": "4_points",
                 "LEARNING_KEYS": ["delta", "delta_hat_12", "delta", "delta_hat_12"]},
    },
    "SOLVER": {"OPTIMIZER": "Adam", "MOMENTUM_1": 0.9, "MOMENTUM_2": 0.999, "LR": 0.005,
               "MILESTONES": [30000, 60000, 90000], "LR_DECAY": 0.1, "LOSS": "MSELoss"},
    "DATA": {"BATCH_SIZE": 64, "RHO": 32, "PATCH_SIZE": 128, "PHOTOMETRIC_MAX_DELTA": 0, "TARGET_GEN": "4_points"},
}


# Nguyen et al.'s unsupervised photometric baseline (config/s-coco/nguyen-orig-lr-5e-3.yaml): the DeTone regressor (OneLine) + the
# PhotometricHead, L1Loss between patch_2 and the crop of image_1 warped by the predicted homography.  The batch carries the whole
# grayscale, standardised image_1 and the patch corners as well (DATA IMAGE_KEYS: what batch producers emit on top of the patches).
NGUYEN_ORIG = {
    "MODEL": {
        "BACKBONE": {
            "NAME": "ResNet34", "VARIANT": "OneLine", "IMAGE_SIZE": 128, "PRETRAINED_RESNET": False,      # reference: True
            "IMAGE_KEY": ["image"], "PATCH_KEYS": ["patch_1", "patch_2"], "TARGET_KEYS": ["delta_hat_12"],
        },
        "HEAD": {"NAME": "PhotometricHead", "LEARNING_KEYS": ["patch_2", "image_1", "delta", "delta_hat_12"]},
    },
    "SOLVER": {"OPTIMIZER": "Adam", "MOMENTUM_1": 0.9, "MOMENTUM_2": 0.999, "LR": 0.005,
               "MILESTONES": [30000, 60000, 90000], "LR_DECAY": 0.1, "LOSS": "L1Loss"},
    "DATA": {"BATCH_SIZE": 64, "RHO": 32, "PATCH_SIZE": 128, "PHOTOMETRIC_MAX_DELTA": 0, "TARGET_GEN": "4_points",
             "IMAGE_KEYS": ["image_1"]},
}

# config/pds-coco/nguyen-orig-lr-5e-3.yaml is NOT the photometric head on distorted data: it is the supervised DeTone regressor
# (NoOpHead, '4_points') under L1Loss with photometric max_delta 32 - its own values, not the generic '-pds' rule applied to NGUYEN_ORIG
NGUYEN_ORIG_PDS = {
    "MODEL": {
        "BACKBONE": copy.deepcopy(NGUYEN_ORIG["MODEL"]["BACKBONE"]),
        "HEAD": {"NAME": "NoOpHead", "TARGET_GEN": "4_points",
                 "LEARNING_KEYS": ["delta", "delta_hat_12", "delta", "delta_hat_12"]},
    },
    "SOLVER": copy.deepcopy(NGUYEN_ORIG["SOLVER"]),
    # (TARGET_GEN as the yaml's HomographyNetPrep: the batch carries the 'all_points' target, which the '4_points' head does not read)
    "DATA": {"BATCH_SIZE": 64, "RHO": 32, "PATCH_SIZE": 128, "PHOTOMETRIC_MAX_DELTA": 32, "TARGET_GEN": "all_points"},
}


# Zhang et al. "Content-Aware" baselines (config/s-coco/zhang-orig-lr-1e-2.yaml: ContentAware backbone + TripletHead;
# zhang-bihome-lr-1e-2.yaml: the same backbone under the biHomE PerceptualHead with directly regressed offsets)
ZHANG_ORIG = {
    "MODEL": {
        "BACKBONE": {
            "NAME": "ContentAware", "VARIANT": "DoubleLine", "IMAGE_SIZE": 128, "PRETRAINED_RESNET": False,      # reference: True
            "IMAGE_KEY": ["image"], "PATCH_KEYS": ["patch_1", "patch_2"], "MASK_KEYS": ["mask_1", "mask_2"], "FIX_MASK": True,
            "FEATURE_KEYS": ["feature_1", "feature_2"], "TARGET_KEYS": ["delta_hat_12", "delta_hat_21"],
        },
        "HEAD": {
            "NAME": "TripletHead", "VARIANT": "DoubleLine", "PATCH_SIZE": 128, "PATCH_KEYS": ["patch_1", "patch_2"],
            "MASK_KEYS": ["mask_1", "mask_2"], "FEATURE_KEYS": ["feature_1", "feature_2"],
            "TARGET_KEYS": ["delta_hat_12", "delta_hat_21"], "LD": 2, "MU": 0.01, "TRIPLET_MARGIN": 1.0,
            "TRIPLET_AGGREGATION": "channel-agnostic",
        },
    },
    "SOLVER": {"OPTIMIZER": "Adam", "MOMENTUM_1": 0.9, "MOMENTUM_2": 0.999, "LR": 0.01,
               "MILESTONES": [30000, 60000, 90000], "LR_DECAY": 0.1, "LOSS": "TripletLoss"},
    "DATA": {"BATCH_SIZE": 64, "RHO": 32, "PATCH_SIZE": 128, "PHOTOMETRIC_MAX_DELTA": 0},
}
ZHANG_BIHOME = copy.deepcopy(ZHANG_ORIG)
ZHANG_BIHOME["MODEL"]["HEAD"] = copy.deepcopy(DETONE_BIHOME["MODEL"]["HEAD"])
ZHANG_BIHOME["SOLVER"]["LOSS"] = "biHomE"


def _ihome(base):
    """iHomE (one-line) variant of a biHomE config: one direction, hinge with a numeric margin (PerceptualHead.py:465-538).
    No yaml for it ships upstream (train.py:330 names the loss 'iHomE'); the kwargs follow the biHomE configs."""
    cfg = copy.deepcopy(base)
    cfg["MODEL"]["BACKBONE"]["VARIANT"] = "OneLine"
    cfg["MODEL"]["BACKBONE"]["TARGET_KEYS"] = cfg["MODEL"]["BACKBONE"]["TARGET_KEYS"][:1]
    h = cfg["MODEL"]["HEAD"]
    h["TRIPLET_LOSS"], h["TRIPLET_MARGIN"] = "one-line", 1.0
    h["DELTA_HAT_KEYS"], h["PF_KEYS"] = h["DELTA_HAT_KEYS"][:1], h["PF_KEYS"][:1]
    cfg["SOLVER"]["LOSS"] = "iHomE"
    return cfg


def _ihome_cos(base):
    """iHomE on cosine distances (PerceptualHead.py:485-499): `_ihome` with TRIPLET_DISTANCE 'cosine'.  No yaml for it ships upstream
    (the distance is one of the paper's ablation axes); the kwargs follow the biHomE configs."""
    cfg = _ihome(base)
    cfg["MODEL"]["HEAD"]["TRIPLET_DISTANCE"] = "cosine"
    return cfg


def _bihome_aware(base):
    """biHomE with the hinge inside the channel sum (PerceptualHead.py:624-625,644-645): TRIPLET_AGGREGATION 'channel-aware' and a
    numeric TRIPLET_MARGIN.  No yaml for it ships upstream (the aggregation and the margin are ablation axes of the paper); everything
    else as in the biHomE configs."""
    cfg = copy.deepcopy(base)
    cfg["MODEL"]["HEAD"].update(TRIPLET_AGGREGATION="channel-aware", TRIPLET_MARGIN=1.0)
    return cfg


def _multihead(base):
    """multihead_resnet_loss variant (PerceptualHead.py:230-235,245-315): TRIPLET_LOSS '' - the head returns the extractor
    features of patch_2 and of the warped patch_1 and the driver applies a torch loss to them (train.py:318-322).  No
    yaml for it ships upstream; one direction, kwargs as in the biHomE configs."""
    cfg = _ihome(base)
    cfg["MODEL"]["HEAD"]["TRIPLET_LOSS"] = ""
    cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = "inf"
    cfg["SOLVER"]["LOSS"] = "L1Loss"
    return cfg


def _proj(cfg):
    """A config with the trainable projection head on the perceptual features (WITH_PROJECTION_HEAD, PerceptualHead.py:41-48,69-74):
    64 -> 128 -> 64 on the layer-1 features.  No yaml for it ships upstream (the kwarg is read with a None default)."""
    cfg["MODEL"]["HEAD"]["WITH_PROJECTION_HEAD"] = [[64, 128], [128, 64]]
    return cfg


def get(name):
    """'zeng-bihome' / 'detone-bihome' = config/s-coco/*; the '-pds' variants = config/pds-coco/* (the two trees differ
    only in HomographyNetPrep's photometric max_delta, 0 vs 32, and the log dir).  'zeng-bihome-rgb256' is the
    build-side extension BASELINE.json configs[4] names (256x256 RGB patches, 6-channel stem; no upstream
    counterpart - SURVEY.md 0).  'nguyen-orig' = config/s-coco/nguyen-orig-lr-5e-3.yaml (PhotometricHead); 'nguyen-orig-pds' =
    config/pds-coco/nguyen-orig-lr-5e-3.yaml, which upstream made a different experiment (NoOpHead + L1Loss), not a data variant.
    '*-ihome', '*-multihead', '*-ihome-cos' and '*-bihome-aware' are loss-branch variants without a yaml upstream (see their builders);
    'zeng-ihome-proj', 'zeng-ihome-cos-proj' and 'detone-bihome-proj' add the trainable projection head to theirs (`_proj`).
    'zeng-bihome-pds-blobs' = 'zeng-bihome-pds' under CollatorWithBlobs (train.py:130-136,575-577) with the only values upstream shows
    (src/data/coco/dataset.py:442): DATA.AUGMENT_BLOB_POROSITY 0.1, AUGMENT_BLOBINESS 0.2."""
    if name == "zeng-bihome-pds-blobs":
        cfg = get("zeng-bihome-pds")
        cfg["DATA"].update(AUGMENT_BLOB_POROSITY=0.1, AUGMENT_BLOBINESS=0.2)
        return cfg
    if name in ("zeng-ihome-proj", "zeng-ihome-cos-proj", "detone-bihome-proj"):
        return _proj(get(name[:-5]))
    if name == "zeng-bihome-rgb256":
        cfg = copy.deepcopy(ZENG_BIHOME)
        cfg["MODEL"]["BACKBONE"].update(IMAGE_SIZE=256, PATCH_CHANNELS=3)
        cfg["MODEL"]["HEAD"].update(PATCH_SIZE=256)
        cfg["DATA"].update(BATCH_SIZE=32, RHO=64, PATCH_SIZE=256, PATCH_CHANNELS=3)
        return cfg
    if name in ("zeng-multihead", "detone-multihead"):
        return _multihead(ZENG_BIHOME if name == "zeng-multihead" else DETONE_BIHOME)
    if name in ("nguyen-orig", "nguyen-orig-pds"):
        return copy.deepcopy(NGUYEN_ORIG if name == "nguyen-orig" else NGUYEN_ORIG_PDS)
    if name in ("zeng-ihome", "detone-ihome"):
        return _ihome(ZENG_BIHOME if name == "zeng-ihome" else DETONE_BIHOME)
    if name in ("zeng-ihome-cos", "detone-ihome-cos"):
        return _ihome_cos(ZENG_BIHOME if name == "zeng-ihome-cos" else DETONE_BIHOME)
    if name in ("zeng-bihome-aware", "detone-bihome-aware"):
        return _bihome_aware(ZENG_BIHOME if name == "zeng-bihome-aware" else DETONE_BIHOME)
    base = name[:-4] if name.endswith("-pds") else name
    cfg = copy.deepcopy({"zeng-bihome": ZENG_BIHOME, "detone-bihome": DETONE_BIHOME, "zeng-orig": ZENG_ORIG,
                         "detone-orig": DETONE_ORIG, "zhang-orig": ZHANG_ORIG, "zhang-bihome": ZHANG_BIHOME}[base])
    if name.endswith("-pds"):
        cfg["DATA"]["PHOTOMETRIC_MAX_DELTA"] = 32
    return cfg
