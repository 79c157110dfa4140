"""lead-yolo_amd: MI355X-native (gfx950 HIP) implementation of the LEAD-YOLO detector hot path.

Import name: `lead_yolo_amd` (the directory name carries a hyphen; see ../lead_yolo_amd/__init__.py)."""
from . import capi, ops, pack  # noqa: F401
from .modules import *  # noqa: F401,F403
from .modules import Lazy  # noqa: F401
from .model import DEFAULT_CFG, DetectionModel, Model, load_cfg, make_divisible, parse_model  # noqa: F401
from .loss import ComputeLoss  # noqa: F401
from .ddp import GradReducer  # noqa: F401
from .train import (GraphedTrainStep, ModelEMA, MultiScaleTrainStep, forward_backward, freeze_layers, multi_scale_shape, multi_scale_size,  # noqa: F401
                    optimizer_step, smart_optimizer, train_step)
from .optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: F401
from .graph import GraphedForward  # noqa: F401
from .nms import nms_padded, non_max_suppression  # noqa: F401,E402
from .mosaic import ImageBank, MosaicAugment  # noqa: F401,E402
from .metrics import ConfusionMatrix, MatchAccumulator, Validator, ValResult, ap_per_class, compute_ap, match_padded, unpack_correct  # noqa: F401,E402
from .predict import Detector, LetterboxPlan, letterbox, letterbox_plan, load_image_size, scale_boxes  # noqa: F401,E402
from .valrun import ValPlan, ValRun, ValSet, val_labels, val_plan, validate  # noqa: F401,E402
from .anchors import AnchorCheck, anchor_metric, check_anchors, evolve, kmean_anchors, kmeans, label_wh, mutation_table  # noqa: F401,E402
from .scene import SceneDetector, scene_collect, scene_merge, scene_plan, scene_tiles  # noqa: F401,E402
