"""Drop-in for the parts of DeepLabV3Plus-Pytorch/utils/ the embedding drivers use
(utils/__init__.py there re-exports loss, scheduler and the BN helpers)."""
from .loss import CrossEntropyLoss, CrossEntropyLoss_dis, DMLLoss, FocalLoss  # noqa: F401
from .scheduler import PolyLR  # noqa: F401
from .misc import set_bn_momentum, fix_bn, mkdir  # noqa: F401
from .scores import argmax_msp, dissum_score, novel_relabel, mean_prototype, extract_prototype  # noqa: F401
from .scores import open_world_post, novel_relabel_multi, extract_prototypes  # noqa: F401
from .scores import knn_cosine_score, dissum_msp_score, dense_crf_gauss  # noqa: F401
from .scores import rec_cosine_score, rec_confidence  # noqa: F401
from .scores import open_set_predict  # noqa: F401
from .scores import EcdfCalibrator, ecdf_certainty_score, fit_gmm_thresholds  # noqa: F401
from . import ext_transforms  # noqa: F401,E402
from .image_resize import pil_resize_normalize, segm_to_label  # noqa: F401,E402
