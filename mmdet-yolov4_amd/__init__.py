"""MI355X-native YOLOv4 hot path behind the mmdet-yolov4 registry surface.

Importing the package registers ``DarknetCSP``, ``YOLOV4Neck``/``YOLOV5Neck``,
``YOLOCSPHead``, ``SingleStageDetector``, ``YOLOV4AnchorGenerator``,
``YOLOV4BBoxCoder`` and the ``Mish`` activation under the reference's names.  Numbers
come from ``lib/libyv4_hip.so`` (C-ABI: ``include/yv4.h``); there is no CPU fallback.
"""
from . import _lib
from .registry import (ACTIVATION_LAYERS, ANCHOR_GENERATORS, BACKBONES, BBOX_CODERS, DATASETS, DETECTORS, HEADS, LOSSES,
                       MODELS, NECKS, PIPELINES, Config, ConfigDict, Registry, build_anchor_generator, build_backbone,
                       build_bbox_coder, build_detector, build_from_cfg, build_head, build_neck)
from .bricks import Mish, build_activation_layer, build_norm_layer, wrap_fp16_model
from .ops import (MishFunction, batched_nms, get_nms_iou_form, mish_backward, mish_forward, multiclass_nms, nms,
                  set_nms_iou_form, set_deterministic, deterministic, soft_nms)
from .anchor_generator import YOLOAnchorGenerator, YOLOV4AnchorGenerator
from .bbox_coder import YOLOV4BBoxCoder
from .darknetcsp import (Bottleneck, BottleneckCSP, BottleneckCSP2, Conv, CSPStage, DarknetCSP, Focus, SPPV4,
                         SPPV4Stage, SPPV5, SPPV5Stage, BottleneckStage)
from .yolo_neck_csp import YOLOV4Neck, YOLOV5Neck
from .yolocsp_head import YOLOCSPHead
from .single_stage import SingleStageDetector, bbox2result
from .yolov3 import Darknet, DetectionBlock, ResBlock, YOLOBBoxCoder, YOLOV3, YOLOV3Head, YOLOV3Neck
from .plan import Plan
from .preprocess import FusedTestPipeline
from .image_io import LoadImageFromFile, encode_into, imdecode, imencode, imread, imwrite, set_default_entropy
from .augment import FusedTrainPipeline
from .augment_v3 import FusedV3TrainPipeline, build_train_pipeline
from . import tta  # noqa: F401  (YOLOv3 test-time augmentation)
from .apis import (get_root_logger, inference_detector, init_detector, multi_gpu_test, set_random_seed, single_gpu_test,
                   train_detector)
from .draw import color_val, draw_boxes, draw_boxes_into, imshow_gt_det_bboxes
from .eval_utils import (coco_test_annotation, evaluate_fast_bbox, FlexGt, EVAL_BREAKDOWN, EVAL_IOU_CALCULATOR, EVAL_MATCHER, FlexibleStatisticsEval, IOU2DCoCo,
                         MatcherCoCo, ScaleBreakdown, average_precision, eval_map_flexible, iou_coco, match_coco)
from .map_eval import (MapGt, bbox_overlaps, eval_map, evaluate_map, print_map_summary, tpfp_default,  # noqa: F401
                       tpfp_imagenet)
from .recall_eval import RecallGt, eval_recalls, print_recall_summary, recall_device, set_recall_param  # noqa: F401
from .coco_eval import COCOeval, CocoGt, evaluate_bbox, flatten_results  # noqa: F401
from .coco_error import ErrorAnalysis, error_analysis  # noqa: F401
from .results import CocoBBoxDataset, CustomBBoxDataset, DeviceResults  # noqa: F401
from .analysis import ResultVisualizer, bbox_map_eval, image_maps  # noqa: F401
from .datasets import (CocoDataset, DistributedGroupSampler, GroupSampler, TestLoader, TrainLoader,  # noqa: F401
                       build_dataset, build_test_loader, build_train_loader)
from .augment_plain import PlainTrainPipeline  # noqa: F401
from .custom_datasets import (CustomDataset, GarbageDataset, TrafficSignDataset, VOCDataset,  # noqa: F401
                              XMLDataset)
from .dataset_wrappers import ClassBalancedDataset, ConcatDataset, RepeatDataset  # noqa: F401

from .hooks import (EpochBasedRunner, IterTimerHook, StepLrUpdaterHook, TextLoggerHook, build_runner)  # noqa: F401

__version__ = '1.0.0'          # written into every checkpoint's meta by tools/train.py

__all__ = [n for n in dir() if not n.startswith('_')]
