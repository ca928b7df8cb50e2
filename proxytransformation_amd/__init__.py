"""MI355X-native implementation of ProxyTransformation's point-cloud preshaping path.

Only what the path needs lives here:

* ``module.ProxyTransformationNormReverse`` -- the reference's registry entry / nn.Module
  surface (embodiedscan/models/necks/preshape_norm_reverse_drop.py:280-469);
* ``csrc/`` + ``libproxyt_hip.so``           -- hand-written HIP kernels for gfx950 behind
  the C ABI of ``include/proxyt.h`` (bound with ctypes in ``_abi``);
* ``backbone.MinkResNet``                    -- the sparse 3D backbone (backbones/mink_resnet.py) on the layers of ``sparse``;
* ``neck.MinkNeck``                          -- the sparse neck and head (necks/mink_neck.py), eval forward, on ``neck`` / ``sparse``;
* ``query_select.QuerySelect``               -- the detector's ``pre_decoder`` behind the neck: pad, text scores, sorted top-k, box decode;
* ``decoder.GroundingDecoder``               -- the transformer decoder behind it (self, text and scene attention, FFN, box refinement);
* ``grounding_loss.GroundingLoss``           -- the head's loss behind the decoder: 9-DoF box IoU, Hungarian match costs, focal and corner loss;
* ``detector.GroundingDetector``             -- all of the above as one module: ``loss`` and ``predict`` of the whole grounder;
* ``text_encoder.ClipTextEncoder``           -- the CLIP text encoder in front of it: token ids to ``last_hidden_state``;
* ``image_backbone.ResNet``                  -- the 2D image backbone in front of it (mmdet.ResNet, frozen): images to the feature levels;
* ``registry.MODELS``                        -- embodiedscan/mmengine registry or a stand-alone shim;
* ``shard``                                  -- scene sharding across the GPUs of one node;
* ``synth``                                  -- seeded synthetic scenes / closed-form weights.

Importing the package does not need a GPU and does not load the shared library;
``forward`` fails loudly when either is missing (there is no CPU fallback).
"""
from .registry import MODELS, REGISTRY_BACKEND
from .module import ProxyTransformationNormReverse
from .backbone import MinkResNet
from .neck import MinkNeck
from .query_select import QuerySelect
from .decoder import GroundingDecoder
from .grounding_loss import GroundingLoss
from .detector import GroundingDetector
from .text_encoder import ClipTextEncoder
from .image_backbone import ResNet

__all__ = ["MODELS", "REGISTRY_BACKEND", "ClipTextEncoder", "GroundingDecoder", "GroundingDetector", "GroundingLoss", "MinkNeck", "MinkResNet", "ProxyTransformationNormReverse", "QuerySelect", "ResNet"]
__version__ = "0.1.0"
