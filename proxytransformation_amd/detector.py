"""``GroundingDetector``: ``SparseFeatureFusion3DGrounderPreshape`` (detectors/sparse_featfusion_grounder_preshape.py, DET) behind the 2D
backbone and the text encoder, as one module -- the stages of this package called together:

    text_feat_map                                   DET:659        decoder.linear
    preshape -> quantize                            DET:385-397    module.ProxyTransformationNormReverse
    backbone_3d                                     DET:398        backbone.MinkResNet (its levels carry the coordinates)
    sample + concatenate, per level                 DET:428-479    fusion.join_level_features (one launch per level)
    neck_3d                                         DET:482        neck.MinkNeck
    pre_decoder                                     DET:498-580    query_select.QuerySelect
    decoder (after the renaming of DET:605-617)     DET:582-621    decoder.GroundingDecoder
    bbox_head: scores, loss / predict               DET:700, 787   GroundingDecoder.head_scores, grounding_loss.GroundingLoss

By default the 2D backbone and the text encoder stay outside: the detector takes their outputs (``img_features``: one
``(B,V,C_l,H_l,W_l)`` per level; ``encoded_text (B,T,text_width)`` with ``text_token_mask``).  With ``text_encoder=`` (a
``text_encoder.ClipTextEncoder`` or its keywords) the detector holds the encoder and ``loss`` / ``predict`` / ``forward`` take
``input_ids=`` and ``attention_mask=`` in place of the encoded text (DET:661-668, 740-753 behind the tokenizer).  With ``backbone=`` (an
``image_backbone.ResNet`` or its config dict) it holds the 2D backbone (DET:357-379) and the same methods take ``imgs=``
``(B,V,3,H,W)`` in place of ``img_features``.
``share_pred_layer=True`` is the shipped head: ONE classification and ONE regression branch (``self.query_select``) serve the query
selection, every decoder layer and the scores."""
from __future__ import annotations

import inspect
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from ._doors import _np
from .backbone import MinkResNet, SparseLevel
from .decoder import GroundingDecoder, linear
from .fusion import JoinTables, image_transform_scalars, join_level_features, join_level_features_per_scene, prepare_features_many, reverse_3d_flow
from .grounding_loss import GroundingLoss
from .image_backbone import ResNet
from .module import ProxyTransformationNormReverse
from .neck import MinkNeck
from .query_select import QuerySelect
from .registry import MODELS
from .text_encoder import ClipTextEncoder

__all__ = ["GroundingDetector"]

#: the prefixes of a reference checkpoint that belong to modules outside this one: skipped by ``load_reference_state_dict``
#: (each only while the detector does not hold that module)
_OUTSIDE = ("backbone.", "text_encoder.")
_TEXT = "text_encoder."
_IMAGE = "backbone."


def _build(who: str, name: str, cfg, cls, differentiable: bool):
    """A child from its config dict (through ``MODELS`` when it names a type, else ``cls``) with ``differentiable`` forwarded where the
    class takes it; a ready module passes through."""
    if isinstance(cfg, nn.Module):
        return cfg
    if not isinstance(cfg, dict):
        raise TypeError(f"{who}: {name} must be a config dict or a module, got {type(cfg).__name__}")
    cfg = dict(cfg)
    kind = cfg.pop("type", None)
    target = cls if kind is None or kind == cls.__name__ else MODELS.get(kind)
    if target is None:
        raise ValueError(f"{who}: {name}: type {kind!r} is not registered")
    if "differentiable" in inspect.signature(target.__init__).parameters:
        cfg.setdefault("differentiable", bool(differentiable))
    return target(**cfg)


class GroundingDetector(nn.Module):
    """``GroundingDetector(preshape, backbone_3d, neck_3d, decoder, bbox_head, num_queries=256, voxel_size=0.01, use_xyz_feat=True,
    coord_type='DEPTH', train_cfg=None, test_cfg=None, text_width=768, *, differentiable=False, matcher='host', fused_join=True,
    text_encoder=None, backbone=None, pixel_mean=None, pixel_std=None, bgr_to_rgb=False)``:
    the reference's keywords (configs/grounding/*.py, ``model=``), each child a config dict or a ready module.  ``bbox_head`` is the
    ``GroundingHead`` config: it becomes ``self.bbox_head`` (``GroundingLoss``: loss and predict, no parameters) and ``self.query_select``
    (``QuerySelect``: the shared branches).  ``text_width``: the text encoder's hidden size, ``text_feat_map = nn.Linear(text_width,
    embed_dims)``.  ``text_encoder``: None (the default: the module, its ``state_dict`` and its methods are what they were), a
    ``ClipTextEncoder`` or its keyword dict; ``text_width`` then defaults to its ``hidden_size`` and must equal it.  The encoder is never
    trained (``lr_mult=0.0`` in the reference): it runs under ``no_grad`` and its parameters receive no gradient.  ``backbone``: None
    (the default: the module, its ``state_dict`` and its methods are what they were), an ``image_backbone.ResNet`` or its config dict
    (``type='mmdet.ResNet'``); ``pixel_mean`` / ``pixel_std`` / ``bgr_to_rgb``: the data preprocessor's values, applied by the backbone's
    stem.  The detector's own ``differentiable=`` is NOT forwarded to the backbone: a backbone built from a plain config is
    inference-only, the loss's backward stops at its output and its parameters get no gradient.  Training it, as the reference does
    for the convolutions of stages 2 to 4 (``frozen_stages=1``), is asked for with ``backbone=dict(..., differentiable=True)`` or a ready
    ``ResNet(differentiable=True)``: ``loss(..., imgs=imgs)`` then reaches those kernels through the levels' gradient.

    Inputs of every method: ``points`` list of B ``(N_b,3)``; ``encoded_text (B,T,text_width)``, ``text_token_mask (B,T)`` bool (True =
    token); ``img_features`` one ``(B,V,C_l,H_l,W_l)`` per backbone level; ``scenes`` one dict per sample with ``depth2img =
    dict(extrinsic=[V x (4,4)], intrinsic=[V x ...] | one)`` and optionally ``img_meta`` (``scale_factor``, ``flip``,
    ``img_crop_offset``, ``img_shape``, the 3D flow record), as ``pipeline.GroundingFeaturePrefix`` takes them; ``img_pad_shape``.

    ``.train()`` with ``differentiable=True``: one ``loss(...)['...'].backward()`` reaches every parameter, ``encoded_text`` and every
    level of ``img_features`` (the last level receives the preshape's and the join's contributions summed).  Otherwise the module is
    inference-only: the chain runs under ``no_grad`` -- unless grad mode is on and an input requires grad, in which case the children
    are called as they are and raise their own errors.  ``fused_join=False`` takes the per-scene ``batch_point_sample`` calls and the
    two ``torch.cat`` that ``join_level_features`` replaces (same bits), for comparison and timing."""

    def __init__(self, preshape, backbone_3d, neck_3d, decoder, bbox_head, num_queries: int = 256, voxel_size: float = 0.01,
                 use_xyz_feat: bool = True, coord_type: str = "DEPTH", train_cfg: Optional[dict] = None, test_cfg: Optional[dict] = None,
                 text_width: Optional[int] = None, *, differentiable: bool = False, matcher: str = "host", fused_join: bool = True,
                 text_encoder=None, backbone=None, pixel_mean=None, pixel_std=None, bgr_to_rgb: bool = False):
        super().__init__()
        who = "GroundingDetector"
        if backbone is not None:
            if isinstance(backbone, dict) and backbone.get("type") in ("mmdet.ResNet", "ResNet"):
                backbone = dict(backbone, type="ResNet")    # this package's class, also where mmdet's own holds the name in the registry
            backbone = _build(who, "backbone", backbone, ResNet, False)
            if not isinstance(backbone, ResNet):
                raise TypeError(f"{who}: backbone must be an image_backbone.ResNet or its config dict, got {type(backbone).__name__}")
        elif pixel_mean is not None or pixel_std is not None or bgr_to_rgb:
            raise ValueError(f"{who}: pixel_mean / pixel_std / bgr_to_rgb go with backbone=")
        if (pixel_mean is None) != (pixel_std is None):
            raise ValueError(f"{who}: pixel_mean and pixel_std go together")
        if text_encoder is not None:
            text_encoder = _build(who, "text_encoder", text_encoder, ClipTextEncoder, False)
            if not isinstance(text_encoder, ClipTextEncoder):
                raise TypeError(f"{who}: text_encoder must be a ClipTextEncoder or its keyword dict, got {type(text_encoder).__name__}")
            if text_width is not None and int(text_width) != text_encoder.hidden_size:
                raise ValueError(f"{who}: text_width={text_width} differs from the text encoder's hidden_size={text_encoder.hidden_size}")
            text_width = text_encoder.hidden_size
        elif text_width is None:
            text_width = 768
        self.differentiable, self.fused_join = bool(differentiable), bool(fused_join)
        d = self.differentiable
        if not use_xyz_feat:
            raise NotImplementedError(f"{who}: use_xyz_feat=False is not implemented (the shipped configuration feeds the points as features)")
        if str(coord_type).upper() not in ("DEPTH", "LIDAR", "CAMERA"):
            raise ValueError(f"{who}: coord_type must be 'DEPTH', 'LIDAR' or 'CAMERA', got {coord_type!r}")
        if not float(voxel_size) > 0.0:
            raise ValueError(f"{who}: voxel_size must be positive, got {voxel_size}")
        if int(text_width) < 64 or int(text_width) > 2048 or int(text_width) % 64:
            raise ValueError(f"{who}: text_width must be a multiple of 64 from 64 to 2048, got {text_width}")
        if not isinstance(bbox_head, dict):
            raise TypeError(f"{who}: bbox_head must be the GroundingHead config dict, got {type(bbox_head).__name__}")
        head = dict(bbox_head)
        if head.pop("type", "GroundingHead") != "GroundingHead":
            raise ValueError(f"{who}: bbox_head must be of type 'GroundingHead', got {bbox_head.get('type')!r}")
        if not head.get("share_pred_layer", True):
            raise NotImplementedError(f"{who}: bbox_head share_pred_layer=False (one branch per decoder layer) is not implemented; "
                                      "share_pred_layer=True")
        self.num_queries, self.voxel_size, self.use_xyz_feat, self.coord_type = int(num_queries), float(voxel_size), True, str(coord_type)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.preshape = _build(who, "preshape", preshape, ProxyTransformationNormReverse, d)
        self.backbone_3d = _build(who, "backbone_3d", backbone_3d, MinkResNet, d)
        self.neck_3d = _build(who, "neck_3d", neck_3d, MinkNeck, d)
        self.decoder = _build(who, "decoder", decoder, GroundingDecoder, d)
        if float(self.neck_3d.voxel_size) != self.voxel_size:
            raise ValueError(f"{who}: neck_3d voxel_size={self.neck_3d.voxel_size} differs from voxel_size={self.voxel_size}")
        self.embed_dims = int(self.decoder.embed_dims)
        if int(self.neck_3d.out_channels) != self.embed_dims:
            raise ValueError(f"{who}: neck_3d out_channels={self.neck_3d.out_channels} differs from the decoder's embed_dims={self.embed_dims}")
        if int(self.preshape.embed_dim) != self.embed_dims:
            raise ValueError(f"{who}: preshape embed_dim={self.preshape.embed_dim} differs from the decoder's embed_dims={self.embed_dims}")
        if int(head.get("embed_dims", self.embed_dims)) != self.embed_dims:
            raise ValueError(f"{who}: bbox_head embed_dims={head.get('embed_dims')} differs from the decoder's embed_dims={self.embed_dims}")
        NL = int(self.decoder.num_layers)
        if int(head.setdefault("num_pred_layer", NL + 1)) != NL + 1:
            raise ValueError(f"{who}: bbox_head num_pred_layer={head['num_pred_layer']} but the decoder has {NL} layers (num_layers + 1 expected)")
        head.setdefault("embed_dims", self.embed_dims)
        if train_cfg is not None:
            head.setdefault("train_cfg", train_cfg)
        head.setdefault("test_cfg", test_cfg)
        self.bbox_head = GroundingLoss(**head, matcher=matcher)
        cc = self.bbox_head.contrastive_cfg
        self.query_select = QuerySelect(embed_dims=self.embed_dims, num_queries=self.num_queries, num_reg=self.bbox_head.num_reg,
                                        num_reg_fcs=self.bbox_head.num_reg_fcs, log_scale=cc.get("log_scale", "auto"),
                                        bias=cc.get("bias", False), max_text_len=self.bbox_head.max_text_len,
                                        box_coder=self.bbox_head.box_coder, differentiable=d)
        self.text_feat_map = nn.Linear(int(text_width), self.embed_dims)
        self.text_width = int(text_width)
        self.text_encoder = text_encoder     # None: no child, no entry in the state dict
        self.backbone = backbone             # likewise
        if backbone is not None and len(backbone.out_indices) != int(self.backbone_3d.num_stages):
            raise ValueError(f"{who}: the backbone returns {len(backbone.out_indices)} levels, backbone_3d has {self.backbone_3d.num_stages}")
        self.pixel_mean = None if pixel_mean is None else tuple(float(v) for v in pixel_mean)
        self.pixel_std = None if pixel_std is None else tuple(float(v) for v in pixel_std)
        self.bgr_to_rgb = bool(bgr_to_rgb)
        self._staging: dict = {}            # per stream: the pinned staging buffer of the join tables

    def __deepcopy__(self, memo):
        """A copy shares no staging buffer (pinned memory and an event of the stream it was used on) and no ingest."""
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_staging" else None if k == "_ingest" else copy.deepcopy(v, memo)
        return new

    # ------------------------------------------------------------------------------------------------------------- the chain
    def _records(self, *inputs) -> bool:
        """Whether this call runs in the caller's grad mode: the training chain, or an inference call whose input requires grad (the
        children then raise their own errors)."""
        if self.differentiable and self.training:
            return True
        return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.is_floating_point() and t.requires_grad for t in inputs)

    def join_tables(self, scenes: Sequence[dict], img_pad_shape: Sequence[int], device, aligned: bool = False) -> JoinTables:
        """The per-scene tables of the level join from the samples' ``depth2img`` / ``img_meta`` (DET:404-426), one pinned upload."""
        from .pipeline import projection_matrices
        projs, pres, scal = [], [], []
        for sc in scenes:
            meta = sc.get("img_meta") or {}
            projs.append(projection_matrices(sc["depth2img"]))
            pres.append(reverse_3d_flow(meta, self.coord_type))
            scal.append(image_transform_scalars(meta, img_pad_shape))
        return JoinTables(projs, pres, scal, self.voxel_size, device, aligned=aligned, staging=self._staging)

    def _check_inputs(self, points, img_features, scenes):
        who = "GroundingDetector"
        B = len(points)
        if not 1 <= B <= 64 or len(scenes) != B:
            raise ValueError(f"{who}: 1 to 64 scenes with one dict each, got {B} point clouds and {len(scenes)} scene dicts")
        nl = int(self.backbone_3d.num_stages)
        if len(img_features) != nl:
            raise ValueError(f"{who}: {nl} levels of img_features expected, got {len(img_features)}")
        V = None
        for l, f in enumerate(img_features):
            if not isinstance(f, torch.Tensor) or f.dim() != 5 or f.shape[0] != B:
                raise ValueError(f"{who}: img_features[{l}] ({B},V,C,H,W) expected, got {tuple(getattr(f, 'shape', ()))}")
            V = int(f.shape[1]) if V is None else V
            if int(f.shape[1]) != V:
                raise ValueError(f"{who}: img_features[{l}] has {f.shape[1]} views, img_features[0] has {V}")
        return B

    def extract_feat(self, points, text_dict: dict, img_features: Sequence[torch.Tensor], scenes: Sequence[dict],
                     img_pad_shape: Sequence[int] = (480, 480), bbox: Optional[torch.Tensor] = None, keep_out: Optional[list] = None,
                     trace: Optional[dict] = None, _mode: Optional[bool] = None):
        """DET:337-484 behind the 2D backbone: ``(feats, scores, coords)``, each a list of B tensors.  ``text_dict``: the MAPPED text
        (``text_feats (B,T,embed_dims)``, ``text_token_mask``).  ``keep_out``: receives the neck's keep masks; ``trace``: a dict that
        receives the intermediates (``points``, ``coordinates``, ``features``, ``scene_rows``, ``levels``, ``joined``)."""
        B = self._check_inputs(points, img_features, scenes)
        mode = self._records(text_dict["text_feats"], *img_features) if _mode is None else _mode
        with torch.set_grad_enabled(mode):
            dev = img_features[-1].device
            tables = self.join_tables(scenes, img_pad_shape, dev)
            nl = len(img_features)
            prepared = prepare_features_many([img_features[l][b] for l in range(nl) for b in range(B)])
            outs = self.preshape(points, text_dict, img_features[-1], bbox=bbox)                       # DET:385
            coords, feats, ends = self.preshape.quantize(outs, self.voxel_size, return_scene_rows=True)  # DET:388-397
            levels = self.backbone_3d(coords, ends, feats)                                           # DET:398
            joined = []
            for l, lv in enumerate(levels):                                                          # DET:402-479
                prep = prepared[l * B:(l + 1) * B]
                if self.fused_join:
                    f = join_level_features(lv, img_features[l], tables, prepared=prep)
                else:
                    f = join_level_features_per_scene(lv, img_features[l], tables, prepared=prep)
                joined.append(SparseLevel(feats=f, coords=lv.coords, scene_rows=list(lv.scene_rows), tensor_stride=lv.tensor_stride))
            if trace is not None:
                trace.update(points=outs, coordinates=coords, features=feats, scene_rows=ends, levels=levels, joined=joined, tables=tables)
            return self.neck_3d(joined, B, keep_out=keep_out)                                         # DET:482

    def encode_text(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None):
        """``(encoded_text (B,T,text_width), text_token_mask = attention_mask.bool())`` from the tokenizer's output (DET:661-668): the
        text encoder's ``last_hidden_state``, detached.  ``attention_mask=None``: every position is a token."""
        if self.text_encoder is None:
            raise ValueError("GroundingDetector: input_ids need a text encoder; construct the detector with text_encoder=")
        encoded = self.text_encoder(input_ids, attention_mask)
        if attention_mask is None:
            mask = torch.ones(tuple(input_ids.shape), dtype=torch.bool, device=encoded.device)
        else:
            mask = (attention_mask != 0).to(encoded.device)
        return encoded, mask

    def _text(self, encoded_text, text_token_mask, input_ids, attention_mask):
        """The text operands of a call: the encoded text as given, or the encoder's output for ``input_ids`` / ``attention_mask``."""
        if input_ids is None:
            if attention_mask is not None:
                raise ValueError("GroundingDetector: attention_mask goes with input_ids; with encoded_text pass text_token_mask")
            if encoded_text is None or text_token_mask is None:
                raise ValueError("GroundingDetector: encoded_text and text_token_mask, or input_ids (and attention_mask), are required")
            return encoded_text, text_token_mask
        if encoded_text is not None or text_token_mask is not None:
            raise ValueError("GroundingDetector: input_ids / attention_mask take the place of encoded_text / text_token_mask; pass one pair")
        return self.encode_text(input_ids, attention_mask)

    def extract_image_features(self, imgs: torch.Tensor) -> List[torch.Tensor]:
        """DET:357-379: the backbone's levels ``(B,V,C_l,H_l,W_l)`` of ``imgs (B,V,3,H,W)`` (float32 or uint8); the data
        preprocessor's ``pixel_mean`` / ``pixel_std`` / ``bgr_to_rgb`` are applied by the stem.  Detached -- unless the backbone records
        (``ResNet(differentiable=True)``, grad mode on, a trainable kernel that requires grad): then the levels of its trainable stages
        are attached to its kernels."""
        if self.backbone is None:
            raise ValueError("GroundingDetector: imgs need a backbone; construct the detector with backbone=")
        if not isinstance(imgs, torch.Tensor) or imgs.dim() != 5:
            raise ValueError(f"GroundingDetector: imgs (B,V,3,H,W) expected, got {tuple(getattr(imgs, 'shape', ()))}")
        return list(self.backbone(imgs, mean=self.pixel_mean, std=self.pixel_std, bgr_to_rgb=self.bgr_to_rgb))

    def _images(self, img_features, imgs, img_pad_shape):
        """The image operands of a call: the feature levels as given, or the backbone's for ``imgs``; and ``img_pad_shape``, which
        defaults to the images' ``(H, W)`` (without images: to (480, 480), as it always did)."""
        if imgs is None:
            if img_features is None:
                raise ValueError("GroundingDetector: img_features, or imgs (with a backbone), are required")
            return img_features, ((480, 480) if img_pad_shape is None else img_pad_shape)
        if img_features is not None:
            raise ValueError("GroundingDetector: imgs take the place of img_features; pass one of them")
        feats = self.extract_image_features(imgs)
        return feats, (tuple(int(v) for v in imgs.shape[-2:]) if img_pad_shape is None else img_pad_shape)

    def map_text(self, encoded_text: torch.Tensor, _mode: Optional[bool] = None) -> torch.Tensor:
        """``text_feat_map(encoded_text)`` (DET:659) through ``decoder.linear``."""
        rec = self._records(encoded_text) if _mode is None else _mode
        with torch.set_grad_enabled(rec):
            return linear(encoded_text, self.text_feat_map.weight, self.text_feat_map.bias, differentiable=self.differentiable and rec)

    def forward_transformer(self, point_feats: List[torch.Tensor], scores: List[torch.Tensor], point_xyz: List[torch.Tensor],
                            text_dict: dict, keep_out: Optional[dict] = None, trace: Optional[dict] = None,
                            _mode: Optional[bool] = None) -> dict:
        """DET:486-621 and the head's forward: ``dict(text_feats, text_token_mask, hidden_states (NL,B,K,C), all_layers_pred_bboxes
        (NL,B,K,9), all_layers_cls_scores (NL,B,K,max_text_len))``.  ``keep_out``: receives the selection's ``score`` and ``index``;
        ``trace``: receives ``decoder_inputs``."""
        mode = self._records(text_dict["text_feats"], *point_feats) if _mode is None else _mode
        with torch.set_grad_enabled(mode):
            dec, head = self.query_select(point_feats, scores, point_xyz, text_dict["text_feats"], text_dict["text_token_mask"],
                                          keep_out=keep_out)
            if trace is not None:
                trace["decoder_inputs"] = dec
            hidden, boxes = self.decoder(query=dec["query"], key=dec["feats"], value=dec["feats"],              # DET:605-617
                                         key_padding_mask=dec["feats_attention_mask"], self_attn_mask=None, cross_attn_mask=None,
                                         query_coords=dec["query_coords"], key_coords=dec["feats_coords"], pred_bboxes=dec["pred_bboxes"],
                                         text_feats=dec["text_feats"], text_attention_mask=dec["text_attention_mask"],
                                         bbox_head=self.query_select)
            head = dict(head, hidden_states=hidden, all_layers_pred_bboxes=boxes)
            head["all_layers_cls_scores"] = self.decoder.head_scores(hidden, head, self.query_select,
                                                                     differentiable=self.differentiable and mode)
            return head

    def forward(self, points, encoded_text=None, text_token_mask=None, img_features=None, scenes=None, img_pad_shape=None, bbox=None,
                trace: Optional[dict] = None, *, input_ids=None, attention_mask=None, imgs=None) -> dict:
        """The whole chain up to the head's outputs (``forward_transformer``'s dict).  ``input_ids=`` / ``attention_mask=`` (with a text
        encoder) take the place of ``encoded_text`` / ``text_token_mask``; ``imgs=`` (with a backbone) takes the place of
        ``img_features``.  ``img_pad_shape``: None is the images' ``(H, W)``, without images (480, 480)."""
        encoded_text, text_token_mask = self._text(encoded_text, text_token_mask, input_ids, attention_mask)
        img_features, img_pad_shape = self._images(img_features, imgs, img_pad_shape)
        mode = self._records(encoded_text, *img_features)      # one decision for the whole chain, from the caller's inputs
        text_dict = dict(text_feats=self.map_text(encoded_text, mode), text_token_mask=text_token_mask)
        keep: list = []
        sel: dict = {}
        feats, scores, xyz = self.extract_feat(points, text_dict, img_features, scenes, img_pad_shape, bbox=bbox, keep_out=keep, trace=trace,
                                               _mode=mode)
        head = self.forward_transformer(feats, scores, xyz, text_dict, keep_out=sel, trace=trace, _mode=mode)
        if trace is not None:
            trace.update(text_feats=text_dict["text_feats"], neck=(feats, scores, xyz), keep=keep, select=sel)
        return head

    def loss(self, points, encoded_text=None, text_token_mask=None, img_features=None, scenes=None, gt_bboxes=None, positive_maps=None,
             img_pad_shape=None, bbox=None, trace: Optional[dict] = None, *, input_ids=None, attention_mask=None,
             imgs=None) -> Dict[str, torch.Tensor]:
        """DET:623-705: the reference's loss dict (``loss_cls``, ``loss_bbox``, ``d{i}.loss_cls``, ``d{i}.loss_bbox``)."""
        encoded_text, text_token_mask = self._text(encoded_text, text_token_mask, input_ids, attention_mask)
        head = self.forward(points, encoded_text, text_token_mask, img_features, scenes, img_pad_shape, bbox, trace, imgs=imgs)
        return self.bbox_head.loss(head["all_layers_cls_scores"], head["all_layers_pred_bboxes"], text_token_mask, gt_bboxes, positive_maps)

    def predict(self, points, encoded_text=None, text_token_mask=None, img_features=None, scenes=None, img_pad_shape=None, bbox=None,
                trace: Optional[dict] = None, *, input_ids=None, attention_mask=None, imgs=None) -> List[dict]:
        """DET:707-794 with ``GroundingHead.predict`` (grounding_head.py:566-604): per scene ``dict(bboxes_3d (K,9), scores_3d (K,),
        target_scores_3d (K,))``; the reference regards the scores as the target scores at inference."""
        head = self.forward(points, encoded_text, text_token_mask, img_features, scenes, img_pad_shape, bbox, trace, input_ids=input_ids,
                            attention_mask=attention_mask, imgs=imgs)
        boxes, scores = self.bbox_head.predict(head["all_layers_cls_scores"], head["all_layers_pred_bboxes"])
        return [dict(bboxes_3d=boxes[b], scores_3d=scores[b], target_scores_3d=scores[b]) for b in range(boxes.shape[0])]

    def from_scenes(self, scenes: Sequence[dict], n_points: int = 100000, sampler: str = "host", rng=None, seed: Optional[int] = None):
        """For callers that hold depth maps: runs ``ingest.MultiViewIngest`` (N4) on ``scenes`` (``depth_img``, ``depth_cam2img``,
        ``depth2img``, ...; as ``pipeline.GroundingFeaturePrefix`` takes them) and returns ``(points, bbox)`` to pass on to ``loss`` /
        ``predict`` / ``forward`` together with the same ``scenes``."""
        import numpy as np
        from .ingest import MultiViewIngest
        ing = getattr(self, "_ingest", None)
        if ing is None or ing[0] != (int(n_points), sampler):
            ing = self._ingest = ((int(n_points), sampler), MultiViewIngest(int(n_points), sampler=sampler))
        batch = ing[1](scenes, rng=np.random if rng is None else rng, seed=seed)
        return batch.points, batch.bbox

    # ------------------------------------------------------------------------------------------------------------- the host chain
    def forward_host(self, points, encoded_text=None, text_token_mask=None, img_features=None, scenes=None, img_pad_shape=None,
                     dtype=None, decisions: Optional[dict] = None, gt_bboxes=None, positive_maps=None, host=None, *, input_ids=None,
                     attention_mask=None, imgs=None) -> dict:
        """The same chain (eval mode) from the stages' own host restatements in numpy ``dtype`` (float64, the default, or float32):
        ``host.forward`` (the preshape) -> ``host.voxelize`` -> ``MinkResNet.forward_host`` -> ``host.point_sample`` per scene and
        level plus the two concatenations -> ``MinkNeck.forward_host`` -> (with ``imgs=``: ``ResNet.forward_host`` in front of it all; with ``input_ids=``:
        ``ClipTextEncoder.forward_host`` ->)
        ``text_feat_map`` -> ``QuerySelect.forward_host`` -> the
        renaming of DET:605-617 -> ``GroundingDecoder.forward_host`` -> ``contrastive_scores_host`` -> ``predict_host`` (and ``loss_host``
        when ``gt_bboxes`` / ``positive_maps`` are given).  It calls no device code.  ``decisions``: the device's discrete decisions,
        handed in where two precisions may differ -- ``points`` (the preshape's output clouds: which points survive, and through the
        1 cm floor which voxel each falls in; without it ``host.forward`` runs), ``keep`` (the neck's masks), ``index`` (the
        query selection), ``assign`` (the matching; without it the host matcher runs on the host's costs).  Returns every intermediate:
        ``text_feats, points, coordinates, features, scene_rows, levels, joined, neck, keep, select, decoder_inputs, hidden_states,
        all_layers_pred_bboxes, all_layers_cls_scores, bboxes_3d, scores_3d`` (+ ``losses``, ``assign``); ``keep`` and ``select`` hold the
        host's OWN decisions.  ``host``: the module of fp32 CPU restatements the repository keeps beside the package (``forward``,
        ``voxelize``, ``point_sample``); the caller hands it in -- the product imports nothing from it.  The preshape and the sampling are
        fp32 restatements in either ``dtype``."""
        if host is None:
            raise ValueError("GroundingDetector.forward_host: host= (the module of CPU restatements: forward, voxelize, point_sample) is required")
        import numpy as np
        from . import decoder_host, grounding_loss_host as glh
        from .pipeline import projection_matrices
        dt = np.dtype(np.float64 if dtype is None else dtype)
        if imgs is not None:
            if img_features is not None:
                raise ValueError("GroundingDetector.forward_host: imgs take the place of img_features; pass one of them")
            if self.backbone is None:
                raise ValueError("GroundingDetector.forward_host: imgs need a backbone; construct the detector with backbone=")
            img_features = self.backbone.forward_host(imgs, dtype=dt, mean=self.pixel_mean, std=self.pixel_std, bgr_to_rgb=self.bgr_to_rgb)
            if img_pad_shape is None:
                img_pad_shape = tuple(int(v) for v in imgs.shape[-2:])
        elif img_features is None:
            raise ValueError("GroundingDetector.forward_host: img_features, or imgs (with a backbone), are required")
        if img_pad_shape is None:
            img_pad_shape = (480, 480)
        if input_ids is not None:
            if encoded_text is not None or text_token_mask is not None:
                raise ValueError("GroundingDetector.forward_host: input_ids / attention_mask take the place of encoded_text / text_token_mask")
            if self.text_encoder is None:
                raise ValueError("GroundingDetector.forward_host: input_ids need a text encoder; construct the detector with text_encoder=")
            ids = _np(input_ids)
            encoded_text = self.text_encoder.forward_host(ids, attention_mask, dtype=dt)
            text_token_mask = np.ones(ids.shape, bool) if attention_mask is None else _np(attention_mask) != 0
        decisions = dict(decisions or {})
        arr = lambda t, d=None: _np(t.float() if isinstance(t, torch.Tensor) else t, d or dt)      # noqa: E731  (.float(): numpy has no bf16)
        B = len(points)
        mask = arr(text_token_mask, bool)
        w, b = arr(self.text_feat_map.weight), arr(self.text_feat_map.bias)
        text = arr(encoded_text) @ w.T + b                                                          # DET:659
        imgs = [arr(f, np.float32) for f in img_features]
        if decisions.get("points") is not None:
            outs = [arr(p, np.float32) for p in decisions["points"]]
        else:
            pre = self.preshape
            sd = {k: v.detach().cpu().numpy() for k, v in pre.state_dict().items()}
            ref = host.forward(sd, grid_size=pre.grid_size, dynamic_drop_radio=pre.dynamic_drop_radio, num_sub=pre.num_sub,
                                 num_heads=pre.num_heads, text_blocks=pre.text_blocks, img_blocks=pre.img_blocks,
                                 points=np.stack([arr(p, np.float32) for p in points]), text_feats=text.astype(np.float32), text_mask=mask,
                                 img_feat=imgs[-1])
            outs = [np.asarray(o, np.float32) for o in ref["outputs"]]                               # DET:385
        coords, feats, _ = host.voxelize(outs, self.voxel_size)                                   # DET:388-397
        ends = np.cumsum(np.bincount(coords[:, 0], minlength=B)).tolist()
        levels = self.backbone_3d.forward_host(coords, ends, feats, dtype=dt)                       # DET:398
        joined = []
        for l, lv in enumerate(levels):                                                             # DET:402-479
            lo = [0] + list(lv.scene_rows[:-1])
            parts = []
            for sb, sc in enumerate(scenes):
                meta = sc.get("img_meta") or {}
                pts = np.asarray(lv.coords)[lo[sb]:lv.scene_rows[sb], 1:4].astype(np.float32) * np.float32(self.voxel_size)
                A = reverse_3d_flow(meta, self.coord_type)
                if A is not None:                                                                   # one affine, the kernel's fp32 steps
                    A = A.numpy().astype(np.float32)
                    full = lambda v, n=len(pts): np.full(n, v, np.float32)                          # noqa: E731
                    fma = lambda a, b, c: (a.astype(np.float64) * b + c).astype(np.float32)         # noqa: E731  (an fp32 FMA: the product is exact in double)
                    pts = np.stack([fma(full(A[r, 2]), pts[:, 2], fma(full(A[r, 1]), pts[:, 1], full(A[r, 0]) * pts[:, 0]))
                                    + A[r, 3] for r in range(3)], 1)
                sw, sh, cw, ch, flip, ori_w, pad_h, pad_w = image_transform_scalars(meta, img_pad_shape)
                samp, _ = host.point_sample(pts, imgs[l][sb], projection_matrices(sc["depth2img"]), scale=(sw, sh), crop=(cw, ch), flip=flip,
                                              ori_w=ori_w, pad_hw=(pad_h, pad_w))
                parts.append(samp.astype(dt))
            joined.append(SparseLevel(feats=np.concatenate([np.asarray(lv.feats, dt), np.concatenate(parts)], 1), coords=lv.coords,
                                      scene_rows=list(lv.scene_rows), tensor_stride=lv.tensor_stride))
        ntrace: list = []
        nf, ns, nx = self.neck_3d.forward_host(joined, B, dtype=dt, keep=decisions.get("keep"), trace=ntrace)   # DET:482
        sel: dict = {}
        dec, head = self.query_select.forward_host(nf, ns, nx, text, mask, dtype=dt, index=decisions.get("index"), keep_out=sel)
        hidden, boxes = self.decoder.forward_host(query=dec["query"], key=dec["feats"], key_padding_mask=dec["feats_attention_mask"],    # DET:605-617
                                                  query_coords=dec["query_coords"], key_coords=dec["feats_coords"],
                                                  pred_bboxes=dec["pred_bboxes"], text_feats=dec["text_feats"],
                                                  text_attention_mask=dec["text_attention_mask"], bbox_head=self.query_select, dtype=dt)
        qs = self.query_select
        scores = decoder_host.contrastive_scores_host(hidden, head["text_feats"], head["text_token_mask"],
                                                      arr(qs.cls_branch.bias) if qs.has_bias else None, qs.scaled, qs.max_text_len)
        pb, ps = glh.predict_host(scores, boxes)
        out = dict(text_feats=text, points=outs, coordinates=coords, features=feats, scene_rows=ends, levels=levels, joined=joined,
                   neck=(nf, ns, nx), keep=[t["keep"] for t in ntrace], select=sel, decoder_inputs=dec, hidden_states=hidden,
                   all_layers_pred_bboxes=boxes, all_layers_cls_scores=scores, bboxes_3d=pb, scores_3d=ps)
        if gt_bboxes is not None:
            gts, pos = [arr(g, np.float64) for g in gt_bboxes], [arr(p, np.float64) for p in positive_maps]
            head_ = self.bbox_head
            assign = decisions.get("assign")
            if assign is None:
                costs = glh.cost_host(scores, boxes, mask, gts, pos, head_.cost_alpha, head_.cost_gamma, head_.cost_weights)
                assign = glh.assign_host(costs, int(boxes.shape[2]))
            assign = arr(assign, np.int32)
            K = int(boxes.shape[2])
            avg = max(float(sum(min(K, len(g)) for g in gts)), 1.0)
            res = glh.loss_host(scores, boxes, mask, gts, pos, assign, head_.alpha, head_.gamma, head_.decouple_weights, avg, head_.loss_weights)
            out.update(losses=glh.loss_dict(res["loss_cls"], res["loss_bbox"]), assign=assign)
        return out

    # ------------------------------------------------------------------------------------------------------------- checkpoints
    def _reference_names(self):
        """``(reference name, own name)`` for every tensor of ``state_dict()``; the shared branches appear once per alias."""
        NL = int(self.decoder.num_layers)
        pairs = []
        for own in self.state_dict():
            top, rest = own.split(".", 1)
            if top == "query_select":
                branch, tail = rest.split(".", 1)
                for i in range(NL + 1):
                    pairs.append((f"bbox_head.{branch.replace('_branch', '_branches')}.{i}.{tail}", own))
            else:
                pairs.append((own, own))
        return pairs

    def reference_state_dict(self) -> Dict[str, torch.Tensor]:
        """The state dict under the reference's names: ``preshape.*``, ``backbone_3d.*``, ``neck_3d.*``, ``decoder.*``,
        ``text_feat_map.*``, with a text encoder ``text_encoder.text_model.*``, with a backbone ``backbone.*``, and the ``NL + 1`` aliases
        ``bbox_head.cls_branches.{i}.*`` / ``bbox_head.reg_branches.{i}.*``."""
        sd = self.state_dict()
        return {ref: sd[own] for ref, own in self._reference_names()}

    def load_reference_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True) -> dict:
        """Loads a reference checkpoint's ``state_dict``.  While the detector holds no backbone / no text encoder, ``backbone.*`` /
        ``text_encoder.*`` belong to modules outside this one: skipped and listed.  With a backbone its tensors are loaded under
        ``backbone.*`` (mmdet's names).  With a text encoder its tensors are loaded, under
        ``text_encoder.text_model.*`` or ``text_encoder.*`` (``ClipTextEncoder.normalise_names``), a ``position_ids`` buffer ignored.
        The aliases of a shared branch must be equal (``ValueError`` naming the key).  ``strict``: a missing or unexpected key raises
        ``KeyError``.  Returns ``dict(skipped, missing, unexpected)``."""
        outside = _OUTSIDE if self.backbone is None else tuple(p for p in _OUTSIDE if p != _IMAGE)
        if self.text_encoder is not None:
            outside = tuple(p for p in outside if p != _TEXT)
            text = ClipTextEncoder.normalise_names({k[len(_TEXT):]: v for k, v in state_dict.items() if k.startswith(_TEXT)})
            state_dict = {k: v for k, v in state_dict.items() if not k.startswith(_TEXT)}
            state_dict.update({_TEXT + k: v for k, v in text.items()})
        wanted = self._reference_names()
        own_sd, first, missing = {}, {}, []
        for ref, own in wanted:
            if ref not in state_dict:
                missing.append(ref)
                continue
            t = state_dict[ref]
            if own in own_sd:
                if t.shape != own_sd[own].shape or not torch.equal(t.to(own_sd[own].device), own_sd[own]):
                    raise ValueError(f"GroundingDetector.load_reference_state_dict: {ref} differs from {first[own]}; with "
                                     "share_pred_layer=True every layer's branch is the same tensor")
            else:
                own_sd[own], first[own] = t, ref
        names = {ref for ref, _ in wanted}
        skipped = sorted(k for k in state_dict if k.startswith(outside))
        unexpected = sorted(k for k in state_dict if k not in names and not k.startswith(outside))
        if strict and (missing or unexpected):
            raise KeyError(f"GroundingDetector.load_reference_state_dict(strict=True): missing {missing[:8]}"
                           f"{' ...' if len(missing) > 8 else ''}, unexpected {unexpected[:8]}{' ...' if len(unexpected) > 8 else ''}")
        self.load_state_dict(own_sd, strict=not missing)
        return dict(skipped=skipped, missing=missing, unexpected=unexpected)
