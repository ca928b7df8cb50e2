"""The grounding loss behind the decoder: ``GroundingHead.loss`` / ``loss_by_feat`` / ``predict_by_feat`` (dense_heads/grounding_head.py:
537-824) as the shipped configuration runs them, on the device.  It consumes what ``decoder.py`` produces in place:
``contrastive_scores``' ``(NL,B,K,max_text_len)`` with ``-inf`` on masked tokens and behind ``T``, and ``GroundingDecoder``'s
``(NL,B,K,9)`` boxes.

Six calls into ``csrc/grounding_loss.hip`` and ``csrc/grounding_assign.hip`` on the current stream, each restated in numpy by
``grounding_loss_host.py``, which is their specification: ``box_iou3d`` (the IoU of two 9-DoF boxes; the reference takes it from
pytorch3d's CUDA extension, which has no ROCm build), ``match_costs`` (every layer, scene, query and ground-truth box in ONE launch),
the matching on the device (one), the loss forward (two launches), its backward (one) and ``predict_scores``.  fp32 operands and results
(the IoU's geometry and the matching's duals between them run in double: DESIGN.md 5.15, 5.18); no float atomics and fixed summation
orders, so two calls give the same bits.

THE ONE SYNCHRONISE of the stage is in ``assign`` with ``matcher='host'`` (the default): the cost matrices of all layers and scenes
travel to the host in one copy through pinned memory, the stream is waited for once, ``scipy.optimize.linear_sum_assignment`` runs per
(layer, scene) on ``nan_to_num(cost, 100, 100, -100)``, and the assignment goes back in one copy.  The reference does this once per
(layer, scene) -- 36 round trips at 6 layers and 6 scenes -- and sleeps 20 ms before each (hungarian_assigner.py:120); there is no sleep
here.  With ``matcher='device'`` the matching is one more launch (``ptx_gl_assign``: the same shortest-augmenting-path method, one wave
per (layer, scene); ``grounding_loss_host.sap_assign_host`` is its specification, bit for bit) and the stage has NO synchronise: cost,
matching, loss and backward are enqueued without a host wait.  On a tie between optimal matchings the two matchers may pick different
pairs.

The loss is one autograd node ``(scores, boxes) -> (2,NL)``; the matching sees detached values.  Deviations from the reference: a batch
without any ground-truth box raises ``ValueError`` before anything is launched (the reference takes the mean of nothing: NaN); a masked
token is never read (the reference multiplies by a mask).  Unpinned: mmdet's focal loss is restated from its published source (mmdet is
not installed), and pytorch3d's IoU on degenerate pairs (coplanar faces, zero sizes) is not reproduced -- ``grounding_loss_host.py``
states this project's rule.

Out of scope: denoising queries, bf16, double backward, ``norm_decouple_loss``, ``decouple_groups=3``, the
``g4`` corner grouping, ``num_reg=12`` and the FCAF coder.  There is no CPU path: tensors must be on the GPU and the library must be
built."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _abi
from .grounding_loss_host import SAP_MAX_COLS, SAP_MAX_ROWS
from ._doors import MAX_QUERIES, MAX_SCENES, MAX_TEXT, _f32, _f32_grad, _gpu, _mask_bytes, _stream

__all__ = ["GroundingLoss", "box_iou3d", "grounding_loss", "hungarian_assign", "match_costs", "predict_scores"]

F32_EPS = float(np.finfo(np.float32).eps)


def box_iou3d(boxes1: torch.Tensor, boxes2: torch.Tensor) -> torch.Tensor:
    """``(N,M) fp32``: the IoU of every box of ``boxes1 (N,9)`` with every box of ``boxes2 (M,9)``, boxes as
    ``EulerDepthInstance3DBoxes`` holds them with origin (0.5, 0.5, 0.5): ``(cx,cy,cz, sx,sy,sz, a0,a1,a2)``, ``R = Rz(a0) Rx(a1) Ry(a2)``.
    The exact intersection volume of the two hexahedra; NaN for the pairs of a box with a NaN, an inf or a non-positive size
    (``grounding_loss_host.box_iou3d_host``; ``ptx_gl_iou``, one launch)."""
    _gpu("box_iou3d", boxes1, boxes2)
    dev = boxes1.device
    b1, b2 = _f32(boxes1, "box_iou3d", dev), _f32(boxes2, "box_iou3d", dev)
    if b1.dim() != 2 or b2.dim() != 2 or b1.shape[1] != 9 or b2.shape[1] != 9:
        raise ValueError(f"box_iou3d: boxes (N,9) and (M,9) expected, got {tuple(b1.shape)}, {tuple(b2.shape)}")
    N, M = int(b1.shape[0]), int(b2.shape[0])
    out = torch.empty((N, M), dtype=torch.float32, device=dev)
    if N * M:
        _abi.check(_abi.lib().ptx_gl_iou(b1.data_ptr(), N, b2.data_ptr(), M, out.data_ptr(), _stream(dev)), "ptx_gl_iou")
    return out


class _Targets:
    """The ground truth of a batch as the launches take it: boxes ``(SG,9)``, positive maps ``(SG,M)``, and one int32 tensor
    ``[offset (B+1) | scene (SG)]``."""

    def __init__(self, what: str, gt_bboxes: Sequence, positive_maps: Sequence, B: int, M: int, dev):
        if len(gt_bboxes) != B or len(positive_maps) != B:
            raise ValueError(f"{what}: one ground-truth tensor and one positive map per scene ({B}) expected, got {len(gt_bboxes)} and "
                             f"{len(positive_maps)}")
        boxes = [g.tensor if hasattr(g, "tensor") else g for g in gt_bboxes]
        _gpu(what, *boxes, *positive_maps)
        self.G = [int(g.shape[0]) for g in boxes]
        for b, (g, p) in enumerate(zip(boxes, positive_maps)):
            if g.dim() != 2 or g.shape[1] != 9 or tuple(p.shape) != (self.G[b], M):
                raise ValueError(f"{what}: scene {b}: gt_bboxes (G,9) and positive_maps (G,{M}) expected, got {tuple(g.shape)}, {tuple(p.shape)}")
        self.SG = sum(self.G)
        self.offset = np.concatenate([[0], np.cumsum(self.G)]).astype(np.int32)
        self.boxes = torch.cat([_f32(g, what, dev) for g in boxes]) if self.SG else torch.zeros((0, 9), dtype=torch.float32, device=dev)
        self.maps = torch.cat([_f32(p, what, dev) for p in positive_maps]) if self.SG else torch.zeros((0, M), dtype=torch.float32, device=dev)
        meta = np.concatenate([self.offset, np.repeat(np.arange(B, dtype=np.int32), self.G)]).astype(np.int32)
        self.meta = torch.from_numpy(meta).pin_memory().to(dev, non_blocking=True)      # (a pageable copy would wait for the stream)
        self.offset_ptr, self.scene_ptr = self.meta.data_ptr(), self.meta.data_ptr() + 4 * (B + 1)


def _operands(what: str, scores: torch.Tensor, boxes: torch.Tensor, text_token_mask: torch.Tensor):
    _gpu(what, scores, boxes, text_token_mask)
    if scores.dim() != 4 or boxes.dim() != 4 or tuple(boxes.shape) != tuple(scores.shape[:3]) + (9,):
        raise ValueError(f"{what}: scores (NL,B,K,M) and boxes (NL,B,K,9) expected, got {tuple(scores.shape)}, {tuple(boxes.shape)}")
    NL, B, K, M = (int(s) for s in scores.shape)
    T = int(text_token_mask.shape[-1])
    if not 1 <= NL <= 64 or not 1 <= B <= MAX_SCENES or not 0 <= K <= MAX_QUERIES or not 1 <= T <= M <= MAX_TEXT:
        raise ValueError(f"{what}: 1 to 64 layers, 1 to {MAX_SCENES} scenes, up to {MAX_QUERIES} queries and 1 <= T <= M <= {MAX_TEXT}, got "
                         f"NL={NL}, B={B}, K={K}, T={T}, M={M}")
    return NL, B, K, M, T, _mask_bytes(what, "text_token_mask", text_token_mask, (B, T))


def _focal_args(what: str, alpha: float, gamma: float) -> Tuple[float, float]:
    alpha, gamma = float(alpha), float(gamma)
    if not 0.0 <= alpha <= 1.0 or not 1.0 <= gamma <= 8.0:
        raise ValueError(f"{what}: alpha from 0 to 1 and gamma from 1 to 8, got alpha={alpha}, gamma={gamma}")
    return alpha, gamma


def match_costs(scores: torch.Tensor, boxes: torch.Tensor, text_token_mask: torch.Tensor, gt_bboxes: Sequence[torch.Tensor],
                positive_maps: Sequence[torch.Tensor], alpha: float = 0.25, gamma: float = 2.0, weights=(1.0, 2.0, 2.0),
                _targets: Optional[_Targets] = None) -> Tuple[torch.Tensor, List[int]]:
    """``(cost (NL,K,sum G) fp32, G)``: the matching costs of ``HungarianAssigner3D`` for every layer and scene; scene b's ``K x G_b``
    matrix of layer l is ``cost[l][:, sum(G[:b]) : sum(G[:b+1])]`` -- ``weights[0]`` ``BinaryFocalLossCost`` over the unmasked tokens
    (``alpha``, ``gamma``; fractional targets) ``+ weights[1]`` L1 of the nine box values ``- weights[2]`` IoU
    (``grounding_loss_host.cost_host``; ``ptx_gl_cost``, one launch)."""
    NL, B, K, M, T, mask = _operands("match_costs", scores, boxes, text_token_mask)
    dev = scores.device
    alpha, gamma = _focal_args("match_costs", alpha, gamma)
    tg = _targets or _Targets("match_costs", gt_bboxes, positive_maps, B, M, dev)
    s, bx = _f32(scores, "match_costs", dev), _f32(boxes, "match_costs", dev)
    cost = torch.empty((NL, K, tg.SG), dtype=torch.float32, device=dev)
    if K and tg.SG:
        _abi.check(_abi.lib().ptx_gl_cost(s.data_ptr(), bx.data_ptr(), NL, B, K, M, mask.data_ptr(), T, tg.boxes.data_ptr(), tg.maps.data_ptr(),
                                          tg.scene_ptr, tg.SG, alpha, gamma, float(weights[0]), float(weights[1]), float(weights[2]),
                                          cost.data_ptr(), _stream(dev)), "ptx_gl_cost")
    return cost, list(tg.G)


def _solve(cost: np.ndarray, G: Sequence[int], B: int) -> np.ndarray:
    from scipy.optimize import linear_sum_assignment
    NL, K, _ = cost.shape
    cost = np.nan_to_num(cost, nan=100.0, posinf=100.0, neginf=-100.0)
    out = np.full((NL, B, K), -1, np.int32)
    lo = 0
    for b in range(B):
        if G[b] and K:
            for l in range(NL):
                rows, cols = linear_sum_assignment(cost[l][:, lo:lo + G[b]])
                out[l, b, rows] = cols
        lo += G[b]
    return out


MATCHERS = ("host", "device")


def _matcher(what: str, matcher: str, scores=None, gt_bboxes: Sequence = ()) -> str:
    """``matcher`` checked; with the operands: the device solver's limits on every scene, from the shapes alone (before any launch)."""
    if matcher not in MATCHERS:
        raise ValueError(f"{what}: matcher must be 'host' or 'device', got {matcher!r}")
    if matcher == "device" and scores is not None and scores.dim() == 4:
        K = int(scores.shape[2])
        for b, g in enumerate(gt_bboxes):
            G = int((g.tensor if hasattr(g, "tensor") else g).shape[0])
            if min(K, G) > SAP_MAX_ROWS or max(K, G) > SAP_MAX_COLS:
                raise ValueError(f"{what}: matcher='device' takes min(K, G_b) <= {SAP_MAX_ROWS} and max(K, G_b) <= {SAP_MAX_COLS}, got K={K}, "
                                 f"G_b={G} in scene {b}; use matcher='host'")
    return matcher


def hungarian_assign(scores: torch.Tensor, boxes: torch.Tensor, text_token_mask: torch.Tensor, gt_bboxes: Sequence[torch.Tensor],
                     positive_maps: Sequence[torch.Tensor], alpha: float = 0.25, gamma: float = 2.0, weights=(1.0, 2.0, 2.0),
                     _targets: Optional[_Targets] = None, matcher: str = "host") -> torch.Tensor:
    """``assign (NL,B,K) int32`` on the device: the index of the matched ground-truth box within its scene, -1 for an unmatched query.
    ``matcher='host'``: one launch, one device-to-host copy through pinned memory, ONE synchronise, scipy per (layer, scene), one copy
    back.  ``matcher='device'``: two launches (``ptx_gl_cost``, ``ptx_gl_assign``), no copy and no synchronise; ``min(K, G_b) <= 256`` and
    ``max(K, G_b) <= 1024`` in every scene, else ``ValueError``; the matching of ``grounding_loss_host.sap_assign_host``, which has
    scipy's total cost and, off ties, scipy's pairs.  A scene without a box assigns -1 everywhere; ``G_b > K`` matches ``K`` pairs."""
    _matcher("hungarian_assign", matcher, scores, gt_bboxes)
    with torch.no_grad():
        if matcher == "device" and _targets is None and scores.dim() == 4:      # (the offsets of the second launch: built once)
            _gpu("hungarian_assign", scores)
            _targets = _Targets("hungarian_assign", gt_bboxes, positive_maps, int(scores.shape[1]), int(scores.shape[3]), scores.device)
        cost, G = match_costs(scores, boxes, text_token_mask, gt_bboxes, positive_maps, alpha, gamma, weights, _targets)
        dev, (NL, K, SG) = cost.device, cost.shape
        B = len(G)
        if K == 0 or SG == 0:
            return torch.full((NL, B, K), -1, dtype=torch.int32, device=dev)
        if matcher == "device":
            assign = torch.empty((NL, B, K), dtype=torch.int32, device=dev)
            _abi.check(_abi.lib().ptx_gl_assign(cost.data_ptr(), NL, B, K, _targets.offset_ptr, SG, max(G), assign.data_ptr(), _stream(dev)),
                       "ptx_gl_assign")
            return assign
        host = torch.empty(cost.shape, dtype=torch.float32, pin_memory=True)
        host.copy_(cost, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()         # the stage's one synchronise
        back = torch.from_numpy(_solve(host.numpy(), G, B)).pin_memory()
        return back.to(dev, non_blocking=True)


class _LossFn(torch.autograd.Function):
    """``(scores, boxes) -> losses (2,NL)``: row 0 the classification loss of every layer, row 1 the box loss."""

    @staticmethod
    def forward(ctx, scores, boxes, mask, tg, assign, alpha, gamma, dw, cls_scale, box_weight):
        dev = scores.device
        NL, B, K, M = (int(s) for s in scores.shape)
        s, bx = _f32(scores, "grounding_loss", dev), _f32(boxes, "grounding_loss", dev)
        rows = torch.empty((2, NL, B, K), dtype=torch.float32, device=dev)
        losses = torch.empty((2, NL), dtype=torch.float32, device=dev)
        counts = torch.empty((NL,), dtype=torch.int32, device=dev)
        dwa = (ctypes.c_float * 4)(*dw)
        _abi.check(_abi.lib().ptx_gl_loss_fwd(s.data_ptr(), bx.data_ptr(), NL, B, K, M, mask.data_ptr(), int(mask.shape[1]), tg.boxes.data_ptr(),
                                              tg.maps.data_ptr(), tg.offset_ptr, tg.SG, assign.data_ptr(), alpha, gamma, dwa, cls_scale,
                                              box_weight, rows.data_ptr(), losses.data_ptr(), counts.data_ptr(), _stream(dev)),
                   "ptx_gl_loss_fwd")
        ctx.saved = (s, bx, mask, tg, assign, counts)
        ctx.consts = (alpha, gamma, dwa, cls_scale, box_weight)
        return losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        s, bx, mask, tg, assign, counts = ctx.saved
        alpha, gamma, dwa, cls_scale, box_weight = ctx.consts
        dev = s.device
        NL, B, K, M = (int(v) for v in s.shape)
        g = _f32_grad(g.detach())
        dscores, dboxes = torch.empty_like(s), torch.empty_like(bx)
        _abi.check(_abi.lib().ptx_gl_loss_bwd(s.data_ptr(), bx.data_ptr(), NL, B, K, M, mask.data_ptr(), int(mask.shape[1]), tg.boxes.data_ptr(),
                                              tg.maps.data_ptr(), tg.offset_ptr, tg.SG, assign.data_ptr(), alpha, gamma, dwa, cls_scale,
                                              box_weight, g.data_ptr(), g.data_ptr() + 4 * NL, counts.data_ptr(), dscores.data_ptr(),
                                              dboxes.data_ptr(), _stream(dev)), "ptx_gl_loss_bwd")
        return (dscores if ctx.needs_input_grad[0] else None, dboxes if ctx.needs_input_grad[1] else None) + (None,) * 8


def grounding_loss(scores: torch.Tensor, boxes: torch.Tensor, text_token_mask: torch.Tensor, gt_bboxes: Sequence[torch.Tensor],
                   positive_maps: Sequence[torch.Tensor], assign: torch.Tensor, avg_factor: Optional[float] = None, alpha: float = 0.25,
                   gamma: float = 2.0, decouple_weights=(0.2, 0.2, 0.2, 0.4), loss_weights=(1.0, 1.0),
                   _targets: Optional[_Targets] = None) -> torch.Tensor:
    """``losses (2,NL)``: ``losses[0][l]`` the sigmoid focal loss of layer l over the unmasked tokens of every query divided by
    ``avg_factor + float32 eps`` (default: ``max(sum_b min(K, G_b), 1)``), ``losses[1][l]`` the four Chamfer terms of its matched pairs,
    weighted by ``decouple_weights``, as a mean over ``8 P`` corners -- one autograd node with gradients to ``scores`` and ``boxes``
    (``grounding_loss_host.loss_host``; ``ptx_gl_loss_fwd`` / ``ptx_gl_loss_bwd``).  ``assign (NL,B,K) int32`` as ``hungarian_assign``
    returns it; an entry ``>= G_b`` or ``< -1`` is an unmatched query.  Raises ``ValueError`` before any launch when no scene has a
    ground-truth box.  A layer whose ``assign`` holds no pair, in a batch that has ground truth, gets NaN as its ``losses[1][l]`` (the mean
    of nothing, which is what the reference returns); its ``dboxes`` are exactly 0, its classification loss and every other layer are
    untouched."""
    NL, B, K, M, T, mask = _operands("grounding_loss", scores, boxes, text_token_mask)
    dev = scores.device
    alpha, gamma = _focal_args("grounding_loss", alpha, gamma)
    tg = _targets or _Targets("grounding_loss", gt_bboxes, positive_maps, B, M, dev)
    num_pos = sum(min(K, g) for g in tg.G)
    if num_pos == 0:
        raise ValueError("grounding_loss: no matched pair in the batch (no scene has a ground-truth box, or there is no query); the "
                         "reference returns NaN here")
    if len(decouple_weights) != 4:
        raise ValueError(f"grounding_loss: four decouple_weights expected, got {len(decouple_weights)}")
    if assign.dtype != torch.int32 or tuple(assign.shape) != (NL, B, K) or not assign.is_contiguous() or assign.device != dev:
        raise ValueError(f"grounding_loss: assign must be contiguous int32 ({NL},{B},{K}) on {dev}, got {assign.dtype} {tuple(assign.shape)}")
    avg = max(float(num_pos), 1.0) if avg_factor is None else float(avg_factor)
    return _LossFn.apply(_f32_grad(scores), _f32_grad(boxes), mask, tg, assign, alpha, gamma, tuple(float(w) for w in decouple_weights),
                         float(loss_weights[0]) / (avg + F32_EPS), float(loss_weights[1]))


def predict_scores(scores: torch.Tensor) -> torch.Tensor:
    """``(...,) fp32 = max_t sigmoid(scores[..., t])`` over all columns: a ``-inf`` column gives 0, never NaN
    (``grounding_loss_host.predict_host``; ``ptx_gl_predict``, one launch)."""
    _gpu("predict_scores", scores)
    dev = scores.device
    s = _f32(scores, "predict_scores", dev)
    M = int(s.shape[-1])
    if s.dim() < 2 or not 1 <= M <= MAX_TEXT:
        raise ValueError(f"predict_scores: scores (...,M) with 1 <= M <= {MAX_TEXT} expected, got {tuple(s.shape)}")
    out = torch.empty(tuple(s.shape[:-1]), dtype=torch.float32, device=dev)
    if out.numel():
        _abi.check(_abi.lib().ptx_gl_predict(s.data_ptr(), out.numel(), M, out.data_ptr(), _stream(dev)), "ptx_gl_predict")
    return out


def _average_over_ranks(value: float, dev) -> float:
    """mmdet's ``reduce_mean`` of a host count: the mean over the ranks of an initialised process group, else the value."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return value
    t = torch.tensor([value], dtype=torch.float32, device=dev)
    dist.all_reduce(t.div_(dist.get_world_size()))
    return float(t.item())


_FOCAL, _CHAMFER = ("mmdet.FocalLoss", "FocalLoss"), ("BBoxCDLoss",)
_COSTS = ("BinaryFocalLossCost", "BBox3DL1Cost", "IoU3DCost")


class GroundingLoss(nn.Module):
    """The loss side of ``GroundingHead``, with its keyword arguments; the defaults are the shipped configuration's
    (configs/grounding/*.py): ``decouple_bbox_loss=True, decouple_groups=4, decouple_weights=[.2,.2,.2,.4]``, ``mmdet.FocalLoss(use_sigmoid,
    gamma 2, alpha .25)``, ``BBoxCDLoss(mode='l1', group='g8')`` and ``HungarianAssigner3D`` with ``BinaryFocalLossCost`` 1.0,
    ``BBox3DL1Cost`` 2.0 and ``IoU3DCost`` 2.0.  It has no parameters (the branches live in ``QuerySelect`` and ``GroundingDecoder``).

    ``loss(all_layers_cls_scores (NL,B,K,max_text_len), all_layers_pred_bboxes (NL,B,K,9), text_token_mask (B,T), gt_bboxes: list of
    (G_b,9), positive_maps: list of (G_b,max_text_len))`` returns the reference's dict: ``loss_cls``, ``loss_bbox`` (the last layer) and
    ``d{i}.loss_cls``, ``d{i}.loss_bbox`` for the layers ``0 .. NL-2``.  ``assign(...)`` (same arguments) returns the matching alone,
    ``(NL,B,K) int32``.  ``matcher`` (keyword only): ``'host'`` (the default: scipy behind the stage's one synchronise) or ``'device'``
    (``ptx_gl_assign``: ``loss`` then enqueues cost, matching and loss and returns without a host wait; ``min(K, G_b) <= 256`` and
    ``max(K, G_b) <= 1024``, else ``ValueError``).  ``predict(all_layers_cls_scores, all_layers_pred_bboxes)`` is ``predict_by_feat``:
    ``(bboxes_3d (B,K,9), scores_3d (B,K))`` of the last layer.

    With ``sync_cls_avg_factor=True`` and ``torch.distributed`` initialised, the number of matched pairs is averaged over the ranks for
    the classification divisor, as ``reduce_mean`` does.  Raises ``NotImplementedError`` with the argument's name on what is not built:
    ``norm_decouple_loss=True``, ``decouple_groups=3``, ``group='g4'``, a ``mode`` other than ``'l1'``, a ``loss_cls`` that is not the
    sigmoid focal loss, other match costs, ``num_reg=12``, ``box_coder='FCAF'``."""

    def __init__(self, num_classes: int = 256, embed_dims: int = 256, num_pred_layer: int = 7, num_reg_fcs: int = 2, num_reg: int = 9,
                 box_coder: str = "baseline", sync_cls_avg_factor: bool = True, decouple_bbox_loss: bool = True, decouple_groups: int = 4,
                 decouple_weights: Optional[Sequence[float]] = (0.2, 0.2, 0.2, 0.4), norm_decouple_loss: bool = False,
                 loss_cls: Optional[dict] = None, loss_bbox: Optional[dict] = None, train_cfg: Optional[dict] = None,
                 contrastive_cfg: Optional[dict] = None, share_pred_layer: bool = True, test_cfg=None, init_cfg=None, *,
                 matcher: str = "host"):
        super().__init__()
        who = "GroundingLoss"
        self.matcher = _matcher(who, matcher)
        if int(num_reg) == 12:
            raise NotImplementedError(f"{who}: num_reg=12 (the 6D rotation) is not implemented; num_reg=9")
        if int(num_reg) != 9:
            raise ValueError(f"{who}: num_reg must be 9 (or 12, not implemented), got {num_reg}")
        if box_coder == "FCAF":
            raise NotImplementedError(f"{who}: box_coder='FCAF' is not implemented; 'baseline'")
        if box_coder != "baseline":
            raise ValueError(f"{who}: box_coder must be 'baseline' or 'FCAF', got {box_coder!r}")
        if norm_decouple_loss:
            raise NotImplementedError(f"{who}: norm_decouple_loss=True is not implemented")
        if decouple_bbox_loss and int(decouple_groups) == 3:
            raise NotImplementedError(f"{who}: decouple_groups=3 is not implemented; decouple_groups=4")
        if decouple_bbox_loss and int(decouple_groups) != 4:
            raise ValueError(f"{who}: decouple_groups must be 4 (or 3, not implemented), got {decouple_groups}")
        loss_cls = dict(type="mmdet.FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0) if loss_cls is None else dict(loss_cls)
        loss_bbox = dict(type="BBoxCDLoss", mode="l1", loss_weight=1.0, group="g8") if loss_bbox is None else dict(loss_bbox)
        if loss_cls.get("type") not in _FOCAL or not loss_cls.get("use_sigmoid", False) or loss_cls.get("reduction", "mean") != "mean":
            raise NotImplementedError(f"{who}: loss_cls must be the sigmoid focal loss (type 'mmdet.FocalLoss', use_sigmoid=True, "
                                      f"reduction 'mean'), got {loss_cls!r}")
        if loss_bbox.get("type") not in _CHAMFER or loss_bbox.get("reduction", "mean") != "mean":
            raise NotImplementedError(f"{who}: loss_bbox must be BBoxCDLoss with reduction 'mean', got {loss_bbox!r}")
        if loss_bbox.get("mode", "l2") != "l1":
            raise NotImplementedError(f"{who}: loss_bbox mode={loss_bbox.get('mode', 'l2')!r} is not implemented; mode='l1'")
        if loss_bbox.get("group", "g8") != "g8":
            raise NotImplementedError(f"{who}: loss_bbox group={loss_bbox.get('group')!r} is not implemented; group='g8'")
        if train_cfg is None:
            train_cfg = dict(assigner=dict(type="HungarianAssigner3D", match_costs=[dict(type="BinaryFocalLossCost", weight=1.0),
                                                                                     dict(type="BBox3DL1Cost", weight=2.0),
                                                                                     dict(type="IoU3DCost", weight=2.0)]))
        assigner = dict(train_cfg).get("assigner") or {}
        costs = list(assigner.get("match_costs", []))
        if assigner.get("type") != "HungarianAssigner3D" or tuple(c.get("type") for c in costs) != _COSTS:
            raise NotImplementedError(f"{who}: train_cfg must name HungarianAssigner3D with the match_costs {_COSTS} in this order, got "
                                      f"{assigner!r}")
        extra = {k for k in costs[0] if k not in ("type", "weight", "alpha", "gamma", "eps", "binary_input")}
        if extra or costs[0].get("binary_input") or costs[0].get("eps", 1e-12) != 1e-12:
            raise NotImplementedError(f"{who}: match_costs BinaryFocalLossCost takes weight, alpha and gamma (eps 1e-12), got {costs[0]!r}")
        contrastive_cfg = dict(max_text_len=256) if contrastive_cfg is None else dict(contrastive_cfg)
        self.max_text_len = int(contrastive_cfg.get("max_text_len", 256))
        if not 1 <= self.max_text_len <= MAX_TEXT:
            raise ValueError(f"{who}: max_text_len must be 1 to {MAX_TEXT}, got {self.max_text_len}")
        self.num_classes, self.embed_dims, self.num_pred_layer, self.num_reg_fcs = int(num_classes), int(embed_dims), int(num_pred_layer), int(num_reg_fcs)
        self.num_reg, self.box_coder, self.share_pred_layer = int(num_reg), box_coder, bool(share_pred_layer)
        self.sync_cls_avg_factor, self.decouple_bbox_loss, self.decouple_groups = bool(sync_cls_avg_factor), bool(decouple_bbox_loss), int(decouple_groups)
        self.norm_decouple_loss, self.bg_cls_weight = False, 0
        if not self.decouple_bbox_loss:
            self.decouple_weights = [0.0, 0.0, 0.0, 1.0]      # the full prediction alone
        elif decouple_weights is None:
            self.decouple_weights = [0.25] * 4
        else:
            self.decouple_weights = [float(w) for w in decouple_weights]
            if len(self.decouple_weights) != 4:
                raise ValueError(f"{who}: four decouple_weights expected, got {len(self.decouple_weights)}")
        self.loss_cls_cfg, self.loss_bbox_cfg, self.train_cfg, self.contrastive_cfg, self.test_cfg = loss_cls, loss_bbox, train_cfg, contrastive_cfg, test_cfg
        self.alpha, self.gamma = _focal_args(who, loss_cls.get("alpha", 0.25), loss_cls.get("gamma", 2.0))
        self.loss_weights = (float(loss_cls.get("loss_weight", 1.0)), float(loss_bbox.get("loss_weight", 1.0)))
        self.cost_alpha, self.cost_gamma = _focal_args(who, costs[0].get("alpha", 0.25), costs[0].get("gamma", 2.0))
        self.cost_weights = tuple(float(c.get("weight", 1.0)) for c in costs)

    def _targets(self, scores, boxes, mask, gt_bboxes, positive_maps) -> _Targets:
        NL, B, K, M, T, _ = _operands("GroundingLoss", scores, boxes, mask)
        if M != self.max_text_len:
            raise ValueError(f"GroundingLoss: scores with max_text_len={self.max_text_len} columns expected, got {M}")
        return _Targets("GroundingLoss", gt_bboxes, positive_maps, B, M, scores.device)

    def assign(self, all_layers_cls_scores, all_layers_pred_bboxes, text_token_mask, gt_bboxes, positive_maps, _targets=None) -> torch.Tensor:
        _matcher("GroundingLoss", self.matcher, all_layers_cls_scores, gt_bboxes)
        tg = _targets or self._targets(all_layers_cls_scores, all_layers_pred_bboxes, text_token_mask, gt_bboxes, positive_maps)
        return hungarian_assign(all_layers_cls_scores, all_layers_pred_bboxes, text_token_mask, gt_bboxes, positive_maps, self.cost_alpha,
                                self.cost_gamma, self.cost_weights, tg, self.matcher)

    def loss(self, all_layers_cls_scores, all_layers_pred_bboxes, text_token_mask, gt_bboxes, positive_maps) -> dict:
        scores, boxes = all_layers_cls_scores, all_layers_pred_bboxes
        _matcher("GroundingLoss", self.matcher, scores, gt_bboxes)
        tg = self._targets(scores, boxes, text_token_mask, gt_bboxes, positive_maps)
        K = int(scores.shape[2])
        num_pos = sum(min(K, g) for g in tg.G)
        if num_pos == 0:
            raise ValueError("GroundingLoss: no matched pair in the batch (no scene has a ground-truth box, or there is no query); the "
                             "reference returns NaN here")
        assign = self.assign(scores, boxes, text_token_mask, gt_bboxes, positive_maps, tg)
        avg = float(num_pos)
        if self.sync_cls_avg_factor:
            avg = _average_over_ranks(avg, scores.device)
        # (the reference averages the same count once more for the box branch and never reads it: its Chamfer mean is over 8 P corners)
        losses = grounding_loss(scores, boxes, text_token_mask, gt_bboxes, positive_maps, assign, max(avg, 1.0), self.alpha, self.gamma,
                                self.decouple_weights, self.loss_weights, tg)
        NL = int(scores.shape[0])
        out = {"loss_cls": losses[0, NL - 1], "loss_bbox": losses[1, NL - 1]}
        for i in range(NL - 1):
            out[f"d{i}.loss_cls"], out[f"d{i}.loss_bbox"] = losses[0, i], losses[1, i]
        return out

    forward = loss

    def predict(self, all_layers_cls_scores, all_layers_pred_bboxes):
        if all_layers_cls_scores.dim() != 4 or tuple(all_layers_pred_bboxes.shape) != tuple(all_layers_cls_scores.shape[:3]) + (9,):
            raise ValueError(f"GroundingLoss.predict: scores (NL,B,K,M) and boxes (NL,B,K,9) expected, got "
                             f"{tuple(all_layers_cls_scores.shape)}, {tuple(all_layers_pred_bboxes.shape)}")
        with torch.no_grad():
            return all_layers_pred_bboxes[-1], predict_scores(all_layers_cls_scores[-1])
