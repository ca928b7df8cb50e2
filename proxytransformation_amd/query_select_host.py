"""The numpy restatement of the query selection behind the neck (``pre_decoder``, detectors/sparse_featfusion_grounder_preshape.py:498-580):
the specification the kernels of ``query_select.py`` (``csrc/query_select.hip``) are held to, bit for bit resp. to fp32 rounding.
Imports only numpy and ``neck_host``; every function computes in the dtype of its first floating operand.

Parity-unpinned against torch: the tie rule of the sorted top-k (``torch.topk`` leaves the order of equal scores unspecified; here the
lower row index comes first) and the place of a NaN whose sign bit is set (``neck_host.topk_key`` puts it below ``-inf``, torch treats
every NaN as the largest value)."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from .neck_host import topk_key

__all__ = ["backward_host", "boxes_host", "forward_host", "pack_host", "score_host", "topk_sorted_host"]

SIZE_MIN = 0.02                    # `.clamp(min=2e-2)` of _bbox_pred_to_bbox


def pack_host(feats_list: Sequence, xyz_list: Sequence):
    """``(feats (B,Lmax,C), coords (B,Lmax,3), pad_mask (B,Lmax) bool)``: scene b's rows at ``[b, :L_b]``, zeros behind them, the mask True
    on padding."""
    B, Lmax = len(feats_list), max(int(np.asarray(f).shape[0]) for f in feats_list)
    f0 = np.asarray(feats_list[0])
    feats = np.zeros((B, Lmax, f0.shape[1]), f0.dtype)
    coords = np.zeros((B, Lmax, 3), np.asarray(xyz_list[0]).dtype)
    pad = np.ones((B, Lmax), bool)
    for b, (f, p) in enumerate(zip(feats_list, xyz_list)):
        n = int(np.asarray(f).shape[0])
        feats[b, :n], coords[b, :n], pad[b, :n] = f, p, False
    return feats, coords, pad


def score_host(feats, pad_mask, text_feats, text_token_mask, bias=None, scaled: bool = True) -> np.ndarray:
    """``ContrastiveEmbed(...).max(-1)[0]``: ``(B,Lmax)`` with ``s[b,r,t] = feats[b,r] . text[b,t] (/ sqrt(C)) (+ bias)`` and the maximum
    over the tokens with ``text_token_mask[b,t]``; ``-inf`` on padded rows and in a scene without a token.  The maximum is numpy's: a NaN
    among a row's unmasked ``s`` makes its score NaN, as ``torch.max`` does."""
    feats = np.asarray(feats)
    dt = feats.dtype
    text = np.asarray(text_feats, dt)
    tmask = np.asarray(text_token_mask, bool)
    s = np.matmul(feats, np.swapaxes(text, 1, 2)).astype(dt, copy=False)
    if scaled:
        s = s / dt.type(math.sqrt(feats.shape[2]))
    if bias is not None:
        s = s + np.asarray(bias, dt).reshape(-1)[0]
    s = np.where(tmask[:, None, :], s, dt.type(-np.inf)).astype(dt, copy=False)
    with np.errstate(invalid="ignore"):
        out = s.max(axis=2)
    return np.where(np.asarray(pad_mask, bool), dt.type(-np.inf), out).astype(dt, copy=False)


def topk_sorted_host(score, rows: Sequence[int], k: int) -> np.ndarray:
    """``torch.topk(score, k, dim=1, sorted=True)[1]`` over the rows ``0 .. rows[b] - 1`` of every scene: ``(B,k)`` int64 in descending
    ``neck_host.topk_key``, the lower row first among equal keys (parity-unpinned against torch, like the place of a sign-set NaN)."""
    score = np.asarray(score)
    out = np.empty((score.shape[0], int(k)), np.int64)
    for b, n in enumerate(int(r) for r in rows):
        if n < k:
            raise ValueError(f"topk_sorted_host: scene {b} has {n} rows, fewer than k={k}")
        out[b] = np.argsort(~topk_key(score[b, :n]), kind="stable")[:int(k)]
    return out


def boxes_host(query, coords, weights: Sequence, biases: Sequence) -> np.ndarray:
    """The regression branch (Linear + ReLU per hidden layer, a last Linear to 9 values) on ``query (...,C)`` and the baseline decode with
    ``coords (...,3)``: ``center = p[0:3] + coords``, ``size = max(exp(p[3:6]), 0.02)``, ``euler = p[6:9]``.  ``weights[i]`` is
    ``(out,in)`` as ``nn.Linear`` holds it.  ReLU and the clamp are numpy's ``maximum``: a NaN stays NaN."""
    h = np.asarray(query)
    dt = h.dtype
    for i, (w, b) in enumerate(zip(weights, biases)):
        h = (h @ np.asarray(w, dt).T + np.asarray(b, dt)).astype(dt, copy=False)
        if i + 1 < len(weights):
            h = np.maximum(h, dt.type(0))
    if h.shape[-1] != 9:
        raise NotImplementedError(f"boxes_host: the baseline decode of 9 values, got {h.shape[-1]}")
    with np.errstate(over="ignore"):
        size = np.maximum(np.exp(h[..., 3:6]), dt.type(SIZE_MIN))
    return np.concatenate([h[..., 0:3] + np.asarray(coords, dt), size, h[..., 6:9]], axis=-1).astype(dt, copy=False)


def forward_host(feats_list, xyz_list, text_feats, text_token_mask, weights, biases, cls_bias=None, scaled: bool = True,
                 num_queries: int = 256, dtype=np.float64, index: Optional[np.ndarray] = None, keep_out: Optional[dict] = None):
    """The whole stage in numpy ``dtype``: ``(decoder_inputs_dict, head_inputs_dict)`` of arrays with the reference's keys.  ``index``
    ``(B,K)``: replaces the host's own selection -- the device's, when a test holds the device's outputs on the device's rows.
    ``keep_out``: a dict that receives ``score (B,Lmax)`` and the host's OWN ``index (B,K)``."""
    dt = np.dtype(dtype)
    feats_list = [np.asarray(f, dt) for f in feats_list]
    xyz_list = [np.asarray(p, dt) for p in xyz_list]
    rows = [f.shape[0] for f in feats_list]
    text = np.asarray(text_feats, dt)
    tmask = np.asarray(text_token_mask, bool)
    feats, coords, pad = pack_host(feats_list, xyz_list)
    score = score_host(feats, pad, text, tmask, None if cls_bias is None else np.asarray(cls_bias, dt), scaled)
    K = min(int(num_queries), min(rows))
    own = topk_sorted_host(score, rows, K)
    if keep_out is not None:
        keep_out.update(score=score, index=own)
    idx = own if index is None else np.asarray(index, np.int64).reshape(len(rows), K)
    take = idx[:, :, None]
    query = np.take_along_axis(feats, take, axis=1)
    qcoords = np.take_along_axis(coords, take, axis=1)
    boxes = boxes_host(query, qcoords, [np.asarray(w, dt) for w in weights], [np.asarray(b, dt) for b in biases])
    dec = dict(query=query, feats=feats, feats_attention_mask=pad, query_coords=qcoords, feats_coords=coords, pred_bboxes=boxes,
               text_feats=text, text_attention_mask=~tmask)
    return dec, dict(text_feats=text, text_token_mask=tmask)


def backward_host(dfeats, dquery, index, rows: Sequence[int]) -> list:
    """The gradients of the per-scene features behind ``(feats, query)``: ``d_b[r] = dfeats[b, r]``, plus ``dquery[b, q]`` where
    ``index[b, q] = r`` (one add; a scene's indices are distinct).  Either gradient may be ``None`` (zeros).  Rows that were not selected
    are pure copies."""
    ref = dfeats if dfeats is not None else dquery
    dt, C = np.asarray(ref).dtype, np.asarray(ref).shape[2]
    out = []
    for b, n in enumerate(int(r) for r in rows):
        d = np.array(np.asarray(dfeats)[b, :n], dt) if dfeats is not None else np.zeros((n, C), dt)
        if dquery is not None:
            i = np.asarray(index)[b]
            d[i] = d[i] + np.asarray(dquery, dt)[b]
        out.append(d)
    return out
