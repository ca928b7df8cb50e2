"""The numpy restatement of the transformer decoder behind the query selection (``SparseFeatureFusionTransformerDecoder``,
models/layers/ground_transformer/decoder.py, and the per-layer text scores of ``GroundingHead.forward``): the specification the kernels of
``decoder.py`` (``csrc/decoder.hip``) are held to.  Imports only numpy and ``query_select_host``; every function computes in the dtype of
its first floating operand.

The rules of mmcv's ``MultiheadAttention`` wrapper as read from its source: the output is ``identity + attention`` with the identity the
query BEFORE its positions are added; positions go to ``q`` and ``k`` only, never to ``v``; when ``key_pos`` is None and
``query_pos.shape == key.shape`` the keys receive ``query_pos`` -- in the text cross attention that happens exactly when ``T == K``.

Parity-unpinned against ``nn.MultiheadAttention``: a masked key is never read, so a NaN or inf under it leaves no trace (torch multiplies
it by a zero weight and gets NaN).  A query whose every key is masked gets zeros from the attention (torch 2.10 gives zeros as well;
older releases give NaN)."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from .query_select_host import boxes_host

__all__ = ["attention_host", "contrastive_scores_host", "fold_posembed", "forward_host", "layer_norm_host", "linear_add_ln_host",
           "linear_host", "posembed_host"]

LN_EPS = 1e-5


def fold_posembed(conv1_w, conv1_b, bn_w, bn_b, bn_mean, bn_var, bn_eps: float = 1e-5):
    """Eval BatchNorm folded into the first Conv1d(k=1), in float64: ``(w1 (C,cin), b1 (C))`` with ``bn(conv(x)) = x @ w1.T + b1``."""
    s = np.asarray(bn_w, np.float64) / np.sqrt(np.asarray(bn_var, np.float64) + float(bn_eps))
    w = np.asarray(conv1_w, np.float64).reshape(len(s), -1) * s[:, None]
    b = (np.asarray(conv1_b, np.float64) - np.asarray(bn_mean, np.float64)) * s + np.asarray(bn_b, np.float64)
    return w, b


def posembed_host(x, w1, b1, w2, b2) -> np.ndarray:
    """``relu(x @ w1.T + b1) @ w2.T + b2`` on ``x (...,cin)`` with the folded first layer; the ReLU keeps a NaN."""
    x = np.asarray(x)
    dt = x.dtype
    h = np.maximum((x @ np.asarray(w1, dt).T + np.asarray(b1, dt)).astype(dt, copy=False), dt.type(0))
    return (h @ np.asarray(w2, dt).reshape(h.shape[-1], -1).T + np.asarray(b2, dt)).astype(dt, copy=False)


def linear_host(x, weight, bias=None, add=None, relu: bool = False, add_cols: Optional[int] = None) -> np.ndarray:
    """``act((x + add) @ weight.T + bias)``; ``add_cols``: the add reaches the output columns below it only.  ReLU keeps a NaN."""
    x = np.asarray(x)
    dt = x.dtype
    w = np.asarray(weight, dt)
    if add is None or add_cols == 0:
        out = x @ w.T
    elif add_cols is None or add_cols >= w.shape[0]:
        out = (x + np.asarray(add, dt)) @ w.T
    else:
        out = np.concatenate([(x + np.asarray(add, dt)) @ w[:add_cols].T, x @ w[add_cols:].T], axis=-1)
    out = out.astype(dt, copy=False)
    if bias is not None:
        out = out + np.asarray(bias, dt)
    return np.maximum(out, dt.type(0)) if relu else out


def layer_norm_host(x, weight, bias, eps: float = LN_EPS) -> np.ndarray:
    """LayerNorm over the last axis: the mean first, then the centred squares."""
    x = np.asarray(x)
    dt = x.dtype
    d = x - x.mean(axis=-1, keepdims=True, dtype=dt)
    var = (d * d).mean(axis=-1, keepdims=True, dtype=dt)
    return (d / np.sqrt(var + dt.type(eps)) * np.asarray(weight, dt) + np.asarray(bias, dt)).astype(dt, copy=False)


def linear_add_ln_host(x, weight, bias, residual, ln, ln2=None):
    """``LayerNorm(x @ weight.T + bias + residual)`` with ``ln = (weight, bias)``; with ``ln2`` also ``LayerNorm2`` of that result:
    ``(out, out2)``."""
    y = linear_host(x, weight, bias) + np.asarray(residual, np.asarray(x).dtype)
    out = layer_norm_host(y, *ln)
    return out if ln2 is None else (out, layer_norm_host(out, *ln2))


def attention_host(q, k, v, mask, num_heads: int) -> np.ndarray:
    """``(B,Kq,C)``: per head ``softmax((q / sqrt(hd)) k^T) v`` over the keys with ``mask[b,l]`` False.  Masked keys and values are
    replaced by zeros before any arithmetic (never read); a query without a key gets zeros."""
    q = np.asarray(q)
    dt = q.dtype
    B, Kq, C = q.shape
    L, H = np.asarray(k).shape[1], int(num_heads)
    hd = C // H
    mask = np.asarray(mask, bool)
    keep = ~mask[:, :, None]
    k = np.where(keep, np.asarray(k, dt), dt.type(0)).reshape(B, L, H, hd).transpose(0, 2, 1, 3)
    v = np.where(keep, np.asarray(v, dt), dt.type(0)).reshape(B, L, H, hd).transpose(0, 2, 1, 3)
    qh = (q * dt.type(1.0 / math.sqrt(hd))).reshape(B, Kq, H, hd).transpose(0, 2, 1, 3)
    s = np.matmul(qh, k.transpose(0, 1, 3, 2)).astype(dt, copy=False)
    s = np.where(mask[:, None, None, :], dt.type(-np.inf), s)
    with np.errstate(invalid="ignore", over="ignore"):
        m = s.max(axis=-1, keepdims=True) if L else np.full(s.shape[:-1] + (1,), -np.inf, dt)
        m = np.where(np.isneginf(m), dt.type(0), m)
        p = np.exp(s - m).astype(dt, copy=False)
        l = p.sum(axis=-1, keepdims=True, dtype=dt)
        o = np.matmul(p, v).astype(dt, copy=False)
        o = np.where(l == 0, dt.type(0), o / np.where(l == 0, dt.type(1), l))
    return o.transpose(0, 2, 1, 3).reshape(B, Kq, C).astype(dt, copy=False)


def contrastive_scores_host(hidden_states, text_feats, text_token_mask, bias=None, scaled: bool = True, max_text_len: int = 256):
    """``ContrastiveEmbed`` on every layer: ``(NL,B,K,max_text_len)``, ``-inf`` on masked tokens and from ``T`` on."""
    hs = np.asarray(hidden_states)
    dt = hs.dtype
    text = np.asarray(text_feats, dt)
    tmask = np.asarray(text_token_mask, bool)
    s = np.matmul(hs, np.swapaxes(text, 1, 2)[None]).astype(dt, copy=False)
    if scaled:
        s = s / dt.type(math.sqrt(hs.shape[-1]))
    if bias is not None:
        s = s + np.asarray(bias, dt).reshape(-1)[0]
    s = np.where(tmask[None, :, None, :], s, dt.type(-np.inf)).astype(dt, copy=False)
    out = np.full(s.shape[:-1] + (int(max_text_len),), -np.inf, dt)
    out[..., :s.shape[-1]] = s
    return out


def _mha(p: dict, prefix: str, query, key, value, query_pos, key_pos, mask, H: int, dt):
    """mmcv's wrapper around ``nn.MultiheadAttention``: ``identity + out_proj(attention)``; the projections as three Linears of
    ``in_proj_weight``'s row blocks."""
    C = query.shape[-1]
    w, b = np.asarray(p[prefix + "in_proj_weight"], dt), np.asarray(p[prefix + "in_proj_bias"], dt)
    q = linear_host(query if query_pos is None else query + query_pos, w[:C], b[:C])
    k = linear_host(key if key_pos is None else key + key_pos, w[C:2 * C], b[C:2 * C])
    v = linear_host(value, w[2 * C:], b[2 * C:])
    o = attention_host(q, k, v, mask, H)
    return query + linear_host(o, p[prefix + "out_proj.weight"], p[prefix + "out_proj.bias"])


def forward_host(params: dict, num_layers: int, num_heads: Sequence[int], query, key, key_padding_mask, query_coords, key_coords,
                 pred_bboxes, text_feats, text_attention_mask, reg_weights: Sequence, reg_biases: Sequence, dtype=np.float64,
                 return_intermediate: bool = True, text_keys_take_pos: Optional[bool] = None):
    """The decoder's eval forward in numpy ``dtype``.  ``params``: the module's ``state_dict`` as arrays (the reference's names);
    ``num_heads = (self, text, scene)``; ``reg_weights[lid]`` / ``reg_biases[lid]``: the Linears of layer ``lid``'s regression branch.
    ``text_keys_take_pos``: overrides mmcv's rule (``T == K``) for the text keys, for the test that isolates it.  Returns ``(hidden_states (NL,B,K,C), boxes (NL,B,K,9))``, or the last layer's un-normed query and boxes."""
    dt = np.dtype(dtype)
    P = {n: np.asarray(a, np.float64) for n, a in params.items() if not n.endswith("num_batches_tracked")}
    cast = lambda a: np.asarray(a, dt)                       # noqa: E731

    def posembed(name, x):
        h = name + ".position_embedding_head."
        w1, b1 = fold_posembed(P[h + "0.weight"], P[h + "0.bias"], P[h + "1.weight"], P[h + "1.bias"], P[h + "1.running_mean"],
                               P[h + "1.running_var"])
        return posembed_host(x, cast(w1), cast(b1), cast(P[h + "3.weight"]), cast(P[h + "3.bias"]))

    query, key, text = cast(query), cast(key), cast(text_feats)
    qcoords, boxes = cast(query_coords), cast(pred_bboxes)
    pad, tmask = np.asarray(key_padding_mask, bool), np.asarray(text_attention_mask, bool)
    key_pos = posembed("cross_posembed", cast(key_coords))
    hidden, all_boxes = [], []
    for lid in range(int(num_layers)):
        pre = f"layers.{lid}."
        ln = lambda i: (cast(P[f"{pre}norms.{i}.weight"]), cast(P[f"{pre}norms.{i}.bias"]))      # noqa: E731
        query_pos = posembed("self_posembed", boxes)
        query = layer_norm_host(_mha(P, pre + "self_attn.attn.", query, query, query, query_pos, query_pos,
                                     np.zeros(query.shape[:2], bool), num_heads[0], dt), *ln(0))
        take = query_pos.shape == text.shape if text_keys_take_pos is None else bool(text_keys_take_pos)      # mmcv's key_pos default: T == K
        text_pos = query_pos if take else None
        query = layer_norm_host(_mha(P, pre + "cross_attn_text.attn.", query, text, text, query_pos, text_pos, tmask, num_heads[1], dt), *ln(1))
        query = layer_norm_host(_mha(P, pre + "cross_attn.attn.", query, key, key, query_pos, key_pos, pad, num_heads[2], dt), *ln(2))
        h = linear_host(query, P[pre + "ffn.layers.0.0.weight"], P[pre + "ffn.layers.0.0.bias"], relu=True)
        query = layer_norm_host(query + linear_host(h, P[pre + "ffn.layers.1.weight"], P[pre + "ffn.layers.1.bias"]), *ln(3))
        boxes = boxes_host(query, qcoords, [cast(w) for w in reg_weights[lid]], [cast(b) for b in reg_biases[lid]])
        hidden.append(layer_norm_host(query, cast(P["norm.weight"]), cast(P["norm.bias"])))
        all_boxes.append(boxes)
    if not return_intermediate:
        return query, boxes
    C = query.shape[-1]
    if not hidden:
        return np.zeros((0,) + query.shape, dt), np.zeros((0,) + query.shape[:2] + (9,), dt)
    return np.stack(hidden).reshape((-1,) + query.shape[:2] + (C,)), np.stack(all_boxes)
