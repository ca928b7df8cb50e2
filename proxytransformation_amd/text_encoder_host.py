"""The numpy specification of ``text_encoder.py``: the eval forward of ``CLIPTextModel`` up to ``last_hidden_state``, stage by stage as
``csrc/text_encoder.hip`` launches it.  Every array is of the ``dtype`` asked for (float64: the reference the device is held to; float32:
the yardstick of its error).  It calls no device code and needs only numpy.

The rules it states:

* an id outside ``[0, vocab)`` reads no table row: its embedding row is NaN;
* LayerNorm: the row mean first, then the centred variance; ``(x - mean) * (1 / sqrt(var + eps)) * weight + bias``;
* quick-GELU: ``v / (1 + exp(-1.702 v))``;
* attention: ``q`` scaled by ``1/8`` (head dimension 64); key ``j`` is admitted for query ``t`` iff ``j <= t`` and ``mask[b, j]``; a key that
  is not admitted is never read (a NaN under it leaves no trace -- parity-unpinned: torch adds ``-inf`` to its logit and multiplies its
  value by a zero weight); a query without an admitted key gets zeros (parity-unpinned: it cannot occur with ``mask[b, 0]`` true);
  all ``T`` query rows are computed, padded ones too;
* pre-norm layers: ``x = x + out_proj(attention(LN1(x)))``, ``x = x + fc2(quick_gelu(fc1(LN2(x))))``; ``final_layer_norm`` at the end."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

__all__ = ["attention_host", "embed_host", "forward_host", "layer_norm_host", "linear_host", "ln_linear_host", "quick_gelu_host",
           "row_stats_host"]

HEAD_DIM = 64


def embed_host(ids: np.ndarray, token_embedding: np.ndarray, position_embedding: np.ndarray) -> np.ndarray:
    """``(B,T,C)``: ``token_embedding[ids[b,t]] + position_embedding[t]``; NaN rows where the id is outside the table."""
    ids = np.asarray(ids).astype(np.int64)
    B, T = ids.shape
    ok = (ids >= 0) & (ids < token_embedding.shape[0])
    x = token_embedding[np.where(ok, ids, 0)] + position_embedding[None, :T]
    x[~ok] = np.nan
    return x


def row_stats_host(x: np.ndarray, eps: float):
    """``(mean, rstd)`` of every row, each of ``x.shape[:-1]``: the row mean first, then ``1 / sqrt(var + eps)`` of the centred variance --
    what ``ptx_txt_ln_linear`` leaves in ``stats[:, 0]`` and ``stats[:, 1]``."""
    dt = x.dtype
    mean = x.mean(-1, keepdims=True, dtype=dt)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True, dtype=dt)
    rstd = dt.type(1.0) / np.sqrt(var + dt.type(eps))
    return mean[..., 0], rstd[..., 0]


def layer_norm_host(x: np.ndarray, weight: np.ndarray, bias: np.ndarray, eps: float) -> np.ndarray:
    mean, rstd = row_stats_host(x, eps)
    return (x - mean[..., None]) * rstd[..., None] * weight + bias


def quick_gelu_host(v: np.ndarray) -> np.ndarray:
    dt = v.dtype
    return v / (dt.type(1.0) + np.exp(dt.type(-1.702) * v))


def ln_linear_host(x: np.ndarray, ln_w: np.ndarray, ln_b: np.ndarray, eps: float, w: np.ndarray, bias: Optional[np.ndarray],
                   act: int) -> np.ndarray:
    """``act(LayerNorm(x) @ w^T + bias)`` (``ptx_txt_ln_linear``): ``w (Cout,Cin)``, ``bias (Cout)`` or None; act 0: none, 1: quick-GELU."""
    v = layer_norm_host(x, ln_w, ln_b, eps) @ w.T
    if bias is not None:
        v = v + bias
    return quick_gelu_host(v) if act else v


def linear_host(x: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray], residual: Optional[np.ndarray]) -> np.ndarray:
    """``x @ w^T + bias + residual`` in that order (``ptx_txt_linear``): ``w (Cout,Cin)``; ``bias (Cout)`` and ``residual`` may be None."""
    v = x @ w.T
    if bias is not None:
        v = v + bias
    return v if residual is None else v + residual


def attention_host(qkv: np.ndarray, mask: Optional[np.ndarray], num_heads: int) -> np.ndarray:
    """``(B,T,C)`` from ``qkv (B,T,3 C) = [q|k|v]`` and ``mask (B,T)`` bool (True = a token; None: all): causal, heads of 64 merged in the
    output.  Only the admitted keys of a query are indexed."""
    dt = qkv.dtype
    B, T, C3 = qkv.shape
    C, H = C3 // 3, int(num_heads)
    q = (qkv[..., :C] * dt.type(0.125)).reshape(B, T, H, HEAD_DIM)
    k = qkv[..., C:2 * C].reshape(B, T, H, HEAD_DIM)
    v = qkv[..., 2 * C:].reshape(B, T, H, HEAD_DIM)
    out = np.zeros((B, T, H, HEAD_DIM), dt)
    for b in range(B):
        valid = np.ones(T, bool) if mask is None else np.asarray(mask[b], bool)
        for t in range(T):
            adm = np.nonzero(valid[:t + 1])[0]
            if adm.size == 0:
                continue                                    # no admitted key: zeros
            s = np.einsum("hd,jhd->hj", q[b, t], k[b, adm])
            p = np.exp(s - s.max(-1, keepdims=True))
            out[b, t] = np.einsum("hj,jhd->hd", p, v[b, adm]) / p.sum(-1, keepdims=True, dtype=dt)
    return out.reshape(B, T, C)


def forward_host(params: Dict[str, np.ndarray], input_ids, attention_mask, num_heads: int, eps: float = 1e-5,
                 dtype=np.float64, prefix: str = "text_model.") -> np.ndarray:
    """``last_hidden_state (B,T,C)`` in ``dtype`` from ``params`` under ``CLIPTextModel``'s names (``prefix`` + ``embeddings...``)."""
    dt = np.dtype(dtype)
    P = lambda name: np.asarray(params[prefix + name]).astype(dt)      # noqa: E731
    ids = np.asarray(input_ids)
    mask = None if attention_mask is None else np.asarray(attention_mask).astype(bool)
    x = embed_host(ids, P("embeddings.token_embedding.weight"), P("embeddings.position_embedding.weight"))
    layers = 0
    while f"{prefix}encoder.layers.{layers}.layer_norm1.weight" in params:
        layers += 1
    for i in range(layers):
        L = lambda name, i=i: P(f"encoder.layers.{i}.{name}")      # noqa: E731
        w = np.concatenate([L("self_attn.q_proj.weight"), L("self_attn.k_proj.weight"), L("self_attn.v_proj.weight")])
        bq = np.concatenate([L("self_attn.q_proj.bias"), L("self_attn.k_proj.bias"), L("self_attn.v_proj.bias")])
        a = attention_host(ln_linear_host(x, L("layer_norm1.weight"), L("layer_norm1.bias"), eps, w, bq, 0), mask, num_heads)
        x = linear_host(a, L("self_attn.out_proj.weight"), L("self_attn.out_proj.bias"), x)
        h = ln_linear_host(x, L("layer_norm2.weight"), L("layer_norm2.bias"), eps, L("mlp.fc1.weight"), L("mlp.fc1.bias"), 1)
        x = linear_host(h, L("mlp.fc2.weight"), L("mlp.fc2.bias"), x)
    out = layer_norm_host(x, P("final_layer_norm.weight"), P("final_layer_norm.bias"), eps)
    assert out.dtype == dt
    return out
