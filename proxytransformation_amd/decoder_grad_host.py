"""The numpy restatement of the backward of the decoder's operators -- the flash attention, the fused Linear and the (double) LayerNorm of
``decoder.py`` with ``differentiable=True`` (``csrc/decoder_bwd.hip``; the Linear over ``ptx_op_gemm`` / ``ptx_op_colsum``): the
specification the gradients are held to.  Imports only numpy and ``decoder_host``; every function computes in the dtype of its first
floating operand.

The mask rules are the forward's (``decoder_host.attention_host``): masked keys and values are replaced by zeros before any arithmetic
(never read) and get zero gradients; a query without a key has zero probabilities, so it passes nothing on and gets a zero ``dq``."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from .decoder_host import LN_EPS, linear_host

__all__ = ["attention_bwd_host", "layer_norm_bwd_host", "linear_bwd_host"]


def attention_bwd_host(q, k, v, mask, num_heads: int, dout):
    """``(dq (B,Kq,C), dk (B,L,C), dv (B,L,C))`` of ``decoder_host.attention_host(q, k, v, mask, num_heads)`` under ``dout (B,Kq,C)``:
    with ``P = softmax((q / sqrt(hd)) k^T)`` over the unmasked keys, ``D = rowsum(dO * O)``, ``dP = dO v^T``, ``dS = P (dP - D)``:
    ``dv = P^T dO``, ``dq = dS k / sqrt(hd)``, ``dk = dS^T (q / sqrt(hd))``."""
    q = np.asarray(q)
    dt = q.dtype
    B, Kq, C = q.shape
    L, H = np.asarray(k).shape[1], int(num_heads)
    hd = C // H
    mask = np.zeros((B, L), bool) if mask is None else np.asarray(mask, bool)
    keep = ~mask[:, :, None]
    scale = dt.type(1.0 / math.sqrt(hd))
    heads = lambda t, n: t.reshape(B, n, H, hd).transpose(0, 2, 1, 3)      # noqa: E731
    merge = lambda t, n: t.transpose(0, 2, 1, 3).reshape(B, n, C).astype(dt, copy=False)      # noqa: E731
    kh = heads(np.where(keep, np.asarray(k, dt), dt.type(0)), L)
    vh = heads(np.where(keep, np.asarray(v, dt), dt.type(0)), L)
    qh = heads(q * scale, Kq)
    do = heads(np.asarray(dout, dt), Kq)
    s = np.matmul(qh, kh.transpose(0, 1, 3, 2)).astype(dt, copy=False)
    s = np.where(mask[:, None, None, :], dt.type(-np.inf), s)
    with np.errstate(invalid="ignore", over="ignore"):
        m = s.max(axis=-1, keepdims=True) if L else np.full(s.shape[:-1] + (1,), -np.inf, dt)
        m = np.where(np.isneginf(m), dt.type(0), m)
        e = np.exp(s - m).astype(dt, copy=False)
        l = e.sum(axis=-1, keepdims=True, dtype=dt)
        p = np.where(l == 0, dt.type(0), e / np.where(l == 0, dt.type(1), l)).astype(dt, copy=False)
    o = np.matmul(p, vh).astype(dt, copy=False)
    D = (do * o).sum(axis=-1, keepdims=True, dtype=dt)
    dv = np.matmul(p.transpose(0, 1, 3, 2), do).astype(dt, copy=False)
    dp = np.matmul(do, vh.transpose(0, 1, 3, 2)).astype(dt, copy=False)
    ds = np.where(mask[:, None, None, :], dt.type(0), p * (dp - D)).astype(dt, copy=False)
    dq = np.matmul(ds, kh).astype(dt, copy=False) * scale
    dk = np.matmul(ds.transpose(0, 1, 3, 2), qh).astype(dt, copy=False)
    dk, dv = merge(dk, L), merge(dv, L)
    return merge(dq, Kq), np.where(keep, dk, dt.type(0)), np.where(keep, dv, dt.type(0))


def linear_bwd_host(x, weight, dy, bias=None, add=None, relu: bool = False, add_cols: Optional[int] = None, residual: bool = False,
                    out=None) -> dict:
    """The gradients of ``decoder_host.linear_host(x, weight, bias, add, relu, add_cols) (+ residual)`` under ``dy``: a dict with
    ``dx``, ``dweight`` and, where the operand exists, ``dadd``, ``dbias``, ``dresidual``.  ``out``: the forward's result, whose sign is
    the ReLU's mask (``dy * (out > 0)``: a NaN passes nothing); recomputed when missing.  The weight rows below ``add_cols`` see
    ``x + add`` (rounded as the forward rounds it), the others ``x``."""
    x = np.asarray(x)
    dt = x.dtype
    w = np.asarray(weight, dt)
    cout, cin = w.shape
    dy = np.asarray(dy, dt)
    cols = 0 if add is None else (cout if add_cols is None else int(add_cols))
    g = dy
    if relu:
        if out is None:
            out = linear_host(x, w, bias, add, True, add_cols)
        g = np.where(np.asarray(out) > 0, dy, dt.type(0))
    g2, x2 = g.reshape(-1, cout), x.reshape(-1, cin)
    res = dict(dx=(g2 @ w).astype(dt, copy=False).reshape(x.shape))
    xa = x2 if add is None else (x2 + np.asarray(add, dt).reshape(-1, cin))
    res["dweight"] = np.concatenate([g2[:, :cols].T @ xa, g2[:, cols:].T @ x2], axis=0).astype(dt, copy=False)
    if add is not None:
        res["dadd"] = (g2[:, :cols] @ w[:cols]).astype(dt, copy=False).reshape(x.shape)
    if bias is not None:
        res["dbias"] = g2.sum(axis=0, dtype=dt)
    if residual:
        res["dresidual"] = dy
    return res


def _ln_parts(x, weight, bias, eps):
    dt = x.dtype
    d = x - x.mean(axis=-1, keepdims=True, dtype=dt)
    den = np.sqrt((d * d).mean(axis=-1, keepdims=True, dtype=dt) + dt.type(eps))
    xhat = d / den
    return xhat, den, (xhat * weight + bias).astype(dt, copy=False)


def _ln_back(g, xhat, den, weight):
    dt = xhat.dtype
    gw = g * weight
    m1 = gw.mean(axis=-1, keepdims=True, dtype=dt)
    m2 = (gw * xhat).mean(axis=-1, keepdims=True, dtype=dt)
    return ((gw - m1 - xhat * m2) / den).astype(dt, copy=False)


def layer_norm_bwd_host(x, ln, dy=None, ln2=None, dy2=None, eps: float = LN_EPS) -> dict:
    """The gradients of ``layer_norm_host(x, *ln)`` under ``dy`` -- ``dx``, ``dweight``, ``dbias`` -- and, with ``ln2``, of the pair
    ``out = LN(x)``, ``out2 = LN2(out)`` under ``(dy, dy2)``, either of which may be None: ``dx = LN^T(dy + LN2^T(dy2))``, also
    ``dweight2``, ``dbias2``.  ``ln``, ``ln2``: ``(weight, bias)``.  The mean first, then the centred squares, as the forward."""
    x = np.asarray(x)
    dt = x.dtype
    C = x.shape[-1]
    w, b = np.asarray(ln[0], dt), np.asarray(ln[1], dt)
    xhat, den, y = _ln_parts(x, w, b, eps)
    g = np.zeros_like(x) if dy is None else np.asarray(dy, dt)
    res = {}
    if ln2 is not None:
        w2, b2 = np.asarray(ln2[0], dt), np.asarray(ln2[1], dt)
        g2 = np.zeros_like(x) if dy2 is None else np.asarray(dy2, dt)
        yhat, den2, _ = _ln_parts(y, w2, b2, eps)
        res["dweight2"] = (yhat * g2).reshape(-1, C).sum(axis=0, dtype=dt)
        res["dbias2"] = g2.reshape(-1, C).sum(axis=0, dtype=dt)
        g = g + _ln_back(g2, yhat, den2, w2)
    res["dweight"] = (xhat * g).reshape(-1, C).sum(axis=0, dtype=dt)
    res["dbias"] = g.reshape(-1, C).sum(axis=0, dtype=dt)
    res["dx"] = _ln_back(g, xhat, den, w)
    return res
