"""The numpy restatement of the backward of the decoder's operators -- the flash attention, the fused Linear and the (double) LayerNorm of
``decoder.py`` with ``differentiable=True`` (``csrc/decoder_bwd.hip``; the Linear over ``ptx_op_gemm`` / ``ptx_op_colsum``) and, from
``csrc/decoder_train.hip``, the position embedding with a training-mode BatchNorm (forward with its running-statistics rule, and
backward), the box head's backward and the text scores' backward: the specification the gradients are held to.  Imports only numpy and
``decoder_host``; every function computes in the dtype of its first floating operand.

The mask rules are the forward's (``decoder_host.attention_host``): masked keys and values are replaced by zeros before any arithmetic
(never read) and get zero gradients; a query without a key has zero probabilities, so it passes nothing on and gets a zero ``dq``."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from .decoder_host import LN_EPS, linear_host

__all__ = ["attention_bwd_host", "boxes_bwd_host", "decoder_train_host", "layer_norm_bwd_host", "linear_bwd_host", "posembed_train_bwd_host", "posembed_train_host",
           "scores_bwd_host"]


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


# ------------------------------------------------------------------------------------------------------------------ training position embedding
def _pe_parts(x, conv1_w, conv1_b, bn_w, bn_b, eps):
    """The rows, ``z = x W1^T + b1``, its batch mean, centred values, centred sum of squares and ``rstd`` (biased variance), the
    normalised ``zhat`` and the value in front of the ReLU."""
    x = np.asarray(x)
    dt = x.dtype
    w1 = np.asarray(conv1_w, dt)
    w1 = w1.reshape(w1.shape[0], -1)
    x2 = x.reshape(-1, w1.shape[1])
    n = x2.shape[0]
    if n < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    z = (x2 @ w1.T + np.asarray(conv1_b, dt)).astype(dt, copy=False)
    mean = z.mean(axis=0, dtype=dt)
    d = z - mean
    m2 = (d * d).sum(axis=0, dtype=dt)
    rstd = (1 / np.sqrt(m2 / dt.type(n) + dt.type(eps))).astype(dt, copy=False)
    zhat = d * rstd
    pre = (zhat * np.asarray(bn_w, dt) + np.asarray(bn_b, dt)).astype(dt, copy=False)
    return x2, w1, n, mean, m2, rstd, zhat, pre


def posembed_train_host(x, conv1_w, conv1_b, bn_w, bn_b, conv2_w, conv2_b, eps: float = 1e-5, running_mean=None, running_var=None,
                        momentum: float = 0.1, repeat: int = 1):
    """``PositionEmbeddingLearned`` under ``.train()`` on ``x (...,cin)``: ``(out (...,C), (mean, rstd), (running_mean, running_var))``.
    The BatchNorm takes the statistics of ALL rows it is given (padding rows included): the mean first, then the centred squares, the
    biased variance ``M2 / n`` to normalise.  The running statistics move ``repeat`` times, one call after the other on the same rows:
    ``r = (1 - momentum) r + momentum v`` with the batch mean and the unbiased variance ``M2 / (n - 1)``; the caller adds ``repeat`` to
    ``num_batches_tracked``.  One row is refused as torch refuses it.  The ReLU keeps a NaN."""
    x2, w1, n, mean, m2, rstd, zhat, pre = _pe_parts(x, conv1_w, conv1_b, bn_w, bn_b, eps)
    dt = x2.dtype
    h = np.maximum(pre, dt.type(0))
    w2 = np.asarray(conv2_w, dt)
    out = (h @ w2.reshape(w2.shape[0], -1).T + np.asarray(conv2_b, dt)).astype(dt, copy=False)
    running = None
    if running_mean is not None:
        rm, rv = np.array(running_mean, dt), np.array(running_var, dt)
        unbiased = m2 / dt.type(n - 1)
        for _ in range(int(repeat)):
            rm = (dt.type(1) - dt.type(momentum)) * rm + dt.type(momentum) * mean
            rv = (dt.type(1) - dt.type(momentum)) * rv + dt.type(momentum) * unbiased
        running = (rm, rv)
    return out.reshape(np.asarray(x).shape[:-1] + (out.shape[-1],)), (mean, rstd), running


def posembed_train_bwd_host(x, conv1_w, conv1_b, bn_w, bn_b, conv2_w, dout, eps: float = 1e-5) -> dict:
    """The gradients of ``posembed_train_host`` under ``dout (...,C)``: ``dconv1_w (C,cin)``, ``dconv1_b``, ``dbn_w``, ``dbn_b``,
    ``dconv2_w (C,C)``, ``dconv2_b``; ``x`` gets none.  ``dh = dout W2``; ``dpre = dh`` where the value in front of the ReLU is ``> 0`` (a
    NaN passes nothing); ``dbeta = sum dpre``, ``dgamma = sum dpre zhat``; ``dz = gamma rstd (dpre - dbeta / n - zhat dgamma / n)``;
    ``dW1 = dz^T x``, ``db1 = sum dz`` (zero in exact arithmetic: a bias in front of batch statistics)."""
    x2, w1, n, mean, m2, rstd, zhat, pre = _pe_parts(x, conv1_w, conv1_b, bn_w, bn_b, eps)
    dt = x2.dtype
    C = w1.shape[0]
    g = np.asarray(dout, dt).reshape(-1, C)
    w2 = np.asarray(conv2_w, dt).reshape(C, C)
    h = np.maximum(pre, dt.type(0))
    dpre = np.where(pre > 0, (g @ w2).astype(dt, copy=False), dt.type(0))
    dbeta = dpre.sum(axis=0, dtype=dt)
    dgamma = (dpre * zhat).sum(axis=0, dtype=dt)
    dz = (np.asarray(bn_w, dt) * rstd) * (dpre - dbeta / dt.type(n) - zhat * (dgamma / dt.type(n)))
    return dict(dconv1_w=(dz.T @ x2).astype(dt, copy=False), dconv1_b=dz.sum(axis=0, dtype=dt), dbn_w=dgamma, dbn_b=dbeta,
                dconv2_w=(g.T @ h).astype(dt, copy=False), dconv2_b=g.sum(axis=0, dtype=dt))


# ------------------------------------------------------------------------------------------------------------------ boxes, scores
def boxes_bwd_host(h, weight, bias, dboxes) -> dict:
    """The gradients of ``query_select_host.boxes_host``'s last Linear and decode under ``dboxes (...,9)``: ``dh``, ``dweight (9,C)``,
    ``dbias (9)``; the coordinates get none.  With ``p = h W^T + b`` recomputed: ``dp = d`` on the centre and the angles and
    ``dp = (exp(p) >= 0.02 ? d : 0) * exp(p)`` on the sizes -- what torch's autograd gives for ``exp(p).clamp(min=0.02)``: the clamp passes
    the gradient where ``exp(p) >= 0.02`` (on the clamp itself too) and zero elsewhere, exp multiplies by its own result.  So a NaN ``p``
    gives NaN (``0 * NaN``), ``p = +inf`` gives ``d * inf`` and ``p = -inf`` gives 0."""
    h = np.asarray(h)
    dt = h.dtype
    w = np.asarray(weight, dt)
    C = w.shape[1]
    h2, d = h.reshape(-1, C), np.asarray(dboxes, dt).reshape(-1, 9)
    p = (h2 @ w.T).astype(dt, copy=False)
    if bias is not None:
        p = p + np.asarray(bias, dt)
    dp = d.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(p[:, 3:6]).astype(dt, copy=False)
        dp[:, 3:6] = np.where(e >= dt.type(0.02), d[:, 3:6], dt.type(0)) * e
    res = dict(dh=(dp @ w).astype(dt, copy=False).reshape(h.shape), dweight=(dp.T @ h2).astype(dt, copy=False))
    if bias is not None:
        res["dbias"] = dp.sum(axis=0, dtype=dt)
    return res


def scores_bwd_host(hidden_states, text_feats, text_token_mask, dscores, has_bias: bool = False, scaled: bool = True) -> dict:
    """The gradients of ``decoder_host.contrastive_scores_host`` under ``dscores (NL,B,K,max_text_len)``: ``dhidden (NL,B,K,C)``,
    ``dtext (B,T,C)`` and, with a bias, ``dbias`` (a scalar).  ``dscores`` counts on the tokens ``t < T`` with ``text_token_mask[b,t]``
    only and is replaced by zeros elsewhere before any arithmetic (never read: the forward wrote ``-inf`` there and a loss may leave a
    NaN under it)."""
    hs = np.asarray(hidden_states)
    dt = hs.dtype
    text = np.asarray(text_feats, dt)
    tmask = np.asarray(text_token_mask, bool)
    T = text.shape[1]
    ds = np.where(tmask[None, :, None, :], np.asarray(dscores, dt)[..., :T], dt.type(0))
    dhidden = np.matmul(ds, text[None]).astype(dt, copy=False)
    dtext = np.einsum("lbkt,lbkc->btc", ds, hs).astype(dt, copy=False)
    if scaled:
        div = dt.type(math.sqrt(hs.shape[-1]))
        dhidden, dtext = dhidden / div, dtext / div
    res = dict(dhidden=dhidden, dtext=dtext)
    if has_bias:
        res["dbias"] = ds.sum(dtype=dt)
    return res


# ------------------------------------------------------------------------------------------------------------------ the whole training chain
def _mha_fwd(P, prefix, query, key_in, value_in, qpos, kpos, mask, H, dt):
    from .decoder_host import attention_host
    C = query.shape[-1]
    w, b = np.asarray(P[prefix + "in_proj_weight"], dt), np.asarray(P[prefix + "in_proj_bias"], dt)
    wo, bo = np.asarray(P[prefix + "out_proj.weight"], dt), np.asarray(P[prefix + "out_proj.bias"], dt)
    xq = query if qpos is None else query + qpos
    xk = key_in if kpos is None else key_in + kpos
    q, k, v = linear_host(xq, w[:C], b[:C]), linear_host(xk, w[C:2 * C], b[C:2 * C]), linear_host(value_in, w[2 * C:], b[2 * C:])
    o = attention_host(q, k, v, mask, H)
    return query + linear_host(o, wo, bo), (prefix, xq, xk, value_in, q, k, v, o, mask, H, w, b, wo, bo)


def _mha_bwd(cache, dy, grads):
    """``(d xq, d xk, d value_in)`` of the projections' operands; the identity's share (``dy`` itself) is the caller's."""
    prefix, xq, xk, xv, q, k, v, o, mask, H, w, b, wo, bo = cache
    C = xq.shape[-1]
    r = linear_bwd_host(o, wo, dy, bias=bo)
    dq, dk, dv = attention_bwd_host(q, k, v, mask, H, r["dx"])
    rq, rk, rv = (linear_bwd_host(x, w[i * C:(i + 1) * C], g, bias=b[i * C:(i + 1) * C]) for i, (x, g) in enumerate(((xq, dq), (xk, dk), (xv, dv))))
    _acc(grads, prefix + "in_proj_weight", np.concatenate([rq["dweight"], rk["dweight"], rv["dweight"]]))
    _acc(grads, prefix + "in_proj_bias", np.concatenate([rq["dbias"], rk["dbias"], rv["dbias"]]))
    _acc(grads, prefix + "out_proj.weight", r["dweight"])
    _acc(grads, prefix + "out_proj.bias", r["dbias"])
    return rq["dx"], rk["dx"], rv["dx"]


def _acc(grads, name, g):
    grads[name] = g if name not in grads else grads[name] + g


def decoder_train_host(params: dict, num_layers: int, num_heads, query, key, key_padding_mask, query_coords, key_coords, pred_bboxes,
                       text_feats, text_attention_mask, reg_weights, reg_biases, G, dtype=np.float64, return_intermediate: bool = True,
                       bn_eps: float = 1e-5):
    """One training step of the decoder in numpy ``dtype``: the chain of ``decoder_host.forward_host`` with both position embeddings
    on batch statistics (``cross_posembed`` on the same rows in every layer, so once), the boxes detached between layers, and the
    backward of ``loss = sum(out0 * G[0]) + sum(out1 * G[1])`` composed from this module's operator gradients.  ``params``: the module's
    ``state_dict`` as arrays.  Returns ``(out, grads)``: ``grads`` under the parameters' names (``reg.{layer}.{2 i}.weight`` / ``.bias``
    for the i-th Linear of a regression branch) and ``query``, ``key``, ``text_feats``.  No gradient goes to the coordinates or
    ``pred_bboxes``."""
    from .decoder_host import layer_norm_host
    dt = np.dtype(dtype)
    P = {n: np.asarray(a, dt) for n, a in params.items() if not n.endswith("num_batches_tracked")}
    cast = lambda a: np.asarray(a, dt)                       # noqa: E731
    query, key, text, qcoords, boxes = cast(query), cast(key), cast(text_feats), cast(query_coords), cast(pred_bboxes)
    pad, tmask = np.asarray(key_padding_mask, bool), np.asarray(text_attention_mask, bool)
    NL, C = int(num_layers), query.shape[-1]
    pe = lambda name: [P[name + ".position_embedding_head." + k] for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias")]      # noqa: E731
    ln = lambda pre, i: (P[f"{pre}norms.{i}.weight"], P[f"{pre}norms.{i}.bias"])      # noqa: E731
    key_pos = posembed_train_host(cast(key_coords), *pe("cross_posembed"), eps=bn_eps)[0]
    take = text.shape[1] == query.shape[1]                   # mmcv: the text keys take query_pos when T == K
    no_mask = np.zeros(query.shape[:2], bool)
    caches, hidden, all_boxes = [], [], []
    for lid in range(NL):
        pre = f"layers.{lid}."
        c = dict(boxes=boxes, query=query)
        query_pos = posembed_train_host(boxes, *pe("self_posembed"), eps=bn_eps)[0]
        c["pre0"], c["sa"] = _mha_fwd(P, pre + "self_attn.attn.", query, query, query, query_pos, query_pos, no_mask, num_heads[0], dt)
        q1 = layer_norm_host(c["pre0"], *ln(pre, 0))
        c["pre1"], c["ta"] = _mha_fwd(P, pre + "cross_attn_text.attn.", q1, text, text, query_pos, query_pos if take else None, tmask,
                                      num_heads[1], dt)
        q2 = layer_norm_host(c["pre1"], *ln(pre, 1))
        c["pre2"], c["ca"] = _mha_fwd(P, pre + "cross_attn.attn.", q2, key, key, query_pos, key_pos, pad, num_heads[2], dt)
        q3 = layer_norm_host(c["pre2"], *ln(pre, 2))
        c["q3"] = q3
        c["h"] = linear_host(q3, P[pre + "ffn.layers.0.0.weight"], P[pre + "ffn.layers.0.0.bias"], relu=True)
        c["pre3"] = q3 + linear_host(c["h"], P[pre + "ffn.layers.1.weight"], P[pre + "ffn.layers.1.bias"])
        query = layer_norm_host(c["pre3"], *ln(pre, 3))
        acts = [query]
        for w, b in zip(reg_weights[lid][:-1], reg_biases[lid][:-1]):
            acts.append(linear_host(acts[-1], cast(w), cast(b), relu=True))
        c["acts"] = acts
        p = linear_host(acts[-1], cast(reg_weights[lid][-1]), cast(reg_biases[lid][-1]))
        with np.errstate(over="ignore"):
            boxes = np.concatenate([p[..., :3] + qcoords, np.maximum(np.exp(p[..., 3:6]), dt.type(0.02)), p[..., 6:]], axis=-1).astype(dt, copy=False)
        hidden.append(layer_norm_host(query, P["norm.weight"], P["norm.bias"]))
        all_boxes.append(boxes)
        caches.append(c)
    out = (np.stack(hidden), np.stack(all_boxes)) if return_intermediate else (query, boxes)
    Gh, Gb = cast(G[0]), cast(G[1])
    grads = {}
    dkey, dtext, dkey_pos = np.zeros_like(key), np.zeros_like(text), np.zeros_like(key_pos)
    dnext = None if return_intermediate else Gh              # the gradient of a layer's result as the next layer's query
    for lid in reversed(range(NL)):
        pre, c = f"layers.{lid}.", caches[lid]
        gb = Gb[lid] if return_intermediate else (Gb if lid == NL - 1 else None)
        dq4 = np.zeros_like(c["query"]) if dnext is None else dnext
        if gb is not None:                                   # the boxes: decode, last Linear, the branch's hidden Linears
            ws, bs, acts = reg_weights[lid], reg_biases[lid], c["acts"]
            r = boxes_bwd_host(acts[-1], cast(ws[-1]), cast(bs[-1]), gb)
            n_lin = len(ws)
            _acc(grads, f"reg.{lid}.{2 * (n_lin - 1)}.weight", r["dweight"])
            _acc(grads, f"reg.{lid}.{2 * (n_lin - 1)}.bias", r["dbias"])
            g = r["dh"]
            for i in reversed(range(n_lin - 1)):
                r = linear_bwd_host(acts[i], cast(ws[i]), g, bias=cast(bs[i]), relu=True, out=acts[i + 1])
                _acc(grads, f"reg.{lid}.{2 * i}.weight", r["dweight"])
                _acc(grads, f"reg.{lid}.{2 * i}.bias", r["dbias"])
                g = r["dx"]
            dq4 = dq4 + g
        if return_intermediate:
            r = layer_norm_bwd_host(c["pre3"], ln(pre, 3), dq4, (P["norm.weight"], P["norm.bias"]), Gh[lid])
            _acc(grads, "norm.weight", r["dweight2"])
            _acc(grads, "norm.bias", r["dbias2"])
        else:
            r = layer_norm_bwd_host(c["pre3"], ln(pre, 3), dq4)
        _acc(grads, pre + "norms.3.weight", r["dweight"])
        _acc(grads, pre + "norms.3.bias", r["dbias"])
        dy = r["dx"]
        r2 = linear_bwd_host(c["h"], P[pre + "ffn.layers.1.weight"], dy, bias=P[pre + "ffn.layers.1.bias"])
        r1 = linear_bwd_host(c["q3"], P[pre + "ffn.layers.0.0.weight"], r2["dx"], bias=P[pre + "ffn.layers.0.0.bias"], relu=True, out=c["h"])
        for name, rr in (("ffn.layers.1.", r2), ("ffn.layers.0.0.", r1)):
            _acc(grads, pre + name + "weight", rr["dweight"])
            _acc(grads, pre + name + "bias", rr["dbias"])
        dq = dy + r1["dx"]
        dqpos = None
        for i, name in ((2, "ca"), (1, "ta"), (0, "sa")):
            r = layer_norm_bwd_host(c[f"pre{i}"], ln(pre, i), dq)
            _acc(grads, f"{pre}norms.{i}.weight", r["dweight"])
            _acc(grads, f"{pre}norms.{i}.bias", r["dbias"])
            dxq, dxk, dxv = _mha_bwd(c[name], r["dx"], grads)
            dq = r["dx"] + dxq
            dqpos = dxq if dqpos is None else dqpos + dxq
            if name == "ca":
                dkey, dkey_pos = dkey + dxk + dxv, dkey_pos + dxk
            elif name == "ta":
                dtext = dtext + dxk + dxv
                if take:
                    dqpos = dqpos + dxk
            else:
                dq, dqpos = dq + dxk + dxv, dqpos + dxk
        w1, b1, g_, b_, w2, _ = pe("self_posembed")
        r = posembed_train_bwd_host(c["boxes"], w1, b1, g_, b_, w2, dqpos, bn_eps)
        for k, n in (("dconv1_w", "0.weight"), ("dconv1_b", "0.bias"), ("dbn_w", "1.weight"), ("dbn_b", "1.bias"), ("dconv2_w", "3.weight"),
                     ("dconv2_b", "3.bias")):
            _acc(grads, "self_posembed.position_embedding_head." + n, r[k].reshape(P["self_posembed.position_embedding_head." + n].shape))
        dnext = dq
    w1, b1, g_, b_, w2, _ = pe("cross_posembed")
    r = posembed_train_bwd_host(cast(key_coords), w1, b1, g_, b_, w2, dkey_pos, bn_eps)
    for k, n in (("dconv1_w", "0.weight"), ("dconv1_b", "0.bias"), ("dbn_w", "1.weight"), ("dbn_b", "1.bias"), ("dconv2_w", "3.weight"),
                 ("dconv2_b", "3.bias")):
        grads["cross_posembed.position_embedding_head." + n] = r[k].reshape(P["cross_posembed.position_embedding_head." + n].shape)
    grads.update(query=dnext, key=dkey, text_feats=dtext)
    return out, grads
