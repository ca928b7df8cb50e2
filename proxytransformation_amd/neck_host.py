"""The numpy restatements of the sparse neck's operations: the specification the kernels of ``neck.py`` (``csrc/neck.hip`` and the neck
instantiations of ``csrc/sparse.hip``) are held to, bit for bit resp. to fp32 rounding.  Imports only numpy and ``sparse_host``; it plays
the role ``sparse_host.py`` plays for the backbone's layers.  Rows, scene ends and tensor strides are ``sparse.py``'s.

Where a rule is OUR READING of MinkowskiEngine -- which is not available to check against -- it is "parity-unpinned against ME itself":
the offset order of the generative transposed convolution (``kernel_offsets``), the order of the union's rows, the treatment of absent
corners in ``features_at_coordinates`` (no renormalisation), and the tie rule of the top-k (``torch.topk`` leaves it unspecified)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from .sparse_host import kernel_offsets, sparse_conv3d_host

__all__ = ["ACT_NONE", "ACT_RELU", "ACT_ELU", "act_host", "conv_transpose_gen_bwd_host", "conv_transpose_gen_host", "head_bwd_host",
           "head_host", "prune_dest_host", "prune_host", "prune_scores_host", "rows_gather_host", "sparse_conv3d_act_host", "topk_keep_host",
           "topk_key", "topk_scene_rows", "union_add_host", "union_dest_host"]

ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2


def act_host(x: np.ndarray, act: int) -> np.ndarray:
    """The activation selector of the neck's convolutions: 0 none, 1 ReLU, 2 ELU with alpha = 1, ``v > 0 ? v : expm1(v)``."""
    if act == ACT_NONE:
        return x
    if act == ACT_RELU:
        return np.maximum(x, 0)
    if act == ACT_ELU:
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0))).astype(x.dtype, copy=False)
    raise ValueError(f"act must be 0 (none), 1 (ReLU) or 2 (ELU), got {act}")


def _affine(out, scale, shift, dt):
    if scale is not None:
        out = out * np.asarray(scale, dt).reshape(1, -1)
    if shift is not None:
        out = out + np.asarray(shift, dt).reshape(1, -1)
    return out


def sparse_conv3d_act_host(feats, nbr, weight, bias=None, scale=None, shift=None, residual=None, act: int = ACT_NONE) -> np.ndarray:
    """``sparse_conv3d_host`` with the activation selector behind the epilogue."""
    return act_host(sparse_conv3d_host(feats, nbr, weight, bias, scale, shift, residual, relu=False), act)


def conv_transpose_gen_host(coords, scene_rows: Sequence[int], tensor_stride: int, feats, kernel, scale=None, shift=None,
                            act: int = ACT_NONE):
    """``MinkowskiGenerativeConvolutionTranspose(kernel_size=2, stride=2)``: ``(coords_out (8n,4) int32, out_scene_rows, out (8n,Cout))`` in
    the dtype of ``feats``.  Row ``8 i + j`` lies at ``coords[i] + kernel_offsets(2, tensor_stride / 2)[j]`` (x fastest, then y, then z:
    parity-unpinned against ME itself) and carries ``act((feats[i] @ kernel[j]) * scale + shift)``; children of distinct parents are
    distinct, so nothing is looked up."""
    ts = int(tensor_stride)
    if ts < 2 or ts & (ts - 1) or ts > (1 << 15):
        raise ValueError(f"tensor_stride must be a power of two from 2 to 2^15, got {tensor_stride}")
    feats = np.asarray(feats)
    dt = feats.dtype
    kernel = np.asarray(kernel, dt)
    c = np.asarray(coords).astype(np.int64).reshape(-1, 4)
    n = c.shape[0]
    offs = kernel_offsets(2, ts // 2)                            # (8,3)
    out_c = np.repeat(c, 8, axis=0)
    out_c[:, 1:] += np.tile(offs, (n, 1))
    out = np.empty((n, 8, kernel.shape[2]), dt)
    for j in range(8):
        out[:, j] = feats @ kernel[j]
    out = act_host(_affine(out.reshape(8 * n, -1), scale, shift, dt).astype(dt, copy=False), act)
    return out_c.astype(np.int32), [8 * int(e) for e in scene_rows], out


def conv_transpose_gen_bwd_host(g, feats, kernel) -> dict:
    """Backward of the raw generative transposed convolution (no epilogue) in the dtype of ``g (8n, Cout)``: ``dict(dfeats, dkernel)`` with
    ``dfeats[i] = sum_j g[8 i + j] @ kernel[j].T`` (j ascending) and ``dkernel[j] = feats.T @ g[j::8]``."""
    g = np.asarray(g)
    dt = g.dtype
    feats, kernel = np.asarray(feats, dt), np.asarray(kernel, dt)
    dfeats = np.zeros_like(feats)
    dkernel = np.empty_like(kernel)
    for j in range(8):
        dfeats = dfeats + g[j::8] @ kernel[j].T
        dkernel[j] = feats.T @ g[j::8]
    return dict(dfeats=dfeats.astype(dt, copy=False), dkernel=dkernel)


def rows_gather_host(g, dest) -> np.ndarray:
    """``out[i] = g[dest[i]]`` where ``dest[i] >= 0``, else ``+0.0``: the backward of the row routings (``dA = g[a_dest]``,
    ``dB = g[b_dest]`` of the union, ``dU = g[dest]`` of the prune).  Pure copies."""
    g, dest = np.asarray(g), np.asarray(dest).reshape(-1)
    out = np.zeros((dest.shape[0], g.shape[1]), g.dtype)
    hit = (dest >= 0) & (dest < g.shape[0])
    out[hit] = g[dest[hit]]
    return out


def union_dest_host(a_coords, a_rows: Sequence[int], b_coords, b_rows: Sequence[int]):
    """``(a_dest (nA,), b_dest (nB,))`` int32: the row of ``union_add_host``'s result that holds ``A[a]`` resp. ``B[k]`` -- a matched pair
    shares one."""
    ac, bc = np.asarray(a_coords).reshape(-1, 4), np.asarray(b_coords).reshape(-1, 4)
    a_dest, b_dest = np.full(ac.shape[0], -1, np.int32), np.full(bc.shape[0], -1, np.int32)
    alo = blo = out0 = 0
    for ahi, bhi in zip((int(e) for e in a_rows), (int(e) for e in b_rows)):
        index = {tuple(int(v) for v in row[1:]): alo + i for i, row in enumerate(ac[alo:ahi])}
        a_dest[alo:ahi] = out0 + np.arange(ahi - alo)
        extra = 0
        for k in range(blo, bhi):
            a = index.get(tuple(int(v) for v in bc[k, 1:]), -1)
            if a >= 0:
                b_dest[k] = a_dest[a]
            else:
                b_dest[k] = out0 + (ahi - alo) + extra
                extra += 1
        out0 += (ahi - alo) + extra
        alo, blo = ahi, bhi
    return a_dest, b_dest


def prune_dest_host(keep) -> np.ndarray:
    """``dest (n,)`` int32 of ``MinkowskiPruning``: the place of each kept row among the kept rows, ``-1`` for a dropped one."""
    keep = np.asarray(keep, bool)
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


def union_add_host(a_coords, a_rows: Sequence[int], a_feats, b_coords, b_rows: Sequence[int], b_feats):
    """``A + B`` of two sparse tensors of one tensor stride over the union of their rows: ``(coords, scene_rows, feats)``.  Scene b of the
    result: A's rows of b in A's order, then the rows of B in b that are absent from A, in B's order; ``A[a] + B[k]`` (one add) where both
    exist, the single operand's row elsewhere.  The row order is parity-unpinned against ME itself (nothing downstream depends on it but
    the order of the returned lists)."""
    a_feats, b_feats = np.asarray(a_feats), np.asarray(b_feats)
    dt = a_feats.dtype
    ac, bc = np.asarray(a_coords).reshape(-1, 4), np.asarray(b_coords).reshape(-1, 4)
    rows: List[np.ndarray] = []
    feats: List[np.ndarray] = []
    ends: List[int] = []
    alo = blo = 0
    for ahi, bhi in zip((int(e) for e in a_rows), (int(e) for e in b_rows)):
        index = {tuple(int(v) for v in row[1:]): alo + i for i, row in enumerate(ac[alo:ahi])}
        fa = a_feats[alo:ahi].copy()
        alone = []
        for k in range(blo, bhi):
            a = index.get(tuple(int(v) for v in bc[k, 1:]), -1)
            if a >= 0:
                fa[a - alo] = fa[a - alo] + b_feats[k].astype(dt)
            else:
                alone.append(k)
        rows += [ac[alo:ahi], bc[alone].reshape(-1, 4)]
        feats += [fa, b_feats[alone].astype(dt).reshape(-1, a_feats.shape[1])]
        ends.append((ends[-1] if ends else 0) + (ahi - alo) + len(alone))
        alo, blo = ahi, bhi
    return np.concatenate(rows).astype(np.int32), ends, np.concatenate(feats).astype(dt, copy=False)


def prune_scores_host(q_coords, s_coords, s_rows: Sequence[int], tensor_stride: int, scores) -> np.ndarray:
    """``scores.features_at_coordinates(q)``: ``(n_q,)`` in the dtype of ``scores`` ``(m,)`` / ``(m,1)``, which live on the rows
    ``s_coords`` of tensor stride ts.  Per axis ``l = floor(q / ts) * ts``; corners ``c = l + {0, ts}^3`` indexed x fastest;
    ``w_c = prod (1 - |q - c| / ts)``; the sum over the corners present in the query's scene of ``w_c * s[c]`` in ascending corner index,
    starting from 0: absent corners contribute nothing, nothing is renormalised, no corner gives 0.0 (parity-unpinned against ME itself)."""
    s = np.asarray(scores).reshape(-1)
    dt = s.dtype
    ts = int(tensor_stride)
    sc = np.asarray(s_coords).reshape(-1, 4)
    q = np.asarray(q_coords).astype(np.int64).reshape(-1, 4)
    index = {}
    lo = 0
    for b, hi in enumerate(int(e) for e in s_rows):
        for i in range(lo, hi):
            index[(b, int(sc[i, 1]), int(sc[i, 2]), int(sc[i, 3]))] = i
        lo = hi
    out = np.zeros(q.shape[0], dt)
    one, inv = dt.type(1), dt.type(1) / dt.type(ts)
    offs = kernel_offsets(2, ts)
    for i, row in enumerate(q):
        l = np.floor_divide(row[1:], ts) * ts
        acc = dt.type(0)
        for d in offs:
            c = l + d
            r = index.get((int(row[0]), int(c[0]), int(c[1]), int(c[2])), -1)
            if r < 0:
                continue
            w = one
            for ax in range(3):
                w = w * (one - dt.type(abs(int(row[1 + ax]) - int(c[ax]))) * inv)
            acc = acc + w * s[r]
        out[i] = acc
    return out


def topk_key(scores) -> np.ndarray:
    """The order the top-k compares in, as unsigned integers of the scores' width: a larger score has a larger key, ``-0.0`` and ``+0.0``
    share one.  Scores are meant to be finite; a NaN orders by its bits -- above ``+inf`` with the sign bit clear, below ``-inf`` with it
    set -- so a positive NaN is always kept and nothing raises."""
    s = np.ascontiguousarray(np.asarray(scores).reshape(-1))
    if s.dtype == np.float32:
        u, top, full = s.view(np.uint32).copy(), np.uint32(1 << 31), np.uint32(0xFFFFFFFF)
    elif s.dtype == np.float64:
        u, top, full = s.view(np.uint64).copy(), np.uint64(1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF)
    else:
        raise TypeError(f"float32 or float64 scores expected, got {s.dtype}")
    u[(u & ~top) == 0] = 0
    neg = (u & top) != 0
    return np.where(neg, u ^ full, u | top)


def topk_scene_rows(scene_rows: Sequence[int], k: int) -> List[int]:
    """The scene ends behind the prune: ``min(rows_b, k)`` accumulated -- known without looking at a score."""
    ends, lo = [], 0
    for hi in (int(e) for e in scene_rows):
        ends.append((ends[-1] if ends else 0) + min(hi - lo, int(k)))
        lo = hi
    return ends


def topk_keep_host(scores, scene_rows: Sequence[int], k: int) -> np.ndarray:
    """The keep mask ``(n,) bool`` of the per-scene top-k: scene b keeps its ``min(rows_b, k)`` rows with the largest scores in the order
    of ``topk_key``; among equal keys the lower row index wins (``torch.topk`` leaves ties unspecified)."""
    key = topk_key(scores)
    keep = np.zeros(key.shape[0], bool)
    lo = 0
    for hi in (int(e) for e in scene_rows):
        order = np.argsort(~key[lo:hi], kind="stable")           # descending key, ascending row index among equals
        keep[lo + order[:min(hi - lo, int(k))]] = True
        lo = hi
    return keep


def prune_host(keep, coords, scene_rows: Sequence[int], feats):
    """``MinkowskiPruning``: the kept rows in their order -- ``(coords, scene_rows, feats)``."""
    keep = np.asarray(keep, bool)
    ends, lo = [], 0
    for hi in (int(e) for e in scene_rows):
        ends.append((ends[-1] if ends else 0) + int(keep[lo:hi].sum()))
        lo = hi
    return np.asarray(coords)[keep], ends, np.asarray(feats)[keep]


def head_host(feats, weight, bias=None):
    """``conv_cls`` (kernel 1) and the prune score: ``(cls (n,K), score (n,))`` with ``cls = feats @ weight (C,K) + bias`` and
    ``score = max_k cls`` in the dtype of ``feats``.  The maximum is numpy's: a NaN class score, in whichever class, makes the score
    NaN (the kernel complies: a row whose features went NaN must not reach the prune with a finite score)."""
    feats = np.asarray(feats)
    dt = feats.dtype
    cls = feats @ np.asarray(weight, dt).reshape(feats.shape[1], -1)
    if bias is not None:
        cls = cls + np.asarray(bias, dt).reshape(1, -1)
    cls = cls.astype(dt, copy=False)
    return cls, cls.max(axis=1)


def head_bwd_host(dcls, feats, weight) -> dict:
    """Backward of ``conv_cls`` in the dtype of ``dcls (n, K)``: ``dict(dfeats = dcls @ weight.T, dweight (C, K) = feats.T @ dcls,
    dbias (K) = sum_rows dcls)``.  The prune score gets no gradient (the reference takes it under ``torch.no_grad()``)."""
    dcls = np.asarray(dcls)
    dt = dcls.dtype
    feats = np.asarray(feats, dt)
    w = np.asarray(weight, dt).reshape(feats.shape[1], -1)
    return dict(dfeats=(dcls @ w.T).astype(dt, copy=False), dweight=(feats.T @ dcls).astype(dt, copy=False), dbias=dcls.sum(axis=0, dtype=dt))
