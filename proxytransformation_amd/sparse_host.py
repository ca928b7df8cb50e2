"""The numpy restatements of the sparse layers: the specification the kernels of ``sparse.py`` are held to (bit for bit, resp. to fp32
rounding), and the geometry both sides share.  Imports only numpy; ``sparse.py`` re-exports every name, which is where the semantics
are described (its module docstring)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

__all__ = ["kernel_map_host", "kernel_map_transpose_host", "kernel_offsets", "sparse_conv3d_bwd_host", "sparse_conv3d_host",
           "sparse_max_pool3d_bwd_host", "sparse_max_pool3d_host", "sparse_norm_bwd_host", "sparse_norm_host"]


def kernel_offsets(kernel_size: int, tensor_stride: int) -> np.ndarray:
    """The ``k^3`` offsets ``(dx, dy, dz)`` of a kernel in the order of the weight tensor's rows: x fastest, then y, then z; odd k
    centred, even k from 0 upwards.  The ONE place that fixes this order (our reading of MinkowskiEngine's region iterator; parity
    unpinned against ME itself)."""
    k = int(kernel_size)
    lo = -(k // 2) if k % 2 else 0
    r = np.arange(lo, lo + k, dtype=np.int64) * int(tensor_stride)
    z, y, x = np.meshgrid(r, r, r, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


def _check_geometry(tensor_stride: int, kernel_size: int, stride: int) -> None:
    ts = int(tensor_stride)
    if ts < 1 or ts & (ts - 1) or ts > (1 << 15):
        raise ValueError(f"tensor_stride must be a power of two up to 2^15, got {tensor_stride}")
    if int(kernel_size) not in (1, 2, 3) or int(stride) not in (1, 2):
        raise ValueError(f"kernel_size must be 1, 2 or 3 and stride 1 or 2, got {kernel_size}, {stride}")


def kernel_map_host(coords, scene_rows: Sequence[int], tensor_stride: int, kernel_size: int, stride: int):
    """numpy restatement of ``kernel_map``: ``(coords_out (n_out,4) int32, out_scene_rows, nbr (n_out,k^3) int32)``."""
    _check_geometry(tensor_stride, kernel_size, stride)
    c = np.asarray(coords).astype(np.int64).reshape(-1, 4)
    ts, k = int(tensor_stride), int(kernel_size)
    offs = kernel_offsets(k, ts)
    out_rows: List[np.ndarray] = []
    out_ends: List[int] = []
    nbrs: List[np.ndarray] = []
    lo = 0
    for b, hi in enumerate(int(e) for e in scene_rows):
        cin = c[lo:hi, 1:]
        if int(stride) == 1:
            cout = cin
        else:                                                    # floor division, first occurrence
            q = np.floor_divide(cin, 2 * ts) * (2 * ts)
            _, first = np.unique(q, axis=0, return_index=True)
            cout = q[np.sort(first)] if len(q) else q
        index = {tuple(int(v) for v in row): lo + i for i, row in enumerate(cin)}
        nb = np.full((len(cout), k ** 3), -1, np.int32)
        for o, row in enumerate(cout):
            for j, d in enumerate(offs):
                nb[o, j] = index.get((int(row[0] + d[0]), int(row[1] + d[1]), int(row[2] + d[2])), -1)
        out_rows.append(np.concatenate([np.full((len(cout), 1), b, np.int64), cout], axis=1))
        nbrs.append(nb)
        out_ends.append((out_ends[-1] if out_ends else 0) + len(cout))
        lo = hi
    coords_out = np.concatenate(out_rows, axis=0).astype(np.int32) if out_rows else np.zeros((0, 4), np.int32)
    nbr = np.concatenate(nbrs, axis=0) if nbrs else np.zeros((0, k ** 3), np.int32)
    return coords_out, out_ends, nbr


def sparse_conv3d_host(feats, nbr, weight, bias=None, scale=None, shift=None, residual=None, relu: bool = False) -> np.ndarray:
    """numpy restatement of ``sparse_conv3d`` in the dtype of ``feats`` (float64: the reference of the tests; float32: the same chain in
    the kernel's precision, summed in another order)."""
    feats = np.asarray(feats)
    dt = feats.dtype
    nbr = np.asarray(nbr)
    weight = np.asarray(weight, dt)
    out = np.zeros((nbr.shape[0], weight.shape[2]), dt)
    for j in range(nbr.shape[1]):
        m = nbr[:, j] >= 0
        if m.any():
            out[m] += feats[nbr[m, j]] @ weight[j]
    if bias is not None:
        out = out + np.asarray(bias, dt).reshape(1, -1)
    if scale is not None:
        out = out * np.asarray(scale, dt).reshape(1, -1)
    if shift is not None:
        out = out + np.asarray(shift, dt).reshape(1, -1)
    if residual is not None:
        out = out + np.asarray(residual, dt)
    if relu:
        out = np.maximum(out, 0)
    return out.astype(dt, copy=False)


def sparse_max_pool3d_host(feats, nbr) -> np.ndarray:
    """numpy restatement of ``sparse_max_pool3d`` (a row without a neighbour stays -inf)."""
    feats = np.asarray(feats)
    nbr = np.asarray(nbr)
    out = np.full((nbr.shape[0], feats.shape[1]), -np.inf, feats.dtype)
    for j in range(nbr.shape[1]):
        m = nbr[:, j] >= 0
        out[m] = np.maximum(out[m], feats[nbr[m, j]])
    return out


def kernel_map_transpose_host(nbr, n_in: int) -> np.ndarray:
    """numpy restatement of the transposed map: ``nbr_t (n_in, k^3) int32``, ``nbr_t[i, j] = o`` with ``nbr[o, j] == i``, else -1 (at most
    one such ``o`` exists).  Entries of ``nbr`` below 0 or ``>= n_in`` are skipped."""
    nbr = np.asarray(nbr)
    nbr_t = np.full((int(n_in), nbr.shape[1]), -1, np.int32)
    o, j = np.nonzero((nbr >= 0) & (nbr < int(n_in)))
    nbr_t[nbr[o, j], j] = o
    return nbr_t


def sparse_conv3d_bwd_host(g, feats, nbr, weight, out=None, scale=None, relu: bool = False, has_bias: bool = False,
                           has_residual: bool = False) -> dict:
    """numpy restatement of the backward of ``sparse_conv3d`` in the dtype of ``g``: ``dict(dfeats, dweight, dbias, dresidual)`` (the last
    two ``None`` unless ``has_bias`` / ``has_residual``).  The ReLU mask is taken from the ``out`` it is handed (the forward's result);
    ``scale`` is a constant the gradient passes through multiplied by."""
    g = np.asarray(g)
    dt = g.dtype
    feats, nbr, weight = np.asarray(feats, dt), np.asarray(nbr), np.asarray(weight, dt)
    d = g
    if relu:
        d = np.where(np.asarray(out) > 0, g, np.zeros((), dt)).astype(dt, copy=False)
    gz = d if scale is None else (d * np.asarray(scale, dt).reshape(1, -1)).astype(dt, copy=False)
    dfeats = np.zeros((feats.shape[0], weight.shape[1]), dt)
    dweight = np.zeros(weight.shape, dt)
    for j in range(nbr.shape[1]):
        m = nbr[:, j] >= 0
        if m.any():
            dweight[j] = feats[nbr[m, j]].T @ gz[m]
            dfeats[nbr[m, j]] += gz[m] @ weight[j].T          # (the rows nbr[m, j] are distinct: no collisions)
    return dict(dfeats=dfeats, dweight=dweight, dbias=gz.sum(0).astype(dt, copy=False) if has_bias else None,
                dresidual=d if has_residual else None)


def sparse_max_pool3d_bwd_host(g, feats, nbr) -> np.ndarray:
    """numpy restatement of the backward of ``sparse_max_pool3d``: every output element's gradient goes to the input row of the offset
    that supplied the maximum -- ties to the smallest ``j`` --, summed per input row over ascending ``j``, in the dtype of ``g``."""
    g, feats, nbr = np.asarray(g), np.asarray(feats), np.asarray(nbr)
    n_out, C = g.shape
    best = np.full((n_out, C), -np.inf, feats.dtype)
    arg = np.full((n_out, C), 255, np.int64)
    for j in range(nbr.shape[1]):
        m = nbr[:, j] >= 0
        x = feats[nbr[m, j]]
        take = (x > best[m]) | (arg[m] == 255)              # strictly larger: a tie keeps the smaller j
        arg[m] = np.where(take, j, arg[m])
        best[m] = np.maximum(best[m], x)
    dfeats = np.zeros((feats.shape[0], C), g.dtype)
    for j in range(nbr.shape[1]):
        m = nbr[:, j] >= 0
        dfeats[nbr[m, j]] += np.where(arg[m] == j, g[m], np.zeros((), g.dtype))
    return dfeats


def _segments(seg_end: Sequence[int], n: int) -> List[int]:
    ends = [int(e) for e in seg_end]
    if not 1 <= len(ends) <= 64:
        raise ValueError(f"1 to 64 segments, got {len(ends)}")
    if any(b < a for a, b in zip([0] + ends[:-1], ends)) or ends[-1] != int(n):
        raise ValueError(f"segment ends must ascend from 0 to the {n} rows, got {ends}")
    return ends


def sparse_norm_host(x, seg_end: Sequence[int], eps: float, weight=None, bias=None, residual=None, relu: bool = False,
                     return_stats: bool = False, running=None, momentum: float = 0.1, elu: bool = False):
    """numpy restatement of the norm kernels' forward in the dtype of ``x``, two-pass: per segment ``[seg_end[s-1], seg_end[s])`` and
    column ``mean``, biased ``var = mean((x - mean)^2)``, ``rstd = 1 / sqrt(var + eps)``;
    ``out = relu?(((x - mean) * rstd) * weight + bias (+ residual))``.  ``return_stats``: also ``stats (S, 2, C) = (mean, rstd)``, an
    empty segment ``(0, 0)``.  ``running = (running_mean, running_var)`` (one segment of at least 2 rows): the two arrays are updated in
    place as the kernel updates them, ``(1 - momentum) * old + momentum * new`` with the unbiased variance (``nn.BatchNorm1d``'s rule).
    ``elu`` (not with ``relu``): the ELU with alpha = 1, ``v > 0 ? v : expm1(v)``, in the place of the ReLU."""
    if relu and elu:
        raise ValueError("relu and elu are one activation slot")
    x = np.asarray(x)
    dt = x.dtype
    ends = _segments(seg_end, x.shape[0])
    out = np.empty_like(x)
    stats = np.zeros((len(ends), 2, x.shape[1]), dt)
    lo = 0
    for s, hi in enumerate(ends):
        if hi > lo:
            seg = x[lo:hi]
            mean = seg.mean(axis=0, dtype=dt)
            var = np.square(seg - mean).mean(axis=0, dtype=dt)
            rstd = (1 / np.sqrt(var + dt.type(eps))).astype(dt, copy=False)
            stats[s, 0], stats[s, 1] = mean, rstd
            out[lo:hi] = (seg - mean) * rstd
            if running is not None:
                if len(ends) != 1 or hi < 2:
                    raise ValueError("running statistics need one segment of at least 2 rows")
                m = dt.type(momentum)
                running[0][...] = (1 - m) * running[0] + m * mean
                running[1][...] = (1 - m) * running[1] + m * (var * dt.type(hi) / dt.type(hi - 1))
        lo = hi
    if weight is not None:
        out = out * np.asarray(weight, dt).reshape(1, -1)
    if bias is not None:
        out = out + np.asarray(bias, dt).reshape(1, -1)
    if residual is not None:
        out = out + np.asarray(residual, dt)
    if relu:
        out = np.maximum(out, 0)
    if elu:
        out = np.where(out > 0, out, np.expm1(np.minimum(out, 0)))
    out = out.astype(dt, copy=False)
    return (out, stats) if return_stats else out


def sparse_norm_bwd_host(g, x, seg_end: Sequence[int], eps: float, weight=None, out=None, relu: bool = False, stats=None,
                         elu: bool = False) -> dict:
    """numpy restatement of the norm kernels' backward in the dtype of ``g``: ``dict(dx, dweight, dbias, dresidual)``.  ``gy = g * [out > 0]``
    with the ReLU mask taken from the ``out`` it is handed (``g`` itself without ReLU); ``xhat`` from ``x`` and ``stats`` (default: the
    two-pass statistics of ``x``); ``dresidual = gy``, ``dbias = sum gy``, ``dweight = sum gy * xhat``; per segment ``a = mean gy``,
    ``b = mean gy * xhat``, ``dx = weight * rstd * (gy - a - xhat * b)``.  ``elu``: ``gy = g * (out > 0 ? 1 : out + 1)`` from the ``out`` it
    is handed -- exactly 0 where ``out == -1``; a NaN ``out`` gives a NaN ``gy`` and is never dropped (behind the ReLU ``[NaN > 0] = 0``)."""
    g = np.asarray(g)
    dt = g.dtype
    x = np.asarray(x, dt)
    ends = _segments(seg_end, x.shape[0])
    if stats is None:
        _, stats = sparse_norm_host(x, ends, eps, return_stats=True)
    stats = np.asarray(stats, dt)
    gy = np.where(np.asarray(out) > 0, g, np.zeros((), dt)).astype(dt, copy=False) if relu else g
    if elu:
        o = np.asarray(out, dt)
        gy = np.where(o > 0, g, g * (o + dt.type(1))).astype(dt, copy=False)
    w = np.ones((1, x.shape[1]), dt) if weight is None else np.asarray(weight, dt).reshape(1, -1)
    dx = np.empty_like(x)
    xhat = np.empty_like(x)
    lo = 0
    for s, hi in enumerate(ends):
        if hi > lo:
            xh = (x[lo:hi] - stats[s, 0]) * stats[s, 1]
            a = gy[lo:hi].mean(axis=0, dtype=dt)
            b = (gy[lo:hi] * xh).mean(axis=0, dtype=dt)
            dx[lo:hi] = (w * stats[s, 1]) * (gy[lo:hi] - a - xh * b)
            xhat[lo:hi] = xh
        lo = hi
    return dict(dx=dx.astype(dt, copy=False), dweight=(gy * xhat).sum(axis=0, dtype=dt), dbias=gy.sum(axis=0, dtype=dt), dresidual=gy)
