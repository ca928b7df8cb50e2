"""The sparse neck ``MinkNeck`` (``feats, scores, coords = self.neck_3d(x, batch_size)``; necks/mink_neck.py) on the device: the last stage of the
detector's feature path before the (plain torch) transformer decoder.  Eval mode by default; ``MinkNeck(..., differentiable=True)`` with its
BatchNorms in training mode is the training chain, forward and backward (below).

Beside ``sparse.py``'s kernel maps and convolution (here with an ELU behind the folded BatchNorm and inputs up to 1024 channels wide:
``sparse_conv3d(..., elu=True)``, ``ptx_sparse_conv3d_act``) the neck needs four operations, each one call into ``csrc/neck.hip`` /
``csrc/sparse.hip`` on the current stream and each restated in numpy by ``neck_host.py``, which is their specification:

* ``conv_transpose_gen``  -- ``MinkowskiGenerativeConvolutionTranspose(kernel_size=2, stride=2)``: 8 children per row, features
  ``x[i] @ kernel[j]`` (+ folded BatchNorm + activation), no table;
* ``union_add``           -- ``inputs[i] + x``: the sum over the union of two row sets; the host waits for the row count through pinned
  words, as ``kernel_map`` does;
* ``prune_scores``        -- ``scores.features_at_coordinates(x.C.float())``: trilinear lookup, absent corners contribute nothing;
* ``topk_prune``          -- the per-scene top-k and ``MinkowskiPruning``; ties go to the lower row index, the new scene ends are known
  on the host without a wait;
* ``neck_head``           -- ``conv_cls`` and the prune score ``max`` over the classes in one kernel.

The offset order of the transposed convolution, the union's row order, the corner rule and the tie rule are OUR READING of
MinkowskiEngine, parity-unpinned against ME itself (``neck_host.py``).

Training (opt-in, ``differentiable=True`` on every operation and on the modules, as in ``sparse.py``; ``csrc/neck_bwd.hip``,
``csrc/sparse_bwd.hip``, ``csrc/sparse_norm.hip``).  The reference trains the neck with its BatchNorms in training mode and prunes under
``torch.no_grad()`` (mink_neck.py:163-186): features and ``cls_preds`` carry gradient; the prune scores, the trilinear lookup and the
top-k do not.  Every block runs as a raw convolution followed by a training BatchNorm with the ELU fused (``sparse_batch_norm(elu=True)``);
the generative convolution's backward is ``ptx_sparse_conv_transpose_gen_bwd``; ``union_add`` routes the gradient to both operands and
``topk_prune`` to the kept rows through one gather kernel (``ptx_neck_rows_gather``); the head's backward is ``ptx_neck_head_bwd`` with
the score detached.  No float atomics, fixed orders: two calls give the same bits.

Out of scope: training through frozen (eval-mode) BatchNorms, double backward, bf16, reading the backbone and image halves of the
concatenated level features in place (the caller concatenates), the decoder.  There is no CPU path: tensors must be on the GPU and the
library must be built."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _abi, neck_host, sparse
from ._doors import _channel_vectors, _f32, _f32_grad, _int32_array, _np, _ptr, _stream, _train, _wants_grad, _workspace
from .backbone import SparseLevel
from .neck_host import ACT_ELU, ACT_NONE
from .registry import MODELS, REGISTRY_BACKEND
from .sparse import SparseBatchNorm, SparseConv3d

__all__ = ["GenerativeConvTranspose", "MinkNeck", "conv_transpose_gen", "neck_head", "prune_scores", "rows_gather", "topk_prune", "union_add"]


def _rows(what: str, coords: torch.Tensor, n: int) -> torch.Tensor:
    if not coords.is_cuda:
        raise RuntimeError(f"{what} (HIP) needs GPU tensors: there is no CPU path")
    if coords.dtype != torch.int32 or not coords.is_contiguous():
        coords = coords.to(torch.int32).contiguous()
    if coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] != n:
        raise ValueError(f"{what}: coords must be ({n},4), got {tuple(coords.shape)}")
    return coords


def _neck_workspace(what: str, B: int, ncap: int, rows: int, dev) -> torch.Tensor:
    nbytes = _abi.lib().ptx_neck_workspace_bytes(B, max(ncap, 1), rows)
    if nbytes == 0:
        raise ValueError(f"{what}: unsupported size, {B} scenes of up to {ncap} rows")
    return _workspace("neck", nbytes, dev)


def _ncap(scene_rows: Sequence[int]) -> int:
    lo = [0] + [int(e) for e in scene_rows[:-1]]
    return max(max(int(e) - l for e, l in zip(scene_rows, lo)), 1)


def rows_gather(g: torch.Tensor, dest: torch.Tensor) -> torch.Tensor:
    """``out (n, C)`` with ``out[i] = g[dest[i]]`` where ``dest[i] >= 0``, else ``+0.0`` (``neck_host.rows_gather_host``, bit for bit;
    ``ptx_neck_rows_gather``): the backward of the row routings of ``union_add`` and ``topk_prune``.  Zero rows need no launch."""
    g = _f32_grad(g.detach())
    n, C = int(dest.shape[0]), int(g.shape[1])
    out = torch.empty((n, C), dtype=torch.float32, device=g.device)
    _abi.check(_abi.lib().ptx_neck_rows_gather(g.data_ptr(), int(g.shape[0]), dest.data_ptr(), n, C, out.data_ptr(), _stream(g.device)),
               "ptx_neck_rows_gather")
    return out


class _GenConvFn(torch.autograd.Function):
    """feats (n,Cin), kernel (8,Cin,Cout): fp32, contiguous, on the device; the raw product, no epilogue."""

    @staticmethod
    def forward(ctx, feats, kernel, coords, tensor_stride):
        n, cin, cout = int(feats.shape[0]), int(kernel.shape[1]), int(kernel.shape[2])
        dev = feats.device
        out_c = torch.empty((8 * n, 4), dtype=torch.int32, device=dev)
        out = torch.empty((8 * n, cout), dtype=torch.float32, device=dev)
        _abi.check(_abi.lib().ptx_sparse_conv_transpose_gen(coords.data_ptr(), n, int(tensor_stride), feats.data_ptr(), kernel.data_ptr(), cin,
                                                            cout, None, None, ACT_NONE, out_c.data_ptr(), out.data_ptr(), _stream(dev)),
                   "ptx_sparse_conv_transpose_gen")
        ctx.save_for_backward(feats, kernel)
        ctx.mark_non_differentiable(out_c)
        return out, out_c

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gc):
        feats, kernel = ctx.saved_tensors
        need_f, need_k = ctx.needs_input_grad[:2]
        dev = feats.device
        g = _f32_grad(g)
        n, cin, cout = int(feats.shape[0]), int(kernel.shape[1]), int(kernel.shape[2])
        lib = _abi.lib()
        dfeats = torch.empty((n, cin), dtype=torch.float32, device=dev) if need_f else None
        dkernel = torch.empty((8, cin, cout), dtype=torch.float32, device=dev) if need_k else None
        nbytes = lib.ptx_sparse_conv_transpose_gen_bwd_workspace_bytes(n, cin, cout)
        if nbytes == 0:
            raise ValueError(f"conv_transpose_gen backward: unsupported size, {n} rows, Cin={cin}, Cout={cout}")
        ws = _workspace("conv_bwd", nbytes, dev) if need_k else None
        _abi.check(lib.ptx_sparse_conv_transpose_gen_bwd(g.data_ptr(), feats.data_ptr(), n, kernel.data_ptr(), cin, cout, _ptr(dfeats),
                                                         _ptr(dkernel), _ptr(ws), 0 if ws is None else ws.numel(), _stream(dev)),
                   "ptx_sparse_conv_transpose_gen_bwd")
        return dfeats, dkernel, None, None


def conv_transpose_gen(coords: torch.Tensor, scene_rows: Sequence[int], tensor_stride: int, feats: torch.Tensor, kernel: torch.Tensor,
                       scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                       differentiable: bool = False):
    """``(coords_out (8n,4) int32, out_scene_rows, out (8n,Cout) fp32)`` of a generative transposed convolution, kernel 2, stride 2
    (``neck_host.conv_transpose_gen_host``; ``ptx_sparse_conv_transpose_gen``): row ``8 i + j`` is child ``j`` of row ``i`` at tensor stride
    ``tensor_stride / 2`` with ``act((feats[i] @ kernel[j]) * scale + shift)``.  ``kernel (8, Cin, Cout)``, Cin a multiple of 64 up to
    1024, Cout a multiple of 64 up to 512; ``act``: 0 none, 1 ReLU, 2 ELU.  Inference-only unless ``differentiable=True``: then, with
    grad mode on and ``feats`` / ``kernel`` requiring grad, the raw product (no ``scale`` / ``shift`` / ``act``: the training BatchNorm is a
    layer of its own) is recorded for autograd (``neck_host.conv_transpose_gen_bwd_host``; ``ptx_sparse_conv_transpose_gen_bwd``; same
    output bits)."""
    train = _train("conv_transpose_gen", differentiable, feats, kernel, scale, shift)
    if train and (scale is not None or shift is not None or act != ACT_NONE):
        raise NotImplementedError("conv_transpose_gen(differentiable=True) records the raw product only: the backward through a folded "
                                  "epilogue (scale / shift / act) is not implemented; follow it with sparse_batch_norm(elu=True)")
    grad_in = (feats, kernel)
    if not feats.is_cuda:
        raise RuntimeError("conv_transpose_gen (HIP) needs GPU tensors: there is no CPU path")
    dev = feats.device
    feats, kernel = _f32(feats, "conv_transpose_gen", dev), _f32(kernel, "conv_transpose_gen", dev)
    n = int(scene_rows[-1])
    coords = _rows("conv_transpose_gen", coords, n)
    if feats.dim() != 2 or kernel.dim() != 3 or kernel.shape[0] != 8 or kernel.shape[1] != feats.shape[1] or feats.shape[0] != n:
        raise ValueError(f"conv_transpose_gen: feats ({n},Cin) and kernel (8,Cin,Cout) expected, got {tuple(feats.shape)}, {tuple(kernel.shape)}")
    cin, cout = int(kernel.shape[1]), int(kernel.shape[2])
    vecs = _channel_vectors("conv_transpose_gen", cout, dev, scale=scale, shift=shift)
    if train:
        ts = int(tensor_stride)
        if n > (1 << 24) or ts < 2 or ts & (ts - 1) or ts > (1 << 15) or cin % 64 or not 64 <= cin <= 1024 or cout % 64 or not 64 <= cout <= 512:
            raise ValueError(f"conv_transpose_gen(differentiable=True): n={n} tensor_stride={ts} Cin={cin} Cout={cout} (at most 2^24 rows; "
                             f"tensor_stride a power of two from 2 to 2^15; Cin a multiple of 64 up to 1024; Cout a multiple of 64 up to 512)")
        out, out_c = _GenConvFn.apply(_f32_grad(grad_in[0]), _f32_grad(grad_in[1]), coords, ts)
        return out_c, [8 * int(e) for e in scene_rows], out
    out_c = torch.empty((8 * n, 4), dtype=torch.int32, device=dev)
    out = torch.empty((8 * n, cout), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_sparse_conv_transpose_gen(coords.data_ptr(), n, int(tensor_stride), feats.data_ptr(), kernel.data_ptr(), cin, cout,
                                                        _ptr(vecs[0]), _ptr(vecs[1]), int(act), out_c.data_ptr(), out.data_ptr(), _stream(dev)),
               "ptx_sparse_conv_transpose_gen")
    return out_c, [8 * int(e) for e in scene_rows], out


_WORDS: dict = {}                  # stream -> pinned count words of union_add


class _RouteFn(torch.autograd.Function):
    """Marks ``out`` -- rows already routed by a kernel -- as a function of the ``srcs``: ``out[dest_i[r]]`` received ``src_i[r]``
    (added where two sources share a row), so ``d src_i = g[dest_i]`` (``ptx_neck_rows_gather``)."""

    @staticmethod
    def forward(ctx, out, dests, *srcs):
        ctx.dests = dests
        return out.view_as(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return (None, None) + tuple(rows_gather(g, d) if need else None for d, need in zip(ctx.dests, ctx.needs_input_grad[2:]))


def union_add(a_coords: torch.Tensor, a_rows: Sequence[int], a_feats: torch.Tensor, b_coords: torch.Tensor, b_rows: Sequence[int],
              b_feats: torch.Tensor, tensor_stride: int, differentiable: bool = False, return_dest: bool = False):
    """``(coords, scene_rows, feats)`` of ``A + B`` over the union of the rows of two sparse tensors of one tensor stride and width
    (``neck_host.union_add_host``; ``ptx_neck_union_add``).  The host waits only for the row counts, published through pinned words;
    nothing synchronises the device.  ``return_dest``: also ``(a_dest (nA,), b_dest (nB,))`` int32, the output row of every input row
    (``neck_host.union_dest_host``; ``ptx_neck_union_add_dest``, same results bit for bit).  Inference-only unless ``differentiable=True``:
    then, with grad mode on and ``a_feats`` / ``b_feats`` requiring grad, the gradient flows to both operands, ``dA = g[a_dest]`` and
    ``dB = g[b_dest]``, pure copies."""
    train = _train("union_add", differentiable, a_feats, b_feats)
    grad_in = (a_feats, b_feats)
    if not (a_feats.is_cuda and b_feats.is_cuda):
        raise RuntimeError("union_add (HIP) needs GPU tensors: there is no CPU path")
    dev = a_feats.device
    B = len(a_rows)
    if B < 1 or B > 64 or len(b_rows) != B:
        raise ValueError(f"union_add: 1 to 64 scenes on both sides, got {B} and {len(b_rows)}")
    a_feats, b_feats = _f32(a_feats, "union_add", dev), _f32(b_feats, "union_add", dev)
    nA, nB = int(a_rows[-1]), int(b_rows[-1])
    a_coords, b_coords = _rows("union_add", a_coords, nA), _rows("union_add", b_coords, nB)
    C = int(a_feats.shape[1])
    if tuple(a_feats.shape) != (nA, C) or tuple(b_feats.shape) != (nB, C):
        raise ValueError(f"union_add: feats ({nA},C) and ({nB},C) expected, got {tuple(a_feats.shape)}, {tuple(b_feats.shape)}")
    ws = _neck_workspace("union_add", B, _ncap(a_rows), max(nA, nB), dev)
    st = _stream(dev)
    info = _WORDS.get((st, B))
    if info is None:
        info = _WORDS[(st, B)] = torch.empty((2 + B,), dtype=torch.int32).pin_memory()
    info_np = info.numpy()
    info_np[:] = -1
    out_c = torch.empty((nA + nB, 4), dtype=torch.int32, device=dev)
    out = torch.empty((nA + nB, C), dtype=torch.float32, device=dev)
    lib = _abi.lib()
    dests = None
    if train or return_dest:
        dests = (torch.empty((nA,), dtype=torch.int32, device=dev), torch.empty((nB,), dtype=torch.int32, device=dev))
        _abi.check(lib.ptx_neck_union_add_dest(a_coords.data_ptr(), _int32_array(a_rows), a_feats.data_ptr(), b_coords.data_ptr(),
                                               _int32_array(b_rows), b_feats.data_ptr(), B, int(tensor_stride), C, out_c.data_ptr(),
                                               out.data_ptr(), info.data_ptr() + 8, info.data_ptr(), dests[0].data_ptr(), dests[1].data_ptr(),
                                               ws.data_ptr(), ws.numel(), st), "ptx_neck_union_add_dest")
    else:
        _abi.check(lib.ptx_neck_union_add(a_coords.data_ptr(), _int32_array(a_rows), a_feats.data_ptr(), b_coords.data_ptr(),
                                          _int32_array(b_rows), b_feats.data_ptr(), B, int(tensor_stride), C, out_c.data_ptr(), out.data_ptr(),
                                          info.data_ptr() + 8, info.data_ptr(), ws.data_ptr(), ws.numel(), st), "ptx_neck_union_add")
    if lib.ptx_wait_counts(info.data_ptr(), 2 + B, 20_000_000) != 0:
        torch.cuda.current_stream(dev).synchronize()
    n, overflow = int(info_np[0]), int(info_np[1])
    if n < nA or n > nA + nB or overflow:
        raise RuntimeError(f"ptx_neck_union_add failed (rows {n}, {overflow} rows with a coordinate outside +-2^18 tensor strides)")
    res = out[:n]
    if train:
        res = _RouteFn.apply(res, dests, _f32_grad(grad_in[0]), _f32_grad(grad_in[1]))
    if return_dest:
        return out_c[:n], info_np[2:2 + B].tolist(), res, dests
    return out_c[:n], info_np[2:2 + B].tolist(), res


def prune_scores(q_coords: torch.Tensor, s_coords: torch.Tensor, s_rows: Sequence[int], tensor_stride: int,
                 scores: torch.Tensor) -> torch.Tensor:
    """``(n_q,) fp32``: the scores ``(m,)`` / ``(m,1)`` on the rows ``s_coords`` of tensor stride ``tensor_stride`` looked up trilinearly
    at ``q_coords`` (``neck_host.prune_scores_host``, bit for bit; ``ptx_neck_prune_scores``)."""
    _train("prune_scores", False, scores)
    if not scores.is_cuda:
        raise RuntimeError("prune_scores (HIP) needs GPU tensors: there is no CPU path")
    dev = scores.device
    B = len(s_rows)
    m = int(s_rows[-1])
    scores = _f32(scores, "prune_scores", dev).reshape(-1)
    if scores.numel() != m:
        raise ValueError(f"prune_scores: {m} scores expected, got {scores.numel()}")
    s_coords = _rows("prune_scores", s_coords, m)
    q_coords = _rows("prune_scores", q_coords, int(q_coords.shape[0]))
    ws = _neck_workspace("prune_scores", B, _ncap(s_rows), 0, dev)
    out = torch.empty((q_coords.shape[0],), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_neck_prune_scores(q_coords.data_ptr(), int(q_coords.shape[0]), s_coords.data_ptr(), _int32_array(s_rows), B,
                                                int(tensor_stride), scores.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
               "ptx_neck_prune_scores")
    return out


def topk_prune(scores: torch.Tensor, coords: torch.Tensor, scene_rows: Sequence[int], feats: torch.Tensor, k: int,
               differentiable: bool = False):
    """``(coords, scene_rows, feats, keep (n,) bool)`` of the per-scene top-k prune: every scene keeps its ``min(rows, k)`` rows with the
    largest scores in their order (``neck_host.topk_keep_host`` / ``prune_host``, bit for bit; ``ptx_neck_topk_prune``).  Ties go to the
    lower row index; the new scene ends need no wait.  Inference-only unless ``differentiable=True``: then, with grad mode on and
    ``feats`` requiring grad, the gradient flows to the kept rows (``dfeats[i] = g[dest[i]]``, dropped rows ``+0.0``, pure copies); the
    scores never get one (the reference selects under ``torch.no_grad()``) and must not require grad."""
    if differentiable and _wants_grad(scores):
        raise ValueError("topk_prune(differentiable=True): the scores select rows and get no gradient, but they require grad; detach them")
    train = _train("topk_prune", differentiable, scores, feats)
    feats_in = feats
    if not (scores.is_cuda and feats.is_cuda):
        raise RuntimeError("topk_prune (HIP) needs GPU tensors: there is no CPU path")
    dev = feats.device
    B, n = len(scene_rows), int(scene_rows[-1])
    scores, feats = _f32(scores, "topk_prune", dev).reshape(-1), _f32(feats, "topk_prune", dev)
    coords = _rows("topk_prune", coords, n)
    if scores.numel() != n or feats.dim() != 2 or feats.shape[0] != n:
        raise ValueError(f"topk_prune: {n} scores and feats ({n},C) expected, got {scores.numel()}, {tuple(feats.shape)}")
    ends = neck_host.topk_scene_rows(scene_rows, k)
    C = int(feats.shape[1])
    dest = torch.empty((n,), dtype=torch.int32, device=dev)
    out_c = torch.empty((ends[-1], 4), dtype=torch.int32, device=dev)
    out = torch.empty((ends[-1], C), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_neck_topk_prune(scores.data_ptr(), _int32_array(scene_rows), B, int(k), coords.data_ptr(), feats.data_ptr(), C,
                                              dest.data_ptr(), out_c.data_ptr(), out.data_ptr(), _stream(dev)), "ptx_neck_topk_prune")
    if train:
        out = _RouteFn.apply(out, (dest,), _f32_grad(feats_in))
    return out_c, ends, out, dest >= 0


class _HeadFn(torch.autograd.Function):
    """feats (n,C), kernel (any shape of C x K elements, (C,K) order), bias (any shape of K elements) or None -> (cls, score); the score is
    not differentiable."""

    @staticmethod
    def forward(ctx, feats, kernel, bias):
        n, C = int(feats.shape[0]), int(feats.shape[1])
        K = kernel.numel() // C
        dev = feats.device
        cls = torch.empty((n, K), dtype=torch.float32, device=dev)
        score = torch.empty((n,), dtype=torch.float32, device=dev)
        _abi.check(_abi.lib().ptx_neck_head(feats.data_ptr(), n, C, kernel.data_ptr(), _ptr(bias), K, cls.data_ptr(), score.data_ptr(),
                                            _stream(dev)), "ptx_neck_head")
        ctx.save_for_backward(feats, kernel)
        ctx.shapes = (tuple(kernel.shape), None if bias is None else tuple(bias.shape))
        ctx.mark_non_differentiable(score)
        return cls, score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dcls, _dscore):
        feats, kernel = ctx.saved_tensors
        need_f, need_k, need_b = ctx.needs_input_grad
        dev = feats.device
        dcls = _f32_grad(dcls)
        n, C = int(feats.shape[0]), int(feats.shape[1])
        K = kernel.numel() // C
        lib = _abi.lib()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
        dfeats = new(n, C) if need_f else None
        dk = new(C, K) if need_k else None
        db = new(K) if need_b else None
        nbytes = lib.ptx_neck_head_bwd_workspace_bytes(n, C, K)
        if nbytes == 0:
            raise ValueError(f"neck_head backward: unsupported size, {n} rows, C={C}, K={K}")
        ws = _workspace("head_bwd", nbytes, dev) if (need_k or need_b) else None
        _abi.check(lib.ptx_neck_head_bwd(dcls.data_ptr(), feats.data_ptr(), kernel.data_ptr(), n, C, K, _ptr(dfeats), _ptr(dk), _ptr(db), _ptr(ws),
                                         0 if ws is None else ws.numel(), _stream(dev)), "ptx_neck_head_bwd")
        return (dfeats, None if dk is None else dk.reshape(ctx.shapes[0]), None if db is None else db.reshape(ctx.shapes[1]))


def neck_head(feats: torch.Tensor, kernel: torch.Tensor, bias: Optional[torch.Tensor] = None, differentiable: bool = False):
    """``(cls (n,K) fp32, score (n,) fp32)``: ``feats (n,C) @ kernel (1,C,K) + bias`` and its maximum over the classes in one kernel
    (``neck_host.head_host``; ``ptx_neck_head``).  C a multiple of 64 up to 512, 1 <= K <= 16.  A NaN class score makes the row's
    score NaN, as numpy's ``max`` does.  Inference-only unless ``differentiable=True``: then, with grad mode on and ``feats`` /
    ``kernel`` / ``bias`` requiring grad, ``cls`` is recorded for autograd (``neck_host.head_bwd_host``; ``ptx_neck_head_bwd``; same output
    bits) and ``score`` is returned detached, as the reference takes it under ``torch.no_grad()``."""
    train = _train("neck_head", differentiable, feats, kernel, bias)
    grad_in = (feats, kernel, bias)
    if not feats.is_cuda:
        raise RuntimeError("neck_head (HIP) needs GPU tensors: there is no CPU path")
    dev = feats.device
    feats, kernel = _f32(feats, "neck_head", dev), _f32(kernel, "neck_head", dev)
    if feats.dim() != 2 or kernel.numel() % max(int(feats.shape[1]), 1) or kernel.reshape(-1, kernel.shape[-1]).shape[0] != feats.shape[1]:
        raise ValueError(f"neck_head: feats (n,C) and kernel (1,C,K) expected, got {tuple(feats.shape)}, {tuple(kernel.shape)}")
    n, C, K = int(feats.shape[0]), int(feats.shape[1]), int(kernel.shape[-1])
    (b,) = _channel_vectors("neck_head", K, dev, bias=bias)
    if train:
        return _HeadFn.apply(*(_f32_grad(t) for t in grad_in))
    cls = torch.empty((n, K), dtype=torch.float32, device=dev)
    score = torch.empty((n,), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_neck_head(feats.data_ptr(), n, C, kernel.data_ptr(), _ptr(b), K, cls.data_ptr(), score.data_ptr(), _stream(dev)),
               "ptx_neck_head")
    return cls, score


class GenerativeConvTranspose(nn.Module):
    """``ME.MinkowskiGenerativeConvolutionTranspose(in_channels, out_channels, kernel_size=2, stride=2, dimension=3)``: the parameter is
    ME's ``kernel (8, Cin, Cout)``, no bias.  ``forward(coords, scene_rows, tensor_stride, feats, scale=, shift=, act=)`` =
    ``conv_transpose_gen``.  ``differentiable=True`` (an attribute, forwarded by ``forward``) makes the layer trainable; the default
    stays inference-only."""

    def __init__(self, in_channels: int, out_channels: int, differentiable: bool = False):
        super().__init__()
        self.differentiable = bool(differentiable)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel = nn.Parameter(torch.empty(8, self.in_channels, self.out_channels))
        with torch.no_grad():
            self.kernel.normal_(0.0, (2.0 / (8 * self.out_channels)) ** 0.5)

    def forward(self, coords, scene_rows, tensor_stride, feats, scale=None, shift=None, act: int = ACT_NONE):
        return conv_transpose_gen(coords, scene_rows, tensor_stride, feats, self.kernel, scale, shift, act, differentiable=self.differentiable)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, kernel_size=2, stride=2"


class _ELU(nn.Module):
    """The place of ``ME.MinkowskiELU`` in a block: no parameters; the activation itself rides in the preceding convolution's epilogue."""

    def forward(self, x):
        return x


def _fold_host(bn, dt):
    w, b, mean, var = (_np(t, dt) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    scale = w * (1 / np.sqrt(var + dt.type(bn.eps))).astype(dt)
    return scale, b - mean * scale


class MinkNeck(nn.Module):
    """``MinkNeck(num_classes, in_channels, out_channels, voxel_size, pts_prune_threshold)`` of the reference (necks/mink_neck.py): the
    sparse FPN and the classification head whose scores prune the next finer level.  The ``state_dict`` is the reference's by name and
    shape -- ``up_block_{i}.0.kernel (8, C_i, C_{i-1})``, ``up_block_{i}.1.bn.*``, ``up_block_{i}.3.kernel (27, C_{i-1}, C_{i-1})``,
    ``up_block_{i}.4.bn.*``, ``out_block_{i}.0.kernel (27, C_i, out)``, ``out_block_{i}.1.bn.*``, ``conv_cls.kernel (1, out, K)``,
    ``conv_cls.bias (1, K)``; the ELUs are parameter-free placeholders -- so a reference checkpoint's ``neck_3d.*`` loads with
    ``strict=True``.

    ``forward(levels, batch_size)``: ``levels`` = the backbone's ``SparseLevel`` list, finest first, with the sampled image features
    already concatenated to ``feats`` by the caller; returns ``(feats, scores, points)``, each a list of ``batch_size`` tensors with the
    levels concatenated per scene from the coarsest to the finest, ``points = coords[:, 1:4] * voxel_size`` in fp32.  The loop is
    mink_neck.py:142-161.  Every BatchNorm is folded into its convolution's ``scale`` / ``shift`` with the ELU in the same epilogue.
    Inference-only by default: a BatchNorm in training mode, or an input or parameter that requires grad with grad mode on, raises
    ``NotImplementedError``.  ``differentiable=True`` (the last constructor argument, forwarded to the children) adds the training chain:
    with every BatchNorm in training mode each block runs as a raw convolution followed by the BatchNorm on the batch statistics with the
    ELU fused (running statistics and ``num_batches_tracked`` updated), the prune scores and the top-k see the detached score, and
    autograd reaches every parameter and every level's ``feats``; in ``.eval()`` with nothing requiring grad (or under ``no_grad``) the
    module takes the folded route above, bit for bit; eval-mode BatchNorms with grads wanted raise ``NotImplementedError`` (call
    ``bn.train()``: training through frozen BatchNorms is out of scope).  The two k3 convolutions of a level read different row sets
    (``up_block.3`` the generated children, ``out_block.0`` the pruned union), so each has its own kernel map."""

    def __init__(self, num_classes: int, in_channels: Sequence[int], out_channels: int, voxel_size: float, pts_prune_threshold: int,
                 train_cfg: Optional[dict] = None, test_cfg: Optional[dict] = None, init_cfg: Optional[dict] = None,
                 differentiable: bool = False):
        super().__init__()
        self.differentiable = d = bool(differentiable)
        if not 1 <= int(num_classes) <= 16:
            raise ValueError(f"MinkNeck: num_classes must be 1 to 16, got {num_classes}")
        self.num_classes, self.in_channels, self.out_channels = int(num_classes), tuple(int(c) for c in in_channels), int(out_channels)
        self.voxel_size, self.pts_prune_threshold = voxel_size, int(pts_prune_threshold)
        self.train_cfg, self.test_cfg, self.init_cfg = train_cfg, test_cfg, init_cfg
        for i, c in enumerate(self.in_channels):
            if i > 0:
                lower = self.in_channels[i - 1]
                setattr(self, f"up_block_{i}", nn.Sequential(GenerativeConvTranspose(c, lower, differentiable=d),
                                                             SparseBatchNorm(lower, differentiable=d), _ELU(),
                                                             SparseConv3d(lower, lower, kernel_size=3, differentiable=d),
                                                             SparseBatchNorm(lower, differentiable=d), _ELU()))
            setattr(self, f"out_block_{i}", nn.Sequential(SparseConv3d(c, self.out_channels, kernel_size=3, differentiable=d),
                                                          SparseBatchNorm(self.out_channels, differentiable=d), _ELU()))
        self.conv_cls = SparseConv3d(self.out_channels, self.num_classes, kernel_size=1, bias=True, differentiable=d)

    def init_weights(self) -> None:
        """mink_neck.py:128-131: ``conv_cls.kernel ~ N(0, 0.01)``, ``conv_cls.bias = bias_init_with_prob(0.01) = -log(99)``."""
        with torch.no_grad():
            nn.init.normal_(self.conv_cls.kernel, std=0.01)
            nn.init.constant_(self.conv_cls.bias, -math.log((1 - 0.01) / 0.01))

    def _training_chain(self, levels) -> bool:
        """Whether this call takes the training chain; the raises of the routes that do not exist."""
        if not self.differentiable:
            self._check_inference(levels)
            return False
        modes = [m.bn.training for m in self.modules() if isinstance(m, SparseBatchNorm)]
        if all(modes):
            return True
        if any(modes):
            raise NotImplementedError("MinkNeck(differentiable=True): some BatchNorms are in training mode and some are not; the training chain "
                                      "needs all of them in training mode (bn.train()), the folded route none")
        if _wants_grad(*[lv.feats for lv in levels if isinstance(lv.feats, torch.Tensor)], *self.parameters()):
            raise NotImplementedError("MinkNeck(differentiable=True) with eval-mode BatchNorms: training through frozen BatchNorms is not "
                                      "implemented; call bn.train() on the neck's BatchNorms (module.train()), or run under torch.no_grad()")
        return False

    def _check_inference(self, levels) -> None:
        for m in self.modules():
            if isinstance(m, SparseBatchNorm) and m.bn.training:
                raise NotImplementedError("MinkNeck is inference-only: a BatchNorm in training mode needs the backward pass and the batch "
                                          "statistics of the neck, which are not implemented; call .eval()")
        _train("MinkNeck", False, *[lv.feats for lv in levels if isinstance(lv.feats, torch.Tensor)], *self.parameters())

    def forward(self, levels: Sequence[SparseLevel], batch_size: int, keep_out: Optional[list] = None):
        """``keep_out``: a list that receives the keep mask ``(rows,) bool`` of every pruning step, coarsest step first."""
        if len(levels) != len(self.in_channels):
            raise ValueError(f"MinkNeck: {len(self.in_channels)} levels expected, got {len(levels)}")
        chain = self._training_chain(levels)
        if not all(isinstance(lv.feats, torch.Tensor) and lv.feats.is_cuda for lv in levels):
            raise RuntimeError("MinkNeck (HIP) needs GPU tensors: there is no CPU path")
        top = len(levels) - 1
        c, ends, ts, x = levels[top].coords, list(levels[top].scene_rows), int(levels[top].tensor_stride), levels[top].feats
        if len(ends) != int(batch_size):
            raise ValueError(f"MinkNeck: batch_size={batch_size} but the levels hold {len(ends)} scenes")
        d = self.differentiable
        out_levels = []
        score = None
        for i in range(top, -1, -1):
            if i < top:
                up = getattr(self, f"up_block_{i + 1}")
                if chain:                                    # conv (raw) -> training BatchNorm + ELU, twice (backbone._conv_bn's training branch)
                    gc, ge, g = up[0](c, ends, ts, x)
                    g = up[1](g, elu=True)
                    g = up[4](up[3](g, sparse.kernel_map(gc, ge, ts // 2, 3, 1)), elu=True)
                else:
                    s0, h0 = sparse.bn_fold(up[1].bn)
                    gc, ge, g = up[0](c, ends, ts, x, scale=s0, shift=h0, act=ACT_ELU)
                    s1, h1 = sparse.bn_fold(up[4].bn)
                    g = up[3](g, sparse.kernel_map(gc, ge, ts // 2, 3, 1), scale=s1, shift=h1, elu=True)
                lv = levels[i]
                if int(lv.tensor_stride) != ts // 2:
                    raise ValueError(f"MinkNeck: level {i} has tensor stride {lv.tensor_stride}, {ts // 2} expected")
                uc, ue, u = union_add(lv.coords, lv.scene_rows, lv.feats, gc, ge, g, ts // 2, differentiable=d)
                with torch.no_grad():                        # mink_neck.py:163-186: the prune is taken under no_grad
                    q = prune_scores(uc, c, ends, ts, score)
                c, ends, x, keep = topk_prune(q, uc, ue, u, self.pts_prune_threshold, differentiable=d)
                ts //= 2
                if keep_out is not None:
                    keep_out.append(keep)
            ob = getattr(self, f"out_block_{i}")
            if chain:
                out = ob[1](ob[0](x, sparse.kernel_map(c, ends, ts, 3, 1)), elu=True)
            else:
                so, ho = sparse.bn_fold(ob[1].bn)
                out = ob[0](x, sparse.kernel_map(c, ends, ts, 3, 1), scale=so, shift=ho, elu=True)
            cls, score = neck_head(out, self.conv_cls.kernel, self.conv_cls.bias, differentiable=d)
            out_levels.append((out, cls, c[:, 1:4].to(torch.float32) * self.voxel_size, ends))
        return self._to_batch(out_levels, int(batch_size), torch.cat)

    @staticmethod
    def _to_batch(out_levels, batch_size: int, cat):
        feats, scores, points = [], [], []
        for b in range(batch_size):
            parts = [[t[(e[b - 1] if b else 0):e[b]] for t in (f, s, p)] for f, s, p, e in out_levels]
            feats.append(cat([p[0] for p in parts]))
            scores.append(cat([p[1] for p in parts]))
            points.append(cat([p[2] for p in parts]))
        return feats, scores, points

    def forward_host(self, levels: Sequence[SparseLevel], batch_size: int, dtype=np.float64, keep: Optional[list] = None,
                     trace: Optional[list] = None, training: bool = False):
        """The same chain from ``neck_host.py`` / ``sparse_host.py`` in numpy ``dtype`` with this module's parameters.  ``keep``: one keep
        mask per pruning step (coarsest step first) that replaces the host's own top-k -- the device's, when a test holds the device's
        features to this chain on the device's row sets.  ``trace``: a list that receives, per pruning step,
        ``dict(scores, scene_rows, keep)`` -- the interpolated scores, the scene ends before the prune and the host's OWN top-k mask.
        ``training``: the training chain's forward -- every BatchNorm on the batch statistics through ``sparse_norm_host`` plus the ELU;
        the running statistics are not updated."""
        dt = np.dtype(dtype)

        def block(z, bn):                                    # a training BatchNorm + ELU on the raw convolution z
            return sparse.sparse_norm_host(z, [z.shape[0]], bn.eps, _np(bn.weight, dt), _np(bn.bias, dt), elu=True)

        top = len(levels) - 1
        c, ends, ts = _np(levels[top].coords, np.int32), [int(e) for e in levels[top].scene_rows], int(levels[top].tensor_stride)
        x = _np(levels[top].feats, dt)
        out_levels = []
        score = None
        step = 0
        for i in range(top, -1, -1):
            if i < top:
                up = getattr(self, f"up_block_{i + 1}")
                if training:
                    gc, ge, g = neck_host.conv_transpose_gen_host(c, ends, ts, x, _np(up[0].kernel, dt))
                    g = block(g, up[1].bn)
                    g = block(sparse.sparse_conv3d_host(g, sparse.kernel_map_host(gc, ge, ts // 2, 3, 1)[2], _np(up[3].kernel, dt)), up[4].bn)
                else:
                    s0, h0 = _fold_host(up[1].bn, dt)
                    gc, ge, g = neck_host.conv_transpose_gen_host(c, ends, ts, x, _np(up[0].kernel, dt), s0, h0, ACT_ELU)
                    s1, h1 = _fold_host(up[4].bn, dt)
                    g = neck_host.sparse_conv3d_act_host(g, sparse.kernel_map_host(gc, ge, ts // 2, 3, 1)[2], _np(up[3].kernel, dt), scale=s1,
                                                         shift=h1, act=ACT_ELU)
                lv = levels[i]
                uc, ue, u = neck_host.union_add_host(_np(lv.coords, np.int32), lv.scene_rows, _np(lv.feats, dt), gc, ge, g)
                q = neck_host.prune_scores_host(uc, c, ends, ts, score)
                own = neck_host.topk_keep_host(q, ue, self.pts_prune_threshold)
                if trace is not None:
                    trace.append(dict(scores=q, scene_rows=list(ue), keep=own))
                mask = own if keep is None else _np(keep[step], bool)
                step += 1
                c, ends, x = neck_host.prune_host(mask, uc, ue, u)
                ts //= 2
            ob = getattr(self, f"out_block_{i}")
            if training:
                out = block(sparse.sparse_conv3d_host(x, sparse.kernel_map_host(c, ends, ts, 3, 1)[2], _np(ob[0].kernel, dt)), ob[1].bn)
            else:
                so, ho = _fold_host(ob[1].bn, dt)
                out = neck_host.sparse_conv3d_act_host(x, sparse.kernel_map_host(c, ends, ts, 3, 1)[2], _np(ob[0].kernel, dt), scale=so,
                                                       shift=ho, act=ACT_ELU)
            cls, score = neck_host.head_host(out, _np(self.conv_cls.kernel, dt)[0], _np(self.conv_cls.bias, dt))
            out_levels.append((out, cls, c[:, 1:4].astype(np.float32) * np.float32(self.voxel_size), ends))
        return self._to_batch(out_levels, int(batch_size), np.concatenate)


# (as for MinkResNet: in a real EmbodiedScan install the reference's own class holds the name)
if REGISTRY_BACKEND != "embodiedscan" and MODELS.get("MinkNeck") is None:
    MODELS.register_module(name="MinkNeck", module=MinkNeck)
