"""The transformer decoder behind ``QuerySelect``: the eval forward of ``SparseFeatureFusionTransformerDecoder``
(models/layers/ground_transformer/decoder.py; called by ``forward_decoder``, detectors/sparse_featfusion_grounder_preshape.py:582-621)
and the per-layer text scores of ``GroundingHead.forward`` (dense_heads/grounding_head.py:427-467) on the device.

Six calls into ``csrc/decoder.hip`` on the current stream -- ``posembed``, ``linear``, ``attention``, ``layer_norm`` (with ``linear``:
``linear_add_ln``), ``boxes`` and ``contrastive_scores`` -- each restated in numpy by ``decoder_host.py``, which is their specification.
No device synchronise, no torch op on the data path; fp32 on the exact-fp32 matrix instruction; no float atomics and fixed summation
orders, so two calls give the same bits.  ``key`` and ``key_pos`` do not change across the layers, so the key and value projections of
every layer's scene attention leave the layer loop: one ``linear`` launch per group of layers (``[K_0 .. K_n | V_0 .. V_n]``, at most 4096
columns) ahead of it; the text keys and values likewise unless ``T == K`` (below).

The rules of mmcv's attention wrapper: identity (the query before its positions) plus the attention output; positions on ``q`` and ``k``
only; when ``key_pos`` is None and ``query_pos.shape == key.shape`` the keys receive ``query_pos`` -- so when ``T == K`` the TEXT keys of
the text cross attention receive ``query_pos``, as in the reference.

Parity-unpinned against ``nn.MultiheadAttention``: a masked key is never read (a NaN or inf under it leaves no trace; torch multiplies it
by a zero weight).  A query whose every key is masked gets zeros from the attention, so the layer adds ``out_proj.bias`` only: what torch
2.10 gives in both grad modes; older releases give NaN.

Under autograd: ``attention``, ``linear``, ``layer_norm``, ``linear_add_ln``, ``posembed`` (with its BatchNorm in training mode: batch
statistics), ``boxes`` and ``contrastive_scores`` take ``differentiable=True`` and are then one ``torch.autograd.Function`` node each
(``linear_add_ln``: two), with the same forward bits, gradients specified by ``decoder_grad_host.py``, no synchronise and no atomics.
``GroundingDecoder(..., differentiable=True)`` in ``.train()`` runs the chain built from them: a loss on the hidden states and boxes
reaches ``query``, ``key``, ``text_feats``, every parameter the reference trains and the regression branches.  Without the keyword
they detach their operands as before and the module is the eval forward.

Out of scope: training through frozen BatchNorms, double backward, dropout, attention masks, bf16, ``num_reg=12`` and
the FCAF coder, the loss and ``predict_by_feat``.  There is no CPU path: tensors must be on the GPU and the library must be built."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _abi, decoder_host, query_select
from . import train as _train_ops
from ._doors import (MAX_QUERIES, MAX_SCENES, MAX_TEXT, PreparedOperands, _f32, _f32_grad, _gpu, _mask_bytes, _np, _ptr, _stream, _wants_grad,
                     _width)
from .query_select import QuerySelect

__all__ = ["GroundingDecoder", "attention", "boxes", "contrastive_scores", "layer_norm", "linear", "linear_add_ln", "posembed", "posembed_folded"]

MAX_CIN, MAX_COUT, MAX_FFN = 2048, 4096, 2048
LN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------ the operators
class _Folded:
    """A ``PositionEmbeddingLearned`` in eval as ``ptx_dec_posembed`` takes it: the BatchNorm folded into the first Conv1d in float64 on
    the host, rounded once."""

    def __init__(self, head: nn.Sequential, dev):
        conv1, bn, conv2 = head[0], head[1], head[3]
        f64 = lambda t: t.detach().cpu().double().numpy()      # noqa: E731
        w1, b1 = decoder_host.fold_posembed(f64(conv1.weight), f64(conv1.bias), f64(bn.weight), f64(bn.bias), f64(bn.running_mean),
                                            f64(bn.running_var), bn.eps)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)      # noqa: E731
        self.cin, self.C = int(w1.shape[1]), int(w1.shape[0])
        self.w1, self.b1 = put(w1), put(b1)
        self.w2 = conv2.weight.detach().to(dev, torch.float32).reshape(self.C, self.C).contiguous()
        self.b2 = conv2.bias.detach().to(dev, torch.float32).contiguous()


def _fold(module, dev) -> _Folded:
    if isinstance(module, _Folded):
        return module
    head = module.position_embedding_head if hasattr(module, "position_embedding_head") else module
    if head[1].training:
        raise NotImplementedError("posembed: the BatchNorm is in training mode; the eval forward only")
    return _Folded(head, dev)


def _posembed_head(module) -> nn.Sequential:
    return module.position_embedding_head if hasattr(module, "position_embedding_head") else module


def posembed(x: torch.Tensor, module, differentiable: bool = False, repeat: int = 1) -> torch.Tensor:
    """``(B,N,C) fp32``: ``PositionEmbeddingLearned`` in eval on ``x (B,N,cin)``, ``cin`` 1 to 9 -- Conv1d, the BatchNorm folded into it,
    ReLU (a NaN kept), Conv1d (``decoder_host.posembed_host``; ``ptx_dec_posembed``, one launch).  ``module``: the reference's module
    (or its ``position_embedding_head``).  ``differentiable=True`` with the BatchNorm in training mode: batch statistics over all ``B N``
    rows (``decoder_grad_host.posembed_train_host``; ``ptx_dec_posembed_stats`` folds them on the device, then the same launch), the
    running statistics moved ``repeat`` times and ``num_batches_tracked`` advanced by ``repeat``; one autograd node with gradients to the
    six parameters, none to ``x`` (an ``x`` that requires grad is refused).  In eval with a parameter that requires grad it raises: a
    frozen BatchNorm is not trained through."""
    if differentiable and not isinstance(module, _Folded):
        head = _posembed_head(module)
        conv1, bn, conv2 = head[0], head[1], head[3]
        if bn.training:
            if _wants_grad(x):
                raise NotImplementedError("posembed: x requires grad; the position embedding passes no gradient to its coordinates (the "
                                          "reference detaches them): detach x")
            return _posembed_train(x, conv1, bn, conv2, int(repeat))
        if _wants_grad(conv1.weight, conv1.bias, bn.weight, bn.bias, conv2.weight, conv2.bias):
            raise NotImplementedError("posembed: differentiable=True with the BatchNorm in eval mode and a parameter that requires grad: "
                                      "training through a frozen BatchNorm is not implemented; call .train() or freeze the parameters")
    _gpu("posembed", x)
    dev = x.device
    x = _f32(x, "posembed", dev)
    f = _fold(module, dev)
    if x.dim() != 3 or x.shape[2] != f.cin:
        raise ValueError(f"posembed: x (B,N,{f.cin}) expected, got {tuple(x.shape)}")
    _width("posembed", f.C)
    B, N = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((B, N, f.C), dtype=torch.float32, device=dev)
    if B * N:
        _abi.check(_abi.lib().ptx_dec_posembed(x.data_ptr(), B * N, f.cin, f.w1.data_ptr(), f.b1.data_ptr(), f.w2.data_ptr(),
                                               f.b2.data_ptr(), f.C, out.data_ptr(), _stream(dev)), "ptx_dec_posembed")
    return out


def _slab_workspace(n: int, C: int, nv: int, dev) -> torch.Tensor:
    """The doubles the row-slab reductions of ``csrc/decoder_train.hip`` take for ``nv`` values per channel."""
    nbytes = int(_abi.lib().ptx_dec_train_workspace_bytes(n, C, nv))
    if nbytes == 0:
        raise ValueError(f"decoder: {n} rows of width {C} are outside the training operators' range (1 to 2^24 rows)")
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)


def _posembed_train(x, conv1, bn, conv2, repeat: int) -> torch.Tensor:
    """``posembed``'s checks on the training path, all before the first launch."""
    _gpu("posembed", x, conv1.weight)
    dev = x.device
    cin, C = int(conv1.in_channels), _width("posembed", conv1.out_channels)
    if x.dim() != 3 or x.shape[2] != cin or not 1 <= cin <= 9:
        raise ValueError(f"posembed: x (B,N,{cin}) with cin from 1 to 9 expected, got {tuple(x.shape)}")
    n = int(x.shape[0]) * int(x.shape[1])
    if n == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {[1, C, 1]}")
    if not 1 <= repeat <= 64:
        raise ValueError(f"posembed: repeat must be 1 to 64, got {repeat}")
    if bn.momentum is None or not bn.affine:
        raise NotImplementedError("posembed: a BatchNorm with momentum=None (cumulative average) or without affine parameters is not "
                                  "implemented")
    if bn.track_running_stats:
        for t in (bn.running_mean, bn.running_var):
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"posembed: the running statistics must be contiguous fp32 on {dev}")
    if n == 0:
        return torch.empty((int(x.shape[0]), int(x.shape[1]), C), dtype=torch.float32, device=dev)
    return _PosembedTrainFn.apply(x, conv1.weight, conv1.bias, bn.weight, bn.bias, conv2.weight, conv2.bias, bn, repeat)


def _fold_batch(x, n: int, w1, b1, gamma, beta, bn, repeat: int):
    """``ptx_dec_posembed_stats`` on fp32 operands: ``(w1' (C,cin), b1' (C), stats (2,C) = (mean | rstd))`` of the ``n`` rows of ``x``;
    with ``repeat > 0`` the BatchNorm's running statistics move ``repeat`` times and ``num_batches_tracked`` advances by ``repeat``."""
    dev = x.device
    C, cin = int(w1.shape[0]), int(w1.shape[1])
    w1f, b1f = torch.empty((C, cin), dtype=torch.float32, device=dev), torch.empty((C,), dtype=torch.float32, device=dev)
    stats = torch.empty((2, C), dtype=torch.float32, device=dev)
    ws = _slab_workspace(n, C, 2, dev)
    track = bool(bn.track_running_stats) and repeat > 0
    _abi.check(_abi.lib().ptx_dec_posembed_stats(x.data_ptr(), n, cin, w1.data_ptr(), b1.data_ptr(), gamma.data_ptr(), beta.data_ptr(), C,
                                                 float(bn.eps), float(bn.momentum), repeat, _ptr(bn.running_mean if track else None),
                                                 _ptr(bn.running_var if track else None), w1f.data_ptr(), b1f.data_ptr(), stats.data_ptr(),
                                                 ws.data_ptr(), ws.numel() * 8, _stream(dev)), "ptx_dec_posembed_stats")
    if track:
        torch.autograd.graph.increment_version(bn.running_mean)      # the kernel wrote them: the prepared eval operands are keyed on this
        torch.autograd.graph.increment_version(bn.running_var)
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(repeat)
    return w1f, b1f, stats


def posembed_folded(x: torch.Tensor, module) -> _Folded:
    """The operands ``posembed``'s training forward hands to its ``ptx_dec_posembed`` launch: the BatchNorm's batch statistics over the
    rows of ``x`` and its affine folded into the first Conv1d on the device.  Moves no running statistics.  ``posembed(x, <this>)`` is
    the training forward's result bit for bit."""
    _gpu("posembed", x)
    dev = x.device
    head = _posembed_head(module)
    conv1, bn, conv2 = head[0], head[1], head[3]
    x = _f32(x, "posembed", dev)
    n = x.numel() // int(conv1.in_channels)
    if n < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got {n} rows")
    f = _Folded.__new__(_Folded)
    f.cin, f.C = int(conv1.in_channels), _width("posembed", conv1.out_channels)
    put = lambda t: _f32(t, "posembed", dev)      # noqa: E731
    f.w1, f.b1, _ = _fold_batch(x, n, put(conv1.weight), put(conv1.bias), put(bn.weight), put(bn.bias), bn, 0)
    f.w2, f.b2 = put(conv2.weight).reshape(f.C, f.C), put(conv2.bias)
    return f


class _PosembedTrainFn(torch.autograd.Function):
    """``posembed`` with batch statistics as one node.  Forward: ``ptx_dec_posembed_stats`` (the moments of ``z = x W1^T + b1`` over
    row slabs, merged by Chan's formula in double; the fold; the running statistics) and ``ptx_dec_posembed`` on the folded first
    layer -- the hidden tensor never exists.  Saved: ``x``, the parameters, ``(mean, rstd)`` and the folded ``(w1', b1')`` (``C (cin +
    1)`` floats, so that the backward's ReLU mask is the forward's).  Backward: the hidden tensor recomputed
    (``ptx_dec_posembed_hidden``), ``dW2 = dout^T h`` and ``dh = dout W2`` (``ptx_op_gemm``), ``db2`` (``ptx_op_colsum``), the rest in
    ``ptx_dec_posembed_bwd``."""

    @staticmethod
    def forward(ctx, x, w1, b1, gamma, beta, w2, b2, bn, repeat):
        dev = x.device
        C, cin = int(w1.shape[0]), int(w1.shape[1])
        B, N = int(x.shape[0]), int(x.shape[1])
        n = B * N
        ctx.meta = [(tuple(t.shape), t.dtype) for t in (w1, b1, gamma, beta, w2, b2)]
        x = _f32(x, "posembed", dev)
        w1, b1, gamma, beta = (_f32(t, "posembed", dev) for t in (w1, b1, gamma, beta))
        w2, b2 = _f32(w2, "posembed", dev), _f32(b2, "posembed", dev)
        w1f, b1f, stats = _fold_batch(x, n, w1, b1, gamma, beta, bn, repeat)
        out = torch.empty((B, N, C), dtype=torch.float32, device=dev)
        _abi.check(_abi.lib().ptx_dec_posembed(x.data_ptr(), n, cin, w1f.data_ptr(), b1f.data_ptr(), w2.data_ptr(), b2.data_ptr(), C,
                                               out.data_ptr(), _stream(dev)), "ptx_dec_posembed")
        ctx.save_for_backward(x, w1, b1, gamma, w2, stats, w1f, b1f)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, w1, b1, gamma, w2, stats, w1f, b1f = ctx.saved_tensors
        dev = x.device
        C, cin = int(w1.shape[0]), int(w1.shape[1])
        n = x.numel() // cin
        lib = _abi.lib()
        g = _f32(dout, "posembed", dev).view(n, C)
        need = ctx.needs_input_grad[1:7]
        grads = [None] * 6
        with torch.cuda.device(dev):
            w2m = w2.view(C, C)
            if need[4]:
                h = torch.empty((n, C), dtype=torch.float32, device=dev)
                _abi.check(lib.ptx_dec_posembed_hidden(x.data_ptr(), n, cin, w1f.data_ptr(), b1f.data_ptr(), C, h.data_ptr(), _stream(dev)),
                           "ptx_dec_posembed_hidden")
                dw2 = torch.empty((C, C), dtype=torch.float32, device=dev)
                _dweight_rows(g, 0, C, h, dw2)
                grads[4] = dw2
            if need[5]:
                grads[5] = _train_ops.colsum(g)
            if any(need[:4]):
                dh = _train_ops.mm(g, w2m)
                dgb = torch.empty((2, C), dtype=torch.float32, device=dev)
                dw1, db1 = torch.empty((C, cin), dtype=torch.float32, device=dev), torch.empty((C,), dtype=torch.float32, device=dev)
                ws = _slab_workspace(n, C, max(cin + 1, 2), dev)
                _abi.check(lib.ptx_dec_posembed_bwd(x.data_ptr(), n, cin, w1.data_ptr(), b1.data_ptr(), gamma.data_ptr(), stats.data_ptr(),
                                                    w1f.data_ptr(), b1f.data_ptr(), dh.data_ptr(), C, dgb.data_ptr(), dw1.data_ptr(),
                                                    db1.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(dev)), "ptx_dec_posembed_bwd")
                grads[0], grads[1], grads[2], grads[3] = dw1, db1, dgb[1], dgb[0]
        out = [g_.reshape(shape).to(dt) if (g_ is not None and wanted) else None for g_, (shape, dt), wanted in zip(grads, ctx.meta, need)]
        return (None,) + tuple(out) + (None, None)


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], add: Optional[torch.Tensor] = None, relu: bool = False,
           add_cols: Optional[int] = None, residual: Optional[torch.Tensor] = None, differentiable: bool = False) -> torch.Tensor:
    """``(...,Cout) fp32 = act((x + add) @ weight.T + bias) (+ residual)`` on ``x (...,Cin)``: the add is fused into the operand load and
    reaches the output columns below ``add_cols`` only (a multiple of 64; default: all).  ``Cin``: a multiple of 64 up to 2048;
    ``Cout``: a multiple of 64 up to 4096.  The ReLU keeps a NaN (``decoder_host.linear_host``; ``ptx_dec_linear``, one launch).
    ``differentiable=True``: one autograd node with gradients to ``x``, ``add``, ``weight``, ``bias``, ``residual``, the same forward
    bits (``decoder_grad_host.linear_bwd_host``); ``relu`` together with ``residual`` is refused there."""
    if differentiable:
        if relu and residual is not None:
            raise NotImplementedError("linear: differentiable=True with relu and a residual is not implemented (the decoder never uses it; "
                                      "the ReLU's mask would need a second saved tensor)")
        if _wants_grad(x, weight, bias, add, residual):
            return _LinearFn.apply(x, weight, bias, add, residual, bool(relu), add_cols)
    _gpu("linear", x, weight, bias, add, residual)
    dev = x.device
    x, weight, bias = _f32(x, "linear", dev), _f32(weight, "linear", dev), _f32(bias, "linear", dev)
    add, residual = _f32(add, "linear", dev), _f32(residual, "linear", dev)
    if x.dim() < 2 or weight.dim() != 2 or weight.shape[1] != x.shape[-1]:
        raise ValueError(f"linear: x (...,Cin) and weight (Cout,Cin) expected, got {tuple(x.shape)}, {tuple(weight.shape)}")
    cin, cout = int(x.shape[-1]), int(weight.shape[0])
    if cin % 64 or not 64 <= cin <= MAX_CIN or cout % 64 or not 64 <= cout <= MAX_COUT:
        raise ValueError(f"linear: Cin a multiple of 64 up to {MAX_CIN} and Cout a multiple of 64 up to {MAX_COUT}, got {cin}, {cout}")
    if add is not None and tuple(add.shape) != tuple(x.shape):
        raise ValueError(f"linear: add must have x's shape {tuple(x.shape)}, got {tuple(add.shape)}")
    cols = cout if add_cols is None else int(add_cols)
    if cols % 64 or not 0 <= cols <= cout:
        raise ValueError(f"linear: add_cols must be a multiple of 64 from 0 to {cout}, got {cols}")
    if bias is not None and bias.numel() != cout:
        raise ValueError(f"linear: bias ({cout}) expected, got {tuple(bias.shape)}")
    out = torch.empty(tuple(x.shape[:-1]) + (cout,), dtype=torch.float32, device=dev)
    if residual is not None and tuple(residual.shape) != tuple(out.shape):
        raise ValueError(f"linear: residual {tuple(out.shape)} expected, got {tuple(residual.shape)}")
    n = x.numel() // cin
    if n:
        _abi.check(_abi.lib().ptx_dec_linear(x.data_ptr(), _ptr(add), cols, n, weight.data_ptr(), _ptr(bias), cin, cout, int(bool(relu)),
                                             _ptr(residual), out.data_ptr(), _stream(dev)), "ptx_dec_linear")
    return out


def _dweight_rows(g: torch.Tensor, lo: int, hi: int, xs: torch.Tensor, dw: torch.Tensor) -> None:
    """``dw[lo:hi] = g[:, lo:hi].T @ xs`` with ``g (n,Cout)``, ``xs (n,Cin)``: ``ptx_op_gemm`` on the strided column range through
    ``train.mm_rows``, which cuts a long contraction into few tiles into slices over the rows (``ksplit``) that ``ptx_op_colsum`` adds
    in double -- the one rule ``train.mm`` follows too."""
    n, cout = g.shape
    cin = int(xs.shape[1])
    _train_ops.mm_rows(g, xs, dw, hi - lo, cin, n, a=(1, cout), b=(cin, 1), a_off=lo, c_off=lo * cin)


class _LinearFn(torch.autograd.Function):
    """``linear`` as one node.  Saved: ``x``, ``add``, ``weight`` and, behind a ReLU, the result (its sign is the mask).  The backward is
    the training operators' kernels: ``dpre = dy * (out > 0)`` (``ptx_op_eltwise`` 5), ``dx = dpre W`` and
    ``dadd = dpre[:, :add_cols] W[:add_cols]`` (``ptx_op_gemm``), ``dW[:add_cols] = dpre[:, :add_cols]^T (x + add)`` on the materialised
    sum (rounded as the forward's operand load rounds it) and ``dW[add_cols:] = dpre[:, add_cols:]^T x`` -- every row of ``dW`` written
    once, no accumulate call -- ``dbias = colsum(dpre)`` in double (``ptx_op_colsum``), ``dresidual = dy``."""

    @staticmethod
    def forward(ctx, x, weight, bias, add, residual, relu, add_cols):
        out = linear(x, weight, bias, add, relu, add_cols, residual)
        dev = out.device
        cout = int(weight.shape[0])
        ctx.relu, ctx.cols = relu, (0 if add is None else cout if add_cols is None else int(add_cols))
        ctx.have = (add is not None, relu)
        ctx.meta = [(None, None) if t is None else (tuple(t.shape), t.dtype) for t in (x, weight, bias, add, residual)]
        keep = [_f32(x, "linear", dev), _f32(weight, "linear", dev)]
        if add is not None:
            keep.append(_f32(add, "linear", dev))
        if relu:
            keep.append(out)
        ctx.save_for_backward(*keep)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        saved = list(ctx.saved_tensors)
        x, w = saved[0], saved[1]
        add = saved[2] if ctx.have[0] else None
        out = saved[-1] if ctx.have[1] else None
        dev = dy.device
        cout, cin = int(w.shape[0]), int(w.shape[1])
        n, cols = x.numel() // cin, ctx.cols
        need_x, need_w, need_b, need_add, need_res = ctx.needs_input_grad[:5]
        dy = _f32(dy, "linear", dev)
        grads = [None] * 5
        if need_res:
            grads[4] = dy
        if n == 0:
            for i, (shape, dt) in enumerate(ctx.meta[:4]):
                if shape is not None and ctx.needs_input_grad[i]:
                    grads[i] = torch.zeros(shape, dtype=dt, device=dev)
        else:
            with torch.cuda.device(dev):
                g = dy.view(n, cout)
                if ctx.relu:
                    g = _train_ops.eltwise(5, out.view(n, cout), g)
                x2 = x.view(n, cin)
                if need_x or (need_add and cols == cout):
                    grads[0] = _train_ops.mm(g, w).view(x.shape)
                if need_add:
                    if cols == cout:
                        grads[3] = grads[0]
                    elif cols == 0:
                        grads[3] = torch.zeros_like(x)
                    else:
                        grads[3] = torch.empty_like(x)
                        _train_ops.gemm(g, w, grads[3], n, cin, cols, a=(cout, 1), b=(cin, 1), c=(cin, 1))
                if not need_x:
                    grads[0] = None
                if need_w:
                    dw = torch.empty_like(w)
                    if cols:
                        _dweight_rows(g, 0, cols, x2 if add is None else _train_ops.eltwise(0, x2, add.view(n, cin)), dw)
                    if cols < cout:
                        _dweight_rows(g, cols, cout, x2, dw)
                    grads[1] = dw
                if need_b:
                    grads[2] = _train_ops.colsum(g)
        for i, (shape, dt) in enumerate(ctx.meta):
            if grads[i] is not None:
                grads[i] = grads[i].reshape(shape).to(dt)
        return tuple(grads) + (None, None)


def _rows_view(what: str, t: torch.Tensor, dev) -> Tuple[torch.Tensor, int]:
    """``t (B,n,C)`` as the attention takes it: fp32, unit stride along C, scene b a whole number of rows behind scene b - 1."""
    if t.device != dev or t.dim() != 3:
        raise ValueError(f"{what}: (B,n,C) tensors on {dev} expected, got {tuple(t.shape)} on {t.device}")
    t = t.detach()
    ok = t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(1) % 4 == 0 and t.stride(1) >= t.shape[2] and \
        (t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1)) and t.data_ptr() % 16 == 0
    if not ok:
        t = t.to(torch.float32).contiguous()
    return t, int(t.stride(1))


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], num_heads: int,
              differentiable: bool = False) -> torch.Tensor:
    """``(B,Kq,C) fp32``: multi-head attention of ``q (B,Kq,C)`` over ``k``, ``v (B,L,C)`` with the key padding mask ``mask (B,L)`` bool,
    True = ignore (``None``: no key is masked); ``q`` is scaled by ``1/sqrt(hd)``, heads are merged in the output.  The operands may be column ranges of a wider
    projection output (strided views).  Head dimension 32 or 64.  One flash-style launch: key tiles of 64 in ascending order, an online
    maximum and sum; a tile that is masked throughout is skipped.  A masked key is never read -- a NaN under it leaves no trace
    (parity-unpinned: ``nn.MultiheadAttention`` multiplies it by a zero weight).  A query whose every key is masked gets zeros (torch 2.10;
    older torch gives NaN).  A NaN in an unmasked key or value of a head reaches the outputs of that scene and head
    (``decoder_host.attention_host``; ``ptx_dec_attention``).  ``differentiable=True``: one autograd node with gradients to ``q``, ``k``,
    ``v`` (contiguous ``(B,n,C)``; the slice backward of a strided operand places them), the same forward bits
    (``decoder_grad_host.attention_bwd_host``; ``ptx_dec_attention_stats`` / ``ptx_dec_attention_bwd``)."""
    if differentiable and _wants_grad(q, k, v):
        return _AttentionFn.apply(q, k, v, mask, int(num_heads))
    return _attention(q, k, v, mask, num_heads, False)[0]


def _attention(q, k, v, mask, num_heads, want_stats: bool):
    """``attention``'s checks and launch: ``(out, (q, k, v, mask, stats) as the launch took them)``; ``stats (B,H,Kq,2)`` -- the final
    maximum and sum of every query -- only with ``want_stats``, None when nothing was launched."""
    _gpu("attention", q, k, v, mask)
    dev = q.device
    if q.dim() != 3 or k.dim() != 3 or tuple(v.shape) != tuple(k.shape) or k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2]:
        raise ValueError(f"attention: q (B,Kq,C), k and v (B,L,C) expected, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    B, Kq, C = (int(s) for s in q.shape)
    L, H = int(k.shape[1]), int(num_heads)
    if H < 1 or C % H or C // H not in (32, 64) or C > 512:
        raise ValueError(f"attention: a head dimension of 32 or 64 and C up to 512, got C={C} with {H} heads")
    if not 1 <= B <= MAX_SCENES or not 0 <= Kq <= MAX_QUERIES:
        raise ValueError(f"attention: 1 to {MAX_SCENES} scenes and up to {MAX_QUERIES} queries, got B={B}, Kq={Kq}")
    if mask is not None:
        mask = _mask_bytes("attention", "the mask", mask, (B, L))
    out = torch.empty((B, Kq, C), dtype=torch.float32, device=dev)
    if Kq == 0:
        return out, None
    if L == 0:
        return out.zero_(), None
    (q, ldq), (k, ldk), (v, ldv) = _rows_view("attention", q, dev), _rows_view("attention", k, dev), _rows_view("attention", v, dev)
    if want_stats:
        stats = torch.empty((B, H, Kq, 2), dtype=torch.float32, device=dev)
        _abi.check(_abi.lib().ptx_dec_attention_stats(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, _ptr(mask), B, Kq, L, H, C // H,
                                                      out.data_ptr(), stats.data_ptr(), _stream(dev)), "ptx_dec_attention_stats")
        return out, (q, k, v, mask, stats)
    _abi.check(_abi.lib().ptx_dec_attention(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, _ptr(mask), B, Kq, L, H, C // H,
                                            out.data_ptr(), _stream(dev)), "ptx_dec_attention")
    return out, None


class _AttentionFn(torch.autograd.Function):
    """``attention`` as one node: saves the operands as the launch took them, the result and ``(m, l)`` per query; the backward
    recomputes the probabilities (``ptx_dec_attention_bwd``: two launches, every gradient element written once)."""

    @staticmethod
    def forward(ctx, q, k, v, mask, H):
        out, saved = _attention(q, k, v, mask, H, True)
        ctx.H, ctx.shapes, ctx.dtypes = H, (tuple(q.shape), tuple(k.shape)), (q.dtype, k.dtype, v.dtype)
        ctx.launched = saved is not None
        if ctx.launched:
            ctx.has_mask = saved[3] is not None
            ctx.save_for_backward(*(t for t in saved if t is not None), out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (B, Kq, C), (_, L, _) = ctx.shapes
        dev, H = dout.device, ctx.H
        if not ctx.launched:                                 # no query or no key: nothing flowed
            zeros = lambda n, dt: torch.zeros((B, n, C), dtype=dt, device=dev)      # noqa: E731
            return zeros(Kq, ctx.dtypes[0]), zeros(L, ctx.dtypes[1]), zeros(L, ctx.dtypes[2]), None, None
        saved = list(ctx.saved_tensors)
        out = saved.pop()
        q, k, v = saved[:3]
        mask, stats = (saved[3] if ctx.has_mask else None), saved[-1]
        dout = _f32(dout, "attention", dev)
        dq = torch.empty((B, Kq, C), dtype=torch.float32, device=dev)
        dk, dv = torch.empty((B, L, C), dtype=torch.float32, device=dev), torch.empty((B, L, C), dtype=torch.float32, device=dev)
        rowdot = torch.empty((B, H, Kq), dtype=torch.float32, device=dev)
        _abi.check(_abi.lib().ptx_dec_attention_bwd(q.data_ptr(), int(q.stride(1)), k.data_ptr(), int(k.stride(1)), v.data_ptr(),
                                                    int(v.stride(1)), _ptr(mask), B, Kq, L, H, C // H, out.data_ptr(), stats.data_ptr(),
                                                    dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), rowdot.data_ptr(),
                                                    _stream(dev)), "ptx_dec_attention_bwd")
        need = ctx.needs_input_grad
        return tuple(g.to(dt) if n else None for g, dt, n in zip((dq, dk, dv), ctx.dtypes, need[:3])) + (None, None)


def _ln_pair(ln) -> Tuple[torch.Tensor, torch.Tensor, float]:
    if isinstance(ln, nn.LayerNorm):
        return ln.weight, ln.bias, float(ln.eps)
    return ln[0], ln[1], float(ln[2]) if len(ln) > 2 else LN_EPS


def layer_norm(x: torch.Tensor, ln, ln2=None, out2: Optional[torch.Tensor] = None, differentiable: bool = False):
    """``LayerNorm(x)`` over the last axis of ``x (...,C)``; with ``ln2`` also ``LayerNorm2`` of that result: ``(out, out2)``.  ``ln``:
    an ``nn.LayerNorm`` or ``(weight, bias[, eps])``.  The row mean first, then the centred sum of squares
    (``decoder_host.layer_norm_host``; ``ptx_dec_ln``, one launch).  ``out2``: a contiguous fp32 tensor of x's shape that receives the
    second result (a layer's slot of ``hidden_states``).  ``differentiable=True``: one autograd node with gradients to ``x`` and both
    norms' weight and bias, the same forward bits; either result may go unused (``decoder_grad_host.layer_norm_bwd_host``;
    ``ptx_dec_ln_bwd``); ``out2`` is refused there."""
    if differentiable:
        if out2 is not None:
            raise ValueError("layer_norm: out2 cannot be given with differentiable=True (an in-place slot cannot be a graph output)")
        w, b, eps = _ln_pair(ln)
        w2, b2, eps2 = _ln_pair(ln2) if ln2 is not None else (None, None, eps)
        if _wants_grad(x, w, b, w2, b2):
            if eps2 != eps:
                raise ValueError(f"layer_norm: both norms must share eps, got {eps} and {eps2}")
            res = _LayerNormFn.apply(x, w, b, w2, b2, eps)
            return res[0] if ln2 is None else res
    _gpu("layer_norm", x)
    dev = x.device
    x = _f32(x, "layer_norm", dev)
    C = _width("layer_norm", x.shape[-1])
    w, b, eps = _ln_pair(ln)
    w, b = _f32(w, "layer_norm", dev), _f32(b, "layer_norm", dev)
    w2 = b2 = None
    if ln2 is None:
        out2 = None
    else:
        w2, b2, eps2 = _ln_pair(ln2)
        if eps2 != eps:
            raise ValueError(f"layer_norm: both norms must share eps, got {eps} and {eps2}")
        w2, b2 = _f32(w2, "layer_norm", dev), _f32(b2, "layer_norm", dev)
        if out2 is None:
            out2 = torch.empty_like(x)
        elif out2.dtype != torch.float32 or not out2.is_contiguous() or tuple(out2.shape) != tuple(x.shape) or out2.device != dev:
            raise ValueError(f"layer_norm: out2 must be contiguous fp32 {tuple(x.shape)} on {dev}")
    if any(t is not None and t.numel() != C for t in (w, b, w2, b2)):
        raise ValueError(f"layer_norm: weight and bias ({C}) expected")
    out = torch.empty_like(x)
    n = x.numel() // C
    if n:
        _abi.check(_abi.lib().ptx_dec_ln(x.data_ptr(), n, C, w.data_ptr(), b.data_ptr(), eps, out.data_ptr(), _ptr(w2), _ptr(b2), _ptr(out2),
                                         _stream(dev)), "ptx_dec_ln")
    return out if ln2 is None else (out, out2)


class _LayerNormFn(torch.autograd.Function):
    """``layer_norm`` as one node with one or two results.  Saved: ``x`` and the parameters; the statistics (and, with the second norm,
    the first result) are recomputed by ``ptx_dec_ln_bwd``, which writes ``dx = LN1^T(dy + LN2^T(dy2))`` and the per-row terms whose
    column sums in double (``ptx_op_colsum``) are the parameters' gradients.  A result nobody used arrives as None and is not read."""

    @staticmethod
    def forward(ctx, x, w, b, w2, b2, eps):
        two = w2 is not None
        res = layer_norm(x, (w, b, eps), (w2, b2, eps) if two else None)
        dev = x.device
        ctx.eps, ctx.two = eps, two
        ctx.meta = [(None, None) if t is None else (tuple(t.shape), t.dtype) for t in (x, w, b, w2, b2)]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*(_f32(t, "layer_norm", dev) for t in ((x, w, b, w2) if two else (x, w))))
        return res if two else (res,)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        saved = ctx.saved_tensors
        x, w = saved[0], saved[1]
        b, w2 = (saved[2], saved[3]) if ctx.two else (None, None)
        dev = x.device
        C = int(x.shape[-1])
        n = x.numel() // C
        dy = _f32(dys[0], "layer_norm", dev)
        dy2 = _f32(dys[1], "layer_norm", dev) if ctx.two else None
        grads = [None] * 5
        if dy is None and dy2 is None:
            return tuple(grads) + (None,)
        if n == 0:
            grads = [None if shape is None else torch.zeros(shape, dtype=dt, device=dev) for shape, dt in ctx.meta]
            return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad)) + (None,)
        dx, xdy = torch.empty_like(x), torch.empty_like(x)
        g1, xdy2 = (torch.empty_like(x), torch.empty_like(x)) if ctx.two else (None, None)
        _abi.check(_abi.lib().ptx_dec_ln_bwd(x.data_ptr(), n, C, w.data_ptr(), _ptr(b), ctx.eps, _ptr(w2), _ptr(dy), _ptr(dy2), dx.data_ptr(),
                                             xdy.data_ptr(), _ptr(g1), _ptr(xdy2), _stream(dev)), "ptx_dec_ln_bwd")
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            grads[0] = dx
            if need[1]:
                grads[1] = _train_ops.colsum(xdy.view(n, C))
            if need[2]:
                grads[2] = _train_ops.colsum((g1 if ctx.two else dy).view(n, C))
            if ctx.two and need[3]:
                grads[3] = _train_ops.colsum(xdy2.view(n, C))
            if ctx.two and need[4]:
                grads[4] = _train_ops.colsum(dy2.view(n, C)) if dy2 is not None else torch.zeros((C,), dtype=torch.float32, device=dev)
        out = []
        for g, (shape, dt), wanted in zip(grads, ctx.meta, need):
            out.append(g.reshape(shape).to(dt) if (g is not None and wanted) else None)
        return tuple(out) + (None,)


def linear_add_ln(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], residual: torch.Tensor, ln, ln2=None,
                  out2: Optional[torch.Tensor] = None, differentiable: bool = False):
    """``LayerNorm(x @ weight.T + bias + residual)``: an attention's out-projection or the FFN's second layer, the identity and the
    norm behind it; with ``ln2`` also the decoder's ``norm`` of that result, ``(out, out2)``.  Two launches: the residual is added in the
    GEMM's epilogue, the norm needs whole rows (``decoder_host.linear_add_ln_host``).  ``differentiable=True``: the composition of
    ``linear`` and ``layer_norm`` under autograd, two nodes; ``out2`` is refused there."""
    if differentiable and out2 is not None:
        raise ValueError("linear_add_ln: out2 cannot be given with differentiable=True (an in-place slot cannot be a graph output)")
    return layer_norm(linear(x, weight, bias, residual=residual, differentiable=differentiable), ln, ln2, out2, differentiable)


def boxes(h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], coords: torch.Tensor,
          out: Optional[torch.Tensor] = None, differentiable: bool = False) -> torch.Tensor:
    """``(B,K,9)``: the last Linear ``weight (9,C)`` of a regression branch on ``h (B,K,C)`` and the baseline decode against
    ``coords (B,K,3)`` -- ``center = p[0:3] + coords``, ``size = max(expf(p[3:6]), 0.02)`` with a NaN kept, ``euler = p[6:9]``
    (``query_select_host.boxes_host``; ``ptx_dec_boxes``, one launch).  ``differentiable=True``: one autograd node with gradients to
    ``h``, ``weight`` and ``bias`` (none to ``coords``), the same forward bits (``decoder_grad_host.boxes_bwd_host``;
    ``ptx_dec_boxes_bwd``); ``out`` is refused there."""
    if differentiable:
        if out is not None:
            raise ValueError("boxes: out cannot be given with differentiable=True (an in-place slot cannot be a graph output)")
        if _wants_grad(h, weight, bias):
            return _BoxesFn.apply(h, weight, bias, coords)
    _gpu("boxes", h, weight, bias, coords)
    dev = h.device
    h, weight, bias, coords = _f32(h, "boxes", dev), _f32(weight, "boxes", dev), _f32(bias, "boxes", dev), _f32(coords, "boxes", dev)
    C = _width("boxes", h.shape[-1])
    if tuple(weight.shape) != (9, C) or (bias is not None and bias.numel() != 9) or tuple(coords.shape) != tuple(h.shape[:-1]) + (3,):
        raise ValueError(f"boxes: weight (9,{C}), bias (9) and coords {tuple(h.shape[:-1]) + (3,)} expected, got {tuple(weight.shape)}, "
                         f"{None if bias is None else tuple(bias.shape)}, {tuple(coords.shape)}")
    if out is None:
        out = torch.empty(tuple(h.shape[:-1]) + (9,), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != tuple(h.shape[:-1]) + (9,) or out.device != dev:
        raise ValueError(f"boxes: out must be contiguous fp32 {tuple(h.shape[:-1]) + (9,)} on {dev}")
    n = h.numel() // C
    if n:
        _abi.check(_abi.lib().ptx_dec_boxes(h.data_ptr(), weight.data_ptr(), _ptr(bias), C, coords.data_ptr(), n, out.data_ptr(),
                                            _stream(dev)), "ptx_dec_boxes")
    return out


class _BoxesFn(torch.autograd.Function):
    """``boxes`` as one node.  Saved: ``h``, ``weight``, ``bias``; the log-sizes are recomputed (a saved size of 0.02 does not say on which
    side of the clamp it was).  ``ptx_dec_boxes_bwd`` writes ``dp``, ``dh = dp W`` and ``dW = dp^T h`` (row slabs in double, ascending);
    ``dbias = colsum(dp)`` in double (``ptx_op_colsum``)."""

    @staticmethod
    def forward(ctx, h, weight, bias, coords):
        res = boxes(h, weight, bias, coords)
        dev = res.device
        ctx.meta = [(None, None) if t is None else (tuple(t.shape), t.dtype) for t in (h, weight, bias)]
        ctx.has_bias = bias is not None
        ctx.save_for_backward(*(_f32(t, "boxes", dev) for t in ((h, weight, bias) if ctx.has_bias else (h, weight))))
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, dboxes):
        saved = ctx.saved_tensors
        h, w = saved[0], saved[1]
        bias = saved[2] if ctx.has_bias else None
        dev = h.device
        C = int(h.shape[-1])
        n = h.numel() // C
        need = ctx.needs_input_grad[:3]
        if n == 0:
            grads = [None if shape is None else torch.zeros(shape, dtype=dt, device=dev) for shape, dt in ctx.meta]
            return tuple(g if wanted else None for g, wanted in zip(grads, need)) + (None,)
        d = _f32(dboxes, "boxes", dev)
        dh, dp = torch.empty_like(h), torch.empty((n, 9), dtype=torch.float32, device=dev)
        dw = torch.empty((9, C), dtype=torch.float32, device=dev)
        ws = _slab_workspace(n, C, 9, dev)
        _abi.check(_abi.lib().ptx_dec_boxes_bwd(h.data_ptr(), w.data_ptr(), _ptr(bias), C, n, d.data_ptr(), dh.data_ptr(), dp.data_ptr(),
                                                dw.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(dev)), "ptx_dec_boxes_bwd")
        grads = [dh, dw, None]
        if ctx.has_bias and need[2]:
            with torch.cuda.device(dev):
                grads[2] = _train_ops.colsum(dp)
        out = [g.reshape(shape).to(dt) if (g is not None and wanted) else None for g, (shape, dt), wanted in zip(grads, ctx.meta, need)]
        return tuple(out) + (None,)


def contrastive_scores(hidden_states: torch.Tensor, text_feats: torch.Tensor, text_token_mask: torch.Tensor,
                       bias: Optional[torch.Tensor] = None, scaled: bool = True, max_text_len: int = 256,
                       differentiable: bool = False) -> torch.Tensor:
    """``(NL,B,K,max_text_len) fp32``: ``ContrastiveEmbed`` in full on every layer's ``hidden_states (NL,B,K,C)`` --
    ``hidden . text[b,t] (/ sqrtf(C)) (+ bias)`` on the tokens with ``text_token_mask[b,t]``, ``-inf`` on masked tokens and on the columns
    from ``T`` on (``decoder_host.contrastive_scores_host``; ``ptx_dec_scores``, one launch).  ``differentiable=True``: one autograd node
    with gradients to ``hidden_states``, ``text_feats`` and the scalar ``bias``, the same forward bits; the incoming gradient under a
    masked token or from column ``T`` on is never read (``decoder_grad_host.scores_bwd_host``; ``ptx_dec_scores_bwd``)."""
    if differentiable and _wants_grad(hidden_states, text_feats, bias):
        return _ScoresFn.apply(hidden_states, text_feats, text_token_mask, bias, bool(scaled), int(max_text_len))
    _gpu("contrastive_scores", hidden_states, text_feats, text_token_mask, bias)
    dev = hidden_states.device
    hs, text, bias = _f32(hidden_states, "contrastive_scores", dev), _f32(text_feats, "contrastive_scores", dev), \
        _f32(bias, "contrastive_scores", dev)
    if hs.dim() != 4 or text.dim() != 3 or text.shape[0] != hs.shape[1] or text.shape[2] != hs.shape[3]:
        raise ValueError(f"contrastive_scores: hidden_states (NL,B,K,C) and text_feats (B,T,C) expected, got {tuple(hs.shape)}, "
                         f"{tuple(text.shape)}")
    NL, B, K, C = (int(s) for s in hs.shape)
    _width("contrastive_scores", C)
    T, M = int(text.shape[1]), int(max_text_len)
    if not 1 <= T <= M <= MAX_TEXT or not 1 <= B <= MAX_SCENES or not 0 <= K <= MAX_QUERIES or NL > 64:
        raise ValueError(f"contrastive_scores: 1 <= T <= max_text_len <= {MAX_TEXT}, 1 to {MAX_SCENES} scenes, up to {MAX_QUERIES} queries and "
                         f"64 layers, got T={T}, max_text_len={M}, B={B}, K={K}, NL={NL}")
    mask = _mask_bytes("contrastive_scores", "the mask", text_token_mask, (B, T))
    out = torch.empty((NL, B, K, M), dtype=torch.float32, device=dev)
    if NL * K:
        _abi.check(_abi.lib().ptx_dec_scores(hs.data_ptr(), NL, B, K, C, text.data_ptr(), mask.data_ptr(), T, M, int(bool(scaled)), _ptr(bias),
                                             out.data_ptr(), _stream(dev)), "ptx_dec_scores")
    return out


class _ScoresFn(torch.autograd.Function):
    """``contrastive_scores`` as one node.  Saved: ``hidden_states``, ``text_feats`` and the mask.  ``ptx_dec_scores_bwd``: two launches on
    the exact-fp32 matrix instruction (``dhidden`` over the tokens, ``dtext`` over ``layer * K + query`` ascending) and, with a bias, its
    sum per (layer, scene) in double, then ascending."""

    @staticmethod
    def forward(ctx, hidden_states, text_feats, text_token_mask, bias, scaled, max_text_len):
        out = contrastive_scores(hidden_states, text_feats, text_token_mask, bias, scaled, max_text_len)
        dev = out.device
        ctx.scaled, ctx.M, ctx.has_bias = scaled, max_text_len, bias is not None
        ctx.meta = [(None, None) if t is None else (tuple(t.shape), t.dtype) for t in (hidden_states, text_feats, bias)]
        B, T = int(text_feats.shape[0]), int(text_feats.shape[1])
        ctx.save_for_backward(_f32(hidden_states, "contrastive_scores", dev), _f32(text_feats, "contrastive_scores", dev),
                              _mask_bytes("contrastive_scores", "the mask", text_token_mask, (B, T)))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dscores):
        hs, text, mask = ctx.saved_tensors
        dev = hs.device
        NL, B, K, C = (int(s) for s in hs.shape)
        T = int(text.shape[1])
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3])
        if NL * K == 0:
            grads = [None if shape is None else torch.zeros(shape, dtype=dt, device=dev) for shape, dt in ctx.meta]
            g = tuple(x if wanted else None for x, wanted in zip(grads, need))
            return g[0], g[1], None, g[2], None, None
        ds = _f32(dscores, "contrastive_scores", dev)
        dh, dt_ = torch.empty_like(hs), torch.empty_like(text)
        want_bias = ctx.has_bias and need[2]
        db = torch.empty((1,), dtype=torch.float32, device=dev) if want_bias else None
        ws = torch.empty((NL * B,), dtype=torch.float64, device=dev) if want_bias else None
        _abi.check(_abi.lib().ptx_dec_scores_bwd(ds.data_ptr(), hs.data_ptr(), NL, B, K, C, text.data_ptr(), mask.data_ptr(), T, ctx.M,
                                                 int(ctx.scaled), dh.data_ptr(), dt_.data_ptr(), _ptr(db), _ptr(ws),
                                                 0 if ws is None else ws.numel() * 8, _stream(dev)), "ptx_dec_scores_bwd")
        out = [g.reshape(shape).to(dt) if (g is not None and wanted) else None
               for g, (shape, dt), wanted in zip((dh, dt_, db), ctx.meta, need)]
        return out[0], out[1], None, out[2], None, None


# ------------------------------------------------------------------------------------------------------------------ the module
class _PositionEmbeddingLearned(nn.Module):
    def __init__(self, input_channel: int, embed_dims: int):
        super().__init__()
        self.position_embedding_head = nn.Sequential(nn.Conv1d(input_channel, embed_dims, kernel_size=1), nn.BatchNorm1d(embed_dims),
                                                     nn.ReLU(inplace=True), nn.Conv1d(embed_dims, embed_dims, kernel_size=1))


class _Attention(nn.Module):
    """The place of mmcv's ``MultiheadAttention``: its parameters live below ``attn`` (an ``nn.MultiheadAttention``, never called)."""

    def __init__(self, embed_dims: int = 256, num_heads: int = 8, attn_drop: float = 0.0, proj_drop: float = 0.0, dropout=None,
                 dropout_layer=None, init_cfg=None, batch_first: bool = True, **kwargs):
        super().__init__()
        self.embed_dims, self.num_heads = _width("GroundingDecoder", embed_dims), int(num_heads)
        if self.num_heads < 1 or self.embed_dims % self.num_heads or self.embed_dims // self.num_heads not in (32, 64):
            raise ValueError(f"GroundingDecoder: the head dimension must be 32 or 64, got embed_dims={embed_dims} with {num_heads} heads")
        if not batch_first:
            raise ValueError("GroundingDecoder: batch_first must be True")
        self.attn = nn.MultiheadAttention(self.embed_dims, self.num_heads, 0.0, **kwargs)


class _FFN(nn.Module):
    def __init__(self, embed_dims: int = 256, feedforward_channels: int = 1024, num_fcs: int = 2, act_cfg=None, ffn_drop: float = 0.0,
                 dropout_layer=None, add_identity: bool = True, init_cfg=None, layer_scale_init_value: float = 0.0, **kwargs):
        super().__init__()
        act = "ReLU" if act_cfg is None else act_cfg.get("type", "ReLU")
        if int(num_fcs) != 2 or act != "ReLU" or not add_identity or layer_scale_init_value:
            raise NotImplementedError(f"GroundingDecoder: the FFN with num_fcs=2, ReLU and the identity is implemented, got num_fcs={num_fcs}, "
                                      f"act {act!r}, add_identity={add_identity}, layer_scale_init_value={layer_scale_init_value}")
        F = int(feedforward_channels)
        if F % 64 or not 64 <= F <= MAX_FFN:
            raise ValueError(f"GroundingDecoder: feedforward_channels must be a multiple of 64 up to {MAX_FFN}, got {F}")
        self.embed_dims, self.feedforward_channels = _width("GroundingDecoder", embed_dims), F
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(self.embed_dims, F), nn.ReLU(inplace=True), nn.Dropout(ffn_drop)),
                                    nn.Linear(F, self.embed_dims), nn.Dropout(ffn_drop))


class _Layer(nn.Module):
    def __init__(self, self_attn_cfg=None, cross_attn_cfg=None, cross_attn_text_cfg=None, ffn_cfg=None, norm_cfg=None, init_cfg=None):
        super().__init__()
        if norm_cfg is not None and norm_cfg.get("type", "LN") != "LN":
            raise NotImplementedError(f"GroundingDecoder: norm_cfg type 'LN' is implemented, got {norm_cfg!r}")
        self.self_attn = _Attention(**(self_attn_cfg or {}))
        self.cross_attn_text = _Attention(**(cross_attn_text_cfg or {}))
        self.cross_attn = _Attention(**(cross_attn_cfg or {}))
        self.embed_dims = self.self_attn.embed_dims
        self.ffn = _FFN(**(ffn_cfg or {}))
        widths = {self.cross_attn_text.embed_dims, self.cross_attn.embed_dims, self.ffn.embed_dims}
        if widths != {self.embed_dims}:
            raise ValueError(f"GroundingDecoder: every part of a layer must share embed_dims={self.embed_dims}, got {sorted(widths)}")
        self.norms = nn.ModuleList([nn.LayerNorm(self.embed_dims) for _ in range(4)])
        self.self_posembed = _PositionEmbeddingLearned(3, self.embed_dims)          # constructed by the reference, never called


class GroundingDecoder(PreparedOperands, nn.Module):
    """``SparseFeatureFusionTransformerDecoder(num_layers, layer_cfg, post_norm_cfg=None, return_intermediate=True, init_cfg=None,
    with_cp=None)``, eval forward.  ``layer_cfg`` holds ``self_attn_cfg``, ``cross_attn_text_cfg``, ``cross_attn_cfg`` (``embed_dims``,
    ``num_heads``; dropout rates are accepted: dropout is the identity in eval) and ``ffn_cfg`` (``embed_dims``, ``feedforward_channels``,
    ``num_fcs=2``, ReLU), the reference's defaults where a key is missing.  The ``state_dict`` carries the reference's names, so a
    checkpoint's ``decoder.*`` loads with ``strict=True``; the per-layer ``layers.{i}.self_posembed`` loads and is never read, as in the
    reference.  ``with_cp`` is accepted and ignored.

    ``forward(query, key, value, key_padding_mask, self_attn_mask, cross_attn_mask, query_coords, key_coords, pred_bboxes, text_feats,
    text_attention_mask, bbox_head, **kwargs)`` takes what ``forward_decoder`` passes -- ``**QuerySelect(...)[0]`` after the detector's
    renaming (``feats -> key`` and ``value``, ``feats_attention_mask -> key_padding_mask``, ``feats_coords -> key_coords``) -- and returns
    ``(hidden_states (NL,B,K,C), all_layers_pred_bboxes (NL,B,K,9))``, or the last layer's ``(query, boxes)`` when
    ``return_intermediate=False``.  ``bbox_head``: an object with an indexable ``reg_branches``, a sequence of ``num_layers`` regression
    branches, or a ``QuerySelect``, whose ``reg_branch`` then serves every layer (``share_pred_layer=True``).

    Accepted: ``embed_dims`` a multiple of 64 from 64 to 512, head dimension 32 or 64, ``feedforward_channels`` a multiple of 64 up to
    2048, ``1 <= B <= 64``, ``0 <= K <= 1024``, ``1 <= T <= 256``; ``K = 0`` or ``Lmax = 0`` returns correctly shaped empties and launches
    nothing.  Refused: ``post_norm_cfg`` (ValueError, as in the reference), attention masks and ``value is not key``
    (NotImplementedError), training mode or an input that requires grad with grad mode on (NotImplementedError; both are accepted with
    ``differentiable=True``, below), ``bbox_head=None`` (ValueError; the reference fails on an undefined name there).

    ``differentiable=True`` (stored as ``self.differentiable``): in ``.train()`` the forward is the training path (``_run_train``) --
    batch statistics in both position embeddings, ``cross_posembed`` once with ``repeat=num_layers``, the boxes detached between layers,
    no gradient to ``key_coords``, ``query_coords`` or ``pred_bboxes``; the hidden Linears of a regression branch run through
    ``linear(relu=True)``, whose summation order differs from the eval path's ``query_select.linear``, so this path is held to float64
    and not to the eval bits.  In ``.eval()`` it is the eval forward, and raises when an input requires grad (frozen BatchNorms).

    The operands the launches take (concatenated projections, folded position embeddings) are prepared once and rebuilt when a parameter
    or buffer is replaced or its ``_version`` changes (``load_state_dict``, in-place updates): ``_doors.PreparedOperands``."""

    def __init__(self, num_layers: int, layer_cfg: dict, post_norm_cfg=None, return_intermediate: bool = True, init_cfg=None, with_cp=None,
                 differentiable: bool = False):
        super().__init__()
        self.differentiable = bool(differentiable)
        self.layer_cfg, self.num_layers = layer_cfg, int(num_layers)
        self.post_norm_cfg, self.return_intermediate, self.with_cp = post_norm_cfg, bool(return_intermediate), with_cp
        if not 1 <= self.num_layers <= 64:
            raise ValueError(f"GroundingDecoder: num_layers must be 1 to 64, got {num_layers}")
        self.layers = nn.ModuleList([_Layer(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in dict(layer_cfg or {}).items()})
                                     for _ in range(self.num_layers)])
        self.embed_dims = self.layers[0].embed_dims
        if post_norm_cfg is not None:
            raise ValueError(f"There is not post_norm in {type(self).__name__}")
        self.self_posembed = _PositionEmbeddingLearned(9, self.embed_dims)
        self.cross_posembed = _PositionEmbeddingLearned(3, self.embed_dims)
        self.norm = nn.LayerNorm(self.embed_dims)

    # -- the operands the launches take (PreparedOperands._prepare caches them)
    def _build_operands(self, dev) -> dict:
        C, NL = self.embed_dims, self.num_layers
        group = max(1, MAX_COUT // (2 * C))                  # layers per hoisted key/value projection
        f = lambda t: t.detach().to(dev, torch.float32)       # noqa: E731
        prep = dict(self_pos=_fold(self.self_posembed, dev), cross_pos=_fold(self.cross_posembed, dev), groups=[], layers=[])
        for lo in range(0, NL, group):
            ids = list(range(lo, min(lo + group, NL)))
            entry = dict(ids=ids)
            for name in ("cross_attn", "cross_attn_text"):
                ws = [f(getattr(self.layers[i], name).attn.in_proj_weight) for i in ids]
                bs = [f(getattr(self.layers[i], name).attn.in_proj_bias) for i in ids]
                entry[name] = (torch.cat([w[C:2 * C] for w in ws] + [w[2 * C:] for w in ws]).contiguous(),
                               torch.cat([b[C:2 * C] for b in bs] + [b[2 * C:] for b in bs]).contiguous())
            prep["groups"].append(entry)
        for layer in self.layers:
            d = {}
            for name in ("self_attn", "cross_attn_text", "cross_attn"):
                a = getattr(layer, name).attn
                w, b = f(a.in_proj_weight).contiguous(), f(a.in_proj_bias).contiguous()
                d[name] = dict(w=w, b=b, wq=w[:C], bq=b[:C], wkv=w[C:], bkv=b[C:], wo=f(a.out_proj.weight).contiguous(),
                               bo=f(a.out_proj.bias).contiguous(), H=getattr(layer, name).num_heads)
            prep["layers"].append(d)
        return prep

    @staticmethod
    def _branches(bbox_head, num_layers: int) -> List[List[nn.Linear]]:
        if bbox_head is None:
            raise ValueError("GroundingDecoder: bbox_head is None; the decoder refines its boxes with the head's regression branches")
        if isinstance(bbox_head, QuerySelect):
            branches = [bbox_head.reg_branch] * num_layers
        elif hasattr(bbox_head, "reg_branches"):
            branches = [bbox_head.reg_branches[i] for i in range(num_layers)]
        else:
            branches = list(bbox_head)
            if len(branches) < num_layers:
                raise ValueError(f"GroundingDecoder: {num_layers} regression branches expected, got {len(branches)}")
        out = []
        for br in branches[:num_layers]:
            lins = [m for m in (br if isinstance(br, (nn.Sequential, list, tuple)) else [br]) if isinstance(m, nn.Linear)]
            if not lins or lins[-1].out_features != 9:
                raise NotImplementedError("GroundingDecoder: a regression branch of Linear (+ ReLU) layers ending in 9 values expected "
                                          "(num_reg=12 is not implemented)")
            out.append(lins)
        return out

    def _check(self, query, key, value, key_padding_mask, self_attn_mask, cross_attn_mask, query_coords, key_coords, pred_bboxes, text_feats,
               text_attention_mask):
        if self_attn_mask is not None or cross_attn_mask is not None:
            raise NotImplementedError("GroundingDecoder: self_attn_mask and cross_attn_mask are not implemented; pass None")
        if value is not key:
            raise NotImplementedError("GroundingDecoder: value must be key (the detector passes the same tensor)")
        tensors = [query, key, key_padding_mask, query_coords, key_coords, pred_bboxes, text_feats, text_attention_mask]
        if not all(isinstance(t, torch.Tensor) for t in tensors):
            raise TypeError("GroundingDecoder: the operands must be tensors")
        wanted = torch.is_grad_enabled() and any(t.is_floating_point() and t.requires_grad for t in tensors)
        if not self.differentiable:
            if self.training:
                raise NotImplementedError("GroundingDecoder: the eval forward only; call .eval() (training through the decoder is not "
                                          "implemented)")
            if wanted:
                raise NotImplementedError("GroundingDecoder is inference-only: an input requires grad; call it under torch.no_grad() or detach")
        elif not self.training and wanted:
            raise NotImplementedError("GroundingDecoder(differentiable=True) in eval mode: an input requires grad, and training through the "
                                      "frozen BatchNorms of the position embeddings is not implemented; call .train(), or call it under "
                                      "torch.no_grad() / detach the inputs for the eval forward")
        C = self.embed_dims
        if query.dim() != 3 or query.shape[2] != C:
            raise ValueError(f"GroundingDecoder: query (B,K,{C}) expected, got {tuple(query.shape)}")
        B, K = int(query.shape[0]), int(query.shape[1])
        if key.dim() != 3 or key.shape[0] != B or key.shape[2] != C:
            raise ValueError(f"GroundingDecoder: key ({B},Lmax,{C}) expected, got {tuple(key.shape)}")
        L = int(key.shape[1])
        if text_feats.dim() != 3 or text_feats.shape[0] != B or text_feats.shape[2] != C:
            raise ValueError(f"GroundingDecoder: text_feats ({B},T,{C}) expected, got {tuple(text_feats.shape)}")
        T = int(text_feats.shape[1])
        if not 1 <= B <= MAX_SCENES or not 0 <= K <= MAX_QUERIES or not 1 <= T <= MAX_TEXT:
            raise ValueError(f"GroundingDecoder: 1 to {MAX_SCENES} scenes, 0 to {MAX_QUERIES} queries and 1 to {MAX_TEXT} text tokens, got B={B}, "
                             f"K={K}, T={T}")
        for name, t, shape in (("key_padding_mask", key_padding_mask, (B, L)), ("query_coords", query_coords, (B, K, 3)),
                               ("key_coords", key_coords, (B, L, 3)), ("pred_bboxes", pred_bboxes, (B, K, 9)),
                               ("text_attention_mask", text_attention_mask, (B, T))):
            if tuple(t.shape) != shape:
                raise ValueError(f"GroundingDecoder: {name} {shape} expected, got {tuple(t.shape)}")
        _gpu("GroundingDecoder", *tensors)
        return B, K, L, T

    def forward(self, query, key, value, key_padding_mask, self_attn_mask, cross_attn_mask, query_coords, key_coords, pred_bboxes, text_feats,
                text_attention_mask, bbox_head, **kwargs):
        branches = self._branches(bbox_head, self.num_layers)
        B, K, L, T = self._check(query, key, value, key_padding_mask, self_attn_mask, cross_attn_mask, query_coords, key_coords, pred_bboxes,
                                 text_feats, text_attention_mask)
        dev, C, NL = query.device, self.embed_dims, self.num_layers
        if K == 0 or L == 0:                                 # nothing to decode: the shapes, no launch
            if self.return_intermediate:
                return (torch.zeros((NL, B, K, C), dtype=torch.float32, device=dev), torch.zeros((NL, B, K, 9), dtype=torch.float32, device=dev))
            return torch.zeros((B, K, C), dtype=torch.float32, device=dev), torch.zeros((B, K, 9), dtype=torch.float32, device=dev)
        if self.differentiable and self.training:
            return self._run_train(branches, _f32_grad(query), _f32_grad(key), key_padding_mask, _f32(query_coords, "GroundingDecoder", dev),
                                   _f32(key_coords, "GroundingDecoder", dev), _f32(pred_bboxes, "GroundingDecoder", dev),
                                   _f32_grad(text_feats), text_attention_mask)
        with torch.no_grad():
            return self._run(branches, _f32(query, "GroundingDecoder", dev), _f32(key, "GroundingDecoder", dev), key_padding_mask,
                             _f32(query_coords, "GroundingDecoder", dev), _f32(key_coords, "GroundingDecoder", dev),
                             _f32(pred_bboxes, "GroundingDecoder", dev), _f32(text_feats, "GroundingDecoder", dev), text_attention_mask)

    def _run(self, branches, query, key, pad, qcoords, kcoords, bboxes, text, tmask):
        dev, C, NL = query.device, self.embed_dims, self.num_layers
        B, K, T = int(query.shape[0]), int(query.shape[1]), int(text.shape[1])
        prep = self._prepare(dev)
        pad = _mask_bytes("GroundingDecoder", "the mask", pad, tuple(key.shape[:2]))
        tmask = _mask_bytes("GroundingDecoder", "the mask", tmask, (B, T))
        text_keys_take_pos = T == K                          # mmcv: key_pos = query_pos when the shapes agree
        key_pos = posembed(kcoords, prep["cross_pos"])
        scene_kv, text_kv = {}, {}
        for g in prep["groups"]:                             # every layer's scene (and text) keys and values, ahead of the layer loop
            n = len(g["ids"])
            w, b = g["cross_attn"]
            kv = linear(key, w, b, add=key_pos, add_cols=n * C)
            for j, lid in enumerate(g["ids"]):
                scene_kv[lid] = (kv[:, :, j * C:(j + 1) * C], kv[:, :, (n + j) * C:(n + j + 1) * C])
            if not text_keys_take_pos:
                w, b = g["cross_attn_text"]
                kv = linear(text, w, b)
                for j, lid in enumerate(g["ids"]):
                    text_kv[lid] = (kv[:, :, j * C:(j + 1) * C], kv[:, :, (n + j) * C:(n + j + 1) * C])
        hidden = torch.empty((NL, B, K, C), dtype=torch.float32, device=dev) if self.return_intermediate else None
        all_boxes = torch.empty((NL, B, K, 9), dtype=torch.float32, device=dev) if self.return_intermediate else None
        for lid, (layer, p) in enumerate(zip(self.layers, prep["layers"])):
            query_pos = posembed(bboxes, prep["self_pos"])
            a = p["self_attn"]
            qkv = linear(query, a["w"], a["b"], add=query_pos, add_cols=2 * C)
            o = attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], None, a["H"])
            query = linear_add_ln(o, a["wo"], a["bo"], query, layer.norms[0])
            a = p["cross_attn_text"]
            q = linear(query, a["wq"], a["bq"], add=query_pos)
            if text_keys_take_pos:
                kv = linear(text, a["wkv"], a["bkv"], add=query_pos, add_cols=C)
                tk, tv = kv[:, :, :C], kv[:, :, C:]
            else:
                tk, tv = text_kv[lid]
            query = linear_add_ln(attention(q, tk, tv, tmask, a["H"]), a["wo"], a["bo"], query, layer.norms[1])
            a = p["cross_attn"]
            q = linear(query, a["wq"], a["bq"], add=query_pos)
            query = linear_add_ln(attention(q, *scene_kv[lid], pad, a["H"]), a["wo"], a["bo"], query, layer.norms[2])
            fc1, fc2 = layer.ffn.layers[0][0], layer.ffn.layers[1]
            h = linear(query, fc1.weight, fc1.bias, relu=True)
            if self.return_intermediate:
                query, _ = linear_add_ln(h, fc2.weight, fc2.bias, query, layer.norms[3], self.norm, out2=hidden[lid])
            else:
                query = linear_add_ln(h, fc2.weight, fc2.bias, query, layer.norms[3])
            lins = branches[lid]
            h = query
            for lin in lins[:-1]:
                h = query_select.linear(h, lin.weight, lin.bias, None, relu=True)
            bboxes = boxes(h, lins[-1].weight, lins[-1].bias, qcoords, out=all_boxes[lid] if self.return_intermediate else None)
        if self.return_intermediate:
            return hidden, all_boxes
        return query, bboxes

    def _run_train(self, branches, query, key, pad, qcoords, kcoords, bboxes, text, tmask):
        """The training path: the chain of ``_run`` built only from the differentiable operators, with the live parameters as the
        autograd leaves (``_prepare``'s cache, keyed on versions that every optimiser step bumps, is not used).  The position embeddings
        take batch statistics; ``cross_posembed`` runs once with ``repeat=NL`` (the reference calls it per layer on the same rows).  The
        hoisted key/value projection stays one launch per group of layers on a ``torch.cat`` of the live weight slices (autograd's slice
        backward hands each layer its rows).  The hidden Linears of a regression branch are ``linear(relu=True)`` -- straight
        accumulation, where the eval path's ``query_select.linear`` adds per 64-wide block: this path is held to float64, not to the
        eval bits.  The boxes carry a gradient to the regression branch and ``query``; they are detached before they become the next
        layer's ``pred_bboxes``, as are the coordinates."""
        dev, C, NL = query.device, self.embed_dims, self.num_layers
        B, K, T = int(query.shape[0]), int(query.shape[1]), int(text.shape[1])
        pad = _mask_bytes("GroundingDecoder", "the mask", pad, tuple(key.shape[:2]))
        tmask = _mask_bytes("GroundingDecoder", "the mask", tmask, (B, T))
        text_keys_take_pos = T == K                          # mmcv: key_pos = query_pos when the shapes agree
        key_pos = posembed(kcoords, self.cross_posembed, differentiable=True, repeat=NL)
        group = max(1, MAX_COUT // (2 * C))
        scene_kv, text_kv = {}, {}
        for lo in range(0, NL, group):
            ids = list(range(lo, min(lo + group, NL)))
            n = len(ids)
            for name, store in (("cross_attn", scene_kv), ("cross_attn_text", text_kv)):
                if name == "cross_attn_text" and text_keys_take_pos:
                    continue
                ws = [getattr(self.layers[i], name).attn.in_proj_weight for i in ids]
                bs = [getattr(self.layers[i], name).attn.in_proj_bias for i in ids]
                w = torch.cat([w_[C:2 * C] for w_ in ws] + [w_[2 * C:] for w_ in ws])
                b = torch.cat([b_[C:2 * C] for b_ in bs] + [b_[2 * C:] for b_ in bs])
                if name == "cross_attn":
                    kv = linear(key, w, b, add=key_pos, add_cols=n * C, differentiable=True)
                else:
                    kv = linear(text, w, b, differentiable=True)
                for j, lid in enumerate(ids):
                    store[lid] = (kv[:, :, j * C:(j + 1) * C], kv[:, :, (n + j) * C:(n + j + 1) * C])
        hidden, all_boxes = [], []
        for lid, layer in enumerate(self.layers):
            query_pos = posembed(bboxes, self.self_posembed, differentiable=True)
            a, H = layer.self_attn.attn, layer.self_attn.num_heads
            qkv = linear(query, a.in_proj_weight, a.in_proj_bias, add=query_pos, add_cols=2 * C, differentiable=True)
            o = attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], None, H, differentiable=True)
            query = linear_add_ln(o, a.out_proj.weight, a.out_proj.bias, query, layer.norms[0], differentiable=True)
            a, H = layer.cross_attn_text.attn, layer.cross_attn_text.num_heads
            q = linear(query, a.in_proj_weight[:C], a.in_proj_bias[:C], add=query_pos, differentiable=True)
            if text_keys_take_pos:
                kv = linear(text, a.in_proj_weight[C:], a.in_proj_bias[C:], add=query_pos, add_cols=C, differentiable=True)
                tk, tv = kv[:, :, :C], kv[:, :, C:]
            else:
                tk, tv = text_kv[lid]
            query = linear_add_ln(attention(q, tk, tv, tmask, H, differentiable=True), a.out_proj.weight, a.out_proj.bias, query,
                                  layer.norms[1], differentiable=True)
            a, H = layer.cross_attn.attn, layer.cross_attn.num_heads
            q = linear(query, a.in_proj_weight[:C], a.in_proj_bias[:C], add=query_pos, differentiable=True)
            query = linear_add_ln(attention(q, *scene_kv[lid], pad, H, differentiable=True), a.out_proj.weight, a.out_proj.bias, query,
                                  layer.norms[2], differentiable=True)
            fc1, fc2 = layer.ffn.layers[0][0], layer.ffn.layers[1]
            h = linear(query, fc1.weight, fc1.bias, relu=True, differentiable=True)
            if self.return_intermediate:
                query, hid = linear_add_ln(h, fc2.weight, fc2.bias, query, layer.norms[3], self.norm, differentiable=True)
                hidden.append(hid)
            else:
                query = linear_add_ln(h, fc2.weight, fc2.bias, query, layer.norms[3], differentiable=True)
            lins = branches[lid]
            h = query
            for lin in lins[:-1]:
                h = linear(h, lin.weight, lin.bias, relu=True, differentiable=True)
            new_boxes = boxes(h, lins[-1].weight, lins[-1].bias, qcoords, differentiable=True)
            all_boxes.append(new_boxes)
            bboxes = new_boxes.detach()
        if self.return_intermediate:
            return torch.stack(hidden), torch.stack(all_boxes)
        return query, new_boxes

    def head_scores(self, hidden_states: torch.Tensor, head_inputs_dict: dict, query_select: QuerySelect,
                    differentiable: bool = False) -> torch.Tensor:
        """``GroundingHead.forward``'s ``all_layers_cls_scores (NL,B,K,max_text_len)`` with the ``QuerySelect``'s ``cls_branch``;
        ``differentiable=True``: ``contrastive_scores`` under autograd."""
        qs = query_select
        return contrastive_scores(hidden_states, head_inputs_dict["text_feats"], head_inputs_dict["text_token_mask"],
                                  qs.cls_branch.bias if qs.has_bias else None, qs.scaled, qs.max_text_len, differentiable=differentiable)

    def forward_host(self, query, key, key_padding_mask, query_coords, key_coords, pred_bboxes, text_feats, text_attention_mask, bbox_head,
                     dtype=np.float64, **kw):
        """The same chain from ``decoder_host.py`` in numpy ``dtype`` with this module's parameters."""
        dt = np.dtype(dtype)
        arr = lambda t, d=dt: _np(t, d)      # noqa: E731
        branches = self._branches(bbox_head, self.num_layers)
        layer = self.layers[0]
        return decoder_host.forward_host(
            {k: arr(v, np.float64) for k, v in self.state_dict().items()}, self.num_layers,
            (layer.self_attn.num_heads, layer.cross_attn_text.num_heads, layer.cross_attn.num_heads), arr(query), arr(key),
            arr(key_padding_mask, bool), arr(query_coords), arr(key_coords), arr(pred_bboxes), arr(text_feats), arr(text_attention_mask, bool),
            [[arr(m.weight) for m in lins] for lins in branches], [[arr(m.bias) for m in lins] for lins in branches], dtype=dt,
            return_intermediate=self.return_intermediate, **kw)
