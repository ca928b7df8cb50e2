"""The image backbone's backward in numpy: the specification of csrc/conv2d_bwd.hip and of ``image_backbone.ResNet(differentiable=True)``.

Every BatchNorm is frozen (``* scale + shift`` of ``bn_fold_host``): only convolution kernels receive a gradient, the kernels of the stages
``>= frozen_stages``, and nothing flows to the images.  ``conv_bwd_host`` is one ``ptx_conv1x1_bwd`` / ``ptx_conv3x3_bwd`` call, in the
library's summation orders -- which matter in float32 and are harmless in float64:

* ``gz = g * [out > 0] * scale``, ``dresidual = g * [out > 0]``;
* ``dx``: k = (ky, kx, co) ascending in blocks of 32 (below 64 input channels, except the strided 3x3 beyond 16) or 64, each block's
  product from zero, then added; ``dx_held``, where given, is added to the completed sum;
* ``dweight``: the flattened pixel index (n, oy, ox) in steps of 64 dealt evenly to ``dweight_chunks_host(...)`` chunks, a chunk's steps
  added in ascending order from zero, then the chunks in ascending order.

Inside a block of k, or a step of pixels, the matrix instruction's own order is not restated: ``np.matmul`` stands for it.

The ReLU masks can be supplied from outside (``masks``): a device-against-host comparison replays the device forward's masks, so that an
activation which rounds to the other side of zero in another precision is not counted as an error of the backward."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from .image_backbone_host import _fold, conv2d_host, epilogue_host, max_pool_host, normalise_host

__all__ = ["bottleneck_grad_host", "conv_bwd_host", "dweight_chunks_host", "resnet_grad_host", "trainable_kernels"]


def dweight_chunks_host(KS: int, N: int, Cin: int, Cout: int, H: int, W: int, stride: int) -> int:
    """``ptx_conv_dweight_chunks``: S, a function of the shapes only."""
    K = KS * KS * Cin
    pixels = N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    tiles = -(-Cout // 64) * -(-K // 64)
    T = -(-pixels // 64)
    return max(1, min(-(-1024 // tiles), (256 << 20) // (Cout * K * 4), -(-T // 4)))


def _dx_block(KS: int, Cin: int, stride: int) -> int:
    return 32 if Cin < 64 and not (KS == 3 and stride == 2 and Cin > 16) else 64


def _taps(k: int, pad: int, stride: int, H: int, Ho: int):
    """For kernel offset ``k`` along one axis: the outputs ``o`` whose input ``stride * o - pad + k`` lies inside ``[0, H)``, and those
    inputs, as two slices."""
    lo = max(0, -(-(pad - k) // stride))
    hi = min(Ho - 1, (H - 1 + pad - k) // stride)
    if hi < lo:
        return slice(0, 0), slice(0, 0)
    return slice(lo, hi + 1), slice(stride * lo - pad + k, stride * hi - pad + k + 1, stride)


def conv_bwd_host(g: np.ndarray, out: Optional[np.ndarray], scale: Optional[np.ndarray], relu: bool, x: np.ndarray, w: np.ndarray,
                  stride: int = 1, pad: int = 0, dx_held: Optional[np.ndarray] = None, want_dx: bool = True):
    """``(gz, dresidual, dx, dweight)`` of ``out = relu((conv2d(x, w, stride, pad) * scale + shift) + residual)`` for ``g = d loss / d out``,
    in ``g``'s dtype.  ``w (Cout,Cin,k,k)`` and ``dweight`` are in the parameter's layout; ``out`` is read only with ``relu`` (only its sign
    matters: a 0 / 1 mask does as well)."""
    dt = g.dtype
    N, Cin, H, W = x.shape
    Cout, _, KS, _ = w.shape
    Ho, Wo = g.shape[2], g.shape[3]
    d = np.where(out > 0, g, dt.type(0)) if relu else g
    gz = d * scale.astype(dt)[None, :, None, None] if scale is not None else d
    w = w.astype(dt, copy=False)
    x = x.astype(dt, copy=False)
    dx = None
    if want_dx:
        # gathered[n, tap, co, y, x] = gz at the output that tap took this pixel into
        gat = np.zeros((N, KS * KS, Cout, H, W), dt)
        for ky in range(KS):
            oy, iy = _taps(ky, pad, stride, H, Ho)
            for kx in range(KS):
                ox, ix = _taps(kx, pad, stride, W, Wo)
                gat[:, ky * KS + kx, :, iy, ix] = gz[:, :, oy, ox]
        gat = gat.reshape(N, KS * KS * Cout, H * W)
        wt = np.ascontiguousarray(w.transpose(1, 2, 3, 0)).reshape(Cin, KS * KS * Cout)       # (ci, ky, kx, co)
        blk = _dx_block(KS, Cin, stride)
        dx = np.zeros((N, Cin, H * W), dt)
        for k0 in range(0, wt.shape[1], blk):
            dx += np.matmul(wt[:, k0:k0 + blk], gat[:, k0:k0 + blk])
        dx = dx.reshape(N, Cin, H, W)
        if dx_held is not None:
            dx = dx + dx_held
    # dweight: columns of x per (tap, ci) over the flattened pixel index
    cols = np.zeros((KS * KS, Cin, N, Ho, Wo), dt)
    for ky in range(KS):
        oy, iy = _taps(ky, pad, stride, H, Ho)
        for kx in range(KS):
            ox, ix = _taps(kx, pad, stride, W, Wo)
            cols[ky * KS + kx, :, :, oy, ox] = x[:, :, iy, ix].transpose(1, 0, 2, 3)
    cols = cols.reshape(KS * KS * Cin, N * Ho * Wo)
    gzf = gz.transpose(1, 0, 2, 3).reshape(Cout, N * Ho * Wo)
    S = dweight_chunks_host(KS, N, Cin, Cout, H, W, stride)
    T = -(-(N * Ho * Wo) // 64)
    dw = None
    for c in range(S):
        part = np.zeros((Cout, KS * KS * Cin), dt)
        for s in range(c * T // S, (c + 1) * T // S):
            part += np.matmul(gzf[:, 64 * s:64 * s + 64], cols[:, 64 * s:64 * s + 64].T)
        dw = part if dw is None else dw + part
    dweight = np.ascontiguousarray(dw.reshape(Cout, KS, KS, Cin).transpose(0, 3, 1, 2))
    return gz, d, dx, dweight


def trainable_kernels(stage_blocks: Sequence[int], frozen_stages: int) -> List[str]:
    """The names of the kernels that train, in the order of the forward: ``layer{s}.{b}.conv1/conv2/conv3.weight`` and
    ``layer{s}.0.downsample.0.weight`` of the stages ``s > frozen_stages``."""
    names = []
    for s, nb in enumerate(stage_blocks):
        if s < frozen_stages:
            continue
        for b in range(nb):
            p = f"layer{s + 1}.{b}."
            names += [p + "conv1.weight", p + "conv2.weight", p + "conv3.weight"]
            if b == 0:
                names.append(p + "downsample.0.weight")
    return names


def _bottleneck_forward(params, prefix, x, stride):
    """``bottleneck_host`` with the intermediates kept."""
    dt = x.dtype
    w = lambda n: np.asarray(params[prefix + n]).astype(dt)      # noqa: E731
    idn = x
    if prefix + "downsample.0.weight" in params:
        idn = epilogue_host(conv2d_host(x, w("downsample.0.weight"), stride, 0), *_fold(params, prefix + "downsample.1", dt))
    t1 = epilogue_host(conv2d_host(x, w("conv1.weight"), 1, 0), *_fold(params, prefix + "bn1", dt), relu=True)
    t2 = epilogue_host(conv2d_host(t1, w("conv2.weight"), stride, 1), *_fold(params, prefix + "bn2", dt), relu=True)
    out = epilogue_host(conv2d_host(t2, w("conv3.weight"), 1, 0), *_fold(params, prefix + "bn3", dt), residual=idn, relu=True)
    return dict(x=x, t1=t1, t2=t2, out=out)


def bottleneck_grad_host(params: Dict[str, np.ndarray], prefix: str, kept: Dict[str, np.ndarray], stride: int, g: np.ndarray,
                         want_dx: bool = True, masks: Optional[Dict[str, np.ndarray]] = None, dx_held: Optional[np.ndarray] = None):
    """One Bottleneck backwards, in the order of the device's calls: ``conv3`` (its ``dresidual`` is the identity branch's gradient),
    ``conv2``, ``downsample`` where the block has one (it writes the block's input gradient), then ``conv1``, whose ``dx`` is added to
    what the identity branch left: ``dx = (identity or downsample) + conv1``.  ``dx_held`` (the gradient of a level that is this block's
    input, blocks with a ``downsample`` only) is what the downsample's ``dx`` is added to: ``dx = (dx_held + downsample) + conv1``.  ``kept``: the forward's ``x, t1, t2, out``; ``masks``: ``[. > 0]``
    of ``t1, t2, out`` under ``prefix + name`` to use in their place.  Returns ``(dx or None, {kernel name: gradient})``."""
    dt = g.dtype
    w = lambda n: np.asarray(params[prefix + n]).astype(dt)      # noqa: E731
    sign = lambda n: (masks[prefix + n] if masks is not None else kept[n] > 0).astype(dt)      # noqa: E731
    grads = {}
    _, dres, dt2, grads[prefix + "conv3.weight"] = conv_bwd_host(g, sign("out"), _fold(params, prefix + "bn3", dt)[0], True, kept["t2"],
                                                                 w("conv3.weight"), 1, 0)
    _, _, dt1, grads[prefix + "conv2.weight"] = conv_bwd_host(dt2, sign("t2"), _fold(params, prefix + "bn2", dt)[0], True, kept["t1"],
                                                              w("conv2.weight"), stride, 1)
    held = dres
    if dx_held is not None and prefix + "downsample.0.weight" not in params:
        raise NotImplementedError("bottleneck_grad_host: dx_held needs a block with a downsample")
    if prefix + "downsample.0.weight" in params:
        _, _, held, grads[prefix + "downsample.0.weight"] = conv_bwd_host(dres, None, _fold(params, prefix + "downsample.1", dt)[0], False,
                                                                          kept["x"], w("downsample.0.weight"), stride, 0, dx_held=dx_held,
                                                                          want_dx=want_dx)
    _, _, dx, grads[prefix + "conv1.weight"] = conv_bwd_host(dt1, sign("t1"), _fold(params, prefix + "bn1", dt)[0], True, kept["x"],
                                                             w("conv1.weight"), 1, 0, dx_held=held if want_dx else None, want_dx=want_dx)
    return dx, grads


def resnet_grad_host(params: Dict[str, np.ndarray], imgs: np.ndarray, grads_of_levels: Sequence[np.ndarray], stage_blocks: Sequence[int],
                     strides: Sequence[int] = (1, 2, 2, 2), out_indices: Sequence[int] = (0, 1, 2, 3), frozen_stages: int = 1,
                     dtype=np.float64, masks: Optional[Dict[str, np.ndarray]] = None, mean=None, std=None,
                     bgr_to_rgb: bool = False) -> Dict[str, np.ndarray]:
    """The gradient of every trainable kernel (``trainable_kernels``; parameter layout, ``dtype``) for the gradients ``grads_of_levels``
    of the ``out_indices`` levels ``(N,C_l,H_l,W_l)``.  The forward is ``resnet_host``'s in ``dtype``; frozen stages and BatchNorms get no
    entry.  A level that is an output and the next stage's input takes ``(level gradient + downsample's dx) + conv1's dx`` of the next
    stage's first block, in that order (``bottleneck_grad_host``'s ``dx_held``)."""
    if frozen_stages < 1:
        raise NotImplementedError("resnet_grad_host: frozen_stages < 1 (the stem's and the max-pool's backward) is out of scope")
    dt = np.dtype(dtype)
    imgs = np.asarray(imgs)
    x = normalise_host(imgs[:, ::-1] if bgr_to_rgb else imgs, mean, std).astype(dt)
    x = epilogue_host(conv2d_host(x, np.asarray(params["conv1.weight"]).astype(dt), 2, 3), *_fold(params, "bn1", dt), relu=True)
    x = max_pool_host(x)
    kept = {}
    for s, nb in enumerate(stage_blocks):
        for b in range(nb):
            p = f"layer{s + 1}.{b}."
            kept[p] = _bottleneck_forward(params, p, x, strides[s] if b == 0 else 1)
            x = kept[p]["out"]
    level_grad = {s: np.asarray(g).astype(dt) for s, g in zip(out_indices, grads_of_levels)}
    grads: Dict[str, np.ndarray] = {}
    g = None
    for s in range(len(stage_blocks) - 1, frozen_stages - 1, -1):
        if g is None:
            g = level_grad[s]                               # the last stage: stage_blocks ends at the last output
        for b in range(stage_blocks[s] - 1, -1, -1):
            p = f"layer{s + 1}.{b}."
            first = s == frozen_stages and b == 0           # its input comes from a frozen stage
            joined = level_grad.get(s - 1) if b == 0 and not first else None
            g, got = bottleneck_grad_host(params, p, kept[p], strides[s] if b == 0 else 1, g, want_dx=not first, masks=masks, dx_held=joined)
            grads.update(got)
    return grads
