"""The image backbone in numpy: the specification of csrc/conv2d.hip and of ``image_backbone.ResNet.forward``.

``mmdet.ResNet`` with Bottleneck blocks, ``style='pytorch'`` (the stride sits on the 3x3 convolution) and every BatchNorm frozen: the stem
(7x7 stride 2 pad 3 convolution, BatchNorm, ReLU, 3x3 stride 2 pad 1 max-pool), then per block 1x1 -> 3x3 -> 1x1 with the identity (or
its 1x1 strided ``downsample``) added before the last ReLU.  Each BatchNorm is the affine map ``* scale + shift`` of ``bn_fold_host`` --
the formula of ``sparse.bn_fold`` in the chain's dtype -- applied in the device's epilogue order: ``* scale``, ``+ shift``,
``+ residual``, ReLU.  A float32 run is therefore the device's arithmetic up to the order of the sums.

NaN rule, as torch: the ReLU and the max-pool keep a NaN; a NaN pixel reaches exactly the outputs whose receptive field holds it (a zero
weight does not hide it); the padding is zero for the convolutions and ignored by the pool."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

__all__ = ["ARCH", "EPS", "bn_fold_host", "bottleneck_host", "conv2d_host", "epilogue_host", "max_pool_host", "normalise_host",
           "resnet_host"]

#: blocks per stage of the Bottleneck depths
ARCH = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
EPS = 1e-5
EXPANSION = 4


def conv2d_host(x: np.ndarray, w: np.ndarray, stride: int = 1, pad: int = 0) -> np.ndarray:
    """``F.conv2d(x, w, stride=stride, padding=pad)`` on ``x (N,Cin,H,W)``, ``w (Cout,Cin,k,k)`` in ``x``'s dtype: one matrix product per
    tap, taps added in ascending ``(ky, kx)``."""
    N, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    xp = np.zeros((N, Cin, H + 2 * pad, W + 2 * pad), x.dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    w = w.astype(x.dtype, copy=False)
    out = np.zeros((N, Cout, Ho * Wo), x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride].reshape(N, Cin, Ho * Wo)
            out += np.matmul(w[:, :, ky, kx], win)
    return out.reshape(N, Cout, Ho, Wo)


def max_pool_host(x: np.ndarray, kernel: int = 3, stride: int = 2, pad: int = 1) -> np.ndarray:
    """``F.max_pool2d(x, kernel, stride, pad)``: the padding never wins, a NaN in the window does."""
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - kernel) // stride + 1, (W + 2 * pad - kernel) // stride + 1
    xp = np.full((N, C, H + 2 * pad, W + 2 * pad), -np.inf, x.dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    out = np.full((N, C, Ho, Wo), -np.inf, x.dtype)
    for ky in range(kernel):
        for kx in range(kernel):
            out = np.maximum(out, xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride])
    return out


def bn_fold_host(weight, bias, mean, var, eps: float, dt) -> tuple:
    """``(scale, shift)`` of a frozen BatchNorm in dtype ``dt``: ``sparse.bn_fold``'s formula."""
    dt = np.dtype(dt)
    weight, bias, mean, var = (np.asarray(t).astype(dt) for t in (weight, bias, mean, var))
    scale = weight * (1 / np.sqrt(var + dt.type(eps))).astype(dt)
    return scale, bias - mean * scale


def epilogue_host(v: np.ndarray, scale=None, shift=None, residual=None, relu: bool = False) -> np.ndarray:
    """The epilogue of the three launches, in their order: ``* scale``, ``+ shift`` (per output channel), ``+ residual``, ReLU."""
    if scale is not None:
        v = v * scale.astype(v.dtype)[None, :, None, None]
    if shift is not None:
        v = v + shift.astype(v.dtype)[None, :, None, None]
    if residual is not None:
        v = v + residual
    if relu:
        v = np.maximum(v, v.dtype.type(0))                  # np.maximum keeps a NaN
    return v


def normalise_host(imgs: np.ndarray, mean=None, std=None) -> np.ndarray:
    """``(x - mean) / std`` per channel in float32: the expression the stem applies while it stages the pixels (uint8 or float32)."""
    x = np.asarray(imgs).astype(np.float32)
    if mean is None:
        return x
    m, s = (np.asarray(t, np.float32).reshape(1, -1, 1, 1) for t in (mean, std))
    return (x - m) / s


def _fold(params: Dict[str, np.ndarray], name: str, dt) -> tuple:
    return bn_fold_host(params[name + ".weight"], params[name + ".bias"], params[name + ".running_mean"], params[name + ".running_var"],
                        EPS, dt)


def bottleneck_host(params: Dict[str, np.ndarray], prefix: str, x: np.ndarray, stride: int) -> np.ndarray:
    """One Bottleneck, ``style='pytorch'``: ``conv1`` 1x1, ``conv2`` 3x3 with the stride, ``conv3`` 1x1, the identity through
    ``downsample`` (1x1 with the stride + BatchNorm) where the block has one."""
    dt = x.dtype
    w = lambda n: np.asarray(params[prefix + n]).astype(dt)      # noqa: E731
    identity = x
    if prefix + "downsample.0.weight" in params:
        identity = epilogue_host(conv2d_host(x, w("downsample.0.weight"), stride, 0), *_fold(params, prefix + "downsample.1", dt))
    out = epilogue_host(conv2d_host(x, w("conv1.weight"), 1, 0), *_fold(params, prefix + "bn1", dt), relu=True)
    out = epilogue_host(conv2d_host(out, w("conv2.weight"), stride, 1), *_fold(params, prefix + "bn2", dt), relu=True)
    return epilogue_host(conv2d_host(out, w("conv3.weight"), 1, 0), *_fold(params, prefix + "bn3", dt), residual=identity, relu=True)


def resnet_host(params: Dict[str, np.ndarray], imgs: np.ndarray, stage_blocks: Sequence[int], strides: Sequence[int] = (1, 2, 2, 2),
                out_indices: Sequence[int] = (0, 1, 2, 3), dtype=np.float64, mean=None, std=None,
                bgr_to_rgb: bool = False) -> List[np.ndarray]:
    """The levels ``out_indices`` of ``imgs (N,3,H,W)`` (float or uint8), in ``dtype``.  ``params``: the state dict as arrays.  ``mean`` /
    ``std``: the data preprocessor's, applied in float32 first; ``bgr_to_rgb``: the images' planes are reversed before that (the
    device reverses the input planes of the stem's weight, and ``mean`` / ``std``, instead: the same products, added in another order)."""
    dt = np.dtype(dtype)
    imgs = np.asarray(imgs)
    x = normalise_host(imgs[:, ::-1] if bgr_to_rgb else imgs, mean, std).astype(dt)
    w = np.asarray(params["conv1.weight"]).astype(dt)
    x = epilogue_host(conv2d_host(x, w, 2, 3), *_fold(params, "bn1", dt), relu=True)
    x = max_pool_host(x)
    outs: List[Optional[np.ndarray]] = []
    for s, nb in enumerate(stage_blocks):
        for b in range(nb):
            x = bottleneck_host(params, f"layer{s + 1}.{b}.", x, strides[s] if b == 0 else 1)
        if s in out_indices:
            outs.append(x)
    return outs
