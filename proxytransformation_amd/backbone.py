"""The sparse ``MinkResNet`` backbone (``x = self.backbone_3d(x)``, DET:398; backbones/mink_resnet.py:40-124 with MinkowskiEngine's
``BasicBlock``) assembled from the layers of ``sparse.py``: kernel maps, the gather-GEMM convolution, the max-pool and the norm kernels.

The constructor and the ``state_dict`` are the reference's -- ``conv1.kernel (27, Cin, 64)``, ``norm1.weight / .bias (1, 64)``,
``layerL.B.conv1.kernel``, ``layerL.B.norm1.bn.*``, ``layerL.0.downsample.0.kernel``, ``layerL.0.downsample.1.bn.*`` -- so a reference
checkpoint's ``backbone_3d.*`` loads by name with ``strict=True``.  There is no sparse tensor type: ``forward(coords, scene_rows,
feats)`` takes the rows ``quantize`` returns and gives one ``SparseLevel`` per stage.

* eval mode: every BatchNorm is folded into the ``scale`` / ``shift`` of its convolution (``sparse.bn_fold``, cached per BatchNorm),
  the residual and the ReLU ride in the second convolution's epilogue; the stem is conv -> instance norm + ReLU -> max-pool.  With
  ``differentiable=True`` this is frozen-BatchNorm fine-tuning;
* train mode (``differentiable=True``): bare convolutions, then ``sparse_batch_norm`` with the residual and the ReLU fused into it; the
  running statistics are updated as ``nn.BatchNorm1d`` updates them.  Without ``differentiable=True`` the layers raise their
  inference-only error.  Which path a BatchNorm takes is its own ``training`` flag.

``forward_host`` is the same chain from the numpy restatements: the reference of the tests.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch
from torch import nn

from . import sparse
from .registry import MODELS, REGISTRY_BACKEND
from .sparse import SparseBatchNorm, SparseConv3d, SparseInstanceNorm

__all__ = ["BasicBlock", "MinkResNet", "SparseLevel"]


@dataclass
class SparseLevel:
    """One output level: the rows of a ``ME.SparseTensor`` (torch tensors from ``forward``, numpy arrays from ``forward_host``)."""
    feats: object                 # (n_l, 64 * 2^l) fp32
    coords: object                # (n_l, 4) int32 (scene, x, y, z), multiples of tensor_stride
    scene_rows: List[int]         # end of each scene's rows
    tensor_stride: int


class BasicBlock(nn.Module):
    """``MinkowskiEngine.modules.resnet_block.BasicBlock``: conv3 -> norm -> ReLU -> conv3 -> norm, + (downsampled) input, ReLU; the
    convolutions carry no bias.  ``forward(x, m_first, m_same, m_side)``: the kernel maps of ``conv1`` (k3, this block's stride), of
    ``conv2`` (k3 s1 on the output rows) and of ``downsample`` (k1 s2; only read when the block has one)."""
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: nn.Module = None, bn_momentum: float = 0.1,
                 differentiable: bool = False):
        super().__init__()
        self.conv1 = SparseConv3d(inplanes, planes, kernel_size=3, stride=stride, differentiable=differentiable)
        self.norm1 = SparseBatchNorm(planes, momentum=bn_momentum, differentiable=differentiable)
        self.conv2 = SparseConv3d(planes, planes, kernel_size=3, stride=1, differentiable=differentiable)
        self.norm2 = SparseBatchNorm(planes, momentum=bn_momentum, differentiable=differentiable)
        self.downsample = downsample

    def forward(self, x: torch.Tensor, m_first, m_same, m_side=None) -> torch.Tensor:
        h = _conv_bn(self.conv1, self.norm1, x, m_first, None, True)
        side = x if self.downsample is None else _conv_bn(self.downsample[0], self.downsample[1], x, m_side, None, False)
        return _conv_bn(self.conv2, self.norm2, h, m_same, side, True)


def _conv_bn(conv: SparseConv3d, norm: SparseBatchNorm, x, kmap, residual, relu: bool):
    """conv -> BatchNorm (+ residual)(+ ReLU): one fused convolution launch for an eval BatchNorm, convolution + norm kernels for a
    training one."""
    if norm.bn.training:
        return norm(conv(x, kmap), residual=residual, relu=relu)
    scale, shift = sparse.bn_fold(norm.bn)
    return conv(x, kmap, scale=scale, shift=shift, residual=residual, relu=relu)


def _conv_bn_host(conv, norm, x, nbr, residual, relu, dt):
    kernel = conv.kernel.detach().cpu().numpy().astype(dt)
    bn = norm.bn
    w, b = (None if t is None else t.detach().cpu().numpy().astype(dt) for t in (bn.weight, bn.bias))
    if bn.training:
        z = sparse.sparse_conv3d_host(x, nbr, kernel)
        return sparse.sparse_norm_host(z, [z.shape[0]], bn.eps, w, b, residual, relu)
    mean, var = (t.detach().cpu().numpy().astype(dt) for t in (bn.running_mean, bn.running_var))
    scale = (1 / np.sqrt(var + dt.type(bn.eps))).astype(dt)
    if w is not None:
        scale = w * scale
    shift = -mean * scale if b is None else b - mean * scale
    return sparse.sparse_conv3d_host(x, nbr, kernel, scale=scale, shift=shift, residual=residual, relu=relu)


class MinkResNet(nn.Module):
    """``MinkResNet(depth, in_channels, num_stages=4, pool=True)`` of the reference (depths 18 and 34), plus ``differentiable``.

    ``forward(coords (n,4) int32, scene_rows, feats (n, in_channels))`` -> a list of ``num_stages`` ``SparseLevel``; with ``pool=True``
    their tensor strides are ``pipeline.MINK_RESNET_STRIDES`` and their rows are those ``pipeline.level_coordinates`` gives for the same
    input.  Kernel maps per forward: the stem (ts 1, k3, s2), the pool (ts 2, k2, s2), and per stage (k3, s2), (k1, s2) and one
    (k3, s1) shared by every stride-1 layer of the stage.  ``os.getenv('BATCHNORM') == '1'`` at construction makes ``norm1`` a batch
    norm, as in the reference."""
    arch_settings = {18: (BasicBlock, (2, 2, 2, 2)), 34: (BasicBlock, (3, 4, 6, 3)),
                     50: ("Bottleneck", (3, 4, 6, 3)), 101: ("Bottleneck", (3, 4, 23, 3)), 152: ("Bottleneck", (3, 8, 36, 3))}

    def __init__(self, depth: int, in_channels: int, num_stages: int = 4, pool: bool = True, differentiable: bool = False):
        super().__init__()
        if depth not in self.arch_settings:
            raise KeyError(f"invalid depth {depth} for resnet")
        block, stage_blocks = self.arch_settings[depth]
        if block is not BasicBlock:
            raise NotImplementedError(f"MinkResNet depth {depth} is built from the {block} block, which is not implemented (depths 18 "
                                      f"and 34 use BasicBlock)")
        assert 4 >= num_stages >= 1
        stage_blocks = stage_blocks[:num_stages]
        self.num_stages, self.pool, self.differentiable = int(num_stages), bool(pool), bool(differentiable)
        self.inplanes = 64
        self.conv1 = SparseConv3d(in_channels, self.inplanes, kernel_size=3, stride=2, differentiable=differentiable)
        if os.getenv("BATCHNORM", "0") == "1":
            self.norm1 = SparseBatchNorm(self.inplanes, differentiable=differentiable)
        else:
            self.norm1 = SparseInstanceNorm(self.inplanes, differentiable=differentiable)
        for i in range(len(stage_blocks)):
            setattr(self, f"layer{i + 1}", self._make_layer(block, 64 * 2 ** i, stage_blocks[i], stride=2))

    def _make_layer(self, block, planes: int, blocks: int, stride: int) -> nn.Sequential:
        d = self.differentiable
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(SparseConv3d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, differentiable=d),
                                       SparseBatchNorm(planes * block.expansion, differentiable=d))
        layers = [block(self.inplanes, planes, stride=stride, downsample=downsample, differentiable=d)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, stride=1, differentiable=d))
        return nn.Sequential(*layers)

    def init_weights(self) -> None:
        """Kaiming-normal (fan_out, ReLU) kernels, BatchNorm weight 1 and bias 0 (mink_resnet.py:80-90)."""
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, SparseConv3d):
                    m.kernel.normal_(0.0, (2.0 / (m.kernel.shape[0] * m.out_channels)) ** 0.5)
                if isinstance(m, SparseBatchNorm):
                    nn.init.constant_(m.bn.weight, 1)
                    nn.init.constant_(m.bn.bias, 0)

    def forward(self, coords: torch.Tensor, scene_rows: Sequence[int], feats: torch.Tensor) -> List[SparseLevel]:
        stem = sparse.kernel_map(coords, scene_rows, 1, 3, 2)
        if isinstance(self.norm1, SparseBatchNorm):
            x = _conv_bn(self.conv1, self.norm1, feats, stem, None, True)
        else:
            x = self.norm1(self.conv1(feats, stem), stem.scene_rows, relu=True)
        cur = stem
        if self.pool:
            cur = sparse.kernel_map(stem.coords, stem.scene_rows, stem.tensor_stride, 2, 2)
            x = sparse.sparse_max_pool3d(x, cur, differentiable=self.differentiable)
        outs = []
        for i in range(self.num_stages):
            ts = cur.tensor_stride
            m_down = sparse.kernel_map(cur.coords, cur.scene_rows, ts, 3, 2)
            m_side = sparse.kernel_map(cur.coords, cur.scene_rows, ts, 1, 2)
            m_same = sparse.kernel_map(m_down.coords, m_down.scene_rows, 2 * ts, 3, 1)
            for j, blk in enumerate(getattr(self, f"layer{i + 1}")):
                x = blk(x, m_down if j == 0 else m_same, m_same, m_side)
            cur = m_down
            outs.append(SparseLevel(feats=x, coords=cur.coords, scene_rows=list(cur.scene_rows), tensor_stride=cur.tensor_stride))
        return outs

    def host_kernel_maps(self, coords, scene_rows: Sequence[int]) -> dict:
        """The kernel maps of one forward from ``kernel_map_host``: ``{"stem" | "pool" | ("down" | "side" | "same", stage): (coords_out,
        scene_rows_out, nbr)}`` -- what ``forward_host`` walks; computed once, they serve any number of restated forwards."""
        maps = {"stem": sparse.kernel_map_host(np.asarray(coords), scene_rows, 1, 3, 2)}
        c, ends, _ = maps["stem"]
        ts = 2
        if self.pool:
            maps["pool"] = sparse.kernel_map_host(c, ends, ts, 2, 2)
            c, ends, _ = maps["pool"]
            ts = 4
        for i in range(self.num_stages):
            maps["down", i] = sparse.kernel_map_host(c, ends, ts, 3, 2)
            maps["side", i] = sparse.kernel_map_host(c, ends, ts, 1, 2)
            c, ends, _ = maps["down", i]
            ts *= 2
            maps["same", i] = sparse.kernel_map_host(c, ends, ts, 3, 1)
        return maps

    def forward_host(self, coords, scene_rows: Sequence[int], feats, dtype=np.float64, maps: dict = None) -> List[SparseLevel]:
        """The same chain from ``kernel_map_host`` / ``sparse_conv3d_host`` / ``sparse_norm_host`` / ``sparse_max_pool3d_host`` in numpy
        ``dtype`` (float64 or float32), with this module's parameters and modes; the running statistics are not updated.  ``maps``:
        ``host_kernel_maps(coords, scene_rows)`` when the caller already has them."""
        dt = np.dtype(dtype)
        maps = self.host_kernel_maps(coords, scene_rows) if maps is None else maps
        _, ends, nbr = maps["stem"]
        x = np.asarray(feats, dt)
        if isinstance(self.norm1, SparseBatchNorm):
            x = _conv_bn_host(self.conv1, self.norm1, x, nbr, None, True, dt)
        else:
            z = sparse.sparse_conv3d_host(x, nbr, self.conv1.kernel.detach().cpu().numpy().astype(dt))
            x = sparse.sparse_norm_host(z, ends, sparse.INSTANCE_NORM_EPS, self.norm1.weight.detach().cpu().numpy().astype(dt),
                                        self.norm1.bias.detach().cpu().numpy().astype(dt), relu=True)
        ts = 2
        if self.pool:
            x = sparse.sparse_max_pool3d_host(x, maps["pool"][2])
            ts = 4
        outs = []
        for i in range(self.num_stages):
            c_out, e_out, n_down = maps["down", i]
            n_side, n_same = maps["side", i][2], maps["same", i][2]
            for j, blk in enumerate(getattr(self, f"layer{i + 1}")):
                h = _conv_bn_host(blk.conv1, blk.norm1, x, n_down if j == 0 else n_same, None, True, dt)
                side = x if blk.downsample is None else _conv_bn_host(blk.downsample[0], blk.downsample[1], x, n_side, None, False, dt)
                x = _conv_bn_host(blk.conv2, blk.norm2, h, n_same, side, True, dt)
            ts *= 2
            outs.append(SparseLevel(feats=x, coords=c_out, scene_rows=list(e_out), tensor_stride=ts))
        return outs


# The reference's own class holds the name in a real EmbodiedScan install (it registers on import of embodiedscan.models): there the
# class is exported without being registered
if REGISTRY_BACKEND != "embodiedscan" and MODELS.get("MinkResNet") is None:
    MODELS.register_module(name="MinkResNet", module=MinkResNet)
