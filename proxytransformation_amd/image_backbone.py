"""``ResNet``: the 2D image backbone in front of the detector (DET:357-379, ``img_features = self.backbone(img)``) -- ``mmdet.ResNet`` with
Bottleneck blocks, ``style='pytorch'``, every BatchNorm frozen (the shipped ``depth=50, base_channels=16, norm_eval=True,
norm_cfg=dict(type='BN', requires_grad=False)``: levels of 64 / 128 / 256 / 512 channels at strides 4 / 8 / 16 / 32), from the images to
the ``out_indices`` levels on the device.

Per forward: ``ptx_conv_stem`` (7x7 convolution, BatchNorm, ReLU and the max-pool in one launch: the half-resolution map is never
written; uint8 or float32 pixels, the data preprocessor's ``(x - mean) / std`` applied while they are staged), then per Bottleneck
``ptx_conv1x1`` -> ``ptx_conv3x3`` -> (``ptx_conv1x1``: the strided ``downsample``) -> ``ptx_conv1x1`` with the identity added and the ReLU
in its epilogue -- all in ``csrc/conv2d.hip`` on the current stream, restated in numpy by ``image_backbone_host.py``, which is their
specification.  Every BatchNorm is ``sparse.bn_fold``'s ``* scale + shift`` in a convolution's epilogue.  Activations are NCHW float32
between the launches and in the result.  No device synchronise, no torch op on the data path; fp32 on the exact-fp32 matrix instruction
(the stem: plain FMA); no float atomics and a fixed k order: two calls give the same bits, and an image's levels depend neither on the
batch nor on ``chunk``.

By default inference: the forward runs under ``no_grad``, the parameters do not require grad, no gradient reaches the images.
``differentiable=True`` trains what the reference trains (``frozen_stages=1``: the convolutions of stages 2 to 4): the kernels of the
stages ``> frozen_stages`` require grad and a forward in grad mode records the trainable tail as one autograd node, whose backward is
``ptx_conv1x1_bwd`` / ``ptx_conv3x3_bwd`` (csrc/conv2d_bwd.hip) block by block in reverse, restated by ``image_backbone_grad_host.py``.
Out of scope there: ``frozen_stages < 1`` (the stem's and the max-pool's backward), a gradient to the images, a trainable or
training-mode BatchNorm, ``chunk`` while recording, double backward, activation checkpointing (``with_cp``).

Parity-unpinned: the parameter names and shapes are torchvision's / mmdet's as restated from the config and the well-known layout
(tests/golden/image_backbone_state_dict.json), not checked against a real checkpoint file; mmdet and torchvision are not dependencies.

Out of scope: BasicBlock depths (18 / 34), ``style='caffe'``, ``deep_stem``, ``avg_down``, dilation, DCN, plugins, bf16 / fp16.
There is no CPU path: the module must be on the GPU and the library must be built."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _abi, image_backbone_grad_host, image_backbone_host
from ._doors import PreparedOperands, _np, _ptr, _stream, _workspace
from .image_backbone_host import ARCH, EPS, EXPANSION
from .registry import MODELS, REGISTRY_BACKEND
from .sparse import bn_fold

__all__ = ["ResNet"]

MAX_IMAGES = 64 * 64            # per launch (csrc/conv2d.hip: kConvMaxImages)
WHO = "ResNet"


class _Bottleneck(nn.Module):
    def __init__(self, inplanes: int, planes: int, stride: int, downsample: bool):
        super().__init__()
        out = planes * EXPANSION
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes, eps=EPS)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)      # style='pytorch': the stride is here
        self.bn2 = nn.BatchNorm2d(planes, eps=EPS)
        self.conv3 = nn.Conv2d(planes, out, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out, eps=EPS)
        self.stride = int(stride)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, out, 1, stride=stride, bias=False), nn.BatchNorm2d(out, eps=EPS))
        else:
            self.downsample = None


def _refuse(name: str, value, why: str):
    raise NotImplementedError(f"{WHO}: {name}={value!r} is not implemented ({why})")


class _Tail(torch.autograd.Function):
    """The trainable tail as one autograd node: ``(trainable kernels...) -> (the levels of the stages >= frozen)``.  The forward is
    ``ResNet._stages`` with every block's ``x, t1, t2, idn, out`` kept.  The backward walks the blocks in reverse, per block in the
    order of ``image_backbone_grad_host.bottleneck_grad_host``: ``ptx_conv1x1_bwd`` of ``conv3`` (its ``dresidual`` is the identity
    branch's gradient), ``ptx_conv3x3_bwd`` of ``conv2``, ``ptx_conv1x1_bwd`` of the ``downsample`` where there is one (it writes the
    block's input gradient), ``ptx_conv1x1_bwd`` of ``conv1`` with ``dx_accumulate`` onto what the identity branch left.  A level that is
    both an output and the next stage's input: the next stage's first block starts its input gradient from a copy of the level's
    gradient and its downsample accumulates too -- ``(level + downsample) + conv1``; that copy is the one torch op on the data path.
    The first trainable block computes no input gradient.  No device synchronise; no double backward."""

    @staticmethod
    def forward(ctx, net, prep, cur, ch, cw, frozen, levels, *weights):
        keep: list = []
        with torch.no_grad():
            net._stages(prep, cur, ch, cw, frozen, net.out_indices[-1] + 1, levels, 0, keep)
        outs = tuple(levels[s] for s in net.out_indices if s >= frozen)
        ctx.keep, ctx.frozen, ctx.stages = keep, frozen, [s for s in net.out_indices if s >= frozen]
        ctx.names = net._trainable_names(net.out_indices[-1] + 1)
        ctx.save_for_backward(*weights, *outs)              # an in-place write to a kernel or a level before the backward is an error
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        ctx.saved_tensors                                   # (the version check)
        keep, frozen = ctx.keep, ctx.frozen
        dev = keep[0][3].device
        lib, st = _abi.lib(), _stream(dev)
        level_grad = {s: g.to(torch.float32).contiguous() for s, g in zip(ctx.stages, grads)}
        need = dict(zip(ctx.names, ctx.needs_input_grad[7:]))
        like = lambda t: torch.empty(t.shape, dtype=torch.float32, device=dev)      # noqa: E731
        got = {}

        def bwd(KS, name, g, out, scale, relu, x, w, cin, cout, stride, dres, dx, acc):
            n, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
            dw = None
            if need[name]:
                dw = got[name] = torch.empty((cout, cin) if KS == 1 else (cout, 3, 3, cin), dtype=torch.float32, device=dev)
            gz = like(g) if (dx is not None or dw is not None) else None
            nbytes = int(lib.ptx_conv_bwd_workspace_bytes(KS, n, cin, cout, H, W, stride))
            ws = _workspace("conv_bwd", nbytes, dev)
            if KS == 1:
                rc = lib.ptx_conv1x1_bwd(g.data_ptr(), _ptr(out), scale.data_ptr(), relu, x.data_ptr(), n, cin, H, W, w.data_ptr(), cout, stride,
                                         _ptr(gz), _ptr(dres), _ptr(dx), acc, _ptr(dw), ws.data_ptr(), nbytes, st)
            else:
                rc = lib.ptx_conv3x3_bwd(g.data_ptr(), _ptr(out), scale.data_ptr(), relu, x.data_ptr(), n, cin, H, W, w.data_ptr(), stride,
                                         _ptr(gz), _ptr(dres), _ptr(dx), acc, _ptr(dw), ws.data_ptr(), nbytes, st)
            _abi.check(rc, "ptx_conv1x1_bwd" if KS == 1 else "ptx_conv3x3_bwd")

        g = None
        for s, b, d, x, t1, t2, idn, out in reversed(keep):
            p = f"layer{s + 1}.{b}."
            if g is None:
                g = level_grad[s]                           # the last stage
            first = s == frozen and b == 0                  # its input comes from a frozen stage: no input gradient
            dres, dt2, dt1 = like(out), like(t2), like(t1)
            bwd(1, p + "conv3.weight", g, out, d["bn3"][0], 1, t2, d["w3"], d["planes"], d["out"], 1, dres, dt2, 0)
            bwd(3, p + "conv2.weight", dt2, t2, d["bn2"][0], 1, t1, d["w2"], d["planes"], d["planes"], d["stride"], None, dt1, 0)
            dcur, held = None, 1
            if d["wd"] is not None:
                joined = level_grad.get(s - 1) if b == 0 and not first else None
                if not first:
                    dcur = joined.clone() if joined is not None else like(x)
                bwd(1, p + "downsample.0.weight", dres, None, d["bnd"][0], 0, x, d["wd"], d["inplanes"], d["out"], d["stride"], None, dcur,
                    1 if joined is not None else 0)
            elif not first:
                dcur = dres                                 # the identity
            bwd(1, p + "conv1.weight", dt1, t1, d["bn1"][0], 1, x, d["w1"], d["inplanes"], d["planes"], 1, None, dcur, held)
            g = dcur
        dws = []
        for name in ctx.names:
            dw = got.get(name)
            if dw is not None and dw.dim() == 4:
                dw = dw.permute(0, 3, 1, 2)                 # (co,ky,kx,ci) -> the parameter's (co,ci,ky,kx)
            elif dw is not None:
                dw = dw.reshape(dw.shape + (1, 1))
            dws.append(dw)
        return (None,) * 7 + tuple(dws)


class ResNet(PreparedOperands, nn.Module):
    """``ResNet(depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1,2,2,2), dilations=(1,1,1,1),
    out_indices=(0,1,2,3), style='pytorch', ...)``: mmdet's keywords; registered as ``mmdet.ResNet`` and ``ResNet``.  The ``state_dict``
    is torchvision's / mmdet's: ``conv1.weight``, ``bn1.*``, ``layer{s}.{b}.conv{1,2,3}.weight``, ``layer{s}.{b}.bn{1,2,3}.*``,
    ``layer{s}.0.downsample.{0.weight,1.*}``; BatchNorm ``eps`` 1e-5.

    Accepted: ``depth`` 50 / 101 / 152, ``in_channels=3``, ``stem_channels`` (None: ``base_channels``) a multiple of 16 up to 64,
    ``base_channels`` a multiple of 16 up to 64, 1 to 4 stages with mmdet's strides and no dilation.  Accepted and, without
    ``differentiable``, inert (every BatchNorm is frozen in both modes, nothing is initialised from a file): ``frozen_stages``,
    ``norm_cfg`` (``BN``), ``norm_eval``, ``init_cfg``, ``with_cp``, ``zero_init_residual``.  ``differentiable`` (not one of mmdet's; last;
    default False): train the convolution kernels of the stages ``> frozen_stages``, downsamples included -- they get
    ``requires_grad=True``, every BatchNorm parameter and every frozen stage stays False.  It needs ``frozen_stages >= 1``,
    ``norm_eval=True`` and ``norm_cfg=dict(type='BN', requires_grad=False)``, else ``NotImplementedError`` naming the keyword.  ``NotImplementedError`` naming the keyword: ``style='caffe'``, ``deep_stem``,
    ``avg_down``, ``dcn``, ``plugins``, ``conv_cfg``, other ``strides`` / ``dilations``, depths 18 / 34.

    The folded operands the launches take are prepared once per device and rebuilt when a parameter or floating-point buffer is replaced
    or its ``_version`` changes (``load_state_dict``, ``.to()``): ``_doors.PreparedOperands``."""

    def __init__(self, depth: int, in_channels: int = 3, stem_channels: Optional[int] = None, base_channels: int = 64, num_stages: int = 4,
                 strides: Sequence[int] = (1, 2, 2, 2), dilations: Sequence[int] = (1, 1, 1, 1), out_indices: Sequence[int] = (0, 1, 2, 3),
                 style: str = "pytorch", deep_stem: bool = False, avg_down: bool = False, frozen_stages: int = -1, conv_cfg=None,
                 norm_cfg=None, norm_eval: bool = True, dcn=None, stage_with_dcn=(False, False, False, False), plugins=None,
                 with_cp: bool = False, zero_init_residual: bool = True, pretrained=None, init_cfg=None, differentiable: bool = False):
        super().__init__()
        if depth in (18, 34):
            _refuse("depth", depth, "BasicBlock depths are out of scope; 50, 101 or 152")
        if depth not in ARCH:
            raise KeyError(f"{WHO}: invalid depth {depth} for resnet")
        if style != "pytorch":
            _refuse("style", style, "the stride on the 3x3 convolution only: style='pytorch'")
        if deep_stem:
            _refuse("deep_stem", deep_stem, "the 7x7 stem only")
        if avg_down:
            _refuse("avg_down", avg_down, "the strided 1x1 downsample only")
        if dcn is not None:
            _refuse("dcn", dcn, "no deformable convolution")
        if plugins is not None:
            _refuse("plugins", plugins, "no plugins")
        if conv_cfg is not None:
            _refuse("conv_cfg", conv_cfg, "nn.Conv2d only")
        if norm_cfg is not None and dict(norm_cfg).get("type", "BN") not in ("BN", "BN2d"):
            _refuse("norm_cfg", norm_cfg, "frozen BatchNorm only")
        if int(in_channels) != 3:
            _refuse("in_channels", in_channels, "images of 3 planes only")
        if not 1 <= int(num_stages) <= 4:
            raise ValueError(f"{WHO}: num_stages must be 1 to 4, got {num_stages}")
        ns = int(num_stages)
        strides, dilations = tuple(int(s) for s in strides), tuple(int(d) for d in dilations)
        if len(strides) < ns or len(dilations) < ns:
            raise ValueError(f"{WHO}: strides and dilations need {ns} entries, got {strides} and {dilations}")
        if strides[:ns] != (1, 2, 2, 2)[:ns]:
            _refuse("strides", strides, "mmdet's (1, 2, 2, 2) only")
        if any(d != 1 for d in dilations[:ns]):
            _refuse("dilations", dilations, "no dilation")
        out_indices = tuple(int(i) for i in out_indices)
        if not out_indices or list(out_indices) != sorted(set(out_indices)) or out_indices[0] < 0 or out_indices[-1] >= ns:
            raise ValueError(f"{WHO}: out_indices must be ascending stages below num_stages={ns}, got {out_indices}")
        base = int(base_channels)
        stem = base if stem_channels is None else int(stem_channels)
        for name, v in (("base_channels", base), ("stem_channels", stem)):
            if v < 16 or v > 64 or v % 16:
                raise ValueError(f"{WHO}: {name} must be a multiple of 16 from 16 to 64, got {v}")
        self.depth, self.in_channels, self.stem_channels, self.base_channels, self.num_stages = int(depth), 3, stem, base, ns
        self.strides, self.dilations, self.out_indices, self.style = strides[:ns], dilations[:ns], out_indices, style
        self.frozen_stages, self.norm_eval, self.with_cp, self.zero_init_residual = frozen_stages, norm_eval, with_cp, zero_init_residual
        self.stage_blocks = ARCH[depth][:ns]
        self.differentiable = bool(differentiable)
        if self.differentiable:
            # what the backward does not have: the stem's and the max-pool's, a gradient to the images, a BatchNorm that trains
            if not int(frozen_stages) >= 1:
                _refuse("differentiable", differentiable, f"needs frozen_stages >= 1, got {frozen_stages}: the stem and the max-pool have "
                                                          f"no backward and no gradient reaches the images")
            if not norm_eval:
                _refuse("differentiable", differentiable, "needs norm_eval=True: every BatchNorm is the fixed * scale + shift")
            if norm_cfg is None or dict(norm_cfg).get("requires_grad", True):
                _refuse("differentiable", differentiable, "needs norm_cfg=dict(type='BN', requires_grad=False): no BatchNorm parameter is trained")
        self.conv1 = nn.Conv2d(3, stem, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(stem, eps=EPS)
        inplanes = stem
        for s, nb in enumerate(self.stage_blocks):
            planes = base * 2 ** s
            blocks = []
            for b in range(nb):
                stride = self.strides[s] if b == 0 else 1
                blocks.append(_Bottleneck(inplanes, planes, stride, b == 0 and (stride != 1 or inplanes != planes * EXPANSION)))
                inplanes = planes * EXPANSION
            setattr(self, f"layer{s + 1}", nn.Sequential(*blocks))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        for p in self.parameters():
            p.requires_grad_(False)                          # every BatchNorm frozen; no convolution trained without differentiable
        if self.differentiable:
            for name in self._trainable_names():             # the kernels of the stages > frozen_stages, their downsamples included
                self.get_parameter(name).requires_grad_(True)

    @property
    def out_channels(self) -> List[int]:
        return [self.base_channels * 2 ** s * EXPANSION for s in self.out_indices]

    def train(self, mode: bool = True):
        """Every BatchNorm stays in eval mode (``norm_eval=True`` with all of them frozen): both modes run the same forward."""
        super().train(mode)
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.training = False
        return self

    # -- the operands the launches take (PreparedOperands._prepare caches them)
    def _build_operands(self, dev) -> dict:
        f = lambda t: t.detach().to(dev, torch.float32).contiguous()      # noqa: E731
        fold = lambda bn: tuple(f(t) for t in bn_fold(bn))            # noqa: E731
        w = f(self.conv1.weight)                                      # (C0,3,7,7) -> (ci,ky,kx,co): output channel contiguous
        prep = dict(stem=w.permute(1, 2, 3, 0).contiguous(), stem_bgr=w.flip(1).permute(1, 2, 3, 0).contiguous(), bn1=fold(self.bn1),
                    stages=[], norm={})
        for s in range(self.num_stages):
            blocks = []
            for blk in getattr(self, f"layer{s + 1}"):
                planes, out = blk.conv1.out_channels, blk.conv3.out_channels
                d = dict(stride=blk.stride, planes=planes, out=out, inplanes=blk.conv1.in_channels,
                         w1=f(blk.conv1.weight).reshape(planes, -1), bn1=fold(blk.bn1),
                         w2=f(blk.conv2.weight).permute(0, 2, 3, 1).contiguous(), bn2=fold(blk.bn2),     # (co,ky,kx,ci)
                         w3=f(blk.conv3.weight).reshape(out, planes), bn3=fold(blk.bn3), wd=None, bnd=None)
                if blk.downsample is not None:
                    d["wd"], d["bnd"] = f(blk.downsample[0].weight).reshape(out, -1), fold(blk.downsample[1])
                blocks.append(d)
            prep["stages"].append(blocks)
        return prep

    def _norm(self, prep, dev, mean, std, bgr_to_rgb):
        """``mean`` / ``std`` as the two 3-float device vectors the stem takes, in the order of the images' planes."""
        if (mean is None) != (std is None):
            raise ValueError(f"{WHO}: mean and std go together")
        if mean is None:
            return None, None
        m, s = (tuple(float(v) for v in (t.tolist() if hasattr(t, "tolist") else t)) for t in (mean, std))
        if len(m) != 3 or len(s) != 3 or any(v == 0.0 for v in s):
            raise ValueError(f"{WHO}: mean and std must have 3 values, std nonzero, got {m} and {s}")
        if bgr_to_rgb:
            m, s = m[::-1], s[::-1]
        if (m, s) not in prep["norm"]:
            prep["norm"][(m, s)] = (torch.tensor(m, dtype=torch.float32, device=dev), torch.tensor(s, dtype=torch.float32, device=dev))
        return prep["norm"][(m, s)]

    # -- the forward
    def _check(self, imgs):
        if not isinstance(imgs, torch.Tensor) or imgs.dim() not in (4, 5) or imgs.shape[-3] != 3:
            raise ValueError(f"{WHO}: imgs must be (N,3,H,W) or (B,V,3,H,W), got {tuple(getattr(imgs, 'shape', ()))}")
        if imgs.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"{WHO}: imgs must be float32 or uint8, got {imgs.dtype}")
        H, W = int(imgs.shape[-2]), int(imgs.shape[-1])
        if not (32 <= H <= 2048 and 32 <= W <= 2048) or imgs.numel() == 0:
            raise ValueError(f"{WHO}: 1 or more images of 32 to 2048 pixels a side, got {tuple(imgs.shape)}")
        return H, W

    def level_shapes(self, H: int, W: int) -> List[tuple]:
        """``(C_l, H_l, W_l)`` of every stage for images of ``H x W``, sized as torch sizes them."""
        h, w = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
        shapes = []
        for s in range(self.num_stages):
            if self.strides[s] == 2:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            shapes.append((self.base_channels * 2 ** s * EXPANSION, h, w))
        return shapes

    def forward(self, imgs: torch.Tensor, *, mean=None, std=None, bgr_to_rgb: bool = False, chunk: Optional[int] = None):
        """The ``out_indices`` levels, ``(N,C_l,H_l,W_l)`` or ``(B,V,C_l,H_l,W_l)`` float32, of ``imgs (N,3,H,W)`` or ``(B,V,3,H,W)``
        (float32 or uint8, on the device).  ``mean`` / ``std`` (3 values each): the data preprocessor's ``(x - mean) / std``, applied in
        the stem; ``bgr_to_rgb``: its channel swap, which costs nothing (the stem's weight is prepared with its input planes reversed).
        ``chunk``: images per pass (default: all, at most 4096), to bound the workspace; the result has the same bits for every
        ``chunk``.

        With ``differentiable=True``, grad mode on and a trainable kernel that requires grad, the call records for autograd: the stem
        and the frozen stages run as always, the trainable tail is ONE autograd node ``(trainable kernels...) -> (the levels of the
        stages >= frozen_stages)`` whose forward is the same launch sequence with every block's intermediates kept -- the levels have the
        inference forward's bits -- and whose backward is ``_Tail.backward``.  The levels of frozen stages come without ``grad_fn``; no
        gradient is produced for ``imgs``.  ``chunk`` must then be ``None`` or at least the number of images (``ValueError``: the weight
        gradient's bits would depend on it).  Under ``no_grad``, or when no trainable kernel requires grad, this is the inference path and
        nothing is saved."""
        return self._forward(imgs, mean, std, bgr_to_rgb, chunk)

    def _forward(self, imgs, mean, std, bgr_to_rgb, chunk, keep=None):
        """``forward``; ``keep`` (a list, one pass, not recording): the blocks of the stages ``>= frozen_stages`` leave their
        intermediates in it (``relu_masks``)."""
        H, W = self._check(imgs)
        dev = self.conv1.weight.device
        if dev.type != "cuda" or not imgs.is_cuda:
            raise RuntimeError(f"{WHO} (HIP) needs the module and the images on the GPU: there is no CPU path")
        if imgs.device != dev:
            raise ValueError(f"{WHO}: imgs on {imgs.device}, the module on {dev}")
        lead = tuple(imgs.shape[:-3])
        x = imgs.detach().reshape((-1, 3, H, W)).contiguous()
        N = int(x.shape[0])
        step = MAX_IMAGES if chunk is None else int(chunk)
        if step < 1:
            raise ValueError(f"{WHO}: chunk must be positive, got {chunk}")
        recording = keep is None and self._records()
        if recording and step < N:
            raise ValueError(f"{WHO}: chunk={chunk} below the {N} images while recording for autograd: the weight gradient is summed over "
                             f"the pixels of one pass in chunks, so its bits would depend on chunk; pass chunk=None (or >= {N}), or "
                             f"call under torch.no_grad()")
        if recording and N > MAX_IMAGES:
            raise ValueError(f"{WHO}: at most {MAX_IMAGES} images while recording for autograd, got {N}")
        step = min(step, MAX_IMAGES, N)
        with torch.no_grad():
            prep = self._prepare(dev)
            mean_t, std_t = self._norm(prep, dev, mean, std, bgr_to_rgb)
            shapes = self.level_shapes(H, W)
            last = self.out_indices[-1]
            levels = {s: torch.empty((N,) + shapes[s], dtype=torch.float32, device=dev) for s in self.out_indices}
            h2, w2 = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
            # the stages that run here, outside autograd
            frozen = min(self.frozen_stages, last + 1) if recording or keep is not None else last + 1
            for i0 in range(0, N, step):
                n = min(step, N - i0)
                cur = self._stem(prep, x[i0:i0 + n], n, H, W, h2, w2, bgr_to_rgb, mean_t, std_t)
                cur = self._stages(prep, cur, h2, w2, 0, frozen, levels, i0)
            if keep is not None:
                if step < N:
                    raise ValueError(f"{WHO}: the intermediates are kept for one pass only, got chunk={chunk} for {N} images")
                self._stages(prep, cur, *shapes[frozen - 1][1:], frozen, last + 1, levels, 0, keep)
        if recording and frozen <= last:
            ch, cw = shapes[frozen - 1][1:]
            weights = [self.get_parameter(name) for name in self._trainable_names(last + 1)]
            tail = _Tail.apply(self, prep, cur, ch, cw, frozen, levels, *weights)
            levels = {**levels, **dict(zip([s for s in self.out_indices if s >= frozen], tail))}
        return [levels[s].reshape(lead + tuple(levels[s].shape[1:])) for s in self.out_indices]

    def _records(self) -> bool:
        """Whether this call records for autograd: ``differentiable=True``, grad mode on, and a trainable kernel that requires grad."""
        return (self.differentiable and torch.is_grad_enabled()
                and any(self.get_parameter(name).requires_grad for name in self._trainable_names(self.out_indices[-1] + 1)))

    def _trainable_names(self, stages: Optional[int] = None) -> List[str]:
        return image_backbone_grad_host.trainable_kernels(self.stage_blocks[:stages], self.frozen_stages)

    def _stem(self, prep, xin, n, H, W, h2, w2, bgr_to_rgb, mean_t, std_t):
        cur = torch.empty((n, self.stem_channels, h2, w2), dtype=torch.float32, device=xin.device)
        _abi.check(_abi.lib().ptx_conv_stem(xin.data_ptr(), 1 if xin.dtype == torch.uint8 else 0, n, H, W,
                                            prep["stem_bgr" if bgr_to_rgb else "stem"].data_ptr(), self.stem_channels,
                                            prep["bn1"][0].data_ptr(), prep["bn1"][1].data_ptr(), 1, _ptr(mean_t), _ptr(std_t),
                                            cur.data_ptr(), _stream(xin.device)), "ptx_conv_stem")
        return cur

    def _stages(self, prep, cur, ch, cw, s0, s1, levels, i0, keep=None):
        """The launches of stages ``s0 .. s1 - 1`` on ``cur (n,C,ch,cw)``; a stage in ``levels`` ends in ``levels[s][i0:i0 + n]``.  ``keep``:
        a list that receives every block's ``(s, b, operands, x, t1, t2, idn, out)`` -- what the backward reads."""
        dev, n = cur.device, int(cur.shape[0])
        lib, st = _abi.lib(), _stream(dev)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        for s in range(s0, s1):
            blocks = prep["stages"][s]
            for b, d in enumerate(blocks):
                sd = d["stride"]
                ho, wo = (ch - 1) // sd + 1, (cw - 1) // sd + 1
                t1, t2 = new(n, d["planes"], ch, cw), new(n, d["planes"], ho, wo)
                out = levels[s][i0:i0 + n] if (b == len(blocks) - 1 and s in levels) else new(n, d["out"], ho, wo)
                _abi.check(lib.ptx_conv1x1(cur.data_ptr(), n, d["inplanes"], ch, cw, d["w1"].data_ptr(), d["planes"], 1,
                                           d["bn1"][0].data_ptr(), d["bn1"][1].data_ptr(), None, 1, t1.data_ptr(), st), "ptx_conv1x1")
                _abi.check(lib.ptx_conv3x3(t1.data_ptr(), n, d["planes"], ch, cw, d["w2"].data_ptr(), sd, d["bn2"][0].data_ptr(),
                                           d["bn2"][1].data_ptr(), None, 1, t2.data_ptr(), st), "ptx_conv3x3")
                idn = cur
                if d["wd"] is not None:
                    idn = new(n, d["out"], ho, wo)
                    _abi.check(lib.ptx_conv1x1(cur.data_ptr(), n, d["inplanes"], ch, cw, d["wd"].data_ptr(), d["out"], sd,
                                               d["bnd"][0].data_ptr(), d["bnd"][1].data_ptr(), None, 0, idn.data_ptr(), st),
                               "ptx_conv1x1")
                _abi.check(lib.ptx_conv1x1(t2.data_ptr(), n, d["planes"], ho, wo, d["w3"].data_ptr(), d["out"], 1,
                                           d["bn3"][0].data_ptr(), d["bn3"][1].data_ptr(), idn.data_ptr(), 1, out.data_ptr(), st),
                           "ptx_conv1x1")
                if keep is not None:
                    keep.append((s, b, d, cur, t1, t2, idn, out))
                cur, ch, cw = out, ho, wo
        return cur

    def relu_masks(self, imgs: torch.Tensor, *, mean=None, std=None, bgr_to_rgb: bool = False) -> dict:
        """``{"layer{s}.{b}.t1" / ".t2" / ".out": [. > 0]}`` (numpy bool) of every block of the stages ``>= frozen_stages`` in the device's
        own forward: what ``grad_host(..., masks=)`` replays when a device backward is compared with the host's."""
        keep: list = []
        self._forward(imgs, mean, std, bgr_to_rgb, None, keep)
        masks = {}
        for s, b, _, _, t1, t2, _, out in keep:
            for name, t in (("t1", t1), ("t2", t2), ("out", out)):
                masks[f"layer{s + 1}.{b}.{name}"] = (t > 0).cpu().numpy()
        return masks

    def grad_host(self, imgs, grads, dtype=np.float64, masks=None, mean=None, std=None, bgr_to_rgb: bool = False) -> dict:
        """``{kernel name: d loss / d kernel}`` of every trainable kernel, in numpy ``dtype``, for the gradients ``grads`` of the
        ``out_indices`` levels (``image_backbone_grad_host.resnet_grad_host``): the specification of the recorded backward.  It calls no
        device code.  ``masks``: ``relu_masks``'s, to replay a device forward's ReLU decisions."""
        x = _np(imgs)
        params = {k: _np(v) for k, v in self.state_dict().items()}
        gs = [_np(g).reshape((-1,) + tuple(_np(g).shape[-3:])) for g in grads]
        return image_backbone_grad_host.resnet_grad_host(params, x.reshape((-1,) + x.shape[-3:]),  gs,
                                                         self.stage_blocks[:self.out_indices[-1] + 1], self.strides, self.out_indices,
                                                         self.frozen_stages, dtype, masks, mean, std, bgr_to_rgb)

    def forward_host(self, imgs, dtype=np.float64, mean=None, std=None, bgr_to_rgb: bool = False) -> List[np.ndarray]:
        """The same chain in numpy ``dtype`` (``image_backbone_host.resnet_host``): the specification.  It calls no device code."""
        x = _np(imgs)
        if x.ndim not in (4, 5) or x.shape[-3] != 3:
            raise ValueError(f"{WHO}.forward_host: imgs must be (N,3,H,W) or (B,V,3,H,W), got {x.shape}")
        lead = x.shape[:-3]
        params = {k: _np(v) for k, v in self.state_dict().items()}
        outs = image_backbone_host.resnet_host(params, x.reshape((-1,) + x.shape[-3:]), self.stage_blocks[:self.out_indices[-1] + 1],
                                               self.strides, self.out_indices, dtype, mean, std, bgr_to_rgb)
        return [o.reshape(lead + o.shape[1:]) for o in outs]


# In a real EmbodiedScan install mmdet's own class holds both names: there the class is exported without being registered
if REGISTRY_BACKEND != "embodiedscan":
    for _name in ("mmdet.ResNet", "ResNet"):
        if MODELS.get(_name) is None:
            MODELS.register_module(name=_name, module=ResNet)
