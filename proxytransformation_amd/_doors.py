"""What every stage does at the door of the C ABI, in one place: operands made fp32 / contiguous / checked, a tensor as a pointer, the
current stream as a handle, the opt-in rule of autograd, the shared workspaces, the limits of ``csrc/head.h``, and the cache of
prepared operands (``PreparedOperands``) of the modules whose launches read rearranged weights.  It imports none of the stages, so all
of them import it.  ``train.py`` keeps its raw-handle fast forms (``_st`` / ``_ck`` / ``_p`` / ``_c``): about 500 launches per step pay
for every attribute lookup."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

MAX_SCENES, MAX_QUERIES, MAX_TEXT = 64, 1024, 256     # the limits of the stages behind the neck (csrc/head.h)


def _f32(t: Optional[torch.Tensor], what: str, dev) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{what} (HIP) needs GPU tensors: there is no CPU path")
    if t.device != dev:
        raise ValueError(f"{what}: all tensors must be on {dev}")
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    return t


def _f32_grad(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """fp32 and contiguous WITHOUT leaving the graph: the differentiable path's twin of ``_f32``, and what a backward makes of ``g``."""
    if t is None or (t.dtype == torch.float32 and t.is_contiguous()):
        return t
    return t.to(torch.float32).contiguous()


def _channel_vectors(what: str, C: int, dev, **vecs) -> list:
    """The per-channel operands of a layer, each ``None`` or detached fp32 of ``C`` elements, flat."""
    out = []
    for name, v in vecs.items():
        v = _f32(v, what, dev)
        if v is not None:
            v = v.reshape(-1)
            if v.numel() != C:
                raise ValueError(f"{what}: {name} must have {C} elements, got {v.numel()}")
        out.append(v)
    return out


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _int32_array(values: Sequence[int]):
    """Scene / segment ends as the host array the entry points take."""
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _gpu(what: str, *tensors) -> None:
    if not all(t.is_cuda for t in tensors if t is not None):
        raise RuntimeError(f"{what} (HIP) needs GPU tensors: there is no CPU path")


def _width(what: str, C: int) -> int:
    C = int(C)
    if C % 64 or not 64 <= C <= 512:
        raise ValueError(f"{what}: the feature width must be a multiple of 64 from 64 to 512, got {C}")
    return C


def _mask_bytes(what: str, name: str, mask: torch.Tensor, shape) -> torch.Tensor:
    """``mask`` (the operand ``name`` of ``what``) as the contiguous bool tensor of ``shape`` the entry points read as bytes."""
    _gpu(what, mask)
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {tuple(shape)}, got {tuple(mask.shape)}")
    if mask.dtype != torch.bool or not mask.is_contiguous():
        mask = mask.to(torch.bool).contiguous()
    return mask


def _index(what: str, index: torch.Tensor, B: int) -> int:
    """``K`` of a selection ``index (B,K)``: contiguous int64, as the entry points read it."""
    if index.dtype != torch.int64 or index.dim() != 2 or index.shape[0] != B or not index.is_contiguous():
        raise ValueError(f"{what}: index must be contiguous int64 (B,K), got {index.dtype} {tuple(index.shape)}")
    return int(index.shape[1])


def _np(t, dt=None):
    """A tensor (detached, on the host) or anything array-like as a numpy array of ``dt``; None: of the type it has."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dt is None else a.astype(dt)


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.is_floating_point() and t.requires_grad for t in tensors)


def _train(what: str, differentiable: bool, *tensors) -> bool:
    """The opt-in rule of every layer: record for autograd only with ``differentiable=True`` and an input that requires grad; without the
    flag such an input is refused instead of being answered with a detached result."""
    wanted = _wants_grad(*tensors)
    if wanted and not differentiable:
        raise NotImplementedError(f"{what} is inference-only by default: its backward pass is not enabled, and an input requires grad. "
                                  f"Pass differentiable=True, or call it under torch.no_grad() (or detach the inputs)")
    return wanted


_WORKSPACES: dict = {}             # (tag, device, stream) -> uint8 workspace, reused across layers and steps, grown on demand


def _workspace(tag: str, nbytes: int, dev) -> torch.Tensor:
    key = (tag, str(dev), _stream(dev))
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WORKSPACES[key] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    return ws


class PreparedOperands:
    """Mixin in front of ``nn.Module`` for a module whose launches read operands derived from its weights (concatenated projections,
    folded BatchNorms, transposed kernels): ``_prepare(dev)`` returns the dict that the subclass's ``_build_operands(dev)`` makes, built
    once per device and rebuilt when a parameter or floating-point buffer is replaced or its ``_version`` changes (``load_state_dict`` in
    either form, in-place updates, ``.to()``).  Integer buffers are not watched: ``num_batches_tracked`` moves with every training step
    and no operand reads it.  A write through ``.data`` bumps no version and is not seen: move the module (``.to``) or write in place
    under ``no_grad`` instead.  The walk is host time per forward -- about 0.1 ms over the shipped ResNet's tensors, beside 53 launches."""

    _prepared = None

    def _apply(self, fn, *args, **kwargs):
        self._prepared = None
        return super()._apply(fn, *args, **kwargs)

    def _watched(self) -> list:
        return list(self.parameters()) + [b for b in self.buffers() if b.is_floating_point()]

    def _state_key(self, dev):
        """The device and every watched tensor's identity, storage and ``_version``: a parameter REPLACED by another one of the same
        version is a change too.  ``_prepare`` keeps the tensors it was built from alive, so that no new tensor can take the ``id`` of
        a freed one."""
        return (str(dev),) + tuple((id(t), t.data_ptr(), t._version) for t in self._watched())

    def _prepare(self, dev) -> dict:
        key = self._state_key(dev)
        if self._prepared is not None and self._prepared["key"] == key:
            return self._prepared
        with torch.no_grad():
            prep = self._build_operands(dev)
        prep["key"], prep["tensors"] = key, self._watched()
        self._prepared = prep
        return prep
