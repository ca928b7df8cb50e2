"""Sparse 3D convolution on the voxel rows: kernel maps + gather-GEMM (``csrc/sparse.hip``).

The one line of the reference's detector that ``pipeline.py`` sidesteps is ``x = self.backbone_3d(x)`` (DET:398): a MinkowskiEngine
ResNet (backbones/mink_resnet.py), and MinkowskiEngine has no ROCm build.  What torch cannot substitute is ME's coordinate manager --
"which input row lies at offset d from this output row".  This module supplies that table (``kernel_map``) and the two layers that
consume it (``sparse_conv3d`` with a bias / folded-BatchNorm / residual / ReLU epilogue, ``sparse_max_pool3d``), which is enough to
express every ``MinkowskiConvolution`` and the stem's ``MinkowskiMaxPooling`` of an eval-mode MinkResNet-34.

Semantics (pinned by the numpy restatements ``kernel_map_host`` / ``sparse_conv3d_host`` / ``sparse_max_pool3d_host`` below, which the
kernels are held to bit for bit / to fp32 rounding; they play the role ``ingest.device_choices`` plays for the draws):

* rows ``coords (n,4) int32 = (scene, x, y, z)`` grouped by scene, ``scene_rows[b]`` = end of scene b's rows (what
  ``quantize(..., return_scene_rows=True)`` and ``pipeline.level_coordinates`` return), every coordinate a multiple of the power-of-two
  ``tensor_stride`` ts;
* output rows: stride 1 -- the input rows; stride 2 -- the distinct ``floor(c / 2ts) * 2ts`` per scene in first-occurrence order,
  i.e. exactly ``level_coordinates(coords, scene_rows, 2 * ts, ...)`` (the same kernels emit them);
* offsets (``kernel_offsets``): odd k ``{-(k//2) .. k//2} * ts`` per axis around the output coordinate, even k ``{0 .. k-1} * ts``; never
  across scenes; the offset index -- the row of the weight tensor -- counts x fastest, then y, then z.  That order is OUR READING of
  MinkowskiEngine's region iterator: ME is not available to check it against ("parity unpinned against ME itself");
* ``nbr (n_out, k^3) int32``: the input row at output coordinate + offset, or -1;
* ``out[o] = sum_j feats[nbr[o,j]] @ weight[j]``, ``weight (k^3, Cin, Cout)`` as ME's ``kernel`` parameter; a missing neighbour
  contributes nothing, a row without any is zero before the epilogue (a 1x1 stride-2 convolution has such rows);
* max-pool: the maximum over the present neighbours.

Backward (opt-in, ``differentiable=True`` on both layers and on ``SparseConv3d``; ``csrc/sparse_bwd.hip``): the transposed kernel map
``nbr_t (n_in, k^3)`` -- ``nbr_t[i, j] = o`` with ``nbr[o, j] == i``, filled lazily on the ``KernelMap`` and shared by every layer and
step on that map --, ``dfeats[i] = sum_j gz[nbr_t[i, j]] @ weight[j].T``, ``dweight[j] = sum_o feats[nbr[o, j]].T @ gz[o]``,
``dbias = sum_o gz[o]``, ``dresidual = g * [out > 0]`` with ``gz = g * [out > 0] * scale``; the pool routes each gradient to the offset
that supplied the maximum, ties to the smallest ``j``.  ``scale`` / ``shift`` are a folded FROZEN BatchNorm: constants, no gradient.
Restated in numpy by ``kernel_map_transpose_host`` / ``sparse_conv3d_bwd_host`` / ``sparse_max_pool3d_bwd_host``.  Without
``differentiable=True`` both layers stay inference-only and say so instead of returning a detached result.  In differentiable mode
the widths are a MinkResNet's: Cin a multiple of 64 (or the stem's 3), Cout a multiple of 64.

Not here (out of scope): assembling the backbone, ``MinkowskiInstanceNorm`` (a per-scene segment reduction in plain torch), ``neck_3d``,
double backward, bf16, gradients to ``scale`` / ``shift``.  There is no CPU path for the layers themselves: tensors must be on the GPU
and the library must be built.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _abi

__all__ = ["KernelMap", "SparseConv3d", "kernel_map", "kernel_map_host", "kernel_map_transpose_host", "kernel_offsets", "sparse_conv3d",
           "sparse_conv3d_bwd_host", "sparse_conv3d_host", "sparse_max_pool3d", "sparse_max_pool3d_bwd_host", "sparse_max_pool3d_host"]


# ---------------------------------------------------------------------------------------------------------------- host restatement
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


# ---------------------------------------------------------------------------------------------------------------- device
@dataclass
class KernelMap:
    """The neighbour table of one (kernel_size, stride) pair over the rows of a level; reusable by every layer on those rows."""
    coords: torch.Tensor          # (n_out, 4) int32 output rows (the input tensor itself at stride 1)
    scene_rows: List[int]         # end of each scene's output rows
    nbr: torch.Tensor             # (n_out, kernel_size^3) int32 input row per offset, -1 = absent
    kernel_size: int
    stride: int
    tensor_stride: int            # of the OUTPUT rows
    n_in: int = 0                 # rows of the level the map reads from
    nbr_t: Optional[torch.Tensor] = None      # (n_in, kernel_size^3) int32 transposed map; filled by the first differentiable call


class _MapScratch:
    """Workspace + pinned count words of ``kernel_map`` (one per stream, reused across calls; ``pipeline._CoarsenScratch``'s twin)."""

    def __init__(self, B: int, ncap: int, dev):
        lib = _abi.lib()
        nbytes = lib.ptx_sparse_kernel_map_workspace_bytes(B, ncap)
        if nbytes == 0:
            raise RuntimeError(f"kernel_map: unsupported size B={B}, rows per scene={ncap}")
        self.key = (B, ncap, str(dev))
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self.info = torch.empty((2 + B,), dtype=torch.int32).pin_memory()
        self.info_np = self.info.numpy()


_SCRATCH: dict = {}


def kernel_map(coords: torch.Tensor, scene_rows: Sequence[int], tensor_stride: int, kernel_size: int, stride: int,
               scratch: Optional[dict] = None) -> KernelMap:
    """Kernel map of a ``kernel_size^3`` / ``stride`` layer over the rows ``coords`` (n,4) int32 of tensor stride ``tensor_stride`` (module
    docstring) -- one call of ``ptx_sparse_kernel_map`` on the current stream.  The host waits only for the row count, which the kernel
    publishes through pinned memory; nothing synchronises the device.  ``scratch``: a dict that keeps the workspace per stream (default:
    one shared by the process)."""
    _check_geometry(tensor_stride, kernel_size, stride)
    if not coords.is_cuda:
        raise RuntimeError("kernel_map (HIP) needs GPU tensors: there is no CPU path")
    lib = _abi.lib()
    B = len(scene_rows)
    if B < 1 or B > 64:
        raise ValueError(f"kernel_map: 1 to 64 scenes, got {B}")
    if coords.dtype != torch.int32 or not coords.is_contiguous():
        coords = coords.to(torch.int32).contiguous()
    n_in = int(scene_rows[-1])
    if coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] < n_in:
        raise ValueError(f"kernel_map: coords must be (n,4) with n >= scene_rows[-1] = {n_in}, got {tuple(coords.shape)}")
    dev = coords.device
    lo = [0] + [int(e) for e in scene_rows[:-1]]
    ncap = max(max(int(e) - l for e, l in zip(scene_rows, lo)), 1)
    cap = 1 << (ncap - 1).bit_length()
    scratch = _SCRATCH if scratch is None else scratch
    st = torch.cuda.current_stream(dev)
    sc = scratch.get(st.cuda_stream)
    if sc is None or sc.key[0] != B or sc.key[1] < cap or sc.key[2] != str(dev):
        sc = scratch[st.cuda_stream] = _MapScratch(B, cap, dev)
    kvol = int(kernel_size) ** 3
    nbr = torch.empty((n_in, kvol), dtype=torch.int32, device=dev)
    out_c = torch.empty((n_in, 4), dtype=torch.int32, device=dev) if int(stride) == 2 else coords
    ends_in = (ctypes.c_int32 * B)(*[int(e) for e in scene_rows])
    sc.info_np[:] = -1
    _abi.check(lib.ptx_sparse_kernel_map(coords.data_ptr(), ends_in, B, int(tensor_stride), int(kernel_size), int(stride),
                                         out_c.data_ptr() if int(stride) == 2 else None, sc.info.data_ptr() + 8, nbr.data_ptr(),
                                         sc.info.data_ptr(), sc.ws.data_ptr(), sc.ws.numel(), st.cuda_stream), "ptx_sparse_kernel_map")
    if lib.ptx_wait_counts(sc.info.data_ptr(), 2 + B, 20_000_000) != 0:
        st.synchronize()
    n, overflow = int(sc.info_np[0]), int(sc.info_np[1])
    if n < 0 or n == 0x7fffffff or n > n_in or overflow:
        raise RuntimeError(f"ptx_sparse_kernel_map failed (rows {n}, {overflow} rows with a coordinate outside +-2^18 tensor strides)")
    ends = sc.info_np[2:2 + B].tolist()
    return KernelMap(coords=out_c[:n], scene_rows=ends, nbr=nbr[:n], kernel_size=int(kernel_size), stride=int(stride),
                     tensor_stride=int(tensor_stride) * int(stride), n_in=n_in)


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


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.is_floating_point() and t.requires_grad for t in tensors)


def _inference_only(what: str, *tensors) -> None:
    if _wants_grad(*tensors):
        raise NotImplementedError(f"{what} is inference-only by default: its backward pass is not enabled, and an input requires grad. "
                                  f"Pass differentiable=True, or call it under torch.no_grad() (or detach the inputs)")


_BWD_WS: dict = {}                 # stream -> uint8 workspace of ptx_sparse_conv3d_bwd (reused across layers and steps, grown on demand)


def _bwd_workspace(nbytes: int, dev) -> torch.Tensor:
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    ws = _BWD_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _BWD_WS[key] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    return ws


def _transposed(kmap: KernelMap, n_in: int) -> torch.Tensor:
    """``kmap.nbr_t``, built by one call of ``ptx_sparse_kernel_map_transpose`` on the current stream the first time it is asked for."""
    if kmap.nbr_t is None:
        n_out, kvol = kmap.nbr.shape
        nbr = kmap.nbr if kmap.nbr.is_contiguous() else kmap.nbr.contiguous()
        nbr_t = torch.empty((n_in, kvol), dtype=torch.int32, device=nbr.device)
        _abi.check(_abi.lib().ptx_sparse_kernel_map_transpose(nbr.data_ptr(), n_out, kvol, n_in, nbr_t.data_ptr(),
                                                              torch.cuda.current_stream(nbr.device).cuda_stream),
                   "ptx_sparse_kernel_map_transpose")
        kmap.nbr_t = nbr_t
    return kmap.nbr_t


def _conv_forward(feats, kmap, weight, vecs, residual, relu) -> torch.Tensor:
    n_out, kvol = kmap.nbr.shape
    cin, cout = int(weight.shape[1]), int(weight.shape[2])
    out = torch.empty((n_out, cout), dtype=torch.float32, device=feats.device)
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    _abi.check(_abi.lib().ptx_sparse_conv3d(feats.data_ptr(), feats.shape[0], kmap.nbr.data_ptr(), n_out, kvol, weight.data_ptr(), cin,
                                            cout, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), ptr(residual), int(bool(relu)),
                                            out.data_ptr(), torch.cuda.current_stream(feats.device).cuda_stream), "ptx_sparse_conv3d")
    return out


class _SparseConv3dFn(torch.autograd.Function):
    """feats (n_in,Cin), weight (kvol,Cin,Cout), bias (any shape of Cout elements) or None, residual (n_out,Cout) or None: fp32,
    contiguous, on the device; scale / shift: detached constants."""

    @staticmethod
    def forward(ctx, feats, weight, bias, residual, kmap, scale, shift, relu):
        out = _conv_forward(feats, kmap, weight, (None if bias is None else bias.reshape(-1), scale, shift), residual, relu)
        ctx.kmap, ctx.relu, ctx.scale = kmap, bool(relu), scale
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        ctx.save_for_backward(feats, weight, out if relu else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        feats, weight, out = ctx.saved_tensors
        kmap, scale, relu = ctx.kmap, ctx.scale, ctx.relu
        need_f, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        dev = feats.device
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        n_out, kvol = kmap.nbr.shape
        n_in, cin, cout = int(feats.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        lib = _abi.lib()
        epi = relu or scale is not None
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
        gz = new(n_out, cout) if epi and (need_f or need_w or (need_r and relu and scale is None)) else None
        dres = None
        if need_r:                                           # g * [out > 0]: g itself without ReLU, gz itself without scale
            dres = g if not relu else (gz if scale is None else new(n_out, cout))
        dfeats = new(n_in, cin) if need_f else None
        dweight = new(kvol, cin, cout) if need_w else None
        dbias = new(cout) if need_b else None
        nbytes = lib.ptx_sparse_conv3d_bwd_workspace_bytes(n_out, kvol, cin, cout)
        if nbytes == 0:
            raise ValueError(f"sparse_conv3d backward: unsupported widths Cin={cin} Cout={cout} with {kvol} offsets")
        ws = _bwd_workspace(nbytes, dev) if (need_w or need_b) else None
        nbr_t = _transposed(kmap, n_in) if need_f else None
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        _abi.check(lib.ptx_sparse_conv3d_bwd(g.data_ptr(), ptr(out), ptr(scale), int(relu), feats.data_ptr(), n_in, kmap.nbr.data_ptr(),
                                             ptr(nbr_t), n_out, kvol, weight.data_ptr(), cin, cout, ptr(gz),
                                             ptr(dres) if (relu and scale is not None) else None, ptr(dbias), ptr(dfeats), ptr(dweight),
                                             ptr(ws), 0 if ws is None else ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                   "ptx_sparse_conv3d_bwd")
        if dbias is not None:
            dbias = dbias.reshape(ctx.bias_shape)
        return dfeats, dweight, dbias, dres, None, None, None, None


class _SparseMaxPool3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, kmap):
        n_out, kvol = kmap.nbr.shape
        C = int(feats.shape[1])
        out = torch.empty((n_out, C), dtype=torch.float32, device=feats.device)
        arg = torch.empty((n_out, C), dtype=torch.uint8, device=feats.device)
        _abi.check(_abi.lib().ptx_sparse_max_pool3d_arg(feats.data_ptr(), kmap.nbr.data_ptr(), n_out, kvol, C, out.data_ptr(), arg.data_ptr(),
                                                        torch.cuda.current_stream(feats.device).cuda_stream), "ptx_sparse_max_pool3d_arg")
        ctx.kmap, ctx.n_in = kmap, int(feats.shape[0])
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        kmap, n_in = ctx.kmap, ctx.n_in
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        n_out, kvol = kmap.nbr.shape
        C = int(arg.shape[1])
        dfeats = torch.empty((n_in, C), dtype=torch.float32, device=g.device)
        nbr_t = _transposed(kmap, n_in)
        _abi.check(_abi.lib().ptx_sparse_max_pool3d_bwd(g.data_ptr(), arg.data_ptr(), nbr_t.data_ptr(), n_in, n_out, kvol, C,
                                                        dfeats.data_ptr(), torch.cuda.current_stream(g.device).cuda_stream),
                   "ptx_sparse_max_pool3d_bwd")
        return dfeats, None


def _f32_grad(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """fp32 and contiguous WITHOUT leaving the graph (the differentiable path's twin of ``_f32``)."""
    if t is None or (t.dtype == torch.float32 and t.is_contiguous()):
        return t
    return t.to(torch.float32).contiguous()


def sparse_conv3d(feats: torch.Tensor, kmap: KernelMap, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                  residual: Optional[torch.Tensor] = None, relu: bool = False, differentiable: bool = False) -> torch.Tensor:
    """``out (n_out, Cout) fp32 = epilogue(sum_j feats[nbr[:, j]] @ weight[j])`` -- one launch of ``ptx_sparse_conv3d`` on the current
    stream.  ``weight (k^3, Cin, Cout)``; epilogue, each part optional: ``+ bias``, ``* scale + shift`` (an eval BatchNorm folded by the
    caller), ``+ residual (n_out, Cout)``, ReLU.  Cout a multiple of 64 up to 512; Cin a multiple of 16 up to 512, or 3 with a 3x3x3
    kernel (the stem).  Inference-only unless ``differentiable=True``: then, with grad mode on and ``feats`` / ``weight`` / ``bias`` /
    ``residual`` requiring grad, the same launch is recorded for autograd (``ptx_sparse_conv3d_bwd``; same output bits) -- Cin a
    multiple of 64 up to 512 or the stem's 3; ``scale`` / ``shift`` are constants (a folded frozen BatchNorm) and must not require
    grad: the gradient passes through multiplied by ``scale``."""
    train = False
    if differentiable:
        if _wants_grad(scale, shift):
            raise ValueError("sparse_conv3d(differentiable=True): scale / shift are the constants of a folded frozen BatchNorm and get no "
                             "gradient, but one of them requires grad; detach them (a training BatchNorm is nn.BatchNorm1d on the rows)")
        train = _wants_grad(feats, weight, bias, residual)
    else:
        _inference_only("sparse_conv3d", feats, weight, bias, scale, shift, residual)
    if not (feats.is_cuda and kmap.nbr.is_cuda):
        raise RuntimeError("sparse_conv3d (HIP) needs GPU tensors: there is no CPU path")
    dev = feats.device
    grad_in = (feats, weight, bias, residual)
    feats, weight = _f32(feats, "sparse_conv3d", dev), _f32(weight, "sparse_conv3d", dev)
    kvol = kmap.nbr.shape[1]
    if feats.dim() != 2 or weight.dim() != 3 or weight.shape[0] != kvol or weight.shape[1] != feats.shape[1]:
        raise ValueError(f"sparse_conv3d: feats (n,Cin) and weight ({kvol},Cin,Cout) expected, got {tuple(feats.shape)}, {tuple(weight.shape)}")
    if kmap.n_in and feats.shape[0] != kmap.n_in:
        raise ValueError(f"sparse_conv3d: the kernel map was built over {kmap.n_in} rows, feats has {feats.shape[0]}")
    n_out, cin, cout = kmap.nbr.shape[0], int(weight.shape[1]), int(weight.shape[2])
    vecs = []
    for name, v in (("bias", bias), ("scale", scale), ("shift", shift)):
        v = _f32(v, "sparse_conv3d", dev)
        if v is not None:
            v = v.reshape(-1)
            if v.numel() != cout:
                raise ValueError(f"sparse_conv3d: {name} must have {cout} elements, got {v.numel()}")
        vecs.append(v)
    residual = _f32(residual, "sparse_conv3d", dev)
    if residual is not None and tuple(residual.shape) != (n_out, cout):
        raise ValueError(f"sparse_conv3d: residual must be {(n_out, cout)}, got {tuple(residual.shape)}")
    if not train:
        return _conv_forward(feats, kmap, weight, vecs, residual, relu)
    if not ((cin == 3 and kvol == 27) or (64 <= cin <= 512 and cin % 64 == 0)) or not (64 <= cout <= 512 and cout % 64 == 0):
        raise ValueError(f"sparse_conv3d(differentiable=True): Cin={cin} Cout={cout} with {kvol} offsets -- the backward takes Cin a multiple "
                         f"of 64 up to 512 (or 3 with 27 offsets) and Cout a multiple of 64 up to 512")
    if not kmap.nbr.is_contiguous():
        raise ValueError("sparse_conv3d: the kernel map's nbr must be contiguous")
    f_in, w_in, b_in, r_in = (_f32_grad(t) for t in grad_in)     # the validated operands again, this time inside the graph
    return _SparseConv3dFn.apply(f_in, w_in, b_in, r_in, kmap, vecs[1], vecs[2], bool(relu))


def sparse_max_pool3d(feats: torch.Tensor, kmap: KernelMap, differentiable: bool = False) -> torch.Tensor:
    """``out (n_out, C) fp32 = max_j feats[nbr[:, j]]`` over the present neighbours (``ptx_sparse_max_pool3d``; C a multiple of 4).
    Inference-only unless ``differentiable=True``: then, with grad mode on and ``feats`` requiring grad, ``ptx_sparse_max_pool3d_arg``
    also records which offset supplied each maximum (same output bits) and the backward routes the gradient there.  Ties go to the
    smallest offset index ``j``."""
    train = differentiable and _wants_grad(feats)
    if not differentiable:
        _inference_only("sparse_max_pool3d", feats)
    if not (feats.is_cuda and kmap.nbr.is_cuda):
        raise RuntimeError("sparse_max_pool3d (HIP) needs GPU tensors: there is no CPU path")
    dev = feats.device
    feats_in = feats
    feats = _f32(feats, "sparse_max_pool3d", dev)
    if feats.dim() != 2 or (kmap.n_in and feats.shape[0] != kmap.n_in):
        raise ValueError(f"sparse_max_pool3d: feats ({kmap.n_in},C) expected, got {tuple(feats.shape)}")
    n_out, kvol = kmap.nbr.shape
    if train:
        if feats.shape[1] < 4 or feats.shape[1] % 4 or not kmap.nbr.is_contiguous():
            raise ValueError(f"sparse_max_pool3d(differentiable=True): C={feats.shape[1]} must be a multiple of 4 and nbr contiguous")
        return _SparseMaxPool3dFn.apply(_f32_grad(feats_in), kmap)
    out = torch.empty((n_out, feats.shape[1]), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_sparse_max_pool3d(feats.data_ptr(), kmap.nbr.data_ptr(), n_out, kvol, int(feats.shape[1]), out.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "ptx_sparse_max_pool3d")
    return out


class SparseConv3d(nn.Module):
    """``ME.MinkowskiConvolution(in_channels, out_channels, kernel_size, stride, bias, dimension=3)`` over a ``KernelMap``.  The
    parameters carry ME's names and shapes -- ``kernel (k^3, Cin, Cout)``, ``bias (1, Cout)`` -- so that a reference checkpoint's
    ``backbone_3d.conv1.kernel`` loads by name.  ``forward(feats, kmap, scale=, shift=, residual=, relu=)``: the optional epilogue of
    ``sparse_conv3d`` behind the layer's own bias.  ``differentiable=True`` (an attribute, forwarded by ``forward``) makes the layer
    trainable; the default stays inference-only."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, bias: bool = False,
                 differentiable: bool = False):
        super().__init__()
        self.differentiable = bool(differentiable)
        _check_geometry(1, kernel_size, stride)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride = int(kernel_size), int(stride)
        kvol = self.kernel_size ** 3
        self.kernel = nn.Parameter(torch.empty(kvol, self.in_channels, self.out_channels))
        if bias:
            self.bias = nn.Parameter(torch.zeros(1, self.out_channels))
        else:
            self.register_parameter("bias", None)
        with torch.no_grad():                                    # mink_resnet.py:79-81: kaiming normal, fan_out, relu
            self.kernel.normal_(0.0, (2.0 / (kvol * self.out_channels)) ** 0.5)

    def forward(self, feats: torch.Tensor, kmap: KernelMap, scale=None, shift=None, residual=None, relu: bool = False) -> torch.Tensor:
        if (kmap.kernel_size, kmap.stride) != (self.kernel_size, self.stride):
            raise ValueError(f"SparseConv3d(kernel_size={self.kernel_size}, stride={self.stride}) got a kernel map of "
                             f"kernel_size={kmap.kernel_size}, stride={kmap.stride}")
        return sparse_conv3d(feats, kmap, self.kernel, self.bias, scale, shift, residual, relu, differentiable=self.differentiable)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, bias={self.bias is not None}"
