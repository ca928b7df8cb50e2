"""Sparse 3D convolution on the voxel rows: kernel maps + gather-GEMM (``csrc/sparse.hip``).

The one line of the reference's detector that ``pipeline.py`` sidesteps is ``x = self.backbone_3d(x)`` (DET:398): a MinkowskiEngine
ResNet (backbones/mink_resnet.py), and MinkowskiEngine has no ROCm build.  What torch cannot substitute is ME's coordinate manager --
"which input row lies at offset d from this output row".  This module supplies that table (``kernel_map``) and the two layers that
consume it (``sparse_conv3d`` with a bias / folded-BatchNorm / residual / ReLU epilogue, ``sparse_max_pool3d``), which is enough to
express every ``MinkowskiConvolution`` and the stem's ``MinkowskiMaxPooling`` of an eval-mode MinkResNet-34.

Semantics (pinned by the numpy restatements ``kernel_map_host`` / ``sparse_conv3d_host`` / ``sparse_max_pool3d_host`` of
``sparse_host.py``, re-exported here, which the kernels are held to bit for bit / to fp32 rounding; they play the role ``ingest.device_choices`` plays for the draws):

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

Norms (``csrc/sparse_norm.hip``): ``sparse_instance_norm`` (``MinkowskiInstanceNorm``: per scene, biased variance, ``INSTANCE_NORM_EPS``
inside the square root -- OUR READING of ``MinkowskiInstanceNormFunction``, parity unpinned against ME itself) and ``sparse_batch_norm``
(an ``nn.BatchNorm1d`` on the rows: in training mode one segment over all rows with the running statistics updated by the kernel, in
eval mode the affine map from the running statistics) are one family of streaming kernels, "column moments per row segment ->
normalise -> affine (+ residual)(+ ReLU)", forward and backward, restated in numpy by ``sparse_norm_host`` / ``sparse_norm_bwd_host``.
The same opt-in rule: inference-only unless ``differentiable=True``.  ``backbone.MinkResNet`` assembles all of this.

``neck_3d`` is ``neck.MinkNeck`` (``neck.py``; eval forward, and with ``differentiable=True`` the training chain).  Not here (out of scope): double backward, bf16, gradients to ``scale`` / ``shift``, SyncBatchNorm across ranks.  There is no
CPU path for the layers themselves: tensors must be on the GPU and the library must be built.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch
from torch import nn

from . import _abi
from ._doors import _channel_vectors, _f32, _f32_grad, _int32_array, _ptr, _stream, _train, _wants_grad, _workspace
from .sparse_host import (_check_geometry, _segments, kernel_map_host, kernel_map_transpose_host, kernel_offsets,     # noqa: F401
                          sparse_conv3d_bwd_host, sparse_conv3d_host, sparse_max_pool3d_bwd_host, sparse_max_pool3d_host,
                          sparse_norm_bwd_host, sparse_norm_host)

__all__ = ["INSTANCE_NORM_EPS", "KernelMap", "SparseBatchNorm", "SparseConv3d", "SparseInstanceNorm", "bn_fold", "kernel_map",
           "kernel_map_host", "kernel_map_transpose_host", "kernel_offsets", "sparse_batch_norm", "sparse_conv3d", "sparse_conv3d_bwd_host",
           "sparse_conv3d_host", "sparse_instance_norm", "sparse_max_pool3d", "sparse_max_pool3d_bwd_host", "sparse_max_pool3d_host",
           "sparse_norm_bwd_host", "sparse_norm_host", "sparse_segment_norm"]

# MinkowskiInstanceNorm's epsilon, inside the square root: 1 / (var_biased + 1e-8).sqrt() per scene.  The ONE place that fixes it (our
# reading of MinkowskiInstanceNormFunction; parity unpinned against ME itself)
INSTANCE_NORM_EPS = 1e-8


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
    ends_in = _int32_array(scene_rows)
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


def _transposed(kmap: KernelMap, n_in: int) -> torch.Tensor:
    """``kmap.nbr_t``, built by one call of ``ptx_sparse_kernel_map_transpose`` on the current stream the first time it is asked for."""
    if kmap.nbr_t is None:
        n_out, kvol = kmap.nbr.shape
        nbr = kmap.nbr if kmap.nbr.is_contiguous() else kmap.nbr.contiguous()
        nbr_t = torch.empty((n_in, kvol), dtype=torch.int32, device=nbr.device)
        _abi.check(_abi.lib().ptx_sparse_kernel_map_transpose(nbr.data_ptr(), n_out, kvol, n_in, nbr_t.data_ptr(),
                                                              _stream(nbr.device)), "ptx_sparse_kernel_map_transpose")
        kmap.nbr_t = nbr_t
    return kmap.nbr_t


def _conv_forward(feats, kmap, weight, vecs, residual, relu, elu=False) -> torch.Tensor:
    n_out, kvol = kmap.nbr.shape
    cin, cout = int(weight.shape[1]), int(weight.shape[2])
    out = torch.empty((n_out, cout), dtype=torch.float32, device=feats.device)
    if elu or cin > 512:                                     # the neck's entry point: activation selector, Cin up to 1024
        _abi.check(_abi.lib().ptx_sparse_conv3d_act(feats.data_ptr(), feats.shape[0], kmap.nbr.data_ptr(), n_out, kvol, weight.data_ptr(), cin,
                                                    cout, _ptr(vecs[0]), _ptr(vecs[1]), _ptr(vecs[2]), _ptr(residual),
                                                    2 if elu else int(bool(relu)), out.data_ptr(), _stream(feats.device)),
                   "ptx_sparse_conv3d_act")
        return out
    _abi.check(_abi.lib().ptx_sparse_conv3d(feats.data_ptr(), feats.shape[0], kmap.nbr.data_ptr(), n_out, kvol, weight.data_ptr(), cin,
                                            cout, _ptr(vecs[0]), _ptr(vecs[1]), _ptr(vecs[2]), _ptr(residual), int(bool(relu)),
                                            out.data_ptr(), _stream(feats.device)), "ptx_sparse_conv3d")
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
        g = _f32_grad(g)
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
        ws = _workspace("conv_bwd", nbytes, dev) if (need_w or need_b) else None
        nbr_t = _transposed(kmap, n_in) if need_f else None
        _abi.check(lib.ptx_sparse_conv3d_bwd(g.data_ptr(), _ptr(out), _ptr(scale), int(relu), feats.data_ptr(), n_in, kmap.nbr.data_ptr(),
                                             _ptr(nbr_t), n_out, kvol, weight.data_ptr(), cin, cout, _ptr(gz),
                                             _ptr(dres) if (relu and scale is not None) else None, _ptr(dbias), _ptr(dfeats), _ptr(dweight),
                                             _ptr(ws), 0 if ws is None else ws.numel(), _stream(dev)),
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
                                                        _stream(feats.device)), "ptx_sparse_max_pool3d_arg")
        ctx.kmap, ctx.n_in = kmap, int(feats.shape[0])
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        kmap, n_in = ctx.kmap, ctx.n_in
        g = _f32_grad(g)
        n_out, kvol = kmap.nbr.shape
        C = int(arg.shape[1])
        dfeats = torch.empty((n_in, C), dtype=torch.float32, device=g.device)
        nbr_t = _transposed(kmap, n_in)
        _abi.check(_abi.lib().ptx_sparse_max_pool3d_bwd(g.data_ptr(), arg.data_ptr(), nbr_t.data_ptr(), n_in, n_out, kvol, C,
                                                        dfeats.data_ptr(), _stream(g.device)),
                   "ptx_sparse_max_pool3d_bwd")
        return dfeats, None


def sparse_conv3d(feats: torch.Tensor, kmap: KernelMap, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                  residual: Optional[torch.Tensor] = None, relu: bool = False, differentiable: bool = False,
                  elu: bool = False) -> torch.Tensor:
    """``out (n_out, Cout) fp32 = epilogue(sum_j feats[nbr[:, j]] @ weight[j])`` -- one launch of ``ptx_sparse_conv3d`` on the current
    stream.  ``weight (k^3, Cin, Cout)``; epilogue, each part optional: ``+ bias``, ``* scale + shift`` (an eval BatchNorm folded by the
    caller), ``+ residual (n_out, Cout)``, ReLU.  Cout a multiple of 64 up to 512; Cin a multiple of 16 up to 512, or 3 with a 3x3x3
    kernel (the stem).  Inference-only unless ``differentiable=True``: then, with grad mode on and ``feats`` / ``weight`` / ``bias`` /
    ``residual`` requiring grad, the same launch is recorded for autograd (``ptx_sparse_conv3d_bwd``; same output bits) -- Cin a
    multiple of 64 up to 1024 or the stem's 3; ``scale`` / ``shift`` are constants (a folded frozen BatchNorm) and must not require
    grad: the gradient passes through multiplied by ``scale``.  ``elu=True`` (the neck's layers: ELU with alpha = 1 instead of the ReLU;
    not both) or ``Cin > 512`` (up to 1024) goes through ``ptx_sparse_conv3d_act``, the same kernel; ``elu`` is inference-only."""
    if elu and relu:
        raise ValueError("sparse_conv3d: elu and relu are one activation slot; pass one of them")
    if elu and differentiable and _wants_grad(feats, weight, bias, residual):
        raise NotImplementedError("sparse_conv3d(elu=True) is inference-only: the backward pass through the ELU epilogue is not implemented")
    if differentiable and _wants_grad(scale, shift):
        raise ValueError("sparse_conv3d(differentiable=True): scale / shift are the constants of a folded frozen BatchNorm and get no "
                         "gradient, but one of them requires grad; detach them (a training BatchNorm is nn.BatchNorm1d on the rows)")
    train = _train("sparse_conv3d", differentiable, feats, weight, bias, scale, shift, residual)
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
    vecs = _channel_vectors("sparse_conv3d", cout, dev, bias=bias, scale=scale, shift=shift)
    residual = _f32(residual, "sparse_conv3d", dev)
    if residual is not None and tuple(residual.shape) != (n_out, cout):
        raise ValueError(f"sparse_conv3d: residual must be {(n_out, cout)}, got {tuple(residual.shape)}")
    if not train:
        return _conv_forward(feats, kmap, weight, vecs, residual, relu, elu)
    if not ((cin == 3 and kvol == 27) or (64 <= cin <= 1024 and cin % 64 == 0)) or not (64 <= cout <= 512 and cout % 64 == 0):
        raise ValueError(f"sparse_conv3d(differentiable=True): Cin={cin} Cout={cout} with {kvol} offsets -- the backward takes Cin a multiple "
                         f"of 64 up to 1024 (or 3 with 27 offsets) and Cout a multiple of 64 up to 512")
    if not kmap.nbr.is_contiguous():
        raise ValueError("sparse_conv3d: the kernel map's nbr must be contiguous")
    f_in, w_in, b_in, r_in = (_f32_grad(t) for t in grad_in)     # the validated operands again, this time inside the graph
    return _SparseConv3dFn.apply(f_in, w_in, b_in, r_in, kmap, vecs[1], vecs[2], bool(relu))


def sparse_max_pool3d(feats: torch.Tensor, kmap: KernelMap, differentiable: bool = False) -> torch.Tensor:
    """``out (n_out, C) fp32 = max_j feats[nbr[:, j]]`` over the present neighbours (``ptx_sparse_max_pool3d``; C a multiple of 4).
    Inference-only unless ``differentiable=True``: then, with grad mode on and ``feats`` requiring grad, ``ptx_sparse_max_pool3d_arg``
    also records which offset supplied each maximum (same output bits) and the backward routes the gradient there.  Ties go to the
    smallest offset index ``j``."""
    train = _train("sparse_max_pool3d", differentiable, feats)
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
                                                _stream(dev)), "ptx_sparse_max_pool3d")
    return out


# ---------------------------------------------------------------------------------------------------------------- norms
def _norm_workspace(n: int, S: int, C: int, dev) -> torch.Tensor:
    nbytes = _abi.lib().ptx_sparse_norm_workspace_bytes(n, S, C)
    if nbytes == 0:
        raise ValueError(f"sparse norm: unsupported size, {n} rows x {C} channels in {S} segments (channels: a multiple of 64 up to 512; "
                         f"1 to 64 segments)")
    return _workspace("norm", nbytes, dev)


def _norm_forward(x, ends, eps, weight, bias, residual, relu, running=None, momentum=0.0, elu=False):
    """One call of ``ptx_sparse_norm_fwd`` (``elu``: ``ptx_sparse_norm_fwd_act`` with selector 2) on the current stream:
    ``(out, stats)``."""
    n, C = int(x.shape[0]), int(x.shape[1])
    S = len(ends)
    dev = x.device
    ws = _norm_workspace(n, S, C, dev)
    out = torch.empty_like(x)
    stats = torch.empty((S, 2, C), dtype=torch.float32, device=dev)
    seg = _int32_array(ends)
    rm, rv = running if running is not None else (None, None)
    if elu:
        _abi.check(_abi.lib().ptx_sparse_norm_fwd_act(x.data_ptr(), seg, S, n, C, float(eps), _ptr(weight), _ptr(bias), _ptr(residual), 2, _ptr(rm),
                                                      _ptr(rv), float(momentum), stats.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      _stream(dev)), "ptx_sparse_norm_fwd_act")
        return out, stats
    _abi.check(_abi.lib().ptx_sparse_norm_fwd(x.data_ptr(), seg, S, n, C, float(eps), _ptr(weight), _ptr(bias), _ptr(residual), int(bool(relu)),
                                              _ptr(rm), _ptr(rv), float(momentum), stats.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _stream(dev)), "ptx_sparse_norm_fwd")
    return out, stats


def _norm_apply(x, ends, stats, weight, bias, residual, relu):
    n, C = int(x.shape[0]), int(x.shape[1])
    S = len(ends)
    out = torch.empty_like(x)
    seg = _int32_array(ends)
    _abi.check(_abi.lib().ptx_sparse_norm_apply(x.data_ptr(), seg, S, n, C, stats.data_ptr(), _ptr(weight), _ptr(bias), _ptr(residual),
                                                int(bool(relu)), out.data_ptr(), _stream(x.device)),
               "ptx_sparse_norm_apply")
    return out


class _SparseNormFn(torch.autograd.Function):
    """x (n,C), weight / bias (any shape of C elements) or None, residual (n,C) or None: fp32, contiguous, on the device; ``running``:
    ``(running_mean, running_var)`` updated in place by the kernel, or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, ends, eps, relu, running, momentum, elu):
        w = None if weight is None else weight.reshape(-1)
        out, stats = _norm_forward(x, ends, eps, w, None if bias is None else bias.reshape(-1), residual, relu, running, momentum, elu)
        ctx.ends, ctx.relu, ctx.elu = ends, bool(relu), bool(elu)
        ctx.shapes = (None if weight is None else tuple(weight.shape), None if bias is None else tuple(bias.shape))
        ctx.save_for_backward(x, stats, w, out if (relu or elu) else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, stats, w, out = ctx.saved_tensors
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        dev = x.device
        g = _f32_grad(g)
        n, C = int(x.shape[0]), int(x.shape[1])
        S = len(ctx.ends)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
        dx = new(n, C) if need_x else None
        dw = new(C) if need_w else None
        db = new(C) if need_b else None
        dres = None
        act = ctx.relu or ctx.elu
        if need_r:                                           # g * [out > 0] (ELU: g * (out > 0 ? 1 : out + 1)): g itself without activation
            dres = new(n, C) if act else g
        if ctx.elu and (need_x or need_w or need_b or need_r):
            ws = _norm_workspace(n, S, C, dev)
            _abi.check(_abi.lib().ptx_sparse_norm_bwd_act(g.data_ptr(), x.data_ptr(), _ptr(out), 2, _int32_array(ctx.ends), S, n, C,
                                                          stats.data_ptr(), _ptr(w), _ptr(dx), _ptr(dw), _ptr(db), _ptr(dres), ws.data_ptr(),
                                                          ws.numel(), _stream(dev)), "ptx_sparse_norm_bwd_act")
        elif need_x or need_w or need_b or (need_r and ctx.relu):
            ws = _norm_workspace(n, S, C, dev)
            seg = _int32_array(ctx.ends)
            _abi.check(_abi.lib().ptx_sparse_norm_bwd(g.data_ptr(), x.data_ptr(), _ptr(out), seg, S, n, C, stats.data_ptr(), _ptr(w), _ptr(dx),
                                                      _ptr(dw), _ptr(db), _ptr(dres) if ctx.relu else None, ws.data_ptr(), ws.numel(),
                                                      _stream(dev)), "ptx_sparse_norm_bwd")
        if dw is not None:
            dw = dw.reshape(ctx.shapes[0])
        if db is not None:
            db = db.reshape(ctx.shapes[1])
        return dx, dw, db, dres, None, None, None, None, None, None


def _norm_operands(what: str, feats, weight, bias, residual):
    """The validated, detached fp32 operands of a norm call: ``(x, weight (C) or None, bias (C) or None, residual or None)``."""
    if not feats.is_cuda:
        raise RuntimeError(f"{what} (HIP) needs GPU tensors: there is no CPU path")
    dev = feats.device
    x = _f32(feats, what, dev)
    if x.dim() != 2 or x.shape[1] < 64 or x.shape[1] > 512 or x.shape[1] % 64:
        raise ValueError(f"{what}: feats (n,C) with C a multiple of 64 up to 512 expected, got {tuple(x.shape)}")
    C = int(x.shape[1])
    vecs = _channel_vectors(what, C, dev, weight=weight, bias=bias)
    residual = _f32(residual, what, dev)
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
        raise ValueError(f"{what}: residual must be {tuple(x.shape)}, got {tuple(residual.shape)}")
    return x, vecs[0], vecs[1], residual


def sparse_segment_norm(feats: torch.Tensor, seg_end: Sequence[int], eps: float, weight: Optional[torch.Tensor] = None,
                        bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, relu: bool = False,
                        differentiable: bool = False, return_stats: bool = False):
    """The norm kernels as they are: per segment ``[seg_end[s-1], seg_end[s])`` of the rows ``feats (n, C)`` fp32 (C a multiple of 64 up to
    512; 1 to 64 segments, empty ones allowed) and column, ``out = relu?((feats - mean) / sqrt(var_biased + eps) * weight + bias
    (+ residual))`` -- one call of ``ptx_sparse_norm_fwd`` on the current stream (two reads and one write of the rows).  An empty
    segment writes nothing; a one-row segment gives ``bias (+ residual)``.  ``return_stats`` (inference only): ``(out, stats (S, 2, C))``
    with the segments' ``(mean, rstd)``.  Inference-only unless ``differentiable=True``: then, with grad mode on and ``feats`` /
    ``weight`` / ``bias`` / ``residual`` requiring grad, the same launches are recorded for autograd (``ptx_sparse_norm_bwd``; same
    output bits)."""
    train = _train("sparse_segment_norm", differentiable, feats, weight, bias, residual)
    x, w, b, res = _norm_operands("sparse_segment_norm", feats, weight, bias, residual)
    ends = _segments(seg_end, x.shape[0])
    if not train:
        out, stats = _norm_forward(x, ends, eps, w, b, res, relu)
        return (out, stats) if return_stats else out
    if return_stats:
        raise ValueError("sparse_segment_norm: return_stats is for inference calls")
    return _SparseNormFn.apply(_f32_grad(feats), _f32_grad(weight), _f32_grad(bias), _f32_grad(residual), ends, float(eps), bool(relu), None,
                               0.0, False)


def sparse_instance_norm(feats: torch.Tensor, scene_rows: Sequence[int], weight: Optional[torch.Tensor] = None,
                         bias: Optional[torch.Tensor] = None, relu: bool = False, differentiable: bool = False) -> torch.Tensor:
    """``MinkowskiInstanceNorm`` on the rows: ``sparse_segment_norm`` per scene -- ``scene_rows[b]`` = end of scene b's rows -- with the
    biased variance and ``INSTANCE_NORM_EPS`` inside the square root, ``weight`` / ``bias`` of ``C`` elements in any shape (ME's are
    ``(1, C)``), an optional fused ReLU.  Inference-only unless ``differentiable=True``."""
    return sparse_segment_norm(feats, scene_rows, INSTANCE_NORM_EPS, weight, bias, None, relu, differentiable)


_BN_CACHE: dict = {}               # id(bn) -> (weak reference, key, {"fold": (scale, shift), "stats": (1,2,C)})


def _bn_cached(bn: nn.Module, kind: str):
    """Vectors derived from an eval BatchNorm's four tensors, cached per module and rebuilt when any tensor's ``_version`` (or storage)
    changes -- a backbone of 36 BatchNorms must not pay 36 x 5 tiny launches per forward.  Tensors made under ``torch.inference_mode()``
    carry no version: for them the vectors are rebuilt on every call."""
    import weakref
    tensors = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if any(t is not None and t.is_inference() for t in tensors):
        made = {}                                            # an inference tensor has no version counter: nothing to key on, no caching
    else:
        key = tuple((None if t is None else (t._version, t.data_ptr(), str(t.device))) for t in tensors) + (float(bn.eps),)
        hit = _BN_CACHE.get(id(bn))
        if hit is None or hit[0]() is not bn or hit[1] != key:
            ident = id(bn)
            hit = _BN_CACHE[ident] = (weakref.ref(bn, lambda _r, ident=ident: _BN_CACHE.pop(ident, None)), key, {})
        made = hit[2]
    if kind not in made:
        with torch.no_grad():
            mean, var = bn.running_mean.float(), bn.running_var.float()
            rstd = torch.rsqrt(var + bn.eps)
            if kind == "stats":
                made[kind] = torch.stack([mean, rstd]).unsqueeze(0).contiguous()
            else:
                scale = rstd if bn.weight is None else bn.weight.detach().float() * rstd
                shift = -mean * scale if bn.bias is None else bn.bias.detach().float() - mean * scale
                made[kind] = (scale.contiguous(), shift.contiguous())
    return made[kind]


def bn_fold(bn: nn.Module):
    """``(scale, shift)`` of an eval-mode ``nn.BatchNorm1d`` -- ``y = x * scale + shift`` --, the operands of ``sparse_conv3d``'s
    epilogue; cached per module, rebuilt when the ``_version`` of any of its four tensors changes."""
    _check_bn(bn)
    return _bn_cached(bn, "fold")


def _check_bn(bn) -> None:
    if not isinstance(bn, nn.modules.batchnorm._BatchNorm):
        raise TypeError(f"an nn.BatchNorm1d expected, got {type(bn).__name__}")
    if not bn.track_running_stats or bn.running_mean is None:
        raise ValueError("sparse_batch_norm: track_running_stats=False is not supported (the eval path is the affine map from the running "
                         "statistics)")
    if bn.momentum is None:
        raise ValueError("sparse_batch_norm: momentum=None (cumulative moving average) is not supported; give the BatchNorm a momentum")


def sparse_batch_norm(feats: torch.Tensor, bn: nn.Module, residual: Optional[torch.Tensor] = None, relu: bool = False,
                      differentiable: bool = False, elu: bool = False) -> torch.Tensor:
    """``act(bn(feats) (+ residual))``, ``act`` the ReLU (``relu``), the ELU with alpha = 1 (``elu``, training mode only: the neck's
    blocks, ``ptx_sparse_norm_fwd_act`` / ``ptx_sparse_norm_bwd_act``; not both) or nothing, for an ``nn.BatchNorm1d`` on the rows
    ``feats (n, C)`` (C a multiple of 64 up to 512).
    ``bn.training``: the batch statistics of one segment over all rows; the kernel updates ``bn.running_mean`` / ``bn.running_var`` in
    place by ``nn.BatchNorm1d``'s rule (unbiased variance) and ``bn.num_batches_tracked`` is incremented; ``n == 1`` is refused with
    torch's own ``ValueError``.  Eval: the affine map from the running statistics through the same apply kernel.  Inference-only unless
    ``differentiable=True``; then the training-mode call is recorded for autograd (gradients to ``feats``, ``bn.weight``, ``bn.bias``,
    ``residual``).  An eval-mode BatchNorm is a constant affine map: to train through it fold it into ``sparse_conv3d`` (``bn_fold``)."""
    if elu and relu:
        raise ValueError("sparse_batch_norm: elu and relu are one activation slot; pass one of them")
    _check_bn(bn)
    if elu and not bn.training:
        raise NotImplementedError("sparse_batch_norm(elu=True) in eval mode: fold the BatchNorm into the convolution's epilogue "
                                  "(bn_fold, sparse_conv3d(elu=True)), or call bn.train()")
    train = _train("sparse_batch_norm", differentiable, feats, bn.weight, bn.bias, residual)
    if feats.dim() == 2 and bn.num_features != feats.shape[1]:
        raise ValueError(f"sparse_batch_norm: the BatchNorm has {bn.num_features} features, feats has {feats.shape[1]} channels")
    x, w, b, res = _norm_operands("sparse_batch_norm", feats, bn.weight, bn.bias, residual)
    n, C = int(x.shape[0]), int(x.shape[1])
    if not bn.training:
        if train:
            raise NotImplementedError("sparse_batch_norm(differentiable=True) in eval mode: a frozen BatchNorm is a constant affine map; fold "
                                      "it into sparse_conv3d's scale / shift (bn_fold) to train through it, or call bn.train()")
        return _norm_apply(x, [n], _bn_cached(bn, "stats"), w, b, res, relu)
    if n <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([n, C])}")
    running = (bn.running_mean, bn.running_var)
    if any(t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device for t in running):
        raise ValueError("sparse_batch_norm: running_mean / running_var must be contiguous fp32 tensors on the device of feats")
    if train:
        out = _SparseNormFn.apply(_f32_grad(feats), _f32_grad(bn.weight), _f32_grad(bn.bias), _f32_grad(residual), [n], float(bn.eps),
                                  bool(relu), running, float(bn.momentum), bool(elu))
    else:
        out = _norm_forward(x, [n], float(bn.eps), w, b, res, relu, running, float(bn.momentum), bool(elu))[0]
    for t in running:                                        # written by the kernel: tell torch (the fold cache watches _version)
        torch.autograd.graph.increment_version(t)
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
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

    def forward(self, feats: torch.Tensor, kmap: KernelMap, scale=None, shift=None, residual=None, relu: bool = False,
                elu: bool = False) -> torch.Tensor:
        if (kmap.kernel_size, kmap.stride) != (self.kernel_size, self.stride):
            raise ValueError(f"SparseConv3d(kernel_size={self.kernel_size}, stride={self.stride}) got a kernel map of "
                             f"kernel_size={kmap.kernel_size}, stride={kmap.stride}")
        return sparse_conv3d(feats, kmap, self.kernel, self.bias, scale, shift, residual, relu, differentiable=self.differentiable, elu=elu)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, bias={self.bias is not None}"


class SparseInstanceNorm(nn.Module):
    """``ME.MinkowskiInstanceNorm(num_features)``: ``weight (1, C)`` ones and ``bias (1, C)`` zeros, ME's names and shapes.
    ``forward(feats, scene_rows, relu=False)`` = ``sparse_instance_norm``."""

    def __init__(self, num_features: int, differentiable: bool = False):
        super().__init__()
        self.num_features, self.differentiable = int(num_features), bool(differentiable)
        self.weight = nn.Parameter(torch.ones(1, self.num_features))
        self.bias = nn.Parameter(torch.zeros(1, self.num_features))

    def forward(self, feats: torch.Tensor, scene_rows: Sequence[int], relu: bool = False) -> torch.Tensor:
        return sparse_instance_norm(feats, scene_rows, self.weight, self.bias, relu, differentiable=self.differentiable)

    def extra_repr(self) -> str:
        return f"{self.num_features}"


class SparseBatchNorm(nn.Module):
    """``ME.MinkowskiBatchNorm(num_features, eps, momentum)``: a child ``bn = nn.BatchNorm1d`` as in ME, so the keys are ``bn.weight``,
    ``bn.bias``, ``bn.running_mean``, ``bn.running_var``, ``bn.num_batches_tracked``.  ``forward(feats, residual=None, relu=False, elu=False)`` =
    ``sparse_batch_norm``."""

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: float = 0.1, differentiable: bool = False):
        super().__init__()
        self.differentiable = bool(differentiable)
        self.bn = nn.BatchNorm1d(int(num_features), eps=eps, momentum=momentum)

    def forward(self, feats: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = False, elu: bool = False) -> torch.Tensor:
        return sparse_batch_norm(feats, self.bn, residual, relu, differentiable=self.differentiable, elu=elu)
