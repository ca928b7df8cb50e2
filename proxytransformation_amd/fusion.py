"""Image feature -> point sampling on the GPU: the reference's ``batch_point_sample``
(embodiedscan/models/layers/fusion_layers/point_fusion.py:208-313) with the argument list its detector uses
(detectors/sparse_featfusion_grounder_preshape.py:428-444), executed by ``ptx_point_sample`` (csrc/pointsample.hip)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _abi
from ._doors import _stream

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _pair(v, dev):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    if isinstance(v, (int, float)):
        return float(v), float(v)
    return float(v[0]), float(v[1])


def reverse_3d_flow(img_meta: Optional[dict], coord_type: str = "DEPTH") -> Optional[torch.Tensor]:
    """``apply_3d_transformation(points, coord_type, img_meta, reverse=True)`` (point_fusion.py:20-107) as ONE (3,4) affine
    ``[A | t]`` (p' = A p + t), composed on the host in float64: the recorded ``transformation_3d_flow`` is undone back to
    front -- 'T': p - pcd_trans, 'S': p / pcd_scale_factor, 'R': p @ inverse(pcd_rotation), 'HF' / 'VF': the BEV flips of
    the coordinate type (DEPTH: x -> -x / y -> -y, depth_points.py:47-50; LIDAR: y -> -y / x -> -x, lidar_points.py:47-50;
    CAMERA: x -> -x / z -> -z, cam_points.py:47-50).  Returns
    ``None`` when nothing was recorded."""
    flow = list(img_meta.get("transformation_3d_flow", [])) if img_meta else []
    if not flow:
        return None
    import numpy as np
    A, t = np.eye(3), np.zeros(3)

    def host(x):
        return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64)
    rot = host(img_meta["pcd_rotation"]).reshape(3, 3) if "pcd_rotation" in img_meta else np.eye(3)
    scale = float(img_meta.get("pcd_scale_factor", 1.0))
    trans = host(img_meta["pcd_trans"]).reshape(3) if "pcd_trans" in img_meta else np.zeros(3)
    ct = coord_type.upper()
    if ct not in ("DEPTH", "LIDAR", "CAMERA"):
        raise ValueError(f"coord_type {coord_type!r}")
    for op in flow[::-1]:
        if op == "T":
            t = t - trans
        elif op == "S":
            A, t = A / scale, t / scale
        elif op == "R":                                  # row vectors: p @ inv(rot)  <=>  column vectors: inv(rot)^T p
            M = np.linalg.inv(rot).T
            A, t = M @ A, M @ t
        elif op in ("HF", "VF"):
            flipped = bool(img_meta.get("pcd_horizontal_flip" if op == "HF" else "pcd_vertical_flip", False))
            if flipped:
                # the axis each Points class negates (structures/points/depth_points.py:47-50, lidar_points.py:47-50,
                # cam_points.py:47-50): DEPTH x / y, LIDAR y / x, CAMERA x / z
                axis = {"DEPTH": (0, 1), "LIDAR": (1, 0), "CAMERA": (0, 2)}[ct][op == "VF"]
                F = np.eye(3)
                F[axis, axis] = -1.0
                A, t = F @ A, F @ t
        else:
            raise AssertionError(f"This 3D data transformation op ({op}) is not supported")     # point_fusion.py:101-102
    return torch.from_numpy(np.concatenate([A, t[:, None]], 1).astype(np.float32))


def batch_point_sample(img_meta: Optional[dict], img_features: torch.Tensor, points: torch.Tensor, proj_mat: torch.Tensor,
                       coord_type: str = "DEPTH", img_scale_factor=1.0, img_crop_offset=0.0, img_flip: bool = False,
                       img_pad_shape: Sequence[int] = (480, 640), img_shape: Sequence[int] = (480, 640),
                       aligned: bool = False, padding_mode: str = "zeros", align_corners: bool = True,
                       valid_flag: bool = True, pre_transform: Optional[torch.Tensor] = None,
                       prepared: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Same arguments as the reference function.  img_features (V,C,H,W) on the GPU (fp32 / bf16 / fp16), points (N,3)
    fp32, proj_mat (V,4,4) = intrinsic @ extrinsic.  Returns (N,C) fp32.

    ``aligned=False`` (the detector's call: nearest) and ``aligned=True`` (bilinear) are both HIP; zeros padding,
    align_corners and valid_flag as the detector passes them.  The reverse 3D augmentation of
    ``apply_3d_transformation`` (point_fusion.py:20-107) is composed from ``img_meta['transformation_3d_flow']``
    (``reverse_3d_flow``; the training pipeline's GlobalRotScaleTrans records 'R', 'S', 'T') unless an explicit
    ``pre_transform`` (3,4) is given.  ``prepared``: the workspace ``prepare_features(img_features)`` returned (the channels-last copy
    made earlier, e.g. on another stream): the call then only samples.

    Training: with grad mode on and ``img_features.requires_grad`` the result carries a ``grad_fn`` whose backward is HIP as well
    (``ptx_point_sample_bwd``: no float atomics, bitwise reproducible) and returns the gradient in the shape and dtype of
    ``img_features`` (with ``prepared=`` too: the gradient goes to the ``img_features`` argument).  Otherwise the call is the plain
    forward and the result has no ``grad_fn``.  The points stay detached: in the detector they are integer voxel coordinates times
    the voxel size, and a bilinear gradient with respect to them is out of scope."""
    if padding_mode != "zeros" or not align_corners or not valid_flag:
        raise NotImplementedError("HIP path: padding_mode='zeros', align_corners=True, valid_flag=True "
                                  "(the call at sparse_featfusion_grounder_preshape.py:428-444)")
    if pre_transform is None:
        pre_transform = reverse_3d_flow(img_meta, coord_type)
    if not (img_features.is_cuda and points.is_cuda and proj_mat.is_cuda):
        raise RuntimeError("batch_point_sample (HIP) needs GPU tensors: there is no CPU path")
    if img_features.dtype not in _DT:
        img_features = img_features.float()
    V, C, H, W = img_features.shape
    feats = img_features.contiguous()
    pts = points.detach().to(torch.float32).contiguous()
    proj = proj_mat.detach().to(torch.float32).contiguous()
    if proj.shape != (V, 4, 4) or pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError(f"expected points (N,3) and proj_mat ({V},4,4), got {tuple(pts.shape)}, {tuple(proj.shape)}")
    dev = pts.device
    sw, sh = _pair(img_scale_factor, dev)
    cw, ch = _pair(img_crop_offset, dev)
    pre = None if pre_transform is None else pre_transform.detach().to(device=dev, dtype=torch.float32).contiguous()
    scal = (sw, sh, cw, ch, 1 if img_flip else 0, float(img_shape[1]), float(img_pad_shape[0]), float(img_pad_shape[1]),
            1 if aligned else 0)
    if torch.is_grad_enabled() and feats.requires_grad:
        return _PointSampleFn.apply(feats, prepared, pts, proj, pre, scal)
    return _sample(feats, prepared, pts, proj, pre, scal, None)


def _sample(feats, prepared, pts, proj, pre, scal, valid_num):
    """The ``ptx_point_sample`` call of ``batch_point_sample``: arguments already checked and converted; ``scal`` = the image-transform
    scalars and the bilinear flag in the order of the C signature; valid_num (N) int32 or None."""
    V, C, H, W = feats.shape
    N = pts.shape[0]
    dev = pts.device
    out = torch.empty((N, C), dtype=torch.float32, device=dev)
    if N == 0:
        return out
    lib = _abi.lib()
    nbytes = lib.ptx_point_sample_workspace_bytes(V, C, H, W)
    if nbytes == 0:
        raise RuntimeError(f"unsupported feature shape {tuple(feats.shape)} (C <= 512)")
    if prepared is not None:
        if prepared.numel() < nbytes or prepared.device != dev:
            raise RuntimeError("prepared: not the workspace of prepare_features() for these feature maps")
        ws, feats_ptr = prepared, None
    else:
        ws, feats_ptr = torch.empty((nbytes,), dtype=torch.uint8, device=dev), feats.data_ptr()
    _abi.check(lib.ptx_point_sample(pts.data_ptr(), N, feats_ptr, _DT[feats.dtype], V, C, H, W, proj.data_ptr(),
                                    None if pre is None else pre.data_ptr(), *scal, out.data_ptr(),
                                    None if valid_num is None else valid_num.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _stream(dev)),
               "ptx_point_sample")
    return out


class _PointSampleFn(torch.autograd.Function):
    """``batch_point_sample`` as an autograd node: the gradient reaches the feature maps (``ptx_point_sample_bwd``), nothing else.
    The sampling is linear in the features, so the backward needs the geometry only: the points, the matrices, the pre-transform,
    the scalars and the forward's ``valid_num`` are saved -- not the feature maps."""

    @staticmethod
    def forward(ctx, feats, prepared, pts, proj, pre, scal):
        valid_num = torch.empty((pts.shape[0],), dtype=torch.int32, device=pts.device)
        out = _sample(feats, prepared, pts, proj, pre, scal, valid_num)
        ctx.save_for_backward(pts, proj, pre, valid_num)
        ctx.scal, ctx.feat_shape, ctx.feat_dtype = scal, tuple(feats.shape), feats.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        pts, proj, pre, valid_num = ctx.saved_tensors
        V, C, H, W = ctx.feat_shape
        N, dev = pts.shape[0], pts.device
        if N == 0:
            return torch.zeros(ctx.feat_shape, dtype=ctx.feat_dtype, device=dev), None, None, None, None, None
        dfeats = torch.empty(ctx.feat_shape, dtype=ctx.feat_dtype, device=dev)     # every element is written by the kernel
        dout = dout.to(torch.float32).contiguous()
        lib = _abi.lib()
        bilinear = ctx.scal[-1]
        nbytes = lib.ptx_point_sample_bwd_workspace_bytes(N, V, H, W, bilinear)
        if nbytes == 0:
            raise RuntimeError(f"point-sample backward: N={N} V={V} H={H} W={W} is outside the 32-bit index range")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _abi.check(lib.ptx_point_sample_bwd(pts.data_ptr(), N, dout.data_ptr(), valid_num.data_ptr(), V, C, H, W, proj.data_ptr(),
                                            None if pre is None else pre.data_ptr(), *ctx.scal, dfeats.data_ptr(),
                                            _DT[ctx.feat_dtype], ws.data_ptr(), ws.numel(),
                                            _stream(dev)), "ptx_point_sample_bwd")
        return dfeats, None, None, None, None, None


def prepare_features(img_features: torch.Tensor) -> torch.Tensor:
    """The channels-last copy of one sample's feature maps (V,C,H,W) that ``batch_point_sample`` gathers from, made on the CURRENT
    stream: returns the workspace to pass as ``prepared=``.  The detector knows the feature maps (2D backbone) long before it knows
    the points (neck + sparse backbone): ``pipeline.GroundingFeaturePrefix`` makes these copies on a side stream beside the ingest."""
    if not img_features.is_cuda:
        raise RuntimeError("prepare_features (HIP) needs GPU tensors: there is no CPU path")
    if img_features.dtype not in _DT:
        img_features = img_features.float()
    feats = img_features.contiguous()
    V, C, H, W = feats.shape
    lib = _abi.lib()
    nbytes = lib.ptx_point_sample_workspace_bytes(V, C, H, W)
    if nbytes == 0:
        raise RuntimeError(f"unsupported feature shape {tuple(feats.shape)} (C <= 512)")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=feats.device)
    _abi.check(lib.ptx_point_sample_prepare(feats.data_ptr(), _DT[feats.dtype], V, C, H, W, ws.data_ptr(), ws.numel(),
                                            _stream(feats.device)), "ptx_point_sample_prepare")
    return ws


def prepare_features_many(maps) -> list:
    """``prepare_features`` for a list of (V,C,H,W) feature maps with ONE allocation (the pipeline prepares scenes x levels maps at the
    start of a call: 24 allocations + calls were 0.3 ms of host time in front of the ingest).  Returns one workspace view per map."""
    lib = _abi.lib()
    maps = [m if m.dtype in _DT else m.float() for m in maps]
    maps = [m.contiguous() for m in maps]
    sizes = []
    for m in maps:
        if not m.is_cuda:
            raise RuntimeError("prepare_features (HIP) needs GPU tensors: there is no CPU path")
        V, C, H, W = m.shape
        n = lib.ptx_point_sample_workspace_bytes(V, C, H, W)
        if n == 0:
            raise RuntimeError(f"unsupported feature shape {tuple(m.shape)} (C <= 512)")
        sizes.append(n)                                   # multiples of 256 bytes
    dev = maps[0].device
    flat = torch.empty((sum(sizes),), dtype=torch.uint8, device=dev)
    views = list(flat.split_with_sizes(sizes))
    st = _stream(dev)
    for m, ws in zip(maps, views):
        V, C, H, W = m.shape
        _abi.check(lib.ptx_point_sample_prepare(m.data_ptr(), _DT[m.dtype], V, C, H, W, ws.data_ptr(), ws.numel(), st),
                   "ptx_point_sample_prepare")
    return views


# ---------------------------------------------------------------------------------------------------------------- level join
_LJ_WORDS = 32          # one scene's table, in floats (include/proxyt.h: ptx_level_join)


def image_transform_scalars(img_meta: Optional[dict], img_pad_shape: Sequence[int]) -> tuple:
    """``(scale_w, scale_h, crop_w, crop_h, flip, ori_w, pad_h, pad_w)`` of one sample, as the detector reads them off its ``img_meta``
    (DET:404-410, 440-441): what ``JoinTables`` takes per scene."""
    meta = img_meta or {}
    sw, sh = _pair(meta["scale_factor"][:2], None) if "scale_factor" in meta else (1.0, 1.0)
    cw, ch = _pair(meta.get("img_crop_offset", 0.0), None)
    shape = tuple(meta.get("img_shape", img_pad_shape))[:2]
    return (sw, sh, cw, ch, bool(meta.get("flip", False)), float(shape[1]), float(img_pad_shape[0]), float(img_pad_shape[1]))


class JoinTables:
    """What differs between the scenes of one ``join_level_features`` call -- projection matrices (V,4,4), the reverse 3D
    augmentation (3,4) or ``None``, the eight image-transform scalars ``(scale_w, scale_h, crop_w, crop_h, flip, ori_w, pad_h,
    pad_w)`` -- laid out as ``ptx_level_join`` reads it and brought to the device through ONE pinned staging copy (a ``.to(device)``
    from pageable memory would block the host behind everything queued on the stream).  The same tables serve every level of a
    call and its backward.  ``staging``: a dict the caller keeps between calls so that the pinned buffer is allocated once per
    stream.  ``proj[b]`` / ``pre[b]`` / ``scal[b]`` are the per-scene arguments of ``batch_point_sample``'s own launch (device views
    of the same upload), for the per-scene route."""

    def __init__(self, projs, pres, scalars, voxel_size: float, device, aligned: bool = False, staging: Optional[dict] = None):
        import numpy as np
        B = len(projs)
        if not (len(pres) == len(scalars) == B):
            raise ValueError(f"JoinTables: {B} projection stacks, {len(pres)} pre-transforms, {len(scalars)} scalar sets")
        projs = [np.ascontiguousarray(p, np.float32) for p in projs]
        V = projs[0].shape[0] if B and projs[0].ndim == 3 else 0
        for p in projs:
            if p.shape != (V, 4, 4):
                raise ValueError(f"JoinTables: every scene needs ({V},4,4) projection matrices (V is uniform per call), got {p.shape}")
        if not float(voxel_size) > 0.0:
            raise ValueError(f"JoinTables: voxel_size={voxel_size}")
        n = _abi.lib().ptx_level_join_table_floats(B, V)
        if n == 0:
            raise ValueError(f"JoinTables: B={B} (1..64), V={V} (>= 1)")
        host = np.zeros((n,), np.float32)                # the library's checks read this copy, in forward and backward
        for b in range(B):
            t = host[_LJ_WORDS * b:_LJ_WORDS * (b + 1)]
            if pres[b] is not None:
                pre = pres[b].detach().cpu().numpy() if isinstance(pres[b], torch.Tensor) else np.asarray(pres[b])
                t[0:12] = pre.astype(np.float32).reshape(12)
                t[12] = 1.0
            s = scalars[b]
            if len(s) != 8:
                raise ValueError("JoinTables: scalars = (scale_w, scale_h, crop_w, crop_h, flip, ori_w, pad_h, pad_w) per scene")
            t[13:21] = [float(s[0]), float(s[1]), float(s[2]), float(s[3]), 1.0 if s[4] else 0.0, float(s[5]), float(s[6]), float(s[7])]
            if not (t[19] > 0.0 and t[20] > 0.0):
                raise ValueError(f"JoinTables: scene {b}: pad_h={s[6]}, pad_w={s[7]}")
            host[_LJ_WORDS * B + b * V * 16:_LJ_WORDS * B + (b + 1) * V * 16] = projs[b].reshape(-1)
        device = torch.device(device)
        st = torch.cuda.current_stream(device)
        staging = {} if staging is None else staging
        stg = staging.get(st.cuda_stream)
        if stg is None or stg["host"].numel() < n:
            stg = staging[st.cuda_stream] = dict(host=torch.empty((n,), dtype=torch.float32).pin_memory(), done=None)
            stg["np"] = stg["host"].numpy()
        if stg["done"] is not None and not stg["done"].query():
            stg["done"].synchronize()                    # the previous call's copy out of the staging buffer (long done)
        stg["np"][:n] = host
        # this call's own device buffer: the join's autograd nodes keep it until their backward
        self.dev = torch.empty((n,), dtype=torch.float32, device=device)
        self.dev.copy_(stg["host"][:n], non_blocking=True)
        stg["done"] = torch.cuda.Event()
        stg["done"].record(st)
        self.host, self.B, self.V, self.voxel_size, self.aligned = host, B, V, float(voxel_size), bool(aligned)
        self.proj = [self.dev[_LJ_WORDS * B + b * V * 16:_LJ_WORDS * B + (b + 1) * V * 16].view(V, 4, 4) for b in range(B)]
        self.pre = [None if pres[b] is None else self.dev[_LJ_WORDS * b:_LJ_WORDS * b + 12].view(3, 4) for b in range(B)]
        self.scal = [tuple(float(x) for x in host[_LJ_WORDS * b + 13:_LJ_WORDS * b + 17]) + (int(host[_LJ_WORDS * b + 17] != 0),)
                     + tuple(float(x) for x in host[_LJ_WORDS * b + 18:_LJ_WORDS * b + 21]) + (1 if aligned else 0,) for b in range(B)]


def join_level_features(level, img_features_l: torch.Tensor, tables: JoinTables, prepared: Optional[Sequence[torch.Tensor]] = None
                        ) -> torch.Tensor:
    """DET:428-479 for one backbone level and all scenes in ONE launch (``ptx_level_join``, csrc/level_join.hip): every row of
    ``level`` (a ``SparseLevel``: ``feats (n,Cb)`` fp32, ``coords (n,4)`` int32 with the scene in column 0, ``scene_rows``) gets the
    image features of ``img_features_l (B,V,Ci,H,W)`` sampled at ``coords[:,1:4] * tables.voxel_size`` appended.  Returns
    ``(n, Cb+Ci)`` fp32, bit for bit ``torch.cat([level.feats, torch.cat([batch_point_sample(...) per scene])], 1)``.

    ``prepared``: the B workspaces ``prepare_features_many([img_features_l[b] for b in range(B)])`` returned (made earlier, e.g. on a
    side stream), read in place; ``None``: made here.  Cb, Ci: multiples of 64 up to 512; a scene may have no row; ``n = 0`` launches
    nothing.  With grad mode on and ``level.feats`` or ``img_features_l`` requiring grad the result is ONE autograd node whose backward
    is one library call (``ptx_level_join_bwd``: no float atomics, bitwise reproducible); otherwise it is the plain forward."""
    feats, coords, ends = level.feats, level.coords, [int(e) for e in level.scene_rows]
    if not (isinstance(feats, torch.Tensor) and feats.is_cuda and coords.is_cuda and img_features_l.is_cuda):
        raise RuntimeError("join_level_features (HIP) needs GPU tensors: there is no CPU path")
    if img_features_l.dim() != 5:
        raise ValueError(f"img_features_l: (B,V,C,H,W) expected, got {tuple(img_features_l.shape)}")
    if img_features_l.dtype not in _DT:
        img_features_l = img_features_l.float()
    img = img_features_l.contiguous()
    B, V, Ci, H, W = img.shape
    n = feats.shape[0]
    if feats.dim() != 2 or feats.dtype != torch.float32 or coords.dtype != torch.int32 or tuple(coords.shape) != (n, 4):
        raise ValueError(f"level: feats (n,Cb) fp32 and coords (n,4) int32 expected, got {tuple(feats.shape)} {feats.dtype}, "
                         f"{tuple(coords.shape)} {coords.dtype}")
    Cb = feats.shape[1]
    for name, c in (("Cb", Cb), ("Ci", Ci)):
        if c < 64 or c > 512 or c % 64:
            raise ValueError(f"join_level_features: {name}={c}: a multiple of 64 up to 512")
    if B != tables.B or V != tables.V:
        raise ValueError(f"join_level_features: img_features_l has B={B}, V={V}; the tables were built for B={tables.B}, V={tables.V}")
    if len(ends) != B or any(e < s for s, e in zip([0] + ends[:-1], ends)) or ends[-1] != n:
        raise ValueError(f"level.scene_rows={ends}: {B} ascending row ends, the last one n={n}")
    dev = feats.device
    if tables.dev.device != dev or img.device != dev:
        raise ValueError("join_level_features: level, img_features_l and tables live on different devices")
    if prepared is not None:
        need = _abi.lib().ptx_point_sample_workspace_bytes(V, Ci, H, W)
        if len(prepared) != B or any(p.numel() < need or p.device != dev for p in prepared):
            raise RuntimeError("prepared: not the workspaces of prepare_features_many() for these feature maps")
    elif n > 0:
        prepared = prepare_features_many([img[b] for b in range(B)])
    coords = coords.contiguous()
    if torch.is_grad_enabled() and (feats.requires_grad or img.requires_grad):
        return _LevelJoinFn.apply(feats, img, coords, ends, tables, prepared)
    return _join(feats.detach().contiguous(), img, coords, tables, prepared, None)


def join_level_features_per_scene(level, img_features_l: torch.Tensor, tables: JoinTables, prepared: Optional[Sequence[torch.Tensor]] = None
                                  ) -> torch.Tensor:
    """The route ``join_level_features`` replaces, DET:428-479 literally and with the same arguments: one ``batch_point_sample`` launch per
    scene, a ``torch.cat`` over the scenes and one over the channels.  Same bits, forward and backward; kept for comparison and timing
    (``GroundingDetector(fused_join=False)``, ``tools/detector_time.py``, the tests)."""
    img = img_features_l if img_features_l.dtype in _DT else img_features_l.float()
    lo = [0] + [int(e) for e in level.scene_rows[:-1]]
    parts = []
    for b, (s, e) in enumerate(zip(lo, level.scene_rows)):
        pts = level.coords[s:e, 1:4].to(torch.float32) * tables.voxel_size
        feats = img[b].contiguous()
        prep = None if prepared is None else prepared[b]
        if torch.is_grad_enabled() and feats.requires_grad:
            parts.append(_PointSampleFn.apply(feats, prep, pts, tables.proj[b], tables.pre[b], tables.scal[b]))
        else:
            parts.append(_sample(feats, prep, pts, tables.proj[b], tables.pre[b], tables.scal[b], None))
    return torch.cat([level.feats, torch.cat(parts)], 1)


def _join(feats, img, coords, tables, prepared, valid_num):
    """The ``ptx_level_join`` call: arguments already checked."""
    import ctypes
    B, V, Ci, H, W = img.shape
    n, Cb = feats.shape
    out = torch.empty((n, Cb + Ci), dtype=torch.float32, device=feats.device)
    if n == 0:
        return out
    if feats.data_ptr() % 16:
        feats = feats.clone()
    ptrs = (ctypes.c_void_p * B)(*[p.data_ptr() for p in prepared])
    _abi.check(_abi.lib().ptx_level_join(coords.data_ptr(), n, feats.data_ptr(), Cb, ptrs, tables.host.ctypes.data, tables.dev.data_ptr(),
                                         B, V, Ci, H, W, tables.voxel_size, 1 if tables.aligned else 0, out.data_ptr(),
                                         None if valid_num is None else valid_num.data_ptr(),
                                         _stream(feats.device)), "ptx_level_join")
    return out


class _LevelJoinFn(torch.autograd.Function):
    """``join_level_features`` as ONE autograd node.  Both halves of the output are linear in their inputs and the sampling's
    backward needs the geometry only, so the coordinates, the tables and the forward's ``valid_num`` are kept -- no feature maps."""

    @staticmethod
    def forward(ctx, feats, img, coords, ends, tables, prepared):
        valid_num = torch.empty((feats.shape[0],), dtype=torch.int32, device=feats.device)
        out = _join(feats.detach().contiguous(), img, coords, tables, prepared, valid_num)
        ctx.save_for_backward(coords, valid_num)
        ctx.tables, ctx.ends, ctx.img_shape, ctx.img_dtype, ctx.Cb = tables, ends, tuple(img.shape), img.dtype, feats.shape[1]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        import ctypes
        coords, valid_num = ctx.saved_tensors
        tables, ends, Cb = ctx.tables, ctx.ends, ctx.Cb
        B, V, Ci, H, W = ctx.img_shape
        n, dev = coords.shape[0], coords.device
        want_f, want_i = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dfeats = torch.empty((n, Cb), dtype=torch.float32, device=dev) if want_f else None
        if n == 0:
            dimg = torch.zeros(ctx.img_shape, dtype=ctx.img_dtype, device=dev) if want_i else None
            return dfeats, dimg, None, None, None, None
        dimg = torch.empty(ctx.img_shape, dtype=ctx.img_dtype, device=dev) if want_i else None   # every element is written
        g = g.to(torch.float32).contiguous()
        if g.data_ptr() % 16:
            g = g.clone()
        lib = _abi.lib()
        bil = 1 if tables.aligned else 0
        ws = None
        if want_i:
            rows = max(e - s for s, e in zip([0] + ends[:-1], ends))
            nbytes = lib.ptx_level_join_bwd_workspace_bytes(rows, V, H, W, bil)
            if nbytes == 0:
                raise RuntimeError(f"level-join backward: rows={rows} V={V} H={H} W={W} is outside the 32-bit index range")
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _abi.check(lib.ptx_level_join_bwd(coords.data_ptr(), n, (ctypes.c_int32 * B)(*ends), g.data_ptr(), Cb, valid_num.data_ptr(),
                                          tables.host.ctypes.data, tables.dev.data_ptr(), B, V, Ci, H, W, tables.voxel_size, bil,
                                          None if dfeats is None else dfeats.data_ptr(), None if dimg is None else dimg.data_ptr(),
                                          _DT[ctx.img_dtype], None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(),
                                          _stream(dev)), "ptx_level_join_bwd")
        return dfeats, dimg, None, None, None, None
