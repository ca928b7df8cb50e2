"""What the geometry-edge tests share (tests/test_geometry_edges_host.py, tests/test_gpu_geometry_edges.py): references of the
geometric front end written from the operations' definitions -- not from the kernels' fp32 steps -- and inputs that sit ON the
decisions these operators take.  A plain module: no tests, no marks.

``ref_point_sample``  batch_point_sample in float64 torch on the CPU (docstring of oracle.point_sample): project, clamp
                      the depth at 1e-3, scale -> crop -> flip, normalise by the padded size, F.grid_sample(align_corners=True,
                      zeros), sum ALL views, divide by the number of valid views, zero rows where none is valid.  Differentiable
                      with respect to the feature maps (autograd, double).
``ref_voxelize``      floor(p / voxel_size) as torch forms it in fp32 on the CPU (DET:388-397), the first point of every voxel in
                      (scene, point) order, rows in that order.
the lattice           points, maps and cameras on which every fp32 step of the sampling is exact, so that a float64 evaluation takes
                      the same decisions and float32(reference) is the only right answer, bit for bit."""
import functools

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------------------------ point sampling
def ref_point_sample(points, feats, proj, *, scale=(1.0, 1.0), crop=(0.0, 0.0), flip=False, ori_w=0.0, pad_hw=(480.0, 640.0),
                     bilinear=False, pre=None, geometry=False):
    """(out (N,C) float64 tensor, nvalid (N) int64 array[, geometry dict]).  points (N,3) finite; feats (V,C,H,W) array or tensor (a
    tensor that requires grad keeps its graph); proj (V,4,4); pre: a (3,4) affine applied to the points first."""
    p = torch.as_tensor(np.asarray(points, np.float64))
    f = feats if isinstance(feats, torch.Tensor) else torch.as_tensor(np.asarray(feats))
    f = f.double()
    P = torch.as_tensor(np.asarray(proj, np.float64))
    if pre is not None:
        A = torch.as_tensor(np.asarray(pre, np.float64)).reshape(3, 4)
        p = p @ A[:, :3].T + A[:, 3]
    V, _, H, W = f.shape
    N = p.shape[0]
    pad_h, pad_w = float(pad_hw[0]), float(pad_hw[1])
    q = torch.einsum("vrk,nk->vnr", P[:, :3, :3], p) + P[:, None, :3, 3]              # (V,N,3)
    depth = q[..., 2]
    z = depth.clamp(min=1e-3)
    cx = q[..., 0] / z * float(scale[0]) - float(crop[0])
    cy = q[..., 1] / z * float(scale[1]) - float(crop[1])
    if flip:
        cx = float(ori_w) - cx
    grid = torch.stack([cx / pad_w * 2 - 1, cy / pad_h * 2 - 1], -1).view(V, 1, N, 2)
    samp = F.grid_sample(f, grid, mode="bilinear" if bilinear else "nearest", padding_mode="zeros", align_corners=True)
    valid = (cx < pad_w) & (cx > 0) & (cy < pad_h) & (cy > 0) & (depth > 0)
    nvalid = valid.sum(0)
    out = samp[:, :, 0].sum(0).T / nvalid.clamp(min=1)[:, None]
    out = torch.where((nvalid > 0)[:, None], out, torch.zeros_like(out))          # +0.0, as the definition's `out[~valid] = 0`
    if not geometry:
        return out, nvalid.numpy()
    geo = dict(cx=cx.numpy(), cy=cy.numpy(), depth=depth.numpy(), ix=(cx / pad_w * (W - 1)).numpy(), iy=(cy / pad_h * (H - 1)).numpy(),
               valid=valid.numpy())
    return out, nvalid.numpy(), geo


def ref_point_sample_grad(points, feats, proj, dout, **kw):
    """(out float64 (N,C), nvalid, dfeats float64 (V,C,H,W)): autograd through ``ref_point_sample``, in double."""
    f = torch.as_tensor(np.asarray(feats, np.float64)).requires_grad_()
    out, nvalid = ref_point_sample(points, f, proj, **kw)
    out.backward(torch.as_tensor(np.asarray(dout, np.float64)))
    return out.detach().numpy(), nvalid, f.grad.numpy()


# ------------------------------------------------------------------------------------------------------------------ voxelisation
def ref_voxelize(outs, voxel_size):
    """coords (Nv,4) int32, feats (Nv,3) fp32, per-scene inverse maps (int32), rep (Nv) = flat index (scene, point) of the point
    each row keeps, counted over the concatenated scenes.  The voxel is ``torch.floor(p / voxel_size).int()`` on the CPU in fp32."""
    coords, feats, inverse, rep = [], [], [], []
    seen = {}
    base = 0
    for b, p in enumerate(outs):
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        v = torch.floor(torch.from_numpy(p) / voxel_size).int().numpy()
        inv = np.empty(len(p), np.int32)
        for i, key in enumerate(map(tuple, v.tolist())):
            row = seen.get((b,) + key)
            if row is None:
                row = seen[(b,) + key] = len(coords)
                coords.append((b,) + key)
                feats.append(p[i])
                rep.append(base + i)
            inv[i] = row
        inverse.append(inv)
        base += len(p)
    return (np.asarray(coords, np.int32).reshape(-1, 4), np.asarray(feats, np.float32).reshape(-1, 3), inverse,
            np.asarray(rep, np.int64))


VOXEL_SIZES = (0.01, 0.02, 0.05, 0.25)
BOUNDARY_K = np.arange(-3000, 3000)


def boundary_values(voxel_size):
    """fl(k * voxel_size) for k in [-3000, 3000) -- the positions the project itself emits for a level's rows -- and the fp32
    neighbour to either side; then -0.0, the smallest negative subnormal (voxel -1) and the smallest positive one (voxel 0)."""
    c = BOUNDARY_K.astype(np.float32) * np.float32(voxel_size)
    tiny = np.float32(1e-45)
    return np.concatenate([c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf)),
                           np.array([-0.0, -tiny, tiny], np.float32)]).astype(np.float32)


def floor_misses(voxel_size):
    """How many k in [-3000, 3000) have floor(fl(k * vs) / vs) != k in fp32 (the division, not a reciprocal)."""
    c = BOUNDARY_K.astype(np.float32) * np.float32(voxel_size)
    return int((np.floor(c / np.float32(voxel_size)).astype(np.int64) != BOUNDARY_K).sum())


def boundary_cloud(voxel_size):
    """The boundary values as one scene's points (n,3): the values in a fixed shuffle, three to a point."""
    v = boundary_values(voxel_size)
    v = v[np.random.default_rng(17).permutation(len(v))]
    return np.ascontiguousarray(v[:len(v) // 3 * 3].reshape(-1, 3)), v


# ------------------------------------------------------------------------------------------------------------------ the exact lattice
LAT_H, LAT_W, LAT_PAD = 9, 17, (32.0, 64.0)                       # ix = cx / 4, iy = cy / 4
LAT_X = (-2.5, -2.0, -1.0, -0.0, 0.0, 1.0, 2.0, 6.0, 10.0, 30.0, 62.0, 63.0, 64.0, 65.0, 66.0, 66.5)
LAT_Y = (-2.0, 0.0, 2.0, 6.0, 14.0, 30.0, 32.0, 34.0)
LAT_Z = (0.5, 1.0, 2.0)
LAT_PRE = np.array([[0, 1, 0, 0.25], [0, 0, 1, -0.5], [1, 0, 0, 0.75]], np.float32)      # p' = (y, z, x) + t
LAT_CONFIGS = {
    "plain": dict(scale=(1.0, 1.0), crop=(0.0, 0.0), flip=False, ori_w=64.0, pre=False),
    "flip": dict(scale=(1.0, 1.0), crop=(0.0, 0.0), flip=True, ori_w=64.0, pre=False),
    "aug": dict(scale=(0.5, 2.0), crop=(2.0, -4.0), flip=True, ori_w=64.0, pre=False),
    "pre": dict(scale=(1.0, 1.0), crop=(0.0, 0.0), flip=False, ori_w=64.0, pre=True),
}


def lattice_points():
    """(384,3) fp32: (x z, y z, z) over LAT_X x LAT_Y x LAT_Z; every product is exact."""
    x, y, z = np.meshgrid(np.array(LAT_X, np.float32), np.array(LAT_Y, np.float32), np.array(LAT_Z, np.float32), indexing="ij")
    return np.stack([x * z, y * z, z], -1).reshape(-1, 3).astype(np.float32)


def lattice_shifts(V):
    """Whole-pixel shifts (multiples of 4 image units) per view: three fixed ones, then a pattern that moves the lattice partly off
    the map."""
    s = [(0, 0), (4, -4), (-8, 4)]
    for v in range(3, V):
        s.append((4 * ((7 * v) % 23 - 11), 4 * ((5 * v) % 9 - 4)))
    return s[:V]


def shift_proj(shifts):
    """(V,4,4): the identity plus a shift of the image plane, q = (x + sx z, y + sy z, z)."""
    P = np.tile(np.eye(4, dtype=np.float32), (len(shifts), 1, 1))
    for v, (sx, sy) in enumerate(shifts):
        P[v, 0, 2], P[v, 1, 2] = sx, sy
    return P


def undo_pre(points, pre=LAT_PRE):
    """The points whose image under the permuting pre-transform is ``points`` (exact: a permutation and dyadic shifts)."""
    A = np.asarray(pre, np.float32).reshape(3, 4)
    return ((points - A[:, 3]) @ A[:, :3]).astype(np.float32)


def lattice_case(name, V=3):
    """points, proj, keyword arguments of ``ref_point_sample`` / ``oracle.point_sample`` (``pre`` separately) for one configuration."""
    cfg = LAT_CONFIGS[name]
    pts = lattice_points()
    pre = LAT_PRE if cfg["pre"] else None
    if pre is not None:
        pts = undo_pre(pts)
    kw = dict(scale=cfg["scale"], crop=cfg["crop"], flip=cfg["flip"], ori_w=cfg["ori_w"], pad_hw=LAT_PAD)
    return pts, shift_proj(lattice_shifts(V)), kw, pre


def apply_pre32(points, pre):
    """The pre-transform in fp32 (exact on the lattice), for restatements that take no ``pre``."""
    if pre is None:
        return points
    A = np.asarray(pre, np.float32).reshape(3, 4)
    return (points.astype(np.float32) @ A[:, :3].T + A[:, 3]).astype(np.float32)


def integer_maps(V, C, H=LAT_H, W=LAT_W, seed=0):
    """(V,C,H,W) fp32 of non-zero integers in [-8, 8]: exact in fp32, bf16 and fp16."""
    f = np.random.default_rng(seed).integers(-8, 9, (V, C, H, W)).astype(np.float32)
    f[f == 0] = 1.0
    return f


def integer_dout(N, C, seed=1):
    return np.random.default_rng(seed).integers(-8, 9, (N, C)).astype(np.float32)


def lattice_classes(name="plain", V=3):
    """Counts of the decisions the lattice is there for, from a float64 evaluation of one configuration (nearest)."""
    pts, proj, kw, pre = lattice_case(name, V)
    _, nvalid, g = ref_point_sample(pts, np.zeros((V, 1, LAT_H, LAT_W)), proj, pre=pre, geometry=True, **kw)
    ix, iy, cx, valid = g["ix"], g["iy"], g["cx"], g["valid"]
    tie = (np.abs(ix - np.floor(ix) - 0.5) == 0) & (ix > -1) & (ix < LAT_W)
    inb = (np.rint(ix) >= 0) & (np.rint(ix) <= LAT_W - 1) & (np.rint(iy) >= 0) & (np.rint(iy) <= LAT_H - 1)
    others = nvalid[None, :] - valid
    return dict(tie_even_down=int((tie & (np.floor(ix) % 2 == 0)).sum()), tie_even_up=int((tie & (np.floor(ix) % 2 == 1)).sum()),
                ix_minus_half=int(((ix == -0.5) & inb).sum()), ix_top_half=int(((ix == LAT_W - 0.5) & inb).sum()),
                cx_zero_other_valid=int(((cx == 0) & inb & (others > 0)).sum()),
                cx_pad_other_valid=int(((cx == LAT_PAD[1]) & inb & (others > 0)).sum()),
                sampled_not_valid=int((inb & ~valid & (others > 0)).sum()), one_outside=int((np.rint(ix) == LAT_W).sum()),
                none_valid=int((nvalid == 0).sum()), nvalid_hist=np.bincount(nvalid, minlength=V + 1).tolist())


# ------------------------------------------------------------------------------------------------------------------ the generic case
def generic_scene(seed, N=2000, V=3):
    """The non-dyadic camera set of tests/test_gpu_point_sample.py (V cameras on a circle), N random points."""
    rng = np.random.default_rng(seed)
    H, W = 17, 23
    proj = np.zeros((V, 4, 4), np.float32)
    for v in range(V):
        ang = 2 * np.pi * v / V
        ext = np.eye(4)
        ext[:3, :3] = [[np.cos(ang), 0, -np.sin(ang)], [0, 1, 0], [np.sin(ang), 0, np.cos(ang)]]
        ext[:3, 3] = [0.1 * v - 1.0, 0.2, 3.0]
        K = np.eye(4); K[0, 0] = K[1, 1] = 300.0; K[0, 2] = 320.0; K[1, 2] = 240.0
        proj[v] = (K @ ext).astype(np.float32)
    pts = ((rng.random((N, 3)) - 0.5) * 14).astype(np.float32)
    return rng, H, W, pts, proj


GENERIC_KW = dict(scale=(0.95, 1.05), crop=(3.0, 5.0), flip=True, ori_w=640.0, pad_hw=(480.0, 640.0))
GENERIC_SEED = 3


def restated_pixels32(points, proj, H, W, *, scale, crop, flip, ori_w, pad_hw):
    """(fx, fy) (V,N) fp32: the pixel coordinates as oracle.point_sample (= ps_project) rounds them, step by step."""
    from oracle.oracle import _f32, _fma32
    p, P = _f32(points), _f32(proj)
    N = len(p)
    one, two = np.float32(1), np.float32(2)
    fxs, fys = [], []
    with np.errstate(all="ignore"):
        for v in range(len(P)):
            q = []
            for r in range(3):
                t = p[:, 0] * P[v, r, 0]
                t = _fma32(p[:, 1], np.full(N, P[v, r, 1], np.float32), t)
                t = _fma32(p[:, 2], np.full(N, P[v, r, 2], np.float32), t)
                q.append(t + P[v, r, 3])
            z = np.maximum(q[2], np.float32(1e-3))
            cx = (q[0] / z) * np.float32(scale[0]) - np.float32(crop[0])
            cy = (q[1] / z) * np.float32(scale[1]) - np.float32(crop[1])
            if flip:
                cx = np.float32(ori_w) - cx
            fxs.append(((cx / np.float32(pad_hw[1]) * two - one + one) / two) * np.float32(W - 1))
            fys.append(((cy / np.float32(pad_hw[0]) * two - one + one) / two) * np.float32(H - 1))
    return np.stack(fxs), np.stack(fys)


@functools.lru_cache(maxsize=None)
def generic_margin():
    """(margin, largest |ix32 - ix64|, share of in-map pairs within 1e-3 px of a half pixel), in pixels: the margin of the generic
    case is 4 x the largest difference between the fp32 restatement's pixel coordinate and the float64 reference's over the in-map
    (point, view) pairs of the 50-view scene of tests/test_gpu_point_sample.py.  Measured on the CPU, never on the device."""
    _, H, W, pts, proj = generic_scene(50, N=5000, V=50)
    fx, fy = restated_pixels32(pts, proj, H, W, **GENERIC_KW)
    _, _, g = ref_point_sample(pts, np.zeros((50, 1, H, W)), proj, geometry=True, **GENERIC_KW)
    inmap = (g["ix"] > -1) & (g["ix"] < W) & (g["iy"] > -1) & (g["iy"] < H)
    worst = max(float(np.abs(fx - g["ix"])[inmap].max()), float(np.abs(fy - g["iy"])[inmap].max()))
    fr = g["ix"][inmap] - np.floor(g["ix"][inmap])
    return 4.0 * worst, worst, float((np.abs(fr - 0.5) < 1e-3).mean())


def generic_keep(geo, H, W, pad_hw, margin_px, bilinear=False):
    """Points none of whose views lies, in float64, within the margin of a decision: a half pixel (nearest) or a whole pixel
    (bilinear: where the neighbours change), the image border (valid test, in pixels of the map), depth 0 and the depth clamp."""
    ix, iy, cx, cy, depth = geo["ix"], geo["iy"], geo["cx"], geo["cy"], geo["depth"]
    keep = np.ones(ix.shape[1], bool)
    for pix, size, c, hi in ((ix, W, cx, pad_hw[1]), (iy, H, cy, pad_hw[0])):
        near_map = (pix > -2) & (pix < size + 1)
        frac = pix - np.floor(pix)
        edge = np.minimum(frac, 1 - frac) if bilinear else np.abs(frac - 0.5)
        keep &= (~near_map | (edge > margin_px)).all(0)
        per_px = hi / (size - 1)                                          # image units per pixel of the map
        keep &= (np.abs(c) > margin_px * per_px).all(0) & (np.abs(c - hi) > margin_px * per_px).all(0)
    keep &= (np.abs(depth) > 1e-2).all(0)
    return keep
