"""Backward of batch_point_sample with respect to the feature maps (``ptx_point_sample_bwd`` behind the autograd node of
``fusion.batch_point_sample``): against the gradient the reference's own function gives (tests/golden/g7_point_sample_grad.npz,
tests/golden/gen_point_sample_grad.py), against columns of the forward operator (adjoint identity, no capture involved), and its
structural promises -- exact zeros, one rounding on 16-bit stores, bitwise reproducibility, unchanged no-grad path.

The bound of the value checks is derived, not measured.  An element of the gradient is a sum of k terms w * (dout / valid_num):
two roundings per term, k - 1 per sum, so in fp32 (unit roundoff 2^-24) any summation order stays within (k + 1) 2^-24 sum|terms|
of the exact value; two such results (ours and the reference's, whatever its order) are within (k + 1) 2^-23 sum|terms| of each
other.  The tests allow (k + 4) 2^-23 sum|terms|, with k and sum|terms| from a float64 pass over the same index."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import load_golden

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def hit_index(points, proj, H, W, *, scale=(1.0, 1.0), crop=(0.0, 0.0), flip=False, ori_w=0.0, pad_hw=(480.0, 640.0),
              bilinear=False, pre=None):
    """The (point, view, pixel, weight) entries of the sampling operator, from the geometry alone, with the fp32 steps of
    oracle.point_sample (= k_point_sample).  Returns n, d = v * H * W + y * W + x, w (fp32) -- one entry per in-bounds sample
    (per in-bounds neighbour when bilinear) -- and nvalid (N)."""
    from oracle.oracle import _f32, _fma32
    p, P = _f32(points), _f32(proj)
    N, V = p.shape[0], P.shape[0]
    if pre is not None:
        A = _f32(pre).reshape(3, 4)
        full = lambda s: np.full(N, s, np.float32)
        p = np.stack([_fma32(full(A[r, 2]), p[:, 2], _fma32(full(A[r, 1]), p[:, 1], full(A[r, 0]) * p[:, 0])) + A[r, 3]
                      for r in range(3)], 1)
    pad_h, pad_w = np.float32(pad_hw[0]), np.float32(pad_hw[1])
    one, two = np.float32(1), np.float32(2)
    ns, ds, ws = [], [], []
    nvalid = np.zeros(N, np.int64)
    idx = np.arange(N)
    with np.errstate(all="ignore"):
        for v in range(V):
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
            fx = ((cx / pad_w * two - one + one) / two) * np.float32(W - 1)
            fy = ((cy / pad_h * two - one + one) / two) * np.float32(H - 1)
            if not bilinear:
                ix, iy = np.rint(fx), np.rint(fy)
                ok = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
                ns.append(idx[ok]); ws.append(np.ones(ok.sum(), np.float32))
                ds.append(v * H * W + iy[ok].astype(np.int64) * W + ix[ok].astype(np.int64))
            else:
                x0, y0 = np.floor(fx), np.floor(fy)
                wx1, wy1 = fx - x0, fy - y0
                wx0, wy0 = one - wx1, one - wy1
                for dx, dy, w in ((0, 0, wx0 * wy0), (1, 0, wx1 * wy0), (0, 1, wx0 * wy1), (1, 1, wx1 * wy1)):
                    xx, yy = x0 + dx, y0 + dy
                    ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
                    ns.append(idx[ok]); ws.append(w[ok].astype(np.float32))
                    ds.append(v * H * W + yy[ok].astype(np.int64) * W + xx[ok].astype(np.int64))
            nvalid += (cx < pad_w) & (cx > 0) & (cy < pad_h) & (cy > 0) & (q[2] > 0)
    return np.concatenate(ns), np.concatenate(ds), np.concatenate(ws), nvalid


def bound_terms(n, d, w, nvalid, dout, shape):
    """float64 pass over the index: k (V,1,H,W) = contributions per pixel, S (V,C,H,W) = sum of |w * dout / valid_num|, and the
    exact gradient E (V,C,H,W)."""
    V, C, H, W = shape
    keep = nvalid[n] > 0
    n, d, w = n[keep], d[keep], w[keep].astype(np.float64)
    k = np.bincount(d, minlength=V * H * W).astype(np.float64)
    coef = (w / nvalid[n])[:, None]
    g = dout.astype(np.float64)[n]
    S = np.zeros((V * H * W, C))
    E = np.zeros((V * H * W, C))
    np.add.at(S, d, coef * np.abs(g))
    np.add.at(E, d, coef * g)
    to = lambda a: np.ascontiguousarray(a.reshape(V, H, W, -1).transpose(0, 3, 1, 2))
    return to(k[:, None]), to(S), to(E)


def check_bound(got, want, k, S, what, require_max_k=None):
    """|got - want| <= (k + 4) 2^-23 sum|terms| for EVERY element; prints the worst ratio before asserting.  ``require_max_k``: the
    longest list of the case must reach it (a case that is about long lists fails when its geometry does not produce them)."""
    if require_max_k is not None:
        assert int(k.max()) >= require_max_k, f"{what}: longest list {int(k.max())} < {require_max_k}"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    lim = (k + 4.0) * EPS * S
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"{what}: worst |err| / bound = {ratio.max():.3g}, max |err| = {err.max():.3g}, elements {err.size}, "
          f"max k = {int(k.max())}")
    assert (err <= lim).all(), f"{what}: {(err > lim).sum()} of {err.size} elements outside the bound, worst ratio {ratio.max():.3g}"


def _grad(feats, pts, proj, dout, **kw):
    from proxytransformation_amd.fusion import batch_point_sample
    f = feats.detach().clone().requires_grad_()
    out = batch_point_sample(kw.pop("meta", None), f, pts, proj, "DEPTH", **kw)
    assert out.grad_fn is not None
    out.backward(dout)
    assert f.grad.shape == f.shape and f.grad.dtype == f.dtype
    return out.detach(), f.grad


@pytest.mark.parametrize("case", ["plain", "aug", "flow3d", "bilinear"])
def test_feature_gradient_matches_the_reference_capture(case):
    """The four g5 cases, gradient of the reference's own batch_point_sample (first 8 channels of g5's feature maps: the
    capture's size), every element inside the derived bound."""
    from proxytransformation_amd.fusion import reverse_3d_flow
    from tests.test_oracle_golden import _meta3d
    g5, g7 = load_golden("g5_point_sample"), load_golden("g7_point_sample_grad")
    dout, want = g7[f"{case}_dout"], g7[f"{case}_dfeats"]
    CH = dout.shape[1]
    feats = np.ascontiguousarray(g5["feats"][:, :CH])
    V, _, H, W = feats.shape
    sx, sy, cw, ch, flip, ori_w = [float(x) for x in g5[f"{case}_cfg"]]
    meta = _meta3d(g5) if case == "flow3d" else {}
    pad = (int(g5["pad"][0]), int(g5["pad"][1]))
    _, got = _grad(_t(feats), _t(g5[f"{case}_points"]), _t(g5["proj"]), _t(dout), meta=dict(meta),
                   img_scale_factor=torch.tensor([sx, sy]), img_crop_offset=torch.tensor([cw, ch]), img_flip=bool(flip),
                   img_pad_shape=pad, img_shape=(600, int(ori_w)), aligned=case == "bilinear")
    pre = reverse_3d_flow(meta).numpy() if meta else None
    n, d, w, nvalid = hit_index(g5[f"{case}_points"], g5["proj"], H, W, scale=(sx, sy), crop=(cw, ch), flip=bool(flip),
                                ori_w=ori_w, pad_hw=(float(pad[0]), float(pad[1])), bilinear=case == "bilinear", pre=pre)
    k, S, _ = bound_terms(n, d, w, nvalid, dout, feats.shape)
    assert want.shape == feats.shape and k.max() >= 2
    check_bound(got.cpu().numpy(), want, k, S, f"capture/{case}")


def _restatement_scene(V, N=5000):
    """The cameras and the point cloud of test_gpu_point_sample.py::test_point_sample_matches_the_restatement: points behind
    the cameras and outside every image."""
    rng = np.random.default_rng(V)
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


KW = dict(img_scale_factor=(0.95, 1.05), img_crop_offset=(3.0, 5.0), img_flip=True, img_pad_shape=(480, 640),
          img_shape=(480, 640))
IKW = dict(scale=(0.95, 1.05), crop=(3.0, 5.0), flip=True, ori_w=640.0, pad_hw=(480.0, 640.0))


@pytest.mark.parametrize("aligned", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("V,C", [(50, 256), (70, 96), (3, 512)])
def test_gradient_is_the_adjoint_of_the_forward(V, C, aligned):
    """Channel c of the feature maps holds a single 1 at a random (view, pixel) j_c: the forward's output is column j_c of the
    operator, so the gradient at j_c must be sum_n out[n, c] dout[n, c] (float64), inside the same bound with k = the column's
    nonzeros and sum|terms| = sum_n |out[n, c] dout[n, c]|.  More views than lanes, channel counts that are no multiple of 64."""
    from proxytransformation_amd.fusion import batch_point_sample
    rng, H, W, pts, proj = _restatement_scene(V)
    N = len(pts)
    j = rng.integers(0, V * H * W, size=C)
    feats = np.zeros((V, C, H * W), np.float32)
    feats[j // (H * W), np.arange(C), j % (H * W)] = 1.0
    feats = feats.reshape(V, C, H, W)
    dout = rng.standard_normal((N, C), dtype=np.float32)
    out, grad = _grad(_t(feats), _t(pts), _t(proj), _t(dout), aligned=aligned, **KW)
    with torch.no_grad():
        plain = batch_point_sample(None, _t(feats), _t(pts), _t(proj), "DEPTH", aligned=aligned, **KW)
    assert torch.equal(out, plain)                                  # the node's forward is the forward
    col = out.cpu().numpy().astype(np.float64) * dout.astype(np.float64)          # (N, C)
    want = col.sum(0)
    S = np.abs(col).sum(0)
    k = (col != 0).sum(0).astype(np.float64)
    got = grad.cpu().numpy().reshape(V, C, H * W)[j // (H * W), np.arange(C), j % (H * W)]
    assert (k > 0).sum() > C // 4                                   # the columns are not trivially empty
    # out[n, c] itself is w / valid_num rounded once more than the backward's term: one more 2^-24 per term, inside the + 4
    check_bound(got, want, k, S, f"adjoint V={V} C={C} {'bilinear' if aligned else 'nearest'}")


@pytest.mark.parametrize("aligned", [False, True], ids=["nearest", "bilinear"])
def test_unhit_pixels_are_exactly_zero_and_hit_pixels_inside_the_bound(aligned):
    """Every element of the gradient against the float64 sum over the index; pixels no (point, view) pair reaches are exact
    zeros (the kernel writes them: the gradient buffer is torch.empty and is never cleared)."""
    V, C = 9, 70
    rng, H, W, pts, proj = _restatement_scene(V, N=300)
    feats = rng.standard_normal((V, C, H, W), dtype=np.float32)
    dout = rng.standard_normal((len(pts), C), dtype=np.float32)
    _, grad = _grad(_t(feats), _t(pts), _t(proj), _t(dout), aligned=aligned, **KW)
    n, d, w, nvalid = hit_index(pts, proj, H, W, bilinear=aligned, **IKW)
    k, S, E = bound_terms(n, d, w, nvalid, dout, feats.shape)
    got = grad.cpu().numpy()
    empty = np.broadcast_to(k == 0, got.shape)
    assert empty.mean() > 0.2 and (~empty).mean() > 0.05
    assert (got[empty] == 0).all() and not np.signbit(got[empty]).any()
    check_bound(got, E, k, S, f"all elements {'bilinear' if aligned else 'nearest'}")


def test_scene_without_a_valid_point_gives_a_zero_gradient():
    V, C, H, W = 5, 33, 11, 13
    rng = np.random.default_rng(0)
    proj = np.tile(np.array([[300, 0, 320, 0], [0, 300, 240, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32), (V, 1, 1))
    pts = np.concatenate([rng.random((200, 2)) * 4 - 2, -1.0 - rng.random((200, 1))], 1).astype(np.float32)   # all behind the cameras
    feats = rng.standard_normal((V, C, H, W), dtype=np.float32)
    out, grad = _grad(_t(feats), _t(pts), _t(proj), _t(rng.standard_normal((200, C), dtype=np.float32)))
    assert (out == 0).all() and (grad == 0).all()
    # no point at all
    out0, grad0 = _grad(_t(feats), _t(pts[:0]), _t(proj), torch.zeros((0, C), device="cuda"))
    assert out0.shape == (0, C) and grad0.shape == feats.shape and (grad0 == 0).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("aligned", [False, True], ids=["nearest", "bilinear"])
def test_16_bit_gradient_is_the_fp32_gradient_rounded_once(dtype, aligned):
    V, C = 7, 100
    rng, H, W, pts, proj = _restatement_scene(V, N=2000)
    feats = torch.from_numpy(rng.standard_normal((V, C, H, W), dtype=np.float32)).to(dtype)
    dout = _t(rng.standard_normal((len(pts), C), dtype=np.float32))
    _, g16 = _grad(feats.cuda(), _t(pts), _t(proj), dout, aligned=aligned, **KW)
    _, g32 = _grad(feats.float().cuda(), _t(pts), _t(proj), dout, aligned=aligned, **KW)
    assert g16.dtype == dtype and g32.dtype == torch.float32
    assert torch.equal(g16.view(torch.int16), g32.to(dtype).view(torch.int16))


@pytest.mark.parametrize("aligned", [False, True], ids=["nearest", "bilinear"])
def test_two_runs_are_bitwise_equal(aligned):
    V, C = 70, 96
    rng, H, W, pts, proj = _restatement_scene(V)
    feats = _t(rng.standard_normal((V, C, H, W), dtype=np.float32))
    dout = _t(rng.standard_normal((len(pts), C), dtype=np.float32))
    runs = [_grad(feats, _t(pts), _t(proj), dout, aligned=aligned, **KW)[1] for _ in range(3)]
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    assert torch.equal(runs[0].view(torch.int32), runs[2].view(torch.int32))


def _grid_sample_restatement(feats, pts, proj, aligned, pad=(480.0, 640.0), scale=(0.95, 1.05), crop=(3.0, 5.0), ori_w=640.0):
    """batch_point_sample as differentiable torch on the GPU (the structure of point_fusion.py:208-313: F.grid_sample per view,
    sum over the views, division by the number of valid views), flip on, for the end-to-end comparison."""
    V = feats.shape[0]
    p4 = torch.cat([pts, pts.new_ones(len(pts), 1)], 1)
    q = torch.einsum("vrk,nk->vnr", proj, p4)
    z = q[..., 2].clamp(min=1e-3)
    cx = ori_w - (q[..., 0] / z * scale[0] - crop[0])
    cy = q[..., 1] / z * scale[1] - crop[1]
    grid = torch.stack([cx / pad[1] * 2 - 1, cy / pad[0] * 2 - 1], -1).view(V, 1, -1, 2)
    samp = F.grid_sample(feats, grid, mode="bilinear" if aligned else "nearest", padding_mode="zeros", align_corners=True)
    valid = ((cx < pad[1]) & (cx > 0) & (cy < pad[0]) & (cy > 0) & (q[..., 2] > 0)).sum(0)
    out = samp.squeeze(2).sum(0).t() / valid.clamp(min=1)[:, None]
    return out * (valid > 0)[:, None]


def _away_from_boundaries(pts, proj, H, W, pad=(480.0, 640.0), scale=(0.95, 1.05), crop=(3.0, 5.0), ori_w=640.0):
    """Points whose projection, in float64, is at least 1e-3 px from a pixel-rounding boundary and 1e-2 from a validity
    boundary in every view (the filter of gen_golden.gen_point_sample): the restatement's fp32 projection is not the pinned
    order, and a point ON a boundary may pick another pixel there."""
    p4 = np.concatenate([pts.astype(np.float64), np.ones((len(pts), 1))], 1)
    q = np.einsum("vrk,nk->vnr", proj.astype(np.float64), p4)
    z = np.maximum(q[..., 2], 1e-3)
    cx = ori_w - (q[..., 0] / z * scale[0] - crop[0])
    cy = q[..., 1] / z * scale[1] - crop[1]
    safe = np.ones(len(pts), bool)
    for arr, size, hi in ((cx, W, pad[1]), (cy, H, pad[0])):
        pix = arr / hi * (size - 1)
        inside = (pix > -2) & (pix < size + 1)                       # far outside the map nothing can flip
        safe &= (~inside | (np.abs(pix - np.floor(pix) - 0.5) > 1e-3)).all(0)
        safe &= (np.abs(arr) > 1e-2).all(0) & (np.abs(arr - hi) > 1e-2).all(0)
    safe &= (np.abs(q[..., 2]) > 1e-2).all(0) & (np.abs(q[..., 2] - 1e-3) > 1e-4).all(0)
    return pts[safe]


@pytest.mark.parametrize("aligned", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("use_prepared", [False, True], ids=["direct", "prepared"])
def test_conv_weight_gradient_end_to_end(aligned, use_prepared):
    """Conv2d -> batch_point_sample -> weighted sum: the conv's weight gradient against the same graph through the
    F.grid_sample restatement, to 1e-5 of the gradient's scale.  prepared=: the gradient still reaches img_features."""
    from proxytransformation_amd.fusion import batch_point_sample, prepare_features
    V, C = 6, 48
    rng, H, W, pts, proj = _restatement_scene(V, N=3000)
    pts = _away_from_boundaries(pts, proj, H, W)
    assert len(pts) > 2500
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(8, C, 3, padding=1).cuda()
    img = _t(rng.standard_normal((V, 8, H, W), dtype=np.float32))
    wsum = _t(rng.standard_normal((len(pts), C), dtype=np.float32))
    pts_t, proj_t = _t(pts), _t(proj)
    grads = []
    for ours in (True, False):
        conv.zero_grad()
        f = conv(img)
        if ours:
            prepared = prepare_features(f.detach()) if use_prepared else None
            out = batch_point_sample(None, f, pts_t, proj_t, "DEPTH", aligned=aligned, prepared=prepared, **KW)
        else:
            out = _grid_sample_restatement(f, pts_t, proj_t, aligned)
        (out * wsum).sum().backward()
        grads.append((conv.weight.grad.clone(), conv.bias.grad.clone(), out.detach()))
    (gw, gb, o1), (rw, rb, o2) = grads
    assert (o1 != 0).any() and (o1 - o2).abs().max().item() <= 1e-4          # the two graphs are the same function
    scale = rw.abs().max().item()
    print(f"conv weight gradient: scale {scale:.4g}, max |diff| {(gw - rw).abs().max().item():.3g}")
    assert (gw - rw).abs().max().item() <= 1e-5 * scale
    assert (gb - rb).abs().max().item() <= 1e-5 * rb.abs().max().item()


@pytest.mark.parametrize("how", ["requires_grad_false", "no_grad"])
def test_paths_without_gradient_are_unchanged(how):
    """No grad_fn, and bit-identical to the restatement the forward is pinned to (what the call returned before the node existed)."""
    from oracle import oracle
    from proxytransformation_amd.fusion import batch_point_sample
    V, C = 50, 256
    rng, H, W, pts, proj = _restatement_scene(V)
    feats = rng.standard_normal((V, C, H, W), dtype=np.float32)
    ref, _ = oracle.point_sample(pts, feats, proj, **IKW)
    f = _t(feats)
    if how == "no_grad":
        f.requires_grad_()
        with torch.no_grad():
            out = batch_point_sample(None, f, _t(pts), _t(proj), "DEPTH", **KW)
    else:
        out = batch_point_sample(None, f, _t(pts), _t(proj), "DEPTH", **KW)
    assert out.grad_fn is None and not out.requires_grad
    assert np.array_equal(out.cpu().numpy(), ref)
    # and the node's forward gives the same bits
    out_g, _ = _grad(_t(feats), _t(pts), _t(proj), torch.ones((len(pts), C), device="cuda"), **KW)
    assert torch.equal(out_g, out)
