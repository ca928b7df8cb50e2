"""The geometric front end -- voxelisation (csrc/voxel.hip), point sampling forward and backward (csrc/pointsample.hip) and the level
join (csrc/level_join.hip) -- held ON the decisions these operators take, against references written from the definitions
(tests/geometry_edges_util.py): torch's own fp32 ``floor(p / vs)`` and a float64 ``F.grid_sample`` statement with autograd's gradient.
On the exact lattice every fp32 step is exact, so the device must give ``float32(reference64)`` bit for bit.  Every output of a
library call lies in front of sentinel words that must keep their bits, and every call runs twice and must give the same bits.
tests/test_geometry_edges_host.py shows that a restatement wrong in one decision fails these inputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import geometry_edges_util as U

pytestmark = pytest.mark.gpu

TAIL = 1024
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _lib():
    from proxytransformation_amd import _abi
    return _abi, _abi.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_bits(got, want, what=""):
    """fp32 device tensor against a float64 / float32 CPU reference rounded to fp32: equal bits (so +0.0 is not -0.0)."""
    w = np.ascontiguousarray(np.asarray(want).astype(np.float32))
    g = got.detach().cpu().numpy()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g.view(np.int32) != w.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{g[bad][0]!r} against {w[bad][0]!r}"


def _twice(fn):
    """Run a case twice: same bits in every output."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8) if x.is_floating_point() else x, y.view(torch.uint8) if y.is_floating_point() else y), \
            "two runs differ"
    return a


# ================================================================================================================== voxelisation
def _vox_raw(outs, voxel_size, Ncap=None):
    """ptx_voxelize_rep itself on a packed copy of ``outs``, every output in front of sentinels.  Returns numpy
    (coords, feats, inverse (B,Ncap), rep, ends, nvox, overflow) and the device tensors the backward reads."""
    _abi, lib = _lib()
    B = len(outs)
    n = [len(o) for o in outs]
    Ncap = max(max(n), 1) if Ncap is None else Ncap
    buf = torch.zeros((B, Ncap, 3), device="cuda")
    for b, o in enumerate(outs):
        if n[b]:
            buf[b, :n[b]] = _t(np.ascontiguousarray(o, np.float32))
    counts = torch.tensor(n, dtype=torch.int32).cuda()
    cap = B * Ncap
    coords = torch.full((cap * 4 + TAIL,), -7, dtype=torch.int32, device="cuda")
    feats = torch.full((cap * 3 + TAIL,), -7.5, device="cuda")
    inverse = torch.full((cap + TAIL,), -7, dtype=torch.int32, device="cuda")
    rep = torch.full((cap + TAIL,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((2 + TAIL,), -1, dtype=torch.int32, device="cuda")
    ends = torch.full((B + TAIL,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.ptx_voxel_workspace_bytes(B, Ncap)
    assert nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    _abi.check(lib.ptx_voxelize_rep(buf.data_ptr(), counts.data_ptr(), B, Ncap, float(voxel_size), coords.data_ptr(), feats.data_ptr(),
                                    inverse.data_ptr(), rep.data_ptr(), info.data_ptr(), ends.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _stream()), "ptx_voxelize_rep")
    torch.cuda.synchronize()
    nvox, overflow = int(info[0]), int(info[1])
    assert 0 <= nvox <= cap
    assert (coords[cap * 4:] == -7).all() and (feats[cap * 3:] == -7.5).all() and (inverse[cap:] == -7).all()
    assert (rep[cap:] == -7).all() and (info[2:] == -1).all() and (ends[B:] == -1).all()
    assert (coords[nvox * 4:cap * 4] == -7).all() and (feats[nvox * 3:cap * 3] == -7.5).all() and (rep[nvox:cap] == -7).all(), \
        "rows past the published count were written"
    dev = dict(inverse=inverse, rep=rep, counts=counts, B=B, Ncap=Ncap, n=n)
    return (coords[:nvox * 4].view(-1, 4).cpu().numpy(), feats[:nvox * 3].view(-1, 3).cpu().numpy(), inverse[:cap].view(B, Ncap).cpu().numpy(),
            rep[:nvox].cpu().numpy(), ends[:B].cpu().numpy(), nvox, overflow, dev)


def _check_voxels(outs, voxel_size, Ncap=None):
    """The raw call against the torch statement, bit for bit; returns what the backward check needs."""
    res = []
    for _ in range(2):
        res.append(_vox_raw(outs, voxel_size, Ncap))
    for x, y in zip(res[0][:7], res[1][:7]):
        assert np.array_equal(x, y), "two runs differ"
    coords, feats, inverse, rep, ends, nvox, overflow, dev = res[0]
    c, f, inv, r = U.ref_voxelize(outs, voxel_size)
    assert overflow == 0 and nvox == len(c)
    assert np.array_equal(coords, c)
    assert np.array_equal(feats.view(np.int32), f.view(np.int32))
    n, cap = dev["n"], dev["Ncap"]
    sizes = np.cumsum([0] + n)
    for b in range(len(outs)):
        assert np.array_equal(inverse[b, :n[b]], inv[b]) and (inverse[b, n[b]:] == -1).all()
    b_of = np.searchsorted(sizes, r, side="right") - 1
    assert np.array_equal(rep, b_of * cap + (r - sizes[b_of]))                       # flat PADDED index of the kept point
    assert np.array_equal(ends, np.cumsum(np.bincount(c[:, 0], minlength=len(outs))))
    return c, f, inv, r, dev


@functools.lru_cache(maxsize=None)
def _module():
    from proxytransformation_amd.synth import PreshapeConfig
    from tests.util import build_module
    cfg = PreshapeConfig("ge", B=2, N=1024, grid_size=4, dynamic_drop_radio=0.5, L=4, V=2, seed_base=77)
    return build_module(cfg)[0].cuda()


def _check_quantize(outs, voxel_size, c, f, inv):
    """``quantize`` (no grad, return_inverse) and its differentiable route (rep) against the same statement."""
    m = _module()
    touts = [_t(np.ascontiguousarray(o, np.float32).reshape(-1, 3)) for o in outs]
    coords, feats, inverse, ends = m.quantize(touts, voxel_size, return_inverse=True, return_scene_rows=True)
    assert coords.dtype == torch.int32 and np.array_equal(coords.cpu().numpy(), c)
    assert np.array_equal(feats.cpu().numpy().view(np.int32), f.view(np.int32))
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(inverse, inv))
    assert list(ends) == np.cumsum(np.bincount(c[:, 0], minlength=len(outs))).tolist()
    leaves = [o.clone().requires_grad_() for o in touts]
    coords2, feats2, inverse2 = m.quantize(leaves, voxel_size, return_inverse=True)
    assert feats2.grad_fn is not None and torch.equal(feats2.detach(), feats) and torch.equal(coords2, coords)
    assert all(torch.equal(a, b) for a, b in zip(inverse2, inverse))
    g = np.random.default_rng(2).integers(1, 9, (len(c), 3)).astype(np.float32)
    feats2.backward(_t(g))
    first = {}
    for b, iv in enumerate(inv):
        want = np.zeros((len(iv), 3), np.float32)
        for i, r in enumerate(iv.tolist()):
            if r not in first:
                first[r] = (b, i)
                want[i] = g[r]
        got = leaves[b].grad
        if len(iv) == 0:
            assert got is None or got.numel() == 0
            continue
        _same_bits(got, want, f"dpoints of scene {b}")                       # dropped duplicates: exactly +0.0


@pytest.mark.parametrize("voxel_size", U.VOXEL_SIZES)
def test_voxel_boundaries_equal_torch_floor_division(voxel_size):
    """fl(k vs) for k in [-3000, 3000) and the neighbour to either side, -0.0, the smallest subnormals: the voxel is torch's
    floor(p / vs) in fp32 -- k - 1 at hundreds of these k -- in ``quantize``, its inverse, its differentiable route and the raw call."""
    from proxytransformation_amd.pipeline import level_coordinates
    cloud, _ = U.boundary_cloud(voxel_size)
    outs = [cloud, np.concatenate([cloud[::-1], cloud + np.float32(voxel_size / 4)])]
    c, f, inv, _, _ = _check_voxels(outs, voxel_size)
    _check_quantize(outs, voxel_size, c, f, inv)
    # the level positions the project emits (coordinate * voxel_size, one rounded multiply) fall back into torch's voxel of them
    ends = np.cumsum(np.bincount(c[:, 0], minlength=2)).tolist()
    lc, lp, le = level_coordinates(_t(c), ends, 1, voxel_size, {})
    assert np.array_equal(lc.cpu().numpy(), c) and le == ends
    pos = c[:, 1:].astype(np.float32) * np.float32(voxel_size)
    assert np.array_equal(lp.cpu().numpy().view(np.int32), pos.view(np.int32))
    c2, _, inv2, _, _ = _check_voxels([pos[:ends[0]], pos[ends[0]:]], voxel_size)
    moved = int((c2[inv2[0]][:, 1:] != c[:ends[0], 1:]).any(1).sum())
    print(f"voxel size {voxel_size}: {len(c)} rows; {moved} of {ends[0]} emitted positions of scene 0 fall into the voxel below")
    assert (moved > 0) == (U.floor_misses(voxel_size) > 0)


SCENE_SIZES = (1, 2047, 2048, 2049, 0, 4097)


def _scene_size_clouds():
    rng = np.random.default_rng(11)
    outs = [((rng.random((k, 3)) - 0.5) * 6).astype(np.float32) for k in SCENE_SIZES]
    outs.append((np.float32(0.5) + rng.random((4097, 3)) * 0.2).astype(np.float32))            # one voxel of size 0.25: [0.5, 0.75)^3
    return outs


@pytest.mark.parametrize("pad", [0, 3], ids=["Ncap=4097", "Ncap=4100"])
def test_voxel_scene_sizes_at_the_tile_edge_and_the_features_backward(pad):
    """Scenes of 1 / 2047 / 2048 / 2049 / 0 / 4097 points in one call (2 048-point tiles) and a scene whose 4 097 points share one
    voxel; then ptx_voxel_features_bwd on them: the one-point-per-thread path (capacity 4 097) and the four-point path (4 100), counts
    that end inside a group of four, dropped duplicates exactly +0.0, rows past a count untouched (the four-point path finishes the group of four it began
    with +0.0)."""
    _abi, lib = _lib()
    outs = _scene_size_clouds()
    c, f, inv, r, dev = _check_voxels(outs, 0.25, Ncap=4097 + pad)
    last = len(outs) - 1
    mine = np.nonzero(c[:, 0] == last)[0]
    assert len(mine) == 1 and np.array_equal(f[mine[0]], outs[last][0]) and (inv[last] == mine[0]).all()
    assert len(c) < sum(len(o) for o in outs) - 4096                                   # duplicates occur in the other scenes too
    if pad == 0:
        _check_quantize(outs, 0.25, c, f, inv)
    B, Ncap, n = dev["B"], dev["Ncap"], dev["n"]
    g = np.random.default_rng(3).integers(1, 9, (len(c), 3)).astype(np.float32)

    def run():
        dpoints = torch.full((B * Ncap * 3 + TAIL,), -7.5, device="cuda")
        _abi.check(lib.ptx_voxel_features_bwd(_t(g).data_ptr(), len(c), dev["inverse"].data_ptr(), dev["rep"].data_ptr(),
                                              dev["counts"].data_ptr(), B, Ncap, dpoints.data_ptr(), _stream()), "ptx_voxel_features_bwd")
        torch.cuda.synchronize()
        return (dpoints,)
    dpoints = _twice(run)[0]
    assert (dpoints[B * Ncap * 3:] == -7.5).all()
    got = dpoints[:B * Ncap * 3].view(B, Ncap, 3)
    sizes = np.cumsum([0] + n)
    for b in range(B):
        want = np.zeros((n[b], 3), np.float32)
        rows = np.nonzero((r >= sizes[b]) & (r < sizes[b + 1]))[0]
        want[r[rows] - sizes[b]] = g[rows]
        _same_bits(got[b, :n[b]], want, f"dpoints of scene {b}")
        past = n[b] if Ncap % 4 else -(-n[b] // 4) * 4              # the four-point path writes the rest of its last group: +0.0
        assert (got[b, n[b]:past].cpu().numpy().view(np.int32) == 0).all(), "the rest of the last group of four is not +0.0"
        assert (got[b, past:] == -7.5).all(), "a point past its scene's count was written"


def test_voxel_key_range_and_packing():
    """voxel_size 0.5 (exact quotients), scene 63 of 64: -2^18 and 2^18 - 1 on every axis are rows with those integers (the top of the
    key packing, all fields at their extremes); 2^18 and -2^18 - 1 are refused and counted.  The same through level_coordinates at
    strides 1, 2 and 64: a coordinate c is kept when floor(c / stride) lies in [-2^18, 2^18)."""
    from proxytransformation_amd.pipeline import level_coordinates
    lo, hi = -(1 << 18), (1 << 18) - 1
    corners = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.int64)
    pts = (corners.astype(np.float32) * np.float32(0.5) + np.float32(0.25)).astype(np.float32)       # interior of the voxel, exact
    outs = [np.zeros((1, 3), np.float32) for _ in range(63)] + [np.concatenate([pts, pts[::-1]])]
    c, f, inv, _, _ = _check_voxels(outs, 0.5)
    assert np.array_equal(c[63:, 1:], corners) and (c[63:, 0] == 63).all() and len(c) == 63 + 8
    _check_quantize(outs, 0.5, c, f, inv)
    bad = np.array([[(hi + 1) * 0.5, 0, 0], [0, (lo - 1) * 0.5, 0], [0, 0, (hi + 1) * 0.5], [1.0, 1.0, 1.0]], np.float32)
    outs[63] = np.concatenate([pts, bad])
    assert _vox_raw(outs, 0.5)[6] == 3
    with pytest.raises(RuntimeError, match="quantize: 3 points fall outside"):
        _module().quantize([_t(o) for o in outs], 0.5)
    for stride in (1, 2, 64):
        rows = np.concatenate([np.concatenate([np.full((1, 1), b), np.zeros((1, 3))], 1) for b in range(63)] +
                              [np.concatenate([np.full((8, 1), 63), corners * stride + (corners > 0) * (stride - 1)], 1)]).astype(np.int32)
        ends = list(range(1, 64)) + [63 + 8]
        lc, lp, le = level_coordinates(_t(rows), ends, stride, 0.5, {})
        want = rows.copy()
        want[:, 1:] = np.floor_divide(rows[:, 1:], stride) * stride
        assert le == ends and np.array_equal(lc.cpu().numpy(), want)
        assert np.array_equal(lp.cpu().numpy().view(np.int32), (want[:, 1:].astype(np.float32) * np.float32(0.5)).view(np.int32))
        rows[-1, 2] = (hi + 1) * stride
        with pytest.raises(RuntimeError, match="overflow 1"):
            level_coordinates(_t(rows), ends, stride, 0.5, {})
        rows[-1, 2] = lo * stride - 1                                                   # floor(c / stride) = -2^18 - 1
        with pytest.raises(RuntimeError, match="overflow 1"):
            level_coordinates(_t(rows), ends, stride, 0.5, {})


def test_voxel_non_finite_points_are_outside_the_range():
    """The rule (include/proxyt.h): a NaN or infinite coordinate is outside the key range -- counted like a coordinate past +-2^18 and
    refused by ``quantize``; the rows of the finite points of other calls keep their bits (every other voxel test)."""
    rng = np.random.default_rng(5)
    base = ((rng.random((300, 3)) - 0.5) * 6).astype(np.float32)
    for name, bad in (("nan", [np.nan]), ("inf", [np.inf, -np.inf]), ("all", [np.nan, np.inf, -np.inf])):
        p = base.copy()
        rows = []
        for j, v in enumerate(bad):
            for axis in range(3):
                p[10 + 7 * (3 * j + axis), axis] = v
                rows.append(10 + 7 * (3 * j + axis))
        overflow = _vox_raw([base, p], 0.01)[6]
        print(f"non-finite voxelisation ({name}): {len(rows)} such points, {overflow} counted outside")
        assert overflow == len(rows), f"{name}: {len(rows)} non-finite points, {overflow} counted outside the range"
        with pytest.raises(RuntimeError, match=f"quantize: {len(rows)} points fall outside"):
            _module().quantize([_t(base), _t(p)], 0.01)


# ================================================================================================================== sampling, forward
def _scal(kw, bilinear):
    return (float(kw["scale"][0]), float(kw["scale"][1]), float(kw["crop"][0]), float(kw["crop"][1]), 1 if kw["flip"] else 0,
            float(kw["ori_w"]), float(kw["pad_hw"][0]), float(kw["pad_hw"][1]), 1 if bilinear else 0)


def _api_kw(kw, pre, bilinear):
    return dict(img_scale_factor=kw["scale"], img_crop_offset=kw["crop"], img_flip=bool(kw["flip"]),
                img_pad_shape=(int(kw["pad_hw"][0]), int(kw["pad_hw"][1])), img_shape=(int(kw["pad_hw"][0]), int(kw["ori_w"])),
                aligned=bool(bilinear), pre_transform=None if pre is None else torch.from_numpy(np.asarray(pre, np.float32)))


def _ps_raw(feats, pts, proj, pre, scal, prepared=False):
    """ptx_point_sample itself (direct: the maps are transposed in the call; prepared: ptx_point_sample_prepare first), out and
    valid_num in front of sentinels.  Returns (out (N,C), valid_num (N)) device tensors."""
    _abi, lib = _lib()
    feats = feats.contiguous()
    V, C, H, W = feats.shape
    N = pts.shape[0]
    out = torch.full((N * C + TAIL,), -7.5, device="cuda")
    vn = torch.full((N + TAIL,), -7, dtype=torch.int32, device="cuda")
    nbytes = lib.ptx_point_sample_workspace_bytes(V, C, H, W)
    assert nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    fptr = feats.data_ptr()
    if prepared:
        _abi.check(lib.ptx_point_sample_prepare(feats.data_ptr(), _DT[feats.dtype], V, C, H, W, ws.data_ptr(), ws.numel(), _stream()),
                   "ptx_point_sample_prepare")
        fptr = None
    _abi.check(lib.ptx_point_sample(pts.data_ptr(), N, fptr, _DT[feats.dtype], V, C, H, W, proj.data_ptr(),
                                    None if pre is None else pre.data_ptr(), *scal, out.data_ptr(), vn.data_ptr(), ws.data_ptr(),
                                    ws.numel(), _stream()), "ptx_point_sample")
    torch.cuda.synchronize()
    assert (out[N * C:] == -7.5).all() and (vn[N:] == -7).all(), "sentinels behind out / valid_num"
    return out[:N * C].view(N, C), vn[:N]


def _forward(feats, pts, proj, pre, kw, bilinear, prepared=False):
    f, p, P = (feats if isinstance(feats, torch.Tensor) else _t(feats)), _t(pts), _t(proj)
    A = None if pre is None else _t(np.asarray(pre, np.float32))
    return _twice(lambda: _ps_raw(f, p, P, A, _scal(kw, bilinear), prepared))


@functools.lru_cache(maxsize=None)
def _lattice_ref(name, bilinear, V=3, C=512):
    pts, proj, kw, pre = U.lattice_case(name, V)
    feats = U.integer_maps(V, C, seed=V)
    ref, nv = U.ref_point_sample(pts, feats, proj, bilinear=bilinear, pre=pre, **kw)
    return pts, proj, kw, pre, feats, ref.numpy(), nv


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("name", list(U.LAT_CONFIGS))
def test_forward_on_the_lattice_is_the_float64_reference_bit_for_bit(name, bilinear):
    """Ties on both parities, cx exactly 0 and pad_w, ix = -0.5 and W - 1 + 0.5, one step outside; flip / scale / crop / pre-transform;
    fp32 / bf16 / fp16 maps; C in {1, 63, 64, 65, 512}; N in {1, 4, 5} and the whole lattice; direct and prepared route; the API."""
    from proxytransformation_amd.fusion import batch_point_sample, prepare_features
    pts, proj, kw, pre, feats, ref, nv = _lattice_ref(name, bilinear)
    some = np.nonzero(nv > 0)[0][::7][:5]
    assert len(some) == 5
    for dtype, C, prepared in ((torch.float32, 1, False), (torch.float32, 63, True), (torch.bfloat16, 64, False),
                               (torch.float16, 65, True), (torch.float32, 512, False), (torch.bfloat16, 512, True)):
        f = _t(feats[:, :C]).to(dtype)
        out, vn = _forward(f, pts, proj, pre, kw, bilinear, prepared)
        _same_bits(out, ref[:, :C], f"{name} C={C} {dtype}")
        assert np.array_equal(vn.cpu().numpy(), nv)
        for N in (1, 4, 5):
            o, v = _forward(f, pts[some[:N]], proj, pre, kw, bilinear, prepared)
            _same_bits(o, ref[some[:N], :C], f"{name} C={C} N={N}")
            assert np.array_equal(v.cpu().numpy(), nv[some[:N]])
    f = _t(feats[:, :65])
    api = batch_point_sample(None, f, _t(pts), _t(proj), "DEPTH", **_api_kw(kw, pre, bilinear))
    _same_bits(api, ref[:, :65], "batch_point_sample")
    api2 = batch_point_sample(None, f, _t(pts), _t(proj), "DEPTH", prepared=prepare_features(f), **_api_kw(kw, pre, bilinear))
    assert torch.equal(api, api2)
    print(f"lattice forward {name} {'bilinear' if bilinear else 'nearest'}: bit-equal; valid views per point "
          f"{np.bincount(nv, minlength=4).tolist()}")


MARKED = (0, 63, 64, 127, 128)


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("V", [1, 64, 65, 128, 129])
def test_forward_view_counts_around_the_64_view_passes(V, bilinear):
    """ps_accumulate takes the views 64 at a time.  The first and the last view of every pass carry a one-hot map (8 in a channel of
    their own, every pixel), so a dropped or doubled view shows in the bits; valid_num against the reference's count."""
    pts, proj, kw, pre = U.lattice_case("plain", V)
    feats = U.integer_maps(V, 64, seed=V)
    for m, v in enumerate(MARKED):
        if v < V:
            feats[v] = 0
            feats[v, m] = 8
    ref, nv = U.ref_point_sample(pts, feats, proj, bilinear=bilinear, **kw)
    out, vn = _forward(feats, pts, proj, pre, kw, bilinear, prepared=V % 2 == 0)
    assert np.array_equal(vn.cpu().numpy(), nv)
    _same_bits(out, ref.numpy(), f"V={V}")
    print(f"V={V} {'bilinear' if bilinear else 'nearest'}: bit-equal, valid views per point {nv.min()} .. {nv.max()}")


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("H,W", [(1, 17), (9, 1), (1, 1)])
def test_forward_degenerate_maps(H, W, bilinear):
    pts, proj, kw, pre = U.lattice_case("flip")
    feats = U.integer_maps(3, 65, H, W, seed=H * 100 + W)
    ref, nv = U.ref_point_sample(pts, feats, proj, bilinear=bilinear, **kw)
    out, vn = _forward(feats, pts, proj, pre, kw, bilinear)
    assert np.array_equal(vn.cpu().numpy(), nv) and (nv > 0).any()
    _same_bits(out, ref.numpy(), f"H={H} W={W}")


def _extreme_points():
    """Rows that ps_project's rule makes zero with valid_num 0 in EVERY view of the plain lattice cameras (identity plus shifts):
    NaN in any coordinate, infinities, 1e30 in the image plane, depth 0 / -0.0 / 1e-3f / the smallest subnormal with an image-plane
    coordinate of 3 (3 / 1e-3 lies far outside the 64-unit image), negative depth -- also with a projection INSIDE the image
    (sampled, never valid: depth > 0 fails)."""
    nan, inf, tiny = np.nan, np.inf, np.float32(1e-45)
    return np.array([[nan, 5, 1], [3, nan, 1], [3, 5, nan], [nan, nan, nan], [inf, 5, 1], [-inf, 5, 1], [3, inf, 1], [3, -inf, 1],
                     [inf, 5, inf], [3, 5, inf], [3, 5, -inf], [inf, inf, inf], [1e30, 5, 1], [3, -1e30, 1], [1e30, 1e30, 1],
                     [3, 5, 0.0], [3, 5, -0.0], [3, 5, np.float32(1e-3)], [3, 5, tiny], [3, 5, -tiny], [3, 5, -1], [0.008, 0.008, 0.0],
                     [0.008, 0.008, -0.0], [0.008, 0.008, -1.0], [6, 6, -2.0]], np.float32)


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_forward_non_finite_and_extreme_points_give_zero_rows(bilinear):
    """Held to the stated rule, not to torch's grid sampler: these rows are exactly +0.0 with valid_num 0, and every other row of the
    same call is what it is without them."""
    pts, proj, kw, pre, feats, ref, nv = _lattice_ref("plain", bilinear)
    ext = _extreme_points()
    every = 384 // len(ext)
    mixed, is_ext = [], []
    for i, p in enumerate(pts):
        mixed.append(p); is_ext.append(False)
        if i % every == 0 and i // every < len(ext):
            mixed.append(ext[i // every]); is_ext.append(True)
    mixed, is_ext = np.array(mixed, np.float32), np.array(is_ext)
    assert is_ext.sum() == len(ext)
    for C, dtype in ((65, torch.float32), (512, torch.bfloat16)):
        out, vn = _forward(_t(feats[:, :C]).to(dtype), mixed, proj, pre, kw, bilinear)
        o, v = out.cpu().numpy(), vn.cpu().numpy()
        assert (v[is_ext] == 0).all(), f"valid_num of the extreme rows: {v[is_ext].tolist()}"
        assert (o[is_ext].view(np.int32) == 0).all(), "an extreme row is not exactly +0.0"
        _same_bits(out[torch.from_numpy(~is_ext).cuda()], ref[:, :C], "the other rows")
        assert np.array_equal(v[~is_ext], nv)


def test_forward_depth_clamp_on_a_valid_point():
    """(0.004, 0.004, 1e-4): a positive depth below the clamp.  The view is valid and the point is projected with 1e-3, not with
    its own depth (pixel 1 instead of pixel 10); nearest, against the float64 reference, among lattice rows."""
    pts, proj, kw, pre, feats, _, _ = _lattice_ref("plain", False)
    pts = np.concatenate([pts[:7], np.array([[0.004, 0.004, 1e-4]], np.float32), pts[7:20]])
    ref, nv, g = U.ref_point_sample(pts, feats[:, :65], proj, geometry=True, **kw)
    assert nv[7] >= 1 and g["valid"][0, 7] and abs(g["ix"][0, 7] - 1.0) < 1e-3 and abs(g["iy"][0, 7] - 1.0) < 1e-3
    assert np.abs(ref.numpy()[7]).max() > 0
    out, vn = _forward(feats[:, :65], pts, proj, pre, kw, False)
    assert np.array_equal(vn.cpu().numpy(), nv)
    _same_bits(out, ref.numpy(), "depth clamp")


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_forward_generic_case_against_float64(bilinear):
    """3 non-dyadic cameras, 2 000 random points, C = 64.  Points within the margin of a decision in float64 (a half pixel, the image
    border, depth 0) are left out -- the margin is measured on the CPU (4 x the largest pixel-coordinate difference of the fp32
    restatement), at most 5 % -- and for the others valid_num and the chosen pixels equal the reference's and the values are held by
    sparse_util.hold against the restatement and float64."""
    from oracle import oracle
    from tests.sparse_util import hold
    margin, worst, _ = U.generic_margin()
    rng, H, W, pts, proj = U.generic_scene(U.GENERIC_SEED)
    kw = U.GENERIC_KW
    feats = rng.standard_normal((3, 64, H, W)).astype(np.float32)
    ref64, nv, g = U.ref_point_sample(pts, feats, proj, bilinear=bilinear, geometry=True, **kw)
    keep = U.generic_keep(g, H, W, kw["pad_hw"], margin, bilinear)
    print(f"generic {'bilinear' if bilinear else 'nearest'}: margin {margin:.3g} px (largest |ix32 - ix64| {worst:.3g}), left out "
          f"{100 * (1 - keep.mean()):.2f} % of {len(pts)} points")
    assert 1 - keep.mean() <= 0.05
    ref32, _ = oracle.point_sample(pts, feats, proj, bilinear=bilinear, **kw)
    out, vn = _forward(feats, pts, proj, None, kw, bilinear)
    assert np.array_equal(vn.cpu().numpy()[keep], nv[keep]) and (nv[keep] > 0).sum() > 100
    hold(f"point_sample generic {'bilinear' if bilinear else 'nearest'}", out.cpu().numpy()[keep], ref32[keep], ref64.numpy()[keep])
    if bilinear:
        return                                              # (the four neighbours and their weights are what the values hold)
    # the chosen pixels: view v's map holds its pixel number + 1 in channel v and nothing else, so out[:, v] * valid_num is the pixel
    # number + 1 of view v (0: none), for the device and for the reference
    code = np.zeros((3, 64, H, W), np.float32)
    for v in range(3):
        code[v, v] = np.arange(1, H * W + 1, dtype=np.float32).reshape(H, W)
    cref, _ = U.ref_point_sample(pts, code, proj, **kw)
    cout, _ = _forward(code, pts, proj, None, kw, False)
    got = cout.cpu().numpy()[keep, :3].astype(np.float64) * np.maximum(nv[keep], 1)[:, None]
    want = cref.numpy()[keep, :3] * np.maximum(nv[keep], 1)[:, None]
    assert np.abs(got - np.rint(got)).max() < 1e-3 and np.array_equal(np.rint(got), np.rint(want))
    assert (np.rint(want) > 0).sum() > 100


# ================================================================================================================== sampling, backward
def _psb_raw(pts, dout, vn, shape, proj, pre, scal, dtype=torch.float32):
    """ptx_point_sample_bwd itself, the gradient in front of sentinels (the buffer is never cleared: every element is written)."""
    _abi, lib = _lib()
    V, C, H, W = shape
    N = pts.shape[0]
    numel = V * C * H * W
    dfe = torch.full((numel + TAIL,), -7.5, device="cuda").to(dtype)
    nbytes = lib.ptx_point_sample_bwd_workspace_bytes(N, V, H, W, scal[-1])
    assert nbytes > 0
    # zeroed: an index entry that a broken build never writes then reads point 0 with weight 0 (a wrong value, caught below) instead
    # of an arbitrary address
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    _abi.check(lib.ptx_point_sample_bwd(pts.data_ptr(), N, dout.data_ptr(), vn.data_ptr(), V, C, H, W, proj.data_ptr(),
                                        None if pre is None else pre.data_ptr(), *scal, dfe.data_ptr(), _DT[dtype], ws.data_ptr(),
                                        ws.numel(), _stream()), "ptx_point_sample_bwd")
    torch.cuda.synchronize()
    assert (dfe[numel:] == -7.5).all(), "sentinels behind the gradient"
    return dfe[:numel].view(V, C, H, W)


def _backward(pts, proj, pre, kw, bilinear, dout, shape):
    """Forward (for valid_num; zero maps) and backward, twice; returns (gradient, valid_num) on the device."""
    p, P, d = _t(pts), _t(proj), _t(dout)
    A = None if pre is None else _t(np.asarray(pre, np.float32))
    scal = _scal(kw, bilinear)
    _, vn = _ps_raw(torch.zeros(shape, device="cuda"), p, P, A, scal)
    vn = vn.contiguous()
    return _twice(lambda: (_psb_raw(p, d, vn, shape, P, A, scal),))[0], vn


def _index_terms(pts, proj, pre, kw, bilinear, dout, shape):
    from tests.test_gpu_point_sample_grad import bound_terms, hit_index
    n, d, w, nv = hit_index(pts, proj, shape[2], shape[3], bilinear=bilinear, pre=pre,
                            **{k: kw[k] for k in ("scale", "crop", "flip", "ori_w", "pad_hw")})
    k, S, _ = bound_terms(n, d, w, nv, dout, shape)
    return k, S, nv


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("name", list(U.LAT_CONFIGS))
def test_backward_on_the_lattice(name, bilinear):
    """Integer dout.  The points with 1, 2 or 4 valid views alone: every term is exact, the gradient equals autograd's in float64 bit for
    bit.  The whole lattice (1/3 occurs): the project's own per-element bound.  Unhit pixels exactly +0.0 in both."""
    from tests.test_gpu_point_sample_grad import _grad, check_bound
    pts, proj, kw, pre = U.lattice_case(name)
    C = 65
    shape = (3, C, U.LAT_H, U.LAT_W)
    dout = U.integer_dout(len(pts), C)
    zeros = np.zeros(shape, np.float32)
    _, nv, want = U.ref_point_sample_grad(pts, zeros, proj, dout, bilinear=bilinear, pre=pre, **kw)
    got, vn = _backward(pts, proj, pre, kw, bilinear, dout, shape)
    assert np.array_equal(vn.cpu().numpy(), nv)
    k, S, _ = _index_terms(pts, proj, pre, kw, bilinear, dout, shape)
    g = got.cpu().numpy()
    empty = np.broadcast_to(k == 0, g.shape)
    assert empty.any() and (g[empty].view(np.int32) == 0).all(), "an unhit pixel is not exactly +0.0"
    check_bound(g, want, k, S, f"lattice gradient {name} {'bilinear' if bilinear else 'nearest'}", require_max_k=3)
    exact = np.isin(nv, (1, 2, 4))
    assert exact.sum() > 60
    _, _, want1 = U.ref_point_sample_grad(pts[exact], zeros, proj, dout[exact], bilinear=bilinear, pre=pre, **kw)
    got1, _ = _backward(pts[exact], proj, pre, kw, bilinear, dout[exact], shape)
    _same_bits(got1, want1, f"lattice gradient, {int(exact.sum())} points with 1 / 2 valid views")
    # the autograd node gives the raw call's bits
    _, api = _grad(torch.zeros(shape, device="cuda"), _t(pts), _t(proj), _t(dout), **_api_kw(kw, pre, bilinear))
    assert torch.equal(api, got)


def _points_on_pixels(counts, W, shift=(0, 0), H=None):
    """``counts``: {(py, px): n}.  n distinct points that project EXACTLY onto image position (4 px (+-1 on a border column / row so
    that the view stays valid), 4 py) at depths 1 + j / 256.  Returns (N,3) fp32 in list order."""
    out = []
    for (py, px), n in counts.items():
        x = 4.0 * px + (1.0 if px == 0 else -1.0 if px == W - 1 else 0.0) - shift[0]
        y = 4.0 * py + (1.0 if py == 0 else -1.0 if H is not None and py == H - 1 else 0.0) - shift[1]
        for j in range(n):
            z = 1.0 + j / 256.0
            out.append((x * z, y * z, z))
    return np.array(out, np.float32).reshape(-1, 3)


LIST_LENGTHS = {(1, 1): 1, (2, 3): 32, (3, 5): 33, (4, 7): 64, (5, 9): 65, (6, 11): 129, (7, 13): 0}


@pytest.mark.parametrize("order", ["descending", "shuffled"])
@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_backward_list_lengths(bilinear, order):
    """Lists of exactly 0, 1, 32, 33, 64, 65 and 129 points on chosen pixels of one view: the one-lane and the wave path of k_psb_order
    (32 | 33) and the first and second trip of k_point_sample_grad's entry loop (64 | 65, 129).  One valid view and integer dout:
    exact, bit for bit; the lengths are asserted on the CPU."""
    from tests.test_gpu_point_sample_grad import check_bound
    H, W, C = U.LAT_H, U.LAT_W, 70
    kw = dict(scale=(1.0, 1.0), crop=(0.0, 0.0), flip=False, ori_w=64.0, pad_hw=U.LAT_PAD)
    pts = _points_on_pixels(LIST_LENGTHS, W, H=H)
    perm = np.arange(len(pts))[::-1] if order == "descending" else np.random.default_rng(4).permutation(len(pts))
    pts = np.ascontiguousarray(pts[perm])
    proj = U.shift_proj([(0, 0)])
    shape = (1, C, H, W)
    dout = U.integer_dout(len(pts), C)
    k, S, nv = _index_terms(pts, proj, None, kw, bilinear, dout, shape)
    assert (nv == 1).all()
    for (py, px), n in LIST_LENGTHS.items():
        assert int(k[0, 0, py, px]) == n, ((py, px), int(k[0, 0, py, px]), n)
    _, _, want = U.ref_point_sample_grad(pts, np.zeros(shape, np.float32), proj, dout, bilinear=bilinear, **kw)
    got, vn = _backward(pts, proj, None, kw, bilinear, dout, shape)
    assert (vn == 1).all()
    check_bound(got.cpu().numpy(), want, k, S, f"list lengths {order} {'bilinear' if bilinear else 'nearest'}", require_max_k=129)
    _same_bits(got, want, "list lengths")


def _dyadic_kw(H, W):
    return dict(scale=(1.0, 1.0), crop=(0.0, 0.0), flip=False, ori_w=4.0 * (W - 1), pad_hw=(4.0 * (H - 1), 4.0 * (W - 1)))


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_backward_scan_chunk_edge_on_a_dyadic_map(bilinear):
    """33 x 65: lists on pixels 2 047 and 2 048, the last of the first scan chunk and the first of the second."""
    H, W, C = 33, 65, 3
    kw = _dyadic_kw(H, W)
    counts = {(2047 // W, 2047 % W): 3, (2048 // W, 2048 % W): 5, (0, 0): 2, (H - 1, W - 1): 2}
    pts = _points_on_pixels(counts, W, H=H)
    proj = U.shift_proj([(0, 0)])
    shape = (1, C, H, W)
    dout = U.integer_dout(len(pts), C)
    k, _, nv = _index_terms(pts, proj, None, kw, False, dout, shape)
    assert (nv == 1).all() and all(int(k[0, 0, py, px]) == n for (py, px), n in counts.items())
    _, _, want = U.ref_point_sample_grad(pts, np.zeros(shape, np.float32), proj, dout, bilinear=bilinear, **kw)
    got, _ = _backward(pts, proj, None, kw, bilinear, dout, shape)
    _same_bits(got, want, "33 x 65")


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("V,H,W", [(1, 23, 89), (2, 32, 32)])
def test_backward_scan_sentinel_entry(V, H, W, bilinear):
    """D + 1 = 2 048 (one full chunk) and D + 1 = 2 049 (the sentinel entry psb_start(D) alone in the second chunk).  Maps whose sizes
    are no powers of two; the image positions are multiples of pad / 128, so the geometry is still exact (ties included) and float64
    takes the same decisions; dout is random, so the sums round: the project's own per-element bound against autograd in float64."""
    from tests.test_gpu_point_sample_grad import check_bound
    assert V * H * W + 1 == (2048 if V == 1 else 2049)
    rng = np.random.default_rng(H)
    N, C = 700, 5
    kw = _dyadic_kw(H, W)
    jx, jy, z = rng.integers(-6, 135, N), rng.integers(-6, 135, N), rng.choice([0.5, 1.0, 2.0], N)
    cx, cy = (W - 1) * jx / 32.0, (H - 1) * jy / 32.0                     # cx / pad_w = jx / 128
    shifts = [(0, 0), ((W - 1) / 4.0, -(H - 1) / 4.0)][:V]
    # three points on the LAST pixel of the LAST view, whose list length is psb_start(D) - psb_start(D - 1): 255 / 256 of the padded
    # size rounds to pixel (H - 1, W - 1) and is still inside the image (valid)
    lx, ly = (W - 1) * 255 / 64.0 - shifts[-1][0], (H - 1) * 255 / 64.0 - shifts[-1][1]
    cx, cy, z = np.append(cx, [lx] * 3), np.append(cy, [ly] * 3), np.append(z, [0.5, 1.0, 2.0])
    N += 3
    pts = np.stack([cx * z, cy * z, z], 1).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), np.stack([cx * z, cy * z, z], 1))
    proj = U.shift_proj(shifts)
    shape = (V, C, H, W)
    dout = rng.standard_normal((N, C)).astype(np.float32)
    _, nv, want = U.ref_point_sample_grad(pts, np.zeros(shape, np.float32), proj, dout, bilinear=bilinear, **kw)
    k, S, nvi = _index_terms(pts, proj, None, kw, bilinear, dout, shape)
    assert np.array_equal(nv, nvi)
    got, vn = _backward(pts, proj, None, kw, bilinear, dout, shape)
    assert np.array_equal(vn.cpu().numpy(), nv)
    g = got.cpu().numpy()
    assert (g[np.broadcast_to(k == 0, g.shape)].view(np.int32) == 0).all()
    assert k[-1, 0, H - 1, W - 1] >= 3 and nv[-3:].min() >= 1, "no list on the last pixel of the last view"
    check_bound(g, want, k, S, f"V={V} {H} x {W} {'bilinear' if bilinear else 'nearest'}", require_max_k=2)


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("V", [1, 2])
def test_backward_scan_carry_past_256_chunks(V, bilinear):
    """513 x 1025 maps, C = 2: 257 (V = 1) and 514 (V = 2) chunks of 2 048, so k_psb_scan_top's carry loop makes two and three trips.
    Lists in the first chunk, on both sides of the chunk edges 255 / 256 / 257 (and 512 / 513 with two views) and on the last pixel of
    the last view; dyadic, exact: bit for bit against autograd in float64."""
    H, W, C = 513, 1025, 2
    HW = H * W
    kw = _dyadic_kw(H, W)
    shifts = [(0, 0), (8, 8)][:V]
    edges = [5, 255 * 2048 - 1, 255 * 2048, 256 * 2048 - 1, 256 * 2048]
    if V == 2:
        edges += [257 * 2048 - 1, 257 * 2048, 512 * 2048 - 1, 512 * 2048, 513 * 2048 - 1, 513 * 2048]
    edges.append(V * HW - 1)
    assert -(-(V * HW + 1) // 2048) == (257 if V == 1 else 514)
    parts, flat = [], {}
    for i, d in enumerate(edges):
        v, pix = divmod(d, HW)
        n = 1 + i % 3
        parts.append(_points_on_pixels({(pix // W, pix % W): n}, W, shifts[v], H=H))
        flat[d] = n
    pts = np.concatenate(parts)
    proj = U.shift_proj(shifts)
    shape = (V, C, H, W)
    dout = U.integer_dout(len(pts), C)
    _, nv, want = U.ref_point_sample_grad(pts, np.zeros(shape, np.float32), proj, dout, bilinear=bilinear, **kw)
    assert set(np.unique(nv)) <= {1, 2} and (nv > 0).all()
    kn = (U.ref_point_sample_grad(pts, np.zeros((V, 1, H, W), np.float32), proj, nv[:, None].astype(np.float64), **kw)[2]).reshape(-1)
    for d, n in flat.items():
        assert kn[d] >= n, (d, kn[d], n)                      # (nearest lists: at least the points aimed there)
    got, vn = _backward(pts, proj, None, kw, bilinear, dout, shape)
    assert np.array_equal(vn.cpu().numpy(), nv)
    _same_bits(got, want, f"V={V} 513 x 1025")
    print(f"carry loop V={V} {'bilinear' if bilinear else 'nearest'}: {-(-(V * HW + 1) // 2048)} chunks, bit-equal, "
          f"{int((want != 0).sum())} non-zero elements")


# ================================================================================================================== level join
JOIN_B = 64


def _join_case(V, bilinear, seed):
    """64 scenes with 0 .. 5 rows of the lattice as integer coordinates (voxel size 0.25), the scenes differing in flip / scale / crop /
    pre-transform and in their cameras' shifts; rows with 1, 2, 4, ... (a power of two) or no valid view, so that integer gradients
    are exact.  Two rows inside scenes 5 and 40 carry the scene indices -1 and 64."""
    rng = np.random.default_rng(seed)
    names = list(U.LAT_CONFIGS)
    scenes, coords, ends = [], [], []
    total = 0
    for b in range(JOIN_B):
        name = names[b % 4]
        cfg = U.LAT_CONFIGS[name]
        pts = U.lattice_points()
        pre = U.LAT_PRE if cfg["pre"] else None
        if pre is not None:
            pts = U.undo_pre(pts)
        shifts = U.lattice_shifts(V)
        shifts = shifts[b % V:] + shifts[:b % V]
        proj = U.shift_proj(shifts)
        kw = dict(scale=cfg["scale"], crop=cfg["crop"], flip=cfg["flip"], ori_w=cfg["ori_w"], pad_hw=U.LAT_PAD)
        _, nv = U.ref_point_sample(pts, np.zeros((V, 1, U.LAT_H, U.LAT_W)), proj, bilinear=bilinear, pre=pre, **kw)
        ok = np.nonzero((nv == 0) | ((nv & (nv - 1)) == 0))[0]
        seen = np.nonzero((nv > 0) & ((nv & (nv - 1)) == 0))[0]
        nrows = (b * 7) % 6
        nseen = 2 if b in (5, 40) else min(nrows, 1)           # (5, 40: the row that gets a scene index outside the tables is SEEN)
        pick = np.concatenate([rng.choice(seen, nseen, replace=False), rng.choice(ok, nrows - nseen, replace=False)])
        ci = np.rint(pts[pick] * 4).astype(np.int32)
        assert np.array_equal(ci.astype(np.float32) * np.float32(0.25), pts[pick])
        rows = np.concatenate([np.full((len(ci), 1), b, np.int32), ci], 1)
        if b in (5, 40):
            # under its range's scene this row would be sampled and counted: only the scene index makes it zero
            assert nrows >= 2 and nv[pick[1]] > 0
            rows[1, 0] = -1 if b == 5 else JOIN_B
        coords.append(rows)
        total += nrows
        ends.append(total)
        scenes.append(dict(proj=proj, pre=pre, kw=kw, scal=(kw["scale"][0], kw["scale"][1], kw["crop"][0], kw["crop"][1], kw["flip"],
                                                             kw["ori_w"], kw["pad_hw"][0], kw["pad_hw"][1])))
    return scenes, np.concatenate(coords), ends


@pytest.mark.parametrize("V,Cw,bilinear,dtype", [(3, 64, False, torch.float32), (3, 64, True, torch.bfloat16), (65, 64, False, torch.float16),
                                                   (65, 64, True, torch.float32), (3, 512, False, torch.float32), (3, 512, True, torch.float32),
                                                   (65, 512, False, torch.bfloat16), (65, 512, True, torch.float32)])
def test_level_join_at_64_scenes_against_float64(V, Cw, bilinear, dtype):
    """join_level_features' two library calls, forward and backward, against [level.feats | reference64] and autograd's gradient in
    float64: B = 64 with empty scenes, widths (64, 64) and (512, 512), 3 and 65 views, and two rows whose scene index lies outside the
    tables (zeros in the image columns, valid_num 0, nothing added to any map's gradient, dlevel_feats still g[:, :Cb])."""
    from proxytransformation_amd.fusion import JoinTables, join_level_features, prepare_features_many
    from proxytransformation_amd.backbone import SparseLevel
    _abi, lib = _lib()
    scenes, coords, ends = _join_case(V, bilinear, seed=V + Cw)
    n, B, Cb, Ci, H, W = len(coords), JOIN_B, Cw, Cw, U.LAT_H, U.LAT_W
    ld = Cb + Ci
    assert ends[-1] == n and 0 in np.diff([0] + ends) and n > 100
    pool = [U.integer_maps(V, Ci, seed=100 + j) for j in range(4)]
    img = torch.stack([_t(pool[(b // 4) % 4]) for b in range(B)]).to(dtype)
    rng = np.random.default_rng(9)
    feats = rng.standard_normal((n, Cb)).astype(np.float32)
    g = np.concatenate([rng.standard_normal((n, Cb)).astype(np.float32), U.integer_dout(n, Ci, seed=V)], 1)
    tables = JoinTables([s["proj"] for s in scenes], [None if s["pre"] is None else torch.from_numpy(s["pre"]) for s in scenes],
                        [s["scal"] for s in scenes], 0.25, "cuda", aligned=bilinear)
    # the reference, scene by scene
    want = np.zeros((n, ld), np.float32)
    want[:, :Cb] = feats
    want_vn = np.zeros(n, np.int64)
    want_grads = []
    outside = np.nonzero((coords[:, 0] < 0) | (coords[:, 0] >= B))[0]
    assert len(outside) == 2
    for b, (s, e) in enumerate(zip([0] + ends[:-1], ends)):
        rows = np.arange(s, e)
        rows = rows[coords[rows, 0] == b]
        sc = scenes[b]
        if len(rows) == 0:
            want_grads.append(None)
            continue
        pts = coords[rows, 1:].astype(np.float32) * np.float32(0.25)
        o, nv, df = U.ref_point_sample_grad(pts, pool[(b // 4) % 4], sc["proj"], g[rows, Cb:], bilinear=bilinear, pre=sc["pre"], **sc["kw"])
        want[rows, Cb:] = o
        want_vn[rows] = nv
        want_grads.append(df)
    assert (want_vn > 0).sum() > 50
    cd, fd, gd = _t(coords), _t(feats), _t(g)
    prepared = prepare_features_many([img[b] for b in range(B)])
    ptrs = (ctypes.c_void_p * B)(*[p.data_ptr() for p in prepared])

    def run():
        out = torch.full((n * ld + TAIL,), -7.5, device="cuda")
        vn = torch.full((n + TAIL,), -7, dtype=torch.int32, device="cuda")
        _abi.check(lib.ptx_level_join(cd.data_ptr(), n, fd.data_ptr(), Cb, ptrs, tables.host.ctypes.data, tables.dev.data_ptr(), B, V, Ci,
                                      H, W, 0.25, 1 if bilinear else 0, out.data_ptr(), vn.data_ptr(), _stream()), "ptx_level_join")
        df = torch.full((n * Cb + TAIL,), -7.5, device="cuda")
        di = torch.full((img.numel() + TAIL,), -7.5, device="cuda").to(dtype)
        rows = max(e - s for s, e in zip([0] + ends[:-1], ends))
        nbytes = lib.ptx_level_join_bwd_workspace_bytes(rows, V, H, W, 1 if bilinear else 0)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        _abi.check(lib.ptx_level_join_bwd(cd.data_ptr(), n, (ctypes.c_int32 * B)(*ends), gd.data_ptr(), Cb, vn.data_ptr(),
                                          tables.host.ctypes.data, tables.dev.data_ptr(), B, V, Ci, H, W, 0.25, 1 if bilinear else 0,
                                          df.data_ptr(), di.data_ptr(), _DT[dtype], ws.data_ptr(), ws.numel(), _stream()),
                   "ptx_level_join_bwd")
        torch.cuda.synchronize()
        return out, vn, df, di
    out, vn, df, di = _twice(run)
    assert (out[n * ld:] == -7.5).all() and (vn[n:] == -7).all() and (df[n * Cb:] == -7.5).all() and (di[img.numel():] == -7.5).all()
    _same_bits(out[:n * ld].view(n, ld), want, "join forward")
    assert np.array_equal(vn[:n].cpu().numpy(), want_vn)
    o = out[:n * ld].view(n, ld).cpu().numpy()
    assert (o[outside, Cb:].view(np.int32) == 0).all() and (want_vn[outside] == 0).all()
    _same_bits(df[:n * Cb].view(n, Cb), g[:, :Cb], "dlevel_feats")
    dimg = di[:img.numel()].view(img.shape).float().cpu().numpy()
    for b in range(B):
        w = np.zeros((V, Ci, H, W)) if want_grads[b] is None else want_grads[b]
        if dtype == torch.float32:
            _same_bits(torch.from_numpy(dimg[b]), w, f"dimg of scene {b}")
        else:                                             # one rounding on the 16-bit store, of an exact fp32 value
            w16 = torch.from_numpy(w.astype(np.float32)).to(dtype).float().numpy()
            assert np.array_equal(dimg[b].view(np.int32), w16.view(np.int32)), f"dimg of scene {b}"
    # the API gives the raw calls' bits
    lv = SparseLevel(feats=fd.clone().requires_grad_(), coords=cd, scene_rows=ends, tensor_stride=1)
    im = img.clone().requires_grad_()
    res = join_level_features(lv, im, tables)
    res.backward(gd)
    assert torch.equal(res.detach(), out[:n * ld].view(n, ld)) and torch.equal(im.grad, di[:img.numel()].view(img.shape))
    print(f"level join B=64 V={V} widths ({Cb}, {Ci}) {'bilinear' if bilinear else 'nearest'} {dtype}: bit-equal, {n} rows, "
          f"{int((want_vn > 0).sum())} seen")
