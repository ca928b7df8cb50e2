"""The rule of the geometry-edge tests has teeth (no GPU): on the exact lattice and on the voxel boundaries the fp32 restatements the
device is pinned to (oracle.point_sample, hit_index, oracle.voxelize) agree bit for bit with references written from the definitions
(tests/geometry_edges_util.py: float64 torch, torch's own fp32 floor(p / vs)) -- and a restatement that is wrong in ONE decision does
not: each deliberately wrong variant below (written here only) fails a case, and the test names it.  The preconditions are asserted
too: the inputs really sit on the decisions they claim (floor(fl(k vs) / vs) != k occurs; every lattice class is non-empty)."""
import numpy as np
import pytest

from tests import geometry_edges_util as U


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------ restatements
def _sample32(points, feats, proj, *, scale, crop, flip, ori_w, pad_hw, bilinear=False, wrong=None):
    """batch_point_sample in the fp32 steps of oracle.point_sample; ``wrong`` changes ONE decision:
    half_up | valid_le | depth_ge | no_clamp | sum_valid.  Returns (out (N,C) fp32, nvalid)."""
    from oracle.oracle import _f32, _fma32
    p, f, P = _f32(points), _f32(feats), _f32(proj)
    V, C, H, W = f.shape
    N = len(p)
    pad_h, pad_w = np.float32(pad_hw[0]), np.float32(pad_hw[1])
    one, two = np.float32(1), np.float32(2)
    acc = np.zeros((N, C), np.float32)
    nvalid = np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        for v in range(V):
            q = []
            for r in range(3):
                t = p[:, 0] * P[v, r, 0]
                t = _fma32(p[:, 1], np.full(N, P[v, r, 1], np.float32), t)
                t = _fma32(p[:, 2], np.full(N, P[v, r, 2], np.float32), t)
                q.append(t + P[v, r, 3])
            z = q[2] if wrong == "no_clamp" else np.maximum(q[2], np.float32(1e-3))
            cx = (q[0] / z) * np.float32(scale[0]) - np.float32(crop[0])
            cy = (q[1] / z) * np.float32(scale[1]) - np.float32(crop[1])
            if flip:
                cx = np.float32(ori_w) - cx
            fx = ((cx / pad_w * two - one + one) / two) * np.float32(W - 1)
            fy = ((cy / pad_h * two - one + one) / two) * np.float32(H - 1)
            if wrong == "valid_le":
                valid = (cx <= pad_w) & (cx >= 0) & (cy <= pad_h) & (cy >= 0) & (q[2] > 0)
            elif wrong == "depth_ge":
                valid = (cx < pad_w) & (cx > 0) & (cy < pad_h) & (cy > 0) & (q[2] >= 0)
            else:
                valid = (cx < pad_w) & (cx > 0) & (cy < pad_h) & (cy > 0) & (q[2] > 0)
            if not bilinear:
                rnd = (lambda a: np.floor(a + np.float32(0.5))) if wrong == "half_up" else np.rint
                ix, iy = rnd(fx), rnd(fy)
                inb = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
                xi, yi = np.where(inb, ix, 0).astype(np.int64), np.where(inb, iy, 0).astype(np.int64)
                s = np.where(inb[:, None], f[v][:, yi, xi].T, np.float32(0))
            else:
                x0, y0 = np.floor(fx), np.floor(fy)
                wx1, wy1 = fx - x0, fy - y0
                wx0, wy0 = one - wx1, one - wy1
                s = np.zeros((N, C), np.float32)
                for dx, dy, w in ((0, 0, wx0 * wy0), (1, 0, wx1 * wy0), (0, 1, wx0 * wy1), (1, 1, wx1 * wy1)):
                    xx, yy = x0 + dx, y0 + dy
                    ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
                    xi, yi = np.where(ok, xx, 0).astype(np.int64), np.where(ok, yy, 0).astype(np.int64)
                    s = s + np.where(ok[:, None], f[v][:, yi, xi].T * w[:, None].astype(np.float32), np.float32(0))
            if wrong == "sum_valid":
                s = np.where(valid[:, None], s, np.float32(0))
            acc = acc + s
            nvalid += valid
    out = acc / np.maximum(nvalid, 1)[:, None].astype(np.float32)
    out[nvalid == 0] = 0
    return out, nvalid


def _voxel32(outs, voxel_size, wrong=None):
    """oracle.voxelize's statement; ``wrong``: trunc | reciprocal | last.  Returns coords, feats, inverse list."""
    vs = np.float32(voxel_size)
    coords, feats = [], []
    for b, p in enumerate(outs):
        p = np.ascontiguousarray(p, np.float32)
        q = p * (np.float32(1) / vs) if wrong == "reciprocal" else p / vs
        v = (np.trunc(q) if wrong == "trunc" else np.floor(q)).astype(np.int32)
        coords.append(np.concatenate([np.full((len(p), 1), b, np.int32), v], 1))
        feats.append(p)
    coords, feats = np.concatenate(coords), np.concatenate(feats)
    n = len(coords)
    order = np.arange(n)[::-1] if wrong == "last" else np.arange(n)
    _, first, inv = np.unique(coords[order], axis=0, return_index=True, return_inverse=True)
    keep = np.sort(order[first])
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(order[first])] = np.arange(len(first))
    inverse = np.empty(n, np.int32)
    inverse[order] = rank[inv.reshape(-1)]
    sizes = np.cumsum([0] + [len(p) for p in outs])
    return coords[keep], feats[keep], [inverse[sizes[b]:sizes[b + 1]] for b in range(len(outs))]


def _voxel_outs(cloud, voxel_size):
    """Two scenes: the boundary cloud, and the cloud backwards followed by every point moved a quarter voxel up (at 0.25 exactly the
    same voxels again, with other features: duplicates whose representative matters)."""
    return [cloud, np.concatenate([cloud[::-1], cloud + np.float32(voxel_size / 4)])]


# the points beside the lattice that carry the depth decisions: (row, what the rule says)
def _depth_points():
    """depth exactly 0 and -0.0 with an in-map projection (the clamp puts x / 1e-3 inside the image: sampled, never valid), and a
    positive depth below the clamp (valid, projected with 1e-3 rather than with its own depth)."""
    return np.array([[0.008, 0.008, 0.0], [0.008, 0.008, -0.0], [0.004, 0.004, 1e-4]], np.float32)


def _lattice_run(fn, name, bilinear, extra=None, **kw_fn):
    pts, proj, kw, pre = U.lattice_case(name)
    if extra is not None:
        pts = np.concatenate([pts, extra])
    feats = U.integer_maps(3, 5)
    return fn(U.apply_pre32(pts, pre), feats, proj, bilinear=bilinear, **kw, **kw_fn), (pts, feats, proj, kw, pre)


# ------------------------------------------------------------------------------------------------------------------ what must pass
@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("name", list(U.LAT_CONFIGS))
def test_restatements_equal_the_float64_reference_on_the_lattice(name, bilinear):
    from oracle import oracle
    from tests.test_gpu_point_sample_grad import bound_terms, hit_index
    extra = _depth_points() if name in ("plain", "flip") and not bilinear else None       # (bilinear weights off the lattice round)
    (o32, nv32), (pts, feats, proj, kw, pre) = _lattice_run(oracle.point_sample, name, bilinear, extra)
    ref, nv = U.ref_point_sample(pts, feats, proj, bilinear=bilinear, pre=pre, **kw)
    assert np.array_equal(nv32, nv)
    assert np.array_equal(_bits(o32), _bits(ref.numpy()))
    (mine, nv_mine), _ = _lattice_run(_sample32, name, bilinear, extra)
    assert np.array_equal(_bits(mine), _bits(o32)) and np.array_equal(nv_mine, nv)      # the unmutated variant IS the restatement
    # hit_index (the backward's restatement): its exact float64 gradient is autograd's
    dout = U.integer_dout(len(pts), 5)
    _, _, want = U.ref_point_sample_grad(pts, feats, proj, dout, bilinear=bilinear, pre=pre, **kw)
    n, d, w, nvi = hit_index(pts, proj, U.LAT_H, U.LAT_W, bilinear=bilinear, pre=pre,
                             **{k: kw[k] for k in ("scale", "crop", "flip", "ori_w", "pad_hw")})
    _, _, E = bound_terms(n, d, w, nvi, dout, feats.shape)
    assert np.array_equal(nvi, nv)
    exact = np.isin(nv, (1, 2, 4))
    assert exact.sum() > 100
    assert np.abs(E - want).max() <= 2.0 ** -40 * np.abs(want).max()                    # 1/3 is the only inexact factor
    n_, d_, w_, _ = hit_index(pts[exact], proj, U.LAT_H, U.LAT_W, bilinear=bilinear, pre=pre,
                              **{k: kw[k] for k in ("scale", "crop", "flip", "ori_w", "pad_hw")})
    _, _, E1 = bound_terms(n_, d_, w_, nv[exact], dout[exact], feats.shape)
    _, _, want1 = U.ref_point_sample_grad(pts[exact], feats, proj, dout[exact], bilinear=bilinear, pre=pre, **kw)
    assert np.array_equal(E1, want1)                                                    # counts 1, 2, 4: exact


@pytest.mark.parametrize("voxel_size", U.VOXEL_SIZES)
def test_voxel_restatement_equals_torch_on_the_boundaries(voxel_size):
    from oracle import oracle
    cloud, _ = U.boundary_cloud(voxel_size)
    outs = _voxel_outs(cloud, voxel_size) + [np.zeros((5, 3), np.float32)]
    c, f, inv, _ = U.ref_voxelize(outs, voxel_size)
    rc, rf, rinv = oracle.voxelize(outs, voxel_size)
    assert np.array_equal(c, rc) and np.array_equal(_bits(f), _bits(rf))
    assert all(np.array_equal(a, b) for a, b in zip(inv, rinv))
    mc, mf, minv = _voxel32(outs, voxel_size)
    assert np.array_equal(mc, rc) and np.array_equal(_bits(mf), _bits(rf)) and all(np.array_equal(a, b) for a, b in zip(minv, rinv))


# ------------------------------------------------------------------------------------------------------------------ preconditions
def test_the_inputs_sit_on_the_decisions():
    misses = {vs: U.floor_misses(vs) for vs in U.VOXEL_SIZES}
    print("floor(fl(k vs) / vs) != k for k in [-3000, 3000):", misses)
    assert misses[0.01] > 0 and misses[0.02] > 0 and misses[0.05] > 0 and misses[0.25] == 0
    for vs in U.VOXEL_SIZES:
        v = U.boundary_values(vs)
        vox = np.floor(v / np.float32(vs))
        assert vox[-3] == 0 and vox[-2] == -1 and vox[-1] == 0 and np.signbit(v[-3])          # -0.0, -denormal, +denormal
    for name in ("plain", "flip", "pre"):
        c = U.lattice_classes(name)
        print(f"lattice classes {name}:", c)
        for k in ("tie_even_down", "tie_even_up", "ix_minus_half", "ix_top_half", "cx_zero_other_valid", "cx_pad_other_valid",
                  "sampled_not_valid", "one_outside", "none_valid"):
            assert c[k] > 0, (name, k)
        assert all(h > 0 for h in c["nvalid_hist"])
    c = U.lattice_classes("aug")
    print("lattice classes aug:", c)
    assert c["tie_even_down"] > 0 and c["tie_even_up"] > 0 and c["sampled_not_valid"] > 0 and all(h > 0 for h in c["nvalid_hist"])
    for V in (64, 65, 128, 129):
        c = U.lattice_classes("plain", V)
        counts = [i for i, h in enumerate(c["nvalid_hist"]) if h]
        print(f"lattice, {V} views: valid views per point {counts[0]} .. {counts[-1]}, one step outside {c['one_outside']}")
        assert counts[-1] >= 3 and counts[-1] < V and len(counts) >= 3 and c["one_outside"] > 0 and c["sampled_not_valid"] > 0


def test_margin_of_the_generic_case_is_measured_here_and_leaves_enough_points():
    """The margin (4 x the largest pixel-coordinate difference between the fp32 restatement and float64, CPU only) and the share of
    the generic case's points it leaves out: at most 5 %."""
    margin, worst, near = U.generic_margin()
    print(f"generic case: largest |ix32 - ix64| = {worst:.3g} px, margin = {margin:.3g} px, in-map pairs within 1e-3 px of a half "
          f"pixel: {100 * near:.2f} %")
    assert 0 < worst < 1e-3
    for bilinear in (False, True):
        _, H, W, pts, proj = U.generic_scene(U.GENERIC_SEED)
        _, _, g = U.ref_point_sample(pts, np.zeros((3, 1, H, W)), proj, geometry=True, bilinear=bilinear, **U.GENERIC_KW)
        keep = U.generic_keep(g, H, W, U.GENERIC_KW["pad_hw"], margin, bilinear)
        print(f"generic case {'bilinear' if bilinear else 'nearest'}: left out {100 * (1 - keep.mean()):.2f} % of {len(pts)} points")
        assert 1 - keep.mean() <= 0.05
        # the restatement alone keeps the rule on the kept points: same valid counts, same pixels
        fx, fy = U.restated_pixels32(pts[keep], proj, H, W, **U.GENERIC_KW)
        rnd = np.floor if bilinear else np.rint
        near_map = (g["ix"][:, keep] > -2) & (g["ix"][:, keep] < W + 1) & (g["iy"][:, keep] > -2) & (g["iy"][:, keep] < H + 1)
        assert np.array_equal(rnd(fx)[near_map], rnd(g["ix"][:, keep])[near_map])
        assert np.array_equal(rnd(fy)[near_map], rnd(g["iy"][:, keep])[near_map])


# ------------------------------------------------------------------------------------------------------------------ what must fail
WRONG_SAMPLING = {
    # wrong decision: (configuration, bilinear, what differs, the class of points it differs on)
    "half_up": ("plain", False, "out", "ties at x.5 with an even pixel below (ix = 0.5, 2.5: half to even rounds down)"),
    "valid_le": ("plain", False, "nvalid", "cx exactly 0 and exactly pad_w (sampled, not counted)"),
    "depth_ge": ("plain", False, "nvalid", "depth exactly 0 and -0.0 (clamped into the image, not valid)"),
    "no_clamp": ("plain", False, "out", "the point at depth 1e-4 (projected with 1e-3)"),
    "sum_valid": ("plain", False, "out", "a view that samples at cx = 0 / pad_w while another view is valid"),
}


@pytest.mark.parametrize("wrong", list(WRONG_SAMPLING))
def test_a_wrong_sampling_decision_fails_the_lattice(wrong):
    name, bilinear, what, where = WRONG_SAMPLING[wrong]
    (out, nv), (pts, feats, proj, kw, pre) = _lattice_run(_sample32, name, bilinear, _depth_points(), wrong=wrong)
    ref, nv64 = U.ref_point_sample(pts, feats, proj, bilinear=bilinear, pre=pre, **kw)
    bad_rows = np.nonzero((_bits(out) != _bits(ref.numpy())).any(1) | (nv != nv64))[0]
    print(f"{wrong}: {len(bad_rows)} of {len(pts)} rows differ -- {where}")
    assert len(bad_rows) > 0, f"the lattice does not notice '{wrong}'"
    if what == "nvalid":
        assert (nv != nv64).any()
    n_lat = len(U.lattice_points())
    if wrong in ("depth_ge", "no_clamp"):                     # carried by the depth points alone
        assert (bad_rows >= n_lat).all() and set(bad_rows - n_lat) == ({0, 1} if wrong == "depth_ge" else {2})
    else:
        assert (bad_rows < n_lat).all()
        if wrong == "half_up":                                 # every differing row has a tie in some view
            g = U.ref_point_sample(pts, feats, proj, pre=pre, geometry=True, **kw)[2]
            tie = ((g["ix"] - np.floor(g["ix"]) == 0.5) | (g["iy"] - np.floor(g["iy"]) == 0.5)).any(0)
            assert tie[bad_rows].all()


WRONG_VOXEL = {
    "trunc": (0.25, "every negative coordinate that is no multiple of the voxel size"),
    "reciprocal": (0.01, "boundary points fl(k vs) and their neighbours where p * (1 / vs) and p / vs floor differently"),
    "last": (0.25, "voxels with more than one point: the LAST one's features"),
}


@pytest.mark.parametrize("wrong", list(WRONG_VOXEL))
def test_a_wrong_voxel_decision_fails_the_boundaries(wrong):
    vs, where = WRONG_VOXEL[wrong]
    cloud, _ = U.boundary_cloud(vs)
    outs = _voxel_outs(cloud, vs)
    c, f, inv, _ = U.ref_voxelize(outs, vs)
    mc, mf, minv = _voxel32(outs, vs, wrong)
    same = mc.shape == c.shape and np.array_equal(mc, c) and np.array_equal(_bits(mf), _bits(f)) and \
        all(np.array_equal(a, b) for a, b in zip(minv, inv))
    print(f"{wrong} at voxel size {vs}: rows {len(mc)} against {len(c)} -- {where}")
    assert not same, f"the boundary cloud does not notice '{wrong}'"
    if wrong == "last":
        assert np.array_equal(mc[np.lexsort(mc.T[::-1])], c[np.lexsort(c.T[::-1])])          # same voxels, other representatives
