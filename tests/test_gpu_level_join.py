"""Level join (``fusion.join_level_features`` -> ``ptx_level_join`` / ``ptx_level_join_bwd``, csrc/level_join.hip): DET:428-479 for one
backbone level and all scenes in one launch, held bit for bit to the route it replaces --

    forward   torch.cat([level.feats, torch.cat([batch_point_sample(...) per scene])], 1)
    backward  g[:, :Cb]  and, per scene, the standalone batch_point_sample backward on g[rows, Cb:]

-- on feature maps of 5 x 4 pixels.  Nothing here is a tolerance: both routes run the same rounded statements in the same order."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOXEL = 0.01
PAD = (96, 96)
H, W = 5, 4


def _scene_tables(B, V, seed):
    """Per scene: (V,4,4) projection matrices, a pre-transform or None, the eight scalars.  The scenes differ in flip, scale factor,
    crop offset and pre-transform; scene 0 has none of them."""
    rng = np.random.default_rng(seed)
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 40.0
    K[0, 2] = K[1, 2] = 48.0
    projs, pres, scal = [], [], []
    for b in range(B):
        P = np.empty((V, 4, 4), np.float32)
        for v in range(V):
            a = rng.uniform(-0.2, 0.2)
            E = np.eye(4, dtype=np.float32)
            E[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
            E[:3, 3] = np.array([-1.0, -1.0, 2.5], np.float32) + rng.uniform(-0.3, 0.3, 3).astype(np.float32)
            if V > 1 and v == V - 1:
                E[2, 3] = -50.0                       # a view behind which every point lies: never valid
            P[v] = K @ E
        projs.append(P)
        if b == 0:
            pres.append(None)
            scal.append((1.0, 1.0, 0.0, 0.0, False, float(PAD[1]), float(PAD[0]), float(PAD[1])))
        else:
            c, s = np.cos(0.1 * b), np.sin(0.1 * b)
            A = np.array([[c, -s, 0, 0.05 * b], [s, c, 0, -0.03 * b], [0, 0, 1.0 / (1.0 + 0.1 * b), 0.02]], np.float32)
            pres.append(torch.from_numpy(A))
            scal.append((1.0 + 0.1 * b, 1.0 - 0.05 * b, 3.0 * b, -2.0 * b, b % 2 == 1, float(PAD[1]) - 4.0 * b, float(PAD[0]),
                         float(PAD[1])))
    return projs, pres, scal


def _level(rows, Cb, seed):
    from proxytransformation_amd.backbone import SparseLevel
    rng = np.random.default_rng(seed)
    n = sum(rows)
    coords = np.zeros((n, 4), np.int32)
    ends, o = [], 0
    for b, nb in enumerate(rows):
        coords[o:o + nb, 0] = b
        coords[o:o + nb, 1:] = rng.integers(0, 25, (nb, 3)) * 8
        if nb >= 3:
            coords[o + 1, 1:] = (8, 8, -100000)          # behind every camera: no view sees this row
        o += nb
        ends.append(o)
    feats = rng.standard_normal((n, Cb)).astype(np.float32)
    return SparseLevel(feats=torch.from_numpy(feats).cuda(), coords=torch.from_numpy(coords).cuda(), scene_rows=ends, tensor_stride=8)


def _setup(rows, Cb, Ci, V, aligned, dtype, seed=0):
    from proxytransformation_amd.fusion import JoinTables
    B = len(rows)
    projs, pres, scal = _scene_tables(B, V, seed)
    level = _level(rows, Cb, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    img = torch.randn((B, V, Ci, H, W), generator=g).to(dtype).cuda()
    tables = JoinTables(projs, pres, scal, VOXEL, "cuda", aligned=aligned)
    return level, img, tables


def _reference(level, img, tables, g=None):
    """The route the join replaces: one batch_point_sample per scene, the concatenation over the scenes, the one over the channels;
    with ``g`` also the per-scene backward on g[rows, Cb:]."""
    from proxytransformation_amd.fusion import batch_point_sample
    Cb = level.feats.shape[1]
    lo = [0] + level.scene_rows[:-1]
    outs, dimg = [], []
    for b, (s, e) in enumerate(zip(lo, level.scene_rows)):
        pts = level.coords[s:e, 1:4].float() * VOXEL
        sw, sh, cw, ch, flip, ori_w, pad_h, pad_w, al = tables.scal[b]
        f = img[b].detach().clone().requires_grad_(g is not None)
        out = batch_point_sample(None, f, pts, tables.proj[b], "DEPTH", img_scale_factor=(sw, sh), img_crop_offset=(cw, ch),
                                 img_flip=bool(flip), img_pad_shape=(int(pad_h), int(pad_w)), img_shape=(int(pad_h), int(ori_w)),
                                 aligned=bool(al), pre_transform=tables.pre[b])
        if g is not None:
            out.backward(g[s:e, Cb:])
            dimg.append(f.grad)
        outs.append(out.detach())
    want = torch.cat([level.feats, torch.cat(outs)], 1)
    return (want, g[:, :Cb], torch.stack(dimg)) if g is not None else want


CASES = [
    # rows per scene, Cb, Ci, V, aligned, storage
    ((3, 0, 5), 64, 64, 3, False, torch.float32),
    ((1,), 64, 128, 1, True, torch.bfloat16),
    ((4, 257), 512, 512, 3, False, torch.float16),
    ((3, 0, 5), 64, 128, 65, True, torch.float32),
    ((4, 257), 64, 64, 65, False, torch.bfloat16),
    ((3, 0, 5), 512, 512, 3, True, torch.float32),
    ((1,), 64, 64, 3, False, torch.float16),
    ((4, 257), 64, 128, 1, True, torch.float16),
    # the pairs the rows above leave out: a one-row scene with the second pass of the view loop and with the widest rows, bf16 at the
    # widest rows, more than one work-group in fp32, the empty scene at the widest rows and 65 views
    ((1,), 512, 512, 65, False, torch.bfloat16),
    ((1,), 64, 128, 65, True, torch.float32),
    ((4, 257), 512, 512, 3, True, torch.bfloat16),
    ((4, 257), 64, 64, 3, False, torch.float32),
    ((3, 0, 5), 512, 512, 65, True, torch.float16),
    ((4, 257), 64, 128, 65, False, torch.float32),
]


def _valid_nums(level, img, tables):
    """``valid_num`` of the join's launch and of the per-scene launches it replaces."""
    from proxytransformation_amd import fusion
    B_ = img.shape[0]
    n = level.feats.shape[0]
    prepared = fusion.prepare_features_many([img[b] for b in range(B_)])
    got = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    fusion._join(level.feats, img, level.coords, tables, prepared, got)
    want = []
    for b, (s, e) in enumerate(zip([0] + level.scene_rows[:-1], level.scene_rows)):
        vn = torch.full((e - s,), -7, dtype=torch.int32, device="cuda")
        fusion._sample(img[b].contiguous(), prepared[b], level.coords[s:e, 1:4].float() * VOXEL, tables.proj[b], tables.pre[b], tables.scal[b], vn)
        want.append(vn)
    return got, torch.cat(want)


@pytest.mark.parametrize("rows,Cb,Ci,V,aligned,dtype", CASES)
def test_forward_and_backward_equal_the_per_scene_route_bit_for_bit(rows, Cb, Ci, V, aligned, dtype):
    from proxytransformation_amd.fusion import join_level_features
    level, img, tables = _setup(rows, Cb, Ci, V, aligned, dtype)
    n = sum(rows)
    g = torch.randn((n, Cb + Ci), generator=torch.Generator().manual_seed(7)).cuda()
    want, want_df, want_di = _reference(level, img, tables, g)

    plain = join_level_features(level, img, tables)                     # no grad: the plain forward
    assert plain.grad_fn is None and plain.shape == (n, Cb + Ci) and plain.dtype == torch.float32
    assert torch.equal(plain, want)
    sampled = plain[:, Cb:]
    assert sampled.abs().sum() > 0, "the case samples nothing: the geometry is off"
    vn, vn_want = _valid_nums(level, img, tables)
    assert torch.equal(vn, vn_want) and (vn >= 0).all() and (vn <= V).all() and (vn > 0).any()
    for b, (s, e) in enumerate(zip([0] + level.scene_rows[:-1], level.scene_rows)):
        if e - s >= 3:
            assert not sampled[s + 1].any() and int(vn[s + 1]) == 0, "a row that no view sees: zeros, valid_num 0"
            assert sampled[s].any() or sampled[s + 2].any()

    runs = []
    for _ in range(2):
        f = level.feats.detach().clone().requires_grad_()
        im = img.detach().clone().requires_grad_()
        lv = type(level)(feats=f, coords=level.coords, scene_rows=level.scene_rows, tensor_stride=level.tensor_stride)
        out = join_level_features(lv, im, tables)
        assert out.grad_fn is not None
        out.backward(g)
        runs.append((out.detach(), f.grad, im.grad))
    out, df, di = runs[0]
    assert torch.equal(out, want)
    assert df.shape == want_df.shape and torch.equal(df, want_df)
    assert di.shape == img.shape and di.dtype == dtype and torch.equal(di, want_di)
    assert di.float().abs().sum() > 0
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "two runs give equal bits"


def test_only_one_input_requires_grad():
    from proxytransformation_amd.fusion import join_level_features
    level, img, tables = _setup((3, 0, 5), 64, 64, 3, False, torch.float32)
    g = torch.randn((8, 128), generator=torch.Generator().manual_seed(3)).cuda()
    _, want_df, want_di = _reference(level, img, tables, g)
    im = img.detach().clone().requires_grad_()
    join_level_features(level, im, tables).backward(g)
    assert torch.equal(im.grad, want_di)
    f = level.feats.detach().clone().requires_grad_()
    lv = type(level)(feats=f, coords=level.coords, scene_rows=level.scene_rows, tensor_stride=8)
    join_level_features(lv, img, tables).backward(g)
    assert torch.equal(f.grad, want_df)


def test_prepared_workspaces_are_read_in_place():
    from proxytransformation_amd.fusion import join_level_features, prepare_features_many
    level, img, tables = _setup((4, 257), 64, 128, 3, False, torch.bfloat16)
    prepared = prepare_features_many([img[b] for b in range(2)])
    assert torch.equal(join_level_features(level, img, tables, prepared=prepared), _reference(level, img, tables))
    with pytest.raises(RuntimeError, match="prepared"):
        join_level_features(level, img, tables, prepared=prepared[:1])


def test_no_rows_launches_nothing_and_returns_the_shape():
    from proxytransformation_amd.fusion import join_level_features
    level, img, tables = _setup((0, 0), 64, 128, 3, False, torch.float32)
    out = join_level_features(level, img, tables)
    assert out.shape == (0, 192) and out.dtype == torch.float32
    f = level.feats.detach().clone().requires_grad_()
    im = img.detach().clone().requires_grad_()
    lv = type(level)(feats=f, coords=level.coords, scene_rows=level.scene_rows, tensor_stride=8)
    out = join_level_features(lv, im, tables)
    out.sum().backward()
    assert f.grad.shape == (0, 64) and im.grad.shape == img.shape and not im.grad.any()


def test_sentinels_behind_every_output_stay_intact():
    """The library calls themselves, with every output embedded in a larger buffer of sentinels."""
    from proxytransformation_amd import _abi
    from proxytransformation_amd.fusion import prepare_features_many
    rows, Cb, Ci, V = (4, 257), 64, 128, 3
    level, img, tables = _setup(rows, Cb, Ci, V, True, torch.float32)
    n, B, ld, tail = sum(rows), len(rows), Cb + Ci, 1024
    lib = _abi.lib()
    st = torch.cuda.current_stream().cuda_stream
    prepared = prepare_features_many([img[b] for b in range(B)])
    ptrs = (ctypes.c_void_p * B)(*[p.data_ptr() for p in prepared])
    out = torch.full((n * ld + tail,), -7.5, device="cuda")
    vn = torch.full((n + tail,), -7, dtype=torch.int32, device="cuda")
    _abi.check(lib.ptx_level_join(level.coords.data_ptr(), n, level.feats.data_ptr(), Cb, ptrs, tables.host.ctypes.data,
                                  tables.dev.data_ptr(), B, V, Ci, H, W, VOXEL, 1, out.data_ptr(), vn.data_ptr(), st), "ptx_level_join")
    assert torch.equal(out[:n * ld].view(n, ld), _reference(level, img, tables))
    assert (out[n * ld:] == -7.5).all() and (vn[n:] == -7).all()
    assert torch.equal(vn[:n], _valid_nums(level, img, tables)[1]) and int(vn[1]) == 0 and int(vn[5]) == 0      # the rows no view sees

    g = torch.randn((n, ld), generator=torch.Generator().manual_seed(5)).cuda()
    _, want_df, want_di = _reference(level, img, tables, g)
    df = torch.full((n * Cb + tail,), -7.5, device="cuda")
    di = torch.full((img.numel() + tail,), -7.5, device="cuda")
    nbytes = lib.ptx_level_join_bwd_workspace_bytes(max(rows), V, H, W, 1)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    _abi.check(lib.ptx_level_join_bwd(level.coords.data_ptr(), n, (ctypes.c_int32 * B)(*level.scene_rows), g.data_ptr(), Cb,
                                      vn.data_ptr(), tables.host.ctypes.data, tables.dev.data_ptr(), B, V, Ci, H, W, VOXEL, 1,
                                      df.data_ptr(), di.data_ptr(), 0, ws.data_ptr(), ws.numel(), st), "ptx_level_join_bwd")
    assert torch.equal(df[:n * Cb].view(n, Cb), want_df) and (df[n * Cb:] == -7.5).all()
    assert torch.equal(di[:img.numel()].view(img.shape), want_di) and (di[img.numel():] == -7.5).all()


def test_refusals_name_the_argument():
    from proxytransformation_amd.fusion import JoinTables, join_level_features
    level, img, tables = _setup((3, 0, 5), 64, 64, 3, False, torch.float32)
    with pytest.raises(ValueError, match="Ci=96"):
        join_level_features(level, torch.zeros((3, 3, 96, H, W), device="cuda"), tables)
    with pytest.raises(ValueError, match="B=2"):
        join_level_features(level, img[:2], tables)
    with pytest.raises(ValueError, match="V=2"):
        join_level_features(level, img[:, :2], tables)
    bad = type(level)(feats=level.feats, coords=level.coords, scene_rows=[3, 8], tensor_stride=8)
    with pytest.raises(ValueError, match="scene_rows"):
        join_level_features(bad, img, tables)
    projs, pres, scal = _scene_tables(2, 3, 0)
    with pytest.raises(ValueError, match="V is uniform"):
        JoinTables([projs[0], projs[1][:2]], pres, scal, VOXEL, "cuda")
    with pytest.raises(ValueError, match="pad_h"):
        JoinTables(projs, pres, [scal[0], scal[1][:6] + (0.0, 96.0)], VOXEL, "cuda")
