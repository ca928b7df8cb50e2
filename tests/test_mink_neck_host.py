"""The sparse neck (proxytransformation_amd/neck.py, neck_host.py) pinned without a GPU: the numpy restatements in float64 against
torch's own ``conv_transpose3d`` / ``grid_sample`` / ``topk``, the union order on a hand-written case, the ``state_dict`` of the shipped
``MinkNeck`` against a fixture of the reference's names and shapes, the ABI surface of the new entry points, the inference-only and
no-CPU-path raises, the near-tie count of the end-to-end inputs of tests/test_gpu_mink_neck.py and tests/test_gpu_neck_regimes.py, and
the preconditions of the latter's inputs (tests/neck_util.py): what makes each of its cases reach the branch it is there for."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import MODELS, REGISTRY_BACKEND, MinkNeck, _abi, neck, neck_host, sparse
from proxytransformation_amd.backbone import SparseLevel
from tests import neck_util as nu
from tests import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, ref, tol=1e-12):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64
    assert float(np.abs(got - ref).max()) <= tol * float(np.abs(ref).max()), float(np.abs(got - ref).max())


# ------------------------------------------------------------------------------------------------------------------ restatements
def test_transposed_convolution_restatement_is_torch_conv_transpose3d():
    """A dense 4x4x4 block at tensor stride 2: the children fill an 8x8x8 grid; torch's kernel (Cin, Cout, kD, kH, kW) is ours reshaped
    by the x-fastest rule, j = (dz * 2 + dy) * 2 + dx."""
    rng = np.random.default_rng(11)
    cin, cout = 5, 7
    cells = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(64)]
    coords = np.concatenate([np.zeros((64, 1), np.int64), cells * 2], 1).astype(np.int32)
    x, kernel = rng.standard_normal((64, cin)), rng.standard_normal((8, cin, cout))
    oc, ends, out = neck_host.conv_transpose_gen_host(coords, [64], 2, x, kernel)
    assert ends == [512] and oc.dtype == np.int32 and len({tuple(r) for r in oc.tolist()}) == 512
    assert np.array_equal(oc[8:16] - coords[1], np.concatenate([np.zeros((8, 1), int), sparse.kernel_offsets(2, 1)], 1))
    dense = np.zeros((1, cin, 4, 4, 4))                          # (N, C, D=z, H=y, W=x)
    dense[0][:, cells[:, 2], cells[:, 1], cells[:, 0]] = x.T
    w = torch.from_numpy(kernel.reshape(2, 2, 2, cin, cout)).permute(3, 4, 0, 1, 2)          # [dz, dy, dx, ci, co] -> (ci, co, dz, dy, dx)
    ref = F.conv_transpose3d(torch.from_numpy(dense), w.contiguous(), stride=2)[0].numpy()
    _close(out, ref[:, oc[:, 3], oc[:, 2], oc[:, 1]].T)
    scale, shift = rng.uniform(0.5, 1.5, cout), rng.standard_normal(cout)
    elu = neck_host.conv_transpose_gen_host(coords, [64], 2, x, kernel, scale, shift, neck_host.ACT_ELU)[2]
    _close(elu, F.elu(torch.from_numpy(out * scale + shift)))
    assert (elu < 0).mean() > 0.2
    with pytest.raises(ValueError, match="tensor_stride"):
        neck_host.conv_transpose_gen_host(coords, [64], 1, x, kernel)


def test_interpolation_restatement_is_grid_sample_with_absent_voxels_zero():
    rng = np.random.default_rng(12)
    ts, G = 4, 5
    cells = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), -1).reshape(-1, 3)
    present = cells[rng.permutation(len(cells))[:70]]
    s_coords = np.concatenate([np.zeros((70, 1), np.int64), present * ts], 1).astype(np.int32)
    scores = rng.standard_normal(70)
    dense = np.zeros((1, 1, G, G, G))
    dense[0, 0, present[:, 2], present[:, 1], present[:, 0]] = scores
    q = np.stack(np.meshgrid(*[np.arange(2 * G - 1)] * 3, indexing="ij"), -1).reshape(-1, 3) * (ts // 2)     # every half-stride point
    q_coords = np.concatenate([np.zeros((len(q), 1), np.int64), q], 1).astype(np.int32)
    got = neck_host.prune_scores_host(q_coords, s_coords, [70], ts, scores)
    grid = torch.from_numpy(q / (ts * (G - 1)) * 2 - 1).reshape(1, -1, 1, 1, 3)              # (x, y, z) in [-1, 1], align_corners
    ref = F.grid_sample(torch.from_numpy(dense), grid, mode="bilinear", align_corners=True).reshape(-1).numpy()
    _close(got, ref, 1e-12)
    assert (got == 0).sum() > 0 and got.dtype == np.float64
    other = neck_host.prune_scores_host(np.array([[1, 4, 4, 4]], np.int32), s_coords, [70, 70], ts, scores)
    assert other[0] == 0.0                                   # another scene: no corner present
    neg = neck_host.prune_scores_host(np.array([[0, -2, 0, 0]], np.int32), np.array([[0, -4, 0, 0], [0, 0, 0, 0]], np.int32), [2], ts,
                                      np.array([1.0, 3.0], np.float32))
    assert neg.dtype == np.float32 and neg[0] == 2.0         # floor division below zero: corners -4 and 0, half each


def test_topk_restatement_is_torch_topk_and_fixes_ties():
    rng = np.random.default_rng(13)
    s = rng.permutation(1000).astype(np.float64) - 300.5     # tie-free
    ends = [400, 400, 405, 1000]
    for k in (1, 100, 400, 700):
        keep = neck_host.topk_keep_host(s, ends, k)
        lo = 0
        for hi in ends:
            idx = torch.topk(torch.from_numpy(s[lo:hi]), min(hi - lo, k)).indices.numpy()
            ref = np.zeros(hi - lo, bool)
            ref[idx] = True
            assert np.array_equal(keep[lo:hi], ref)
            lo = hi
        assert neck_host.topk_scene_rows(ends, k) == np.cumsum([min(n, k) for n in (400, 0, 5, 595)]).tolist()
    v = np.array([1.0, 0.0, -0.0, 2.0, 0.0, -0.0, -1.0, 0.0], np.float32)
    assert neck_host.topk_keep_host(v, [8], 4).tolist() == [True, True, True, True, False, False, False, False]      # -0.0 == +0.0, lower index
    assert neck_host.topk_keep_host(v, [8], 5).tolist() == [True, True, True, True, True, False, False, False]
    assert neck_host.topk_keep_host(v.astype(np.float64), [8], 4).tolist() == neck_host.topk_keep_host(v, [8], 4).tolist()
    w = np.array([np.inf, np.nan, -np.inf, 0.0, -np.nan], np.float32)
    w[4] = np.float32(np.nan).view(np.uint32).__or__(np.uint32(1 << 31)).view(np.float32)        # a NaN with the sign bit set
    key = neck_host.topk_key(w)
    assert key[1] > key[0] > key[3] > key[2] > key[4]        # +NaN above +inf, -NaN below -inf: documented, restated by the kernel
    c, e, f = neck_host.prune_host(np.array([True, False, True, True]), np.arange(16).reshape(4, 4), [1, 4], np.arange(8.).reshape(4, 2))
    assert e == [1, 3] and c[:, 0].tolist() == [0, 8, 12] and f[:, 0].tolist() == [0., 4., 6.]


def test_union_order_on_six_rows():
    a = np.array([[0, 0, 0, 0], [0, 4, 0, 0], [1, 0, 0, 0]], np.int32)
    b = np.array([[0, 8, 0, 0], [0, 4, 0, 0], [0, -4, 0, 0], [1, 0, 4, 0], [1, 0, 0, 0], [1, 4, 4, 4]], np.int32)
    fa, fb = np.array([[1.], [2.], [3.]]), np.array([[10.], [20.], [30.], [40.], [50.], [60.]])
    c, e, f = neck_host.union_add_host(a, [2, 3], fa, b, [3, 6], fb)
    assert e == [4, 7] and c.dtype == np.int32
    assert c.tolist() == [[0, 0, 0, 0], [0, 4, 0, 0], [0, 8, 0, 0], [0, -4, 0, 0], [1, 0, 0, 0], [1, 0, 4, 0], [1, 4, 4, 4]]
    assert f[:, 0].tolist() == [1., 22., 10., 30., 53., 40., 60.]
    c2, e2, f2 = neck_host.union_add_host(a[:0], [0, 0], fa[:0], b, [3, 6], fb)      # A empty: B in its order
    assert e2 == [3, 6] and np.array_equal(c2, b) and np.array_equal(f2, fb)


def test_head_and_activation_restatements():
    rng = np.random.default_rng(14)
    x, w, b = rng.standard_normal((9, 64)), rng.standard_normal((64, 3)), rng.standard_normal((1, 3))
    cls, score = neck_host.head_host(x, w, b)
    _close(cls, x @ w + b)
    assert np.array_equal(score, cls.max(1))
    v = np.array([-2.0, -0.0, 0.0, 3.0])
    assert np.array_equal(neck_host.act_host(v, 0), v) and np.array_equal(neck_host.act_host(v, 1), np.maximum(v, 0))
    _close(neck_host.act_host(v, 2), F.elu(torch.from_numpy(v)))
    with pytest.raises(ValueError, match="act"):
        neck_host.act_host(v, 3)


# ------------------------------------------------------------------------------------------------------------------ the module
def test_state_dict_is_the_reference_layout():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "mink_neck_state_dict.json")))
    assert len(want) == 62
    m = MinkNeck(num_classes=1, in_channels=[128, 256, 512, 1024], out_channels=256, voxel_size=0.01, pts_prune_threshold=1000)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want
    sd = {k: torch.randn(*shape) if shape else torch.tensor(3) for k, shape in want}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.up_block_3[0].kernel, sd["up_block_3.0.kernel"]) and not list(m.up_block_1[2].parameters())
    m.init_weights()
    assert float(m.conv_cls.bias.detach()[0, 0]) == pytest.approx(-math.log(99)) and abs(float(m.conv_cls.kernel.detach().std()) - 0.01) < 0.003
    assert tuple(MinkNeck(3, [64, 128], 128, 0.02, 10).state_dict()["conv_cls.kernel"].shape) == (1, 128, 3)
    with pytest.raises(ValueError, match="num_classes"):
        MinkNeck(17, [64, 128], 128, 0.02, 10)
    if REGISTRY_BACKEND != "embodiedscan":
        assert MODELS.get("MinkNeck") is MinkNeck
        built = MODELS.build(dict(type="MinkNeck", num_classes=1, in_channels=[64, 128], out_channels=64, voxel_size=0.01, pts_prune_threshold=5))
        assert isinstance(built, MinkNeck) and built.pts_prune_threshold == 5


def test_header_binding_and_exports_declare_the_neck_entry_points():
    lib = _abi.lib()
    hooks = ctypes.CDLL(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip_testhooks.so"))
    for name, params in su.assert_declared(nu.NECK_ENTRY_POINTS).items():
        assert len(params.split(",")) == len(_abi.SIGNATURES[name][1]), name
        getattr(hooks, name)
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13 and hooks.ptx_abi_version() == 13
    assert "neck.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()
    ws = lib.ptx_neck_workspace_bytes
    assert ws(6, 20000, 40000) > ws(6, 20000, 0) > 0 and ws(0, 1, 1) == 0 and ws(65, 1, 1) == 0 and ws(1, 0, 1) == 0 and ws(1, 1, -1) == 0


def test_argument_checks_answer_einval_before_touching_a_device():
    lib = _abi.lib()
    EINVAL = -1
    ends = lambda *e: (ctypes.c_int32 * len(e))(*e)          # noqa: E731
    conv = lambda cin, cout, act=2: lib.ptx_sparse_conv3d_act(None, 10, None, 10, 27, None, cin, cout, None, None, None, None, act, None, None)  # noqa: E731
    assert conv(1040, 64) == EINVAL and b"Cin=1040" in lib.ptx_last_error() and b"up to 1024" in lib.ptx_last_error()
    assert conv(1024, 96) == EINVAL and b"Cout=96" in lib.ptx_last_error()
    assert conv(64, 64, act=3) == EINVAL and b"act=3" in lib.ptx_last_error()
    assert conv(1024, 64) == EINVAL and b"null" in lib.ptx_last_error()          # the widths pass
    old = lib.ptx_sparse_conv3d(None, 10, None, 10, 27, None, 1024, 64, None, None, None, None, 0, None, None)
    assert old == EINVAL and b"ptx_sparse_conv3d: Cin=1024" in lib.ptx_last_error() and b"up to 512;" in lib.ptx_last_error()
    gen = lambda ts, cin, cout, n=10: lib.ptx_sparse_conv_transpose_gen(None, n, ts, None, None, cin, cout, None, None, 2, None, None, None)  # noqa: E731
    assert gen(1, 64, 64) == EINVAL and b"tensor_stride=1" in lib.ptx_last_error()
    assert gen(2, 1040, 64) == EINVAL and b"Cin=1040" in lib.ptx_last_error()
    assert gen(2, 64, 96) == EINVAL and b"Cout=96" in lib.ptx_last_error()
    assert gen(2, 1024, 512) == EINVAL and b"null" in lib.ptx_last_error() and gen(2, 1024, 512, n=0) == 0
    head = lambda C, K: lib.ptx_neck_head(None, 10, C, None, None, K, None, None, None)      # noqa: E731
    assert head(256, 17) == EINVAL and b"num_classes=17" in lib.ptx_last_error()
    assert head(100, 1) == EINVAL and b"C=100" in lib.ptx_last_error() and head(256, 1) == EINVAL and b"null" in lib.ptx_last_error()
    union = lambda a, b, ts=4, C=128: lib.ptx_neck_union_add(None, a, None, None, b, None, 2, ts, C, None, None, None, None, None, 0, None)  # noqa: E731
    assert union(ends(5, 3), ends(1, 2)) == EINVAL and b"a_scene_end must not decrease" in lib.ptx_last_error()
    assert union(ends(1, 2), ends(1, 2), ts=3) == EINVAL and b"tensor_stride=3" in lib.ptx_last_error()
    assert union(ends(1, 2), ends(1, 2), C=6) == EINVAL and b"C=6" in lib.ptx_last_error()
    assert union(ends(1, 2), None) == EINVAL and b"b_scene_end is null" in lib.ptx_last_error()
    topk = lambda k: lib.ptx_neck_topk_prune(None, ends(4), 1, k, None, None, 64, None, None, None, None)      # noqa: E731
    assert topk(0) == EINVAL and b"k=0" in lib.ptx_last_error() and topk(3) == EINVAL and b"null" in lib.ptx_last_error()
    assert lib.ptx_neck_prune_scores(None, 5, None, ends(4), 1, 6, None, None, None, 0, None) == EINVAL and b"tensor_stride=6" in lib.ptx_last_error()


def test_neck_is_inference_only_and_has_no_cpu_path():
    x = torch.zeros(4, 64)
    km = sparse.KernelMap(coords=torch.zeros(4, 4, dtype=torch.int32), scene_rows=[4], nbr=torch.zeros(4, 27, dtype=torch.int32), kernel_size=3,
                          stride=1, tensor_stride=1, n_in=4)
    w = torch.zeros(27, 64, 64)
    with pytest.raises(ValueError, match="elu and relu"):
        sparse.sparse_conv3d(x, km, w, relu=True, elu=True)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_conv3d(x.clone().requires_grad_(), km, w, elu=True, differentiable=True)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_conv3d(x.clone().requires_grad_(), km, w, elu=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.sparse_conv3d(x, km, w, elu=True)
    c = torch.zeros(4, 4, dtype=torch.int32)
    for call in (lambda t: neck.conv_transpose_gen(c, [4], 2, t, torch.zeros(8, 64, 64)),
                 lambda t: neck.union_add(c, [4], t, c, [4], x, 2),
                 lambda t: neck.prune_scores(c, c, [4], 2, t[:, 0]),
                 lambda t: neck.topk_prune(x[:, 0], c, [4], t, 2),
                 lambda t: neck.neck_head(t, torch.zeros(1, 64, 1))):
        with pytest.raises(NotImplementedError, match="backward"):
            call(x.clone().requires_grad_())
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(x)
    m = MinkNeck(1, [64, 128], 64, 0.01, 5)
    levels = [SparseLevel(torch.zeros(4, 64), c, [4], 8), SparseLevel(torch.zeros(4, 128), c, [4], 16)]
    with pytest.raises(NotImplementedError, match="inference-only"):
        with torch.no_grad():
            m(levels, 1)                                     # BatchNorms in training mode
    m.eval()
    with pytest.raises(NotImplementedError, match="backward"):
        m(levels, 1)                                         # its parameters require grad
    with pytest.raises(RuntimeError, match="no CPU path"):
        with torch.no_grad():
            m(levels, 1)
    with pytest.raises(ValueError, match="levels expected"):
        with torch.no_grad():
            m(levels[:1], 1)


# ------------------------------------------------------------------------------------------------------------------ the end-to-end inputs
def test_end_to_end_inputs_have_few_near_ties():
    """The inputs of tests/test_gpu_mink_neck.py's end-to-end test: pruning is active at every step, the zero score of rows without a
    present corner sits at the threshold of the later steps, and at most 2 % of k rows per scene lie within the near-tie margin of the
    step's k-th score (``neck_util.near_ties``: exact ties excluded, they are decided by the row index on both sides).  If this fails,
    change the seed of ``neck_util.e2e_levels``, not the cap."""
    levels, m = nu.e2e_levels(), nu.e2e_neck()
    trace = []
    feats, scores, points = m.forward_host(levels, 3, np.float64, trace=trace)
    assert len(trace) == 3 and [len(f) for f in feats] == [64 + 3 * 150, 64 + 3 * 150, 1 + 8 + 64 + 150]
    zero_threshold = 0
    for step in trace:
        ties = nu.near_ties(step["scores"], step["scene_rows"], nu.K_PRUNE)
        assert len(ties) >= 2                                # the two large scenes are pruned at every step
        for scene, count, kth in ties:
            print(f"rows {step['scene_rows']} scene {scene}: k-th score {kth:+.4f}, {count} near-ties")
            assert count <= 0.02 * nu.K_PRUNE, (scene, count)
            zero_threshold += kth == 0.0
        assert (step["scores"] > 0).any() and (step["scores"] < 0).any()
    assert zero_threshold >= 2
    assert all(p.dtype == np.float32 and p.shape == (f.shape[0], 3) for p, f in zip(points, feats))
    assert all(s.shape == (f.shape[0], 1) and float((s < 0).mean()) > 0.5 for s, f in zip(scores, feats))


def test_second_end_to_end_inputs_have_few_near_ties():
    """The inputs of tests/test_gpu_neck_regimes.py's end-to-end test (``neck_util.e2e_levels_b`` / ``e2e_neck_b``: three classes, k = 520,
    scenes of 1500 / 0 / 40 / 600 rows), under the same cap of 2 % of k near-ties per step and scene.  The float64 chain gives, per step,
    the rows before the prune and the near-ties of the pruned scenes: step 0: 64 / 0 / 8 / 512 rows, nothing pruned; step 1: 512 / 0 / 64
    / 4096, scene 3 pruned, 0 near-ties; step 2: 4096 / 0 / 512 / 4673, scenes 0 and 3 pruned, 0 and 0 near-ties.  The empty scene stays
    empty, the 40-row scene is never pruned, the 600-row scene is pruned at two of the three steps.  If this fails, change the seed of
    ``neck_util.e2e_levels_b``, not the cap."""
    levels, m = nu.e2e_levels_b(), nu.e2e_neck_b()
    assert m.num_classes == 3 and m.pts_prune_threshold == nu.K_PRUNE_B
    trace = []
    feats, scores, points = m.forward_host(levels, 4, np.float64, trace=trace)
    pruned = []
    for step in trace:
        ends = [0] + step["scene_rows"]
        print("rows", np.diff(ends).tolist())
        ties = nu.near_ties(step["scores"], step["scene_rows"], nu.K_PRUNE_B)
        pruned.append([scene for scene, _, _ in ties])
        assert ends[2] == ends[1] and 0 < ends[3] - ends[2] <= nu.K_PRUNE_B
        for scene, count, kth in ties:
            print(f"scene {scene}: k-th score {kth:+.4f}, {count} near-ties")
            assert count <= 0.02 * nu.K_PRUNE_B, (scene, count)
    assert pruned == [[], [3], [0, 3]]
    assert len(feats[1]) == 0 and len(feats[2]) == 1 + 8 + 64 + 512 and len(feats[3]) == 64 + 512 + 2 * nu.K_PRUNE_B
    assert all(s.shape == (f.shape[0], 3) and p.shape == (f.shape[0], 3) for s, f, p in zip(scores, feats, points))
    best = np.concatenate(scores).argmax(axis=1)
    assert all((best == c).mean() > 0.1 for c in range(3))   # the maximum over the classes matters


# ------------------------------------------------------------------------------------------------------------------ the regimes' inputs
@pytest.mark.parametrize("kind", ["positive", "negative", "mixed", "normal"])
def test_low_byte_scores_split_in_the_last_two_radix_passes(kind):
    """``neck_util.radix_trace`` restates the four passes; in the low-byte inputs the passes at shift 8 and 0 each see >= 2 occupied
    digits at every k of the device test (N(0, 1): the passes at shift 24 and 16), and the traced threshold is the k-th largest key."""
    nu.check_low_byte_passes(kind)
    if kind == "positive":                                   # the existing test's 16 levels, by contrast, are decided after two passes
        levels = np.linspace(-1.0, 1.0, 16).astype(np.float32)[np.random.default_rng(12).integers(0, 16, 2000)]
        assert all(p[0] == 1 for p in nu.radix_trace(levels, 0, 2000, 100)[0][2:])


def test_special_scores_put_the_threshold_where_they_say():
    s, ks = nu.special_scores()
    key = np.sort(neck_host.topk_key(s))[::-1]
    pos_nan = neck_host.topk_key(np.array([0x7F800001], np.uint32).view(np.float32))[0]
    at = lambda x: int(neck_host.topk_key(np.array([x], np.float32))[0])      # noqa: E731
    assert int(key[ks["+inf"] - 1]) == at(np.inf) and key[ks["+inf"] - 2] == pos_nan and key[1] > key[2]
    assert int(key[ks["-inf"] - 1]) == at(-np.inf) and int(key[ks["zero"] - 1]) == at(0.0) == at(-0.0) == 1 << 31
    assert int(key[ks["+denormal"] - 1]) == (1 << 31) + 0x1234 and int(key[ks["-denormal"] - 1]) == 0x7FFFFFFF - 0x1234
    for k in (ks["+inf"], ks["zero"], ks["-inf"]):            # ties straddle these thresholds: the lower row index wins
        keep = neck_host.topk_keep_host(s, [len(s)], k)
        tied = neck_host.topk_key(s) == key[k - 1]
        assert 0 < keep[tied].sum() < tied.sum() and keep[tied][0] and not keep[tied][-1]
    assert np.isnan(s).sum() == 4 and (np.abs(s[np.isfinite(s)]) < 1.2e-38).sum() == 10


def test_union_regime_inputs_hold_every_scene_kind():
    a, a_ends, b, b_ends = nu.union_regime_case()
    kinds = nu.union_kinds(a, a_ends, b, b_ends)
    assert kinds == [nu.UNION_KINDS[i % 7] for i in range(64)] and len(b) > len(a)
    a, a_ends, b, b_ends = nu.union_key_range_case()
    c, e, _ = neck_host.union_add_host(a, a_ends, np.ones((len(a), 4), np.float32), b, b_ends, np.ones((len(b), 4), np.float32))
    assert e == [6, 9] and c[:, 1:].max() == 4 << 18 and c[:, 1:].min() == -(4 << 18) and c[5].tolist() == [0, 0, 0, 4 << 18]
    assert len(nu.union_key_range_case(True)[0]) == 7


@pytest.mark.parametrize("ts", [8, 32768])
def test_score_queries_have_inexact_products(ts):
    corners = nu.check_score_query_case(ts)
    assert corners.shape[1] == 8
    for axis in range(3):                                    # the range-edge case: the host sees no alias
        q, s_coords, s_ends, scores = nu.score_edge_case(axis)
        ref = neck_host.prune_scores_host(q, s_coords, s_ends, 4, scores)
        assert (scores == 1e6).sum() == 1 and (0 < ref).all() and (ref < 10).all() and q[:, 1 + axis].min() > 4 * nu.M_VOX
    q, s_coords, s_ends, scores = nu.score_64_case()
    ref = neck_host.prune_scores_host(q, s_coords, s_ends, 2, scores)
    empty = np.diff([0] + s_ends)[q[:, 0]] == 0
    assert len(s_ends) == 64 and empty.sum() == 16 * 20 and (ref[empty] == 0).all() and (ref[~empty] != 0).mean() > 0.5
