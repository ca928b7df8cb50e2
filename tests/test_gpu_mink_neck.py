"""The sparse neck on the device (proxytransformation_amd/neck.py; csrc/neck.hip and the neck instantiations of csrc/sparse.hip) held to
the numpy restatements of neck_host.py: bit for bit where the operation is exact (coordinates, ends, orders, the union's adds, the score
lookup, the prune), by ``sparse_util.hold`` (8 x the fp32 CPU chain's error against float64) where it sums."""
import numpy as np
import pytest
import torch

from proxytransformation_amd import _abi, neck, neck_host, sparse
from tests import neck_util as nu
from tests import sparse_util as su

pytestmark = pytest.mark.gpu
ELU = neck_host.ACT_ELU


_bits = nu.bits


# ------------------------------------------------------------------------------------------------------------------ convolution + ELU
@pytest.mark.parametrize("cin,cout,cut", [(1024, 64, 600), (128, 256, 0)])
def test_conv_elu(cin, cout, cut):
    """1024 -> 64 on 600 rows: 16 K-chunks per offset and a partial last tile; 128 -> 256 on all rows: an empty scene, a one-row scene,
    a row count off the 64-row tile.  The shift puts about half of the pre-activations below zero."""
    nbr = su.host_map(4, 3, 1, cut)[2]
    km = su.device_map(4, 3, 1, cut)
    ops = su.operands(nbr.shape[0], nbr.shape[0], cin, cout, 27, 7)
    use = ("scale", "shift")
    with torch.no_grad():
        got = sparse.sparse_conv3d(su.dev(ops["feats"]), km, su.dev(ops["weight"]), elu=True, **{u: su.dev(ops[u]) for u in use}).cpu().numpy()
    refs = [neck_host.sparse_conv3d_act_host(ops["feats"].astype(dt), nbr, ops["weight"].astype(dt), scale=ops["scale"].astype(dt),
                                             shift=ops["shift"].astype(dt), act=ELU) for dt in (np.float32, np.float64)]
    assert 0.3 < float((refs[1] < 0).mean()) < 0.7 and refs[0].dtype == np.float32
    su.hold(f"conv+ELU {cin}->{cout}", got, refs[0], refs[1])


def test_selector_relu_gives_the_old_entry_points_bits():
    nbr = su.host_map(4, 3, 1)[2]
    km = su.device_map(4, 3, 1)
    ops = su.operands(nbr.shape[0], nbr.shape[0], 128, 64, 27, 8)
    old = su.conv_run(km, ops, ("bias", "scale", "shift", "residual"), relu=True)
    f, w = su.dev(ops["feats"]), su.dev(ops["weight"])
    vec = {u: su.dev(ops[u]) for u in ("bias", "scale", "shift", "residual")}
    new = torch.empty_like(old)
    _abi.check(_abi.lib().ptx_sparse_conv3d_act(f.data_ptr(), f.shape[0], km.nbr.data_ptr(), km.nbr.shape[0], 27, w.data_ptr(), 128, 64,
                                                vec["bias"].data_ptr(), vec["scale"].data_ptr(), vec["shift"].data_ptr(),
                                                vec["residual"].data_ptr(), 1, new.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "ptx_sparse_conv3d_act")
    assert float((old == 0).float().mean()) > 0.2
    _bits(new, old.cpu().numpy())
    r32, r64 = su.conv_refs(nbr, ops, ("bias", "scale", "shift", "residual"), relu=True)
    su.hold("conv+ReLU 128->64", old.cpu().numpy(), r32, r64)                # the old entry point, after the change


# ------------------------------------------------------------------------------------------------------------------ transposed convolution
@pytest.mark.parametrize("cin,cout,cut", [(64, 64, 0), (1024, 512, 70)])
def test_generative_transposed_convolution(cin, cout, cut):
    rows, ends = su.rows(8)
    if cut:
        rows, ends = rows[:cut], (cut,)
    rng = np.random.default_rng(9)
    x = rng.standard_normal((rows.shape[0], cin)).astype(np.float32)
    kernel = (rng.standard_normal((8, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    scale, shift = rng.uniform(0.5, 1.5, cout).astype(np.float32), (rng.standard_normal(cout) * 0.5).astype(np.float32)
    with torch.no_grad():
        oc, oe, out = neck.conv_transpose_gen(su.dev(rows), list(ends), 8, su.dev(x), su.dev(kernel), su.dev(scale), su.dev(shift), ELU)
    c32, e32, r32 = neck_host.conv_transpose_gen_host(rows, list(ends), 8, x, kernel, scale, shift, ELU)
    r64 = neck_host.conv_transpose_gen_host(rows, list(ends), 8, x.astype(np.float64), kernel.astype(np.float64), scale.astype(np.float64),
                                            shift.astype(np.float64), ELU)[2]
    assert oe == e32 and out.shape[0] == 8 * rows.shape[0] and (cut == 0 or out.shape[0] == 560)
    _bits(oc, c32)
    assert 0.3 < float((r64 < 0).mean()) < 0.7
    su.hold(f"generative conv {cin}->{cout}", out.cpu().numpy(), r32, r64)


# ------------------------------------------------------------------------------------------------------------------ union, scores, prune
def _union_operands():
    a, a_ends, b, b_ends = nu.union_case()
    rng = np.random.default_rng(10)
    return a, a_ends, rng.standard_normal((a.shape[0], 128)).astype(np.float32), b, b_ends, rng.standard_normal((b.shape[0], 128)).astype(np.float32)


def test_union_add():
    a, a_ends, fa, b, b_ends, fb = _union_operands()
    c, e, f = neck_host.union_add_host(a, a_ends, fa, b, b_ends, fb)
    both = len(a) + len(b) - len(c)
    # rows in both, rows only in B; the empty scene stays empty; the one-row scene's row is among B's children of its parent
    assert both > 300 and len(c) - len(a) > 300 and a_ends[2] == a_ends[1] and e[2] == e[1] and e[3] - e[2] == b_ends[3] - b_ends[2] > 8
    with torch.no_grad():
        for _ in range(2):                                   # the second call: same bits (no atomics on floats, no stale workspace)
            gc, ge, gf = neck.union_add(su.dev(a), a_ends, su.dev(fa), su.dev(b), b_ends, su.dev(fb), 4)
            assert ge == e
            _bits(gc, c)
            _bits(gf, f)


def test_prune_scores():
    a, a_ends, _, b, b_ends, _ = _union_operands()
    q, q_ends, _ = neck_host.union_add_host(a, a_ends, np.zeros((len(a), 1), np.float32), b, b_ends, np.zeros((len(b), 1), np.float32))
    s_coords, s_ends, _ = sparse.kernel_map_host(a, a_ends, 4, 1, 2)         # the score rows: A's parents (tensor stride 8)
    scores = np.random.default_rng(11).standard_normal(len(s_coords)).astype(np.float32)
    ref = neck_host.prune_scores_host(q, s_coords, s_ends, 8, scores)
    index = {tuple(r) for r in s_coords.tolist()}
    corners = np.array([sum((int(r[0]), *(int(v) // 8 * 8 + int(d) for v, d in zip(r[1:], off))) in index
                            for off in sparse.kernel_offsets(2, 8)) for r in q])
    assert (corners == 0).any() and (corners == 1).any() and (corners == 8).any() and (ref > 0).any() and (ref < 0).any()
    assert ref.dtype == np.float32 and (ref[corners == 0] == 0).all()
    with torch.no_grad():
        got = neck.prune_scores(su.dev(q), su.dev(s_coords), s_ends, 8, su.dev(scores))
    _bits(got, ref)


def test_topk_prune():
    rows, ends = su.rows(4)
    ends = list(ends)
    rng = np.random.default_rng(12)
    levels = np.linspace(-1.0, 1.0, 16).astype(np.float32)
    levels[7], levels[8] = -0.0, 0.0                          # +-0.0 among the 16 levels
    scores = levels[rng.integers(0, 16, rows.shape[0])]
    feats = rng.standard_normal((rows.shape[0], 64)).astype(np.float32)
    n1 = ends[1] - ends[0]                                    # the random scene's row count
    for k in (1, 100, 1000, n1, n1 + 5):                     # (1000: the threshold of the random scene is the zero level, both signs)
        keep = neck_host.topk_keep_host(scores, ends, k)
        c, e, f = neck_host.prune_host(keep, rows, ends, feats)
        assert e == neck_host.topk_scene_rows(ends, k)
        if k == 1000:
            at = keep[ends[0]:ends[1]] != (scores[ends[0]:ends[1]] > 0)
            z = scores[ends[0]:ends[1]][at]
            assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
        if k == 100:                                         # ties straddle the threshold
            kth = np.sort(scores[ends[0]:ends[1]])[::-1][k - 1]
            at = scores[ends[0]:ends[1]] == kth
            assert 0 < keep[ends[0]:ends[1]][at].sum() < at.sum()
        with torch.no_grad():
            for _ in range(2):
                gc, ge, gf, gk = neck.topk_prune(su.dev(scores), su.dev(rows), ends, su.dev(feats), k)
                assert ge == e and np.array_equal(gk.cpu().numpy(), keep)
                _bits(gc, c)
                _bits(gf, f)
    zeros = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -0.0], np.float32)          # signed zeros AT the threshold: the lower index wins
    with torch.no_grad():
        gk = neck.topk_prune(su.dev(zeros), su.dev(rows[:6]), [6], su.dev(feats[:6]), 3)[3]
    assert gk.cpu().numpy().tolist() == neck_host.topk_keep_host(zeros, [6], 3).tolist() == [True, True, False, False, True, False]


@pytest.mark.parametrize("K", [1, 3])
def test_head(K):
    rng = np.random.default_rng(13)
    n = 2317
    x = rng.standard_normal((n, 256)).astype(np.float32)
    w, b = (rng.standard_normal((1, 256, K)) / 16).astype(np.float32), rng.standard_normal((1, K)).astype(np.float32)
    with torch.no_grad():
        cls, score = neck.neck_head(su.dev(x), su.dev(w), su.dev(b))
    cls, score = cls.cpu().numpy(), score.cpu().numpy()
    r32 = neck_host.head_host(x, w[0], b)[0]
    r64 = neck_host.head_host(x.astype(np.float64), w[0].astype(np.float64), b.astype(np.float64))[0]
    assert cls.shape == (n, K) and score.shape == (n,)
    su.hold(f"head 256->{K}", cls, r32, r64)
    assert np.array_equal(score.view(np.uint32), cls.max(axis=1).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_shipped_configuration():
    """(a) ``forward`` against ``forward_host(keep=the device's masks)``: row sets, order and points bit for bit, feats and scores by
    ``hold``; (b) per pruning step the device's mask and the host's own float64 mask differ only on rows within ``NEAR_TIE * max |score|``
    of the step's k-th score, and on no more rows than that step and scene has near-ties (``neck_util.near_ties``, which the host test caps at
    2 % of k)."""
    nu.end_to_end(nu.e2e_levels(), nu.e2e_neck(), 3, nu.K_PRUNE)             # (the protocol is shared with tests/test_gpu_neck_regimes.py)


# ------------------------------------------------------------------------------------------------------------------ raises
def test_refused_widths_name_their_numbers():
    c = torch.zeros(8, 4, dtype=torch.int32, device=su.DEV)
    km = sparse.kernel_map(torch.arange(32, dtype=torch.int32, device=su.DEV).reshape(8, 4) * 4, [8], 4, 3, 1)
    z = lambda *shape: torch.zeros(*shape, device=su.DEV)    # noqa: E731
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="Cin=1040"):
            sparse.sparse_conv3d(z(8, 1040), km, z(27, 1040, 64), elu=True)
        with pytest.raises(RuntimeError, match="Cout=96"):
            neck.conv_transpose_gen(c, [8], 2, z(8, 64), z(8, 64, 96))
        with pytest.raises(RuntimeError, match="tensor_stride=1"):
            neck.conv_transpose_gen(c, [8], 1, z(8, 64), z(8, 64, 64))
        with pytest.raises(RuntimeError, match="num_classes=17"):
            neck.neck_head(z(8, 256), z(1, 256, 17))
