"""The sparse neck's kernels (csrc/neck.hip and the neck instantiations of csrc/sparse.hip) at the edges tests/test_gpu_mink_neck.py does not
reach, each at the smallest shape that takes the branch.  References: the numpy restatements of ``neck_host.py`` / ``sparse_host.py``; bit for
bit where the operation is exact, ``sparse_util.hold`` (8 x the fp32 CPU chain's error against float64) where it sums.  The inputs and what
makes each of them reach its branch are in ``tests/neck_util.py``; those preconditions are also held without a GPU in
tests/test_mink_neck_host.py.

top-k   scores that differ in their low 16 bits only (5000 rows; positive, negative, mixed): the radix passes at shift 8 and 0 split;
        rows on and one past the 256-row ranking run with k = rows - 1 and k = 1; 64 scenes of 0 to 300 rows at k = 100 (9583 rows, C = 4
        and 512); +-inf, denormals, signed zeros and NaNs of both signs with the threshold on each in turn; 700 equal scores.
union   64 scenes cycling through: both empty, A only, B only, disjoint, B in A, A in B, mixed with 820 rows of B (5400 + 9090 rows, C = 4
        and 512; the largest case first and again last); rows at the first and last voxel of the key range, a row of B outside it
        (appended), a row of A outside it (refused).
scores  ~3300 queries at arbitrary integer coordinates over score rows of tensor stride 8 (inexact ``w * s``) and 32768 (the weight's own
        product inexact: the order of its factors shows); tensor stride 1; a +1 corner that leaves the key range while the row it would
        alias carries 1e6; 64 scenes, 16 of them without score rows.
head    (C, K) = (64, 1), (64, 16), (256, 16), (512, 5), (512, 16) on 1, 15, 17 and 2317 rows, per-class weights, with and without bias;
        a NaN class score, in the first, a middle or the last class, makes the prune score NaN.
convs   ELU at Cin 16, 528, 1008 (a last chunk of 16 and of 48 channels above 512) on 600 rows; bias + scale + shift + residual + ELU;
        selectors 0 and 1 at Cin 1024; the generative convolution at 64 -> 512 on 65 rows, 1024 -> 64 on one row and 128 -> 128 on 2357
        rows, plain, with ReLU and with ELU.
end to end  three classes, scenes of 1500 / 0 / 40 / 600 rows, k = 520: the empty scene in the middle, one scene never pruned, one pruned
        at the last step only, one at the last two."""
import numpy as np
import pytest
import torch

from proxytransformation_amd import _abi, neck, neck_host, sparse
from tests import neck_util as nu
from tests import sparse_util as su
from tests.sparse_util import dev

pytestmark = pytest.mark.gpu
NONE, RELU, ELU = neck_host.ACT_NONE, neck_host.ACT_RELU, neck_host.ACT_ELU


# ------------------------------------------------------------------------------------------------------------------ top-k
def _topk(scores, rows, ends, feats, k):
    """Two calls of ``topk_prune`` against ``topk_keep_host`` / ``prune_host`` / ``topk_scene_rows``, bit for bit; returns the mask."""
    keep = neck_host.topk_keep_host(scores, ends, k)
    c, e, f = neck_host.prune_host(keep, rows, ends, feats)
    assert e == neck_host.topk_scene_rows(ends, k)
    with torch.no_grad():
        for _ in range(2):
            gc, ge, gf, gk = neck.topk_prune(dev(scores), dev(rows), ends, dev(feats), k)
            assert ge == e
            assert np.array_equal(gk.cpu().numpy(), keep), (k, np.nonzero(gk.cpu().numpy() != keep)[0][:8])
            nu.bits(gc, c)
            nu.bits(gf, f)
    return keep


def _feats(n, C, seed):
    return np.random.default_rng(seed).standard_normal((n, C)).astype(np.float32)


@pytest.mark.parametrize("kind", ["positive", "negative", "mixed", "normal"])
def test_topk_low_byte_passes(kind):
    """One scene of 5000 rows whose scores differ in the low 16 bits only, so that the threshold is decided by the passes at shift 8 and
    0 (``check_low_byte_passes``: each sees >= 2 occupied digits at every k); ``negative``: the inverted-key branch; ``normal``: N(0, 1),
    for the first two passes."""
    nu.check_low_byte_passes(kind)
    scores = nu.low_byte_scores(kind)
    rows, ends = nu.scene_rows_of([len(scores)])
    feats = _feats(len(scores), 4, 1)
    for k in nu.LOW_BYTE_K:
        keep = _topk(scores, rows, ends, feats, k)
        assert keep.sum() == k


@pytest.mark.parametrize("n", [2, 256, 257, 512, 513])
def test_topk_run_boundaries(n):
    """Row counts on and one past the 256-row ranking run; ``k = rows - 1`` drops exactly the minimum, ``k = 1`` keeps the maximum."""
    scores = np.random.default_rng(100 + n).standard_normal(n).astype(np.float32)
    rows, ends = nu.scene_rows_of([n])
    feats = _feats(n, 8, 2)
    keep = _topk(scores, rows, ends, feats, n - 1)
    assert np.nonzero(~keep)[0].tolist() == [int(scores.argmin())]
    keep = _topk(scores, rows, ends, feats, 1)
    assert np.nonzero(keep)[0].tolist() == [int(scores.argmax())]


@pytest.mark.parametrize("C", [4, 512])
def test_topk_sixty_four_scenes(C):
    """k = 100 over 64 scenes of 0, 1, 99, 100, 101, 255, 256, 257, 300 rows in turn: pruned and unpruned scenes interleave, and the
    places of a scene's rows follow from the 63 before it."""
    sizes = [nu.TOPK_64_SIZES[b % 9] for b in range(64)]
    rows, ends = nu.scene_rows_of(sizes)
    assert len(ends) == 64 and ends[-1] == 9583 and sum(n > nu.TOPK_64_K for n in sizes) == 35
    scores = np.random.default_rng(33).standard_normal(ends[-1]).astype(np.float32)
    keep = _topk(scores, rows, ends, _feats(ends[-1], C, 3), nu.TOPK_64_K)
    assert keep.sum() == sum(min(n, nu.TOPK_64_K) for n in sizes)


def test_topk_specials():
    """+-inf, denormals, signed zeros and NaNs of both signs in one scene; the threshold on +inf (just below the positive NaNs), a positive
    denormal, the zero key, a negative denormal and -inf in turn.  The rule is ``neck_host.topk_key`` as written: a NaN orders by its
    bits.  Then 700 equal scores with k = 300: rows 0 to 299 stay."""
    scores, ks = nu.special_scores()
    rows, ends = nu.scene_rows_of([len(scores)])
    feats = _feats(len(scores), 4, 4)
    pos_nan = np.isnan(scores) & ~np.signbit(scores)
    for name, k in ks.items():
        keep = _topk(scores, rows, ends, feats, k)
        assert keep[pos_nan].all() and keep.sum() == k, name
    keep = _topk(scores, rows, ends, feats, len(scores) - 1)  # everything but one of the negative NaNs
    assert np.isnan(scores[~keep]).all() and np.signbit(scores[~keep]).all()
    equal = np.full(700, np.float32(-0.75))
    rows, ends = nu.scene_rows_of([700])
    keep = _topk(equal, rows, ends, _feats(700, 4, 5), 300)
    assert keep[:300].all() and not keep[300:].any()


# ------------------------------------------------------------------------------------------------------------------ union
def _union(a, a_ends, fa, b, b_ends, fb, ts):
    c, e, f = neck_host.union_add_host(a, a_ends, fa, b, b_ends, fb)
    with torch.no_grad():
        for _ in range(2):
            gc, ge, gf = neck.union_add(dev(a), a_ends, dev(fa), dev(b), b_ends, dev(fb), ts)
            assert ge == e
            nu.bits(gc, c)
            nu.bits(gf, f)
    return c, e


def _key_range_union():
    a, a_ends, b, b_ends = nu.union_key_range_case()
    c, e = _union(a, a_ends, _feats(len(a), 8, 6), b, b_ends, _feats(len(b), 8, 7), 4)
    assert e == [6, 9] and c[5].tolist() == [0, 0, 0, 4 << 18]          # the row of B outside the key range: appended, no error


def test_union_sixty_four_scenes():
    """Every scene kind (``union_kinds``) over 64 scenes, more rows in B than in A; C = 512 first, then C = 4 (one thread per row), the
    six-row scenes of the key-range case (a much smaller table in the same workspace), and C = 512 again: a stale workspace would show."""
    a, a_ends, b, b_ends = nu.union_regime_case()
    assert nu.union_kinds(a, a_ends, b, b_ends) == [nu.UNION_KINDS[i % 7] for i in range(64)] and len(b) > len(a)
    wide = (a, a_ends, _feats(len(a), 512, 8), b, b_ends, _feats(len(b), 512, 9), 4)
    _union(*wide)
    _union(a, a_ends, _feats(len(a), 4, 10), b, b_ends, _feats(len(b), 4, 11), 4)
    _key_range_union()
    _union(*wide)


def test_union_key_range():
    """Rows at the first and last voxel of the key range (tensor stride 4): the pairs one step apart across the end of a key field, one row
    of each in both sets.  A row of B at 2^18 -- whose key, were it formed, would be that of A's row (0, 1, m) -- is appended unmatched;
    a row of A at 2^18 is refused with the range in the message."""
    _key_range_union()
    a, a_ends, b, b_ends = nu.union_key_range_case(a_outside=True)
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"2\^18"):
        neck.union_add(dev(a), a_ends, dev(_feats(len(a), 8, 6)), dev(b), b_ends, dev(_feats(len(b), 8, 7)), 4)
    _key_range_union()                                        # and the next call is served as before


# ------------------------------------------------------------------------------------------------------------------ score lookup
def _lookup(q, s_coords, s_ends, ts, scores):
    ref = neck_host.prune_scores_host(q, s_coords, s_ends, ts, scores)
    assert ref.dtype == np.float32
    with torch.no_grad():
        for _ in range(2):
            nu.bits(neck.prune_scores(dev(q), dev(s_coords), s_ends, ts, dev(scores)), ref)
    return ref


@pytest.mark.parametrize("ts", [8, 32768])
def test_prune_scores_inexact_weights(ts):
    """Queries at arbitrary integer coordinates: ``w * s`` is inexact for most present corners (a contracted multiply-add would show);
    at tensor stride 32768 the three factors of ``w`` no longer multiply exactly either, so their order shows too."""
    nu.check_score_query_case(ts)
    q, s_coords, s_ends, scores = nu.score_query_case(ts)
    ref = _lookup(q, s_coords, s_ends, ts, scores)
    assert (ref > 0).any() and (ref < 0).any() and (ref == 0).any()


def test_prune_scores_tensor_stride_one():
    """Tensor stride 1: every query is on the lattice; the score rows themselves, their neighbours one step down each axis, and random
    coordinates."""
    s_coords, s_ends = su.rows(1)
    rng = np.random.default_rng(52)
    scores = rng.standard_normal(len(s_coords)).astype(np.float32)
    shifted = np.concatenate([s_coords - np.array([0, *(int(i == d) for i in range(3))], np.int32) for d in range(3)])
    rnd = np.concatenate([rng.integers(0, 4, (500, 1)), rng.integers(-6, 6, (500, 3))], 1).astype(np.int32)
    q = np.concatenate([s_coords, shifted, rnd])
    ref = _lookup(q, s_coords, list(s_ends), 1, scores)
    assert np.array_equal(ref[:len(s_coords)], scores) and (ref[len(s_coords):] == 0).any() and (ref[len(s_coords):] != 0).any()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_prune_scores_corner_past_the_key_range(axis):
    """A query in the last voxel of ``axis``: its +1 corners are outside the key range and absent -- not the row of the next key field,
    which is present with score 1e6 (``score_edge_case``).  The expected value is the host's."""
    q, s_coords, s_ends, scores = nu.score_edge_case(axis)
    ref = _lookup(q, s_coords, s_ends, 4, scores)
    assert (ref > 0).all() and (ref < 10).all()


def test_prune_scores_sixty_four_scenes():
    q, s_coords, s_ends, scores = nu.score_64_case()
    ref = _lookup(q, s_coords, s_ends, 2, scores)
    empty = np.diff([0] + s_ends)[q[:, 0]] == 0
    assert empty.sum() == 320 and (ref[empty] == 0).all() and not np.signbit(ref[empty]).any() and (ref[~empty] != 0).mean() > 0.5


# ------------------------------------------------------------------------------------------------------------------ head
HEAD_ROWS = (1, 15, 17, 2317)


def _head_operands(C, K, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((HEAD_ROWS[-1], C)).astype(np.float32)
    w = (rng.standard_normal((1, C, K)) / 16).astype(np.float32) * np.arange(1, K + 1, dtype=np.float32)    # class k scaled by k + 1
    return x, w, rng.standard_normal((1, K)).astype(np.float32)


@pytest.mark.parametrize("C,K", [(64, 1), (64, 16), (256, 16), (512, 5), (512, 16)])
def test_head_shapes(C, K):
    """``cls`` by ``hold`` over the four row counts together (a one-row result alone has too few values for its fp32 yardstick to be
    anything but luck), the results on the first 1, 15 and 17 rows bit-equal to those rows of the 2317-row call, ``score`` bit-equal to
    the maximum of the device's own ``cls``.  Every class has its own weight scale: a swapped class or channel cannot pass."""
    x, w, b = _head_operands(C, K, 60 + C + K)
    for bias in (b, None):
        got, ref32, ref64 = [], [], []
        for n in HEAD_ROWS:
            with torch.no_grad():
                cls, score = neck.neck_head(dev(x[:n]), dev(w), None if bias is None else dev(bias))
            cls, score = cls.cpu().numpy(), score.cpu().numpy()
            assert cls.shape == (n, K) and score.shape == (n,)
            assert np.array_equal(score.view(np.uint32), cls.max(axis=1).view(np.uint32))
            got.append(cls)
            ref32.append(neck_host.head_host(x[:n], w[0], bias)[0])
            ref64.append(neck_host.head_host(x[:n].astype(np.float64), w[0].astype(np.float64), None if bias is None else bias.astype(np.float64))[0])
        for part in got[:3]:
            assert np.array_equal(part.view(np.uint32), got[3][:len(part)].view(np.uint32))
        su.hold(f"head {C}->{K} bias={bias is not None}", np.concatenate(got), np.concatenate(ref32), np.concatenate(ref64))
        if K > 1 and bias is None:
            assert float(np.abs(got[3][:, K - 1]).mean()) > 2 * float(np.abs(got[3][:, 0]).mean())


@pytest.mark.parametrize("C,K", [(256, 16), (512, 5), (64, 1)])
def test_head_nan_rule(C, K):
    """The specification is ``head_host``: a row with a NaN class score has a NaN ``score``, whichever class it appears in.  A NaN feature
    makes every class NaN; +inf in two channels whose weights have opposite signs in ONE class makes that class alone NaN (inf - inf)
    and the others +inf -- the first, a middle and the last class, one row each.  ``isnan`` on those rows, bits elsewhere."""
    x, w, b = _head_operands(C, K, 70 + C + K)
    x = x[:300].copy()
    x[[5, 16, 299], 9] = np.nan
    single = {40: 0, 41: K // 2, 42: K - 1} if K > 1 else {}
    w[0, 3] = np.abs(w[0, 3])
    for row, k in single.items():                            # channel 3 and a channel of the row's own, negative in class k alone
        w[0, row - 20] = np.abs(w[0, row - 20])
        w[0, row - 20, k] *= -1
        x[row, 3] = x[row, row - 20] = np.inf
    ref_cls, ref_score = neck_host.head_host(x, w[0], b)
    with torch.no_grad():
        cls, score = neck.neck_head(dev(x), dev(w), dev(b))
    cls, score = cls.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(np.isnan(cls), np.isnan(ref_cls)) and np.isnan(ref_cls[[5, 16, 299]]).all()
    for row in single:
        assert 0 < np.isnan(ref_cls[row]).sum() < K and np.isinf(ref_cls[row][~np.isnan(ref_cls[row])]).all()
    bad = np.isnan(ref_score)
    assert bad.sum() == 3 + len(single) and np.array_equal(np.isnan(score), bad)
    assert np.array_equal(score[~bad].view(np.uint32), cls[~bad].max(axis=1).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ convolutions
def _conv_refs(ops, nbr, use, act):
    return [neck_host.sparse_conv3d_act_host(ops["feats"].astype(dt), nbr, ops["weight"].astype(dt), act=act,
                                             **{u: ops[u].astype(dt) for u in use}) for dt in (np.float32, np.float64)]


@pytest.mark.parametrize("cin,cout,use", [(16, 64, ("scale", "shift")), (528, 64, ("scale", "shift")), (1008, 64, ("scale", "shift")),
                                          (256, 128, ("bias", "scale", "shift", "residual"))])
def test_conv_act_elu_widths(cin, cout, use):
    """ELU on 600 rows: one short chunk (16); above 512 a last chunk of 16 channels (528: one half-step) and of 48 (1008: both, the second
    half full of staged zeros); and the whole epilogue -- bias, scale, shift, residual -- in front of the ELU."""
    nbr = su.host_map(4, 3, 1, 600)[2]
    km = su.device_map(4, 3, 1, 600)
    ops = su.operands(600, 600, cin, cout, 27, 80 + cin)
    assert float(np.abs(ops["feats"]).min()) > 0 and float(np.abs(ops["weight"]).min()) > 0
    with torch.no_grad():
        got = sparse.sparse_conv3d(dev(ops["feats"]), km, dev(ops["weight"]), elu=True, **{u: dev(ops[u]) for u in use})
        again = sparse.sparse_conv3d(dev(ops["feats"]), km, dev(ops["weight"]), elu=True, **{u: dev(ops[u]) for u in use})
    assert torch.equal(got, again)
    r32, r64 = _conv_refs(ops, nbr, use, ELU)
    assert 0.3 < float((r64 < 0).mean()) < 0.7 and r32.dtype == np.float32
    su.hold(f"regime conv+ELU {cin}->{cout} {'+'.join(use)}", got.cpu().numpy(), r32, r64)


@pytest.mark.parametrize("act", [NONE, RELU])
def test_conv_act_selectors_at_1024(act):
    """Selector 0 (none) and 1 (ReLU) at Cin 1024 through ``ptx_sparse_conv3d_act`` itself."""
    nbr = su.host_map(4, 3, 1, 600)[2]
    km = su.device_map(4, 3, 1, 600)
    ops = su.operands(600, 600, 1024, 64, 27, 90 + act)
    use = ("scale", "shift")
    f, w = dev(ops["feats"]), dev(ops["weight"])
    vec = {u: dev(ops[u]) for u in use}
    got = torch.empty((600, 64), dtype=torch.float32, device=su.DEV)
    _abi.check(_abi.lib().ptx_sparse_conv3d_act(f.data_ptr(), 600, km.nbr.data_ptr(), 600, 27, w.data_ptr(), 1024, 64, None,
                                                vec["scale"].data_ptr(), vec["shift"].data_ptr(), None, act, got.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "ptx_sparse_conv3d_act")
    r32, r64 = _conv_refs(ops, nbr, use, act)
    assert 0.3 < float((r64 < 0).mean() if act == NONE else (r64 == 0).mean()) < 0.7
    assert act == NONE or float(got.min()) == 0.0
    su.hold(f"regime conv selector {act} 1024->64", got.cpu().numpy(), r32, r64)


@pytest.mark.parametrize("act", [NONE, RELU, ELU])
@pytest.mark.parametrize("cin,cout,n", [(64, 512, 65), (1024, 64, 1), (128, 128, 2357)])
def test_generative_shapes(cin, cout, n, act):
    """65 rows: a second tile holding one row, 8 column tiles x 8 offsets; one row; 2357 rows in two scenes.  ``act`` none: no scale, no
    shift; ReLU and ELU: behind scale and shift.  Coordinates bit for bit."""
    rows, ends = su.random_rows(95, 8, (n - n // 3, n // 3) if n > 1 else (1,), -8, 8)
    rng = np.random.default_rng(96 + cin)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    kernel = (rng.standard_normal((8, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    scale, shift = (None, None) if act == NONE else (rng.uniform(0.5, 1.5, cout).astype(np.float32), (rng.standard_normal(cout) * 0.5).astype(np.float32))
    opt = lambda v, f: None if v is None else f(v)           # noqa: E731
    with torch.no_grad():
        oc, oe, out = neck.conv_transpose_gen(dev(rows), list(ends), 8, dev(x), dev(kernel), opt(scale, dev), opt(shift, dev), act)
    c32, e32, r32 = neck_host.conv_transpose_gen_host(rows, list(ends), 8, x, kernel, scale, shift, act)
    f64 = lambda v: v.astype(np.float64)                     # noqa: E731
    r64 = neck_host.conv_transpose_gen_host(rows, list(ends), 8, f64(x), f64(kernel), opt(scale, f64), opt(shift, f64), act)[2]
    assert rows.shape[0] == n and oe == e32 and out.shape == (8 * n, cout)
    nu.bits(oc, c32)
    if n > 1:                                                # (one row x 64 columns x 8 offsets: 512 values, no stable share)
        assert 0.3 < float((r64 == 0).mean() if act == RELU else (r64 < 0).mean()) < 0.7
    su.hold(f"regime generative conv {cin}->{cout} n={n} act={act}", out.cpu().numpy(), r32, r64)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_three_classes_and_an_empty_scene():
    """``neck_util.end_to_end`` (the protocol of test_gpu_mink_neck.py's end-to-end test, same asserts) on the second configuration:
    three classes, so the maximum over the classes decides the prune; scenes of 1500 / 0 / 40 / 600 rows with k = 520: the empty scene in
    the middle, the 40-row scene never pruned, the 1500-row scene pruned at the last step only, the 600-row scene at the last two."""
    trace = nu.end_to_end(nu.e2e_levels_b(), nu.e2e_neck_b(), 4, nu.K_PRUNE_B)
    pruned = [[s for s in range(4) if np.diff([0] + tr["scene_rows"])[s] > nu.K_PRUNE_B] for tr in trace]
    assert pruned == [[], [3], [0, 3]]
