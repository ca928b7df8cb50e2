"""Inputs and the correctness criterion shared by tests/test_grounding_assign_host.py and tests/test_gpu_grounding_assign.py: the
matching on the device (``ptx_gl_assign``) and its numpy specification (``grounding_loss_host.sap_assign_host``) against scipy.

THE CRITERION (derived, not measured).  ``assign`` is a matching: every box at most once, every query at most once, exactly
``min(K, G_b)`` pairs per (layer, scene), every entry in ``[0, G_b)`` or -1.  Its total cost, summed in float64 from the fp32 matrix
after the NaN / inf mapping, equals scipy's within ``TOTAL_TOL = 1e-9``: at most 2 x 1024 float64 additions of magnitudes <= 100 round
by about 2e-11, and the smallest optimality gap of the random inputs (4.7e-4) is five orders above the bound.  On an input with a UNIQUE
optimum the pairs themselves equal scipy's; uniqueness is checked, not assumed: forbidding any one of scipy's pairs (cost 1e6) must raise
the optimum by at least ``MIN_GAP = 1e-6``."""
import functools

import numpy as np
from scipy.optimize import linear_sum_assignment

GA_ENTRY_POINTS = ("ptx_gl_assign",)
TOTAL_TOL = 1e-9
MIN_GAP = 1e-6
# (K, G) of the random problems: a box or a few against the shipped 256 queries, both sides of K = G, the widest columns
RANDOM_SHAPES = ((256, 1), (256, 4), (256, 17), (256, 64), (64, 65), (8, 20), (1, 5), (63, 63), (1024, 32))


# (K, G of every scene) on both sides of the switch of ``ptx_gl_assign`` at min(K, max G) * max(K, max G) <= 32768 between the matrix
# staged in LDS and the matrix read in place: staged at exactly 128 KiB with the boxes as the rows (written transposed) and with the
# queries as the rows; the first shapes read in place, by columns and by rows; one large scene that takes the whole launch out of staging
# while the 3-, 0- and 40-box scenes beside it run on the in-place path.  Random and special matrices are drawn with seed 7 + K
# (``stage_edge_cost``); the random ones have a unique optimum (gaps 2e-3 to 2e-2, ``require_unique`` guards it).
STAGE_EDGE_SHAPES = ((256, (128,)), (128, (256,)), (256, (129,)), (129, (256,)), (256, (3, 129, 0, 40)))
STAGE_EDGE_NL = 2
STAGE_FLOATS = 32768


def staged(K, max_g):
    """Whether ``ptx_gl_assign`` stages the matrices of a launch in LDS (csrc/grounding_assign.hip, ``kGaStageFloats``)."""
    return min(K, max_g) * max(K, max_g) <= STAGE_FLOATS


def mapped(cost):
    """The matrix the matchers solve: float64 of the fp32 values with ``hungarian_assign``'s mapping of NaN and the infinities."""
    return np.nan_to_num(np.asarray(cost, np.float32).astype(np.float64), nan=100.0, posinf=100.0, neginf=-100.0)


def random_cost(NL, K, G, seed):
    """``cost (NL,K,sum G) fp32 = 2 N(0,1) + U(0,8)`` per query row: far from ties (the smallest gap of ``random_case`` over six seeds of every
    ``RANDOM_SHAPES`` pair is 4.7e-4, at (256, 17))."""
    rng = np.random.default_rng(seed)
    SG = int(sum(G))
    return (2.0 * rng.standard_normal((NL, K, SG)) + rng.uniform(0.0, 8.0, (NL, K, 1))).astype(np.float32)


def constant_cost(NL, K, G, value=0.5):
    return np.full((NL, K, int(sum(G))), value, np.float32)


def dyadic_cost(NL, K, G, seed):
    """Multiples of 0.5 from 0 to 3.5: every sum on the way is exact, ties are the rule."""
    return (np.random.default_rng(seed).integers(0, 8, (NL, K, int(sum(G)))) * 0.5).astype(np.float32)


def product_cost(n):
    """``cost[i,j] = (i+1)(j+1)``: the optimum is the anti-diagonal and the augmenting paths grow long."""
    i = np.arange(1, n + 1, dtype=np.float64)
    return (i[:, None] * i[None, :]).astype(np.float32)[None]


def product_cost_rect(K, G):
    """``cost[k,g] = (k+1)(g+1)`` as a ``K x G`` matrix (every entry exact in fp32 up to 256 x 128): long augmenting paths on a
    rectangle, either side as the rows.  The expected matching comes from the specification, not from a formula."""
    return (np.arange(1, K + 1, dtype=np.float64)[:, None] * np.arange(1, G + 1, dtype=np.float64)[None, :]).astype(np.float32)[None]


@functools.lru_cache(maxsize=None)
def stage_edge_cost(kind, K, G):
    """The ``random`` / ``special`` / ``dyadic`` matrix of a ``STAGE_EDGE_SHAPES`` entry (read-only: drawn once, shared)."""
    draw = dict(random=random_cost, special=special_cost, dyadic=dyadic_cost)[kind]
    cost = draw(STAGE_EDGE_NL, K, G, 7 + K)
    cost.setflags(write=False)
    return cost


def special_cost(NL, K, G, seed):
    """A random matrix with about a tenth of its entries NaN, +inf or -inf, and one query row and one box column entirely NaN."""
    rng = np.random.default_rng(seed)
    cost = random_cost(NL, K, G, seed + 1)
    kind = rng.integers(0, 30, cost.shape)
    cost[kind == 0], cost[kind == 1], cost[kind == 2] = np.nan, np.inf, -np.inf
    cost[:, K // 2, :] = np.nan
    cost[:, :, 0] = np.nan
    return cost


def scipy_assign(cost, G, B):
    """``(NL,B,K) int32``: scipy per (layer, scene) on the mapped matrix."""
    m = mapped(cost)
    NL, K, _ = m.shape
    out = np.full((NL, B, K), -1, np.int32)
    lo = 0
    for b in range(B):
        if G[b] and K:
            for l in range(NL):
                rows, cols = linear_sum_assignment(m[l][:, lo:lo + G[b]])
                out[l, b, rows] = cols
        lo += G[b]
    return out


def totals(assign, cost, G):
    """``(NL,B)`` float64: the cost of every (layer, scene) matching, summed in query order from the mapped matrix."""
    m = mapped(cost)
    NL, B, K = assign.shape
    out = np.zeros((NL, B))
    lo = 0
    for b in range(B):
        for l in range(NL):
            q = np.nonzero(assign[l, b] >= 0)[0]
            out[l, b] = m[l][q, lo + assign[l, b, q]].sum()
        lo += G[b]
    return out


def check_matching(assign, cost, G, ref=None):
    """The criterion of the module docstring against scipy (``ref``: scipy's matching when the caller has it); returns scipy's."""
    assign = np.asarray(assign)
    NL, K, SG = np.asarray(cost).shape
    B = len(G)
    assert assign.shape == (NL, B, K) and assign.dtype == np.int32 and SG == sum(G), (assign.shape, assign.dtype)
    for b in range(B):
        a = assign[:, b]
        assert ((a >= -1) & (a < G[b])).all(), (b, a.min(), a.max())           # (G_b = 0: -1 alone)
        for l in range(NL):
            got = a[l][a[l] >= 0]
            assert len(got) == min(K, G[b]) and len(set(got.tolist())) == len(got), (l, b, len(got))
    ref = scipy_assign(cost, G, B) if ref is None else ref
    diff = np.abs(totals(assign, cost, G) - totals(ref, cost, G))
    assert float(diff.max()) <= TOTAL_TOL, float(diff.max())
    return ref


def uniqueness_gap(cost, G):
    """The smallest rise of any (layer, scene) optimum when one of scipy's pairs is forbidden (cost 1e6): > 0 means every optimum is
    unique.  ``inf`` when no problem has a pair."""
    m = mapped(cost)
    gap, lo = np.inf, 0
    for b, g in enumerate(G):
        for l in range(m.shape[0] if g and m.shape[1] else 0):
            C = m[l][:, lo:lo + g]
            rows, cols = linear_sum_assignment(C)
            base = C[rows, cols].sum()
            for r, c in zip(rows, cols):
                other = C.copy()
                other[r, c] = 1e6
                r2, c2 = linear_sum_assignment(other)
                gap = min(gap, other[r2, c2].sum() - base)
        lo += g
    return float(gap)


def require_unique(cost, G):
    """A seed that fails this is a test error: no case is dropped or skipped for it."""
    gap = uniqueness_gap(cost, G)
    assert gap >= MIN_GAP, f"the input has no unique optimum (gap {gap:.3e}): choose another seed"
    return gap


@functools.lru_cache(maxsize=None)
def random_case(K, G, NL=2, seed=0):
    """``(cost, scipy's matching, gap)`` of one ``RANDOM_SHAPES`` pair as a single scene, its unique optimum established."""
    cost = random_cost(NL, K, (G,), 1000 * K + G + 7919 * seed)
    gap = require_unique(cost, (G,))
    ref = scipy_assign(cost, (G,), 1)
    cost.setflags(write=False)
    ref.setflags(write=False)
    return cost, ref, gap


# the tie rule on a hand-worked example (lowest column index among the equal smallest path costs).
# Three queries, three boxes; K = G: the rows are the boxes, the columns the queries, and the matrix is symmetric, so it reads either way.
#   box 0: path costs (1, 1, 2): queries 0 and 1 tie, query 0 is taken and is free -> box 0 - query 0, u0 = 1.
#   box 1: path costs (1, 1, 2): query 0 is taken first although it is matched; box 0's row then offers (1 + 1) - 1 = 1 for query 1, no
#          better than the 1 it has from box 1; query 1 is the lowest remaining -> box 1 - query 1, box 0 keeps query 0.
#   box 2: path costs (2, 2, 1): query 2.
# A "highest index" rule would give box 0 - query 1 and box 1 - query 0, an optimum of the same total 3.
TIE_EXAMPLE = np.array([[[1.0, 1.0, 2.0], [1.0, 1.0, 2.0], [2.0, 2.0, 1.0]]], np.float32)
TIE_EXAMPLE_ASSIGN = np.array([[[0, 1, 2]]], np.int32)
# Three queries, two boxes, every cost 0.5 (K > G: the rows are the boxes): box 0 takes query 0; box 1 meets query 0 first, box 0 offers
# nothing better, query 1 is the lowest remaining -> queries (0, 1, none).  And two queries, three boxes (K < G: the rows are the
# queries): query 0 takes box 0, query 1 box 1.
TIE_WIDE = (np.full((1, 3, 2), 0.5, np.float32), np.array([[[0, 1, -1]]], np.int32))
TIE_TALL = (np.full((1, 2, 3), 0.5, np.float32), np.array([[[0, 1]]], np.int32))
