"""Inputs shared by tests/test_grounding_loss_host.py, tests/test_gpu_grounding_loss.py and tests/test_gpu_grounding_loss_edges.py: the
random boxes of the IoU tests, the closed-form pairs, the batches of the cost / matching / loss tests; and for the edge tests the IoU
regimes, near-duplicates and same-box pairs with the bound the coplanarity rule admits on them, batches with an explicit matching,
saturated scores and dyadic boxes with real ties."""
import math

import numpy as np

GL_ENTRY_POINTS = ("ptx_gl_iou", "ptx_gl_cost", "ptx_gl_loss_fwd", "ptx_gl_loss_bwd", "ptx_gl_predict")
PARITY = 1e-4                      # the project's parity bound: device against the float64 specification, of each tensor's scale


def random_boxes(n, seed):
    """Centres N(0, 0.3), sizes U(0.2, 1.5), angles U(-pi, pi)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(0.0, 0.3, (n, 3)), rng.uniform(0.2, 1.5, (n, 3)), rng.uniform(-math.pi, math.pi, (n, 3))], 1)


def _box(c=(0, 0, 0), s=(1, 1, 1), a=(0, 0, 0)):
    return np.array(list(c) + list(s) + list(a), np.float64)


def rotation_zxy(a):
    """``Rz(a0) Rx(a1) Ry(a2)`` written out on its own (the tests' side of the convention)."""
    c0, s0, c1, s1, c2, s2 = math.cos(a[0]), math.sin(a[0]), math.cos(a[1]), math.sin(a[1]), math.cos(a[2]), math.sin(a[2])
    rz = np.array([[c0, -s0, 0], [s0, c0, 0], [0, 0, 1.0]])
    rx = np.array([[1.0, 0, 0], [0, c1, -s1], [0, s1, c1]])
    ry = np.array([[c2, 0, s2], [0, 1.0, 0], [-s2, 0, c2]])
    return rz @ rx @ ry


ROT = (0.5, -0.8, 1.2)


def closed_forms():
    """``[(name, box1, box2, expected IoU)]``; every one holds in both argument orders."""
    s2 = math.sqrt(2.0)
    ulp = _box(c=(0.3, -0.2, 0.7), s=(0.9, 0.6, 1.1), a=ROT)
    moved = ulp.copy()
    moved[0] = float(np.nextafter(np.float32(moved[0]), np.float32(2.0)))
    ulp[0] = float(np.float32(ulp[0]))
    return [
        ("identical axis-aligned", _box(), _box(), 1.0),
        ("identical rotated", _box(c=(0.3, -0.2, 0.7), s=(0.9, 0.6, 1.1), a=ROT), _box(c=(0.3, -0.2, 0.7), s=(0.9, 0.6, 1.1), a=ROT), 1.0),
        ("unit cubes shifted by 0.5", _box(), _box(c=(0.5, 0, 0)), 1.0 / 3.0),
        ("unit cube turned pi/4 about z", _box(), _box(a=(math.pi / 4, 0, 0)), (2 * s2 - 2) / (4 - 2 * s2)),
        ("touching on a face", _box(), _box(c=(1, 0, 0)), 0.0),
        ("touching on a face with a lateral offset", _box(), _box(c=(1, 0.3, -0.2)), 0.0),
        ("touching on an edge", _box(), _box(c=(1, 1, 0)), 0.0),
        ("a half-size cube inside", _box(), _box(c=(0.1, -0.05, 0.15), s=(0.5, 0.5, 0.5)), 1.0 / 8.0),
        ("a half-size cube inside, flush with a face plane", _box(), _box(c=(0.25, 0.1, 0), s=(0.5, 0.5, 0.5)), 1.0 / 8.0),
        ("a half-width slab flush with a face", _box(), _box(c=(0.25, 0, 0), s=(0.5, 1, 1)), 0.5),
        ("identical rotated, one centre moved by one float32 ulp", ulp, moved, 1.0),
    ]


def coplanar_admit(b1, b2):
    """The IoU error the coplanarity rule admits on a pair whose faces lie within its tolerance of each other: COPLANAR_TOL * the largest
    of the six sizes * (face area / volume = 1 / thickness) summed over the six coplanar faces (of the box where that sum is larger),
    twice (the intersection shrinks, the union grows).  ``b1, b2 (..., 9)``; one value per pair."""
    b1, b2 = np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    largest = np.maximum(b1[..., 3:6].max(-1), b2[..., 3:6].max(-1))
    thin = np.maximum((1.0 / b1[..., 3:6]).sum(-1), (1.0 / b2[..., 3:6]).sum(-1))
    return 2 * 1e-5 * largest * 2 * thin


# the same on the ulp pair of ``closed_forms``
ULP_TOL = float(coplanar_admit(_box(s=(0.9, 0.6, 1.1)), _box(s=(0.9, 0.6, 1.1))))


def coplanar_bound(b1, b2):
    """The bound of a near-duplicate or same-box pair: an fp32 and an fp64 decision of the rule can fall on different sides of the
    tolerance, so the device may differ from the specification by ``PARITY`` and by what the rule admits on the pair."""
    return PARITY + coplanar_admit(b1, b2)


def batch(NL, B, K, M, T, tokens, G, seed, spread=1.0):
    """``scores (NL,B,K,M)`` with ``-inf`` on masked tokens and on the columns from ``T`` on (as ``contrastive_scores`` leaves them),
    ``boxes (NL,B,K,9)``, ``mask (B,T)`` with ``tokens[b]`` tokens set, per scene ``G[b]`` ground-truth boxes at least 1 m apart and
    their positive maps (rows summing to 1 over a few unmasked tokens).  The first ``min(K, G_b)`` queries of a scene lie near a
    ground-truth box each, so that the matching is far from a tie."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((B, T), bool)
    for b in range(B):
        mask[b, rng.permutation(T)[:tokens[b]]] = True
    scores = np.full((NL, B, K, M), -np.inf, np.float64)
    scores[..., :T] = np.where(mask[None, :, None, :], rng.normal(0.0, 2.0, (NL, B, K, T)), -np.inf)
    gts, pms = [], []
    for b in range(B):
        g = np.concatenate([np.stack([np.arange(G[b]) * 1.5, rng.normal(0, 0.2, G[b]), rng.normal(0, 0.2, G[b])], 1),
                            rng.uniform(0.3, 1.2, (G[b], 3)), rng.uniform(-math.pi, math.pi, (G[b], 3))], 1).reshape(G[b], 9)
        pm = np.zeros((G[b], M))
        idx = np.nonzero(mask[b])[0]
        for i in range(G[b]):
            pick = idx[rng.permutation(len(idx))[:min(len(idx), 1 + i % 3)]]
            pm[i, pick] = 1.0 / max(len(pick), 1)            # (a scene without a token keeps a zero map)
        gts.append(g)
        pms.append(pm)
    boxes = np.concatenate([rng.normal(0.0, 3.0, (NL, B, K, 3)) + np.array([0, 6.0, 0]), rng.uniform(0.3, 1.2, (NL, B, K, 3)),
                            rng.uniform(-math.pi, math.pi, (NL, B, K, 3))], -1)
    for l in range(NL):
        for b in range(B):
            for i, q in enumerate(rng.permutation(K)[:min(K, G[b])]):
                boxes[l, b, q] = gts[b][i] + np.concatenate([rng.normal(0, 0.03 * spread, 3), rng.normal(0, 0.03 * spread, 3),
                                                             rng.normal(0, 0.05 * spread, 3)])
    return scores, boxes, mask, gts, pms


SHAPES = {
    "small": dict(NL=2, B=3, K=5, M=16, T=7, tokens=(7, 3, 1), G=(3, 0, 7), seed=11),
    "wave": dict(NL=2, B=3, K=70, M=16, T=7, tokens=(7, 3, 1), G=(1, 2, 1), seed=12),
    "full": dict(NL=1, B=1, K=3, M=256, T=256, tokens=(200,), G=(1,), seed=13),
}


def scale(a):
    a = np.asarray(a, np.float64)
    fin = a[np.isfinite(a)]
    return max(float(np.abs(fin).max()) if fin.size else 0.0, 1e-30)


def close(got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    assert err <= tol * scale(ref), (err, tol * scale(ref))
    return err


# ------------------------------------------------------------------------------------------------------------------ the Qhull oracle
def halfspaces(box):
    """The six half-spaces ``n . x + d <= 0`` of a box, rows ``(n, d)``."""
    R = rotation_zxy(box[6:9])
    rows = []
    for m in range(3):
        for sg in (1.0, -1.0):
            n = sg * R[:, m]
            rows.append(np.concatenate([n, [-(n @ box[:3] + box[3 + m] / 2)]]))
    return np.array(rows)


def qhull_iou(a, b):
    """IoU through scipy: the Chebyshev centre of the twelve half-spaces by ``linprog`` as the interior point, ``HalfspaceIntersection``
    for the vertices, ``ConvexHull`` for the volume."""
    from scipy.optimize import linprog
    from scipy.spatial import ConvexHull, HalfspaceIntersection
    hs = np.concatenate([halfspaces(a), halfspaces(b)])
    res = linprog([0, 0, 0, -1], A_ub=np.concatenate([hs[:, :3], np.ones((12, 1))], 1), b_ub=-hs[:, 3], bounds=[(None, None)] * 3 + [(0, None)])
    vi = 0.0
    if res.status == 0 and res.x[3] > 1e-9:
        vi = ConvexHull(HalfspaceIntersection(hs, res.x[:3]).intersections).volume
    va, vb = np.prod(a[3:6]), np.prod(b[3:6])
    return vi / (va + vb - vi)


# ------------------------------------------------------------------------------------------------------------------ boxes on a grid
def grid_boxes(n, seed):
    """Boxes whose faces meet all the time: centres on a 0.25 grid, sizes multiples of 0.5, every angle a multiple of pi/2 -- pairs
    that are flush, touch on faces, edges and corners, or coincide are the rule here, not the exception."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(-4, 5, (n, 3)) * 0.25, rng.integers(1, 5, (n, 3)) * 0.5, rng.integers(-1, 3, (n, 3)) * (math.pi / 2)], 1)


def axis_aligned_iou(a, b):
    """The closed form for two boxes turned by right angles only: the product of the three interval overlaps."""
    lo, hi = [], []
    for box in (a, b):
        ext = np.abs(np.round(rotation_zxy(box[6:9]))) @ box[3:6]
        lo.append(box[:3] - ext / 2)
        hi.append(box[:3] + ext / 2)
    inter = float(np.prod(np.clip(np.minimum(hi[0], hi[1]) - np.maximum(lo[0], lo[1]), 0.0, None)))
    va, vb = float(np.prod(a[3:6])), float(np.prod(b[3:6]))
    return inter / (va + vb - inter)


# ------------------------------------------------------------------------------------------------------------------ the IoU regimes
def f32(a):
    """Rounded to fp32 once and widened again: the same values on both sides."""
    return np.asarray(a, np.float32).astype(np.float64)


IOU_REGIMES = ("plain", "thin", "far", "angles", "small", "large", "inside")
IOU_N = 24
# (the default seed below is one at which the specification meets the overlap shares over all 576 pairs: test_grounding_loss_host.py)
OVERLAP_SHARE = {"thin": 0.3}                               # the others: 0.5


def iou_regime(name, n=IOU_N, seed=2):
    """Two lists of ``n`` boxes (fp32 values): ``plain`` as ``random_boxes``; ``thin`` one size per box from U(0.02, 0.05); ``far`` both
    lists shifted by (40, -25, 3); ``angles`` U(-20 pi, 20 pi); ``small`` / ``large`` centres and sizes x 1e-2 / x 20; ``inside`` the
    second list is the first with sizes x 0.4 and its own angles."""
    rng = np.random.default_rng(500 + seed + IOU_REGIMES.index(name))
    A, B = random_boxes(n, 600 + seed), random_boxes(n, 700 + seed)
    if name == "thin":
        for X in (A, B):
            X[np.arange(n), 3 + rng.integers(0, 3, n)] = rng.uniform(0.02, 0.05, n)
    elif name == "far":
        A[:, :3] += (40.0, -25.0, 3.0)
        B[:, :3] += (40.0, -25.0, 3.0)
    elif name == "angles":
        A[:, 6:], B[:, 6:] = rng.uniform(-20 * math.pi, 20 * math.pi, (n, 3)), rng.uniform(-20 * math.pi, 20 * math.pi, (n, 3))
    elif name in ("small", "large"):
        A[:, :6] *= 1e-2 if name == "small" else 20.0
        B[:, :6] *= 1e-2 if name == "small" else 20.0
    elif name == "inside":
        B[:, :6] = A[:, :6]
        B[:, 3:6] *= 0.4
    return f32(A), f32(B)


def contained(A, B):
    """Per row: box B (same centre as A) lies inside A whatever its angles -- its half diagonal is within A's smallest half size."""
    return np.sqrt(((B[:, 3:6] / 2) ** 2).sum(-1)) <= A[:, 3:6].min(-1) / 2


def ulp_moved(boxes, rng):
    """Every value moved by one fp32 ulp in a random direction."""
    b = np.asarray(boxes, np.float32)
    return np.nextafter(b, np.where(rng.integers(0, 2, b.shape) > 0, np.inf, -np.inf).astype(np.float32)).astype(np.float64)


def ulp_sensitivity(iou, A, B, pairs, draws=4, seed=0):
    """The largest movement of ``iou(a, b)`` over ``pairs`` (index pairs) when every input moves one fp32 ulp in a random direction,
    over ``draws`` draws: how far two correct fp32 evaluations of the regime may lie apart."""
    rng = np.random.default_rng(900 + seed)
    base = np.array([iou(A[i][None], B[j][None])[0, 0] for i, j in pairs])
    worst = 0.0
    for _ in range(draws):
        A2, B2 = ulp_moved(A, rng), ulp_moved(B, rng)
        worst = max(worst, float(np.abs(np.array([iou(A2[i][None], B2[j][None])[0, 0] for i, j in pairs]) - base).max()))
    return worst


DELTAS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)


def near_duplicates(kind, delta, n=IOU_N, seed=0):
    """What converged predictions look like: ``B = A + delta * N(0, 1) * (size, size, 1)``; ``kind``: ``cubes`` (three equal sizes
    from U(0.2, 1.5)) or ``thin`` (one size from U(0.02, 0.05))."""
    rng = np.random.default_rng(800 + seed + DELTAS.index(delta))
    A = random_boxes(n, 810 + seed)
    if kind == "cubes":
        A[:, 3:6] = A[:, 3:4]
    else:
        A[np.arange(n), 3 + rng.integers(0, 3, n)] = rng.uniform(0.02, 0.05, n)
    B = A + delta * rng.standard_normal((n, 9)) * np.concatenate([A[:, 3:6], A[:, 3:6], np.ones((n, 3))], 1)
    return f32(A), f32(B)


def same_box_names(n=64, seed=0):
    """``[(name, A, B)]`` with ``B[i]`` the box ``A[i]`` by another name, up to the fp32 rounding of the angle: itself; ``a0 + 2 pi``;
    cubes about z turned by pi/2 about z; cubes of any attitude turned by pi/2 about their own y axis (``R Ry(pi/2)``: the last factor)."""
    A = random_boxes(n, 820 + seed)
    turn = A.copy()
    turn[:, 6] += 2 * math.pi
    cz = A.copy()
    cz[:, 3:6], cz[:, 7:9] = cz[:, 3:4], 0.0
    cz2 = cz.copy()
    cz2[:, 6] += math.pi / 2
    cy = A.copy()
    cy[:, 3:6] = cy[:, 3:4]
    cy2 = cy.copy()
    cy2[:, 8] += math.pi / 2
    return [("itself", f32(A), f32(A)), ("a0 + 2 pi", f32(A), f32(turn)), ("cube about z, + pi/2", f32(cz), f32(cz2)),
            ("cube, own y + pi/2", f32(cy), f32(cy2))]


# ------------------------------------------------------------------------------------------------------------------ batches with a given matching
def soft_maps(mask, G, M, rng, hard=False):
    """Positive maps with fractional targets U(0, 1) on the unmasked tokens (``hard``: 0 / 1), zero elsewhere."""
    out = []
    for b, g in enumerate(G):
        pm = np.zeros((g, M))
        idx = np.nonzero(mask[b])[0]
        pm[:, idx] = rng.integers(0, 2, (g, len(idx))) if hard else rng.uniform(0.0, 1.0, (g, len(idx)))
        out.append(pm)
    return out


def explicit_batch(NL, B, K, M, T, tokens, G, seed, pairs=None, soft=True):
    """A batch with its matching given (no Hungarian step): ``scores, boxes, mask, gts, pms`` as ``batch`` lays them out and ``assign
    (NL,B,K) int32``, per (layer, scene) ``pairs[l][b]`` (default ``min(K, G_b)``) random queries matched to distinct random boxes of
    the scene, each prediction near its box.  Fractional positive maps unless ``soft=False``.  Values rounded to fp32 once."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((B, T), bool)
    for b in range(B):
        mask[b, rng.permutation(T)[:tokens[b]]] = True
    scores = np.full((NL, B, K, M), -np.inf)
    scores[..., :T] = np.where(mask[None, :, None, :], rng.normal(0.0, 2.0, (NL, B, K, T)), -np.inf)
    gts = [np.concatenate([rng.normal(0.0, 2.0, (g, 3)), rng.uniform(0.3, 1.2, (g, 3)), rng.uniform(-math.pi, math.pi, (g, 3))], 1) for g in G]
    pms = soft_maps(mask, G, M, rng, hard=not soft)
    boxes = np.concatenate([rng.normal(0.0, 2.0, (NL, B, K, 3)), rng.uniform(0.3, 1.2, (NL, B, K, 3)),
                            rng.uniform(-math.pi, math.pi, (NL, B, K, 3))], -1)
    assign = np.full((NL, B, K), -1, np.int32)
    for l in range(NL):
        for b in range(B):
            p = min(K, G[b]) if pairs is None else pairs[l][b]
            q, g = rng.permutation(K)[:p], rng.permutation(G[b])[:p]
            assign[l, b, q] = g
            boxes[l, b, q] = gts[b][g] + rng.normal(0.0, 0.05, (p, 9))
    return dict(scores=f32(scores), boxes=f32(boxes), mask=mask, gts=[f32(g) for g in gts], pms=[f32(p) for p in pms], assign=assign)


def saturate(scores, mask, lo, hi, seed):
    """The unmasked scores replaced by +-U(lo, hi), signs at random."""
    rng = np.random.default_rng(seed)
    out = np.array(scores, np.float64)
    T = mask.shape[1]
    big = rng.uniform(lo, hi, out[..., :T].shape) * np.where(rng.integers(0, 2, out[..., :T].shape) > 0, 1.0, -1.0)
    out[..., :T] = np.where(mask[None, :, None, :], big, out[..., :T])
    return f32(out)


FOCAL_PARAMS = ((0.25, 2.0), (0.5, 1.0), (0.1, 1.5), (0.9, 3.0), (0.0, 2.0), (1.0, 8.0))
COST_WEIGHTS = ((0.5, 3.0, 1.0), (0.0, 0.0, 1.0))
TOKEN_EDGES = sorted({(T, M) for T in (1, 15, 16, 17, 33) for M in (T, 48, 256)})


def dyadic_ties():
    """``(pred (8,9), gt (8,9))``: angles 0, sizes 1 and 0.5, every prediction its target shifted by exactly half a size along one, two
    and three axes (and once against the axis): each source corner is equally far from two, four or eight target corners, and every
    number on the way is a dyadic fraction, exact in fp32."""
    gt, pred = [], []
    for size in (1.0, 0.5):
        for shift in ((1, 0, 0), (0, 1, 1), (1, 1, 1), (0, 0, -1)):
            gt.append(_box(c=(0.25, -0.5, 1.0), s=(size,) * 3))
            pred.append(_box(c=tuple(c + 0.5 * size * s for c, s in zip((0.25, -0.5, 1.0), shift)), s=(size,) * 3))
    return np.stack(pred), np.stack(gt)
