"""Inputs shared by tests/test_grounding_loss_host.py and tests/test_gpu_grounding_loss.py: the random boxes of the IoU tests, the
closed-form pairs, and the batches of the cost / matching / loss tests."""
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


# the volume error the coplanarity rule admits on the ulp pair, as IoU: COPLANAR_TOL * max size * (face area / volume = 1 / thickness)
# summed over the six coplanar faces, twice (the intersection shrinks, the union grows)
ULP_TOL = 2 * 1e-5 * 1.1 * 2 * (1 / 0.9 + 1 / 0.6 + 1 / 1.1)


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
            pm[i, pick] = 1.0 / len(pick)
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
