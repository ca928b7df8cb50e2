"""The grounding loss (``grounding_loss.py``, ``csrc/grounding_loss.hip``) restated in numpy: the specification of every ``ptx_gl_*`` launch,
float64 throughout.  Boxes are ``(cx,cy,cz, sx,sy,sz, a0,a1,a2)`` with the rotation ``R = Rz(a0) Rx(a1) Ry(a2)`` (pytorch3d's
``euler_angles_to_matrix(., 'ZXY')``, structures/bbox_3d/utils.py:67) and the corners ``c + R (+-s/2)``.

``box_iou3d_host``: the exact intersection volume of two oriented boxes.  Every one of the 12 face quads is clipped by the other box's
six half-spaces (Sutherland-Hodgman; a new vertex is always interpolated from the inside end of its edge, so it does not depend on the
direction the edge is walked in) and contributes ``(n . (p - o)) area / 3`` with ``o`` the first box's centre.  THE COPLANARITY RULE: a
face ``i`` of the first box and a face ``j`` of the second are coplanar when all four vertices of each lie within ``COPLANAR_TOL`` times
the largest of the six sizes of the other's plane.  The decision is taken once per ``(i, j)`` and used in both directions: if the two
faces look the same way the FIRST box's face stands for the shared surface (it is not clipped by plane ``j``; the second box's face ``j``
is dropped), if they face each other both are dropped (two boxes that touch share no volume).  Without the rule, rounding puts each of two
coincident faces "inside" the other independently (two identical rotated boxes: IoU 4) and a face lying on an opposite plane is counted
(two touching boxes: 0.09).  A pair of faces closer than the tolerance is moved onto one plane: the intersection volume is off by at most
``COPLANAR_TOL * max size * (the shared face's area)`` per coplanar pair, nothing otherwise.

The costs, the loss and its gradients follow the reference's lines: models/losses/match_cost.py:227-237 (``BinaryFocalLossCost``),
``BBox3DL1Cost`` (an L1 ``cdist``), models/losses/chamfer_distance.py:58-63, 160-203, dense_heads/grounding_head.py:686-824 as the shipped
configuration runs it, and mmdet's sigmoid focal loss (``py_sigmoid_focal_loss`` with ``weight_reduce_loss``), restated from the
published source and not pinned against an installed mmdet.

Two matchings: ``assign_host`` is the host matcher's (scipy); ``sap_assign_host`` writes the shortest-augmenting-path method out with
one stated tie rule and is what the device matcher (``ptx_gl_assign``, csrc/grounding_assign.hip) reproduces bit for bit."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

__all__ = ["COPLANAR_TOL", "SIGNS", "assign_host", "box_iou3d_host", "corners_host", "cost_host", "euler_matrix", "loss_dict", "loss_host", "predict_host", "sap_assign_host"]

COPLANAR_TOL = 1e-5
F32_EPS = float(np.finfo(np.float32).eps)
# bbox_to_corners' signs: x ++++----, y ++--++--, z +-+-+-+-
SIGNS = np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, 1, 1], [-1, 1, -1], [-1, -1, 1], [-1, -1, -1]], np.float64)
_QUAD = ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))     # a face's four vertices along its two in-plane axes
MAX_POLY = 12


def euler_matrix(angles: np.ndarray, derivative: Optional[int] = None) -> np.ndarray:
    """``(...,3,3)``: ``Rz(a0) Rx(a1) Ry(a2)``; ``derivative = k``: its derivative by ``a_k``."""
    a = np.asarray(angles, np.float64)
    c, s = np.cos(a), np.sin(a)
    one, zero = np.ones_like(c[..., 0]), np.zeros_like(c[..., 0])

    def mat(rows):
        return np.stack([np.stack(r, -1) for r in rows], -2)

    def part(k):
        ck, sk = (c[..., k], s[..., k]) if derivative != k else (-s[..., k], c[..., k])
        u = one if derivative != k else zero
        if k == 0:
            return mat([[ck, -sk, zero], [sk, ck, zero], [zero, zero, u]])
        if k == 1:
            return mat([[u, zero, zero], [zero, ck, -sk], [zero, sk, ck]])
        return mat([[ck, zero, sk], [zero, u, zero], [-sk, zero, ck]])

    return part(0) @ part(1) @ part(2)


def corners_host(boxes: np.ndarray) -> np.ndarray:
    """``(n,8,3)``: ``bbox_to_corners`` of ``boxes (n,9)``."""
    b = np.asarray(boxes, np.float64).reshape(-1, 9)
    local = SIGNS[None] * (b[:, None, 3:6] / 2)
    return b[:, None, :3] + np.einsum("nij,nkj->nki", euler_matrix(b[:, 6:]), local)


# ------------------------------------------------------------------------------------------------------------------ the IoU
class _Box:
    """A box in the pair's frame: centre, half sizes and the three axes (the columns of R) as tuples of Python floats."""

    def __init__(self, c, size, angles):
        R = euler_matrix(np.asarray(angles, np.float64))
        self.c = tuple(float(v) for v in c)
        self.h = tuple(float(v) / 2 for v in size)
        self.ax = tuple(tuple(float(R[r, m]) for r in range(3)) for m in range(3))

    def dist(self, f, p):
        """The signed distance of ``p`` to the plane of face ``f = 2 m + (sigma < 0)``, positive outside."""
        m, sg = f >> 1, (1.0 if f & 1 == 0 else -1.0)
        a, c = self.ax[m], self.c
        return sg * (a[0] * (p[0] - c[0]) + a[1] * (p[1] - c[1]) + a[2] * (p[2] - c[2])) - self.h[m]

    def normal(self, f):
        sg = 1.0 if f & 1 == 0 else -1.0
        return tuple(sg * v for v in self.ax[f >> 1])

    def quad(self, f):
        m, sg = f >> 1, (1.0 if f & 1 == 0 else -1.0)
        u, v = (m + 1) % 3, (m + 2) % 3
        out = []
        for su, sv in _QUAD:
            out.append(tuple(self.c[r] + sg * self.h[m] * self.ax[m][r] + su * self.h[u] * self.ax[u][r] + sv * self.h[v] * self.ax[v][r]
                             for r in range(3)))
        return out


def _coplanar(A: _Box, i: int, qa, B: _Box, j: int, qb, tol: float) -> int:
    """0: not coplanar; +1: coplanar and facing the same way; -1: coplanar and facing each other."""
    d = 0.0
    for p in qa:
        d = max(d, abs(B.dist(j, p)))
    for p in qb:
        d = max(d, abs(A.dist(i, p)))
    if not d <= tol:
        return 0
    na, nb = A.normal(i), B.normal(j)
    return 1 if na[0] * nb[0] + na[1] * nb[1] + na[2] * nb[2] > 0 else -1


def _clip(poly, Y: _Box, j: int):
    d = [Y.dist(j, p) for p in poly]
    out = []
    n = len(poly)
    for k in range(n):
        k2 = (k + 1) % n
        ins, ins2 = d[k] <= 0, d[k2] <= 0
        if ins:
            out.append(poly[k])
        if ins != ins2:
            (pi, di), (po, do) = ((poly[k], d[k]), (poly[k2], d[k2])) if ins else ((poly[k2], d[k2]), (poly[k], d[k]))
            t = di / (di - do)
            out.append(tuple(pi[r] + t * (po[r] - pi[r]) for r in range(3)))
    return out[:MAX_POLY]


def _face_volume(poly, normal, height) -> float:
    if len(poly) < 3:
        return 0.0
    sx = sy = sz = 0.0
    p0 = poly[0]
    for k in range(1, len(poly) - 1):
        a = tuple(poly[k][r] - p0[r] for r in range(3))
        b = tuple(poly[k + 1][r] - p0[r] for r in range(3))
        sx += a[1] * b[2] - a[2] * b[1]
        sy += a[2] * b[0] - a[0] * b[2]
        sz += a[0] * b[1] - a[1] * b[0]
    area = 0.5 * abs(normal[0] * sx + normal[1] * sy + normal[2] * sz)
    return height * area / 3.0


def _pair_iou(b1: np.ndarray, b2: np.ndarray) -> float:
    if not (np.isfinite(b1).all() and np.isfinite(b2).all() and (b1[3:6] > 0).all() and (b2[3:6] > 0).all()):
        return math.nan
    va, vb = float(np.prod(b1[3:6])), float(np.prod(b2[3:6]))
    A, B = _Box((0.0, 0.0, 0.0), b1[3:6], b1[6:9]), _Box(b2[:3] - b1[:3], b2[3:6], b2[6:9])
    ra, rb = math.sqrt(sum(v * v for v in A.h)), math.sqrt(sum(v * v for v in B.h))
    vi = 0.0
    if sum(v * v for v in B.c) <= (ra + rb) ** 2:
        tol = COPLANAR_TOL * float(max(b1[3:6].max(), b2[3:6].max()))
        qa, qb = [A.quad(f) for f in range(6)], [B.quad(f) for f in range(6)]
        cop = [[_coplanar(A, i, qa[i], B, j, qb[j], tol) for j in range(6)] for i in range(6)]
        for f in range(12):                                  # the first box's faces, then the second's: the order of the sum
            first = f < 6
            X, Y, fx = (A, B, f) if first else (B, A, f - 6)
            poly = (qa if first else qb)[fx]
            for j in range(6):
                flag = cop[fx][j] if first else cop[j][fx]
                if flag == 1 and first:
                    continue                                 # the shared surface: this face stands for it
                if flag != 0:
                    poly = []
                    break
                poly = _clip(poly, Y, j)
                if len(poly) < 3:
                    break
            n = X.normal(fx)
            height = X.h[fx >> 1] + (n[0] * X.c[0] + n[1] * X.c[1] + n[2] * X.c[2])
            vi += _face_volume(poly, n, height)
        vi = min(max(vi, 0.0), min(va, vb))
    return vi / (va + vb - vi)


def box_iou3d_host(boxes1: np.ndarray, boxes2: np.ndarray) -> np.ndarray:
    """``(N,M) float64``: ``vol(A n B) / (vol A + vol B - vol(A n B))`` for every pair; NaN for a box with a NaN, an inf or a
    non-positive size."""
    b1, b2 = np.asarray(boxes1, np.float64).reshape(-1, 9), np.asarray(boxes2, np.float64).reshape(-1, 9)
    out = np.empty((len(b1), len(b2)), np.float64)
    for i in range(len(b1)):
        for j in range(len(b2)):
            out[i, j] = _pair_iou(b1[i], b2[j])
    return out


# ------------------------------------------------------------------------------------------------------------------ costs and matching
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def cost_host(scores: np.ndarray, boxes: np.ndarray, text_token_mask: np.ndarray, gt_boxes: Sequence[np.ndarray],
              positive_maps: Sequence[np.ndarray], alpha: float = 0.25, gamma: float = 2.0, weights=(1.0, 2.0, 2.0),
              iou: Optional[np.ndarray] = None) -> List[List[np.ndarray]]:
    """``cost[l][b] (K,G_b)``: ``weights[0]`` BinaryFocalLossCost over the unmasked tokens + ``weights[1]`` L1 of the nine box values
    - ``weights[2]`` IoU.  ``iou (NL,K,sum G)``: replaces the host's own IoU."""
    scores, boxes = np.asarray(scores, np.float64), np.asarray(boxes, np.float64)
    mask = np.asarray(text_token_mask, bool)
    NL, B, K, _ = scores.shape
    out, lo = [[None] * B for _ in range(NL)], 0
    for b in range(B):
        gt, y = np.asarray(gt_boxes[b], np.float64).reshape(-1, 9), np.asarray(positive_maps[b], np.float64)
        idx = np.nonzero(mask[b])[0]
        y = y.reshape(len(gt), scores.shape[3])[:, idx]
        for l in range(NL):
            p = _sigmoid(scores[l, b][:, idx])
            neg = -np.log(1 - p + 1e-12) * (1 - alpha) * p ** gamma
            pos = -np.log(p + 1e-12) * alpha * (1 - p) ** gamma
            cls = pos @ y.T + neg @ (1 - y).T
            l1 = np.abs(boxes[l, b][:, None, :] - gt[None]).sum(-1)
            ov = box_iou3d_host(boxes[l, b], gt) if iou is None else np.asarray(iou, np.float64)[l, :, lo:lo + len(gt)]
            out[l][b] = weights[0] * cls + weights[1] * l1 - weights[2] * ov
        lo += len(gt)
    return out


def assign_host(costs: List[List[np.ndarray]], K: int) -> np.ndarray:
    """``assign (NL,B,K) int32``: scipy's ``linear_sum_assignment`` on ``nan_to_num(cost, 100, 100, -100)``; -1 where unmatched."""
    from scipy.optimize import linear_sum_assignment
    NL, B = len(costs), len(costs[0])
    out = np.full((NL, B, K), -1, np.int32)
    for l in range(NL):
        for b in range(B):
            c = costs[l][b]
            if c.shape[1] == 0 or c.shape[0] == 0:
                continue
            rows, cols = linear_sum_assignment(np.nan_to_num(c, nan=100.0, posinf=100.0, neginf=-100.0))
            out[l, b, rows] = cols
    return out


SAP_MAX_ROWS, SAP_MAX_COLS = 256, 1024                     # the device solver's limits on min(K, G_b) and max(K, G_b)


def _sap(C: np.ndarray) -> np.ndarray:
    """``col4row (n)`` of the ``n x m`` float64 matrix ``C`` (``n <= m``, every entry finite): one augmentation per row in increasing
    index, every loop bounded as the kernel bounds it."""
    n, m = C.shape
    u, v = np.zeros(n), np.zeros(m)
    col4row, row4col = np.full(n, -1, np.int64), np.full(m, -1, np.int64)
    for cur in range(n):
        spc = np.full(m, np.inf)                            # the shortest path cost to every column
        path = np.full(m, -1, np.int64)
        remaining = np.ones(m, bool)
        tree, reached = [], []                              # the matched rows the tree took in, the path cost at which each was reached
        min_val, i, sink = 0.0, cur, -1
        for _ in range(n + 1):
            r = ((min_val + C[i]) - u[i]) - v               # in this order: the kernel forms the same doubles
            better = remaining & (r < spc)
            spc[better], path[better] = r[better], i
            lowest = spc[remaining].min()
            if not lowest < np.inf:
                return col4row
            j = int(np.nonzero(remaining & (spc == lowest))[0][0])          # THE TIE RULE: the lowest column index
            min_val = lowest
            remaining[j] = False
            if row4col[j] < 0:
                sink = j
                break
            i = int(row4col[j])
            tree.append(i)
            reached.append(lowest)                          # = spc[col4row[i]]: a scanned column's path cost no longer moves
        if sink < 0:
            return col4row
        u[cur] = u[cur] + min_val
        for i, d in zip(tree, reached):
            u[i] = u[i] + (min_val - d)
        v[~remaining] = v[~remaining] - (min_val - spc[~remaining])
        j = sink
        for _ in range(len(tree) + 1):                      # walk back from the sink
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row


def sap_assign_host(cost: np.ndarray, G: Sequence[int], B: int) -> np.ndarray:
    """``assign (NL,B,K) int32`` of ``cost (NL,K,sum G)`` as ``ptx_gl_cost`` leaves it: the specification of ``ptx_gl_assign``
    (``hungarian_assign(matcher='device')``), which the device reproduces bit for bit.  No scipy: the rectangular shortest-augmenting-path
    method (Jonker-Volgenant as Crouse states it, which is what scipy runs) written out, per (layer, scene) on the scene's ``K x G_b``
    column range.

    * Every entry is mapped as it is read, as ``hungarian_assign``'s host path maps it: NaN -> 100, +inf -> 100, -inf -> -100; fp32
      values widened to float64.
    * The smaller side supplies the rows, ``n = min(K, G_b)``, augmented in increasing index; the larger side the columns.
    * Duals, path costs and every comparison in float64; a path cost is ``((min_val + c) - u[i]) - v[j]``, a dual moves by
      ``u[i] + (min_val - spc[col4row[i]])`` and ``v[j] - (min_val - spc[j])``: additions and subtractions only, in this order.
    * THE TIE RULE: among the columns not yet scanned that share the smallest path cost, the one with the LOWEST COLUMN INDEX is
      scanned next -- whether it is free or matched.  (scipy prefers a free column and otherwise the last of its shrinking list; on a
      tie both matchings are optimal, the pairs may differ.)
    * ``n`` augmentations of at most ``n + 1`` tree steps each.  All entries are finite after the mapping, so a step always finds a
      column; if it ever did not, the problem stops and the rows it has not matched keep -1.
    A scene without a box, and ``K = 0``, give -1 everywhere."""
    cost = np.asarray(cost)
    NL, K, SG = cost.shape
    if len(G) != B or sum(G) != SG:
        raise ValueError(f"sap_assign_host: {B} box counts that sum to {SG} expected, got {list(G)}")
    mapped = np.nan_to_num(cost.astype(np.float64), nan=100.0, posinf=100.0, neginf=-100.0)
    out = np.full((NL, B, K), -1, np.int32)
    lo = 0
    for b in range(B):
        if G[b] and K:
            for l in range(NL):
                C = mapped[l][:, lo:lo + G[b]]
                if G[b] > K:                                # the rows are the queries
                    out[l, b] = _sap(C)
                else:                                       # the rows are the boxes
                    col4row = _sap(np.ascontiguousarray(C.T))
                    matched = col4row >= 0
                    out[l, b, col4row[matched]] = np.nonzero(matched)[0]
        lo += G[b]
    return out


# ------------------------------------------------------------------------------------------------------------------ the loss
def _corners_one(box: np.ndarray) -> np.ndarray:
    """The corners of one box by the one expression both sides of a Chamfer term use: a prediction equal to its target is at distance
    exactly 0."""
    return box[:3] + (SIGNS * (box[3:6] / 2)) @ euler_matrix(box[6:9]).T


def _chamfer(src_box: np.ndarray, tgt_corners: np.ndarray):
    """One Chamfer term of one pair: ``sum_k min_j |S_k - T_j|_1`` and its gradient by the nine values of the source box."""
    R = euler_matrix(src_box[6:9])
    local = SIGNS * (src_box[3:6] / 2)
    S = _corners_one(src_box)
    dist = np.abs(S[:, None, :] - tgt_corners[None]).sum(-1)
    j = dist.argmin(1)                                       # ties: the lower corner
    value = dist[np.arange(8), j].sum()
    sgn = np.sign(S - tgt_corners[j])                        # d|u|/du, 0 at 0
    g = np.zeros(9)
    g[:3] = sgn.sum(0)
    g[3:6] = ((sgn @ R) * SIGNS).sum(0) / 2
    for k in range(3):
        g[6 + k] = (sgn * (local @ euler_matrix(src_box[6:9], k).T)).sum()
    return value, g


def loss_host(scores: np.ndarray, boxes: np.ndarray, text_token_mask: np.ndarray, gt_boxes: Sequence[np.ndarray],
              positive_maps: Sequence[np.ndarray], assign: np.ndarray, alpha: float = 0.25, gamma: float = 2.0,
              decouple_weights=(0.2, 0.2, 0.2, 0.4), avg_factor: Optional[float] = None, loss_weights=(1.0, 1.0),
              upstream_cls: Optional[np.ndarray] = None, upstream_bbox: Optional[np.ndarray] = None) -> dict:
    """``loss_by_feat_single`` for every layer: ``loss_cls (NL,)``, ``loss_bbox (NL,)`` and the gradients ``dscores``, ``dboxes`` of
    ``sum_l upstream_cls[l] loss_cls[l] + upstream_bbox[l] loss_bbox[l]`` (ones by default).  ``avg_factor``: the classification
    divisor before the ``+ float32 eps`` (default ``max(matched pairs of a layer, 1)``)."""
    scores, boxes = np.asarray(scores, np.float64), np.asarray(boxes, np.float64)
    mask, assign = np.asarray(text_token_mask, bool), np.asarray(assign)
    NL, B, K, M = scores.shape
    T = mask.shape[1]
    up_c = np.ones(NL) if upstream_cls is None else np.asarray(upstream_cls, np.float64)
    up_b = np.ones(NL) if upstream_bbox is None else np.asarray(upstream_bbox, np.float64)
    gts = [np.asarray(g, np.float64).reshape(-1, 9) for g in gt_boxes]
    pms = [np.asarray(p, np.float64).reshape(len(g), M) for p, g in zip(positive_maps, gts)]
    gt_corners = [[_corners_one(box) for box in g] for g in gts]
    loss_cls, loss_bbox = np.zeros(NL), np.zeros(NL)
    dscores, dboxes = np.zeros_like(scores), np.zeros_like(boxes)
    for l in range(NL):
        P = int((assign[l] >= 0).sum())
        if P == 0:
            raise ValueError("loss: no matched pair in the batch (every scene is without a ground-truth box)")
        avg = max(float(P), 1.0) if avg_factor is None else float(avg_factor)
        for b in range(B):
            idx = np.nonzero(mask[b])[0]
            x = scores[l, b][:, idx]
            y = np.zeros_like(x)
            for q in np.nonzero(assign[l, b] >= 0)[0]:
                y[q] = pms[b][assign[l, b, q]][idx]
            p = _sigmoid(x)
            pt = (1 - p) * y + p * (1 - y)
            aw = alpha * y + (1 - alpha) * (1 - y)
            bce = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
            loss_cls[l] += (bce * aw * pt ** gamma).sum()
            dx = (p - y) * aw * pt ** gamma + bce * aw * gamma * pt ** (gamma - 1) * (1 - 2 * y) * p * (1 - p)
            dscores[l, b][:, idx] = dx * (up_c[l] * loss_weights[0] / (avg + F32_EPS))
            for q in np.nonzero(assign[l, b] >= 0)[0]:
                g = assign[l, b, q]
                pred, tgt = boxes[l, b, q], gts[b][g]
                sources = (np.concatenate([pred[:3], tgt[3:]]), np.concatenate([tgt[:3], pred[3:6], tgt[6:]]),
                           np.concatenate([tgt[:6], pred[6:]]), pred)
                keep = (slice(0, 3), slice(3, 6), slice(6, 9), slice(0, 9))
                for w, src, sl in zip(decouple_weights, sources, keep):
                    value, grad = _chamfer(src, gt_corners[b][g])
                    loss_bbox[l] += w * value
                    dboxes[l, b, q, sl] += w * grad[sl] * (up_b[l] * loss_weights[1] / (P * 8))
        loss_cls[l] *= loss_weights[0] / (avg + F32_EPS)
        loss_bbox[l] *= loss_weights[1] / (P * 8)
    return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, dscores=dscores, dboxes=dboxes)


def loss_dict(loss_cls, loss_bbox) -> dict:
    """The reference's dict: the last layer first, then ``d{i}.*`` for the layers ``0 .. NL - 2``."""
    out = {"loss_cls": loss_cls[-1], "loss_bbox": loss_bbox[-1]}
    for i in range(len(loss_cls) - 1):
        out[f"d{i}.loss_cls"], out[f"d{i}.loss_bbox"] = loss_cls[i], loss_bbox[i]
    return out


def predict_host(scores: np.ndarray, boxes: np.ndarray):
    """``predict_by_feat``: the last layer's boxes and ``max_t sigmoid(x)`` per query (a ``-inf`` column gives 0)."""
    s = np.asarray(scores, np.float64)[-1]
    with np.errstate(over="ignore"):
        return np.asarray(boxes, np.float64)[-1], _sigmoid(s).max(-1)
