"""The grounding loss (proxytransformation_amd/grounding_loss.py, grounding_loss_host.py) pinned without a GPU: the IoU specification
against Qhull and against closed forms (coplanar faces included), the costs, the loss and its gradients against the reference's torch
lines typed out here in float64 (match_cost.py:227-237, chamfer_distance.py:58-63 and 160-203, grounding_head.py:686-824, mmdet's sigmoid
focal loss) and against ``torch.autograd`` on them, the matching's edge cases, the module's refusals and the ABI rows."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import GroundingLoss, _abi, grounding_loss, grounding_loss_host as gh
from tests import grounding_loss_util as gu
from tests import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the IoU
def test_iou_specification_is_qhull_on_random_pairs():
    A, B = gu.random_boxes(300, 1), gu.random_boxes(300, 2)
    ref = np.array([gu.qhull_iou(a, b) for a, b in zip(A, B)])
    overlapping = float((ref > 1e-3).mean())
    print(f"{overlapping:.0%} of the pairs overlap by more than 1e-3")
    assert overlapping >= 0.60                                # the test cannot pass on empty intersections
    got = np.array([gh.box_iou3d_host(a[None], b[None])[0, 0] for a, b in zip(A, B)])
    err = float(np.abs(got - ref).max())
    print(f"max |IoU - Qhull| = {err:.2e}")
    assert err <= 1e-9
    assert np.array_equal(gh.box_iou3d_host(A[:4], B[:3]), np.array([[gh.box_iou3d_host(a[None], b[None])[0, 0] for b in B[:3]] for a in A[:4]]))


@pytest.mark.parametrize("name,b1,b2,want", gu.closed_forms(), ids=[c[0] for c in gu.closed_forms()])
def test_iou_closed_forms_hold_in_both_orders(name, b1, b2, want):
    tol = gu.ULP_TOL if "ulp" in name else 1e-9
    for x, y in ((b1, b2), (b2, b1)):
        got = float(gh.box_iou3d_host(x[None], y[None])[0, 0])
        assert 0.0 <= got <= 1.0 and abs(got - want) <= tol, (name, got, want)


def test_iou_on_grid_aligned_boxes_is_the_interval_closed_form():
    """Centres on a 0.25 grid, sizes multiples of 0.5, right angles only: flush, touching and coinciding faces in most pairs, which
    is where the coplanarity rule decides.  Also with the inputs rounded to fp32 (pi/2 is then 4e-8 off a right angle): the error
    stays within the rule's bound, 1e-5 x max size x area / volume <= 1e-5 x 2 / 0.5."""
    A, B = gu.grid_boxes(25, 41), gu.grid_boxes(25, 42)
    ref = np.array([[gu.axis_aligned_iou(a, b) for b in B] for a in A])
    assert (ref > 0).mean() >= 0.25 and (ref == 0).mean() >= 0.25
    got = gh.box_iou3d_host(A, B)
    assert float(np.abs(got - ref).max()) <= 1e-9
    rounded = gh.box_iou3d_host(A.astype(np.float32), B.astype(np.float32))
    assert float(np.abs(rounded - ref).max()) <= 4e-5


def test_iou_of_a_nan_or_non_positive_box_is_nan_for_its_pairs_only():
    A, B = gu.random_boxes(4, 3), gu.random_boxes(3, 4)
    A[1, 7], B[2, 4], A[3, 3] = np.nan, 0.0, -0.5
    got = gh.box_iou3d_host(A, B)
    bad = np.zeros((4, 3), bool)
    bad[1], bad[3], bad[:, 2] = True, True, True
    assert np.array_equal(np.isnan(got), bad) and ((got[~bad] >= 0) & (got[~bad] <= 1)).all()
    assert gh.box_iou3d_host(A[:0], B).shape == (0, 3) and gh.box_iou3d_host(A, B[:0]).shape == (4, 0)


def test_rotation_and_corners_follow_the_zxy_convention():
    a = np.array([0.5, -0.8, 1.2])
    assert np.abs(gh.euler_matrix(a) - gu.rotation_zxy(a)).max() <= 1e-15
    h = 1e-6
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        assert np.abs(gh.euler_matrix(a, k) - (gu.rotation_zxy(a + d) - gu.rotation_zxy(a - d)) / (2 * h)).max() <= 1e-8
    box = np.array([1.0, 2.0, 3.0, 0.4, 0.6, 0.8, *a])
    assert np.abs(gh.corners_host(box[None])[0] - bbox_to_corners(torch.from_numpy(box)[None])[0].numpy()).max() <= 1e-15


# ------------------------------------------------------------------------------------------------------------------ the reference's lines
def euler_zxy(angles):
    """pytorch3d's ``euler_angles_to_matrix(angles, 'ZXY')`` in torch."""
    c, s = torch.cos(angles), torch.sin(angles)
    one, zero = torch.ones_like(c[..., 0]), torch.zeros_like(c[..., 0])
    rz = torch.stack([c[..., 0], -s[..., 0], zero, s[..., 0], c[..., 0], zero, zero, zero, one], -1).reshape(angles.shape[:-1] + (3, 3))
    rx = torch.stack([one, zero, zero, zero, c[..., 1], -s[..., 1], zero, s[..., 1], c[..., 1]], -1).reshape(angles.shape[:-1] + (3, 3))
    ry = torch.stack([c[..., 2], zero, s[..., 2], zero, one, zero, -s[..., 2], zero, c[..., 2]], -1).reshape(angles.shape[:-1] + (3, 3))
    return rz @ rx @ ry


def bbox_to_corners(bbox):
    """chamfer_distance.py:160-203."""
    rot_mat = euler_zxy(bbox[:, 6:])
    centers = bbox[:, :3].unsqueeze(1).repeat(1, 8, 1)
    half_sizes = bbox[:, 3:6].unsqueeze(1).repeat(1, 8, 1) / 2
    x = torch.tensor([1, 1, 1, 1, -1, -1, -1, -1]).unsqueeze(0).repeat(bbox.shape[0], 1)
    y = torch.tensor([1, 1, -1, -1, 1, 1, -1, -1]).unsqueeze(0).repeat(bbox.shape[0], 1)
    z = torch.tensor([1, -1, 1, -1, 1, -1, 1, -1]).unsqueeze(0).repeat(bbox.shape[0], 1)
    eight_corners = torch.stack((x, y, z), dim=-1) * half_sizes
    return centers + torch.matmul(eight_corners, rot_mat.transpose(1, 2))


def bbox_cd_loss(source, target):
    """``BBoxCDLoss(mode='l1', group='g8')``: chamfer_distance.py:58-63 with the L1 criterion, the mean of the source side."""
    src, dst = bbox_to_corners(source), bbox_to_corners(target)
    src_expand = src.unsqueeze(2).repeat(1, 1, dst.shape[1], 1)
    dst_expand = dst.unsqueeze(1).repeat(1, src.shape[1], 1, 1)
    distance = F.l1_loss(src_expand, dst_expand, reduction="none").sum(-1)
    return torch.mean(torch.min(distance, dim=2)[0])


def focal_cost(cls_pred, gt_labels, alpha=0.25, gamma=2.0, eps=1e-12):
    """match_cost.py:227-237."""
    cls_pred = cls_pred.flatten(1).sigmoid()
    gt_labels = gt_labels.flatten(1)
    neg_cost = -(1 - cls_pred + eps).log() * (1 - alpha) * cls_pred.pow(gamma)
    pos_cost = -(cls_pred + eps).log() * alpha * (1 - cls_pred).pow(gamma)
    return torch.einsum("nc,mc->nm", pos_cost, gt_labels) + torch.einsum("nc,mc->nm", neg_cost, (1 - gt_labels))


def layer_loss(cls_scores, pred_bboxes, mask, gts, pms, assign, alpha=0.25, gamma=2.0, weights=(0.2, 0.2, 0.2, 0.4)):
    """``loss_by_feat_single`` (grounding_head.py:686-824) of one layer with the matching given: ``(loss_cls, loss_bbox)``."""
    B, K, M = cls_scores.shape
    labels = torch.zeros((B, K, M), dtype=cls_scores.dtype)
    for b in range(B):
        for q in range(K):
            if assign[b, q] >= 0:
                labels[b, q] = pms[b][assign[b, q]]
    text_masks = torch.zeros((B, M), dtype=torch.bool)
    text_masks[:, :mask.shape[1]] = mask
    text_mask = text_masks.unsqueeze(1).repeat(1, K, 1)
    pred, target = torch.masked_select(cls_scores, text_mask), torch.masked_select(labels, text_mask)
    num_total_pos = int((assign >= 0).sum())
    p = pred.sigmoid()                                       # mmdet's py_sigmoid_focal_loss and weight_reduce_loss
    pt = (1 - p) * target + p * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    loss_cls = (F.binary_cross_entropy_with_logits(pred, target, reduction="none") * focal_weight).sum() / \
        (max(num_total_pos, 1) + torch.finfo(torch.float32).eps)
    valid = torch.from_numpy(assign.reshape(-1) >= 0)
    preds = pred_bboxes.reshape(-1, 9)[valid]
    targets = torch.cat([gts[b][assign[b][assign[b] >= 0]] for b in range(B)])
    loss_bbox = weights[0] * bbox_cd_loss(torch.cat((preds[:, :3], targets[:, 3:6], targets[:, 6:]), -1), targets)
    loss_bbox = loss_bbox + weights[1] * bbox_cd_loss(torch.cat((targets[:, :3], preds[:, 3:6], targets[:, 6:]), -1), targets)
    loss_bbox = loss_bbox + weights[2] * bbox_cd_loss(torch.cat((targets[:, :3], targets[:, 3:6], preds[:, 6:]), -1), targets)
    loss_bbox = loss_bbox + weights[3] * bbox_cd_loss(preds, targets)
    return loss_cls, loss_bbox


@pytest.mark.parametrize("shape", ["small", "wave"])
def test_costs_are_the_reference_lines_with_qhull_for_the_iou(shape):
    scores, boxes, mask, gts, pms = gu.batch(**gu.SHAPES[shape])
    costs = gh.cost_host(scores, boxes, mask, gts, pms)
    NL, B, K, _ = scores.shape
    for l in range(NL):
        for b in range(B):
            idx = torch.nonzero(torch.from_numpy(mask[b])).squeeze(-1)
            cls = focal_cost(torch.from_numpy(scores[l, b])[:, idx], torch.from_numpy(pms[b])[:, idx])
            l1 = torch.cdist(torch.from_numpy(boxes[l, b]), torch.from_numpy(gts[b]), p=1)
            iou = np.array([[gu.qhull_iou(p, g) for g in gts[b]] for p in boxes[l, b]]).reshape(K, len(gts[b]))
            ref = cls.numpy() + 2.0 * l1.numpy() - 2.0 * iou
            assert costs[l][b].shape == (K, len(gts[b]))
            if ref.size:
                assert np.isfinite(costs[l][b]).all()
                assert float(np.abs(costs[l][b] - ref).max()) <= 1e-10 * gu.scale(ref)


def test_assignment_without_ground_truth_and_with_more_of_it_than_queries():
    scores, boxes, mask, gts, pms = gu.batch(**gu.SHAPES["small"])
    assign = gh.assign_host(gh.cost_host(scores, boxes, mask, gts, pms), 5)
    assert assign.shape == (2, 3, 5) and assign.dtype == np.int32
    assert (assign[:, 1] == -1).all()                                                      # G = 0
    assert ((assign[:, 0] >= 0).sum(-1) == 3).all() and ((assign[:, 2] >= 0).sum(-1) == 5).all()      # G = 3 < K; G = 7 > K: K pairs
    for l in range(2):
        assert sorted(assign[l, 0][assign[l, 0] >= 0].tolist()) == [0, 1, 2] and len(set(assign[l, 2].tolist())) == 5
    nan = [[np.full((5, 2), np.nan)]]                        # nan_to_num: a NaN cost is 100, the matching still comes back
    assert (gh.assign_host(nan, 5)[0, 0] >= 0).sum() == 2


@pytest.mark.parametrize("shape", ["small", "wave", "full"])
def test_loss_and_gradients_are_the_reference_lines_and_autograd(shape):
    scores, boxes, mask, gts, pms = gu.batch(**gu.SHAPES[shape])
    NL, B, K, M = scores.shape
    assign = gh.assign_host(gh.cost_host(scores, boxes, mask, gts, pms), K)
    rng = np.random.default_rng(5)
    up_c, up_b = rng.uniform(0.5, 2.0, NL), rng.uniform(0.5, 2.0, NL)
    got = gh.loss_host(scores, boxes, mask, gts, pms, assign, upstream_cls=up_c, upstream_bbox=up_b)
    ts = torch.from_numpy(np.where(np.isfinite(scores), scores, 0.0)).requires_grad_()       # (the reference never reads a masked score)
    tb = torch.from_numpy(boxes).requires_grad_()
    total = 0
    for l in range(NL):
        lc, lb = layer_loss(ts[l], tb[l], torch.from_numpy(mask), [torch.from_numpy(g) for g in gts], [torch.from_numpy(p) for p in pms], assign[l])
        assert abs(got["loss_cls"][l] - float(lc.detach())) <= 1e-10 * abs(float(lc.detach())) and abs(got["loss_bbox"][l] - float(lb.detach())) <= 1e-10 * abs(float(lb.detach()))
        total = total + up_c[l] * lc + up_b[l] * lb
    total.backward()
    gu.close(got["dscores"], ts.grad.numpy(), 1e-10)
    gu.close(got["dboxes"], tb.grad.numpy(), 1e-10)
    full = np.zeros((B, M), bool)
    full[:, :mask.shape[1]] = mask
    assert not got["dscores"][np.broadcast_to(~full[None, :, None, :], got["dscores"].shape)].any() and not got["dboxes"][assign < 0].any() and got["dboxes"][assign >= 0].any()
    d = gh.loss_dict(got["loss_cls"], got["loss_bbox"])
    assert list(d)[:2] == ["loss_cls", "loss_bbox"] and len(d) == 2 * NL and d["loss_cls"] == got["loss_cls"][-1]
    if NL > 1:
        assert d["d0.loss_bbox"] == got["loss_bbox"][0]


def test_a_prediction_on_its_target_costs_nothing_and_a_batch_without_pairs_raises():
    scores, boxes, mask, gts, pms = gu.batch(**gu.SHAPES["full"])
    assign = np.full((1, 1, 3), -1, np.int32)
    assign[0, 0, 1] = 0
    boxes[0, 0, 1] = gts[0][0]
    got = gh.loss_host(scores, boxes, mask, gts, pms, assign)
    assert got["loss_bbox"][0] == 0.0 and np.isfinite(got["dboxes"]).all() and not got["dboxes"].any()
    with pytest.raises(ValueError, match="no matched pair"):
        gh.loss_host(scores, boxes, mask, gts, pms, np.full((1, 1, 3), -1, np.int32))


def test_predict_gives_zero_under_minus_infinity():
    s = np.full((2, 1, 3, 8), -np.inf)
    s[1, 0, 0, 2], s[1, 0, 1, :3] = 0.0, (1.0, -2.0, 3.0)
    boxes, score = gh.predict_host(s, np.zeros((2, 1, 3, 9)))
    assert boxes.shape == (1, 3, 9) and np.allclose(score, [[0.5, 1 / (1 + math.exp(-3.0)), 0.0]])


# ------------------------------------------------------------------------------------------------------------------ the module
def test_refusals_name_their_arguments():
    for kw, match in ((dict(norm_decouple_loss=True), "norm_decouple_loss"), (dict(decouple_groups=3), "decouple_groups=3"),
                      (dict(loss_bbox=dict(type="BBoxCDLoss", mode="l1", group="g4")), "group='g4'"),
                      (dict(loss_bbox=dict(type="BBoxCDLoss", mode="l2", group="g8")), "mode='l2'"),
                      (dict(loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False)), "loss_cls"),
                      (dict(loss_cls=dict(type="mmdet.FocalLoss", use_sigmoid=False)), "loss_cls"),
                      (dict(train_cfg=dict(assigner=dict(type="HungarianAssigner3D", match_costs=[dict(type="ClassificationCost", weight=1.0)]))),
                       "match_costs"), (dict(num_reg=12), "num_reg=12"), (dict(box_coder="FCAF"), "FCAF")):
        with pytest.raises(NotImplementedError, match=match):
            GroundingLoss(**kw)
    m = GroundingLoss(num_classes=256, sync_cls_avg_factor=True, decouple_bbox_loss=True, decouple_groups=4, share_pred_layer=True,
                      decouple_weights=[0.2, 0.2, 0.2, 0.4], contrastive_cfg=dict(max_text_len=256, log_scale="auto", bias=True),
                      loss_cls=dict(type="mmdet.FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                      loss_bbox=dict(type="BBoxCDLoss", mode="l1", loss_weight=1.0, group="g8"),
                      train_cfg=dict(assigner=dict(type="HungarianAssigner3D", match_costs=[dict(type="BinaryFocalLossCost", weight=1.0),
                                                                                          dict(type="BBox3DL1Cost", weight=2.0),
                                                                                          dict(type="IoU3DCost", weight=2.0)])))
    assert m.cost_weights == (1.0, 2.0, 2.0) and m.decouple_weights == [0.2, 0.2, 0.2, 0.4] and (m.alpha, m.gamma) == (0.25, 2.0)
    assert not list(m.parameters()) and GroundingLoss(decouple_bbox_loss=False).decouple_weights == [0.0, 0.0, 0.0, 1.0]
    s, b, mask = torch.zeros(1, 1, 2, 256), torch.zeros(1, 1, 2, 9), torch.ones(1, 4, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.loss(s, b, mask, [torch.zeros(1, 9)], [torch.zeros(1, 256)])
    for call in (lambda: grounding_loss.box_iou3d(torch.zeros(1, 9), torch.zeros(1, 9)), lambda: grounding_loss.predict_scores(s),
                 lambda: m.predict(s, b), lambda: m.assign(s, b, mask, [torch.zeros(1, 9)], [torch.zeros(1, 256)])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_header_binding_and_exports_declare_the_entry_points():
    lib = _abi.lib()
    hooks = ctypes.CDLL(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip_testhooks.so"))
    for name, params in su.assert_declared(gu.GL_ENTRY_POINTS).items():
        assert len(params.split(",")) == len(_abi.SIGNATURES[name][1]), name
        getattr(hooks, name)
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13 and hooks.ptx_abi_version() == 13
    assert "grounding_loss.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()


def test_argument_checks_answer_einval_before_touching_a_device():
    lib = _abi.lib()
    EINVAL = -1
    err = lambda: lib.ptx_last_error()                       # noqa: E731
    assert lib.ptx_gl_iou(None, 0, None, 3, None, None) == EINVAL and b"N=0" in err()
    assert lib.ptx_gl_iou(None, 2, None, 3, None, None) == EINVAL and b"null" in err()
    cost = lambda NL=2, K=5, M=16, T=7, SG=3, alpha=0.25, gamma=2.0: lib.ptx_gl_cost(      # noqa: E731
        None, None, NL, 3, K, M, None, T, None, None, None, SG, alpha, gamma, 1.0, 2.0, 2.0, None, None)
    assert cost(NL=65) == EINVAL and b"NL=65" in err() and cost(K=1025) == EINVAL and b"K=1025" in err()
    assert cost(T=17) == EINVAL and b"T=17" in err() and cost(M=257, T=7) == EINVAL and b"M=257" in err()
    assert cost(SG=0) == EINVAL and b"SG=0" in err() and cost(gamma=0.5) == EINVAL and b"gamma=0.5" in err()
    assert cost() == EINVAL and b"null" in err()
    assert lib.ptx_gl_loss_fwd(None, None, 2, 3, 5, 16, None, 7, None, None, None, 3, None, 0.25, 2.0, None, 1.0, 1.0, None, None, None,
                               None) == EINVAL and b"null" in err()
    assert lib.ptx_gl_loss_bwd(None, None, 2, 65, 5, 16, None, 7, None, None, None, 3, None, 0.25, 2.0, None, 1.0, 1.0, None, None, None, None,
                               None, None) == EINVAL and b"B=65" in err()
    assert lib.ptx_gl_predict(None, 0, 16, None, None) == EINVAL and b"n=0" in err()
    assert lib.ptx_gl_predict(None, 4, 300, None, None) == EINVAL and b"M=300" in err()


# ------------------------------------------------------------------------------------------------------------------ preconditions of the edge tests
# (tests/test_gpu_grounding_loss_edges.py): what its inputs must be for its assertions to mean something, held on the specification alone
def _diag_iou(A, B):
    return np.array([gh.box_iou3d_host(a[None], b[None])[0, 0] for a, b in zip(A, B)])


@pytest.mark.parametrize("regime", gu.IOU_REGIMES)
def test_iou_regimes_overlap_and_are_well_conditioned(regime):
    """A regime cannot pass on empty intersections (more than half of the 576 pairs overlap, 30 % of the thin ones), and two correct
    fp32 evaluations cannot lie further apart than a quarter of the parity bound: the specification moves by at most ``PARITY / 4``
    when every input moves one fp32 ulp (72 pairs, 4 draws)."""
    A, B = gu.iou_regime(regime)
    assert A.shape == B.shape == (gu.IOU_N, 9) and np.array_equal(A, gu.f32(A)) and np.array_equal(B, gu.f32(B))
    ref = gh.box_iou3d_host(A, B)
    share = float((ref > 1e-3).mean())
    pairs = [(i, j % gu.IOU_N) for i in range(gu.IOU_N) for j in (i, i + 1, i + 7)]
    moved = gu.ulp_sensitivity(gh.box_iou3d_host, A, B, pairs)
    print(f"{regime}: {share:.0%} of 576 pairs overlap by more than 1e-3; ulp sensitivity {moved:.2e}")
    assert share > gu.OVERLAP_SHARE.get(regime, 0.5) and moved <= gu.PARITY / 4
    if regime == "thin":
        assert ((A[:, 3:6].min(-1) <= 0.05) & (B[:, 3:6].min(-1) >= 0.02)).all()
    if regime == "far":
        assert np.abs(A[:, :3]).max() > 40 and np.abs(B[:, 1]).min() > 20
    if regime == "angles":
        assert np.abs(A[:, 6:]).max() > 10 * math.pi
    if regime == "inside":                                   # the partner is met everywhere, and where it is inside by its half diagonal
        inside = gu.contained(A, B)                          # the IoU is the ratio of the volumes
        assert (np.diag(ref) > 1e-3).all() and inside.sum() >= 4 and np.abs(np.diag(ref)[inside] - 0.4 ** 3).max() <= 1e-6


@pytest.mark.parametrize("kind", ["cubes", "thin"])
def test_near_duplicates_converge_and_stay_within_the_rule_in_both_orders(kind):
    """The diagonal IoU rises to 1 with ``delta``; where the coplanarity rule starts to fire the specification's two argument orders
    differ, by less than the rule admits on the pair."""
    floors = {"cubes": {1e-1: 0.24, 1e-2: 0.86, 1e-3: 0.98, 1e-4: 0.998}, "thin": {1e-2: 0.18}}[kind]
    for delta in gu.DELTAS:
        A, B = gu.near_duplicates(kind, delta)
        fwd, bwd = _diag_iou(A, B), _diag_iou(B, A)
        print(f"{kind} delta {delta:g}: smallest IoU {fwd.min():.4f}, order asymmetry {np.abs(fwd - bwd).max():.2e}")
        assert fwd.min() >= floors.get(delta, 0.0) and (np.abs(fwd - bwd) <= gu.coplanar_admit(A, B)).all()
        if delta <= 1e-5:
            assert fwd.min() >= 0.99
    thin = gu.near_duplicates("thin", 1e-5)
    assert ((thin[0][:, 3:6].min(-1) <= 0.05)).all() and float(gu.coplanar_bound(*thin).max()) <= 3.1e-3      # not loose by orders


def test_one_box_by_two_names_is_one_box_to_the_specification():
    for name, A, B in gu.same_box_names():
        assert len(A) == 64 and (name == "itself") == np.array_equal(A, B)
        R = lambda X: gh.euler_matrix(X[:, 6:])              # noqa: E731
        if "cube" in name:                                   # the same set of face normals, another order: coplanar pairs with i != j
            assert np.abs(np.abs(np.einsum("nij,nik->njk", R(A), R(B))).max(-1) - 1).max() <= 1e-6
            assert np.abs(np.einsum("nij,nij->nj", R(A), R(B)) - 1).max() > 0.5
        else:
            assert np.abs(R(A) - R(B)).max() <= 1e-6
        for x, y in ((A, B), (B, A)):
            assert (np.abs(_diag_iou(x, y) - 1.0) <= gu.coplanar_admit(x, y)).all(), name


def test_the_specification_does_not_stick_at_a_saturated_score():
    """at ``x > 17`` an fp32 ``1 - p`` is 0 and the cost would stick at ``-log(1e-12)`` x its weight; float64 follows
    ``x``.  One token, target 0, the IoU handed in as 0."""
    one = lambda x: float(gh.cost_host(np.full((1, 1, 1, 1), x), np.zeros((1, 1, 1, 9)), np.ones((1, 1), bool), [np.zeros((1, 9))],      # noqa: E731
                                       [np.zeros((1, 1))], weights=(1.0, 0.0, 0.0), iou=np.zeros((1, 1, 1)))[0][0][0, 0])
    stuck = -math.log(1e-12) * 0.75
    assert abs(one(30.0) - stuck) > 0.05 and abs(one(30.0) - 0.75 * -math.log(math.exp(-30.0) + 1e-12)) <= 1e-3
    assert abs(one(20.0) - 0.75 * 20.0) <= 1e-2 and one(17.5) < one(20.0) < one(30.0) < stuck + 1e-9


def test_edge_batches_are_what_their_tests_say():
    c = gu.explicit_batch(NL=2, B=3, K=300, M=16, T=7, tokens=(7, 3, 1), G=(48, 48, 48), seed=41)
    assert c["assign"].shape == (2, 3, 300) and ((c["assign"] >= 0).sum(-1) == 48).all()
    rows = np.nonzero((c["assign"].reshape(2, -1) >= 0))[1]
    assert (rows >= 512).any() and (rows < 256).any()        # matched rows in every stride of the layer reduction
    for b in range(3):
        for l in range(2):
            g = c["assign"][l, b][c["assign"][l, b] >= 0]
            assert len(set(g.tolist())) == len(g) and g.max() < 48
        assert ((c["pms"][b] > 0) & (c["pms"][b] < 1)).any() and not c["pms"][b][:, 7:].any() and not c["pms"][b][:, :7][:, ~c["mask"][b]].any()
    sat = gu.saturate(c["scores"], c["mask"], 88.0, 100.0, 1)
    live = np.broadcast_to(c["mask"][None, :, None, :], sat[..., :7].shape)
    assert (np.abs(sat[..., :7][live]) >= 88).all() and (sat[..., :7][live] > 0).any() and (sat[..., :7][live] < 0).any()
    assert np.isneginf(sat[..., :7][~live]).all() and np.isneginf(sat[..., 7:]).all()
    part = gu.explicit_batch(NL=2, B=2, K=6, M=16, T=7, tokens=(7, 3), G=(4, 3), seed=42, pairs=((1, 0), (2, 2)))
    assert ((part["assign"] >= 0).sum((1, 2)) == (1, 4)).all()
    pred, gt = gu.dyadic_ties()
    S, T = gh.corners_host(pred), gh.corners_host(gt)
    dist = np.abs(S[:, :, None] - T[:, None]).sum(-1)
    ties = (dist == dist.min(-1, keepdims=True)).sum(-1)
    assert sorted(set(ties.ravel().tolist())) == [1, 2, 4, 8] or sorted(set(ties.ravel().tolist())) == [2, 4, 8], ties
    assert np.array_equal(S, S.astype(np.float32)) and ((S[:, :, None] - T[:, None]) == 0).any()
    assert (17, 48) in gu.TOKEN_EDGES and (1, 1) in gu.TOKEN_EDGES and len(gu.TOKEN_EDGES) == 15
