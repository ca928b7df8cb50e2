"""The grounding loss on the device (proxytransformation_amd/grounding_loss.py, csrc/grounding_loss.hip) against its float64
specification (grounding_loss_host.py) within the project's parity bound, 1e-4 of each tensor's scale: the box IoU on random pairs, on
every closed form and on NaN boxes; the cost matrices with ``-inf`` on the masked columns, without ground truth and with more of it than
queries; the matching; the loss, its gradients and their exact zeros; ``predict``; and the decoder's outputs through the loss."""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from proxytransformation_amd import GroundingLoss, grounding_loss as gl, grounding_loss_host as gh
from tests import decoder_util as du
from tests import grounding_loss_util as gu
from tests import query_select_util as qu
from tests import sparse_util as su

pytestmark = pytest.mark.gpu
DEV = su.DEV
TOL = gu.PARITY


def dev(a, dtype=torch.float32):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if t.is_floating_point() else t).to(DEV)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def case(shape):
    """A batch, the same values on both sides (rounded to fp32 once), the specification's costs, matching and loss on it."""
    scores, boxes, mask, gts, pms = gu.batch(**gu.SHAPES[shape])
    r = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    scores, boxes, gts, pms = r(scores), r(boxes), [r(g) for g in gts], [r(p) for p in pms]
    costs = gh.cost_host(scores, boxes, mask, gts, pms)
    assign = gh.assign_host(costs, scores.shape[2])
    rng = np.random.default_rng(7)
    up = rng.uniform(0.5, 2.0, (2, scores.shape[0]))
    loss = gh.loss_host(scores, boxes, mask, gts, pms, assign, upstream_cls=up[0], upstream_bbox=up[1])
    return dict(scores=scores, boxes=boxes, mask=mask, gts=gts, pms=pms, costs=costs, assign=assign, loss=loss, up=up)


def device_args(c):
    return dev(c["scores"]), dev(c["boxes"]), dev(c["mask"]), [dev(g) for g in c["gts"]], [dev(p) for p in c["pms"]]


# ------------------------------------------------------------------------------------------------------------------ box_iou3d
@pytest.mark.parametrize("N,M", [(37, 5), (1, 1)])
def test_iou_on_random_boxes(N, M):
    A, B = gu.random_boxes(N, 21).astype(np.float32), gu.random_boxes(M, 22).astype(np.float32)
    ref = gh.box_iou3d_host(A, B)
    got = gl.box_iou3d(dev(A), dev(B))
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, M)
    err = gu.close(got.cpu().numpy(), ref, TOL)
    print(f"({N},{M}): max |IoU - specification| = {err:.2e}, {float((ref > 1e-3).mean()):.0%} of the pairs overlap")
    assert (ref > 1e-3).mean() >= 0.5 and bits_equal(got, gl.box_iou3d(dev(A), dev(B)))


def test_iou_of_empty_lists_is_empty():
    A = dev(gu.random_boxes(3, 1))
    assert tuple(gl.box_iou3d(A[:0], A).shape) == (0, 3) and tuple(gl.box_iou3d(A, A[:0]).shape) == (3, 0)


def test_iou_closed_forms_hold_in_both_orders():
    forms = gu.closed_forms()
    b1, b2 = np.stack([f[1] for f in forms]), np.stack([f[2] for f in forms])
    fwd, bwd = gl.box_iou3d(dev(b1), dev(b2)).cpu().numpy(), gl.box_iou3d(dev(b2), dev(b1)).cpu().numpy()
    for i, (name, _, _, want) in enumerate(forms):
        tol = gu.ULP_TOL if "ulp" in name else TOL
        for got in (float(fwd[i, i]), float(bwd[i, i])):
            print(f"{name}: {got:.8f} (expected {want:.8f})")
            assert 0.0 <= got <= 1.0 and abs(got - want) <= tol, (name, got, want)


def test_iou_on_grid_aligned_boxes_is_the_interval_closed_form():
    """Flush, touching and coinciding faces in most pairs (``grounding_loss_util.grid_boxes``): the coplanarity rule at work in fp32."""
    A, B = gu.grid_boxes(25, 41).astype(np.float32), gu.grid_boxes(25, 42).astype(np.float32)
    ref = np.array([[gu.axis_aligned_iou(a, b) for b in B] for a in A.astype(np.float64)])
    got = gl.box_iou3d(dev(A), dev(B)).cpu().numpy()
    print(f"grid boxes: max |IoU - closed form| = {float(np.abs(got - ref).max()):.2e}, {float((ref > 0).mean()):.0%} of the pairs overlap")
    assert ((got >= 0) & (got <= 1)).all() and float(np.abs(got - ref).max()) <= TOL
    gu.close(got, gh.box_iou3d_host(A, B), TOL)


def test_a_nan_box_poisons_exactly_its_row_or_column():
    A, B = gu.random_boxes(5, 3).astype(np.float32), gu.random_boxes(4, 4).astype(np.float32)
    A[1, 7], B[2, 4], A[3, 3], B[0, 0] = np.nan, 0.0, -0.5, np.inf
    got = gl.box_iou3d(dev(A), dev(B)).cpu().numpy()
    bad = np.zeros((5, 4), bool)
    bad[1], bad[3], bad[:, 2], bad[:, 0] = True, True, True, True
    assert np.array_equal(np.isnan(got), bad)
    gu.close(got[~bad], gh.box_iou3d_host(A, B)[~bad], TOL)


# ------------------------------------------------------------------------------------------------------------------ costs and matching
@pytest.mark.parametrize("shape", ["small", "wave"])
def test_cost_matrices(shape):
    c = case(shape)
    s, b, m, gts, pms = device_args(c)
    full = np.zeros((s.shape[1], s.shape[3]), bool)
    full[:, :c["mask"].shape[1]] = c["mask"]
    assert torch.isneginf(s.permute(1, 3, 0, 2)[dev(~full)]).all()          # -inf on every masked column, as contrastive_scores leaves them
    cost, G = gl.match_costs(s, b, m, gts, pms)
    assert G == [len(g) for g in c["gts"]] and tuple(cost.shape) == (s.shape[0], s.shape[2], sum(G))
    got = cost.cpu().numpy()
    assert np.isfinite(got).all()
    ref = np.concatenate([np.concatenate(row, 1)[None] for row in c["costs"]])
    err = gu.close(got, ref, TOL)
    print(f"{shape}: max |cost - specification| = {err:.2e} of scale {gu.scale(ref):.2f}")
    assert bits_equal(cost, gl.match_costs(s, b, m, gts, pms)[0])


@pytest.mark.parametrize("shape", ["small", "wave"])
def test_assignment(shape):
    c = case(shape)
    NL, B, K, _ = c["scores"].shape
    G = [len(g) for g in c["gts"]]
    for l in range(NL):                                      # the input is far from a tie: forbidding a matched pair costs at least 1e-2
        for b in range(B):
            cm = c["costs"][l][b]
            if not cm.size:
                continue
            rows, cols = linear_sum_assignment(cm)
            base = cm[rows, cols].sum()
            for r, g in zip(rows, cols):
                other = cm.copy()
                other[r, g] = 1e6
                r2, c2 = linear_sum_assignment(other)
                assert other[r2, c2].sum() - base >= 1e-2, (l, b, r, g)
    s, bx, m, gts, pms = device_args(c)
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=s.shape[-1]))
    got = mod.assign(s, bx, m, gts, pms)
    assert got.dtype == torch.int32 and tuple(got.shape) == (NL, B, K) and got.is_cuda
    cost = np.nan_to_num(gl.match_costs(s, bx, m, gts, pms)[0].cpu().numpy(), nan=100.0, posinf=100.0, neginf=-100.0)
    own, lo = np.full((NL, B, K), -1, np.int32), 0
    for b in range(B):
        for l in range(NL):
            if G[b]:
                rows, cols = linear_sum_assignment(cost[l][:, lo:lo + G[b]])
                own[l, b, rows] = cols
        lo += G[b]
    assert np.array_equal(got.cpu().numpy(), own)            # scipy on the device's own matrices, exactly
    assert np.array_equal(own, c["assign"])                  # and the specification's matching
    for b in range(B):
        assert ((own[:, b] >= 0).sum(-1) == min(K, G[b])).all()


# ------------------------------------------------------------------------------------------------------------------ the loss
@pytest.mark.parametrize("shape", ["small", "wave", "full"])
def test_loss_and_gradients(shape):
    c = case(shape)
    NL, B, K, M = c["scores"].shape
    s, bx, m, gts, pms = device_args(c)
    s.requires_grad_()
    bx.requires_grad_()
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=M))
    out = mod.loss(s, bx, m, gts, pms)
    ref = gh.loss_dict(c["loss"]["loss_cls"], c["loss"]["loss_bbox"])
    assert list(out) == list(ref) and len(out) == 2 * NL
    for k in ref:
        assert out[k].dim() == 0 and abs(float(out[k].detach()) - ref[k]) <= TOL * abs(ref[k]), (k, float(out[k].detach()), ref[k])
    up = gh.loss_dict(c["up"][0], c["up"][1])                # non-unit upstream gradients per dict entry
    keys = list(out)
    ds, db = torch.autograd.grad([out[k] for k in keys], [s, bx], [torch.tensor(up[k], dtype=torch.float32, device=DEV) for k in keys],
                                 retain_graph=True)
    e1, e2 = gu.close(ds.cpu().numpy(), c["loss"]["dscores"], TOL), gu.close(db.cpu().numpy(), c["loss"]["dboxes"], TOL)
    print(f"{shape}: max error dscores {e1:.2e} of {gu.scale(c['loss']['dscores']):.2e}, dboxes {e2:.2e} of {gu.scale(c['loss']['dboxes']):.2e}")
    full = np.zeros((B, M), bool)
    full[:, :c["mask"].shape[1]] = c["mask"]
    dsn, dbn = ds.cpu().numpy(), db.cpu().numpy()
    assert not dsn[np.broadcast_to(~full[None, :, None, :], dsn.shape)].any()          # exactly 0 on masked tokens and from T on
    assert not dbn[c["assign"] < 0].any() and dbn[c["assign"] >= 0].any()              # exactly 0 for an unmatched query
    ds2, db2 = torch.autograd.grad([out[k] for k in keys], [s, bx], [torch.tensor(up[k], dtype=torch.float32, device=DEV) for k in keys])
    assert bits_equal(ds, ds2) and bits_equal(db, db2)
    again = mod.loss(s, bx, m, gts, pms)
    assert all(bits_equal(out[k].detach(), again[k].detach()) for k in keys)


def test_a_prediction_on_its_target_adds_nothing_to_the_box_loss():
    c = case("full")
    boxes = c["boxes"].copy()
    q = int(np.nonzero(c["assign"][0, 0] >= 0)[0][0])
    boxes[0, 0, q] = c["gts"][0][c["assign"][0, 0, q]]
    s, _, m, gts, pms = device_args(c)
    bx = dev(boxes).requires_grad_()
    losses = gl.grounding_loss(s, bx, m, gts, pms, dev(c["assign"]))
    assert tuple(losses.shape) == (2, 1) and float(losses[1, 0].detach()) == 0.0
    losses[1, 0].backward()
    assert torch.isfinite(bx.grad).all() and not bx.grad.any()


def test_predict_is_the_largest_sigmoid_and_zero_where_every_token_is_masked():
    c = case("small")
    scores = c["scores"].copy()
    scores[-1, 1, 2, :] = -np.inf                            # a query whose every token is masked
    s, bx, _, _, _ = device_args(dict(c, scores=scores))
    boxes, got = GroundingLoss(contrastive_cfg=dict(max_text_len=16)).predict(s, bx)
    ref_boxes, ref = gh.predict_host(scores, c["boxes"])
    assert tuple(got.shape) == ref.shape and torch.equal(boxes, bx[-1]) and np.array_equal(boxes.cpu().numpy().astype(np.float64), ref_boxes)
    gu.close(got.cpu().numpy(), ref, TOL)
    assert float(got[1, 2]) == 0.0 and (got.cpu().numpy() > 0).sum() == got.numel() - 1


def test_a_batch_without_ground_truth_raises_before_any_launch():
    c = case("small")
    s, bx, m, _, _ = device_args(c)
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=16))
    none = [torch.zeros((0, 9), device=DEV) for _ in range(3)], [torch.zeros((0, 16), device=DEV) for _ in range(3)]
    with pytest.raises(ValueError, match="no matched pair"):
        mod.loss(s, bx, m, *none)
    assert (mod.assign(s, bx, m, *none) == -1).all()


def test_decoder_outputs_go_through_the_loss_without_a_copy():
    """``decoder_util``'s small module -> ``head_scores`` -> ``GroundingLoss.loss`` -> backward into the decoder's outputs."""
    cfg = du.SMALL
    C, NL, rows, K, T = cfg["C"], cfg["layers"], (40, 9, 70), 6, 7
    tmask = np.zeros((3, T), bool)
    tmask[1, [0, T - 1]] = True                              # True = ignore
    ops = du.operands(rows, K, T, C, seed=31, text_mask=tmask)
    dec = du.module(**cfg).to(DEV)
    qs = qu.module(C=C, num_queries=K).to(DEV)
    with torch.no_grad():
        hidden, boxes = du.device(dec, ops, du.reg_branches(C, NL).to(DEV))
        token_mask = dev(~tmask)
        scores = dec.head_scores(hidden, dict(text_feats=dev(ops["text_feats"]), text_token_mask=token_mask), qs)
    assert tuple(scores.shape) == (NL, 3, K, 256) and tuple(boxes.shape) == (NL, 3, K, 9) and scores.is_contiguous() and boxes.is_contiguous()
    rng = np.random.default_rng(32)
    G = (2, 0, 1)
    gts = []
    for b, g in enumerate(G):
        gt = boxes[-1, b, :g].cpu().numpy() + rng.normal(0, 0.05, (g, 9))
        gt[:, 3:6] = np.abs(gt[:, 3:6]) + 0.05
        gts.append(dev(gt))
    pms = []
    for b, g in enumerate(G):
        pm = np.zeros((g, 256), np.float32)
        pm[:, np.nonzero(~tmask[b])[0][:2]] = 0.5
        pms.append(dev(pm))
    scores.requires_grad_()
    boxes.requires_grad_()
    mod = GroundingLoss()
    out = mod.loss(scores, boxes, token_mask, gts, pms)
    sn, bn = scores.detach().cpu().numpy().astype(np.float64), boxes.detach().cpu().numpy().astype(np.float64)
    g64, p64 = [g.cpu().numpy().astype(np.float64) for g in gts], [p.cpu().numpy().astype(np.float64) for p in pms]
    assign = gh.assign_host(gh.cost_host(sn, bn, ~tmask, g64, p64), K)
    assert np.array_equal(mod.assign(scores, boxes, token_mask, gts, pms).cpu().numpy(), assign)
    ref = gh.loss_host(sn, bn, ~tmask, g64, p64, assign)
    refd = gh.loss_dict(ref["loss_cls"], ref["loss_bbox"])
    for k in refd:
        assert abs(float(out[k].detach()) - refd[k]) <= TOL * abs(refd[k]), k
    sum(out.values()).backward()
    gu.close(scores.grad.cpu().numpy(), ref["dscores"], TOL)
    gu.close(boxes.grad.cpu().numpy(), ref["dboxes"], TOL)
