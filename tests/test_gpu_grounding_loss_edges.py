"""The grounding loss's kernels (csrc/grounding_loss.hip, proxytransformation_amd/grounding_loss.py) at the edges
tests/test_gpu_grounding_loss.py does not reach, each at the smallest shape that takes the path.  Every reference is
``grounding_loss_host.py`` in float64 on operands rounded to fp32 once; the matching is handed in as an explicit ``assign`` wherever it is
not the subject.  Bounds: ``PARITY`` (1e-4 of the tensor's scale); for pairs of boxes nearer than the coplanarity
tolerance ``grounding_loss_util.coplanar_bound`` (``PARITY`` + what the rule admits on the pair's own sizes); bit equality where the
arithmetic is exact or two calls must agree.  The inputs' preconditions (overlap shares, the specification's ulp sensitivity, the floors of
the near-duplicates) are held without a GPU in tests/test_grounding_loss_host.py.  Every figure is printed behind ``gl-edges`` before it
is asserted (profiles/grounding_loss_edges.txt).

iou        seven regimes of 24 x 24 pairs (plain, thin, far, angles, small, large, inside) against the specification and in both
           argument orders; near-duplicates ``A + delta N(0, 1)`` for delta 1e-1 .. 1e-6, cubes and thin boxes; one box by two names
           (itself, ``a0 + 2 pi``, cubes turned by pi/2 about z and about their own y); grids (17, 1), (1, 17), (16, 16).
cost       T in 1, 15, 16, 17, 33 with M in T, 48, 256 at 70 pairs (no multiple of 16), one scene without a token whose cost is exactly
           ``w_l1 l1 - w_iou iou``; G layouts (0, 2, 3), (3, 2, 0), (1,), G > K with the matching; NaN under masked tokens and from T on
           leaves no trace; scores at +-U(17, 60) and +-U(88, 100) with fractional targets; six (alpha, gamma) x two weight triples;
           NaN, zero and negative sizes in prediction boxes.
loss       B K in 260, 900, 1024 rows per layer (the reduction's later strides); another pair count per layer; out-of-range ``assign``
           entries; a layer without a pair; 128 predictions on their targets (plain, far, wide angles): exactly 0; one decoupled group
           moved: the other terms exactly 0; dyadic ties bit for bit; (alpha, gamma), ``decouple_weights``, ``loss_weights`` and the cost
           parameters through the module; saturated scores; the T and M edges with their exact zeros.
doors      backward from one dict entry, ``sum(out.values())`` at NL = 1, one leaf without grad; scores as a slice of a wider buffer,
           boxes as a strided view, float64 and fp16 leaves, a uint8 mask; a side stream.
predict    rows in 15, 16, 17, 1000 with M in 1, 17, 256: a NaN, a ``+inf`` and a row of ``-inf``."""
import functools
import math

import numpy as np
import pytest
import torch

from proxytransformation_amd import GroundingLoss, grounding_loss as gl, grounding_loss_host as gh
from tests import grounding_loss_util as gu
from tests import sparse_util as su
from tests.test_gpu_grounding_loss import bits_equal, dev

pytestmark = pytest.mark.gpu
DEV = su.DEV
TOL = gu.PARITY


def host(t):
    return t.detach().cpu().numpy()


def say(text):
    print(f"gl-edges {text}")


# ------------------------------------------------------------------------------------------------------------------ 1. box_iou3d
@functools.lru_cache(maxsize=None)
def regime(name):
    A, B = gu.iou_regime(name)
    return A, B, gh.box_iou3d_host(A, B)


def diag_spec(A, B):
    return np.array([gh.box_iou3d_host(a[None], b[None])[0, 0] for a, b in zip(A, B)])


def diag_device(A, B):
    return np.diag(host(gl.box_iou3d(dev(A), dev(B)))).astype(np.float64)


@pytest.mark.parametrize("name", gu.IOU_REGIMES)
def test_iou_regimes(name):
    A, B, ref = regime(name)
    got = gl.box_iou3d(dev(A), dev(B))
    pairs = [(i, j % gu.IOU_N) for i in range(gu.IOU_N) for j in (i, i + 1, i + 7)]
    moved = gu.ulp_sensitivity(gh.box_iou3d_host, A, B, pairs)
    err = float(np.abs(host(got) - ref).max())
    say(f"iou {name}: max |IoU - specification| = {err:.2e} over 576 pairs ({float((ref > 1e-3).mean()):.0%} overlap); the specification's "
        f"ulp sensitivity {moved:.2e}; bound {TOL * gu.scale(ref):.2e}")
    assert ((host(got) >= 0) & (host(got) <= 1)).all()
    gu.close(host(got), ref, TOL)
    assert bits_equal(got, gl.box_iou3d(dev(A), dev(B)))


@pytest.mark.parametrize("name", gu.IOU_REGIMES)
def test_iou_is_symmetric_within_the_bound(name):
    A, B, ref = regime(name)
    fwd, bwd = host(gl.box_iou3d(dev(A), dev(B))), host(gl.box_iou3d(dev(B), dev(A))).T
    gap = float(np.abs(fwd.astype(np.float64) - bwd).max())
    say(f"iou {name}: max |IoU(A, B) - IoU(B, A)| = {gap:.2e}; bound {TOL * gu.scale(ref):.2e}")
    assert gap <= TOL * gu.scale(ref)
    gu.close(bwd, ref, TOL)


@pytest.mark.parametrize("kind", ["cubes", "thin"])
def test_iou_of_near_duplicates(kind):
    """Converged predictions: faces move through the coplanarity tolerance as ``delta`` falls, and an fp32 and an fp64 decision can
    fall on different sides of it -- by no more than the rule admits on the pair."""
    for delta in gu.DELTAS:
        A, B = gu.near_duplicates(kind, delta)
        bound = gu.coplanar_bound(A, B)
        worst = 0.0
        for x, y in ((A, B), (B, A)):
            got, ref = diag_device(x, y), diag_spec(x, y)
            assert ((got >= 0) & (got <= 1)).all()
            worst = max(worst, float(np.abs(got - ref).max()))
            assert (np.abs(got - ref) <= bound).all(), (kind, delta, float((np.abs(got - ref) / bound).max()))
        gap = np.abs(diag_device(A, B) - diag_device(B, A))
        say(f"iou near-duplicate {kind} delta {delta:g}: max |IoU - specification| = {worst:.2e} (both orders), order gap {float(gap.max()):.2e}; "
            f"bound per pair {float(bound.min()):.2e} .. {float(bound.max()):.2e}; smallest IoU {float(diag_spec(A, B).min()):.4f}")
        assert (gap <= bound).all()


def test_iou_of_one_box_by_two_names_is_one():
    for name, A, B in gu.same_box_names():
        bound = gu.coplanar_bound(A, B)
        worst = 0.0
        for x, y in ((A, B), (B, A)):
            got = diag_device(x, y)
            worst = max(worst, float(np.abs(got - 1.0).max()))
            assert (got <= 1.0).all() and (np.abs(got - 1.0) <= bound).all(), (name, float((np.abs(got - 1.0) / bound).max()))
            assert (np.abs(got - diag_spec(x, y)) <= bound).all()
        say(f"iou same box, {name}: max |IoU - 1| = {worst:.2e} (64 boxes, both orders); bound per pair {float(bound.min()):.2e} .. {float(bound.max()):.2e}")


@pytest.mark.parametrize("N,M", [(17, 1), (1, 17), (16, 16)])
def test_iou_grids_one_group_past_a_work_group_and_exactly_full(N, M):
    A, B, ref = regime("plain")
    got = gl.box_iou3d(dev(A[:N]), dev(B[:M]))
    assert tuple(got.shape) == (N, M)
    err = gu.close(host(got), ref[:N, :M], TOL)
    say(f"iou grid ({N}, {M}): max error {err:.2e}")
    assert bits_equal(got, gl.box_iou3d(dev(A), dev(B))[:N, :M].contiguous())       # a pair does not depend on its place in the grid


# ------------------------------------------------------------------------------------------------------------------ 2. costs and matching
def ops(c, **over):
    c = dict(c, **over)
    return dev(c["scores"]), dev(c["boxes"]), dev(c["mask"]), [dev(g) for g in c["gts"]], [dev(p) for p in c["pms"]]


@functools.lru_cache(maxsize=None)
def hungarian_case(NL=2, B=3, K=5, M=16, T=7, tokens=(7, 3, 1), G=(3, 0, 7), seed=51, soft=False):
    """``grounding_loss_util.batch`` (a matching far from a tie) rounded to fp32 once, and the specification's IoU of it."""
    scores, boxes, mask, gts, pms = gu.batch(NL=NL, B=B, K=K, M=M, T=T, tokens=tokens, G=G, seed=seed)
    if soft:
        pms = gu.soft_maps(mask, G, M, np.random.default_rng(seed + 1))
    c = dict(scores=gu.f32(scores), boxes=gu.f32(boxes), mask=mask, gts=[gu.f32(g) for g in gts], pms=[gu.f32(p) for p in pms])
    c["iou"] = np.concatenate([np.concatenate([gh.box_iou3d_host(c["boxes"][l, b], c["gts"][b]) for b in range(B)], 1)[None] for l in range(NL)])
    return c


def spec_costs(c, **kw):
    return gh.cost_host(c["scores"], c["boxes"], c["mask"], c["gts"], c["pms"], iou=c.get("iou"), **kw)


def flat(costs):
    return np.concatenate([np.concatenate(row, 1)[None] for row in costs])


@pytest.mark.parametrize("T,M", gu.TOKEN_EDGES)
def test_costs_at_the_token_edges_and_in_a_scene_without_a_token(T, M):
    c = hungarian_case(T=T, M=M, tokens=(T, 0, (T + 1) // 2), G=(2, 3, 2), seed=60 + T, soft=True)
    s, b, m, gts, pms = ops(c)
    cost, G = gl.match_costs(s, b, m, gts, pms)
    assert G == [2, 3, 2] and (2 * 5 * 7) % 16 and not c["mask"][1].any()
    ref = flat(spec_costs(c))
    err = gu.close(host(cost), ref, TOL)
    say(f"cost T={T} M={M}: max error {err:.2e} of scale {gu.scale(ref):.2f} ({err / gu.scale(ref):.2e})")
    # the scene without a token: exactly w_l1 l1 - w_iou iou of the device's own l1 and iou, in fp32
    w = (np.float32(0.5), np.float32(3.0), np.float32(0.7))
    l1 = host(gl.match_costs(s, b, m, gts, pms, weights=(0.0, 1.0, 0.0))[0])[:, :, 2:5]
    iou = -host(gl.match_costs(s, b, m, gts, pms, weights=(0.0, 0.0, 1.0))[0])[:, :, 2:5]
    got = host(gl.match_costs(s, b, m, gts, pms, weights=tuple(float(v) for v in w))[0])[:, :, 2:5]
    assert (l1 > 0).all() and (iou >= 0).all() and np.array_equal(got, w[1] * l1 - w[2] * iou) and got.dtype == np.float32
    gu.close(iou, c["iou"][:, :, 2:5], TOL)


LAYOUTS = {"(0,2,3)": dict(G=(0, 2, 3)), "(3,2,0)": dict(G=(3, 2, 0)), "B=1 G=1": dict(B=1, tokens=(4,), G=(1,)), "G>K": dict(B=1, tokens=(7,), G=(7,))}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_cost_and_matching_on_ground_truth_layouts(layout):
    c = hungarian_case(seed=70, **LAYOUTS[layout])
    s, b, m, gts, pms = ops(c)
    K, G = 5, [len(g) for g in c["gts"]]
    cost, got_G = gl.match_costs(s, b, m, gts, pms)
    ref = spec_costs(c)
    assert got_G == G and tuple(cost.shape) == (2, K, sum(G))
    err = gu.close(host(cost), flat(ref), TOL)
    say(f"cost G={layout}: max error {err:.2e} of scale {gu.scale(flat(ref)):.2f}")
    assign = host(GroundingLoss(contrastive_cfg=dict(max_text_len=16)).assign(s, b, m, gts, pms))
    assert np.array_equal(assign, gh.assign_host(ref, K))
    for i, g in enumerate(G):
        assert ((assign[:, i] >= 0).sum(-1) == min(K, g)).all()


def test_what_is_masked_is_never_read():
    """NaN scores under masked tokens and from T on, NaN and nonzero positive-map entries there: the same bits as the clean batch, in
    the costs, the matching, the loss and both gradients."""
    c = hungarian_case()
    T = c["mask"].shape[1]
    dead = np.ones((3, 16), bool)
    dead[:, :T] = ~c["mask"]
    scores = np.where(dead[None, :, None, :], np.nan, c["scores"])
    rng = np.random.default_rng(3)
    pms = [np.where(dead[i][None], np.where(rng.integers(0, 2, p.shape) > 0, np.nan, 0.75), p) for i, p in enumerate(c["pms"])]
    assert np.isnan(scores).sum() == dead.sum() * 10 and all(np.isnan(p).any() and (p == 0.75).any() for p in pms if len(p))
    assign = dev(gh.assign_host(spec_costs(c), 5))
    out = []
    for case in (c, dict(c, scores=scores, pms=pms)):
        s, b, m, gts, pm = ops(case)
        s.requires_grad_()
        b.requires_grad_()
        cost = gl.match_costs(s, b, m, gts, pm)[0]
        losses = gl.grounding_loss(s, b, m, gts, pm, assign)
        losses.sum().backward()
        out.append((cost, GroundingLoss(contrastive_cfg=dict(max_text_len=16)).assign(s, b, m, gts, pm), losses.detach(), s.grad, b.grad))
    assert torch.equal(out[0][1], assign) and torch.equal(out[1][1], assign)
    for clean, dirty in zip(out[0], out[1]):
        assert torch.isfinite(clean.float()).all() and (torch.equal(clean, dirty) if clean.dtype == torch.int32 else bits_equal(clean, dirty))


@pytest.mark.parametrize("lo,hi", [(17.0, 60.0), (88.0, 100.0)])
def test_costs_at_saturated_scores(lo, hi):
    """``1 - p`` as ``sigmoid(-x)``: beyond x = 17 the cost follows float64, and ``expf`` overflowing to inf beyond 88.7 leaves it finite."""
    c = hungarian_case(soft=True)
    c = dict(c, scores=gu.saturate(c["scores"], c["mask"], lo, hi, 5))
    got = host(gl.match_costs(*ops(c))[0])
    ref = flat(spec_costs(c))
    assert np.isfinite(got).all()
    err = gu.close(got, ref, TOL)
    say(f"cost at scores +-U({lo:g}, {hi:g}): max error {err:.2e} of scale {gu.scale(ref):.2f} ({err / gu.scale(ref):.2e})")


def test_the_cost_at_x_30_follows_x_and_does_not_stick():
    one = dict(scores=np.full((1, 1, 1, 1), 30.0), boxes=gu.f32(gu.random_boxes(1, 1))[None, None], mask=np.ones((1, 1), bool),
               gts=[gu.f32(gu.random_boxes(1, 2))], pms=[np.zeros((1, 1))])
    got = float(gl.match_costs(*ops(one), weights=(1.0, 0.0, 0.0))[0])
    ref = float(gh.cost_host(one["scores"], one["boxes"], one["mask"], one["gts"], one["pms"], weights=(1.0, 0.0, 0.0))[0][0][0, 0])
    stuck = -math.log(1e-12) * 0.75
    say(f"cost at x = 30, target 0: device {got:.6f}, specification {ref:.6f}, the stuck value {stuck:.6f}")
    assert abs(ref - stuck) > 0.05 and abs(got - ref) <= TOL * ref


@pytest.mark.parametrize("weights", gu.COST_WEIGHTS)
@pytest.mark.parametrize("alpha,gamma", gu.FOCAL_PARAMS)
def test_costs_under_other_focal_parameters_and_weights(alpha, gamma, weights):
    c = hungarian_case(soft=True)
    got = host(gl.match_costs(*ops(c), alpha=alpha, gamma=gamma, weights=weights)[0])
    ref = flat(spec_costs(c, alpha=alpha, gamma=gamma, weights=weights))
    err = gu.close(got, ref, TOL)
    say(f"cost alpha={alpha:g} gamma={gamma:g} weights={weights}: max error {err:.2e} of scale {gu.scale(ref):.2f} ({err / gu.scale(ref):.2e})")


def test_bad_prediction_boxes_poison_their_rows_and_the_matching_still_comes_back():
    c = hungarian_case(G=(5, 2, 0), seed=80)
    clean = gh.assign_host(spec_costs(c), 5)
    boxes = c["boxes"].copy()
    m0, m1 = int(np.nonzero(clean[0, 0] == 2)[0][0]), int(np.nonzero(clean[1, 1] == 1)[0][0])      # matched queries, G = K and G < K
    u1 = int(np.nonzero(clean[0, 1] < 0)[0][0])                                                     # an unmatched one
    boxes[0, 0, m0, 7], boxes[1, 0, m0, 4], boxes[1, 1, m1, 3], boxes[0, 1, u1, 0] = np.nan, 0.0, -0.4, np.nan
    bad = np.zeros((2, 5, 7), bool)
    bad[0, m0, :5], bad[1, m0, :5], bad[1, m1, 5:], bad[0, u1, 5:] = True, True, True, True
    c = dict(c, boxes=boxes, iou=None)
    s, b, m, gts, pms = ops(c)
    got = host(gl.match_costs(s, b, m, gts, pms)[0])
    ref = gh.cost_host(c["scores"], boxes, c["mask"], c["gts"], c["pms"])
    assert np.array_equal(np.isnan(got), bad) and np.array_equal(np.isnan(flat(ref)), bad)
    gu.close(got[~bad], flat(ref)[~bad], TOL)
    assign = host(GroundingLoss(contrastive_cfg=dict(max_text_len=16)).assign(s, b, m, gts, pms))
    assert np.array_equal(assign, gh.assign_host(ref, 5))
    assert ((assign[:, 0] >= 0).sum(-1) == 5).all() and ((assign[:, 1] >= 0).sum(-1) == 2).all() and (assign[:, 2] == -1).all()
    assert assign[0, 0, m0] >= 0 and assign[1, 1, m1] == -1   # G = K: the NaN row takes what is left; G < K: it loses its box


# ------------------------------------------------------------------------------------------------------------------ 3. the loss
def run_loss(c, up=None, assign=None, **kw):
    """``(losses (2,NL), dscores, dboxes)`` of ``grounding_loss`` on the batch's explicit matching, as numpy; the upstream gradient
    ``up (2,NL)`` defaults to ones."""
    s, b, m, gts, pms = ops(c)
    s.requires_grad_()
    b.requires_grad_()
    losses = gl.grounding_loss(s, b, m, gts, pms, dev(c["assign"] if assign is None else assign), **kw)
    g = torch.ones_like(losses) if up is None else dev(up)
    ds, db = torch.autograd.grad(losses, [s, b], g)
    return losses.detach(), ds, db


def spec_loss(c, up=None, **kw):
    up = np.ones((2, c["scores"].shape[0])) if up is None else up
    return gh.loss_host(c["scores"], c["boxes"], c["mask"], c["gts"], c["pms"], c["assign"], upstream_cls=up[0], upstream_bbox=up[1], **kw)


def hold_loss(name, c, got, ref):
    """Losses within ``PARITY`` of each value, gradients within ``PARITY`` of their tensor's scale, the exact zeros where they belong."""
    losses, ds, db = (host(t) for t in got)
    NL, B, K, M = c["scores"].shape
    e_l = 0.0
    for row, key in ((0, "loss_cls"), (1, "loss_bbox")):
        assert np.isfinite(losses[row]).all()
        rel = np.abs(losses[row] - ref[key]) / np.maximum(np.abs(ref[key]), 1e-30)
        e_l = max(e_l, float(rel.max()))
        assert (np.abs(losses[row] - ref[key]) <= TOL * np.abs(ref[key])).all(), (name, key, losses[row], ref[key])
    e_s, e_b = gu.close(ds, ref["dscores"], TOL), gu.close(db, ref["dboxes"], TOL)
    say(f"loss {name}: losses {e_l:.2e} of their values, dscores {e_s / gu.scale(ref['dscores']):.2e}, dboxes {e_b / gu.scale(ref['dboxes']):.2e} "
        f"of their scales")
    full = np.zeros((B, M), bool)
    full[:, :c["mask"].shape[1]] = c["mask"]
    assert not ds[np.broadcast_to(~full[None, :, None, :], ds.shape)].any()             # exactly 0 on masked tokens and from T on
    assert not db[c["assign"] < 0].any() and db[c["assign"] >= 0].any()                  # exactly 0 for an unmatched query
    return e_l, e_s, e_b


def same_bits(a, b):
    assert all(bits_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B,K", [(2, 130), (3, 300), (1, 1024)])
def test_layers_of_more_than_256_rows(B, K):
    """``k_gl_loss_sum``'s thread t adds the rows t, t + 256, ..: 260, 900 and 1024 rows per layer take its second to fourth trip, with
    matched rows in every stride."""
    c = gu.explicit_batch(NL=2, B=B, K=K, M=16, T=7, tokens=(7, 3, 1)[:B], G=(48,) * B, seed=100 + K)
    rows = np.nonzero(c["assign"].reshape(2, -1) >= 0)[1]
    assert (rows >= 256).any() and (rows < 256).any() and B * K > 256
    up = np.random.default_rng(K).uniform(0.5, 2.0, (2, 2))
    got = run_loss(c, up=up, avg_factor=48.0 * B)
    hold_loss(f"B={B} K={K}", c, got, spec_loss(c, up=up, avg_factor=48.0 * B))
    same_bits(got, run_loss(c, up=up, avg_factor=48.0 * B))


def test_every_layer_divides_by_its_own_pair_count():
    """1 pair in layer 0 and 4 in layer 1, 7 by the host's ``num_pos`` and 3 as ``avg_factor``: the box loss and ``dboxes`` follow the
    device's count of each layer."""
    c = gu.explicit_batch(NL=2, B=2, K=6, M=16, T=7, tokens=(7, 3), G=(4, 3), seed=42, pairs=((1, 0), (2, 2)))
    assert ((c["assign"] >= 0).sum((1, 2)) == (1, 4)).all()
    up = np.array([[1.5, 0.5], [0.75, 2.0]])
    got = run_loss(c, up=up, avg_factor=3.0)
    ref = spec_loss(c, up=up, avg_factor=3.0)
    hold_loss("pair counts (1, 4)", c, got, ref)
    for l in range(2):                                       # (no other count passes: the nearest, 7 / 4, is off by 75 %)
        assert abs(float(got[0][1, l]) / ref["loss_bbox"][l] - 1) <= TOL and host(got[2])[l].any()


def test_out_of_range_assign_entries_are_unmatched():
    c = gu.explicit_batch(NL=2, B=3, K=5, M=16, T=7, tokens=(7, 3, 1), G=(3, 0, 7), seed=43, pairs=((2, 0, 3), (3, 0, 2)))
    junk = c["assign"].copy()
    free = np.argwhere(junk < 0)
    for (l, b, q), v in zip(free[np.random.default_rng(1).permutation(len(free))[:8]], (3, 4, 7, 8, -2, -100, 2 ** 30, -2 ** 31)):
        junk[l, b, q] = v if v < 0 or v >= (3, 0, 7)[b] else (3, 0, 7)[b]
    assert (junk != c["assign"]).sum() == 8 and ((junk >= np.array((3, 0, 7))[None, :, None]) | (junk < -1)).sum() == 8
    got = run_loss(c, avg_factor=5.0)
    same_bits(got, run_loss(c, assign=junk, avg_factor=5.0))
    hold_loss("out-of-range entries", c, got, spec_loss(c, avg_factor=5.0))


def test_a_layer_without_a_pair_is_nan_in_its_box_loss_alone():
    """The mean of nothing, as the reference returns it; its ``dboxes`` are exactly 0 and the other layers do not notice."""
    c = gu.explicit_batch(NL=3, B=2, K=6, M=16, T=7, tokens=(7, 3), G=(4, 3), seed=44, pairs=((2, 1), (0, 0), (1, 3)))
    losses, ds, db = run_loss(c, avg_factor=4.0)
    assert torch.isnan(losses[1, 1]) and torch.isfinite(losses[0]).all() and torch.isfinite(losses[1, [0, 2]]).all()
    assert torch.isfinite(ds).all() and torch.isfinite(db).all() and not db[1].any() and ds[1].any()
    keep = [0, 2]
    rest = dict(c, scores=c["scores"][keep], boxes=c["boxes"][keep], assign=c["assign"][keep])
    hold_loss("a layer without a pair, the others", rest, (losses[:, keep], ds[keep], db[keep]), spec_loss(rest, avg_factor=4.0))
    same_bits((losses[:, keep].contiguous(), ds[keep], db[keep]), run_loss(rest, avg_factor=4.0))
    # the classification side of the empty layer: every target 0, written out
    x = c["scores"][1][:, :, :7]
    p = 1 / (1 + np.exp(-x))
    zero_target = (np.where(c["mask"][:, None, :], (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))) * 0.75 * p ** 2, 0.0)).sum() / (4.0 + gh.F32_EPS)
    assert abs(float(losses[0, 1]) - zero_target) <= TOL * zero_target


@pytest.mark.parametrize("variant", ["plain", "far", "angles"])
def test_128_predictions_on_their_targets_add_exactly_nothing(variant):
    """Both sides of a Chamfer term round one corner expression alike: distance 0.0, not 1e-8, over random sizes and attitudes, 40 m
    from the origin and at angles of many turns."""
    gt = gu.random_boxes(128, 90)
    if variant == "far":
        gt[:, :3] += (40.0, -25.0, 3.0)
    if variant == "angles":
        gt[:, 6:] = np.random.default_rng(91).uniform(-20 * math.pi, 20 * math.pi, (128, 3))
    c = gu.explicit_batch(NL=1, B=1, K=128, M=16, T=7, tokens=(5,), G=(128,), seed=92)
    c["gts"] = [gu.f32(gt)]
    c["assign"] = np.arange(128, dtype=np.int32)[None, None]
    c["boxes"] = c["gts"][0][None, None].copy()
    losses, ds, db = run_loss(c)
    say(f"loss on target, {variant}: loss_bbox {float(losses[1, 0])!r}, max |dboxes| {float(db.abs().max())!r}")
    assert float(losses[1, 0]) == 0.0 and torch.isfinite(db).all() and not db.any()
    assert torch.isfinite(losses[0]).all() and float(losses[0, 0]) > 0 and ds.any()


@pytest.mark.parametrize("moved", [0, 1, 2])
def test_a_moved_group_leaves_the_other_decoupled_terms_at_zero(moved):
    c = gu.explicit_batch(NL=1, B=1, K=16, M=16, T=7, tokens=(5,), G=(16,), seed=93)
    c["assign"] = np.arange(16, dtype=np.int32)[None, None]
    boxes = c["gts"][0][None, None].copy()
    off = np.random.default_rng(94).normal(0.0, 0.1, (16, 3))
    boxes[0, 0, :, 3 * moved:3 * moved + 3] += np.abs(off) if moved == 1 else off
    c["boxes"] = gu.f32(boxes)
    for k in range(3):
        dw = tuple(1.0 if i == k else 0.0 for i in range(4))
        got = run_loss(c, decouple_weights=dw)
        if k == moved:
            hold_loss(f"group {moved} moved, its own term", c, got, spec_loss(c, decouple_weights=dw))
            other = np.ones(9, bool)
            other[3 * k:3 * k + 3] = False
            assert float(got[0][1, 0]) > 0 and not host(got[2])[..., other].any()
        else:
            assert float(got[0][1, 0]) == 0.0 and torch.isfinite(got[2]).all() and not got[2].any(), (moved, k)


@pytest.mark.parametrize("dw,lw", [((0.25, 0.25, 0.25, 0.25), (1.0, 1.0)), ((0.0, 0.0, 0.0, 1.0), (1.0, 1.0)), ((0.5, 0.125, 0.125, 0.25), (2.0, 0.5))])
def test_ties_go_to_the_lower_corner_and_a_zero_coordinate_has_no_slope(dw, lw):
    """Dyadic boxes (``grounding_loss_util.dyadic_ties``): every intermediate is exact in fp32 and in float64, eight pairs make the
    divisor 64, so value and gradient are the specification's after the fp32 cast, bit for bit (``+ 0.0``: zeros without a sign)."""
    pred, gt = gu.dyadic_ties()
    c = gu.explicit_batch(NL=1, B=1, K=8, M=16, T=7, tokens=(5,), G=(8,), seed=95)
    c.update(boxes=pred[None, None], gts=[gt], assign=np.arange(8, dtype=np.int32)[None, None])
    ref = spec_loss(c, decouple_weights=dw, loss_weights=lw)
    losses, _, db = run_loss(c, decouple_weights=dw, loss_weights=lw)
    want = ref["dboxes"].astype(np.float32) + np.float32(0.0)
    assert np.array_equal(want.astype(np.float64), ref["dboxes"]) and (want == 0).any() and (want != 0).any()
    assert bits_equal(losses[1] + 0.0, dev(ref["loss_bbox"])) and bits_equal(db + 0.0, dev(want))
    # shifted along +x alone: no slope in y and z; and in x the four tied corners take the lower (+x) target corner and cancel the four
    # untied ones -- the higher corner would give 8 / 64 per term
    assert not host(db)[0, 0, 0, :3].any() and host(db)[0, 0, 3, 2] != 0


@pytest.mark.parametrize("alpha,gamma", gu.FOCAL_PARAMS)
def test_loss_under_other_focal_parameters(alpha, gamma):
    c = gu.explicit_batch(NL=2, B=3, K=5, M=16, T=7, tokens=(7, 3, 1), G=(3, 0, 7), seed=96)
    kw = dict(alpha=alpha, gamma=gamma, avg_factor=8.0, loss_weights=(2.0, 0.5), decouple_weights=(0.7, 0.1, 0.1, 0.1))
    up = np.array([[1.5, 0.5], [0.75, 2.0]])
    hold_loss(f"alpha={alpha:g} gamma={gamma:g}", c, run_loss(c, up=up, **kw), spec_loss(c, up=up, **kw))


@pytest.mark.parametrize("alpha,gamma", [(0.25, 2.0), (0.5, 1.0), (0.1, 1.5)])
@pytest.mark.parametrize("lo,hi", [(17.0, 60.0), (88.0, 100.0)])
def test_loss_at_saturated_scores(lo, hi, alpha, gamma):
    """Matched rows with soft targets and unmatched rows with target 0 at |x| up to 100: ``pt`` reaches 0 (``powf(0, 0)`` at gamma 1),
    ``expf`` overflows, and everything stays finite and on the specification."""
    c = gu.explicit_batch(NL=2, B=3, K=5, M=16, T=7, tokens=(7, 3, 1), G=(3, 0, 7), seed=97)
    c["scores"] = gu.saturate(c["scores"], c["mask"], lo, hi, 6)
    got = run_loss(c, alpha=alpha, gamma=gamma, avg_factor=8.0)
    assert all(torch.isfinite(t).all() for t in got)
    hold_loss(f"scores +-U({lo:g}, {hi:g}) alpha={alpha:g} gamma={gamma:g}", c, got, spec_loss(c, alpha=alpha, gamma=gamma, avg_factor=8.0))


@pytest.mark.parametrize("T,M", gu.TOKEN_EDGES)
def test_loss_at_the_token_edges(T, M):
    c = gu.explicit_batch(NL=2, B=3, K=5, M=M, T=T, tokens=(T, 0, (T + 1) // 2), G=(2, 3, 2), seed=110 + T)
    got = run_loss(c, avg_factor=7.0)
    hold_loss(f"T={T} M={M}", c, got, spec_loss(c, avg_factor=7.0))
    assert not got[1][:, 1].any() and tuple(got[1].shape) == (2, 3, 5, M)               # the scene without a token: no score has a slope


MODULES = {
    "decouple_bbox_loss=False": (dict(decouple_bbox_loss=False), dict(decouple_weights=(0.0, 0.0, 0.0, 1.0))),
    "decouple_weights=None": (dict(decouple_weights=None), dict(decouple_weights=(0.25, 0.25, 0.25, 0.25))),
    "decouple_weights=(.7,.1,.1,.1)": (dict(decouple_weights=(0.7, 0.1, 0.1, 0.1)), dict(decouple_weights=(0.7, 0.1, 0.1, 0.1))),
    "loss parameters": (dict(loss_cls=dict(type="mmdet.FocalLoss", use_sigmoid=True, gamma=1.5, alpha=0.1, loss_weight=2.0),
                             loss_bbox=dict(type="BBoxCDLoss", mode="l1", loss_weight=0.5, group="g8")),
                        dict(alpha=0.1, gamma=1.5, loss_weights=(2.0, 0.5))),
    "cost parameters": (dict(train_cfg=dict(assigner=dict(type="HungarianAssigner3D", match_costs=[
        dict(type="BinaryFocalLossCost", weight=0.5, alpha=0.5, gamma=1.0), dict(type="BBox3DL1Cost", weight=3.0), dict(type="IoU3DCost", weight=1.0)]))),
        dict()),
}


@pytest.mark.parametrize("name", list(MODULES))
def test_the_module_hands_its_parameters_on(name):
    kwargs, spec_kw = MODULES[name]
    c = dict(hungarian_case(soft=True))
    cost_kw = dict(alpha=0.5, gamma=1.0, weights=(0.5, 3.0, 1.0)) if name == "cost parameters" else {}
    c["assign"] = gh.assign_host(spec_costs(c, **cost_kw), 5)
    s, b, m, gts, pms = ops(c)
    s.requires_grad_()
    b.requires_grad_()
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=16), **kwargs)
    assert np.array_equal(host(mod.assign(s, b, m, gts, pms)), c["assign"])
    out = mod.loss(s, b, m, gts, pms)
    sum(out.values()).backward()
    losses = torch.stack([torch.stack([out["d0.loss_cls"], out["loss_cls"]]), torch.stack([out["d0.loss_bbox"], out["loss_bbox"]])])
    hold_loss(f"module, {name}", c, (losses, s.grad, b.grad), spec_loss(c, avg_factor=8.0, **spec_kw))


# ------------------------------------------------------------------------------------------------------------------ 4. the doors
def test_backward_from_one_entry_reaches_its_layer_and_branch_alone():
    c = dict(hungarian_case(NL=3, seed=52))
    c["assign"] = gh.assign_host(spec_costs(c), 5)
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=16))
    for key, row, layer in (("loss_cls", 0, 2), ("d0.loss_bbox", 1, 0), ("d1.loss_cls", 0, 1)):
        s, b, m, gts, pms = ops(c)
        s.requires_grad_()
        b.requires_grad_()
        mod.loss(s, b, m, gts, pms)[key].backward()
        up = np.zeros((2, 3))
        up[row, layer] = 1.0
        ref = spec_loss(c, up=up, avg_factor=8.0)
        touched, untouched = (s.grad, b.grad) if row == 0 else (b.grad, s.grad)
        others = [l for l in range(3) if l != layer]
        assert not untouched.any() and not touched[others].any() and touched[layer].any() and torch.isfinite(touched).all()
        gu.close(host(s.grad), ref["dscores"], TOL)
        gu.close(host(b.grad), ref["dboxes"], TOL)


def test_the_summed_dict_at_one_layer_and_leaves_without_grad():
    c = dict(hungarian_case(NL=1, seed=53))
    c["assign"] = gh.assign_host(spec_costs(c), 5)
    ref = spec_loss(c, avg_factor=8.0)
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=16))
    grads = {}
    for wants in ((True, True), (True, False), (False, True)):
        s, b, m, gts, pms = ops(c)
        s.requires_grad_(wants[0])
        b.requires_grad_(wants[1])
        out = mod.loss(s, b, m, gts, pms)
        assert list(out) == ["loss_cls", "loss_bbox"]
        sum(out.values()).backward()
        grads[wants] = (s.grad, b.grad)
    gu.close(host(grads[True, True][0]), ref["dscores"], TOL)
    gu.close(host(grads[True, True][1]), ref["dboxes"], TOL)
    assert grads[True, False][1] is None and grads[False, True][0] is None
    assert bits_equal(grads[True, False][0], grads[True, True][0]) and bits_equal(grads[False, True][1], grads[True, True][1])


def _door_call(s, b, m, gts, pms, assign):
    cost = gl.match_costs(s, b, m, gts, pms)[0]
    losses = gl.grounding_loss(s, b, m, gts, pms, assign)
    ds, db = torch.autograd.grad(losses, [s, b], torch.ones_like(losses))
    return cost, losses.detach(), ds, db


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16])
def test_strided_and_typed_operands_give_the_bits_of_their_fp32_copies(dtype):
    c = dict(hungarian_case())
    c["assign"] = gh.assign_host(spec_costs(c), 5)
    s0, b0, m, gts, pms = ops(c)
    s0, b0 = s0.to(dtype), b0.to(dtype)                      # the values both calls see
    assign = dev(c["assign"])
    base = _door_call(s0.float().clone().requires_grad_(), b0.float().clone().requires_grad_(), m, gts, pms, assign)      # fp32 contiguous copies
    wide = torch.full((2, 3, 5, 21), float("nan"), dtype=dtype, device=DEV)
    wide[..., 3:19] = s0
    pairs = torch.full((2, 3, 5, 18), float("nan"), dtype=dtype, device=DEV)
    pairs[..., ::2] = b0
    wide.requires_grad_()
    pairs.requires_grad_()
    sv, bv = wide[..., 3:19], pairs[..., ::2]
    assert not sv.is_contiguous() and not bv.is_contiguous()
    mask8 = m.to(torch.uint8)
    gts_t = gts if dtype == torch.float16 else [g.to(dtype) for g in gts]      # (rounded to fp16 the ground truth would be another batch)
    cost = gl.match_costs(sv, bv, mask8, gts_t, [p.to(torch.float64) for p in pms])[0]
    losses = gl.grounding_loss(sv, bv, mask8, gts_t, pms, assign)
    losses.sum().backward()
    assert bits_equal(cost, base[0]) and bits_equal(losses.detach(), base[1]) and losses.dtype == torch.float32
    assert wide.grad.dtype == dtype and wide.grad.shape == wide.shape and pairs.grad.dtype == dtype and pairs.grad.shape == pairs.shape
    assert torch.equal(wide.grad[..., 3:19], base[2].to(dtype)) and not wide.grad[..., :3].any() and not wide.grad[..., 19:].any()
    assert torch.equal(pairs.grad[..., ::2], base[3].to(dtype)) and not pairs.grad[..., 1::2].any() and base[3].any()


def test_a_side_stream_gives_the_bits_of_the_default_stream():
    c = dict(hungarian_case())
    s, b, m, gts, pms = ops(c)
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=16))

    def call():
        sg, bg = s.clone().requires_grad_(), b.clone().requires_grad_()
        out = mod.loss(sg, bg, m, gts, pms)
        sum(out.values()).backward()
        return [mod.assign(s, b, m, gts, pms), mod.predict(s, b)[1], gl.match_costs(s, b, m, gts, pms)[0], gl.box_iou3d(b[0, 0], gts[0]),
                sg.grad, bg.grad] + [v.detach() for v in out.values()]

    first = call()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        second = call()
    torch.cuda.current_stream(DEV).wait_stream(side)
    side.synchronize()
    assert torch.equal(first[0], second[0]) and (first[0] >= 0).any()
    for x, y in zip(first[1:], second[1:]):
        assert torch.isfinite(x).all() and bits_equal(x.reshape(-1), y.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------ 5. predict
@pytest.mark.parametrize("M", [1, 17, 256])
@pytest.mark.parametrize("rows", [15, 16, 17, 1000])
def test_predict_at_the_row_and_token_edges(rows, M):
    rng = np.random.default_rng(rows + M)
    scores = gu.f32(rng.normal(0.0, 2.0, (rows, M)))
    scores[rng.uniform(size=scores.shape) < 0.3] = -np.inf   # masked columns
    scores[1, 0] = 0.5                                       # (a row that is not all -inf)
    nan_row, inf_row, dead_row = rows - 1, 0, rows // 2
    scores[nan_row, M - 1], scores[inf_row, M // 2], scores[dead_row] = np.nan, np.inf, -np.inf
    got = host(gl.predict_scores(dev(scores)))
    _, ref = gh.predict_host(scores[None], np.zeros((1, rows, 9)))
    bad = np.arange(rows) == nan_row
    assert got.shape == (rows,) and np.array_equal(np.isnan(got), bad) and np.array_equal(np.isnan(ref), bad)
    assert got[inf_row] == 1.0 and got[dead_row] == 0.0 and ((got[~bad] >= 0) & (got[~bad] <= 1)).all()
    err = gu.close(got[~bad], ref[~bad], TOL)
    say(f"predict rows={rows} M={M}: max error {err:.2e}")
    boxes = dev(gu.random_boxes(2 * rows, 1).reshape(2, 1, rows, 9))
    out_boxes, out = GroundingLoss(contrastive_cfg=dict(max_text_len=M)).predict(dev(np.stack([np.zeros_like(scores), scores])[:, None]), boxes)
    assert torch.equal(out_boxes, boxes[-1]) and tuple(out.shape) == (1, rows) and np.array_equal(host(out)[0][~bad], got[~bad])
