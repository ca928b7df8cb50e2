"""The matching on the device (``ptx_gl_assign``, ``hungarian_assign(matcher='device')``, csrc/grounding_assign.hip): equal to its numpy
specification ``grounding_loss_host.sap_assign_host`` at every position, ties included; against scipy by the criterion of
tests/grounding_assign_util.py on inputs whose optimum is unique (established per input); written entirely, reproducible, on any stream;
through ``GroundingLoss(matcher='device')`` the same matching, loss and gradients as ``matcher='host'`` bit for bit, and no synchronise
from the decoder's first launch to the end of the backward."""
import copy
import functools

import numpy as np
import pytest
import torch

from proxytransformation_amd import GroundingLoss, _abi, grounding_loss as gl, grounding_loss_host as gh
from tests import decoder_train_util as tu
from tests import grounding_assign_util as au
from tests import grounding_loss_util as gu
from tests import query_select_util as qu
from tests import sparse_util as su
from tests.test_gpu_decoder import count_synchronises

pytestmark = pytest.mark.gpu
DEV = su.DEV
SENTINEL = -77


def dev(a, dtype=torch.float32):
    t = torch.from_numpy(np.array(a))                        # (a copy: the cached cases are read-only)
    return (t.to(dtype) if t.is_floating_point() else t).to(DEV)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def device_assign(cost, G, stream=None):
    """``ptx_gl_assign`` on ``cost (NL,K,sum G)`` into an output filled with a sentinel; returns the int32 tensor."""
    NL, K, SG = cost.shape
    B = len(G)
    c = dev(cost)
    offset = dev(np.concatenate([[0], np.cumsum(G)]).astype(np.int32))
    out = torch.full((NL, B, K), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    _abi.check(_abi.lib().ptx_gl_assign(c.data_ptr(), NL, B, K, offset.data_ptr(), SG, max(G), out.data_ptr(), s.cuda_stream), "ptx_gl_assign")
    s.synchronize()
    return out


def against_specification(cost, G):
    """Device == specification at every position; nothing of the sentinel left; -1 in the scenes without a box."""
    got = device_assign(cost, G).cpu().numpy()
    assert not (got == SENTINEL).any()
    for b, g in enumerate(G):
        if g == 0:
            assert (got[:, b] == -1).all()
    assert np.array_equal(got, gh.sap_assign_host(cost, G, len(G)))
    return got


@pytest.mark.parametrize("K", [1, 63, 64, 65, 256, 1024])
def test_lane_striping_edges(K):
    """Columns j = lane + 64 slot: one, just under / at / over a full slot, four slots, all sixteen; a few boxes, and more boxes than
    queries where that stays inside the limits."""
    G = (3, 1, min(K + 2, 256)) if K > 1 else (3, 1, 2)
    against_specification(au.random_cost(2, K, G, 40 + K), G)


@pytest.mark.parametrize("g", [0, 1, 4, 17, 65])
def test_box_counts_at_64_queries(g):
    """``G_b`` below and above K = 64: the rows are the boxes (read transposed), then the queries."""
    G = (g, 2)
    got = against_specification(au.random_cost(3, 64, G, 50 + g), G)
    assert ((got[:, 0] >= 0).sum(-1) == min(64, g)).all()


@pytest.mark.parametrize("K,g", [(K, K + d) for K in (5, 64) for d in (-1, 0, 1)])
def test_box_counts_around_the_number_of_queries(K, g):
    against_specification(au.random_cost(2, K, (g,), 60 + K + g), (g,))


@pytest.mark.parametrize("K,g", [(1024, 256), (256, 1024)])
def test_the_limit_shapes(K, g):
    """Too large for LDS: the matrix is read in place, by columns (K > G) and by rows."""
    cost = au.random_cost(1, K, (g,), 70 + K)
    got = against_specification(cost, (g,))
    au.check_matching(got, cost, (g,))


def test_many_layers_and_scenes_with_empty_ones():
    G = (0, 5, 0)
    got = against_specification(au.random_cost(6, 16, G, 81), G)
    assert (got[:, 0] == -1).all() and (got[:, 2] == -1).all() and ((got[:, 1] >= 0).sum(-1) == 5).all()
    G = tuple(int(g) for g in np.random.default_rng(82).integers(0, 12, 64))
    against_specification(au.random_cost(2, 8, G, 83), G)


@pytest.mark.parametrize("K,G", [(5, (5,)), (64, (3, 0, 70)), (9, (4, 9, 12))])
def test_ties_follow_the_specification(K, G):
    for cost in (au.constant_cost(2, K, G), au.dyadic_cost(2, K, G, 3 + K)):
        au.check_matching(against_specification(cost, G), cost, G)
    assert np.array_equal(against_specification(au.TIE_EXAMPLE, (3,)), au.TIE_EXAMPLE_ASSIGN)
    for cost, want in (au.TIE_WIDE, au.TIE_TALL):
        assert np.array_equal(against_specification(cost, (cost.shape[2],)), want)


@pytest.mark.parametrize("n", [64, 256])
def test_long_augmenting_paths_on_the_product_matrix(n):
    got = against_specification(au.product_cost(n), (n,))
    assert np.array_equal(got[0, 0], np.arange(n)[::-1])


@pytest.mark.parametrize("K,G", [(8, (3, 5)), (5, (9,)), (64, (17,))])
def test_nan_and_infinite_entries(K, G):
    cost = au.special_cost(2, K, G, 5 + K)
    got = against_specification(cost, G)
    au.check_matching(got, cost, G, gl._solve(cost, G, len(G)))


@pytest.mark.parametrize("K,G", au.RANDOM_SHAPES)
def test_device_against_scipy_on_random_problems_with_a_unique_optimum(K, G):
    cost, ref, gap = au.random_case(K, G)
    got = device_assign(cost, (G,)).cpu().numpy()
    au.check_matching(got, cost, (G,), ref)
    assert np.array_equal(got, ref), f"gap {gap:.2e}"


def test_two_launches_and_another_stream_give_the_same_bits():
    G = (7, 0, 40)
    cost = au.dyadic_cost(2, 70, G, 91)
    first = device_assign(cost, G)
    assert torch.equal(first, device_assign(cost, G))
    side = torch.cuda.Stream(device=DEV)
    assert torch.equal(first, device_assign(cost, G, side))
    bad = torch.tensor([0, 9, 3, 47], dtype=torch.int32, device=DEV)          # offsets out of order: the scenes they bound read nothing
    out = torch.full((2, 3, 70), SENTINEL, dtype=torch.int32, device=DEV)
    c = dev(cost)
    _abi.check(_abi.lib().ptx_gl_assign(c.data_ptr(), 2, 3, 70, bad.data_ptr(), 47, 40, out.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream),
               "ptx_gl_assign")
    got = out.cpu().numpy()
    assert (got[:, 1] == -1).all() and (got[:, 2] == -1).all()                # hi < lo; hi - lo = 44 > max_g
    assert np.array_equal(got[:, 0], gh.sap_assign_host(cost[:, :, :9], (9,), 1)[:, 0])


# ------------------------------------------------------------------------------------------------------------------ through the module
MODULE_SHAPE = dict(NL=2, B=3, K=32, M=16, T=7, tokens=(7, 3, 1), G=(3, 0, 7), seed=14)


@functools.lru_cache(maxsize=None)
def module_case():
    scores, boxes, mask, gts, pms = gu.batch(**MODULE_SHAPE)
    r = lambda a: np.asarray(a, np.float32)                  # noqa: E731
    return r(scores), r(boxes), mask, [r(g) for g in gts], [r(p) for p in pms]


def module_args(grad=False):
    scores, boxes, mask, gts, pms = module_case()
    s, b = dev(scores), dev(boxes)
    if grad:
        s.requires_grad_()
        b.requires_grad_()
    return s, b, dev(mask), [dev(g) for g in gts], [dev(p) for p in pms]


def test_module_assign_is_the_host_matchers():
    s, b, m, gts, pms = module_args()
    cost, G = gl.match_costs(s, b, m, gts, pms)
    au.require_unique(cost.cpu().numpy(), G)                 # the precondition, on the device's own matrices
    host = GroundingLoss(contrastive_cfg=dict(max_text_len=16)).assign(s, b, m, gts, pms)
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=16), matcher="device")
    got = mod.assign(s, b, m, gts, pms)
    assert got.dtype == torch.int32 and got.is_cuda and torch.equal(got, host)
    assert torch.equal(got, gl.hungarian_assign(s, b, m, gts, pms, matcher="device"))
    none = [torch.zeros((0, 9), device=DEV) for _ in range(3)], [torch.zeros((0, 16), device=DEV) for _ in range(3)]
    assert (mod.assign(s, b, m, *none) == -1).all()          # no box at all: no launch


def module_step(matcher):
    s, b, m, gts, pms = module_args(grad=True)
    mod = GroundingLoss(contrastive_cfg=dict(max_text_len=16), matcher=matcher)
    torch.cuda.synchronize()
    with count_synchronises() as calls:
        out = mod.loss(s, b, m, gts, pms)
        sum(out.values()).backward()
    return out, s.grad, b.grad, list(calls)


def test_module_loss_and_gradients_are_bit_identical_and_the_device_matcher_never_waits():
    host, hs, hb, host_calls = module_step("host")
    got, ds, db, calls = module_step("device")
    assert calls == [], f"matcher='device' synchronised: {calls}"
    assert host_calls == ["Stream.synchronize"], host_calls   # the counter sees the wait this removes
    assert list(got) == list(host) and all(bits_equal(got[k].detach(), host[k].detach()) for k in host)
    assert bits_equal(ds, hs) and bits_equal(db, hb) and bool(ds.abs().max() > 0) and bool(db.abs().max() > 0)


def chain_step(matcher, gts=None):
    """The smallest case of tests/decoder_train_util.py: decoder (differentiable) -> ``head_scores`` -> ``GroundingLoss.loss`` ->
    backward, everything from the decoder's first launch on under the counter."""
    m, branches, ops, _ = tu.dec_setup("small")
    md, bd = copy.deepcopy(m).to(DEV).train(), copy.deepcopy(branches).to(DEV).train()
    qs = qu.module(C=m.embed_dims, num_queries=ops["query"].shape[1]).to(DEV)
    t = {k: dev(v) for k, v in ops.items()}
    for k in ("query", "key", "text_feats"):
        t[k].requires_grad_()
    token_mask = ~t["text_attention_mask"]
    B = token_mask.shape[0]
    if gts is None:                                          # a pass without the counter: the targets sit next to the first predictions
        with torch.no_grad():                                # (eval: the running statistics stay)
            boxes = md.eval()(t["query"], t["key"], t["key"], t["key_padding_mask"], None, None, t["query_coords"], t["key_coords"], t["pred_bboxes"],
                       t["text_feats"], t["text_attention_mask"], bd)[1].cpu().numpy()
        rng = np.random.default_rng(33)
        gts = []
        for b, g in enumerate((2, 3)[:B]):
            gt = boxes[-1, b, :g] + rng.normal(0, 0.05, (g, 9))
            gt[:, 3:6] = np.abs(gt[:, 3:6]) + 0.05
            gts.append(dev(gt))
        md.train()
    pms = []
    for b, gt in enumerate(gts):
        pm = np.zeros((gt.shape[0], qs.max_text_len), np.float32)
        pm[:, np.nonzero(~ops["text_attention_mask"][b])[0][:2]] = 0.5
        pms.append(dev(pm))
    mod = GroundingLoss(matcher=matcher)
    torch.cuda.synchronize()
    with count_synchronises() as calls:
        hidden, boxes = md(t["query"], t["key"], t["key"], t["key_padding_mask"], None, None, t["query_coords"], t["key_coords"],
                           t["pred_bboxes"], t["text_feats"], t["text_attention_mask"], bd)
        scores = md.head_scores(hidden, dict(text_feats=t["text_feats"], text_token_mask=token_mask), qs, differentiable=True)
        out = mod.loss(scores, boxes, token_mask, gts, pms)
        sum(out.values()).backward()
    torch.cuda.synchronize()
    grads = {k: t[k].grad for k in ("query", "key", "text_feats")}
    grads.update({n: p.grad for n, p in md.named_parameters() if p.grad is not None})
    assign = mod.assign(scores.detach(), boxes.detach(), token_mask, gts, pms)
    return dict(grads=grads, calls=list(calls), gts=gts, assign=assign, out=out)


def test_the_chain_from_the_decoder_to_the_backward_never_waits():
    host = chain_step("host")
    got = chain_step("device", host["gts"])
    assert got["calls"] == [], f"the chain synchronised: {got['calls']}"
    assert host["calls"] == ["Stream.synchronize"], host["calls"]
    assert torch.equal(got["assign"], host["assign"]) and int((got["assign"] >= 0).sum()) == 5 * got["assign"].shape[0]
    assert set(got["grads"]) == set(host["grads"]) and len(got["grads"]) > 3
    for n, g in host["grads"].items():
        assert bits_equal(got["grads"][n], g), n
    assert all(bits_equal(got["out"][k].detach(), host["out"][k].detach()) for k in host["out"])
    assert bool(got["grads"]["query"].abs().max() > 0)
