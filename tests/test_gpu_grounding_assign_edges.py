"""``ptx_gl_assign`` on both sides of its switch between the matrix staged in LDS and the matrix read in place
(csrc/grounding_assign.hip: staged while min(K, max G) * max(K, max G) <= 32768 floats): the shapes of
``grounding_assign_util.STAGE_EDGE_SHAPES`` -- staged at exactly 128 KiB in either orientation, the first shapes read in place in either
orientation, and scenes of very different sizes in one launch that one of them takes out of staging -- by the rules of
tests/test_gpu_grounding_assign.py: the specification ``sap_assign_host`` at every position, scipy's total everywhere and scipy's pairs
where the optimum is unique (tests/test_grounding_assign_host.py establishes it per input).  The in-place path is fed NaN and the
infinities here (``ga_map`` at every read); a scene larger than ``max_g`` is answered with -1 and none of its columns read."""
import numpy as np
import pytest
import torch

from proxytransformation_amd import GroundingLoss, _abi, grounding_loss as gl, grounding_loss_host as gh
from tests import grounding_assign_util as au
from tests import grounding_loss_util as gu
from tests import sparse_util as su
from tests import test_gpu_grounding_assign as base

pytestmark = pytest.mark.gpu
DEV = su.DEV
SENTINEL = base.SENTINEL
dev, against_specification = base.dev, base.against_specification


@pytest.mark.parametrize("kind", ["random", "special", "dyadic"])
@pytest.mark.parametrize("K,G", au.STAGE_EDGE_SHAPES)
def test_both_sides_of_the_staging_switch(K, G, kind):
    cost = au.stage_edge_cost(kind, K, G)
    if kind == "special":
        assert np.isnan(cost).any() and np.isposinf(cost).any() and np.isneginf(cost).any()
    got = against_specification(cost, G)
    ref = au.check_matching(got, cost, G)
    if kind == "random":                                     # a unique optimum (the host module establishes it): scipy's pairs
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("K,g", [(256, 128), (128, 256)])
def test_long_augmenting_paths_at_the_staged_limit(K, g):
    """The product matrix on the 128 KiB rectangle, the boxes as the rows and the queries as the rows."""
    assert au.staged(K, g) and K * g == au.STAGE_FLOATS
    cost = au.product_cost_rect(K, g)
    au.check_matching(against_specification(cost, (g,)), cost, (g,))


def test_a_scene_over_max_g_is_answered_without_reading_it():
    """The matrix of (3, 129, 0, 40) boxes launched with ``max_g = 128``: the launch is staged, the 129-box scene exceeds ``max_g`` and
    comes back -1 everywhere although its columns hold NaN (read, they would be mapped to 100 and matched); the other scenes are the
    specification's, unchanged by what lies in those columns."""
    K, G = au.STAGE_EDGE_SHAPES[4]
    NL, B, SG, max_g = au.STAGE_EDGE_NL, len(G), sum(G), 128
    assert G[1] > max_g and max(G[0], G[2], G[3]) <= max_g and au.staged(K, max_g) and not au.staged(K, max(G))
    clean = au.stage_edge_cost("random", K, G)
    dirty = np.array(clean)
    dirty[:, :, G[0]:G[0] + G[1]] = np.nan
    offset = dev(np.concatenate([[0], np.cumsum(G)]).astype(np.int32))
    results = []
    for cost in (clean, dirty):
        c = dev(cost)
        out = torch.full((NL, B, K), SENTINEL, dtype=torch.int32, device=DEV)
        _abi.check(_abi.lib().ptx_gl_assign(c.data_ptr(), NL, B, K, offset.data_ptr(), SG, max_g, out.data_ptr(),
                                            torch.cuda.current_stream(DEV).cuda_stream), "ptx_gl_assign")
        results.append(out.cpu().numpy())
    spec = gh.sap_assign_host(clean, G, B)
    for got in results:
        assert not (got == SENTINEL).any()
        assert (got[:, 1] == -1).all() and (got[:, 2] == -1).all()
        for b in (0, 3):
            assert np.array_equal(got[:, b], spec[:, b]), b
            assert ((got[:, b] >= 0).sum(-1) == G[b]).all()
    assert np.array_equal(results[0], results[1])


def test_module_assign_at_the_staged_limit_is_the_host_matchers():
    """``GroundingLoss(matcher='device').assign`` with 256 queries and scenes of (128, 0, 5) boxes -- the launch stages 128 KiB, the boxes
    as the rows -- equals ``matcher='host'``; the optimum's uniqueness is established on the device's own matrices."""
    scores, boxes, mask, gts, pms = gu.batch(NL=2, B=3, K=256, M=16, T=7, tokens=(7, 3, 1), G=(128, 0, 5), seed=15)
    s, b, m = dev(np.asarray(scores, np.float32)), dev(np.asarray(boxes, np.float32)), dev(mask)
    gts, pms = [dev(np.asarray(g, np.float32)) for g in gts], [dev(np.asarray(p, np.float32)) for p in pms]
    cost, G = gl.match_costs(s, b, m, gts, pms)
    assert tuple(G) == (128, 0, 5) and au.staged(256, max(G))
    au.require_unique(cost.cpu().numpy(), G)
    host = GroundingLoss(contrastive_cfg=dict(max_text_len=16)).assign(s, b, m, gts, pms)
    got = GroundingLoss(contrastive_cfg=dict(max_text_len=16), matcher="device").assign(s, b, m, gts, pms)
    assert got.dtype == torch.int32 and got.is_cuda and torch.equal(got, host)
    counts = (got >= 0).sum(-1).cpu().numpy()
    assert (counts == np.array([128, 0, 5])[None]).all()
