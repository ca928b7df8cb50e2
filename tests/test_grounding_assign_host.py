"""The matching's numpy specification (``grounding_loss_host.sap_assign_host``, which ``ptx_gl_assign`` reproduces bit for bit) against
scipy without a GPU, by the criterion of tests/grounding_assign_util.py: a matching of scipy's total cost everywhere, scipy's pairs on
inputs whose optimum is unique (established per input), the stated tie rule on hand-worked examples; the ``matcher`` keyword's refusals,
the declaration of the entry point and its argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from proxytransformation_amd import GroundingLoss, _abi, grounding_loss as gl, grounding_loss_host as gh
from tests import grounding_assign_util as au
from tests import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("K,G", au.RANDOM_SHAPES)
def test_specification_is_scipy_on_random_problems_with_a_unique_optimum(K, G, seed):
    cost, ref, gap = au.random_case(K, G, seed=seed)
    got = gh.sap_assign_host(cost, (G,), 1)
    print(f"K={K} G={G} seed {seed}: optimality gap {gap:.2e}")
    au.check_matching(got, cost, (G,), ref)
    assert np.array_equal(got, ref)


def _edge_sizes(K):
    return sorted({0, 1, K - 1, K, K + 1})


@pytest.mark.parametrize("NL,B", [(1, 1), (1, 3), (3, 1), (3, 3)])
@pytest.mark.parametrize("K,g", [(K, g) for K in (1, 5, 64) for g in _edge_sizes(K)])
def test_specification_at_the_edges_of_the_two_sides(K, g, NL, B):
    """``G_b`` around ``K`` (where the rows change sides) and 0; three scenes: an empty first one, the edge, a single box."""
    G = (g,) if B == 1 else (0, g, 1)
    cost = au.random_cost(NL, K, G, 31 * K + g + NL)
    au.require_unique(cost, G)
    got = gh.sap_assign_host(cost, G, B)
    ref = au.check_matching(got, cost, G)
    assert np.array_equal(got, ref)
    for b in range(B):
        assert ((got[:, b] >= 0).sum(-1) == min(K, G[b])).all()


@pytest.mark.parametrize("G", [(0, 4, 3), (4, 3, 0), (1,), (0, 1, 0), (0, 0)])
def test_specification_on_the_layouts_of_the_box_list(G):
    cost = au.random_cost(2, 6, G, 77 + len(G))
    au.require_unique(cost, G)
    got = gh.sap_assign_host(cost, G, len(G))
    assert np.array_equal(got, au.check_matching(got, cost, G))
    for b, g in enumerate(G):
        if g == 0:
            assert (got[:, b] == -1).all()
    with pytest.raises(ValueError, match="sum to"):
        gh.sap_assign_host(cost, G + (1,), len(G) + 1)
    assert gh.sap_assign_host(np.zeros((2, 0, 3), np.float32), (3,), 1).shape == (2, 1, 0)


@pytest.mark.parametrize("K,G", [(8, (3, 5)), (5, (9,)), (64, (17,))])
def test_nan_and_infinite_entries_are_mapped_as_the_host_path_maps_them(K, G):
    """NaN -> 100, +inf -> 100, -inf -> -100 (``grounding_loss._solve``): the specification's matching costs what ``_solve``'s costs on
    that mapped matrix (equal entries of 100 are ties: the pairs may differ)."""
    cost = au.special_cost(2, K, G, 5 + K)
    assert np.isnan(cost).any() and np.isposinf(cost).any() and np.isneginf(cost).any()
    got = gh.sap_assign_host(cost, G, len(G))
    today = gl._solve(cost, G, len(G))
    au.check_matching(got, cost, G, today)
    solo = np.array([[[np.nan, np.inf], [-np.inf, 3.0]]], np.float32)          # mapped: (100, 100; -100, 3): query 0 - box 1, query 1 - box 0
    assert np.array_equal(gh.sap_assign_host(solo, (2,), 1), [[[1, 0]]]) and np.array_equal(gl._solve(solo, (2,), 1), [[[1, 0]]])


@pytest.mark.parametrize("K,G", [(5, (5,)), (64, (3, 0, 70)), (9, (4, 9, 12))])
def test_ties_give_a_matching_of_the_optimal_total(K, G):
    for cost in (au.constant_cost(2, K, G), au.dyadic_cost(2, K, G, 3 + K)):
        got = gh.sap_assign_host(cost, G, len(G))
        au.check_matching(got, cost, G)


def test_the_tie_rule_takes_the_lowest_column_index():
    assert np.array_equal(gh.sap_assign_host(au.TIE_EXAMPLE, (3,), 1), au.TIE_EXAMPLE_ASSIGN)
    for cost, want in (au.TIE_WIDE, au.TIE_TALL):
        assert np.array_equal(gh.sap_assign_host(cost, (cost.shape[2],), 1), want)
    # a constant square matrix: every box meets query 0 first and ends on the lowest free query: the identity
    assert np.array_equal(gh.sap_assign_host(au.constant_cost(1, 7, (7,)), (7,), 1)[0, 0], np.arange(7))
    assert "LOWEST COLUMN INDEX" in gh.sap_assign_host.__doc__


@pytest.mark.parametrize("n", [32, 64])
def test_long_augmenting_paths_on_the_product_matrix(n):
    cost = au.product_cost(n)
    got = gh.sap_assign_host(cost, (n,), 1)
    au.check_matching(got, cost, (n,))
    assert np.array_equal(got[0, 0], np.arange(n)[::-1])     # the rearrangement inequality: the anti-diagonal, strictly


@pytest.mark.parametrize("K,G", au.STAGE_EDGE_SHAPES)
def test_specification_on_both_sides_of_the_staging_switch(K, G):
    """The shapes tests/test_gpu_grounding_assign_edges.py launches: on the random matrix (a unique optimum, established here) the
    specification's pairs are scipy's; on the special one (NaN and infinities mapped to +-100, many ties) a matching of scipy's total."""
    B = len(G)
    assert au.staged(K, max(G)) == (max(G) <= 128 or K <= 128)
    cost = au.stage_edge_cost("random", K, G)
    gap = au.require_unique(cost, G)
    print(f"K={K} G={G}: optimality gap {gap:.2e}")
    got = gh.sap_assign_host(cost, G, B)
    assert np.array_equal(got, au.check_matching(got, cost, G))
    cost = au.stage_edge_cost("special", K, G)
    assert np.isnan(cost).any() and np.isposinf(cost).any() and np.isneginf(cost).any()
    got = gh.sap_assign_host(cost, G, B)
    au.check_matching(got, cost, G)
    for b, g in enumerate(G):
        assert ((got[:, b] >= 0).sum(-1) == min(K, g)).all()


@pytest.mark.parametrize("K,g", [(256, 128), (128, 256)])
def test_long_augmenting_paths_on_the_product_rectangle(K, g):
    cost = au.product_cost_rect(K, g)
    assert cost.shape == (1, K, g) and float(cost.max()) == K * g
    au.check_matching(gh.sap_assign_host(cost, (g,), 1), cost, (g,))


def test_matcher_keyword_refusals_carry_the_numbers():
    for bad in ("gpu", "", None):
        with pytest.raises(ValueError, match="matcher must be 'host' or 'device'"):
            GroundingLoss(matcher=bad)
    with pytest.raises(TypeError):
        GroundingLoss(256, 256, 7, 2, 9, "baseline", True, True, 4, (0.2, 0.2, 0.2, 0.4), False, None, None, None, None, True, None, None,
                      "device")                              # keyword only
    assert GroundingLoss().matcher == "host" and GroundingLoss(matcher="device").matcher == "device"
    mask = torch.ones(1, 4, dtype=torch.bool)
    s, b = torch.zeros(1, 1, 300, 256), torch.zeros(1, 1, 300, 9)
    big = lambda g: ([torch.zeros(g, 9)], [torch.zeros(g, 256)])          # noqa: E731
    with pytest.raises(ValueError, match="matcher must be"):
        gl.hungarian_assign(s, b, mask, *big(1), matcher="scipy")
    mod = GroundingLoss(matcher="device")
    for call in (lambda: gl.hungarian_assign(s, b, mask, *big(257), matcher="device"), lambda: mod.assign(s, b, mask, *big(257)),
                 lambda: mod.loss(s, b, mask, *big(257))):
        with pytest.raises(ValueError, match=r"K=300, G_b=257 in scene 0.*matcher='host'"):
            call()
    with pytest.raises(ValueError, match=r"K=8, G_b=1025 in scene 0.*matcher='host'"):
        gl.hungarian_assign(s[:, :, :8], b[:, :, :8], mask, *big(1025), matcher="device")
    with pytest.raises(RuntimeError, match="no CPU path"):   # inside the limits the call goes on to the device
        mod.assign(s, b, mask, *big(256))
    with pytest.raises(RuntimeError, match="no CPU path"):   # and the host matcher has no such limit
        GroundingLoss().assign(s, b, mask, *big(257))


def test_header_binding_and_exports_declare_the_entry_point():
    lib = _abi.lib()
    hooks = ctypes.CDLL(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip_testhooks.so"))
    for name, params in su.assert_declared(au.GA_ENTRY_POINTS).items():
        assert len(params.split(",")) == len(_abi.SIGNATURES[name][1]) == 9, name
        getattr(hooks, name)
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13 and hooks.ptx_abi_version() == 13      # added without a new version
    assert "grounding_assign.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()


def test_argument_checks_answer_einval_before_touching_a_device():
    lib = _abi.lib()
    EINVAL = -1
    err = lambda: lib.ptx_last_error()                       # noqa: E731
    call = lambda NL=2, B=3, K=5, SG=9, max_g=4: lib.ptx_gl_assign(None, NL, B, K, None, SG, max_g, None, None)      # noqa: E731
    assert call(NL=0) == EINVAL and b"NL=0" in err() and call(NL=65) == EINVAL and b"NL=65" in err()
    assert call(B=65) == EINVAL and b"B=65" in err() and call(K=0) == EINVAL and b"K=0" in err()
    assert call(K=1025) == EINVAL and b"K=1025" in err() and call(SG=0) == EINVAL and b"SG=0" in err()
    assert call(max_g=0) == EINVAL and b"max_g=0" in err() and call(max_g=10) == EINVAL and b"max_g=10" in err()
    assert call(K=300, SG=900, max_g=257) == EINVAL and b"K=300 max_g=257" in err()
    assert call(K=8, SG=2000, max_g=1025) == EINVAL and b"K=8 max_g=1025" in err()
    assert call() == EINVAL and b"null" in err()
    assert call(K=256, SG=2000, max_g=1024) == EINVAL and b"null" in err()      # the limit itself passes the size checks
