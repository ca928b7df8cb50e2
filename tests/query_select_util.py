"""What the query selection's test modules share: the entry points, the small and the end-to-end inputs, the module with random weights,
the near-tie count per scene.  A plain module: no tests, no marks."""
import functools

import numpy as np
import torch

from proxytransformation_amd import QuerySelect
from tests import neck_util as nu

QS_ENTRY_POINTS = ("ptx_qs_pack", "ptx_qs_score", "ptx_qs_topk", "ptx_qs_linear", "ptx_qs_decode", "ptx_qs_bwd")
SMALL_ROWS = (65, 1, 257)          # crosses the 64-row tile on both sides; a one-row scene
E2E_ROWS, E2E_T, E2E_C, E2E_QUERIES = (700, 300, 1200), 77, 256, 256


def text_mask(B, T, seed):
    """(B,T) bool: scene 0 with tokens masked in the middle of a 64-token tile (every third token, and token T // 2), scene 1 without any
    token, the others a valid prefix of random length >= 1."""
    rng = np.random.default_rng(seed)
    m = np.zeros((B, T), bool)
    m[0] = np.arange(T) % 3 != 1
    m[0, T // 2] = T < 3
    for b in range(2, B):
        m[b, :int(rng.integers(1, T + 1))] = True
    return m


def inputs(rows, T, C, seed, integer=False):
    """``(feats_list, xyz_list, text (B,T,C), mask (B,T))`` as fp32 numpy arrays: N(0, 1), or small integers (every product and sum of the
    score is then exact in fp32)."""
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-4, 5, s).astype(np.float32)) if integer else (lambda *s: rng.standard_normal(s).astype(np.float32))
    feats = [draw(n, C) for n in rows]
    xyz = [(rng.integers(-500, 500, (n, 3)) * 0.01).astype(np.float32) for n in rows]
    return feats, xyz, draw(len(rows), T, C), text_mask(len(rows), T, seed + 1)


@functools.lru_cache(maxsize=None)
def e2e_inputs(seed=11):
    feats, xyz, text, _ = inputs(E2E_ROWS, E2E_T, E2E_C, seed)
    rng = np.random.default_rng(seed + 2)
    mask = np.zeros((len(E2E_ROWS), E2E_T), bool)
    for b in range(len(E2E_ROWS)):
        mask[b, :int(rng.integers(10, E2E_T + 1))] = True
    return feats, xyz, text, mask


def module(C=E2E_C, num_queries=E2E_QUERIES, seed=12, **kw):
    """``QuerySelect`` with N(0, 2 / C) layers and a last layer whose log-sizes p[3:6] are centred on log 0.02 = -3.9: about half
    of the sizes are clamped, and none is much larger than the centres and angles (one rounding error would otherwise decide ``hold``)."""
    torch.manual_seed(seed)
    m = QuerySelect(embed_dims=C, num_queries=num_queries, **kw)
    with torch.no_grad():
        for lin in m.linears():
            lin.weight.normal_(0.0, (2.0 / C) ** 0.5)
            lin.bias.normal_(0.0, 0.5)
        m.linears()[-1].bias[3:6] -= 3.9
    return m.eval()


def scene_scores(score, rows):
    """The scores of the rows that exist, flattened scene by scene, and the scene ends: what ``neck_util.near_ties`` takes."""
    return np.concatenate([np.asarray(score)[b, :n] for b, n in enumerate(rows)]), np.cumsum(rows).tolist()


def near_ties(score, rows, k):
    flat, ends = scene_scores(score, rows)
    return nu.near_ties(flat, ends, k)


def nan_signs():
    """(+NaN, -NaN) as fp32 bit patterns: no conversion touches the sign."""
    return np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
