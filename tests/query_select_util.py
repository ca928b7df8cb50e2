"""What the query selection's test modules share: the entry points, the small and the end-to-end inputs, the module with random weights,
the near-tie count per scene; and for tests/test_gpu_query_select_edges.py the fp32 / float64 reference pairs of the score, a layer and
the decode, scores built from radix keys, and scores with ``+inf`` behind every scene.  A plain module: no tests, no marks."""
import functools

import numpy as np
import torch

from proxytransformation_amd import QuerySelect, query_select_host as qh
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


# ------------------------------------------------------------------------------------------------------------------ the edges module
def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def gather(a, index):
    """``a[b, index[b, q]]`` of ``a (B,L,...)``: ``(B,K,...)``."""
    return np.take_along_axis(a, index[:, :, None], 1)


def score_refs(feats, pad, text, mask, bias, scaled):
    """``score_host`` on the packed fp32 operands and on their float64 copies: ``(ref32, ref64)``.  An ``inf * 0`` or a NaN under a masked
    token is what the callers plant: numpy's warnings about them are not the subject."""
    with np.errstate(invalid="ignore", over="ignore"):
        r32 = qh.score_host(feats, pad, text, mask, bias, scaled)
        r64 = qh.score_host(f64(feats), pad, f64(text), mask, f64(bias), scaled)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    return r32, r64


def linear_ref(rows, weight, bias, relu):
    """One layer of ``boxes_host``'s branch in the dtype of ``rows``: ``rows @ weight.T (+ bias)``, ReLU as ``np.maximum`` (a NaN stays)."""
    dt = rows.dtype
    with np.errstate(invalid="ignore"):
        h = rows @ np.asarray(weight, dt).T
    if bias is not None:
        h = h + np.asarray(bias, dt)
    return (np.maximum(h, dt.type(0)) if relu else h).astype(dt, copy=False)


def linear_refs(rows, weight, bias, relu):
    r32 = linear_ref(rows, weight, bias, relu)
    assert r32.dtype == np.float32
    return r32, linear_ref(f64(rows), weight, bias, relu)


def box_refs(h, weight, bias, coords):
    """``boxes_host`` of the last layer alone, fp32 and float64; ``bias=None`` is a zero bias (adding +0.0 changes no bit but a -0.0's
    sign, which no comparison here looks at)."""
    r32 = qh.boxes_host(h, coords, [weight], [np.zeros(9, np.float32) if bias is None else bias])
    assert r32.dtype == np.float32
    return r32, qh.boxes_host(f64(h), f64(coords), [f64(weight)], [np.zeros(9) if bias is None else f64(bias)])


def key_scores(keys):
    """The fp32 scores whose ``neck_host.topk_key`` are the uint32 ``keys``, as bit patterns (no arithmetic touches them).  The key
    ``0x7FFFFFFF`` belongs to no score: it would be ``-0.0``, which shares ``+0.0``'s key."""
    k = np.asarray(keys, np.uint32)
    assert not (k == np.uint32(0x7FFFFFFF)).any()
    u = np.where((k >> np.uint32(31)) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    s = u.view(np.float32)
    assert np.array_equal(qh.topk_key(s), k)
    return s


def padded_scores(scenes, behind=3):
    """``(B, max rows + behind)`` fp32 with scene b's scores at ``[b, :rows[b]]`` and ``+inf`` behind them, which no selection may read;
    and the row counts."""
    rows = tuple(len(s) for s in scenes)
    out = np.full((len(scenes), max(rows) + behind), np.inf, np.float32)
    for b, s in enumerate(scenes):
        out[b, :rows[b]] = s
    return out, rows
