"""The query selection behind the neck on the device (proxytransformation_amd/query_select.py, csrc/query_select.hip) against its numpy
specification (query_select_host.py): pack + score at rows that cross the 64-row tile and token counts that cross the 64-token tile,
the sorted top-k on tied and special scores, the box decode across its clamp, the whole stage end to end under the neck's near-tie
protocol, and the gradient of ``feats_list -> (feats, query)``."""
import copy

import numpy as np
import pytest
import torch

from proxytransformation_amd import query_select as qs, query_select_host as qh
from tests import neck_util as nu
from tests import query_select_util as qu
from tests import sparse_util as su

pytestmark = pytest.mark.gpu


def _dev_lists(feats, xyz):
    return [su.dev(f) for f in feats], [su.dev(p) for p in xyz]


def _hold_finite(name, got, r32, r64):
    """``su.hold`` on the finite entries; the others (-inf, NaN) must sit where both hosts have them."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    fin = np.isfinite(r64)
    assert got.shape == r64.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(r64)) and np.array_equal(np.isnan(r32), np.isnan(r64))
    assert np.array_equal(np.isneginf(got), np.isneginf(r64)) and np.array_equal(np.isfinite(got), fin) and fin.any()
    su.hold(name, got[fin], r32[fin], r64[fin])


# ------------------------------------------------------------------------------------------------------------------ pack + score
@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("T", [1, 7, 77, 256])
def test_pack_and_score(T, C):
    """B = 3, L = (65, 1, 257); scene 0 has tokens masked inside a 64-token tile, scene 1 no token at all; a NaN under a masked token
    (scene 0's token T // 2 when T >= 3, scene 1's token 0) leaves no trace, a NaN in every product of row 100 of scene 2 makes that score
    NaN.  Integer-valued operands: bit for bit against the fp32 host; N(0, 1): by ``hold``."""
    rows = qu.SMALL_ROWS
    for integer in (True, False):
        feats, xyz, text, mask = qu.inputs(rows, T, C, seed=20 + T + C, integer=integer)
        assert not mask[1].any() and mask[2].any() and mask[0].any() and (T < 3 or not mask[0, T // 2])
        if T >= 3:
            text[0, T // 2, 3] = np.nan
        text[1, 0, 0] = np.nan
        feats[2][100, 5] = np.nan
        bias = np.array([-4.5], np.float32)
        df, dx = _dev_lists(feats, xyz)
        pf, pc, pad, attn = qs.pack(df, dx, su.dev(mask))
        hf, hc, hpad = qh.pack_host(feats, xyz)
        nan_at = np.zeros(hf.shape, bool)
        nan_at[2, 100, 5] = True
        got_f = pf.cpu().numpy()
        assert np.array_equal(np.isnan(got_f), nan_at) and np.array_equal(got_f[~nan_at].view(np.uint32), hf[~nan_at].view(np.uint32))
        nu.bits(pc, hc)
        assert pad.dtype == torch.bool and np.array_equal(pad.cpu().numpy(), hpad) and hpad[1, 1:].all() and not hpad[2].any()
        assert attn.dtype == torch.bool and np.array_equal(attn.cpu().numpy(), ~mask)
        assert not got_f[0, 65:].any() and not pc.cpu().numpy()[1, 1:].any()          # zeros behind the rows
        for scaled in (True, False):
            s = qs.score(pf, rows, su.dev(text), su.dev(mask), su.dev(bias), scaled=scaled).cpu().numpy()
            r32 = qh.score_host(hf, hpad, text, mask, bias, scaled)
            r64 = qh.score_host(hf.astype(np.float64), hpad, text.astype(np.float64), mask, bias.astype(np.float64), scaled)
            assert np.isneginf(s[0, 65:]).all() and np.isneginf(s[1]).all() and np.isnan(s[2, 100]) and np.isnan(s).sum() == 1
            assert np.isfinite(s[0, :65]).all() and np.isfinite(np.delete(s[2], 100)).all()
            if integer:
                keep = ~np.isnan(r32)
                assert np.array_equal(np.isnan(s), np.isnan(r32)) and np.array_equal(s[keep].view(np.uint32), r32[keep].view(np.uint32))
            else:
                _hold_finite(f"score T={T} C={C} scaled={scaled}", s, r32, r64)
        if integer:                                          # without a bias: the raw maximum
            s = qs.score(pf, rows, su.dev(text), su.dev(mask), None, scaled=False).cpu().numpy()
            r32 = qh.score_host(hf, hpad, text, mask, None, False)
            keep = ~np.isnan(r32)
            assert np.array_equal(s[keep], r32[keep]) and np.array_equal(np.isnan(s), np.isnan(r32))


# ------------------------------------------------------------------------------------------------------------------ top-k
@pytest.mark.parametrize("K", [1, 3, 256, 300])
def test_sorted_topk_on_tied_and_special_scores(K):
    """Scores from 16 levels with +-0.0, +-inf and both NaN signs among them, in scenes of 700, 300 and 1200 rows (min L = 300); +inf
    behind every scene's rows, which must never be read.  Ties straddle the K-th place.  Indices equal to the host rule, in order, twice."""
    rows = qu.E2E_ROWS
    rng = np.random.default_rng(30)
    levels = np.concatenate([np.linspace(-1.0, 1.0, 10).astype(np.float32), np.array([0.0, -0.0, np.inf, -np.inf], np.float32), qu.nan_signs()])
    assert len(levels) == 16
    s = np.full((3, max(rows)), np.inf, np.float32)
    for b, n in enumerate(rows):
        s[b, :n] = levels[rng.integers(0, 16, n)]
    ref = qh.topk_sorted_host(s, rows, K)
    for b, n in enumerate(rows):                              # a tie straddles the K-th place
        key = np.sort(qh.topk_key(s[b, :n]))[::-1]
        assert n == K or key[K - 1] == key[K] or K == 1
    assert np.isnan(s[0, ref[0, 0]]) and not np.signbit(s[0, ref[0, 0]]) and all(np.signbit(s[b, :n][np.isnan(s[b, :n])]).any() for b, n in enumerate(rows))
    ds = su.dev(s)
    first, inv = qs.topk_sorted(ds, rows, K, return_inverse=True)
    second = qs.topk_sorted(ds, rows, K)
    assert first.dtype == torch.int64 and tuple(first.shape) == (3, K)
    assert np.array_equal(first.cpu().numpy(), ref) and np.array_equal(second.cpu().numpy(), ref)
    want = np.full(s.shape, -1, np.int32)
    for b in range(3):
        want[b, ref[b]] = np.arange(K)
    nu.bits(inv, want)


def test_sorted_topk_at_the_largest_k():
    """K = 1024, the most the sort holds (every thread carries four pairs per stage), on N(0, 1) scores with a block of equal ones across
    the K-th place of the first scene; the second scene has exactly K rows."""
    rows, K = (1500, 1024), 1024
    rng = np.random.default_rng(31)
    s = rng.standard_normal((2, 1500)).astype(np.float32)
    kth = np.sort(s[0])[::-1][K - 1]
    s[0, rng.permutation(1500)[:40]] = kth
    ref = qh.topk_sorted_host(s, rows, K)
    key = np.sort(qh.topk_key(s[0]))[::-1]
    assert key[K - 2] == key[K - 1] == key[K]
    got, inv = qs.topk_sorted(su.dev(s), rows, K, return_inverse=True)
    assert np.array_equal(got.cpu().numpy(), ref) and sorted(ref[1].tolist()) == list(range(1024))
    assert (inv.cpu().numpy()[1, 1024:] == -1).all() and (inv.cpu().numpy()[0] >= 0).sum() == K


def test_sixty_four_scenes():
    """B = 64, the most the kernel-argument structs hold: 1 to 64 rows per scene (K = 1), every output against the hosts on the device's
    indices, the indices by the host rule on the device's scores."""
    rows = tuple(1 + (7 * b) % 70 for b in range(64))
    feats, xyz, text, mask = qu.inputs(rows, 5, 64, seed=32)
    mask[1, 0] = True
    m = qu.module(C=64, num_queries=3)
    keep = {}
    with torch.no_grad():
        dec, _ = copy.deepcopy(m).to(su.DEV)([su.dev(f) for f in feats], None, [su.dev(p) for p in xyz], su.dev(text), su.dev(mask), keep_out=keep)
    index, score = keep["index"].cpu().numpy(), keep["score"].cpu().numpy()
    assert index.shape == (64, 1) and min(rows) == 1 and max(rows) == 64
    assert np.array_equal(index, qh.topk_sorted_host(score, rows, 1))
    d32, _ = m.forward_host(feats, None, xyz, text, mask, np.float32, index=index)
    d64, _ = m.forward_host(feats, None, xyz, text, mask, np.float64, index=index)
    for k in ("query", "feats", "query_coords", "feats_coords"):
        nu.bits(dec[k], d32[k])
    assert np.array_equal(dec["feats_attention_mask"].cpu().numpy(), d64["feats_attention_mask"])
    su.hold("64 scenes pred_bboxes", dec["pred_bboxes"].cpu().numpy(), d32["pred_bboxes"], d64["pred_bboxes"])
    h32, h64 = {}, {}
    m.forward_host(feats, None, xyz, text, mask, np.float32, keep_out=h32)
    m.forward_host(feats, None, xyz, text, mask, np.float64, keep_out=h64)
    _hold_finite("64 scenes score", score, h32["score"], h64["score"])


# ------------------------------------------------------------------------------------------------------------------ boxes
@pytest.mark.parametrize("C,fcs", [(256, 2), (64, 2), (128, 0), (64, 1)])
def test_boxes_and_gathers(C, fcs):
    """70 selected rows per scene (past the 64-row tile) out of 90: log-sizes on both sides of log 0.02, one selected row with a NaN.
    Boxes by ``hold`` against the hosts, the NaN row stays NaN; ``query`` / ``query_coords`` are the gathered rows bit for bit."""
    rng = np.random.default_rng(40 + C)
    B, L, K = 2, 90, 70
    feats = rng.standard_normal((B, L, C)).astype(np.float32)
    coords = (rng.integers(-500, 500, (B, L, 3)) * 0.01).astype(np.float32)
    index = np.stack([rng.permutation(L)[:K] for _ in range(B)]).astype(np.int64)
    feats[0, index[0, 5], 3] = np.nan
    m = qu.module(C=C, num_queries=K, num_reg_fcs=fcs)
    lins = m.linears()
    W = [l.weight.detach().numpy() for l in lins]
    bs = [l.bias.detach().numpy() for l in lins]
    df, dc, di = su.dev(feats), su.dev(coords), su.dev(index)
    h = None
    for i, l in enumerate(lins[:-1]):
        h = qs.linear(df if i == 0 else h, su.dev(W[i]), su.dev(bs[i]), di if i == 0 else None, relu=True)
    query, qcoords, boxes = qs.decode(h, su.dev(W[-1]), su.dev(bs[-1]), df, dc, di)
    q_ref = np.take_along_axis(feats, index[:, :, None], 1)
    c_ref = np.take_along_axis(coords, index[:, :, None], 1)
    got_q = query.cpu().numpy()
    nan_at = np.isnan(q_ref)
    assert nan_at.sum() == 1 and np.array_equal(np.isnan(got_q), nan_at) and np.array_equal(got_q[~nan_at].view(np.uint32), q_ref[~nan_at].view(np.uint32))
    nu.bits(qcoords, c_ref)
    r32 = qh.boxes_host(q_ref, c_ref, W, bs)
    r64 = qh.boxes_host(q_ref.astype(np.float64), c_ref.astype(np.float64), [w.astype(np.float64) for w in W], [b.astype(np.float64) for b in bs])
    got = boxes.cpu().numpy()
    assert np.isnan(got[0, 5]).all() and np.isnan(r64[0, 5]).all() and np.isnan(got).sum() == 9 == np.isnan(r32).sum()
    p = np.log(r64[..., 3:6][np.isfinite(r64[..., 3:6])])
    assert (r64[..., 3:6] == 0.02).mean() > 0.05 and (p > np.log(0.05)).mean() > 0.05          # below and above log 0.02
    ok = ~np.isnan(r64)
    su.hold(f"boxes C={C} fcs={fcs}", got[ok], r32[ok], r64[ok])
    small = (r64[..., 3:6] == 0.02) & (r32[..., 3:6] == np.float32(0.02))
    assert (got[..., 3:6][small] == np.float32(0.02)).all()


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def e2e():
    feats, xyz, text, mask = qu.e2e_inputs()
    m = qu.module()
    refs = {}
    for dt in (np.float32, np.float64):
        keep = {}
        m.forward_host(feats, None, xyz, text, mask, dt, keep_out=keep)
        refs[np.dtype(dt).name] = keep
    return feats, xyz, text, mask, m, refs


def test_end_to_end(e2e):
    feats, xyz, text, mask, m, refs = e2e
    rows, K = qu.E2E_ROWS, 256
    gm = copy.deepcopy(m).to(su.DEV)
    df, dx = _dev_lists(feats, xyz)
    dtext, dmask = su.dev(text), su.dev(mask)
    keep = {}
    with torch.no_grad():
        dec, head = gm(df, None, dx, dtext, dmask, keep_out=keep)
    score, index = keep["score"].cpu().numpy(), keep["index"].cpu().numpy()
    assert index.shape == (3, K) and index.dtype == np.int64 and score.shape == (3, 1200)
    # (a) the device's indices are the host rule applied to the device's own scores
    assert np.array_equal(index, qh.topk_sorted_host(score, rows, K))
    # (b) against the float64 host's own selection: differences only inside the near-tie margin, no more than there are near-ties
    s64, own = refs["float64"]["score"], refs["float64"]["index"]
    flat, _ = qu.scene_scores(s64, rows)
    margin = nu.NEAR_TIE * float(np.abs(flat).max())
    ties = {scene: count for scene, count, _ in qu.near_ties(s64, rows, K)}
    for b, n in enumerate(rows):
        d = np.array(sorted(set(index[b].tolist()) ^ set(own[b].tolist())), np.int64)
        kth = np.sort(s64[b, :n])[::-1][K - 1]
        print(f"scene {b}: {len(d)} rows differ, K-th score {kth:+.5f}, {ties[b]} near-ties")
        assert (np.abs(s64[b, d] - kth) <= margin).all() and len(d) <= ties[b] <= 0.02 * K
    _hold_finite("e2e score", score, refs["float32"]["score"], s64)
    # (c) every output by hold, with the device's indices handed to the hosts
    d32, _ = m.forward_host(feats, None, xyz, text, mask, np.float32, index=index)
    d64, h64 = m.forward_host(feats, None, xyz, text, mask, np.float64, index=index)
    assert list(dec) == list(d64) and list(head) == list(h64)
    for k in ("query", "feats", "query_coords", "feats_coords"):
        nu.bits(dec[k], d32[k])
    su.hold("e2e pred_bboxes", dec["pred_bboxes"].cpu().numpy(), d32["pred_bboxes"], d64["pred_bboxes"])
    assert not dec["pred_bboxes"].requires_grad and dec["pred_bboxes"].dtype == torch.float32 and tuple(dec["pred_bboxes"].shape) == (3, K, 9)
    assert dec["feats_attention_mask"].dtype == torch.bool and np.array_equal(dec["feats_attention_mask"].cpu().numpy(), d64["feats_attention_mask"])
    assert dec["text_attention_mask"].dtype == torch.bool and np.array_equal(dec["text_attention_mask"].cpu().numpy(), ~mask)
    assert dec["text_feats"] is dtext and head["text_feats"] is dtext and head["text_token_mask"] is dmask
    with torch.no_grad():                                        # twice: the same bits
        again, _ = gm(df, None, dx, dtext, dmask)
    assert all(torch.equal(dec[k], again[k]) for k in dec)


# ------------------------------------------------------------------------------------------------------------------ gradient
def _grad_case(m, feats, xyz, text, mask, use_feats=True, use_query=True, seed=50):
    gm = copy.deepcopy(m).to(su.DEV)
    gm.differentiable = True
    leaves = [su.dev(f, grad=True) for f in feats]
    keep = {}
    dec, _ = gm(leaves, None, [su.dev(p) for p in xyz], su.dev(text), su.dev(mask), keep_out=keep)
    assert dec["query"].requires_grad and dec["feats"].requires_grad and not dec["pred_bboxes"].requires_grad
    assert not dec["query_coords"].requires_grad and not dec["feats_coords"].requires_grad
    rng = np.random.default_rng(seed)
    G1 = rng.standard_normal(tuple(dec["feats"].shape)).astype(np.float32)
    G2 = rng.standard_normal(tuple(dec["query"].shape)).astype(np.float32)
    loss = 0
    if use_feats:
        loss = loss + (dec["feats"] * su.dev(G1)).sum()
    if use_query:
        loss = loss + (dec["query"] * su.dev(G2)).sum()
    loss.backward()
    index = keep["index"].cpu().numpy()
    ref = qh.backward_host(G1 if use_feats else None, G2 if use_query else None, index, [len(f) for f in feats])
    return [l.grad for l in leaves], ref, index


@pytest.mark.parametrize("shape", ["small", "e2e"])
def test_gradient_of_feats_and_query(shape, e2e):
    """``differentiable=True`` at L = (65, 1, 257) with K = 1 and at the end-to-end shape: dfeats bit for bit against the host backward --
    selected and unselected rows, padded (scenes 0 and 1) and unpadded (the longest) scenes -- with both outputs used, with the query
    alone and with the padded features alone; two runs give the same bits; without the flag it raises."""
    if shape == "small":
        feats, xyz, text, mask = qu.inputs(qu.SMALL_ROWS, 7, 64, seed=51)
        mask[1, 0] = True
        m = qu.module(C=64, num_queries=5)
        K = 1
    else:
        feats, xyz, text, mask, m, _ = e2e
        K = 256
    grads, ref, index = _grad_case(m, feats, xyz, text, mask)
    assert index.shape == (3, K)
    for b, (g, r) in enumerate(zip(grads, ref)):
        nu.bits(g, r)
        assert len(set(index[b].tolist())) == K and (len(r) == K or not np.isin(np.arange(len(r)), index[b]).all())
    again, _, index2 = _grad_case(m, feats, xyz, text, mask)
    assert np.array_equal(index, index2) and all(torch.equal(a, g) for a, g in zip(again, grads))
    for kw in (dict(use_feats=False), dict(use_query=False)):
        g1, r1, _ = _grad_case(m, feats, xyz, text, mask, **kw)
        for g, r in zip(g1, r1):
            nu.bits(g, r)
    gm = copy.deepcopy(m).to(su.DEV)
    with pytest.raises(NotImplementedError, match="differentiable=True"):
        gm([su.dev(f, grad=True) for f in feats], None, [su.dev(p) for p in xyz], su.dev(text), su.dev(mask))


# ------------------------------------------------------------------------------------------------------------------ edges
def test_an_empty_scene_gives_empties_and_refused_widths_name_their_number():
    feats, xyz, text, mask = qu.inputs((5, 0, 3), 7, 64, seed=60)
    gm = qu.module(C=64, num_queries=4).to(su.DEV)
    keep = {}
    with torch.no_grad():
        dec, _ = gm([su.dev(f) for f in feats], None, [su.dev(p) for p in xyz], su.dev(text), su.dev(mask), keep_out=keep)
    assert tuple(dec["query"].shape) == (3, 0, 64) and tuple(dec["query_coords"].shape) == (3, 0, 3) and tuple(dec["pred_bboxes"].shape) == (3, 0, 9)
    assert tuple(keep["index"].shape) == (3, 0) and keep["index"].dtype == torch.int64 and tuple(keep["score"].shape) == (3, 5)
    hf, hc, hpad = qh.pack_host(feats, xyz)
    nu.bits(dec["feats"], hf)
    nu.bits(dec["feats_coords"], hc)
    assert np.array_equal(dec["feats_attention_mask"].cpu().numpy(), hpad) and np.array_equal(dec["text_attention_mask"].cpu().numpy(), ~mask)
    gm.differentiable = True                                     # K = 0 in training: the padded features alone carry gradient
    leaves = [su.dev(f, grad=True) for f in feats]
    dec, _ = gm(leaves, None, [su.dev(p) for p in xyz], su.dev(text), su.dev(mask))
    G = np.random.default_rng(61).standard_normal((3, 5, 64)).astype(np.float32)
    (dec["feats"] * su.dev(G)).sum().backward()
    for leaf, ref in zip(leaves, qh.backward_host(G, None, np.zeros((3, 0), np.int64), (5, 0, 3))):
        nu.bits(leaf.grad, ref)
    gm.differentiable = False
    none = [su.dev(np.zeros((0, 64), np.float32))] * 2
    with torch.no_grad():
        dec, _ = gm(none, None, [su.dev(np.zeros((0, 3), np.float32))] * 2, su.dev(text[:2]), su.dev(mask[:2]))
    assert tuple(dec["query"].shape) == (2, 0, 64) and tuple(dec["feats"].shape) == (2, 0, 64) and tuple(dec["feats_attention_mask"].shape) == (2, 0)
    wide = su.dev(np.zeros((2, 6, 96), np.float32))
    with pytest.raises(ValueError, match="got 96"):
        qs.score(wide, [6, 6], su.dev(np.zeros((2, 7, 96), np.float32)), su.dev(mask[:2]))
    with pytest.raises(ValueError, match="got 576"):
        qs.pack([su.dev(np.zeros((4, 576), np.float32))], [su.dev(np.zeros((4, 3), np.float32))], su.dev(mask[:1]))
    with pytest.raises(ValueError, match="k=7 must be 1 to 1024 and at most the smallest scene's 6 rows"):
        qs.topk_sorted(su.dev(np.zeros((2, 9), np.float32)), [9, 6], 7)
    with pytest.raises(ValueError, match="got 32"):
        qs.linear(su.dev(np.zeros((2, 6, 64), np.float32)), su.dev(np.zeros((32, 64), np.float32)), None)
    with pytest.raises(ValueError, match="T=300"):
        qs.score(su.dev(np.zeros((1, 6, 64), np.float32)), [6], su.dev(np.zeros((1, 300, 64), np.float32)), su.dev(np.ones((1, 300), bool)))
