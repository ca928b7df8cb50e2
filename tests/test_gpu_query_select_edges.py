"""The query selection's kernels (csrc/query_select.hip, proxytransformation_amd/query_select.py) at the edges tests/test_gpu_query_select.py
does not reach, each at the smallest shape that takes the path.  References: the numpy restatements of ``query_select_host.py`` in float32
and float64; bit for bit where the arithmetic is exact (pack, gathers, indices, ``inv``, the backward, scores and layers on integer-valued
operands), ``sparse_util.hold`` (8 x the fp32 host's error against float64) where a result is a rounded sum, ``_hold_finite`` where
``-inf`` / NaN entries must sit where both hosts have them, ``sparse_util.hold_pooled`` where a call has fewer than 64 results.
Selections need no near-tie statistics: indices are held against ``topk_sorted_host`` on the device's own scores or on scores the test
built, everything downstream on the device's indices handed to the hosts.

score      C = 64 .. 512 in steps of 64 (``sqrtf(C)`` is no power of two at six of them; 1 to 8 channel chunks) on rows (63, 0, 64, 128,
           1) -- the empty scene between non-empty ones -- at T in 1, 63, 64, 65, 129, 256: the four (scaled, bias) pairs, integer
           operands bit for bit, N(0, 1) by ``hold``, ``-inf`` exactly on padded rows and in the empty scene.
masks      per scene of one batch at T = 129 and 256: only the last token; a leading 64-token tile masked; only tokens 32 .. 63 (the
           upper column half of a tile) with a row's true maximum built at token 40; only token 0; no token.  NaNs in the text under
           masked tokens and ``inf * 0`` under a masked token leave no trace, NaN feature rows in both halves of the C/D layout give NaN
           in exactly those rows.
top-k      keys built from bit patterns: all equal but one radix digit that takes all 256 values, the K-th key's digit at 255, in between
           and at 0; scenes of one value (0.5, ``-inf``, +NaN); K = rows at 5, 255, 257, 300; K on both sides of the sort's powers of
           two with a tie across the K-th place; signed zeros by row; ``inv`` behind short scenes; ``+inf`` behind every scene's rows;
           every call twice.  A ``scores`` / a ``feats`` of the wrong rank is refused with the ``ValueError`` that names its shape.
linear     (Cin, Cout) in (64, 512), (512, 64), (192, 320), (512, 512) on (B, K) in (1, 1), (1, 63), (1, 64), (3, 21), (3, 22) and
           (2, 1024): with an index into K + 7 rows and without, with and without bias and ReLU, a NaN source row.
decode     C in 64, 192, 320, 448, 512 on (B, K) in (1, 1), (1, 15), (1, 16), (1, 17), (3, 7), (1, 257): with ``h`` and without, with and
           without a bias, sizes on both sides of the clamp, a NaN in ``h``, a NaN coordinate, integer operands.
backward   C in 64, 192, 512 on rows (65, 1, 130) with K = 1, and rows (40, 40) with every row selected: stride-0 gradients, the weighted
           form, some leaves without grad, a float64 leaf, twice.
module     masks as uint8 / int64 / a slice of a wider mask, ``text_feats`` as a strided view, scenes as slices of one buffer, float64 and
           fp16 features; ``bias=False, log_scale=None``; ``num_reg_fcs=0``; no scene with a token; a scene alone against its batch."""
import copy
import math

import numpy as np
import pytest
import torch

from proxytransformation_amd import query_select as qs, query_select_host as qh
from tests import neck_util as nu
from tests import query_select_util as qu
from tests import sparse_util as su
from tests.sparse_util import hold_pooled
from tests.test_gpu_query_select import _dev_lists, _hold_finite

pytestmark = pytest.mark.gpu
BIAS = np.array([-4.5], np.float32)
PAIRS = [(scaled, bias) for scaled in (True, False) for bias in (BIAS, None)]          # the four (scaled, bias) pairs


def host(t):
    return t.cpu().numpy()


def opt(a):
    return None if a is None else su.dev(a)


def ints(rng, *shape, lo=-4, hi=5):
    return rng.integers(lo, hi, shape).astype(np.float32)


def normal(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def same_bits_but(out, clean, at):
    """``out`` has the bits of ``clean`` everywhere but at ``at`` (an index tuple)."""
    out = out.copy()
    out[at] = clean[at]
    nu.bits(out, clean)


# ------------------------------------------------------------------------------------------------------------------ 1. score at every width
SCORE_ROWS = (63, 0, 64, 128, 1)
SCORE_T = (1, 63, 64, 65, 129, 256)
SCORE_CASES = sorted({(C, T) for C in range(64, 513, 64) for T in (65, 256)} | {(C, T) for C in (128, 512) for T in SCORE_T})


@pytest.mark.parametrize("C,T", SCORE_CASES)
def test_score_at_every_width(C, T):
    """Integer operands from -4 .. 4: at C = 512 every partial sum stays below 2^24 and the division by ``float32(sqrt(C))`` is one
    correctly rounded operation on both sides.  Scene 0 has every third token masked, scene 1 is empty (and has no token), the others a
    valid prefix."""
    rows = SCORE_ROWS
    for integer in (True, False):
        feats, xyz, text, mask = qu.inputs(rows, T, C, seed=1000 + C + T, integer=integer)
        assert not mask[1].any() and all(mask[b].any() for b in (0, 2, 3, 4))
        pf, _, pad, _ = qs.pack(*_dev_lists(feats, xyz), su.dev(mask))
        hf, _, hpad = qh.pack_host(feats, xyz)
        nu.bits(pf, hf)
        assert np.array_equal(host(pad), hpad) and hpad[1].all() and hpad.shape == (5, 128)
        dtext, dmask = su.dev(text), su.dev(mask)
        for scaled, bias in PAIRS:
            s = host(qs.score(pf, rows, dtext, dmask, opt(bias), scaled=scaled))
            r32, r64 = qu.score_refs(hf, hpad, text, mask, bias, scaled)
            assert np.isneginf(s[hpad]).all() and np.isneginf(s[1]).all() and np.isfinite(s[~hpad]).all() and (~hpad).sum() == 256
            if integer:
                nu.bits(s, r32)
            else:
                _hold_finite(f"score C={C} T={T} scaled={scaled} bias={bias is not None}", s, r32, r64)


# ------------------------------------------------------------------------------------------------------------------ 2. score under mask shapes
MASK_ROWS = (101, 64, 65, 40, 70)


def _mask_shapes(T):
    """(a) only token T - 1; (b) the first 64 tokens masked; (c) only tokens 32 .. 63; (d) only token 0; (e) no token."""
    m = np.zeros((5, T), bool)
    m[0, T - 1], m[1, 64:], m[2, 32:64], m[3, 0] = True, True, True, True
    return m


@pytest.mark.parametrize("T", [129, 256])
def test_score_under_mask_shapes(T):
    C, rows, row = 128, MASK_ROWS, 5
    mask = _mask_shapes(T)
    for integer in (True, False):
        feats, xyz, text, _ = qu.inputs(rows, T, C, seed=1100 + T, integer=integer)
        # (c): the true maximum of row 5 sits at token 40, in the upper column half of the tile, by construction
        f = feats[2][row]
        text[2, 40] = np.where(f > 0, 4.0, -4.0).astype(np.float32) if integer else (0.5 * f).astype(np.float32)
        products = qu.f64(f) @ qu.f64(text[2]).T
        products[~mask[2]] = -np.inf
        assert int(np.argmax(products)) == 40 and (np.delete(products, 40) < products[40]).all()
        # NaNs under masked tokens, beside the valid ones and in both column halves; (e): under every token
        planted = [(0, 0, 3), (0, T - 2, 0), (1, 10, 1), (1, 63, 2), (2, 5, 0), (2, 31, 0), (2, 64, 0), (3, 1, 0), (3, 32, 0), (3, T - 1, 5)]
        for at in planted:
            assert not mask[at[0], at[1]]
            text[at] = np.nan
        text[4] = np.nan
        # +inf in a feature row: inf * 0 = NaN under the masked token 1, inf * 2 = +inf under the only valid one
        feats[0][7, 9], text[0, 1, 9], text[0, T - 1, 9] = np.inf, 0.0, 2.0
        # NaN feature rows: tile-local row 36 of the second tile (hh = 1 of the C/D layout) and tile-local row 3 (hh = 0)
        feats[0][64 + 36, 11], feats[2][3, 0] = np.nan, np.nan
        nan_at = np.zeros((5, max(rows)), bool)
        nan_at[0, 100], nan_at[2, 3] = True, True
        pf, _, _, attn = qs.pack(*_dev_lists(feats, xyz), su.dev(mask))
        hf, _, hpad = qh.pack_host(feats, xyz)
        assert np.array_equal(host(attn), ~mask)
        for scaled, bias in PAIRS:
            s = host(qs.score(pf, rows, su.dev(text), su.dev(mask), opt(bias), scaled=scaled))
            r32, r64 = qu.score_refs(hf, hpad, text, mask, bias, scaled)
            assert np.isnan(s).sum() == 2 and np.array_equal(np.isnan(s), nan_at) and np.array_equal(np.isnan(r64), nan_at)
            assert s[0, 7] == np.inf and r64[0, 7] == np.inf and r32[0, 7] == np.inf
            assert np.isneginf(s[4]).all() and np.isneginf(s[hpad]).all()
            live = ~hpad & ~nan_at
            live[4], live[0, 7] = False, False
            assert np.isfinite(s[live]).all()
            if integer:
                keep = ~nan_at
                assert np.array_equal(s[keep].view(np.uint32), r32[keep].view(np.uint32))
                want = np.float32(4.0 * np.abs(f).sum())
                if scaled:
                    want = want / np.float32(math.sqrt(C))
                if bias is not None:
                    want = want + bias[0]
                assert s[2, row] == np.float32(want)
            else:
                _hold_finite(f"score masks T={T} scaled={scaled} bias={bias is not None}", s, r32, r64)


# ------------------------------------------------------------------------------------------------------------------ 3. top-k on constructed keys
def _topk(scenes, K):
    """The scenes' scores with ``+inf`` behind them; both forms of the call; the host rule's indices and inverse, bit for bit."""
    s, rows = qu.padded_scores(scenes)
    assert all(np.isposinf(s[b, n:]).all() and s.shape[1] >= n + 3 for b, n in enumerate(rows))
    ref = qh.topk_sorted_host(s, rows, K)
    ds = su.dev(s)
    first, inv = qs.topk_sorted(ds, rows, K, return_inverse=True)
    second = qs.topk_sorted(ds, rows, K)
    assert first.dtype == torch.int64 and inv.dtype == torch.int32
    nu.bits(first, ref)
    nu.bits(second, ref)
    want = np.full(s.shape, -1, np.int32)
    for b in range(len(rows)):
        want[b, ref[b]] = np.arange(K)
    nu.bits(inv, want)
    return ref


BASE_KEY = 0xC1234567                                        # the scores around 10.2 where the top digit is the base's


@pytest.mark.parametrize("digit", [0, 1, 2, 3])
def test_topk_on_keys_that_differ_in_one_radix_digit(digit):
    """600 rows whose keys are ``BASE_KEY`` but for one 8-bit digit, which takes all 256 values: 255 .. 88 twice, 87 .. 0 three times (at
    digit 3 the scores are finite values of both signs, denormals and a sign-set NaN).  In descending order the K-th key's digit is 255 at
    K = 1 (one of its two rows), 106 at K = 299 (one of two) and 0 at K = 599 (two of three): the ends of the suffix scan."""
    n, shift = 600, np.uint32(8 * digit)
    rng = np.random.default_rng(1200 + digit)
    values = rng.permutation(np.arange(n) % 256).astype(np.uint32)
    keys = (np.uint32(BASE_KEY) & ~(np.uint32(0xFF) << shift)) | (values << shift)
    s = qu.key_scores(keys)
    ordered = np.sort(keys)[::-1]
    assert len(np.unique(keys)) == 256 and len(np.unique(keys & ~(np.uint32(0xFF) << shift))) == 1
    for K, want in ((1, 255), (299, 106), (599, 0)):
        assert int((ordered[K - 1] >> shift) & np.uint32(255)) == want and ordered[K - 1] == ordered[K]
        ref = _topk([s], K)
        assert np.array_equal(keys[ref[0]], ordered[:K])


@pytest.mark.parametrize("n", [257, 5])
def test_topk_on_a_scene_that_is_one_value(n):
    """``need = K`` and no row above the threshold: 0.5, ``-inf`` and +NaN throughout, one scene each.  Rows 0 .. K - 1 in order."""
    scenes = [np.full(n, v, np.float32) for v in (np.float32(0.5), np.float32(-np.inf), qu.nan_signs()[0])]
    assert np.isnan(scenes[2]).all() and not np.signbit(scenes[2]).any()
    for K in sorted({1, 5, n}):
        ref = _topk(scenes, K)
        assert (ref == np.arange(K)).all()


@pytest.mark.parametrize("n", [5, 255, 257, 300])
def test_topk_that_takes_every_row(n):
    """K = rows, no power of two: the sort's padding pairs stay behind the real ones, and below 256 rows most threads own no row."""
    s = normal(np.random.default_rng(1300 + n), n)
    ref = _topk([s], n)
    assert sorted(ref[0].tolist()) == list(range(n)) and (np.diff(s[ref[0]]) < 0).all()


@pytest.mark.parametrize("K", [255, 256, 257, 511, 513])
def test_topk_on_both_sides_of_the_sorts_powers_of_two(K):
    """1 100 rows of N(0, 1) with 40 equal scores laid across the K-th place (20 above it, 20 below, at random rows)."""
    rng = np.random.default_rng(1400 + K)
    s = normal(rng, 1100)
    order = np.argsort(-s, kind="stable")
    s[order[K - 20:K + 20]] = s[order[K - 1]]
    key = np.sort(qh.topk_key(s))[::-1]
    assert key[K - 21] > key[K - 20] == key[K - 2] == key[K - 1] == key[K] == key[K + 19] > key[K + 20]
    ref = _topk([s], K)
    tied = np.sort(order[K - 20:K + 20])
    assert sorted(ref[0, K - 20:].tolist()) == tied[:20].tolist()          # of the tie: the 20 lowest rows


def test_topk_orders_signed_zeros_by_row():
    """``-0.0`` and ``+0.0`` alternate over 30 rows across the K-th place: one key, so the row decides, whatever the sign."""
    n, K = 90, 25
    rng = np.random.default_rng(1500)
    place = rng.permutation(n)
    zeros = np.sort(place[10:40])
    s = np.empty(n, np.float32)
    s[place[:10]] = rng.uniform(1.0, 2.0, 10).astype(np.float32)
    s[place[40:]] = -rng.uniform(1.0, 2.0, 50).astype(np.float32)
    s[zeros] = np.where(np.arange(30) % 2 == 0, -0.0, 0.0).astype(np.float32)
    assert np.signbit(s[zeros]).sum() == 15 and not s[zeros].any()
    ref = _topk([s], K)
    assert ref[0, 10:].tolist() == zeros[:15].tolist() and 0 < np.signbit(s[ref[0, 10:]]).sum() < 15


def test_topk_inverse_behind_short_scenes_and_a_refused_rank():
    """Rows (1 100, 5, 300) at K = 5: ``inv`` is ``-1`` behind the short scenes' rows (``_topk`` holds every element).  A ``scores`` that
    is not ``(B, Lmax)``, and a ``feats`` that is not ``(B, Lmax, C)`` in ``decode``, are refused with the ``ValueError`` that names the shape."""
    rng = np.random.default_rng(1600)
    _topk([normal(rng, 1100), normal(rng, 5), normal(rng, 300)], 5)
    for bad in (np.zeros(9, np.float32), np.zeros((1, 9, 1), np.float32)):
        with pytest.raises(ValueError, match=r"scores \(B,Lmax\)"):
            qs.topk_sorted(su.dev(bad), [9], 3)
    flat = su.dev(np.zeros((9, 64), np.float32))
    with pytest.raises(ValueError, match=r"feats \(B,Lmax,C\) expected, got \(9, 64\)"):
        qs.decode(None, su.dev(np.zeros((9, 64), np.float32)), None, flat, su.dev(np.zeros((9, 3), np.float32)), su.dev(np.zeros((1, 3), np.int64)))


# ------------------------------------------------------------------------------------------------------------------ 4. linear
LINEAR_CASES = [(cin, cout, B, K) for cin, cout in ((64, 512), (512, 64), (192, 320), (512, 512))
                for B, K in ((1, 1), (1, 63), (1, 64), (3, 21), (3, 22))] + [(512, 512, 2, 1024)]


@pytest.mark.parametrize("cin,cout,B,K", LINEAR_CASES)
def test_linear_off_the_square(cin, cout, B, K):
    """With an index the rows are gathered out of ``K + 7`` in permuted order (3 x 21 = 63 and 3 x 22 = 66 rows: the scene boundaries lie
    inside a 64-row tile), without one the K rows themselves.  Integer operands (weights from -2 .. 2) bit for bit, N(0, 1) by ``hold``."""
    rng = np.random.default_rng(2000 + cin + 3 * cout + 7 * B + K)
    L = K + 7
    index = np.stack([rng.permutation(L)[:K] for _ in range(B)]).astype(np.int64)
    forms = [(L, index), (K, None)]
    run = lambda x, w, b, idx, relu: host(qs.linear(su.dev(x), su.dev(w), opt(b), opt(idx), relu=relu))      # noqa: E731
    rows_of = lambda x, idx: x if idx is None else qu.gather(x, idx)      # noqa: E731
    wi, bi = ints(rng, cout, cin, lo=-2, hi=3), ints(rng, cout)
    w, b = (normal(rng, cout, cin) / np.float32(cin ** 0.5)).astype(np.float32), normal(rng, cout)
    for n, idx in forms:
        xi = ints(rng, B, n, cin)
        x = normal(rng, B, n, cin)
        assert (qu.linear_ref(rows_of(xi, idx), wi, bi, False) < 0).mean() > 0.2
        for bias_on in (True, False):
            for relu in (True, False):
                got = run(xi, wi, bi if bias_on else None, idx, relu)
                assert got.shape == (B, K, cout)
                nu.bits(got, qu.linear_ref(rows_of(xi, idx), wi, bi if bias_on else None, relu))
                bb = b if bias_on else None
                hold_pooled(f"linear {cin}->{cout} rows=({B}, {K}) index={idx is not None} bias={bias_on} relu={relu}", B * K * cout,
                            lambda: (normal(rng, B, n, cin),), lambda x_: run(x_, w, bb, idx, relu),
                            lambda x_: qu.linear_refs(rows_of(x_, idx), w, bb, relu))
        # a NaN in a source row: the ReLU keeps it, every other row keeps its bits; behind an index, an unselected NaN row leaves no trace
        clean = run(x, w, b, idx, True)
        bad, b0, q0 = x.copy(), B - 1, K // 2
        if idx is None:
            bad[b0, q0, cin - 3] = np.nan
        else:
            bad[b0, idx[b0, q0], cin - 3] = np.nan
            bad[0, np.setdiff1d(np.arange(L), idx[0])[0], 0] = np.nan
        out = run(bad, w, b, idx, True)
        assert np.isnan(out[b0, q0]).all() and np.isnan(out).sum() == cout
        same_bits_but(out, clean, (b0, q0))


# ------------------------------------------------------------------------------------------------------------------ 5. decode
DECODE_ROWS = ((1, 1), (1, 15), (1, 16), (1, 17), (3, 7), (1, 257))


@pytest.mark.parametrize("C", [64, 192, 320, 448, 512])
def test_decode_at_every_lane_count(C):
    rng = np.random.default_rng(3000 + C)
    w = (normal(rng, 9, C) * np.float32((2.0 / C) ** 0.5)).astype(np.float32)
    b = (normal(rng, 9) * np.float32(0.5)).astype(np.float32)
    b[3:6] -= np.float32(3.9)                                # the log-sizes centred on log 0.02, as query_select_util.module
    sizes = []
    for B, K in DECODE_ROWS:
        L = K + 7
        index = np.stack([rng.permutation(L)[:K] for _ in range(B)]).astype(np.int64)
        di = su.dev(index)
        draw = lambda: (normal(rng, B, L, C), (rng.integers(-500, 500, (B, L, 3)) * 0.01).astype(np.float32), normal(rng, B, K, C))      # noqa: E731
        for use_h in (True, False):
            src = lambda f, h: h if use_h else qu.gather(f, index)      # noqa: E731
            for bias in (None, b):                           # (the NaN cases below run with the bias)
                call = lambda f, c, h: tuple(host(t) for t in qs.decode(su.dev(h) if use_h else None, su.dev(w), opt(bias), su.dev(f), su.dev(c), di))      # noqa: E731
                name = f"decode C={C} rows=({B}, {K}) h={use_h} bias={bias is not None}"
                (f, c, h), got = hold_pooled(name, 9 * B * K, draw, lambda f, c, h: call(f, c, h)[2],
                                             lambda f, c, h: qu.box_refs(src(f, h), w, bias, qu.gather(c, index)))
                query, qcoords, boxes = call(f, c, h)
                nu.bits(query, qu.gather(f, index))
                nu.bits(qcoords, qu.gather(c, index))
                nu.bits(boxes, got)
                assert got.shape == (B, K, 9)
                r32, r64 = qu.box_refs(src(f, h), w, bias, qu.gather(c, index))
                small = (r64[..., 3:6] == 0.02) & (r32[..., 3:6] == np.float32(0.02))
                assert (got[..., 3:6][small] == np.float32(0.02)).all()
                if bias is not None:
                    sizes.append(r64[..., 3:6].ravel())
            # a NaN in the branch's input (h, or the selected feature row): the nine values of that row are NaN, the clamp keeps it
            b0, q0 = B - 1, K // 2
            fb, hb = f.copy(), h.copy()
            if use_h:
                hb[b0, q0, C - 2] = np.nan
            else:
                fb[b0, index[b0, q0], C - 2] = np.nan
            out = call(fb, c, hb)[2]
            clean = call(f, c, h)[2]
            assert np.isnan(out[b0, q0]).all() and np.isnan(out).sum() == 9
            same_bits_but(out, clean, (b0, q0))
            # a NaN coordinate: that centre value only, and the same NaN bits in query_coords
            cb = c.copy()
            cb[b0, index[b0, q0], 1] = np.array([0x7FC01234], np.uint32).view(np.float32)[0]
            _, qc, out = call(f, cb, h)
            assert np.isnan(out[b0, q0, 1]) and np.isnan(out).sum() == 1
            same_bits_but(out, clean, (b0, q0, 1))
            nu.bits(qc, qu.gather(cb, index))
            assert qc[b0, q0, 1:2].view(np.uint32)[0] == 0x7FC01234
            # integer-valued operands: centre and euler bit for bit
            fi, hi, wi, bi = ints(rng, B, L, C, lo=-2, hi=3), ints(rng, B, K, C, lo=-2, hi=3), ints(rng, 9, C, lo=-2, hi=3), ints(rng, 9)
            ci = ints(rng, B, L, 3, lo=-9, hi=10)
            exact = host(qs.decode(su.dev(hi) if use_h else None, su.dev(wi), su.dev(bi), su.dev(fi), su.dev(ci), di)[2])
            ref = qh.boxes_host(hi if use_h else qu.gather(fi, index), qu.gather(ci, index), [wi], [bi])
            nu.bits(np.ascontiguousarray(exact[..., :3]), np.ascontiguousarray(ref[..., :3]))
            nu.bits(np.ascontiguousarray(exact[..., 6:]), np.ascontiguousarray(ref[..., 6:]))
    sizes = np.concatenate(sizes)
    assert (sizes == 0.02).mean() > 0.05 and (np.log(sizes) > np.log(0.05)).mean() > 0.05          # below and above log 0.02


# ------------------------------------------------------------------------------------------------------------------ 6. backward
def _grad_run(m, feats, xyz, text, mask, loss, need=None, double=()):
    """One differentiable forward + backward.  ``loss``: 'sum' (``feats.sum() + query.sum()``: both incoming gradients have stride 0),
    'query' (``query.sum()`` alone: no gradient of the padded features at all) or 'weighted'.  ``need[b]``: does leaf b require grad; ``double``: the leaves handed over as float64.  Returns the leaves' gradients, the
    host backward on the device's indices, and the indices."""
    gm = copy.deepcopy(m).to(su.DEV)
    gm.differentiable = True
    need = need or (True,) * len(feats)
    leaves = [su.dev(f.astype(np.float64) if b in double else f, grad=need[b]) for b, f in enumerate(feats)]
    keep = {}
    dec, _ = gm(leaves, None, [su.dev(p) for p in xyz], su.dev(text), su.dev(mask), keep_out=keep)
    assert dec["query"].requires_grad and dec["feats"].requires_grad and dec["feats"].dtype == torch.float32
    if loss == "sum":
        G1, G2 = np.ones(tuple(dec["feats"].shape), np.float32), np.ones(tuple(dec["query"].shape), np.float32)
        (dec["feats"].sum() + dec["query"].sum()).backward()
    elif loss == "query":
        G1, G2 = None, np.ones(tuple(dec["query"].shape), np.float32)
        dec["query"].sum().backward()
    else:
        rng = np.random.default_rng(61)
        G1, G2 = normal(rng, *dec["feats"].shape), normal(rng, *dec["query"].shape)
        ((dec["feats"] * su.dev(G1)).sum() + (dec["query"] * su.dev(G2)).sum()).backward()
    index = host(keep["index"])
    return [l.grad for l in leaves], qh.backward_host(G1, G2, index, [len(f) for f in feats]), index


def _grad_edges(C, rows, num_queries, K):
    feats, xyz, text, mask = qu.inputs(rows, 7, C, seed=4000 + C + len(rows))
    mask[1, 0] = True
    m = qu.module(C=C, num_queries=num_queries)
    for loss in ("sum", "query", "weighted"):
        grads, ref, index = _grad_run(m, feats, xyz, text, mask, loss)
        assert index.shape == (len(rows), K) and all(len(set(i.tolist())) == K for i in index)
        for g, r in zip(grads, ref):
            nu.bits(g, r)
        again, _, index2 = _grad_run(m, feats, xyz, text, mask, loss)
        assert np.array_equal(index, index2) and all(torch.equal(a, g) for a, g in zip(again, grads))
        if loss == "sum":                                    # selected rows carry 2, the others 1: the add happened exactly where it should
            for b, g in enumerate(grads):
                want = np.ones((rows[b], C), np.float32)
                want[index[b]] = 2.0
                nu.bits(g, want)
    # only the first and the last leaf require grad
    need = tuple(b in (0, len(rows) - 1) for b in range(len(rows)))
    grads, ref, _ = _grad_run(m, feats, xyz, text, mask, "weighted", need=need)
    for b, (g, r) in enumerate(zip(grads, ref)):
        if need[b]:
            nu.bits(g, r)
        else:
            assert g is None
    # a float64 leaf: a float64 gradient whose values are the fp32 host's
    last = len(rows) - 1
    grads, ref, _ = _grad_run(m, feats, xyz, text, mask, "weighted", double=(last,))
    assert grads[last].dtype == torch.float64 and np.array_equal(host(grads[last]), ref[last].astype(np.float64))
    for g, r in zip(grads[:last], ref[:last]):
        nu.bits(g, r)
    return index


@pytest.mark.parametrize("C", [64, 192, 512])
def test_gradient_at_the_widths_and_doors_of_the_backward(C):
    index = _grad_edges(C, (65, 1, 130), 5, 1)
    assert index.shape == (3, 1)


def test_gradient_with_every_row_selected():
    index = _grad_edges(64, (40, 40), 40, 40)
    assert all(sorted(i.tolist()) == list(range(40)) for i in index)


# ------------------------------------------------------------------------------------------------------------------ 7. the module's doors
DOOR_ROWS, DOOR_T, DOOR_C, DOOR_K = (70, 9, 33), 9, 128, 8
NUMERIC = ("query", "feats", "feats_attention_mask", "query_coords", "feats_coords", "pred_bboxes", "text_attention_mask")


def _door_inputs(seed=5000):
    feats, xyz, text, mask = qu.inputs(DOOR_ROWS, DOOR_T, DOOR_C, seed=seed)
    mask[1, :4] = True
    return feats, xyz, text, mask


def _door_run(gm, feats, xyz, text, mask):
    """The module on device tensors as they are handed in: every numeric output, the score and the index, as numpy arrays."""
    keep = {}
    with torch.no_grad():
        dec, head = gm(feats, None, xyz, text, mask, keep_out=keep)
    assert dec["text_feats"] is text and head["text_token_mask"] is mask
    out = {k: host(dec[k]) for k in NUMERIC}
    out.update(score=host(keep["score"]), index=host(keep["index"]))
    assert out["index"].shape == (len(feats), DOOR_K) and out["query"].dtype == np.float32 and out["feats_attention_mask"].dtype == bool
    return out


def _same_outputs(got, want):
    assert list(got) == list(want)
    for k in want:
        nu.bits(got[k], want[k])


def test_the_modules_doors():
    feats, xyz, text, mask = _door_inputs()
    B, T, C = len(feats), DOOR_T, DOOR_C
    gm = qu.module(C=C, num_queries=DOOR_K).to(su.DEV)
    df, dx = _dev_lists(feats, xyz)
    dtext, dmask = su.dev(text), su.dev(mask)
    want = _door_run(gm, df, dx, dtext, dmask)
    assert np.array_equal(want["index"], qh.topk_sorted_host(want["score"], DOOR_ROWS, DOOR_K)) and np.isfinite(want["score"][1, :9]).all()
    # the token mask as uint8, as int64, and as the first T columns of a (B, 256) tokenizer mask
    _same_outputs(_door_run(gm, df, dx, dtext, dmask.to(torch.uint8)), want)
    _same_outputs(_door_run(gm, df, dx, dtext, dmask.to(torch.int64)), want)
    big = torch.ones((B, 256), dtype=torch.bool, device=su.DEV)
    big[:, :T] = dmask
    assert not big[:, :T].is_contiguous()
    _same_outputs(_door_run(gm, df, dx, dtext, big[:, :T]), want)
    # text_feats as the first C channels of a (B, T, 2C) tensor
    rng = np.random.default_rng(5001)
    wide = su.dev(np.concatenate([text, normal(rng, B, T, C)], axis=2))[:, :, :C]
    assert not wide.is_contiguous()
    _same_outputs(_door_run(gm, df, dx, wide, dmask), want)
    # the scenes as row slices of one concatenated buffer
    ends = np.cumsum((0,) + DOOR_ROWS)
    all_f, all_x = su.dev(np.concatenate(feats)), su.dev(np.concatenate(xyz))
    slices = lambda t: [t[lo:hi] for lo, hi in zip(ends[:-1], ends[1:])]      # noqa: E731
    assert slices(all_f)[1].data_ptr() != df[1].data_ptr() and slices(all_f)[1].storage_offset() == 70 * C
    _same_outputs(_door_run(gm, slices(all_f), slices(all_x), dtext, dmask), want)
    # float64 and fp16 features: the plain call on the same values rounded to fp32
    f64s = [f.astype(np.float64) * (1.0 + 2.0 ** -30) for f in feats]
    x64s = [p.astype(np.float64) * (1.0 + 2.0 ** -30) for p in xyz]
    assert any((f.astype(np.float32) != f).any() for f in f64s)
    plain = _door_run(gm, [su.dev(f.astype(np.float32)) for f in f64s], [su.dev(p.astype(np.float32)) for p in x64s], dtext, dmask)
    _same_outputs(_door_run(gm, [su.dev(f) for f in f64s], [su.dev(p) for p in x64s], dtext, dmask), plain)
    f16s, x16s = [f.astype(np.float16) for f in feats], [p.astype(np.float16) for p in xyz]
    plain = _door_run(gm, [su.dev(f.astype(np.float32)) for f in f16s], [su.dev(p.astype(np.float32)) for p in x16s], dtext, dmask)
    assert not np.array_equal(plain["score"], want["score"])
    _same_outputs(_door_run(gm, [su.dev(f) for f in f16s], [su.dev(p) for p in x16s], dtext, dmask), plain)


def _hold_on_the_devices_rows(name, m, got, feats, xyz, text, mask):
    """The device's indices by the host rule on the device's scores; every output against the hosts on those indices."""
    index = got["index"]
    assert np.array_equal(index, qh.topk_sorted_host(got["score"], DOOR_ROWS, DOOR_K))
    h32, h64 = {}, {}
    d32, _ = m.forward_host(feats, None, xyz, text, mask, np.float32, index=index, keep_out=h32)
    d64, _ = m.forward_host(feats, None, xyz, text, mask, np.float64, index=index, keep_out=h64)
    for k in ("query", "feats", "query_coords", "feats_coords"):
        nu.bits(got[k], d32[k])
    assert np.array_equal(got["feats_attention_mask"], d64["feats_attention_mask"]) and np.array_equal(got["text_attention_mask"], ~mask)
    su.hold(f"{name} pred_bboxes", got["pred_bboxes"], d32["pred_bboxes"], d64["pred_bboxes"])
    return h32["score"], h64["score"]


@pytest.mark.parametrize("kw", [dict(bias=False, log_scale=None), dict(num_reg_fcs=0)], ids=["unscaled-no-bias", "no-hidden-layer"])
def test_the_modules_other_configurations(kw):
    feats, xyz, text, mask = _door_inputs(5100)
    m = qu.module(C=DOOR_C, num_queries=DOOR_K, **kw)
    got = _door_run(copy.deepcopy(m).to(su.DEV), *_dev_lists(feats, xyz), su.dev(text), su.dev(mask))
    s32, s64 = _hold_on_the_devices_rows(f"module {kw}", m, got, feats, xyz, text, mask)
    _hold_finite(f"module {kw} score", got["score"], s32, s64)


def test_a_module_whose_every_scene_has_no_token():
    """Every score is ``-inf``: one tie throughout, the rows 0 .. K - 1 in order."""
    feats, xyz, text, _ = _door_inputs(5200)
    mask = np.zeros((3, DOOR_T), bool)
    m = qu.module(C=DOOR_C, num_queries=DOOR_K)
    got = _door_run(copy.deepcopy(m).to(su.DEV), *_dev_lists(feats, xyz), su.dev(text), su.dev(mask))
    assert np.isneginf(got["score"]).all() and (got["index"] == np.arange(DOOR_K)).all()
    s32, s64 = _hold_on_the_devices_rows("module without a token", m, got, feats, xyz, text, mask)
    assert np.isneginf(s32).all() and np.isneginf(s64).all()


def test_a_scene_alone_has_the_bits_it_has_in_the_batch():
    """Scene 1 has 9 rows and ``num_queries = 8``: K = 8 alone and in the batch."""
    feats, xyz, text, mask = _door_inputs(5300)
    gm = qu.module(C=DOOR_C, num_queries=DOOR_K).to(su.DEV)
    batch = _door_run(gm, *_dev_lists(feats, xyz), su.dev(text), su.dev(mask))
    alone = _door_run(gm, [su.dev(feats[1])], [su.dev(xyz[1])], su.dev(text[1:2]), su.dev(mask[1:2]))
    assert np.array_equal(alone["index"][0], batch["index"][1]) and alone["feats"].shape == (1, 9, DOOR_C)
    for k in ("query", "query_coords", "pred_bboxes"):
        nu.bits(alone[k][0], np.ascontiguousarray(batch[k][1]))
    nu.bits(alone["feats"][0], np.ascontiguousarray(batch["feats"][1, :9]))
    nu.bits(alone["score"][0], np.ascontiguousarray(batch["score"][1, :9]))
