"""The transformer decoder's kernels (csrc/decoder.hip, proxytransformation_amd/decoder.py) at the edges tests/test_gpu_decoder.py does not
reach, each at the smallest shape that takes the path.  References: the numpy restatements of ``decoder_host.py`` and
``query_select_host.boxes_host`` in float32 and float64; bit for bit where the arithmetic is exact, ``sparse_util.hold`` (8 x the fp32
host's error against float64) where it sums, ``_hold_finite`` where a result has ``-inf`` entries.

layer_norm  C = 64 .. 512 in steps of 64 (the mean is inexact where C is no power of two) on 1, 15, 16, 17, 257 rows (16 rows per
            work-group): one and two outputs, ``out2`` as a slot of a larger tensor, a constant row (the bias, bit for bit), a NaN / +inf
            element (its row NaN, the others untouched), ``eps = 1e-3`` on rows of variance 1e-4, two norms of different eps refused.
boxes       C in 64, 192, 320, 512 on (1, n) rows, n in 1, 15, 16, 17, 257, and (3, 7): sizes on both sides of the clamp, ``bias=None``,
            ``out=`` as a slot, integer operands bit for bit, a NaN row, a NaN coordinate.
attention   (Kq, L) at the tile edges -- (64, 1), (63, 63), (64, 64), (1024, 65), (1023, 128) -- at H = 1 and C = 512 for both head
            dimensions; key tiles masked throughout AHEAD of the first unmasked key; padding a scene changes no bit of its result;
            views the call takes as they are and views it copies; float64 operands; uint8 and strided masks.
scores      ``max_text_len`` in 1, 63, 64, 65, 100, 255 (tiles cut by the output width) at K in 1, 64, 1024 and C in 64, 512, one and
            three layers: the four (scaled, bias) pairs bit for bit, ``-inf`` exactly on masked and missing tokens, a NaN hidden row.
posembed    cin = 1 .. 9 at C in 64, 320, 512 on 1, 63, 64, 65 rows, the bare ``nn.Sequential`` head; training mode refused.
linear      2048 -> 4096 (the largest accepted); 63 and 64 rows; ``add`` with ``add_cols = 0`` and ``= Cout``; bias, ReLU and residual in
            one call: the ReLU first, then the residual.
module      two groups of hoisted key / value projections (C = 512 with 5 layers: 4 + 1, a head count per attention; C = 256 with 9
            layers: 8 + 1), the text projections hoisted (T = 5) or not (T = K = 3); a scene's result is the same bits alone and in a
            batch; weights changed after a forward (``load_state_dict``, in place, a parameter replaced) are the weights of the next
            forward; ``bbox_head`` with ``reg_branches``, single-``Linear`` branches, float64 operands with a uint8 mask."""
import functools
import types

import numpy as np
import pytest
import torch
from torch import nn

from proxytransformation_amd import decoder, decoder_host as dh, query_select_host as qh
from tests import decoder_util as du
from tests import sparse_util as su
from tests.sparse_util import hold_pooled
from tests.test_gpu_decoder import _attn_refs, _hold_finite, _hold_layers, _ln_params, bits_equal, dev, f64, host, ints

pytestmark = pytest.mark.gpu
DEV = su.DEV
EDGE_ROWS = (1, 15, 16, 17, 257)                             # k_dec_ln and k_head_boxes: 16 rows per work-group


def normal(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def both(fn, *arrays, **kw):
    """``fn`` on the fp32 arrays and on their float64 copies: ``(ref32, ref64)``."""
    r32 = fn(*arrays, **kw)
    assert (r32[0] if isinstance(r32, tuple) else r32).dtype == np.float32
    return r32, fn(*[f64(a) if a is not None and a.dtype == np.float32 else a for a in arrays], **kw)


def same_rows_but(a, b, row):
    """Every row of ``a (n,C)`` but ``row`` has the bits of ``b``'s."""
    keep = np.arange(len(a)) != row
    return bits_equal(np.ascontiguousarray(a[keep]), np.ascontiguousarray(b[keep]))


# ------------------------------------------------------------------------------------------------------------------ 1. layer_norm
def _ln_host2(x, w, b, w2, b2, eps=dh.LN_EPS):
    first = dh.layer_norm_host(x, w, b, eps)
    return first, dh.layer_norm_host(first, w2, b2, eps)


@pytest.mark.parametrize("C", list(range(64, 513, 64)))
def test_layer_norm_alone(C):
    rng = np.random.default_rng(1000 + C)
    ln, ln2 = _ln_params(rng, C), _ln_params(rng, C)
    dln, dln2 = tuple(dev(t) for t in ln), tuple(dev(t) for t in ln2)
    for n in EDGE_ROWS:
        x = (3 * normal(rng, n, C) + 2).astype(np.float32)
        one = host(decoder.layer_norm(dev(x), dln))
        got, got2 = (host(t) for t in decoder.layer_norm(dev(x), dln, dln2))
        assert bits_equal(one, got)
        (r32, r32b), (r64, r64b) = both(_ln_host2, x, *ln, *ln2)
        su.hold(f"layer_norm C={C} n={n}", got, r32, r64)
        su.hold(f"layer_norm C={C} n={n} second norm", got2, r32b, r64b)
        # out2: a layer's slot of a larger tensor; its neighbours keep their bits
        big = torch.full((3, n, C), 7.0, dtype=torch.float32, device=DEV)
        a, b = decoder.layer_norm(dev(x), dln, dln2, out2=big[1])
        assert b.data_ptr() == big[1].data_ptr() and bits_equal(host(a), got)
        big = host(big)
        assert bits_equal(big[1], got2) and bits_equal(big[0], np.full((n, C), 7.0, np.float32)) and bits_equal(big[2], big[0])
        # a constant row: sum and mean are exact, the centred row is zero, the result is the bias
        r = n // 2
        flat = x.copy()
        flat[r] = 3.0
        out = host(decoder.layer_norm(dev(flat), dln))
        assert bits_equal(out[r], ln[1]) and same_rows_but(out, got, r)
        # one NaN or +inf element: its row is NaN in both outputs, every other row keeps its bits
        for bad in (np.nan, np.inf):
            xb = x.copy()
            xb[r, C - 3] = bad
            o1, o2 = (host(t) for t in decoder.layer_norm(dev(xb), dln, dln2))
            assert np.isnan(o1[r]).all() and np.isnan(o2[r]).all() and np.isnan(o1).sum() == C == np.isnan(o2).sum(), (n, bad)
            assert same_rows_but(o1, got, r) and same_rows_but(o2, got2, r), (n, bad)
    # eps: rows of variance 1e-4 under eps = 1e-3 -- a dropped or default eps shows
    x = (0.01 * normal(rng, 17, C)).astype(np.float32)
    got, got2 = (host(t) for t in decoder.layer_norm(dev(x), dln + (1e-3,), dln2 + (1e-3,)))
    (r32, r32b), (r64, r64b) = both(_ln_host2, x, *ln, *ln2, eps=1e-3)
    su.hold(f"layer_norm C={C} eps=1e-3", got, r32, r64)
    su.hold(f"layer_norm C={C} eps=1e-3 second norm", got2, r32b, r64b)
    assert su.rel(dh.layer_norm_host(f64(x), f64(ln[0]), f64(ln[1])), r64) > 0.1          # the default eps is another result
    assert bits_equal(host(decoder.layer_norm(dev(x), dln + (1e-3,))), got)
    with pytest.raises(ValueError, match="share eps"):
        decoder.layer_norm(dev(x), dln + (1e-3,), dln2)


# ------------------------------------------------------------------------------------------------------------------ 2. boxes
def _box_refs(h, w, b, coords):
    r32 = qh.boxes_host(h, coords, [w], [np.zeros(9, np.float32) if b is None else b])
    assert r32.dtype == np.float32
    return r32, qh.boxes_host(f64(h), f64(coords), [f64(w)], [np.zeros(9) if b is None else f64(b)])


@pytest.mark.parametrize("C", [64, 192, 320, 512])
def test_boxes_alone(C):
    rng = np.random.default_rng(2000 + C)
    w = (normal(rng, 9, C) * (2.0 / C) ** 0.5).astype(np.float32)
    b = (normal(rng, 9) * 0.5).astype(np.float32)
    b[3:6] -= np.float32(3.9)                                # the log-sizes centred on log 0.02, as decoder_util.reg_branches
    sizes = []
    for shape in [(1, n) for n in EDGE_ROWS] + [(3, 7)]:
        draw = lambda: (normal(rng, *shape, C), (rng.integers(-500, 500, shape + (3,)) * 0.01).astype(np.float32))      # noqa: E731
        size = 9 * int(np.prod(shape))
        (h, coords), got = hold_pooled(f"boxes C={C} rows={shape}", size, draw, lambda h, c: host(decoder.boxes(dev(h), dev(w), dev(b), dev(c))),
                                       lambda h, c: _box_refs(h, w, b, c))
        assert got.shape == shape + (9,)
        r32, r64 = _box_refs(h, w, b, coords)
        small = (r64[..., 3:6] == 0.02) & (r32[..., 3:6] == np.float32(0.02))
        assert (got[..., 3:6][small] == np.float32(0.02)).all()
        sizes.append(r64[..., 3:6].ravel())
        # without a bias
        hold_pooled(f"boxes C={C} rows={shape} bias=None", size, draw, lambda h, c: host(decoder.boxes(dev(h), dev(w), None, dev(c))),
                    lambda h, c: _box_refs(h, w, None, c))
        # out: a layer's slot of a larger tensor
        big = torch.full((3,) + shape + (9,), -5.0, dtype=torch.float32, device=DEV)
        ret = decoder.boxes(dev(h), dev(w), dev(b), dev(coords), out=big[1])
        assert ret.data_ptr() == big[1].data_ptr()
        big = host(big)
        assert bits_equal(big[1], got) and bits_equal(big[0], np.full(shape + (9,), -5.0, np.float32)) and bits_equal(big[2], big[0])
        # integer-valued operands: centre and euler bit for bit
        hi, wi, bi = ints(rng, *shape, C, lo=-2, hi=3), ints(rng, 9, C, lo=-2, hi=3), ints(rng, 9)
        ci = ints(rng, *shape, 3, lo=-9, hi=10)
        exact = host(decoder.boxes(dev(hi), dev(wi), dev(bi), dev(ci)))
        ref = qh.boxes_host(hi, ci, [wi], [bi])
        assert bits_equal(np.ascontiguousarray(exact[..., :3]), np.ascontiguousarray(ref[..., :3]))
        assert bits_equal(np.ascontiguousarray(exact[..., 6:]), np.ascontiguousarray(ref[..., 6:]))
        # a NaN in h[r]: the nine values of that row are NaN (the clamp keeps it); a NaN coordinate: that centre value only
        r = tuple(s // 2 for s in shape)
        hb = h.copy()
        hb[r + (C - 2,)] = np.nan
        out = host(decoder.boxes(dev(hb), dev(w), dev(b), dev(coords)))
        assert np.isnan(out[r]).all() and np.isnan(out).sum() == 9
        out[r] = got[r]
        assert bits_equal(out, got)
        cb = coords.copy()
        cb[r + (1,)] = np.nan
        out = host(decoder.boxes(dev(h), dev(w), dev(b), dev(cb)))
        assert np.isnan(out[r + (1,)]) and np.isnan(out).sum() == 1
        out[r + (1,)] = got[r + (1,)]
        assert bits_equal(out, got)
    sizes = np.concatenate(sizes)
    assert (sizes == 0.02).mean() > 0.05 and (np.log(sizes) > np.log(0.05)).mean() > 0.05          # below and above log 0.02


# ------------------------------------------------------------------------------------------------------------------ 3. attention
def _attn_twice(q, k, v, mask, H):
    a, b = (host(decoder.attention(dev(q), dev(k), dev(v), None if mask is None else dev(mask), H)) for _ in range(2))
    assert bits_equal(a, b)
    return a


@pytest.mark.parametrize("H,hd", [(1, 32), (1, 64), (16, 32), (8, 64)])
@pytest.mark.parametrize("Kq,L", [(64, 1), (63, 63), (64, 64), (1024, 65), (1023, 128)])
def test_attention_lengths_at_the_tile_edges(Kq, L, H, hd):
    C, B = H * hd, 2
    rng = np.random.default_rng(3000 + Kq * 3 + L * 5 + C + hd)
    q, k, v = normal(rng, B, Kq, C), normal(rng, B, L, C), normal(rng, B, L, C)
    zeros = np.zeros((B, L), bool)
    got = _attn_twice(q, k, v, None, H)
    su.hold(f"attention Kq={Kq} L={L} H={H} hd={hd}", got, *_attn_refs(q, k, v, zeros, H))
    if L == 1:                                               # one key: its value, whatever the logit
        assert bits_equal(got, np.ascontiguousarray(np.broadcast_to(v, got.shape)))
    mask = zeros.copy()
    mask[1, L // 3] = True                                   # at L = 1: scene 1 has no key left
    if L > 1:
        mask[0, [0, L // 2, L - 1]] = True
    got = _attn_twice(q, k, v, mask, H)
    su.hold(f"attention Kq={Kq} L={L} H={H} hd={hd}, single keys masked", got, *_attn_refs(q, k, v, mask, H))
    if L == 1:
        assert not got[1].any() and bits_equal(got[0], np.ascontiguousarray(np.broadcast_to(v[0], got[0].shape)))


@pytest.mark.parametrize("hd", [32, 64])
def test_attention_leading_key_tiles_masked_throughout(hd):
    """The first arithmetic of a work-group happens on tile 1, 2 or 3 with the running maximum still at ``-inf``."""
    H, L, Kq = 2, 200, 65
    rng = np.random.default_rng(3100 + hd)
    q, k, v = normal(rng, 3, Kq, H * hd), normal(rng, 3, L, H * hd), normal(rng, 3, L, H * hd)
    mask = np.zeros((3, L), bool)
    mask[0, :64], mask[1, :128], mask[2, :192] = True, True, True
    got = _attn_twice(q, k, v, mask, H)
    su.hold(f"attention hd={hd}, leading tiles masked", got, *_attn_refs(q, k, v, mask, H))
    k2, v2 = k.copy(), v.copy()
    k2[0, 5, 1], v2[0, 63, 2], k2[1, 64, 0], v2[1, 127, hd], k2[2, 191, 3], v2[2, 0, 0] = np.nan, np.inf, np.inf, np.nan, np.nan, -np.inf
    assert bits_equal(_attn_twice(q, k2, v2, mask, H), got)


@pytest.mark.parametrize("hd", [32, 64])
def test_attention_padding_a_scene_changes_no_bit(hd):
    """A masked key and a key behind ``L`` both stage zeros and both leave the ballot; a tile masked throughout is skipped: the scene
    alone, its keys cut to its own length, gives the bits it has in the padded batch."""
    H, Kq, rows = 2, 65, (65, 1, 257)
    rng = np.random.default_rng(3200 + hd)
    q, k, v = normal(rng, 3, Kq, H * hd), normal(rng, 3, 257, H * hd), normal(rng, 3, 257, H * hd)
    mask = np.stack([np.arange(257) >= n for n in rows])
    batch = _attn_twice(q, k, v, mask, H)
    su.hold(f"attention hd={hd}, padded batch", batch, *_attn_refs(q, k, v, mask, H))
    for b, n in enumerate(rows):
        alone = _attn_twice(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], None, H)
        assert bits_equal(alone[0], batch[b]), (b, n)


def test_attention_views_taken_as_they_are_and_views_copied():
    H, hd, B, Kq, L = 2, 32, 2, 65, 130
    C = H * hd
    rng = np.random.default_rng(3300)
    q, k, v = normal(rng, B, Kq, C), normal(rng, B, L, C), normal(rng, B, L, C)
    mask = np.zeros((B, L), bool)
    mask[0, [0, 70]], mask[1, 100:] = True, True
    want = _attn_twice(q, k, v, mask, H)
    dq, dk, dv, dm = dev(q), dev(k), dev(v), dev(mask)
    run = lambda q_=dq, k_=dk, v_=dv, m_=dm: host(decoder.attention(q_, k_, v_, m_, H))      # noqa: E731
    assert bits_equal(run(), want)
    wide = dev(np.concatenate([q, normal(rng, B, Kq, 2 * C)], axis=2))[:, :, :C]              # a view with ldq = 3C, taken as it is
    assert decoder._rows_view("attention", wide, wide.device)[0].data_ptr() == wide.data_ptr()
    assert decoder._rows_view("attention", wide, wide.device)[1] == 3 * C and bits_equal(run(q_=wide), want)
    off = dev(np.concatenate([normal(rng, B, Kq, 1), q, normal(rng, B, Kq, 3)], axis=2))[:, :, 1:C + 1]      # misaligned: copied
    copied = decoder._rows_view("attention", off, off.device)
    assert copied[0].data_ptr() != off.data_ptr() and copied[1] == C and bits_equal(run(q_=off), want)
    longer_k = dev(np.concatenate([k, normal(rng, B, 7, C)], axis=1))[:, :L]                  # the scene stride is not L rows: copied
    longer_v = dev(np.concatenate([v, normal(rng, B, 7, C)], axis=1))[:, :L]
    assert decoder._rows_view("attention", longer_k, longer_k.device)[0].data_ptr() != longer_k.data_ptr()
    assert bits_equal(run(k_=longer_k, v_=longer_v), want)
    spread = lambda a: dev(np.stack([a, normal(rng, *a.shape)], axis=-1).reshape(a.shape[:-1] + (2 * a.shape[-1],)))[:, :, ::2]      # noqa: E731
    sq, sk, sv = spread(q), spread(k), spread(v)                                              # a last stride of 2
    assert sq.stride(2) == 2 and bits_equal(run(q_=sq, k_=sk, v_=sv), want)
    assert bits_equal(run(q_=dq.double(), k_=dk.double(), v_=dv.double()), want)
    assert bits_equal(run(m_=dm.to(torch.uint8)), want)
    every_other = dev(np.stack([mask, ~mask], axis=-1).reshape(B, 2 * L))[:, ::2]
    assert not every_other.is_contiguous() and bits_equal(run(m_=every_other), want)


# ------------------------------------------------------------------------------------------------------------------ 4. scores
@pytest.mark.parametrize("K,C", [(1, 64), (64, 512), (1024, 64)])
@pytest.mark.parametrize("M,T", [(1, 1), (63, 63), (64, 1), (65, 65), (100, 77), (255, 200)])
def test_contrastive_scores_on_output_widths_that_cut_a_tile(M, T, K, C):
    B = 2
    rng = np.random.default_rng(4000 + M * 7 + T + K + C)
    tok = np.ones((B, T), bool)
    tok[1] = rng.random(T) < 0.6                             # one scene's tokens partly masked
    tok[1, T // 2] = False
    gone = np.ones((B, M), bool)
    gone[:, :T] = ~tok
    bias = np.array([-4.5], np.float32)
    for NL in (1, 3):
        hs, text = ints(rng, NL, B, K, C), ints(rng, B, T, C)
        clean = {}
        for scaled in (True, False):
            for b in (bias, None):
                got = host(decoder.contrastive_scores(dev(hs), dev(text), dev(tok), None if b is None else dev(b), scaled, M))
                assert got.shape == (NL, B, K, M)
                assert bits_equal(got, dh.contrastive_scores_host(hs, text, tok, b, scaled, M)), (NL, scaled, b is None)
                by_token = got.transpose(0, 2, 1, 3)
                assert np.isneginf(by_token[:, :, gone]).all() and np.isfinite(by_token[:, :, ~gone]).all()
                clean[scaled, b is None] = got
        draw = lambda: (normal(rng, NL, B, K, C), normal(rng, B, T, C))      # noqa: E731
        for scaled, b in ((True, None), (False, bias)):
            hold_pooled(f"contrastive_scores M={M} T={T} K={K} C={C} NL={NL} scaled={scaled} bias={b is not None}", NL * K * int(tok.sum()), draw,
                        lambda x, t: host(decoder.contrastive_scores(dev(x), dev(t), dev(tok), None if b is None else dev(b), scaled, M)),
                        lambda x, t: (dh.contrastive_scores_host(x, t, tok, b, scaled, M),
                                      dh.contrastive_scores_host(f64(x), f64(t), tok, f64(b), scaled, M)), rule=_hold_finite)
        # a NaN in one hidden row: NaN on that layer's, scene's and row's tokens, its -inf entries stay, nothing else moves
        l, s, r = NL - 1, 0, K // 2
        bad = hs.copy()
        bad[l, s, r, C - 1] = np.nan
        out = host(decoder.contrastive_scores(dev(bad), dev(text), dev(tok), dev(bias), True, M))
        assert np.isnan(out[l, s, r, ~gone[s]]).all() and np.isneginf(out[l, s, r, gone[s]]).all() and np.isnan(out).sum() == (~gone[s]).sum()
        out[l, s, r] = clean[True, False][l, s, r]
        assert bits_equal(out, clean[True, False])


# ------------------------------------------------------------------------------------------------------------------ 5. posembed
def _pos_head(cin, C, seed):
    """The bare head of a ``PositionEmbeddingLearned`` in eval, running statistics off their initial values."""
    rng = np.random.default_rng(seed)
    put = lambda t, a: t.copy_(torch.from_numpy(np.asarray(a, np.float32)).reshape(t.shape))      # noqa: E731
    head = nn.Sequential(nn.Conv1d(cin, C, 1), nn.BatchNorm1d(C), nn.ReLU(), nn.Conv1d(C, C, 1))
    with torch.no_grad():
        put(head[0].weight, rng.standard_normal((C, cin)) / cin ** 0.5)
        put(head[3].weight, rng.standard_normal((C, C)) / C ** 0.5)
        for t in (head[0].bias, head[3].bias, head[1].bias, head[1].running_mean):
            put(t, rng.standard_normal(C) * 0.1)
        for t in (head[1].weight, head[1].running_var):
            put(t, rng.uniform(0.5, 1.5, C))
    return head.eval()


def _pos_head_refs(h, x):
    a = lambda t: t.detach().cpu().double().numpy()          # noqa: E731
    w1, b1 = dh.fold_posembed(a(h[0].weight), a(h[0].bias), a(h[1].weight), a(h[1].bias), a(h[1].running_mean), a(h[1].running_var), h[1].eps)
    w2, b2 = a(h[3].weight), a(h[3].bias)
    r32 = dh.posembed_host(x, w1.astype(np.float32), b1.astype(np.float32), w2.astype(np.float32), b2.astype(np.float32))
    assert r32.dtype == np.float32
    return r32, dh.posembed_host(x.astype(np.float64), w1, b1, w2, b2)


@pytest.mark.parametrize("C", [64, 320, 512])
@pytest.mark.parametrize("cin", list(range(1, 10)))
def test_posembed_at_every_input_width(cin, C):
    head = _pos_head(cin, C, 5000 + cin * 7 + C)
    rng = np.random.default_rng(5000 + cin + C)
    for n in (1, 63, 64, 65):
        x = (3 * normal(rng, 1, n, cin)).astype(np.float32)
        got = host(decoder.posembed(dev(x), head))
        assert got.shape == (1, n, C)
        su.hold(f"posembed cin={cin} C={C} n={n}", got, *_pos_head_refs(head, x))
    head[1].train()
    with pytest.raises(NotImplementedError, match="training mode"):
        decoder.posembed(dev(x), head)


# ------------------------------------------------------------------------------------------------------------------ 6. linear
def test_linear_at_the_largest_accepted_shape():
    cin, cout, n = 2048, 4096, 65
    rng = np.random.default_rng(6000)
    x, w, b = ints(rng, 1, n, cin, lo=-2, hi=3), ints(rng, cout, cin, lo=-2, hi=3), ints(rng, cout)
    dw = dev(w)
    assert bits_equal(host(decoder.linear(dev(x), dw, dev(b))), dh.linear_host(x, w, b))
    x, b = normal(rng, 1, n, cin), normal(rng, cout)
    w = (normal(rng, cout, cin) / cin ** 0.5).astype(np.float32)
    su.hold(f"linear {cin}->{cout} n={n}", host(decoder.linear(dev(x), dev(w), dev(b))), *both(dh.linear_host, x, w, b))


@pytest.mark.parametrize("n", [63, 64])
def test_linear_on_one_row_tile_less_one_and_exactly(n):
    cin, cout = 192, 320
    rng = np.random.default_rng(6100 + n)
    x, add, w, b = ints(rng, 1, n, cin, lo=-2, hi=3), ints(rng, 1, n, cin, lo=-2, hi=3), ints(rng, cout, cin, lo=-2, hi=3), ints(rng, cout)
    dx, da, dw, db = dev(x), dev(add), dev(w), dev(b)
    plain, added = host(decoder.linear(dx, dw, db)), host(decoder.linear(dx, dw, db, add=da))
    assert bits_equal(plain, dh.linear_host(x, w, b)) and bits_equal(added, dh.linear_host(x, w, b, add=add))
    assert not bits_equal(plain, added)
    assert bits_equal(host(decoder.linear(dx, dw, db, add=da, add_cols=0)), plain)            # an add that reaches no column
    assert bits_equal(host(decoder.linear(dx, dw, db, add=da, add_cols=cout)), added)         # and one that reaches them all
    x, add, b = normal(rng, 1, n, cin), normal(rng, 1, n, cin), normal(rng, cout)
    w = (normal(rng, cout, cin) / cin ** 0.5).astype(np.float32)
    got = host(decoder.linear(dev(x), dev(w), dev(b), add=dev(add), add_cols=128, relu=True))
    su.hold(f"linear {cin}->{cout} n={n}", got, *both(dh.linear_host, x, w, b, add=add, add_cols=128, relu=True))


def test_linear_applies_the_relu_before_the_residual():
    cin, cout, n = 192, 320, 65
    rng = np.random.default_rng(6200)
    x, w, b = ints(rng, 1, n, cin, lo=-2, hi=3), ints(rng, cout, cin, lo=-2, hi=3), ints(rng, cout)
    res = ints(rng, 1, n, cout, lo=-40, hi=10)
    pre = dh.linear_host(x, w, b)
    assert (pre < 0).mean() > 0.2 and (res < 0).mean() > 0.5 and ((pre > 0) & (pre + res < 0)).mean() > 0.05
    got = host(decoder.linear(dev(x), dev(w), dev(b), relu=True, residual=dev(res)))
    assert bits_equal(got, np.maximum(pre, np.float32(0)) + res)
    assert not bits_equal(got, np.maximum(pre + res, np.float32(0)))


# ------------------------------------------------------------------------------------------------------------------ 7. the module
@functools.lru_cache(maxsize=None)
def _group_case(which, T):
    """The module with two groups of hoisted projections, its branches, operands and both host chains, computed once."""
    cfg = dict(wide=du.WIDE, deep=du.DEEP)[which]
    m, br = du.module(**cfg), du.reg_branches(cfg["C"], cfg["layers"])
    ops = du.group_operands(cfg["C"], T, 7000 + T)
    return m, br, ops, du.host(m, ops, br, np.float32), du.host(m, ops, br, np.float64)


@pytest.mark.parametrize("T", [5, 3])
@pytest.mark.parametrize("which", ["wide", "deep"])
def test_module_with_two_groups_of_hoisted_projections(which, T):
    """``wide``: C = 512, heads (self 8, text 16, scene 8), 5 layers in groups of 4 + 1; ``deep``: C = 256, 9 layers in groups of 8 + 1.
    At T = 5 the text keys and values are hoisted too; at T = K = 3 they take ``query_pos`` per layer."""
    m, br, ops, r32, r64 = _group_case(which, T)
    m, br = m.to(DEV), br.to(DEV)
    got = du.device(m, ops, br)
    assert [len(g["ids"]) for g in m._prepared["groups"]] == ([4, 1] if which == "wide" else [8, 1])
    _hold_layers(f"{which} module T={T}", got, r32, r64)


def _scenes_alone_have_the_bits_of_the_batch(m, br, ops):
    hidden, boxes = (host(t) for t in du.device(m, ops, br))
    for b in range(hidden.shape[1]):
        h1, b1 = (host(t) for t in du.device(m, du.scene_alone(ops, b), br))
        assert bits_equal(h1[:, 0], np.ascontiguousarray(hidden[:, b])) and bits_equal(b1[:, 0], np.ascontiguousarray(boxes[:, b])), b


def test_a_scenes_result_does_not_depend_on_its_batch():
    """Each scene alone, its keys cut to its own length, against its rows of the batch, bit for bit; T != K in both runs."""
    m, br = du.module(**du.SMALL).to(DEV), du.reg_branches(64, 2).to(DEV)
    tm = np.zeros((3, 5), bool)
    tm[1, :3] = True
    _scenes_alone_have_the_bits_of_the_batch(m, br, du.operands((65, 1, 257), 7, 5, 64, 71, tm))
    m, br, ops, _, _ = _group_case("wide", 5)
    _scenes_alone_have_the_bits_of_the_batch(m.to(DEV), br.to(DEV), ops)


def test_weights_changed_after_a_forward_are_the_weights_of_the_next():
    br = du.reg_branches(64, 2).to(DEV)
    tm = np.zeros((3, 5), bool)
    tm[2, 4] = True
    ops = du.operands((65, 1, 257), 7, 5, 64, 72, tm)
    run = lambda mod: tuple(host(t) for t in du.device(mod, ops, br))      # noqa: E731
    same = lambda a, b: bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])      # noqa: E731
    m = du.module(**du.SMALL).to(DEV)
    first = run(m)
    fresh = du.module(**du.SMALL, seed=5)
    m.load_state_dict(fresh.state_dict())
    second = run(m)
    assert not same(second, first) and same(second, run(fresh.to(DEV)))
    changes = (lambda mod: mod.layers[1].cross_attn.attn.in_proj_weight.mul_(1.5),
               lambda mod: mod.cross_posembed.position_embedding_head[1].running_var.mul_(3.0))
    last = second
    for change in changes:                                   # in place under no_grad: the version moves
        with torch.no_grad():
            change(m), change(fresh)
        fresh._prepared = None
        now = run(m)
        assert not same(now, last) and same(now, run(fresh))
        last = now
    # a parameter replaced by a new one of the same version
    attn = m.layers[0].cross_attn.attn
    old = attn.in_proj_weight
    new = nn.Parameter(old.detach().clone() * 0.5)
    with torch.no_grad():
        while new._version < old._version:
            new.add_(0.0)
        fresh.layers[0].cross_attn.attn.in_proj_weight.mul_(0.5)
    assert new._version == old._version
    attn.in_proj_weight = new
    fresh._prepared = None
    now = run(m)
    assert not same(now, last) and same(now, run(fresh))


def test_the_modules_other_doors():
    m = du.module(**du.SMALL).to(DEV)
    br = du.reg_branches(64, 2).to(DEV)
    tm = np.zeros((3, 5), bool)
    tm[0, 1] = True
    ops = du.operands((65, 1, 257), 7, 5, 64, 73, tm)
    want = tuple(host(t) for t in du.device(m, ops, list(br)))
    got = tuple(host(t) for t in du.device(m, ops, types.SimpleNamespace(reg_branches=br)))          # a head with reg_branches
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])
    # float64 operands and a uint8 padding mask
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in ops.items()}
    t = {k: v.double() if v.is_floating_point() else v.to(torch.uint8) for k, v in t.items()}
    got = m(t["query"], t["key"], t["key"], t["key_padding_mask"], None, None, t["query_coords"], t["key_coords"], t["pred_bboxes"],
            t["text_feats"], t["text_attention_mask"], br)
    assert got[0].dtype == torch.float32 and bits_equal(host(got[0]), want[0]) and bits_equal(host(got[1]), want[1])
    # regression branches of a single Linear
    rng = np.random.default_rng(74)
    single = nn.ModuleList([nn.Linear(64, 9) for _ in range(2)])
    with torch.no_grad():
        for lin in single:
            lin.weight.copy_(torch.from_numpy(normal(rng, 9, 64) * np.float32((2.0 / 64) ** 0.5)))
            lin.bias.copy_(torch.from_numpy(normal(rng, 9) * np.float32(0.5)))
    _hold_layers("single Linear branches", du.device(m, ops, single.to(DEV)), du.host(m, ops, single, np.float32), du.host(m, ops, single, np.float64))
