"""The transformer decoder behind the query selection on the device (proxytransformation_amd/decoder.py, csrc/decoder.hip) against its
numpy specification (decoder_host.py): every operator at its edges -- integer-valued operands bit for bit against the fp32 host, N(0, 1)
operands by ``sparse_util.hold`` (the device error against float64 is at most 8 times the fp32 host's) --, the small whole module, and the
end-to-end case behind ``QuerySelect`` at C = 256, 8 heads, FFN 2048, 6 layers."""
import contextlib

import numpy as np
import pytest
import torch

from proxytransformation_amd import decoder, decoder_host as dh
from tests import decoder_util as du
from tests import query_select_util as qu
from tests import sparse_util as su

pytestmark = pytest.mark.gpu
DEV = su.DEV
ROWS = (1, 65, 257)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ints(rng, *shape, lo=-4, hi=5):
    return rng.integers(lo, hi, shape).astype(np.float32)


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


@contextlib.contextmanager
def count_synchronises():
    """The Python-level synchronise entry points, counted the way tests/test_gpu_pipeline.py counts them."""
    calls = []
    saved = (torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize)

    def wrap(name, fn):
        def inner(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return inner

    torch.cuda.synchronize = wrap("torch.cuda.synchronize", saved[0])
    torch.cuda.Stream.synchronize = wrap("Stream.synchronize", saved[1])
    torch.cuda.Event.synchronize = wrap("Event.synchronize", saved[2])
    try:
        yield calls
    finally:
        torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize = saved


# ------------------------------------------------------------------------------------------------------------------ posembed
def _pos_refs(pe, x):
    h = pe.position_embedding_head
    a = lambda t: t.detach().cpu().double().numpy()          # noqa: E731
    w1, b1 = dh.fold_posembed(a(h[0].weight), a(h[0].bias), a(h[1].weight), a(h[1].bias), a(h[1].running_mean), a(h[1].running_var), h[1].eps)
    w2, b2 = a(h[3].weight), a(h[3].bias)
    r32 = dh.posembed_host(x, w1.astype(np.float32), b1.astype(np.float32), w2.astype(np.float32), b2.astype(np.float32))
    assert r32.dtype == np.float32
    return r32, dh.posembed_host(x.astype(np.float64), w1, b1, w2, b2)


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("cin", [3, 9])
def test_posembed_holds_and_a_nan_coordinate_stays_in_its_row(cin, C):
    m = du.module(C=C, heads=C // 32, ffn=64, layers=1, seed=30 + cin)
    pe = m.self_posembed if cin == 9 else m.cross_posembed
    rng = np.random.default_rng(cin * C)
    for n in ROWS:
        x = rng.standard_normal((2, n, cin)).astype(np.float32) * 3
        got = host(decoder.posembed(dev(x), pe))
        assert got.shape == (2, n, C)
        su.hold(f"posembed cin={cin} C={C} n={n}", got, *_pos_refs(pe, x))
    bad = x.copy()
    bad[1, 70, cin - 1] = np.nan
    out = host(decoder.posembed(dev(bad), pe))
    assert np.isnan(out[1, 70]).all() and np.isnan(out).sum() == C
    keep = np.ones(out.shape[:2], bool)
    keep[1, 70] = False
    assert bits_equal(out[keep], got[keep])


# ------------------------------------------------------------------------------------------------------------------ linear
LINEAR_SHAPES = [(64, 64), (192, 320), (256, 768), (256, 2048), (2048, 256), (256, 3072)]


@pytest.mark.parametrize("cin,cout", LINEAR_SHAPES)
def test_linear_is_the_fp32_host_bit_for_bit_on_integer_operands(cin, cout):
    rng = np.random.default_rng(cin + cout)
    w, b = ints(rng, cout, cin, lo=-2, hi=3), ints(rng, cout)
    for n in ROWS:
        x, add, res = ints(rng, 1, n, cin, lo=-2, hi=3), ints(rng, 1, n, cin, lo=-2, hi=3), ints(rng, 1, n, cout)
        for use_add, relu in ((False, False), (True, False), (False, True), (True, True)):
            got = host(decoder.linear(dev(x), dev(w), dev(b), add=dev(add) if use_add else None, relu=relu))
            assert bits_equal(got, dh.linear_host(x, w, b, add=add if use_add else None, relu=relu)), (n, use_add, relu)
        cols = (cout // 64 + 1) // 2 * 64                  # the add on the lower column tiles only: [q|k] with positions, v without
        got = host(decoder.linear(dev(x), dev(w), None, add=dev(add), add_cols=cols, residual=dev(res)))
        assert bits_equal(got, dh.linear_host(x, w, None, add=add, add_cols=cols) + res), (n, cols)


@pytest.mark.parametrize("cin,cout", [(192, 320), (2048, 256), (256, 3072)])
def test_linear_holds_on_normal_operands_and_the_relu_keeps_a_nan(cin, cout):
    rng = np.random.default_rng(cin * 3 + cout)
    x, add = rng.standard_normal((2, 65, cin)).astype(np.float32), rng.standard_normal((2, 65, cin)).astype(np.float32)
    w, b = (rng.standard_normal((cout, cin)) / cin ** 0.5).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    got = host(decoder.linear(dev(x), dev(w), dev(b), add=dev(add), relu=True))
    su.hold(f"linear {cin}->{cout}", got, dh.linear_host(x, w, b, add=add, relu=True), dh.linear_host(f64(x), f64(w), f64(b), add=f64(add), relu=True))
    x[1, 7, 5] = np.nan
    out = host(decoder.linear(dev(x), dev(w), dev(b), add=dev(add), relu=True))
    assert np.isnan(out[1, 7]).all() and np.isnan(out).sum() == cout
    out[1, 7] = got[1, 7]
    assert bits_equal(out, got)


# ------------------------------------------------------------------------------------------------------------------ linear_add_ln
def _ln_params(rng, C):
    return rng.uniform(0.5, 1.5, C).astype(np.float32), (rng.standard_normal(C) * 0.5).astype(np.float32)


@pytest.mark.parametrize("cin,C", [(64, 64), (256, 256), (2048, 256), (192, 512), (2048, 512)])
def test_linear_add_ln_holds_with_both_outputs(cin, C):
    rng = np.random.default_rng(cin + C)
    x = rng.standard_normal((257, cin)).astype(np.float32)
    w, b = (rng.standard_normal((C, cin)) / cin ** 0.5).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    res, ln, ln2 = rng.standard_normal((257, C)).astype(np.float32), _ln_params(rng, C), _ln_params(rng, C)
    one = host(decoder.linear_add_ln(dev(x), dev(w), dev(b), dev(res), tuple(dev(t) for t in ln)))
    got, got2 = (host(t) for t in decoder.linear_add_ln(dev(x), dev(w), dev(b), dev(res), tuple(dev(t) for t in ln), tuple(dev(t) for t in ln2)))
    assert bits_equal(one, got)
    r32, r32b = dh.linear_add_ln_host(x, w, b, res, ln, ln2)
    r64, r64b = dh.linear_add_ln_host(f64(x), f64(w), f64(b), f64(res), tuple(f64(t) for t in ln), tuple(f64(t) for t in ln2))
    su.hold(f"linear_add_ln {cin}->{C}", got, r32, r64)
    su.hold(f"linear_add_ln {cin}->{C} second norm", got2, r32b, r64b)


@pytest.mark.parametrize("C", [64, 256, 512])
def test_linear_add_ln_on_rows_whose_mean_is_1000_times_their_spread(C):
    """Integer-valued rows around 1000 with a spread of about 1: the sum of a row and its mean (C is a power of two) are exact in fp32,
    so the centred form loses nothing -- ``E[x^2] - E[x]^2`` would lose everything: the squares are near 1e6, the variance near 1."""
    rng = np.random.default_rng(C)
    x = ints(rng, 257, C, lo=-1, hi=2)
    w = np.eye(C, dtype=np.float32)[rng.permutation(C)] * np.where(rng.random((C, 1)) < 0.5, -1, 1).astype(np.float32)
    res = (1000 + ints(rng, 257, C, lo=-1, hi=2)).astype(np.float32)
    ln, ln2 = _ln_params(rng, C), _ln_params(rng, C)
    got, got2 = (host(t) for t in decoder.linear_add_ln(dev(x), dev(w), None, dev(res), tuple(dev(t) for t in ln), tuple(dev(t) for t in ln2)))
    y = x @ w.T + res
    assert 0.5 < float(y.std(axis=1).mean()) < 2.0 and abs(float(y.mean()) - 1000) < 1
    r32, r32b = dh.linear_add_ln_host(x, w, None, res, ln, ln2)
    r64, r64b = dh.linear_add_ln_host(f64(x), f64(w), None, f64(res), tuple(f64(t) for t in ln), tuple(f64(t) for t in ln2))
    su.hold(f"linear_add_ln off-mean C={C}", got, r32, r64)
    su.hold(f"linear_add_ln off-mean C={C} second norm", got2, r32b, r64b)


# ------------------------------------------------------------------------------------------------------------------ attention
def _attn_mask(L=257):
    """Unmasked lengths 65, 1 and 257, plus single masked keys inside a tile."""
    mask = np.stack([np.arange(L) >= n for n in (65, 1, 257)])
    mask[0, [3, 40, 64]] = True
    mask[2, [0, 130, 191, 256]] = True
    return mask


def _attn_refs(q, k, v, mask, H):
    r32 = dh.attention_host(q, k, v, mask, H)
    assert r32.dtype == np.float32
    return r32, dh.attention_host(f64(q), f64(k), f64(v), mask, H)


def _attn(q, k, v, mask, H):
    a, b = (host(decoder.attention(dev(q), dev(k), dev(v), dev(mask), H)) for _ in range(2))
    assert bits_equal(a, b)                                  # two calls, the same bits
    return a


@pytest.mark.parametrize("H,hd", [(2, 32), (8, 32), (2, 64), (8, 64)])
@pytest.mark.parametrize("Kq", [1, 65, 256])
def test_attention_holds_with_masks_inside_and_across_tiles(Kq, H, hd):
    C, L = H * hd, 257
    rng = np.random.default_rng(Kq * 7 + C)
    q, k, v = (rng.standard_normal((3, n, C)).astype(np.float32) for n in (Kq, L, L))
    mask = _attn_mask(L)
    got = _attn(q, k, v, mask, H)
    su.hold(f"attention Kq={Kq} H={H} hd={hd}", got, *_attn_refs(q, k, v, mask, H))
    # strided operands: column ranges of a wider projection output
    wide = np.concatenate([k, v, k], axis=2)
    wd = dev(wide)
    strided = host(decoder.attention(dev(q), wd[:, :, :C], wd[:, :, C:2 * C], dev(mask), H))
    assert bits_equal(strided, got)
    if Kq == 65:                                             # no mask at all is the mask of zeros
        assert bits_equal(host(decoder.attention(dev(q), dev(k), dev(v), None, H)), _attn(q, k, v, np.zeros_like(mask), H))


def test_attention_masked_scene_nan_rules_and_overflow():
    H, hd, L, Kq = 2, 32, 257, 65
    C = H * hd
    rng = np.random.default_rng(77)
    q, k, v = (rng.standard_normal((3, n, C)).astype(np.float32) for n in (Kq, L, L))
    mask = _attn_mask(L)
    mask[1] = True                                           # one scene fully masked: exact zeros
    got = _attn(q, k, v, mask, H)
    assert not got[1].any() and got[0].any() and got[2].any()
    su.hold("attention, a scene fully masked", got, *_attn_refs(q, k, v, mask, H))
    # a NaN or inf under a masked key leaves no trace
    k2, v2 = k.copy(), v.copy()
    k2[0, 40, 5], v2[0, 64, 40], k2[1, 9, 0], v2[2, 130, 3] = np.nan, np.nan, np.inf, np.nan
    assert bits_equal(_attn(q, k2, v2, mask, H), got)
    # a NaN in an unmasked value reaches its column of that scene and head (every query), a NaN in an unmasked key the whole head
    v3 = v.copy()
    v3[2, 100, hd + 2] = np.nan
    bad = _attn(q, k, v3, mask, H)
    assert np.isnan(bad[2, :, hd + 2]).all() and np.isnan(bad).sum() == Kq
    bad[2, :, hd + 2] = got[2, :, hd + 2]
    assert bits_equal(bad, got)
    k3 = k.copy()
    k3[0, 10, 1] = np.nan
    bad = _attn(q, k3, v, mask, H)
    assert np.isnan(bad[0, :, :hd]).all() and bits_equal(bad[0, :, hd:], got[0, :, hd:]) and bits_equal(bad[1:], got[1:])


def test_attention_keeps_a_running_maximum():
    """Integer-valued q and k at head dimension 64: every logit is a multiple of 1/8, exact on the device and in both hosts, so the
    yardstick stays an fp32 rounding error.  One key per scene-2 query lies at 128 = 32 * 32 / 8, the others within about +-30:
    ``expf(128)`` overflows without the running maximum.  The largest key once in the first tile and once in the last."""
    H, hd, L, Kq = 2, 64, 257, 65
    rng = np.random.default_rng(79)
    q, k = ints(rng, 3, Kq, H * hd), ints(rng, 3, L, H * hd)
    v = rng.standard_normal((3, L, H * hd)).astype(np.float32)
    mask = _attn_mask(L)
    q[:, :, 0::hd], k[:, :, 0::hd] = 32.0, 0.0
    for where in (2, 250):
        ks = k.copy()
        ks[2, where, 0::hd] = 32.0
        got = _attn(q, ks, v, mask, H)
        assert np.isfinite(got).all() and bits_equal(got[2], np.broadcast_to(v[2, where], got[2].shape).copy())
        su.hold(f"attention, overflowing logits, the largest key at {where}", got, *_attn_refs(q, ks, v, mask, H))


def test_attention_long_key_loop():
    H, hd, L, Kq = 8, 32, 3500, 64
    rng = np.random.default_rng(78)
    q, k, v = (rng.standard_normal((1, n, H * hd)).astype(np.float32) for n in (Kq, L, L))
    mask = np.zeros((1, L), bool)
    mask[0, 3460:] = True
    mask[0, 1000:1200] = True                                # three tiles masked throughout inside the loop
    got = _attn(q, k, v, mask, H)
    su.hold("attention L=3500", got, *_attn_refs(q, k, v, mask, H))


# ------------------------------------------------------------------------------------------------------------------ contrastive scores
@pytest.mark.parametrize("T", [1, 77, 256])
def test_contrastive_scores_bit_for_bit_with_inf_on_masked_and_missing_columns(T):
    rng = np.random.default_rng(T)
    NL, B, K, C = 2, 3, 65, 64
    hs, text = ints(rng, NL, B, K, C), ints(rng, B, T, C)
    tok = rng.random((B, T)) < 0.7
    tok[0, T // 2], tok[1], tok[2, 0] = False, False, True
    bias = np.array([-4.5], np.float32)
    for scaled, b in ((True, bias), (False, None)):
        got = host(decoder.contrastive_scores(dev(hs), dev(text), dev(tok), None if b is None else dev(b), scaled, 256))
        assert got.shape == (NL, B, K, 256) and bits_equal(got, dh.contrastive_scores_host(hs, text, tok, b, scaled, 256))
        gone = np.ones((B, 256), bool)
        gone[:, :T] = ~tok
        assert np.isneginf(got.transpose(0, 2, 1, 3)[:, :, gone]).all() and np.isfinite(got.transpose(0, 2, 1, 3)[:, :, ~gone]).all()
    x, t = rng.standard_normal((NL, B, K, 256)).astype(np.float32), rng.standard_normal((B, T, 256)).astype(np.float32)
    got = host(decoder.contrastive_scores(dev(x), dev(t), dev(tok), dev(bias), True, 256))
    _hold_finite(f"contrastive_scores T={T}", got, dh.contrastive_scores_host(x, t, tok, bias, True, 256),
                 dh.contrastive_scores_host(f64(x), f64(t), tok, f64(bias), True, 256))


def _hold_finite(name, got, r32, r64):
    """``hold`` on the finite entries; the ``-inf`` entries must agree exactly."""
    fin = np.isfinite(r64)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(fin, np.isfinite(r32)) and np.isneginf(got[~fin]).all()
    if fin.any():
        su.hold(name, got[fin], r32[fin], r64[fin])


# ------------------------------------------------------------------------------------------------------------------ the module
def _hold_layers(name, got, r32, r64):
    hidden, boxes = (host(t) for t in got)
    assert hidden.shape == r64[0].shape and boxes.shape == r64[1].shape and hidden.dtype == np.float32
    for lid in range(len(hidden)):
        su.hold(f"{name} hidden layer {lid}", hidden[lid], r32[0][lid], r64[0][lid])
        su.hold(f"{name} boxes layer {lid}", boxes[lid], r32[1][lid], r64[1][lid])


def test_small_module_with_text_keys_taking_the_query_positions():
    tm = np.zeros((3, 7), bool)
    tm[1, :3] = True
    m, br = du.module(**du.SMALL).to(DEV), du.reg_branches(64, 2).to(DEV)
    ops = du.operands((65, 1, 257), 7, 7, 64, 5, tm)
    got = du.device(m, ops, br)
    _hold_layers("T == K = 7", got, du.host(m, ops, br, np.float32), du.host(m, ops, br, np.float64))
    off = du.host(m, ops, br, np.float64, text_keys_take_pos=False)
    assert su.rel(host(got[0]), off[0]) > 1e-3                                    # the rule is in the device's result
    last = du.module(**du.SMALL, return_intermediate=False).to(DEV)
    q, b = du.device(last, ops, br)
    assert q.shape == (3, 7, 64) and bits_equal(host(b), host(got[1][-1]))
    normed = host(decoder.layer_norm(q, last.norm))
    assert bits_equal(normed, host(got[0][-1]))


def test_small_module_on_64_scenes_with_one_query():
    rows = tuple(range(1, 65))
    m, br = du.module(**du.SMALL).to(DEV), du.reg_branches(64, 2).to(DEV)
    tm = np.zeros((64, 9), bool)
    tm[5], tm[6, 4:] = True, True
    ops = du.operands(rows, 1, 9, 64, 8, tm)
    got = du.device(m, ops, br)
    assert got[0].shape == (2, 64, 1, 64) and got[1].shape == (2, 64, 1, 9)
    _hold_layers("B = 64, K = 1", got, du.host(m, ops, br, np.float32), du.host(m, ops, br, np.float64))


def test_empties_return_shapes_and_launch_nothing():
    m, br = du.module(**du.SMALL).to(DEV), du.reg_branches(64, 2).to(DEV)
    for rows, K in (((5, 6), 0), ((0, 0), 0)):
        ops = du.operands(rows, K, 3, 64, 1)
        hidden, boxes = du.device(m, ops, br)
        assert hidden.shape == (2, 2, K, 64) and boxes.shape == (2, 2, K, 9) and hidden.dtype == torch.float32
    last = du.module(**du.SMALL, return_intermediate=False).to(DEV)
    q, b = du.device(last, du.operands((5, 6), 0, 3, 64, 1), br)
    assert q.shape == (2, 0, 64) and b.shape == (2, 0, 9)
    s = decoder.contrastive_scores(torch.zeros(2, 2, 0, 64, device=DEV), torch.zeros(2, 3, 64, device=DEV),
                                   torch.ones(2, 3, dtype=torch.bool, device=DEV))
    assert s.shape == (2, 2, 0, 256)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_behind_query_select():
    """``QuerySelect`` on rows (700, 300, 1200), K = 256, T = 77; its ``decoder_inputs_dict`` goes to the decoder on the device, the host
    chains run on the device's selection index.  Every layer's hidden states, boxes and head scores by ``hold``; two calls, equal bits;
    no device synchronise in the call."""
    feats, xyz, text, mask = qu.e2e_inputs()
    qs, dec = du.e2e_modules()
    qs, dec = qs.to(DEV), dec.to(DEV)
    keep = {}
    with torch.no_grad():
        d, head = qs([dev(f) for f in feats], None, [dev(p) for p in xyz], dev(text), dev(mask), keep_out=keep)

        def call():
            hs, bx = dec(query=d["query"], key=d["feats"], value=d["feats"], key_padding_mask=d["feats_attention_mask"], self_attn_mask=None,
                         cross_attn_mask=None, query_coords=d["query_coords"], key_coords=d["feats_coords"], pred_bboxes=d["pred_bboxes"],
                         text_feats=d["text_feats"], text_attention_mask=d["text_attention_mask"], bbox_head=qs)
            return hs, bx, dec.head_scores(hs, head, qs)

        first = call()
        torch.cuda.synchronize()
        with count_synchronises() as calls:
            second = call()
        assert calls == [], f"the decoder synchronised: {calls}"
        torch.cuda.synchronize()
    hidden, boxes, scores = (host(t) for t in first)
    assert hidden.shape == (6, 3, 256, 256) and boxes.shape == (6, 3, 256, 9) and scores.shape == (6, 3, 256, 256)
    for a, b in zip(first, second):
        assert bits_equal(host(a), host(b))
    ref = du.e2e_host(host(keep["index"]))
    r32, r64 = ref["float32"], ref["float64"]
    for lid in range(6):
        su.hold(f"end to end hidden layer {lid}", hidden[lid], r32[0][lid], r64[0][lid])
        su.hold(f"end to end boxes layer {lid}", boxes[lid], r32[1][lid], r64[1][lid])
        _hold_finite(f"end to end scores layer {lid}", scores[lid], r32[2][lid], r64[2][lid])
    gone = np.ones((3, 256), bool)
    gone[:, :77] = ~mask
    assert np.isneginf(scores.transpose(0, 2, 1, 3)[:, :, gone]).all() and np.isfinite(scores.transpose(0, 2, 1, 3)[:, :, ~gone]).all()
