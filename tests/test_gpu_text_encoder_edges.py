"""The text encoder's entry points (csrc/text_encoder.hip) one by one, at the edges tests/test_gpu_text_encoder.py does not reach: it runs
the chain from ids to ``last_hidden_state`` only.  Each entry point is called through ``_abi.lib()`` as ``text_encoder.py`` calls it
(tests/text_encoder_ops_util.py has the thin calls, the operands and the guard zones), at the smallest shape that takes the path.

The rule is ``sparse_util.hold``: the device's ``max|a - f64| / max|f64|`` at most 8 x that of the float32 host, which itself is
below 1e-5; the references are ``text_encoder_host``'s ``layer_norm_host`` / ``row_stats_host`` / ``ln_linear_host`` / ``linear_host`` /
``attention_host`` on the same fp32 operands in float32 and in float64; per call, the mean and the rstd column apart;
``hold_pooled`` where a call yields fewer than 64 values (the statistics of fewer than 64 rows).  tests/test_text_encoder_ops_host.py
shows on the same operands that the rule catches an uncentred variance, a dropped step of a slice, an admitted key t + 1, a
missing maximum and a wrong quick-GELU slope.  Everything else is bit for bit.

Every output is the first n rows of an allocation with 64 rows of 7.0 behind them; every operand read by rows has 64 rows of NaN behind
its end; ``stats`` is (n, 2) inside (n + 16, 2); the workspace is ``ptx_txt_linear_workspace_bytes`` exactly inside a longer tensor:
the zones keep their bits and the results are finite (``Guarded.read``, ``held``).

ln         C in 64, 192, 768, 1280 on n in 1, 15, 16, 17, 65 rows of ``30 + N(0, 1)`` and of ``N(0, 1)``: ``ptx_txt_ln``, and the
           ``stats`` and the output of ``ptx_txt_ln_linear`` (Cout = 64); a constant row, one NaN element, two calls, a row alone.
ln_linear  (Cin, Cout, act) in (64, 64, 0), (1280, 64, 0), (64, 5120, 0), (128, 320, 1), (1280, 5120, 1) on 1, 63, 64, 65, 129 rows
           (1 and 65 at Cout = 5120), with and without bias, rows ``30 + N(0, 1)`` at one shape per act, both quick-GELU tails.
linear     Cin in 64, 768, 832 (7 + 6 steps), 1536 (12 + 12), 1600 (9 + 9 + 7), 5120 (6 x 12 + 8) to Cout 64 and 192, and 64 -> 5120,
           on 1, 64, 65, 129 rows: bias x residual, in place and out of place (``out`` NaN before the call); an all-zero x.
attention  (B, T, H) from (1, 1, 1) to (64, 17, 1) and (1, 20, 20) under no mask, a random one, an empty key tile, no admitted key for
           queries 0 .. 4; logits up to +/-290; NaN k / v rows behind a query and under masked keys; a text alone; a uint8 mask.
embed      T = positions = 256, B = 64, C = 1280: bits against ``embed_host(float32)``; ids 0 and vocab - 1; ids outside the table at the
           last row; NaN rows behind both tables."""
import numpy as np
import pytest

from proxytransformation_amd import text_encoder_host as th
from tests import text_encoder_ops_util as O
from tests.sparse_util import hold, hold_pooled
from tests.text_encoder_util import EPS

pytestmark = pytest.mark.gpu


def _both(fn, *ops):
    """``fn`` on the fp32 operands and on the same operands in float64."""
    wide = [a.astype(np.float64) if isinstance(a, np.ndarray) and a.dtype == np.float32 else a for a in ops]
    return fn(*ops), fn(*wide)


def _same_but_row(out, clean, row):
    """``out`` has the bits of ``clean`` in every row but ``row``."""
    keep = np.arange(len(clean)) != row
    assert O.bits_equal(out[keep], clean[keep])


# ---------------------------------------------------------------------------------------------------------------------- 1. ln and the statistics
@pytest.mark.parametrize("kind", O.LN_KINDS)
@pytest.mark.parametrize("C", O.LN_WIDTHS)
def test_ln_and_the_statistics_off_zero_mean(C, kind):
    wl, bl = O.lnl_operands(C, 64, 0, 1)[3:]
    for n in O.LN_ROWS:
        x, w, b = O.ln_operands(C, n, kind)
        name = f"C={C} n={n} {kind}"
        O.held("ln " + name, O.ln(x, w, b), *_both(lambda x_, w_, b_: th.layer_norm_host(x_, w_, b_, EPS), x, w, b), hold)
        out, stats = O.ln_linear(x, w, b, wl, bl, 0)
        O.held("ln_linear(stats) " + name, out, *_both(lambda x_, w_, b_, wl_, bl_: th.ln_linear_host(x_, w_, b_, EPS, wl_, bl_, 0),
                                                         x, w, b, wl, bl), hold)
        for col, what in ((0, "mean"), (1, "rstd")):
            draws = iter(range(1, 1000))
            refs = lambda x_: tuple(r[col] for r in _both(lambda v: th.row_stats_host(v, EPS), x_))      # noqa: E731
            if n >= 64:
                O.held(f"stats {what} {name}", stats[:, col], *refs(x), hold)
                continue
            first = [x]
            draw = lambda: (first.pop() if first else O.ln_operands(C, n, kind, next(draws))[0],)      # noqa: E731
            call = lambda x_: O.ln_linear(x_, w, b, wl, bl, 0)[1][:, col]      # noqa: E731
            (x0,), got = hold_pooled(f"stats {what} {name}", n, draw, call, refs)
            assert x0 is x and O.bits_equal(got, stats[:, col]) and np.isfinite(got).all()


@pytest.mark.parametrize("C", O.LN_WIDTHS)
def test_ln_structure_bit_for_bit(C):
    n = 65
    x, w, b = O.ln_operands(C, n, "offset")
    wl, bl = O.lnl_operands(C, 64, 0, 1)[3:]
    clean = O.ln(x, w, b)
    clean_l, clean_s = O.ln_linear(x, w, b, wl, bl, 0)
    assert O.bits_equal(O.ln(x, w, b), clean)               # two calls
    again_l, again_s = O.ln_linear(x, w, b, wl, bl, 0)
    assert O.bits_equal(again_l, clean_l) and O.bits_equal(again_s, clean_s)
    for r in (0, 15, 16, 63, 64):                           # a row alone
        assert O.bits_equal(O.ln(x[r:r + 1], w, b)[0], clean[r]), r
        alone_l, alone_s = O.ln_linear(x[r:r + 1], w, b, wl, bl, 0)
        assert O.bits_equal(alone_l[0], clean_l[r]) and O.bits_equal(alone_s[0], clean_s[r]), r
    for r in (16, 64):
        const = x.copy()
        const[r] = 3.0                                      # mean 3 exactly, every centred value 0: the output is the bias
        out = O.ln(const, w, b)
        assert O.bits_equal(out[r], b)
        _same_but_row(out, clean, r)
        out_l, out_s = O.ln_linear(const, w, b, wl, bl, 0)
        assert out_s[r, 0] == 3.0 and out_s[r, 1] == np.float32(1.0) / np.sqrt(np.float32(EPS))
        _same_but_row(out_l, clean_l, r)
        _same_but_row(out_s, clean_s, r)
        bad = x.copy()
        bad[r, C - 3] = np.nan
        out = O.ln(bad, w, b)
        assert np.isnan(out[r]).all() and np.isnan(out).sum() == C
        _same_but_row(out, clean, r)
        out_l, out_s = O.ln_linear(bad, w, b, wl, bl, 0)
        assert np.isnan(out_l[r]).all() and np.isnan(out_s[r]).all() and np.isnan(out_l).sum() == 64
        _same_but_row(out_l, clean_l, r)
        _same_but_row(out_s, clean_s, r)


# ---------------------------------------------------------------------------------------------------------------------- 2. ln_linear
@pytest.mark.parametrize("cin,cout,act", O.LNL_SHAPES)
def test_ln_linear_off_the_modules_shapes(cin, cout, act):
    ref = lambda x_, g_, h_, w_, b_: th.ln_linear_host(x_, g_, h_, EPS, w_, b_, act)      # noqa: E731
    for n in O.lnl_rows(cout):
        for kind in ("zero", "offset") if (cin, cout, act) in O.LNL_OFFSET else ("zero",):
            x, g, h, w, b = O.lnl_operands(cin, cout, act, n, kind)
            for bias in (b, None):
                out, stats = O.ln_linear(x, g, h, w, bias, act)
                O.held(f"ln_linear {cin}->{cout} act={act} n={n} {kind} bias={bias is not None}", out, *_both(ref, x, g, h, w, bias), hold)
            assert not O.bits_equal(out, O.ln_linear(x, g, h, w, None, 1 - act)[0])          # act is read


@pytest.mark.parametrize("cin,cout,act", [(64, 64, 0), (128, 320, 1), (1280, 64, 0)])
def test_ln_linear_a_rows_bits_do_not_depend_on_the_rows_beside_it(cin, cout, act):
    x, g, h, w, b = O.lnl_operands(cin, cout, act, 129)
    full, full_s = O.ln_linear(x, g, h, w, b, act)
    again, again_s = O.ln_linear(x, g, h, w, b, act)
    assert O.bits_equal(again, full) and O.bits_equal(again_s, full_s)
    part, part_s = O.ln_linear(x[:65], g, h, w, b, act)
    assert O.bits_equal(part, full[:65]) and O.bits_equal(part_s, full_s[:65])
    for r in (0, 63, 64, 128):
        alone, alone_s = O.ln_linear(x[r:r + 1], g, h, w, b, act)
        assert O.bits_equal(alone[0], full[r]) and O.bits_equal(alone_s[0], full_s[r]), r


# ---------------------------------------------------------------------------------------------------------------------- 3. linear
@pytest.mark.parametrize("cin,cout", O.LIN_SHAPES)
def test_linear_across_slices_and_row_tiles(cin, cout):
    for n in O.LIN_ROWS:
        x, w, b, r = O.lin_operands(cin, cout, n)
        for bias in (b, None):
            for res in (r, None):
                name = f"linear {cin}->{cout} n={n} bias={bias is not None} residual={res is not None}"
                out = O.linear(x, w, bias, res)             # out of place: out is NaN before the call and is never read
                O.held(name, out, *_both(th.linear_host, x, w, bias, res), hold)
                assert O.bits_equal(O.linear(x, w, bias, res), out)          # two calls
                if res is not None:
                    assert O.bits_equal(O.linear(x, w, bias, res, in_place=True), out)          # residual = out, as the module calls it
        zero = O.linear(np.zeros_like(x), w, b, r, in_place=True)
        assert O.bits_equal(zero, b + r) and O.bits_equal(O.linear(np.zeros_like(x), w, b, r), b + r)


@pytest.mark.parametrize("cin", O.LIN_CIN)
def test_linear_a_rows_bits_do_not_depend_on_the_rows_beside_it(cin):
    cout = 64
    x, w, b, r = O.lin_operands(cin, cout, 129)
    full = O.linear(x, w, b, r)
    assert O.bits_equal(O.linear(x[:65], w, b, r[:65]), full[:65])
    for row in (0, 63, 64, 128):
        assert O.bits_equal(O.linear(x[row:row + 1], w, b, r[row:row + 1], in_place=True)[0], full[row]), row
    bad = x.copy()
    bad[64, cin - 1] = np.nan                               # the last channel of the last slice, first row of the second row tile
    out = O.linear(bad, w, b, r)
    assert np.isnan(out[64]).all() and np.isnan(out).sum() == cout
    _same_but_row(out, full, 64)


# ---------------------------------------------------------------------------------------------------------------------- 4. attention
@pytest.mark.parametrize("B,T,H", O.ATT_SHAPES)
def test_attention_at_every_tile_edge_and_mask(B, T, H):
    qkv = O.att_operands(B, T, H)
    for kind, mask in O.att_masks(B, T).items():
        out = O.attention(qkv, mask, H)
        O.held(f"attention B={B} T={T} H={H} mask={kind}", out, *_both(lambda q: th.attention_host(q, mask, H), qkv), hold)
        assert O.bits_equal(O.attention(qkv, mask, H), out)
        if kind == "late":
            assert not out[:, :5].any() and not np.signbit(out[:, :5]).any()          # no admitted key: zeros
        if mask is not None:                                # any nonzero byte is a token
            assert O.bits_equal(O.attention(qkv, np.where(mask, np.where(np.arange(T) % 2 == 0, 1, 255), 0).astype(np.uint8), H), out)
    if T == 1:
        assert O.bits_equal(out, qkv[..., 2 * 64 * H:])     # one key: its value


@pytest.mark.parametrize("B,T,H", O.ATT_LARGE)
def test_attention_at_large_logits(B, T, H):
    qkv = O.att_operands(B, T, H, large=True)
    for kind, mask in O.att_masks(B, T).items():
        O.held(f"attention large B={B} T={T} H={H} mask={kind}", O.attention(qkv, mask, H),
               *_both(lambda q: th.attention_host(q, mask, H), qkv), hold)


def test_attention_a_key_behind_a_query_and_a_masked_key_are_never_read():
    B, T, H = 2, O.POISON_T, 2
    C = 64 * H
    qkv = O.att_operands(B, T, H)
    clean = O.attention(qkv, None, H)
    text, head = 1, 1
    for j in O.POISON_AT:
        bad = qkv.copy()
        for part in (1, 2):                                 # k and v of (text, head) at position j; its q stays clean
            bad[text, j, part * C + 64 * head:part * C + 64 * head + 64] = np.nan
        out = O.attention(bad, None, H)
        hit = np.zeros((B, T, C), bool)
        hit[text, j:, 64 * head:64 * head + 64] = True
        assert np.isnan(out[hit]).all() and np.isfinite(out[~hit]).all(), j
        assert np.array_equal(out[~hit].view(np.uint32), clean[~hit].view(np.uint32)), j
    for kind in ("random", "late"):
        mask = O.att_masks(B, T)[kind]
        want = O.attention(qkv, mask, H)
        bad = qkv.copy()
        bad[..., C:][~mask] = np.nan                        # k and v under every masked key, all heads
        assert np.isnan(bad).any() and np.isfinite(bad[..., :C]).all()
        assert O.bits_equal(O.attention(bad, mask, H), want), kind


def test_attention_a_text_alone_has_the_bits_it_has_among_64():
    B, T, H = 64, 17, 1
    qkv = O.att_operands(B, T, H)
    for kind in ("none", "random"):
        mask = O.att_masks(B, T)[kind]
        full = O.attention(qkv, mask, H)
        for b in (0, 31, 63):
            alone = O.attention(qkv[b:b + 1], None if mask is None else mask[b:b + 1], H)
            assert O.bits_equal(alone[0], full[b]), (kind, b)


# ---------------------------------------------------------------------------------------------------------------------- 5. embed
@pytest.mark.parametrize("B,T,C,vocab,positions", O.EMBED_SHAPES)
def test_embed_at_the_ends_of_both_tables(B, T, C, vocab, positions):
    ids, tok, pos = O.embed_operands(B, T, C, vocab, positions)
    want = th.embed_host(ids, tok, pos)
    out = O.embed(ids, tok, pos)
    assert want.dtype == np.float32 and np.isfinite(out).all() and O.bits_equal(out, want)
    assert O.bits_equal(O.embed(ids, tok, pos), out)
    # a table with more rows than ``vocab`` says: the rows behind it are NaN here, and an id that points there is outside
    longer = np.concatenate([tok, np.full((3, C), np.nan, np.float32)])
    assert O.bits_equal(O.embed(ids, longer, pos, vocab=vocab), want)
    for bad_id in O.BAD_IDS:
        bad = ids.copy()
        bad[-1, -1] = bad_id                                # the last row of the last text: nothing behind it but the guard rows
        got = O.embed(bad, longer, pos, vocab=vocab).reshape(B * T, C)
        assert np.isnan(got[-1]).all() and O.bits_equal(got[:-1], want.reshape(B * T, C)[:-1]), bad_id
