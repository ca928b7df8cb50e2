"""What makes tests/test_gpu_text_encoder_edges.py non-vacuous, without a GPU, on the very operands it uses
(tests/text_encoder_ops_util.py):

* ``forward_host`` through ``row_stats_host`` / ``ln_linear_host`` / ``linear_host`` keeps the bits of the inline expressions it had;
* the rule (``sparse_util.hold``: at most 8 x the float32 host's error against float64, that error below 1e-5) has teeth: a float32
  restatement of each operator in the kernel's manner passes it on every case, and five deliberately wrong ones break it -- the
  uncentred variance, a sliced sum that drops the last slice's last step, an attention that admits key t + 1, an attention without the
  maximum at the large logits, a quick-GELU with 1.7;
* every mask does what its case claims, both quick-GELU tails occur, the large logits are large;
* every stated slice pattern is what ``ptx_txt_linear_workspace_bytes`` and the restated plan give, and no Cin leaves a slice empty."""
import numpy as np
import pytest

from proxytransformation_amd import _abi, text_encoder_host as th
from tests import text_encoder_ops_util as O
from tests import text_encoder_util as U
from tests.sparse_util import hold

EPS = U.EPS


def _both(fn, *ops):
    """``fn`` on the fp32 operands and on the same operands in float64."""
    wide = [None if a is None else (a.astype(np.float64) if isinstance(a, np.ndarray) and a.dtype == np.float32 else a) for a in ops]
    return fn(*ops), fn(*wide)


def breaks(name, got, ref32, ref64):
    """``got`` misses the rule (a non-finite result misses it too)."""
    if not np.isfinite(got).all():
        return
    with pytest.raises(AssertionError):
        hold(name, got, ref32, ref64)


# ---------------------------------------------------------------------------------------------------------------------- forward_host keeps its bits
def _forward_inline(params, input_ids, attention_mask, num_heads, eps, dtype, prefix="text_model."):
    """``forward_host`` as it was before the per-operator references existed: every expression inline."""
    dt = np.dtype(dtype)
    P = lambda name: np.asarray(params[prefix + name]).astype(dt)      # noqa: E731

    def layer_norm(x, weight, bias):
        mean = x.mean(-1, keepdims=True, dtype=dt)
        d = x - mean
        var = (d * d).mean(-1, keepdims=True, dtype=dt)
        rstd = dt.type(1.0) / np.sqrt(var + dt.type(eps))
        return d * rstd * weight + bias

    mask = None if attention_mask is None else np.asarray(attention_mask).astype(bool)
    x = th.embed_host(np.asarray(input_ids), P("embeddings.token_embedding.weight"), P("embeddings.position_embedding.weight"))
    i = 0
    while f"{prefix}encoder.layers.{i}.layer_norm1.weight" in params:
        L = lambda name, i=i: P(f"encoder.layers.{i}.{name}")      # noqa: E731
        h = layer_norm(x, L("layer_norm1.weight"), L("layer_norm1.bias"))
        w = np.concatenate([L("self_attn.q_proj.weight"), L("self_attn.k_proj.weight"), L("self_attn.v_proj.weight")])
        bq = np.concatenate([L("self_attn.q_proj.bias"), L("self_attn.k_proj.bias"), L("self_attn.v_proj.bias")])
        a = th.attention_host(h @ w.T + bq, mask, num_heads)
        x = x + (a @ L("self_attn.out_proj.weight").T + L("self_attn.out_proj.bias"))
        h = layer_norm(x, L("layer_norm2.weight"), L("layer_norm2.bias"))
        h = h @ L("mlp.fc1.weight").T + L("mlp.fc1.bias")
        h = h / (dt.type(1.0) + np.exp(dt.type(-1.702) * h))
        x = x + (h @ L("mlp.fc2.weight").T + L("mlp.fc2.bias"))
        i += 1
    return layer_norm(x, P("final_layer_norm.weight"), P("final_layer_norm.bias"))


@pytest.mark.parametrize("shape", U.HOST_CASES, ids=lambda s: "x".join(map(str, s)))
def test_forward_host_keeps_its_bits(shape):
    C, H, I, layers, B, T = shape
    params, ids, mask = U.make_params(C, I, layers), U.make_ids(B, T), U.make_mask("tail", B, T)
    for dtype in (np.float64, np.float32):
        got = th.forward_host(params, ids, mask, H, EPS, dtype)
        want = _forward_inline(params, ids, mask, H, EPS, dtype)
        assert got.dtype == want.dtype == np.dtype(dtype) and np.array_equal(got, want), (shape, dtype)


def test_the_operator_references_are_generic_in_dtype_and_take_none():
    x, g, h, w, b = O.lnl_operands(128, 320, 1, 17)
    for dt in (np.float32, np.float64):
        a = [t.astype(dt) for t in (x, g, h, w, b)]
        mean, rstd = th.row_stats_host(a[0], EPS)
        assert mean.dtype == rstd.dtype == dt and mean.shape == rstd.shape == (17,)
        assert th.ln_linear_host(a[0], a[1], a[2], EPS, a[3], None, 0).dtype == dt
        full = th.ln_linear_host(a[0], a[1], a[2], EPS, a[3], a[4], 1)
        assert full.dtype == dt and np.array_equal(full, th.quick_gelu_host(th.layer_norm_host(a[0], a[1], a[2], EPS) @ a[3].T + a[4]))
        r = a[0][:, :64]
        y = th.linear_host(a[0], a[3][:64], a[4][:64], r)
        assert y.dtype == dt and np.array_equal(y, (a[0] @ a[3][:64].T + a[4][:64]) + r)
        assert np.array_equal(th.linear_host(a[0], a[3][:64], None, None), a[0] @ a[3][:64].T)


# ---------------------------------------------------------------------------------------------------------------------- 1. LayerNorm and the statistics
@pytest.mark.parametrize("C", O.LN_WIDTHS)
def test_layer_norm_the_restatement_passes_and_the_uncentred_variance_breaks_the_rule(C):
    for kind in O.LN_KINDS:
        for n in O.LN_ROWS:
            parts = {k: [] for k in ("out", "mean", "rstd", "bad_out", "bad_rstd")}
            refs = {k: ([], []) for k in ("out", "mean", "rstd")}
            for draw in range(max(1, -(-64 // n))):         # pooled to 64 rows, as the device's statistics are
                x, w, b = O.ln_operands(C, n, kind, draw)
                r32, r64 = _both(lambda x_, w_, b_: th.layer_norm_host(x_, w_, b_, EPS), x, w, b)
                (m32, s32), (m64, s64) = _both(lambda x_: th.row_stats_host(x_, EPS), x)
                mean, rstd = O.stats32(x, EPS)
                bad_mean, bad_rstd = O.stats32(x, EPS, centred=False)
                assert np.array_equal(mean, bad_mean)
                for k, v in (("out", O.ln32(x, w, b, EPS)), ("mean", mean), ("rstd", rstd), ("bad_out", O.ln32(x, w, b, EPS, centred=False)),
                             ("bad_rstd", bad_rstd)):
                    parts[k].append(v.ravel())
                for k, (a32, a64) in (("out", (r32, r64)), ("mean", (m32, m64)), ("rstd", (s32, s64))):
                    refs[k][0].append(a32.ravel())
                    refs[k][1].append(a64.ravel())
            cat = lambda v: np.concatenate(v)      # noqa: E731
            for k in ("out", "mean", "rstd"):
                hold(f"host ln {k} C={C} n={n} {kind}", cat(parts[k]), cat(refs[k][0]), cat(refs[k][1]))
            if kind == "offset":
                breaks(f"uncentred out C={C} n={n}", cat(parts["bad_out"]), cat(refs["out"][0]), cat(refs["out"][1]))
                breaks(f"uncentred rstd C={C} n={n}", cat(parts["bad_rstd"]), cat(refs["rstd"][0]), cat(refs["rstd"][1]))


# ---------------------------------------------------------------------------------------------------------------------- 2. LayerNorm -> Linear
@pytest.mark.parametrize("cin,cout,act", O.LNL_SHAPES)
def test_ln_linear_the_restatement_passes_and_a_wrong_gelu_slope_breaks_the_rule(cin, cout, act):
    for n in O.lnl_rows(cout):
        for kind in ("zero", "offset") if (cin, cout, act) in O.LNL_OFFSET else ("zero",):
            x, g, h, w, b = O.lnl_operands(cin, cout, act, n, kind)
            for bias in (b, None):
                r32, r64 = _both(lambda x_, g_, h_, w_, b_: th.ln_linear_host(x_, g_, h_, EPS, w_, b_, act), x, g, h, w, bias)
                name = f"host ln_linear {cin}->{cout} act={act} n={n} {kind} bias={bias is not None}"
                hold(name, O.ln_linear32(x, g, h, EPS, w, bias, act), r32, r64)
                if act and bias is not None:
                    breaks(name + " slope 1.7", O.ln_linear32(x, g, h, EPS, w, bias, act, slope=1.7), r32, r64)
                if kind == "offset" and bias is not None:
                    breaks(name + " uncentred", O.ln_linear32(x, g, h, EPS, w, bias, act, centred=False), r32, r64)
            if act:
                fc1 = th.ln_linear_host(*(a.astype(np.float64) for a in (x, g, h)), EPS, w.astype(np.float64), b.astype(np.float64), 0)
                assert (fc1 < -6).any() and (fc1 > 6).any(), (cin, cout, n, kind)          # both tails of the quick-GELU


# ---------------------------------------------------------------------------------------------------------------------- 3. Linear and its slices
@pytest.mark.parametrize("cin", sorted(set(O.LIN_CIN) | {2112, 3072}))
def test_the_slice_patterns(cin):
    lib = _abi.lib()
    plan = O.slice_plan(cin)
    if cin in O.SLICE_PATTERNS:
        assert plan == O.SLICE_PATTERNS[cin]
    else:
        assert plan == [cin // 64] and cin <= 768
    assert sum(plan) == cin // 64 and len(plan) == -(-cin // 768)
    for n, cout in ((1, 64), (65, 192), (129, 64)):
        assert lib.ptx_txt_linear_workspace_bytes(n, cin, cout) == (len(plan) * n * cout * 4 if len(plan) > 1 else 0)


def test_no_width_leaves_a_slice_empty():
    lib = _abi.lib()
    for cin in range(64, 5121, 64):
        plan = O.slice_plan(cin)
        assert min(plan) >= 1 and sum(plan) == cin // 64 and max(plan) <= 12 and max(plan) - min(plan[:-1] or plan) == 0, (cin, plan)
        assert lib.ptx_txt_linear_workspace_bytes(3, cin, 64) == (len(plan) * 3 * 64 * 4 if cin > 768 else 0), cin


@pytest.mark.parametrize("cin,cout", O.LIN_SHAPES)
def test_linear_the_restatement_passes_and_a_dropped_step_breaks_the_rule(cin, cout):
    for n in O.LIN_ROWS:
        x, w, b, r = O.lin_operands(cin, cout, n)
        sums, short = O.sums32(x, w), O.sums32(x, w, drop_last_step=True) if cin > 768 else None
        for bias in (b, None):
            for res in (r, None):
                r32, r64 = _both(th.linear_host, x, w, bias, res)
                name = f"host linear {cin}->{cout} n={n} bias={bias is not None} residual={res is not None}"
                tail = lambda v: (v if bias is None else v + bias) if res is None else (v if bias is None else v + bias) + res      # noqa: E731
                hold(name, tail(sums), r32, r64)
                if short is not None:
                    breaks(name + " dropped step", tail(short), r32, r64)
        assert O.bits_equal(O.linear32(x, w, b, r), (sums + b) + r)


# ---------------------------------------------------------------------------------------------------------------------- 4. attention
def test_every_mask_does_what_its_case_claims():
    seen = set()
    for B, T, H in O.ATT_SHAPES + [(2, O.POISON_T, 2)]:
        masks = O.att_masks(B, T)
        seen |= set(masks)
        assert masks["none"] is None and masks["random"][:, 0].all() and masks["random"].shape == (B, T)
        assert T < 8 or not masks["random"].all()
        if "tile" in masks:
            assert T == 256 and not masks["tile"][0, 64:128].any() and masks["tile"][0, :64].any() and masks["tile"][0, 128:].any()
            assert masks["tile"][:, 0].all()
        assert ("late" in masks) == (T >= 15)
        if "late" in masks:
            m = masks["late"]
            assert not m[:, :5].any() and m[:, 5].all() and not m[:, 6:].all()
            out = th.attention_host(O.att_operands(B, T, H).astype(np.float64), m, H)
            assert not out[:, :5].any() and np.abs(out[:, 5:]).min() > 0          # queries 0 .. 4: no admitted key, zeros
    assert seen == {"none", "random", "tile", "late"}


@pytest.mark.parametrize("B,T,H", O.ATT_SHAPES)
def test_attention_the_restatement_passes_and_key_t_plus_1_breaks_the_rule(B, T, H):
    qkv = O.att_operands(B, T, H)
    for kind, mask in O.att_masks(B, T).items():
        r32, r64 = _both(lambda q: th.attention_host(q, mask, H), qkv)
        name = f"host attention B={B} T={T} H={H} mask={kind}"
        hold(name, O.attention32(qkv, mask, H), r32, r64)
        if T > 1 and (mask is None or mask[:, 1:].any()):
            breaks(name + " admits t + 1", O.attention32(qkv, mask, H, admit=1), r32, r64)


@pytest.mark.parametrize("B,T,H", O.ATT_LARGE)
def test_attention_at_large_logits_the_maximum_is_what_keeps_it_finite(B, T, H):
    qkv = O.att_operands(B, T, H, large=True)
    C = 64 * H
    q, k = qkv[0, :, :64].astype(np.float64) * 0.125, qkv[0, :, C:C + 64].astype(np.float64)
    assert np.abs(q @ k.T).max() > 89.0                     # beyond expf's range: exp(89) overflows float32
    for kind, mask in O.att_masks(B, T).items():
        r32, r64 = _both(lambda q_: th.attention_host(q_, mask, H), qkv)
        assert np.isfinite(r64).all() and np.isfinite(r32).all()
        name = f"host attention large B={B} T={T} H={H} mask={kind}"
        hold(name, O.attention32(qkv, mask, H), r32, r64)    # asserts the yardstick below 1e-5 as well
        wrong = O.attention32(qkv, mask, H, use_max=False)
        assert not np.isfinite(wrong).all()
        breaks(name + " without the maximum", wrong, r32, r64)


# ---------------------------------------------------------------------------------------------------------------------- 5. embed
@pytest.mark.parametrize("B,T,C,vocab,positions", O.EMBED_SHAPES)
def test_the_embed_operands_reach_both_ends_of_the_table(B, T, C, vocab, positions):
    ids, tok, pos = O.embed_operands(B, T, C, vocab, positions)
    assert ids.min() == 0 and ids.max() == vocab - 1 and T <= positions and tok.shape == (vocab, C) and pos.shape == (positions, C)
    out = th.embed_host(ids, tok, pos)
    assert out.dtype == np.float32 and np.array_equal(out[-1, -1], tok[vocab - 1] + pos[T - 1])
    for bad in O.BAD_IDS:
        other = ids.copy()
        other[-1, -1] = bad
        got = th.embed_host(other, tok, pos)
        assert np.isnan(got[-1, -1]).all() and np.isnan(got).sum() == C
