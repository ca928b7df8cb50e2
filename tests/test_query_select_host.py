"""The query selection behind the neck (proxytransformation_amd/query_select.py, query_select_host.py) pinned without a GPU: the numpy
restatement against a torch-CPU restatement of ``pre_decoder`` written here (matmul, ``masked_fill``, ``max``, ``torch.topk``, an
``nn.Sequential`` of Linears) in float64 on tie-free inputs and in fp32 on integer-valued operands; the dicts; ``load_from_head``; the
ABI surface; the raises; the backward restatement against autograd; and the near-tie count of the end-to-end input of
tests/test_gpu_query_select.py."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

from proxytransformation_amd import QuerySelect, _abi, query_select, query_select_host as qh
from tests import query_select_util as qu
from tests import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_stage(m, feats_list, xyz_list, text, mask, dtype):
    """``pre_decoder`` in torch on the CPU with the module's parameters: every intermediate the host restatement has, the boxes of ALL rows
    included (the reference runs the regression branch over every row and gathers afterwards)."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)          # noqa: E731
    reg = nn.Sequential(*[nn.Linear(l.in_features, l.out_features) if isinstance(l, nn.Linear) else nn.ReLU() for l in m.reg_branch]).to(dtype)
    reg.load_state_dict({k: v.to(dtype) for k, v in m.reg_branch.state_dict().items()})
    rows = [len(f) for f in feats_list]
    Lmax, C = max(rows), m.embed_dims
    joined = [torch.cat([t(f), t(p)], -1) for f, p in zip(feats_list, xyz_list)]
    padded = torch.stack([torch.cat([j, j.new_zeros(Lmax - len(j), C + 3)]) for j in joined])
    valid = torch.stack([torch.arange(Lmax) < n for n in rows])
    feats, coords = padded[..., :-3], padded[..., -3:]
    text, mask = t(text), torch.as_tensor(np.asarray(mask)).bool()
    res = feats @ text.transpose(-1, -2)
    if m.scaled:
        res = res / math.sqrt(C)
    if m.has_bias:
        res = res + m.cls_branch.bias.detach().to(dtype)
    res = res.masked_fill(~mask[:, None, :], float("-inf")).masked_fill(~valid[:, :, None], float("-inf"))
    full = torch.full((*res.shape[:-1], m.max_text_len), float("-inf"), dtype=dtype)
    full[..., :res.shape[-1]] = res
    score = full.max(-1)[0]
    K = min(m.num_queries, min(rows))
    values, index = torch.topk(score, k=K, dim=1)
    with torch.no_grad():
        p = reg(feats)
    boxes = torch.cat([p[..., :3] + coords, torch.exp(p[..., 3:6]).clamp(min=2e-2), p[..., 6:]], -1)
    return dict(feats=feats, coords=coords, pad=~valid, score=score, values=values, index=index, boxes_all=boxes, attn=~mask)


def _close(got, ref, tol=1e-12):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin])
    assert float(np.abs(got[fin] - ref[fin]).max()) <= tol * float(np.abs(ref[fin]).max())


def _gather(t, index):
    return torch.gather(t, 1, torch.as_tensor(index)[:, :, None].expand(-1, -1, t.shape[-1])).numpy()


# ------------------------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("log_scale,bias", [("auto", True), (None, False), ("none", True)])
def test_restatement_is_the_torch_stage_in_float64(log_scale, bias):
    feats, xyz, text, mask = qu.inputs((90, 41, 130), 13, 64, seed=3)
    mask[1] = True                                               # (a scene without a token ties every row at -inf: its own test below)
    m = qu.module(C=64, num_queries=40, log_scale=log_scale, bias=bias)
    keep = {}
    dec, head = m.forward_host(feats, None, xyz, text, mask, np.float64, keep_out=keep)
    ref = torch_stage(m, feats, xyz, text, mask, torch.float64)
    assert np.array_equal(keep["index"], ref["index"].numpy()) and keep["index"].dtype == np.int64 and keep["index"].shape == (3, 40)
    _close(keep["score"], ref["score"])
    _close(dec["feats"], ref["feats"], 0.0)
    _close(dec["feats_coords"], ref["coords"], 0.0)
    assert np.array_equal(dec["feats_attention_mask"], ref["pad"].numpy()) and np.array_equal(dec["text_attention_mask"], ref["attn"].numpy())
    _close(dec["query"], _gather(ref["feats"], keep["index"]), 0.0)
    _close(dec["query_coords"], _gather(ref["coords"], keep["index"]), 0.0)
    _close(dec["pred_bboxes"], _gather(ref["boxes_all"], keep["index"]))
    size = dec["pred_bboxes"][..., 3:6]
    assert (size == 0.02).any() and (size > 0.05).any()           # the clamp is active and inactive
    assert list(dec) == ["query", "feats", "feats_attention_mask", "query_coords", "feats_coords", "pred_bboxes", "text_feats",
                         "text_attention_mask"] and list(head) == ["text_feats", "text_token_mask"]
    assert dec["query"].shape == (3, 40, 64) and dec["feats"].shape == (3, 130, 64) and dec["pred_bboxes"].shape == (3, 40, 9)
    assert dec["feats_attention_mask"].dtype == bool and dec["text_attention_mask"].shape == (3, 13) and head["text_token_mask"].dtype == bool
    assert all(dec[k].dtype == np.float64 for k in ("query", "feats", "query_coords", "feats_coords", "pred_bboxes", "text_feats"))


def test_restatement_in_fp32_on_integer_operands_is_exact():
    """Integer-valued features and text: every product and sum of the score is exact in fp32, so the host's fp32 scores are torch's bit
    for bit.  Integers tie, and ``torch.topk`` leaves ties open: the selected VALUES are held in order, the host's own rows by the rule."""
    feats, xyz, text, mask = qu.inputs((90, 41, 130), 13, 64, seed=4, integer=True)
    m = qu.module(C=64, num_queries=40)
    with torch.no_grad():
        m.cls_branch.bias.fill_(-4.5)
    keep = {}
    dec, _ = m.forward_host(feats, None, xyz, text, mask, np.float32, keep_out=keep)
    ref = torch_stage(m, feats, xyz, text, mask, torch.float32)
    assert keep["score"].dtype == np.float32 and np.array_equal(keep["score"].view(np.uint32), ref["score"].numpy().view(np.uint32))
    assert np.isneginf(keep["score"][1]).all() and np.isneginf(keep["score"][0, 90:]).all()      # no token; padding
    assert np.array_equal(np.take_along_axis(keep["score"], keep["index"], 1), ref["values"].numpy())
    assert keep["index"][1].tolist() == list(range(40))          # every row at -inf: the lower row first
    for b, n in enumerate((90, 41, 130)):
        s = keep["score"][b, :n]
        order = keep["index"][b]
        assert len(set(order.tolist())) == 40 and all(s[i] > s[j] or (s[i] == s[j] and i < j) for i, j in zip(order[:-1], order[1:]))
    ref_boxes = _gather(ref["boxes_all"], keep["index"])
    assert dec["pred_bboxes"].dtype == np.float32 and float(np.abs(dec["pred_bboxes"] - ref_boxes).max()) <= 1e-5 * float(np.abs(ref_boxes).max())


def test_score_keeps_a_nan_under_an_unmasked_token_only():
    feats, xyz, text, mask = qu.inputs(qu.SMALL_ROWS, 7, 64, seed=5)
    assert not mask[0, 3] and mask[0, 2] and not mask[1].any()
    text[0, 3, 9] = np.nan                                       # under a masked token: no trace
    feats[2][100, 5] = np.nan                                    # a row's every product: NaN score
    f, c, pad = qh.pack_host(feats, xyz)
    for dt, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        s = qh.score_host(f.astype(dt), pad, text.astype(dt), mask, np.array([-1.5], dt))
        assert np.isfinite(s[0, :65]).all() and np.isneginf(s[0, 65:]).all() and np.isneginf(s[1]).all()
        assert np.isnan(s[2, 100]) and np.isnan(s[2]).sum() == 1
    m = qu.module(C=64, num_queries=1)
    ref = torch_stage(m, feats, xyz, text, mask, torch.float64)["score"].numpy()
    assert np.isnan(ref[2, 100]) and np.isnan(ref).sum() == 1    # torch.max's rule


def test_sorted_topk_rule():
    pos, neg = qu.nan_signs()
    s = np.array([[1.0, 0.0, -0.0, 2.0, 0.0, np.inf, -np.inf, pos, neg, 1.0, 99.0]], np.float32)
    s[0, 7], s[0, 8] = pos, neg
    assert qh.topk_sorted_host(s, [10], 10).tolist() == [[7, 5, 3, 0, 9, 1, 2, 4, 6, 8]]        # row 10 is padding
    assert qh.topk_sorted_host(s, [10], 5).tolist() == [[7, 5, 3, 0, 9]]
    assert qh.topk_sorted_host(s.astype(np.float64), [10], 6).tolist() == [[7, 5, 3, 0, 9, 1]]
    with pytest.raises(ValueError, match="fewer than k=4"):
        qh.topk_sorted_host(s, [3], 4)


def test_sorted_topk_rule_where_a_scene_has_no_order_and_where_it_takes_every_row():
    """What tests/test_gpu_query_select_edges.py relies on.  A scene of one value, all ``-inf`` or all NaN of one sign is one tie: the rows
    0 .. k - 1 in order (the stated rule; torch leaves ties open).  k = rows on tie-free scores: ``torch.topk``'s permutation."""
    pos, neg = qu.nan_signs()
    for value in (np.float32(0.5), np.float32(-np.inf), pos, neg, np.float32(-0.0)):
        s = np.full((1, 9), np.inf, np.float32)
        s[0, :7] = value
        for k in (1, 5, 7):
            assert qh.topk_sorted_host(s, [7], k).tolist() == [list(range(k))]
    s = np.random.default_rng(8).standard_normal((2, 300)).astype(np.float32)
    got = qh.topk_sorted_host(s, [300, 300], 300)
    assert np.array_equal(got, torch.topk(torch.from_numpy(s), 300, dim=1)[1].numpy()) and sorted(got[1].tolist()) == list(range(300))
    mixed = np.array([[neg, 1.0, pos, -np.inf, pos, np.inf]], np.float32)          # +NaN above +inf, -NaN below -inf, equal NaNs by row
    mixed[0, [0, 2, 4]] = neg, pos, pos
    assert qh.topk_sorted_host(mixed, [6], 6).tolist() == [[2, 4, 5, 1, 3, 0]]


def test_score_with_a_leading_tile_of_masked_tokens_is_the_torch_stage():
    """T = 70 with the first 64 tokens masked in scene 0, only the last token in scene 1, only token 40 in scene 2: the maximum starts
    behind a whole 64-token tile."""
    feats, xyz, text, mask = qu.inputs((90, 41, 130), 70, 64, seed=9)
    mask[:] = False
    mask[0, 64:], mask[1, 69], mask[2, 40] = True, True, True
    m = qu.module(C=64, num_queries=40)
    keep = {}
    m.forward_host(feats, None, xyz, text, mask, np.float64, keep_out=keep)
    ref = torch_stage(m, feats, xyz, text, mask, torch.float64)
    _close(keep["score"], ref["score"])
    assert np.isfinite(keep["score"][0, :90]).all() and np.isneginf(keep["score"][0, 90:]).all()
    assert np.array_equal(keep["index"], ref["index"].numpy())


def test_backward_restatement_is_autograd_in_float64():
    rng = np.random.default_rng(6)
    rows, C, K = (9, 4, 12), 5, 4
    leaves = [torch.from_numpy(rng.standard_normal((n, C))).requires_grad_() for n in rows]
    index = np.stack([rng.permutation(n)[:K] for n in rows])
    padded = torch.stack([torch.cat([f, f.new_zeros(max(rows) - len(f), C)]) for f in leaves])
    query = torch.gather(padded, 1, torch.from_numpy(index)[:, :, None].expand(-1, -1, C))
    G1, G2 = rng.standard_normal(tuple(padded.shape)), rng.standard_normal(tuple(query.shape))
    ((padded * torch.from_numpy(G1)).sum() + (query * torch.from_numpy(G2)).sum()).backward()
    for got, leaf in zip(qh.backward_host(G1, G2, index, rows), leaves):
        _close(got, leaf.grad)
    only_q = qh.backward_host(None, G2, index, rows)
    assert all((g != 0).any(axis=1).sum() == K for g in only_q) and np.array_equal(only_q[1][index[1]], G2[1])
    only_f = qh.backward_host(G1.astype(np.float32), None, index, rows)
    assert only_f[0].dtype == np.float32 and np.array_equal(only_f[2], G1.astype(np.float32)[2, :12])


# ------------------------------------------------------------------------------------------------------------------ the module
def test_parameters_carry_the_reference_names_and_load_from_a_head():
    m = QuerySelect()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [
        ("cls_branch.bias", (1,)), ("reg_branch.0.weight", (256, 256)), ("reg_branch.0.bias", (256,)), ("reg_branch.2.weight", (256, 256)),
        ("reg_branch.2.bias", (256,)), ("reg_branch.4.weight", (9, 256)), ("reg_branch.4.bias", (9,))]
    assert float(m.cls_branch.bias.detach()) == pytest.approx(-math.log(99))
    assert "cls_branch.bias" not in QuerySelect(bias=False).state_dict()
    assert list(QuerySelect(embed_dims=64, num_reg_fcs=1).state_dict()) == ["cls_branch.bias", "reg_branch.0.weight", "reg_branch.0.bias",
                                                                           "reg_branch.2.weight", "reg_branch.2.bias"]
    m.init_weights()
    assert not m.reg_branch[4].weight.detach().any() and not m.reg_branch[4].bias.detach().any() and m.reg_branch[0].weight.detach().any()
    torch.manual_seed(1)
    sd = {}
    for layer in range(7):                                       # the reference head: 7 prediction layers, the last one is ours
        sd[f"bbox_head.cls_branches.{layer}.bias"] = torch.randn(1)
        for i, shape in ((0, (256, 256)), (2, (256, 256)), (4, (9, 256))):
            sd[f"bbox_head.reg_branches.{layer}.{i}.weight"] = torch.randn(*shape)
            sd[f"bbox_head.reg_branches.{layer}.{i}.bias"] = torch.randn(shape[0])
    sd["decoder.layers.0.norm.weight"] = torch.randn(256)
    m.load_from_head(sd, 6)
    assert torch.equal(m.cls_branch.bias, sd["bbox_head.cls_branches.6.bias"])
    assert all(torch.equal(getattr(m.reg_branch[i], p), sd[f"bbox_head.reg_branches.6.{i}.{p}"]) for i in (0, 2, 4) for p in ("weight", "bias"))
    with pytest.raises(KeyError, match="cls_branches.7.bias"):
        m.load_from_head(sd, 7)
    m.load_from_head({k[len("bbox_head."):]: v for k, v in sd.items()}, 0, prefix="")
    assert torch.equal(m.reg_branch[2].bias, sd["bbox_head.reg_branches.0.2.bias"])


def test_refusals_name_their_numbers():
    for kw, exc, match in ((dict(num_reg=12), NotImplementedError, "num_reg=12"), (dict(box_coder="FCAF"), NotImplementedError, "FCAF"),
                           (dict(log_scale=0.5), NotImplementedError, "0.5"), (dict(log_scale="manual"), ValueError, "but got manual"),
                           (dict(embed_dims=100), ValueError, "got 100"), (dict(embed_dims=576), ValueError, "got 576"),
                           (dict(num_queries=1025), ValueError, "got 1025"), (dict(num_queries=0), ValueError, "got 0"),
                           (dict(max_text_len=257), ValueError, "got 257"), (dict(num_reg=7), ValueError, "got 7"),
                           (dict(box_coder="other"), ValueError, "other")):
        with pytest.raises(exc, match=match):
            QuerySelect(**kw)
    m = QuerySelect(embed_dims=64, num_queries=4, max_text_len=8)
    f, p = [torch.zeros(5, 64), torch.zeros(6, 64)], [torch.zeros(5, 3), torch.zeros(6, 3)]
    text, mask = torch.zeros(2, 8, 64), torch.ones(2, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(f, None, p, text, mask)
    with pytest.raises(NotImplementedError, match="differentiable=True"):
        m([f[0].clone().requires_grad_(), f[1]], None, p, text, mask)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU path"):
            m([f[0].clone().requires_grad_(), f[1]], None, p, text, mask)
    with pytest.raises(ValueError, match="max_text_len=8 text tokens, got 9"):
        m(f, None, p, torch.zeros(2, 9, 64), torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"feats \(L,64\) expected, got \(5, 128\)"):
        m([torch.zeros(5, 128), f[1]], None, p, text, mask)
    with pytest.raises(ValueError, match="got 66 and 66"):
        m(f * 33, None, p * 33, text, mask)
    for call in (lambda: query_select.pack(f, p, mask), lambda: query_select.score(torch.zeros(2, 6, 64), [5, 6], text, mask),
                 lambda: query_select.topk_sorted(torch.zeros(2, 6), [5, 6], 2),
                 lambda: query_select.linear(torch.zeros(2, 6, 64), torch.zeros(64, 64), None),
                 lambda: query_select.decode(None, torch.zeros(9, 64), None, torch.zeros(2, 6, 64), torch.zeros(2, 6, 3),
                                             torch.zeros(2, 2, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_header_binding_and_exports_declare_the_entry_points():
    lib = _abi.lib()
    hooks = ctypes.CDLL(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip_testhooks.so"))
    for name, params in su.assert_declared(qu.QS_ENTRY_POINTS).items():
        assert len(params.split(",")) == len(_abi.SIGNATURES[name][1]), name
        getattr(hooks, name)
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13 and hooks.ptx_abi_version() == 13
    assert "query_select.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()


def test_argument_checks_answer_einval_before_touching_a_device():
    lib = _abi.lib()
    EINVAL = -1
    ints = lambda *e: (ctypes.c_int32 * len(e))(*e)          # noqa: E731
    err = lambda: lib.ptx_last_error()                       # noqa: E731
    pack = lambda B, C, Lmax, T, rows: lib.ptx_qs_pack(None, None, rows, B, C, Lmax, None, T, None, None, None, None, None)      # noqa: E731
    assert pack(65, 256, 10, 8, ints(1)) == EINVAL and b"B=65" in err()
    assert pack(1, 96, 10, 8, ints(1)) == EINVAL and b"C=96" in err() and pack(1, 576, 10, 8, ints(1)) == EINVAL and b"C=576" in err()
    assert pack(1, 256, 10, 257, ints(1)) == EINVAL and b"T=257" in err() and pack(1, 256, 10, 0, ints(1)) == EINVAL and b"T=0" in err()
    assert pack(2, 256, 10, 8, ints(3, 11)) == EINVAL and b"rows[1]=11" in err() and b"Lmax=10" in err()
    assert pack(1, 256, 10, 8, None) == EINVAL and b"rows is null" in err() and pack(1, 256, 10, 8, ints(10)) == EINVAL and b"null" in err()
    score = lambda C, T, scaled=1: lib.ptx_qs_score(None, ints(4), 1, 4, C, None, None, T, scaled, None, None, None)      # noqa: E731
    assert score(100, 8) == EINVAL and b"C=100" in err() and score(64, 300) == EINVAL and b"T=300" in err()
    assert score(64, 8, 2) == EINVAL and b"scaled=2" in err() and score(64, 8) == EINVAL and b"null" in err()
    topk = lambda K, rows, Lmax=2000: lib.ptx_qs_topk(None, rows, 1, Lmax, K, None, None, None)      # noqa: E731
    assert topk(1025, ints(1500)) == EINVAL and b"K=1025" in err() and topk(0, ints(5)) == EINVAL and b"K=0" in err()
    assert topk(7, ints(6)) == EINVAL and b"rows[0]=6 is below K=7" in err() and topk(6, ints(6)) == EINVAL and b"null" in err()
    lin = lambda cin, cout, relu=1: lib.ptx_qs_linear(None, 40, None, 2, 20, 20, None, None, cin, cout, relu, None, None)      # noqa: E731
    assert lin(80, 64) == EINVAL and b"C=80" in err() and lin(64, 9) == EINVAL and b"Cout=9" in err()
    assert lin(64, 64, 3) == EINVAL and b"relu=3" in err() and lin(64, 64) == EINVAL and b"null" in err()
    dec = lambda C, K=4, Lmax=9: lib.ptx_qs_decode(None, None, None, C, None, None, None, 2, K, Lmax, None, None, None, None)      # noqa: E731
    assert dec(32) == EINVAL and b"C=32" in err() and dec(64, K=10) == EINVAL and b"K=10 Lmax=9" in err() and dec(64) == EINVAL and b"null" in err()
    bwd = lambda C, rows: lib.ptx_qs_bwd(None, None, None, rows, 2, 9, 4, C, None, None)      # noqa: E731
    assert bwd(200, ints(5, 9)) == EINVAL and b"C=200" in err() and bwd(64, ints(5, 10)) == EINVAL and b"rows[1]=10" in err()
    assert bwd(64, ints(5, 9)) == EINVAL and b"null" in err() and bwd(64, ints(0, 0)) == 0


# ------------------------------------------------------------------------------------------------------------------ the end-to-end input
def test_end_to_end_input_has_few_near_ties():
    """The input of tests/test_gpu_query_select.py's end-to-end test: all three scenes have more rows than K = 256, and in the fp32 and
    the float64 host scores at most 2 % of K rows per scene lie within ``neck_util.NEAR_TIE * max |score|`` of the K-th score.  If this
    fails, change the seed of ``query_select_util.e2e_inputs``, not the cap."""
    feats, xyz, text, mask = qu.e2e_inputs()
    m = qu.module()
    K = min(qu.E2E_QUERIES, min(qu.E2E_ROWS))
    assert K == 256 and sum(n > K for n in qu.E2E_ROWS) >= 2
    for dt in (np.float32, np.float64):
        keep = {}
        dec, _ = m.forward_host(feats, None, xyz, text, mask, dt, keep_out=keep)
        ties = qu.near_ties(keep["score"], qu.E2E_ROWS, K)
        assert len(ties) >= 2
        for scene, count, kth in ties:
            print(f"{np.dtype(dt).name} scene {scene}: K-th score {kth:+.5f}, {count} near-ties")
            assert count <= 0.02 * K, (scene, count)
        flat, _ = qu.scene_scores(keep["score"], qu.E2E_ROWS)
        assert np.isfinite(flat).all() and len(np.unique(flat)) == len(flat)     # tie-free: torch.topk would agree
        size = dec["pred_bboxes"][..., 3:6]
        assert (size == dt(0.02)).mean() > 0.05 and (size > 0.05).mean() > 0.05
