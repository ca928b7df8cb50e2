"""The transformer decoder behind the query selection (proxytransformation_amd/decoder.py, decoder_host.py) pinned without a GPU: the numpy
restatement against a torch-CPU restatement of the stage written in tests/decoder_util.py (``nn.MultiheadAttention``, ``nn.Conv1d``,
``nn.BatchNorm1d`` in eval, ``nn.LayerNorm``, ``nn.Linear`` with mmcv's wrapper rules) in float64; the ``T == K`` rule; a scene without a
text token; the state dict against the manifest; the raises; the ABI surface; the argument checks; and the fp32 yardstick of the
end-to-end input of tests/test_gpu_decoder.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from proxytransformation_amd import ClipTextEncoder, GroundingDecoder, ResNet, _abi, decoder, decoder_host as dh
from tests import decoder_util as du
from tests import query_select_util as qu
from tests import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (65, 1, 257)


def _close(got, ref, tol=1e-12):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    for lid in range(len(ref)):
        assert float(np.abs(got[lid] - ref[lid]).max()) <= tol * float(np.abs(ref[lid]).max()), lid


def _small(T, seed, text_mask):
    m, br = du.module(**du.SMALL), du.reg_branches(64, 2)
    return m, br, du.operands(ROWS, 7, T, 64, seed, text_mask)


# ------------------------------------------------------------------------------------------------------------------ restatement
def test_host_chain_is_the_torch_stage_and_keeps_mmcvs_key_pos_rule():
    """C = 64, 2 heads, FFN 128, 2 layers, rows (65, 1, 257), K = T = 7: the text keys receive ``query_pos``.  At T = 8 with a masked
    eighth token they do not, and nothing else differs: the T = 8 result is the T = 7 result with the rule switched off."""
    tm7 = np.zeros((3, 7), bool)
    tm7[1, :3] = True
    m, br, ops7 = _small(7, 5, tm7)
    h7, b7 = du.host(m, ops7, br, np.float64)
    assert h7.shape == (2, 3, 7, 64) and b7.shape == (2, 3, 7, 9) and h7.dtype == np.float64
    th, tb = du.torch_stage(m, ops7, br)
    _close(h7, th)
    _close(b7, tb)
    ops8 = dict(ops7)
    rng = np.random.default_rng(9)
    ops8["text_feats"] = np.concatenate([ops7["text_feats"], rng.standard_normal((3, 1, 64)).astype(np.float32)], 1)
    ops8["text_attention_mask"] = np.concatenate([tm7, np.ones((3, 1), bool)], 1)
    h8, b8 = du.host(m, ops8, br, np.float64)
    th8, tb8 = du.torch_stage(m, ops8, br)
    _close(h8, th8)
    _close(b8, tb8)
    assert float(np.abs(h8 - h7).max()) > 1e-3 * float(np.abs(h7).max())          # the rule matters
    off_h, off_b = du.host(m, ops7, br, np.float64, text_keys_take_pos=False)
    _close(h8, off_h)
    _close(b8, off_b)
    size = b7[..., 3:6]
    assert (size == 0.02).any() and (size > 0.03).any()                            # the clamp is active and inactive


def test_a_scene_without_a_text_token_gets_zeros_plus_bias_as_torch_does():
    tm = np.zeros((3, 5), bool)
    tm[1] = True
    m, br, ops = _small(5, 6, tm)
    h, b = du.host(m, ops, br, np.float64)
    th, tb = du.torch_stage(m, ops, br)
    _close(h, th)
    _close(b, tb)
    q = np.random.default_rng(1).standard_normal((3, 7, 64))
    o = dh.attention_host(q, ops["text_feats"].astype(np.float64), ops["text_feats"].astype(np.float64), tm, 2)
    assert not o[1].any() and o[0].any() and o[2].any()                           # exact zeros from the attention itself
    nan = ops["text_feats"].astype(np.float64)
    nan[1, 2, 3] = np.nan                                                         # under a masked key: never read
    assert np.array_equal(dh.attention_host(q, nan, nan, tm, 2), o)
    nan[0, 2, 3] = np.nan                                                         # head 0 of scene 0, unmasked: that scene and head
    bad = dh.attention_host(q, nan, nan, tm, 2)
    assert np.isnan(bad[0, :, :32]).all() and np.array_equal(bad[0, :, 32:], o[0, :, 32:]) and np.array_equal(bad[1:], o[1:])


def test_operator_restatements():
    rng = np.random.default_rng(2)
    x, add = rng.standard_normal((5, 64)), rng.standard_normal((5, 64))
    w, b = rng.standard_normal((128, 64)), rng.standard_normal(128)
    full = dh.linear_host(x, w, b, add=add, add_cols=64)
    assert np.allclose(full[:, :64], (x + add) @ w[:64].T + b[:64]) and np.allclose(full[:, 64:], x @ w[64:].T + b[64:])
    x[0, 0] = np.nan
    assert np.isnan(dh.linear_host(x, w, b, relu=True)[0]).all()                  # the ReLU keeps a NaN
    y = rng.standard_normal((4, 64)) + 1000.0
    ln = torch.nn.LayerNorm(64).double()
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5), ln.bias.normal_()
    ref = ln(torch.from_numpy(y)).detach().numpy()
    assert np.abs(dh.layer_norm_host(y, ln.weight.detach().numpy(), ln.bias.detach().numpy()) - ref).max() < 1e-9
    hs, text = rng.standard_normal((2, 3, 4, 64)), rng.standard_normal((3, 5, 64))
    tok = np.ones((3, 5), bool)
    tok[0, 1] = False
    s = dh.contrastive_scores_host(hs, text, tok, np.array([-4.5]), True, 8)
    assert s.shape == (2, 3, 4, 8) and np.isneginf(s[..., 5:]).all() and np.isneginf(s[:, 0, :, 1]).all() and np.isfinite(s[:, 1:, :, :5]).all()
    assert np.allclose(s[1, 2, 3, 4], hs[1, 2, 3] @ text[2, 4] / 8.0 - 4.5)


# ------------------------------------------------------------------------------------------------------------------ the module
def test_state_dict_is_the_manifest_and_loads_strictly():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "decoder_state_dict.json")))
    m = GroundingDecoder(6, du.layer_cfg(256, 8, 2048))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want
    names = dict((k, tuple(s)) for k, s in want)
    assert names["layers.5.cross_attn_text.attn.in_proj_weight"] == (768, 256) and names["layers.0.ffn.layers.0.0.weight"] == (2048, 256)
    assert names["layers.0.ffn.layers.1.weight"] == (256, 2048) and names["layers.3.norms.3.bias"] == (256,)
    assert names["self_posembed.position_embedding_head.0.weight"] == (256, 9, 1)
    assert names["cross_posembed.position_embedding_head.0.weight"] == (256, 3, 1)
    assert names["layers.2.self_posembed.position_embedding_head.0.weight"] == (256, 3, 1)
    assert names["self_posembed.position_embedding_head.1.num_batches_tracked"] == () and names["norm.weight"] == (256,)
    torch.manual_seed(3)
    sd = {k: (torch.randn(*s) if "num_batches" not in k else torch.tensor(7)) for k, s in want}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.layers[4].cross_attn.attn.out_proj.weight, sd["layers.4.cross_attn.attn.out_proj.weight"])
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "norm.bias"}, strict=True)
    # the reference's defaults where a key is missing: 256 wide, 8 heads, FFN 1024
    d = GroundingDecoder(1, {})
    assert d.embed_dims == 256 and tuple(d.state_dict()["layers.0.ffn.layers.0.0.weight"].shape) == (1024, 256)


def test_the_per_layer_self_posembed_loads_and_is_never_read():
    m, br, ops = _small(5, 7, None)
    before = du.host(m, ops, br, np.float64)
    with torch.no_grad():
        for layer in m.layers:
            for p in list(layer.self_posembed.parameters()) + list(layer.self_posembed.buffers()):
                if p.is_floating_point():
                    p.mul_(3.0).add_(1.0)
    after = du.host(m, ops, br, np.float64)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_refusals():
    cfg = du.layer_cfg(64, 2, 128)
    with pytest.raises(ValueError, match="There is not post_norm"):
        GroundingDecoder(2, cfg, post_norm_cfg=dict(type="LN"))
    for bad, match in ((du.layer_cfg(100, 2, 128), "got 100"), (du.layer_cfg(64, 4, 128), "head dimension"),
                       (du.layer_cfg(64, 2, 100), "got 100"), (du.layer_cfg(64, 2, 4096), "got 4096")):
        with pytest.raises(ValueError, match=match):
            GroundingDecoder(1, bad)
    m, br = GroundingDecoder(2, cfg, with_cp=True).eval(), du.reg_branches(64, 2)
    o = {k: torch.from_numpy(v) for k, v in du.operands((5, 6), 4, 3, 64, 1).items()}
    args = lambda **kw: {**dict(query=o["query"], key=o["key"], value=o["key"], key_padding_mask=o["key_padding_mask"], self_attn_mask=None,      # noqa: E731
                                cross_attn_mask=None, query_coords=o["query_coords"], key_coords=o["key_coords"],
                                pred_bboxes=o["pred_bboxes"], text_feats=o["text_feats"], text_attention_mask=o["text_attention_mask"],
                                bbox_head=br), **kw}
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(**args())
    with pytest.raises(NotImplementedError, match="self_attn_mask"):
        m(**args(self_attn_mask=torch.zeros(4, 4, dtype=torch.bool)))
    with pytest.raises(NotImplementedError, match="cross_attn_mask"):
        m(**args(cross_attn_mask=torch.zeros(4, 6, dtype=torch.bool)))
    with pytest.raises(NotImplementedError, match="value must be key"):
        m(**args(value=o["key"].clone()))
    with pytest.raises(ValueError, match="bbox_head is None"):
        m(**args(bbox_head=None))
    with pytest.raises(NotImplementedError, match="requires grad"):
        m(**args(query=o["query"].clone().requires_grad_()))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(**args(query=o["query"].clone().requires_grad_()))
    m.train()
    with pytest.raises(NotImplementedError, match="eval forward only"):
        m(**args())
    m.eval()
    with pytest.raises(ValueError, match=r"pred_bboxes \(2, 4, 9\) expected"):
        m(**args(pred_bboxes=o["pred_bboxes"][:, :, :6]))
    with pytest.raises(ValueError, match="2 regression branches expected, got 1"):
        m(**args(bbox_head=list(br)[:1]))
    z = torch.zeros
    for call in (lambda: decoder.posembed(z(1, 4, 3), m.cross_posembed), lambda: decoder.linear(z(1, 4, 64), z(64, 64), None),
                 lambda: decoder.attention(z(1, 4, 64), z(1, 5, 64), z(1, 5, 64), z(1, 5, dtype=torch.bool), 2),
                 lambda: decoder.layer_norm(z(4, 64), m.norm), lambda: decoder.linear_add_ln(z(4, 64), z(64, 64), None, z(4, 64), m.norm),
                 lambda: decoder.boxes(z(1, 4, 64), z(9, 64), None, z(1, 4, 3)),
                 lambda: decoder.contrastive_scores(z(2, 1, 4, 64), z(1, 3, 64), z(1, 3, dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_host_chain_with_two_groups_of_hoisted_projections_is_the_torch_stage():
    """C = 512, heads (self 8, text 16, scene 8), FFN 64, 5 layers -- the module tests/test_gpu_decoder_edges.py runs because its key /
    value projections leave the layer loop in two groups (4 + 1 layers) -- on rows (65, 1, 130), K = 3, at T = 5 and at T = K = 3: the
    float64 host chain is the torch stage, and the fp32 host chain is a yardstick (within 1e-5 of float64); the latter also for the
    C = 256 module of 9 layers (8 + 1)."""
    m, br = du.module(**du.WIDE), du.reg_branches(512, 5)
    layer = m.layers[0]
    assert (layer.self_attn.num_heads, layer.cross_attn_text.num_heads, layer.cross_attn.num_heads) == (8, 16, 8)
    assert [g["ids"] for g in m._prepare(torch.device("cpu"))["groups"]] == [[0, 1, 2, 3], [4]]
    deep, dbr = du.module(**du.DEEP), du.reg_branches(256, 9)
    assert [g["ids"] for g in deep._prepare(torch.device("cpu"))["groups"]] == [list(range(8)), [8]]
    for T in (5, 3):
        ops = du.group_operands(512, T, 11)
        assert ops["text_attention_mask"].sum() == 2 and ops["key"].shape == (3, 130, 512)
        h64, b64 = du.host(m, ops, br, np.float64)
        th, tb = du.torch_stage(m, ops, br)
        _close(h64, th)
        _close(b64, tb)
        cases = [("C=512", du.host(m, ops, br, np.float32), (h64, b64))]
        dops = du.group_operands(256, T, 12)
        cases.append(("C=256", du.host(deep, dops, dbr, np.float32), du.host(deep, dops, dbr, np.float64)))
        for name, r32, r64 in cases:
            for a32, a64 in zip(r32, r64):
                assert a32.dtype == np.float32 and a64.dtype == np.float64
                for lid in range(len(a64)):
                    assert su.rel(a32[lid], a64[lid]) < 1e-5, (name, T, lid)


def _cached_decoder(seed=21):
    m = du.module(**du.SMALL, seed=seed)
    return m, m.layers[0].cross_attn.attn, "in_proj_weight", lambda prep: prep["layers"][0]["cross_attn"]["w"]


def _cached_text_encoder(seed=21):
    torch.manual_seed(seed)
    m = ClipTextEncoder(vocab_size=64, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1,
                        max_position_embeddings=8)
    return m, m.text_model.encoder.layers[0].self_attn.out_proj, "weight", lambda prep: prep["layers"][0]["wo"]


def _cached_resnet(seed=21):
    torch.manual_seed(seed)
    m = ResNet(depth=50, base_channels=16, num_stages=1, out_indices=(0,))
    return m, m.layer1[0].conv1, "weight", lambda prep: prep["stages"][0][0]["w1"].reshape(16, 16, 1, 1)


@pytest.mark.parametrize("make", [_cached_decoder, _cached_text_encoder, _cached_resnet], ids=["decoder", "text_encoder", "resnet"])
def test_prepared_operands_are_rebuilt_when_a_parameter_is_replaced_or_changed(make):
    """The one cache of prepared operands (``_doors.PreparedOperands``) under its three modules, each at its smallest size: ``_prepare``
    returns the same object while nothing changed, and a new one after ``load_state_dict`` (copying, and with ``assign=True``), an
    in-place update under ``no_grad`` (a parameter, a BatchNorm's floating-point buffer) and after a parameter is REPLACED by a new
    ``nn.Parameter`` of the same ``_version`` -- the version alone does not identify a tensor.  An integer buffer
    (``num_batches_tracked``) is not watched: no operand reads it."""
    cpu = torch.device("cpu")
    m, holder, attr, operand = make()
    first = m._prepare(cpu)
    assert m._prepare(cpu) is first
    old = getattr(holder, attr)
    new = torch.nn.Parameter(old.detach().clone() * 2)
    with torch.no_grad():
        while new._version < old._version:
            new.add_(0.0)
    assert new._version == old._version and new is not old
    setattr(holder, attr, new)
    second = m._prepare(cpu)
    assert second is not first and m._prepare(cpu) is second
    assert torch.equal(operand(second), new.detach()) and torch.equal(operand(first), old.detach())
    if make is _cached_decoder:
        assert torch.equal(second["groups"][0]["cross_attn"][0][:64], new.detach()[64:128])      # the hoisted [K_0 K_1 | V_0 V_1]
        assert torch.equal(first["groups"][0]["cross_attn"][0][:64], old.detach()[64:128])
    other = make(seed=5)[0]
    changes = [lambda: new.mul_(0.5), lambda: m.load_state_dict(other.state_dict()),
               lambda: m.load_state_dict(make(seed=6)[0].state_dict(), assign=True)]
    if make is _cached_decoder:
        changes.insert(1, lambda: m.cross_posembed.position_embedding_head[1].running_var.mul_(1.5))
    if make is _cached_resnet:
        changes.insert(1, lambda: m.bn1.running_var.mul_(2))
    last = second
    for i, change in enumerate(changes):
        with torch.no_grad():
            change()
        again = m._prepare(cpu)
        assert again is not last and m._prepare(cpu) is again, i
        last = again
        if change is changes[-2]:
            assert torch.equal(operand(last), getattr(make(seed=5)[1], attr).detach())
    assert torch.equal(operand(last), getattr(make(seed=6)[1], attr).detach())
    if make is _cached_resnet:
        before = m.bn1.num_batches_tracked.item()
        m.bn1.num_batches_tracked.add_(1)
        assert m.bn1.num_batches_tracked.item() == before + 1 and m._prepare(cpu) is last


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_exports_declare_the_entry_points():
    lib = _abi.lib()
    hooks = ctypes.CDLL(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip_testhooks.so"))
    for name, params in su.assert_declared(du.DEC_ENTRY_POINTS).items():
        assert len(params.split(",")) == len(_abi.SIGNATURES[name][1]), name
        getattr(hooks, name)
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13 and hooks.ptx_abi_version() == 13
    assert "decoder.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()


def test_argument_checks_answer_einval_before_touching_a_device():
    lib = _abi.lib()
    EINVAL = -1
    err = lambda: lib.ptx_last_error()                       # noqa: E731
    pos = lambda n, cin, C: lib.ptx_dec_posembed(None, n, cin, None, None, None, None, C, None, None)      # noqa: E731
    assert pos(0, 3, 64) == EINVAL and b"n=0" in err() and pos(4, 10, 64) == EINVAL and b"cin=10" in err()
    assert pos(4, 3, 96) == EINVAL and b"C=96" in err() and pos(4, 3, 64) == EINVAL and b"null" in err()
    lin = lambda n, cin, cout, relu=0, cols=0: lib.ptx_dec_linear(None, None, cols, n, None, None, cin, cout, relu, None, None, None)      # noqa: E731
    assert lin(0, 64, 64) == EINVAL and b"n=0" in err() and lin(4, 80, 64) == EINVAL and b"Cin=80" in err()
    assert lin(4, 2112, 64) == EINVAL and b"Cin=2112" in err() and lin(4, 64, 4160) == EINVAL and b"Cout=4160" in err()
    assert lin(4, 64, 64, 2) == EINVAL and b"relu=2" in err() and lin(4, 64, 128, 0, 32) == EINVAL and b"add_cols=32" in err()
    assert lin(4, 64, 128, 0, 192) == EINVAL and b"add_cols=192" in err() and lin(4, 64, 64) == EINVAL and b"null" in err()
    att = lambda B=1, Kq=4, L=5, H=2, hd=32, ld=64: lib.ptx_dec_attention(None, ld, None, ld, None, ld, None, B, Kq, L, H, hd, None, None)      # noqa: E731
    assert att(B=65) == EINVAL and b"B=65" in err() and att(Kq=1025) == EINVAL and b"Kq=1025" in err() and att(L=0) == EINVAL and b"L=0" in err()
    assert att(hd=48) == EINVAL and b"hd=48" in err() and att(H=9, hd=64, ld=576) == EINVAL and b"H=9" in err()
    assert att(ld=60) == EINVAL and b"ldq=60" in err() and att(ld=66) == EINVAL and b"ldq=66" in err() and att() == EINVAL and b"null" in err()
    ln = lambda n, C, eps=1e-5: lib.ptx_dec_ln(None, n, C, None, None, eps, None, None, None, None, None)      # noqa: E731
    assert ln(0, 64) == EINVAL and b"n=0" in err() and ln(4, 576) == EINVAL and b"C=576" in err() and ln(4, 64, 0.0) == EINVAL and b"eps=0" in err()
    assert ln(4, 64) == EINVAL and b"null" in err()
    box = lambda n, C: lib.ptx_dec_boxes(None, None, None, C, None, n, None, None)      # noqa: E731
    assert box(0, 64) == EINVAL and b"n=0" in err() and box(4, 32) == EINVAL and b"C=32" in err() and box(4, 64) == EINVAL and b"null" in err()
    sc = lambda NL=1, B=1, K=4, C=64, T=3, M=8, scaled=1: lib.ptx_dec_scores(None, NL, B, K, C, None, None, T, M, scaled, None, None, None)      # noqa: E731
    assert sc(NL=0) == EINVAL and b"NL=0" in err() and sc(K=1025) == EINVAL and b"K=1025" in err() and sc(C=100) == EINVAL and b"C=100" in err()
    assert sc(T=9) == EINVAL and b"T=9" in err() and sc(M=257, T=3) == EINVAL and b"max_text_len=257" in err()
    assert sc(scaled=2) == EINVAL and b"scaled=2" in err() and sc() == EINVAL and b"null" in err()


# ------------------------------------------------------------------------------------------------------------------ the end-to-end input
def test_fp32_host_chain_of_the_end_to_end_input_is_a_yardstick():
    """The precondition ``sparse_util.hold`` asserts, at every layer of tests/test_gpu_decoder.py's end-to-end case: the fp32 host chain
    lies within 1e-5 of the float64 chain in ``sparse_util.rel``'s measure.  If this fails, fix the host chain's summation, not the bound."""
    assert qu.E2E_ROWS == (700, 300, 1200) and qu.E2E_T == 77
    out = du.e2e_host()
    for i, name in enumerate(("hidden", "boxes", "scores")):
        a32, a64 = out["float32"][i], out["float64"][i]
        assert a32.shape == a64.shape and len(a64) == 6 and a32.dtype == np.float32 and a64.dtype == np.float64
        for lid in range(6):
            fin = np.isfinite(a64[lid])
            assert np.array_equal(fin, np.isfinite(a32[lid])) and (name == "scores") == (not fin.all())
            e = float(np.abs(a32[lid][fin].astype(np.float64) - a64[lid][fin]).max() / np.abs(a64[lid][fin]).max())
            print(f"{name} layer {lid}: fp32 host against float64 {e:.3e}")
            assert e < 1e-5, (name, lid, e)
