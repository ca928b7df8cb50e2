"""``GroundingDetector`` and the level join without a GPU: the ABI surface of ``ptx_level_join`` / ``ptx_level_join_bwd`` (header, bindings,
export table, ABI still 13), the host-side refusals of the two entry points (nothing is enqueued: no device is touched), the state
dict under the reference's names against the manifest ``tests/golden/grounder_state_dict.json`` (names and shapes read off the
reference's constructors, like the per-module manifests it is assembled from; NOT pinned against a real checkpoint), the checkpoint
round trip with its raises, and the constructor's refusals, each naming its argument."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import oracle

from proxytransformation_amd import _abi
from tests.detector_util import PAD, inputs, make_detector, small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptx_level_join_table_floats", "ptx_level_join", "ptx_level_join_bwd_workspace_bytes", "ptx_level_join_bwd")
PTX_EINVAL, PTX_ENOSPACE = -1, -3


def shipped_cfg():
    """configs/grounding/proxy-tiblock33-gs12-wbias-ddr0.6-clip.py, ``model=`` (CFG:19-100); CLIP ViT-L/14's text width is 768."""
    cfg = small_cfg(num_queries=256, text_width=768)
    cfg["preshape"] = dict(type="ProxyTransformationNormReverse", n_points=100000, grid_size=12, text_blocks=3, img_blocks=3,
                           dynamic_drop_radio=0.6, num_sub=30)
    cfg["backbone_3d"]["depth"] = 34
    cfg["neck_3d"]["pts_prune_threshold"] = 1000
    cfg["decoder"]["num_layers"] = 6
    cfg["decoder"]["layer_cfg"]["ffn_cfg"]["feedforward_channels"] = 2048
    return cfg


def build(**over):
    from proxytransformation_amd import GroundingDetector
    return GroundingDetector(**small_cfg(**over))


# ------------------------------------------------------------------------------------------------------------------ ABI surface
def test_header_bindings_and_export_table_agree_and_the_abi_is_still_13():
    src = open(os.path.join(ROOT, "include", "proxyt.h")).read()
    assert "#define PTX_ABI_VERSION 13" in src and _abi.ABI_VERSION == 13
    lib = _abi.lib()
    assert lib.ptx_abi_version() == 13
    for name in NAMES:
        m = re.search(r"PTX_API (size_t|int) " + name + r"\(([^;]*)\);", src)
        assert m, name
        nargs = len([a for a in m.group(2).replace("\n", " ").split(",") if a.strip()])
        res, args = _abi.SIGNATURES[name]
        assert len(args) == nargs, (name, len(args), nargs)
        assert res is (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int), name
        getattr(lib, name)
    assert re.search(r"global:\s*ptx_\*;", open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "exports.map")).read())
    assert "level_join.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()
    pkg = os.path.join(ROOT, "proxytransformation_amd")
    for so in ("libproxyt_hip.so", "libproxyt_hip_testhooks.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pkg, so)], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for name in NAMES:
            assert name in exported, (so, name)
        assert all(n.startswith("ptx_") or n.startswith("__") or "_Z" in n for n in exported if "level_join" in n or "psb_" in n)
        assert not any(n.startswith("_ZN3ptx7psb_run") or n.startswith("_ZN3ptx9psb_bytes") for n in exported), "internals stay hidden"


def _tables(B, V, pad=(96.0, 96.0)):
    t = np.zeros((_abi.lib().ptx_level_join_table_floats(B, V),), np.float32)
    for b in range(B):
        t[32 * b + 13:32 * b + 21] = (1, 1, 0, 0, 0, 96, pad[0], pad[1])
    return t


def test_sizes():
    lib = _abi.lib()
    assert lib.ptx_level_join_table_floats(2, 3) == 2 * 32 + 2 * 3 * 16
    assert lib.ptx_level_join_table_floats(0, 3) == 0 and lib.ptx_level_join_table_floats(65, 3) == 0 and lib.ptx_level_join_table_floats(1, 0) == 0
    for args in ((10, 3, 5, 4, 0), (257, 65, 5, 4, 1)):
        assert lib.ptx_level_join_bwd_workspace_bytes(*args) == lib.ptx_point_sample_bwd_workspace_bytes(*args) > 0
    assert lib.ptx_level_join_bwd_workspace_bytes(0, 3, 5, 4, 0) == 0


@pytest.mark.parametrize("what,kw,word", [
    ("Cb", dict(Cb=96), "Cb=96"), ("Ci", dict(Ci=576), "Ci=576"), ("Cb0", dict(Cb=0), "Cb=0"), ("B", dict(B=65), "B=65"),
    ("V", dict(V=0), "V=0"), ("voxel", dict(voxel=0.0), "voxel_size=0"), ("pad", dict(pad=(0.0, 96.0)), "pad=(0"), ("n", dict(n=-1), "n=-1"),
])
def test_the_checks_run_on_the_host_before_anything_is_enqueued(what, kw, word):
    """Every refusal returns PTX_EINVAL with the argument in the message; the device pointers are never read (they are fakes)."""
    lib = _abi.lib()
    a = dict(n=4, Cb=64, Ci=64, B=2, V=3, voxel=0.01, pad=(96.0, 96.0))
    a.update(kw)
    t = _tables(min(max(a["B"], 1), 64), max(a["V"], 1), a["pad"])
    fake = 0x1000
    ptrs = (ctypes.c_void_p * 65)(*([fake] * 65))
    rc = lib.ptx_level_join(fake, a["n"], fake, a["Cb"], ptrs, t.ctypes.data, fake, a["B"], a["V"], a["Ci"], 5, 4, a["voxel"], 0, fake, None, None)
    assert rc == PTX_EINVAL and word in lib.ptx_last_error().decode(), lib.ptx_last_error()
    ends = (ctypes.c_int32 * 65)(*([max(a["n"], 0)] * 65))
    rc = lib.ptx_level_join_bwd(fake, a["n"], ends, fake, a["Cb"], fake, t.ctypes.data, fake, a["B"], a["V"], a["Ci"], 5, 4, a["voxel"], 0,
                                fake, fake, 0, fake, 1 << 30, None)
    assert rc == PTX_EINVAL and word in lib.ptx_last_error().decode(), lib.ptx_last_error()


def test_backward_refuses_bad_scene_ends_and_a_small_workspace_on_the_host():
    lib = _abi.lib()
    t = _tables(2, 3)
    fake = 0x1000
    call = lambda ends, ws_bytes, dtype=0: lib.ptx_level_join_bwd(fake, 8, (ctypes.c_int32 * 2)(*ends), fake, 64, fake, t.ctypes.data, fake,    # noqa: E731
                                                                  2, 3, 64, 5, 4, 0.01, 0, fake, fake, dtype, fake, ws_bytes, None)
    assert call((5, 3), 1 << 30) == PTX_EINVAL and "scene_end[1]=3" in lib.ptx_last_error().decode()
    assert call((3, 7), 1 << 30) == PTX_EINVAL and "!= n=8" in lib.ptx_last_error().decode()
    assert call((3, 8), 1 << 30, dtype=3) == PTX_EINVAL and "dtype=3" in lib.ptx_last_error().decode()
    assert call((3, 8), 16) == PTX_ENOSPACE and "workspace too small" in lib.ptx_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------ checkpoints
def test_reference_state_dict_is_the_manifest_at_the_shipped_configuration():
    from proxytransformation_amd import GroundingDetector
    want = [(n, tuple(s)) for n, s in json.load(open(os.path.join(ROOT, "tests", "golden", "grounder_state_dict.json")))]
    det = GroundingDetector(**shipped_cfg())
    got = [(n, tuple(t.shape)) for n, t in det.reference_state_dict().items()]
    assert sorted(got) == sorted(want)
    assert len({n for n, _ in got}) == len(got)


@pytest.fixture(scope="module")
def pair():
    torch.manual_seed(0)
    a, b = build(), build()
    with torch.no_grad():
        for p in a.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    return a, b


def test_round_trip_loads_strictly_and_reproduces_every_tensor(pair):
    a, b = pair
    sd = a.reference_state_dict()
    NL = a.decoder.num_layers
    assert sum(k.startswith("bbox_head.cls_branches.") for k in sd) == NL + 1
    assert sum(k.startswith("bbox_head.reg_branches.") for k in sd) == 6 * (NL + 1)
    assert "text_feat_map.weight" in sd and not any(k.startswith("query_select") for k in sd)
    report = b.load_reference_state_dict(sd, strict=True)
    assert report == dict(skipped=[], missing=[], unexpected=[])
    for (ka, ta), (kb, tb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(ta, tb), ka


def test_load_raises_on_missing_unequal_alias_and_unexpected_and_skips_the_outside_modules(pair):
    a, b = pair
    sd = a.reference_state_dict()
    missing = {k: v for k, v in sd.items() if k != "neck_3d.conv_cls.bias"}
    with pytest.raises(KeyError, match="neck_3d.conv_cls.bias"):
        b.load_reference_state_dict(missing, strict=True)
    assert b.load_reference_state_dict(missing, strict=False)["missing"] == ["neck_3d.conv_cls.bias"]
    alias = dict(sd)
    alias["bbox_head.reg_branches.1.2.weight"] = sd["bbox_head.reg_branches.1.2.weight"] + 1.0
    with pytest.raises(ValueError, match=r"bbox_head\.reg_branches\.1\.2\.weight"):
        b.load_reference_state_dict(alias, strict=False)
    extra = dict(sd, **{"neck.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="neck.weight"):
        b.load_reference_state_dict(extra, strict=True)
    assert b.load_reference_state_dict(extra, strict=False)["unexpected"] == ["neck.weight"]
    outside = dict(sd, **{"backbone.conv1.weight": torch.zeros(1), "text_encoder.embeddings.weight": torch.zeros(1)})
    report = b.load_reference_state_dict(outside, strict=True)
    assert report["skipped"] == ["backbone.conv1.weight", "text_encoder.embeddings.weight"] and not report["unexpected"]


# ------------------------------------------------------------------------------------------------------------------ constructor
def test_share_pred_layer_false_raises():
    cfg = small_cfg()
    cfg["bbox_head"]["share_pred_layer"] = False
    from proxytransformation_amd import GroundingDetector
    with pytest.raises(NotImplementedError, match="share_pred_layer"):
        GroundingDetector(**cfg)


def _head(**kw):
    return dict(small_cfg()["bbox_head"], **kw)


def _neck(**kw):
    return dict(small_cfg()["neck_3d"], **kw)


@pytest.mark.parametrize("over,exc,word", [
    (dict(use_xyz_feat=False), NotImplementedError, "use_xyz_feat"),
    (dict(coord_type="POLAR"), ValueError, "coord_type"),
    (dict(voxel_size=0.0), ValueError, "voxel_size"),
    (dict(text_width=100), ValueError, "text_width"),
    (dict(num_queries=0), ValueError, "num_queries"),
    (dict(matcher="gpu"), ValueError, "matcher"),
    (dict(bbox_head=None), TypeError, "bbox_head"),
    (dict(bbox_head=_head(type="FCAF3DHead")), ValueError, "bbox_head"),
    (dict(bbox_head=_head(num_pred_layer=5)), ValueError, "num_pred_layer"),
    (dict(bbox_head=_head(embed_dims=128)), ValueError, "bbox_head embed_dims"),
    (dict(bbox_head=_head(num_reg=12)), NotImplementedError, "num_reg"),
    (dict(neck_3d=_neck(voxel_size=0.02)), ValueError, "neck_3d voxel_size"),
    (dict(neck_3d=_neck(out_channels=128)), ValueError, "neck_3d out_channels"),
    (dict(neck_3d=3), TypeError, "neck_3d"),
    (dict(backbone_3d=dict(type="NoSuchBackbone")), ValueError, "backbone_3d"),
    (dict(decoder=dict(small_cfg()["decoder"], post_norm_cfg=dict(type="LN"))), ValueError, "post_norm"),
])
def test_constructor_refusals_name_the_argument(over, exc, word):
    with pytest.raises(exc, match=word):
        build(**over)


def test_children_carry_the_keywords():
    det = build(differentiable=True, matcher="device", fused_join=False)
    assert det.backbone_3d.differentiable and det.neck_3d.differentiable and det.decoder.differentiable and det.query_select.differentiable
    assert det.bbox_head.matcher == "device" and det.fused_join is False and det.differentiable
    assert det.text_feat_map.weight.shape == (256, 128) and det.query_select.num_queries == 32
    plain = build()
    assert not plain.differentiable and plain.fused_join and not plain.neck_3d.differentiable and plain.bbox_head.matcher == "host"


# ------------------------------------------------------------------------------------------------------------------ the host chain
@pytest.fixture(scope="module")
def host_chain():
    """``forward_host`` in float32 with the host's own decisions, on the inputs and the detector of tests/test_gpu_detector.py."""
    x = inputs("cpu")
    det = make_detector(differentiable=True).eval()
    return x, det, det.forward_host(x["points"], x["text"], x["mask"], x["img"], x["scenes"], img_pad_shape=PAD, dtype=np.float32,
                                    gt_bboxes=x["gt"], positive_maps=x["pos"], host=oracle)


def test_the_gpu_tests_shape_reaches_what_it_is_chosen_for_on_the_host_chain(host_chain):
    """Every level of both scenes is non-empty, at least one prune step drops rows, and ``K = num_queries`` is smaller than the
    smallest scene's rows -- on the host chain, without a device."""
    x, det, h = host_chain
    assert len(h["joined"]) == 4
    for lv, width in zip(h["joined"], (128, 256, 512, 1024)):
        rows = np.diff([0] + list(lv.scene_rows))
        assert len(rows) == 2 and (rows > 0).all() and lv.feats.shape == (lv.scene_rows[-1], width), (lv.tensor_stride, rows)
    assert len(h["keep"]) == 3 and any(k.size > k.sum() for k in h["keep"])
    smallest = min(f.shape[0] for f in h["neck"][0])
    assert h["decoder_inputs"]["query"].shape == (2, 32, 256) and det.num_queries == 32 < smallest


def test_host_chain_outputs_have_the_devices_shapes_and_are_finite(host_chain):
    x, det, h = host_chain
    NL = det.decoder.num_layers
    assert h["hidden_states"].shape == (NL, 2, 32, 256) and h["all_layers_pred_bboxes"].shape == (NL, 2, 32, 9)
    assert h["all_layers_cls_scores"].shape == (NL, 2, 32, 256) and h["bboxes_3d"].shape == (2, 32, 9) and h["scores_3d"].shape == (2, 32)
    assert np.isfinite(h["hidden_states"]).all() and np.isfinite(h["bboxes_3d"]).all() and ((h["scores_3d"] > 0) & (h["scores_3d"] < 1)).all()
    s = h["all_layers_cls_scores"]
    assert np.isfinite(s[:, 0, :, :9]).all() and np.isneginf(s[:, 0, :, 9:]).all() and np.isneginf(s[:, 1, :, 7:]).all()   # the masked tokens
    assert set(h["losses"]) == {"loss_cls", "loss_bbox", "d0.loss_cls", "d0.loss_bbox"} and all(np.isfinite(v) and v > 0 for v in h["losses"].values())
    assert h["assign"].shape == (NL, 2, 32) and ((h["assign"] >= 0).sum(-1) == np.array([1, 3])).all()
    # the renaming of DET:605-617 against the selection itself: the queries are the selected rows of the padded features
    dec, idx = h["decoder_inputs"], h["select"]["index"]
    for b in range(2):
        assert np.array_equal(dec["query"][b], dec["feats"][b][idx[b]]) and np.array_equal(dec["query_coords"][b], dec["feats_coords"][b][idx[b]])
