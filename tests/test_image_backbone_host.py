"""The image backbone without a GPU: ``image_backbone_host.resnet_host`` -- the specification of csrc/conv2d.hip and of
``image_backbone.ResNet`` -- against a float64 composition of torch's own ``F.conv2d`` / ``F.batch_norm(training=False)`` / ``F.relu`` /
``F.max_pool2d`` (tests/image_backbone_util.torch_levels) to 1e-12 of each level's scale; ``conv2d_host`` / ``max_pool_host`` on the
kernels' case tables; the state-dict manifest; the constructor's refusals; the detector's host chain with ``imgs=``; the ABI surface of
the three entry points and their host-side refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import MODELS, ResNet, _abi, image_backbone_host as H
from tests import image_backbone_util as U
from tests.detector_util import inputs, make_detector, small_cfg
from tests.sparse_util import assert_declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("ptx_conv_stem", "ptx_conv1x1", "ptx_conv3x3")
PTX_EINVAL = -1


# ------------------------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize("shape", [(6, 3, 96, 96), (2, 3, 33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_resnet_host_is_the_torch_composition_in_double(shape):
    net = U.build_backbone()
    imgs = U.make_images(shape)
    want = U.torch_levels(net, imgs)
    got = net.forward_host(imgs, dtype=np.float64)
    f32 = net.forward_host(imgs, dtype=np.float32)
    assert len(got) == len(want) == 4
    for l, (g, w, s) in enumerate(zip(got, want, f32)):
        e, e32, scale = U.err(g, w), U.err(s, w), float(np.abs(w).max())
        print(f"{shape} level {l}: shape {g.shape}, scale {scale:.1f}, positive {float((w > 0).mean()):.2f}, err {e:.3e}, float32 chain {e32:.3e}")
        assert g.shape == w.shape == (shape[0], 64 << l) + tuple(net.level_shapes(*shape[2:])[l][1:])
        assert g.dtype == np.float64 and s.dtype == np.float32
        assert (w > 0).mean() > 0.3 and scale > 1.0          # the level is alive: the comparison says something
        assert e <= 1e-12, (shape, l, e)
        assert e32 <= 1e-5, (shape, l, e32)                 # a float32 chain (2^-24 per rounding), not a broken one


def test_the_deeper_network_and_the_early_exit_against_torch():
    net = U.build_backbone(**U.DEEP)
    imgs = U.make_images((2, 3, 64, 64))
    want, got = U.torch_levels(net, imgs), net.forward_host(imgs)
    assert [g.shape for g in got] == [(2, 64, 16, 16), (2, 256, 4, 4)] and net.stage_blocks == (3, 4, 23)
    for g, w in zip(got, want):
        assert U.err(g, w) <= 1e-12


def test_leading_dimensions_mean_std_and_the_channel_swap():
    net = U.build_backbone()
    x = torch.randint(0, 256, (2, 2, 3, 40, 36), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    got = net.forward_host(x, mean=U.MEAN, std=U.STD)
    xn = (x.float() - torch.tensor(U.MEAN).view(1, 1, 3, 1, 1)) / torch.tensor(U.STD).view(1, 1, 3, 1, 1)
    assert np.array_equal(H.normalise_host(x.numpy().reshape(4, 3, 40, 36), U.MEAN, U.STD), xn.numpy().reshape(4, 3, 40, 36))
    want = U.torch_levels(net, xn)
    for g, w in zip(got, want):
        assert g.shape == (2, 2) + w.shape[1:] and U.err(g.reshape(w.shape), w) <= 1e-12
    swapped = net.forward_host(x.flip(2), mean=U.MEAN, std=U.STD, bgr_to_rgb=True)
    assert all(np.array_equal(a, b) for a, b in zip(swapped, got))


# ------------------------------------------------------------------------------------------------------------------ kernel specifications
def test_conv2d_host_on_the_kernels_case_tables():
    rng = np.random.default_rng(0)
    for (cin, cout), (h, w) in [(c, s) for c in U.CONV1_CHANNELS for s in U.CONV1_SIZES]:
        x, k = rng.standard_normal((U.N_IMAGES, cin, h, w)), rng.standard_normal((cout, cin, 1, 1))
        want = F.conv2d(torch.from_numpy(x), torch.from_numpy(k)).numpy()
        assert U.err(H.conv2d_host(x, k), want) <= 1e-12, (cin, cout, h, w)
    for h, w in U.CONV1_STRIDED:
        for cin, cout in U.CONV1_CHANNELS:
            x, k = rng.standard_normal((U.N_IMAGES, cin, h, w)), rng.standard_normal((cout, cin, 1, 1))
            want = F.conv2d(torch.from_numpy(x), torch.from_numpy(k), stride=2).numpy()
            got = H.conv2d_host(x, k, 2, 0)
            assert got.shape == want.shape == (U.N_IMAGES, cout, U.out_side(h, 2), U.out_side(w, 2)) and U.err(got, want) <= 1e-12
    for n, h, w in U.STEM_CASES:
        for c0 in U.STEM_C0:
            x, k = rng.standard_normal((n, 3, h, w)), rng.standard_normal((c0, 3, 7, 7))
            want = F.max_pool2d(F.conv2d(torch.from_numpy(x), torch.from_numpy(k), stride=2, padding=3), 3, 2, 1).numpy()
            got = H.max_pool_host(H.conv2d_host(x, k, 2, 3))
            assert got.shape == want.shape == (n, c0, U.pooled(h), U.pooled(w)) and U.err(got, want) <= 1e-12, (n, h, w, c0)


@pytest.mark.parametrize("c", U.CONV3_CHANNELS)
def test_conv2d_host_on_the_3x3_case_table(c):
    rng = np.random.default_rng(c)
    k = rng.standard_normal((c, c, 3, 3))
    for (h, w), stride in [(s, st) for s in U.CONV3_SIZES for st in (1, 2)]:
        x = rng.standard_normal((U.N_IMAGES, c, h, w))
        want = F.conv2d(torch.from_numpy(x), torch.from_numpy(k), stride=stride, padding=1).numpy()
        got = H.conv2d_host(x, k, stride, 1)
        assert got.shape == want.shape and U.err(got, want) <= 1e-12, (c, h, w, stride)


def test_the_stem_case_table_names_the_kernels_tile():
    """The last stem case is one pooled pixel past whole tiles in each dimension -- of the tile the kernel really has."""
    th, tw = U.STEM_TILE
    src = open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "conv2d.hip")).read()
    assert f"kStemTH = {th}, kStemTW = {tw}" in src
    N, Hh, W = U.STEM_CASES[-1]
    assert U.pooled(Hh) % th == 1 and U.pooled(W) % tw == 1 and U.pooled(Hh) > th and U.pooled(W) > tw


def test_the_nan_rule_of_the_specification_is_torchs():
    rng = np.random.default_rng(1)
    x, k = rng.standard_normal((1, 3, 40, 44)), rng.standard_normal((16, 3, 7, 7))
    k[3] = 0.0                                              # a zero weight does not hide a NaN
    for y, xx in ((0, 0), (0, 20), (17, 23)):
        bad = x.copy()
        bad[0, 1, y, xx] = np.nan
        want = F.max_pool2d(F.relu(F.conv2d(torch.from_numpy(bad), torch.from_numpy(k), stride=2, padding=3)), 3, 2, 1).numpy()
        got = H.max_pool_host(H.epilogue_host(H.conv2d_host(bad, k, 2, 3), relu=True))
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any() and not np.isnan(got).all()
        assert np.isnan(got[0, 3]).any()
    x3, k3 = rng.standard_normal((2, 16, 7, 9)), rng.standard_normal((16, 16, 3, 3))
    x3[1, 5, 3, 4] = np.nan
    got = H.epilogue_host(H.conv2d_host(x3, k3, 1, 1), relu=True)
    nan = np.isnan(got)
    assert nan[1, :, 2:5, 3:6].all() and nan.sum() == 16 * 9


# ------------------------------------------------------------------------------------------------------------------ state dict
def test_the_state_dict_is_the_manifest_and_round_trips_strictly():
    want = [(n, tuple(s)) for n, s in json.load(open(os.path.join(GOLDEN, "image_backbone_state_dict.json")))]
    with torch.device("meta"):
        shipped = MODELS.build(dict(U.SHIPPED))
    assert isinstance(shipped, ResNet) and MODELS.get("ResNet") is ResNet and MODELS.get("mmdet.ResNet") is ResNet
    got = [(n, tuple(t.shape)) for n, t in shipped.state_dict().items()]
    assert got == want
    blocks = sum(H.ARCH[50])
    assert len(want) == 6 + blocks * 18 + 4 * 6             # stem; three convolutions and BatchNorms per block; four downsamples
    assert ("conv1.weight", (16, 3, 7, 7)) in want and ("layer4.0.downsample.0.weight", (512, 256, 1, 1)) in want
    assert ("layer1.0.bn1.num_batches_tracked", ()) in want and ("layer3.5.conv2.weight", (64, 64, 3, 3)) in want
    assert not any(p.requires_grad for p in shipped.parameters()) and shipped.out_channels == [64, 128, 256, 512]
    a, b = U.build_backbone(seed=1), U.build_backbone(seed=2)
    rep = b.load_state_dict(a.state_dict(), strict=True)
    assert not rep.missing_keys and not rep.unexpected_keys
    assert all(torch.equal(t, b.state_dict()[n]) for n, t in a.state_dict().items())
    with pytest.raises(RuntimeError, match="layer2.0.conv2"):
        b.load_state_dict({k: v for k, v in a.state_dict().items() if k != "layer2.0.conv2.weight"})
    assert not b.train().bn1.training and not b.layer3[2].bn2.training          # norm_eval with everything frozen: both modes are one


@pytest.mark.parametrize("kw,word", [
    (dict(style="caffe"), "style"), (dict(deep_stem=True), "deep_stem"), (dict(avg_down=True), "avg_down"),
    (dict(dcn=dict(type="DCNv2")), "dcn"), (dict(plugins=[dict(cfg=dict(type="ContextBlock"))]), "plugins"),
    (dict(strides=(1, 2, 2, 1)), "strides"), (dict(strides=(2, 2, 2, 2)), "strides"), (dict(dilations=(1, 1, 2, 4)), "dilations"),
    (dict(depth=18), "depth"), (dict(depth=34), "depth"), (dict(in_channels=4), "in_channels"), (dict(conv_cfg=dict(type="ConvWS")), "conv_cfg"),
    (dict(norm_cfg=dict(type="GN", num_groups=32)), "norm_cfg"),
])
def test_every_rejected_keyword_raises_naming_itself(kw, word):
    cfg = dict(depth=50, base_channels=16)
    cfg.update(kw)
    with torch.device("meta"), pytest.raises(NotImplementedError, match=word):
        ResNet(**cfg)


def test_accepted_keywords_and_limits():
    with torch.device("meta"):
        net = ResNet(depth=152, base_channels=64, frozen_stages=4, norm_cfg=dict(type="BN", requires_grad=True), norm_eval=False,
                     init_cfg=dict(type="Pretrained", checkpoint="torchvision://resnet152"), with_cp=True, zero_init_residual=False)
        assert net.stage_blocks == (3, 8, 36, 3) and net.out_channels == [256, 512, 1024, 2048] and net.stem_channels == 64
        assert ResNet(depth=50, base_channels=32, stem_channels=48, num_stages=2, out_indices=(1,), strides=(1, 2), dilations=(1, 1)).out_channels == [256]
        for kw in (dict(base_channels=24), dict(base_channels=128), dict(stem_channels=8), dict(num_stages=5), dict(num_stages=0),
                   dict(out_indices=(0, 4)), dict(out_indices=()), dict(out_indices=(1, 0))):
            with pytest.raises(ValueError):
                ResNet(**dict(dict(depth=50, base_channels=16), **kw))
        with pytest.raises(KeyError):
            ResNet(depth=51)


def test_the_forward_checks_its_inputs_before_it_needs_a_device():
    net = U.build_backbone(num_stages=1, out_indices=(0,))
    for bad in (torch.zeros(3, 64, 64), torch.zeros(1, 4, 64, 64), torch.zeros(1, 3, 31, 64), torch.zeros(1, 3, 64, 2049),
                torch.zeros((1, 3, 64, 64), dtype=torch.float64), torch.zeros((0, 3, 64, 64))):
        with pytest.raises(ValueError):
            net(bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(1, 3, 64, 64))


# ------------------------------------------------------------------------------------------------------------------ the detector
BACKBONE = dict(U.SHIPPED)


def test_the_detector_without_a_backbone_is_what_it_was():
    from proxytransformation_amd import GroundingDetector
    det = GroundingDetector(**small_cfg())
    assert det.backbone is None and "backbone" not in dict(det.named_children())
    assert not any(k.startswith("backbone.") for k in det.state_dict())
    want = sorted((n, tuple(s)) for n, s in json.load(open(os.path.join(GOLDEN, "grounder_state_dict.json"))))
    cfg = small_cfg(num_queries=256, text_width=768)
    cfg["preshape"] = dict(type="ProxyTransformationNormReverse", n_points=100000, grid_size=12, text_blocks=3, img_blocks=3,
                           dynamic_drop_radio=0.6, num_sub=30)
    cfg["backbone_3d"]["depth"] = 34
    cfg["neck_3d"]["pts_prune_threshold"] = 1000
    cfg["decoder"]["num_layers"] = 6
    cfg["decoder"]["layer_cfg"]["ffn_cfg"]["feedforward_channels"] = 2048
    shipped = GroundingDetector(**cfg)
    assert sorted((n, tuple(t.shape)) for n, t in shipped.reference_state_dict().items()) == want
    rep = det.load_reference_state_dict(dict(det.reference_state_dict(), **{"backbone.conv1.weight": torch.ones(2)}))
    assert rep == dict(skipped=["backbone.conv1.weight"], missing=[], unexpected=[])
    with pytest.raises(ValueError, match="backbone"):
        det.predict([torch.zeros(8, 3)], torch.zeros(1, 4, 128), torch.ones(1, 4, dtype=torch.bool), scenes=[{}], imgs=torch.zeros(1, 1, 3, 32, 32))
    with pytest.raises(ValueError, match="backbone="):
        GroundingDetector(**small_cfg(pixel_mean=U.MEAN, pixel_std=U.STD))


def test_the_detector_with_a_backbone_holds_it_and_loads_it():
    from proxytransformation_amd import GroundingDetector
    det = GroundingDetector(**small_cfg(backbone=dict(BACKBONE), pixel_mean=U.MEAN, pixel_std=U.STD, bgr_to_rgb=True))
    assert isinstance(det.backbone, ResNet) and det.pixel_mean == U.MEAN and det.bgr_to_rgb
    assert isinstance(GroundingDetector(**small_cfg(backbone=U.build_backbone())).backbone, ResNet)
    manifest = json.load(open(os.path.join(GOLDEN, "image_backbone_state_dict.json")))
    ref = {k: v.clone() for k, v in det.reference_state_dict().items()}
    names = [k for k in ref if k.startswith("backbone.")]
    assert sorted(names) == sorted("backbone." + n for n, _ in manifest) and len(names) == len(manifest)
    torch.manual_seed(1)
    new = {k: (torch.rand_like(v) + 0.5 if k in names and v.is_floating_point() else v) for k, v in ref.items()}
    rep = det.load_reference_state_dict(dict(new, **{"text_encoder.text_model.final_layer_norm.weight": torch.ones(4)}))
    assert rep == dict(skipped=["text_encoder.text_model.final_layer_norm.weight"], missing=[], unexpected=[])
    assert all(torch.equal(det.state_dict()[k], new[k]) for k in names)
    with pytest.raises(KeyError, match="backbone.conv1.weight"):
        det.load_reference_state_dict({k: v for k, v in ref.items() if k != "backbone.conv1.weight"})
    with pytest.raises(ValueError, match="levels"):
        GroundingDetector(**small_cfg(backbone=dict(BACKBONE, out_indices=(0, 1, 2))))
    with pytest.raises(TypeError, match="backbone"):
        GroundingDetector(**small_cfg(backbone=torch.nn.Identity()))
    text, mask = torch.zeros(1, 4, 128), torch.ones(1, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="one of them"):
        det.predict([torch.zeros(8, 3)], text, mask, [torch.zeros(1)], [{}], imgs=torch.zeros(1, 1, 3, 32, 32))
    with pytest.raises(ValueError, match="required"):
        det.predict([torch.zeros(8, 3)], text, mask, scenes=[{}])
    with pytest.raises(ValueError, match="B,V,3,H,W"):
        det.predict([torch.zeros(8, 3)], text, mask, scenes=[{}], imgs=torch.zeros(1, 3, 32, 32))


def test_the_detector_host_chain_takes_imgs_in_place_of_the_features():
    from oracle import oracle
    x = inputs()
    det = make_detector(backbone=dict(BACKBONE)).eval()
    U.seed_backbone(det.backbone, gain=0.5)                 # levels of a scale near 1, like the features of inputs()
    imgs = U.make_images((2, 3, 3, 96, 96))
    feats = det.backbone.forward_host(imgs)
    assert [f.shape for f in feats] == [tuple(f.shape) for f in x["img"]]          # 24 / 12 / 6 / 3, as inputs() has them
    kw = dict(scenes=x["scenes"], host=oracle)
    got = det.forward_host(x["points"], x["text"], x["mask"], imgs=imgs, **kw)
    want = det.forward_host(x["points"], x["text"], x["mask"], feats, img_pad_shape=(96, 96), **kw)
    for k in ("bboxes_3d", "scores_3d", "all_layers_cls_scores", "hidden_states"):
        assert np.array_equal(got[k], want[k]), k
    assert np.isfinite(got["bboxes_3d"]).all() and np.isfinite(got["hidden_states"]).all()
    with pytest.raises(ValueError, match="one of them"):
        det.forward_host(x["points"], x["text"], x["mask"], feats, imgs=imgs, **kw)
    with pytest.raises(ValueError, match="required"):
        det.forward_host(x["points"], x["text"], x["mask"], **kw)


# ------------------------------------------------------------------------------------------------------------------ ABI surface
def test_header_bindings_and_export_table_agree_for_the_convolutions_and_the_abi_is_still_13():
    assert _abi.ABI_VERSION == 13 and _abi.lib().ptx_abi_version() == 13
    params = assert_declared(NAMES)
    for name in NAMES:
        res, args = _abi.SIGNATURES[name]
        assert len(args) == len([a for a in params[name].replace("\n", " ").split(",") if a.strip()]), name
        assert res is ctypes.c_int, name
    assert "conv2d.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()
    header = open(os.path.join(ROOT, "include", "proxyt.h")).read()
    assert "((float)x - mean[c]) / std[c]" in header        # the expression the uint8 path is bit-pinned to


def test_the_entry_points_refuse_on_the_host_before_anything_is_enqueued():
    """Every refusal returns PTX_EINVAL with the argument in the message; the device pointers are never read (they are fakes)."""
    lib, f = _abi.lib(), 0x1000
    said = lambda: lib.ptx_last_error().decode()      # noqa: E731
    for kw, word in U.STEM_REFUSALS:
        a = dict(U.STEM_OK)
        a.update(kw)
        rc = lib.ptx_conv_stem(f, a["dtype"], a["N"], a["H"], a["W"], f, a["C0"], f, f, a["relu"], f, f if a["std"] else None, f, None)
        assert rc == PTX_EINVAL and word in said(), (kw, said())
    for kw, word in U.CONV1_REFUSALS:
        a = dict(U.CONV1_OK)
        a.update(kw)
        rc = lib.ptx_conv1x1(f, a["N"], a["Cin"], a["H"], a["W"], f, a["Cout"], a["stride"], f, f, None, a["relu"], 2 * f, None)
        assert rc == PTX_EINVAL and word in said(), (kw, said())
    for kw, word in U.CONV3_REFUSALS:
        a = dict(U.CONV3_OK)
        a.update(kw)
        rc = lib.ptx_conv3x3(f, a["N"], a["C"], a["H"], a["W"], f, a["stride"], f, f, None, a["relu"], 2 * f, None)
        assert rc == PTX_EINVAL and word in said(), (kw, said())
    assert lib.ptx_conv1x1(f, 1, 16, 4, 4, f, 16, 1, None, None, None, 0, f, None) == PTX_EINVAL and "must not be x" in said()
    assert lib.ptx_conv1x1(f + 4, 1, 16, 4, 4, f, 16, 1, None, None, None, 0, 2 * f, None) == PTX_EINVAL and "aligned" in said()
    assert lib.ptx_conv3x3(f, 1, 16, 4, 4, None, 1, None, None, None, 0, 2 * f, None) == PTX_EINVAL and "null" in said()


def test_the_detector_builds_this_packages_resnet_whatever_holds_the_name_in_the_registry(monkeypatch):
    from proxytransformation_amd import GroundingDetector, detector
    monkeypatch.setattr(detector.MODELS, "get", lambda key: torch.nn.Identity)          # as where mmdet's own class is registered
    assert isinstance(GroundingDetector(**small_cfg(backbone=dict(BACKBONE))).backbone, ResNet)
    assert isinstance(GroundingDetector(**small_cfg(backbone=dict(BACKBONE, type="ResNet"))).backbone, ResNet)
