"""The image backbone on the device: the three kernels of csrc/conv2d.hip one by one through the C ABI, ``image_backbone.ResNet`` against its
numpy specification, and ``GroundingDetector`` with it.

Kernels: integer operands (inputs in [-4, 4], weights in [-2, 2], scale in {1, 2}, integer shift and residual; the worst |sum| is
512 x 9 x 8 < 2^24), so torch's float64 ``F.conv2d`` / ``F.max_pool2d`` is the exact answer and the comparison is ``torch.equal``.  Every
output lies between sentinel rows that must stay untouched.

Module: with err(t) = max|t - f64| / max|f64| against ``forward_host(float64)``, every level must satisfy err <= 4 x err of
``forward_host(float32)`` -- the rule of tests/test_gpu_detector.py and tests/test_gpu_text_encoder.py, unchanged (the float32 chain's
own error is 3.2e-7 .. 8.9e-7 of a level's scale).  The ratios are printed here; tools/image_backbone_time.py computes the same ratios on
the same cases and writes them to profiles/image_backbone.txt.  Structure, bit for
bit: two calls, ``chunk``, an image alone and as the last of five, ``(B,V,...)`` against the flattened call, uint8 with mean / std
against the float call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import _abi
from tests import image_backbone_util as U
from tests.detector_util import inputs, make_detector

pytestmark = pytest.mark.gpu

MARGIN = 4.0
PTX_EINVAL = -1


def _ptr(t):
    return None if t is None else t.data_ptr()


def _cuda(*ts):
    return [None if t is None else t.cuda().contiguous() for t in ts]


def run_stem(x, w, scale=None, shift=None, relu=True, mean=None, std=None):
    """``ptx_conv_stem`` on CPU operands (``w`` as torch spells it); returns the output on the CPU, the guards checked."""
    N, _, H, W = x.shape
    C0 = w.shape[0]
    xd, wd, sc, sh, md, sd = _cuda(x, U.stem_weight_operand(w), scale, shift, mean, std)
    g = U.Guarded((N, C0, U.pooled(H), U.pooled(W)))
    rc = _abi.lib().ptx_conv_stem(xd.data_ptr(), 1 if x.dtype == torch.uint8 else 0, N, H, W, wd.data_ptr(), C0, _ptr(sc), _ptr(sh), int(relu),
                                  _ptr(md), _ptr(sd), g.out.data_ptr(), None)
    _abi.check(rc, "ptx_conv_stem")
    torch.cuda.synchronize()
    assert g.guards_untouched()
    return g.out.cpu()


def run_conv1(x, w, stride=1, scale=None, shift=None, residual=None, relu=False):
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    xd, wd, sc, sh, rd = _cuda(x, w.reshape(Cout, Cin), scale, shift, residual)
    g = U.Guarded((N, Cout, U.out_side(H, stride), U.out_side(W, stride)))
    rc = _abi.lib().ptx_conv1x1(xd.data_ptr(), N, Cin, H, W, wd.data_ptr(), Cout, stride, _ptr(sc), _ptr(sh), _ptr(rd), int(relu),
                                g.out.data_ptr(), None)
    _abi.check(rc, "ptx_conv1x1")
    torch.cuda.synchronize()
    assert g.guards_untouched()
    return g.out.cpu()


def run_conv3(x, w, stride=1, scale=None, shift=None, residual=None, relu=False):
    N, C, H, W = x.shape
    xd, wd, sc, sh, rd = _cuda(x, U.conv3_weight_operand(w), scale, shift, residual)
    g = U.Guarded((N, C, U.out_side(H, stride), U.out_side(W, stride)))
    rc = _abi.lib().ptx_conv3x3(xd.data_ptr(), N, C, H, W, wd.data_ptr(), stride, _ptr(sc), _ptr(sh), _ptr(rd), int(relu), g.out.data_ptr(), None)
    _abi.check(rc, "ptx_conv3x3")
    torch.cuda.synchronize()
    assert g.guards_untouched()
    return g.out.cpu()


def _exact(got, want, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), what
    assert torch.equal(got.double(), want), (what, float((got.double() - want).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ the stem
@pytest.mark.parametrize("case", U.STEM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_is_exact_on_integer_operands(case):
    N, H, W = case
    rng = np.random.default_rng(N * 10000 + H * 100 + W)
    for C0 in U.STEM_C0:
        x, w = U.ints(rng, (N, 3, H, W), -4, 4), U.ints(rng, (C0, 3, 7, 7), -2, 2)
        scale, shift, _ = U.epilogue_operands(rng, C0, None, True, False)
        _exact(run_stem(x, w, scale, shift), U.stem_torch(x, w, scale, shift), (case, C0))
    _exact(run_stem(x, w, None, None, relu=False), U.stem_torch(x, w, None, None, relu=False), (case, "bare"))


def test_stem_uint8_with_mean_and_std_is_the_float_path_on_the_normalised_pixels():
    rng = np.random.default_rng(7)
    N, H, W, C0 = 2, 45, 70, 32
    x8 = torch.from_numpy(rng.integers(0, 256, size=(N, 3, H, W)).astype(np.uint8))
    w = torch.from_numpy(rng.standard_normal((C0, 3, 7, 7)).astype(np.float32) * 0.1)
    scale, shift = torch.from_numpy(rng.random(C0).astype(np.float32) + 0.5), torch.from_numpy(rng.standard_normal(C0).astype(np.float32))
    mean, std = torch.tensor(U.MEAN), torch.tensor(U.STD)
    xn = (x8.float() - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)          # float32, the header's expression
    a = run_stem(x8, w, scale, shift, mean=mean, std=std)
    b = run_stem(xn, w, scale, shift)
    c = run_stem(x8.float(), w, scale, shift, mean=mean, std=std)
    assert torch.equal(a, b) and torch.equal(a, c)
    want = U.stem_torch(xn, w, scale, shift)
    assert U.err(a.numpy(), want.numpy()) <= 1e-5 and float(want.abs().max()) > 1.0


def test_stem_all_ones_counts_the_valid_taps():
    for N, H, W in ((1, 32, 32), (1, 33, 47), (1, 49, 65)):
        x, w = torch.ones(N, 3, H, W), torch.ones(16, 3, 7, 7)
        got = run_stem(x, w)
        _exact(got, U.stem_torch(x, w, None, None), (H, W))
        assert float(got.max()) == 147.0 and float(got[0, 0, 0, 0]) == 3 * 6 * 6          # the corner's best window is cut by one row and one column


def test_stem_nan_set_is_torchs():
    rng = np.random.default_rng(9)
    N, H, W, C0 = 2, 49, 65, 16
    x, w = U.ints(rng, (N, 3, H, W), -4, 4), U.ints(rng, (C0, 3, 7, 7), -2, 2)
    w[5] = 0.0                                              # a zero weight does not hide a NaN
    clean = run_stem(x, w)
    for n, c, y, xx in ((0, 0, 0, 0), (1, 2, H - 1, W - 1), (0, 1, 0, 31), (1, 0, 24, W - 1), (0, 2, 23, 37)):
        bad = x.clone()
        bad[n, c, y, xx] = float("nan")
        got, want = run_stem(bad, w), U.stem_torch(bad, w, None, None)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.isnan(got).any(), (n, c, y, xx)
        keep = ~torch.isnan(want)
        assert torch.equal(got[keep], clean[keep])
        assert not torch.isnan(got[1 - n]).any()


# ------------------------------------------------------------------------------------------------------------------ 1x1
@pytest.mark.parametrize("channels", U.CONV1_CHANNELS, ids=lambda c: "x".join(map(str, c)))
def test_conv1x1_is_exact_on_integer_operands(channels):
    cin, cout = channels
    rng = np.random.default_rng(cin * 4096 + cout)
    w = U.ints(rng, (cout, cin, 1, 1), -2, 2)
    for H, W in U.CONV1_SIZES:
        x = U.ints(rng, (U.N_IMAGES, cin, H, W), -4, 4)
        scale, shift, res = U.epilogue_operands(rng, cout, (U.N_IMAGES, cout, H, W), True, True)
        want = U.epilogue_torch(F.conv2d(x.double(), w.double()), scale, shift, res, True)
        _exact(run_conv1(x, w, 1, scale, shift, res, True), want, (channels, H, W))
    for H, W in U.CONV1_STRIDED:
        x = U.ints(rng, (U.N_IMAGES, cin, H, W), -4, 4)
        want = F.conv2d(x.double(), w.double(), stride=2)
        assert tuple(want.shape[2:]) == (U.out_side(H, 2), U.out_side(W, 2))
        _exact(run_conv1(x, w, 2), want, (channels, H, W, "stride 2"))


@pytest.mark.parametrize("epilogue", U.EPILOGUES, ids=lambda e: "".join("sSrRaA"[2 * i + int(v)] for i, v in enumerate(e)))
def test_conv1x1_every_epilogue_subset(epilogue):
    scale_shift, residual, relu = epilogue
    rng = np.random.default_rng(3)
    cin, cout = 80, 48
    for (H, W), stride in (((7, 9), 1), ((5, 7), 2)):
        x, w = U.ints(rng, (U.N_IMAGES, cin, H, W), -4, 4), U.ints(rng, (cout, cin, 1, 1), -2, 2)
        shape = (U.N_IMAGES, cout, U.out_side(H, stride), U.out_side(W, stride))
        scale, shift, res = U.epilogue_operands(rng, cout, shape, scale_shift, residual)
        want = U.epilogue_torch(F.conv2d(x.double(), w.double(), stride=stride), scale, shift, res, relu)
        assert relu or bool((want < 0).any())
        _exact(run_conv1(x, w, stride, scale, shift, res, relu), want, (epilogue, stride))


def test_conv1x1_nan_reaches_its_own_pixel_only():
    rng = np.random.default_rng(4)
    x, w = U.ints(rng, (U.N_IMAGES, 32, 7, 9), -4, 4), U.ints(rng, (48, 32, 1, 1), -2, 2)
    w[7] = 0.0
    x[1, 5, 3, 4] = float("nan")
    got = run_conv1(x, w, relu=True)
    nan = torch.isnan(got)
    assert nan[1, :, 3, 4].all() and int(nan.sum()) == 48
    want = F.relu(F.conv2d(x.double(), w.double()))
    assert torch.equal(nan, torch.isnan(want)) and torch.equal(got[~nan].double(), want[~nan])


# ------------------------------------------------------------------------------------------------------------------ 3x3
@pytest.mark.parametrize("C", U.CONV3_CHANNELS)
def test_conv3x3_is_exact_on_integer_operands(C):
    rng = np.random.default_rng(C)
    w = U.ints(rng, (C, C, 3, 3), -2, 2)
    for H, W in U.CONV3_SIZES:
        for stride in (1, 2):
            x = U.ints(rng, (U.N_IMAGES, C, H, W), -4, 4)
            shape = (U.N_IMAGES, C, U.out_side(H, stride), U.out_side(W, stride))
            scale, shift, res = U.epilogue_operands(rng, C, shape, True, True)
            want = U.epilogue_torch(F.conv2d(x.double(), w.double(), stride=stride, padding=1), scale, shift, res, True)
            _exact(run_conv3(x, w, stride, scale, shift, res, True), want, (C, H, W, stride))
    x = U.ints(rng, (U.N_IMAGES, C, 7, 9), -4, 4)
    _exact(run_conv3(x, w), F.conv2d(x.double(), w.double(), padding=1), (C, "bare"))


def test_conv3x3_all_ones_counts_the_valid_taps():
    for (H, W), stride in (((7, 9), 1), ((7, 9), 2), ((24, 24), 2), ((1, 1), 1), ((2, 3), 1)):
        x, w = torch.ones(U.N_IMAGES, 16, H, W), torch.ones(16, 16, 3, 3)
        got = run_conv3(x, w, stride)
        _exact(got, F.conv2d(x.double(), w.double(), stride=stride, padding=1), (H, W, stride))
        assert float(got[0, 0, 0, 0]) == 16 * min(H, 2) * min(W, 2)


def test_conv3x3_nan_spreads_to_its_neighbourhood_and_no_further():
    rng = np.random.default_rng(5)
    x, w = U.ints(rng, (U.N_IMAGES, 16, 7, 9), -4, 4), U.ints(rng, (16, 16, 3, 3), -2, 2)
    w[3] = 0.0
    x[1, 5, 3, 4] = float("nan")
    x[2, 0, 0, 8] = float("nan")
    got = run_conv3(x, w, relu=True)
    nan = torch.isnan(got)
    assert nan[1, :, 2:5, 3:6].all() and nan[2, :, 0:2, 7:9].all() and int(nan.sum()) == 16 * (9 + 4) and not nan[0].any()
    assert torch.equal(nan, torch.isnan(F.relu(F.conv2d(x.double(), w.double(), padding=1))))
    got2 = run_conv3(x, w, 2, relu=True)
    assert torch.equal(torch.isnan(got2), torch.isnan(F.relu(F.conv2d(x.double(), w.double(), stride=2, padding=1))))


# ------------------------------------------------------------------------------------------------------------------ argument limits
def test_out_of_range_arguments_return_the_error_and_launch_nothing():
    lib = _abi.lib()
    said = lambda: lib.ptx_last_error().decode()      # noqa: E731
    big = torch.zeros(1 << 20, device="cuda")
    g = U.Guarded((1 << 16,))
    for kw, word in U.STEM_REFUSALS:
        a = dict(U.STEM_OK)
        a.update(kw)
        rc = lib.ptx_conv_stem(big.data_ptr(), a["dtype"], a["N"], a["H"], a["W"], big.data_ptr(), a["C0"], big.data_ptr(), big.data_ptr(),
                               a["relu"], big.data_ptr(), big.data_ptr() if a["std"] else None, g.out.data_ptr(), None)
        assert rc == PTX_EINVAL and word in said(), (kw, said())
    for kw, word in U.CONV1_REFUSALS:
        a = dict(U.CONV1_OK)
        a.update(kw)
        rc = lib.ptx_conv1x1(big.data_ptr(), a["N"], a["Cin"], a["H"], a["W"], big.data_ptr(), a["Cout"], a["stride"], big.data_ptr(),
                             big.data_ptr(), None, a["relu"], g.out.data_ptr(), None)
        assert rc == PTX_EINVAL and word in said(), (kw, said())
    for kw, word in U.CONV3_REFUSALS:
        a = dict(U.CONV3_OK)
        a.update(kw)
        rc = lib.ptx_conv3x3(big.data_ptr(), a["N"], a["C"], a["H"], a["W"], big.data_ptr(), a["stride"], big.data_ptr(), big.data_ptr(), None,
                             a["relu"], g.out.data_ptr(), None)
        assert rc == PTX_EINVAL and word in said(), (kw, said())
    torch.cuda.synchronize()
    assert g.untouched()


# ------------------------------------------------------------------------------------------------------------------ the module
def _held(name, dev, f32, f64):
    worst = 0.0
    for l, (d, s, w) in enumerate(zip(dev, f32, f64)):
        d = d.cpu().numpy()
        ed, e32 = U.err(d, w), U.err(s, w)
        print(f"{name} level {l}: device {ed:.3e}, float32 chain {e32:.3e}, ratio {ed / e32:.2f}")
        assert d.shape == w.shape and np.isfinite(d).all() and ed <= MARGIN * e32, (name, l, ed, e32)
        worst = max(worst, ed / e32)
    return worst


@pytest.mark.parametrize("case", sorted(U.MODULE_CASES))
def test_device_against_forward_host_float64(case):
    ref = U.reference(case)
    net = ref["net"].cuda()
    out = net(ref["imgs"].cuda())
    assert all(o.dtype == torch.float32 and o.grad_fn is None and not o.requires_grad for o in out)
    _held(case, out, ref["f32"], ref["f64"])
    net.cpu()


@pytest.fixture(scope="module")
def small():
    net = U.build_backbone().cuda()
    imgs = U.make_images((5, 3, 64, 80)).cuda()
    return dict(net=net, imgs=imgs, out=net(imgs))


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def test_two_calls_chunks_and_an_images_place_in_the_batch_give_equal_bits(small):
    net, imgs, out = small["net"], small["imgs"], small["out"]
    assert [tuple(o.shape) for o in out] == [(5, 64, 16, 20), (5, 128, 8, 10), (5, 256, 4, 5), (5, 512, 2, 3)]
    assert _same(net(imgs), out)
    assert _same(net(imgs, chunk=1), out) and _same(net(imgs, chunk=2), out) and _same(net(imgs, chunk=None), out)
    alone = net(imgs[4:5])
    assert all(torch.equal(a[0], o[4]) for a, o in zip(alone, out))
    x = imgs.requires_grad_(True)
    got = net.train()(x)
    assert _same(got, out) and all(not o.requires_grad for o in got) and x.grad is None
    net.eval()
    imgs.requires_grad_(False)
    with pytest.raises(ValueError, match="chunk"):
        net(imgs, chunk=0)


def test_leading_dimensions_and_uint8_with_mean_and_std(small):
    net = small["net"]
    x8 = torch.randint(0, 256, (2, 3, 3, 40, 36), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    out = net(x8, mean=U.MEAN, std=U.STD)
    flat = net(x8.reshape(6, 3, 40, 36), mean=U.MEAN, std=U.STD)
    assert all(tuple(o.shape) == (2, 3) + tuple(f.shape[1:]) and torch.equal(o.reshape(f.shape), f) for o, f in zip(out, flat))
    mean, std = torch.tensor(U.MEAN, device="cuda").view(1, 1, 3, 1, 1), torch.tensor(U.STD, device="cuda").view(1, 1, 3, 1, 1)
    assert _same(net((x8.float() - mean) / std), out)
    assert _same(net(x8.float(), mean=torch.tensor(U.MEAN), std=np.asarray(U.STD)), out)
    _held("uint8", out, net.forward_host(x8, np.float32, U.MEAN, U.STD), net.forward_host(x8, np.float64, U.MEAN, U.STD))
    swapped = net(x8.flip(2), mean=U.MEAN, std=U.STD, bgr_to_rgb=True)          # the same products in another order
    _held("bgr", swapped, net.forward_host(x8, np.float32, U.MEAN, U.STD), net.forward_host(x8, np.float64, U.MEAN, U.STD))


def test_prepared_operands_follow_the_parameters(small):
    imgs, out = small["imgs"], small["out"]
    net = U.build_backbone().cuda()
    assert _same(net(imgs), out)
    net.load_state_dict(U.build_backbone(seed=1).state_dict())
    got = net(imgs)
    assert not torch.equal(got[0], out[0])
    _held("after load_state_dict", got, net.forward_host(imgs, np.float32), net.forward_host(imgs))
    with torch.no_grad():
        net.bn1.running_var.mul_(2.0)                       # a buffer, in place
    assert not torch.equal(net(imgs)[0], got[0])


# ------------------------------------------------------------------------------------------------------------------ the detector
@pytest.fixture(scope="module")
def world():
    x = inputs("cuda")
    det = make_detector(differentiable=True, backbone=dict(U.SHIPPED))
    U.seed_backbone(det.backbone, gain=0.5)                 # levels of a scale near 1, like the features of inputs()
    imgs = U.make_images((2, 3, 3, 96, 96)).cuda()
    return dict(x=x, det=det.cuda(), imgs=imgs)


def test_predict_takes_imgs_in_place_of_the_features(world):
    x, det, imgs = world["x"], world["det"].eval(), world["imgs"]
    got = det.predict(x["points"], x["text"], x["mask"], scenes=x["scenes"], imgs=imgs)          # img_pad_shape: the images' (96, 96)
    feats = det.extract_image_features(imgs)
    assert [tuple(f.shape) for f in feats] == [tuple(f.shape) for f in x["img"]]
    assert _same(feats, det.backbone(imgs))
    want = det.predict(x["points"], x["text"], x["mask"], feats, x["scenes"], img_pad_shape=(96, 96))
    for g, w in zip(got, want):
        assert g.keys() == w.keys() and all(torch.equal(g[k], w[k]) for k in g)
        assert torch.isfinite(g["bboxes_3d"]).all()
    with pytest.raises(ValueError, match="one of them"):
        det.predict(x["points"], x["text"], x["mask"], feats, x["scenes"], imgs=imgs)


def test_loss_takes_imgs_and_the_backbone_receives_no_gradient(world):
    x, det, imgs = world["x"], world["det"].train(), world["imgs"]
    got = det.loss(x["points"], x["text"], x["mask"], scenes=x["scenes"], gt_bboxes=x["gt"], positive_maps=x["pos"], imgs=imgs)
    sum(got.values()).backward()
    assert all(p.grad is None and not p.requires_grad for p in det.backbone.parameters())
    assert det.text_feat_map.weight.grad is not None and det.text_feat_map.weight.grad.abs().sum() > 0
    want = det.loss(x["points"], x["text"], x["mask"], det.extract_image_features(imgs), x["scenes"], x["gt"], x["pos"], img_pad_shape=(96, 96))
    assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) and torch.isfinite(got[k]) for k in got)
    det.zero_grad(set_to_none=True)


def test_reference_checkpoint_round_trip_with_the_backbone(world):
    x, det, imgs = world["x"], world["det"].eval(), world["imgs"]
    sd = {k: v.detach().clone() for k, v in det.reference_state_dict().items()}
    assert sum(k.startswith("backbone.") for k in sd) == len(det.backbone.state_dict())
    other = make_detector(differentiable=True, backbone=dict(U.SHIPPED)).cuda().eval()
    rep = other.load_reference_state_dict(sd)
    assert not rep["skipped"] and not rep["missing"] and not rep["unexpected"]
    kw = dict(scenes=x["scenes"], imgs=imgs)
    for g, w in zip(other.predict(x["points"], x["text"], x["mask"], **kw), det.predict(x["points"], x["text"], x["mask"], **kw)):
        assert all(torch.equal(g[k], w[k]) for k in g)


def test_a_detector_without_a_backbone_has_the_keys_it_had():
    with_b, without = make_detector(backbone=dict(U.SHIPPED)), make_detector()
    keys = set(without.state_dict())
    assert not any(k.startswith("backbone.") for k in keys) and without.backbone is None
    assert {k for k in with_b.state_dict() if not k.startswith("backbone.")} == keys
