"""The image backbone's backward without a GPU: the numpy specification (``image_backbone_grad_host``) against torch's float64 autograd,
``ResNet(differentiable=...)``'s constructor, and the two plan functions of the C ABI, which answer without a device.

Bound: 1e-12 of each tensor's scale, the bound tests/test_image_backbone_host.py uses for the forward's float64 chain."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import ResNet, _abi
from proxytransformation_amd import image_backbone_grad_host as H
from tests import image_backbone_util as U
from tests.util import header_prototypes

BOUND = 1e-12
PTX_EINVAL = -1
CASES = [(1, 32, 48, hw, 1) for hw in U.CONV1_SIZES] + [(1, 32, 48, hw, 2) for hw in U.CONV1_STRIDED + ((7, 9), (8, 8))] + \
    [(3, 16, 16, hw, s) for hw in U.CONV3_SIZES for s in (1, 2)]


def _held(got, want, what):
    assert got.shape == want.shape, what
    assert np.abs(got - want).max() <= BOUND * max(np.abs(want).max(), 1e-300), (what, np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "k{}-{}to{}-{}x{}-s{}".format(c[0], c[1], c[2], c[3][0], c[3][1], c[4]))
def test_conv_bwd_host_is_torchs_autograd_for_every_epilogue(case):
    KS, cin, cout, (Hh, Ww), stride = case
    gen = torch.Generator().manual_seed(KS * 1000 + Hh * 10 + Ww + stride)
    rnd = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)      # noqa: E731
    N = U.N_IMAGES
    for scale, residual, relu in U.EPILOGUES:
        x, w = rnd(N, cin, Hh, Ww).requires_grad_(), rnd(cout, cin, KS, KS).requires_grad_()
        v = F.conv2d(x, w, stride=stride, padding=KS // 2)
        bn = [rnd(cout), 1.0 + torch.rand(cout, generator=gen, dtype=torch.float64), rnd(cout), rnd(cout)]      # mean, var, weight, bias
        if scale:
            v = F.batch_norm(v, bn[0], bn[1], bn[2], bn[3], False, 0.0, U.EPS)
        res = rnd(*v.shape).requires_grad_()
        if residual:
            v = v + res
        out = F.relu(v) if relu else v
        g = rnd(*out.shape)
        dx, dw = torch.autograd.grad(out, (x, w), g, retain_graph=True)
        folded = (bn[2] / torch.sqrt(bn[1] + U.EPS)).numpy() if scale else None
        gz, dres, hx, hw = H.conv_bwd_host(g.numpy(), out.detach().numpy(), folded, relu, x.detach().numpy(), w.detach().numpy(), stride, KS // 2)
        what = (case, scale, residual, relu)
        _held(hx, dx.numpy(), what + ("dx",))
        _held(hw, dw.numpy(), what + ("dweight",))
        if residual:
            _held(dres, torch.autograd.grad(out, res, g)[0].numpy(), what + ("dresidual",))
        held = rnd(N, cin, Hh, Ww).numpy()
        assert np.array_equal(H.conv_bwd_host(g.numpy(), out.detach().numpy(), folded, relu, x.detach().numpy(), w.detach().numpy(), stride,
                                              KS // 2, dx_held=held)[2], hx + held)


def _torch_grads(net, imgs, grads):
    """The kernels' gradients from torch's own functions in float64 (tests/image_backbone_util.torch_levels' composition, under autograd)."""
    sd = {k: v.detach().double() for k, v in net.state_dict().items() if v.is_floating_point()}
    names = H.trainable_kernels(net.stage_blocks[:net.out_indices[-1] + 1], net.frozen_stages)
    for n in names:
        sd[n].requires_grad_()
    bn = lambda x, p: F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, U.EPS)   # noqa: E731
    x = F.max_pool2d(F.relu(bn(F.conv2d(imgs.double(), sd["conv1.weight"], stride=2, padding=3), "bn1")), 3, 2, 1)
    outs = []
    for s, nb in enumerate(net.stage_blocks[:net.out_indices[-1] + 1]):
        for b in range(nb):
            p = f"layer{s + 1}.{b}."
            stride = 2 if (b == 0 and s > 0) else 1
            identity = x
            if p + "downsample.0.weight" in sd:
                identity = bn(F.conv2d(x, sd[p + "downsample.0.weight"], stride=stride), p + "downsample.1")
            y = F.relu(bn(F.conv2d(x, sd[p + "conv1.weight"]), p + "bn1"))
            y = F.relu(bn(F.conv2d(y, sd[p + "conv2.weight"], stride=stride, padding=1), p + "bn2"))
            x = F.relu(bn(F.conv2d(y, sd[p + "conv3.weight"]), p + "bn3") + identity)
        if s in net.out_indices:
            outs.append(x)
    attached = [(o, g.double()) for o, g in zip(outs, grads) if o.requires_grad]
    got = torch.autograd.grad([o for o, _ in attached], [sd[n] for n in names], [g for _, g in attached])
    return {n: t.numpy() for n, t in zip(names, got)}, [tuple(o.shape) for o in outs]


@pytest.mark.parametrize("kw,shape", [({}, (2, 3, 64, 80)), (dict(U.DEEP, frozen_stages=1), (1, 3, 64, 64))], ids=["shipped", "deep"])
def test_resnet_grad_host_is_torchs_autograd(kw, shape):
    net = U.build_backbone(differentiable=True, **kw)
    imgs = U.make_images(shape)
    gen = torch.Generator().manual_seed(3)
    shapes = [(shape[0], c, h, w) for s, (c, h, w) in enumerate(net.level_shapes(*shape[-2:])) if s in net.out_indices]
    grads = [torch.randn(s, generator=gen) for s in shapes]
    want, level_shapes = _torch_grads(net, imgs, grads)
    assert level_shapes == shapes
    got = net.grad_host(imgs, grads, np.float64)
    assert sorted(got) == sorted(want) and got
    assert not any(".bn" in n or "downsample.1" in n or n.startswith(("conv1", "bn1", "layer1.")) for n in got)      # frozen: no entry
    for n in want:
        _held(got[n], want[n], n)
    # the float32 chain follows (its masks replayed from the float64 forward would be the device test's business)
    f32 = net.grad_host(imgs, grads, np.float32)
    assert all(f32[n].dtype == np.float32 and U.err(f32[n], want[n]) < 1e-3 for n in want)


def test_masks_from_outside_take_the_place_of_the_forwards_signs():
    net = U.build_backbone(differentiable=True)
    imgs = U.make_images((1, 3, 64, 64))
    grads = [np.ones((1, c, h, w)) for c, h, w in net.level_shapes(64, 64)]
    params = {k: v.numpy() for k, v in net.state_dict().items()}
    x = imgs.numpy().astype(np.float64)
    own = net.grad_host(imgs, grads, np.float64)
    masks = {}
    from proxytransformation_amd import image_backbone_host as FH
    x = FH.max_pool_host(FH.epilogue_host(FH.conv2d_host(x, params["conv1.weight"].astype(np.float64), 2, 3), *FH._fold(params, "bn1", np.float64),
                                          relu=True))
    for s, nb in enumerate(net.stage_blocks):
        for b in range(nb):
            p = f"layer{s + 1}.{b}."
            kept = H._bottleneck_forward(params, p, x, 2 if (b == 0 and s > 0) else 1)
            x = kept["out"]
            masks.update({p + n: kept[n] > 0 for n in ("t1", "t2", "out")})
    same = net.grad_host(imgs, grads, np.float64, masks)
    assert all(np.array_equal(own[n], same[n]) for n in own)
    shut = net.grad_host(imgs, grads, np.float64, {k: np.zeros_like(v) for k, v in masks.items()})
    assert all(not shut[n].any() for n in shut)             # every ReLU closed: nothing flows


# ------------------------------------------------------------------------------------------------------------------ the constructor
def _cfg(**kw):
    cfg = dict(U.SHIPPED)
    cfg.pop("type")
    cfg.update(kw)
    return cfg


def test_differentiable_needs_frozen_stages_norm_eval_and_frozen_batchnorms():
    for kw in (dict(frozen_stages=0), dict(frozen_stages=-1), dict(norm_eval=False), dict(norm_cfg=dict(type="BN", requires_grad=True)),
               dict(norm_cfg=dict(type="BN")), dict(norm_cfg=None)):
        with pytest.raises(NotImplementedError, match="differentiable"):
            ResNet(**_cfg(differentiable=True, **kw))
        ResNet(**_cfg(**kw))                                # without the keyword they are what they were


@pytest.mark.parametrize("frozen", [1, 2, 4])
def test_the_kernels_behind_the_frozen_stages_require_grad(frozen):
    net = ResNet(**_cfg(differentiable=True, frozen_stages=frozen))
    assert net.differentiable
    want = set(H.trainable_kernels(net.stage_blocks, frozen))
    assert (len(want) > 0) == (frozen < 4)
    for name, p in net.named_parameters():
        trainable = name.startswith(tuple(f"layer{s + 1}." for s in range(frozen, 4))) and p.dim() == 4
        assert p.requires_grad == trainable == (name in want), name
    assert any("downsample.0.weight" in n for n in want) or frozen == 4
    net.train()
    assert all(not m.training for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))


def test_without_the_keyword_every_flag_is_false():
    for net in (ResNet(**_cfg()), ResNet(**_cfg(differentiable=False)), U.build_backbone()):
        assert not net.differentiable and not any(p.requires_grad for p in net.parameters())
    import inspect
    assert list(inspect.signature(ResNet.__init__).parameters)[-1] == "differentiable"


# ------------------------------------------------------------------------------------------------------------------ the ABI
NAMES = ("ptx_conv_bwd_workspace_bytes", "ptx_conv_dweight_chunks", "ptx_conv1x1_bwd", "ptx_conv3x3_bwd")


def test_the_four_entry_points_are_in_the_header_and_bound():
    protos = header_prototypes()
    assert all(n in protos and n in _abi.SIGNATURES for n in NAMES)
    assert _abi.ABI_VERSION == 13
    assert len(_abi.SIGNATURES["ptx_conv1x1_bwd"][1]) == 20 and len(_abi.SIGNATURES["ptx_conv3x3_bwd"][1]) == 19


def test_the_plan_functions_answer_without_a_device():
    lib = _abi.lib()
    assert lib.ptx_abi_version() == 13
    good = [(1, 3, 32, 32, 8, 8, 1), (1, 3, 80, 48, 7, 9, 2), (3, 5, 32, 32, 40, 36, 1), (3, 3, 512, 512, 17, 33, 2), (1, 300, 64, 32, 120, 120, 1)]
    for a in good:
        S, nbytes = lib.ptx_conv_dweight_chunks(*a), lib.ptx_conv_bwd_workspace_bytes(*a)
        assert S >= 1 and nbytes > 0 and nbytes % 16 == 0
        assert (S, nbytes) == (lib.ptx_conv_dweight_chunks(*a), lib.ptx_conv_bwd_workspace_bytes(*a))        # the same value twice
        assert S == H.dweight_chunks_host(*a)               # and the host's restatement of the plan
        KS, N, cin, cout = a[:4]
        assert nbytes >= 4 * cout * KS * KS * cin * (1 + (S if S > 1 else 0))
    bad = [(1, 3, 24, 32, 8, 8, 1), (1, 3, 32, 24, 8, 8, 1), (3, 3, 24, 24, 8, 8, 1), (1, 3, 32, 32, 8, 8, 3), (3, 3, 32, 32, 8, 8, 3),
           (2, 3, 32, 32, 8, 8, 1), (3, 3, 32, 48, 8, 8, 1), (1, 0, 32, 32, 8, 8, 1), (3, 3, 528, 528, 8, 8, 1), (1, 3, 32, 32, 0, 8, 1)]
    for a in bad:
        assert lib.ptx_conv_bwd_workspace_bytes(*a) == 0, a
        assert lib.ptx_conv_dweight_chunks(*a) == PTX_EINVAL, a
        msg = lib.ptx_last_error().decode()
        assert "ptx_conv_dweight_chunks" in msg and f"Cin={a[2]}" in msg and f"stride={a[6]}" in msg


def test_the_plan_is_monotone_in_the_number_of_images():
    lib = _abi.lib()
    for KS, cin, cout, Hh, Ww, stride in ((1, 64, 32, 120, 120, 1), (3, 32, 32, 120, 120, 2), (1, 16, 16, 9, 9, 1), (3, 512, 512, 15, 15, 1),
                                             (1, 2048, 2048, 15, 15, 1), (3, 48, 48, 40, 36, 1)):
        last = (0, 0)
        for N in list(range(1, 70)) + [100, 299, 300, 301, 1000, 4096]:
            now = (lib.ptx_conv_dweight_chunks(KS, N, cin, cout, Hh, Ww, stride), lib.ptx_conv_bwd_workspace_bytes(KS, N, cin, cout, Hh, Ww, stride))
            assert now[0] >= last[0] and now[1] >= last[1], (KS, cin, cout, Hh, Ww, stride, N, now, last)
            last = now
    # the smallest trainable output at the shipped shape (layer2's 3x3: 32 x 288 on 300 maps of 60 x 60) fills the machine
    S = lib.ptx_conv_dweight_chunks(3, 300, 32, 32, 120, 120, 2)
    assert S * 5 >= 1024
