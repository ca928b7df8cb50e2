"""``GroundingFeaturePrefix(differentiable=True)``: one ``loss.backward()`` from the prefix's outputs -- the voxel features
(DET:388-397) and the sampled image features of the four levels (DET:428-448) -- to the neck's parameters, the text features and all
four levels of the 2D backbone's feature maps, at the reduced size of tests/test_gpu_pipeline.py (V = 8 views, N = 20 000, two
scenes, the shipped neck configuration with drop rates 0).

Every gradient is held bit for bit against the same pieces driven separately: a twin module fed the same ingested clouds and the
host-scattered gradient of the voxel features (tests/test_voxel_grad_host.py), and the standalone ``batch_point_sample`` backward
on the same level points; the last level receives the sum of the two."""
import copy

import numpy as np
import pytest
import torch

from proxytransformation_amd.fusion import batch_point_sample
from proxytransformation_amd.pipeline import GroundingFeaturePrefix, projection_matrices
from proxytransformation_amd.synth import CONFIGS, FPN_LEVELS, PreshapeConfig, fill_state_dict
from tests.test_gpu_pipeline import _inputs
from tests.test_voxel_grad_host import features_bwd_rule

pytestmark = pytest.mark.gpu

SEED = 7300


def _cfg():
    base = CONFIGS["cfg4_room"]
    return PreshapeConfig("pipe_small", B=2, N=20000, grid_size=base.grid_size, dynamic_drop_radio=base.dynamic_drop_radio,
                          L=base.L, V=8, text_blocks=3, img_blocks=3, extent=base.extent, seed_base=SEED)


def _module(cfg):
    from proxytransformation_amd import MODELS
    m = MODELS.build(dict(type="ProxyTransformationNormReverse", drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                          **cfg.module_kwargs()))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state_dict(m.state_dict()).items()})
    return m


def _weights(res, seed):
    g = torch.Generator().manual_seed(seed)
    dev = res.features.device
    w = torch.randn(tuple(res.features.shape), generator=g).to(dev)
    wl = [[torch.randn(tuple(f.shape), generator=g).to(dev) for f in per_level] for per_level in res.points_imgfeats]
    return w, wl


def test_one_backward_reaches_the_neck_the_text_and_every_feature_level():
    from oracle import oracle
    cfg = _cfg()
    m0 = _module(cfg)
    m, twin = copy.deepcopy(m0).cuda().train(), copy.deepcopy(m0).cuda().train()
    scenes_np, scenes, text_dict, feats = _inputs(cfg, 2, 8, SEED)
    feats = [f.requires_grad_(True) for f in feats]
    text = text_dict["text_feats"].requires_grad_(True)
    pipe = GroundingFeaturePrefix(m, n_points=cfg.N, differentiable=True)
    res = pipe(scenes, text_dict, feats, rng=np.random.RandomState(SEED))
    assert res.features.grad_fn is not None and all(p.grad_fn is not None for p in res.points)
    assert all(f.grad_fn is not None for per_level in res.points_imgfeats for f in per_level)
    assert not res.coordinates.requires_grad and not any(p.requires_grad for p in res.ingested.points)
    assert not any(p.requires_grad for lv in res.level_points for p in lv)
    w, wl = _weights(res, 5)
    loss = (res.features * w).sum() + sum((f * wl[b][li]).sum() for b, per_level in enumerate(res.points_imgfeats)
                                          for li, f in enumerate(per_level))
    loss.backward()
    torch.cuda.synchronize()

    # the twin: the same ingested clouds through the neck, the gradient of the voxel features scattered on the host
    text2 = text.detach().clone().requires_grad_(True)
    img2 = feats[-1].detach().clone().requires_grad_(True)
    outs2 = twin(res.ingested.points, {"text_feats": text2, "text_token_mask": text_dict["text_token_mask"]}, img2)
    for a, b in zip(res.points, outs2):
        assert torch.equal(a.detach(), b.detach())
    rc, rf, rinv = oracle.voxelize([o.detach().cpu().numpy() for o in outs2], pipe.voxel_size)
    assert np.array_equal(res.coordinates.cpu().numpy(), rc) and np.array_equal(res.features.detach().cpu().numpy(), rf)
    douts = [torch.from_numpy(d).cuda() for d in features_bwd_rule(w.cpu().numpy(), rinv)]
    torch.autograd.backward(outs2, douts)
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    want = {k: p.grad for k, p in twin.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(want) and len(got) > 20
    for k in got:
        assert torch.equal(got[k], want[k]), k
    assert float(text.grad.abs().max()) > 0.0 and torch.equal(text.grad, text2.grad)

    # the sampling of every level on its own: the standalone backward on the same level points and upstream gradient
    alone = []
    for li in range(len(FPN_LEVELS)):
        per_scene = []
        for b, sc in enumerate(scenes_np):
            meta = sc["img_meta"]
            f = feats[li][b].detach().clone().requires_grad_(True)
            proj = torch.from_numpy(projection_matrices(sc["depth2img"])).cuda()
            out = batch_point_sample(meta, f, res.level_points[li][b], proj, "DEPTH", img_scale_factor=meta["scale_factor"][:2],
                                     img_crop_offset=0.0, img_flip=False, img_pad_shape=(480, 480), img_shape=tuple(meta["img_shape"])[:2],
                                     aligned=False)
            assert torch.equal(out.detach(), res.points_imgfeats[b][li].detach())
            out.backward(wl[b][li])
            per_scene.append(f.grad)
        alone.append(torch.stack(per_scene))
    for li in range(3):
        assert float(feats[li].grad.abs().max()) > 0.0
        assert torch.equal(feats[li].grad, alone[li]), f"level {li}"
    # the last level feeds the neck as well: torch's own accumulation adds the two contributions
    assert float(img2.grad.abs().max()) > 0.0 and float(alone[3].abs().max()) > 0.0
    assert torch.equal(feats[3].grad, alone[3] + img2.grad)


def test_default_stays_under_no_grad_with_the_same_values():
    cfg = _cfg()
    m = _module(cfg).cuda().train()
    scenes_np, scenes, text_dict, feats = _inputs(cfg, 2, 8, SEED)
    feats = [f.requires_grad_(True) for f in feats]
    text_dict["text_feats"].requires_grad_(True)
    res_d = GroundingFeaturePrefix(m, n_points=cfg.N, differentiable=True)(scenes, text_dict, feats, rng=np.random.RandomState(SEED))
    res_p = GroundingFeaturePrefix(m, n_points=cfg.N)(scenes, text_dict, feats, rng=np.random.RandomState(SEED))
    assert res_d.features.grad_fn is not None
    assert res_p.features.grad_fn is None and not res_p.features.requires_grad
    assert all(p.grad_fn is None for p in res_p.points)
    assert all(f.grad_fn is None and not f.requires_grad for per_level in res_p.points_imgfeats for f in per_level)
    # the stages that do not depend on the module's mode -- ingest, level coordinates, sampling -- and, with drop rates 0, the neck
    # and the quantisation too (train mode normalises with batch statistics in both calls): the same bits
    for a, b in zip(res_d.ingested.points, res_p.ingested.points):
        assert torch.equal(a, b)
    for a, b in zip(res_d.points, res_p.points):
        assert torch.equal(a.detach(), b)
    assert torch.equal(res_d.coordinates, res_p.coordinates) and torch.equal(res_d.features.detach(), res_p.features)
    assert res_d.scene_rows == res_p.scene_rows
    for li in range(len(FPN_LEVELS)):
        for b in range(2):
            assert torch.equal(res_d.level_coords[li][b], res_p.level_coords[li][b])
            assert torch.equal(res_d.level_points[li][b], res_p.level_points[li][b])
            assert torch.equal(res_d.points_imgfeats[b][li].detach(), res_p.points_imgfeats[b][li])
    # the caller's no_grad is respected by the differentiable prefix
    with torch.no_grad():
        res_n = GroundingFeaturePrefix(m, n_points=cfg.N, differentiable=True)(scenes, text_dict, feats, rng=np.random.RandomState(SEED))
    assert res_n.features.grad_fn is None and torch.equal(res_n.features, res_p.features)
    # an eval module has no differentiable path
    m.eval()
    with pytest.raises(RuntimeError, match=r"call \.train\(\)"):
        GroundingFeaturePrefix(m, n_points=cfg.N, differentiable=True)(scenes, text_dict, feats, rng=np.random.RandomState(SEED))
    res_e = GroundingFeaturePrefix(m, n_points=cfg.N)(scenes, text_dict, feats, rng=np.random.RandomState(SEED))
    assert res_e.features.grad_fn is None
    for a, b in zip(res_e.ingested.points, res_p.ingested.points):
        assert torch.equal(a, b)


def test_two_calls_before_their_backwards_in_reverse_order():
    """Gradient accumulation with delayed backwards: the same prefix is called twice (the second time on the scenes in swapped
    order, so other matrices land where the first call's were staged) before either backward runs, and the backwards run in
    reverse order.  What the nodes of the first call saved -- the projection matrices and reverse flows of the sampling, the
    inverse map of the quantisation -- must still be that call's: the gradients of the sampled features with respect to all four
    feature levels and of the voxel features with respect to the neck's outputs equal, bit for bit, those of the same call made
    alone on a fresh prefix."""
    cfg = _cfg()
    m = _module(cfg).cuda().train()
    _, scenes, text_dict, feats = _inputs(cfg, 2, 8, SEED)
    feats = [f.requires_grad_(True) for f in feats]

    def grads(res, seed):
        w, wl = _weights(res, seed)
        sampled = sum((f * wl[b][li]).sum() for b, per_level in enumerate(res.points_imgfeats) for li, f in enumerate(per_level))
        g_levels = torch.autograd.grad(sampled, feats, retain_graph=True)
        g_points = torch.autograd.grad((res.features * w).sum(), res.points, retain_graph=True)
        return [g.clone() for g in g_levels + g_points]

    orders = (list(scenes), list(scenes[::-1]))
    alone = [grads(GroundingFeaturePrefix(m, n_points=cfg.N, differentiable=True)(sc, text_dict, feats, rng=np.random.RandomState(SEED)),
                   50 + i) for i, sc in enumerate(orders)]
    assert any(not torch.equal(a, b) for a, b in zip(alone[0][:4], alone[1][:4]))       # the two calls really differ
    pipe = GroundingFeaturePrefix(m, n_points=cfg.N, differentiable=True)
    first = pipe(orders[0], text_dict, feats, rng=np.random.RandomState(SEED))
    second = pipe(orders[1], text_dict, feats, rng=np.random.RandomState(SEED))
    late = [grads(second, 51), grads(first, 50)][::-1]                                   # the second call's backward runs first
    for i in range(2):
        assert len(late[i]) == len(alone[i]) == 4 + 2
        for k, (a, b) in enumerate(zip(late[i], alone[i])):
            assert float(b.abs().max()) > 0.0 and torch.equal(a, b), (i, k)
