"""Differentiable voxel quantisation (``module.quantize`` with grad mode on; csrc/voxel.hip: ptx_voxelize_rep /
ptx_voxel_features_bwd): ``features = p[unique_index]`` of detectors/sparse_featfusion_grounder_preshape.py:388-397 hands each
row's gradient back to the point the row kept.  The operator against the host rule of tests/test_voxel_grad_host.py (bit for
bit), the chain neck -> quantize against the float64 oracle (no duplicates: the loss IS the oracle's) and against a twin module
driven by host-scattered gradients (duplicates), the lifetime of what the node saves, and the paths that must stay plain."""
import copy

import numpy as np
import pytest
import torch

from proxytransformation_amd.synth import PreshapeConfig, fill_state_dict, make_scene_batch
from tests.test_voxel_grad_host import features_bwd_rule, first_index
from tests.util import assert_close, build_module, oracle_kwargs

pytestmark = pytest.mark.gpu

VX = PreshapeConfig("vx", B=3, N=6000, grid_size=4, dynamic_drop_radio=0.5, L=4, V=2, seed_base=9100)
TR1 = PreshapeConfig("tr1", B=3, N=5000, grid_size=5, dynamic_drop_radio=0.6, L=9, V=4, seed_base=8100)


def _node(feats):
    """The autograd node of the differentiable ``quantize`` behind ``features``."""
    fn = feats.grad_fn
    assert fn is not None, "features carry no grad_fn"
    seen = [fn]
    while seen:
        f = seen.pop()
        if "VoxelFeatures" in f.name():
            return f
        seen += [g for g, _ in f.next_functions if g is not None]
    raise AssertionError("no _VoxelFeatures node behind the features")


def _train_outs(cfg):
    from tests.gpu_util import t
    m, _ = build_module(cfg)
    m = m.cuda().train()
    pts, text, mask, img = make_scene_batch(cfg)
    outs = m([t(p) for p in pts], {"text_feats": t(text), "text_token_mask": t(mask)}, t(img))
    assert all(o.grad_fn is not None for o in outs)
    return m, outs


def _np(ts):
    return [x.detach().cpu().numpy() for x in ts]


def _rand_like(x, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(x.shape), generator=g).to(x.device)


def _check_operator(m, outs, voxel_size, ncap):
    """One differentiable call on ``outs`` against the plain call, the oracle and the host rule; returns (nvox, total).  ``ncap``:
    the row capacity per scene that tells the route taken -- the padded buffer's for a list used in place, max(n) for a packed one."""
    from oracle import oracle
    B = len(outs)
    coords, feats, inv = m.quantize(outs, voxel_size, return_inverse=True)
    assert feats.grad_fn is not None and not coords.requires_grad and not any(i.requires_grad for i in inv)
    with torch.no_grad():
        c0, f0, i0 = m.quantize(outs, voxel_size, return_inverse=True)
    assert f0.grad_fn is None and not f0.requires_grad
    rc, rf, rinv = oracle.voxelize(_np(outs), voxel_size)
    for got_c, got_f, got_i in ((coords, feats, inv), (c0, f0, i0)):
        assert got_c.dtype == torch.int32 and np.array_equal(got_c.cpu().numpy(), rc)
        assert np.array_equal(got_f.detach().cpu().numpy(), rf)
        assert len(got_i) == B and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got_i, rinv))
    nvox, n = len(rc), [int(o.shape[0]) for o in outs]
    # rep: the first index of every row, as the flat PADDED index b * Ncap + i
    s_inv, s_rep, s_counts = _node(feats).saved_tensors
    Ncap = s_inv.shape[1]
    assert Ncap == ncap, f"capacity {Ncap} per scene, {ncap} expected: the other route was taken"
    assert s_inv.shape[0] == B and s_rep.dtype == torch.int32 and s_counts.cpu().tolist() == n
    want = first_index(rinv, nvox)
    sizes = np.cumsum([0] + n)
    scene = np.searchsorted(sizes, want, side="right") - 1
    assert np.array_equal(s_rep[:nvox].cpu().numpy().astype(np.int64), scene * Ncap + (want - sizes[scene]))
    # the backward of a random dfeats, bit for bit
    dfeats = _rand_like(feats, 11)
    grads = torch.autograd.grad(feats, outs, dfeats, retain_graph=True, allow_unused=False)
    rule = features_bwd_rule(dfeats.cpu().numpy(), rinv)
    for b in range(B):
        assert grads[b].shape == (n[b], 3) and grads[b].dtype == torch.float32
        assert np.array_equal(grads[b].cpu().numpy(), rule[b]), (voxel_size, b)
    # one buffer behind the per-scene gradients (the shape _TrainStepC.backward / ptx_op_affine_bwd_list take)
    live = [g for g in grads if g.numel()]
    assert len({g.untyped_storage().data_ptr() for g in live}) == 1 and all(g.is_contiguous() for g in live)
    return nvox, sum(n)


@pytest.mark.parametrize("voxel_size", [0.01, 0.25, 2.0])
def test_operator_matches_the_host_rule(voxel_size):
    m, outs = _train_outs(VX)
    # the train-mode outputs are views of the step's one padded (B,N,3) buffer and are used in place: capacity N, not max(n)
    assert max(int(o.shape[0]) for o in outs) < VX.N
    nvox, total = _check_operator(m, outs, voxel_size, VX.N)
    if voxel_size >= 0.25:
        assert nvox < total                                              # duplicates really occur at this size
    # a list that is NOT the module's own padded buffer (leaf copies, negative coordinates): the packing route
    shifted = [(o.detach().clone() - 5.0).requires_grad_(True) for o in outs]
    nvox2, _ = _check_operator(m, shifted, voxel_size, max(int(o.shape[0]) for o in shifted))
    if voxel_size >= 0.25:
        assert nvox2 < total
    # ... through .backward() into the leaves, with a dfeats of another dtype and layout
    from oracle import oracle
    coords, feats = m.quantize(shifted, voxel_size)
    d64 = _rand_like(feats, 12).double().t().contiguous().t()
    assert not d64.is_contiguous() or d64.shape[0] <= 1
    feats.backward(d64)
    rule = features_bwd_rule(d64.float().cpu().numpy(), oracle.voxelize(_np(shifted), voxel_size)[2])
    for b, leaf in enumerate(shifted):
        assert np.array_equal(leaf.grad.cpu().numpy(), rule[b])


def _build_train(cfg):
    from proxytransformation_amd import MODELS
    m = MODELS.build(dict(type="ProxyTransformationNormReverse", drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                          **cfg.module_kwargs()))
    sd = fill_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m, sd


def test_chain_matches_the_float64_oracle():
    """The ``f32`` case of test_training_step_matches_the_oracle_on_fresh_scenes with the loss taken BEHIND quantize at a voxel
    size (1 mm) at which no two points share a voxel: features = cat(outs), so sum <features, cat_b W_b> is the oracle's loss and
    every gradient is held to the same bar (max error <= 1e-4 of the tensor's RMS, same small-tensor rule, same none_grads)."""
    from oracle import oracle
    from tests.gpu_util import t
    cfg = TR1
    m, sd = _build_train(cfg)
    m = m.cuda().train()
    pts, text, mask, img = make_scene_batch(cfg)
    img_t = torch.from_numpy(img)
    ref = oracle.forward_train(sd, **oracle_kwargs(cfg), points=pts, text_feats=text, text_mask=mask,
                               img_feat=img_t.numpy(), float64=True)
    m._centers_override = torch.from_numpy(ref["centers"].astype(np.float32))
    tx = t(text).requires_grad_(True)
    ix = img_t.cuda().requires_grad_(True)
    outs = m([t(p) for p in pts], {"text_feats": tx, "text_token_mask": t(mask)}, ix)
    for b in range(cfg.B):
        assert_close(outs[b].detach().cpu().numpy(), ref["outputs"][b], atol=1e-4, what=f"output {b}")
    coords, feats = m.quantize(outs, 1e-3)
    total = sum(int(o.shape[0]) for o in outs)
    assert feats.shape[0] == total, f"{total - feats.shape[0]} duplicates at 1 mm: the loss would not be the oracle's"
    assert int(coords[:, 1:].abs().max()) < (1 << 18)
    w = torch.cat([torch.from_numpy(oracle.loss_weights(b, int(o.shape[0]))) for b, o in enumerate(outs)]).to(feats.device)
    (feats * w).sum().backward()
    assert sorted(n for n, p in m.named_parameters() if p.grad is None) == sorted(ref["none_grads"])
    named = dict(m.named_parameters())
    named["input.text_feats"] = tx
    named["input.img_feat"] = ix
    worst = {}
    for name, gref in ref["grads"].items():
        got = named[name].grad.detach().float().cpu().numpy().astype(np.float64).reshape(gref.shape)
        rms = np.sqrt((gref.astype(np.float64) ** 2).mean())
        if rms * np.sqrt(gref.size) < 2e-3:
            continue
        err = np.abs(got - gref).max() / rms
        worst[name] = err
        print(f"grad {name}: max err / rms = {err:.3e}")
        assert err < 1e-4, f"grad {name}: max err / rms = {err:.3e} (bar 1e-4)"
    assert len(worst) > 20
    print("worst gradient errors behind quantize (max err / rms vs the float64 oracle):",
          sorted(((round(v, 6), k) for k, v in worst.items()), reverse=True)[:5])


def test_chain_with_duplicates_equals_host_scattered_gradients():
    """25 cm voxels: some hundred points of the three clouds share a voxel with an earlier one and must receive exact zeros.  One module backpropagates through quantize from a random dfeats; its twin gets the
    same dfeats scattered on the host (oracle.voxelize's inverse + the rule) as the upstream gradients of ``outs``: every parameter
    and input gradient has the same bits (the step itself is bit-reproducible: test_training_step_is_bit_reproducible)."""
    from oracle import oracle
    from tests.gpu_util import t
    cfg = TR1
    m0, _ = _build_train(cfg)
    pts, text, mask, img = make_scene_batch(cfg)
    runs = []
    for through_quantize in (True, False):
        m = copy.deepcopy(m0).cuda().train()
        tx, ix = t(text).requires_grad_(True), t(img).requires_grad_(True)
        outs = m([t(p) for p in pts], {"text_feats": tx, "text_token_mask": t(mask)}, ix)
        rc, _, rinv = oracle.voxelize(_np(outs), 0.25)
        total = sum(int(o.shape[0]) for o in outs)
        assert len(rc) < total                                          # duplicates really occur
        dfeats = torch.randn((len(rc), 3), generator=torch.Generator().manual_seed(21))
        if through_quantize:
            coords, feats = m.quantize(outs, 0.25)
            assert np.array_equal(coords.cpu().numpy(), rc)
            feats.backward(dfeats.cuda())
        else:
            douts = [torch.from_numpy(d).cuda() for d in features_bwd_rule(dfeats.numpy(), rinv)]
            torch.autograd.backward(outs, douts)
        torch.cuda.synchronize()
        runs.append(([o.detach().clone() for o in outs], {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
                     tx.grad.clone(), ix.grad.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert sorted(runs[0][1]) == sorted(runs[1][1]) and len(runs[0][1]) > 20
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
        assert bool(torch.isfinite(runs[0][1][k]).all()), k
    assert sum(float(g.abs().max()) > 0.0 for g in runs[0][1].values()) > 20
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])
    assert float(runs[0][2].abs().max()) > 0.0 and float(runs[0][3].abs().max()) > 0.0


def test_saved_state_survives_later_calls_and_repeated_backwards():
    from oracle import oracle
    m, outs = _train_outs(VX)
    _, f1 = m.quantize(outs, 0.01)
    _, f2 = m.quantize(outs, 2.0)                                       # the same lane, the same scratch
    assert f2.shape[0] < f1.shape[0]
    d1, d2 = _rand_like(f1, 31), _rand_like(f2, 32)
    m.quantize([o.detach() * 0.5 for o in outs], 0.05)                  # and a plain call of another list in between
    g2 = torch.autograd.grad(f2, outs, d2, retain_graph=True)           # the backwards in reverse order
    g1 = torch.autograd.grad(f1, outs, d1, retain_graph=True)
    for f, d, g, vs in ((f1, d1, g1, 0.01), (f2, d2, g2, 2.0)):
        rule = features_bwd_rule(d.cpu().numpy(), oracle.voxelize(_np(outs), vs)[2])
        for b in range(len(outs)):
            assert np.array_equal(g[b].cpu().numpy(), rule[b]), (vs, b)
    again = torch.autograd.grad(f1, outs, d1, retain_graph=True)
    for a, b in zip(g1, again):
        assert torch.equal(a, b)
    # all the way into a parameter, twice: the same bits
    prm = [p for p in m.parameters() if p.requires_grad]
    ga = torch.autograd.grad(f2, prm, d2, retain_graph=True, allow_unused=True)
    gb = torch.autograd.grad(f2, prm, d2, retain_graph=True, allow_unused=True)
    assert sum(g is not None for g in ga) > 20
    for a, b in zip(ga, gb):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


def test_empty_scenes_and_no_rows():
    from oracle import oracle
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(41)
    a = (torch.rand((1501, 3), generator=g) * 3.0).to(dev).requires_grad_(True)
    e = torch.zeros((0, 3), device=dev, requires_grad=True)
    c = (torch.rand((777, 3), generator=g) * 3.0 - 1.0).to(dev).requires_grad_(True)
    m, _ = build_module(VX)
    m = m.cuda()
    outs = [a, e, c]                                                    # an empty scene in the middle
    coords, feats, inv, ends = m.quantize(outs, 0.1, return_inverse=True, return_scene_rows=True)
    rc, rf, rinv = oracle.voxelize(_np(outs), 0.1)
    assert np.array_equal(coords.cpu().numpy(), rc) and np.array_equal(feats.detach().cpu().numpy(), rf)
    assert ends[0] == ends[1] and ends[2] == len(rc) and inv[1].shape == (0,)
    assert len(rc) < 1501 + 777
    d = _rand_like(feats, 42)
    feats.backward(d)
    rule = features_bwd_rule(d.cpu().numpy(), rinv)
    for leaf, want in zip(outs, rule):
        assert leaf.grad.shape == leaf.shape and np.array_equal(leaf.grad.cpu().numpy(), want)
    # no rows at all
    e1, e2 = (torch.zeros((0, 3), device=dev, requires_grad=True) for _ in range(2))
    coords, feats = m.quantize([e1, e2], 0.1)
    assert coords.shape == (0, 4) and feats.shape == (0, 3) and feats.grad_fn is not None
    feats.sum().backward()
    assert e1.grad.shape == (0, 3) and e2.grad.shape == (0, 3)
    # only one scene of the list requires grad: the others get none
    a2, c2 = a.detach().clone().requires_grad_(True), c.detach().clone()
    _, feats = m.quantize([a2, c2], 0.1)
    feats.backward(torch.ones_like(feats))
    assert a2.grad is not None and c2.grad is None


def test_plain_paths_stay_plain_and_synchronise_alike():
    from tests.gpu_util import t
    from tests.test_gpu_pipeline import _count_synchronises
    m, outs = _train_outs(VX)
    with torch.no_grad():
        _, f = m.quantize(outs, 0.01)
    assert f.grad_fn is None and not f.requires_grad
    _, f = m.quantize([o.detach() for o in outs], 0.01)                 # nothing requires grad
    assert f.grad_fn is None and not f.requires_grad
    m.eval()
    pts, text, mask, img = make_scene_batch(VX)
    with torch.no_grad():
        eouts = m([t(p) for p in pts], {"text_feats": t(text), "text_token_mask": t(mask)}, t(img))
    _, f = m.quantize(eouts, 0.01)                                       # eval outputs, grad mode on
    assert f.grad_fn is None and not f.requires_grad
    # the differentiable forward waits for the host exactly as often as the plain one (both warmed up above)
    torch.cuda.synchronize()
    with _count_synchronises() as plain:
        with torch.no_grad():
            m.quantize(outs, 0.01)
    torch.cuda.synchronize()
    with _count_synchronises() as diff:
        _, f = m.quantize(outs, 0.01)
    assert f.grad_fn is not None
    assert list(diff) == list(plain), (diff, plain)
