"""The assembled sparse MinkResNet (proxytransformation_amd/backbone.py) on the GPU.

Eval: ``MinkResNet(34, 3)`` with seeded kaiming kernels, BatchNorm weights in U(0.5, 1.5), running means N(0, 0.1) and running variances
in U(0.5, 1.5) on the rows of the convolution's tests (2351 rows, four scenes of which one is empty and one has a single row): every
level's rows bit for bit against ``forward_host`` and ``pipeline.level_coordinates``, every level's features against ``forward_host``
in float64 under the rule of the convolution's tests (``sparse_util.hold``: at most 8 x the error of ``forward_host`` in float32).

Train: one step of ``MinkResNet(18, 3, differentiable=True)``, loss = sum_l (out_l * G_l).sum(), against the same network composed from
torch ops over the host kernel maps in float64 on the CPU (``composition`` of tests/sparse_util.py, ``F.batch_norm``, the
restated instance norm, a stacked max), yardstick the same composition in float32, 8 x; the ReLU masks of both references are the
GPU's outputs', as in the layer tests.  Both torch references run with ``CPU_THREADS`` threads, set and restored around them: torch
splits its fp32 reductions over the rows by thread, so the yardstick's own error depends on the count -- 2e-6 of scale with 8 or 16
threads, 8e-6 to 1.1e-5 with the single thread that ``oracle.forward_train`` leaves set for the rest of a process that ran it --, and a
bar that moved with the tests that ran before would not be one."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import MinkResNet, sparse
from proxytransformation_amd.pipeline import MINK_RESNET_STRIDES, level_coordinates
from tests import sparse_util as su

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seeded(depth, **kw):
    torch.manual_seed(1234 + depth)
    m = MinkResNet(depth, 3, **kw)
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, sparse.SparseBatchNorm):
                mod.bn.weight.uniform_(0.5, 1.5, generator=g)
                mod.bn.running_mean.normal_(0.0, 0.1, generator=g)
                mod.bn.running_var.uniform_(0.5, 1.5, generator=g)
    return m


@functools.lru_cache(maxsize=None)
def _inputs():
    rows, ends = su.rows(1)
    feats = np.random.default_rng(11).uniform(0.0, 1.0, (rows.shape[0], 3)).astype(np.float32)      # colours
    return rows, list(ends), feats


# ------------------------------------------------------------------------------------------------------------------ eval
def test_eval_forward_against_the_host_restatement():
    rows, ends, feats = _inputs()
    assert rows.shape[0] > 2200 and ends[2] == ends[1] and ends[3] == ends[2] + 1      # an empty scene and a one-row scene
    m = _seeded(34).eval()
    maps = m.host_kernel_maps(rows, ends)
    ref64 = m.forward_host(rows, ends, feats, np.float64, maps)
    ref32 = m.forward_host(rows, ends, feats, np.float32, maps)
    gpu = m.to(DEV)
    coords = torch.from_numpy(rows).to(DEV)
    with torch.no_grad():
        got = gpu(coords, ends, torch.from_numpy(feats).to(DEV))
        again = gpu(coords, ends, torch.from_numpy(feats).to(DEV))
    assert len(got) == 4 and tuple(lv.tensor_stride for lv in got) == MINK_RESNET_STRIDES
    for l, (lv, r32, r64) in enumerate(zip(got, ref32, ref64)):
        assert lv.coords.dtype == torch.int32 and np.array_equal(lv.coords.cpu().numpy(), r64.coords) and lv.scene_rows == r64.scene_rows
        lc, _, le = level_coordinates(coords, ends, lv.tensor_stride, 0.01)
        assert le == lv.scene_rows and torch.equal(lc, lv.coords)
        assert lv.scene_rows[2] == lv.scene_rows[1]            # the empty scene stays empty
        assert lv.feats.shape == (r64.coords.shape[0], 64 * 2 ** l) and lv.feats.dtype == torch.float32
        assert torch.equal(lv.feats, again[l].feats), "two forwards on the same inputs differ"
        su.hold(f"MinkResNet34 eval level {l} rows={lv.feats.shape[0]}", lv.feats.cpu().numpy(), r32.feats, r64.feats)


def test_golden_names_load_strictly_and_the_fold_is_cached():
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "mink_resnet34_state_dict.json")))
    m = _seeded(34).to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    sd = {k: (torch.rand(shape, generator=g) + 0.5 if shape else torch.tensor(3)) for k, shape in names}
    sd["conv1.kernel"] = sd["conv1.kernel"] - 1.0
    m.load_state_dict(sd, strict=True)
    assert int(m.layer4[2].norm2.bn.num_batches_tracked) == 3 and torch.equal(m.conv1.kernel.cpu(), sd["conv1.kernel"])
    bn = m.layer1[0].norm1.bn
    scale, shift = sparse.bn_fold(bn)
    assert sparse.bn_fold(bn)[0] is scale and sparse.bn_fold(bn)[1] is shift      # no launches per forward
    assert torch.allclose(scale, bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps), rtol=1e-6, atol=0)
    assert torch.allclose(shift, bn.bias.detach() - bn.running_mean * scale, rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        bn.running_var.mul_(2.0)
    assert sparse.bn_fold(bn)[0] is not scale                 # rebuilt when a tensor's version changes
    m.load_state_dict(sd, strict=True)
    assert torch.allclose(sparse.bn_fold(bn)[0], scale)


# ------------------------------------------------------------------------------------------------------------------ train
CPU_THREADS = 8     # of the two torch references below: the order of their fp32 sums, and so the yardstick, depends on the thread count


def _instance_norm(x, ends, weight, bias):
    parts, lo = [], 0
    for hi in ends:
        if hi > lo:
            seg = x[lo:hi]
            mean = seg.mean(0, keepdim=True)
            var = ((seg - mean) ** 2).mean(0, keepdim=True)
            parts.append((seg - mean) / torch.sqrt(var + sparse.INSTANCE_NORM_EPS))
        lo = hi
    return torch.cat(parts) * weight + bias


def _torch_network(ref, maps, feats, masks):
    """``ref``: a CPU copy of the model in the dtype of ``feats``; ``masks[name]``: [out > 0] of the GPU's output of norm ``name``."""
    def bn(name, norm, x, residual=None, relu=True):
        y = F.batch_norm(x, norm.bn.running_mean, norm.bn.running_var, norm.bn.weight, norm.bn.bias, True, norm.bn.momentum, norm.bn.eps)
        if residual is not None:
            y = y + residual
        return y * masks[name].to(y.dtype) if relu else y

    x = _instance_norm(su.composition(feats, maps["stem"][2], ref.conv1.kernel), maps["stem"][1], ref.norm1.weight, ref.norm1.bias)
    x = x * masks["norm1"].to(x.dtype)
    idx = torch.from_numpy(maps["pool"][2]).long()
    x = x[idx.clamp(min=0)].masked_fill((idx < 0).unsqueeze(-1), -np.inf).max(dim=1).values
    outs = []
    for i in range(ref.num_stages):
        n_down, n_side, n_same = maps["down", i][2], maps["side", i][2], maps["same", i][2]
        for j, blk in enumerate(getattr(ref, f"layer{i + 1}")):
            pre = f"layer{i + 1}.{j}."
            h = bn(pre + "norm1", blk.norm1, su.composition(x, n_down if j == 0 else n_same, blk.conv1.kernel))
            side = x
            if blk.downsample is not None:
                side = bn(pre + "downsample.1", blk.downsample[1], su.composition(x, n_side, blk.downsample[0].kernel), relu=False)
            x = bn(pre + "norm2", blk.norm2, su.composition(h, n_same, blk.conv2.kernel), residual=side)
        outs.append(x)
    return outs


def test_train_step_against_the_torch_composition():
    rows, ends, feats = _inputs()
    model = _seeded(18, differentiable=True)
    maps = model.host_kernel_maps(rows, ends)
    rng = np.random.default_rng(3)
    G = [rng.standard_normal((maps["down", i][0].shape[0], 64 * 2 ** i)).astype(np.float32) for i in range(4)]
    refs = {dt: copy.deepcopy(model).to(dt).train() for dt in (torch.float64, torch.float32)}
    gpu = model.to(DEV).train()
    masks, hooks = {}, []
    for name, mod in gpu.named_modules():
        if isinstance(mod, (sparse.SparseBatchNorm, sparse.SparseInstanceNorm)):
            hooks.append(mod.register_forward_hook(lambda _m, _i, out, name=name: masks.__setitem__(name, (out.detach() > 0).cpu())))
    x = torch.from_numpy(feats).to(DEV).requires_grad_()
    outs = gpu(torch.from_numpy(rows).to(DEV), ends, x)
    sum((lv.feats * torch.from_numpy(g).to(DEV)).sum() for lv, g in zip(outs, G)).backward()
    for h in hooks:
        h.remove()
    assert len(masks) == 1 + 8 * 2 + 4

    wrt = ["conv1.kernel", "norm1.weight", "layer1.1.conv2.kernel", "layer1.0.norm1.bn.weight", "layer2.0.conv1.kernel",
           "layer2.0.downsample.1.bn.weight", "layer3.0.downsample.0.kernel", "layer3.1.norm2.bn.weight", "layer4.1.conv1.kernel",
           "layer4.0.norm2.bn.weight"]
    done = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)                       # an earlier test of the process may have left it at 1 (see the docstring)
    try:
        for dt, ref in refs.items():
            f = torch.from_numpy(feats).to(dt).requires_grad_()
            r_outs = _torch_network(ref, maps, f, masks)
            sum((o * torch.from_numpy(g).to(dt)).sum() for o, g in zip(r_outs, G)).backward()
            params = dict(ref.named_parameters())
            done[dt] = dict(outs=[o.detach().numpy() for o in r_outs], feats=f.grad.numpy(),
                            grads={k: params[k].grad.numpy() for k in wrt}, buffers={k: v.numpy() for k, v in ref.named_buffers()})
    finally:
        torch.set_num_threads(threads)
    r64, r32 = done[torch.float64], done[torch.float32]
    for l, lv in enumerate(outs):
        assert lv.feats.shape == r64["outs"][l].shape
        su.hold(f"train level {l} out", lv.feats.detach().cpu().numpy(), r32["outs"][l], r64["outs"][l])
    g_params = dict(gpu.named_parameters())
    for k in wrt:
        assert g_params[k].grad is not None and g_params[k].grad.shape == g_params[k].shape, k
        su.hold(f"train d {k}", g_params[k].grad.cpu().numpy(), r32["grads"][k], r64["grads"][k])
    su.hold("train d feats", x.grad.cpu().numpy(), r32["feats"], r64["feats"])
    for k, v in gpu.named_buffers():                         # the running statistics after the step
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
        elif k in ("layer1.0.norm1.bn.running_mean", "layer1.0.norm1.bn.running_var", "layer2.0.downsample.1.bn.running_var",
                   "layer3.1.norm2.bn.running_mean", "layer4.1.norm2.bn.running_var"):
            su.hold(f"train {k}", v.cpu().numpy(), r32["buffers"][k], r64["buffers"][k])


def test_train_mode_without_differentiable_raises():
    rows, ends, feats = _inputs()
    m = MinkResNet(18, 3, num_stages=1).to(DEV).train()
    with pytest.raises(NotImplementedError, match="inference-only by default"):
        m(torch.from_numpy(rows).to(DEV), ends, torch.from_numpy(feats).to(DEV))
    frozen = MinkResNet(18, 3, num_stages=1, differentiable=True).to(DEV).eval()       # frozen BatchNorm fine-tuning: nothing new
    out = frozen(torch.from_numpy(rows).to(DEV), ends, torch.from_numpy(feats).to(DEV))[0].feats
    out.sum().backward()
    assert frozen.layer1[0].conv1.kernel.grad is not None and frozen.layer1[0].norm1.bn.weight.grad is None
    assert frozen.norm1.weight.grad is not None and int(frozen.layer1[0].norm1.bn.num_batches_tracked) == 0
