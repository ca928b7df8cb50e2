"""The norm layers and the assembled MinkResNet (proxytransformation_amd/sparse.py, backbone.py), pinned without a GPU: the numpy
restatements ``sparse_norm_host`` / ``sparse_norm_bwd_host`` in float64 against torch's own ``F.instance_norm`` / ``F.batch_norm`` and
torch-CPU float64 autograd of the same composition; the ``state_dict`` of ``MinkResNet(34, 3)`` against a hand-written fixture of the
reference's names and shapes; ``forward_host`` on the rows of the convolution's tests; and the ABI surface of the new entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import MODELS, REGISTRY_BACKEND, MinkResNet, _abi, backbone, sparse
from tests import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_ENTRY_POINTS = ("ptx_sparse_norm_workspace_bytes", "ptx_sparse_norm_fwd", "ptx_sparse_norm_apply", "ptx_sparse_norm_bwd")
SEGMENTS = [256, 513, 513, 514, 1514]                        # rows 256, 257, 0, 1, 1000


def _close(got, ref, tol=1e-12):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64
    assert float(np.abs(got - ref).max()) <= tol * float(np.abs(ref).max()), float(np.abs(got - ref).max())


# ------------------------------------------------------------------------------------------------------------------ restatements
def test_norm_restatement_is_torch_instance_norm_per_scene():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1514, 64)) * 3 + rng.standard_normal(64) * 5
    w, b = rng.uniform(0.5, 1.5, (1, 64)), rng.standard_normal((1, 64))
    assert sparse.INSTANCE_NORM_EPS == 1e-8
    got, stats = sparse.sparse_norm_host(x, SEGMENTS, sparse.INSTANCE_NORM_EPS, w, b, return_stats=True)
    lo = 0
    for s, hi in enumerate(SEGMENTS):
        if hi - lo > 1:                                      # (torch refuses a single value per channel; see below)
            ref = F.instance_norm(torch.from_numpy(x[lo:hi].T.copy())[None], weight=torch.from_numpy(w[0]), bias=torch.from_numpy(b[0]),
                                  eps=1e-8)[0].T
            _close(got[lo:hi], ref)
            _close(stats[s, 0], x[lo:hi].mean(0))
            _close(stats[s, 1], 1 / np.sqrt(x[lo:hi].var(0) + 1e-8))
        lo = hi
    assert np.array_equal(stats[2], np.zeros((2, 64)))       # the empty segment
    assert np.array_equal(got[513], b[0])                    # the one-row segment: variance 0, the output is the bias
    res = rng.standard_normal(x.shape)
    full = sparse.sparse_norm_host(x, SEGMENTS, 1e-8, w, b, res, relu=True)
    assert np.array_equal(full, np.maximum(got + res, 0)) and full.dtype == np.float64
    assert sparse.sparse_norm_host(x.astype(np.float32), SEGMENTS, 1e-8, w, b).dtype == np.float32
    with pytest.raises(ValueError, match="segment ends"):
        sparse.sparse_norm_host(x, [256, 1000], 1e-8)


def test_norm_restatement_is_torch_batch_norm_in_training_mode():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((777, 128)) * 2 + 1
    bn = torch.nn.BatchNorm1d(128, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 1.5)
    rm0, rv0 = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    ref = bn(torch.from_numpy(x))
    run = (rm0.copy(), rv0.copy())
    got = sparse.sparse_norm_host(x, [777], bn.eps, bn.weight.detach().numpy(), bn.bias.detach().numpy(), running=run, momentum=0.1)
    _close(got, ref)
    _close(run[0], bn.running_mean)                          # the running statistics as the kernel updates them: the mean,
    _close(run[1], bn.running_var)                           # and the unbiased variance
    assert not np.array_equal(run[1], rv0)
    ref2 = bn(torch.from_numpy(x[:300]))                     # a second step, from the updated statistics
    _close(sparse.sparse_norm_host(x[:300], [300], bn.eps, bn.weight.detach().numpy(), bn.bias.detach().numpy(), running=run), ref2)
    _close(run[0], bn.running_mean)
    _close(run[1], bn.running_var)
    with pytest.raises(ValueError, match="at least 2 rows"):
        sparse.sparse_norm_host(x[:1], [1], bn.eps, running=run)


def test_norm_backward_restatement_equals_autograd():
    rng = np.random.default_rng(3)
    t = lambda a: torch.from_numpy(a).requires_grad_()       # noqa: E731
    x, res = t(rng.standard_normal((1514, 64)) + 2), t(rng.standard_normal((1514, 64)))
    w, b = t(rng.uniform(0.5, 1.5, 64)), t(rng.standard_normal(64))
    G = rng.standard_normal((1514, 64))
    for ends, eps in ((SEGMENTS, 1e-8), ([1514], 1e-5)):
        parts, lo = [], 0
        for hi in ends:
            if hi > lo:
                seg = x[lo:hi]
                mean = seg.mean(0, keepdim=True)
                var = ((seg - mean) ** 2).mean(0, keepdim=True)
                parts.append((seg - mean) / torch.sqrt(var + eps))
            lo = hi
        out = torch.relu(torch.cat(parts) * w + b + res)
        grads = torch.autograd.grad((out * torch.from_numpy(G)).sum(), (x, w, b, res))
        got = sparse.sparse_norm_bwd_host(G, x.detach().numpy(), ends, eps, w.detach().numpy(), out=out.detach().numpy(), relu=True)
        assert 0.2 < (out.detach().numpy() == 0).mean() < 0.8  # the mask is not trivial
        _close(got["dx"], grads[0])
        _close(got["dweight"], grads[1])
        _close(got["dbias"], grads[2])
        _close(got["dresidual"], grads[3])
    plain = sparse.sparse_norm_bwd_host(G, x.detach().numpy(), [1514], 1e-5)
    y = F.batch_norm(x, None, None, training=True, eps=1e-5)
    _close(plain["dx"], torch.autograd.grad((y * torch.from_numpy(G)).sum(), x)[0])
    assert plain["dresidual"] is not None and np.array_equal(plain["dresidual"], G)


# ------------------------------------------------------------------------------------------------------------------ the backbone
def test_state_dict_is_the_reference_layout():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "mink_resnet34_state_dict.json")))
    assert len(want) == 219
    sd = MinkResNet(34, 3).state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == want
    assert sum(k.endswith("conv1.kernel") or k.endswith("conv2.kernel") for k in sd) == 1 + 2 * 16
    sd18 = MinkResNet(18, 3).state_dict()
    assert sum(".conv1.kernel" in k for k in sd18) == 8 and len(sd18) == 3 + 8 * 12 + 4 * 6
    assert tuple(MinkResNet(18, 3, num_stages=2).state_dict()["layer2.0.downsample.0.kernel"].shape) == (1, 64, 128)
    for depth in (50, 101, 152):
        with pytest.raises(NotImplementedError, match="Bottleneck"):
            MinkResNet(depth, 3)
    with pytest.raises(KeyError):
        MinkResNet(20, 3)
    m = MinkResNet(18, 3)
    assert isinstance(m.norm1, sparse.SparseInstanceNorm) and bool((m.norm1.weight == 1).all()) and bool((m.norm1.bias == 0).all())
    k = m.layer2[0].conv1.kernel
    assert abs(float(k.detach().std()) / (2.0 / (27 * 128)) ** 0.5 - 1) < 0.05      # kaiming normal, fan_out
    m.layer1[0].norm1.bn.weight.data.fill_(3.0)
    m.init_weights()
    assert float(m.layer1[0].norm1.bn.weight.detach()[0]) == 1.0
    if REGISTRY_BACKEND != "embodiedscan":
        assert MODELS.get("MinkResNet") is MinkResNet
        assert isinstance(MODELS.build(dict(type="MinkResNet", depth=18, in_channels=3)), MinkResNet)


def test_batchnorm_environment_switch(monkeypatch):
    monkeypatch.setenv("BATCHNORM", "1")
    m = MinkResNet(18, 3, num_stages=1)
    assert isinstance(m.norm1, sparse.SparseBatchNorm) and "norm1.bn.running_var" in m.state_dict()
    monkeypatch.setenv("BATCHNORM", "0")
    assert isinstance(MinkResNet(18, 3, num_stages=1).norm1, sparse.SparseInstanceNorm)


def test_forward_host_levels():
    rows, ends = su.rows(1)
    torch.manual_seed(0)
    m = MinkResNet(18, 3).eval()
    feats = np.random.default_rng(4).standard_normal((rows.shape[0], 3))
    levels = m.forward_host(rows, list(ends), feats, np.float64)
    assert [lv.tensor_stride for lv in levels] == [8, 16, 32, 64]
    c, e, ts = rows, list(ends), 1
    for step in range(2):                                    # the stem and the pool
        c, e, _ = sparse.kernel_map_host(c, e, ts, 3 if step == 0 else 2, 2)
        ts *= 2
    for l, lv in enumerate(levels):
        c, e, _ = sparse.kernel_map_host(c, e, ts, 3, 2)
        ts *= 2
        assert np.array_equal(lv.coords, c) and lv.scene_rows == e and lv.coords.dtype == np.int32
        assert lv.feats.shape == (c.shape[0], 64 * 2 ** l) and lv.feats.dtype == np.float64
        assert np.isfinite(lv.feats).all() and float(lv.feats.min()) == 0.0 and float(lv.feats.max()) > 0
        assert lv.scene_rows[2] == lv.scene_rows[1]            # the empty scene stays empty
        assert lv.scene_rows[3] == lv.scene_rows[2] + 1        # the one-row scene keeps its row
        assert (lv.coords[:, 1:] % lv.tensor_stride == 0).all()
    lv32 = m.forward_host(rows, list(ends), feats, np.float32)
    assert lv32[3].feats.dtype == np.float32
    assert float(np.abs(lv32[3].feats - levels[3].feats).max()) < 1e-4 * float(np.abs(levels[3].feats).max())


# ------------------------------------------------------------------------------------------------------------------ ABI surface
def test_header_binding_and_exports_declare_the_norm_entry_points():
    lib = _abi.lib()
    hooks = ctypes.CDLL(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip_testhooks.so"))
    for name, params in su.assert_declared(NORM_ENTRY_POINTS).items():
        assert len(params.split(",")) == len(_abi.SIGNATURES[name][1]), name
        getattr(hooks, name)
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13 and hooks.ptx_abi_version() == 13
    assert "sparse_norm.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()
    ws = lib.ptx_sparse_norm_workspace_bytes
    assert ws(400000, 6, 64) > 0 and ws(0, 1, 512) > 0 and ws(1514, 64, 64) > 0
    assert ws(100, 1, 32) == 0 and ws(100, 1, 96) == 0 and ws(100, 1, 576) == 0 and ws(100, 0, 64) == 0 and ws(100, 65, 64) == 0
    assert ws(-1, 1, 64) == 0 and ws(1514, 5, 64) == ws(1514, 5, 64)
    assert ws(400000, 6, 64) <= 2 * 4 * 64 * (400000 // 256 + 6) + 2 * (2 * 4 * 64 * 6) + 1024      # two floats per tile and column; a segment's means, its sums


def test_norm_workspace_is_the_restated_tile_bound():
    """``sparse_util.norm_plan`` restates the norms' private workspace plan (at most n // 256 + S tiles); the library's total is its at
    the segment layouts of tests/test_gpu_sparse_regimes.py, whose tile counts -- 17 and 34 per segment, 96 -- are what that module is
    about and stay inside the bound."""
    ws = _abi.lib().ptx_sparse_norm_workspace_bytes
    tiles = {name: su.seg_tiles(sizes) for name, sizes in su.NORM_REGIMES.items()}
    assert tiles["four"] == [17, 0, 34, 1] and tiles["sixty-four"][:4] == tiles["four"] and tiles["one"] == [96]
    assert [sum(s) for s in su.NORM_REGIMES.values()] == [12598, 27645, 24548] and len(su.NORM_REGIMES["sixty-four"]) == 64
    assert [-(-t // 16) for t in (17, 34, 96)] == [2, 3, 6]    # tiles per slot run
    for name, sizes in su.NORM_REGIMES.items():
        n, S = sum(sizes), len(sizes)
        for C in (64, 128):
            bound, total = su.norm_plan(n, S, C)
            assert sum(tiles[name]) <= bound == n // 256 + S and ws(n, S, C) == total, (name, C)
    assert ws(400000, 6, 64) == su.norm_plan(400000, 6, 64)[1] and ws(0, 1, 512) == su.norm_plan(0, 1, 512)[1]


def test_norm_argument_checks_answer_einval_before_touching_a_device():
    lib = _abi.lib()
    EINVAL = -1
    ends = lambda *e: (ctypes.c_int32 * len(e))(*e)          # noqa: E731
    fwd = lambda seg, S, n, C, eps=1e-5, rm=None, rv=None, mom=0.1, stats=None: lib.ptx_sparse_norm_fwd(     # noqa: E731
        None, seg, S, n, C, eps, None, None, None, 0, rm, rv, mom, stats, None, None, 0, None)
    assert fwd(ends(100), 1, 100, 64) == EINVAL and b"null" in lib.ptx_last_error()          # every device pointer null
    assert fwd(ends(100), 1, 100, 96) == EINVAL and b"C=96" in lib.ptx_last_error()
    assert fwd(ends(100), 1, 100, 576) == EINVAL
    assert fwd(ends(100), 0, 100, 64) == EINVAL and fwd(ends(*[1] * 65), 65, 1, 64) == EINVAL
    assert fwd(None, 1, 100, 64) == EINVAL and b"seg_end" in lib.ptx_last_error()
    assert fwd(ends(60, 50, 100), 3, 100, 64) == EINVAL and b"ascend" in lib.ptx_last_error()
    assert fwd(ends(50, 90), 2, 100, 64) == EINVAL and b"n = 100" in lib.ptx_last_error()
    assert fwd(ends(100), 1, -1, 64) == EINVAL
    assert fwd(ends(100), 1, 100, 64, eps=-1.0, stats=16) == EINVAL and b"eps" in lib.ptx_last_error()
    assert fwd(ends(100), 1, 100, 64, rm=16, stats=16) == EINVAL and b"together" in lib.ptx_last_error()
    assert fwd(ends(50, 100), 2, 100, 64, rm=16, rv=16, stats=16) == EINVAL and b"one segment" in lib.ptx_last_error()
    assert fwd(ends(1), 1, 1, 64, rm=16, rv=16, stats=16) == EINVAL and b"at least 2 rows" in lib.ptx_last_error()
    assert fwd(ends(0), 1, 0, 64, stats=8) == EINVAL and b"aligned" in lib.ptx_last_error()
    apply_ = lambda seg, S, n, C: lib.ptx_sparse_norm_apply(None, seg, S, n, C, None, None, None, None, 0, None, None)      # noqa: E731
    assert apply_(ends(100), 1, 100, 64) == EINVAL and apply_(ends(100), 1, 100, 100) == EINVAL and apply_(ends(99), 1, 100, 64) == EINVAL
    bwd = lambda seg, S, n, C: lib.ptx_sparse_norm_bwd(None, None, None, seg, S, n, C, None, None, None, None, None, None, None, 0, None)  # noqa: E731
    assert bwd(ends(100), 1, 100, 64) == EINVAL and b"null" in lib.ptx_last_error()
    assert bwd(ends(100), 1, 100, 48) == EINVAL and bwd(ends(10, 5), 2, 5, 64) == EINVAL and bwd(None, 1, 100, 64) == EINVAL


def test_norms_stay_inference_only_by_default_and_have_no_cpu_path():
    x = torch.zeros(4, 64)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_instance_norm(torch.zeros(4, 64, requires_grad=True), [4])
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.SparseInstanceNorm(64)(x, [4])                # its own parameters require grad
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.SparseBatchNorm(64)(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.sparse_instance_norm(x, [4])
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.SparseBatchNorm(64, differentiable=True)(x)
    bn = torch.nn.BatchNorm1d(64, momentum=None)
    with pytest.raises(ValueError, match="momentum=None"):
        sparse.sparse_batch_norm(x, bn)
    with pytest.raises(ValueError, match="track_running_stats"):
        sparse.sparse_batch_norm(x, torch.nn.BatchNorm1d(64, track_running_stats=False))
    m = MinkResNet(18, 3, num_stages=1)
    assert not m.differentiable and MinkResNet(18, 3, num_stages=1, differentiable=True).layer1[0].conv2.differentiable
    assert sparse.SparseBatchNorm(64).bn.momentum == 0.1 and sparse.SparseBatchNorm(64).bn.eps == 1e-5
    with pytest.raises(RuntimeError, match="no CPU path"):
        with torch.no_grad():
            m(torch.zeros(4, 4, dtype=torch.int32), [4], torch.zeros(4, 3))
    assert backbone.SparseLevel(None, None, [0], 8).tensor_stride == 8


def test_bn_fold_of_a_batch_norm_made_under_inference_mode():
    """Inference tensors have no version counter to key the cache on: the fold is rebuilt per call instead of failing."""
    with torch.inference_mode():
        bn = torch.nn.BatchNorm1d(64).eval()
        bn.running_mean.normal_(generator=torch.Generator().manual_seed(1))
        scale, shift = sparse.bn_fold(bn)
        assert torch.allclose(scale, bn.weight / torch.sqrt(bn.running_var + bn.eps))
        assert torch.allclose(shift, bn.bias - bn.running_mean * scale)
        bn.running_mean.zero_()
        assert torch.equal(sparse.bn_fold(bn)[1], torch.zeros(64))
