"""The norm kernels on the voxel rows (proxytransformation_amd/sparse.py, csrc/sparse_norm.hip): instance norm and training batch norm,
forward and backward, against the float64 restatement ``sparse_norm_host`` / ``sparse_norm_bwd_host`` under the rule of the
convolution's tests (``sparse_util.hold``: at most 8 x the error of the same fp32 chain on the CPU, which itself must be below 1e-5).

Segments of 256, 257, 0, 1 and 1000 rows (1514 in all): a full tile, a tile plus one row, an empty segment, a single row and a
partial last tile; widths 64 and 512.  The conditioning case puts the columns at +-16 with unit spread: the fp32 two-pass restatement
errs 2e-6 to 8e-6 of scale there and a tile-wise Chan merge below 1e-6, while E[x^2] - E[x]^2 in fp32 errs 1.6e-4 to 4.3e-4, so the
bar separates them by more than 20 x."""
import functools

import numpy as np
import pytest
import torch

from proxytransformation_amd import sparse
from tests import sparse_util as su

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEGMENTS = [256, 513, 513, 514, 1514]
N = SEGMENTS[-1]
EPS = sparse.INSTANCE_NORM_EPS


def t(a):
    return torch.from_numpy(a).to(DEV)


@functools.lru_cache(maxsize=None)
def _data(C, offset):
    return su.norm_operands(N, C, offset, 100 + C + offset)


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("C", [64, 512])
def test_conditioning_columns_far_from_zero(C):
    """(a) x = N(0,1) + 16 * (+-1 per column): what E[x^2] - E[x]^2 cannot do in fp32."""
    ops = _data(C, 16)
    got, stats = sparse.sparse_segment_norm(t(ops["x"]), SEGMENTS, EPS, return_stats=True)
    r32, r64 = su.norm_refs(ops, SEGMENTS, EPS)
    su.hold(f"norm conditioning C={C}", got.cpu().numpy(), r32, r64)
    su.hold_norm_stats(stats.cpu().numpy(), ops, SEGMENTS, EPS, (0, 1, 4), 16)


@pytest.mark.parametrize("C", [64, 512])
def test_affine_residual_relu_and_the_edge_segments(C):
    """(b), (e), (f): zero-mean data with weight, bias, residual and ReLU; two calls give equal bits; the empty segment's stats are zero,
    the one-row segment's output is bias + residual exactly."""
    ops = _data(C, 0)
    use = ("weight", "bias", "residual")
    call = lambda relu: sparse.sparse_segment_norm(t(ops["x"]), SEGMENTS, EPS, t(ops["weight"]), t(ops["bias"]), t(ops["residual"]), relu,  # noqa: E731
                                                   return_stats=True)
    got, stats = call(True)
    again, stats2 = call(True)
    assert got.dtype == torch.float32 and got.shape == (N, C)
    assert torch.equal(got, again) and torch.equal(stats, stats2), "two calls on the same inputs differ"
    r32, r64 = su.norm_refs(ops, SEGMENTS, EPS, use, True)
    su.hold(f"norm affine+residual+relu C={C}", got.cpu().numpy(), r32, r64)
    assert float(got.min()) == 0.0
    plain, _ = call(False)
    r32, r64 = su.norm_refs(ops, SEGMENTS, EPS, use, False)
    su.hold(f"norm affine+residual C={C}", plain.cpu().numpy(), r32, r64)
    stats = stats.cpu().numpy()
    assert stats.shape == (5, 2, C) and np.array_equal(stats[2], np.zeros((2, C), np.float32))
    assert np.array_equal(plain.cpu().numpy()[513], ops["bias"] + ops["residual"][513])
    assert np.array_equal(stats[3, 0], ops["x"][513])
    bare = sparse.sparse_instance_norm(t(ops["x"]), SEGMENTS)
    r32, r64 = su.norm_refs(ops, SEGMENTS, EPS)
    su.hold(f"instance norm C={C}", bare.cpu().numpy(), r32, r64)
    mod = sparse.SparseInstanceNorm(C).to(DEV)
    with torch.no_grad():
        assert torch.equal(mod(t(ops["x"]), SEGMENTS), bare)  # weight 1, bias 0: x * 1 + 0


@pytest.mark.parametrize("C", [64, 512])
def test_training_batch_norm_two_steps_against_torch(C):
    """(c) one segment with the running statistics, two consecutive steps, against nn.BatchNorm1d in float64 on the CPU (yardstick: the
    same module in float32 on the CPU)."""
    ops = _data(C, 0)
    bn64, bn32, gpu = su.bn_pair(C, 7)
    for step, rows in enumerate((slice(0, N), slice(200, 1101))):
        x = np.ascontiguousarray(ops["x"][rows]) * np.float32(1.5) + np.float32(0.25)
        with torch.no_grad():
            ref64 = bn64(torch.from_numpy(x).double()).numpy()
            ref32 = bn32(torch.from_numpy(x)).numpy()
            got = sparse.sparse_batch_norm(t(x), gpu)
        su.hold(f"batch norm C={C} step {step} out", got.cpu().numpy(), ref32, ref64)
        su.hold(f"batch norm C={C} step {step} running_mean", gpu.running_mean.cpu().numpy(), bn32.running_mean.numpy(), bn64.running_mean.numpy())
        su.hold(f"batch norm C={C} step {step} running_var", gpu.running_var.cpu().numpy(), bn32.running_var.numpy(), bn64.running_var.numpy())
        assert int(gpu.num_batches_tracked) == step + 1
    version = gpu.running_var._version
    with torch.no_grad():
        x = t(ops["x"])
        want = bn32.eval()(torch.from_numpy(ops["x"])).numpy()
        ref64 = bn64.eval()(torch.from_numpy(ops["x"]).double()).numpy()
        got = sparse.sparse_batch_norm(x, gpu.eval())           # eval: the affine map from the running statistics
        su.hold(f"batch norm C={C} eval", got.cpu().numpy(), want, ref64)
        assert gpu.running_var._version == version and int(gpu.num_batches_tracked) == 2
        scale, shift = sparse.bn_fold(gpu)
        assert sparse.bn_fold(gpu)[0] is scale                # cached
        gpu.train()
        sparse.sparse_batch_norm(x, gpu)
        assert sparse.bn_fold(gpu.eval())[0] is not scale     # the kernel's update is seen: the fold is rebuilt
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            sparse.sparse_batch_norm(x[:1], gpu.train())


# ------------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("C", [64, 512])
def test_backward_of_the_segment_norm(C):
    """(d), (e) for (b): dx, dweight, dbias, dresidual; dresidual is bit-equal to where(out > 0, g, 0); two backwards give equal bits."""
    ops = _data(C, 0)

    def step(relu, wrt):
        leaves = {k: t(ops[k]).requires_grad_(k in wrt) for k in ("x", "weight", "bias", "residual")}
        out = sparse.sparse_segment_norm(leaves["x"], SEGMENTS, EPS, leaves["weight"], leaves["bias"], leaves["residual"], relu,
                                         differentiable=True)
        out.backward(t(ops["g"]))
        return out.detach(), {k: v.grad for k, v in leaves.items()}

    every = ("x", "weight", "bias", "residual")
    out, grads = step(True, every)
    out2, grads2 = step(True, every)
    with torch.no_grad():
        assert torch.equal(out, sparse.sparse_segment_norm(t(ops["x"]), SEGMENTS, EPS, t(ops["weight"]), t(ops["bias"]), t(ops["residual"]), True))
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in every), "two backwards on the same inputs differ"
    out_np = out.cpu().numpy()
    assert 0.2 < float((out_np == 0).mean()) < 0.8
    assert np.array_equal(grads["residual"].cpu().numpy(), np.where(out_np > 0, ops["g"], np.float32(0)))
    assert grads["weight"].shape == (C,) and grads["x"].shape == (N, C)
    got = dict(dx=grads["x"].cpu().numpy(), dweight=grads["weight"].cpu().numpy(), dbias=grads["bias"].cpu().numpy(),
               dresidual=grads["residual"].cpu().numpy())
    su.hold_norm_grads(f"norm bwd relu C={C}", got, ops, SEGMENTS, EPS, out_np, True)
    # needs_input_grad is honoured: only what was asked for comes back, with the same bits
    _, only_x = step(True, ("x",))
    assert torch.equal(only_x["x"], grads["x"]) and only_x["weight"] is None and only_x["residual"] is None
    _, only_w = step(True, ("weight", "bias"))
    assert torch.equal(only_w["weight"], grads["weight"]) and torch.equal(only_w["bias"], grads["bias"]) and only_w["x"] is None
    # without ReLU: the gradient itself is dresidual
    out, grads = step(False, every)
    assert torch.equal(grads["residual"], t(ops["g"]))
    got = dict(dx=grads["x"].cpu().numpy(), dweight=grads["weight"].cpu().numpy(), dbias=grads["bias"].cpu().numpy())
    su.hold_norm_grads(f"norm bwd C={C}", got, ops, SEGMENTS, EPS, None, False)


@pytest.mark.parametrize("C", [64, 512])
def test_backward_of_the_training_batch_norm(C):
    """(d) for (c): one segment, through ``sparse_batch_norm`` and the module's own parameters, with residual and ReLU."""
    ops = _data(C, 0)
    _, _, gpu = su.bn_pair(C, 9)
    with torch.no_grad():
        gpu.weight.copy_(t(ops["weight"]))
    x, res = t(ops["x"]).requires_grad_(), t(ops["residual"]).requires_grad_()
    out = sparse.sparse_batch_norm(x, gpu, residual=res, relu=True, differentiable=True)
    out.backward(t(ops["g"]))
    out_np = out.detach().cpu().numpy()
    assert np.array_equal(res.grad.cpu().numpy(), np.where(out_np > 0, ops["g"], np.float32(0)))
    got = dict(dx=x.grad.cpu().numpy(), dweight=gpu.weight.grad.cpu().numpy(), dbias=gpu.bias.grad.cpu().numpy(), dresidual=res.grad.cpu().numpy())
    su.hold_norm_grads(f"batch norm bwd C={C}", got, ops, [N], gpu.eps, out_np, True)
    assert int(gpu.num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------------------------ surface
def test_opt_in_surface_and_rejections():
    """(g)"""
    x = torch.zeros(8, 64, device=DEV)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_instance_norm(x.clone().requires_grad_(), [8])
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_segment_norm(x, [8], 1e-5, weight=torch.ones(64, device=DEV, requires_grad=True))
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.SparseBatchNorm(64).to(DEV)(x)                # its own parameters require grad
    with pytest.raises(NotImplementedError, match="eval mode"):
        sparse.SparseBatchNorm(64, differentiable=True).to(DEV).eval()(x)
    with torch.no_grad():
        assert sparse.SparseBatchNorm(64).to(DEV).eval()(x).shape == (8, 64)
        with pytest.raises(ValueError, match="multiple of 64"):
            sparse.sparse_instance_norm(torch.zeros(8, 96, device=DEV), [8])
        with pytest.raises(ValueError, match="segment ends"):
            sparse.sparse_instance_norm(x, [5, 3])
        with pytest.raises(ValueError, match="residual must be"):
            sparse.sparse_segment_norm(x, [8], 1e-5, residual=torch.zeros(8, 128, device=DEV))
        with pytest.raises(ValueError, match="64 features"):
            sparse.sparse_batch_norm(torch.zeros(8, 128, device=DEV), torch.nn.BatchNorm1d(64).to(DEV))
        empty = sparse.sparse_segment_norm(torch.zeros(0, 64, device=DEV), [0, 0], 1e-5, return_stats=True)
        assert empty[0].shape == (0, 64) and float(empty[1].abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.sparse_instance_norm(torch.zeros(8, 64), [8])
