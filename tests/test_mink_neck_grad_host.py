"""Training through the sparse neck, pinned without a GPU: the numpy restatements of the new backward pieces (``neck_host.py``,
``sparse_host.py``) in float64 against torch's own autograd on the CPU -- the generative transposed convolution against
``F.conv_transpose3d``, the ELU norm against ``F.elu(F.batch_norm(training=True))``, the union / prune routing against torch indexing,
the head against ``x @ W + b`` --, the NaN rule of the ELU's backward, the ABI surface of the new entry points, their argument checks and
workspace queries, the opt-in raises of ``MinkNeck(differentiable=True)``, and the near-tie count of the end-to-end inputs under the
TRAINING-mode scores (tests/test_gpu_mink_neck_grad.py relies on it)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import MinkNeck, _abi, neck, neck_host, sparse
from proxytransformation_amd.backbone import SparseLevel
from tests import neck_util as nu
from tests import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_ENTRY_POINTS = ("ptx_sparse_norm_fwd_act", "ptx_sparse_norm_bwd_act", "ptx_sparse_conv_transpose_gen_bwd_workspace_bytes",
                     "ptx_sparse_conv_transpose_gen_bwd", "ptx_neck_union_add_dest", "ptx_neck_rows_gather",
                     "ptx_neck_head_bwd_workspace_bytes", "ptx_neck_head_bwd")


def _close(got, ref, tol=1e-12):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64
    assert float(np.abs(got - ref).max()) <= tol * float(np.abs(ref).max()), float(np.abs(got - ref).max())


# ------------------------------------------------------------------------------------------------------------------ restatements
def test_generative_backward_restatement_is_torch_conv_transpose3d():
    """The dense 4x4x4 block of tests/test_mink_neck_host.py: the gradients of ``sum(out * G)`` through ``F.conv_transpose3d(stride=2)``
    with respect to the dense input and the kernel are ``conv_transpose_gen_bwd_host``'s ``dfeats`` / ``dkernel``."""
    rng = np.random.default_rng(11)
    cin, cout = 5, 7
    cells = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(64)]
    coords = np.concatenate([np.zeros((64, 1), np.int64), cells * 2], 1).astype(np.int32)
    x, kernel = rng.standard_normal((64, cin)), rng.standard_normal((8, cin, cout))
    oc, _, out = neck_host.conv_transpose_gen_host(coords, [64], 2, x, kernel)
    G = rng.standard_normal(out.shape)
    dense = np.zeros((1, cin, 4, 4, 4))
    dense[0][:, cells[:, 2], cells[:, 1], cells[:, 0]] = x.T
    td = torch.from_numpy(dense).requires_grad_()
    tk = torch.from_numpy(kernel).requires_grad_()
    w = tk.reshape(2, 2, 2, cin, cout).permute(3, 4, 0, 1, 2)
    ref = F.conv_transpose3d(td, w.contiguous(), stride=2)[0]
    (ref[:, oc[:, 3], oc[:, 2], oc[:, 1]].T * torch.from_numpy(G)).sum().backward()
    got = neck_host.conv_transpose_gen_bwd_host(G, x, kernel)
    _close(got["dfeats"], td.grad[0][:, cells[:, 2], cells[:, 1], cells[:, 0]].T)
    _close(got["dkernel"], tk.grad)
    g32 = neck_host.conv_transpose_gen_bwd_host(G.astype(np.float32), x, kernel)
    assert g32["dfeats"].dtype == np.float32 and g32["dkernel"].dtype == np.float32


@pytest.mark.parametrize("residual", [False, True])
def test_elu_norm_restatement_is_torch_batch_norm_and_elu(residual):
    rng = np.random.default_rng(12)
    n, C, eps = 300, 6, 1e-5
    x, g = rng.standard_normal((n, C)) * 2 + 0.5, rng.standard_normal((n, C))
    w, b, res = rng.uniform(0.5, 1.5, C), rng.standard_normal(C), rng.standard_normal((n, C))
    run = [rng.standard_normal(C), rng.uniform(0.5, 1.5, C)]
    tx, tw, tb, tr = (torch.from_numpy(a.copy()).requires_grad_() for a in (x, w, b, res))
    rm, rv = torch.from_numpy(run[0].copy()), torch.from_numpy(run[1].copy())
    y = F.batch_norm(tx, rm, rv, tw, tb, training=True, momentum=0.1, eps=eps)
    ref = F.elu(y + tr if residual else y)
    (ref * torch.from_numpy(g)).sum().backward()
    out = sparse.sparse_norm_host(x, [n], eps, w, b, res if residual else None, elu=True, running=run, momentum=0.1)
    _close(out, ref)
    _close(run[0], rm)
    _close(run[1], rv)
    assert 0.2 < float((out < 0).mean()) < 0.8
    got = sparse.sparse_norm_bwd_host(g, x, [n], eps, w, out=out, elu=True)
    _close(got["dx"], tx.grad, 1e-11)
    _close(got["dweight"], tw.grad, 1e-11)
    _close(got["dbias"], tb.grad, 1e-11)
    if residual:
        _close(got["dresidual"], tr.grad)
    with pytest.raises(ValueError, match="one activation"):
        sparse.sparse_norm_host(x, [n], eps, relu=True, elu=True)


def test_elu_backward_keeps_a_nan_and_is_zero_at_minus_one():
    """THE NaN RULE (include/proxyt.h): ``gy = g * (out > 0 ? 1 : out + 1)`` -- a NaN ``out`` gives a NaN ``gy``, never a dropped one (the
    ReLU's ``[NaN > 0]`` is 0); ``out == -1`` gives exactly 0."""
    out = np.array([[2.0, -1.0, np.nan, -0.25]], np.float32)
    g = np.array([[3.0, 5.0, 7.0, 8.0]], np.float32)
    x = np.zeros((1, 4), np.float32)
    gy = sparse.sparse_norm_bwd_host(g, x, [1], 1e-5, out=out, elu=True)["dresidual"]
    assert gy.dtype == np.float32 and gy[0, 0] == 3.0 and gy[0, 1] == 0.0 and np.isnan(gy[0, 2]) and gy[0, 3] == 6.0
    assert sparse.sparse_norm_bwd_host(g, x, [1], 1e-5, out=out, relu=True)["dresidual"][0, 2] == 0.0
    assert "NaN" in sparse.sparse_norm_bwd_host.__doc__
    header = open(os.path.join(ROOT, "include", "proxyt.h")).read()
    assert "THE NaN RULE" in header and "out > 0 ? 1 : out + 1" in header


def test_union_and_prune_routing_restatements_are_torch_indexing():
    a, a_ends, b, b_ends = nu.union_case()
    rng = np.random.default_rng(13)
    C = 3
    fa, fb = rng.standard_normal((len(a), C)), rng.standard_normal((len(b), C))
    uc, ue, u = neck_host.union_add_host(a, a_ends, fa, b, b_ends, fb)
    a_dest, b_dest = neck_host.union_dest_host(a, a_ends, b, b_ends)
    assert a_dest.dtype == np.int32 and a_dest.min() >= 0 and b_dest.min() >= 0
    assert np.array_equal(uc[a_dest], a) and np.array_equal(uc[b_dest], b)       # consistent with the returned coordinates
    assert len(np.unique(a_dest)) == len(a) and len(np.unique(b_dest)) == len(b)
    assert 0 < np.isin(b_dest, a_dest).sum() < len(b) and len(np.union1d(a_dest, b_dest)) == len(uc)
    ta, tb = torch.from_numpy(fa).requires_grad_(), torch.from_numpy(fb).requires_grad_()
    tu = torch.zeros(len(uc), C, dtype=torch.float64).index_add(0, torch.from_numpy(a_dest).long(), ta)
    tu = tu.index_add(0, torch.from_numpy(b_dest).long(), tb)
    _close(u, tu)
    scores = rng.standard_normal(len(uc))
    keep = neck_host.topk_keep_host(scores, ue, 40)
    dest = neck_host.prune_dest_host(keep)
    pc, pe, pf = neck_host.prune_host(keep, uc, ue, u)
    assert np.array_equal(dest >= 0, keep) and np.array_equal(dest[keep], np.arange(keep.sum())) and 0 < keep.sum() < len(keep)
    G = rng.standard_normal(pf.shape)
    (tu[torch.from_numpy(keep)] * torch.from_numpy(G)).sum().backward()
    dU = neck_host.rows_gather_host(G, dest)
    assert not np.signbit(dU[~keep]).any() and (dU[~keep] == 0).all()             # dropped rows: +0.0
    assert np.array_equal(neck_host.rows_gather_host(dU, a_dest), ta.grad.numpy())
    assert np.array_equal(neck_host.rows_gather_host(dU, b_dest), tb.grad.numpy())
    assert np.array_equal(neck_host.rows_gather_host(G, np.array([-1, 0, len(G)])), np.stack([G[0] * 0, G[0], G[0] * 0]))


@pytest.mark.parametrize("bias", [False, True])
def test_head_backward_restatement_is_torch_linear(bias):
    rng = np.random.default_rng(14)
    n, C, K = 37, 12, 5
    x, w, b, g = rng.standard_normal((n, C)), rng.standard_normal((1, C, K)), rng.standard_normal((1, K)), rng.standard_normal((n, K))
    tx, tw, tb = (torch.from_numpy(a).requires_grad_() for a in (x, w, b))
    cls = tx @ tw[0] + (tb if bias else 0)
    (cls * torch.from_numpy(g)).sum().backward()
    _close(neck_host.head_host(x, w[0], b if bias else None)[0], cls)
    got = neck_host.head_bwd_host(g, x, w)
    _close(got["dfeats"], tx.grad)
    _close(got["dweight"], tw.grad[0])
    if bias:
        _close(got["dbias"], tb.grad[0])


# ------------------------------------------------------------------------------------------------------------------ ABI surface
def test_header_binding_and_exports_declare_the_new_entry_points():
    lib = _abi.lib()
    hooks = ctypes.CDLL(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip_testhooks.so"))
    for name, params in su.assert_declared(GRAD_ENTRY_POINTS).items():
        assert len(params.split(",")) == len(_abi.SIGNATURES[name][1]), name
        getattr(hooks, name)
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13 and hooks.ptx_abi_version() == 13
    assert "neck_bwd.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()
    assert _abi.SIGNATURES["ptx_sparse_norm_fwd_act"] == _abi.SIGNATURES["ptx_sparse_norm_fwd"]


def test_workspace_queries_are_functions_of_the_shapes():
    lib = _abi.lib()
    gen, conv, head = (lib.ptx_sparse_conv_transpose_gen_bwd_workspace_bytes, lib.ptx_sparse_conv3d_bwd_workspace_bytes,
                       lib.ptx_neck_head_bwd_workspace_bytes)
    for n, cin, cout in ((65, 64, 64), (1, 1024, 512), (2357, 128, 128), (100000, 64, 64), (0, 64, 64)):
        assert gen(n, cin, cout) == gen(n, cin, cout) == conv(8 * n, 8, cin, cout) == su.dw_plan(8 * n, 8, cin, cout)[2] > 0
    assert gen(10, 1088, 64) == 0 and gen(10, 96, 64) == 0 and gen(10, 64, 576) == 0 and gen(-1, 64, 64) == 0 and gen(10, 3, 64) == 0
    assert gen((1 << 24) + 1, 64, 64) == 0
    # the convolution's backward takes the neck's widths; the plan restated by sparse_util.dw_plan is the library's there too
    for sh in ((2233, 27, 1024, 256), (2233, 27, 576, 64), (600, 27, 1024, 64), (100000, 27, 1024, 256)):
        assert conv(*sh) == su.dw_plan(*sh)[2] > 0, sh
    assert conv(1000, 27, 1088, 64) == 0 and conv(1000, 27, 1024, 576) == 0
    T = lambda n: -(-max(n, 1) // 256)                       # noqa: E731
    for n, C, K in ((1, 64, 1), (17, 256, 16), (2317, 512, 5), (0, 64, 1)):
        assert head(n, C, K) == head(n, C, K) == -(-(T(n) * (C * K + K) * 8) // 256) * 256 > 0       # double partials per 256-row tile
    assert head(10, 96, 1) == 0 and head(10, 576, 1) == 0 and head(10, 64, 0) == 0 and head(10, 64, 17) == 0 and head(-1, 64, 1) == 0


def test_argument_checks_answer_einval_before_touching_a_device():
    lib = _abi.lib()
    EINVAL = -1
    ends = lambda *e: (ctypes.c_int32 * len(e))(*e)          # noqa: E731
    fwd = lambda act, C=64: lib.ptx_sparse_norm_fwd_act(None, ends(10), 1, 10, C, 1e-5, None, None, None, act, None, None, 0.1, None, None,  # noqa: E731
                                                        None, 0, None)
    assert fwd(3) == EINVAL and b"ptx_sparse_norm_fwd_act: act=3" in lib.ptx_last_error()
    assert fwd(2, C=576) == EINVAL and b"ptx_sparse_norm_fwd_act: n=10 S=1 C=576" in lib.ptx_last_error()
    assert fwd(2) == EINVAL and b"ptx_sparse_norm_fwd_act: null" in lib.ptx_last_error()
    bwd = lambda act, out=None, C=64: lib.ptx_sparse_norm_bwd_act(16, 16, out, act, ends(10), 1, 10, C, None, None, None, None, None, None,  # noqa: E731
                                                                  None, 0, None)
    assert bwd(-1) == EINVAL and b"act=-1" in lib.ptx_last_error()
    assert bwd(2) == EINVAL and b"act=2 needs the forward's out" in lib.ptx_last_error()
    assert bwd(2, out=16, C=100) == EINVAL and b"ptx_sparse_norm_bwd_act: n=10 S=1 C=100" in lib.ptx_last_error()
    assert bwd(0) == EINVAL and b"stats" in lib.ptx_last_error()
    gen = lambda n, cin, cout: lib.ptx_sparse_conv_transpose_gen_bwd(None, None, n, None, cin, cout, None, None, None, 0, None)      # noqa: E731
    assert gen(10, 1088, 64) == EINVAL and b"ptx_sparse_conv_transpose_gen_bwd" in lib.ptx_last_error() and b"Cin=1088" in lib.ptx_last_error()
    assert gen(10, 64, 576) == EINVAL and b"Cout=576" in lib.ptx_last_error()
    assert gen((1 << 24) + 1, 64, 64) == EINVAL and b"n=16777217" in lib.ptx_last_error()
    assert gen(10, 64, 64) == EINVAL and b"g is null" in lib.ptx_last_error()
    conv = lib.ptx_sparse_conv3d_bwd(None, None, None, 0, None, 10, None, None, 10, 27, None, 1088, 64, None, None, None, None, None, None, 0, None)
    assert conv == EINVAL and b"ptx_sparse_conv3d_bwd: n_in=10 n_out=10 Cin=1088" in lib.ptx_last_error() and b"up to 1024" in lib.ptx_last_error()
    gather = lambda n, C, n_src=5: lib.ptx_neck_rows_gather(None, n_src, None, n, C, None, None)      # noqa: E731
    assert gather(10, 6) == EINVAL and b"C=6" in lib.ptx_last_error()
    assert gather(-1, 64) == EINVAL and b"n=-1" in lib.ptx_last_error()
    assert gather(10, 64) == EINVAL and b"null" in lib.ptx_last_error() and gather(0, 64) == 0
    head = lambda C, K, n=10: lib.ptx_neck_head_bwd(None, None, None, n, C, K, None, None, None, None, 0, None)      # noqa: E731
    assert head(100, 1) == EINVAL and b"C=100" in lib.ptx_last_error()
    assert head(256, 17) == EINVAL and b"num_classes=17" in lib.ptx_last_error()
    assert head(256, 1) == EINVAL and b"null" in lib.ptx_last_error() and head(256, 1, n=0) == 0
    union = lambda a, b, ad=16, ts=4, C=128: lib.ptx_neck_union_add_dest(None, a, None, None, b, None, 2, ts, C, None, None, None, None, ad, 16,  # noqa: E731
                                                                         None, 0, None)
    assert union(ends(1, 2), ends(1, 2), ad=None) == EINVAL and b"a_dest / b_dest is null" in lib.ptx_last_error()
    assert union(ends(5, 3), ends(1, 2)) == EINVAL and b"ptx_neck_union_add_dest: a_scene_end must not decrease" in lib.ptx_last_error()
    assert union(ends(1, 2), ends(1, 2), C=6) == EINVAL and b"ptx_neck_union_add_dest: C=6" in lib.ptx_last_error()


# ------------------------------------------------------------------------------------------------------------------ the opt-in rule
def test_differentiable_neck_raises_where_there_is_no_route():
    c = torch.zeros(4, 4, dtype=torch.int32)
    x = torch.zeros(4, 64)
    bn = torch.nn.BatchNorm1d(64)
    with pytest.raises(ValueError, match="elu and relu"):
        sparse.sparse_batch_norm(x, bn, relu=True, elu=True)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_batch_norm(x.clone().requires_grad_(), bn, elu=True)
    with pytest.raises(NotImplementedError, match="eval mode"):
        with torch.no_grad():
            sparse.sparse_batch_norm(x, bn.eval(), elu=True)
    with pytest.raises(NotImplementedError, match="raw product"):
        neck.conv_transpose_gen(c, [4], 2, x.clone().requires_grad_(), torch.zeros(8, 64, 64), act=neck_host.ACT_ELU, differentiable=True)
    with pytest.raises(ValueError, match="scores select rows"):
        neck.topk_prune(x[:, 0].clone().requires_grad_(), c, [4], x, 2, differentiable=True)
    for call in (lambda t: neck.conv_transpose_gen(c, [4], 2, t, torch.zeros(8, 64, 64), differentiable=True),
                 lambda t: neck.union_add(c, [4], t, c, [4], x, 2, differentiable=True),
                 lambda t: neck.topk_prune(x[:, 0], c, [4], t, 2, differentiable=True),
                 lambda t: neck.neck_head(t, torch.zeros(1, 64, 1), differentiable=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(x.clone().requires_grad_())
    levels = [SparseLevel(torch.zeros(4, 64), c, [4], 8), SparseLevel(torch.zeros(4, 128), c, [4], 16)]
    m = MinkNeck(1, [64, 128], 64, 0.01, 5, differentiable=True)
    assert m.differentiable and all(getattr(mod, "differentiable", True) for mod in m.modules())
    assert list(m.state_dict()) == list(MinkNeck(1, [64, 128], 64, 0.01, 5).state_dict())
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(levels, 1)                                         # training mode: the chain exists, a CPU path does not
    m.eval()
    with pytest.raises(NotImplementedError, match=r"bn\.train\(\)"):
        m(levels, 1)                                         # frozen BatchNorms, grads wanted
    with pytest.raises(RuntimeError, match="no CPU path"):
        with torch.no_grad():
            m(levels, 1)                                     # the folded route
    m.up_block_1[1].bn.train()
    with pytest.raises(NotImplementedError, match="some BatchNorms"):
        m(levels, 1)
    d = MinkNeck(1, [64, 128], 64, 0.01, 5)                  # the default module: today's raises
    assert not d.differentiable
    with pytest.raises(NotImplementedError, match="inference-only"):
        with torch.no_grad():
            d(levels, 1)
    with pytest.raises(NotImplementedError, match="backward"):
        d.eval()(levels, 1)


# ------------------------------------------------------------------------------------------------------------------ the end-to-end inputs
def test_end_to_end_inputs_have_few_near_ties_under_the_training_scores():
    """The near-tie precondition of tests/test_mink_neck_host.py re-checked for the TRAINING chain's scores (batch statistics instead of
    the running ones) on both end-to-end inputs of ``neck_util``: at most 2 % of k rows per pruned scene within ``NEAR_TIE * max |score|``
    of the step's k-th score, and pruning is active.  tests/test_gpu_mink_neck_grad.py's end-to-end test relies on it."""
    for levels, m, batch, k in ((nu.e2e_levels(), nu.e2e_neck(), 3, nu.K_PRUNE), (nu.e2e_levels_b(), nu.e2e_neck_b(), 4, nu.K_PRUNE_B)):
        trace = []
        feats, scores, _ = m.forward_host(levels, batch, np.float64, trace=trace, training=True)
        pruned = 0
        for step in trace:
            for scene, count, kth in nu.near_ties(step["scores"], step["scene_rows"], k):
                print(f"k = {k} rows {step['scene_rows']} scene {scene}: k-th score {kth:+.4f}, {count} near-ties")
                assert count <= 0.02 * k, (scene, count)
                pruned += 1
        assert len(trace) == 3 and pruned >= 3
        eval_scores = m.forward_host(levels, batch, np.float64)[1]
        assert not np.array_equal(np.concatenate(scores)[:8], np.concatenate(eval_scores)[:8])      # the training branch is another chain
