"""The backward of the sparse convolution and max-pool (proxytransformation_amd/sparse.py), pinned without a GPU: the numpy restatements
``sparse_conv3d_bwd_host`` / ``sparse_max_pool3d_bwd_host`` / ``kernel_map_transpose_host`` in float64 against torch-CPU float64 AUTOGRAD
of the composition written out here independently (27 x ``index_select`` + ``mm``, resp. dense ``F.conv3d`` on the densified grid), the
smallest-``j`` tie rule of the pool, and the ABI / opt-in surface of the new entry points."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import _abi, sparse
from tests import sparse_util as su

BWD_ENTRY_POINTS = ("ptx_sparse_kernel_map_transpose", "ptx_sparse_conv3d_bwd_workspace_bytes", "ptx_sparse_conv3d_bwd",
                    "ptx_sparse_max_pool3d_arg", "ptx_sparse_max_pool3d_bwd")


def _close(got, ref):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape and got.dtype == np.float64
    assert float(np.abs(got - ref).max()) <= 1e-12 * float(np.abs(ref).max()), float(np.abs(got - ref).max())


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (1, 2), (2, 2)])
def test_conv_backward_restatement_equals_autograd_of_the_composition(k, s):
    ts, cin, cout = 4, 8, 12
    coords, ends = su.random_rows(21 + k + s, ts)
    _, _, nbr = sparse.kernel_map_host(coords, ends, ts, k, s)
    rng = np.random.default_rng(3)
    t = lambda a: torch.from_numpy(a).requires_grad_()       # noqa: E731
    feats, weight = t(rng.standard_normal((coords.shape[0], cin))), t(rng.standard_normal((k ** 3, cin, cout)) / np.sqrt(k ** 3 * cin))
    bias, residual = t(rng.standard_normal((1, cout))), t(rng.standard_normal((nbr.shape[0], cout)))
    scale, shift = torch.from_numpy(rng.uniform(0.5, 1.5, cout)), torch.from_numpy(rng.standard_normal(cout))
    G = rng.standard_normal((nbr.shape[0], cout))
    for full in (True, False):                               # the whole epilogue with ReLU, and the bare convolution
        kw = dict(bias=bias, scale=scale, shift=shift, residual=residual, relu=True) if full else {}
        out = su.composition(feats, nbr, weight, **kw)
        wrt = (feats, weight, bias, residual) if full else (feats, weight)
        grads = torch.autograd.grad((out * torch.from_numpy(G)).sum(), wrt)
        got = sparse.sparse_conv3d_bwd_host(G, feats.detach().numpy(), nbr, weight.detach().numpy(), out=out.detach().numpy() if full else None,
                                            scale=scale.numpy() if full else None, relu=full, has_bias=full, has_residual=full)
        _close(got["dfeats"], grads[0])
        _close(got["dweight"], grads[1])
        if full:
            assert (out.detach().numpy() == 0).mean() > 0.2     # the mask is not trivial
            _close(got["dbias"], grads[2].reshape(-1))
            _close(got["dresidual"], grads[3])
        else:
            assert got["dbias"] is None and got["dresidual"] is None
    if (k, s) == (1, 2):
        assert (nbr < 0).all(axis=1).any()                   # rows without a neighbour: they feed dbias / dresidual only


def test_conv_backward_restatement_equals_dense_conv3d_autograd():
    k, s, ts, cin, cout = 3, 1, 4, 6, 10
    coords, ends = su.random_rows(14, ts)
    out_c, out_ends, nbr = sparse.kernel_map_host(coords, ends, ts, k, s)
    rng = np.random.default_rng(8)
    feats = rng.standard_normal((coords.shape[0], cin))
    weight = rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)
    G = rng.standard_normal((nbr.shape[0], cout))
    got = sparse.sparse_conv3d_bwd_host(G, feats, nbr, weight)
    origin = -4 * ts
    w_t = torch.from_numpy(weight).requires_grad_()
    wd = w_t.reshape(k, k, k, cin, cout).permute(4, 3, 2, 1, 0)      # [cout][cin][x][y][z], x fastest in the offset index
    dfeats = np.zeros_like(feats)
    dweight = torch.zeros_like(w_t)
    lo = 0
    for e in ends:
        c3 = (coords[lo:e, 1:].astype(np.int64) - origin) // ts
        f_t = torch.from_numpy(feats[lo:e]).requires_grad_()
        grid = torch.zeros(8, 8, 8, cin, dtype=torch.float64).index_put(tuple(torch.from_numpy(c3[:, d]) for d in range(3)), f_t)
        dense = F.conv3d(grid.permute(3, 0, 1, 2)[None], wd, padding=1)
        rows = dense[0][:, c3[:, 0], c3[:, 1], c3[:, 2]].T     # stride 1: the output rows are the input rows
        gf, gw = torch.autograd.grad((rows * torch.from_numpy(G[lo:e])).sum(), (f_t, w_t))
        dfeats[lo:e] = gf.numpy()
        dweight = dweight + gw
        lo = e
    _close(got["dfeats"], dfeats)
    _close(got["dweight"], dweight)


@pytest.mark.parametrize("k,s", [(2, 2), (3, 1)])
def test_pool_backward_restatement_equals_autograd_of_the_stacked_max(k, s):
    ts = 4
    coords, ends = su.random_rows(5, ts)
    _, _, nbr = sparse.kernel_map_host(coords, ends, ts, k, s)
    rng = np.random.default_rng(2)
    feats = rng.standard_normal((coords.shape[0], 8))         # continuous draws: no ties
    G = rng.standard_normal((nbr.shape[0], 8))
    f_t = torch.from_numpy(feats).requires_grad_()
    idx = torch.from_numpy(nbr).long()
    stacked = f_t[idx.clamp(min=0)].masked_fill((idx < 0).unsqueeze(-1), -np.inf)      # (n_out, kvol, C)
    out = stacked.max(dim=1).values
    assert np.array_equal(out.detach().numpy(), sparse.sparse_max_pool3d_host(feats, nbr))
    (ref,) = torch.autograd.grad((out * torch.from_numpy(G)).sum(), f_t)
    got = sparse.sparse_max_pool3d_bwd_host(G, feats, nbr)
    _close(got, ref)                                         # overlapping windows (k3 s1): several outputs add into one row, in some order
    if (k, s) == (2, 2):
        assert np.array_equal(got, ref.numpy())              # disjoint windows: one term per element, exact
    else:
        assert ((sparse.kernel_map_transpose_host(nbr, len(feats)) >= 0).sum(1) > 1).any()


def test_pool_backward_ties_go_to_the_smallest_offset():
    nbr = np.array([[1, 0]], np.int32)                        # offset 0 reads row 1, offset 1 reads row 0
    feats = np.array([[2.0, 5.0, -1.0, 0.0], [2.0, 3.0, -1.0, 0.5]])
    G = np.array([[10.0, 20.0, 30.0, 40.0]])
    got = sparse.sparse_max_pool3d_bwd_host(G, feats, nbr)
    assert got.tolist() == [[0.0, 20.0, 0.0, 0.0], [10.0, 0.0, 30.0, 40.0]]       # the ties (channels 0, 2) go to j = 0, i.e. row 1
    assert "smallest" in sparse.sparse_max_pool3d_bwd_host.__doc__ and "smallest" in sparse.sparse_max_pool3d.__doc__


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (1, 2), (2, 2)])
def test_transposed_map_inverts_the_map(k, s):
    ts = 2
    coords, ends = su.random_rows(9, ts, counts=(200, 1, 90))
    _, _, nbr = sparse.kernel_map_host(coords, ends, ts, k, s)
    n_in = coords.shape[0]
    nbr_t = sparse.kernel_map_transpose_host(nbr, n_in)
    assert nbr_t.shape == (n_in, k ** 3) and nbr_t.dtype == np.int32
    o, j = np.nonzero(nbr >= 0)
    assert len(np.unique(nbr[o, j].astype(np.int64) * k ** 3 + j)) == len(o)      # no (i, j) is claimed twice
    assert np.array_equal(nbr_t[nbr[o, j], j], o)              # every present (o, j) round-trips
    assert (nbr_t >= 0).sum() == len(o)                        # and every other entry is -1
    assert ((nbr_t >= 0) | (nbr_t == -1)).all()
    clipped = sparse.kernel_map_transpose_host(nbr, n_in - 50)
    assert np.array_equal(clipped, np.where(nbr_t[:n_in - 50] >= 0, nbr_t[:n_in - 50], -1)) and clipped.shape[0] == n_in - 50


def test_header_binding_and_exports_declare_the_backward_entry_points():
    su.assert_declared(BWD_ENTRY_POINTS)
    lib = _abi.lib()
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13
    assert len(_abi.SIGNATURES["ptx_sparse_conv3d_bwd"][1]) == 21 and len(_abi.SIGNATURES["ptx_sparse_kernel_map_transpose"][1]) == 6
    ws = lib.ptx_sparse_conv3d_bwd_workspace_bytes
    assert ws(100000, 27, 64, 64) > 0 and ws(600, 27, 512, 512) > 0 and ws(5000, 27, 3, 64) > 0 and ws(0, 1, 64, 64) > 0
    assert ws(1000, 27, 16, 64) == 0 and ws(1000, 27, 64, 96) == 0 and ws(1000, 8, 3, 64) == 0 and ws(1000, 9, 64, 64) == 0
    assert ws(1000, 27, 64, 64) == ws(1000, 27, 64, 64)        # a function of the shapes only
    assert ws(2_000_000, 27, 512, 512) <= (256 << 20) + 28 * (1 << 20) + 8 * (1 << 20)     # bounded: 256 MiB of slabs + one + the tiles


def test_dweight_plan_restatement_is_the_library_s():
    """``sparse_util.dw_plan`` restates the library's private split of dweight over the rows; its workspace total is the library's at the
    shapes of the layer tests and of ``DW_REGIMES``, and at the latter it gives the chunk sizes tests/test_gpu_sparse_regimes.py is
    about: more than the 1024 rows of one compaction round, in 1, 2 and 5 chunks.  A changed plan fails here, not silently there."""
    ws = _abi.lib().ptx_sparse_conv3d_bwd_workspace_bytes
    shapes = []
    for cin, cout, k, s in su.LAYER_SHAPES:
        ts, cut = su.layer_rows(cin)
        n_out = su.host_map(ts, k, s, cut)[2].shape[0]
        shapes.append((n_out, k ** 3, cin, cout))
    assert [su.dw_plan(*sh)[:2] for sh in shapes] == [(1024, 3), (256, 10), (256, 9), (256, 9), (640, 1)]
    for name, c in su.DW_REGIMES.items():
        n = sum(c["counts"])
        R, S, _ = su.dw_plan(n, 27, c["cin"], c["cout"])
        assert (R, S) == (c["R"], c["S"]) and R > 1024 and (S - 1) * R < n <= S * R, name
        assert su.dense_map(name)[0].shape[0] == n
        shapes.append((n, 27, c["cin"], c["cout"]))
    assert [su.DW_REGIMES[k]["S"] for k in ("512->512", "256->512", "stem")] == [1, 2, 5]
    assert su.DW_REGIMES["stem"]["R"] // 4 == 272 and 272 % 64 != 0       # the stem's wave quarter, off the 64-row grid
    for sh in shapes + [(0, 1, 64, 64), (400000, 27, 64, 64), (2_000_000, 27, 512, 512), (100000, 8, 64, 128)]:
        assert ws(*sh) == su.dw_plan(*sh)[2] > 0, sh


def test_default_stays_inference_only_and_there_is_no_cpu_path():
    km = sparse.KernelMap(coords=torch.zeros(2, 4, dtype=torch.int32), scene_rows=[2], nbr=torch.zeros(2, 1, dtype=torch.int32),
                          kernel_size=1, stride=1, tensor_stride=1)
    assert km.nbr_t is None
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_conv3d(torch.zeros(2, 64, requires_grad=True), km, torch.zeros(1, 64, 64))
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_max_pool3d(torch.zeros(2, 64, requires_grad=True), km)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.SparseConv3d(64, 64, 1)(torch.zeros(2, 64), km)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.sparse_conv3d(torch.zeros(2, 64, requires_grad=True), km, torch.zeros(1, 64, 64), differentiable=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.sparse_max_pool3d(torch.zeros(2, 64, requires_grad=True), km, differentiable=True)
    m = sparse.SparseConv3d(64, 64, 1, differentiable=True)
    assert m.differentiable and not sparse.SparseConv3d(64, 64, 1).differentiable
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 64), km)
    with pytest.raises(ValueError, match="scale"):
        sparse.sparse_conv3d(torch.zeros(2, 64), km, torch.zeros(1, 64, 64), scale=torch.ones(64, requires_grad=True), differentiable=True)
