"""Sparse 3D convolution on the voxel rows (proxytransformation_amd/sparse.py, csrc/sparse.hip): the kernel maps bit for bit against
``kernel_map_host`` and ``pipeline.level_coordinates``; the gather-GEMM convolution, its epilogue and an eval BasicBlock composed of
the calls against the float64 restatement, with a bar measured in the test -- 8 x the error of the SAME fp32 chain computed on the
CPU (``sparse_conv3d_host`` in float32, resp. torch's dense fp32 ops for the block): both are fp32 sums of the same length and
differ only in summation order, a dropped term shows at 1e-2; the max-pool bit for bit; the rejections.

Rows (``tests/sparse_util.py``): a dense 6x6x6 block (all 27 neighbours present), ~2100 random rows in [-40,40)^3 * ts (most neighbours
missing; the row count is no multiple of the 64-row tile), an empty scene, and a last scene with one row."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import sparse
from tests import sparse_util as su
from tests.sparse_util import DEV

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ kernel map
@pytest.mark.parametrize("ts", [1, 4])
@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (1, 2), (2, 2)])
def test_kernel_map_is_the_host_restatement(k, s, ts):
    rows, ends = su.rows(ts)
    want_c, want_e, want_n = su.host_map(ts, k, s)
    km = su.device_map(ts, k, s)
    assert km.scene_rows == want_e and km.kernel_size == k and km.stride == s and km.tensor_stride == ts * s
    assert np.array_equal(km.coords.cpu().numpy(), want_c)
    assert km.nbr.dtype == torch.int32 and np.array_equal(km.nbr.cpu().numpy(), want_n)
    if (k, s) == (3, 1):
        n = want_n[:216]                                     # the dense block: its interior rows see all 27 neighbours
        assert (n >= 0).all(axis=1).sum() == 4 ** 3 and (want_n[216:-1] < 0).mean() > 0.9
    if s == 2:
        from proxytransformation_amd.pipeline import level_coordinates
        lc, _, le = level_coordinates(torch.from_numpy(rows).to(DEV), list(ends), 2 * ts, 0.01)
        assert le == km.scene_rows and torch.equal(lc, km.coords)


def test_kernel_map_rejects_a_coordinate_outside_the_key_range():
    """The range is checked where the coordinates are, on the device: the call raises before it returns a map, so nothing that
    would consume one is ever enqueued; the scratch stays good for the next call."""
    rows, ends = su.rows(1)
    bad = rows.copy()
    bad[300, 2] = 1 << 18
    for k, s in ((3, 1), (3, 2)):
        with pytest.raises(RuntimeError, match="ptx_sparse_kernel_map failed"):
            sparse.kernel_map(torch.from_numpy(bad).to(DEV), list(ends), 1, k, s)
    km = su.device_map(1, 3, 2)
    assert np.array_equal(km.nbr.cpu().numpy(), su.host_map(1, 3, 2)[2])
    with pytest.raises(RuntimeError, match="tensor_stride=3"):
        from proxytransformation_amd import _abi
        import ctypes
        e = (ctypes.c_int32 * 1)(4)
        _abi.check(_abi.lib().ptx_sparse_kernel_map(km.coords.data_ptr(), e, 1, 3, 3, 1, None, km.nbr.data_ptr(), km.nbr.data_ptr(),
                                                    km.nbr.data_ptr(), km.nbr.data_ptr(), 0, None), "ptx_sparse_kernel_map")


# ------------------------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("cin,cout,k,s", su.LAYER_SHAPES)
def test_convolution_against_the_float64_restatement(cin, cout, k, s):
    ts, cut = su.layer_rows(cin)                             # the 512-wide case: the random scene alone, cut to 600 rows
    _, _, nbr = su.host_map(ts, k, s, cut)
    km = su.device_map(ts, k, s, cut)
    assert np.array_equal(km.nbr.cpu().numpy(), nbr)
    n_in = su.rows(ts, cut)[0].shape[0]
    ops = su.operands(n_in, nbr.shape[0], cin, cout, k ** 3, seed=cin + cout)
    use = ("bias", "scale", "shift") if k == 1 else ()
    got = su.conv_run(km, ops, use)
    again = su.conv_run(km, ops, use)
    assert got.shape == (nbr.shape[0], cout) and got.dtype == torch.float32
    assert torch.equal(got, again), "two launches on the same inputs differ"
    r32, r64 = su.conv_refs(nbr, ops, use)
    su.hold(f"Cin={cin} Cout={cout} k={k} s={s} rows={n_in}->{nbr.shape[0]}", got.cpu().numpy(), r32, r64)
    if k == 1:                                               # 1x1 stride 2: a coarse cell without a row AT its corner has no neighbour
        lone = (nbr < 0).all(axis=1)
        assert lone.sum() > 100
        want = ops["bias"] * ops["scale"] + ops["shift"]      # fp32, two roundings
        assert np.array_equal(got.cpu().numpy()[lone], np.broadcast_to(want, (int(lone.sum()), cout)))


@pytest.mark.parametrize("use,relu", [(("bias",), False), (("scale", "shift"), True), (("residual",), False),
                                      (("bias", "scale", "shift", "residual"), True), ((), True)])
def test_epilogue_parts(use, relu):
    _, _, nbr = su.host_map(4, 3, 1)
    km = su.device_map(4, 3, 1)
    ops = su.operands(nbr.shape[0], nbr.shape[0], 64, 64, 27, seed=77)
    got = su.conv_run(km, ops, use, relu)
    r32, r64 = su.conv_refs(nbr, ops, use, relu)
    su.hold("epilogue " + "+".join(use) + ("+relu" if relu else ""), got.cpu().numpy(), r32, r64)
    if relu:
        assert float(got.min()) == 0.0


def test_module_forward_and_conversions():
    """SparseConv3d.forward = sparse_conv3d on its ``kernel`` / ``bias``; fp64 / non-contiguous inputs are converted."""
    _, _, nbr = su.host_map(4, 3, 2)
    km = su.device_map(4, 3, 2)
    n_in = su.rows(4)[0].shape[0]
    ops = su.operands(n_in, nbr.shape[0], 64, 128, 27, seed=5)
    m = sparse.SparseConv3d(64, 128, kernel_size=3, stride=2, bias=True).to(DEV).eval()
    m.load_state_dict({"kernel": torch.from_numpy(ops["weight"]), "bias": torch.from_numpy(ops["bias"]).view(1, -1)})
    with torch.no_grad():
        want = su.conv_run(km, ops, ("bias",))
        assert torch.equal(m(torch.from_numpy(ops["feats"]).to(DEV), km), want)
        wide = torch.from_numpy(np.concatenate([ops["feats"], ops["feats"]], 1)).to(DEV).double()
        assert torch.equal(m(wide[:, :64], km), want)
    with pytest.raises(ValueError, match="kernel map"):
        with torch.no_grad():
            m(torch.from_numpy(ops["feats"]).to(DEV), su.device_map(4, 3, 1))


def test_max_pool_is_the_restatement_bit_for_bit():
    _, _, nbr = su.host_map(4, 2, 2)
    km = su.device_map(4, 2, 2)
    feats = np.random.default_rng(9).standard_normal((su.rows(4)[0].shape[0], 64)).astype(np.float32)
    got = sparse.sparse_max_pool3d(torch.from_numpy(feats).to(DEV), km)
    assert np.array_equal(got.cpu().numpy(), sparse.sparse_max_pool3d_host(feats, nbr))
    assert np.isfinite(got.cpu().numpy()).all()


def test_rejections():
    km = su.device_map(4, 3, 1)
    n = km.nbr.shape[0]
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"ptx_sparse_conv3d: Cin=24 Cout=64"):
            sparse.sparse_conv3d(torch.zeros(n, 24, device=DEV), km, torch.zeros(27, 24, 64, device=DEV))
        with pytest.raises(RuntimeError, match=r"ptx_sparse_conv3d: Cin=64 Cout=96"):
            sparse.sparse_conv3d(torch.zeros(n, 64, device=DEV), km, torch.zeros(27, 64, 96, device=DEV))
        with pytest.raises(RuntimeError, match=r"ptx_sparse_max_pool3d: .*C=6"):
            sparse.sparse_max_pool3d(torch.zeros(n, 6, device=DEV), km)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_conv3d(torch.zeros(n, 64, device=DEV, requires_grad=True), km, torch.zeros(27, 64, 64, device=DEV))
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.SparseConv3d(64, 64, 3).to(DEV)(torch.zeros(n, 64, device=DEV), km)     # its own parameters require grad
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_max_pool3d(torch.zeros(n, 64, device=DEV, requires_grad=True), km)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.sparse_conv3d(torch.zeros(n, 64), km, torch.zeros(27, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.kernel_map(torch.zeros(4, 4, dtype=torch.int32), [4], 1, 3, 1)


# ------------------------------------------------------------------------------------------------------------------ composition
def _fold_bn(rng, c):
    gamma, beta = rng.uniform(0.5, 1.5, c), rng.standard_normal(c) * 0.2
    mean, var = rng.standard_normal(c) * 0.2, rng.uniform(0.5, 1.5, c)
    scale = gamma / np.sqrt(var + 1e-5)
    return scale.astype(np.float32), (beta - mean * scale).astype(np.float32)


def test_basic_block_against_dense_torch():
    """An eval BasicBlock (mink_resnet.py:88-119 with ME's resnet_block.BasicBlock): conv k3 s2 -> BN -> ReLU -> conv k3 s1 -> BN,
    + (1x1 s2 conv -> BN) of the input, -> ReLU, 64 -> 128, on ~2000 rows of tensor stride 4.  Reference: the float64 restatement;
    yardstick: the same block from torch's dense fp32 CPU ops on the densified grid, masked to the occupied cells after every layer."""
    ts, ext = 4, 12
    rng = np.random.default_rng(31)
    cells = np.stack(np.meshgrid(*[np.arange(-ext, ext)] * 3, indexing="ij"), -1).reshape(-1, 3)
    c3 = cells[rng.permutation(len(cells))[:2000]] * ts
    rows = np.concatenate([np.zeros((2000, 1), np.int64), c3], 1).astype(np.int32)
    ends = [2000]
    x = rng.standard_normal((2000, 64)).astype(np.float32)
    w1 = (rng.standard_normal((27, 64, 128)) / np.sqrt(27 * 64)).astype(np.float32)
    w2 = (rng.standard_normal((27, 128, 128)) / np.sqrt(27 * 128)).astype(np.float32)
    wd = (rng.standard_normal((1, 64, 128)) / np.sqrt(64)).astype(np.float32)
    (s1, b1), (s2, b2), (sd, bd) = _fold_bn(rng, 128), _fold_bn(rng, 128), _fold_bn(rng, 128)

    # the calls
    t = lambda a: torch.from_numpy(a).to(DEV)                # noqa: E731
    coords = t(rows)
    with torch.no_grad():
        m_down = sparse.kernel_map(coords, ends, ts, 3, 2)
        m_side = sparse.kernel_map(coords, ends, ts, 1, 2)
        m_same = sparse.kernel_map(m_down.coords, m_down.scene_rows, 2 * ts, 3, 1)
        assert torch.equal(m_side.coords, m_down.coords)
        h = sparse.sparse_conv3d(t(x), m_down, t(w1), scale=t(s1), shift=t(b1), relu=True)
        side = sparse.sparse_conv3d(t(x), m_side, t(wd), scale=t(sd), shift=t(bd))
        got = sparse.sparse_conv3d(h, m_same, t(w2), scale=t(s2), shift=t(b2), residual=side, relu=True).cpu().numpy()

    # float64 restatement
    oc, oe, n_down = sparse.kernel_map_host(rows, ends, ts, 3, 2)
    _, _, n_side = sparse.kernel_map_host(rows, ends, ts, 1, 2)
    _, _, n_same = sparse.kernel_map_host(oc, oe, 2 * ts, 3, 1)
    d = lambda a: a.astype(np.float64)                       # noqa: E731
    h64 = sparse.sparse_conv3d_host(d(x), n_down, d(w1), scale=d(s1), shift=d(b1), relu=True)
    side64 = sparse.sparse_conv3d_host(d(x), n_side, d(wd), scale=d(sd), shift=d(bd))
    ref64 = sparse.sparse_conv3d_host(h64, n_same, d(w2), scale=d(s2), shift=d(b2), residual=side64, relu=True)
    assert np.array_equal(m_down.coords.cpu().numpy(), oc)

    # dense fp32 torch on the CPU
    origin = -ext * ts
    def dense_w(w, k):
        return torch.from_numpy(w).reshape(k, k, k, w.shape[1], w.shape[2]).permute(4, 3, 2, 1, 0).contiguous()
    g = torch.zeros(1, 64, 2 * ext, 2 * ext, 2 * ext)
    gi = (c3 - origin) // ts
    g[0, :, gi[:, 0], gi[:, 1], gi[:, 2]] = torch.from_numpy(x.T.copy())
    oi = (oc[:, 1:].astype(np.int64) - origin) // (2 * ts)
    mask = torch.zeros(1, 1, ext, ext, ext)
    mask[0, 0, oi[:, 0], oi[:, 1], oi[:, 2]] = 1.0
    bn = lambda y, s, b: y * torch.from_numpy(s).view(1, -1, 1, 1, 1) + torch.from_numpy(b).view(1, -1, 1, 1, 1)      # noqa: E731
    hd = F.relu(bn(F.conv3d(g, dense_w(w1, 3), padding=1, stride=2), s1, b1)) * mask
    sided = bn(F.conv3d(g, dense_w(wd, 1), stride=2), sd, bd)
    outd = F.relu(bn(F.conv3d(hd, dense_w(w2, 3), padding=1), s2, b2) + sided) * mask
    ref32 = outd[0][:, oi[:, 0], oi[:, 1], oi[:, 2]].numpy().T
    su.hold("BasicBlock 64->128 rows=2000->%d" % oc.shape[0], got, ref32, ref64)
