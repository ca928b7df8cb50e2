"""The semantics of the sparse convolution (proxytransformation_amd/sparse.py), pinned without a GPU: the numpy restatements
``kernel_map_host`` / ``sparse_conv3d_host`` / ``sparse_max_pool3d_host`` against dense ``F.conv3d`` / ``F.max_pool3d`` on the densified
grid in float64, the stride-2 output rows against the coarsening rule, and the ABI / nn.Module surface of the new entry points."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import _abi, sparse
from tests import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ptx_sparse_kernel_map_workspace_bytes", "ptx_sparse_kernel_map", "ptx_sparse_conv3d", "ptx_sparse_max_pool3d")


def _densify(c3, feats, origin, ts, size, fill=0.0):
    """(n,3) coordinates + (n,C) features -> (1,C,X,Y,Z) float64 grid in units of ts from ``origin``."""
    g = torch.full((1, feats.shape[1], size, size, size), fill, dtype=torch.float64)
    idx = (c3 - origin) // ts
    g[0, :, idx[:, 0], idx[:, 1], idx[:, 2]] = torch.from_numpy(np.ascontiguousarray(feats.T))
    return g


def _dense_weight(weight, k):
    """wd[:, :, x, y, z] = weight[z*k*k + y*k + x].T  (x fastest in the offset index)"""
    kvol, cin, cout = weight.shape
    wd = torch.from_numpy(weight).reshape(k, k, k, cin, cout)        # [z][y][x][cin][cout]
    return wd.permute(4, 3, 2, 1, 0).contiguous()                   # [cout][cin][x][y][z]


@pytest.mark.parametrize("k,s,ts,cin,cout", [(3, 2, 1, 3, 64), (3, 1, 4, 64, 64), (1, 2, 4, 64, 128), (3, 2, 4, 64, 128), (3, 1, 8, 512, 512)])
def test_restatement_equals_dense_conv3d(k, s, ts, cin, cout):
    coords, ends = su.random_rows(11 + k + s + ts, ts, counts=(230, 120) if cin < 512 else (150,))
    rng = np.random.default_rng(5)
    feats = rng.standard_normal((coords.shape[0], cin))
    weight = rng.standard_normal((k ** 3, cin, cout)) / np.sqrt(k ** 3 * cin)
    out_c, out_ends, nbr = sparse.kernel_map_host(coords, ends, ts, k, s)
    got = sparse.sparse_conv3d_host(feats, nbr, weight)
    assert got.dtype == np.float64 and got.shape == (out_c.shape[0], cout)
    origin = -4 * ts                                            # a multiple of 2 ts
    wd = _dense_weight(weight, k)
    lo_in = lo_out = 0
    worst = 0.0
    for b, (e_in, e_out) in enumerate(zip(ends, out_ends)):
        dense = F.conv3d(_densify(coords[lo_in:e_in, 1:].astype(np.int64), feats[lo_in:e_in], origin, ts, 8), wd, padding=k // 2, stride=s)
        oc = (out_c[lo_out:e_out, 1:].astype(np.int64) - origin) // (ts * s)
        assert (out_c[lo_out:e_out, 0] == b).all()
        ref = dense[0][:, oc[:, 0], oc[:, 1], oc[:, 2]].numpy().T
        worst = max(worst, float(np.abs(got[lo_out:e_out] - ref).max()))
        lo_in, lo_out = e_in, e_out
    assert worst <= 1e-12 * float(np.abs(got).max()), worst


def test_restatement_equals_dense_max_pool():
    ts = 4
    coords, ends = su.random_rows(3, ts)
    feats = np.random.default_rng(1).standard_normal((coords.shape[0], 8))
    out_c, out_ends, nbr = sparse.kernel_map_host(coords, ends, ts, 2, 2)
    got = sparse.sparse_max_pool3d_host(feats, nbr)
    assert (nbr >= 0).any(axis=1).all()                         # k = 2, s = 2: every output row has a neighbour
    origin = -4 * ts
    lo_in = lo_out = 0
    for e_in, e_out in zip(ends, out_ends):
        dense = F.max_pool3d(_densify(coords[lo_in:e_in, 1:].astype(np.int64), feats[lo_in:e_in], origin, ts, 8, fill=-np.inf), 2, 2)
        oc = (out_c[lo_out:e_out, 1:].astype(np.int64) - origin) // (2 * ts)
        assert np.array_equal(got[lo_out:e_out], dense[0][:, oc[:, 0], oc[:, 1], oc[:, 2]].numpy().T)
        lo_in, lo_out = e_in, e_out


@pytest.mark.parametrize("ts", [1, 4])
def test_stride2_rows_are_the_coarsening_rule(ts):
    """floor (not truncation: negative coordinates), first occurrence, row for row."""
    coords, ends = su.random_rows(7, ts, counts=(200, 1, 90), lo=-5, hi=3)
    out_c, out_ends, nbr = sparse.kernel_map_host(coords, ends, ts, 3, 2)
    want, want_ends, lo = [], [], 0
    for b, e in enumerate(ends):
        seen = set()
        for row in coords[lo:e, 1:].tolist():
            q = tuple((v // (2 * ts)) * (2 * ts) for v in row)          # python's // floors
            if q not in seen:
                seen.add(q)
                want.append((b,) + q)
        want_ends.append(len(want))
        lo = e
    assert out_c.tolist() == [list(w) for w in want] and out_ends == want_ends
    assert (coords[:, 1:] < 0).any() and (np.array(want)[:, 1:] < 0).any()
    # the centre offset of a 3x3x3 stride-2 map is the input row AT the output coordinate, when there is one
    index = {tuple(r): i for i, r in enumerate(coords.tolist())}
    assert [index.get(tuple(r), -1) for r in out_c.tolist()] == nbr[:, 13].tolist()


def test_kernel_offsets_order():
    o = sparse.kernel_offsets(3, 4)
    assert o.shape == (27, 3) and o[0].tolist() == [-4, -4, -4] and o[1].tolist() == [0, -4, -4] and o[3].tolist() == [-4, 0, -4]
    assert o[9].tolist() == [-4, -4, 0] and o[13].tolist() == [0, 0, 0] and o[26].tolist() == [4, 4, 4]
    assert sparse.kernel_offsets(2, 2).tolist() == [[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0], [0, 0, 2], [2, 0, 2], [0, 2, 2], [2, 2, 2]]
    assert sparse.kernel_offsets(1, 8).tolist() == [[0, 0, 0]]


def test_header_and_binding_declare_the_entry_points():
    su.assert_declared(NEW_ENTRY_POINTS)
    src = open(os.path.join(ROOT, "include", "proxyt.h")).read()
    section = src[src.index("sparse 3D convolution on the voxel rows"):src.index("image feature -> point sampling")]
    for ref in ("DET:398", "mink_resnet.py:58-63", "mink_resnet.py:67-69", "mink_resnet.py:103-109"):
        assert ref in section, ref
    assert len(_abi.SIGNATURES["ptx_sparse_kernel_map"][1]) == 13 and len(_abi.SIGNATURES["ptx_sparse_conv3d"][1]) == 15
    assert len(_abi.SIGNATURES["ptx_sparse_max_pool3d"][1]) == 7
    lib = _abi.lib()
    assert lib.ptx_sparse_kernel_map_workspace_bytes(4, 4096) >= 2 * lib.ptx_voxel_workspace_bytes(4, 4096)
    assert lib.ptx_sparse_kernel_map_workspace_bytes(65, 16) == 0


def test_module_parameters_carry_minkowski_names_and_shapes():
    m = sparse.SparseConv3d(3, 64, kernel_size=3, stride=2)
    sd = m.state_dict()
    assert list(sd) == ["kernel"] and tuple(sd["kernel"].shape) == (27, 3, 64)
    m = sparse.SparseConv3d(64, 128, kernel_size=1, stride=2, bias=True)
    sd = m.state_dict()
    assert sorted(sd) == ["bias", "kernel"] and tuple(sd["kernel"].shape) == (1, 64, 128) and tuple(sd["bias"].shape) == (1, 128)
    m.load_state_dict({"kernel": torch.ones(1, 64, 128), "bias": torch.zeros(1, 128)})       # a checkpoint loads by name
    km = sparse.KernelMap(coords=torch.zeros(0, 4, dtype=torch.int32), scene_rows=[0], nbr=torch.zeros(0, 1, dtype=torch.int32),
                          kernel_size=1, stride=2, tensor_stride=8)
    assert [f for f in km.__dataclass_fields__][:6] == ["coords", "scene_rows", "nbr", "kernel_size", "stride", "tensor_stride"]


def test_layers_refuse_cpu_tensors_and_grad():
    km = sparse.KernelMap(coords=torch.zeros(2, 4, dtype=torch.int32), scene_rows=[2], nbr=torch.zeros(2, 1, dtype=torch.int32),
                          kernel_size=1, stride=1, tensor_stride=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.sparse_conv3d(torch.zeros(2, 16), km, torch.zeros(1, 16, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.sparse_max_pool3d(torch.zeros(2, 16), km)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse.kernel_map(torch.zeros(2, 4, dtype=torch.int32), [2], 1, 3, 1)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_conv3d(torch.zeros(2, 16, requires_grad=True), km, torch.zeros(1, 16, 64))
