"""Host side of the differentiable voxel quantisation (no GPU): the ABI surface of the two entry points that were added for it
(``ptx_voxelize_rep``, ``ptx_voxel_features_bwd``) and the backward RULE itself, restated in numpy and held against torch's CPU
autograd of what the reference computes -- ``features = p[unique_index]`` (detectors/sparse_featfusion_grounder_preshape.py:388-397,
``use_xyz_feat``), with the surviving point pinned to the first of every voxel in (scene, point) order.

The GPU tests (tests/test_gpu_voxel_grad.py, tests/test_gpu_pipeline_train.py) import ``first_index`` / ``features_bwd_rule``
from here."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import torch

from tests.util import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptx_voxelize_rep", "ptx_voxel_features_bwd")


# ------------------------------------------------------------------ the rule
def first_index(inverse, nvox):
    """``rep``: per voxel row the smallest index (in the concatenation of the scenes) of a point that maps to it."""
    inv = np.concatenate([np.asarray(i, np.int64).reshape(-1) for i in inverse]) if isinstance(inverse, (list, tuple)) \
        else np.asarray(inverse, np.int64)
    rep = np.full(nvox, len(inv), np.int64)
    np.minimum.at(rep, inv, np.arange(len(inv)))
    return rep


def features_bwd_rule(dfeats, inverse):
    """The backward of ``features = cat(outs)[rep]``: point j receives ``dfeats[inverse[j]]`` if it is the point its row kept
    (``rep[inverse[j]] == j``) and exact zeros otherwise.  ``inverse``: list of per-scene maps; returns one (n_b,3) array per scene."""
    dfeats = np.asarray(dfeats, np.float32)
    sizes = np.cumsum([0] + [len(i) for i in inverse])
    inv = np.concatenate([np.asarray(i, np.int64).reshape(-1) for i in inverse])
    rep = first_index(inv, len(dfeats))
    d = np.zeros((len(inv), 3), np.float32)
    mine = np.nonzero(rep[inv] == np.arange(len(inv)))[0] if len(inv) else np.zeros((0,), np.int64)
    d[mine] = dfeats[inv[mine]]
    return [d[sizes[b]:sizes[b + 1]] for b in range(len(inverse))]


def _scenes(seed):
    rng = np.random.default_rng(seed)
    # three scenes of different sizes in a few metres, some exact duplicates and some negative coordinates
    outs = [(rng.random((n, 3)) * np.array([7.0, 5.0, 3.0]) - 1.0).astype(np.float32) for n in (3000, 1700, 2300)]
    outs[1][100:110] = outs[1][5]
    return outs


def test_the_rule_equals_torch_autograd_of_the_gather():
    from oracle import oracle
    for vs in (0.25, 0.01):
        outs = _scenes(int(vs * 1000))
        coords, feats, inverse = oracle.voxelize(outs, vs)
        total, nvox = sum(len(o) for o in outs), len(coords)
        assert nvox < total                                           # duplicates occur at both sizes (ten planted ones at 1 cm)
        rep = first_index(inverse, nvox)
        assert np.array_equal(np.concatenate(outs)[rep], feats)        # the oracle's rows ARE cat(outs)[first index]
        assert np.all(np.diff(rep) > 0)                                # ... in (scene, point) order
        leaves = [torch.from_numpy(o).requires_grad_(True) for o in outs]
        f = torch.cat(leaves)[torch.from_numpy(rep)]
        dfeats = np.random.default_rng(7).standard_normal((nvox, 3)).astype(np.float32)
        f.backward(torch.from_numpy(dfeats))
        got = features_bwd_rule(dfeats, inverse)
        for g, leaf in zip(got, leaves):
            assert g.dtype == np.float32 and np.array_equal(g, leaf.grad.numpy())
        # every row's gradient arrives exactly once; everything else is an exact zero
        assert sum(int((g != 0).any(axis=1).sum()) for g in got) == nvox


def test_the_rule_on_empty_inputs():
    got = features_bwd_rule(np.zeros((0, 3), np.float32), [np.zeros((0,), np.int32)] * 2)
    assert [g.shape for g in got] == [(0, 3), (0, 3)]
    inv = [np.array([0, 0, 1], np.int32), np.zeros((0,), np.int32), np.array([2, 1], np.int32)]
    d = np.arange(9, dtype=np.float32).reshape(3, 3) + 1
    got = features_bwd_rule(d, inv)
    assert np.array_equal(got[0], np.stack([d[0], 0 * d[0], d[1]])) and got[1].shape == (0, 3)
    assert np.array_equal(got[2], np.stack([d[2], 0 * d[1]]))


# ------------------------------------------------------------------ the ABI surface
def test_header_declares_the_two_entry_points_and_the_binding_matches():
    from proxytransformation_amd import _abi
    protos = {name: ", ".join(params) for name, (_, params) in header_prototypes().items()}
    assert len(protos) >= 90 and "ptx_voxelize_ex" in protos
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/proxyt.h"
        assert name in _abi.SIGNATURES, f"{name} is not bound in _abi.SIGNATURES"
        nargs = len([a for a in protos[name].split(",") if a.strip()])
        assert nargs == len(_abi.SIGNATURES[name][1]), (name, nargs, len(_abi.SIGNATURES[name][1]))
    # ptx_voxelize_rep = ptx_voxelize_ex + one pointer (rep) behind `inverse`; no existing signature changed
    ex, rep = _abi.SIGNATURES["ptx_voxelize_ex"][1], _abi.SIGNATURES["ptx_voxelize_rep"][1]
    assert rep[:8] + rep[9:] == ex and rep[8] is _abi._P
    assert len(_abi.SIGNATURES["ptx_voxelize_ex"][1]) == 13 and len(_abi.SIGNATURES["ptx_voxelize"][1]) == 12
    assert "int32_t *rep" in protos["ptx_voxelize_rep"] and "dpoints" in protos["ptx_voxel_features_bwd"]
    assert _abi.ABI_VERSION == 13                                       # grown by addition
    # each entry's header comment cites the detector lines it restates
    raw = open(os.path.join(ROOT, "include", "proxyt.h")).read()
    for name in NEW:
        comment = raw[:raw.index("PTX_API int " + name)].rsplit("/*", 1)[1]
        assert "DET:388-397" in comment, name


def test_the_library_exports_the_two_entry_points():
    from proxytransformation_amd import _abi
    vs = open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "exports.map")).read()
    vs = re.sub(r"/\*.*?\*/", "", vs, flags=re.S)
    globs = [g.strip() for g in re.search(r"global:(.*?);", vs, flags=re.S).group(1).split()]
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), f"exports.map does not list {name}"
    lib = _abi.lib()                                                   # resolves every bound symbol
    here = os.path.join(ROOT, "proxytransformation_amd")
    for so in ("libproxyt_hip.so", "libproxyt_hip_testhooks.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(here, so)], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(NEW) <= exported, (so, sorted(set(NEW) - exported))
    # the argument checks are made on the host before anything is enqueued (no device is touched by these calls)
    assert lib.ptx_voxel_features_bwd(None, 0, None, None, None, 1, 4, None, None) != 0
    assert b"ptx_voxel_features_bwd" in lib.ptx_last_error()
    assert lib.ptx_voxelize_rep(None, None, 1, 4, 0.01, None, None, None, None, None, None, None, 0, None) != 0
