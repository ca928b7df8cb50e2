"""What the sparse test modules (and tools/sparse_conv_bwd_time.py --model) share: the voxel rows, the kernel maps over them, the operands
of a layer, the accuracy rule, the torch composition of a layer, and the check that an entry point is declared everywhere.  A plain
module: no tests, no marks."""
import functools
import os
import re

import numpy as np
import torch

from proxytransformation_amd import _abi, sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------------ rows
def random_rows(seed, ts, counts=(230, 120), lo=-4, hi=4):
    """Distinct voxel rows of ``len(counts)`` scenes, coordinates in [lo, hi) * ts (negative and positive), in random order."""
    rng = np.random.default_rng(seed)
    cells = np.stack(np.meshgrid(*[np.arange(lo, hi)] * 3, indexing="ij"), -1).reshape(-1, 3)
    rows, ends = [], []
    for b, n in enumerate(counts):
        pick = cells[rng.permutation(len(cells))[:n]] * ts
        rows.append(np.concatenate([np.full((n, 1), b), pick], 1))
        ends.append((ends[-1] if ends else 0) + n)
    return np.concatenate(rows).astype(np.int32), ends


@functools.lru_cache(maxsize=None)
def rows(ts, only_random=0):
    """The rows of the GPU tests: a dense 6x6x6 block (all 27 neighbours present), ~2100 random rows in [-40,40)^3 * ts (most neighbours
    missing; the row count is no multiple of the 64-row tile), an empty scene, and a last scene with one row.  ``only_random``: the
    random scene alone, cut to that many rows."""
    rng = np.random.default_rng(2024)
    block = np.stack(np.meshgrid(*[np.arange(-3, 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    block = block[rng.permutation(len(block))]
    rnd = rng.integers(-40, 40, size=(2140, 3))
    _, first = np.unique(rnd, axis=0, return_index=True)
    rnd = rnd[np.sort(first)]
    if only_random:
        rnd = rnd[:only_random]
        return np.concatenate([np.zeros((len(rnd), 1), np.int64), rnd * ts], 1).astype(np.int32), (len(rnd),)
    one = np.array([[5, -7, 2]])
    scenes = [block, rnd, rnd[:0], one]
    out = np.concatenate([np.concatenate([np.full((len(c), 1), b), c * ts], 1) for b, c in enumerate(scenes)]).astype(np.int32)
    ends = tuple(np.cumsum([len(c) for c in scenes]).tolist())
    assert out.shape[0] % 64 != 0 and out.shape[0] > 2200
    return out, ends


@functools.lru_cache(maxsize=None)
def host_map(ts, k, s, only_random=0):
    r, ends = rows(ts, only_random)
    return sparse.kernel_map_host(r, list(ends), ts, k, s)


def device_map(ts, k, s, only_random=0):
    r, ends = rows(ts, only_random)
    return sparse.kernel_map(torch.from_numpy(r).to(DEV), list(ends), ts, k, s)


def operands(n_in, n_out, cin, cout, kvol, seed):
    rng = np.random.default_rng(seed)
    return dict(feats=rng.standard_normal((n_in, cin)).astype(np.float32),
                weight=(rng.standard_normal((kvol, cin, cout)) / np.sqrt(kvol * cin)).astype(np.float32),
                bias=rng.standard_normal(cout).astype(np.float32) * 0.5,
                scale=rng.uniform(0.5, 1.5, cout).astype(np.float32), shift=rng.standard_normal(cout).astype(np.float32) * 0.5,
                residual=rng.standard_normal((n_out, cout)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ the accuracy rule
def rel(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())


def hold(name, got, ref32, ref64):
    """max |got - ref64| / max |ref64| against 8 x the same statistic of the fp32 CPU chain, both printed."""
    e_gpu, e_cpu = rel(got, ref64), rel(ref32, ref64)
    print(f"sparse_conv {name}: gpu {e_gpu:.3e}  fp32-cpu {e_cpu:.3e}  ratio {e_gpu / max(e_cpu, 1e-30):.2f}")
    assert e_cpu < 1e-5, (name, e_cpu)                       # the yardstick itself is an fp32 rounding error, not a wrong answer
    assert e_gpu <= 8.0 * e_cpu, (name, e_gpu, e_cpu)


# ------------------------------------------------------------------------------------------------------------------ torch twin
def composition(feats, nbr, weight, bias=None, scale=None, shift=None, residual=None, relu=False):
    """The layer as a user could write it from ``nbr`` in plain torch: out = sum_j index_select(feats, nbr_j) @ W_j (missing rows
    masked), + bias, * scale + shift, + residual, ReLU.  Differentiable by autograd."""
    nbr = torch.as_tensor(nbr).long()
    out = feats.new_zeros((nbr.shape[0], weight.shape[2]))
    for j in range(nbr.shape[1]):
        present = (nbr[:, j] >= 0).to(feats.dtype).unsqueeze(1)
        out = out + (feats.index_select(0, nbr[:, j].clamp(min=0)) * present) @ weight[j]
    if bias is not None:
        out = out + bias.reshape(1, -1)
    if scale is not None:
        out = out * scale.reshape(1, -1)
    if shift is not None:
        out = out + shift.reshape(1, -1)
    if residual is not None:
        out = out + residual
    return torch.relu(out) if relu else out


# ------------------------------------------------------------------------------------------------------------------ ABI surface
def assert_declared(names):
    """Every name is declared ``PTX_API`` in include/proxyt.h, bound in ``_abi.SIGNATURES``, exported by csrc/exports.map and found in the
    loaded library.  Returns ``{name: its parameter list as the header spells it}``."""
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "proxyt.h")).read(), flags=re.S)
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "exports.map")).read())
    assert patterns
    lib = _abi.lib()
    params = {}
    for name in names:
        m = re.search(r"PTX_API\s+\w+\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        assert name in _abi.SIGNATURES, name
        assert any(re.fullmatch(p.strip().replace("*", ".*"), name) for p in patterns), name
        getattr(lib, name)
        params[name] = m.group(1)
    return params
