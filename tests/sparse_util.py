"""What the sparse test modules (and tools/sparse_conv_bwd_time.py --model) share: the voxel rows, the kernel maps over them, the operands
of a layer, the accuracy rule, the calls and references of the convolution and the norms, the library's private plans restated (the
split of dweight over the rows, the norms' tile bound) with the shapes that reach the branches past one tile run / one compaction
round, the torch composition of a layer, and the check that an entry point is declared everywhere.  A plain module: no tests, no
marks."""
import functools
import os
import re

import numpy as np
import torch

from proxytransformation_amd import _abi, sparse
from tests.util import header_prototypes

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


def dense_map(name):
    """The rows, scene ends and host kernel map (k3 s1) of one ``DW_REGIMES`` entry: ``random_rows`` on a grid small enough that about
    half of all neighbours exist, so every offset has pairs in every compaction round of every row chunk."""
    return _dense_map(name)


@functools.lru_cache(maxsize=None)
def _dense_map(name):
    c = DW_REGIMES[name]
    r, ends = random_rows(c["seed"], c["ts"], c["counts"], c["lo"], c["hi"])
    nbr = sparse.kernel_map_host(r, ends, c["ts"], 3, 1)[2]
    assert 0.3 < float((nbr >= 0).mean()) < 0.7, name
    return r, ends, nbr


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


MIN_SAMPLE = 64


def hold_pooled(name, size, draw, call, refs, rule=hold):
    """``hold`` compares two maxima, and a maximum over a handful of values is no yardstick: the fp32 host's only value can be exact by
    luck while the device's is one ulp off (seen at K = T = 1: 9.5e-9 against 1.2e-7, one value).  So a call with fewer than 64 results
    (``size``) is repeated on fresh draws of the SAME shape until 64 are pooled, and the rule is applied to the pool.  Returns the first
    draw and its device result."""
    parts = []
    for _ in range(max(1, -(-MIN_SAMPLE // max(size, 1)))):
        ops = draw()
        parts.append((ops, call(*ops)) + tuple(refs(*ops)))
    rule(name, *(np.concatenate([p[i].ravel() for p in parts]) for i in (1, 2, 3)))
    return parts[0][0], parts[0][1]


# ------------------------------------------------------------------------------------------------------------------ convolution
# (Cin, Cout, kernel_size, stride) of the layer tests, forward and backward
LAYER_SHAPES = [(3, 64, 3, 2), (64, 64, 3, 1), (64, 128, 3, 2), (128, 256, 1, 2), (512, 512, 3, 1)]


def layer_rows(cin):
    """(tensor stride, cut of the random scene) the layer tests run a shape of ``LAYER_SHAPES`` on."""
    return (1 if cin == 3 else 4), (600 if cin == 512 else 0)


def dev(a, grad=False):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x.requires_grad_() if grad else x


def conv_run(km, ops, use=(), relu=False):
    with torch.no_grad():
        return sparse.sparse_conv3d(dev(ops["feats"]), km, dev(ops["weight"]), relu=relu, **{u: dev(ops[u]) for u in use})


def conv_refs(nbr, ops, use=(), relu=False):
    r64 = sparse.sparse_conv3d_host(ops["feats"].astype(np.float64), nbr, ops["weight"].astype(np.float64), relu=relu,
                                    **{u: ops[u].astype(np.float64) for u in use})
    r32 = sparse.sparse_conv3d_host(ops["feats"], nbr, ops["weight"], relu=relu, **{u: ops[u] for u in use})
    assert r32.dtype == np.float32
    return r32, r64


def grad_case(km, nbr, ops, full, relu, seed, wrt=("feats", "weight", "bias", "residual")):
    """One differentiable call + backward of loss = (out * G).sum(); returns (out, G, {name: grad})."""
    names = ("feats", "weight") + (("bias", "residual") if full else ())
    leaves = {n: dev(ops[n], grad=n in wrt) for n in names}
    kw = dict(bias=leaves["bias"], scale=dev(ops["scale"]), shift=dev(ops["shift"]), residual=leaves["residual"]) if full else {}
    out = sparse.sparse_conv3d(leaves["feats"], km, leaves["weight"], relu=relu, differentiable=True, **kw)
    G = np.random.default_rng(seed).standard_normal(tuple(out.shape)).astype(np.float32)
    (out * dev(G)).sum().backward()
    return out.detach(), G, {n: v.grad for n, v in leaves.items()}


def grad_refs(nbr, ops, out, G, full, relu):
    kw32 = dict(out=out, scale=ops["scale"] if full else None, relu=relu, has_bias=full, has_residual=full)
    r32 = sparse.sparse_conv3d_bwd_host(G, ops["feats"], nbr, ops["weight"], **kw32)
    kw64 = dict(kw32, scale=ops["scale"].astype(np.float64) if full else None)
    r64 = sparse.sparse_conv3d_bwd_host(G.astype(np.float64), ops["feats"].astype(np.float64), nbr, ops["weight"].astype(np.float64), **kw64)
    assert r32["dfeats"].dtype == np.float32 and r64["dweight"].dtype == np.float64
    return r32, r64


def _align(nbytes, to=256):
    return -(-nbytes // to) * to


def dw_plan(n_out, kvol, cin, cout):
    """``dw_plan`` of csrc/sparse_bwd.hip restated: ``(R, S, workspace bytes)``.  dweight is split over S chunks of R output rows: enough
    work-groups (S x kvol x Cin/64 x Cout/64; the stem: S x kvol x Cout/64) to cover the chip about four times (1024), slabs of at most
    256 MiB in all, R a multiple of 64 and at least 256 (the stem: 1024); S > 1 needs S slabs of kvol x Cin x Cout floats, and dbias the
    column sums of every 256-row tile."""
    stem = cin == 3
    groups = kvol * (cout // 64) * (1 if stem else cin // 64)
    slab = kvol * cin * cout
    target = max(1, min(-(-1024 // groups), (256 << 20) // (slab * 4)))
    R = max(-(-(-(-n_out // target)) // 64) * 64, 1024 if stem else 256)
    S = -(-n_out // R)
    slabs = _align(S * slab * 4) if S > 1 else 0
    tiles = _align(-(-max(n_out, 1) // 256) * cout * 4)
    return R, S, slabs + tiles + 256


# the smallest shapes (k3 s1) whose row chunk exceeds the 1024 rows k_sparse_dweight compacts per round -- 512 -> 512: one chunk, a full
# round of 4 passes and a round of 276 rows; 256 -> 512: two chunks of two rounds, added by k_sparse_slab_sum -- and the stem past
# R = 1024: wave quarters of 272 rows, off the 64 grid, each ending in a partial block.  R, S: what dw_plan must give for them
DW_REGIMES = {
    "512->512": dict(cin=512, cout=512, ts=4, counts=(1100, 200), lo=-6, hi=6, seed=41, R=1344, S=1),
    "256->512": dict(cin=256, cout=512, ts=4, counts=(1500, 700), lo=-7, hi=7, seed=42, R=1152, S=2),
    "stem": dict(cin=3, cout=512, ts=1, counts=(3000, 2300), lo=-9, hi=9, seed=43, R=1088, S=5),
}


# ------------------------------------------------------------------------------------------------------------------ norms
NORM_TILE = 256                    # rows per tile of csrc/sparse_norm.hip; a segment's tiles go to 16 slots in runs of ceil(tiles / 16)
# segment SIZES.  4097 rows: 17 tiles, runs of 2, slot 8 holds the one-row tile alone, slots 9 to 15 none; 8500 rows: 34 tiles, runs of
# 3, 12 slots, a last tile of 52 rows; then the same followed by 60 more (64 segments, the limit); one segment of 96 tiles, runs of 6
NORM_REGIMES = {
    "four": [4097, 0, 8500, 1],
    "sixty-four": [4097, 0, 8500, 1] + [[0, 1, 255, 256, 257, 64, 511, 512, 513][i % 9] for i in range(60)],
    "one": [24548],
}


def seg_ends(sizes):
    return np.cumsum(sizes).tolist()


def seg_tiles(sizes):
    return [-(-s // NORM_TILE) for s in sizes]


def norm_plan(n, S, C):
    """``sn_plan`` of csrc/sparse_norm.hip restated: ``(tile bound, workspace bytes)`` -- at most ``n // 256 + S`` tiles of two floats
    per column, and twice the S segments' two floats per column (their means, their sums)."""
    bound = n // NORM_TILE + S
    return bound, _align(bound * 2 * C * 4) + 2 * _align(S * 2 * C * 4) + 256


def norm_operands(n, C, offset, seed):
    """x = N(0, 1) (+ ``offset`` * (+-1 per column)), weight, bias, residual and the gradient g of a norm over (n, C) rows."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, C)).astype(np.float32)
    if offset:
        x += (offset * np.where(rng.random(C) < 0.5, -1.0, 1.0)).astype(np.float32)
    return dict(x=x, weight=rng.uniform(0.5, 1.5, C).astype(np.float32), bias=(rng.standard_normal(C) * 0.5).astype(np.float32),
                residual=rng.standard_normal((n, C)).astype(np.float32), g=rng.standard_normal((n, C)).astype(np.float32))


def norm_refs(ops, ends, eps, use=(), relu=False):
    r64 = sparse.sparse_norm_host(ops["x"].astype(np.float64), ends, eps, relu=relu, **{u: ops[u].astype(np.float64) for u in use})
    r32 = sparse.sparse_norm_host(ops["x"], ends, eps, relu=relu, **{u: ops[u] for u in use})
    assert r32.dtype == np.float32
    return r32, r64


def hold_norm_stats(stats, ops, ends, eps, segments, size):
    """The statistics themselves against float64, to a few fp32 ulps of their size: the mean to 4e-6 of ``size`` (the magnitude of the
    data), rstd to 4e-6 of itself."""
    _, s64 = sparse.sparse_norm_host(ops["x"].astype(np.float64), ends, eps, return_stats=True)
    for s in segments:
        assert float(np.abs(stats[s, 0] - s64[s, 0]).max()) <= 4e-6 * size, s
        assert float(np.abs(stats[s, 1] / s64[s, 1] - 1).max()) <= 4e-6, s


def norm_grad_refs(ops, ends, eps, out, relu, weight=True):
    kw = dict(out=out, relu=relu)
    r64 = sparse.sparse_norm_bwd_host(ops["g"].astype(np.float64), ops["x"].astype(np.float64), ends, eps,
                                      ops["weight"].astype(np.float64) if weight else None, **kw)
    r32 = sparse.sparse_norm_bwd_host(ops["g"], ops["x"], ends, eps, ops["weight"] if weight else None, **kw)
    return r32, r64


def hold_norm_grads(name, got, ops, ends, eps, out, relu, weight=True):
    """``got``: dict of numpy gradients; the ReLU mask of both references is the GPU's ``out``."""
    r32, r64 = norm_grad_refs(ops, ends, eps, out, relu, weight)
    for k, v in got.items():
        assert v.shape == r64[k].shape and v.dtype == np.float32, k
        hold(f"{name} {k}", v, r32[k], r64[k])


def bn_pair(C, seed):
    """An ``nn.BatchNorm1d`` in training mode three times over, same state: float64 and float32 on the CPU, float32 on the device."""
    rng = np.random.default_rng(seed)
    bn64 = torch.nn.BatchNorm1d(C, eps=1e-5, momentum=0.1).double()
    with torch.no_grad():
        bn64.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))
        bn64.bias.copy_(torch.from_numpy((rng.standard_normal(C) * 0.5).astype(np.float32)))
        bn64.running_mean.copy_(torch.from_numpy((rng.standard_normal(C) * 0.1).astype(np.float32)))
        bn64.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))
    bn32 = torch.nn.BatchNorm1d(C, eps=1e-5, momentum=0.1)
    bn32.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in bn64.state_dict().items()})
    gpu = torch.nn.BatchNorm1d(C, eps=1e-5, momentum=0.1)
    gpu.load_state_dict(bn32.state_dict())
    return bn64.train(), bn32.train(), gpu.to(DEV).train()


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
    protos = header_prototypes()
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "exports.map")).read())
    assert patterns
    lib = _abi.lib()
    params = {}
    for name in names:
        assert name in protos, name
        assert name in _abi.SIGNATURES, name
        assert any(re.fullmatch(p.strip().replace("*", ".*"), name) for p in patterns), name
        getattr(lib, name)
        params[name] = ", ".join(protos[name][1])
    return params
