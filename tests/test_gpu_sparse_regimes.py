"""The sparse layers at the tile, chunk and key counts the other sparse modules never reach -- the branches a workload of 400 000 rows
lives in, each at the smallest shape that takes it (``tests/sparse_util.py``: ``NORM_REGIMES``, ``DW_REGIMES``).  References: the numpy
restatements of ``sparse_host.py`` in float64; the rule: ``sparse_util.hold`` (at most 8 x the error of the same restatement in fp32,
which itself stays below 1e-5).

A  segment norms past 16 tiles per segment: a slot's run of tiles folds more than one (k_sparse_norm_finalise's Chan merge with
   ``cn > 0``, k_sparse_norm_bwd_finalise's run), slots in the middle of the 16 hold no tile, the last tile is partial; 64 segments;
   a training batch norm over 96 tiles; columns at +-4.
B  dweight past one compaction round of 1024 rows (``tot`` carried across rounds), with and without slabs; the stem's wave quarters
   off the 64-row grid.
C  the widths the forward accepts between the tested ones -- a short single chunk, a second chunk of one or of both half-steps -- and
   the 8-offset convolution, forward and backward.
D  kernel maps with rows at the first and last voxel of the key range, where only the per-axis range test keeps a neighbour one step
   outside from carrying into the next key field (the next y, the next x, the next scene), and with 64 scenes.

What the restated plans promise for these shapes (R, S; the tile bound) is held without a GPU in tests/test_sparse_conv_grad_host.py and
tests/test_sparse_backbone_host.py; the tile counts are asserted here."""
import functools

import numpy as np
import pytest
import torch

from proxytransformation_amd import sparse
from tests import sparse_util as su
from tests.sparse_util import dev

pytestmark = pytest.mark.gpu

EPS = sparse.INSTANCE_NORM_EPS
CPU_THREADS = 8     # of the torch references of the batch norm: the order of their fp32 sums, and so the yardstick, depends on the count


# ------------------------------------------------------------------------------------------------------------------ A: norms
@functools.lru_cache(maxsize=None)
def _norm_case(layout, C, offset):
    sizes = su.NORM_REGIMES[layout]
    ends = su.seg_ends(sizes)
    # the seed base: one at which the fp32 restatement itself stays a factor 2 inside the 1e-5 cap of ``hold`` in every case (dweight with
    # the columns at +-4 ranges from 4e-6 to 1.2e-5 over seeds)
    return sizes, ends, su.norm_operands(ends[-1], C, offset, 7007 + len(sizes) + C + offset)


def _norm_forward(layout, C, offset):
    """Forward with weight, bias, residual and ReLU: the output, two calls, the statistics of the long segments, the edge segments."""
    sizes, ends, ops = _norm_case(layout, C, offset)
    use = ("weight", "bias", "residual")
    call = lambda relu: sparse.sparse_segment_norm(dev(ops["x"]), ends, EPS, dev(ops["weight"]), dev(ops["bias"]), dev(ops["residual"]),  # noqa: E731
                                                   relu, return_stats=True)
    got, stats = call(True)
    again, stats2 = call(True)
    assert torch.equal(got, again) and torch.equal(stats, stats2), "two calls on the same inputs differ"
    tag = f"regime norm {layout} C={C} offset={offset}"
    su.hold(f"{tag} out", got.cpu().numpy(), *su.norm_refs(ops, ends, EPS, use, True))
    assert float(got.min()) == 0.0
    stats = stats.cpu().numpy()
    assert stats.shape == (len(sizes), 2, C)
    su.hold_norm_stats(stats, ops, ends, EPS, (0, 2), max(offset, 1))
    plain = call(False)[0].cpu().numpy()
    for s, n in enumerate(sizes):
        if n == 0:                                           # an empty segment's stats are zero
            assert np.array_equal(stats[s], np.zeros((2, C), np.float32)), s
        if n == 1:                                           # a one-row segment: its mean is the row, its output bias + residual exactly
            row = ends[s] - 1
            assert np.array_equal(stats[s, 0], ops["x"][row]), s
            assert np.array_equal(plain[row], ops["bias"] + ops["residual"][row]), s
    return sizes


def _norm_backward(layout, C, offset):
    """dx, dweight, dbias, dresidual; dresidual bit-equal to where(out > 0, g, 0); two backwards give equal bits."""
    sizes, ends, ops = _norm_case(layout, C, offset)
    every = ("x", "weight", "bias", "residual")

    def step():
        leaves = {k: dev(ops[k], grad=True) for k in every}
        out = sparse.sparse_segment_norm(leaves["x"], ends, EPS, leaves["weight"], leaves["bias"], leaves["residual"], True, differentiable=True)
        out.backward(dev(ops["g"]))
        return out.detach(), {k: v.grad for k, v in leaves.items()}

    out, grads = step()
    out2, grads2 = step()
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in every), "two backwards on the same inputs differ"
    out_np = out.cpu().numpy()
    assert 0.2 < float((out_np == 0).mean()) < 0.8
    assert np.array_equal(grads["residual"].cpu().numpy(), np.where(out_np > 0, ops["g"], np.float32(0)))
    got = dict(dx=grads["x"].cpu().numpy(), dweight=grads["weight"].cpu().numpy(), dbias=grads["bias"].cpu().numpy(),
               dresidual=grads["residual"].cpu().numpy())
    su.hold_norm_grads(f"regime norm {layout} C={C} offset={offset} bwd", got, ops, ends, EPS, out_np, True)


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("C", [64, 128])
def test_norm_with_runs_of_two_and_three_tiles_per_slot(C, offset):
    """Segments of 4097, 0, 8500 and 1 rows; ``offset`` 4: the conditioning case, columns at +-4 with unit spread (C = 128: the second
    work-group column reads its own columns of the partials)."""
    sizes = _norm_forward("four", C, offset)
    assert su.seg_tiles(sizes) == [17, 0, 34, 1] and sum(sizes) == 12598 and sizes[2] % su.NORM_TILE == 52
    _norm_backward("four", C, offset)


@pytest.mark.parametrize("C", [64, 128])
def test_norm_with_sixty_four_segments(C):
    """The same four segments followed by 60 of 0 to 513 rows: the segment table full."""
    sizes = _norm_forward("sixty-four", C, 0)
    assert len(sizes) == 64 and sum(sizes) == 27645 and su.seg_tiles(sizes)[:4] == [17, 0, 34, 1]
    assert sizes.count(0) >= 7 and sizes.count(1) >= 7
    _norm_backward("sixty-four", C, 0)


@pytest.mark.parametrize("C", [64, 128])
def test_training_batch_norm_over_ninety_six_tiles(C):
    """One segment of 24 548 rows (runs of 6 tiles per slot) through ``sparse_batch_norm``, running statistics on, one step, with
    residual and ReLU: forward, running_mean, running_var and the four gradients against ``nn.BatchNorm1d`` in float64 on the CPU,
    yardstick the same module in float32; the ReLU mask of both references is the GPU's output's."""
    sizes, ends, ops = _norm_case("one", C, 0)
    assert su.seg_tiles(sizes) == [96]
    x_np = ops["x"] * np.float32(1.5) + np.float32(0.25)
    bn64, bn32, gpu = su.bn_pair(C, 11)
    x, res = dev(x_np, grad=True), dev(ops["residual"], grad=True)
    out = sparse.sparse_batch_norm(x, gpu, residual=res, relu=True, differentiable=True)
    out.backward(dev(ops["g"]))
    out_np = out.detach().cpu().numpy()
    assert int(gpu.num_batches_tracked) == 1 and 0.2 < float((out_np == 0).mean()) < 0.8
    assert np.array_equal(res.grad.cpu().numpy(), np.where(out_np > 0, ops["g"], np.float32(0)))
    got = dict(out=out_np, running_mean=gpu.running_mean.cpu().numpy(), running_var=gpu.running_var.cpu().numpy(),
               dx=x.grad.cpu().numpy(), dweight=gpu.weight.grad.cpu().numpy(), dbias=gpu.bias.grad.cpu().numpy(),
               dresidual=res.grad.cpu().numpy())
    refs = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)                       # an earlier test of the process may have left another count
    try:
        for dt, bn in ((torch.float64, bn64), (torch.float32, bn32)):
            xr, rr = (torch.from_numpy(a).to(dt).requires_grad_() for a in (x_np, ops["residual"]))
            y = bn(xr) + rr
            (y * torch.from_numpy((out_np > 0) * ops["g"]).to(dt)).sum().backward()
            refs[dt] = dict(out=torch.relu(y).detach().numpy(), running_mean=bn.running_mean.numpy(), running_var=bn.running_var.numpy(),
                            dx=xr.grad.numpy(), dweight=bn.weight.grad.numpy(), dbias=bn.bias.grad.numpy(), dresidual=rr.grad.numpy())
    finally:
        torch.set_num_threads(threads)
    for k, v in got.items():
        su.hold(f"regime batch norm 96 tiles C={C} {k}", v, refs[torch.float32][k], refs[torch.float64][k])


# ------------------------------------------------------------------------------------------------------------------ B: dweight
def _hold_grads(tag, nbr, ops, out, G, got, again, full):
    r32, r64 = su.grad_refs(nbr, ops, out.cpu().numpy(), G, full, relu=full)
    for name, key in (("feats", "dfeats"), ("weight", "dweight")) + ((("bias", "dbias"), ("residual", "dresidual")) if full else ()):
        g = got[name]
        assert g is not None and g.dtype == torch.float32 and tuple(g.shape) == tuple(ops[name].shape), name
        assert torch.equal(g, again[name]), f"{name}: two backward calls on the same inputs differ"
        su.hold(f"{tag} {key}", g.cpu().numpy().reshape(r64[key].shape), r32[key], r64[key])


@pytest.mark.parametrize("name", list(su.DW_REGIMES))
def test_dweight_past_one_compaction_round(name):
    """dfeats and dweight (and the forward) of the three shapes whose row chunk exceeds 1024 rows; 256 -> 512 also through the full
    epilogue, with dbias and dresidual.  About half of all neighbours exist: every offset has pairs in both rounds of every chunk."""
    c = su.DW_REGIMES[name]
    rows, ends, nbr = su.dense_map(name)
    n = rows.shape[0]
    R, S, _ = su.dw_plan(n, 27, c["cin"], c["cout"])
    assert (R, S) == (c["R"], c["S"]) and R > 1024 and n == sum(c["counts"])
    for j in range(27 if c["cin"] != 3 else 0):              # every offset has pairs in every round of every chunk
        for lo in range(0, n, R):
            for sub in range(lo, min(lo + R, n), 1024):
                assert (nbr[sub:min(sub + 1024, lo + R, n), j] >= 0).any(), (j, lo, sub)
    km = sparse.kernel_map(dev(rows), ends, c["ts"], 3, 1)
    assert np.array_equal(km.nbr.cpu().numpy(), nbr)
    ops = su.operands(n, n, c["cin"], c["cout"], 27, seed=c["seed"])
    for full in (False, True) if name == "256->512" else (False,):
        out, G, got = su.grad_case(km, nbr, ops, full, relu=full, seed=c["seed"] + full)
        out2, _, again = su.grad_case(km, nbr, ops, full, relu=full, seed=c["seed"] + full)
        assert torch.equal(out, out2)
        tag = f"regime {name} rows={n} R={R} S={S}" + (" epilogue" if full else "")
        use = ("bias", "scale", "shift", "residual") if full else ()
        su.hold(f"{tag} out", out.cpu().numpy(), *su.conv_refs(nbr, ops, use, relu=full))
        _hold_grads(tag, nbr, ops, out, G, got, again, full)
        if full:
            out_np = out.cpu().numpy()
            assert 0.2 < float((out_np == 0).mean()) < 0.8
            assert np.array_equal(got["residual"].cpu().numpy(), np.where(out_np > 0, G, np.float32(0)))


# ------------------------------------------------------------------------------------------------------------------ C: widths, 8 offsets
@pytest.mark.parametrize("cin,cout,k,s", [(16, 64, 3, 1), (48, 64, 3, 1), (80, 64, 3, 1), (96, 128, 3, 1), (112, 64, 3, 1), (80, 64, 1, 2),
                                          (48, 64, 1, 2)])
def test_forward_widths_between_the_layer_widths(cin, cout, k, s):
    """Cin 16, 48: one short chunk (48: its second half-step half full); 80, 96: a second chunk of one half-step; 112: of both."""
    _, _, nbr = su.host_map(4, k, s)
    km = su.device_map(4, k, s)
    n_in = su.rows(4)[0].shape[0]
    ops = su.operands(n_in, nbr.shape[0], cin, cout, k ** 3, seed=cin + cout + k)
    assert float(np.abs(ops["feats"]).min()) > 0 and float(np.abs(ops["weight"]).min()) > 0
    got = su.conv_run(km, ops)
    assert got.shape == (nbr.shape[0], cout) and torch.equal(got, su.conv_run(km, ops)), "two launches on the same inputs differ"
    su.hold(f"regime width Cin={cin} Cout={cout} k={k} s={s}", got.cpu().numpy(), *su.conv_refs(nbr, ops))


def test_eight_offset_convolution_forward_and_backward():
    """kernel_size 2, stride 2, 64 -> 128: the forward and, with ``differentiable=True``, dfeats and dweight."""
    _, _, nbr = su.host_map(4, 2, 2)
    km = su.device_map(4, 2, 2)
    assert nbr.shape[1] == 8 and np.array_equal(km.nbr.cpu().numpy(), nbr)
    n_in = su.rows(4)[0].shape[0]
    ops = su.operands(n_in, nbr.shape[0], 64, 128, 8, seed=208)
    tag = f"regime k=2 s=2 64->128 rows={n_in}->{nbr.shape[0]}"
    plain = su.conv_run(km, ops)
    su.hold(f"{tag} out", plain.cpu().numpy(), *su.conv_refs(nbr, ops))
    out, G, got = su.grad_case(km, nbr, ops, False, relu=False, seed=8)
    out2, _, again = su.grad_case(km, nbr, ops, False, relu=False, seed=8)
    assert torch.equal(out, plain) and torch.equal(out2, plain)
    _hold_grads(tag, nbr, ops, out, G, got, again, False)


# ------------------------------------------------------------------------------------------------------------------ D: key range
M, m = (1 << 18) - 1, -(1 << 18)     # the last and the first voxel of the key range, in tensor strides


@functools.lru_cache(maxsize=None)
def _edge_rows():
    """64 scenes, rows in 0, 1, 62 and 63 only, in voxel units.  Pairs one step apart across the end of a key field -- a neighbour at
    2^18 would carry into the next field and alias the other row of the pair: (0, 0, M) / (0, 1, m) the next y, (0, M, 5) / (1, m, 5)
    the next x, (M, 7, 7) in scene b / (m, 7, 7) in scene b + 1 the next scene -- with ordinary neighbours of each, and the corners."""
    pairs = [(0, 0, M), (0, 1, m), (0, M, 5), (1, m, 5)]
    near = [(0, 0, M - 1), (0, 1, m + 1), (0, M - 1, 5), (1, m + 1, 5), (0, 1, M), (0, 0, m), (1, M, 5), (0, m, 5)]
    top, bottom = [(M, 7, 7), (M - 1, 7, 7), (M, 8, 7), (M, M, M), (M - 1, M, M)], [(m, 7, 7), (m + 1, 7, 7), (m, 6, 7), (m, m, m), (m, m + 1, m)]
    scenes = {0: pairs + near + top + bottom[3:], 1: bottom + pairs[:2] + top[:1], 62: top + pairs + near[:4] + bottom[:1],
              63: bottom + top + pairs[2:]}
    rows, ends = [], []
    for b in range(64):
        rows += [(b,) + c for c in scenes.get(b, [])]
        ends.append(len(rows))
    return np.array(rows, np.int32), ends


@pytest.mark.parametrize("ts", [1, 4])
@pytest.mark.parametrize("k,s", [(3, 1), (2, 2), (3, 2)])
def test_kernel_map_at_the_ends_of_the_key_range(k, s, ts):
    """``nbr``, ``coords`` and ``scene_rows`` bit for bit against ``kernel_map_host`` (a dictionary: it cannot alias); the call neither
    raises nor reports overflow: these rows are inside the range.  ``ts`` 4: coordinates 4 * M and 4 * m."""
    rows, ends = _edge_rows()
    rows = rows * np.array([1, ts, ts, ts], np.int32)
    assert len(ends) == 64 and rows[:, 1:].max() == ts * M and rows[:, 1:].min() == ts * m
    want_c, want_e, want_n = sparse.kernel_map_host(rows, ends, ts, k, s)
    km = sparse.kernel_map(dev(rows), ends, ts, k, s)
    assert km.scene_rows == want_e and len(km.scene_rows) == 64
    assert np.array_equal(km.coords.cpu().numpy(), want_c)
    assert km.nbr.dtype == torch.int32 and np.array_equal(km.nbr.cpu().numpy(), want_n)
    assert ((want_n >= 0).sum(axis=1) > 1).sum() >= 8         # true hits exist too
    if (k, s) == (3, 1):                                     # the neighbours one step outside the range are absent, not aliased
        at = {tuple(r): i for i, r in enumerate(rows.tolist())}
        for b in (0, 62):
            assert want_n[at[(b, 0, 0, ts * M)], 13 + 9] == -1 and want_n[at[(b, 0, ts, ts * m)], 13 - 9] == -1
            assert want_n[at[(b, 0, ts * M, 5 * ts)], 13 + 3] == -1 and want_n[at[(b, ts * M, 7 * ts, 7 * ts)], 13 + 1] == -1
            assert want_n[at[(b + 1, ts * m, 7 * ts, 7 * ts)], 13 - 1] == -1
            assert want_n[at[(b, 0, 0, ts * M)], 13 - 9] == at[(b, 0, 0, ts * (M - 1))]
