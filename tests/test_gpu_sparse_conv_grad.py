"""Backward of the sparse convolution and max-pool (``differentiable=True``; csrc/sparse_bwd.hip): the transposed kernel map bit for bit
against ``kernel_map_transpose_host``; dfeats / dweight / dbias / dresidual against the float64 restatement ``sparse_conv3d_bwd_host``
under the rule of tests/test_gpu_sparse_conv.py (``sparse_util.hold``: 8 x the error of the SAME chain in fp32 on the CPU, the ReLU mask of both
references taken from the GPU's forward ``out``); bitwise repeatability; the split of dweight over row chunks at its boundaries; the
opt-in surface; the pool's routing bit for bit; a training BasicBlock with ``nn.BatchNorm1d`` on the rows; and the link the backward
exists for: neck (train) -> differentiable quantize -> kernel map -> stem convolution -> loss.backward().

Rows: those of tests/test_gpu_sparse_conv.py (a dense 6x6x6 block, ~2100 random rows with over 90 % of the neighbours missing, an empty
scene, a one-row scene; the total is no multiple of 64), the 512-wide case on 600 random rows."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from proxytransformation_amd import sparse
from tests import sparse_util as su
from tests.sparse_util import DEV

pytestmark = pytest.mark.gpu


_t = su.dev


# ------------------------------------------------------------------------------------------------------------------ transposed map
@pytest.mark.parametrize("ts", [1, 4])
@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (1, 2), (2, 2)])
def test_transposed_map_is_the_host_restatement(k, s, ts):
    """``KernelMap.nbr_t`` is filled by the first differentiable call on the map (here: the pool's backward) and reused afterwards."""
    _, _, nbr = su.host_map(ts, k, s)
    km = su.device_map(ts, k, s)
    n_in = su.rows(ts)[0].shape[0]
    assert km.nbr_t is None and km.n_in == n_in
    x = torch.zeros(n_in, 4, device=DEV, requires_grad=True)
    sparse.sparse_max_pool3d(x, km, differentiable=True).sum().backward()
    first = km.nbr_t
    assert first is not None and first.dtype == torch.int32 and tuple(first.shape) == (n_in, k ** 3)
    assert np.array_equal(first.cpu().numpy(), sparse.kernel_map_transpose_host(nbr, n_in))
    sparse.sparse_max_pool3d(x, km, differentiable=True).sum().backward()
    assert km.nbr_t is first                                 # built once per map


# ------------------------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("cin,cout,k,s", su.LAYER_SHAPES)
def test_gradients_against_the_float64_restatement(cin, cout, k, s):
    """The full set splits dweight over several row chunks with a partial last one (64 -> 64: 10 chunks of 256 rows over 2351)."""
    ts, cut = su.layer_rows(cin)
    _, _, nbr = su.host_map(ts, k, s, cut)
    km = su.device_map(ts, k, s, cut)
    n_in = su.rows(ts, cut)[0].shape[0]
    ops = su.operands(n_in, nbr.shape[0], cin, cout, k ** 3, seed=cin + cout)
    full = k == 1                                            # bias + scale + shift + residual + ReLU on the 1x1 stride-2 layer
    out, G, got = su.grad_case(km, nbr, ops, full, relu=full, seed=cin)
    out2, _, again = su.grad_case(km, nbr, ops, full, relu=full, seed=cin)
    with torch.no_grad():                                    # forward identity: the plain call, and differentiable under no_grad
        kw = {u: _t(ops[u]) for u in ("bias", "scale", "shift", "residual")} if full else {}
        plain = sparse.sparse_conv3d(_t(ops["feats"]), km, _t(ops["weight"]), relu=full, **kw)
        quiet = sparse.sparse_conv3d(_t(ops["feats"]), km, _t(ops["weight"]), relu=full, differentiable=True, **kw)
    assert torch.equal(out, plain) and torch.equal(quiet, plain) and torch.equal(out2, plain) and quiet.grad_fn is None
    r32, r64 = su.grad_refs(nbr, ops, out.cpu().numpy(), G, full, relu=full)
    tag = f"bwd Cin={cin} Cout={cout} k={k} s={s} rows={n_in}->{nbr.shape[0]}"
    for name, key in (("feats", "dfeats"), ("weight", "dweight")) + ((("bias", "dbias"), ("residual", "dresidual")) if full else ()):
        g = got[name]
        assert g is not None and g.dtype == torch.float32 and tuple(g.shape) == tuple(ops[name].shape), name
        assert torch.equal(g, again[name]), f"{name}: two backward calls on the same inputs differ"
        su.hold(f"{tag} {key}", g.cpu().numpy().reshape(r64[key].shape), r32[key], r64[key])
    if full:
        lone = (nbr < 0).all(axis=1)                         # rows without a neighbour feed dbias / dresidual, not dfeats / dweight
        assert lone.sum() > 100 and (out.cpu().numpy()[lone] > 0).any()
        assert np.array_equal(got["residual"].cpu().numpy(), np.where(out.cpu().numpy() > 0, G, np.float32(0)))


def test_one_row_scene_alone():
    """Fewer output rows than one row chunk -- and than one tile of anything."""
    rows = np.array([[0, 5, -7, 2]], np.int32)
    km = sparse.kernel_map(_t(rows), [1], 1, 3, 1)
    nbr = sparse.kernel_map_host(rows, [1], 1, 3, 1)[2]
    assert np.array_equal(km.nbr.cpu().numpy(), nbr) and (nbr >= 0).sum() == 1
    ops = su.operands(1, 1, 64, 64, 27, seed=3)
    out, G, got = su.grad_case(km, nbr, ops, full=True, relu=False, seed=1)
    r32, r64 = su.grad_refs(nbr, ops, out.cpu().numpy(), G, True, relu=False)
    for name, key in (("feats", "dfeats"), ("weight", "dweight"), ("bias", "dbias"), ("residual", "dresidual")):
        su.hold(f"bwd one row {key}", got[name].cpu().numpy().reshape(r64[key].shape), r32[key], r64[key])
    assert (got["weight"].cpu().numpy()[np.arange(27) != 13] == 0).all()      # only the centre offset has a pair


def test_needs_input_grad_and_rejections():
    _, _, nbr = su.host_map(4, 3, 1)
    km = su.device_map(4, 3, 1)
    ops = su.operands(nbr.shape[0], nbr.shape[0], 64, 64, 27, seed=77)
    _, _, both = su.grad_case(km, nbr, ops, full=True, relu=True, seed=5)
    assert tuple(both["bias"].shape) == tuple(ops["bias"].shape)
    _, _, only_f = su.grad_case(km, nbr, ops, full=True, relu=True, seed=5, wrt=("feats",))
    assert only_f["weight"] is None and only_f["bias"] is None and only_f["residual"] is None
    assert torch.equal(only_f["feats"], both["feats"])
    _, _, only_w = su.grad_case(km, nbr, ops, full=True, relu=True, seed=5, wrt=("weight",))
    assert only_w["feats"] is None and only_w["bias"] is None and torch.equal(only_w["weight"], both["weight"])
    _, _, only_b = su.grad_case(km, nbr, ops, full=True, relu=True, seed=5, wrt=("bias", "residual"))
    assert only_b["feats"] is None and only_b["weight"] is None
    assert torch.equal(only_b["bias"], both["bias"]) and torch.equal(only_b["residual"], both["residual"])
    # ReLU without scale: dresidual is gz itself
    f, r = _t(ops["feats"], grad=True), _t(ops["residual"], grad=True)
    out = sparse.sparse_conv3d(f, km, _t(ops["weight"]), residual=r, relu=True, differentiable=True)
    G = torch.randn(tuple(out.shape), generator=torch.Generator().manual_seed(2)).to(DEV)
    (out * G).sum().backward()
    assert torch.equal(r.grad, torch.where(out.detach() > 0, G, torch.zeros_like(G)))
    ref = sparse.sparse_conv3d_bwd_host(G.cpu().numpy().astype(np.float64), ops["feats"].astype(np.float64), nbr, ops["weight"].astype(np.float64),
                                        out=out.detach().cpu().numpy(), relu=True)["dfeats"]
    assert float(np.abs(f.grad.cpu().numpy() - ref).max()) <= 1e-5 * float(np.abs(ref).max())
    # the module hands its (1, Cout) bias parameter through: the gradient comes back in that shape
    m = sparse.SparseConv3d(64, 64, 3, bias=True, differentiable=True).to(DEV)
    m(_t(ops["feats"]), km).sum().backward()
    assert tuple(m.bias.grad.shape) == (1, 64) and tuple(m.kernel.grad.shape) == (27, 64, 64)
    n = nbr.shape[0]
    with pytest.raises(ValueError, match="scale"):
        sparse.sparse_conv3d(_t(ops["feats"], grad=True), km, _t(ops["weight"]), scale=_t(ops["scale"], grad=True), differentiable=True)
    with pytest.raises(ValueError, match="Cin=16"):
        sparse.sparse_conv3d(torch.zeros(n, 16, device=DEV, requires_grad=True), km, torch.zeros(27, 16, 64, device=DEV), differentiable=True)
    with torch.no_grad():                                    # forward-only keeps accepting that width
        assert sparse.sparse_conv3d(torch.zeros(n, 16, device=DEV), km, torch.zeros(27, 16, 64, device=DEV), differentiable=True).shape == (n, 64)
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_conv3d(_t(ops["feats"], grad=True), km, _t(ops["weight"]))
    with pytest.raises(NotImplementedError, match="backward"):
        sparse.sparse_max_pool3d(_t(ops["feats"], grad=True), km)


# ------------------------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("k,s", [(2, 2), (3, 1)])
def test_pool_routes_the_gradient_bit_for_bit(k, s):
    _, _, nbr = su.host_map(4, k, s)
    km = su.device_map(4, k, s)
    rng = np.random.default_rng(9)
    feats = rng.standard_normal((su.rows(4)[0].shape[0], 64)).astype(np.float32)
    feats[:, :8] = np.round(feats[:, :8])                    # ties: they go to the smallest j
    G = rng.standard_normal((nbr.shape[0], 64)).astype(np.float32)
    x = _t(feats, grad=True)
    out = sparse.sparse_max_pool3d(x, km, differentiable=True)
    with torch.no_grad():
        plain = sparse.sparse_max_pool3d(_t(feats), km)
        assert torch.equal(sparse.sparse_max_pool3d(x, km, differentiable=True), plain)
    assert torch.equal(out.detach(), plain) and np.array_equal(plain.cpu().numpy(), sparse.sparse_max_pool3d_host(feats, nbr))
    out.backward(_t(G))
    want = sparse.sparse_max_pool3d_bwd_host(G, feats, nbr)
    assert want.dtype == np.float32 and np.array_equal(x.grad.cpu().numpy(), want)
    if k == 3:
        assert ((sparse.kernel_map_transpose_host(nbr, len(feats)) >= 0).sum(1) > 1).any()      # overlapping windows


# ------------------------------------------------------------------------------------------------------------------ composition
class _TorchConv(nn.Module):
    """The same layer as the composition a user could write from ``nbr`` (the reference block's convolution)."""

    def __init__(self, kernel, nbr):
        super().__init__()
        self.kernel, self.nbr = nn.Parameter(kernel), nbr

    def forward(self, x):
        return su.composition(x, self.nbr, self.kernel)


def _block(conv1, bn1, conv2, bn2, x):
    h = torch.relu(bn1(conv1(x)))
    return torch.relu(bn2(conv2(h)) + x)


def test_training_basic_block_against_float64_torch():
    """SparseConv3d(64, 64, 3, differentiable=True) -> nn.BatchNorm1d(64).train() -> ReLU -> conv -> BN -> + x -> ReLU on 600 random
    rows; every parameter gradient and dx against the same block in torch float64 on the CPU, yardstick: that block in float32."""
    ts = 4
    _, _, nbr = su.host_map(ts, 3, 1, 600)
    km = su.device_map(ts, 3, 1, 600)
    rng = np.random.default_rng(17)
    x_np = rng.standard_normal((nbr.shape[0], 64)).astype(np.float32)
    G = rng.standard_normal((nbr.shape[0], 64)).astype(np.float32)
    torch.manual_seed(3)
    convs = [sparse.SparseConv3d(64, 64, 3, differentiable=True) for _ in range(2)]
    bns = [nn.BatchNorm1d(64) for _ in range(2)]
    with torch.no_grad():
        for bn in bns:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.2)

    def run(dtype, device):
        if device == "cpu":
            cs = [_TorchConv(c.kernel.detach().to(dtype).clone(), torch.from_numpy(nbr)) for c in convs]
        else:
            cs = [copy.deepcopy(c).to(device) for c in convs]
        bs = [copy.deepcopy(b).to(device=device, dtype=dtype).train() for b in bns]
        x = torch.from_numpy(x_np).to(device=device, dtype=dtype).requires_grad_()
        if device == "cpu":
            out = _block(cs[0], bs[0], cs[1], bs[1], x)
        else:
            out = _block(lambda v: cs[0](v, km), bs[0], lambda v: cs[1](v, km), bs[1], x)
        (out * torch.from_numpy(G).to(device=device, dtype=dtype)).sum().backward()
        grads = {"dx": x.grad, "kernel1": cs[0].kernel.grad, "kernel2": cs[1].kernel.grad, "bn1.weight": bs[0].weight.grad,
                 "bn1.bias": bs[0].bias.grad, "bn2.weight": bs[1].weight.grad, "bn2.bias": bs[1].bias.grad}
        return out.detach().cpu().numpy(), {k: v.detach().cpu().numpy() for k, v in grads.items()}, cs

    out_gpu, got, cs = run(torch.float32, DEV)
    out64, ref64, _ = run(torch.float64, "cpu")
    out32, ref32, _ = run(torch.float32, "cpu")
    su.hold("train BasicBlock out", out_gpu, out32, out64)
    for name in got:
        su.hold(f"train BasicBlock {name}", got[name], ref32[name], ref64[name])
    before = cs[0].kernel.detach().clone()
    torch.optim.SGD(cs[0].parameters(), lr=0.1).step()
    assert not torch.equal(cs[0].kernel.detach(), before) and bool(torch.isfinite(cs[0].kernel).all())


def test_the_neck_trains_through_the_stem_convolution():
    """neck (train) -> quantize(0.01, grad) -> kernel_map(k3 s2) -> SparseConv3d(3, 64, 3, 2, differentiable=True) -> loss.backward():
    the gradient on the neck's outputs is non-zero exactly on the points the voxel rows kept and equals the twin's whose stem is
    the torch composition over the same nbr (float64 the reference, float32 the yardstick; the scatter to the points is exact)."""
    from oracle import oracle
    from tests.test_gpu_voxel_grad import VX, _np, _train_outs
    from tests.test_voxel_grad_host import first_index
    m, outs = _train_outs(VX)
    coords, feats, ends = m.quantize(outs, 0.01, return_scene_rows=True)
    assert feats.grad_fn is not None
    km = sparse.kernel_map(coords, ends, 1, 3, 2)
    torch.manual_seed(5)
    stem = sparse.SparseConv3d(3, 64, 3, 2, differentiable=True).to(DEV)
    out = stem(feats, km)
    G = torch.randn(tuple(out.shape), generator=torch.Generator().manual_seed(6)).to(DEV)
    prm = [p for p in m.parameters() if p.requires_grad]
    grads = torch.autograd.grad((out * G).sum(), list(outs) + [stem.kernel] + prm, allow_unused=True)
    douts, dkernel, dprm = grads[:len(outs)], grads[len(outs)], grads[len(outs) + 1:]
    # kept points: the first point of every voxel row
    rc, rf, rinv = oracle.voxelize(_np(outs), 0.01)
    assert np.array_equal(coords.cpu().numpy(), rc)
    rep = first_index(rinv, len(rc))
    kept = np.zeros(sum(int(o.shape[0]) for o in outs), bool)
    kept[rep] = True
    flat = np.concatenate([g.cpu().numpy() for g in douts])
    assert np.array_equal((flat != 0).any(axis=1), kept) and 0 < kept.sum()
    # the twin: the torch composition over the same nbr, on the same feature values
    nbr = km.nbr.cpu()
    twins = {}
    for dt in (torch.float64, torch.float32):
        f = feats.detach().cpu().to(dt).requires_grad_()
        w = stem.kernel.detach().cpu().to(dt).requires_grad_()
        gf, gw = torch.autograd.grad((su.composition(f, nbr, w) * G.cpu().to(dt)).sum(), (f, w))
        scattered = np.zeros((len(kept), 3), gf.numpy().dtype)          # features = cat(outs)[rep]: row r's gradient goes to point rep[r]
        scattered[rep] = gf.numpy()
        twins[dt] = (scattered, gw.numpy())
    su.hold("link d outs", flat, twins[torch.float32][0], twins[torch.float64][0])
    su.hold("link d stem kernel", dkernel.cpu().numpy(), twins[torch.float32][1], twins[torch.float64][1])
    assert sum(g is not None and float(g.abs().max()) > 0 and bool(torch.isfinite(g).all()) for g in dprm) > 20      # it reaches the neck
