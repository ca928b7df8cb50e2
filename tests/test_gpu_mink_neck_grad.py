"""Training through the sparse neck on the device (``MinkNeck(differentiable=True)``; csrc/neck_bwd.hip, the ``_act`` entry points of
csrc/sparse_norm.hip, the wide and the generative backward of csrc/sparse_bwd.hip).  Every case is called twice and must give the same
bits.  Float results are held by ``sparse_util.hold`` (max |got - ref64| / max |ref64| at most 8 x the same statistic of the fp32 CPU
chain), row routing bit for bit.  The near-tie precondition of the end-to-end inputs under the training scores is checked without a GPU
in tests/test_mink_neck_grad_host.py."""
import copy
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proxytransformation_amd import MinkNeck, _abi, neck, neck_host, sparse
from proxytransformation_amd.backbone import SparseLevel
from tests import neck_util as nu
from tests import sparse_util as su

pytestmark = pytest.mark.gpu
_bits = nu.bits
GOLDEN = os.path.join(su.ROOT, "tests", "golden", "sparse_conv_bwd_128_64_digests.json")


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """Two calls, the same bits (tensors or dicts of tensors)."""
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k])
    else:
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ norm + ELU
DEAD = slice(16, 24)               # the column block whose pre-activation sits at -100: out = expm1f(-100) = -1, derivative exactly 0


def _norm_case(C, n, residual, seed):
    ops = su.norm_operands(n, C, 0.0, seed)
    _, bn32, gpu = su.bn_pair(C, seed + 1)
    with torch.no_grad():
        for bn in (bn32, gpu):
            bn.bias[DEAD] = -100.0
    return ops, bn32, gpu


def _hold_two_rows(name, got, r32, r64):
    """``hold`` without its cap on the yardstick.  With two rows ``xhat = +-1 / sqrt(1 + eps / var)`` and ``dx = w rstd ((gy - a) - xhat b)``
    is a difference of terms that agree to ``eps / var``: the fp32 CPU chain itself is only good to ~1e-5 .. 1e-4 of max |dx| there (which
    ``sparse_util.hold`` refuses as a yardstick), so the rule -- 8 x the fp32 CPU chain's statistic -- is applied as it stands."""
    e_gpu, e_cpu = su.rel(got, r64), su.rel(r32, r64)
    print(f"sparse_conv {name}: gpu {e_gpu:.3e}  fp32-cpu {e_cpu:.3e}  ratio {e_gpu / max(e_cpu, 1e-30):.2f}")
    assert e_cpu < 1e-3 and e_gpu <= 8.0 * e_cpu, (name, e_gpu, e_cpu)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("n", [2, 256, 257, 2317])
@pytest.mark.parametrize("C", [64, 512])
def test_norm_elu_forward_and_backward(C, n, residual):
    """A training BatchNorm with the fused ELU through ``sparse_batch_norm(elu=True, differentiable=True)``: x ~ N(0, 1); the bias of
    columns 16 .. 23 is -100, so their pre-activation sits at -100, ``out = -1`` exactly and every gradient through them is exactly 0."""
    ops, bn32, gpu0 = _norm_case(C, n, residual, 300 + n + C)
    eps, w, b = bn32.eps, _np(bn32.weight), _np(bn32.bias)
    runs = []
    for _ in range(2):
        gpu = copy.deepcopy(gpu0)
        x, res = su.dev(ops["x"], grad=True), su.dev(ops["residual"], grad=True) if residual else None
        out = sparse.sparse_batch_norm(x, gpu, res, elu=True, differentiable=True)
        (out * su.dev(ops["g"])).sum().backward()
        assert int(gpu.num_batches_tracked) == 1
        runs.append(dict(out=out.detach(), dx=x.grad, dweight=gpu.weight.grad, dbias=gpu.bias.grad, rm=gpu.running_mean, rv=gpu.running_var,
                         **({"dresidual": res.grad} if residual else {})))
    _same(runs[0], runs[1])
    got = {k: _np(v) for k, v in runs[0].items()}
    use = dict(weight=w, bias=b, **({"residual": ops["residual"]} if residual else {}))
    run32 = [_np(bn32.running_mean).copy(), _np(bn32.running_var).copy()]
    run64 = [r.astype(np.float64) for r in run32]
    r32 = sparse.sparse_norm_host(ops["x"], [n], eps, elu=True, running=run32, momentum=0.1, **use)
    r64 = sparse.sparse_norm_host(ops["x"].astype(np.float64), [n], eps, elu=True, running=run64, momentum=0.1,
                                  **{k: v.astype(np.float64) for k, v in use.items()})
    name = f"norm+ELU C={C} n={n} res={int(residual)}"
    su.hold(f"{name} out", got["out"], r32, r64)
    su.hold(f"{name} running_mean", got["rm"], run32[0], run64[0])
    su.hold(f"{name} running_var", got["rv"], run32[1], run64[1])
    assert 0.2 < float((got["out"] < 0).mean()) < 0.8
    if not residual:
        assert (got["out"][:, DEAD] == -1.0).all()
    g32 = sparse.sparse_norm_bwd_host(ops["g"], ops["x"], [n], eps, w, out=got["out"], elu=True)
    g64 = sparse.sparse_norm_bwd_host(ops["g"].astype(np.float64), ops["x"].astype(np.float64), [n], eps, w.astype(np.float64), out=got["out"],
                                      elu=True)
    for k in ("dx", "dweight", "dbias") + (("dresidual",) if residual else ()):
        assert got[k].shape == g64[k].shape and got[k].dtype == np.float32, k
        (_hold_two_rows if (n == 2 and k == "dx") else su.hold)(f"{name} {k}", got[k], g32[k], g64[k])
    if not residual:                                         # the derivative at out = -1 is exactly 0
        assert (got["dx"][:, DEAD] == 0).all() and (got["dweight"][DEAD] == 0).all() and (got["dbias"][DEAD] == 0).all()


def _raw_norm(act, ops, n, C, new_entry, out_in=None):
    """One forward and one backward through the entry points themselves: ``(out, dx, dweight, dbias, dresidual)``."""
    lib = _abi.lib()
    x, w, b, res, g = (su.dev(ops[k]) for k in ("x", "weight", "bias", "residual", "g"))
    ws = torch.empty(lib.ptx_sparse_norm_workspace_bytes(n, 1, C), dtype=torch.uint8, device=su.DEV)
    stats, out = torch.empty(1, 2, C, device=su.DEV), torch.empty(n, C, device=su.DEV)
    seg = (ctypes.c_int32 * 1)(n)
    fwd = lib.ptx_sparse_norm_fwd_act if new_entry else lib.ptx_sparse_norm_fwd
    _abi.check(fwd(x.data_ptr(), seg, 1, n, C, 1e-5, w.data_ptr(), b.data_ptr(), res.data_ptr(), act, None, None, 0.0, stats.data_ptr(),
                   out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "norm fwd")
    if out_in is not None:
        out = out_in
    dx, dres, dw, db = torch.empty(n, C, device=su.DEV), torch.empty(n, C, device=su.DEV), torch.empty(C, device=su.DEV), torch.empty(C, device=su.DEV)
    if new_entry:
        _abi.check(lib.ptx_sparse_norm_bwd_act(g.data_ptr(), x.data_ptr(), out.data_ptr(), act, seg, 1, n, C, stats.data_ptr(), w.data_ptr(),
                                               dx.data_ptr(), dw.data_ptr(), db.data_ptr(), dres.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   "norm bwd act")
    else:
        _abi.check(lib.ptx_sparse_norm_bwd(g.data_ptr(), x.data_ptr(), out.data_ptr() if act else None, seg, 1, n, C, stats.data_ptr(),
                                           w.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), dres.data_ptr(), ws.data_ptr(), ws.numel(),
                                           _stream()), "norm bwd")
    return dict(out=out, dx=dx, dweight=dw, dbias=db, dresidual=dres)


@pytest.mark.parametrize("act", [0, 1])
def test_norm_selectors_none_and_relu_give_the_old_entry_points_bits(act):
    n, C = 2317, 128
    ops = su.norm_operands(n, C, 0.0, 340 + act)
    old, new, again = _raw_norm(act, ops, n, C, False), _raw_norm(act, ops, n, C, True), _raw_norm(act, ops, n, C, True)
    _same(old, new)
    _same(new, again)
    if act:
        assert 0.3 < float((old["out"] == 0).float().mean()) < 0.7


def test_elu_backward_keeps_a_nan_on_the_device():
    """THE NaN RULE: an ``out`` of NaN gives a NaN ``gy`` (``dresidual``) and NaN column sums -- never a dropped gradient; -1 gives 0."""
    n, C = 257, 64
    ops = su.norm_operands(n, C, 0.0, 350)
    clean = _raw_norm(2, ops, n, C, True)
    out = clean["out"].clone()
    out[5, 3], out[200, 7], out[6, 3] = float("nan"), float("nan"), -1.0
    runs = [_raw_norm(2, ops, n, C, True, out_in=out) for _ in range(2)]
    ref = sparse.sparse_norm_bwd_host(ops["g"], ops["x"], [n], 1e-5, ops["weight"], out=_np(out), elu=True)
    for r in runs:
        gy = _np(r["dresidual"])
        assert np.isnan(gy[5, 3]) and np.isnan(gy[200, 7]) and gy[6, 3] == 0.0 and np.isnan(gy).sum() == 2
        ok = ~np.isnan(gy)
        assert np.array_equal(gy[ok].view(np.uint32), ref["dresidual"][ok].view(np.uint32)) and np.isnan(ref["dresidual"][~ok]).all()
        for k in ("dbias", "dweight"):
            v = _np(r[k])
            assert np.isnan(v[[3, 7]]).all() and np.isnan(v).sum() == 2, k
        dx = _np(r["dx"])
        assert np.isnan(dx[:, [3, 7]]).all() and np.isnan(dx).sum() == 2 * n
    keep = [c for c in range(C) if c not in (3, 7)]
    assert torch.equal(runs[0]["dx"][:, keep], clean["dx"][:, keep])


# ------------------------------------------------------------------------------------------------------------------ convolution backward
@pytest.mark.parametrize("cin,cout,cut", [(1024, 256, 600), (576, 64, 0), (1024, 64, 600)])
def test_conv_backward_past_512_input_channels(cin, cout, cut):
    """dfeats and dweight of the raw k3 convolution on ``sparse_util.rows`` (the 1024-wide shapes on the random scene cut to 600 rows, as
    the 512 -> 512 layer test does), the widths of ``out_block_3`` (27 x 1024 -> 256) among them."""
    nbr = su.host_map(4, 3, 1, cut)[2]
    km = su.device_map(4, 3, 1, cut)
    ops = su.operands(nbr.shape[0], nbr.shape[0], cin, cout, 27, 360 + cin + cout)
    runs = [su.grad_case(km, nbr, ops, False, False, 361) for _ in range(2)]
    _same(runs[0][0], runs[1][0])
    _same({k: v for k, v in runs[0][2].items()}, {k: v for k, v in runs[1][2].items()})
    out, G, grads = runs[0]
    r32, r64 = su.conv_refs(nbr, ops)
    su.hold(f"conv {cin}->{cout} out", _np(out), r32, r64)
    g32, g64 = su.grad_refs(nbr, ops, _np(out), G, False, False)
    su.hold(f"conv {cin}->{cout} dfeats", _np(grads["feats"]), g32["dfeats"], g64["dfeats"])
    su.hold(f"conv {cin}->{cout} dweight", _np(grads["weight"]), g32["dweight"], g64["dweight"])
    assert _abi.lib().ptx_sparse_conv3d_bwd_workspace_bytes(nbr.shape[0], 27, cin, cout) == su.dw_plan(nbr.shape[0], 27, cin, cout)[2]


def _digest(t):
    return hashlib.sha256(_np(t).tobytes()).hexdigest()


def test_conv_backward_at_128_64_is_the_parent_commits_bits():
    """One shape at Cin <= 512: the gradients are bit for bit those of the library before the backward learned the wide inputs and the
    table-less map -- tests/golden/sparse_conv_bwd_128_64_digests.json holds the SHA-256 of out, dfeats, dweight, dbias and dresidual as
    that library computed them for these operands (full epilogue with ReLU; all rows of ``sparse_util.rows(4)``)."""
    nbr = su.host_map(4, 3, 1)[2]
    km = su.device_map(4, 3, 1)
    ops = su.operands(nbr.shape[0], nbr.shape[0], 128, 64, 27, 370)
    out, _, grads = su.grad_case(km, nbr, ops, True, True, 371)
    got = dict(out=_digest(out), **{k: _digest(v) for k, v in grads.items()})
    print(json.dumps(got))
    assert got == json.load(open(GOLDEN))


# ------------------------------------------------------------------------------------------------------------------ generative backward
@pytest.mark.parametrize("cin,cout,n", [(64, 64, 65), (1024, 512, 1), (128, 128, 2357), (64, 128, 700)])
def test_generative_backward(cin, cout, n):
    """``dfeats[i] = sum_j g[8 i + j] @ kernel[j]^T`` and ``dkernel[j] = feats^T @ g[j::8]``; at 65, 2357 and 700 rows the dkernel plan
    (``sparse_util.dw_plan`` over the 8 n children) uses 3, 30 and 22 chunks, added as slabs in ascending order."""
    rows = nu.scene_rows_of([n])[0] * np.array([1, 8, 8, 8], np.int32)
    rng = np.random.default_rng(380 + n)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    kernel = (rng.standard_normal((8, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    G = rng.standard_normal((8 * n, cout)).astype(np.float32)
    S = su.dw_plan(8 * n, 8, cin, cout)[1]
    assert S == {65: 3, 1: 1, 2357: 30, 700: 22}[n]
    runs = []
    for _ in range(2):
        tx, tk = su.dev(x, grad=True), su.dev(kernel, grad=True)
        oc, oe, out = neck.conv_transpose_gen(su.dev(rows), [n], 8, tx, tk, differentiable=True)
        (out * su.dev(G)).sum().backward()
        runs.append(dict(out=out.detach(), oc=oc, dfeats=tx.grad, dkernel=tk.grad))
    _same(runs[0], runs[1])
    with torch.no_grad():
        plain = neck.conv_transpose_gen(su.dev(rows), [n], 8, su.dev(x), su.dev(kernel))
    _same(runs[0]["out"], plain[2])                          # the recorded forward: the inference call's bits
    _bits(runs[0]["oc"], neck_host.conv_transpose_gen_host(rows, [n], 8, x, kernel)[0])
    g32 = neck_host.conv_transpose_gen_bwd_host(G, x, kernel)
    g64 = neck_host.conv_transpose_gen_bwd_host(G.astype(np.float64), x.astype(np.float64), kernel.astype(np.float64))
    su.hold(f"generative {cin}->{cout} n={n} dfeats", _np(runs[0]["dfeats"]), g32["dfeats"], g64["dfeats"])
    su.hold(f"generative {cin}->{cout} n={n} dkernel", _np(runs[0]["dkernel"]), g32["dkernel"], g64["dkernel"])


# ------------------------------------------------------------------------------------------------------------------ row routing
@pytest.mark.parametrize("C", [4, 512])
def test_union_routing(C):
    """``neck_util.union_regime_case`` (64 scenes, every scene kind): ``a_dest`` / ``b_dest`` are the restatement's and consistent with
    the returned coordinates; with an integer-valued ``g`` the gradients ``dA = g[a_dest]``, ``dB = g[b_dest]`` are bit for bit."""
    a, a_ends, b, b_ends = nu.union_regime_case()
    assert set(nu.union_kinds(a, a_ends, b, b_ends)) == set(nu.UNION_KINDS)
    rng = np.random.default_rng(390 + C)
    fa, fb = (rng.integers(-8, 9, (len(r), C)).astype(np.float32) for r in (a, b))
    c, e, f = neck_host.union_add_host(a, a_ends, fa, b, b_ends, fb)
    a_dest, b_dest = neck_host.union_dest_host(a, a_ends, b, b_ends)
    G = rng.integers(-100, 101, f.shape).astype(np.float32)
    runs = []
    for _ in range(2):
        ta, tb = su.dev(fa, grad=True), su.dev(fb, grad=True)
        gc, ge, gf, (ad, bd) = neck.union_add(su.dev(a), a_ends, ta, su.dev(b), b_ends, tb, 4, differentiable=True, return_dest=True)
        (gf * su.dev(G)).sum().backward()
        runs.append(dict(c=gc, f=gf.detach(), ad=ad, bd=bd, dA=ta.grad, dB=tb.grad))
        assert ge == e
    _same(runs[0], runs[1])
    r = runs[0]
    _bits(r["c"], c)
    _bits(r["f"], f)
    _bits(r["ad"], a_dest)
    _bits(r["bd"], b_dest)
    assert np.array_equal(_np(r["c"])[_np(r["ad"])], a) and np.array_equal(_np(r["c"])[_np(r["bd"])], b)
    _bits(r["dA"], neck_host.rows_gather_host(G, a_dest))
    _bits(r["dB"], neck_host.rows_gather_host(G, b_dest))
    with torch.no_grad():                                    # the plain entry point: same results
        pc, pe, pf = neck.union_add(su.dev(a), a_ends, su.dev(fa), su.dev(b), b_ends, su.dev(fb), 4)
    assert pe == e
    _same(pf, r["f"])


def _prune_case(scores, rows, ends, feats, k, G):
    runs = []
    for _ in range(2):
        tf = su.dev(feats, grad=True)
        gc, ge, gf, gk = neck.topk_prune(su.dev(scores), su.dev(rows), ends, tf, k, differentiable=True)
        (gf * su.dev(G[:gf.shape[0]])).sum().backward()
        runs.append(dict(c=gc, f=gf.detach(), keep=gk, dU=tf.grad))
    _same(runs[0], runs[1])
    keep = neck_host.topk_keep_host(scores, ends, k)
    c, e, f = neck_host.prune_host(keep, rows, ends, feats)
    assert ge == e and np.array_equal(_np(runs[0]["keep"]), keep)
    _bits(runs[0]["f"], f)
    dU = neck_host.rows_gather_host(G[:f.shape[0]], neck_host.prune_dest_host(keep))
    _bits(runs[0]["dU"], dU)
    got = _np(runs[0]["dU"])
    assert (got[~keep] == 0).all() and not np.signbit(got[~keep]).any()         # dropped rows: +0.0
    return keep


@pytest.mark.parametrize("n", [2, 256, 257, 513])
def test_prune_routing(n):
    rng = np.random.default_rng(400 + n)
    rows, ends = nu.scene_rows_of([n])
    scores, feats = rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, 128)).astype(np.float32)
    G = rng.standard_normal((n, 128)).astype(np.float32)
    for k in (1, n // 2 + 1, n):
        keep = _prune_case(scores, rows, ends, feats, k, G)
        assert keep.sum() == k


def test_prune_routing_over_64_scenes_with_empty_ones():
    sizes = [nu.TOPK_64_SIZES[i % len(nu.TOPK_64_SIZES)] for i in range(64)]
    rows, ends = nu.scene_rows_of(sizes)
    rng = np.random.default_rng(410)
    n = ends[-1]
    scores, feats = rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, 64)).astype(np.float32)
    keep = _prune_case(scores, rows, ends, feats, nu.TOPK_64_K, rng.standard_normal((n, 64)).astype(np.float32))
    assert 0 in sizes and 0 < keep.sum() < n


# ------------------------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("n", [1, 17, 2317])
@pytest.mark.parametrize("C,K", [(64, 1), (256, 16), (512, 5)])
def test_head_backward(C, K, n, bias):
    rng = np.random.default_rng(420 + C + K + n)
    x = rng.standard_normal((n, C)).astype(np.float32)
    w, b = (rng.standard_normal((1, C, K)) / 16).astype(np.float32), rng.standard_normal((1, K)).astype(np.float32)
    G = rng.standard_normal((n, K)).astype(np.float32)
    runs = []
    for _ in range(2):
        tx, tw, tb = su.dev(x, grad=True), su.dev(w, grad=True), su.dev(b, grad=True) if bias else None
        cls, score = neck.neck_head(tx, tw, tb, differentiable=True)
        assert cls.requires_grad and not score.requires_grad
        (cls * su.dev(G)).sum().backward()
        runs.append(dict(cls=cls.detach(), score=score, dfeats=tx.grad, dweight=tw.grad, **({"dbias": tb.grad} if bias else {})))
    _same(runs[0], runs[1])
    with torch.no_grad():
        plain = neck.neck_head(su.dev(x), su.dev(w), su.dev(b) if bias else None)
    _same(runs[0]["cls"], plain[0])
    _same(runs[0]["score"], plain[1])
    got = {k: _np(v) for k, v in runs[0].items()}
    assert got["dweight"].shape == (1, C, K) and (not bias or got["dbias"].shape == (1, K))
    g32 = neck_host.head_bwd_host(G, x, w)
    g64 = neck_host.head_bwd_host(G.astype(np.float64), x.astype(np.float64), w.astype(np.float64))
    name = f"head bwd C={C} K={K} n={n}"
    su.hold(f"{name} dfeats", got["dfeats"], g32["dfeats"], g64["dfeats"])
    su.hold(f"{name} dweight", got["dweight"][0], g32["dweight"], g64["dweight"])
    if bias:
        su.hold(f"{name} dbias", got["dbias"][0], g32["dbias"], g64["dbias"])


# ------------------------------------------------------------------------------------------------------------------ end to end
def _torch_chain(levels, state, masks, dtype, G_f, G_c, batch, k, classes):
    """The training step as a user could compose it in torch on the CPU in ``dtype`` from the HOST kernel maps and the device's keep
    masks: ``(feats, cls, {parameter / level name: gradient}, the module with its updated buffers)``."""
    m = MinkNeck(classes, list(nu.WIDTHS), nu.OUT, 0.01, k)
    m.load_state_dict(state)
    m = m.to(dtype).train()
    feats_in = [torch.from_numpy(lv.feats).to(dtype).requires_grad_() for lv in levels]

    def block(z, bn):
        return F.elu(F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps))

    top = len(levels) - 1
    c, ends, ts, x = levels[top].coords, list(levels[top].scene_rows), levels[top].tensor_stride, feats_in[top]
    out_levels, step = [], 0
    for i in range(top, -1, -1):
        if i < top:
            up = getattr(m, f"up_block_{i + 1}")
            gc = nu.children(c, ts // 2)
            ge = [8 * e for e in ends]
            g = torch.stack([x @ up[0].kernel[j] for j in range(8)], 1).reshape(8 * x.shape[0], -1)
            g = block(g, up[1].bn)
            g = block(su.composition(g, sparse.kernel_map_host(gc, ge, ts // 2, 3, 1)[2], up[3].kernel), up[4].bn)
            lv = levels[i]
            uc, ue, _ = neck_host.union_add_host(lv.coords, lv.scene_rows, np.zeros((len(lv.coords), 1), np.float32), gc, ge,
                                                 np.zeros((len(gc), 1), np.float32))
            a_dest, b_dest = neck_host.union_dest_host(lv.coords, lv.scene_rows, gc, ge)
            u = torch.zeros(len(uc), g.shape[1], dtype=dtype).index_add(0, torch.from_numpy(a_dest).long(), feats_in[i])
            u = u.index_add(0, torch.from_numpy(b_dest).long(), g)
            mask = np.asarray(masks[step], bool)
            step += 1
            c, ends, _ = neck_host.prune_host(mask, uc, ue, np.zeros((len(uc), 1), np.float32))
            x = u[torch.from_numpy(mask)]
            ts //= 2
        ob = getattr(m, f"out_block_{i}")
        out = block(su.composition(x, sparse.kernel_map_host(c, ends, ts, 3, 1)[2], ob[0].kernel), ob[1].bn)
        cls = out @ m.conv_cls.kernel[0] + m.conv_cls.bias
        out_levels.append((out, cls, torch.zeros(len(c), 3), ends))
    feats, scores, _ = MinkNeck._to_batch(out_levels, batch, torch.cat)
    loss = sum((f * torch.from_numpy(g).to(dtype)).sum() for f, g in zip(feats, G_f)) + \
        sum((s * torch.from_numpy(g).to(dtype)).sum() for s, g in zip(scores, G_c))
    loss.backward()
    grads = {name: p.grad.numpy() for name, p in m.named_parameters()}
    grads.update({f"levels[{i}].feats": t.grad.numpy() for i, t in enumerate(feats_in)})
    return [f.detach().numpy() for f in feats], [s.detach().numpy() for s in scores], grads, m


E2E_CASES = {"one class, three scenes": (nu.e2e_levels, nu.e2e_neck, 3, nu.K_PRUNE),
             "three classes, an empty scene": (nu.e2e_levels_b, nu.e2e_neck_b, 4, nu.K_PRUNE_B)}


@pytest.mark.parametrize("case", list(E2E_CASES))
def test_end_to_end_training_step_shipped_widths(case):
    """One ``forward`` / ``backward`` of ``loss = sum(feats * G_f) + sum(cls * G_c)`` through ``MinkNeck(differentiable=True)`` in training
    mode on the inputs of the two eval end-to-end tests (``neck_util``).  Rows, order, masks and points: bit for bit (twice, and the points
    against ``forward_host(training=True, keep=the device's masks)``); outputs, the gradient of every parameter and of every level's
    ``feats`` and the updated running statistics: ``hold`` against the torch CPU composition in float64 and float32 on the device's row
    sets; ``num_batches_tracked`` + 1 per BatchNorm; the device's masks against the host's own float64 masks as in
    ``neck_util.end_to_end``; the same module in ``.eval()`` under ``no_grad``: the default module's bits."""
    levels, base, batch, k = E2E_CASES[case][0](), E2E_CASES[case][1](), E2E_CASES[case][2], E2E_CASES[case][3]
    classes = base.num_classes
    state = base.state_dict()
    gm0 = MinkNeck(classes, list(nu.WIDTHS), nu.OUT, 0.01, k, differentiable=True)
    gm0.load_state_dict(state)
    gm0 = gm0.to(su.DEV)

    def dev_levels(grad):
        return [SparseLevel(su.dev(lv.feats, grad=grad), su.dev(lv.coords), lv.scene_rows, lv.tensor_stride) for lv in levels]

    with torch.no_grad():                                    # flag set, .eval(), no_grad: today's folded route
        plain = copy.deepcopy(base).to(su.DEV)(dev_levels(False), batch)
        folded = copy.deepcopy(gm0).eval()(dev_levels(False), batch)
    for a, b in zip(plain, folded):
        for ta, tb in zip(a, b):
            _same(ta, tb)

    rng = np.random.default_rng(430)
    G_f = G_c = None
    runs = []
    for _ in range(2):
        gm = copy.deepcopy(gm0).train()
        lv = dev_levels(True)
        keep = []
        feats, scores, points = gm(lv, batch, keep_out=keep)
        if G_f is None:
            G_f = [rng.standard_normal(tuple(f.shape)).astype(np.float32) for f in feats]
            G_c = [rng.standard_normal(tuple(s.shape)).astype(np.float32) for s in scores]
        loss = sum((f * su.dev(g)).sum() for f, g in zip(feats, G_f)) + sum((s * su.dev(g)).sum() for s, g in zip(scores, G_c))
        loss.backward()
        grads = {name: p.grad for name, p in gm.named_parameters()}
        grads.update({f"levels[{i}].feats": l.feats.grad for i, l in enumerate(lv)})
        assert all(g is not None for g in grads.values())
        runs.append(dict(feats=torch.cat(feats).detach(), scores=torch.cat(scores).detach(), points=torch.cat(points), keep=torch.cat(keep),
                         **grads, **{f"buffer {n}": b for n, b in gm.named_buffers()}))
    _same(runs[0], runs[1])
    masks = [_np(m_) for m_ in keep]
    got = {n: _np(v) for n, v in runs[0].items()}

    trace = []
    base_train = copy.deepcopy(base).train()
    f64, s64, p64 = base_train.forward_host(levels, batch, np.float64, keep=masks, trace=trace, training=True)
    f32, s32, _ = base_train.forward_host(levels, batch, np.float32, keep=masks, training=True)
    _bits(got["points"], np.concatenate(p64))
    su.hold("neck train feats", got["feats"], np.concatenate(f32), np.concatenate(f64))
    su.hold("neck train scores", got["scores"], np.concatenate(s32), np.concatenate(s64))
    for step, (mask, tr) in enumerate(zip(masks, trace)):   # the device's masks against the host's own float64 masks
        s = tr["scores"]
        margin = nu.NEAR_TIE * float(np.abs(s).max())
        differ = np.nonzero(mask != tr["keep"])[0]
        ties = {scene: count for scene, count, _ in nu.near_ties(s, tr["scene_rows"], k)}
        lo = 0
        for scene, hi in enumerate(tr["scene_rows"]):
            d = differ[(differ >= lo) & (differ < hi)]
            if hi - lo > k:
                kth = np.sort(s[lo:hi])[::-1][k - 1]
                print(f"step {step} scene {scene}: {len(d)} rows differ, k-th score {kth:+.4f}")
                assert (np.abs(s[d] - kth) <= margin).all() and len(d) <= ties[scene] <= 0.02 * k
            else:
                assert len(d) == 0
            lo = hi

    t64 = _torch_chain(levels, state, masks, torch.float64, G_f, G_c, batch, k, classes)
    t32 = _torch_chain(levels, state, masks, torch.float32, G_f, G_c, batch, k, classes)
    assert float(np.abs(np.concatenate(t64[0]) - np.concatenate(f64)).max()) < 1e-9      # the composition is the restated chain
    su.hold("neck train feats (torch)", got["feats"], np.concatenate(t32[0]), np.concatenate(t64[0]))
    su.hold("neck train scores (torch)", got["scores"], np.concatenate(t32[1]), np.concatenate(t64[1]))
    assert set(t64[2]) == {n for n in got if not n.startswith("buffer ") and n not in ("feats", "scores", "points", "keep")}
    for name in t64[2]:
        assert got[name].shape == t64[2][name].shape, name
        su.hold(f"neck train d {name}", got[name], t32[2][name], t64[2][name])
    b32, b64 = dict(t32[3].named_buffers()), dict(t64[3].named_buffers())
    for name, ref in b64.items():
        if name.endswith("num_batches_tracked"):
            assert int(got[f"buffer {name}"]) == int(state[name]) + 1, name         # incremented once per BatchNorm
        else:
            su.hold(f"neck train {name}", got[f"buffer {name}"], b32[name].numpy(), ref.numpy())
