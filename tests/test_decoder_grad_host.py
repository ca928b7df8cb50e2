"""The numpy specification of the decoder operators' backward (proxytransformation_amd/decoder_grad_host.py) on the CPU: each function in
float64 against torch autograd on a float64 restatement of the matching forward, a finite-difference spot check of the attention, the
precondition of ``sparse_util.hold`` on every input tests/test_gpu_decoder_grad.py draws (so the GPU module cannot trip on its own
yardstick), the exact attention case's independence of the summation order, and the C surface of the new entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

from proxytransformation_amd import _abi, decoder_grad_host as gh, decoder_host as dh
from tests import decoder_grad_util as gu
from tests import sparse_util as su

ROOT = su.ROOT
f64 = gu.f64


def close(name, got, ref, tol=1e-10, floor=1e-300):
    scale = max(float(np.abs(ref).max()), floor)
    assert got.shape == ref.shape, name
    assert float(np.abs(got - ref).max()) <= tol * scale, (name, float(np.abs(got - ref).max()), scale)


def t64(a, grad=True):
    t = torch.from_numpy(np.asarray(a, np.float64).copy())
    return t.requires_grad_() if grad else t


# ------------------------------------------------------------------------------------------------------------------ against autograd
def torch_attention(q, k, v, mask, H):
    """``decoder_host.attention_host`` in torch: masked keys and values replaced by zeros, a query without a key gets zeros."""
    B, Kq, C = q.shape
    L, hd = k.shape[1], C // H
    keep = ~mask[:, :, None]
    heads = lambda t, n: t.reshape(B, n, H, hd).transpose(1, 2)      # noqa: E731
    kh, vh = heads(torch.where(keep, k, torch.zeros_like(k)), L), heads(torch.where(keep, v, torch.zeros_like(v)), L)
    s = (heads(q, Kq) * (1.0 / hd ** 0.5)) @ kh.transpose(2, 3)
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    m = s.detach().amax(dim=-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(l == 0, torch.zeros_like(e), e / torch.where(l == 0, torch.ones_like(l), l))
    return (p @ vh).transpose(1, 2).reshape(B, Kq, C)


@pytest.mark.parametrize("hd,Kq,L,masked", [(32, 5, 70, True), (64, 65, 63, True), (32, 3, 9, False), (64, 2, 1, True)])
def test_attention_bwd_host_is_autograd_of_the_forward(hd, Kq, L, masked):
    c = gu.attn_case(hd, Kq, L, masked, seed=3)
    mask = c["mask"] if masked else np.zeros((gu.ATTN_B, L), bool)
    q, k, v = t64(c["q"]), t64(c["k"]), t64(c["v"])
    out = torch_attention(q, k, v, torch.from_numpy(mask), c["H"])
    close("forward", out.detach().numpy(), dh.attention_host(f64(c["q"]), f64(c["k"]), f64(c["v"]), mask, c["H"]))
    (out * t64(c["dout"], False)).sum().backward()
    got = gh.attention_bwd_host(f64(c["q"]), f64(c["k"]), f64(c["v"]), c["mask"], c["H"], f64(c["dout"]))
    for name, g, t in zip(("dq", "dk", "dv"), got, (q, k, v)):
        assert g.dtype == np.float64
        # one key: P = 1 and dq = dk = 0 exactly in autograd, in the host the rounding of dP - D, two equal sums of N(0, 1) products
        close(name, g, t.grad.numpy(), floor=1.0 if (L == 1 and name != "dv") else 1e-300)
    if masked:
        assert not got[1][mask].any() and not got[2][mask].any() and not got[0][2].any()      # scene 2 has no key


def test_attention_bwd_host_against_central_differences():
    """A handful of coordinates of q, k and v -- among them a masked key and the scene without a key -- at h = 1e-5 in float64."""
    c = gu.attn_case(32, 5, 70, True, seed=4)
    ops = {n: f64(c[n]) for n in ("q", "k", "v")}
    mask, H, dout = c["mask"], c["H"], f64(c["dout"])
    grads = dict(zip(("q", "k", "v"), gh.attention_bwd_host(ops["q"], ops["k"], ops["v"], mask, H, dout)))
    masked_key = int(np.flatnonzero(mask[0])[0])
    kept_key = int(np.flatnonzero(~mask[1])[0])
    spots = [("q", (0, 1, 7)), ("q", (1, 4, 40)), ("q", (2, 0, 3)), ("k", (0, 0, 5)), ("k", (1, kept_key, 33)), ("k", (0, masked_key, 2)),
             ("k", (2, 1, 1)), ("v", (0, 0, 9)), ("v", (1, kept_key, 60)), ("v", (0, masked_key, 11)), ("v", (2, 3, 0))]
    h = 1e-5
    top = max(float(np.abs(g).max()) for g in grads.values())
    for name, at in spots:
        vals = []
        for sign in (1.0, -1.0):
            moved = {n: a.copy() for n, a in ops.items()}
            moved[name][at] += sign * h
            vals.append(float((dh.attention_host(moved["q"], moved["k"], moved["v"], mask, H) * dout).sum()))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - grads[name][at]) <= 1e-7 * top, (name, at, fd, grads[name][at])
    assert grads["k"][0, masked_key, 2] == 0 and grads["v"][0, masked_key, 11] == 0 and grads["q"][2, 0, 3] == 0


def torch_linear(x, w, b, add, relu, cols, residual):
    cout = w.shape[0]
    cols = 0 if add is None else (cout if cols is None else cols)
    out = torch.cat([(x + add) @ w[:cols].T, x @ w[cols:].T], dim=-1) if cols else x @ w.T
    out = out + b
    if relu:
        out = torch.relu(out)
    return out if residual is None else out + residual


@pytest.mark.parametrize("kind", gu.LIN_KINDS)
def test_linear_bwd_host_is_autograd_of_the_forward(kind):
    c = gu.lin_case((192, 320), 65, kind)
    leaves = {n: t64(c[n]) for n in ("x", "weight", "bias", "add", "residual") if c[n] is not None}
    out = torch_linear(leaves["x"], leaves["weight"], leaves["bias"], leaves.get("add"), c["relu"], c["add_cols"], leaves.get("residual"))
    fwd = dh.linear_host(f64(c["x"]), f64(c["weight"]), f64(c["bias"]), f64(c["add"]), c["relu"], c["add_cols"])
    close("forward", out.detach().numpy(), fwd if c["residual"] is None else fwd + f64(c["residual"]))
    (out * t64(c["dy"], False)).sum().backward()
    got = gu.lin_refs_of(c)[1]
    assert set(got) == {"d" + n for n in leaves}
    for n, t in leaves.items():
        assert got["d" + n].dtype == np.float64
        if t.grad is None:                                   # add with add_cols = 0 reaches nothing
            assert n == "add" and kind == "add_0" and not got["d" + n].any()
        else:
            close(n, got["d" + n], t.grad.numpy())


@pytest.mark.parametrize("mode", gu.LN_MODES)
def test_layer_norm_bwd_host_is_autograd_of_the_forward(mode):
    c = gu.ln_case(256, 65, mode)
    x, w, b = t64(c["x"]), t64(c["ln"][0]), t64(c["ln"][1])
    C = x.shape[-1]
    out = torch.nn.functional.layer_norm(x, (C,), w, b, gu.EPS)
    close("forward", out.detach().numpy(), dh.layer_norm_host(f64(c["x"]), f64(c["ln"][0]), f64(c["ln"][1]), gu.EPS))
    loss = (out * t64(c["dy"], False)).sum() if c["dy"] is not None else 0.0
    leaves = dict(dx=x, dweight=w, dbias=b)
    if c["ln2"] is not None:
        w2, b2 = t64(c["ln2"][0]), t64(c["ln2"][1])
        out2 = torch.nn.functional.layer_norm(out, (C,), w2, b2, gu.EPS)
        leaves.update(dweight2=w2, dbias2=b2)
        if c["dy2"] is not None:
            loss = loss + (out2 * t64(c["dy2"], False)).sum()
    loss.backward()
    got = gu.ln_refs(256, 65, mode)[1]
    assert set(got) == set(gu.ln_names(mode))
    for n, t in leaves.items():
        ref = np.zeros(t.shape) if t.grad is None else t.grad.numpy()
        if np.abs(ref).max() == 0:
            assert not got[n].any(), n
        else:
            close(n, got[n], ref)


# ------------------------------------------------------------------------------------------------------------------ hold's precondition
def yardstick(name, r32, r64):
    """What ``sparse_util.hold`` asserts of its fp32 reference, here on the CPU."""
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == r64.shape, name
    if float(np.abs(r64).max()) == 0.0:
        assert not r32.any(), name
        return
    e = su.rel(r32, r64)
    assert e < 1e-5, (name, e)


def test_fp32_host_is_a_yardstick_on_every_attention_case_of_the_gpu_module():
    for case in gu.ATTN_CASES:
        r32, r64 = gu.attn_refs(*case)
        for n in ("dq", "dk", "dv"):
            if case[2] == 1 and n != "dv":
                # one key: P = 1 whatever q and k are, so dq = dk = 0; the references hold the rounding of dP - D, two equal sums.
                # No yardstick exists there: the GPU module holds these to gu.one_key_bound instead
                assert float(np.abs(r64[n]).max()) < 1e-12 and float(np.abs(r32[n]).max()) <= gu.one_key_bound(gu.attn_case(*case), n)
                continue
            yardstick(f"attention {case} {n}", r32[n], r64[n])
    _, _, s32, s64 = gu.strided_case()
    yardstick("attention strided", s32, s64)


def test_fp32_host_is_a_yardstick_on_every_linear_case_of_the_gpu_module():
    for shape, rows, kind in gu.LIN_CASES:
        c = gu.lin_case(shape, rows, kind)
        out = dh.linear_host(c["x"], c["weight"], c["bias"], c["add"], c["relu"], c["add_cols"]) if c["relu"] else None
        r32, r64 = gu.lin_refs_of(c, out)
        assert set(r32) == set(r64)
        for n in r32:
            yardstick(f"linear {shape} {rows} {kind} {n}", r32[n], r64[n])


def test_fp32_host_is_a_yardstick_on_the_nan_column_case_of_the_gpu_module():
    """The NaN-bias case's own ReLU mask (the fp32 host's result stands where the GPU module passes the device's): the gradients it
    holds by ``hold`` meet the precondition, the NaN columns pass nothing and nothing else is touched by the NaN."""
    c = gu.lin_nan_case()
    out = dh.linear_host(c["x"], c["weight"], c["bias"], c["add"], True, c["add_cols"])
    assert np.isnan(out[..., gu.NAN_COLUMNS]).all() and np.isfinite(np.delete(out, gu.NAN_COLUMNS, axis=-1)).all()
    r32, r64 = gu.lin_refs_of(c, out)
    for n in ("dx", "dadd", "dweight", "dbias"):
        assert np.isfinite(r32[n]).all() and np.isfinite(r64[n]).all(), n
        yardstick(f"linear NaN column {n}", r32[n], r64[n])
    assert not r64["dweight"][gu.NAN_COLUMNS].any() and not r64["dbias"][gu.NAN_COLUMNS].any()


def test_split_cases_take_the_ksplit_route_of_the_weight_gradient():
    """``train.mm_rows``'s rule restated: at least 1024 rows into fewer than 512 tiles is cut into slices.  The split cases of the GPU
    module meet it for every call ``_dweight_rows`` makes, the other linear cases and the layer body do not."""
    split = lambda M, N, K: K >= 1024 and ((M + 63) // 64) * ((N + 63) // 64) < 512      # noqa: E731
    for (cin, cout), rows, kind in gu.LIN_CASES:
        has_add, cols, _, _ = gu.lin_kind(kind, cout)
        cols = 0 if not has_add else (cout if cols is None else cols)
        calls = [M for M in (cols, cout - cols) if M]
        assert all(split(M, cin, rows) for M in calls) == (rows == gu.SPLIT_ROWS), ((cin, cout), rows, kind)
    assert sum(1 for c in gu.LIN_CASES if c[1] == gu.SPLIT_ROWS) == 3 and any(c[1] == gu.SPLIT_ROWS for c in gu.LIN_INTEGER_CASES)


def test_fp32_host_is_a_yardstick_on_every_layer_norm_case_of_the_gpu_module():
    for C, rows, mode in gu.LN_CASES:
        c = gu.ln_case(C, rows, mode)
        x = f64(c["x"])
        assert float(x.var(axis=-1).min()) > 0.3, (C, rows, mode)       # rows far from zero variance
        r32, r64 = gu.ln_refs(C, rows, mode)
        for n in gu.ln_names(mode):
            yardstick(f"layer_norm {C} {rows} {mode} {n}", r32[n], r64[n])


def test_fp32_torch_chain_is_a_yardstick_on_the_layer_body():
    c = gu.body_case()
    r32, r64 = gu.body_refs()
    for n in gu.BODY_LEAVES:
        assert r32[n].shape == c[n].shape and r32[n].size >= su.MIN_SAMPLE
        yardstick(f"body {n}", r32[n], r64[n])
    # the restatement is the chain of the host functions
    C, H = gu.BODY["C"], gu.BODY["H"]
    qkv = dh.linear_host(f64(c["query"]), f64(c["w_qkv"]), f64(c["b_qkv"]), f64(c["pos"]), add_cols=2 * C)
    o = dh.attention_host(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], np.zeros(qkv.shape[:2], bool), H)
    y = dh.linear_add_ln_host(o, f64(c["w_o"]), f64(c["b_o"]), f64(c["query"]), (f64(c["ln_w"]), f64(c["ln_b"])))
    got = gu.body_torch({k: torch.from_numpy(f64(c[k])) for k in gu.BODY_LEAVES}, H).numpy()
    close("body forward", got, y)


# ------------------------------------------------------------------------------------------------------------------ the exact cases
def test_exact_attention_case_does_not_depend_on_the_summation_order():
    """The condition for asking the device for the fp32 host's bits: on these operands the fp32 host gives the same bits with the keys
    (and, for dk / dv, the queries) visited in another order, and they are the float64 values."""
    c = gu.exact_attn_case()
    first = gh.attention_bwd_host(c["q"], c["k"], c["v"], c["mask"], c["H"], c["dout"])
    exact = gh.attention_bwd_host(f64(c["q"]), f64(c["k"]), f64(c["v"]), c["mask"], c["H"], f64(c["dout"]))
    rng = np.random.default_rng(5)
    pk, pq = rng.permutation(c["k"].shape[1]), rng.permutation(c["q"].shape[1])
    other = gh.attention_bwd_host(c["q"][:, pq], c["k"][:, pk], c["v"][:, pk], c["mask"][:, pk], c["H"], c["dout"][:, pq])
    back = (np.empty_like(first[0]), np.empty_like(first[1]), np.empty_like(first[2]))
    back[0][:, pq], back[1][:, pk], back[2][:, pk] = other
    assert (~c["mask"]).sum(axis=1).tolist() == [32, 32]
    for n, a, b, e in zip(("dq", "dk", "dv"), first, back, exact):
        assert a.dtype == np.float32 and gu.bits_equal(a, b), n
        assert np.array_equal(a.astype(np.float64), e), n
    assert first[0].any() and first[2].any() and not first[1].any()


def test_integer_linear_case_is_exact_in_fp32():
    for shape, rows, kind in gu.LIN_INTEGER_CASES:
        c = gu.lin_case(shape, rows, kind, integers=True)
        r32, r64 = gu.lin_refs_of(c)
        for n in r32:
            assert np.array_equal(r32[n].astype(np.float64), r64[n]), (kind, n)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_exports_declare_the_new_entry_points():
    lib = _abi.lib()
    hooks = ctypes.CDLL(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip_testhooks.so"))
    for name, params in su.assert_declared(gu.ENTRY_POINTS).items():
        assert len(params.split(",")) == len(_abi.SIGNATURES[name][1]), name
        getattr(hooks, name)
    assert _abi.ABI_VERSION == 13 and lib.ptx_abi_version() == 13 and hooks.ptx_abi_version() == 13
    assert "decoder_bwd.hip" in open(os.path.join(ROOT, "proxytransformation_amd", "csrc", "Makefile")).read()


def test_argument_checks_answer_einval_before_touching_a_device():
    lib = _abi.lib()
    EINVAL = -1
    err = lambda: lib.ptx_last_error()                       # noqa: E731
    st = lambda B=1, Kq=4, L=5, H=2, hd=32, ld=64: lib.ptx_dec_attention_stats(None, ld, None, ld, None, ld, None, B, Kq, L, H, hd, None, None,      # noqa: E731
                                                                                None)
    assert st(B=65) == EINVAL and b"B=65" in err() and st(Kq=0) == EINVAL and b"Kq=0" in err() and st(L=0) == EINVAL and b"L=0" in err()
    assert st(hd=48) == EINVAL and b"hd=48" in err() and st(ld=60) == EINVAL and b"ldq=60" in err() and st() == EINVAL and b"null" in err()
    assert b"ptx_dec_attention_stats" in err()
    bw = lambda B=1, Kq=4, L=5, H=2, hd=32, ld=64: lib.ptx_dec_attention_bwd(None, ld, None, ld, None, ld, None, B, Kq, L, H, hd, None, None, None,      # noqa: E731
                                                                              None, None, None, None, None)
    assert bw(B=0) == EINVAL and b"B=0" in err() and bw(Kq=1025) == EINVAL and b"Kq=1025" in err() and bw(L=0) == EINVAL and b"L=0" in err()
    assert bw(hd=16) == EINVAL and b"hd=16" in err() and bw(H=9, hd=64, ld=576) == EINVAL and b"H=9" in err()
    assert bw(ld=66) == EINVAL and b"ldq=66" in err() and bw() == EINVAL and b"null" in err() and b"ptx_dec_attention_bwd" in err()
    ln = lambda n, C, eps=1e-5: lib.ptx_dec_ln_bwd(None, n, C, None, None, eps, None, None, None, None, None, None, None, None)      # noqa: E731
    assert ln(0, 64) == EINVAL and b"n=0" in err() and ln(4, 576) == EINVAL and b"C=576" in err() and ln(4, 64, 0.0) == EINVAL and b"eps=0" in err()
    assert ln(4, 64) == EINVAL and b"null" in err() and b"ptx_dec_ln_bwd" in err()
