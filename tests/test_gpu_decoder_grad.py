"""The decoder's operators under autograd on the device (``attention``, ``linear``, ``layer_norm``, ``linear_add_ln`` of
proxytransformation_amd/decoder.py with ``differentiable=True``; csrc/decoder_bwd.hip) against their numpy specification
(decoder_grad_host.py): N(0, 1) operands by ``sparse_util.hold`` (the device error against float64 is at most 8 times the fp32 host's;
tests/test_decoder_grad_host.py asserts the yardstick's own precondition on every case drawn here), dyadic operands bit for bit, the mask
rules, forward bits, reproducibility, no synchronise, the refusals.

One rule is this module's own.  With a single key (L = 1) the probabilities are 1 whatever q and k are, so dq and dk are zero and both
references hold nothing but the rounding of ``dP - D``; ``hold`` has no yardstick there (its precondition cannot be met: the float64
reference is 1e-16).  Those two gradients are held to ``decoder_grad_util.one_key_bound``, the plain bound of a rounded sum of hd
products, instead; dv goes by ``hold`` as everywhere."""
import numpy as np
import pytest
import torch

from proxytransformation_amd import decoder, decoder_grad_host as gh, decoder_host as dh
from tests import decoder_grad_util as gu
from tests import sparse_util as su
from tests.test_gpu_decoder import count_synchronises      # the decoder's own counter of the Python-level synchronise entry points

pytestmark = pytest.mark.gpu
DEV = su.DEV
bits_equal = gu.bits_equal


def dev(a, grad=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_() if grad and t.is_floating_point() else t


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ attention
def run_attention(c, differentiable=True):
    q, k, v = dev(c["q"], True), dev(c["k"], True), dev(c["v"], True)
    out = decoder.attention(q, k, v, dev(c["mask"]), c["H"], differentiable=differentiable)
    (out * dev(c["dout"])).sum().backward()
    return out, dict(dq=host(q.grad), dk=host(k.grad), dv=host(v.grad))


@pytest.mark.parametrize("hd,Kq,L,masked", gu.ATTN_CASES)
def test_attention_gradients(hd, Kq, L, masked):
    c = gu.attn_case(hd, Kq, L, masked)
    r32, r64 = gu.attn_refs(hd, Kq, L, masked)
    out, got = run_attention(c)
    with torch.no_grad():
        plain = decoder.attention(dev(c["q"]), dev(c["k"]), dev(c["v"]), dev(c["mask"]), c["H"])
    assert bits_equal(host(out), host(plain))
    for n in ("dq", "dk", "dv"):
        assert got[n].shape == r64[n].shape and got[n].dtype == np.float32
        if L == 1 and n != "dv":                             # zero but for the rounding of dP - D (the module's docstring)
            worst, bound = float(np.abs(got[n]).max()), gu.one_key_bound(c, n)
            print(f"attention {n} at one key: |gpu| {worst:.3e}  bound {bound:.3e}")
            assert worst <= bound, (n, worst, bound)
        else:
            su.hold(f"attention hd={hd} Kq={Kq} L={L} masked={masked} {n}", got[n], r32[n], r64[n])
    if masked:
        m = c["mask"]
        assert not got["dk"][m].view(np.uint32).any() and not got["dv"][m].view(np.uint32).any()      # bit zero under the mask
        assert not got["dq"][2].view(np.uint32).any()                                                  # and for the scene without a key
        assert not got["dk"][2].view(np.uint32).any() and not got["dv"][2].view(np.uint32).any()


def test_attention_on_column_ranges_of_one_projection():
    """q, k, v are the three column ranges of one (B,n,3C) tensor: the gradient of that tensor is [dq | dk | dv]."""
    qkv_h, dout, r32, r64 = gu.strided_case()
    C = qkv_h.shape[2] // 3
    qkv = dev(qkv_h, True)
    out = decoder.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], None, gu.ATTN_H, differentiable=True)
    (out * dev(dout)).sum().backward()
    assert qkv.grad.shape == qkv.shape and qkv.grad.is_contiguous()
    su.hold("attention strided d(qkv)", host(qkv.grad), r32, r64)
    with torch.no_grad():
        plain = decoder.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], None, gu.ATTN_H)
    assert bits_equal(host(out), host(plain))


def test_nan_and_inf_under_masked_keys_leave_no_trace():
    c = dict(gu.attn_case(64, 65, 200, True))
    _, clean = run_attention(c)
    k, v = c["k"].copy(), c["v"].copy()
    rows = np.argwhere(c["mask"])
    for i, (b, l) in enumerate(rows):
        k[b, l, i % k.shape[2]] = np.nan if i % 2 else np.inf
        v[b, l, (3 * i) % v.shape[2]] = -np.inf if i % 2 else np.nan
    k[2], v[0, 64:128] = np.nan, np.inf                      # the scene without a key; the tile that is masked throughout
    _, dirty = run_attention(dict(c, k=k, v=v))
    for n in ("dq", "dk", "dv"):
        assert np.isfinite(dirty[n]).all() and bits_equal(clean[n], dirty[n]), n


def test_exact_attention_case_bit_for_bit():
    """q = 0, 32 unmasked keys, integers in k, v, dout: every intermediate is dyadic (tests/test_decoder_grad_host.py shows the fp32
    host does not depend on the summation order there), so dq and dv are the fp32 host's bit for bit."""
    c = gu.exact_attn_case()
    out, got = run_attention(c)
    dq, dk, dv = gh.attention_bwd_host(c["q"], c["k"], c["v"], c["mask"], c["H"], c["dout"])
    assert bits_equal(host(out), dh.attention_host(c["q"], c["k"], c["v"], c["mask"], c["H"]))
    assert bits_equal(got["dq"], dq) and bits_equal(got["dv"], dv)
    assert dq.any() and dv.any() and not got["dk"].any()


# ------------------------------------------------------------------------------------------------------------------ linear
LIN_LEAVES = ("x", "weight", "bias", "add", "residual")


def run_linear(c, differentiable=True):
    t = {n: dev(c[n], True) for n in LIN_LEAVES}
    out = decoder.linear(t["x"], t["weight"], t["bias"], add=t["add"], relu=c["relu"], add_cols=c["add_cols"], residual=t["residual"],
                         differentiable=differentiable)
    (out * dev(c["dy"])).sum().backward()
    return out, {"d" + n: host(v.grad) for n, v in t.items() if v is not None}


@pytest.mark.parametrize("shape,rows,kind", gu.LIN_CASES)
def test_linear_gradients(shape, rows, kind):
    c = gu.lin_case(shape, rows, kind)
    out, got = run_linear(c)
    with torch.no_grad():
        plain = decoder.linear(dev(c["x"]), dev(c["weight"]), dev(c["bias"]), add=dev(c["add"]), relu=c["relu"], add_cols=c["add_cols"],
                               residual=dev(c["residual"]))
    assert bits_equal(host(out), host(plain))
    r32, r64 = gu.lin_refs_of(c, host(out) if c["relu"] else None)      # the ReLU's mask of both references: the device's result
    assert set(got) == set(r64)
    for n in sorted(got):
        assert got[n].shape == r64[n].shape and got[n].dtype == np.float32 and got[n].size >= su.MIN_SAMPLE, n
        if not r64[n].any():                                 # add with add_cols = 0 (the middle of Cout = 64 too)
            assert c["add_cols"] == 0 and n == "dadd" and not got[n].any()
            continue
        su.hold(f"linear {shape} rows={rows} {kind} {n}", got[n], r32[n], r64[n])


@pytest.mark.parametrize("shape,rows,kind", gu.LIN_INTEGER_CASES)
def test_linear_integer_operands_bit_for_bit(shape, rows, kind):
    """Integers in [-4, 4]: every product and sum is exact in fp32 (and the double column sums of exact slabs stay exact), so the bits
    are the fp32 host's on the plain route (257 rows) and on the k-split route (1100 rows) of the weight gradient."""
    c = gu.lin_case(shape, rows, kind, integers=True)
    _, got = run_linear(c)
    r32, _ = gu.lin_refs_of(c)
    for n in sorted(got):
        assert bits_equal(got[n], r32[n]), n


def test_linear_nan_output_under_relu_passes_no_gradient():
    """A NaN bias makes a whole output column NaN behind the ReLU; ``dy * (out > 0)`` is zero there: the column passes nothing on."""
    c, cols = gu.lin_nan_case(), gu.NAN_COLUMNS
    out, got = run_linear(c)
    assert np.isnan(host(out)[..., cols]).all()
    for n, g in got.items():
        assert np.isfinite(g).all(), n
    assert not got["dweight"][cols].any() and not got["dbias"][cols].any()
    r32, r64 = gu.lin_refs_of(c, host(out))
    for n in ("dx", "dadd", "dweight"):
        su.hold(f"linear NaN column {n}", got[n], r32[n], r64[n])


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def run_layer_norm(c, differentiable=True):
    x = dev(c["x"], True)
    ln = tuple(dev(p, True) for p in c["ln"]) + (gu.EPS,)
    ln2 = None if c["ln2"] is None else tuple(dev(p, True) for p in c["ln2"]) + (gu.EPS,)
    res = decoder.layer_norm(x, ln, ln2, differentiable=differentiable)
    outs = (res,) if ln2 is None else res
    loss = 0.0
    for o, g in zip(outs, (c["dy"], c["dy2"])):
        if g is not None:
            loss = loss + (o * dev(g)).sum()
    loss.backward()
    grads = dict(dx=x.grad, dweight=ln[0].grad, dbias=ln[1].grad)
    if ln2 is not None:
        grads.update(dweight2=ln2[0].grad, dbias2=ln2[1].grad)
    return outs, grads


@pytest.mark.parametrize("C,rows,mode", gu.LN_CASES)
def test_layer_norm_gradients(C, rows, mode):
    c = gu.ln_case(C, rows, mode)
    r32, r64 = gu.ln_refs(C, rows, mode)
    outs, grads = run_layer_norm(c)
    with torch.no_grad():
        plain = decoder.layer_norm(dev(c["x"]), tuple(dev(p) for p in c["ln"]) + (gu.EPS,),
                                   None if c["ln2"] is None else tuple(dev(p) for p in c["ln2"]) + (gu.EPS,))
    for a, b in zip(outs, (plain,) if c["ln2"] is None else plain):
        assert bits_equal(host(a), host(b))
    for n in gu.ln_names(mode):
        if not r64[n].any():                                 # the second norm's parameters when its result went unused
            assert mode == "dy" and n in ("dweight2", "dbias2") and (grads[n] is None or not host(grads[n]).any())
            continue
        g = host(grads[n])
        assert g.shape == r64[n].shape and g.dtype == np.float32 and g.size >= su.MIN_SAMPLE, n
        su.hold(f"layer_norm C={C} rows={rows} {mode} {n}", g, r32[n], r64[n])


# ------------------------------------------------------------------------------------------------------------------ a layer body
def run_body(differentiable=True):
    c = gu.body_case()
    C, H = gu.BODY["C"], gu.BODY["H"]
    t = {n: dev(c[n], True) for n in gu.BODY_LEAVES}
    qkv = decoder.linear(t["query"], t["w_qkv"], t["b_qkv"], add=t["pos"], add_cols=2 * C, differentiable=differentiable)
    o = decoder.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], None, H, differentiable=differentiable)
    y = decoder.linear_add_ln(o, t["w_o"], t["b_o"], t["query"], (t["ln_w"], t["ln_b"], gu.EPS), differentiable=differentiable)
    if differentiable:
        (y * dev(c["G"])).sum().backward()
    return y, {n: v.grad for n, v in t.items()}


def test_layer_body_under_autograd():
    """linear (positions on q and k) -> attention on the three column ranges -> linear + identity + LayerNorm: every leaf's gradient against
    float64 torch autograd of the same chain, the fp32 torch chain on the CPU as the yardstick; the forward bits of the plain calls; two
    backward passes, equal bits; no synchronise in forward plus backward."""
    r32, r64 = gu.body_refs()
    y, first = run_body()
    torch.cuda.synchronize()
    with count_synchronises() as calls:
        y2, second = run_body()
    assert calls == [], f"forward plus backward synchronised: {calls}"
    torch.cuda.synchronize()
    with torch.no_grad():
        plain, _ = run_body(differentiable=False)
    assert bits_equal(host(y), host(plain)) and bits_equal(host(y), host(y2))
    for n in gu.BODY_LEAVES:
        g = host(first[n])
        assert bits_equal(g, host(second[n])), n
        su.hold(f"layer body {n}", g, r32[n], r64[n])


def test_two_backward_calls_give_the_same_bits():
    a = gu.attn_case(64, 130, 200, True)
    assert all(bits_equal(x, y) for x, y in zip(run_attention(a)[1].values(), run_attention(a)[1].values()))
    lin = gu.lin_case((256, 768), 257, "relu")
    assert all(bits_equal(x, y) for x, y in zip(run_linear(lin)[1].values(), run_linear(lin)[1].values()))
    ln = gu.ln_case(512, 257, "both")
    assert all(bits_equal(host(x), host(y)) for x, y in zip(run_layer_norm(ln)[1].values(), run_layer_norm(ln)[1].values()))


def test_without_the_keyword_nothing_changes():
    """``differentiable=False`` (the default) detaches as before: the result carries no graph, the same bits."""
    c = gu.attn_case(32, 65, 65, True)
    q = dev(c["q"], True)
    out = decoder.attention(q, dev(c["k"]), dev(c["v"]), dev(c["mask"]), c["H"])
    assert not out.requires_grad
    tracked = decoder.attention(q, dev(c["k"]), dev(c["v"]), dev(c["mask"]), c["H"], differentiable=True)
    assert tracked.requires_grad and bits_equal(host(out), host(tracked))
    lc = gu.lin_case((64, 64), 65, "plain")
    assert not decoder.linear(dev(lc["x"], True), dev(lc["weight"]), dev(lc["bias"])).requires_grad
    nc = gu.ln_case(64, 65, "single")
    assert not decoder.layer_norm(dev(nc["x"], True), tuple(dev(p) for p in nc["ln"])).requires_grad


def test_refusals_come_before_any_launch():
    x = torch.zeros(1, 4, 64, device=DEV, requires_grad=True)
    w, b = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    slot = torch.full((1, 4, 64), 7.0, device=DEV)
    with pytest.raises(ValueError, match="out2"):
        decoder.layer_norm(x, (w, b), (w, b), out2=slot, differentiable=True)
    with pytest.raises(ValueError, match="out2"):
        decoder.linear_add_ln(x, torch.zeros(64, 64, device=DEV), b, x, (w, b), (w, b), out2=slot, differentiable=True)
    assert bool((slot == 7.0).all())
    with pytest.raises(NotImplementedError, match="relu"):
        decoder.linear(x, torch.zeros(64, 64, device=DEV), b, relu=True, residual=x, differentiable=True)
