"""What the decoder-gradient test modules (and tools/decoder_bwd_time.py) share: the entry points, the cases of the three operators with
their operands, the references of a case in float32 and float64 (computed once, never changed), the exact cases, and the layer body with
its torch restatement.  The CPU module asserts ``sparse_util.hold``'s precondition on every case the GPU module draws.  A plain module: no
tests, no marks."""
import functools
import itertools

import numpy as np
import torch

from proxytransformation_amd import decoder_grad_host as gh

ENTRY_POINTS = ("ptx_dec_attention_stats", "ptx_dec_attention_bwd", "ptx_dec_ln_bwd")
EPS = 1e-5


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ attention
ATTN_B, ATTN_H = 3, 2
# (head dimension, queries, keys, masked): one query, a tile and a row, two tiles and two rows; one key, a tile less / exactly / more than
# one key, four tiles with the last one partial
ATTN_CASES = list(itertools.product((32, 64), (1, 65, 130), (1, 63, 64, 65, 200), (False, True)))


def attn_mask(L, seed=0):
    """``(3,L)`` bool, True = ignore: a fifth of the keys at random; the middle tile 64 .. 127 masked throughout (where L reaches past
    it); the last partial tile masked throughout (where there is one behind a whole tile); scene 2 without a key.  Scenes 0 and 1 keep
    at least one key when L > 1; at L = 1 scene 0 keeps its key and scene 1 has none."""
    rng = np.random.default_rng(1000 + 7 * L + seed)
    m = rng.random((ATTN_B, L)) < 0.2
    if L > 128:
        m[:2, 64:128] = True
    if L > 64 and L % 64:
        m[:2, (L // 64) * 64:] = True
    m[0, 0] = False
    m[1, min(L - 1, 5)] = L == 1
    m[2] = True
    return m


@functools.lru_cache(maxsize=None)
def attn_case(hd, Kq, L, masked, seed=0):
    """q (3,Kq,2 hd), k, v (3,L,2 hd), dout ~ N(0, 1), mask (3,L) or None."""
    rng = np.random.default_rng(hd * 1000003 + Kq * 1009 + L * 7 + int(masked) + 17 * seed)
    C = ATTN_H * hd
    draw = lambda n: rng.standard_normal((ATTN_B, n, C)).astype(np.float32)      # noqa: E731
    return dict(q=draw(Kq), k=draw(L), v=draw(L), dout=draw(Kq), mask=attn_mask(L, seed) if masked else None, H=ATTN_H)


def attn_refs_of(c):
    r32 = gh.attention_bwd_host(c["q"], c["k"], c["v"], c["mask"], c["H"], c["dout"])
    r64 = gh.attention_bwd_host(f64(c["q"]), f64(c["k"]), f64(c["v"]), c["mask"], c["H"], f64(c["dout"]))
    assert all(a.dtype == np.float32 for a in r32) and all(a.dtype == np.float64 for a in r64)
    return dict(zip(("dq", "dk", "dv"), r32)), dict(zip(("dq", "dk", "dv"), r64))


@functools.lru_cache(maxsize=None)
def attn_refs(hd, Kq, L, masked, seed=0):
    return attn_refs_of(attn_case(hd, Kq, L, masked, seed))


def one_key_bound(c, name):
    """With a single key P = 1, so dq and dk are zero and what a fp32 evaluation returns is the rounding of dS = dP - D: two sums of
    hd products dO_c v_c that agree in exact arithmetic, each within hd 2^-24 sum_c |dO_c v_c| of it (the plain bound of a sum of hd
    rounded products).  dq = dS k / sqrt(hd), and dk sums dS q / sqrt(hd) over the Kq queries with Kq more roundings: the bound below
    is that, with the largest operand for each factor."""
    hd = c["q"].shape[2] // c["H"]
    Kq = c["q"].shape[1]
    prod = np.abs(f64(c["dout"])[:, :, None, :] * f64(c["v"])[:, None, :, :])      # (B,Kq,L,C)
    ds = 2.0 * hd * 2.0 ** -24 * float(prod.reshape(prod.shape[:3] + (c["H"], hd)).sum(axis=-1).max())
    if name == "dq":
        return ds * float(np.abs(c["k"]).max()) / np.sqrt(hd) * (1 + 2.0 ** -22)
    return ds * Kq * float(np.abs(c["q"]).max()) / np.sqrt(hd) * (1 + Kq * 2.0 ** -22)


STRIDED = dict(hd=32, n=70, seed=5)


@functools.lru_cache(maxsize=None)
def strided_case():
    """Self attention on the column ranges of one ``(3,n,3C)`` tensor, no mask; the gradient of that tensor is ``[dq | dk | dv]``."""
    rng = np.random.default_rng(STRIDED["seed"])
    C, n = ATTN_H * STRIDED["hd"], STRIDED["n"]
    qkv = rng.standard_normal((ATTN_B, n, 3 * C)).astype(np.float32)
    c = dict(q=qkv[:, :, :C], k=qkv[:, :, C:2 * C], v=qkv[:, :, 2 * C:], dout=rng.standard_normal((ATTN_B, n, C)).astype(np.float32),
             mask=None, H=ATTN_H)
    r32, r64 = attn_refs_of(c)
    cat = lambda r: np.concatenate([r["dq"], r["dk"], r["dv"]], axis=2)      # noqa: E731
    return qkv, c["dout"], cat(r32), cat(r64)


@functools.lru_cache(maxsize=None)
def exact_attn_case():
    """q = 0, hd = 64, 32 unmasked keys of 40 in two scenes, k, v, dout integers in [-2, 2]: every logit is 0, every probability 1 / 32,
    and every intermediate of the backward a dyadic number of fewer than 24 bits, so any summation order gives the same fp32 bits."""
    rng = np.random.default_rng(77)
    B, Kq, L, H, hd = 2, 70, 40, 2, 64
    ints = lambda *s: rng.integers(-2, 3, s).astype(np.float32)      # noqa: E731
    mask = np.zeros((B, L), bool)
    mask[0, [3, 9, 17, 20, 21, 30, 38, 39]] = True
    mask[1, 32:] = True
    return dict(q=np.zeros((B, Kq, H * hd), np.float32), k=ints(B, L, H * hd), v=ints(B, L, H * hd), dout=ints(B, Kq, H * hd), mask=mask, H=H)


# ------------------------------------------------------------------------------------------------------------------ linear
LIN_SHAPES = ((64, 64), (192, 320), (256, 768))
ROWS = (1, 65, 257)
LIN_KINDS = ("plain", "add_all", "add_mid", "add_0", "relu", "residual")
# past 1024 rows the weight gradient takes the k-split route (``train.mm_rows``: slices over the rows into slabs, added in double by
# ``ptx_op_colsum`` onto a row range of dW), as every shape of the decoder does: 1100 rows are 4 slices of 275; "add_mid" splits both
# disjoint row ranges of dW (384 rows each), "plain" the whole of it, "relu" behind the mask
SPLIT_ROWS = 1100
LIN_SPLIT_CASES = [((256, 768), SPLIT_ROWS, kind) for kind in ("plain", "add_mid", "relu")]
LIN_CASES = list(itertools.product(LIN_SHAPES, ROWS, LIN_KINDS)) + LIN_SPLIT_CASES
# (shape, rows, kind) of the integer-operand cases that are held bit for bit: below and past the k-split threshold
LIN_INTEGER_CASES = [((256, 768), 257, "plain"), ((256, 768), 257, "add_mid"), ((256, 768), SPLIT_ROWS, "plain"),
                     ((256, 768), SPLIT_ROWS, "add_mid")]
NAN_COLUMNS = [7, 200]


def lin_kind(kind, cout):
    """``(has add, add_cols, relu, has residual)``; the middle: the multiple of 64 at or below half of Cout (0 at Cout = 64)."""
    return dict(plain=(False, None, False, False), add_all=(True, None, False, False), add_mid=(True, (cout // 128) * 64, False, False),
                add_0=(True, 0, False, False), relu=(True, (cout // 128) * 64, True, False), residual=(False, None, False, True))[kind]


@functools.lru_cache(maxsize=None)
def lin_case(shape, rows, kind, integers=False):
    cin, cout = shape
    has_add, cols, relu, has_res = lin_kind(kind, cout)
    rng = np.random.default_rng(cin * 10007 + cout * 101 + rows * 7 + LIN_KINDS.index(kind) + 50000 * int(integers))
    if integers:
        draw = lambda *s: rng.integers(-4, 5, s).astype(np.float32)      # noqa: E731
        w = draw(cout, cin)
    else:
        draw = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
        w = draw(cout, cin) / np.float32(np.sqrt(cin))
    return dict(x=draw(1, rows, cin), weight=w, bias=draw(cout) * np.float32(1 if integers else 0.5),
                add=draw(1, rows, cin) if has_add else None, add_cols=cols, relu=relu,
                residual=draw(1, rows, cout) if has_res else None, dy=draw(1, rows, cout))


def lin_nan_case():
    """The ReLU case (192 -> 320, 65 rows, add on 128 columns) with a NaN bias in one column on each side of ``add_cols``: those output
    columns are NaN behind the ReLU and pass no gradient."""
    c = dict(lin_case((192, 320), 65, "relu"))
    bias = c["bias"].copy()
    bias[NAN_COLUMNS] = np.nan
    c["bias"] = bias
    return c


def lin_refs_of(c, out=None):
    """``out``: the forward's result whose sign is the ReLU's mask (the device's, so that a logit within an ulp of zero cannot tip one
    reference); None: each reference uses its own."""
    kw = dict(relu=c["relu"], add_cols=c["add_cols"], residual=c["residual"] is not None, out=out)
    r32 = gh.linear_bwd_host(c["x"], c["weight"], c["dy"], c["bias"], c["add"], **kw)
    r64 = gh.linear_bwd_host(f64(c["x"]), f64(c["weight"]), f64(c["dy"]), f64(c["bias"]), f64(c["add"]), **kw)
    return r32, r64


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
LN_WIDTHS = (64, 256, 512)
LN_MODES = ("single", "dy", "dy2", "both")             # one norm; two norms with only the first result used, only the second, both
LN_CASES = list(itertools.product(LN_WIDTHS, ROWS, LN_MODES))


@functools.lru_cache(maxsize=None)
def ln_case(C, rows, mode):
    """x ~ N(0, 1) + 0.3 (rows far from zero variance), weights in [0.5, 1.5], biases N(0, 0.25)."""
    rng = np.random.default_rng(C * 1009 + rows * 7 + LN_MODES.index(mode))
    shape = (1, rows, C)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    u = lambda: rng.uniform(0.5, 1.5, C).astype(np.float32)      # noqa: E731
    two = mode != "single"
    return dict(x=n(*shape) + np.float32(0.3), ln=(u(), n(C) * np.float32(0.5)), ln2=(u(), n(C) * np.float32(0.5)) if two else None,
                dy=n(*shape) if mode in ("single", "dy", "both") else None, dy2=n(*shape) if mode in ("dy2", "both") else None)


def ln_names(mode):
    return ("dx", "dweight", "dbias") + (("dweight2", "dbias2") if mode != "single" else ())


@functools.lru_cache(maxsize=None)
def ln_refs(C, rows, mode):
    c = ln_case(C, rows, mode)
    r32 = gh.layer_norm_bwd_host(c["x"], c["ln"], c["dy"], c["ln2"], c["dy2"], EPS)
    to64 = lambda p: None if p is None else (f64(p[0]), f64(p[1]))      # noqa: E731
    r64 = gh.layer_norm_bwd_host(f64(c["x"]), to64(c["ln"]), f64(c["dy"]), to64(c["ln2"]), f64(c["dy2"]), EPS)
    return r32, r64


# ------------------------------------------------------------------------------------------------------------------ a layer body
BODY = dict(C=64, H=2, B=2, K=65, seed=31)
BODY_LEAVES = ("query", "pos", "w_qkv", "b_qkv", "w_o", "b_o", "ln_w", "ln_b")


@functools.lru_cache(maxsize=None)
def body_case():
    """The self-attention third of a decoder layer: ``qkv = linear(query, add=pos, add_cols=2C)``, ``attention`` on its three column
    ranges, ``linear_add_ln(.., residual=query)``; G: the gradient of the result."""
    rng = np.random.default_rng(BODY["seed"])
    C, B, K = BODY["C"], BODY["B"], BODY["K"]
    n = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    return dict(query=n(B, K, C), pos=n(B, K, C) * np.float32(0.5), w_qkv=n(3 * C, C) / np.float32(np.sqrt(C)), b_qkv=n(3 * C) * np.float32(0.1),
                w_o=n(C, C) / np.float32(np.sqrt(C)), b_o=n(C) * np.float32(0.1), ln_w=rng.uniform(0.5, 1.5, C).astype(np.float32),
                ln_b=n(C) * np.float32(0.5), G=n(B, K, C))


def body_torch(leaves, H):
    """The same chain in plain torch on ``leaves`` (a dict of tensors of one dtype)."""
    C = leaves["query"].shape[-1]
    hd = C // H
    q_in = leaves["query"] + leaves["pos"]
    w, b = leaves["w_qkv"], leaves["b_qkv"]
    qk = q_in @ w[:2 * C].T + b[:2 * C]
    v = leaves["query"] @ w[2 * C:].T + b[2 * C:]
    B, K = q_in.shape[:2]
    heads = lambda t: t.reshape(B, K, H, hd).transpose(1, 2)      # noqa: E731
    q, k, v = heads(qk[..., :C]), heads(qk[..., C:]), heads(v)
    p = torch.softmax((q / hd ** 0.5) @ k.transpose(2, 3), dim=-1)
    o = (p @ v).transpose(1, 2).reshape(B, K, C)
    y = o @ leaves["w_o"].T + leaves["b_o"] + leaves["query"]
    return torch.nn.functional.layer_norm(y, (C,), leaves["ln_w"], leaves["ln_b"], EPS)


@functools.lru_cache(maxsize=None)
def body_refs():
    """The gradients of every leaf by torch autograd on the CPU, ``(float32, float64)``."""
    c = body_case()
    out = []
    for dt in (torch.float32, torch.float64):
        leaves = {k: torch.from_numpy(c[k]).to(dt).requires_grad_() for k in BODY_LEAVES}
        (body_torch(leaves, BODY["H"]) * torch.from_numpy(c["G"]).to(dt)).sum().backward()
        out.append({k: v.grad.numpy() for k, v in leaves.items()})
    return tuple(out)
