"""What tests/test_gpu_text_encoder_edges.py and tests/test_text_encoder_ops_host.py share: the case tables, the seeded operands of every
``ptx_txt_*`` entry point, the masks of the attention cases, the slice plan of ``ptx_txt_linear`` restated, float32 restatements of the
five operators in the kernels' manner (the correct ones and deliberately wrong ones), and one thin device call per entry point with
its guard zones.  A plain module: no tests, no marks.

Operands are drawn in float64 and rounded to float32 once, so numpy in either precision and the device start from the same values.

Guard zones: every device output is the first ``n`` rows of an allocation with ``GUARD`` more rows behind it filled with ``OUT_FILL``;
every operand that must not be read behind its end has ``GUARD`` rows of NaN behind it; ``stats`` is ``(n, 2)`` inside ``(n + 16, 2)``;
the sliced workspace is ``ptx_txt_linear_workspace_bytes`` exactly inside a longer tensor.  After each call the zones must have kept
their bits (``Guarded.read``).  All of it lies inside allocations the test owns."""
import numpy as np
import torch

from proxytransformation_amd import _abi
from tests.text_encoder_util import EPS

GUARD, STATS_GUARD, WS_GUARD, OUT_FILL = 64, 16, 1024, 7.0
DEV = "cuda:0"

# ---------------------------------------------------------------------------------------------------------------------- the case tables
LN_WIDTHS = (64, 192, 768, 1280)
LN_ROWS = (1, 15, 16, 17, 65)                              # 16 rows per work-group
LN_KINDS = ("offset", "zero")                              # rows 30 + N(0, 1) and N(0, 1)

#: (Cin, Cout, act) of ptx_txt_ln_linear
LNL_SHAPES = [(64, 64, 0), (1280, 64, 0), (64, 5120, 0), (128, 320, 1), (1280, 5120, 1)]
LNL_OFFSET = {(64, 64, 0), (128, 320, 1)}                  # the shapes that also run on rows 30 + N(0, 1): one per act


def lnl_rows(cout):
    """Rows of a ptx_txt_ln_linear case: 1 and 65 only at the two widest shapes."""
    return (1, 65) if cout == 5120 else (1, 63, 64, 65, 129)


LIN_CIN = (64, 768, 832, 1536, 1600, 5120)
LIN_ROWS = (1, 64, 65, 129)
LIN_SHAPES = [(cin, cout) for cin in LIN_CIN for cout in (64, 192)] + [(64, 5120)]
SLICE_PATTERNS = {832: [7, 6], 1536: [12, 12], 1600: [9, 9, 7], 5120: [12] * 6 + [8], 2112: [11] * 3, 3072: [12] * 4}

#: (B, T, H) of ptx_txt_attention
ATT_SHAPES = [(1, 1, 1), (2, 15, 2), (2, 16, 2), (2, 17, 2), (1, 64, 1), (1, 65, 1), (1, 255, 1), (2, 256, 1), (64, 17, 1), (1, 20, 20)]
ATT_LARGE = [(2, 17, 2), (1, 65, 1), (2, 256, 1)]          # the shapes that also run with q and k scaled by 8
POISON_T, POISON_AT = 80, (15, 16, 63, 64, 65)

#: (B, T, C, vocab, positions) of ptx_txt_embed
EMBED_SHAPES = [(2, 256, 64, 97, 256), (64, 3, 64, 97, 77), (2, 5, 1280, 97, 77)]
BAD_IDS = (97, -1, 2 ** 40)


def _rng(*key):
    return np.random.default_rng([2025] + [int(k) for k in key])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------- operands
def ln_operands(C, n, kind, draw=0):
    """``(x, weight, bias)``: rows ``30 + N(0, 1)`` ('offset') or ``N(0, 1)`` ('zero'); weight ``1 + N(0, 0.1^2)``, bias ``N(0, 0.1^2)``."""
    rng = _rng(1, C, n, LN_KINDS.index(kind), draw)
    x = rng.standard_normal((n, C)) + (30.0 if kind == "offset" else 0.0)
    return _f32(x), _f32(1.0 + 0.1 * rng.standard_normal(C)), _f32(0.1 * rng.standard_normal(C))


def lnl_operands(cin, cout, act, n, kind="zero", draw=0):
    """``(x, ln_w, ln_b, w, bias)``.  With the quick-GELU the weight's deviation is ``3 / sqrt(Cin)``, so fc1 ~ N(0, 3^2) and both
    tails of the activation occur (values below -6 and above +6); without it ``1 / sqrt(Cin)``."""
    rng = _rng(2, cin, cout, act, n, LN_KINDS.index(kind), draw)
    x = rng.standard_normal((n, cin)) + (30.0 if kind == "offset" else 0.0)
    w = rng.standard_normal((cout, cin)) * ((3.0 if act else 1.0) / np.sqrt(cin))
    return (_f32(x), _f32(1.0 + 0.1 * rng.standard_normal(cin)), _f32(0.1 * rng.standard_normal(cin)), _f32(w),
            _f32(0.5 * rng.standard_normal(cout)))


def lin_operands(cin, cout, n):
    """``(x, w, bias, residual)``: x, residual ~ N(0, 1), w ~ N(0, 1 / Cin), bias ~ N(0, 0.5^2)."""
    rng = _rng(3, cin, cout, n)
    return (_f32(rng.standard_normal((n, cin))), _f32(rng.standard_normal((cout, cin)) / np.sqrt(cin)),
            _f32(0.5 * rng.standard_normal(cout)), _f32(rng.standard_normal((n, cout))))


def att_operands(B, T, H, large=False):
    """``qkv (B,T,3 C)`` ~ N(0, 1): logits ~ N(0, 1).  ``large``: q and k times 8, logits ~ N(0, 64^2), |logit| up to about 290."""
    qkv = _rng(4, B, T, H).standard_normal((B, T, 3 * 64 * H))
    if large:
        qkv[..., :2 * 64 * H] *= 8.0
    return _f32(qkv)


def att_masks(B, T):
    """``{name: (B,T) bool or None}`` of a shape: no mask; a random one with ``mask[:, 0]`` true; at T = 256 key tile 64 .. 127 empty
    in text 0; from T = 15 on the first true key at 5, so queries 0 .. 4 admit no key (the zeros rule)."""
    rng = _rng(5, B, T)
    rnd = rng.random((B, T)) < 0.6
    rnd[:, 0] = True
    out = {"none": None, "random": rnd}
    if T == 256:
        m = rng.random((B, T)) < 0.8
        m[:, 0] = True
        m[0, 64:128] = False
        out["tile"] = m
    if T >= 15:
        m = rng.random((B, T)) < 0.7
        m[:, :5], m[:, 5] = False, True
        out["late"] = m
    return out


def embed_operands(B, T, C, vocab, positions):
    """``(ids, token table, position table)``; ids 0 and ``vocab - 1`` occur."""
    rng = _rng(6, B, T, C)
    ids = rng.integers(0, vocab, size=(B, T), dtype=np.int64)
    ids[0, 0], ids[-1, -1] = 0, vocab - 1
    if T > 1:
        ids[0, 1], ids[-1, 0] = vocab - 1, 0
    return ids, _f32(0.5 * rng.standard_normal((vocab, C))), _f32(0.1 * rng.standard_normal((positions, C)))


# ---------------------------------------------------------------------------------------------------------------------- the slice plan
def slice_plan(cin):
    """The 64-channel steps of every slice of a contraction over ``cin`` channels, as csrc/text_encoder.hip cuts it:
    ``ceil(Cin / 768)`` slices of ``ceil(steps / slices)`` steps, the last one what is left."""
    steps = cin // 64
    slices = -(-cin // 768)
    each = -(-steps // slices)
    return [min(each, steps - z * each) for z in range(slices)]


# ---------------------------------------------------------------------------------------------------------------------- float32 restatements
def _sum16(s):
    """(n, 16) -> (n,): xor 8, 4, 2, 1 as every lane sees it."""
    for step in (8, 4, 2, 1):
        s = s + s[:, np.arange(16) ^ step]
    return s[:, 0]


def stats32(x, eps, centred=True):
    """``(mean, rstd)`` in float32 in the kernel's manner: lane l adds channels ``64 m + 4 l .. + 3`` for ascending m, then ``_sum16``.
    ``centred=False`` is the WRONG formula ``E[x^2] - E[x]^2``."""
    n, C = x.shape
    f = np.float32
    lanes = x.reshape(n, C // 64, 16, 4)
    s = np.zeros((n, 16), f)
    for m in range(C // 64):
        for j in range(4):
            s = s + lanes[:, m, :, j]
    mean = _sum16(s) / f(C)
    ss = np.zeros((n, 16), f)
    for m in range(C // 64):
        for j in range(4):
            d = lanes[:, m, :, j] - mean[:, None] if centred else lanes[:, m, :, j]
            ss = ss + d * d
    var = _sum16(ss) / f(C)
    if not centred:
        var = var - mean * mean
    return mean, f(1.0) / np.sqrt(var + f(eps))


def ln32(x, w, b, eps, centred=True):
    mean, rstd = stats32(x, eps, centred)
    return (x - mean[:, None]) * rstd[:, None] * w + b


def sums32(x, w, drop_last_step=False):
    """``x @ w^T`` in float32: every slice of ``slice_plan`` ascending in k from zero, then the slices added in ascending order.
    ``drop_last_step`` is WRONG: the last slice stops one 64-channel step early."""
    plan = slice_plan(x.shape[1])
    total, k0 = None, 0
    for z, steps in enumerate(plan):
        acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
        stop = k0 + 64 * (steps - 1 if drop_last_step and z == len(plan) - 1 else steps)
        for k in range(k0, stop):
            acc = acc + x[:, k:k + 1] * w[None, :, k]
        total = acc if total is None else total + acc
        k0 += 64 * steps
    return total


def linear32(x, w, bias, residual, drop_last_step=False):
    v = sums32(x, w, drop_last_step)
    if bias is not None:
        v = v + bias
    return v if residual is None else v + residual


def ln_linear32(x, ln_w, ln_b, eps, w, bias, act, centred=True, slope=1.702):
    v = sums32(ln32(x, ln_w, ln_b, eps, centred), w)
    if bias is not None:
        v = v + bias
    return v / (np.float32(1.0) + np.exp(np.float32(-slope) * v)) if act else v


def attention32(qkv, mask, H, admit=0, use_max=True):
    """The attention in float32 over whole score matrices.  ``admit=1`` is WRONG (key t + 1 is admitted); ``use_max=False`` is WRONG
    (``exp(s)`` without the row maximum)."""
    f = np.float32
    B, T, C3 = qkv.shape
    C = C3 // 3
    q = (qkv[..., :C] * f(0.125)).reshape(B, T, H, 64).transpose(0, 2, 1, 3)
    k = qkv[..., C:2 * C].reshape(B, T, H, 64).transpose(0, 2, 1, 3)
    v = qkv[..., 2 * C:].reshape(B, T, H, 64).transpose(0, 2, 1, 3)
    valid = np.ones((B, T), bool) if mask is None else np.asarray(mask, bool)
    adm = (np.arange(T)[None, :] <= np.arange(T)[:, None] + admit)[None, None] & valid[:, None, None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.where(adm, q @ k.transpose(0, 1, 3, 2), f(-np.inf))
        m = s.max(-1, keepdims=True)
        p = np.where(adm, np.exp(s - np.where(np.isfinite(m), m, f(0.0))) if use_max else np.exp(s), f(0.0)).astype(f)
        total = p.sum(-1, keepdims=True, dtype=f)
        out = np.where(total == 0, f(0.0), (p @ v) / np.where(total == 0, f(1.0), total))
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3).reshape(B, T, C).astype(f))


# ---------------------------------------------------------------------------------------------------------------------- the rule
def held(name, got, ref32, ref64, rule):
    """``rule`` (``sparse_util.hold``) on a finite result."""
    assert np.isfinite(got).all() and np.isfinite(ref64).all(), name
    rule(name, got, ref32, ref64)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------- the device calls
class Guarded:
    """``rows`` rows of ``width`` floats with ``guard`` rows of ``fill`` behind them in one allocation."""

    def __init__(self, rows, width, fill, guard=GUARD, data=None):
        self.rows = rows
        self.full = torch.full((rows + guard, width), float(fill), dtype=torch.float32, device=DEV)
        self.view = self.full[:rows]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32).reshape(rows, width)))
        self.tail = self.full[rows:].cpu().numpy().copy()

    def ptr(self):
        return self.view.data_ptr()

    def read(self):
        """The rows as an array, after checking that the rows behind them kept their bits."""
        full = self.full.cpu().numpy()
        assert np.array_equal(full[self.rows:].view(np.uint32), self.tail.view(np.uint32)), "the guard rows behind the end were written"
        return full[:self.rows].copy()


def operand(a):
    """A float operand ``(rows, width)`` on the device with NaN rows behind its end."""
    a = np.asarray(a, np.float32)
    assert a.ndim == 2
    return Guarded(a.shape[0], a.shape[1], np.nan, data=a)


def vector(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def ln(x, w, b, eps=EPS):
    """``ptx_txt_ln`` on arrays: ``(n, C)``."""
    n, C = x.shape
    gx, gw, gb, out = operand(x), vector(w), vector(b), Guarded(n, C, OUT_FILL)
    _abi.check(_abi.lib().ptx_txt_ln(_p(gx), n, C, _p(gw), _p(gb), eps, _p(out), _st()), "ptx_txt_ln")
    return out.read()


def ln_linear(x, ln_w, ln_b, w, bias, act, eps=EPS):
    """``ptx_txt_ln_linear`` on arrays: ``(out (n, Cout), stats (n, 2))``."""
    n, cin = x.shape
    cout = w.shape[0]
    gx, out, stats = operand(x), Guarded(n, cout, OUT_FILL), Guarded(n, 2, OUT_FILL, guard=STATS_GUARD)
    ops = [vector(a) for a in (ln_w, ln_b, w, bias)]
    _abi.check(_abi.lib().ptx_txt_ln_linear(_p(gx), n, _p(ops[0]), _p(ops[1]), eps, _p(ops[2]), _p(ops[3]), cin, cout, act, _p(out),
                                            _p(stats), _st()), "ptx_txt_ln_linear")
    return out.read(), stats.read()


def linear(x, w, bias, residual, in_place=False):
    """``ptx_txt_linear`` on arrays.  ``in_place``: ``out`` starts as the residual and is handed in as both (as the module calls it);
    otherwise ``out`` starts as NaN in its rows and the residual is another tensor.  The workspace is exactly
    ``ptx_txt_linear_workspace_bytes`` at the head of a longer tensor."""
    n, cin = x.shape
    cout = w.shape[0]
    lib = _abi.lib()
    gx, gw, gb = operand(x), vector(w), vector(bias)
    if in_place:
        out = Guarded(n, cout, OUT_FILL, data=residual)
        res = out
    else:
        out = Guarded(n, cout, OUT_FILL, data=np.full((n, cout), np.nan, np.float32))
        res = None if residual is None else operand(residual)
    nbytes = int(lib.ptx_txt_linear_workspace_bytes(n, cin, cout))
    assert nbytes == (4 * len(slice_plan(cin)) * n * cout if cin > 768 else 0)
    ws = Guarded(1, nbytes // 4 + WS_GUARD, OUT_FILL, guard=0) if nbytes else None
    _abi.check(lib.ptx_txt_linear(_p(gx), n, _p(gw), _p(gb), cin, cout, _p(res), _p(out), _p(ws), nbytes, _st()), "ptx_txt_linear")
    if ws is not None:
        assert bool((ws.full[0, nbytes // 4:] == OUT_FILL).all()), "the workspace was written behind ptx_txt_linear_workspace_bytes"
    return out.read()


def attention(qkv, mask, H):
    """``ptx_txt_attention`` on arrays: ``(B, T, C)``.  ``mask``: None, bool, or uint8 (any nonzero value is a token)."""
    B, T, C3 = qkv.shape
    g, out = operand(qkv.reshape(B * T, C3)), Guarded(B * T, C3 // 3, OUT_FILL)
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    assert m is None or m.element_size() == 1
    _abi.check(_abi.lib().ptx_txt_attention(_p(g), _p(m), B, T, H, _p(out), _st()), "ptx_txt_attention")
    return out.read().reshape(B, T, C3 // 3)


def embed(ids, tok, pos, vocab=None):
    """``ptx_txt_embed`` on arrays: ``(B, T, C)``.  Both tables have NaN rows behind their end; ``vocab`` defaults to the table's rows."""
    B, T = ids.shape
    C = tok.shape[1]
    gt, gp, out = operand(tok), operand(pos), Guarded(B * T, C, OUT_FILL)
    gi = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(DEV)
    _abi.check(_abi.lib().ptx_txt_embed(_p(gi), B, T, _p(gt), _p(gp), tok.shape[0] if vocab is None else vocab, pos.shape[0], C, _p(out),
                                        _st()), "ptx_txt_embed")
    return out.read().reshape(B, T, C)
