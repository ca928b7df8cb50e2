"""The train-mode operators (ptx_op_* of csrc/train_ops.hip) called through the C ABI, one regime per case, against float64.

Rules of comparison (none of them measured):
  * products and sums of small integers (|v| <= 8, alpha / scale a power of two): every partial sum is exact in fp32 in any order,
    the result is compared BIT FOR BIT -- all gemm routing and edge cases, colsum, eltwise 0 1 4 5 6 7 8, gathers, scatters, pooling;
  * gemm on random floats: |got - ref| <= |alpha| (Kc + 8) u (|A||B|) + u |ref| componentwise, u = 2^-24, Kc = min(256, slice) for
    k_bgemm (256 k in fp32, chunks summed in double), Kc = K for the thin kernels; the worst err / bound ratio is printed;
  * colsum on random floats: float32(ref) or its neighbour (the sum is formed in double and rounded once);
  * transcendental operators: the rule and the bars of tests/test_gpu_train.py (max err / rms: 1e-5 values, 2e-5 LayerNorm
    gradients, 5e-5 BatchNorm gradients).
Every output is a NaN-filled buffer with guard words in front, behind and in the gaps of a strided result (train_ops_util.Out)."""
import numpy as np
import pytest
import torch

from tests import train_ops_util as U
from tests.train_ops_util import Gemm, Out, dv, ints, op, refused, rel, same_bits

pytestmark = pytest.mark.gpu

BGEMM, THIN_SCALAR, THIN_VEC, THIN_ROW = 0, 1, 2, 3


# ================================================================================================ ptx_op_gemm
def dense(M, N, K, ta=False, tb=False, batch=1, inner=1, **kw):
    """Contiguous operands: A stored (M,K) or, ta, (K,M); B stored (K,N) or, tb, (N,K); C (M,N); batches back to back."""
    d = dict(a=(1, M) if ta else (K, 1), b=(1, K) if tb else (N, 1), c=(N, 1), batch=batch, inner=inner,
             a_bs=(inner * M * K, M * K), b_bs=(inner * K * N, K * N), c_bs=(inner * M * N, M * N))
    d.update(kw)
    return Gemm(M, N, K, **d)


def run_exact(g, seed, what, want_route=None, a_ptr=None, b_ptr=None, operands=None):
    rng = np.random.default_rng(seed)
    na, nb = g.sizes()
    Af, Bf = operands if operands is not None else (ints(rng, na), ints(rng, nb))
    c_old = ints(rng, g.c_index().shape) if g.accumulate else None
    got, route = g.run(Af, Bf, c_old, a_ptr=a_ptr, b_ptr=b_ptr)
    if want_route is not None:
        assert route == want_route, f"{what}: route {route}, wanted {want_route}"
    ref, _ = g.reference(Af, Bf, c_old)
    same_bits(got, ref, what)
    return got, (Af, Bf)


def run_float(g, Af, Bf, Kc, what, want_route, c_old=None):
    got, route = g.run(Af, Bf, c_old)
    assert route == want_route, f"{what}: route {route}, wanted {want_route}"
    prod, mag = Gemm.reference(g.but(accumulate=0), np.asarray(Af, np.float32), np.asarray(Bf, np.float32))
    ref = prod if c_old is None else prod + c_old
    bound = U.gemm_bound(prod, mag, Kc) + (0 if c_old is None else U.U * (np.abs(c_old) + np.abs(ref)))
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"GEMM-RATIO {what}: worst err / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: err / bound = {ratio:.3f}"
    return ratio


PAIRS = [(1, 1), (63, 65), (64, 64), (65, 63), (130, 1), (1, 130), (130, 65)]
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]        # NN NT TN TT
KS = [1, 31, 32, 33, 96, 255, 256, 257, 513]


@pytest.mark.parametrize("K", KS)
def test_bgemm_shapes_and_layouts(K):
    """M, N around the 64 x 64 tile, K around the 32-k step (96 = three steps: the step on zeros; 255 .. 257: the flush into the
    double accumulators after 8 steps); the pairs rotate through NN / NT / TN / TT so that every K meets all four staging maps."""
    for i, (M, N) in enumerate(PAIRS):
        ta, tb = LAYOUTS[(i + KS.index(K)) % 4]
        run_exact(dense(M, N, K, ta, tb, alpha=(-2.0 if i % 2 else 0.5)), 100 * K + i, f"M{M} N{N} K{K} ta{ta} tb{tb}", BGEMM)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_bgemm_all_four_staging_maps(ta, tb):
    for M, N, K in ((65, 63, 96), (130, 130, 257)):
        run_exact(dense(M, N, K, ta, tb, batch=3), 7, f"M{M} N{N} K{K} ta{ta} tb{tb}", BGEMM)


def test_bgemm_strided_views():
    # no unit stride in either operand
    run_exact(Gemm(65, 63, 33, a=(70, 2), b=(130, 2), c=(63, 1)), 1, "no unit stride", BGEMM)
    # the head-split views of _ProxyAttnCore: qkv (B n, 3C) rows, a column block of one head, batch = B heads, inner = heads
    B, heads, hd, n, L = 2, 4, 8, 37, 5
    C, Z = heads * hd, B * heads
    zb = dict(batch=Z, inner=heads)
    # S1 = scale Pt . K^T: B operand = columns C .. 2C of qkv (the offset is the slice handed over), transposed
    g = Gemm(L, n, hd, a=(C, 1), b=(1, 3 * C), c=(n, 1), a_bs=(L * C, hd), b_bs=(n * 3 * C, hd), c_bs=(heads * L * n, L * n), alpha=0.25, **zb)
    run_exact(g, 2, "S1 head-split", BGEMM)
    # PV = D1 V: B = columns 2C .. 3C, row stride 3C
    g = Gemm(L, hd, n, a=(n, 1), b=(3 * C, 1), c=(hd, 1), a_bs=(heads * L * n, L * n), b_bs=(n * 3 * C, hd), c_bs=(heads * L * hd, L * hd), **zb)
    run_exact(g, 3, "PV head-split", BGEMM)
    # dV written into columns 2C .. 3C of dqkv: C with row stride 3C at offset 2C; the other columns are guard words
    g = Gemm(n, hd, L, a=(1, n), b=(hd, 1), c=(3 * C, 1), a_bs=(heads * L * n, L * n), b_bs=(heads * L * hd, L * hd), c_bs=(n * 3 * C, hd),
             c_off=2 * C, **zb)
    run_exact(g, 4, "dV into a column block", BGEMM)
    # dPt accumulated: onto a non-trivial C
    g = Gemm(L, hd, n, a=(n, 1), b=(3 * C, 1), c=(C, 1), a_bs=(heads * L * n, L * n), b_bs=(n * 3 * C, hd), c_bs=(L * C, hd), alpha=-0.5,
             accumulate=1, **zb)
    run_exact(g, 5, "dPt accumulate", BGEMM)
    # stride-0 operands: one row for every m, one matrix for every batch
    run_exact(Gemm(65, 33, 40, a=(0, 1), b=(33, 1), c=(33, 1), batch=3, a_bs=(40, 0), b_bs=(0, 0), c_bs=(65 * 33, 0)), 6, "broadcast", BGEMM)
    run_exact(Gemm(5, 7, 1, a=(0, 0), b=(0, 1), c=(7, 1)), 7, "all broadcast", BGEMM)
    # C with row gaps, a transposed C, both with batches
    run_exact(dense(65, 63, 33, batch=2, c=(70, 1), c_bs=(65 * 70 + 3, 0)), 8, "C row gaps", BGEMM)
    run_exact(dense(65, 63, 33, batch=2, c=(1, 68), c_bs=(63 * 68 + 1, 0), accumulate=1), 9, "C transposed", BGEMM)


@pytest.mark.parametrize("K", [33, 64, 100, 1000])
@pytest.mark.parametrize("ksplit", [2, 3, 7])
def test_bgemm_k_slices(K, ksplit):
    """Every slice holds the product over its own k range (whole 32-k steps by the restated rule; K = 33 in three slices: one partial,
    one EMPTY, written as zeros over the NaN fill), and the slices sum to the full product."""
    M, N = 33, 65
    g = dense(M, N, K, ta=True, batch=2, ksplit=ksplit, c_sk=2 * M * N + 7, c_bs=(M * N, 0), alpha=-2.0)
    got, (Af, Bf) = run_exact(g, K + ksplit, f"K{K} ksplit{ksplit}", BGEMM)
    full, _ = dense(M, N, K, ta=True, batch=2, alpha=-2.0).reference(Af, Bf)
    same_bits(got.astype(np.float64).sum(1, keepdims=True).astype(np.float32), full, "sum of the slices")
    if (K, ksplit) == (33, 3):
        assert g.slices() == [(0, 32), (32, 33), (33, 33)] and not got[:, 2].any() and got[:, 1].any()


@pytest.mark.parametrize("dtype", [1, 2], ids=["bf16", "fp16"])
def test_bgemm_16bit_operands(dtype):
    nimg, Cin, hw, C = 2, 40, 225, 64
    # _ImgTokens: A = img (nimg, Cin, hw) channels-first in its storage type (rows 2-byte aligned: hw is odd), C = rows 1.. of tok
    g = Gemm(hw, C, Cin, a=(1, hw), b=(1, Cin), c=(C, 1), batch=nimg, a_bs=(Cin * hw, 0), b_bs=(0, 0), c_bs=((hw + 1) * C, 0), c_off=C,
             a_dtype=dtype)
    run_exact(g, 11, "img tokens", BGEMM)
    # dWc: B = img, contracted over the pixels
    g = Gemm(C, Cin, hw, a=(1, C), b=(1, hw), c=(Cin, 1), batch=nimg, a_bs=((hw + 1) * C, 0), b_bs=(Cin * hw, 0), c_bs=(C * Cin, 0),
             b_dtype=dtype)
    run_exact(g, 12, "dWc", BGEMM)


def test_bgemm_random_floats():
    rng = np.random.default_rng(5)
    # K = 4113: 16 flushes and a tail; same-sign operands, so nothing cancels and |A||B| = |ref|
    g = dense(65, 33, 4113)
    na, nb = g.sizes()
    run_float(g, rng.uniform(0.5, 1.5, na), rng.uniform(0.5, 1.5, nb), 256, "bgemm K4113 same sign", BGEMM)
    g = dense(70, 130, 513, tb=True, alpha=-0.37)
    na, nb = g.sizes()
    run_float(g, rng.standard_normal(na), rng.standard_normal(nb), 256, "bgemm NT K513", BGEMM)
    g = dense(33, 65, 1000, ta=True, ksplit=3, c_sk=33 * 65)
    na, nb = g.sizes()
    run_float(g, rng.standard_normal(na), rng.standard_normal(nb), 256, "bgemm TN K1000 ksplit3", BGEMM)
    g = dense(64, 64, 96, accumulate=1, alpha=1.5)
    na, nb = g.sizes()
    run_float(g, rng.standard_normal(na), rng.standard_normal(nb), 96, "bgemm accumulate", BGEMM,
              c_old=rng.standard_normal(g.c_index().shape).astype(np.float32).astype(np.float64))


# ---- k_bthin_out
def thin_out(M, N, K, batch, **kw):
    """Both operands contiguous along k: A stored (batch, M, K), B stored (batch, N, K).  batch 96 = 12 x 8 with its own stride per digit."""
    inner = 8 if batch == 96 else 1
    return dense(M, N, K, tb=True, batch=batch, inner=inner, **kw)


THIN_SHAPES = [(1, 226), (2, 226), (226, 1), (226, 2)]


@pytest.mark.parametrize("batch", [64, 96])
@pytest.mark.parametrize("K", [4, 20, 32, 36, 64])
def test_bthin_out_vector(K, batch):
    """K % 16 != 0 (4, 20, 36) runs the clamped tail: requests past K re-read the last four k with weight 0."""
    for i, (M, N) in enumerate(THIN_SHAPES):
        run_exact(thin_out(M, N, K, batch), K + i, f"vec M{M} N{N} K{K} z{batch}", THIN_VEC)


@pytest.mark.parametrize("batch", [64, 96])
@pytest.mark.parametrize("K", [1, 2, 3, 7, 9, 17, 63])
def test_bthin_out_scalar(K, batch):
    for i, (M, N) in enumerate(THIN_SHAPES):
        run_exact(thin_out(M, N, K, batch), K + i, f"scalar M{M} N{N} K{K} z{batch}", THIN_SCALAR)


@pytest.mark.parametrize("batch", [64, 96])
def test_bthin_out_outer_products_and_layouts(batch):
    inner = 8 if batch == 96 else 1
    zb = dict(batch=batch, inner=inner)
    # the outer products of the attention pool's backward: K = 1 with stride-0 "rows", K = 2 with A stored k-major
    run_exact(Gemm(226, 32, 1, a=(1, 0), b=(0, 1), c=(256, 1), a_bs=(inner * 226, 226), b_bs=(256, 32), c_bs=(226 * 256, 32), **zb), 1,
              "outer K1 into head columns", THIN_SCALAR)
    run_exact(Gemm(226, 32, 2, a=(1, 226), b=(32, 1), c=(32, 1), a_bs=(inner * 452, 452), b_bs=(inner * 64, 64),
                   c_bs=(inner * 226 * 32, 226 * 32), **zb), 2, "outer K2", THIN_SCALAR)
    # column-major C (c_rs == 1): the thread -> element map follows m
    for M, N, K, want in ((226, 2, 8, THIN_VEC), (2, 226, 8, THIN_VEC), (226, 2, 7, THIN_SCALAR), (2, 226, 1, THIN_SCALAR)):
        run_exact(thin_out(M, N, K, batch, c=(1, M)), 3 + K, f"column-major C M{M} N{N} K{K}", want)
        run_exact(thin_out(M, N, K, batch, c=(1, M + 3), c_bs=(inner * N * (M + 3), N * (M + 3))), 4 + K, f"column-major C with gaps M{M} N{N} K{K}", want)
    # accumulate and alpha on both forms
    run_exact(thin_out(2, 226, 36, batch, alpha=-0.25, accumulate=1), 5, "vec accumulate", THIN_VEC)
    run_exact(thin_out(226, 2, 17, batch, alpha=4.0, accumulate=1), 6, "scalar accumulate", THIN_SCALAR)
    # the query-0 products as the training step issues them (stride-0 A rows, B = a head's columns of (T, 256) keys)
    g = Gemm(1, 226, 32, a=(0, 1), b=(1, 256), c=(226, 1), a_bs=(256, 32) if inner == 8 else (32, 0),
             b_bs=(226 * 256, 32) if inner == 8 else (226 * 32, 0), c_bs=(inner * 226, 226), alpha=0.125, **zb)
    if inner == 1:
        g.b = (1, 32)
    run_exact(g, 7, "S of the attention pool", THIN_VEC)


@pytest.mark.parametrize("K", [20, 32])
def test_bthin_out_shifted_base_takes_the_scalar_route(K):
    """The same operands from a base pointer one float off a 16-byte boundary: route 1, the same bits."""
    g = thin_out(2, 226, K, 64)
    rng = np.random.default_rng(K)
    na, nb = g.sizes()
    Af, Bf = ints(rng, na), ints(rng, nb)
    got_vec, _ = run_exact(g, 0, "aligned", THIN_VEC, operands=(Af, Bf))
    keep_a, pa = U.shifted(Af)
    got_a, _ = run_exact(g, 0, "A shifted", THIN_SCALAR, a_ptr=pa, operands=(Af, Bf))
    keep_b, pb = U.shifted(Bf)
    got_b, _ = run_exact(g, 0, "B shifted", THIN_SCALAR, b_ptr=pb, operands=(Af, Bf))
    assert np.array_equal(got_vec.view(np.int32), got_a.view(np.int32)) and np.array_equal(got_vec.view(np.int32), got_b.view(np.int32))


# ---- k_bthin_row
def thin_row(M, K, batch, **kw):
    """A stored (batch, M, K); B = 32 columns of one head inside rows of 256 (b_s2 = 32), one (K, 256) matrix per outer batch digit."""
    d = dict(a=(K, 1), b=(256, 1), c=(32, 1), batch=batch, inner=8, a_bs=(8 * M * K, M * K), b_bs=(K * 256, 32), c_bs=(8 * M * 32, M * 32))
    d.update(kw)
    return Gemm(M, 32, K, **d)


@pytest.mark.parametrize("batch", [64, 96])
@pytest.mark.parametrize("K", [65, 128, 226, 255, 256])
def test_bthin_row(K, batch):
    for M in (1, 2):
        run_exact(thin_row(M, K, batch), K + M, f"row M{M} K{K} z{batch}", THIN_ROW)
    run_exact(thin_row(2, K, batch, alpha=-0.5, accumulate=1, c=(40, 1), c_bs=(8 * 2 * 40, 2 * 40)), K, f"row accumulate K{K}", THIN_ROW)


def test_thin_random_floats():
    rng = np.random.default_rng(9)
    for g, Kc, what, want in ((thin_row(2, 226, 64), 226, "row K226", THIN_ROW), (thin_out(2, 226, 36, 64), 36, "vec K36", THIN_VEC),
                              (thin_out(226, 2, 63, 64), 63, "scalar K63", THIN_SCALAR)):
        na, nb = g.sizes()
        run_float(g, rng.standard_normal(na), rng.standard_normal(nb), Kc, what, want)


# ================================================================================================ ptx_op_colsum
CS_N = [1, 3, 4, 63, 64, 65, 256, 260]
CS_R = [1, 3, 4, 5, 31, 1000]
CS_SPLIT = [1, 2, 16, 17, 512, 1024]


def colsum(x, y, mode, scale=1.0, nsplit=1, out_old=None, x_ptr=None, y_ptr=None):
    R, N = x.shape
    xt = None if x_ptr is not None else dv(x.astype(np.float32))
    yt = None if y is None or y_ptr is not None else dv(y.astype(np.float32))
    scratch = torch.full((nsplit * N,), float("nan"), dtype=torch.float64, device=U.dev())
    out = Out.dense(N, init=out_old)
    op("colsum", x_ptr if x_ptr is not None else xt, y_ptr if y_ptr is not None else yt, R, N, mode, float(scale),
       0 if out_old is None else 1, out, scratch, nsplit)
    return out.take()


@pytest.mark.parametrize("N", CS_N)
def test_colsum_exact(N):
    """Integers: bit for bit.  nsplit rotates through 1 .. 1024 (more splits than R / 4 row groups: splits without a row write zeros)."""
    rng = np.random.default_rng(N)
    for ir, R in enumerate(CS_R):
        x = ints(rng, (R, N))
        for mode in range(4):
            y = None if mode in (0, 2) else (ints(rng, (R, N)) if mode == 1 else ints(rng, N))
            nsplit = CS_SPLIT[(CS_N.index(N) + ir + mode) % 6]
            acc = (ir + mode) % 3 == 0
            old = ints(rng, N).astype(np.float32) if acc else None
            got = colsum(x, y, mode, scale=-0.5, nsplit=nsplit, out_old=old)
            ref = U.colsum_ref(x, y, mode, -0.5) + (0 if old is None else old.astype(np.float64))
            same_bits(got, ref, f"colsum N{N} R{R} mode{mode} nsplit{nsplit} acc{acc}")


@pytest.mark.parametrize("nsplit", CS_SPLIT)
def test_colsum_every_split_count(nsplit):
    rng = np.random.default_rng(nsplit)
    for R, N in ((1000, 64), (1000, 65), (5, 260), (31, 4)):
        x, y = ints(rng, (R, N)), ints(rng, (R, N))
        same_bits(colsum(x, y, 1, nsplit=nsplit), U.colsum_ref(x, y, 1, 1.0), f"colsum R{R} N{N} nsplit{nsplit}")


def test_colsum_misaligned_takes_the_scalar_route():
    rng = np.random.default_rng(3)
    for R, N in ((31, 64), (1000, 256), (5, 4)):
        x, y, yv = ints(rng, (R, N)), ints(rng, (R, N)), ints(rng, N)
        kx, px = U.shifted(x)
        ky, py = U.shifted(y)
        kv, pv = U.shifted(yv)
        same_bits(colsum(x, None, 0, x_ptr=px, nsplit=2), U.colsum_ref(x, None, 0, 1.0), "x shifted, mode 0")
        same_bits(colsum(x, y, 1, x_ptr=px, nsplit=2), U.colsum_ref(x, y, 1, 1.0), "x shifted, mode 1")
        same_bits(colsum(x, y, 1, y_ptr=py, nsplit=2), U.colsum_ref(x, y, 1, 1.0), "y shifted, mode 1")
        same_bits(colsum(x, yv, 3, x_ptr=px, nsplit=2), U.colsum_ref(x, yv, 3, 1.0), "x shifted, mode 3")
        same_bits(colsum(x, yv, 3, y_ptr=pv, nsplit=2), U.colsum_ref(x, yv, 3, 1.0), "mean shifted, mode 3 (vector route: y is read word by word)")


def test_colsum_random_floats_round_once():
    rng = np.random.default_rng(4)
    for R, N, nsplit in ((1000, 65, 16), (1000, 256, 17), (31, 260, 1)):
        x, y = rng.standard_normal((R, N)).astype(np.float32), rng.standard_normal((R, N)).astype(np.float32)
        for mode in (0, 1, 2):
            got = colsum(x, y, mode, scale=1.0 / R, nsplit=nsplit)
            r, lo, hi = U.neighbours32(U.colsum_ref(x, y, mode, np.float32(1.0 / R)))
            assert ((got == r) | (got == lo) | (got == hi)).all(), f"colsum floats R{R} N{N} mode{mode}"
    # the variance around the mean of columns that sit at 1e4: the centred sum, where E[x^2] - E[x]^2 has no digit left
    x = (1e4 + rng.standard_normal((1000, 65))).astype(np.float32)
    mean = x.astype(np.float64).mean(0).astype(np.float32)
    got = colsum(x, mean, 3, nsplit=16)
    r, lo, hi = U.neighbours32(U.colsum_ref(x, mean, 3, 1.0))
    assert ((got == r) | (got == lo) | (got == hi)).all() and (got > 800).all() and (got < 1200).all()


def test_colsum_refusals():
    x = dv(np.zeros((4, 4), np.float32))
    out, scratch = Out.dense(4), torch.zeros(64, dtype=torch.float64, device=U.dev())
    for mode in (1, 3):
        refused("colsum", x, None, 4, 4, mode, 1.0, 0, out, scratch, 1)
    refused("colsum", x, None, 4, 4, 4, 1.0, 0, out, scratch, 1)
    refused("colsum", x, None, 4, 4, 0, 1.0, 0, out, scratch, 1025)
    refused("colsum", x, None, 4, 4, 0, 1.0, 0, out, scratch, 0)
    out.take()


# ================================================================================================ ptx_op_eltwise / ptx_op_dropout
def eltwise(opn, a, b=None, s=0.0, ncol=0):
    out = Out.dense(a.size)
    op("eltwise", opn, dv(a.astype(np.float32)), None if b is None else dv(b.astype(np.float32)), float(s), a.size, ncol, out)
    return out.take()


@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_eltwise_all_ops(n):
    rng = np.random.default_rng(n)
    a, b = ints(rng, n), ints(rng, n)
    for opn in (0, 1, 4, 5, 7, 8):
        same_bits(eltwise(opn, a, b, s=-0.5), U.eltwise_ref(opn, a, b, -0.5, 1), f"eltwise op {opn} n {n}")
    for ncol in (1, 3, 256):
        bias = ints(rng, ncol)
        same_bits(eltwise(6, a, bias, ncol=ncol), U.eltwise_ref(6, a, bias, 0.0, ncol), f"eltwise op 6 ncol {ncol} n {n}")
    x, dy = (3 * rng.standard_normal(n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    rel(eltwise(2, x), U.eltwise_ref(2, x, None, 0, 1), 1e-5, f"gelu n {n}")
    rel(eltwise(3, x, dy), U.eltwise_ref(3, x, dy, 0, 1), 1e-5, f"gelu' n {n}")
    rel(eltwise(7, x, dy, s=0.3), U.eltwise_ref(7, x, dy, np.float32(0.3), 1), 1e-5, f"axpy n {n}")


def test_gelu_special_values():
    x = np.array([0.0, 1e-8, -1e-8, 1e-40, -1e-40, 10.0, -10.0, 1.0, -1.0, 5.5, -5.5], np.float32)
    dy = np.ones_like(x)
    g, gg = eltwise(2, x), eltwise(3, x, dy)
    rel(g, U.eltwise_ref(2, x, None, 0, 1), 1e-5, "gelu specials")
    rel(gg, U.eltwise_ref(3, x, dy, 0, 1), 1e-5, "gelu' specials")
    assert g[0] == 0 and gg[0] == 0.5 and g[5] == 10.0 and abs(g[6]) <= 1e-20 and gg[5] == 1.0 and abs(gg[6]) <= 1e-20
    small = np.abs(x) < 1e-6            # the tiny arguments against their own scale, not the rms of the vector
    assert np.allclose(g[small], 0.5 * x[small].astype(np.float64), rtol=1e-5, atol=1e-44)


def test_grid_stride_tail_beyond_the_block_cap():
    """n = 65535 * 4 * 256 + 300: blocks_for() caps the grid, the last 300 elements are reached by the stride loop only.  Compared on
    the device with torch's own fp32 ops (one rounding each: the same bits); the dropout mask has one decision per 1 000 003 elements,
    drawn from the restated rule."""
    n = 65535 * 4 * 256 + 300
    x = torch.randn(n, device=U.dev(), generator=torch.Generator(device=U.dev()).manual_seed(1))
    y = torch.full((n + 64,), float("nan"), device=U.dev())
    op("eltwise", 1, x, None, -0.75, n, 0, y)
    assert torch.equal(y[:n], x * -0.75) and bool(torch.isnan(y[n:]).all())
    group, p, seed = 1000003, 0.5, 77
    keep = dv(U.dropout_keep((n + group - 1) // group, 1, p, seed))
    y.fill_(float("nan"))
    op("dropout", x, n, group, p, seed, y)
    want = torch.where(keep[torch.arange(n, device=U.dev()) // group], x * float(U.drop_keep_scale(p)), torch.zeros_like(x))
    assert torch.equal(y[:n], want) and bool(torch.isnan(y[n:]).all())
    assert 0 < int(keep.sum()) < keep.numel()


@pytest.mark.parametrize("seed", [1, 0xDEADBEEFCAFE1234])
@pytest.mark.parametrize("group", [1, 80])
def test_dropout_mask_bit_for_bit(group, seed):
    rng = np.random.default_rng(group)
    for n in (3 * group + 5, 1000):
        x = (rng.standard_normal(n) + 3).astype(np.float32)
        for p in (0.0, 1e-6, 0.2, 0.5, 0.999):
            out = Out.dense(n)
            op("dropout", dv(x), n, group, p, seed, out)
            same_bits(out.take(), U.dropout_ref(x, group, p, seed).astype(np.float64), f"dropout p{p} group{group} n{n}")
    refused("dropout", dv(x), n, group, 1.0, seed, Out.dense(n))
    refused("dropout", dv(x), n, 0, 0.5, seed, Out.dense(n))


# ================================================================================================ LayerNorm
def ln_case(R, C, rng, add_rows=0, shift=0.0, const_row=False, eps=1e-5):
    x = (shift + rng.standard_normal((R, C))).astype(np.float32)
    if const_row:
        x[R // 2] = np.float32(0.75)
    w, b = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    add = rng.standard_normal((add_rows, C)).astype(np.float32) if add_rows else None
    dy = rng.standard_normal((R, C)).astype(np.float32)
    y, stats, dx, xhat = Out.dense(R, C), Out.dense(R, 2), Out.dense(R, C), Out.dense(R, C)
    xt, wt = dv(x), dv(w)
    op("layernorm_fwd", xt, wt, dv(b), None if add is None else dv(add), add_rows, R, C, eps, y, stats)
    y, stats = y.take(), stats.take()
    op("layernorm_bwd", xt, wt, dv(dy), dv(stats), R, C, dx, xhat)
    xd = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    yd = torch.nn.functional.layer_norm(xd, (C,), torch.from_numpy(w.astype(np.float64)), torch.from_numpy(b.astype(np.float64)), eps)
    yd.backward(torch.from_numpy(dy.astype(np.float64)))
    x64 = x.astype(np.float64)
    mean, var = x64.mean(1), x64.var(1)
    what = f"R{R} C{C} add{add_rows} shift{shift} const{const_row}"
    yref = yd.detach().numpy() + (0 if add is None else add.astype(np.float64)[np.arange(R) % add_rows])
    rel(y, yref, 1e-5, "ln y " + what)
    rel(stats[:, 0], mean, 1e-5, "ln mean " + what)
    rel(stats[:, 1], 1 / np.sqrt(var + eps), 1e-5, "ln rstd " + what)
    rel(xhat.take(), (x64 - mean[:, None]) / np.sqrt(var + eps)[:, None], 1e-5, "ln xhat " + what)
    rel(dx.take(), xd.grad.numpy(), 2e-5, "ln dx " + what)
    return stats


@pytest.mark.parametrize("C", [64, 128, 192, 320, 512])
def test_layernorm(C):
    rng = np.random.default_rng(C)
    for R in (1, 3, 4, 5, 77):
        ln_case(R, C, rng)
    for add_rows in (1, 7, 77):
        ln_case(77, C, rng, add_rows=add_rows)
    stats = ln_case(5, C, rng, const_row=True)
    assert stats[2, 0] == np.float32(0.75) and abs(stats[2, 1] - 1e-5 ** -0.5) <= 1e-5 * 1e-5 ** -0.5       # rstd = eps^-1/2


@pytest.mark.parametrize("C", [64, 512])
def test_layernorm_rows_at_mean_1e3(C):
    ln_case(77, C, np.random.default_rng(C + 1), shift=1e3)


def test_layernorm_refusals():
    x, o = dv(np.zeros((2, 576), np.float32)), Out.dense(2, 576)
    for C in (100, 576):
        refused("layernorm_fwd", x, x, x, None, 0, 2, C, 1e-5, o, o)
        refused("layernorm_bwd", x, x, x, x, 2, C, o, o)


# ================================================================================================ BatchNorm pieces
def test_bn_stats_small_row_counts():
    rng = np.random.default_rng(1)
    C, eps, mom = 9, 1e-5, 0.1
    for R in (1, 2, 1000):
        mean, ssq = rng.standard_normal(C).astype(np.float32), (R * rng.uniform(0.5, 2, C)).astype(np.float32)
        if R == 1:
            ssq[:] = 0
        rm, rv = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
        var = ssq.astype(np.float64) / R
        unb = var * R / (R - 1) if R > 1 else var              # nn.BatchNorm's running variance is unbiased; one row has no such estimate
        for running in (True, False):
            mr = Out.dense(2, C)
            orm, orv = Out.dense(C, init=rm), Out.dense(C, init=rv)
            op("bn_stats", dv(mean), dv(ssq), C, R, eps, mom, mr, orm if running else None, orv if running else None)
            got = mr.take()
            same_bits(got[0], mean.astype(np.float64), "bn mean")
            rel(got[1], 1 / np.sqrt(var + eps), 1e-5, f"bn rstd R{R}")
            if running:
                rel(orm.take(), 0.9 * rm.astype(np.float64) + 0.1 * mean, 1e-5, f"running mean R{R}")
                rel(orv.take(), 0.9 * rv.astype(np.float64) + 0.1 * unb, 1e-5, f"running var R{R}")
            else:
                same_bits(orm.take(), rm.astype(np.float64), "running mean untouched")


@pytest.mark.parametrize("R,C", [(77, 1), (77, 9), (3, 256), (259, 256)])
def test_bn_chain_against_autograd(R, C):
    """mean -> centred squares -> bn_stats -> apply (+ReLU) -> bwd_prep -> two column sums -> bwd_dx, against float64 autograd of
    F.batch_norm(training=True) + relu.  R C is no multiple of the 256-thread block except where C = 256 makes it one.  One channel
    has w = b = 0: every output is exactly 0 and passes no gradient (relu'(0) = 0)."""
    rng = np.random.default_rng(R * C)
    eps = 1e-5
    x = (rng.standard_normal((R, C)) * rng.uniform(0.5, 2, C) + rng.standard_normal(C)).astype(np.float32)
    w, b = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32), (0.3 * rng.standard_normal(C)).astype(np.float32)
    if C > 1:
        w[C // 2] = b[C // 2] = 0
    dy = rng.standard_normal((R, C)).astype(np.float32)
    for relu in (1, 0):
        mean = colsum(x, None, 0, scale=1.0 / R, nsplit=2)
        ssq = colsum(x, mean, 3, nsplit=2)
        mr = Out.dense(2, C)
        op("bn_stats", dv(mean), dv(ssq), C, R, eps, 0.1, mr, None, None)
        mr = mr.take()
        y, g, gx, dx = Out.dense(R, C), Out.dense(R, C), Out.dense(R, C), Out.dense(R, C)
        xt, mrt, wt = dv(x), dv(mr), dv(w)
        op("bn_apply", xt, mrt, wt, dv(b), R, C, relu, y)
        y = y.take()
        op("bn_bwd_prep", xt, dv(y) if relu else None, dv(dy), mrt, R, C, relu, g, gx)
        g, gx = g.take(), gx.take()
        dbeta, dgamma = colsum(g, None, 0, nsplit=2), colsum(gx, None, 0, nsplit=2)
        op("bn_bwd_dx", xt, dv(g), mrt, wt, dv(dbeta), dv(dgamma), R, C, dx)
        xd, wd, bd = (torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for v in (x, w, b))
        yd = torch.nn.functional.batch_norm(xd, None, None, wd, bd, training=True, eps=eps)
        yd = torch.relu(yd) if relu else yd
        yd.backward(torch.from_numpy(dy.astype(np.float64)))
        what = f"R{R} C{C} relu{relu}"
        rel(y, yd.detach().numpy(), 1e-5, "bn y " + what)
        rel(dx.take(), xd.grad.numpy(), 5e-5, "bn dx " + what)
        rel(dgamma, wd.grad.numpy(), 5e-5, "bn dgamma " + what)
        rel(dbeta, bd.grad.numpy(), 5e-5, "bn dbeta " + what)
        if relu and C > 1:
            assert not y[:, C // 2].any() and not g[:, C // 2].any() and (y >= 0).all()
            same_bits(g, np.where(y > 0, dy, 0).astype(np.float64), "bn g = dy (y > 0)")


# ================================================================================================ softmax
SM_L = [1, 5, 63, 64, 65, 200, 691]


def softmax_pair(s, mask, rps, dp):
    rows, L = s.shape
    p, ds = Out.dense(rows, L), Out.dense(rows, L)
    mt = None if mask is None else dv(mask)
    op("softmax_fwd", dv(s), mt, rows, L, rps, p)
    p = p.take()
    op("softmax_bwd", dv(p), dv(dp), mt, rows, L, rps, ds)
    sd = torch.from_numpy(np.where(np.isfinite(s), s, 0).astype(np.float64)).requires_grad_(True)       # non-finite scores sit under the mask only
    s_in = sd
    if mask is not None:
        m = torch.from_numpy(mask).bool()[torch.arange(rows) // rps]
        assert bool((torch.from_numpy(np.isfinite(s)) | ~m).all())
        s_in = sd.masked_fill(~m, float(np.float32(-1e9)))
    pd = torch.softmax(s_in, dim=1)
    pd.backward(torch.from_numpy(dp.astype(np.float64)))
    return p, ds.take(), pd.detach().numpy(), sd.grad.numpy()


@pytest.mark.parametrize("L", SM_L)
def test_softmax(L):
    rng = np.random.default_rng(L)
    for rows in (1, 3, 4, 5, 7):
        s = (3 * rng.standard_normal((rows, L))).astype(np.float32)
        s[0, ::2] = 300
        s[0, 1::2] = -300
        dp = rng.standard_normal((rows, L)).astype(np.float32)
        p, ds, pr, dsr = softmax_pair(s, None, 1, dp)
        rel(p, pr, 1e-5, f"softmax L{L} rows{rows}")
        rel(ds, dsr, 1e-5, f"softmax bwd L{L} rows{rows}")
        assert np.abs(p.astype(np.float64).sum(1) - 1).max() <= 1e-5


@pytest.mark.parametrize("L", SM_L)
def test_softmax_masked(L):
    """rows_per_scene = 3 over 7 rows (scenes 0 0 0 1 1 1 2); scene 1 fully masked: uniform 1 / L forward, zero backward; +inf and NaN
    stored under the mask must not reach either output."""
    rng = np.random.default_rng(L + 1000)
    rows, rps = 7, 3
    mask = (rng.uniform(size=(3, L)) < 0.6).astype(np.uint8)
    mask[0, 0] = 1
    mask[1] = 0
    mask[2, :] = 1
    mask[2, L // 2] = 0 if L > 1 else 1
    s = (3 * rng.standard_normal((rows, L))).astype(np.float32)
    dp = rng.standard_normal((rows, L)).astype(np.float32)
    hidden = np.repeat(mask, rps, axis=0)[:rows] == 0
    s[hidden & (np.arange(L)[None, :] % 2 == 0)] = np.inf
    s[hidden & (np.arange(L)[None, :] % 2 == 1)] = np.nan
    p, ds, pr, dsr = softmax_pair(s, mask, rps, dp)
    assert np.isfinite(p).all() and np.isfinite(ds).all()
    rel(p, pr, 1e-5, f"masked softmax L{L}")
    rel(ds, dsr, 1e-5, f"masked softmax bwd L{L}")
    same_bits(p[3:6], np.full((3, L), np.float32(1.0) / np.float32(L), np.float64), "fully masked scene: uniform")
    assert not ds[3:6].any() and not ds[hidden].any()
    assert (p[hidden & ~np.repeat(mask.sum(1) == 0, rps)[:rows, None]] == 0).all()


# ================================================================================================ slot pieces
def test_slot_inputs_and_backward():
    rng = np.random.default_rng(2)
    for nclus, K, S in ((1, 1, 1), (7, 20, 11), (300, 5, 300)):
        center = ints(rng, (nclus, 3)) / 2
        cluster = ints(rng, (S, K, 3), -3, 3) / 2
        cluster[rng.uniform(size=(S, K)) < 0.3] = 0                      # padding
        cluster[0, 0] = (-0.0, 0.0, 0.0)                                 # -0.0 is zero: padding
        if K > 1:
            cluster[0, 1] = (0.0, 1.5, -2.0)                             # one zero coordinate is a point
        for src in (None, rng.integers(0, S, nclus).astype(np.int32)):
            x6, pm = Out.dense(nclus * K, 6), torch.full((nclus * K + 64,), 0x5a, dtype=torch.uint8, device=U.dev())
            op("slot_inputs", dv(center.astype(np.float32)), dv(cluster.astype(np.float32)), None if src is None else dv(src), nclus, K, x6, pm)
            p = cluster[np.arange(nclus) if src is None else src]         # (nclus, K, 3)
            pad = (p == 0).all(-1)
            ref = np.concatenate([np.where(pad[..., None], 0, p - center[:, None, :]), p], -1).reshape(nclus * K, 6)
            same_bits(x6.take(), ref, f"x6 nclus{nclus} K{K}")
            pm = pm.cpu().numpy()
            assert np.array_equal(pm[:nclus * K], pad.reshape(-1).astype(np.uint8)) and (pm[nclus * K:] == 0x5a).all()
            if nclus == 7 and src is None:
                assert pm[0] == 1 and pm[1] == 0
            dx6, dc = ints(rng, (nclus * K, 6)), Out.dense(nclus, 3)
            op("slot_inputs_bwd", dv(dx6.astype(np.float32)), dv(pm[:nclus * K]), nclus, K, dc)
            same_bits(dc.take(), -(dx6[:, :3].reshape(nclus, K, 3) * ~pad[..., None]).sum(1), "dcenter")


@pytest.mark.parametrize("C", [1, 64, 256])
@pytest.mark.parametrize("K", [1, 2, 64])
def test_slot_pool(K, C):
    """Integers in [-2, 2]: ties in almost every column, the first index wins; mean over K = 1, 2, 64 is exact."""
    rng = np.random.default_rng(K * C)
    nclus = 5
    h = ints(rng, (nclus, K, C), -2, 2)
    dout = ints(rng, (nclus, C))
    for mode in (0, 1):
        out, arg, dh = Out.dense(nclus, C), Out.dense(nclus, C, dtype=np.int32), Out.dense(nclus, K, C)
        op("slot_pool", dv(h.astype(np.float32)), nclus, K, C, mode, out, arg if mode else None)
        if mode == 0:
            same_bits(out.take(), h.mean(1), f"mean pool K{K} C{C}")
            arg_np = arg.take()
            assert (arg_np == U.POISON_I32).all()
            op("slot_pool_bwd", dv(dout.astype(np.float32)), None, nclus, K, C, 0, dh)
            same_bits(dh.take(), np.broadcast_to(dout[:, None, :] / K, (nclus, K, C)), "mean pool bwd")
        else:
            same_bits(out.take(), h.max(1), f"max pool K{K} C{C}")
            arg_np = arg.take()
            same_bits(arg_np, h.argmax(1).astype(np.int32), "first arg-max")
            op("slot_pool_bwd", dv(dout.astype(np.float32)), dv(arg_np), nclus, K, C, 1, dh)
            same_bits(dh.take(), np.where(np.arange(K)[None, :, None] == arg_np[:, None, :], dout[:, None, :], 0), "max pool bwd")


def offset_ref(c0, raw, minmax, M, margin):
    """float64 autograd of PRE:59-62: new = max(min(c0 + tanh(raw) margin, max), min); d new / d raw."""
    rd = torch.from_numpy(raw.astype(np.float64)).requires_grad_(True)
    mm = torch.from_numpy(minmax.astype(np.float64))
    B = mm.shape[0]
    v = torch.from_numpy(c0.astype(np.float64)).view(B, M, 3) + torch.tanh(rd).view(B, M, 3) * float(np.float32(margin))
    out = torch.max(torch.min(v, mm[:, None, 3:]), mm[:, None, :3])
    out.sum().backward()
    return out.detach().numpy().reshape(-1, 3), rd.grad.numpy()


def offset_inputs():
    rng = np.random.default_rng(8)
    B, M = 3, 5
    minmax = np.concatenate([-1 - rng.uniform(size=(B, 3)), 1 + rng.uniform(size=(B, 3))], 1).astype(np.float32)
    c0 = rng.uniform(-0.6, 0.6, (B, M, 3)).astype(np.float32)                # inside
    raw = rng.standard_normal((B, M, 3)).astype(np.float32)
    c0[:, 0] = minmax[:, 3:]; raw[:, 0] = 0                                  # exactly on the upper face: coefficient 0.5
    c0[:, 1] = minmax[:, :3]; raw[:, 1] = 0                                  # exactly on the lower face
    c0[:, 2] = minmax[:, 3:] + 1                                             # outside above: coefficient 0
    c0[:, 3, :2] = minmax[:, :2] - 1                                         # outside below
    return B, M, c0.reshape(-1, 3), raw.reshape(-1, 3), minmax


def test_offset_apply():
    B, M, c0, raw, minmax = offset_inputs()
    margin = 0.3
    cout, dcoef = Out.dense(B * M, 3), Out.dense(B * M, 3)
    op("offset_apply", dv(c0), dv(raw), dv(minmax), B * M, M, margin, cout, dcoef)
    cref, dref = offset_ref(c0, raw, minmax, M, margin)
    cout, dcoef = cout.take(), dcoef.take()
    rel(cout, cref, 1e-5, "offset_apply centres")
    rel(dcoef, dref, 1e-5, "offset_apply d/draw")
    d3 = dcoef.reshape(B, M, 3)
    assert (d3[:, 0] == np.float32(0.5) * np.float32(margin)).all() and (d3[:, 1] == np.float32(0.5) * np.float32(margin)).all()
    assert not d3[:, 2].any() and not d3[:, 3, :2].any() and (d3[:, 4] > 0).all()
    same_bits(cout.reshape(B, M, 3)[:, 2], minmax[:, 3:].astype(np.float64), "clamped to the face")


# ================================================================================================ slot-bias table
SB_CASES = [(s, C) for s in (1, 4, 5, 16, 23) for C in sorted({1, s * s} if s != 23 else {1, 512, 529})]


@pytest.mark.parametrize("s,C", SB_CASES)
def test_slotbias(s, C):
    rng = np.random.default_rng(100 * s + C)
    for Mk in (1, 4, 5, 13):
        pb, pc, pr = (rng.standard_normal(sh).astype(np.float32) for sh in ((Mk, 16), (Mk, s), (Mk, s)))
        table = Out.dense(Mk, C)
        op("slotbias_fwd", dv(pb), dv(pc), dv(pr), Mk, s, C, table)
        leaves = [torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for v in (pb, pc, pr)]
        tref = U.slotbias_torch(*leaves, s, C)
        rel(table.take(), tref.detach().numpy(), 1e-5, f"slot-bias table s{s} C{C} Mk{Mk}")
        if C > 512:
            refused("slotbias_bwd", dv(pb), Mk, s, C, Out.dense(Mk, 16), Out.dense(Mk, s), Out.dense(Mk, s))     # the LDS stage holds 512
            continue
        dt = rng.standard_normal((Mk, C)).astype(np.float32)
        tref.backward(torch.from_numpy(dt.astype(np.float64)))
        dpb, dpc, dpr = Out.dense(Mk, 16), Out.dense(Mk, s), Out.dense(Mk, s)
        op("slotbias_bwd", dv(dt), Mk, s, C, dpb, dpc, dpr)
        for got, leaf, nm in ((dpb, leaves[0], "dpb"), (dpc, leaves[1], "dpc"), (dpr, leaves[2], "dpr")):
            ref = leaf.grad.numpy()
            if not ref.any():
                assert not got.take().any(), nm
            else:
                rel(got.take(), ref, 1e-5, f"slot-bias {nm} s{s} C{C} Mk{Mk}")


def test_slotbias_refusals():
    z = dv(np.zeros(13 * 600, np.float32))
    o = Out.dense(13 * 600)
    refused("slotbias_bwd", z, 4, 24, 512, o, o, o)
    refused("slotbias_fwd", z, z, z, 4, 24, 512, o)                     # the backward stages a slot's table in 512 LDS words: s <= 23
    for s, C in ((4, 17), (1, 2), (22, 485)):
        refused("slotbias_fwd", z, z, z, 4, s, C, o)
        refused("slotbias_bwd", z, 4, s, C, o, o, o)
    o.take()


# ================================================================================================ index and row operators
def test_rows_gather_scatter_keep():
    rng = np.random.default_rng(6)
    for rows, C, S in ((1, 1, 1), (5, 3, 9), (77, 256, 100), (300, 65, 300)):
        x = ints(rng, (S, C))
        src = rng.permutation(S)[:rows].astype(np.int32)
        y = Out.dense(rows, C)
        op("rows_gather", dv(x.astype(np.float32)), dv(src), rows, C, y)
        same_bits(y.take(), x[src], f"gather rows{rows} C{C}")
        dy = ints(rng, (rows, C))
        dx = Out.dense(S, C, init=np.zeros((S, C), np.float32))
        op("rows_scatter", dv(dy.astype(np.float32)), dv(src), rows, C, dx)
        ref = np.zeros((S, C))
        ref[src] = dy
        same_bits(dx.take(), ref, f"scatter rows{rows} C{C}")
    for B, M, Mt, Mk in ((1, 1, 1, 1), (3, 11, 9, 5), (2, 300, 300, 257)):
        order = np.stack([rng.permutation(M)[:Mt] for _ in range(B)]).astype(np.int32)
        keep = np.stack([rng.permutation(Mt)[:Mk] for _ in range(B)]).astype(np.int32)
        src = Out.dense(B * Mk, dtype=np.int32)
        op("keep_rows", dv(order), dv(keep), B, M, Mt, Mk, src)
        ref = (np.arange(B)[:, None] * M + np.take_along_axis(order, keep, 1)).reshape(-1)
        same_bits(src.take(), ref.astype(np.int32), f"keep_rows B{B} M{M}")


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 257])
def test_transpose(rows):
    rng = np.random.default_rng(rows)
    for cols in (1, 31, 32, 33, 257):
        x = ints(rng, (rows, cols), -1000, 1000)
        out = Out.dense(cols, rows)
        op("transpose", dv(x.astype(np.float32)), rows, cols, out)
        same_bits(out.take(), x.T, f"transpose {rows} x {cols}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 2047, 2048, 2049, 5000])
def test_out_positions(N, B):
    rng = np.random.default_rng(N + B)
    low = rng.integers(0, 1 << 31, (B, N)).astype(np.uint32)                  # bits 0 .. 30 carry the slot: only bit 31 drops a point
    pats = {"all kept": np.zeros((B, N), bool), "all dropped": np.ones((B, N), bool),
            "alternating": np.broadcast_to(np.arange(N) % 2 == 1, (B, N)), "random": rng.uniform(size=(B, N)) < 0.4,
            "first tile dropped": np.broadcast_to(np.arange(N) < 2048, (B, N)),
            "middle tile dropped": np.broadcast_to((np.arange(N) >= 2048) & (np.arange(N) < 4096), (B, N))}
    ntiles = (N + 2047) // 2048
    for name, drop in pats.items():
        tag = (low | (drop.astype(np.uint32) << 31)).astype(np.uint32)
        tc, opos, counts = Out.dense(B * ntiles, dtype=np.int32), Out.dense(B, N, dtype=np.int32), Out.dense(B, dtype=np.int32)
        op("out_positions", dv(tag.view(np.int32)), B, N, tc, opos, counts)
        oref, cref = U.out_positions_ref(tag, B, N)
        same_bits(opos.take(), oref, f"opos {name} N{N} B{B}")
        same_bits(counts.take(), cref, f"counts {name}")
        tref = np.stack([(~drop)[:, t * 2048:(t + 1) * 2048].sum(1) for t in range(ntiles)], 1).reshape(-1)
        same_bits(tc.take(), tref.astype(np.int32), f"tile counts {name}")


# ================================================================================================ affine_bwd
def affine_inputs(B, N, Mk, K, rng):
    kidx = rng.integers(0, N, (B, Mk, K)).astype(np.int32)                    # few points, many slots: several slots target one point
    kidx[rng.uniform(size=kidx.shape) < 0.25] = -1                            # padded slots
    kidx[0, 0, 0] = -1
    drop = rng.uniform(size=(B, N)) < 0.3
    opos, counts = U.out_positions_ref((drop.astype(np.uint32) << 31), B, N)
    kcluster = rng.standard_normal((B, Mk, K, 3)).astype(np.float32)
    kcenter = rng.standard_normal((B, Mk, 3)).astype(np.float32)
    transform = (np.eye(3)[None, None] + 0.3 * rng.standard_normal((B, Mk, 3, 3))).astype(np.float32)
    return kidx, opos, counts, kcluster, kcenter, transform


def affine_call(name, dout_arg, opos, kidx, kcluster, kcenter, transform, B, N, Mk, K):
    outs = Out.dense(B, Mk, 3), Out.dense(B, Mk, 3, 3), Out.dense(B, Mk, 3)
    op(name, dout_arg, dv(opos), dv(kidx), dv(kcluster), dv(kcenter), dv(transform), B, N, Mk, K, outs[0], outs[1], outs[2])
    return [o.take() for o in outs]


@pytest.mark.parametrize("K", [1, 20, 64])
def test_affine_bwd(K):
    rng = np.random.default_rng(K)
    B, N, Mk = 3, 40, 5
    kidx, opos, counts, kcluster, kcenter, transform = affine_inputs(B, N, Mk, K, rng)
    assert (opos < 0).any() and (kidx < 0).any() and np.unique(kidx[0][kidx[0] >= 0]).size < (kidx[0] >= 0).sum() or K == 1
    dout = rng.standard_normal((B, N, 3)).astype(np.float32)                  # dense form: row `pos` of scene b; rows past counts[b] unused
    ref = U.affine_bwd_ref([dout[b] for b in range(B)], opos, kidx, kcluster, kcenter, transform, B, N, Mk, K)
    got = affine_call("affine_bwd", dv(dout), opos, kidx, kcluster, kcenter, transform, B, N, Mk, K)
    for g, r, nm in zip(got, ref, ("dtranslate", "dtransform", "dkcenter")):
        rel(g, r, 1e-5, f"affine_bwd {nm} K{K}")
    # the list form: one (n_b, 3) gradient per scene, scene 1 without gradient
    lists = [dv(dout[b, :max(int(counts[b]), 1)].copy()) for b in range(B)]
    keep, pp = U.cptr_array([lists[0].data_ptr(), None, lists[2].data_ptr()])
    ref = U.affine_bwd_ref([dout[0], None, dout[2]], opos, kidx, kcluster, kcenter, transform, B, N, Mk, K)
    got = affine_call("affine_bwd_list", pp, opos, kidx, kcluster, kcenter, transform, B, N, Mk, K)
    for g, r, nm in zip(got, ref, ("dtranslate", "dtransform", "dkcenter")):
        rel(g, r, 1e-5, f"affine_bwd_list {nm} K{K}")
    assert not got[0][1].any() and not got[1][1].any() and not got[2][1].any()


def test_affine_bwd_scene_and_slot_limits():
    rng = np.random.default_rng(32)
    B, N, Mk, K = 32, 6, 2, 3
    kidx, opos, counts, kcluster, kcenter, transform = affine_inputs(B, N, Mk, K, rng)
    dout = rng.standard_normal((B, N, 3)).astype(np.float32)
    lists = [dv(dout[b].copy()) for b in range(B)]
    keep, pp = U.cptr_array([t.data_ptr() for t in lists])
    ref = U.affine_bwd_ref([dout[b] for b in range(B)], opos, kidx, kcluster, kcenter, transform, B, N, Mk, K)
    got = affine_call("affine_bwd_list", pp, opos, kidx, kcluster, kcenter, transform, B, N, Mk, K)
    for g, r, nm in zip(got, ref, ("dtranslate", "dtransform", "dkcenter")):
        rel(g, r, 1e-5, f"affine_bwd_list B32 {nm}")
    z, o = dv(np.zeros(4096, np.float32)), Out.dense(4096)
    zi = dv(np.zeros(4096, np.int32))
    keep33, pp33 = U.cptr_array([z.data_ptr()] * 33)
    refused("affine_bwd_list", pp33, zi, zi, z, z, z, 33, 1, 1, 1, o, o, o)
    refused("affine_bwd_list", pp, zi, zi, z, z, z, 2, 1, 1, 65, o, o, o)
    refused("affine_bwd", z, zi, zi, z, z, z, 2, 1, 1, 65, o, o, o)
    o.take()


# ================================================================================================ image tokens
@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("hw", [1, 121, 225])
def test_tokens_finish(hw, C):
    rng = np.random.default_rng(hw + C)
    for nimg in (1, 6):
        tok = rng.standard_normal((nimg, hw + 1, C)).astype(np.float32)
        pos = rng.standard_normal((hw + 1, C)).astype(np.float32)
        init = tok.copy()
        init[:, 0] = np.nan                                                   # row 0 is written, never read
        buf = Out.dense(nimg, hw + 1, C, init=init)
        op("tokens_finish", buf, dv(pos), nimg, hw, C)
        ref = tok.astype(np.float64)
        ref[:, 0] = ref[:, 1:].mean(1)
        ref += pos.astype(np.float64)[None]
        rel(buf.take(), ref, 1e-5, f"tokens_finish hw{hw} C{C} nimg{nimg}")
        d = rng.standard_normal((nimg, hw + 1, C)).astype(np.float32)
        buf = Out.dense(nimg, hw + 1, C, init=d)
        op("tokens_finish_bwd", buf, nimg, hw, C)
        ref = d.astype(np.float64)
        ref[:, 1:] += ref[:, :1] / hw
        ref[:, 0] = 0
        got = buf.take()
        rel(got, ref, 1e-5, f"tokens_finish_bwd hw{hw} C{C} nimg{nimg}")
        assert not got[:, 0].any()


# ================================================================================================ the NaN rule
# nn.ReLU, torch.max(torch.min(c, max), min) (PRE:62) and torch.max(dim) (PRE:140) return NaN where an input is NaN, the last with the
# index of the first NaN.  One test per operator: NaN in slot 0, in a middle slot, in the last slot, and no NaN.
NAN_AT = {"slot 0": [0], "middle": [3], "last": [-1], "none": [], "first and last": [0, -1]}


@pytest.mark.parametrize("where", list(NAN_AT))
def test_nan_relu_eltwise(where):
    a = np.array([-2.0, 1.5, -0.0, 0.0, 3.0, -1.0, 2.0], np.float32)
    a[NAN_AT[where]] = np.nan
    got = eltwise(4, a)
    want = torch.relu(torch.from_numpy(a)).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == len(NAN_AT[where])
    same_bits(got, want.astype(np.float64), "relu")


@pytest.mark.parametrize("where", list(NAN_AT))
def test_nan_relu_bn_apply(where):
    R, C = 7, 3
    rng = np.random.default_rng(3)
    x = rng.standard_normal((R, C)).astype(np.float32)
    x[NAN_AT[where], 1] = np.nan
    mr = np.stack([np.full(C, 0.25), np.full(C, 2.0)]).astype(np.float32)
    w, b = np.array([1.0, -0.5, 2.0], np.float32), np.array([0.5, 0.25, -1.0], np.float32)
    y = Out.dense(R, C)
    op("bn_apply", dv(x), dv(mr), dv(w), dv(b), R, C, 1, y)
    want = torch.relu((torch.from_numpy(x) - 0.25) * 2.0 * torch.from_numpy(w) + torch.from_numpy(b)).numpy()      # exact steps: same bits
    got = y.take()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == len(NAN_AT[where])
    same_bits(got, want.astype(np.float64), "bn_apply relu")


@pytest.mark.parametrize("where", list(NAN_AT))
def test_nan_clamp_offset_apply(where):
    B, M, c0, raw, minmax = offset_inputs()
    c0, raw = c0.copy(), raw.copy()
    c0[NAN_AT[where], 0] = np.nan                   # a NaN centre
    raw[NAN_AT[where], 2] = np.nan                  # a NaN offset
    cout, dcoef = Out.dense(B * M, 3), Out.dense(B * M, 3)
    op("offset_apply", dv(c0), dv(raw), dv(minmax), B * M, M, 0.3, cout, dcoef)
    cref, _ = offset_ref(c0, raw, minmax, M, 0.3)
    got = cout.take()
    dcoef.take()
    assert np.array_equal(np.isnan(got), np.isnan(cref)) and np.isnan(got).sum() == 2 * len(NAN_AT[where])
    ok = ~np.isnan(cref)
    rel(got[ok], cref[ok], 1e-5, "finite centres next to the NaN ones")


@pytest.mark.parametrize("where", list(NAN_AT))
def test_nan_max_pool(where):
    rng = np.random.default_rng(4)
    nclus, K, C = 3, 7, 5
    h = ints(rng, (nclus, K, C), -2, 2).astype(np.float32)
    h[:, NAN_AT[where], 1] = np.nan
    h[0, :, 3] = 2.0                                 # a tie over every slot next to it
    out, arg = Out.dense(nclus, C), Out.dense(nclus, C, dtype=np.int32)
    op("slot_pool", dv(h), nclus, K, C, 1, out, arg)
    want, warg = torch.from_numpy(h).max(dim=1)
    got = out.take()
    assert np.array_equal(np.isnan(got), np.isnan(want.numpy())) and np.isnan(got).sum() == (nclus if NAN_AT[where] else 0)
    same_bits(got, want.numpy().astype(np.float64), "max pool")
    same_bits(arg.take(), warg.numpy().astype(np.int32), "arg = the first NaN, else the first maximum")
    mean = Out.dense(nclus, C)
    op("slot_pool", dv(h), nclus, K, C, 0, mean, None)
    assert np.array_equal(np.isnan(mean.take()), np.isnan(h).any(1))


@pytest.mark.parametrize("maxpool", [0, 1])
def test_nan_channel_through_the_fused_slot_network(maxpool):
    """k_sn_apply through ptx_op_slotnet_fwd at the smallest channel count it takes (C = 256; two clusters of three slots, one slot padded): a NaN entry of conv_w makes
    that channel's batch statistics and every activation NaN.  torch (Conv -> BatchNorm2d -> ReLU -> mean / max) and the composition
    of the generic operators return NaN for the channel, with arg 0; the other channels are unaffected."""
    rng = np.random.default_rng(5)
    nclus, K, C, eps = 2, 3, 256, 1e-5
    center = rng.standard_normal((nclus, 3)).astype(np.float32)
    cluster = rng.standard_normal((nclus, K, 3)).astype(np.float32)
    cluster[1, 2] = 0
    cw, cb = (0.5 * rng.standard_normal((C, 6))).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    bw, bb = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)
    for bad in ((), (70,)):
        w = cw.copy()
        w[list(bad), 4] = np.nan
        lib_bytes = U._abi.lib().ptx_op_slotnet_scratch_bytes(C)
        scratch = torch.zeros(lib_bytes, dtype=torch.uint8, device=U.dev())
        out, arg, mr, tmp = Out.dense(nclus, C), Out.dense(nclus, C, dtype=np.int32), Out.dense(2, C), Out.dense(2, C)
        op("slotnet_fwd", dv(center), dv(cluster), nclus, K, C, dv(w), dv(cb), dv(bw), dv(bb), eps, 0.1, None, None, maxpool, out,
           arg if maxpool else None, mr, tmp, scratch, lib_bytes)
        got, mr = out.take(), mr.take()
        # the generic composition: slot inputs -> product with conv_w^T -> bias -> statistics -> normalise + ReLU -> pool
        R = nclus * K
        x6, pm = Out.dense(R, 6), torch.zeros(R, dtype=torch.uint8, device=U.dev())
        op("slot_inputs", dv(center), dv(cluster), None, nclus, K, x6, pm)
        x6 = x6.take()
        hh, _ = Gemm(R, C, 6, a=(6, 1), b=(1, 6), c=(C, 1)).run(x6, w.reshape(-1))
        hh = eltwise(6, hh.reshape(-1), cb, ncol=C).reshape(R, C)
        mean = colsum(hh, None, 0, scale=1.0 / R)
        ssq = colsum(hh, mean, 3)
        mrc = Out.dense(2, C)
        op("bn_stats", dv(mean), dv(ssq), C, R, eps, 0.1, mrc, None, None)
        y = Out.dense(R, C)
        op("bn_apply", dv(hh), dv(mrc.take()), dv(bw), dv(bb), R, C, 1, y)
        pooled, parg = Out.dense(nclus, C), Out.dense(nclus, C, dtype=np.int32)
        op("slot_pool", dv(y.take()), nclus, K, C, maxpool, pooled, parg if maxpool else None)
        comp = pooled.take()
        # torch, float64
        xd = torch.from_numpy(x6.astype(np.float64))
        hd = xd @ torch.from_numpy(w.astype(np.float64)).T + torch.from_numpy(cb.astype(np.float64))
        yd = torch.relu(torch.nn.functional.batch_norm(hd, None, None, torch.from_numpy(bw.astype(np.float64)),
                                                       torch.from_numpy(bb.astype(np.float64)), training=True, eps=eps)).view(nclus, K, C)
        want, warg = (yd.max(dim=1) if maxpool else (yd.mean(dim=1), None))
        nanc = np.zeros(C, bool)
        nanc[list(bad)] = True
        for name, v in (("fused", got), ("composition", comp)):
            assert np.isnan(v[:, nanc]).all() and not np.isnan(v[:, ~nanc]).any(), f"{name}: NaN channels {np.nonzero(np.isnan(v).any(0))[0]}"
            rel(v[:, ~nanc], want.numpy()[:, ~nanc], 1e-5, f"{name} slot network, maxpool {maxpool}")
        assert np.isnan(mr[0, nanc]).all() and not np.isnan(mr[:, ~nanc]).any()
        if maxpool:
            ga, ca = arg.take(), parg.take()
            assert (ga[:, nanc] == 0).all() and (ca[:, nanc] == 0).all() and (warg.numpy()[:, nanc] == 0).all()
            same_bits(ga[:, ~nanc], warg.numpy()[:, ~nanc].astype(np.int32), "fused arg-max")
