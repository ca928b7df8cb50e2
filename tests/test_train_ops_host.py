"""Host side of the train-mode operator set, no device: the route ptx_op_gemm takes (ptx_op_gemm_route: the very function the
launch dispatches on) at the products the training step issues and one step either side of every flip of the rule, the calls it
refuses, and the numpy restatements of tests/train_ops_util.py (dropout rule, K slices, bilinear taps) against what defines them."""
import numpy as np
import pytest
import torch

from tests import train_ops_util as U
from tests.train_ops_util import Gemm

BGEMM, THIN_SCALAR, THIN_VEC, THIN_ROW = 0, 1, 2, 3
A0, B0, C0 = 4096, 8192, 12288          # 16-byte aligned dummies: the route reads the pointers' low bits only


# ---- the six generic products of _AttnPoolCore (proxytransformation_amd/train.py) at nimg * heads = 96, T = 226, hd = 32
NIMG, HEADS, T, HD = 12, 8, 226, 32
CC, Z = HEADS * HD, NIMG * HEADS


def attn_pool_products():
    zb = dict(batch=Z, inner=HEADS)
    return {
        "S": Gemm(1, T, HD, a=(0, 1), b=(1, CC), c=(T, 1), a_bs=(CC, HD), b_bs=(T * CC, HD), c_bs=(HEADS * T, T), alpha=HD ** -0.5, **zb),
        "o": Gemm(1, HD, T, a=(0, 1), b=(CC, 1), c=(HD, 1), a_bs=(HEADS * T, T), b_bs=(T * CC, HD), c_bs=(CC, HD), **zb),
        "dP": Gemm(1, T, HD, a=(0, 1), b=(1, CC), c=(T, 1), a_bs=(CC, HD), b_bs=(T * CC, HD), c_bs=(HEADS * T, T), **zb),
        "dVt": Gemm(T, HD, 1, a=(1, 0), b=(0, 1), c=(CC, 1), a_bs=(HEADS * T, T), b_bs=(CC, HD), c_bs=(T * CC, HD), **zb),
        "dq": Gemm(1, HD, T, a=(0, 1), b=(CC, 1), c=(HD, 1), a_bs=(HEADS * T, T), b_bs=(T * CC, HD), c_bs=(CC, HD), alpha=HD ** -0.5, **zb),
        "dKt": Gemm(T, HD, 1, a=(1, 0), b=(0, 1), c=(CC, 1), a_bs=(HEADS * T, T), b_bs=(CC, HD), c_bs=(T * CC, HD), alpha=HD ** -0.5, **zb),
    }


def test_route_of_the_attention_pool_products():
    want = {"S": THIN_VEC, "o": THIN_ROW, "dP": THIN_VEC, "dVt": THIN_SCALAR, "dq": THIN_ROW, "dKt": THIN_SCALAR}
    got = {k: g.route() for k, g in attn_pool_products().items()}
    assert got == want
    # the node test's 6 images x 8 heads stay below the batch floor of the thin kernels
    for g in attn_pool_products().values():
        g.batch = 48
        assert g.route() == BGEMM


def out_k(K, batch=64, **kw):           # one query row against N = 226 keys, both operands contiguous along k
    d = dict(a=(0, 1), b=(1, 256), c=(226, 1), batch=batch, inner=1, a_bs=(256, 0), b_bs=(226 * 256, 0), c_bs=(226, 0))
    d.update(kw)
    return Gemm(1, 226, K, **d)


def row_k(K, N=32, M=1, batch=64, **kw):    # one probability row against (K, 32) values, B contiguous along n
    d = dict(a=(K, 1), b=(256, 1), c=(N, 1), batch=batch, inner=1, a_bs=(M * K, 0), b_bs=(K * 256, 0), c_bs=(M * N, 0))
    d.update(kw)
    return Gemm(M, N, K, **d)


FLIPS = [
    ("batch 63", out_k(32, batch=63), BGEMM), ("batch 64", out_k(32, batch=64), THIN_VEC),
    ("out K 64", out_k(64), THIN_VEC), ("out K 65", out_k(65), BGEMM),
    ("out K 4", out_k(4), THIN_VEC), ("out K % 4 != 0", out_k(30), THIN_SCALAR), ("out K 1", out_k(1), THIN_SCALAR),
    ("row K 64", row_k(64), THIN_SCALAR), ("row K 65", row_k(65), THIN_ROW),
    ("row K 256", row_k(256), THIN_ROW), ("row K 257", row_k(257), BGEMM),
    ("row N 31", row_k(226, N=31), BGEMM), ("row N 32", row_k(226, N=32), THIN_ROW), ("row N 33", row_k(226, N=33), BGEMM),
    ("row M 2", row_k(226, M=2), THIN_ROW), ("row M 3", row_k(226, M=3), BGEMM),
    ("row b_cs != 1", row_k(226, b=(1, 256)), BGEMM),
    ("row b_rs % 4 != 0", row_k(226, b=(258, 1)), BGEMM),
    ("row b_s1 % 4 != 0", row_k(226, b_bs=(226 * 256 + 2, 0)), BGEMM),
    ("out a_cs != 1", out_k(32, a=(0, 2)), THIN_SCALAR), ("out b_rs != 1", out_k(32, b=(226, 1)), THIN_SCALAR),
    ("out b_cs % 4 != 0", out_k(32, b=(1, 258)), THIN_SCALAR),
    ("out a_s1 % 4 != 0", out_k(32, a_bs=(258, 0)), THIN_SCALAR),
    ("out b_s2 % 4 != 0", out_k(32, inner=2, b_bs=(2 * 226 * 256, 226 * 256 + 1)), THIN_SCALAR),
    ("ksplit 2", out_k(32, ksplit=2, c_sk=64 * 226), BGEMM),
    ("A bf16", out_k(32, a_dtype=1), BGEMM), ("B fp16", out_k(32, b_dtype=2), BGEMM),
    ("nothing thin", Gemm(3, 3, 3, a=(3, 1), b=(3, 1), c=(3, 1), batch=64, a_bs=(9, 0), b_bs=(9, 0), c_bs=(9, 0)), BGEMM),
    ("N 2, K 8", Gemm(226, 2, 8, a=(8, 1), b=(1, 8), c=(2, 1), batch=64, a_bs=(226 * 8, 0), b_bs=(16, 0), c_bs=(452, 0)), THIN_VEC),
    ("K 2 outer", Gemm(226, 32, 2, a=(1, 226), b=(32, 1), c=(32, 1), batch=64, a_bs=(452, 0), b_bs=(64, 0), c_bs=(226 * 32, 0)), THIN_SCALAR),
]


@pytest.mark.parametrize("name,g,want", FLIPS, ids=[f[0].replace(" ", "_") for f in FLIPS])
def test_route_flips(name, g, want):
    assert g.route() == want


def test_route_reads_the_base_pointers():
    assert out_k(32).route(A0, B0, C0) == THIN_VEC
    assert out_k(32).route(A0 + 4, B0, C0) == THIN_SCALAR        # one float off: the 16-byte requests are not legal
    assert out_k(32).route(A0, B0 + 8, C0) == THIN_SCALAR
    assert out_k(32).route(A0, B0, C0 + 4) == THIN_VEC           # C is written word by word
    assert row_k(226).route(A0, B0, C0) == THIN_ROW
    assert row_k(226).route(A0 + 4, B0, C0) == BGEMM             # K > 64: no scalar thin kernel to fall back to
    assert row_k(226).route(A0, B0 + 4, C0) == BGEMM


def test_refusals():
    ok = out_k(32)
    assert ok.route() >= 0
    for what, g in (("two 16-bit operands", out_k(32, a_dtype=1, b_dtype=2)),
                    ("ksplit with accumulate", out_k(32, ksplit=2, accumulate=1)),
                    ("batch % inner", out_k(32, batch=64, inner=3)),
                    ("batch * ksplit > 65535", out_k(32, batch=64, ksplit=1024)),
                    ("batch > 65535", out_k(32, batch=65536)),
                    ("K 0", out_k(0)), ("dtype 3", out_k(32, a_dtype=3))):
        assert g.route() < 0, what
        # ptx_op_gemm refuses the same call before it launches anything (no device is touched on this machine)
        U.refused("gemm", *g.args(A0, B0, C0))
    assert ok.route(0, B0, C0) < 0 and ok.route(A0, 0, C0) < 0 and ok.route(A0, B0, 0) < 0
    assert out_k(32, batch=65535).route() == THIN_VEC and out_k(32, batch=13107, ksplit=5).route() == BGEMM


# ---- restatements
def test_kper_rule():
    assert [U.kper_rule(K, s) for K, s in ((33, 3), (33, 2), (64, 2), (100, 3), (100, 7), (1000, 7), (1000, 3), (1, 1), (4113, 1))] == \
        [32, 32, 32, 64, 32, 160, 352, 32, 4128]
    g = Gemm(1, 1, 33, a=(33, 1), b=(1, 1), c=(1, 1), ksplit=3, c_sk=1)
    assert g.slices() == [(0, 32), (32, 33), (33, 33)]          # one partial and one empty slice
    for K in (33, 64, 100, 1000):
        for s in (2, 3, 7):
            sl = Gemm(1, 1, K, a=(K, 1), b=(1, 1), c=(1, 1), ksplit=s, c_sk=1).slices()
            assert sl[0][0] == 0 and sl[-1][1] == K and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
            assert all((k1 - k0) % 32 == 0 for k0, k1 in sl if k1 < K)


def test_dropout_rule():
    # the hash is the finaliser of splitmix64 after one increment: its published first outputs for the states 0 and 1
    assert int(U.drop_mix32(np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF >> 32
    assert int(U.drop_mix32(np.array([0x9E3779B97F4A7C15], np.uint64))[0]) == 0x6E789E6AA1B965F4 >> 32
    assert U.drop_thresh(0.0) == 0 and U.drop_thresh(0.5) == 1 << 31 and U.drop_thresh(0.25) == 1 << 30
    assert U.drop_thresh(0.2) == int(float(np.float32(0.2)) * 2.0 ** 32)         # p travels as a float
    assert U.drop_keep_scale(0.5) == np.float32(2.0) and U.drop_keep_scale(0.0) == np.float32(1.0)
    assert U.dropout_keep(1000, 1, 0.0, 7).all()
    n = 200000
    for p in (0.2, 0.5, 0.999):
        kept = U.dropout_keep(n, 1, p, 3).mean()
        assert abs(kept - (1 - float(np.float32(p)))) <= 5 * np.sqrt(p * (1 - p) / n), (p, kept)      # five sigma of the binomial
    k80 = U.dropout_keep(3 * 80 + 5, 80, 0.5, 11)
    assert all(np.unique(k80[i:i + 80]).size == 1 for i in (0, 80, 160)) and np.unique(k80[240:]).size == 1
    assert np.array_equal(k80[::80][:4], U.dropout_keep(4, 1, 0.5, 11))          # group g draws element g's decision
    assert not np.array_equal(U.dropout_keep(4096, 1, 0.5, 11), U.dropout_keep(4096, 1, 0.5, 12))
    x = np.arange(1, 9, dtype=np.float32)
    y = U.dropout_ref(x, 1, 0.5, 5)
    assert set(np.unique(y / x)) <= {0.0, 2.0}


@pytest.mark.parametrize("s", [1, 4, 5, 16, 23])
def test_bilinear_taps_against_interpolate(s):
    """The restated taps (formed in fp32 like the kernel) against F.interpolate in float64.  The source coordinate
    4 / s (y + 0.5) - 0.5 < 4 carries three fp32 roundings of at most 4 u each (u = 2^-24): 12 u = 7.2e-7 on either weight.  A weight
    error moves the table by at most that times the step between neighbouring parameters (|pb| <= 1: a step <= 2), once along y and
    once along x: 2 x 2 x 7.2e-7 = 2.9e-6."""
    rng = np.random.default_rng(s)
    Mk = 5
    pb, pc, pr = rng.uniform(-1, 1, (Mk, 16)), rng.uniform(-1, 1, (Mk, s)), rng.uniform(-1, 1, (Mk, s))
    want = U.slotbias_torch(*(torch.from_numpy(v) for v in (pb, pc, pr)), s, s * s).numpy()
    got = U.slotbias_taps_ref(pb, pc, pr, s, s * s)
    assert np.abs(got - want).max() <= 2.9e-6
    i0, i1, l0, l1 = U.bilin_taps(s)
    assert i0.min() >= 0 and i1.max() <= 3 and np.all(l0 + l1 == 1) and np.all((l1 >= 0) & (l1 < 1))
    if s == 4:
        assert np.array_equal(got, pb + (pc[:, :, None] + pr[:, None, :]).reshape(Mk, 16))        # the identity resize
