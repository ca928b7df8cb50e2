"""Direct access to the train-mode operators (``ptx_op_*`` of csrc/train_ops.hip) for tests: ctypes wrappers over ``_abi.lib()``,
guarded NaN-filled output buffers, float64 references in numpy / torch-CPU, and numpy restatements of the host rules the kernels
share (the K slices of ptx_op_gemm, the dropout rule of csrc/train_rules.h, the bilinear taps of the slot-bias table).

Nothing here touches a device at import; the reference half (everything that takes numpy arrays) runs on a CPU-only machine."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from proxytransformation_amd import _abi
from tests.gpu_util import GUARD_WORD

U = 2.0 ** -24                      # unit roundoff of fp32
PAD = 64                            # guard words in front of and behind every output (256 B: the base stays 16-byte aligned)
POISON_I32 = -0x7ffffff0            # what an int32 output holds before the call
TAIL = 64                           # NaN words behind every gemm operand


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def dv(x, dtype=None):
    """numpy -> device tensor (contiguous); dtype: torch dtype of the storage (bf16 / fp16 operands)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev())
    return t if dtype is None else t.to(dtype)


def shifted(x):
    """The same fp32 values at a base pointer one float past a 16-byte boundary: returns (keep-alive tensor, pointer)."""
    buf = torch.full((x.size + 1 + TAIL,), float("nan"), dtype=torch.float32, device=dev())
    buf[1:x.size + 1] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).ravel()).to(dev())
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4


def ptr(x):
    if x is None:
        return None
    if isinstance(x, (int, Out)):
        return int(x) if isinstance(x, int) else x.ptr
    return x.data_ptr()


def rel(a, b, tol, what):
    """The rule of tests/test_gpu_train.py: max error over the rms of the reference."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.sqrt((b ** 2).mean()) + 1e-30
    err = np.abs(a - b).max() / scale if a.shape == b.shape else np.inf
    assert a.shape == b.shape and err <= tol, f"{what}: max err / rms = {err:.3e} (tol {tol:g})"


def same_bits(got, ref, what):
    """fp32 results equal bit for bit (ref: float64 or fp32 values that are exact in fp32)."""
    got = np.asarray(got)
    ref32 = np.asarray(ref).astype(got.dtype)
    assert got.shape == ref32.shape, (what, got.shape, ref32.shape)
    if got.dtype == np.float32:
        assert np.array_equal(ref32.astype(np.float64), np.asarray(ref, np.float64), equal_nan=True), f"{what}: reference not exact in fp32"
        bad = got.view(np.int32) != ref32.view(np.int32)
        # the sign of a zero and the payload of a NaN are not compared
        bad &= ~(np.isnan(got) & np.isnan(ref32)) & ~((got == 0) & (ref32 == 0))
    else:
        bad = got != ref32
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"got {got[tuple(np.argwhere(bad)[0])]!r} ref {ref32[tuple(np.argwhere(bad)[0])]!r}"


class Out:
    """An output buffer of a kernel under test.  `live`: element offsets (from the pointer the kernel receives) of every word the
    kernel may write, in the shape of the logical result.  The buffer spans [0, max(live)] plus PAD words on either side; every
    word that is not live -- front, back and the gaps of a strided layout -- holds GUARD_WORD, every live word NaN (fp32), the
    poison value (int32), or `init`.  take() checks the guards and returns the live words."""

    def __init__(self, live, dtype=np.float32, init=None):
        live = np.asarray(live, np.int64)
        assert live.min() >= 0 and np.unique(live).size == live.size
        self.shape, self.dtype = live.shape, np.dtype(dtype)
        self.buf = torch.full((PAD + int(live.max()) + 1 + PAD,), GUARD_WORD, dtype=torch.int32, device=dev())
        self.idx = torch.from_numpy(live.ravel() + PAD).to(dev())
        if init is None:
            init = np.full(live.shape, np.nan, np.float32) if self.dtype == np.float32 else np.full(live.shape, POISON_I32, np.int32)
        self.buf[self.idx] = torch.from_numpy(np.ascontiguousarray(init, dtype=self.dtype).ravel().view(np.int32)).to(dev())
        self.ptr = self.buf.data_ptr() + 4 * PAD

    @classmethod
    def dense(cls, *shape, dtype=np.float32, init=None):
        return cls(np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape), dtype, init)

    def take(self):
        torch.cuda.synchronize()
        words = self.buf.clone()
        live = words[self.idx].cpu().numpy().view(self.dtype).reshape(self.shape)
        words[self.idx] = GUARD_WORD
        bad = torch.nonzero(words != GUARD_WORD).flatten()
        assert bad.numel() == 0, f"{bad.numel()} guard words overwritten, first at offset {int(bad[0]) - PAD} from the output pointer"
        return live


def op(name, *args):
    """Call ptx_op_<name>(*args, stream); device tensors / Out buffers / None are passed as pointers.  Raises on a refusal."""
    fn = getattr(_abi.lib(), "ptx_op_" + name)
    _abi.check(fn(*[ptr(a) if isinstance(a, (torch.Tensor, Out)) or a is None else a for a in args], stream()), "ptx_op_" + name)


def refused(name, *args, with_stream=True):
    """The call must be refused (negative code) without launching anything."""
    fn = getattr(_abi.lib(), "ptx_op_" + name)
    a = [ptr(x) if isinstance(x, (torch.Tensor, Out)) or x is None else x for x in args]
    rc = fn(*a, None) if with_stream else fn(*a)
    assert rc < 0, f"ptx_op_{name} accepted arguments it must refuse (code {rc})"
    return rc


# ------------------------------------------------------------------------------ ptx_op_gemm
class Gemm:
    """One ptx_op_gemm call described by its shape and element strides (a / b / c = (row stride, column stride); *_bs = strides
    of the two batch digits z1 = z // inner, z2 = z % inner).  Operands are flat arrays indexed by those strides."""

    def __init__(self, M, N, K, a, b, c, batch=1, inner=1, a_bs=(0, 0), b_bs=(0, 0), c_bs=(0, 0), a_dtype=0, b_dtype=0,
                 alpha=1.0, accumulate=0, ksplit=1, c_sk=0, c_off=0):
        # c_off: C starts that many elements into its buffer (a column block of a wider matrix); the words before it are guarded
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def but(self, **kw):
        """A copy with some fields replaced."""
        d = dict(self.__dict__)
        d.update(kw)
        return Gemm(**d)

    def args(self, A, B, C):
        return (A, B, C, self.M, self.N, self.K, self.a[0], self.a[1], self.b[0], self.b[1], self.c[0], self.c[1], self.batch,
                self.inner, self.a_bs[0], self.a_bs[1], self.b_bs[0], self.b_bs[1], self.c_bs[0], self.c_bs[1], self.a_dtype,
                self.b_dtype, float(self.alpha), int(self.accumulate), self.ksplit, self.c_sk)

    def route(self, A=4096, B=8192, C=12288):
        """ptx_op_gemm_route for this call; the pointers default to three 16-byte aligned dummies (nothing is dereferenced)."""
        return _abi.lib().ptx_op_gemm_route(*self.args(A, B, C))

    def _z(self):
        z = np.arange(self.batch, dtype=np.int64)
        return z // self.inner, z % self.inner

    def a_index(self):              # (batch, M, K)
        z1, z2 = self._z()
        return (z1 * self.a_bs[0] + z2 * self.a_bs[1])[:, None, None] + np.arange(self.M, dtype=np.int64)[None, :, None] * self.a[0] \
            + np.arange(self.K, dtype=np.int64)[None, None, :] * self.a[1]

    def b_index(self):              # (batch, K, N)
        z1, z2 = self._z()
        return (z1 * self.b_bs[0] + z2 * self.b_bs[1])[:, None, None] + np.arange(self.K, dtype=np.int64)[None, :, None] * self.b[0] \
            + np.arange(self.N, dtype=np.int64)[None, None, :] * self.b[1]

    def c_index(self):              # (batch, ksplit, M, N)
        z1, z2 = self._z()
        return (z1 * self.c_bs[0] + z2 * self.c_bs[1])[:, None, None, None] \
            + (np.arange(self.ksplit, dtype=np.int64) * self.c_sk)[None, :, None, None] \
            + np.arange(self.M, dtype=np.int64)[None, None, :, None] * self.c[0] \
            + np.arange(self.N, dtype=np.int64)[None, None, None, :] * self.c[1]

    def sizes(self):
        return int(self.a_index().max()) + 1, int(self.b_index().max()) + 1

    def slices(self):
        """[k0, k1) of every K slice by the rule of k_bgemm, restated: slices are whole 32-k steps, the last may be partial or empty."""
        kper = kper_rule(self.K, self.ksplit)
        return [(min(self.K, s * kper), min(self.K, (s + 1) * kper)) for s in range(self.ksplit)]

    def reference(self, Af, Bf, c_old=None):
        """float64 product per slice (batch, ksplit, M, N) and the matching sum of |a||b| (for the error bound)."""
        A, B = np.asarray(Af, np.float64)[self.a_index()], np.asarray(Bf, np.float64)[self.b_index()]
        ref = np.zeros((self.batch, self.ksplit, self.M, self.N))
        mag = np.zeros_like(ref)
        for s, (k0, k1) in enumerate(self.slices()):
            ref[:, s] = self.alpha * (A[:, :, k0:k1] @ B[:, k0:k1, :])
            mag[:, s] = abs(self.alpha) * (np.abs(A[:, :, k0:k1]) @ np.abs(B[:, k0:k1, :]))
        if self.accumulate:
            ref = ref + np.asarray(c_old, np.float64)
        return ref, mag

    def run(self, Af, Bf, c_old=None, a_ptr=None, b_ptr=None):
        """Launch on flat operands (numpy, values exact in the storage type); returns (got (batch, ksplit, M, N) after the guard
        check, route).  a_ptr / b_ptr: pointers to use instead of fresh aligned copies."""
        dt = {0: None, 1: torch.bfloat16, 2: torch.float16}
        tail = np.full(TAIL, np.nan, np.float32)        # a request past the last element reads NaN, and 0 x NaN is NaN
        At = None if a_ptr is not None else dv(np.concatenate([np.asarray(Af, np.float32).ravel(), tail]), dt[self.a_dtype])
        Bt = None if b_ptr is not None else dv(np.concatenate([np.asarray(Bf, np.float32).ravel(), tail]), dt[self.b_dtype])
        out = Out(self.c_index() + self.c_off, init=None if not self.accumulate else np.asarray(c_old, np.float32))
        args = self.args(a_ptr if a_ptr is not None else At.data_ptr(), b_ptr if b_ptr is not None else Bt.data_ptr(),
                         out.ptr + 4 * self.c_off)
        route = _abi.lib().ptx_op_gemm_route(*args)
        _abi.check(_abi.lib().ptx_op_gemm(*args, stream()), "ptx_op_gemm")
        return out.take(), route


def kper_rule(K, ksplit):
    """k per slice of ptx_op_gemm: ceil(K / ksplit) rounded up to the 32-k step of k_bgemm."""
    return -(-(-(-K // ksplit)) // 32) * 32


def gemm_bound(ref, mag, Kc):
    """|got - ref| <= (Kc + 8) u |alpha| (|A||B|) + u |ref|: the forward bound of an fp32 dot product of Kc terms, plus one rounding
    for alpha and the store (mag = |alpha| |A||B|).  A caller that accumulates adds u (|C_old| + |ref|) for the final sum."""
    return (Kc + 8) * U * mag + U * np.abs(ref)


def ints(rng, n, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=n).astype(np.float64)


# ------------------------------------------------------------------------------ dropout rule (csrc/train_rules.h)
_M64 = (1 << 64) - 1


def drop_mix32(x):
    """drop_mix32 of train_rules.h on an array of uint64 hash inputs."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((x ^ (x >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def drop_thresh(p):
    return np.uint32(int(float(np.float32(p)) * 4294967296.0))


def drop_keep_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_keep(n, group, p, seed):
    """keep[i] of element i of stream `seed`: one decision per index i // group."""
    base = np.uint64((seed * 0x100000001B3) & _M64)
    with np.errstate(over="ignore"):
        r = drop_mix32(base + (np.arange(n, dtype=np.uint64) // np.uint64(group)))
    return r >= drop_thresh(p)


def dropout_ref(x, group, p, seed):
    x = np.asarray(x, np.float32)
    return np.where(dropout_keep(x.size, group, p, seed), x * drop_keep_scale(p), np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------ slot-bias table
def bilin_taps(s):
    """Restated bilin_taps of train_ops.hip for a 4x4 -> s x s resize (align_corners=False): per output coordinate the two source
    rows / columns and their weights, in float32 as the kernel forms them."""
    sc = np.float32(4.0) / np.float32(s)
    src = np.maximum(sc * (np.arange(s, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < 3)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1.0) - l1).astype(np.float32), l1


def slotbias_taps_ref(pb, pc, pr, s, C):
    """The table from the restated taps, float64 arithmetic: (Mk, C)."""
    i0, i1, l0, l1 = bilin_taps(s)
    pb = np.asarray(pb, np.float64).reshape(-1, 4, 4)
    l0, l1 = l0.astype(np.float64), l1.astype(np.float64)
    rows = l0[None, :, None] * pb[:, i0, :] + l1[None, :, None] * pb[:, i1, :]                   # (Mk, s, 4)
    grid = l0[None, None, :] * rows[:, :, i0] + l1[None, None, :] * rows[:, :, i1]               # (Mk, s, s)
    grid = grid + np.asarray(pc, np.float64)[:, :, None] + np.asarray(pr, np.float64)[:, None, :]
    return grid.reshape(grid.shape[0], s * s)[:, :C]


def slotbias_torch(pb, pc, pr, s, C):
    """PRE:212-215 with torch: float64 leaf tensors (Mk,16), (Mk,s), (Mk,s) -> table (Mk,C), differentiable."""
    Mk = pb.shape[0]
    g = torch.nn.functional.interpolate(pb.view(1, Mk, 4, 4), size=(s, s), mode="bilinear", align_corners=False)[0]
    return (g + pc[:, :, None] + pr[:, None, :]).reshape(Mk, s * s)[:, :C]


# ------------------------------------------------------------------------------ float64 references of the other operators
def colsum_ref(x, y, mode, scale):
    x = np.asarray(x, np.float64)
    if mode == 0:
        t = x
    elif mode == 1:
        t = x * np.asarray(y, np.float64)
    elif mode == 2:
        t = x * x
    else:
        t = (x - np.asarray(y, np.float64)[None, :]) ** 2
    return float(scale) * t.sum(0)


def neighbours32(ref64):
    """float32(ref) and the fp32 numbers next to it on either side."""
    r = np.asarray(ref64, np.float64).astype(np.float32)
    return r, np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))


def eltwise_ref(opn, a, b, s, ncol):
    """float64 value of op `opn` on fp32 inputs (torch.erf in float64 for the GELU pair)."""
    a64 = np.asarray(a, np.float64)
    b64 = None if b is None else np.asarray(b, np.float64)
    if opn == 0:
        return a64 + b64
    if opn == 1:
        return a64 * float(s)
    if opn in (2, 3):
        t = torch.from_numpy(a64)
        cdf = (0.5 * (1.0 + torch.erf(t / np.sqrt(2.0)))).numpy()
        if opn == 2:
            return a64 * cdf
        return b64 * (cdf + a64 * np.exp(-0.5 * a64 * a64) / np.sqrt(2.0 * np.pi))
    if opn == 4:
        return torch.relu(torch.from_numpy(a64)).numpy()
    if opn == 5:
        return np.where(a64 > 0, b64, 0.0)
    if opn == 6:
        return a64 + b64[np.arange(a64.size) % ncol]
    if opn == 7:
        return a64 + float(s) * b64
    return a64 * b64


def softmax_ref(s, mask, rows_per_scene):
    """float64 softmax of fp32 scores with masked_fill(-1e9) (PRE:247); mask (B, L) uint8, 1 = valid."""
    s = torch.from_numpy(np.asarray(s, np.float64)).clone()
    if mask is not None:
        m = torch.from_numpy(np.asarray(mask)).bool()[torch.arange(s.shape[0]) // rows_per_scene]
        s = s.masked_fill(~m, float(np.float32(-1e9)))
    return torch.softmax(s, dim=1)


def out_positions_ref(tag, B, N):
    keep = (np.asarray(tag, np.uint32).reshape(B, N) >> 31) == 0
    pos = np.cumsum(keep, axis=1) - 1
    return np.where(keep, pos, -1).astype(np.int32), keep.sum(1).astype(np.int32)


def affine_bwd_ref(dout_list, opos, kidx, kcluster, kcenter, transform, B, N, Mk, K):
    """float64 autograd of PRE:459-465 in its index_put formulation: new = T (p - c) + c + t of every valid slot is put at its point,
    the surviving points are gathered into the output; dout_list[b] = (n_b, 3) gradient of scene b's output or None."""
    kc = torch.from_numpy(np.asarray(kcenter, np.float64)).requires_grad_(True)                  # (B, Mk, 3)
    T = torch.from_numpy(np.asarray(transform, np.float64)).requires_grad_(True)                 # (B, Mk, 3, 3)
    t = torch.zeros((B, Mk, 3), dtype=torch.float64, requires_grad=True)
    p = torch.from_numpy(np.asarray(kcluster, np.float64))                                       # (B, Mk, K, 3)
    new = torch.einsum("bmij,bmkj->bmki", T, p - kc[:, :, None, :]) + kc[:, :, None, :] + t[:, :, None, :]
    loss = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        if dout_list[b] is None:
            continue
        idx = torch.from_numpy(np.asarray(kidx[b], np.int64)).reshape(-1)
        valid = idx >= 0
        pts = torch.zeros((N, 3), dtype=torch.float64).index_put((idx[valid],), new[b].reshape(-1, 3)[valid])
        op_b = np.asarray(opos[b], np.int64)
        kept = torch.from_numpy(np.nonzero(op_b >= 0)[0])
        g = torch.from_numpy(np.asarray(dout_list[b], np.float64))[torch.from_numpy(op_b[op_b >= 0])]
        loss = loss + (pts[kept] * g).sum()
    if not loss.requires_grad:
        return np.zeros((B, Mk, 3)), np.zeros((B, Mk, 3, 3)), np.zeros((B, Mk, 3))
    gt, gT, gc = torch.autograd.grad(loss, (t, T, kc), allow_unused=True)
    z = lambda g, ref: np.zeros(ref.shape) if g is None else g.numpy()
    return z(gt, t), z(gT, T), z(gc, kc)


def cptr_array(ptrs):
    """A host array of device pointers (NULL for None) for ptx_op_affine_bwd_list."""
    arr = (ctypes.c_void_p * len(ptrs))(*[None if q is None else q for q in ptrs])
    return arr, ctypes.cast(arr, ctypes.c_void_p).value
