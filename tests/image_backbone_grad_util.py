"""What the test modules of the image backbone's backward share: the case tables of ``ptx_conv1x1_bwd`` / ``ptx_conv3x3_bwd`` with their
integer operands, and the exact answer from torch.  A plain module: no tests, no marks.

Integer operands: ``g`` in [-4, 4], ``x`` in [-4, 4], weights in [-2, 2], ``scale`` in {1, 2}, so ``|gz| <= 8``.  Every dx sum is at most
512 x 9 x 16 < 2^24 in magnitude (1x1: 2048 x 16) and every dweight sum at most 32 x pixels, which ``_check`` holds below 2^24 for every
case: all partial sums are integers that float32 holds exactly, in any order, and torch's float64 ``F.conv2d`` autograd on the CPU is the
exact answer -- the comparison is ``torch.equal``."""
import functools
import itertools

import torch
import torch.nn.functional as F

from tests import image_backbone_util as U

N_IMAGES = U.N_IMAGES                                       # 3: a pixel tile spans an image boundary
#: (scale, relu)
EPILOGUES = tuple(itertools.product((False, True), repeat=2))


def case(KS, cin, cout, H, W, stride, N=N_IMAGES):
    return (KS, cin, cout, H, W, stride, N)


#: 1x1: every width pair on every map at stride 1; the strided maps -- odd and even sides -- at stride 2
CONV1_CASES = tuple(case(1, ci, co, h, w, 1) for (ci, co) in U.CONV1_CHANNELS for (h, w) in U.CONV1_SIZES) + \
    tuple(case(1, ci, co, h, w, 2) for (ci, co) in U.CONV1_CHANNELS for (h, w) in U.CONV1_STRIDED + ((7, 9), (8, 8)))
#: 3x3: every width on every map at both strides
CONV3_CASES = tuple(case(3, c, c, h, w, s) for c in U.CONV3_CHANNELS for (h, w) in U.CONV3_SIZES for s in (1, 2))
#: the chunk plan's regimes (S == 1, S == 2, S >= 3 with a ragged last chunk; a pixel count that is no multiple of 64), for each kind at
#: 32 planes, the trainable stages' narrowest.  Which regime a case falls in is asked of ptx_conv_dweight_chunks by the test that uses them
CHUNK_CASES = tuple(case(KS, 32, 32, h, w, s, n) for KS in (1, 3) for (n, h, w, s) in ((3, 8, 8, 1), (3, 8, 13, 1), (5, 40, 36, 1), (5, 40, 36, 2)))
#: all-ones maps
ONES_MAPS = ((7, 9), (8, 8), (1, 1), (2, 3))


def out_pixels(c):
    KS, cin, cout, H, W, stride, N = c
    return N * U.out_side(H, stride) * U.out_side(W, stride)


def _check():
    for c in CONV1_CASES + CONV3_CASES + CHUNK_CASES:
        assert 32 * out_pixels(c) < 2 ** 24, c              # |gz x| <= 32 per pixel: every dweight sum is an exact float32 integer
        assert c[0] * c[0] * c[2] * 16 < 2 ** 24, c         # |w gz| <= 16 per (tap, co): every dx sum too


_check()


def case_id(c):
    return "k{}-{}to{}-{}x{}-s{}-n{}".format(*c)


def operands(c, scale, relu, seed=0):
    """The integer operands of a case, on the CPU, float32: ``x, w (Cout,Cin,k,k), g, scale | None, shift | None, residual, held`` (what dx
    holds before an accumulating call)."""
    KS, cin, cout, H, W, stride, N = c
    rng = torch.Generator().manual_seed(1000 * sum(c) + 2 * int(scale) + int(relu) + 7 * seed)
    ints = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=rng).float()      # noqa: E731
    ho, wo = U.out_side(H, stride), U.out_side(W, stride)
    return dict(x=ints((N, cin, H, W), -4, 4), w=ints((cout, cin, KS, KS), -2, 2), g=ints((N, cout, ho, wo), -4, 4),
                scale=ints((cout,), 1, 2) if scale else None, shift=ints((cout,), -8, 8) if scale else None,
                residual=ints((N, cout, ho, wo), -8, 8), held=ints((N, cin, H, W), -8, 8))


@functools.lru_cache(maxsize=None)
def reference(c, scale, relu, seed=0):
    """The operands of a case and the exact answer, computed once and shared (never modified): ``out`` (the forward's result, float32
    integers), ``dresidual``, ``dx``, ``dweight`` in float64 from ``torch.autograd.grad`` of float64 ``F.conv2d`` -> ``* scale + shift`` ->
    ``+ residual`` -> ``F.relu``."""
    KS, cin, cout, H, W, stride, N = c
    op = operands(c, scale, relu, seed)
    x, w, res = (op[k].double().requires_grad_() for k in ("x", "w", "residual"))
    v = F.conv2d(x, w, stride=stride, padding=KS // 2)
    if scale:
        v = v * op["scale"].double()[None, :, None, None] + op["shift"].double()[None, :, None, None]
    v = v + res
    out = F.relu(v) if relu else v
    dx, dw, dres = torch.autograd.grad(out, (x, w, res), op["g"].double())
    assert float(out.detach().abs().max()) < 2 ** 24
    return dict(op, out=out.detach().float(), dx=dx, dweight=dw, dresidual=dres)


def weight_operand(w):
    """``(co,ci,k,k)`` -> the layout the entry points take and give dweight in: ``(Cout,Cin)`` / ``(co,ky,kx,ci)``."""
    return w.reshape(w.shape[0], w.shape[1]).contiguous() if w.shape[-1] == 1 else U.conv3_weight_operand(w)


def weight_from_operand(d, KS):
    """The inverse, for a dweight: back to ``(co,ci,k,k)``."""
    return d.reshape(d.shape[0], d.shape[1], 1, 1) if KS == 1 else d.permute(0, 3, 1, 2).contiguous()
